// drag_emul.cpp -- datum_amd/csrc/ocean_drag.h walked on the CPU (tests/test_drag_emul.py): the functions ocean_drag_kernel calls, with the
// wave's 64 lanes as an array and the walk of body_emul.cpp.  The velocity records are given (body b's probe k has record offsets[b] + k):
// the fetch and the solve are the several-cascade velocity query's and are pinned there.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_drag.h"

using namespace ocean;

namespace
{
  // the 64 partials of one body; step<S>: p[l] <- p[l] + p[l + S] for l < S
  struct DragWaveArray
  {
    BodyPartial p[BODY_LANES];

    template<int S>
    void step()
    {
      for(int l = 0; l < S; ++l)
        body_add(p[l], p[l + S]);
    }
  };
}

extern "C"
{

size_t drag_motion_sizeof(void) { return sizeof(datum_ocean_body_motion); }
size_t drag_motion_offsetof(int field)
{
  switch(field)
  {
    case 0: return offsetof(datum_ocean_body_motion, linear);
    case 1: return offsetof(datum_ocean_body_motion, angular);
    case 2: return offsetof(datum_ocean_body_motion, cl);
    default: return offsetof(datum_ocean_body_motion, cq);
  }
}

// the kernel's walk with the records given: records_out [nbodies][8]
void drag_reduce(datum_ocean_body const *bodies, datum_ocean_body_motion const *motions, int nbodies, float const *probes, int nprobes, int64_t const *offsets,
                 float const *recs, float *records_out)
{
  for(int b = 0; b < nbodies; ++b)
  {
    datum_ocean_body const &B = bodies[b];
    datum_ocean_body_motion const &M = motions[b];

    bool bad = body_range_bad(B, nprobes) || drag_motion_bad(M);

    int const n = bad ? 0 : B.count;

    DragWaveArray wave;

    for(int l = 0; l < BODY_LANES; ++l)
    {
      wave.p[l] = body_zero();

      for(int k = 0; k < body_lane_probes(n, l); ++k)
      {
        int const i = body_lane_probe(0, l, k);

        BodyProbe const &pr = reinterpret_cast<BodyProbe const*>(probes)[B.first + i];
        BodyWorld const w = body_transform(B, pr);

        if (body_probe_bad(w, pr.a))
        {
          bad = true;
          continue;
        }

        body_add(wave.p[l], drag_terms(B, M, w, pr.a, recs + 8 * (offsets[b] + i)));
      }
    }

    body_tree(wave);

    for(int f = 0; f < BODY_FIELDS; ++f)
      records_out[8 * b + f] = bad ? nanf("") : wave.p[0].f[f];
  }
}

}
