// body_emul.cpp -- datum_amd/csrc/ocean_body.h walked on the CPU (tests/test_body_emul.py): the functions ocean_body_kernel calls, with the
// wave's 64 lanes as an array.  The surface records are given (body b's probe k has record offsets[b] + k): the fetch and the solve are the
// several-cascade query's and are pinned there.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_body.h"

using namespace ocean;

namespace
{
  // the 64 partials of one body; step<S>: p[l] <- p[l] + p[l + S] for l < S
  struct WaveArray
  {
    BodyPartial p[BODY_LANES];

    template<int S>
    void step()
    {
      for(int l = 0; l < S; ++l)
        body_add(p[l], p[l + S]);
    }
  };

  bool range_ok(datum_ocean_body const &b, int nprobes)
  {
    return !body_range_bad(b, nprobes);
  }
}

extern "C"
{

size_t body_sizeof(void) { return sizeof(datum_ocean_body); }
size_t body_offsetof(int field)
{
  switch(field)
  {
    case 0: return offsetof(datum_ocean_body, rotation);
    case 1: return offsetof(datum_ocean_body, position);
    case 2: return offsetof(datum_ocean_body, first);
    case 3: return offsetof(datum_ocean_body, count);
    case 4: return offsetof(datum_ocean_body, cap);
    default: return offsetof(datum_ocean_body, pad);
  }
}

// world positions [offsets[b] + k][3] of every probe of every body whose range lies in the array, and bad[offsets[b] + k] (body_probe_bad)
void body_world(datum_ocean_body const *bodies, int nbodies, float const *probes, int nprobes, int64_t const *offsets, float *world, unsigned char *bad)
{
  for(int b = 0; b < nbodies; ++b)
  {
    if (!range_ok(bodies[b], nprobes))
      continue;

    for(int k = 0; k < bodies[b].count; ++k)
    {
      BodyProbe const &pr = reinterpret_cast<BodyProbe const*>(probes)[bodies[b].first + k];
      BodyWorld const w = body_transform(bodies[b], pr);

      float *o = world + 3 * (offsets[b] + k);
      o[0] = w.x; o[1] = w.y; o[2] = w.z;
      bad[offsets[b] + k] = body_probe_bad(w, pr.a);
    }
  }
}

// the kernel's walk with the records given: records_out [nbodies][8]
void body_reduce(datum_ocean_body const *bodies, int nbodies, float const *probes, int nprobes, int64_t const *offsets, float const *recs, float *records_out)
{
  for(int b = 0; b < nbodies; ++b)
  {
    datum_ocean_body const &B = bodies[b];

    bool bad = body_range_bad(B, nprobes);

    int const n = bad ? 0 : B.count;

    WaveArray wave;

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

        body_add(wave.p[l], body_terms(B, w, pr.a, recs + 8 * (offsets[b] + i)));
      }
    }

    body_tree(wave);

    for(int f = 0; f < BODY_FIELDS; ++f)
      records_out[8 * b + f] = bad ? nanf("") : wave.p[0].f[f];
  }
}

}
