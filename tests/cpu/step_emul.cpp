// step_emul.cpp -- datum_amd/csrc/ocean_step.h walked on the CPU (tests/test_step_emul.py): the functions ocean_step_kernel calls, with the
// wave's 64 lanes as an array and the walk of body_emul.cpp.  The velocity records are given (body b's probe k has record offsets[b] + k):
// the fetch and the solve are the several-cascade velocity query's and are pinned there.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_step.h"

using namespace ocean;

namespace
{
  // the 64 partials of one body; step<S>: p[l] <- p[l] + p[l + S] for l < S
  struct StepWaveArray
  {
    StepPartial p[BODY_LANES];

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

size_t step_props_sizeof(void) { return sizeof(datum_ocean_body_props); }
size_t step_props_offsetof(int field)
{
  switch(field)
  {
    case 0: return offsetof(datum_ocean_body_props, invmass);
    case 1: return offsetof(datum_ocean_body_props, invinertia);
    case 2: return offsetof(datum_ocean_body_props, gravity);
    case 3: return offsetof(datum_ocean_body_props, buoyancy);
    default: return offsetof(datum_ocean_body_props, pad);
  }
}

int step_record_floats(void) { return DATUM_OCEAN_STEP_RECORD_FLOATS; }
int step_max_substeps(void) { return DATUM_OCEAN_STEP_MAX_SUBSTEPS; }
int step_fields(void) { return STEP_FIELDS; }

// one sub-step's walk with the records given: sums_out [nbodies][10], bad_out [nbodies] (1: the range, the motion, the props or a probe)
void step_reduce(datum_ocean_body const *bodies, datum_ocean_body_motion const *motions, datum_ocean_body_props const *props, int nbodies, float const *probes,
                 int nprobes, int64_t const *offsets, float const *recs, float *sums_out, int *bad_out)
{
  for(int b = 0; b < nbodies; ++b)
  {
    datum_ocean_body const &B = bodies[b];
    datum_ocean_body_motion const &M = motions[b];

    bool bad = body_range_bad(B, nprobes) || step_props_bad(props[b]) || drag_motion_bad(M);

    int const n = bad ? 0 : B.count;

    StepWaveArray wave;

    for(int l = 0; l < BODY_LANES; ++l)
    {
      wave.p[l] = step_zero();

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

        body_add(wave.p[l], step_terms(B, M, w, pr.a, recs + 8 * (offsets[b] + i)));
      }
    }

    body_tree(wave);

    for(int f = 0; f < STEP_FIELDS; ++f)
      sums_out[STEP_FIELDS * b + f] = wave.p[0].f[f];

    bad_out[b] = bad;
  }
}

// step_integrate per body, in place: sums [nbodies][10]; totals_out [nbodies][6] force and torque, finite_out [nbodies] step_state_finite after
void step_integrate_bodies(datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, int nbodies, float const *sums, float h,
                           float *totals_out, int *finite_out)
{
  for(int b = 0; b < nbodies; ++b)
  {
    StepPartial s;

    for(int f = 0; f < STEP_FIELDS; ++f)
      s.f[f] = sums[STEP_FIELDS * b + f];

    StepTotals const t = step_integrate(bodies[b], motions[b], props[b], s, h);

    for(int k = 0; k < 3; ++k)
    {
      totals_out[6 * b + k] = t.force[k];
      totals_out[6 * b + 3 + k] = t.torque[k];
    }

    finite_out[b] = step_state_finite(bodies[b], motions[b]);
  }
}

}
