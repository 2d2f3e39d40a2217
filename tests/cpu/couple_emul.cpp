// couple_emul.cpp -- datum_amd/csrc/ocean_couple.h walked on the CPU (tests/test_couple_emul.py): the functions ocean_couple_kernel calls,
// with the wave's 64 lanes as an array, the walk of step_emul.cpp, the layer's state and src plane as plain arrays.  The velocity records
// are given (body b's probe k has record offsets[b] + k): the fetch and the solve are the several-cascade velocity query's and are pinned
// there.  The layer's own sub-step between two of these is ripple_emul.cpp's.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_couple.h"

using namespace ocean;

namespace
{
  // the 64 partials of one body; step<S>: p[l] <- p[l] + p[l + S] for l < S
  struct CoupleWaveArray
  {
    CouplePartial p[BODY_LANES];

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

int couple_record_floats(void) { return DATUM_OCEAN_COUPLED_RECORD_FLOATS; }
int couple_fields(void) { return COUPLE_FIELDS; }

// One launch of the kernel: bodies and motions advanced in place, records [nbodies][12] read (first == 0) and written, deposits into src;
// state [R*R][2] is the layer's current buffer in memory order
void couple_emul_substep(datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, int nbodies, float const *probes,
                         int nprobes, int64_t const *offsets, float const *recs, float const *state, int *src, int R, int ox, int oy, float invs, float h,
                         int first, float *records)
{
  RippleGrid g;
  g.R = R;
  g.ox = ox;
  g.oy = oy;
  g.invs = invs;

  auto cell = [&](int index) { return RippleCell{ state[2 * index], state[2 * index + 1] }; };
  auto splat = [&](float x, float y, float V) { return ripple_splat(g, x, y, V, [&](int index, int q) { src[index] += q; }); };

  for(int b = 0; b < nbodies; ++b)
  {
    // (copies, as the kernel's registers: a body that turns bad leaves memory as it was)
    datum_ocean_body B = bodies[b];
    datum_ocean_body_motion M = motions[b];

    float *record = records + DATUM_OCEAN_COUPLED_RECORD_FLOATS * b;

    bool bad = body_range_bad(B, nprobes) || step_props_bad(props[b]) || drag_motion_bad(M);

    float old7 = 0.0f, old11 = 0.0f;

    if (!first)
    {
      bad = bad || couple_was_bad(record[0]);
      old7 = record[7];
      old11 = record[11];
    }

    CoupleWaveArray wave;

    for(int l = 0; l < BODY_LANES; ++l)
      wave.p[l] = couple_zero();

    if (!bad)
    {
      // (pass by pass, lane by lane, as the wave walks: the deposits are integers and commute)
      for(int l = 0; l < BODY_LANES; ++l)
        for(int k = 0; k < body_lane_probes(B.count, l); ++k)
        {
          int const i = body_lane_probe(0, l, k);

          BodyProbe const &pr = reinterpret_cast<BodyProbe const*>(probes)[B.first + i];
          BodyWorld const w = body_transform(B, pr);

          if (body_probe_bad(w, pr.a))
          {
            bad = true;
            continue;
          }

          float rippled[DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS];

          couple_record(rippled, recs + 8 * (offsets[b] + i), ripple_sample(g, w.x, w.y, cell));

          body_add(wave.p[l], couple_terms(B, M, w, pr.a, rippled, h, splat));
        }
    }

    StepTotals total = {};

    if (!bad)
    {
      body_tree(wave);

      total = step_integrate(B, M, props[b], wave.p[0].s, h);

      bad = !step_state_finite(B, M);
    }

    if (bad)
    {
      for(int f = 0; f < DATUM_OCEAN_COUPLED_RECORD_FLOATS; ++f)
        record[f] = nanf("");
    }
    else
    {
      CoupleRecord const c = couple_fold(total, wave.p[0], first != 0, old7, old11);

      bodies[b] = B;
      motions[b] = M;

      for(int f = 0; f < DATUM_OCEAN_COUPLED_RECORD_FLOATS; ++f)
        record[f] = c.f[f];
    }
  }
}

}
