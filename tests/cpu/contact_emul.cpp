// contact_emul.cpp -- datum_amd/csrc/ocean_contact.h walked on the CPU (tests/test_contact_emul.py): the functions ocean_contact_kernel calls,
// with the wave's 64 lanes as an array, the walk of couple_emul.cpp, the layer's state and src plane, the depth map and the wall list as
// plain arrays.  The velocity records are given, as in couple_emul.cpp.  The layer's own sub-step between two of these is
// ripple_emul.cpp's.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_contact.h"

using namespace ocean;

namespace
{
  // the 64 partials of one body; step<S>: p[l] <- p[l] + p[l + S] for l < S
  struct ContactWaveArray
  {
    ContactPartial p[BODY_LANES];

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

int contact_record_floats(void) { return DATUM_OCEAN_CONTACT_RECORD_FLOATS; }
int contact_fields(void) { return COUPLE_FIELDS + CONTACT_FIELDS; }
int contact_struct_bytes(void) { return (int)sizeof(datum_ocean_body_contact); }

// what datum_ocean_set_ripple_walls does to the handle's copy of the list: inv2 into `reserved`
void contact_emul_prepare_walls(datum_ocean_ripple_wall *walls, int count)
{
  for(int k = 0; k < count; ++k)
    contact_wall_prepare(walls[k]);
}

// One launch of the kernel: couple_emul_substep's arguments and the scene -- the parameters, the bed's ten terms (width, height as floats'
// bits are not used: bedi holds them) with the map [height][width], the prepared wall list.  records [nbodies][16]
void contact_emul_substep(datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, int nbodies, float const *probes,
                          int nprobes, int64_t const *offsets, float const *recs, float const *state, int *src, int R, int ox, int oy, float invs, float h,
                          int first, float *records, datum_ocean_body_contact const *contact, int const *bedi, float const *bedf, float const *map,
                          datum_ocean_ripple_wall const *walls, int nwalls)
{
  RippleGrid g;
  g.R = R;
  g.ox = ox;
  g.oy = oy;
  g.invs = invs;

  ContactScene scene = {};
  scene.k = *contact;
  scene.bed.width = bedi[0];
  scene.bed.height = bedi[1];
  scene.bed.ox = bedf[0];
  scene.bed.oy = bedf[1];
  scene.bed.invt = bedf[2];
  scene.bed.outside = bedf[3];
  scene.walls = walls;
  scene.nwalls = nwalls;

  auto cell = [&](int index) { return RippleCell{ state[2 * index], state[2 * index + 1] }; };
  auto splat = [&](float x, float y, float V) { return ripple_splat(g, x, y, V, [&](int index, int q) { src[index] += q; }); };
  auto texel = [&](int index) { return map[index]; };

  for(int b = 0; b < nbodies; ++b)
  {
    // (copies, as the kernel's registers: a body that turns bad leaves memory as it was)
    datum_ocean_body B = bodies[b];
    datum_ocean_body_motion M = motions[b];

    float *record = records + DATUM_OCEAN_CONTACT_RECORD_FLOATS * b;

    bool bad = body_range_bad(B, nprobes) || step_props_bad(props[b]) || drag_motion_bad(M);

    float old7 = 0.0f, old11 = 0.0f, old15 = 0.0f;

    if (!first)
    {
      bad = bad || couple_was_bad(record[0]);
      old7 = record[7];
      old11 = record[11];
      old15 = record[15];
    }

    ContactWaveArray wave;

    for(int l = 0; l < BODY_LANES; ++l)
      wave.p[l] = contact_zero();

    if (!bad)
    {
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

          ContactPartial t;

          t.c = couple_terms(B, M, w, pr.a, rippled, h, splat);

          contact_terms(t.k, B, M, scene, w, pr.a, texel, [&](int k) { return walls[k]; });

          body_add(wave.p[l], t);
        }
    }

    StepTotals total = {};

    if (!bad)
    {
      body_tree(wave);

      total = contact_integrate(B, M, props[b], wave.p[0], h);

      bad = !step_state_finite(B, M);
    }

    if (bad)
    {
      for(int f = 0; f < DATUM_OCEAN_CONTACT_RECORD_FLOATS; ++f)
        record[f] = nanf("");
    }
    else
    {
      ContactRecord const c = contact_fold(total, wave.p[0], first != 0, old7, old11, old15);

      bodies[b] = B;
      motions[b] = M;

      for(int f = 0; f < DATUM_OCEAN_CONTACT_RECORD_FLOATS; ++f)
        record[f] = c.f[f];
    }
  }
}

// the eight contact terms of single probes, for the pointwise tests: n probes of ONE body b and motion mo, world points w [n][3], weights
// a [n]; out [n][8]
void contact_emul_terms(datum_ocean_body const *b, datum_ocean_body_motion const *mo, float const *w, float const *a, int n, datum_ocean_body_contact const *contact,
                        int const *bedi, float const *bedf, float const *map, datum_ocean_ripple_wall const *walls, int nwalls, float *out)
{
  ContactScene scene = {};
  scene.k = *contact;
  scene.bed.width = bedi[0];
  scene.bed.height = bedi[1];
  scene.bed.ox = bedf[0];
  scene.bed.oy = bedf[1];
  scene.bed.invt = bedf[2];
  scene.bed.outside = bedf[3];
  scene.walls = walls;
  scene.nwalls = nwalls;

  for(int i = 0; i < n; ++i)
  {
    BodyWorld const p = { w[3 * i], w[3 * i + 1], w[3 * i + 2] };

    contact_terms(out + CONTACT_FIELDS * i, *b, *mo, scene, p, a[i], [&](int index) { return map[index]; }, [&](int k) { return walls[k]; });
  }
}

}
