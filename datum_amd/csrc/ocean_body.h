// ocean_body.h -- body buoyancy (include/datum_ocean_hip.h: datum_ocean_reduce_bodies) stated once: the body and probe records, the pose
// transform, the force terms a probe contributes given its surface record, the rule that makes a probe (and so its body) bad, which lane
// takes which probe and the order in which the 64 lanes' partials are added.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/body_emul.cpp, tests/test_body_emul.py): ocean_body_kernel of ocean_body.hip
// calls these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product and sum is one fp32
// operation, rounded as written; there is no fmaf here.

#pragma once

#include <math.h>

#include "../../include/datum_ocean_hip.h"

#if defined(__HIPCC__)
#define OB_HD __host__ __device__ __forceinline__
#else
#define OB_HD inline
#endif

namespace ocean
{
  constexpr int BODY_LANES = 64;                        // one wave per body
  constexpr int BODY_FIELDS = DATUM_OCEAN_BODY_RECORD_FLOATS;

  struct BodyProbe
  {
    float x, y, z;          // body-local position, metres
    float a;                // weight: the cross-section the probe stands for, m^2
  };

  static_assert(sizeof(BodyProbe) == 16, "a probe is one 16-byte load");
  static_assert(sizeof(datum_ocean_body) == 64, "a body is 64 bytes");

  struct BodyWorld { float x, y, z; };

  // w = R p + T, each row ((R0 x + R1 y) + R2 z) + T
  OB_HD BodyWorld body_transform(datum_ocean_body const &b, BodyProbe const &p)
  {
    float const *R = b.rotation;

    BodyWorld w;
    w.x = ((R[0] * p.x + R[1] * p.y) + R[2] * p.z) + b.position[0];
    w.y = ((R[3] * p.x + R[4] * p.y) + R[5] * p.z) + b.position[1];
    w.z = ((R[6] * p.x + R[7] * p.y) + R[8] * p.z) + b.position[2];
    return w;
  }

  OB_HD bool body_finite(float v)
  {
    return fabsf(v) <= 3.4028234663852886e38f;          // false for a NaN
  }

  // a probe with a non-finite world position or weight: nothing is fetched for it, and its body's record is eight NaNs
  OB_HD bool body_probe_bad(BodyWorld const &w, float a)
  {
    return !(body_finite(w.x) && body_finite(w.y) && body_finite(w.z) && body_finite(a));
  }

  // bad whatever its probes hold: a range outside the probe array (no overflow: first, count >= 0 before they are subtracted), a NaN cap
  OB_HD bool body_range_bad(datum_ocean_body const &b, int nprobes)
  {
    return b.first < 0 || b.count < 0 || b.first > nprobes || b.count > nprobes - b.first || b.cap != b.cap;
  }

  // one lane's partials, and what one probe adds to them: Fz, tau x, tau y, wet, m n.x, m n.y, m n.z, max residual
  struct BodyPartial
  {
    float f[BODY_FIELDS];
  };

  OB_HD BodyPartial body_zero()
  {
    BodyPartial p;
    for(int k = 0; k < BODY_FIELDS; ++k)
      p.f[k] = 0.0f;
    return p;
  }

  // the terms of a probe at w with weight a, given the surface record above (w.x, w.y): rec[2] the water height, rec[3] the residual,
  // rec[4..6] the unit normal
  OB_HD BodyPartial body_terms(datum_ocean_body const &b, BodyWorld const &w, float a, float const *rec)
  {
    float const d = fminf(fmaxf(rec[2] - w.z, 0.0f), b.cap);      // submersion
    float const m = a * d;                                        // vertical force term (Archimedes)
    float const rx = w.x - b.position[0], ry = w.y - b.position[1];

    BodyPartial t;
    t.f[0] = m;
    t.f[1] = ry * m;
    t.f[2] = -(rx * m);
    t.f[3] = (d > 0.0f) ? a : 0.0f;
    t.f[4] = m * rec[4];
    t.f[5] = m * rec[5];
    t.f[6] = m * rec[6];
    t.f[7] = rec[3];
    return t;
  }

  // p <- p + t, field 7 the maximum: a lane adding its next probe, and one step p[l] <- p[l] + p[l + s] of the tree
  OB_HD void body_add(BodyPartial &p, BodyPartial const &t)
  {
    for(int k = 0; k < BODY_FIELDS - 1; ++k)
      p.f[k] = p.f[k] + t.f[k];

    p.f[BODY_FIELDS - 1] = fmaxf(p.f[BODY_FIELDS - 1], t.f[BODY_FIELDS - 1]);
  }

  // lane l takes probes first + l, first + l + 64, ... in increasing order: how many of `count`
  OB_HD int body_lane_probes(int count, int lane)
  {
    return (count > lane) ? (count - lane + BODY_LANES - 1) / BODY_LANES : 0;
  }

  OB_HD int body_lane_probe(int first, int lane, int k)
  {
    return first + lane + k * BODY_LANES;
  }

  // The tree: for s = 32, 16, 8, 4, 2, 1: p[l] <- p[l] + p[l + s] for l < s; p[0] is the body's record.  `Wave` holds the 64 partials --
  // on the device one per lane, step<S>() a cross-lane exchange followed by body_add (lanes >= s may hold anything afterwards: nothing
  // reads them); on the CPU an array
  template<typename Wave>
  OB_HD void body_tree(Wave &wave)
  {
    wave.template step<32>();
    wave.template step<16>();
    wave.template step<8>();
    wave.template step<4>();
    wave.template step<2>();
    wave.template step<1>();
  }
}
