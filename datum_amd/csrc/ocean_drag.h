// ocean_drag.h -- body drag (include/datum_ocean_hip.h: datum_ocean_reduce_body_drag) stated once: the rule that makes a motion (and so its
// body) bad, and the force and torque terms a probe contributes given its velocity record.  The probe, the pose transform, the bad-probe
// and bad-range rules, which lane takes which probe, the partials and the tree are body buoyancy's (ocean_body.h), unchanged: the drag's
// record has buoyancy's shape, seven sums and a maximum in field 7.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/drag_emul.cpp, tests/test_drag_emul.py): ocean_drag_kernel of ocean_drag.hip
// calls these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product and sum is one fp32
// operation, rounded as written; sqrtf is the correctly rounded one on the host and on the device.

#pragma once

#include "ocean_body.h"

namespace ocean
{
  static_assert(DATUM_OCEAN_DRAG_RECORD_FLOATS == BODY_FIELDS, "the drag's record is a BodyPartial: body_add and body_tree as they are");
  static_assert(sizeof(datum_ocean_body_motion) == 32, "a motion is 32 bytes");
  static_assert(sizeof(datum_ocean_body_motion) % 16 == 0, "an array of motions keeps its 16-byte alignment");

  // a motion with a non-finite field: nothing is fetched for its body, whose record is eight NaNs
  OB_HD bool drag_motion_bad(datum_ocean_body_motion const &m)
  {
    return !(body_finite(m.linear[0]) && body_finite(m.linear[1]) && body_finite(m.linear[2])
          && body_finite(m.angular[0]) && body_finite(m.angular[1]) && body_finite(m.angular[2]) && body_finite(m.cl) && body_finite(m.cq));
  }

  // the terms of a probe at w with weight a, given the velocity record above (w.x, w.y): rec[2] the water height, rec[3] the residual,
  // rec[4..6] the water's velocity.  Fx, Fy, Fz, tau x, tau y, tau z, m, residual
  OB_HD BodyPartial drag_terms(datum_ocean_body const &b, datum_ocean_body_motion const &mo, BodyWorld const &w, float a, float const *rec)
  {
    float const d = fminf(fmaxf(rec[2] - w.z, 0.0f), b.cap);      // submersion and weight: body_terms' d and m
    float const m = a * d;

    float const rx = w.x - b.position[0], ry = w.y - b.position[1], rz = w.z - b.position[2];

    float const *v = mo.linear, *o = mo.angular;

    // the hull's velocity at the probe, v + omega x r
    float const ux = v[0] + (o[1] * rz - o[2] * ry);
    float const uy = v[1] + (o[2] * rx - o[0] * rz);
    float const uz = v[2] + (o[0] * ry - o[1] * rx);

    // the water relative to the hull
    float const ex = rec[4] - ux, ey = rec[5] - uy, ez = rec[6] - uz;

    float const s = sqrtf((ex * ex + ey * ey) + ez * ez);
    float const k = m * (mo.cl + mo.cq * s);

    float const fx = k * ex, fy = k * ey, fz = k * ez;

    BodyPartial t;
    t.f[0] = fx;
    t.f[1] = fy;
    t.f[2] = fz;
    t.f[3] = ry * fz - rz * fy;
    t.f[4] = rz * fx - rx * fz;
    t.f[5] = rx * fy - ry * fx;
    t.f[6] = m;
    t.f[7] = rec[3];
    return t;
  }
}
