// ocean_step.h -- body stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies) stated once: the rule that makes a body's props (and so
// the body) bad, the ten sums a sub-step forms over the hull probes, what one probe adds to them given its velocity record, and the
// integrator that turns the sums into the next pose and motion.  The probe, the pose transform, the bad-probe, bad-range and bad-motion
// rules, which lane takes which probe and the tree are body buoyancy's and body drag's (ocean_body.h, ocean_drag.h), unchanged; a probe's
// terms are body_terms' fields 0-2 and drag_terms' fields 0-5 and 7, taken from those functions.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/step_emul.cpp, tests/test_step_emul.py): ocean_step_kernel of ocean_step.hip
// calls these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product, sum and quotient is
// one fp32 operation, rounded as written; division and sqrtf are the correctly rounded ones on the host and on the device.

#pragma once

#include "ocean_drag.h"

namespace ocean
{
  static_assert(sizeof(datum_ocean_body_props) == 32, "a body's props are 32 bytes");
  static_assert(sizeof(datum_ocean_body_props) % 16 == 0, "an array of props keeps its 16-byte alignment");
  static_assert(DATUM_OCEAN_STEP_RECORD_FLOATS == 8, "a step record is two 16-byte stores");

  // the sums of a sub-step: M, bx, by (body_terms' fields 0-2), the drag's Fx, Fy, Fz, tau x, tau y, tau z (drag_terms' 0-5), max residual
  constexpr int STEP_FIELDS = 10;

  struct StepPartial
  {
    float f[STEP_FIELDS];
  };

  OB_HD StepPartial step_zero()
  {
    StepPartial p;
    for(int k = 0; k < STEP_FIELDS; ++k)
      p.f[k] = 0.0f;
    return p;
  }

  // body_add for the ten fields, the last one the maximum: a lane adding its next probe, and one step of body_tree
  OB_HD void body_add(StepPartial &p, StepPartial const &t)
  {
    for(int k = 0; k < STEP_FIELDS - 1; ++k)
      p.f[k] = p.f[k] + t.f[k];

    p.f[STEP_FIELDS - 1] = fmaxf(p.f[STEP_FIELDS - 1], t.f[STEP_FIELDS - 1]);
  }

  // props with a non-finite field (the padding is not looked at): the body is bad before its first sub-step
  OB_HD bool step_props_bad(datum_ocean_body_props const &p)
  {
    return !(body_finite(p.invmass) && body_finite(p.invinertia[0]) && body_finite(p.invinertia[1]) && body_finite(p.invinertia[2])
          && body_finite(p.gravity) && body_finite(p.buoyancy));
  }

  // the terms of a probe at w with weight a, given its velocity record: fields 0-3 of that record are the surface record's, so body_terms
  // reads of it what it reads of a surface record (its normal terms are not used)
  OB_HD StepPartial step_terms(datum_ocean_body const &b, datum_ocean_body_motion const &mo, BodyWorld const &w, float a, float const *rec)
  {
    BodyPartial const lift = body_terms(b, w, a, rec);
    BodyPartial const drag = drag_terms(b, mo, w, a, rec);

    StepPartial t;
    t.f[0] = lift.f[0];
    t.f[1] = lift.f[1];
    t.f[2] = lift.f[2];
    for(int k = 0; k < 6; ++k)
      t.f[3 + k] = drag.f[k];
    t.f[9] = drag.f[7];
    return t;
  }

  // force and torque of a sub-step, world space, about the body origin
  struct StepTotals
  {
    float force[3];
    float torque[3];
  };

  OB_HD float step_norm(float x, float y, float z)
  {
    return sqrtf((x * x + y * y) + z * z);
  }

  // One sub-step of length h from the sums s: the totals, then semi-implicit Euler -- the new velocities first, the pose moved with them --
  // and the rotation's first two columns advanced and made orthonormal again (Gram-Schmidt, x first), the third their cross product.  The
  // gyroscopic term omega x I omega is left out.  b and mo are advanced in place; first, count, cap, cl and cq stay
  OB_HD StepTotals step_integrate(datum_ocean_body &b, datum_ocean_body_motion &mo, datum_ocean_body_props const &p, StepPartial const &s, float h)
  {
    float *R = b.rotation, *T = b.position, *v = mo.linear, *o = mo.angular;

    StepTotals t;
    t.force[0] = s.f[3];
    t.force[1] = s.f[4];
    t.force[2] = p.buoyancy * s.f[0] + s.f[5];
    t.torque[0] = p.buoyancy * s.f[1] + s.f[6];
    t.torque[1] = p.buoyancy * s.f[2] + s.f[7];
    t.torque[2] = s.f[8];

    // linear
    v[0] = v[0] + h * (t.force[0] * p.invmass);
    v[1] = v[1] + h * (t.force[1] * p.invmass);
    v[2] = v[2] + h * (t.force[2] * p.invmass - p.gravity);

    for(int k = 0; k < 3; ++k)
      T[k] = T[k] + h * v[k];

    // angular: the torque into the body frame (R transposed), the diagonal inertia there, and back (body_transform's rows)
    float ab[3];
    for(int j = 0; j < 3; ++j)
      ab[j] = ((R[j] * t.torque[0] + R[3 + j] * t.torque[1]) + R[6 + j] * t.torque[2]) * p.invinertia[j];

    for(int k = 0; k < 3; ++k)
      o[k] = o[k] + h * ((R[3 * k] * ab[0] + R[3 * k + 1] * ab[1]) + R[3 * k + 2] * ab[2]);

    // rotation: c_j' = c_j + h (omega' x c_j) for the columns j = 0, 1
    float c[2][3];
    for(int j = 0; j < 2; ++j)
    {
      float const cx = R[j], cy = R[3 + j], cz = R[6 + j];

      c[j][0] = cx + h * (o[1] * cz - o[2] * cy);
      c[j][1] = cy + h * (o[2] * cx - o[0] * cz);
      c[j][2] = cz + h * (o[0] * cy - o[1] * cx);
    }

    float const nx = step_norm(c[0][0], c[0][1], c[0][2]);
    float const x[3] = { c[0][0] / nx, c[0][1] / nx, c[0][2] / nx };

    float const dot = (x[0] * c[1][0] + x[1] * c[1][1]) + x[2] * c[1][2];
    float const y0[3] = { c[1][0] - dot * x[0], c[1][1] - dot * x[1], c[1][2] - dot * x[2] };

    float const ny = step_norm(y0[0], y0[1], y0[2]);
    float const y[3] = { y0[0] / ny, y0[1] / ny, y0[2] / ny };

    float const z[3] = { x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0] };

    for(int k = 0; k < 3; ++k)
    {
      R[3 * k] = x[k];
      R[3 * k + 1] = y[k];
      R[3 * k + 2] = z[k];
    }

    return t;
  }

  // every float of an integrated pose and motion is finite (a column of length zero gives NaNs: false)
  OB_HD bool step_state_finite(datum_ocean_body const &b, datum_ocean_body_motion const &mo)
  {
    bool ok = !drag_motion_bad(mo);

    for(int k = 0; k < 9; ++k)
      ok = ok && body_finite(b.rotation[k]);

    for(int k = 0; k < 3; ++k)
      ok = ok && body_finite(b.position[k]);

    return ok;
  }
}
