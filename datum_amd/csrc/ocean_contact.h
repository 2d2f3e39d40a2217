// ocean_contact.h -- body contact (include/datum_ocean_hip.h: datum_ocean_step_bodies_contact) stated once: the ground under a probe and
// the wall shapes round it, the force one touching contact adds, the eight contact sums beside the coupled sub-step's fourteen, the
// advance under totals that carry them, and the sixteen-float record.  The fourteen sums, the rippled record and the record's fold are
// coupled stepping's (ocean_couple.h), the integrator body stepping's (ocean_step.h: step_integrate, as it stands), the patch of the depth
// map the ripple bed's (ocean_ripple_bed.h: ripple_bed_patch), the cover test the ripple walls' (ocean_ripple_wall.h), unchanged: this
// header calls them and restates none of them.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/contact_emul.cpp, tests/test_contact_emul.py): ocean_contact_kernel of
// ocean_contact.hip calls these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product,
// sum and quotient is one fp32 operation, rounded as written; division and sqrtf are the correctly rounded ones.

#pragma once

#include "ocean_couple.h"
#include "ocean_ripple_bed.h"

namespace ocean
{
  static_assert(sizeof(datum_ocean_body_contact) == 32, "the contact parameters are 32 bytes");
  static_assert(DATUM_OCEAN_CONTACT_RECORD_FLOATS == 16, "a contact record is four 16-byte stores");

  constexpr unsigned int CONTACT_FLAGS = DATUM_OCEAN_CONTACT_BED | DATUM_OCEAN_CONTACT_WALLS;

  // the contact's sums beside the coupled fourteen: F, tau, the count of touching contacts, the deepest penetration (a maximum)
  constexpr int CONTACT_FIELDS = 8;

  struct ContactPartial
  {
    CouplePartial c;
    float k[CONTACT_FIELDS];
  };

  OB_HD ContactPartial contact_zero()
  {
    ContactPartial p;
    p.c = couple_zero();
    for(int k = 0; k < CONTACT_FIELDS; ++k)
      p.k[k] = 0.0f;
    return p;
  }

  // the eight contact fields alone: seven sums and the maximum
  OB_HD void contact_add(float *p, float const *t)
  {
    for(int k = 0; k < CONTACT_FIELDS - 1; ++k)
      p[k] = p[k] + t[k];

    p[CONTACT_FIELDS - 1] = fmaxf(p[CONTACT_FIELDS - 1], t[CONTACT_FIELDS - 1]);
  }

  // the eight contact fields as a partial of their own: a walk over the probes may sum them apart from the fourteen (each field's
  // chain of additions is the same either way)
  struct ContactSums
  {
    float k[CONTACT_FIELDS];
  };

  OB_HD void body_add(ContactSums &p, ContactSums const &t)
  {
    contact_add(p.k, t.k);
  }

  // body_add for the twenty-two fields: the coupled fourteen as they are added there, then the contact's eight
  OB_HD void body_add(ContactPartial &p, ContactPartial const &t)
  {
    body_add(p.c, t.c);
    contact_add(p.k, t.k);
  }

  // the device copy of a wall record keeps inv2 = (float)(1.0 / (axis[0]^2 + axis[1]^2)) in the bits of `reserved`, which no other reader
  // of the list looks at: the host forms it in double and rounds once (contact_wall_prepare; ocean_capi.hip calls it for every record)
  inline void contact_wall_prepare(datum_ocean_ripple_wall &w)
  {
    double const ax = (double)w.axis[0], ay = (double)w.axis[1];

    w.reserved = __builtin_bit_cast(int, (float)(1.0 / (ax * ax + ay * ay)));
  }

  OB_HD float contact_wall_inv2(datum_ocean_ripple_wall const &w)
  {
    return __builtin_bit_cast(float, w.reserved);
  }

  // a contact: the penetration and the normal; it touches when p > 0
  struct Contact
  {
    float p;
    float n[3];
  };

  // the ground under w: the elevation is 0 - raw of the bed's patch (unclamped, `outside` off the map), the normal the patch's slopes
  // normalised, straight up off the map
  template<class Texel>
  OB_HD Contact contact_ground(RippleBed const &b, BodyWorld const &w, Texel &&texel)
  {
    RippleBedPatch const g = ripple_bed_patch(b, w.x, w.y, texel);

    float const zg = 0.0f - g.raw;

    // (selects, not branches: off the map the slopes are +0 and l is 1)
    float const l = step_norm(g.gx, g.gy, 1.0f);

    Contact c;
    c.p = zg - w.z;
    c.n[0] = g.inside ? g.gx / l : 0.0f;
    c.n[1] = g.inside ? g.gy / l : 0.0f;
    c.n[2] = g.inside ? 1.0f / l : 1.0f;
    return c;
  }

  // a shape at (w.x, w.y) (the caller asks ripple_wall_covers whether it counts): u, v as the raster rule has them, the local penetration
  // and normal of the shape, the normal turned by the axis as given, the penetration times inv2
  OB_HD Contact contact_wall(datum_ocean_ripple_wall const &s, BodyWorld const &w)
  {
    float const dx = w.x - s.center[0], dy = w.y - s.center[1];
    float const u = dx * s.axis[0] + dy * s.axis[1];
    float const v = dy * s.axis[0] - dx * s.axis[1];

    float q, mx, my;

    // (selects inside a kind, not branches: a quotient by zero in the arm that is not taken is thrown away)
    if (s.kind == DATUM_OCEAN_RIPPLE_WALL_BOX)
    {
      float const px = s.half[0] - fabsf(u), py = s.half[1] - fabsf(v);
      bool const first = px <= py;

      q = first ? px : py;
      mx = first ? (u >= 0.0f ? 1.0f : -1.0f) : 0.0f;
      my = first ? 0.0f : (v >= 0.0f ? 1.0f : -1.0f);
    }
    else
    {
      float const eu = u / s.half[0], ev = v / s.half[1];
      float const rho = sqrtf(eu * eu + ev * ev);

      q = (1.0f - rho) * fminf(s.half[0], s.half[1]);

      float const lx = eu / s.half[0], ly = ev / s.half[1];
      float const l = sqrtf(lx * lx + ly * ly);

      mx = rho == 0.0f ? 1.0f : lx / l;
      my = rho == 0.0f ? 0.0f : ly / l;
    }

    Contact c;
    c.p = q * contact_wall_inv2(s);
    c.n[0] = mx * s.axis[0] - my * s.axis[1];
    c.n[1] = mx * s.axis[1] + my * s.axis[0];
    c.n[2] = 0.0f;
    return c;
  }

  // the eight terms of ONE touching contact c of a probe at w with weight a: the normal force clamped at 0 from below, the viscous
  // tangential force, their torque about the body origin, a count of one and the penetration
  OB_HD void contact_force(float *t, datum_ocean_body const &b, datum_ocean_body_motion const &mo, datum_ocean_body_contact const &k, BodyWorld const &w, float a,
                           Contact const &c)
  {
    float const rx = w.x - b.position[0], ry = w.y - b.position[1], rz = w.z - b.position[2];

    float const *v = mo.linear, *o = mo.angular;

    // the hull's velocity at the probe, v + omega x r (drag_terms' form)
    float const ux = v[0] + (o[1] * rz - o[2] * ry);
    float const uy = v[1] + (o[2] * rx - o[0] * rz);
    float const uz = v[2] + (o[0] * ry - o[1] * rx);

    float const vn = (ux * c.n[0] + uy * c.n[1]) + uz * c.n[2];
    float const fn = fmaxf(a * (k.stiffness * c.p - k.damping * vn), 0.0f);
    float const g = a * k.friction;

    float const fx = fn * c.n[0] - g * (ux - vn * c.n[0]);
    float const fy = fn * c.n[1] - g * (uy - vn * c.n[1]);
    float const fz = fn * c.n[2] - g * (uz - vn * c.n[2]);

    t[0] = fx;
    t[1] = fy;
    t[2] = fz;
    t[3] = ry * fz - rz * fy;
    t[4] = rz * fx - rx * fz;
    t[5] = rx * fy - ry * fx;
    t[6] = 1.0f;
    t[7] = c.p;
  }

  // a probe's sums take the contact c where it applies (the ground always, a shape where it covers the probe) and touches
  OB_HD void contact_take(float *sum, datum_ocean_body const &b, datum_ocean_body_motion const &mo, datum_ocean_body_contact const &k, BodyWorld const &w, float a,
                          Contact const &c, bool applies)
  {
    if (applies && c.p > 0.0f)
    {
      float t[CONTACT_FIELDS];

      contact_force(t, b, mo, k, w, a, c);
      contact_add(sum, t);
    }
  }

  // what the call looks at: the parameters, and the bed and the list only where their flag is set (the host refuses a flag without its
  // object, so `bed` is valid under BED and `walls`, `nwalls` under WALLS)
  struct ContactScene
  {
    datum_ocean_body_contact k;
    RippleBed bed;
    datum_ocean_ripple_wall const *walls;       // the handle's copy: inv2 in `reserved`
    int nwalls;
  };

  // what the ground adds to a probe's sums: its contact where it touches.  texel(index) returns the depth map's texel
  template<class Texel>
  OB_HD void contact_ground_terms(float *sum, datum_ocean_body const &b, datum_ocean_body_motion const &mo, ContactScene const &s, BodyWorld const &w, float a, Texel &&texel)
  {
    contact_take(sum, b, mo, s.k, w, a, contact_ground(s.bed, w, texel), true);
  }

  // what one shape adds to a probe's sums: nothing unless it covers the probe (asked first: the shape's contact is formed only then),
  // else its contact where it touches
  OB_HD void contact_shape_terms(float *sum, datum_ocean_body const &b, datum_ocean_body_motion const &mo, ContactScene const &s, BodyWorld const &w, float a,
                                 datum_ocean_ripple_wall const &shape)
  {
    if (ripple_wall_covers(shape, w.x, w.y))
      contact_take(sum, b, mo, s.k, w, a, contact_wall(shape, w), true);
  }

  // the eight contact terms of a probe at w with weight a, from +0: the ground's contact where it touches, then every covering shape's
  // that touches, in list order; shape(i) returns record i of the list
  template<class Texel, class Shape>
  OB_HD void contact_terms(float *sum, datum_ocean_body const &b, datum_ocean_body_motion const &mo, ContactScene const &s, BodyWorld const &w, float a, Texel &&texel,
                           Shape &&shape)
  {
    for(int k = 0; k < CONTACT_FIELDS; ++k)
      sum[k] = 0.0f;

    if (s.k.flags & DATUM_OCEAN_CONTACT_BED)
      contact_ground_terms(sum, b, mo, s, w, a, texel);

    if (s.k.flags & DATUM_OCEAN_CONTACT_WALLS)
      for(int i = 0; i < s.nwalls; ++i)
        contact_shape_terms(sum, b, mo, s, w, a, shape(i));
  }

  // One sub-step of length h from the twenty-two sums.  While nothing touches (the count is 0) it is step_integrate on the coupled
  // sums, untouched.  Otherwise the coupled sub-step's totals are step_integrate's own, from an advance of copies that is thrown away
  // (ocean_step.h states the totals nowhere else, and this header restates nothing of it); the contact's force and torque are added, one
  // fp32 addition per component; and the body advances by step_integrate under sums whose drag fields hold those totals, with no
  // buoyancy: its totals are then 0 * 0 + F.z, F.z again (a -0 becomes +0), and its steps 3-5 run on them.  (ocean_step.h is held
  // byte for byte by tests/test_couple_abi.py against its parent commit; once a commit stands between, step_integrate can hand out
  // its totals and its advance apart, and the two calls here become one of each)
  OB_HD StepTotals contact_integrate(datum_ocean_body &b, datum_ocean_body_motion &mo, datum_ocean_body_props const &p, ContactPartial const &s, float h)
  {
    if (s.k[6] == 0.0f)
      return step_integrate(b, mo, p, s.c.s, h);

    datum_ocean_body b0 = b;
    datum_ocean_body_motion m0 = mo;

    StepTotals const t = step_integrate(b0, m0, p, s.c.s, h);

    StepPartial d = step_zero();

    for(int j = 0; j < 3; ++j)
    {
      d.f[3 + j] = t.force[j] + s.k[j];
      d.f[6 + j] = t.torque[j] + s.k[3 + j];
    }

    datum_ocean_body_props q = p;
    q.buoyancy = 0.0f;

    return step_integrate(b, mo, q, d, h);
  }

  struct ContactRecord
  {
    float f[DATUM_OCEAN_CONTACT_RECORD_FLOATS];
  };

  // The record of a sub-step: the coupled record's twelve by couple_fold, the contact force of this sub-step, and the deepest penetration
  // folded over the call's sub-steps by a maximum with the old record's field 15, which the first sub-step does not read
  OB_HD ContactRecord contact_fold(StepTotals const &t, ContactPartial const &sums, bool first, float old7, float old11, float old15)
  {
    CoupleRecord const c = couple_fold(t, sums.c, first, old7, old11);

    ContactRecord r;

    for(int k = 0; k < DATUM_OCEAN_COUPLED_RECORD_FLOATS; ++k)
      r.f[k] = c.f[k];

    for(int k = 0; k < 3; ++k)
      r.f[12 + k] = sums.k[k];

    r.f[15] = first ? sums.k[7] : fmaxf(old15, sums.k[7]);

    return r;
  }
}
