// ocean_couple.h -- coupled stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies_coupled) stated once: the rippled record a probe
// makes of its velocity record and its sample of the ripple layer, the fourteen sums of a coupled sub-step, what one probe adds to them,
// and how a body's record folds from sub-step to sub-step.  The ten sums and the integrator are body stepping's (ocean_step.h), the sample,
// the splat and the wake's terms the ripple layer's (ocean_ripple.h), unchanged: this header calls them and restates none of them.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/couple_emul.cpp, tests/test_couple_emul.py): ocean_couple_kernel of
// ocean_couple.hip calls these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every sum is one
// fp32 operation, rounded as written.

#pragma once

#include "ocean_step.h"
#include "ocean_ripple.h"

namespace ocean
{
  static_assert(DATUM_OCEAN_COUPLED_RECORD_FLOATS == 12, "a coupled record is three 16-byte stores");

  // the wake's sums beside the step's ten: Sum Vh, Sum m sx, Sum m sy, the dropped quanta (wake_terms' fields 0-3)
  constexpr int COUPLE_WAKE_FIELDS = 4;
  constexpr int COUPLE_FIELDS = STEP_FIELDS + COUPLE_WAKE_FIELDS;

  // The rippled record: the velocity record above a probe with the layer's height added to the water height and the layer's rate to the
  // water's vertical velocity, one fp32 addition each; every other field is rec's
  OB_HD void couple_record(float *out, float const *rec, RippleSample const &s)
  {
    for(int k = 0; k < DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS; ++k)
      out[k] = rec[k];

    out[2] = rec[2] + s.eta;
    out[6] = rec[6] + s.rate;
  }

  struct CouplePartial
  {
    StepPartial s;
    float w[COUPLE_WAKE_FIELDS];
  };

  OB_HD CouplePartial couple_zero()
  {
    CouplePartial p;
    p.s = step_zero();
    for(int k = 0; k < COUPLE_WAKE_FIELDS; ++k)
      p.w[k] = 0.0f;
    return p;
  }

  // body_add for the fourteen fields: the step's ten as they are added there (the tenth the maximum), the wake's four sums
  OB_HD void body_add(CouplePartial &p, CouplePartial const &t)
  {
    body_add(p.s, t.s);

    for(int k = 0; k < COUPLE_WAKE_FIELDS; ++k)
      p.w[k] = p.w[k] + t.w[k];
  }

  // the terms of a probe at w with weight a, given its RIPPLED record: the step's ten and the wake's four from the same record.  splat(x,
  // y, V) deposits and returns the dropped quanta (wake_terms)
  template<class Splat>
  OB_HD CouplePartial couple_terms(datum_ocean_body const &b, datum_ocean_body_motion const &mo, BodyWorld const &w, float a, float const *rec, float h, Splat &&splat)
  {
    CouplePartial t;
    t.s = step_terms(b, mo, w, a, rec);

    BodyPartial const wake = wake_terms(b, mo, w, a, rec, h, splat);

    for(int k = 0; k < COUPLE_WAKE_FIELDS; ++k)
      t.w[k] = wake.f[k];

    return t;
  }

  struct CoupleRecord
  {
    float f[DATUM_OCEAN_COUPLED_RECORD_FLOATS];
  };

  // a body that went bad in an earlier sub-step of the call: its record's first float is a NaN (a good body's is F.x, finite: a
  // non-finite force does not leave a finite motion behind)
  OB_HD bool couple_was_bad(float old0)
  {
    return old0 != old0;
  }

  // The record of a sub-step: F, tau and M of this sub-step, the wake's three sums of this sub-step; the residual and the dropped quanta
  // fold over the call's sub-steps -- the maximum and the sum with the old record's fields 7 and 11, which the first sub-step does not read
  OB_HD CoupleRecord couple_fold(StepTotals const &t, CouplePartial const &sums, bool first, float old7, float old11)
  {
    CoupleRecord r;

    for(int k = 0; k < 3; ++k)
    {
      r.f[k] = t.force[k];
      r.f[3 + k] = t.torque[k];
      r.f[8 + k] = sums.w[k];
    }

    r.f[6] = sums.s.f[0];
    r.f[7] = first ? sums.s.f[STEP_FIELDS - 1] : fmaxf(old7, sums.s.f[STEP_FIELDS - 1]);
    r.f[11] = first ? sums.w[3] : old11 + sums.w[3];

    return r;
  }
}
