// ocean_phase.h -- the arithmetic the choice between the two row-pass instantiations rests on, stated once: the range an uploaded phase
// must lie in for the fused advance, the fused advance itself (one conditional subtraction), the general advance (fmod), the host's rule
// for a queued dt, and the sin / cos that takes a phase from anywhere.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/phase_emul.cpp, tests/test_phase_emul.py): the kernels of ocean_kernels.hip
// and the host code of ocean_capi.hip call these functions, there is no second copy.  Built with -ffp-contract=off wherever it is
// built: products and sums are rounded as written, the FMAs are asked for by name.

#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define OP_HD __host__ __device__ __forceinline__
#else
#define OP_HD inline
#endif

namespace ocean
{
  //|---------------------- two slots per value --------------------------------
  // gfx950's packed fp32 instructions do two floats per lane per issue (ocean_kernels.hip, "two slots per instruction"); a host compiler
  // takes the same text element by element
#if defined(__clang__)
  typedef float f2_ __attribute__((ext_vector_type(2)));

  OP_HD f2_ pfma2(f2_ a, f2_ b, f2_ c) { return __builtin_elementwise_fma(a, b, c); }
#else
  typedef float f2_ __attribute__((vector_size(8)));

  OP_HD f2_ pfma2(f2_ a, f2_ b, f2_ c) { return f2_{ fmaf(a[0], b[0], c[0]), fmaf(a[1], b[1], c[1]) }; }
#endif

  //|---------------------- update_ocean ---------------------------------------

  // fmod(phase + w*dt, 2 pi) of ocean.cpp:231, any operands (phase-only kernel).  fmod is exact.
  OP_HD float advance_phase(float phase, float wdt)
  {
    return fmodf(phase + wdt, 6.2831855f);
  }

  // does a stored phase lie in [0, 2 pi)?  (ocean_phaserange_kernel over an uploaded array: the fused advance below is exact only
  // inside.  -0.0 lies inside; a NaN lies nowhere)
  OP_HD bool phase_in_range(float p)
  {
    return p >= 0.0f && p < 6.2831855f;
  }

  // The fused row pass is given 0 <= phase < 2 pi and 0 <= w*dt < 2 pi -- the host checks both (phase_in_range, dt_fusable) and otherwise
  // runs the phase-only kernel first: then 0 <= a < 4 pi and fmod(a, 2 pi) is a or a - 2 pi, the subtraction being exact (Sterbenz),
  // bit-identical to advance_phase's.  The select of one slot ...
  OP_HD float fused_advance_select(float sum, float wrapped)
  {
    return (sum >= 6.2831855f) ? wrapped : sum;
  }

  // ... and two slots per instruction: a = phase + w, b = a - 2 pi (the roundings of phase + w dt, see advance_phase), then the select
  OP_HD f2_ fused_advance_pair(f2_ phase, f2_ w)
  {
    f2_ const sum = phase + w;
    f2_ const wrapped = sum - f2_{ 6.2831855f, 6.2831855f };

    return f2_{ fused_advance_select(sum[0], wrapped[0]), fused_advance_select(sum[1], wrapped[1]) };
  }

  // The host's rule for one queued dt and one cascade (omegamax: the largest dispersion of the cascade, its table's corner): the fused
  // advance may take it.  6 rather than 2 pi: w = omega * dt is rounded, and every w of the table is at most RN(omegamax * dt).  A NaN
  // fails both comparisons.
  OP_HD bool dt_fusable(float dt, float omegamax)
  {
    return dt >= 0.0f && omegamax * dt < 6.0f;
  }

  // ... and whether the general advance keeps a phase inside [0, 2 pi): fmod keeps the sign of its first operand, so a negative dt
  // (or a NaN) can leave phases below zero, which the fused advance must never see -- every cascade is "wild" from then on, until it
  // is given a new state
  OP_HD bool dt_keeps_range(float dt)
  {
    return dt >= 0.0f;
  }

  //|---------------------- ocean.sim: sin and cos of any phase ----------------

  // sin and cos of the phase (sim.comp:61-62) and of the swell phase (gen.comp:99).  update_ocean keeps the phase in [0, 2 pi), so the
  // argument reduction is a two-constant Cody-Waite step to [-pi/4, pi/4] followed by the Cephes single-precision minimax polynomials:
  // about 1 ulp there (measured against float64 in tests/test_phase_emul.py), at a quarter of the instructions and registers of the
  // all-range libm path.
  //
  // Far outside -- the swell phase of a ray at the horizon is 1e5 .. 1e6 -- two things grow with |x| (tests/test_gen64.py measures both
  // up to |x| = 2^21, profiles/gen_pointwise_table.txt):
  //   * pi/2 is HEAD + TAIL only to 1.72e-15, so the reduced argument is off by 1.09e-15 = 2^-49.7 per unit of x: 2.3e-9 at 2^21,
  //     a hundredth of the polynomials' own error.  A third constant would buy nothing below |x| = 2^26;
  //   * the quarter-turn count rint(x * 2/pi) is taken from a ROUNDED product with a rounded constant (4e-8 relative): next to a
  //     quadrant boundary it can be off by one, at |x| = 2^21 wherever the fraction lies within 0.15 of one half.  The reduced
  //     argument then reaches 1.02 instead of pi/4 and the polynomials leave their interval: 3.7e-7 at 2^20 <= |x| < 2^21 (nothing
  //     above 1.1e-7 below 2^20) before the second step below was added.  One more Cody-Waite step on the reduced argument -- its count
  //     is -1, 0 or 1 -- brings it back to [-pi/4, pi/4]; where the first count was right the step multiplies by zero and changes no bit.
  // With it the error stays below 4 * 2^-24 + |x| * 2^-49.7 up to |x| = 2^21 (measured 1.04e-7).  Beyond, accuracy is lost gradually, as
  // GLSL's own sin / cos lose it.
  OP_HD void sincos_phase(float x, float *sin_out, float *cos_out)
  {
    float k = rintf(x * 0.636619772367581343f);                 // x * 2/pi

    float r = fmaf(k, -1.57079637050628662109375f, x);          // pi/2 head
    r = fmaf(k, 4.37113900018624283e-8f, r);                    // pi/2 tail

    float const k2 = rintf(r * 0.636619772367581343f);          // -1, 0, 1: the first count was a rounded product's
    r = fmaf(k2, -1.57079637050628662109375f, r);               // (exact: r and pi/2 within a factor of two of each other, or k2 = 0)
    r = fmaf(k2, 4.37113900018624283e-8f, r);
    k += k2;

    float z = r * r;

    float sp = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * r, r);
    float cp = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z * z, fmaf(z, -0.5f, 1.0f));

    int q = (int)k;

    float s = (q & 1) ? cp : sp;
    float c = (q & 1) ? sp : cp;

    *sin_out = (q & 2) ? -s : s;
    *cos_out = ((q + 1) & 2) ? -c : c;
  }

  // sincos_phase of two arguments: the same reduction and polynomials, packed
  OP_HD void sincos_phase_pair_poly(f2_ x, f2_ &sn, f2_ &cs)
  {
    f2_ const t = x * 0.636619772367581343f;                            // x * 2/pi
    f2_ k = { __builtin_rintf(t[0]), __builtin_rintf(t[1]) };

    f2_ r = pfma2(k, f2_{ -1.57079637050628662109375f, -1.57079637050628662109375f }, x);       // pi/2 head
    r = pfma2(k, f2_{ 4.37113900018624283e-8f, 4.37113900018624283e-8f }, r);                    // pi/2 tail

    f2_ const t2 = r * 0.636619772367581343f;                           // the second step of sincos_phase
    f2_ const k2 = { __builtin_rintf(t2[0]), __builtin_rintf(t2[1]) };

    r = pfma2(k2, f2_{ -1.57079637050628662109375f, -1.57079637050628662109375f }, r);
    r = pfma2(k2, f2_{ 4.37113900018624283e-8f, 4.37113900018624283e-8f }, r);
    k += k2;

    f2_ const z = r * r;

    f2_ const sp = pfma2(pfma2(pfma2(f2_{ -1.9515295891e-4f, -1.9515295891e-4f }, z, f2_{ 8.3321608736e-3f, 8.3321608736e-3f }), z, f2_{ -1.6666654611e-1f, -1.6666654611e-1f }), z * r, r);
    f2_ const cp = pfma2(pfma2(pfma2(f2_{ 2.443315711809948e-5f, 2.443315711809948e-5f }, z, f2_{ -1.388731625493765e-3f, -1.388731625493765e-3f }), z, f2_{ 4.166664568298827e-2f, 4.166664568298827e-2f }), z * z, pfma2(z, f2_{ -0.5f, -0.5f }, f2_{ 1.0f, 1.0f }));

    #pragma unroll
    for(int i = 0; i < 2; ++i)
    {
      int const q = (int)k[i];

      float const s_ = (q & 1) ? cp[i] : sp[i];
      float const c_ = (q & 1) ? sp[i] : cp[i];

      sn[i] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, s_) ^ (((unsigned)q << 30) & 0x80000000u));
      cs[i] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, c_) ^ (((unsigned)(q + 1) << 30) & 0x80000000u));
    }
  }
}
