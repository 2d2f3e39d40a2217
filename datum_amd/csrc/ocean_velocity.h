// ocean_velocity.h -- the spectrum of the surface velocity (include/datum_ocean_hip.h, "surface velocity"), stated once.
//
// The maps are a linear function of h0 e^{i phase} with d phase / dt = omega(k), so their time derivative at a fixed texel is the same
// pair of transforms applied to the derivative of ocean.sim's fields with respect to the phase, times omega:
//
//     ht.re = omega ( -(a.x + m.x) sin - (a.y + m.y) cos )            a = h0[k], m = h0[(N-1-y, N-1-x)]   (sim.comp:59)
//     ht.im = omega (  (a.x - m.x) cos - (a.y - m.y) sin )
//     htx   = ( ht.im k^x, -ht.re k^x ),   hty = ( ht.im k^y, -ht.re k^y )                                  (sim.comp:68-72)
//
// Host/device neutral and free of FMAs, so that a CPU can walk it (tests/cpu/velocity_emul.cpp): every product and sum is rounded as
// written wherever this is built with -ffp-contract=off.  The kernels of ocean_velocity.hip call velocity_khat, velocity_ht and velocity_hk, of
// which velocity_spectrum is made: there is no second copy.

#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define OV_HD __host__ __device__ __forceinline__
#else
#define OV_HD inline
#endif

namespace ocean
{
  struct VelocitySpectrum
  {
    float ht[2], htx[2], hty[2];
  };

  // k^ of sim.comp:52-54 at index (x, y): k = 2 pi (index - N/2) scale, normalised, 0 at k = 0
  OV_HD void velocity_khat(int x, int y, int N, float scale, float *knx, float *kny)
  {
    float const kx = (6.28318530717958647692f * ((float)x - 0.5f * (float)N)) * scale;
    float const ky = (6.28318530717958647692f * ((float)y - 0.5f * (float)N)) * scale;

    *knx = 0.0f;
    *kny = 0.0f;

    if (kx != 0.0f || ky != 0.0f)
    {
      float const len = sqrtf(kx * kx + ky * ky);

      *knx = kx / len;
      *kny = ky / len;
    }
  }

  // one point's ht: a = h0 at the point, m = h0 at ocean.sim's mirror index, (sn, cs) = sin and cos of the point's phase, omega its dispersion
  OV_HD void velocity_ht(float ax, float ay, float mx, float my, float sn, float cs, float omega, float *re, float *im)
  {
    *re = omega * (-(ax + mx) * sn - (ay + my) * cs);
    *im = omega * ((ax - mx) * cs - (ay - my) * sn);
  }

  // htx or hty from ht and the component of k^: ( ht.im k^, -ht.re k^ )
  OV_HD void velocity_hk(float re, float im, float kn, float *out)
  {
    out[0] = im * kn;
    out[1] = -re * kn;
  }

  // the three fields of one point, from the two parts above (the kernels call the parts: ht once per point, velocity_hk once per field)
  OV_HD VelocitySpectrum velocity_spectrum(float ax, float ay, float mx, float my, float sn, float cs, float omega, float knx, float kny)
  {
    VelocitySpectrum v;

    velocity_ht(ax, ay, mx, my, sn, cs, omega, &v.ht[0], &v.ht[1]);
    velocity_hk(v.ht[0], v.ht[1], knx, v.htx);
    velocity_hk(v.ht[0], v.ht[1], kny, v.hty);

    return v;
  }
}
