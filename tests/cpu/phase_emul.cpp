// The phase arithmetic the row pass's dispatch rests on (datum_amd/csrc/ocean_phase.h) behind a C interface, for tests/test_phase_emul.py:
// the very functions the kernels and the host code call, over arrays, no HIP call in sight.

#include <stddef.h>

#include "../../datum_amd/csrc/ocean_phase.h"

using ocean::f2_;

extern "C"
{
  // the fused advance as the row pass takes it -- two slots per call, elements (2i, 2i + 1) -- and the general one, element by element
  void phase_advance(float const *phase, float const *w, size_t n, float *fused, float *general)
  {
    for(size_t i = 0; i + 1 < n; i += 2)
    {
      f2_ const p = ocean::fused_advance_pair(f2_{ phase[i], phase[i + 1] }, f2_{ w[i], w[i + 1] });

      fused[i] = p[0];
      fused[i + 1] = p[1];
    }

    if (n & 1)
      fused[n - 1] = ocean::fused_advance_pair(f2_{ phase[n - 1], 0.0f }, f2_{ w[n - 1], 0.0f })[0];

    for(size_t i = 0; i < n; ++i)
      general[i] = ocean::advance_phase(phase[i], w[i]);
  }

  void phase_in_range(float const *phase, size_t n, unsigned char *inside)
  {
    for(size_t i = 0; i < n; ++i)
      inside[i] = ocean::phase_in_range(phase[i]) ? 1 : 0;
  }

  // sin and cos by the scalar form and by the packed one (elements (2i, 2i + 1); n even)
  void phase_sincos(float const *x, size_t n, float *sn, float *cs, float *sn_pair, float *cs_pair)
  {
    for(size_t i = 0; i < n; ++i)
      ocean::sincos_phase(x[i], &sn[i], &cs[i]);

    for(size_t i = 0; i + 1 < n; i += 2)
    {
      f2_ s, c;
      ocean::sincos_phase_pair_poly(f2_{ x[i], x[i + 1] }, s, c);

      sn_pair[i] = s[0];
      sn_pair[i + 1] = s[1];
      cs_pair[i] = c[0];
      cs_pair[i + 1] = c[1];
    }
  }

  int phase_dt_fusable(float dt, float omegamax) { return ocean::dt_fusable(dt, omegamax) ? 1 : 0; }
  int phase_dt_keeps_range(float dt) { return ocean::dt_keeps_range(dt) ? 1 : 0; }

  // One displace call with dt[0 .. ndt) queued, as ocean_capi.hip decides it (fusable, flush_pending) with the header's two rules: returns 1
  // where the fused row pass advances the phase, 0 where the phase-only kernel does and the any-phase row pass follows, and leaves in
  // wild[cascade] which cascades are wild afterwards (only a new state clears the flag: the caller's business).
  int phase_host_step(float const *dt, int ndt, float const *omegamax, unsigned char *wild, int cascades)
  {
    bool fusable = true;

    for(int c = 0; c < cascades; ++c)
    {
      if (wild[c])
        fusable = false;

      for(int i = 0; i < ndt; ++i)
      {
        if (!ocean::dt_fusable(dt[i], omegamax[c]))
          fusable = false;
      }
    }

    if (ndt == 0)         // nothing to advance: the row pass of the handle's plan, wild or not
      fusable = true;

    if (!fusable)
    {
      for(int i = 0; i < ndt; ++i)
      {
        if (!ocean::dt_keeps_range(dt[i]))
        {
          for(int c = 0; c < cascades; ++c)
            wild[c] = 1;
        }
      }
    }

    bool any = false;

    for(int c = 0; c < cascades; ++c)
      any = any || wild[c];

    return (fusable && !any) ? 1 : 0;
  }
}
