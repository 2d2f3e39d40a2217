// ocean_ripple_deep.h -- the ripple layer's DEEP step (include/datum_ocean_hip.h: "dispersive ripples") stated once: the 13 x 13
// convolution that stands for sqrt(-Laplacian), the rest of a cell's sub-step, and the host-only construction of the weights.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/ripple_deep_emul.cpp, tests/test_ripple_deep_emul.py): the kernel of
// ocean_ripple_deep.hip calls these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product
// and sum is one fp32 operation, rounded as written.  The window test, the sponge index, the height a sub-step reads and the
// cell are ocean_ripple.h's.

#pragma once

#include <math.h>

#include "ocean_ripple.h"

#if defined(__HIPCC__)
#define OB_UNROLL _Pragma("unroll")
#else
#define OB_UNROLL
#endif

namespace ocean
{
  constexpr int RIPPLE_DEEP_P = DATUM_OCEAN_RIPPLE_DEEP_RADIUS;       // the stencil reaches P cells each way
  constexpr int RIPPLE_DEEP_Q = RIPPLE_DEEP_P + 1;                     // a side of the quadrant table G[l][k], l = |dj|, k = |di|
  constexpr int RIPPLE_DEEP_WEIGHTS = RIPPLE_DEEP_Q * RIPPLE_DEEP_Q;   // 49

  static_assert(RIPPLE_DEEP_WEIGHTS == DATUM_OCEAN_RIPPLE_DEEP_WEIGHTS, "the table the getter returns");

  OB_HD int ripple_deep_abs(int d)
  {
    return d < 0 ? -d : d;
  }

  // one row of the sum: acc = acc + Gl[|di|] * e(di) for di = -P .. P in that order; Gl is row l = |dj| of the table
  template<class Row>
  OB_HD float ripple_deep_row(float acc, float const *Gl, Row &&e)
  {
    OB_UNROLL
    for(int di = -RIPPLE_DEEP_P; di <= RIPPLE_DEEP_P; ++di)
      acc = acc + Gl[ripple_deep_abs(di)] * e(di);

    return acc;
  }

  // the sum over the 169 cells round a cell: dj outer, di inner, from 0.0f.  e(di, dj) is the height of cell (I + di, J + dj) as the
  // sub-step reads it, 0.0f where that cell lies outside the window.  (A row of zeros leaves acc as it is, bit for bit: acc is never -0.)
  template<class Height>
  OB_HD float ripple_deep_conv(float const *G, Height &&e)
  {
    float acc = 0.0f;

    OB_UNROLL
    for(int dj = -RIPPLE_DEEP_P; dj <= RIPPLE_DEEP_P; ++dj)
      acc = ripple_deep_row(acc, G + RIPPLE_DEEP_Q * ripple_deep_abs(dj), [&](int di) { return e(di, dj); });

    return acc;
  }

  // the rest of a cell's sub-step: e its height, et its rate, acc the sum above, gs = g / s, f the sponge factor
  OB_HD RippleCell ripple_deep_update(float e, float et, float acc, float h, float gs, float f)
  {
    float const v1 = (et - h * (gs * acc)) * f;

    RippleCell c;
    c.rate = v1;
    c.eta = e + h * v1;
    return c;
  }

  // HOST ONLY.  The weights, in double (the header's three steps).  G[l][k] receives the 49 fp32 weights; the return value is
  // Sum |F| over the 169 fp32 weights, in double, which the stability bound uses
  inline double ripple_deep_weights(float *G)
  {
    constexpr int M = 1024, Q = RIPPLE_DEEP_Q;
    double const step = 2.0 * 3.14159265358979323846 / M;

    double c[Q][M];

    for(int k = 0; k < Q; ++k)
      for(int a = 0; a < M; ++a)
        c[k][a] = cos(k * (step * (a - M / 2)));

    // 1: the truncated Fourier series of the cone, separably: first over b for every a and l, then over a
    double G0[Q][Q] = {};

    for(int a = 0; a < M; ++a)
    {
      double const ta = step * (a - M / 2);
      double t[Q] = {};

      for(int b = 0; b < M; ++b)
      {
        double const tb = step * (b - M / 2);
        double const r = sqrt(ta * ta + tb * tb);

        for(int l = 0; l < Q; ++l)
          t[l] += r * c[l][b];
      }

      for(int l = 0; l < Q; ++l)
        for(int k = 0; k < Q; ++k)
          G0[l][k] += t[l] * c[k][a];
    }

    // 2: the mean of the 169 unfolded weights comes off every one; each is rounded to fp32
    auto const fold = [](int i) { return i == 0 ? 1.0 : 2.0; };

    double total = 0.0;

    for(int l = 0; l < Q; ++l)
      for(int k = 0; k < Q; ++k)
      {
        G0[l][k] /= (double)M * M;
        total += fold(l) * fold(k) * G0[l][k];
      }

    for(int l = 0; l < Q; ++l)
      for(int k = 0; k < Q; ++k)
        G[Q * l + k] = (float)(G0[l][k] - total / ((2 * Q - 1) * (2 * Q - 1)));

    // 3: the centre makes the sum of the 169 fp32 weights, taken in double, the smallest value >= 0
    double rest = 0.0, mass = 0.0;

    for(int dj = -RIPPLE_DEEP_P; dj <= RIPPLE_DEEP_P; ++dj)
      for(int di = -RIPPLE_DEEP_P; di <= RIPPLE_DEEP_P; ++di)
        if (di != 0 || dj != 0)
        {
          double const w = (double)G[Q * ripple_deep_abs(dj) + ripple_deep_abs(di)];

          rest += w;
          mass += fabs(w);
        }

    float centre = (float)-rest;

    if (rest + (double)centre < 0.0)
      centre = nextafterf(centre, INFINITY);

    G[0] = centre;

    return mass + fabs((double)centre);
  }
}
