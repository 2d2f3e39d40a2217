// ocean_ripple_foam.h -- wake foam (include/datum_ocean_hip.h: "wake foam") stated once: what a window cell of the ripple layer adds to the
// coverage plane beside it, and the bilinear sample of that plane.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/ripple_foam_emul.cpp, tests/test_ripple_foam_emul.py): the kernels of
// ocean_ripple_foam.hip call these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product
// and sum is one fp32 operation, rounded as written; there is no fused multiply-add here.

#pragma once

#include "ocean_ripple.h"

namespace ocean
{
  // what an update takes but the cells: hinv = 0.5f * invs, the thresholds and gains of the two sources, fade rounded once on the host from
  // exp(-decay dt) in double
  struct RippleFoamParams
  {
    float hinv;
    float t1, k1;
    float t2, k2;
    float fade;
  };

  // fmaxf, with the one case C leaves open decided: of two zeros of opposite sign, +0 (their sum).  A gain of 0 makes a -0 of every cell
  // below its threshold, so the case is met in every plane; with it decided the plane repeats bit for bit on any host and on the device
  OB_HD float ripple_foam_max(float a, float b)
  {
    float const m = fmaxf(a, b);

    return (a == 0.0f && b == 0.0f) ? a + b : m;
  }

  // one update of a cell: et its rate, eL eR eD eU its neighbours' heights (0 outside the window), old its coverage.  FOAM_ACCUMULATE's
  // rule with two sources: the slope squared over t1, and the rate over t2
  OB_HD float ripple_foam_update(float et, float eL, float eR, float eD, float eU, float old, RippleFoamParams const &p)
  {
    float const hx = (eR - eL) * p.hinv;
    float const hy = (eU - eD) * p.hinv;
    float const q = hx * hx + hy * hy;

    float const g1 = (q - p.t1) * p.k1;
    float const g2 = (fabsf(et) - p.t2) * p.k2;
    float const g = fminf(ripple_foam_max(ripple_foam_max(g1, g2), 0.0f), 1.0f);

    return ripple_foam_max(g, old * p.fade);
  }

  // The sample at (x, y): the bilinear patch between the four cell centres around the point, in ripple_sample's u, I0, wx.  cell(index)
  // returns a cell's coverage; cells outside the window read 0 and are not fetched.  A non-finite x or y: NaN, nothing fetched; a finite
  // coordinate beyond 2^30 cells: 0, nothing fetched
  template<class Cell>
  OB_HD float ripple_foam_sample(RippleGrid const &g, float x, float y, Cell &&cell)
  {
    if (!(body_finite(x) && body_finite(y)))
      return __builtin_nanf("");

    if (!(ripple_coord_ok(x, g.invs) && ripple_coord_ok(y, g.invs)))
      return 0.0f;

    RippleAxis const ax = ripple_axis(x, g.invs), ay = ripple_axis(y, g.invs);

    float f[4];

    for(int k = 0; k < 4; ++k)
    {
      int const I = ax.i + (k & 1), J = ay.i + (k >> 1);

      f[k] = 0.0f;

      if (ripple_inside(g, I, J))
        f[k] = cell(ripple_index(I, J, g.R));
    }

    float const f0 = f[0] + ax.w * (f[1] - f[0]), f1 = f[2] + ax.w * (f[3] - f[2]);

    return f0 + ay.w * (f1 - f0);
  }
}
