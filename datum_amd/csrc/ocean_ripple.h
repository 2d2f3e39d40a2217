// ocean_ripple.h -- the ripple layer (include/datum_ocean_hip.h: "ripple layer") stated once: which memory cell holds a world cell, the
// window test, the sponge index, the sub-step of a cell, the integer splat of a deposit, the bilinear sample, and the terms a hull probe
// contributes to its body's wake.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/ripple_emul.cpp, tests/test_ripple_emul.py): the kernels of ocean_ripple.hip
// call these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product and sum is one fp32
// operation, rounded as written; there is no fmaf here.  floorf and rintf (to nearest, ties to even) are exact operations on both sides.

#pragma once

#include "ocean_drag.h"

namespace ocean
{
  constexpr int RIPPLE_MAX_SPONGE = DATUM_OCEAN_RIPPLE_MAX_SPONGE;
  constexpr float RIPPLE_UNIT = 9.5367431640625e-07f;     // 2^-20 m of height: one unit of the src plane
  constexpr float RIPPLE_PER_METRE = 1048576.0f;          // 2^20
  constexpr float RIPPLE_QMAX = 1073741824.0f;            // 2^30: a deposit is clamped to +-2^30 units, a cell coordinate lies below it

  static_assert(DATUM_OCEAN_RIPPLE_RECORD_FLOATS == BODY_FIELDS, "the wake's record is a BodyPartial: body_add and body_tree as they are");

  // the layer as the arithmetic sees it: R a power of two, the window's origin in cells, 1 / s rounded once on the host from double
  struct RippleGrid
  {
    int R;
    int ox, oy;
    float invs;
  };

  // world cell (I, J) lives at (J mod R) * R + (I mod R), mod the floor one: a torus in memory
  OB_HD int ripple_wrap(int i, int R)
  {
    return i & (R - 1);
  }

  OB_HD int ripple_index(int I, int J, int R)
  {
    return ripple_wrap(J, R) * R + ripple_wrap(I, R);
  }

  // The window at origin (ox, oy) as it lies in memory, for a host that copies a plane out in window order: window columns [0, R - mx)
  // are memory columns [mx, R) and the rest memory columns [0, mx), mx = ox mod R; rows likewise.  One to four rectangles, split where
  // the window wraps, none empty: cell offsets into the plane in memory (from) and into the R x R window (to), width and height in
  // cells.  Returns their number.  No kernel calls it
  struct RippleRect { int from, to, w, h; };

  inline int ripple_window(int ox, int oy, int R, RippleRect rect[4])
  {
    int const mx = ripple_wrap(ox, R), my = ripple_wrap(oy, R);

    int const w[2] = { R - mx, mx }, h[2] = { R - my, my };
    int const sx[2] = { mx, 0 }, sy[2] = { my, 0 }, dx[2] = { 0, R - mx }, dy[2] = { 0, R - my };

    int n = 0;

    for(int j = 0; j < 2; ++j)
      for(int i = 0; i < 2; ++i)
        if (w[i] > 0 && h[j] > 0)
          rect[n++] = RippleRect{ sy[j] * R + sx[i], dy[j] * R + dx[i], w[i], h[j] };

    return n;
  }

  // ox <= I < ox + R and the same for J (the difference taken modulo 2^32: no I, ox below 2^30 + R in size can alias)
  OB_HD bool ripple_inside(RippleGrid const &g, int I, int J)
  {
    return ((unsigned int)I - (unsigned int)g.ox) < (unsigned int)g.R && ((unsigned int)J - (unsigned int)g.oy) < (unsigned int)g.R;
  }

  // sponge index of the window cell (wx, wy), 0 <= wx, wy < R: B less its distance in cells to the nearest edge, not below 0.  The
  // outermost ring has k = B
  OB_HD int ripple_sponge(int wx, int wy, int R, int B)
  {
    int const dx = wx < R - 1 - wx ? wx : R - 1 - wx;
    int const dy = wy < R - 1 - wy ? wy : R - 1 - wy;
    int const d = dx < dy ? dx : dy;

    return B - d > 0 ? B - d : 0;
  }

  // the height a sub-step reads: in a step's first sub-step with the pending deposits of that cell
  OB_HD float ripple_height(float eta, int src, bool first)
  {
    return first ? eta + (float)src * RIPPLE_UNIT : eta;
  }

  struct RippleCell { float eta, rate; };

  // one sub-step of a cell: e its height, et its rate, eL eR eD eU its neighbours' heights (0 outside the window), f the sponge factor
  OB_HD RippleCell ripple_update(float e, float et, float eL, float eR, float eD, float eU, float h, float c2s2, float f)
  {
    float const lap = ((eL + eR) + (eD + eU)) - 4.0f * e;
    float const v1 = (et + h * (c2s2 * lap)) * f;

    RippleCell c;
    c.rate = v1;
    c.eta = e + h * v1;
    return c;
  }

  // a coordinate that can be turned into a cell: finite, and |x invs| < 2^30 (false for a NaN)
  OB_HD bool ripple_coord_ok(float x, float invs)
  {
    return body_finite(x) && fabsf(x * invs) < RIPPLE_QMAX;
  }

  // the cell whose centre lies at or below x, and x's weight towards the next one: centres stand at (I + 1/2) s
  struct RippleAxis { int i; float w; };

  OB_HD RippleAxis ripple_axis(float x, float invs)
  {
    float const u = x * invs - 0.5f;
    float const fl = floorf(u);

    RippleAxis a;
    a.i = (int)fl;
    a.w = u - fl;
    return a;
  }

  // The integer splat of a volume V (m^3) at (x, y): Q = rint(V invs^2 2^20) units, clamped, shared between the four cells around
  // (x, y) in the order 00, 10, 01, 11 so that the four quanta add up to Q exactly.  add(index, q) receives every non-zero quantum
  // whose cell lies in the window; the return value counts the non-zero quanta whose cell does not (they are dropped).  A non-finite
  // x, y or V, or a coordinate that ripple_coord_ok refuses, deposits nothing and drops nothing
  template<class Add>
  OB_HD int ripple_splat(RippleGrid const &g, float x, float y, float V, Add &&add)
  {
    if (!(ripple_coord_ok(x, g.invs) && ripple_coord_ok(y, g.invs) && body_finite(V)))
      return 0;

    float const units = (V * (g.invs * g.invs)) * RIPPLE_PER_METRE;
    int const Q = (int)rintf(fminf(fmaxf(units, -RIPPLE_QMAX), RIPPLE_QMAX));

    if (Q == 0)
      return 0;

    RippleAxis const ax = ripple_axis(x, g.invs), ay = ripple_axis(y, g.invs);

    float const ux = 1.0f - ax.w, uy = 1.0f - ay.w;
    float const fq = (float)Q;

    int q[4];
    q[0] = (int)rintf(fq * (ux * uy));
    q[1] = (int)rintf(fq * (ax.w * uy));
    q[2] = (int)rintf(fq * (ux * ay.w));
    q[3] = Q - ((q[0] + q[1]) + q[2]);

    int dropped = 0;

    for(int k = 0; k < 4; ++k)
    {
      int const I = ax.i + (k & 1), J = ay.i + (k >> 1);

      if (q[k] == 0)
        continue;

      if (ripple_inside(g, I, J))
        add(ripple_index(I, J, g.R), q[k]);
      else
        ++dropped;
    }

    return dropped;
  }

  // The sample at (x, y): eta, d eta / dx, d eta / dy, the rate -- the bilinear patch between the four cell centres around the point and
  // that patch's own derivative times invs.  cell(index) returns a cell's (eta, rate); cells outside the window read 0 and are not
  // fetched.  A non-finite x or y: four NaNs, nothing fetched; a finite coordinate beyond 2^30 cells: zeros, nothing fetched
  struct RippleSample { float eta, dx, dy, rate; };

  template<class Cell>
  OB_HD RippleSample ripple_sample(RippleGrid const &g, float x, float y, Cell &&cell)
  {
    RippleSample s;

    if (!(body_finite(x) && body_finite(y)))
    {
      float const nan = __builtin_nanf("");
      s.eta = s.dx = s.dy = s.rate = nan;
      return s;
    }

    s.eta = s.dx = s.dy = s.rate = 0.0f;

    if (!(ripple_coord_ok(x, g.invs) && ripple_coord_ok(y, g.invs)))
      return s;

    RippleAxis const ax = ripple_axis(x, g.invs), ay = ripple_axis(y, g.invs);

    RippleCell c[4];

    for(int k = 0; k < 4; ++k)
    {
      int const I = ax.i + (k & 1), J = ay.i + (k >> 1);

      c[k].eta = c[k].rate = 0.0f;

      if (ripple_inside(g, I, J))
        c[k] = cell(ripple_index(I, J, g.R));
    }

    float const a0 = c[1].eta - c[0].eta, a1 = c[3].eta - c[2].eta;         // along x, at the lower and the upper row of centres
    float const e0 = c[0].eta + ax.w * a0, e1 = c[2].eta + ax.w * a1;

    s.eta = e0 + ay.w * (e1 - e0);
    s.dx = (a0 + ay.w * (a1 - a0)) * g.invs;
    s.dy = (e1 - e0) * g.invs;

    float const r0 = c[0].rate + ax.w * (c[1].rate - c[0].rate), r1 = c[2].rate + ax.w * (c[3].rate - c[2].rate);

    s.rate = r0 + ay.w * (r1 - r0);

    return s;
  }

  // The wake of a probe at w with weight a, given the velocity record above (w.x, w.y) -- drag_terms' d, m, u and e, bit for bit.  Heave:
  // a column that is partly wet displaces a (-e.z) dt as it sinks relative to the water.  Surge: the column's displaced volume m moves
  // with the hull relative to the water, taken from where the probe stands and put where it stood dt ago in the water's frame.
  // splat(x, y, V) deposits and returns the dropped quanta.  Sum Vh, Sum m (-e.x dt), Sum m (-e.y dt), dropped, 0, 0, Sum m, residual
  template<class Splat>
  OB_HD BodyPartial wake_terms(datum_ocean_body const &b, datum_ocean_body_motion const &mo, BodyWorld const &w, float a, float const *rec, float dt, Splat &&splat)
  {
    float const d = fminf(fmaxf(rec[2] - w.z, 0.0f), b.cap);
    float const m = a * d;

    float const rx = w.x - b.position[0], ry = w.y - b.position[1], rz = w.z - b.position[2];

    float const *v = mo.linear, *o = mo.angular;

    float const ux = v[0] + (o[1] * rz - o[2] * ry);
    float const uy = v[1] + (o[2] * rx - o[0] * rz);
    float const uz = v[2] + (o[0] * ry - o[1] * rx);

    float const ex = rec[4] - ux, ey = rec[5] - uy, ez = rec[6] - uz;

    float const sx = -(ex * dt), sy = -(ey * dt);       // how far the hull moved through the water

    BodyPartial t = body_zero();
    int dropped = 0;

    if (0.0f < d && d < b.cap)
    {
      float const Vh = (a * -ez) * dt;

      dropped += splat(w.x, w.y, Vh);
      t.f[0] = Vh;
    }

    if (d > 0.0f)
    {
      dropped += splat(w.x, w.y, -m);
      dropped += splat(w.x + sx, w.y + sy, m);
      t.f[1] = m * sx;
      t.f[2] = m * sy;
    }

    t.f[3] = (float)dropped;
    t.f[6] = m;
    t.f[7] = rec[3];
    return t;
  }
}
