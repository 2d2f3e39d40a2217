// ocean_ripple_bed.h -- the ripple bed (include/datum_ocean_hip.h: "ripple bed") stated once: the depth a world cell reads from the map,
// the effective depth and the surf level of a cell, the flux through a face of a cell, and the sub-step of a cell over a bed.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/ripple_bed_emul.cpp, tests/test_ripple_bed_emul.py): the kernels of
// ocean_ripple_bed.hip call these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product
// and sum is one fp32 operation, rounded as written; there is no fused multiply-add here and no quotient: the host rounds 1 / texel and
// 1 / surf_depth once from double.  The torus, the window test, the cell centre and the height a sub-step reads are ocean_ripple.h's and
// ocean_ripple_wall.h's, called or restated as they stand.

#pragma once

#include "ocean_ripple_wall.h"

namespace ocean
{
  constexpr int RIPPLE_SURF_LEVELS = DATUM_OCEAN_RIPPLE_SURF_LEVELS;
  constexpr int RIPPLE_BED_MAX_SIDE = DATUM_OCEAN_RIPPLE_BED_MAX_SIDE;

  static_assert(sizeof(datum_ocean_ripple_bed) == 40, "a bed is a 40-byte record");

  // the bed as the arithmetic sees it: datum_ocean_ripple_bed's fields, and 1 / texel and 1 / surf_depth rounded once on the host from
  // double (invsurf is 0 while surf_depth is 0: it is not read then)
  struct RippleBed
  {
    int width, height;
    float ox, oy;
    float invt;
    float outside, max_depth, dry_depth;
    float surf_depth, invsurf;
  };

  // the bilinear patch at (x, y): `outside` and no slope off the map (a NaN coordinate is off the map), else the patch of the four texels
  // round the point in ripple_sample's form, the lower index floor, clamped so that the upper one is a texel, and its two slopes per
  // metre, ripple_sample's again.  texel(index) returns map[index]
  struct RippleBedPatch
  {
    float raw, gx, gy;
    bool inside;
  };

  template<class Texel>
  OB_HD RippleBedPatch ripple_bed_patch(RippleBed const &b, float x, float y, Texel &&texel)
  {
    float const u = (x - b.ox) * b.invt, v = (y - b.oy) * b.invt;

    RippleBedPatch p;

    if (!(u >= 0.0f && u <= (float)(b.width - 1) && v >= 0.0f && v <= (float)(b.height - 1)))
    {
      p.raw = b.outside;
      p.gx = p.gy = 0.0f;
      p.inside = false;
      return p;
    }

    int const fi = (int)floorf(u), fj = (int)floorf(v);
    int const i = fi < b.width - 2 ? fi : b.width - 2, j = fj < b.height - 2 ? fj : b.height - 2;

    float const wu = u - (float)i, wv = v - (float)j;

    float const c0 = texel(j * b.width + i), c1 = texel(j * b.width + i + 1);
    float const c2 = texel((j + 1) * b.width + i), c3 = texel((j + 1) * b.width + i + 1);

    float const a0 = c1 - c0, a1 = c3 - c2;
    float const e0 = c0 + wu * a0, e1 = c2 + wu * a1;

    p.raw = e0 + wv * (e1 - e0);
    p.gx = (a0 + wv * (a1 - a0)) * b.invt;
    p.gy = (e1 - e0) * b.invt;
    p.inside = true;
    return p;
  }

  // the raw depth at (x, y): the patch's value (the slopes are not formed where nothing reads them)
  template<class Texel>
  OB_HD float ripple_bed_raw(RippleBed const &b, float x, float y, Texel &&texel)
  {
    return ripple_bed_patch(b, x, y, texel).raw;
  }

  // the effective depth: the raw one clamped to [0, max_depth]; +0 -- solid -- below dry_depth and where a wall stands
  OB_HD float ripple_bed_depth(RippleBed const &b, float raw, bool wall)
  {
    float const d = fminf(fmaxf(raw, 0.0f), b.max_depth);

    return (wall || d < b.dry_depth) ? 0.0f : d;
  }

  // the surf level of a cell of effective depth d: 0 on solid cells, without a surf zone and at surf_depth or deeper, else rising to
  // RIPPLE_SURF_LEVELS towards the shore
  OB_HD unsigned char ripple_bed_surf(RippleBed const &b, float d)
  {
    if (d == 0.0f || b.surf_depth == 0.0f || d >= b.surf_depth)
      return 0;

    int const q = (int)floorf((1.0f - d * b.invsurf) * (float)RIPPLE_SURF_LEVELS);

    return (unsigned char)(q < RIPPLE_SURF_LEVELS ? q : RIPPLE_SURF_LEVELS);
  }

  // both planes' values of world cell (I, J): the cell's centre as ripple_wall_cell computes it.  s is the fp32 cell side
  struct RippleBedCell { float d; unsigned char q; };

  template<class Texel>
  OB_HD RippleBedCell ripple_bed_cell(RippleBed const &b, int I, int J, float s, bool wall, Texel &&texel)
  {
    float const x = ((float)I + 0.5f) * s, y = ((float)J + 0.5f) * s;

    RippleBedCell c;
    c.d = ripple_bed_depth(b, ripple_bed_raw(b, x, y, texel), wall);
    c.q = ripple_bed_surf(b, c.d);
    return c;
  }

  // what flows into a cell of depth dc and height e through the face it shares with a neighbour of depth dn and height en.  The order of
  // the tests: outside the WINDOW the neighbour is water at rest of the cell's own depth, dn not consulted; a solid neighbour passes
  // nothing; else the face's depth is the mean of the two
  OB_HD float ripple_bed_flux(bool inside, float dc, float dn, float e, float en)
  {
    return !inside ? dc * (0.0f - e) : dn == 0.0f ? 0.0f : (0.5f * (dc + dn)) * (en - e);
  }

  // one sub-step of a cell over the bed: e its height, et its rate, tL tR tD tU the four fluxes, dc its depth, gs2 = g / s^2, fsponge
  // and fsurf the cell's sponge and surf factors (their product is one fp32 operation).  A solid cell's new state is (+0, +0)
  OB_HD RippleCell ripple_bed_update(float e, float et, float tL, float tR, float tD, float tU, float dc, float h, float gs2, float fsponge, float fsurf)
  {
    float const f = fsponge * fsurf;
    float const div = (tL + tR) + (tD + tU);
    float const v1 = (et + h * (gs2 * div)) * f;

    RippleCell c;
    c.rate = v1;
    c.eta = e + h * v1;

    return ripple_wall_pin(dc == 0.0f, c);
  }
}
