// ocean_ripple_wall.h -- ripple walls (include/datum_ocean_hip.h: "ripple walls") stated once: which cell centres a wall record covers,
// the wall plane as a function of (list, world cell), and what a walled sub-step reads for a neighbour in each mode.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/ripple_wall_emul.cpp, tests/test_ripple_wall_emul.py): the kernels of
// ocean_ripple_wall.hip call these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product
// and sum is one fp32 operation, rounded as written; there is no fmaf here, no division, and no sine or cosine: the caller gives the axis.
// The torus, the window test, the height a sub-step reads, ripple_update and the DEEP sum are ocean_ripple.h's and ocean_ripple_deep.h's,
// called as they stand.

#pragma once

#include "ocean_ripple_deep.h"

namespace ocean
{
  constexpr int RIPPLE_MAX_WALLS = DATUM_OCEAN_RIPPLE_MAX_WALLS;

  static_assert(sizeof(datum_ocean_ripple_wall) == 32, "a wall is a 32-byte record");

  // does the record cover the point (x, y)?  u, v are the point in the shape's frame; a non-unit axis scales the shape
  OB_HD bool ripple_wall_covers(datum_ocean_ripple_wall const &w, float x, float y)
  {
    float const dx = x - w.center[0], dy = y - w.center[1];
    float const u = dx * w.axis[0] + dy * w.axis[1];
    float const v = dy * w.axis[0] - dx * w.axis[1];

    if (w.kind == DATUM_OCEAN_RIPPLE_WALL_BOX)
      return fabsf(u) <= w.half[0] && fabsf(v) <= w.half[1];

    float const a = u * w.half[1], b = v * w.half[0], r = w.half[0] * w.half[1];

    return a * a + b * b <= r * r;
  }

  // the plane's byte of world cell (I, J): 1 where any record covers the cell's centre.  s is the fp32 cell side
  OB_HD unsigned char ripple_wall_cell(datum_ocean_ripple_wall const *walls, int count, int I, int J, float s)
  {
    float const x = ((float)I + 0.5f) * s, y = ((float)J + 0.5f) * s;

    bool wall = false;

    for(int k = 0; k < count; ++k)
      wall = wall || ripple_wall_covers(walls[k], x, y);

    return wall ? 1 : 0;
  }

  // WAVE: what a cell of height e reads for a neighbour of height en.  The order of the tests: outside the WINDOW 0, the flag not
  // consulted; a wall the cell's own e (the mirror in the face between the two cells); else the neighbour's height
  OB_HD float ripple_wall_neighbour(bool inside, bool wall, float e, float en)
  {
    return !inside ? 0.0f : wall ? e : en;
  }

  // DEEP: the image a walled sub-step convolves -- a wall cell reads 0, the pending deposit of a first sub-step included
  OB_HD float ripple_wall_height(bool wall, float eta, int src, bool first)
  {
    return wall ? 0.0f : ripple_height(eta, src, first);
  }

  // a wall cell's new state is (+0, +0) in both modes
  OB_HD RippleCell ripple_wall_pin(bool wall, RippleCell c)
  {
    if (wall)
      c.eta = c.rate = 0.0f;

    return c;
  }
}
