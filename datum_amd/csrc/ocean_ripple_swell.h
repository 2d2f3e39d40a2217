// ocean_ripple_swell.h -- ripple swell (include/datum_ocean_hip.h: "ripple swell") stated once: which neighbour of a cell is a source of
// the scattered field, the forcing F of a cell from the summed surface's heights above the cell and its neighbours, and the two WAVE
// sub-steps that read F -- the walled one and the one over a bed.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/ripple_swell_emul.cpp, tests/test_ripple_swell_emul.py): the kernels of
// ocean_ripple_swell.hip call these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product,
// sum and difference is one fp32 operation, rounded as written; there is no fused multiply-add here and no quotient.  The torus, the
// window test, the cell centre, the height a sub-step reads, what a walled sub-step reads for a neighbour, the pin of a solid cell and
// the flux through a face over a bed are ocean_ripple.h's, ocean_ripple_wall.h's and ocean_ripple_bed.h's, called as they stand.  The
// heights themselves are the several-cascade query's (ocean_query.hip), which is device code: a caller hands them in.

#pragma once

#include "ocean_ripple_bed.h"

namespace ocean
{
  // is a cell solid?  Without a bed its wall byte says so (no walls: nothing is solid); over a bed its depth does, +0 where a wall stands
  OB_HD bool ripple_swell_solid(unsigned int wall)
  {
    return wall != 0;
  }

  OB_HD bool ripple_swell_solid_bed(float d)
  {
    return d == 0.0f;
  }

  // does a neighbour count as a source: it lies inside the WINDOW and it is solid.  The order of the tests is the walled sub-step's: the
  // flag of the torus-aliased cell outside the window is not consulted
  OB_HD bool ripple_swell_counts(bool inside, bool solid)
  {
    return inside && solid;
  }

  // the difference across one face: the incident height above the cell's centre less that above the neighbour's, +0 where the
  // neighbour does not count
  OB_HD float ripple_swell_face(bool counts, float Hc, float Hn)
  {
    return counts ? Hc - Hn : 0.0f;
  }

  // the plane's value of a cell from its four differences: +0 on a solid cell, and -- the four being +0 -- where no neighbour counts
  OB_HD float ripple_swell_force(bool solid, float dL, float dR, float dD, float dU)
  {
    return solid ? 0.0f : (dL + dR) + (dD + dU);
  }

  // the centre of world cell I along one axis, as ripple_wall_cell computes it.  s is the fp32 cell side
  OB_HD float ripple_swell_centre(int I, float s)
  {
    return ((float)I + 0.5f) * s;
  }

  // one WAVE sub-step of a cell with walls and swell: ripple_update's, with F behind the five-point sum.  eL eR eD eU are what
  // ripple_wall_neighbour gave; a wall cell is pinned
  OB_HD RippleCell ripple_swell_update(float e, float et, float eL, float eR, float eD, float eU, float F, bool wall, float h, float c2s2, float f)
  {
    float const lap = (((eL + eR) + (eD + eU)) - 4.0f * e) + F;
    float const v1 = (et + h * (c2s2 * lap)) * f;

    RippleCell c;
    c.rate = v1;
    c.eta = e + h * v1;

    return ripple_wall_pin(wall, c);
  }

  // one WAVE sub-step of a cell over a bed with swell: ripple_bed_update's, with dc F behind the four fluxes -- the face at a solid
  // neighbour carries the cell's own depth, as ripple_bed_flux's face at the window's edge does.  tL tR tD tU are what ripple_bed_flux gave
  OB_HD RippleCell ripple_swell_bed_update(float e, float et, float tL, float tR, float tD, float tU, float dc, float F, float h, float gs2, float fsponge, float fsurf)
  {
    float const f = fsponge * fsurf;
    float const div = ((tL + tR) + (tD + tU)) + dc * F;
    float const v1 = (et + h * (gs2 * div)) * f;

    RippleCell c;
    c.rate = v1;
    c.eta = e + h * v1;

    return ripple_wall_pin(dc == 0.0f, c);
  }
}
