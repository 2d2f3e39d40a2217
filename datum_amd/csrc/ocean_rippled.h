// ocean_rippled.h -- the ripple layer on the read side (include/datum_ocean_hip.h: "rippled reads") stated once: what the layer's sample
// adds to a height of the summed surface and to a summed slope before the shading normal is formed.  The sample itself is the ripple
// layer's (ocean_ripple.h: ripple_sample), the march a ray cast's (ocean_ray.h: ray_search over a height callable), unchanged: this header
// calls the first and restates neither.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/rippled_emul.cpp, tests/test_rippled_emul.py): the kernels of ocean_rippled.hip
// call these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product and sum is one fp32
// operation, rounded as written; there is no fused multiply-add here.

#pragma once

#include "ocean_ripple.h"

namespace ocean
{
  // The rippled height: the water height of the summed surface above a point plus the layer's height at that point, one fp32 addition
  // (coupled stepping's rec'[2] = rec[2] + s.eta)
  OB_HD float rippled_height(float height, RippleSample const &s)
  {
    return height + s.eta;
  }

  // The layer as one more entry behind the cascade list, in the map's own slope convention m.x / m.z = -1/2 dz/dx: the summed slope p
  // along one axis and the layer's derivative d along that axis give p + (-0.5f * d), one product and one addition
  OB_HD float rippled_slope(float p, float d)
  {
    return p + (-0.5f * d);
  }
}
