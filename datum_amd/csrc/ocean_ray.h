// ocean_ray.h -- ray casts on the summed surface (include/datum_ocean_hip.h: datum_ocean_cast_rays) stated once: the ray, the rule that makes
// a ray bad, point(t), the march's step and samples, the refinement's mid point, `below`, the status, and the march and the refinement
// themselves as a function over a height callable.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/ray_emul.cpp, tests/test_ray_emul.py): ocean_ray_kernel of ocean_ray.hip calls
// these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every product and sum is one fp32
// operation, rounded as written; there is no fmaf here.

#pragma once

#include <math.h>

#include "../../include/datum_ocean_hip.h"

#if defined(__HIPCC__)
#define OR_HD __host__ __device__ __forceinline__
#else
#define OR_HD inline
#endif

namespace ocean
{
  struct Ray
  {
    float ox, oy, oz, tmin;
    float dx, dy, dz, tmax;
  };

  static_assert(sizeof(Ray) == DATUM_OCEAN_RAY_FLOATS * sizeof(float), "a ray is two 16-byte loads");

  struct RayPoint { float x, y, z; };

  OR_HD RayPoint ray_point(Ray const &r, float t)
  {
    RayPoint p;
    p.x = r.ox + t * r.dx;
    p.y = r.oy + t * r.dy;
    p.z = r.oz + t * r.dz;
    return p;
  }

  OR_HD bool ray_finite(float v)
  {
    return fabsf(v) <= 3.4028234663852886e38f;          // false for a NaN
  }

  OR_HD bool ray_point_finite(RayPoint const &p)
  {
    return ray_finite(p.x) && ray_finite(p.y) && ray_finite(p.z);
  }

  // a ray with a non-finite field, an empty parameter range or a non-finite end point: nothing is fetched for it, its record is twelve NaNs
  OR_HD bool ray_bad(Ray const &r)
  {
    bool const fields = ray_finite(r.ox) && ray_finite(r.oy) && ray_finite(r.oz) && ray_finite(r.tmin)
                     && ray_finite(r.dx) && ray_finite(r.dy) && ray_finite(r.dz) && ray_finite(r.tmax);

    return !fields || r.tmax < r.tmin || !ray_point_finite(ray_point(r, r.tmin)) || !ray_point_finite(ray_point(r, r.tmax));
  }

  // inv = 1.0f / (float)steps, rounded once by the caller
  OR_HD float ray_delta(Ray const &r, float inv)
  {
    return (r.tmax - r.tmin) * inv;
  }

  // t_i for i = 0 ... steps; t_steps is tmax itself
  OR_HD float ray_sample(Ray const &r, float delta, int i, int steps)
  {
    return (i == steps) ? r.tmax : r.tmin + (float)i * delta;
  }

  OR_HD float ray_mid(float lo, float hi)
  {
    return 0.5f * (lo + hi);
  }

  // g = point.z - height and below = g < 0, as written: a NaN is "not below"
  OR_HD float ray_g(float z, float height)
  {
    return z - height;
  }

  OR_HD bool ray_below(float g)
  {
    return g < 0.0f;
  }

  OR_HD float ray_status(bool hit, bool side)
  {
    return !hit ? (float)DATUM_OCEAN_RAY_MISS : (side ? (float)DATUM_OCEAN_RAY_LEAVE : (float)DATUM_OCEAN_RAY_ENTER);
  }

  struct RayBracket
  {
    float lo, hi;
    bool side;              // below(t_0)
    bool hit;
  };

  // The march and the refinement of a ray that is not bad.  height(x, y) is the water height above (x, y): rec.z of the several-cascade
  // query, a NaN where (x, y) is not finite.  It is called for t_0, t_1, ... up to the bracket's t_i, then `refine` times on a bracket
  template<typename Height>
  OR_HD RayBracket ray_search(Ray const &r, int steps, float inv, int refine, Height &&height)
  {
    float const delta = ray_delta(r, inv);

    RayBracket b;
    b.lo = b.hi = r.tmax;
    b.side = false;
    b.hit = false;

    float last = r.tmin;

    for(int i = 0; i <= steps; ++i)
    {
      float const t = ray_sample(r, delta, i, steps);

      RayPoint const p = ray_point(r, t);

      bool const below = ray_below(ray_g(p.z, height(p.x, p.y)));

      if (i == 0)
        b.side = below;
      else if (below != b.side)
      {
        b.lo = last;
        b.hi = t;
        b.hit = true;
        break;
      }

      last = t;
    }

    if (b.hit)
    {
      for(int k = 0; k < refine; ++k)
      {
        float const mid = ray_mid(b.lo, b.hi);

        RayPoint const p = ray_point(r, mid);

        if (ray_below(ray_g(p.z, height(p.x, p.y))) == b.side)
          b.lo = mid;
        else
          b.hi = mid;
      }
    }

    return b;
  }
}
