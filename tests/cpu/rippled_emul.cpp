// rippled_emul.cpp -- datum_amd/csrc/ocean_rippled.h walked on the CPU (tests/test_rippled_emul.py): the two functions the kernels of
// ocean_rippled.hip call, over the layer's state in MEMORY order through ripple_sample, and a cast over an analytic surface plus the layer
// through ocean_ray.h's ray_search.  The several-cascade query's fetch and solve are pinned by their own tests: a height and two summed
// slopes per point are given.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_rippled.h"
#include "../../datum_amd/csrc/ocean_ray.h"

using namespace ocean;

namespace
{
  struct RippledState
  {
    float const *state;     // [R * R][2], memory order
    RippleGrid g;

    RippleSample at(float x, float y) const
    {
      float const *st = state;

      return ripple_sample(g, x, y, [st](int index) { return RippleCell{ st[2 * index], st[2 * index + 1] }; });
    }
  };

  RippledState layer(float const *state, int R, int ox, int oy, float invs)
  {
    RippledState l;
    l.state = state;
    l.g.R = R;
    l.g.ox = ox;
    l.g.oy = oy;
    l.g.invs = invs;
    return l;
  }
}

extern "C"
{

// per point k: out[k] = (rippled_height(height[k], s), rippled_slope(slopes[k][0], s.dx), rippled_slope(slopes[k][1], s.dy), s.rate), s the
// layer's sample at points[k]
void rippled_emul_points(float const *state, int R, int ox, int oy, float invs, float const *points, int64_t n, float const *height, float const *slopes, float *out)
{
  RippledState const l = layer(state, R, ox, oy, invs);

  for(int64_t k = 0; k < n; ++k)
  {
    RippleSample const s = l.at(points[2 * k], points[2 * k + 1]);

    out[4 * k] = rippled_height(height[k], s);
    out[4 * k + 1] = rippled_slope(slopes[2 * k], s.dx);
    out[4 * k + 2] = rippled_slope(slopes[2 * k + 1], s.dy);
    out[4 * k + 3] = s.rate;
  }
}

// the rippled cast's walk over the plane (a x + b y) + c (plane[3], tests/cpu/ray_emul.cpp: ray_height_plane) plus the layer: records [n][12],
// the surface record (x, y, rippled height, 0, 0, 0, 0, 0), eight NaNs above a point that is not finite
void rippled_emul_cast(float const *rays, int64_t n, int steps, float inv, int refine, float const *plane, float const *state, int R, int ox, int oy, float invs, float *records)
{
  RippledState const l = layer(state, R, ox, oy, invs);

  auto height = [&](float x, float y) -> float
  {
    if (!ray_finite(x) || !ray_finite(y))
      return nanf("");

    return rippled_height((plane[0] * x + plane[1] * y) + plane[2], l.at(x, y));
  };

  for(int64_t k = 0; k < n; ++k)
  {
    Ray const &r = reinterpret_cast<Ray const*>(rays)[k];

    float *out = records + DATUM_OCEAN_RAY_RECORD_FLOATS * k;

    if (ray_bad(r))
    {
      for(int j = 0; j < DATUM_OCEAN_RAY_RECORD_FLOATS; ++j)
        out[j] = nanf("");

      continue;
    }

    RayBracket const b = ray_search(r, steps, inv, refine, height);

    RayPoint const at = ray_point(r, b.hi);

    bool const fin = ray_finite(at.x) && ray_finite(at.y);

    for(int j = 4; j < DATUM_OCEAN_RAY_RECORD_FLOATS; ++j)
      out[j] = fin ? 0.0f : nanf("");

    if (fin)
    {
      out[4] = at.x;
      out[5] = at.y;
      out[6] = height(at.x, at.y);
    }

    out[0] = b.hi;
    out[1] = b.lo;
    out[2] = ray_g(at.z, out[6]);
    out[3] = ray_status(b.hit, b.side);
  }
}

}   // extern "C"
