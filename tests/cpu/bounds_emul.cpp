// bounds_emul.cpp -- datum_amd/csrc/ocean_bounds.h walked on the CPU (tests/test_bounds_emul.py): the functions the kernels of
// ocean_bounds.hip and datum_ocean_surface_slab call.  The texel fold as one run and as strided partials merged (the kernels' shape), the
// slab, and ray_search_bounded beside ray_search over ray_emul.cpp's height callbacks, with the height evaluations counted.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_bounds.h"

using namespace ocean;

extern "C"
{

typedef void (*ray_height_fn)(float x, float y, void *user, float *rec);

// (ray_emul.cpp)
void ray_height_eval(ray_height_fn fn, void *user, float const *points, int64_t n, float *recs);

int bounds_record_floats(void) { return BOUNDS_FIELDS; }

// texels [n][4] (dx, dy, dz, nx) as part A holds them, folded by `parts` strided partials (part p takes texels p, p + parts, ...), the
// partials merged in order: rec [8].  parts = 1 is the plain fold
void bounds_fold(float const *texels, int64_t n, int parts, float *rec)
{
  Bounds all = bounds_identity();

  for(int p = 0; p < parts; ++p)
  {
    Bounds b = bounds_identity();

    for(int64_t k = p; k < n; k += parts)
      bounds_texel(b, texels[4 * k], texels[4 * k + 1], texels[4 * k + 2]);

    bounds_merge(all, b);
  }

  bounds_record(all, rec);
}

// out [4]: zlo, zhi, reachx, reachy
void bounds_slab_eval(float const *records, int const *cascades, int count, float basez, float A, float gx, float gy, float *out)
{
  BoundsSlab const s = bounds_slab(records, cascades, count, basez, A, gx, gy);

  out[0] = s.zlo; out[1] = s.zhi; out[2] = s.reachx; out[3] = s.reachy;
}

// ray_emul.cpp's ray_cast with ray_search_bounded: records [n][12]; calls[k] counts ray k's height evaluations (the record's included)
void bounds_cast(float const *rays, int64_t n, int steps, float inv, int refine, float zlo, float zhi, ray_height_fn fn, void *user, float *records, int32_t *calls)
{
  for(int64_t k = 0; k < n; ++k)
  {
    Ray const &r = reinterpret_cast<Ray const*>(rays)[k];

    float *out = records + DATUM_OCEAN_RAY_RECORD_FLOATS * k;

    int32_t count = 0;

    if (ray_bad(r))
    {
      for(int j = 0; j < DATUM_OCEAN_RAY_RECORD_FLOATS; ++j)
        out[j] = nanf("");
    }
    else
    {
      auto record = [&](float x, float y, float *rec)
      {
        ++count;

        float const q[2] = { x, y };

        ray_height_eval(fn, user, q, 1, rec);
      };

      auto height = [&](float x, float y) -> float
      {
        float rec[8];

        record(x, y, rec);

        return rec[2];
      };

      RayBracket const b = ray_search_bounded(r, steps, inv, refine, zlo, zhi, height);

      RayPoint const at = ray_point(r, b.hi);

      record(at.x, at.y, out + 4);

      out[0] = b.hi;
      out[1] = b.lo;
      out[2] = ray_g(at.z, out[6]);
      out[3] = ray_status(b.hit, b.side);
    }

    if (calls)
      calls[k] = count;
  }
}

}
