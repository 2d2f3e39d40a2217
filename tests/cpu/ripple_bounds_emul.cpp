// ripple_bounds_emul.cpp -- datum_amd/csrc/ocean_ripple_bounds.h walked on the CPU (tests/test_ripple_bounds_emul.py): the functions the
// kernels of ocean_ripple_bounds.hip and datum_ocean_surface_slab_rippled call.  The cell fold as strided partials merged in a given order
// (the kernels' shape), the rippled slab, and the rippled cast -- ray_emul.cpp's height callbacks plus the layer in MEMORY order through
// ripple_sample -- through ray_search and through ray_search_bounded, with the height evaluations counted.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_ripple_bounds.h"

using namespace ocean;

extern "C"
{

typedef void (*ray_height_fn)(float x, float y, void *user, float *rec);

// (ray_emul.cpp)
void ray_height_eval(ray_height_fn fn, void *user, float const *points, int64_t n, float *recs);

int ripple_bounds_record_floats(void) { return RIPPLE_BOUNDS_FIELDS; }

// state [n][2] (eta, rate), folded by `parts` strided partials (part p takes cells p, p + parts, ...), the partials merged in the order
// order[0 .. parts - 1] (NULL: 0, 1, ...): rec [8].  parts = 1 is the plain fold
void ripple_bounds_fold(float const *state, int64_t n, int parts, int const *order, float *rec)
{
  RippleBounds all = ripple_bounds_identity();

  for(int j = 0; j < parts; ++j)
  {
    int const p = order ? order[j] : j;

    RippleBounds b = ripple_bounds_identity();

    for(int64_t k = p; k < n; k += parts)
      ripple_bounds_cell(b, state[2 * k], state[2 * k + 1]);

    ripple_bounds_merge(all, b);
  }

  ripple_bounds_record(all, rec);
}

// out [4]: zlo, zhi, reachx, reachy
void ripple_bounds_slab_eval(float const *records, int const *cascades, int count, float basez, float A, float gx, float gy, float const *layer, float *out)
{
  BoundsSlab const s = ripple_bounds_slab(records, cascades, count, basez, A, gx, gy, layer);

  out[0] = s.zlo; out[1] = s.zhi; out[2] = s.reachx; out[3] = s.reachy;
}

// per point k: heights[k] = rippled_height(fn's height at points[k], the layer's sample there), a NaN above a point that is not finite
void ripple_bounds_heights(ray_height_fn fn, void *user, float const *state, int R, int ox, int oy, float invs, float const *points, int64_t n, float *heights)
{
  RippleGrid const g = { R, ox, oy, invs };

  for(int64_t k = 0; k < n; ++k)
  {
    float rec[8];

    ray_height_eval(fn, user, points + 2 * k, 1, rec);

    heights[k] = rippled_height(rec[2], ripple_sample(g, points[2 * k], points[2 * k + 1], [state](int index) { return RippleCell{ state[2 * index], state[2 * index + 1] }; }));
  }
}

// the rippled cast's walk over fn's surface plus the layer: records [n][12], the surface record fn's with the rippled height in field 2;
// bounded != 0: ray_search_bounded with (zlo, zhi), else ray_search.  calls[k] counts ray k's height evaluations (the record's included)
void ripple_bounds_cast(float const *rays, int64_t n, int steps, float inv, int refine, int bounded, float zlo, float zhi, ray_height_fn fn, void *user,
                        float const *state, int R, int ox, int oy, float invs, float *records, int32_t *calls)
{
  RippleGrid const g = { R, ox, oy, invs };

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

        rec[2] = rippled_height(rec[2], ripple_sample(g, x, y, [state](int index) { return RippleCell{ state[2 * index], state[2 * index + 1] }; }));
      };

      auto height = [&](float x, float y) -> float
      {
        float rec[8];

        record(x, y, rec);

        return rec[2];
      };

      RayBracket const b = bounded ? ray_search_bounded(r, steps, inv, refine, zlo, zhi, height) : ray_search(r, steps, inv, refine, height);

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

}   // extern "C"
