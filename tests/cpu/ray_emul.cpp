// ray_emul.cpp -- datum_amd/csrc/ocean_ray.h walked on the CPU (tests/test_ray_emul.py): the functions ocean_ray_kernel calls, with the
// height given by a C callback that fills the query's record of eight floats above (x, y): the fetch and the solve are the several-cascade
// query's and are pinned there.  Two analytic callbacks live here so that a test can hand the SAME function to this walk and, through
// ray_height_eval, to the numpy restatement (tests/ray64.py: cast32): the heights then agree by construction, and what is compared is the cast.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_ray.h"

using namespace ocean;

extern "C"
{

typedef void (*ray_height_fn)(float x, float y, void *user, float *rec);

size_t ray_sizeof(void) { return sizeof(Ray); }
int ray_record_floats(void) { return DATUM_OCEAN_RAY_RECORD_FLOATS; }

// records [n][8] above points [n][2], the callback point by point; a non-finite point gets the query's eight NaNs
void ray_height_eval(ray_height_fn fn, void *user, float const *points, int64_t n, float *recs)
{
  for(int64_t k = 0; k < n; ++k)
  {
    float const x = points[2 * k], y = points[2 * k + 1];

    if (ray_finite(x) && ray_finite(y))
      fn(x, y, user, recs + 8 * k);
    else
      for(int j = 0; j < 8; ++j)
        recs[8 * k + j] = nanf("");
  }
}

// a plane: user = float[3] (a, b, c), height (a x + b y) + c
void ray_height_plane(float x, float y, void *user, float *rec)
{
  float const *u = static_cast<float const*>(user);

  rec[0] = x; rec[1] = y; rec[2] = (u[0] * x + u[1] * y) + u[2]; rec[3] = 0.0f;
  rec[4] = -u[0]; rec[5] = -u[1]; rec[6] = 1.0f; rec[7] = 0.25f;
}

// two superposed periods: user = float[9] (A1, kx1, ky1, p1, A2, kx2, ky2, p2, c), evaluated in double and rounded once
void ray_height_waves(float x, float y, void *user, float *rec)
{
  float const *u = static_cast<float const*>(user);

  double const h = u[0] * sin((double)u[1] * x + (double)u[2] * y + u[3]) + u[4] * sin((double)u[5] * x + (double)u[6] * y + u[7]) + u[8];

  rec[0] = x; rec[1] = y; rec[2] = (float)h; rec[3] = 0.0f;
  rec[4] = 0.0f; rec[5] = 0.0f; rec[6] = 1.0f; rec[7] = 0.5f;
}

// bad[n]: ocean_ray.h's rule
void ray_bad_flags(float const *rays, int64_t n, unsigned char *bad)
{
  for(int64_t k = 0; k < n; ++k)
    bad[k] = ray_bad(reinterpret_cast<Ray const*>(rays)[k]);
}

// t_i of ray k for i = 0 ... steps: samples [n][steps + 1]
void ray_samples(float const *rays, int64_t n, int steps, float inv, float *samples)
{
  for(int64_t k = 0; k < n; ++k)
  {
    Ray const &r = reinterpret_cast<Ray const*>(rays)[k];

    float const delta = ray_delta(r, inv);

    for(int i = 0; i <= steps; ++i)
      samples[k * (steps + 1) + i] = ray_sample(r, delta, i, steps);
  }
}

// the kernel's walk: records [n][12]; calls[k], where given, counts ray k's height evaluations (the record's included)
void ray_cast(float const *rays, int64_t n, int steps, float inv, int refine, ray_height_fn fn, void *user, float *records, int32_t *calls)
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

      RayBracket const b = ray_search(r, steps, inv, refine, height);

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
