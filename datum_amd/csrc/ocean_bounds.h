// ocean_bounds.h -- surface bounds per cascade (include/datum_ocean_hip.h: datum_ocean_reduce_bounds) stated once: the record, the fold of a
// texel into it and of two partial records into one, the slab a blend list's records give under a set, and the ray cast's march and
// refinement with the samples outside that slab decided in arithmetic (ray_search_bounded, beside ocean_ray.h's ray_search).
//
// Host/device neutral so that a CPU can walk it (tests/cpu/bounds_emul.cpp, tests/test_bounds_emul.py): the kernels of ocean_bounds.hip
// and datum_ocean_surface_slab call these functions, there is no second copy.  Built with -ffp-contract=off wherever it is built: every
// product and sum is one fp32 operation, rounded as written; there is no fmaf here.

#pragma once

#include <math.h>

#include "ocean_ray.h"

namespace ocean
{
  constexpr int BOUNDS_FIELDS = DATUM_OCEAN_BOUNDS_RECORD_FLOATS;

  static_assert(BOUNDS_FIELDS == 8, "a record is two 16-byte stores");

  // the extrema of dz, dx, dy of map layer 0 as stored, and the texels with a non-finite component.  A NaN enters no extremum (fminf,
  // fmaxf), an infinity does; either is counted
  struct Bounds
  {
    float zmin, zmax, xmin, xmax, ymin, ymax;
    unsigned int nonfinite;
  };

  OR_HD Bounds bounds_identity()
  {
    Bounds b;
    b.zmin = b.xmin = b.ymin = INFINITY;
    b.zmax = b.xmax = b.ymax = -INFINITY;
    b.nonfinite = 0;
    return b;
  }

  OR_HD void bounds_texel(Bounds &b, float dx, float dy, float dz)
  {
    b.zmin = fminf(b.zmin, dz); b.zmax = fmaxf(b.zmax, dz);
    b.xmin = fminf(b.xmin, dx); b.xmax = fmaxf(b.xmax, dx);
    b.ymin = fminf(b.ymin, dy); b.ymax = fmaxf(b.ymax, dy);

    b.nonfinite += (ray_finite(dx) && ray_finite(dy) && ray_finite(dz)) ? 0u : 1u;
  }

  // order-independent but for the sign of a zero extremum
  OR_HD void bounds_merge(Bounds &b, Bounds const &o)
  {
    b.zmin = fminf(b.zmin, o.zmin); b.zmax = fmaxf(b.zmax, o.zmax);
    b.xmin = fminf(b.xmin, o.xmin); b.xmax = fmaxf(b.xmax, o.xmax);
    b.ymin = fminf(b.ymin, o.ymin); b.ymax = fmaxf(b.ymax, o.ymax);

    b.nonfinite += o.nonfinite;
  }

  // the record: zmin, zmax, xmin, xmax, ymin, ymax, nonfinite (N * N <= 2^24 texels: exact), 0
  OR_HD void bounds_record(Bounds const &b, float *rec)
  {
    rec[0] = b.zmin; rec[1] = b.zmax;
    rec[2] = b.xmin; rec[3] = b.xmax;
    rec[4] = b.ymin; rec[5] = b.ymax;
    rec[6] = (float)b.nonfinite;
    rec[7] = 0.0f;
  }

  // Between zlo and zhi lies every height the several-cascade query can give for the listed cascades under the set: vz = (basez + A st) + sum
  // of the cascades' blended dz.  pad is a stated margin of 2^-16 of the magnitudes involved, about 256 ulp of them, for what the sum of
  // the extrema does not hold: sincos_phase's |st| <= 1 + 5e-7, the four blend weights' sum (1 within a few ulp) and one rounding per
  // cascade sum.  reach bounds how far the query's V(b).xy lies from b along either axis.  A listed cascade with a non-finite texel:
  // zlo = zhi = NaN, which decides no sample
  struct BoundsSlab
  {
    float zlo, zhi, reachx, reachy;
  };

  // records: [cascade][BOUNDS_FIELDS], the handle's; cascades[count]: the list; basez, gx, gy: GenFrame's; A: the set's swellamplitude
  OR_HD BoundsSlab bounds_slab(float const *records, int const *cascades, int count, float basez, float A, float gx, float gy)
  {
    float const absa = fabsf(A);

    float mag = fabsf(basez) + absa;
    float hi = basez + absa;
    float lo = basez - absa;
    float rx = fabsf(gx), ry = fabsf(gy);
    bool nonfinite = false;

    for(int c = 0; c < count; ++c)
    {
      float const *r = records + (size_t)cascades[c] * BOUNDS_FIELDS;

      mag = mag + fmaxf(fabsf(r[0]), fabsf(r[1]));
      hi = hi + r[1];
      lo = lo + r[0];
      rx = rx + fmaxf(fabsf(r[2]), fabsf(r[3]));
      ry = ry + fmaxf(fabsf(r[4]), fabsf(r[5]));

      nonfinite = nonfinite || r[6] > 0.0f;
    }

    float const pad = mag * 1.52587890625e-05f;         // 2^-16

    BoundsSlab s;
    s.zhi = nonfinite ? __builtin_nanf("") : hi + pad;
    s.zlo = nonfinite ? __builtin_nanf("") : lo - pad;
    s.reachx = rx;
    s.reachy = ry;
    return s;
  }

  // a sample whose side the slab decides: its point finite along x and y (elsewhere the height is a NaN by ray_search's contract, "not
  // below", which no z decides) and above zhi or below zlo.  A NaN z or a NaN bound makes both comparisons false
  OR_HD bool ray_known(RayPoint const &p, float zlo, float zhi)
  {
    return ray_finite(p.x) && ray_finite(p.y) && (p.z > zhi || p.z < zlo);
  }

  // ray_search with below'(t) = point(t).z > zhi ? false : point(t).z < zlo ? true : below(t) on the samples ray_known names: the same
  // bracket, side and hit wherever every height lies strictly inside (zlo, zhi), with `height` called for the other samples alone.  Each
  // phase first walks the samples it knows in arithmetic, then evaluates one: `height` has one call site in the march and one in the
  // refinement, and a wave spends the largest number of evaluations among its lanes, not the largest sample index
  template<typename Height>
  OR_HD RayBracket ray_search_bounded(Ray const &r, int steps, float inv, int refine, float zlo, float zhi, Height &&height)
  {
    float const delta = ray_delta(r, inv);

    RayBracket b;
    b.lo = b.hi = r.tmax;
    b.side = false;
    b.hit = false;

    float last = r.tmin;

    int i = 0;

    // sample i's side taken as ray_search's loop body takes it
    auto take = [&](float t, bool below)
    {
      if (i == 0)
        b.side = below;
      else if (below != b.side)
      {
        b.lo = last;
        b.hi = t;
        b.hit = true;
      }

      last = t;
      ++i;
    };

    while (i <= steps && !b.hit)
    {
      float t = ray_sample(r, delta, i, steps);

      RayPoint p = ray_point(r, t);

      while (ray_known(p, zlo, zhi))
      {
        take(t, !(p.z > zhi));

        if (i > steps || b.hit)
          break;

        t = ray_sample(r, delta, i, steps);
        p = ray_point(r, t);
      }

      if (i > steps || b.hit)
        break;

      take(t, ray_below(ray_g(p.z, height(p.x, p.y))));
    }

    if (b.hit)
    {
      int k = 0;

      auto half = [&](float mid, bool below)
      {
        if (below == b.side)
          b.lo = mid;
        else
          b.hi = mid;

        ++k;
      };

      while (k < refine)
      {
        float mid = ray_mid(b.lo, b.hi);

        RayPoint p = ray_point(r, mid);

        while (ray_known(p, zlo, zhi))
        {
          half(mid, !(p.z > zhi));

          if (k >= refine)
            break;

          mid = ray_mid(b.lo, b.hi);
          p = ray_point(r, mid);
        }

        if (k >= refine)
          break;

        half(mid, ray_below(ray_g(p.z, height(p.x, p.y))));
      }
    }

    return b;
  }
}
