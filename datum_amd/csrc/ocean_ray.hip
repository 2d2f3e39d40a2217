// ocean_ray.hip -- ray casts on the summed surface (include/datum_ocean_hip.h: datum_ocean_cast_rays): per ray a fixed march of `steps`
// samples to the first change of side, `refine` bisections of that bracket, and the several-cascade query's record at the bracket's far
// end.  The ray's arithmetic, the march and the refinement are ocean_ray.h's (a CPU walks the same functions); every height is the
// several-cascade query's, the same functions (ocean_query.hip), so its bits are datum_ocean_sample_surface_blend's.
//
//   * one ray per lane, 256-thread workgroups; a lane stops marching at its own bracket, the wave when its last lane has;
//   * a ray is two 16-byte loads, a record three 16-byte stores, through buffer resources laid over exactly the workgroup's rays and
//     records: no index reaches outside either array, and an array beyond 4 GiB needs no 64-bit offset;
//   * the search needs the height alone: its evaluations are query_height and fetch part A of the corners; parts B and the foam planes
//     are fetched once, by query_record for the record at `hi`;
//   * a bad ray fetches nothing; its record is twelve quiet NaNs;
//   * ray_cast is a ray's whole work around a search: ocean_ray_kernel passes ray_search, ocean_ray_bounded_kernel (ocean_bounds.hip)
//     ocean_bounds.h's search with its slab.
// No LDS, no barrier, no atomics, no scratch (make resource-usage).

#pragma once

#include "ocean_ray.h"
#include "ocean_blend.hip"

namespace ocean
{
  // the rays of one cast and how they are searched
  struct RayBatch
  {
    float4 const *rays;     // 2 float4 per ray
    float4 *records;        // 3 float4 per ray
    int n;
    int steps;
    int refine;
    float inv;              // 1.0f / (float)steps, rounded on the host (ray_launch)
  };

  struct RayArgs
  {
    QueryArgs q;
    RayBatch r;
  };

  constexpr int RAY_THREADS = 256;
  constexpr int RAY_BYTES = DATUM_OCEAN_RAY_FLOATS * (int)sizeof(float);
  constexpr int RAY_RECORD_BYTES = DATUM_OCEAN_RAY_RECORD_FLOATS * (int)sizeof(float);

  static_assert(RAY_BYTES == 32 && RAY_RECORD_BYTES == 48, "two 16-byte loads, three 16-byte stores");

  // one lane's ray: `search(ray, height)` gives the bracket, `height(x, y)` being rec.z of the query above (x, y)
  template<int LAYOUT, class Search>
  __device__ __forceinline__ void ray_cast(QueryArgs const &a, RayBatch const &r, Search &&search)
  {
    // the workgroup's rays and records and nothing else (n <= INT32_MAX: first < 2^31)
    int const first = (int)blockIdx.x * RAY_THREADS;
    int const left = r.n - first;
    int const here = left < RAY_THREADS ? left : RAY_THREADS;
    int const lane = (int)threadIdx.x;

    if (lane >= here)
      return;

    __amdgpu_buffer_rsrc_t const rrays = make_rsrc(r.rays + 2 * (size_t)first, (size_t)here * RAY_BYTES);
    __amdgpu_buffer_rsrc_t const rrecords = make_rsrc(r.records + 3 * (size_t)first, (size_t)here * RAY_RECORD_BYTES);

    float4 const r0 = buf_load_f32x4_aux<0>(rrays, lane * RAY_BYTES, 0);
    float4 const r1 = buf_load_f32x4_aux<0>(rrays, lane * RAY_BYTES + 16, 0);

    Ray const ray = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w };

    int const out = lane * RAY_RECORD_BYTES;

    float const nan = __builtin_nanf("");

    if (ray_bad(ray))
    {
      buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecords, out, 0);
      buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecords, out, 16);
      buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecords, out, 32);
      return;
    }

    // a NaN where the query gives NaNs
    auto height = [&](float x, float y) -> float
    {
      if (!ray_finite(x) || !ray_finite(y))
        return nan;

      return query_height<LAYOUT>(a, query_solve<LAYOUT>(a, make_float2(x, y)));
    };

    RayBracket const b = search(ray, height);

    RayPoint const at = ray_point(ray, b.hi);

    QueryRecord rec = { make_float4(nan, nan, nan, nan), make_float4(nan, nan, nan, nan) };

    if (ray_finite(at.x) && ray_finite(at.y))
    {
      float2 const q = make_float2(at.x, at.y);

      rec = query_record<LAYOUT>(a, query_solve<LAYOUT>(a, q), q);
    }

    buf_store_f32x4_aux<0>(make_float4(b.hi, b.lo, ray_g(at.z, rec.v.z), ray_status(b.hit, b.side)), rrecords, out, 0);
    buf_store_f32x4_aux<0>(rec.v, rrecords, out, 16);
    buf_store_f32x4_aux<0>(rec.m, rrecords, out, 32);
  }

  template<int LAYOUT>
  __global__ void __launch_bounds__(RAY_THREADS) ocean_ray_kernel(RayArgs a)
  {
    RayBatch const &r = a.r;

    ray_cast<LAYOUT>(a.q, r, [&](Ray const &ray, auto &height) { return ray_search(ray, r.steps, r.inv, r.refine, height); });
  }

  // what launch_rays and launch_rays_bounded share: q (but its frame) and r (but inv) filled in, r.n > 0; `args` is the kernel's one argument
  inline hipError_t ray_launch(void const *kernel, QueryArgs &q, RayBatch &r, void *args, hipStream_t stream)
  {
    query_frame(q);
    r.inv = 1.0f / (float)r.steps;

    return hipLaunchKernel(kernel, dim3((unsigned)(((size_t)r.n + RAY_THREADS - 1) / RAY_THREADS)), dim3(RAY_THREADS), &args, 0, stream);
  }

  inline hipError_t launch_rays(RayArgs &a, hipStream_t stream)
  {
    return ray_launch(layout_kernel(a.q.N, &ocean_ray_kernel<GEN_PLAIN>, &ocean_ray_kernel<GEN_BANDED>), a.q, a.r, &a, stream);
  }
}
