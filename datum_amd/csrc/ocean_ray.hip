// ocean_ray.hip -- ray casts on the summed surface (include/datum_ocean_hip.h: datum_ocean_cast_rays): per ray a fixed march of `steps`
// samples to the first change of side, `refine` bisections of that bracket, and the several-cascade query's record at the bracket's far
// end.  The ray's arithmetic, the march and the refinement are ocean_ray.h's (a CPU walks the same functions); every height is the
// several-cascade query's, the same text (ocean_surface_blend_point.inc), so its bits are datum_ocean_sample_surface_blend's.
//
//   * one ray per lane, 256-thread workgroups; a lane stops marching at its own bracket, the wave when its last lane has;
//   * a ray is two 16-byte loads, a record three 16-byte stores, through buffer resources laid over exactly the workgroup's rays and
//     records: no index reaches outside either array, and an array beyond 4 GiB needs no 64-bit offset;
//   * the search needs the height alone: its evaluations include the point text with OCEAN_SURFACE_BLEND_POINT_HEIGHT and fetch part A of
//     the corners; parts B and the foam planes are fetched once, for the record at `hi`;
//   * a bad ray fetches nothing; its record is twelve quiet NaNs.
// No LDS, no barrier, no atomics, no scratch (make resource-usage).

#pragma once

#include "ocean_ray.h"
#include "ocean_blend.hip"

namespace ocean
{
  struct RayArgs
  {
    SurfaceArgs s;          // s.set, s.frame, s.N and s.iterations are read
    BlendList list;
    float4 const *rays;     // 2 float4 per ray
    float4 *records;        // 3 float4 per ray
    int n;
    int steps;
    int refine;
    float inv;              // 1.0f / (float)steps, rounded on the host
  };

  constexpr int RAY_THREADS = 256;
  constexpr int RAY_BYTES = DATUM_OCEAN_RAY_FLOATS * (int)sizeof(float);
  constexpr int RAY_RECORD_BYTES = DATUM_OCEAN_RAY_RECORD_FLOATS * (int)sizeof(float);

  static_assert(RAY_BYTES == 32 && RAY_RECORD_BYTES == 48, "two 16-byte loads, three 16-byte stores");

  template<int LAYOUT>
  __global__ void __launch_bounds__(RAY_THREADS) ocean_ray_kernel(RayArgs a)
  {
    // the workgroup's rays and records and nothing else (n <= INT32_MAX: first < 2^31)
    int const first = (int)blockIdx.x * RAY_THREADS;
    int const left = a.n - first;
    int const here = left < RAY_THREADS ? left : RAY_THREADS;
    int const lane = (int)threadIdx.x;

    if (lane >= here)
      return;

    __amdgpu_buffer_rsrc_t const rrays = make_rsrc(a.rays + 2 * (size_t)first, (size_t)here * RAY_BYTES);
    __amdgpu_buffer_rsrc_t const rrecords = make_rsrc(a.records + 3 * (size_t)first, (size_t)here * RAY_RECORD_BYTES);

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

    SurfaceArgs const &s = a.s;
    datum_ocean_set const &p = s.set;
    GenFrame const &f = s.frame;
    BlendList const &list = a.list;

    // rec.z of the query above (x, y), a NaN where the query gives NaNs
    auto height = [&](float x, float y) -> float
    {
      if (!ray_finite(x) || !ray_finite(y))
        return nan;

      float2 const q = make_float2(x, y);

      #define OCEAN_SURFACE_BLEND_POINT_HEIGHT
      #include "ocean_surface_blend_point.inc"
      #undef OCEAN_SURFACE_BLEND_POINT_HEIGHT

      return vz;
    };

    RayBracket const b = ray_search(ray, a.steps, a.inv, a.refine, height);

    RayPoint const at = ray_point(ray, b.hi);

    float4 rec0 = make_float4(nan, nan, nan, nan), rec1 = rec0;

    if (ray_finite(at.x) && ray_finite(at.y))
    {
      float2 const q = make_float2(at.x, at.y);

      #include "ocean_surface_blend_point.inc"

      rec0 = make_float4(vx, vy, vz, residual);
      rec1 = make_float4(mx, my, mz, foam);
    }

    buf_store_f32x4_aux<0>(make_float4(b.hi, b.lo, ray_g(at.z, rec0.z), ray_status(b.hit, b.side)), rrecords, out, 0);
    buf_store_f32x4_aux<0>(rec0, rrecords, out, 16);
    buf_store_f32x4_aux<0>(rec1, rrecords, out, 32);
  }

  inline void const *ray_kernel_for(int N)
  {
    switch(gen_layout(N))
    {
      case GEN_PLAIN: return reinterpret_cast<void const*>(&ocean_ray_kernel<GEN_PLAIN>);
      default: return reinterpret_cast<void const*>(&ocean_ray_kernel<GEN_BANDED>);
    }
  }

  // a.s.set, N, iterations, a.list, rays, records, n (> 0), steps and refine filled in
  inline hipError_t launch_rays(RayArgs &a, hipStream_t stream)
  {
    a.s.frame = make_gen_frame(a.s.set, a.s.N, 2, 2);      // the camera's terms are not read
    a.inv = 1.0f / (float)a.steps;

    void *args[] = { &a };

    return hipLaunchKernel(ray_kernel_for(a.s.N), dim3((unsigned)(((size_t)a.n + RAY_THREADS - 1) / RAY_THREADS)), dim3(RAY_THREADS), args, 0, stream);
  }
}
