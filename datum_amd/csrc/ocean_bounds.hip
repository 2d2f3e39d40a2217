// ocean_bounds.hip -- surface bounds per cascade (include/datum_ocean_hip.h: datum_ocean_reduce_bounds) and the ray cast that skips the
// samples they decide (datum_ocean_cast_rays_bounded).  The record, the folds, the slab and the bounded search are ocean_bounds.h's (a CPU
// walks the same functions).
//
//   * ocean_bounds_partial_kernel: the maps are arrays of 384-byte patches and the extrema do not depend on the order, so there is no
//     layout arithmetic and no LAYOUT form: a cascade is N * N / 16 patches, texel r of that order lies at (r / 16) * 384 + (r % 16) * 16.
//     16 neighbouring lanes read one patch's part A -- (dx, dy, dz, nx), two whole 128-byte lines -- one 16-byte buffer load per lane
//     through a resource laid over the cascade's map block; part B is never read.  256-thread workgroups, grid = G x cascades; a workgroup
//     strides over its cascade's texels, four loads in flight per lane, and folds in registers; then per wave across lanes (the moves of
//     ocean_body.hip), then the four waves through LDS; lane 0 writes the workgroup's partial, two 16-byte stores.  No atomics;
//   * ocean_bounds_final_kernel: one wave per cascade folds the G partials (a workgroup without texels wrote the identity) into the record;
//   * cache policy: plain loads, the foam kernel's choice for the same 16 bytes per point right behind the column pass (ocean_foam.hip;
//     DESIGN.md 5.10): the maps of a resident handle are in the Infinity Cache then, and a streamed handle's are not whatever the load says;
//   * ocean_ray_bounded_kernel: ocean_ray_kernel's body (ocean_ray.hip: ray_cast) with ray_search_bounded in place of ray_search.  The slab
//     is formed at the top from the listed cascades' records in the handle's bounds buffer: wave-uniform reads of at most 16 x 32 bytes.
//     Every height is still query_height, the record at `hi` query_record once (ocean_query.hip).
// LDS: 3 x 32 bytes in the partial kernel; no scratch (make resource-usage).

#pragma once

#include "ocean_bounds.h"
#include "ocean_body.hip"
#include "ocean_ray.hip"

namespace ocean
{
  struct BoundsArgs
  {
    float4 const *maps;     // [cascade] map blocks (map_cascade_bytes each)
    float4 *partials;       // [cascade][groups] 2 float4: the six extrema, the count as an integer's bits, 0
    float4 *records;        // [cascade] 2 float4
    int N;
    int groups;             // workgroups per cascade
  };

  constexpr int BOUNDS_THREADS = 256;
  constexpr int BOUNDS_WAVES = BOUNDS_THREADS / 64;
  constexpr int BOUNDS_UNROLL = 4;
  constexpr int BOUNDS_MAX_GROUPS = 1024;
  constexpr int BOUNDS_BYTES = BOUNDS_FIELDS * (int)sizeof(float);

  static_assert(BOUNDS_BYTES == 32 && MAP_PATCH == 16 && MAP_A_STRIDE == 16, "two 16-byte stores; sixteen 16-byte parts A per patch");

  // workgroups per cascade: enough for the launch to fill the device, none without a texel where the cascade has a workgroup's worth
  // of them (every supported N has), never fewer than one (not a measured choice)
  inline int bounds_groups(int N, int cascades)
  {
    int const most = (int)(((size_t)N * N) / BOUNDS_THREADS);
    int const want = BOUNDS_MAX_GROUPS / cascades;
    int const groups = want > most ? most : want;

    return groups < 1 ? 1 : groups;
  }

  // byte offset of texel r's part A in its cascade's block, the texels counted patch after patch (ocean_layout.h: map_part_a)
  __device__ __forceinline__ int bounds_part_a(int r)
  {
    return (r >> MAP_PATCH_LOG2) * MAP_PATCH_BYTES + (r & (MAP_PATCH - 1)) * MAP_A_STRIDE;
  }

  // the wave's 64 partials folded into lane 0's (what the other lanes end with is not used)
  struct BoundsWave
  {
    Bounds b;

    template<int S>
    __device__ __forceinline__ void step()
    {
      Bounds o;
      o.zmin = body_lane_up<S>(b.zmin); o.zmax = body_lane_up<S>(b.zmax);
      o.xmin = body_lane_up<S>(b.xmin); o.xmax = body_lane_up<S>(b.xmax);
      o.ymin = body_lane_up<S>(b.ymin); o.ymax = body_lane_up<S>(b.ymax);
      o.nonfinite = __builtin_bit_cast(unsigned int, body_lane_up<S>(__builtin_bit_cast(float, b.nonfinite)));

      bounds_merge(b, o);
    }
  };

  __device__ __forceinline__ void bounds_store(Bounds const &b, float count, __amdgpu_buffer_rsrc_t r)
  {
    buf_store_f32x4_aux<0>(make_float4(b.zmin, b.zmax, b.xmin, b.xmax), r, 0, 0);
    buf_store_f32x4_aux<0>(make_float4(b.ymin, b.ymax, count, 0.0f), r, 16, 0);
  }

  __device__ __forceinline__ Bounds bounds_load(__amdgpu_buffer_rsrc_t r, int offset)
  {
    float4 const p0 = buf_load_f32x4_aux<0>(r, offset, 0);
    float4 const p1 = buf_load_f32x4_aux<0>(r, offset + 16, 0);

    Bounds b;
    b.zmin = p0.x; b.zmax = p0.y; b.xmin = p0.z; b.xmax = p0.w;
    b.ymin = p1.x; b.ymax = p1.y;
    b.nonfinite = __builtin_bit_cast(unsigned int, p1.z);
    return b;
  }

  __global__ void __launch_bounds__(BOUNDS_THREADS) ocean_bounds_partial_kernel(BoundsArgs a)
  {
    __shared__ float4 waves[BOUNDS_WAVES - 1][2];

    int const t = (int)threadIdx.x;
    int const group = (int)blockIdx.x;
    int const cascade = (int)blockIdx.y;

    // N <= 4096: texels <= 2^24, a block's bytes (24 per texel) below 2^31
    int const texels = a.N * a.N;
    int const stride = a.groups * BOUNDS_THREADS;

    __amdgpu_buffer_rsrc_t const rmaps = make_rsrc(reinterpret_cast<char const*>(a.maps) + (size_t)cascade * map_cascade_bytes(a.N), map_cascade_bytes(a.N));

    BoundsWave wave;
    wave.b = bounds_identity();

    int r = group * BOUNDS_THREADS + t;

    // (every texel read is one of the cascade's: a load beyond the block would give zeros, which are not the identity)
    for(; r + (BOUNDS_UNROLL - 1) * stride < texels; r += BOUNDS_UNROLL * stride)
    {
      float4 v[BOUNDS_UNROLL];

      #pragma unroll
      for(int u = 0; u < BOUNDS_UNROLL; ++u)
        v[u] = buf_load_f32x4_aux<0>(rmaps, bounds_part_a(r + u * stride), 0);

      #pragma unroll
      for(int u = 0; u < BOUNDS_UNROLL; ++u)
        bounds_texel(wave.b, v[u].x, v[u].y, v[u].z);
    }

    for(; r < texels; r += stride)
    {
      float4 const v = buf_load_f32x4_aux<0>(rmaps, bounds_part_a(r), 0);

      bounds_texel(wave.b, v.x, v.y, v.z);
    }

    body_tree(wave);

    int const w = t >> 6;

    if ((t & 63) == 0 && w > 0)
    {
      waves[w - 1][0] = make_float4(wave.b.zmin, wave.b.zmax, wave.b.xmin, wave.b.xmax);
      waves[w - 1][1] = make_float4(wave.b.ymin, wave.b.ymax, __builtin_bit_cast(float, wave.b.nonfinite), 0.0f);
    }

    __syncthreads();

    if (t == 0)
    {
      #pragma unroll
      for(int k = 0; k < BOUNDS_WAVES - 1; ++k)
      {
        float4 const p0 = waves[k][0], p1 = waves[k][1];

        Bounds o;
        o.zmin = p0.x; o.zmax = p0.y; o.xmin = p0.z; o.xmax = p0.w;
        o.ymin = p1.x; o.ymax = p1.y;
        o.nonfinite = __builtin_bit_cast(unsigned int, p1.z);

        bounds_merge(wave.b, o);
      }

      __amdgpu_buffer_rsrc_t const rpartial = make_rsrc(a.partials + 2 * ((size_t)cascade * a.groups + group), BOUNDS_BYTES);

      bounds_store(wave.b, __builtin_bit_cast(float, wave.b.nonfinite), rpartial);
    }
  }

  // one wave per cascade
  __global__ void __launch_bounds__(64) ocean_bounds_final_kernel(BoundsArgs a)
  {
    int const lane = (int)threadIdx.x;
    int const cascade = (int)blockIdx.x;

    // the cascade's partials and nothing else
    __amdgpu_buffer_rsrc_t const rpartials = make_rsrc(a.partials + 2 * (size_t)cascade * a.groups, (size_t)a.groups * BOUNDS_BYTES);

    BoundsWave wave;
    wave.b = bounds_identity();

    for(int g = lane; g < a.groups; g += 64)
      bounds_merge(wave.b, bounds_load(rpartials, g * BOUNDS_BYTES));

    body_tree(wave);

    if (lane == 0)
    {
      __amdgpu_buffer_rsrc_t const rrecord = make_rsrc(a.records + 2 * (size_t)cascade, BOUNDS_BYTES);

      bounds_store(wave.b, (float)wave.b.nonfinite, rrecord);          // bounds_record's fields
    }
  }

  // a.maps, partials, records (cascades x groups and cascades records), N and groups filled in
  inline hipError_t launch_bounds(BoundsArgs &a, int cascades, hipStream_t stream)
  {
    void *args[] = { &a };

    hipError_t const e = hipLaunchKernel(reinterpret_cast<void const*>(&ocean_bounds_partial_kernel), dim3((unsigned)a.groups, (unsigned)cascades), dim3(BOUNDS_THREADS), args, 0, stream);

    if (e != hipSuccess)
      return e;

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_bounds_final_kernel), dim3((unsigned)cascades), dim3(64), args, 0, stream);
  }

  struct RayBoundedArgs
  {
    QueryArgs q;
    RayBatch r;
    float const *bounds;    // the handle's records, [cascade][BOUNDS_FIELDS]
    int cascades[DATUM_OCEAN_MAX_CASCADES];   // the list as cascade numbers (q.list holds their maps)
  };

  // (eight waves per SIMD as ocean_ray_kernel has them: left alone the compiler takes 106 scalar registers, which leaves room for seven)
  template<int LAYOUT>
  __attribute__((amdgpu_waves_per_eu(8, 8)))
  __global__ void __launch_bounds__(RAY_THREADS) ocean_ray_bounded_kernel(RayBoundedArgs a)
  {
    RayBatch const &r = a.r;

    // the slab of the list under the set: the records through a wave-uniform index (scalar loads)
    BoundsSlab const slab = bounds_slab(a.bounds, a.cascades, a.q.list.count, a.q.frame.basez, a.q.set.swellamplitude, a.q.frame.gx, a.q.frame.gy);

    ray_cast<LAYOUT>(a.q, r, [&](Ray const &ray, auto &height) { return ray_search_bounded(ray, r.steps, r.inv, r.refine, slab.zlo, slab.zhi, height); });
  }

  // a.q and a.r as launch_rays takes them; a.bounds and a.cascades filled in
  inline hipError_t launch_rays_bounded(RayBoundedArgs &a, hipStream_t stream)
  {
    return ray_launch(layout_kernel(a.q.N, &ocean_ray_bounded_kernel<GEN_PLAIN>, &ocean_ray_bounded_kernel<GEN_BANDED>), a.q, a.r, &a, stream);
  }
}
