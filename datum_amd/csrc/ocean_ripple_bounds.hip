// ocean_ripple_bounds.hip -- bounds of the ripple layer (include/datum_ocean_hip.h: datum_ocean_reduce_ripple_bounds) and the rippled ray
// cast that skips the samples the rippled slab decides (datum_ocean_cast_rays_rippled_bounded).  The record, the folds and the slab are
// ocean_ripple_bounds.h's, the bounded search ocean_bounds.h's, the rippled height and record ocean_rippled.hip's (a CPU walks the headers).
//
//   * ocean_ripple_bounds_partial_kernel: the current state is a flat array of R * R float2 and the extrema do not depend on the order, so
//     there is no window or torus arithmetic: every cell in memory is a cell of the window.  A lane takes two cells per 16-byte buffer
//     load through a resource laid over exactly the state plane.  256-thread workgroups, G = min(256, R * R / 512) of them (not a
//     measured choice): R = 64 gives 8 workgroups of one load per lane, R = 1024 gives 256 of eight.  A workgroup strides over the plane,
//     four loads in flight per lane, and folds in registers; then per wave across lanes (the moves of ocean_body.hip), then the four waves
//     through LDS; lane 0 writes the workgroup's partial, two 16-byte stores, the counts as integer bits.  No atomics;
//   * ocean_ripple_bounds_final_kernel: one wave folds the G partials into the record and converts the counts.  Two launches on purpose:
//     a last-workgroup-finishes form needs a release / acquire protocol across the XCDs that this project has not built;
//   * plain loads: the state was written by the ripple step just before, 8 MiB at the most;
//   * ocean_ray_rippled_bounded_kernel: ray_cast_rippled (ocean_rippled.hip) around ray_search_bounded.  The slab is formed at the top
//     from the listed cascades' records and the layer's record: wave-uniform reads of at most 17 x 32 bytes.
// LDS: 3 x 32 bytes in the partial kernel; no scratch (make resource-usage).

#pragma once

#include "ocean_ripple_bounds.h"
#include "ocean_bounds.hip"
#include "ocean_rippled.hip"

namespace ocean
{
  struct RippleBoundsArgs
  {
    float4 const *state;    // [R * R / 2] pairs of cells (eta, rate, eta, rate): the layer's current state
    float4 *partials;       // [groups] 2 float4: the four extrema, the two counts as integers' bits, 0, 0
    float4 *record;         // 2 float4
    int pairs;              // R * R / 2
    int groups;
  };

  constexpr int RIPPLE_BOUNDS_THREADS = 256;
  constexpr int RIPPLE_BOUNDS_WAVES = RIPPLE_BOUNDS_THREADS / 64;
  constexpr int RIPPLE_BOUNDS_UNROLL = 4;
  constexpr int RIPPLE_BOUNDS_MAX_GROUPS = 256;
  constexpr int RIPPLE_BOUNDS_BYTES = RIPPLE_BOUNDS_FIELDS * (int)sizeof(float);

  static_assert(RIPPLE_BOUNDS_BYTES == 32 && sizeof(float2) == 8, "two 16-byte stores; two cells per 16-byte load");

  // workgroups: one 16-byte load per lane up to the cap (every supported R has a workgroup's worth of pairs); not a measured choice
  inline int ripple_bounds_groups(int R)
  {
    int const most = (R * R) / (2 * RIPPLE_BOUNDS_THREADS);

    return most > RIPPLE_BOUNDS_MAX_GROUPS ? RIPPLE_BOUNDS_MAX_GROUPS : most < 1 ? 1 : most;
  }

  // the wave's 64 partials folded into lane 0's (what the other lanes end with is not used)
  struct RippleBoundsWave
  {
    RippleBounds b;

    template<int S>
    __device__ __forceinline__ void step()
    {
      RippleBounds o;
      o.etamin = body_lane_up<S>(b.etamin); o.etamax = body_lane_up<S>(b.etamax);
      o.ratemin = body_lane_up<S>(b.ratemin); o.ratemax = body_lane_up<S>(b.ratemax);
      o.nonfinite = __builtin_bit_cast(unsigned int, body_lane_up<S>(__builtin_bit_cast(float, b.nonfinite)));
      o.active = __builtin_bit_cast(unsigned int, body_lane_up<S>(__builtin_bit_cast(float, b.active)));

      ripple_bounds_merge(b, o);
    }
  };

  __device__ __forceinline__ float4 ripple_bounds_extrema(RippleBounds const &b)
  {
    return make_float4(b.etamin, b.etamax, b.ratemin, b.ratemax);
  }

  // a partial: the counts as integer bits
  __device__ __forceinline__ float4 ripple_bounds_counts(RippleBounds const &b)
  {
    return make_float4(__builtin_bit_cast(float, b.nonfinite), __builtin_bit_cast(float, b.active), 0.0f, 0.0f);
  }

  __device__ __forceinline__ RippleBounds ripple_bounds_partial(float4 p0, float4 p1)
  {
    RippleBounds b;
    b.etamin = p0.x; b.etamax = p0.y; b.ratemin = p0.z; b.ratemax = p0.w;
    b.nonfinite = __builtin_bit_cast(unsigned int, p1.x);
    b.active = __builtin_bit_cast(unsigned int, p1.y);
    return b;
  }

  __device__ __forceinline__ void ripple_bounds_pair(RippleBounds &b, float4 v)
  {
    ripple_bounds_cell(b, v.x, v.y);
    ripple_bounds_cell(b, v.z, v.w);
  }

  __global__ void __launch_bounds__(RIPPLE_BOUNDS_THREADS) ocean_ripple_bounds_partial_kernel(RippleBoundsArgs a)
  {
    __shared__ float4 waves[RIPPLE_BOUNDS_WAVES - 1][2];

    int const t = (int)threadIdx.x;
    int const group = (int)blockIdx.x;

    // R <= 1024: pairs <= 2^19, the plane's bytes <= 2^23
    int const pairs = a.pairs;
    int const stride = a.groups * RIPPLE_BOUNDS_THREADS;

    __amdgpu_buffer_rsrc_t const rstate = make_rsrc(a.state, (size_t)pairs * sizeof(float4));

    RippleBoundsWave wave;
    wave.b = ripple_bounds_identity();

    int r = group * RIPPLE_BOUNDS_THREADS + t;

    // (every pair read is one of the plane's: a load beyond it would give zeros, which are not the identity)
    for(; r + (RIPPLE_BOUNDS_UNROLL - 1) * stride < pairs; r += RIPPLE_BOUNDS_UNROLL * stride)
    {
      float4 v[RIPPLE_BOUNDS_UNROLL];

      #pragma unroll
      for(int u = 0; u < RIPPLE_BOUNDS_UNROLL; ++u)
        v[u] = buf_load_f32x4_aux<0>(rstate, (r + u * stride) * (int)sizeof(float4), 0);

      #pragma unroll
      for(int u = 0; u < RIPPLE_BOUNDS_UNROLL; ++u)
        ripple_bounds_pair(wave.b, v[u]);
    }

    for(; r < pairs; r += stride)
      ripple_bounds_pair(wave.b, buf_load_f32x4_aux<0>(rstate, r * (int)sizeof(float4), 0));

    body_tree(wave);

    int const w = t >> 6;

    if ((t & 63) == 0 && w > 0)
    {
      waves[w - 1][0] = ripple_bounds_extrema(wave.b);
      waves[w - 1][1] = ripple_bounds_counts(wave.b);
    }

    __syncthreads();

    if (t == 0)
    {
      #pragma unroll
      for(int k = 0; k < RIPPLE_BOUNDS_WAVES - 1; ++k)
        ripple_bounds_merge(wave.b, ripple_bounds_partial(waves[k][0], waves[k][1]));

      __amdgpu_buffer_rsrc_t const rpartial = make_rsrc(a.partials + 2 * (size_t)group, RIPPLE_BOUNDS_BYTES);

      buf_store_f32x4_aux<0>(ripple_bounds_extrema(wave.b), rpartial, 0, 0);
      buf_store_f32x4_aux<0>(ripple_bounds_counts(wave.b), rpartial, 16, 0);
    }
  }

  // one wave
  __global__ void __launch_bounds__(64) ocean_ripple_bounds_final_kernel(RippleBoundsArgs a)
  {
    int const lane = (int)threadIdx.x;

    // the partials and nothing else
    __amdgpu_buffer_rsrc_t const rpartials = make_rsrc(a.partials, (size_t)a.groups * RIPPLE_BOUNDS_BYTES);

    RippleBoundsWave wave;
    wave.b = ripple_bounds_identity();

    for(int g = lane; g < a.groups; g += 64)
      ripple_bounds_merge(wave.b, ripple_bounds_partial(buf_load_f32x4_aux<0>(rpartials, g * RIPPLE_BOUNDS_BYTES, 0), buf_load_f32x4_aux<0>(rpartials, g * RIPPLE_BOUNDS_BYTES + 16, 0)));

    body_tree(wave);

    if (lane == 0)
    {
      __amdgpu_buffer_rsrc_t const rrecord = make_rsrc(a.record, RIPPLE_BOUNDS_BYTES);

      float rec[RIPPLE_BOUNDS_FIELDS];

      ripple_bounds_record(wave.b, rec);

      buf_store_f32x4_aux<0>(make_float4(rec[0], rec[1], rec[2], rec[3]), rrecord, 0, 0);
      buf_store_f32x4_aux<0>(make_float4(rec[4], rec[5], rec[6], rec[7]), rrecord, 16, 0);
    }
  }

  // a.state, partials (groups of them), record, pairs and groups filled in
  inline hipError_t launch_ripple_bounds(RippleBoundsArgs &a, hipStream_t stream)
  {
    void *args[] = { &a };

    hipError_t const e = hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_bounds_partial_kernel), dim3((unsigned)a.groups), dim3(RIPPLE_BOUNDS_THREADS), args, 0, stream);

    if (e != hipSuccess)
      return e;

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_bounds_final_kernel), dim3(1), dim3(64), args, 0, stream);
  }

  struct RayRippledBoundedArgs
  {
    RayRippledArgs r;
    float const *bounds;        // the handle's records, [cascade][BOUNDS_FIELDS]
    float const *layerbounds;   // the layer's record, [RIPPLE_BOUNDS_FIELDS]
    int cascades[DATUM_OCEAN_MAX_CASCADES];   // the list as cascade numbers (r.a.q.list holds their maps)
  };

  template<int LAYOUT>
  __global__ void __launch_bounds__(RAY_THREADS) ocean_ray_rippled_bounded_kernel(RayRippledBoundedArgs a)
  {
    QueryArgs const &q = a.r.a.q;
    RayBatch const &r = a.r.a.r;

    // the slab of the list and the layer under the set: the records through wave-uniform indices (scalar loads)
    BoundsSlab const slab = ripple_bounds_slab(a.bounds, a.cascades, q.list.count, q.frame.basez, q.set.swellamplitude, q.frame.gx, q.frame.gy, a.layerbounds);

    ray_cast_rippled<LAYOUT>(q, a.r.layer, r, [&](Ray const &ray, auto &height) { return ray_search_bounded(ray, r.steps, r.inv, r.refine, slab.zlo, slab.zhi, height); });
  }

  // a.r as launch_rays_rippled takes it; a.bounds, a.layerbounds and a.cascades filled in
  inline hipError_t launch_rays_rippled_bounded(RayRippledBoundedArgs &a, hipStream_t stream)
  {
    return ray_launch(layout_kernel(a.r.a.q.N, &ocean_ray_rippled_bounded_kernel<GEN_PLAIN>, &ocean_ray_rippled_bounded_kernel<GEN_BANDED>), a.r.a.q, a.r.a.r, &a, stream);
  }
}
