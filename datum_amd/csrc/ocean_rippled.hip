// ocean_rippled.hip -- the ripple layer on the read side (include/datum_ocean_hip.h: datum_ocean_gen_blend_rippled,
// datum_ocean_sample_surface_blend_rippled, datum_ocean_cast_rays_rippled): the mesh, the surface query and the ray cast of the summed
// surface WITH the layer's height on top and its slopes in the shading normal -- the water coupled stepping floats its bodies on.  What
// is new in arithmetic is ocean_rippled.h's two functions (a CPU walks them); the sample is ripple_sample of ocean_ripple.h, the query
// ocean_query.hip's, the march ocean_ray.h's, the mesh stages the ocean_gen_*.inc texts: this file restates none of them.
//
//   * a sample's four cells of the layer are fetched through a buffer resource over exactly the current state plane; ripple_sample asks
//     only for cells inside the window, whose indices lie inside the plane (ocean_couple_kernel's fetch).  Nothing is written into the layer;
//   * ocean_gen_blend_rippled_kernel is ocean_gen_blend_kernel's text around one more stage: behind the cascade loop, when a cascade's
//     corner registers are dead, each of the thread's two vertices samples the layer at its own stored (x, y), the slopes take the
//     layer's share where the wave is shaded, and the store stage lifts z;
//   * ocean_surface_blend_rippled_kernel is query_each_point over the rippled record: query_sums, the layer's slopes, query_finish, the lift;
//   * ocean_ray_rippled_kernel is ray_cast's sibling (ocean_ray.hip: the same loads, bad-ray rule and stores, which that file keeps to
//     itself) around ray_search over the rippled height (query_height plus the lift) and that rippled record.
// LDS: gen's vertex staging in the mesh kernel, none in the other two; no atomics, no scratch (make resource-usage).

#pragma once

#include "ocean_rippled.h"
#include "ocean_ray.hip"
#include "ocean_ripple.hip"

namespace ocean
{
  // the layer as a read sees it
  struct RippledLayer
  {
    float2 const *state;    // [R][R] (eta, rate): the layer's current state, read only
    RippleGrid g;
  };

  struct GenBlendRippledArgs
  {
    GenBlendArgs b;
    RippledLayer layer;
  };

  struct SurfaceBlendRippledArgs
  {
    SurfaceBlendArgs b;
    RippledLayer layer;
  };

  struct RayRippledArgs
  {
    RayArgs a;
    RippledLayer layer;
  };

  __device__ __forceinline__ __amdgpu_buffer_rsrc_t rippled_rsrc(RippledLayer const &l)
  {
    return make_rsrc(l.state, (size_t)l.g.R * l.g.R * sizeof(float2));
  }

  __device__ __forceinline__ RippleSample rippled_fetch(RippledLayer const &l, __amdgpu_buffer_rsrc_t const &rstate, float x, float y)
  {
    return ripple_sample(l.g, x, y, [&rstate](int index)
    {
      float2 const c = buf_load_f32x2(rstate, index * (int)sizeof(float2), 0);

      return RippleCell{ c.x, c.y };
    });
  }

  // The rippled record above a finite q: the layer sampled at q itself, its slopes behind the list's, its height on the record's
  template<int LAYOUT>
  __device__ __forceinline__ QueryRecord rippled_record(QueryArgs const &a, RippledLayer const &l, __amdgpu_buffer_rsrc_t const &rstate, float2 q)
  {
    QueryBase const b = query_solve<LAYOUT>(a, q);

    QuerySums sums = query_sums<LAYOUT>(a, b);

    RippleSample const s = rippled_fetch(l, rstate, q.x, q.y);

    sums.sx = rippled_slope(sums.sx, s.dx);
    sums.sy = rippled_slope(sums.sy, s.dy);

    QueryRecord r = query_finish(a, b, q, sums);

    r.v.z = rippled_height(r.v.z, s);

    return r;
  }

  // The rippled height above a finite q: query_height and the same lift, the rippled record's field 2 bit for bit
  template<int LAYOUT>
  __device__ __forceinline__ float rippled_height_at(QueryArgs const &a, RippledLayer const &l, __amdgpu_buffer_rsrc_t const &rstate, float2 q)
  {
    float const height = query_height<LAYOUT>(a, query_solve<LAYOUT>(a, q));

    return rippled_height(height, rippled_fetch(l, rstate, q.x, q.y));
  }

  template<int LAYOUT>
  __attribute__((amdgpu_waves_per_eu(4, 4)))
  __global__ void __launch_bounds__(GEN_THREADS) ocean_gen_blend_rippled_kernel(GenBlendRippledArgs ra)
  {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    GenArgs const &g = ra.b.g;

#ifdef OCEAN_STAMPS
    unsigned long long *stampbase = g.stamps + (size_t)blockIdx.x * 16;
#endif

    constexpr int PH = 1;
    constexpr int ph = 0;

    #include "ocean_gen_tile.inc"

    p3 position[PH];
    v2 smoothing[PH], st[PH], ct[PH];

    #include "ocean_gen_ray.inc"

    // wave-uniform, once: the distance smoothing does not depend on the cascade
    bool const shaded = __builtin_amdgcn_ballot_w64(smoothing[ph].x != 1.0f || smoothing[ph].y != 1.0f) != 0;

    p3 displacement = { splat(0.0f), splat(0.0f), splat(0.0f) };
    v2 slopex = splat(0.0f), slopey = splat(0.0f);

    // ocean_gen_blend_kernel's loop: the addressing per cascade, then the shared text of the fetches, the blend and the sums
    #pragma unroll 1
    for(int c = 0; c < ra.b.list.count; ++c)
    {
      BlendCascade const &bc = ra.b.list.casc[c];

      __amdgpu_buffer_rsrc_t const rmap = make_rsrc(bc.map, map_cascade_bytes(g.N));

      v2 w00[PH], w10[PH], w01[PH], w11[PH];
      int o00[PH][2], o10[PH][2], o01[PH][2], o11[PH][2];
      bool near[PH];
      float4 a00[PH][2], a10[PH][2], a01[PH][2], a11[PH][2];
      GenNormalFetch b00[PH][2], b10[PH][2], b01[PH][2], b11[PH][2];
      int q00[PH][2], q10[PH][2], q01[PH][2], q11[PH][2];

      #define OCEAN_GEN_TEXEL_SCALE bc.scale
      #include "ocean_gen_texel.inc"
      #undef OCEAN_GEN_TEXEL_SCALE

      #include "ocean_gen_cascades.inc"
    }

    // the layer at each vertex's own horizontal position, the two floats the vertex stores (ocean_gen_store.inc forms them again from the
    // same operands: the same bits); the two vertices are the halves of the packed registers, so ripple_sample runs per half
    v2 const layerx = position[ph].x - displacement.x, layery = position[ph].y - displacement.y;

    __amdgpu_buffer_rsrc_t const rstate = rippled_rsrc(ra.layer);

    v2 lift;

    #pragma unroll
    for(int i = 0; i < 2; ++i)
    {
      RippleSample const s = rippled_fetch(ra.layer, rstate, layerx[i], layery[i]);

      lift[i] = s.eta;

      if (shaded)
      {
        slopex[i] = rippled_slope(slopex[i], s.dx);
        slopey[i] = rippled_slope(slopey[i], s.dy);
      }
    }

    float4 *mine = reinterpret_cast<float4*>(smem) + 384 * wave;

    p3 const planen = { splat(p.plane[0]), splat(p.plane[1]), splat(p.plane[2]) };

    p3 tbn2;

    if (shaded)
    {
      p3 const dn = normalize3(p3{ slopex, slopey, splat(1.0f) });

      #include "ocean_gen_frame.inc"
    }
    else
      tbn2 = normalize3(planen);

    // pz' = pz + eta: rippled_height's one addition, on both halves
    #define OCEAN_GEN_STORE_LIFT lift
    #include "ocean_gen_store.inc"
    #undef OCEAN_GEN_STORE_LIFT
  }

  template<int LAYOUT>
  __global__ void __launch_bounds__(SURFACE_THREADS) ocean_surface_blend_rippled_kernel(SurfaceBlendRippledArgs r)
  {
    __amdgpu_buffer_rsrc_t const rstate = rippled_rsrc(r.layer);

    query_each_point(r.b.points, r.b.samples, r.b.count, [&](float2 q) { return rippled_record<LAYOUT>(r.b.q, r.layer, rstate, q); });
  }

  // ray_cast's sibling over the rippled water (ocean_ray.hip: ray_cast, whose text and device code stay as they are): a ray's loads, the
  // bad ray's record and the stores as there, the height and the record the rippled ones
  template<int LAYOUT, class Search>
  __device__ __forceinline__ void ray_cast_rippled(QueryArgs const &a, RippledLayer const &l, RayBatch const &r, Search &&search)
  {
    // the workgroup's rays and records and nothing else (n <= INT32_MAX: first < 2^31)
    int const first = (int)blockIdx.x * RAY_THREADS;
    int const left = r.n - first;
    int const here = left < RAY_THREADS ? left : RAY_THREADS;
    int const lane = (int)threadIdx.x;

    if (lane >= here)
      return;

    __amdgpu_buffer_rsrc_t const rstate = rippled_rsrc(l);
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

      return rippled_height_at<LAYOUT>(a, l, rstate, make_float2(x, y));
    };

    RayBracket const b = search(ray, height);

    RayPoint const at = ray_point(ray, b.hi);

    QueryRecord rec = { make_float4(nan, nan, nan, nan), make_float4(nan, nan, nan, nan) };

    if (ray_finite(at.x) && ray_finite(at.y))
      rec = rippled_record<LAYOUT>(a, l, rstate, make_float2(at.x, at.y));

    buf_store_f32x4_aux<0>(make_float4(b.hi, b.lo, ray_g(at.z, rec.v.z), ray_status(b.hit, b.side)), rrecords, out, 0);
    buf_store_f32x4_aux<0>(rec.v, rrecords, out, 16);
    buf_store_f32x4_aux<0>(rec.m, rrecords, out, 32);
  }

  template<int LAYOUT>
  __global__ void __launch_bounds__(RAY_THREADS) ocean_ray_rippled_kernel(RayRippledArgs ra)
  {
    RayBatch const &r = ra.a.r;

    ray_cast_rippled<LAYOUT>(ra.a.q, ra.layer, r, [&](Ray const &ray, auto &height) { return ray_search(ray, r.steps, r.inv, r.refine, height); });
  }

  // r.b as launch_gen_blend wants it, r.layer filled in
  inline hipError_t launch_gen_blend_rippled(GenBlendRippledArgs &r, int N, int sizex, int sizey, hipStream_t stream)
  {
    gen_shape(r.b.g, N, sizex, sizey);

    void *args[] = { &r };

    return hipLaunchKernel(layout_kernel(N, &ocean_gen_blend_rippled_kernel<GEN_PLAIN>, &ocean_gen_blend_rippled_kernel<GEN_BANDED>), dim3(gen_groups(r.b.g)), dim3(GEN_THREADS), args, GEN_LDS, stream);
  }

  // r.b as launch_surface_blend wants it (count > 0), r.layer filled in
  inline hipError_t launch_surface_blend_rippled(SurfaceBlendRippledArgs &r, hipStream_t stream)
  {
    query_frame(r.b.q);

    void *args[] = { &r };

    return hipLaunchKernel(layout_kernel(r.b.q.N, &ocean_surface_blend_rippled_kernel<GEN_PLAIN>, &ocean_surface_blend_rippled_kernel<GEN_BANDED>), dim3((unsigned)((r.b.count + SURFACE_THREADS - 1) / SURFACE_THREADS)), dim3(SURFACE_THREADS), args, 0, stream);
  }

  // r.a as launch_rays wants it (n > 0), r.layer filled in
  inline hipError_t launch_rays_rippled(RayRippledArgs &r, hipStream_t stream)
  {
    return ray_launch(layout_kernel(r.a.q.N, &ocean_ray_rippled_kernel<GEN_PLAIN>, &ocean_ray_rippled_kernel<GEN_BANDED>), r.a.q, r.a.r, &r, stream);
  }
}
