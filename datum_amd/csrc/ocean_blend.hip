// ocean_blend.hip -- several cascades at once on the read side (include/datum_ocean_hip.h: datum_ocean_gen_blend,
// datum_ocean_sample_surface_blend): the mesh of the SUMMED surface, and height, normal and foam of that same surface above world points.
//
// A blend is a list of up to DATUM_OCEAN_MAX_CASCADES cascades of one handle (one N).  At a position P every listed cascade c is sampled
// at P.xy * scale_c with gen's REPEAT bilinear fetch; the displacements add in list order (the first taken as it is, one fp32 addition per
// component for each further one), the normals add as SLOPES: the map stores m = normalize(l.z - r.z, b.z - t.z, 4 wavescale / N), so
// m.x / m.z = -1/2 dz/dx in world units whatever the cascade's wavescale, p = sum of (m.x / m.z, m.y / m.z), dn = normalize(p.x, p.y, 1).
//
//   * ocean_gen_blend_kernel is ocean_gen_kernel's tile, ray stage, texel addressing, shading frame and vertex store -- the same text,
//     ocean_gen_*.inc -- around a loop over the list.  The ray stage runs once per vertex, the addressing once per cascade.  One cascade's
//     fetches are in flight at a time: the accumulators are 6 + 4 registers, a second cascade's 48 registers of corners would cost a wave
//     per SIMD;
//   * gen's per-wave shortcuts, per cascade: `shaded` (the wave needs normals) depends on the distance smoothing alone, `near` (some
//     second texel has a weight) on scale_c -- a fine cascade is beyond 2^23 texels where a coarse one is not;
//   * ocean_surface_blend_kernel is ocean_surface_kernel with V(b) summed over the list; parts B and the foam planes are fetched in the
//     final evaluation only.  The solve and the final evaluations of one point are functions of their own (ocean_query.hip: query_solve,
//     query_record, ...), which the body, ray and velocity kernels call as well;
//   * the list travels in the kernel argument: 16 x (map, foam plane, scale) = 384 bytes.
// LDS: gen's vertex staging; no scratch (make resource-usage).

#pragma once

#include "ocean_gen.hip"
#include "ocean_query.hip"

namespace ocean
{
  struct GenBlendArgs
  {
    GenArgs g;              // g.map and g.set.scale are not read
    BlendList list;
  };

  struct SurfaceBlendArgs
  {
    QueryArgs q;
    float2 const *points;
    float4 *samples;        // 2 float4 per point
    int count;
  };

  template<int LAYOUT>
  __attribute__((amdgpu_waves_per_eu(4, 4)))
  __global__ void __launch_bounds__(GEN_THREADS) ocean_gen_blend_kernel(GenBlendArgs b)
  {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    GenArgs const &g = b.g;

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

    #pragma unroll 1
    for(int c = 0; c < b.list.count; ++c)
    {
      BlendCascade const &bc = b.list.casc[c];

      __amdgpu_buffer_rsrc_t const rmap = make_rsrc(bc.map, map_cascade_bytes(g.N));

      // (declared per cascade: nothing of one cascade's corners is carried into the next one's registers)
      v2 w00[PH], w10[PH], w01[PH], w11[PH];
      int o00[PH][2], o10[PH][2], o01[PH][2], o11[PH][2];
      bool near[PH];
      float4 a00[PH][2], a10[PH][2], a01[PH][2], a11[PH][2];
      GenNormalFetch b00[PH][2], b10[PH][2], b01[PH][2], b11[PH][2];
      int q00[PH][2], q10[PH][2], q01[PH][2], q11[PH][2];

      #define OCEAN_GEN_TEXEL_SCALE bc.scale
      #include "ocean_gen_texel.inc"
      #undef OCEAN_GEN_TEXEL_SCALE

      // (the fetches, the blend and the sums: text shared with ocean_gen_blend_rippled_kernel, ocean_rippled.hip)
      #include "ocean_gen_cascades.inc"
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

    #include "ocean_gen_store.inc"
  }

  template<int LAYOUT>
  __global__ void __launch_bounds__(SURFACE_THREADS) ocean_surface_blend_kernel(SurfaceBlendArgs b)
  {
    query_each_point(b.points, b.samples, b.count, [&](float2 q) { return query_record<LAYOUT>(b.q, query_solve<LAYOUT>(b.q, q), q); });
  }

  // b.g.set, b.g.vertices and b.list filled in
  inline hipError_t launch_gen_blend(GenBlendArgs &b, int N, int sizex, int sizey, hipStream_t stream)
  {
    gen_shape(b.g, N, sizex, sizey);

    void *args[] = { &b };

    return hipLaunchKernel(layout_kernel(N, &ocean_gen_blend_kernel<GEN_PLAIN>, &ocean_gen_blend_kernel<GEN_BANDED>), dim3(gen_groups(b.g)), dim3(GEN_THREADS), args, GEN_LDS, stream);
  }

  // b.q (but its frame), points, samples and count (> 0) filled in
  inline hipError_t launch_surface_blend(SurfaceBlendArgs &b, hipStream_t stream)
  {
    query_frame(b.q);

    void *args[] = { &b };

    return hipLaunchKernel(layout_kernel(b.q.N, &ocean_surface_blend_kernel<GEN_PLAIN>, &ocean_surface_blend_kernel<GEN_BANDED>), dim3((unsigned)((b.count + SURFACE_THREADS - 1) / SURFACE_THREADS)), dim3(SURFACE_THREADS), args, 0, stream);
  }
}
