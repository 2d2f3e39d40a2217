// ocean_surface.hip -- surface queries (include/datum_ocean_hip.h: datum_ocean_sample_surface): the water surface above world points.
//
// ocean.gen places the vertex of base point b at V(b) = P(b) - D(P(b)) horizontally (gen.comp:122-124), so the water above q comes from
// another texel: the query solves V(b).xy = q by the fixed-point iteration b <- b + (q - V(b).xy), a fixed number of times from b = q, and
// evaluates V, the shading normal and the foam plane once more at the final b.  Every term is gen's own fp32 expression (ocean_gen.hip):
// the swell frame of make_gen_frame, sincos_phase, the REPEAT bilinear fetch with its fract wrap and TexelIndex's layout arithmetic, and
// the shading frame of gen.comp:101-120 with smoothing = 0.
//
//   * one point per thread; a point is 8 bytes in (coalesced float2), a record 32 bytes out (two 16-byte stores);
//   * the iterations fetch part A of the four corners (dx, dy, dz, nx: 16 B each); part B (ny, nz) and the foam plane only after the last;
//   * every fetch goes through a buffer resource sized to the cascade's map (foam: plane), so no coordinate can fault; a zero bilinear
//     weight pushes its corner out of range as gen does (beyond |coordinate| = 2^23 texels);
//   * a point with a non-finite coordinate gets a record of quiet NaNs and fetches nothing.
// No LDS, no scratch (make resource-usage).

#pragma once

#include "ocean_layout.h"
#include "ocean_gen.hip"

namespace ocean
{
  struct SurfaceArgs
  {
    datum_ocean_set set;
    GenFrame frame;
    float4 const *map;      // the cascade's displacement map, map_cascade_bytes(N) bytes
    float const *foam;      // the cascade's foam plane, N * N floats; nullptr while foam is OFF
    float2 const *points;
    float4 *samples;        // 2 float4 per point
    int N;
    int count;
    int iterations;
  };

  constexpr int SURFACE_THREADS = 256;

  // the REPEAT bilinear fetch of gen (ocean_gen.hip, gen.comp:113-114) at world position (px, py): weights and byte offsets of part A
  // of the four corners (a zero-weight corner pushed out of the buffer), plus the row / column parts the normal layer and the foam need
  template<int LAYOUT>
  struct SurfaceTexel
  {
    float w00, w10, w01, w11;
    int o00, o10, o01, o11;
    int i0, i1, j0, j1;
    bool wantx, wanty;

    __device__ __forceinline__ SurfaceTexel(TexelIndex<LAYOUT> const &texel, GenFrame const &f, float scale, int nmask, float px, float py)
    {
      float const fx = (px * scale) * f.fn - 0.5f;
      float const fy = (py * scale) * f.fn - 0.5f;

      float const flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);

      float const ax = fx - flx, ay = fy - fly;

      // floor(coordinate) mod N: exact, N is a power of two (ocean_gen.hip)
      float const mx = __builtin_amdgcn_fractf(flx * f.rfn) * f.fn;
      float const my = __builtin_amdgcn_fractf(fly * f.rfn) * f.fn;

      float const bx = 1.0f - ax, by = 1.0f - ay;

      w00 = bx * by; w10 = ax * by; w01 = bx * ay; w11 = ax * ay;

      i0 = (int)mx; j0 = (int)my;
      i1 = (i0 + 1) & nmask; j1 = (j0 + 1) & nmask;

      int const c0 = texel.column(i0), c1 = texel.column(i1);
      int const r0 = texel.row(j0), r1 = texel.row(j1);

      wantx = ax != 0.0f; wanty = ay != 0.0f;

      o00 = r0 + c0; o10 = wantx ? r0 + c1 : -256; o01 = wanty ? r1 + c0 : -256; o11 = (wantx && wanty) ? r1 + c1 : -256;
    }

    // gen's blend order: w11 a11 + (w01 a01 + (w10 a10 + w00 a00)), FMAs
    __device__ __forceinline__ float blend(float a00, float a10, float a01, float a11) const
    {
      return fmaf(w11, a11, fmaf(w01, a01, fmaf(w10, a10, w00 * a00)));
    }
  };

  __device__ __forceinline__ void normalize3(float &x, float &y, float &z)
  {
    float const inv = __builtin_amdgcn_rsqf(fmaf(z, z, fmaf(y, y, x * x)));

    x *= inv; y *= inv; z *= inv;
  }

  template<int LAYOUT>
  __global__ void __launch_bounds__(SURFACE_THREADS) ocean_surface_kernel(SurfaceArgs s)
  {
    int const k = (int)blockIdx.x * SURFACE_THREADS + (int)threadIdx.x;

    if (k >= s.count)
      return;

    datum_ocean_set const &p = s.set;
    GenFrame const &f = s.frame;

    float2 const q = s.points[k];

    float4 *out = s.samples + 2 * (size_t)k;

    if (!__builtin_isfinite(q.x) || !__builtin_isfinite(q.y))
    {
      float const nan = __builtin_nanf("");

      out[0] = make_float4(nan, nan, nan, nan);
      out[1] = make_float4(nan, nan, nan, nan);
      return;
    }

    TexelIndex<LAYOUT> const texel(s.N);

    int const nmask = s.N - 1;

    __amdgpu_buffer_rsrc_t const rmap = make_rsrc(s.map, map_cascade_bytes(s.N));

    float const dirx = p.swelldirection[0], diry = p.swelldirection[1];

    float bx = q.x, by = q.y;

    // V(b) of gen's vertex for base point b; `last` = the final evaluation, which keeps what the normal and the foam need
    float st, ct, px, py;
    float4 a00, a10, a01, a11;

    for(int it = 0; ; ++it)
    {
      float const theta = f.frequency * (dirx * bx + diry * by) + p.swellphase;

      sincos_phase(theta, &st, &ct);

      px = bx + f.gx * ct;
      py = by + f.gy * ct;

      SurfaceTexel<LAYOUT> const t(texel, f, p.scale, nmask, px, py);

      a00 = buf_load_f32x4_aux<0>(rmap, t.o00, 0);
      a10 = buf_load_f32x4_aux<0>(rmap, t.o10, 0);
      a01 = buf_load_f32x4_aux<0>(rmap, t.o01, 0);
      a11 = buf_load_f32x4_aux<0>(rmap, t.o11, 0);

      if (it == s.iterations)
        break;

      float const vx = px - t.blend(a00.x, a10.x, a01.x, a11.x);
      float const vy = py - t.blend(a00.y, a10.y, a01.y, a11.y);

      bx = bx + (q.x - vx);
      by = by + (q.y - vy);
    }

    // the final evaluation at b: the corners' part A is in registers, part B (ny, nz) and the foam are fetched now
    SurfaceTexel<LAYOUT> const t(texel, f, p.scale, nmask, px, py);

    int const bc0 = texel.bcolumn(t.i0), bc1 = texel.bcolumn(t.i1);
    int const br0 = MAP_PART_B - texel.brow(t.j0), br1 = MAP_PART_B - texel.brow(t.j1);

    float2 const b00 = buf_load_f32x2(rmap, t.o00 + br0 - bc0, 0);
    float2 const b10 = buf_load_f32x2(rmap, t.wantx ? t.o10 + br0 - bc1 : -256, 0);
    float2 const b01 = buf_load_f32x2(rmap, t.wanty ? t.o01 + br1 - bc0 : -256, 0);
    float2 const b11 = buf_load_f32x2(rmap, (t.wantx && t.wanty) ? t.o11 + br1 - bc1 : -256, 0);

    float foam = 0.0f;

    if (s.foam)
    {
      __amdgpu_buffer_rsrc_t const rfoam = make_rsrc(s.foam, (size_t)s.N * s.N * sizeof(float));

      int const f00 = ((t.j0 << texel.ln) + t.i0) * 4;

      float const g00 = buf_load_f32(rfoam, f00, 0);
      float const g10 = buf_load_f32(rfoam, t.wantx ? ((t.j0 << texel.ln) + t.i1) * 4 : -256, 0);
      float const g01 = buf_load_f32(rfoam, t.wanty ? ((t.j1 << texel.ln) + t.i0) * 4 : -256, 0);
      float const g11 = buf_load_f32(rfoam, (t.wantx && t.wanty) ? ((t.j1 << texel.ln) + t.i1) * 4 : -256, 0);

      foam = t.blend(g00, g10, g01, g11);
    }

    float const dx = t.blend(a00.x, a10.x, a01.x, a11.x);
    float const dy = t.blend(a00.y, a10.y, a01.y, a11.y);
    float const dz = t.blend(a00.z, a10.z, a01.z, a11.z);

    float const vx = px - dx, vy = py - dy, vz = (f.basez + p.swellamplitude * st) + dz;

    float const rx = vx - q.x, ry = vy - q.y;
    float const residual = __builtin_sqrtf(fmaf(ry, ry, rx * rx));

    // gen's shading frame (gen.comp:101-120) with smoothing = 0: tbn[2] = normalize(t0 m.x + t1 m.y + t2 m.z)
    float const nx = t.blend(a00.w, a10.w, a01.w, a11.w);
    float const ny = t.blend(b00.x, b10.x, b01.x, b11.x);
    float const nz = t.blend(b00.y, b10.y, b01.y, b11.y);

    float t2x = -f.nx * ct, t2y = -f.ny * ct, t2z = fmaf(-f.nz, st, 1.0f);
    float t0x = fmaf(-f.tx, st, 1.0f), t0y = -f.ty * st, t0z = f.tz * ct;

    normalize3(t2x, t2y, t2z);
    normalize3(t0x, t0y, t0z);

    float const t1x = t0y * t2z - t0z * t2y, t1y = t0z * t2x - t0x * t2z, t1z = t0x * t2y - t0y * t2x;

    float mx = fmaf(nz, t2x, fmaf(ny, t1x, nx * t0x));
    float my = fmaf(nz, t2y, fmaf(ny, t1y, nx * t0y));
    float mz = fmaf(nz, t2z, fmaf(ny, t1z, nx * t0z));

    normalize3(mx, my, mz);

    out[0] = make_float4(vx, vy, vz, residual);
    out[1] = make_float4(mx, my, mz, foam);
  }

  // s.set, s.map, s.foam, s.points, s.samples, s.N, s.count and s.iterations filled in; count > 0
  inline hipError_t launch_surface(SurfaceArgs &s, hipStream_t stream)
  {
    s.frame = make_gen_frame(s.set, s.N, 2, 2);      // the camera's terms are not read

    void *args[] = { &s };

    return hipLaunchKernel(layout_kernel(s.N, &ocean_surface_kernel<GEN_PLAIN>, &ocean_surface_kernel<GEN_BANDED>), dim3((unsigned)((s.count + SURFACE_THREADS - 1) / SURFACE_THREADS)), dim3(SURFACE_THREADS), args, 0, stream);
  }
}
