// ocean_ripple.hip -- the ripple layer (include/datum_ocean_hip.h: "ripple layer"): a local R x R height field with a damped wave
// equation, fed by integer deposits, that scrolls with its centre over a torus in memory.  The arithmetic is ocean_ripple.h's (a CPU
// walks the same functions); this file is how the cells reach it.
//
// ocean_ripple_step_kernel, one sub-step:
//   * one 256-thread workgroup per 64 x 16 tile aligned in MEMORY coordinates (the window wraps the torus wherever its origin puts it;
//     window coordinates are derived per cell, (mx - ox) mod R, for the border and the sponge): a wave loads and stores whole 512-byte
//     rows of float2, four 128-byte lines, and whole 256-byte rows of src;
//   * the tile's heights and a one-cell halo (64 above, 64 below, 16 left, 16 right, wrapped; no corners, the stencil has none) are
//     staged in LDS as floats, the first sub-step's deposits already added, 18 x 66 x 4 = 4752 bytes; the rate stays in registers.
//     A row of the image is 66 floats: the 64 lanes of a wave read 64 consecutive banks, the row above or below starts 2 banks on;
//   * a neighbour outside the WINDOW is 0 whatever memory holds there (select on the window coordinate);
//   * the new state is written through (sc0 sc1), as the maps and the foam plane are: the next sub-step's tile runs on any XCD;
//   * every access goes through a buffer resource over exactly the plane: no index can reach outside it.
// The deposits are vector atomics on the int plane (atomicAdd), in any order: integer sums commute.
// No scratch (make resource-usage).

#pragma once

#include "ocean_ripple.h"
#include "ocean_drag.hip"

namespace ocean
{
  constexpr int RIPPLE_TX = 64, RIPPLE_TY = 16, RIPPLE_THREADS = 256;
  constexpr int RIPPLE_PER_THREAD = RIPPLE_TX * RIPPLE_TY / RIPPLE_THREADS;      // 4
  constexpr int RIPPLE_ROWSTEP = RIPPLE_THREADS / RIPPLE_TX;                     // 4
  constexpr int RIPPLE_HALO = 2 * RIPPLE_TX + 2 * RIPPLE_TY;                     // 160 cells
  constexpr int RIPPLE_LX = RIPPLE_TX + 2;
  constexpr int RIPPLE_STORE_AUX = 17;

  static_assert(RIPPLE_TX == 64 && RIPPLE_HALO <= RIPPLE_THREADS, "one wave per tile row; one halo cell per thread");

  struct RippleStepArgs
  {
    float2 const *in;       // [R][R] (eta, rate), memory order
    float2 *out;
    int const *src;         // [R][R] pending deposits, read by the first sub-step only
    RippleGrid g;
    int B;                  // sponge cells, 0 .. RIPPLE_MAX_SPONGE
    float h, c2s2;
    float f[RIPPLE_MAX_SPONGE + 1];   // the sponge table for this h
  };

  template<bool FIRST>
  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_step_kernel(RippleStepArgs a)
  {
    __shared__ float tile[RIPPLE_TY + 2][RIPPLE_LX];

    int const R = a.g.R;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * RIPPLE_TX;
    int const y0 = (int)blockIdx.y * RIPPLE_TY;

    size_t const cells = (size_t)R * R;

    __amdgpu_buffer_rsrc_t const rin = make_rsrc(a.in, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rout = make_rsrc(a.out, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rsrc = make_rsrc(a.src, cells * sizeof(int));

    int const lx = t & (RIPPLE_TX - 1);
    int const ly = t / RIPPLE_TX;

    // body: memory cell (x0 + lx, y0 + ly + 4 s)
    float2 body[RIPPLE_PER_THREAD];
    int bsrc[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const cell = (y0 + ly + RIPPLE_ROWSTEP * s) * R + x0 + lx;

      body[s] = buf_load_f32x2(rin, cell * (int)sizeof(float2), 0);
      bsrc[s] = FIRST ? (int)buf_load_u32(rsrc, cell * (int)sizeof(int), 0) : 0;
    }

    // halo: the rows above and below, then the columns left and right, wrapped on the torus; only the height is needed
    float halo = 0.0f;
    int hsrc = 0;
    int hy = 0, hx = 0;

    if (t < RIPPLE_HALO)
    {
      int x, y;

      if (t < 2 * RIPPLE_TX)
      {
        bool const below = t >= RIPPLE_TX;
        hx = lx + 1;
        hy = below ? RIPPLE_TY + 1 : 0;
        x = x0 + lx;
        y = (y0 + (below ? RIPPLE_TY : -1)) & (R - 1);
      }
      else
      {
        bool const right = t >= 2 * RIPPLE_TX + RIPPLE_TY;
        hy = ((t - 2 * RIPPLE_TX) & (RIPPLE_TY - 1)) + 1;
        hx = right ? RIPPLE_TX + 1 : 0;
        x = (x0 + (right ? RIPPLE_TX : -1)) & (R - 1);
        y = y0 + hy - 1;
      }

      int const cell = y * R + x;

      halo = buf_load_f32(rin, cell * (int)sizeof(float2), 0);
      hsrc = FIRST ? (int)buf_load_u32(rsrc, cell * (int)sizeof(int), 0) : 0;
    }

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
      tile[ly + RIPPLE_ROWSTEP * s + 1][lx + 1] = ripple_height(body[s].x, bsrc[s], FIRST);

    if (t < RIPPLE_HALO)
      tile[hy][hx] = ripple_height(halo, hsrc, FIRST);

    __syncthreads();

    // window coordinates of this thread's column, and the sponge table's last entry
    int const wx = ripple_wrap(x0 + lx - a.g.ox, R);

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const r = ly + RIPPLE_ROWSTEP * s + 1;
      int const my = y0 + r - 1;
      int const wy = ripple_wrap(my - a.g.oy, R);

      float const e = tile[r][lx + 1];
      float const eL = wx == 0 ? 0.0f : tile[r][lx];
      float const eR = wx == R - 1 ? 0.0f : tile[r][lx + 2];
      float const eD = wy == 0 ? 0.0f : tile[r - 1][lx + 1];
      float const eU = wy == R - 1 ? 0.0f : tile[r + 1][lx + 1];

      float const f = a.f[ripple_sponge(wx, wy, R, a.B)];

      RippleCell const c = ripple_update(e, body[s].y, eL, eR, eD, eU, a.h, a.c2s2, f);

      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ c.eta, c.rate }, rout, (my * R + x0 + lx) * (int)sizeof(float2), 0);
    }
  }

  inline hipError_t launch_ripple_step(RippleStepArgs &a, bool first, hipStream_t stream)
  {
    void *args[] = { &a };

    void const *kernel = first ? reinterpret_cast<void const*>(&ocean_ripple_step_kernel<true>) : reinterpret_cast<void const*>(&ocean_ripple_step_kernel<false>);

    return hipLaunchKernel(kernel, dim3((unsigned)(a.g.R / RIPPLE_TX), (unsigned)(a.g.R / RIPPLE_TY)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // The window moved from (oldx, oldy) to g's origin: every memory cell whose world cell changed -- it entered -- becomes water at rest,
  // in both state buffers and in src.  One thread per cell, whole rows per wave; a cell that stayed is not touched
  struct RippleScrollArgs
  {
    float2 *state[2];
    int *src;
    RippleGrid g;           // the NEW origin
    int oldx, oldy;
  };

  // the world coordinate in [o, o + R) that memory coordinate m holds
  __device__ __forceinline__ int ripple_world(int m, int o, int R)
  {
    return o + ripple_wrap(m - o, R);
  }

  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_scroll_kernel(RippleScrollArgs a)
  {
    int const R = a.g.R;
    int const mx = (int)blockIdx.x * RIPPLE_TX + ((int)threadIdx.x & (RIPPLE_TX - 1));
    int const my = (int)blockIdx.y * RIPPLE_ROWSTEP + (int)threadIdx.x / RIPPLE_TX;

    bool const entered = ripple_world(mx, a.g.ox, R) != ripple_world(mx, a.oldx, R) || ripple_world(my, a.g.oy, R) != ripple_world(my, a.oldy, R);

    if (!entered)
      return;

    size_t const cells = (size_t)R * R;
    int const cell = my * R + mx;

    buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ 0.0f, 0.0f }, make_rsrc(a.state[0], cells * sizeof(float2)), cell * (int)sizeof(float2), 0);
    buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ 0.0f, 0.0f }, make_rsrc(a.state[1], cells * sizeof(float2)), cell * (int)sizeof(float2), 0);
    buf_store_f32_aux<RIPPLE_STORE_AUX>(0.0f, make_rsrc(a.src, cells * sizeof(int)), cell * (int)sizeof(int), 0);
  }

  inline hipError_t launch_ripple_scroll(RippleScrollArgs &a, hipStream_t stream)
  {
    void *args[] = { &a };

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_scroll_kernel), dim3((unsigned)(a.g.R / RIPPLE_TX), (unsigned)(a.g.R / RIPPLE_ROWSTEP)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // a quantum into the src plane: a vector atomic on global memory.  ripple_splat hands over only indices inside the plane
  struct RippleDeposit
  {
    int *src;

    __device__ __forceinline__ void operator()(int index, int q) const { atomicAdd(src + index, q); }
  };

  // impulses: one thread per 16-byte record (x, y, V, 0)
  struct RippleImpulseArgs
  {
    float4 const *impulses;
    int *src;
    RippleGrid g;
    int count;
  };

  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_impulse_kernel(RippleImpulseArgs a)
  {
    int const i = (int)blockIdx.x * RIPPLE_THREADS + (int)threadIdx.x;

    if (i >= a.count)
      return;

    float4 const r = buf_load_f32x4_aux<0>(make_rsrc(a.impulses, (size_t)a.count * sizeof(float4)), i * (int)sizeof(float4), 0);

    ripple_splat(a.g, r.x, r.y, r.z, RippleDeposit{ a.src });
  }

  inline hipError_t launch_ripple_impulses(RippleImpulseArgs &a, hipStream_t stream)
  {
    void *args[] = { &a };

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_impulse_kernel), dim3((unsigned)(((size_t)a.count + RIPPLE_THREADS - 1) / RIPPLE_THREADS)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // samples: one thread per point, a 16-byte record each
  struct RippleSampleArgs
  {
    float2 const *state;
    float2 const *points;
    float4 *samples;
    RippleGrid g;
    int count;
  };

  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_sample_kernel(RippleSampleArgs a)
  {
    int const i = (int)blockIdx.x * RIPPLE_THREADS + (int)threadIdx.x;

    if (i >= a.count)
      return;

    __amdgpu_buffer_rsrc_t const rstate = make_rsrc(a.state, (size_t)a.g.R * a.g.R * sizeof(float2));

    float2 const p = buf_load_f32x2(make_rsrc(a.points, (size_t)a.count * sizeof(float2)), i * (int)sizeof(float2), 0);

    RippleSample const s = ripple_sample(a.g, p.x, p.y, [&](int index)
    {
      float2 const c = buf_load_f32x2(rstate, index * (int)sizeof(float2), 0);

      return RippleCell{ c.x, c.y };
    });

    buf_store_f32x4_aux<0>(make_float4(s.eta, s.dx, s.dy, s.rate), make_rsrc(a.samples, (size_t)a.count * sizeof(float4)), i * (int)sizeof(float4), 0);
  }

  inline hipError_t launch_ripple_samples(RippleSampleArgs &a, hipStream_t stream)
  {
    void *args[] = { &a };

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_sample_kernel), dim3((unsigned)(((size_t)a.count + RIPPLE_THREADS - 1) / RIPPLE_THREADS)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // the wake: body drag's walk (body_each_probe) and velocity record with wake_terms; the record has buoyancy's shape
  struct RippleWakeArgs
  {
    DragArgs d;
    int *src;
    RippleGrid g;
    float dt;
  };

  template<int LAYOUT>
  __global__ void __launch_bounds__(BODY_THREADS) ocean_ripple_wake_kernel(RippleWakeArgs a)
  {
    body_each_probe(a.d.b.bodies, a.d.b.probes, a.d.b.records, a.d.b.nbodies, a.d.b.nprobes, [&](int body, datum_ocean_body const &B, bool &bad)
    {
      datum_ocean_body_motion const M = a.d.motions[body];

      bad = bad || drag_motion_bad(M);

      return [&a, &B, M](BodyWorld const &w, float weight)
      {
        float2 const q = make_float2(w.x, w.y);

        QueryRecord const r = query_velocity<LAYOUT>(a.d.b.q, query_solve<LAYOUT>(a.d.b.q, q), q, a.d.vel);

        float const rec[DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS] = { r.v.x, r.v.y, r.v.z, r.v.w, r.m.x, r.m.y, r.m.z, r.m.w };

        return wake_terms(B, M, w, weight, rec, a.dt, [&a](float x, float y, float V) { return ripple_splat(a.g, x, y, V, RippleDeposit{ a.src }); });
      };
    });
  }

  inline void const *wake_kernel_for(int N)
  {
    switch(gen_layout(N))
    {
      case GEN_PLAIN: return reinterpret_cast<void const*>(&ocean_ripple_wake_kernel<GEN_PLAIN>);
      default: return reinterpret_cast<void const*>(&ocean_ripple_wake_kernel<GEN_BANDED>);
    }
  }

  // a.d as launch_body_drag wants it, src, g and dt filled in; a.d.b.nbodies > 0
  inline hipError_t launch_ripple_wake(RippleWakeArgs &a, hipStream_t stream)
  {
    query_frame(a.d.b.q);

    void *args[] = { &a };

    return hipLaunchKernel(wake_kernel_for(a.d.b.q.N), dim3((unsigned)(((size_t)a.d.b.nbodies + BODY_WAVES - 1) / BODY_WAVES)), dim3(BODY_THREADS), args, 0, stream);
  }
}
