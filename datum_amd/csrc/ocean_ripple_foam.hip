// ocean_ripple_foam.hip -- wake foam (include/datum_ocean_hip.h: "wake foam"): an R x R coverage plane beside the ripple layer's state, on
// the layer's torus, updated from the layer's current state by an explicit call.  The arithmetic is ocean_ripple_foam.h's (a CPU walks
// the same functions); this file is how the cells reach it.
//
// ocean_ripple_foam_kernel, one update, in the form of ocean_ripple_step_kernel (ocean_ripple.hip), whose constants it uses:
//   * one 256-thread workgroup per 64 x 16 tile aligned in MEMORY coordinates, whatever the origin; window coordinates are derived per
//     cell, (mx - ox) mod R: a wave loads whole 512-byte rows of the state and loads and stores whole 256-byte rows of the plane;
//   * the tile's heights and a one-cell halo (64 above, 64 below, 16 left, 16 right, wrapped; no corners, the central differences have
//     none) are staged in LDS in rows of 66 floats, 4752 bytes; the rate and the old coverage stay in registers.  The staging is the
//     step's, restated: the step's device code keeps its instructions that way;
//   * a neighbour outside the WINDOW is 0 whatever memory holds there (select on the window coordinate);
//   * a cell's coverage is read and written by the same thread and by no other: the plane is updated in place, written through (sc0 sc1)
//     as the state is;
//   * every access goes through a buffer resource over exactly its plane: no index can reach outside it.
// By design 8 bytes read of the state, 4 read and 4 written of the plane per cell, and the halo: the step's bytes.
// No scratch (make resource-usage).

#pragma once

#include "ocean_ripple_foam.h"
#include "ocean_ripple.hip"

namespace ocean
{
  struct RippleFoamArgs
  {
    float2 const *state;    // [R][R] (eta, rate), memory order: the layer's current buffer
    float *foam;            // [R][R] coverage, memory order
    RippleGrid g;
    RippleFoamParams p;
  };

  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_foam_kernel(RippleFoamArgs a)
  {
    __shared__ float tile[RIPPLE_TY + 2][RIPPLE_LX];

    int const R = a.g.R;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * RIPPLE_TX;
    int const y0 = (int)blockIdx.y * RIPPLE_TY;

    size_t const cells = (size_t)R * R;

    __amdgpu_buffer_rsrc_t const rstate = make_rsrc(a.state, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rfoam = make_rsrc(a.foam, cells * sizeof(float));

    int const lx = t & (RIPPLE_TX - 1);
    int const ly = t / RIPPLE_TX;

    // body: memory cell (x0 + lx, y0 + ly + 4 s)
    float2 body[RIPPLE_PER_THREAD];
    float old[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const cell = (y0 + ly + RIPPLE_ROWSTEP * s) * R + x0 + lx;

      body[s] = buf_load_f32x2(rstate, cell * (int)sizeof(float2), 0);
      old[s] = buf_load_f32(rfoam, cell * (int)sizeof(float), 0);
    }

    // halo: the rows above and below, then the columns left and right, wrapped on the torus; only the height is needed
    float halo = 0.0f;
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

      halo = buf_load_f32(rstate, (y * R + x) * (int)sizeof(float2), 0);
    }

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
      tile[ly + RIPPLE_ROWSTEP * s + 1][lx + 1] = body[s].x;

    if (t < RIPPLE_HALO)
      tile[hy][hx] = halo;

    __syncthreads();

    // window coordinates of this thread's column
    int const wx = ripple_wrap(x0 + lx - a.g.ox, R);

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const r = ly + RIPPLE_ROWSTEP * s + 1;
      int const my = y0 + r - 1;
      int const wy = ripple_wrap(my - a.g.oy, R);

      float const eL = wx == 0 ? 0.0f : tile[r][lx];
      float const eR = wx == R - 1 ? 0.0f : tile[r][lx + 2];
      float const eD = wy == 0 ? 0.0f : tile[r - 1][lx + 1];
      float const eU = wy == R - 1 ? 0.0f : tile[r + 1][lx + 1];

      float const f = ripple_foam_update(body[s].y, eL, eR, eD, eU, old[s], a.p);

      buf_store_f32_aux<RIPPLE_STORE_AUX>(f, rfoam, (my * R + x0 + lx) * (int)sizeof(float), 0);
    }
  }

  inline hipError_t launch_ripple_foam(RippleFoamArgs &a, hipStream_t stream)
  {
    void *args[] = { &a };

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_foam_kernel), dim3((unsigned)(a.g.R / RIPPLE_TX), (unsigned)(a.g.R / RIPPLE_TY)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // The window moved from (oldx, oldy) to g's origin: every memory cell of the plane whose world cell changed -- it entered -- holds no
  // foam.  ocean_ripple_scroll_kernel's test and walk, over the one float plane; a cell that stayed is not touched
  struct RippleFoamScrollArgs
  {
    float *foam;
    RippleGrid g;           // the NEW origin
    int oldx, oldy;
  };

  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_foam_scroll_kernel(RippleFoamScrollArgs a)
  {
    int const R = a.g.R;
    int const mx = (int)blockIdx.x * RIPPLE_TX + ((int)threadIdx.x & (RIPPLE_TX - 1));
    int const my = (int)blockIdx.y * RIPPLE_ROWSTEP + (int)threadIdx.x / RIPPLE_TX;

    bool const entered = ripple_world(mx, a.g.ox, R) != ripple_world(mx, a.oldx, R) || ripple_world(my, a.g.oy, R) != ripple_world(my, a.oldy, R);

    if (!entered)
      return;

    buf_store_f32_aux<RIPPLE_STORE_AUX>(0.0f, make_rsrc(a.foam, (size_t)R * R * sizeof(float)), (my * R + mx) * (int)sizeof(float), 0);
  }

  inline hipError_t launch_ripple_foam_scroll(RippleFoamScrollArgs &a, hipStream_t stream)
  {
    void *args[] = { &a };

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_foam_scroll_kernel), dim3((unsigned)(a.g.R / RIPPLE_TX), (unsigned)(a.g.R / RIPPLE_ROWSTEP)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // samples: one thread per 8-byte point, one float each
  struct RippleFoamSampleArgs
  {
    float const *foam;
    float2 const *points;
    float *samples;
    RippleGrid g;
    int count;
  };

  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_foam_sample_kernel(RippleFoamSampleArgs a)
  {
    int const i = (int)blockIdx.x * RIPPLE_THREADS + (int)threadIdx.x;

    if (i >= a.count)
      return;

    __amdgpu_buffer_rsrc_t const rfoam = make_rsrc(a.foam, (size_t)a.g.R * a.g.R * sizeof(float));

    float2 const p = buf_load_f32x2(make_rsrc(a.points, (size_t)a.count * sizeof(float2)), i * (int)sizeof(float2), 0);

    float const f = ripple_foam_sample(a.g, p.x, p.y, [&](int index) { return buf_load_f32(rfoam, index * (int)sizeof(float), 0); });

    buf_store_f32_aux<0>(f, make_rsrc(a.samples, (size_t)a.count * sizeof(float)), i * (int)sizeof(float), 0);
  }

  inline hipError_t launch_ripple_foam_samples(RippleFoamSampleArgs &a, hipStream_t stream)
  {
    void *args[] = { &a };

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_foam_sample_kernel), dim3((unsigned)(((size_t)a.count + RIPPLE_THREADS - 1) / RIPPLE_THREADS)), dim3(RIPPLE_THREADS), args, 0, stream);
  }
}
