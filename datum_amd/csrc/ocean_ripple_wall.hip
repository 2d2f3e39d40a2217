// ocean_ripple_wall.hip -- ripple walls (include/datum_ocean_hip.h: "ripple walls"): an R x R byte plane on the layer's torus, 1 where a
// wall record covers the cell's centre, and the two sub-steps that reflect off it.  The arithmetic is ocean_ripple_wall.h's (a CPU walks
// the same functions); this file is how the cells reach it.
//
// ocean_ripple_wall_raster_kernel: one thread per memory cell, whole memory rows per wave, the WHOLE plane on every launch (the plane is a
// function of the list and the world cell, so a rebuild gives the bytes that writing only the entered cells would).  The records are read
// with a wave-uniform index ahead of every store (scalar loads); the byte, and with `zero` the (+0, +0) of a wall cell in both state
// buffers, go through buffer resources over exactly their planes, written through.
//
// ocean_ripple_step_walls_kernel and ocean_ripple_deep_step_walls_kernel, one sub-step each, are ocean_ripple_step_kernel and
// ocean_ripple_deep_step_kernel restated with the plane -- those two are not touched and keep their instructions:
//   * the same 256 threads over a 64 x 16 tile aligned in memory coordinates, the same halo, rates in registers, write-through, resources;
//   * the wall flags of the tile and its halo are staged beside the heights as a second image of dwords with the heights' own pitch: a
//     wave reads a flag as it reads a height, 64 consecutive dwords, so NO CONFLICT IS EXPECTED by the same argument (the conflict counter
//     was not read).  A byte image would put four lanes on one dword of a bank;
//   * WAVE needs the four neighbours' flags at the update (ripple_wall_neighbour) and the cell's own at the store (ripple_wall_pin);
//   * DEEP needs the flag where the image is filled (ripple_wall_height: a wall cell is 0 in the convolution) and at the store;
//   * a walled sub-step reads one byte per cell and halo cell more than its parent.
// No scratch (make resource-usage).

#pragma once

#include "ocean_ripple_wall.h"
#include "ocean_ripple_deep.hip"

namespace ocean
{
  __device__ __forceinline__ unsigned int buf_load_u8(__amdgpu_buffer_rsrc_t r, int voffset, int soffset)
  {
    return __builtin_amdgcn_raw_buffer_load_b8(r, voffset, soffset, 0);
  }

  template<int AUX>
  __device__ __forceinline__ void buf_store_u8_aux(unsigned int v, __amdgpu_buffer_rsrc_t r, int voffset, int soffset)
  {
    __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, r, voffset + soffset, 0, AUX);
  }

  struct RippleWallRasterArgs
  {
    unsigned char *wall;                        // [R][R], memory order
    float2 *state[2];
    datum_ocean_ripple_wall const *walls;       // [count], device
    int count;
    int zero;                                   // wall cells become (+0, +0) in both state buffers (datum_ocean_set_ripple_walls)
    RippleGrid g;
    float s;                                    // the cell side
  };

  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_wall_raster_kernel(RippleWallRasterArgs a)
  {
    int const R = a.g.R;
    int const mx = (int)blockIdx.x * RIPPLE_TX + ((int)threadIdx.x & (RIPPLE_TX - 1));
    int const my = (int)blockIdx.y * RIPPLE_ROWSTEP + (int)threadIdx.x / RIPPLE_TX;

    unsigned int const wall = ripple_wall_cell(a.walls, a.count, ripple_world(mx, a.g.ox, R), ripple_world(my, a.g.oy, R), a.s);

    size_t const cells = (size_t)R * R;
    int const cell = my * R + mx;

    buf_store_u8_aux<RIPPLE_STORE_AUX>(wall, make_rsrc(a.wall, cells), cell, 0);

    if (a.zero && wall)
    {
      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ 0.0f, 0.0f }, make_rsrc(a.state[0], cells * sizeof(float2)), cell * (int)sizeof(float2), 0);
      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ 0.0f, 0.0f }, make_rsrc(a.state[1], cells * sizeof(float2)), cell * (int)sizeof(float2), 0);
    }
  }

  inline hipError_t launch_ripple_wall_raster(RippleWallRasterArgs &a, hipStream_t stream)
  {
    void *args[] = { &a };

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_wall_raster_kernel), dim3((unsigned)(a.g.R / RIPPLE_TX), (unsigned)(a.g.R / RIPPLE_ROWSTEP)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // the WAVE sub-step with walls: ocean_ripple_step_kernel's form
  struct RippleWallStepArgs
  {
    RippleStepArgs s;
    unsigned char const *wall;
  };

  template<bool FIRST>
  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_step_walls_kernel(RippleWallStepArgs a)
  {
    __shared__ float tile[RIPPLE_TY + 2][RIPPLE_LX];
    __shared__ unsigned int flag[RIPPLE_TY + 2][RIPPLE_LX];

    int const R = a.s.g.R;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * RIPPLE_TX;
    int const y0 = (int)blockIdx.y * RIPPLE_TY;

    size_t const cells = (size_t)R * R;

    __amdgpu_buffer_rsrc_t const rin = make_rsrc(a.s.in, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rout = make_rsrc(a.s.out, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rsrc = make_rsrc(a.s.src, cells * sizeof(int));
    __amdgpu_buffer_rsrc_t const rwall = make_rsrc(a.wall, cells);

    int const lx = t & (RIPPLE_TX - 1);
    int const ly = t / RIPPLE_TX;

    // body: memory cell (x0 + lx, y0 + ly + 4 s)
    float2 body[RIPPLE_PER_THREAD];
    int bsrc[RIPPLE_PER_THREAD];
    unsigned int bwall[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const cell = (y0 + ly + RIPPLE_ROWSTEP * s) * R + x0 + lx;

      body[s] = buf_load_f32x2(rin, cell * (int)sizeof(float2), 0);
      bsrc[s] = FIRST ? (int)buf_load_u32(rsrc, cell * (int)sizeof(int), 0) : 0;
      bwall[s] = buf_load_u8(rwall, cell, 0);
    }

    // halo: the rows above and below, then the columns left and right, wrapped on the torus; the height and the flag
    float halo = 0.0f;
    int hsrc = 0;
    unsigned int hwall = 0;
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
      hwall = buf_load_u8(rwall, cell, 0);
    }

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      tile[ly + RIPPLE_ROWSTEP * s + 1][lx + 1] = ripple_height(body[s].x, bsrc[s], FIRST);
      flag[ly + RIPPLE_ROWSTEP * s + 1][lx + 1] = bwall[s];
    }

    if (t < RIPPLE_HALO)
    {
      tile[hy][hx] = ripple_height(halo, hsrc, FIRST);
      flag[hy][hx] = hwall;
    }

    __syncthreads();

    int const wx = ripple_wrap(x0 + lx - a.s.g.ox, R);

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const r = ly + RIPPLE_ROWSTEP * s + 1;
      int const my = y0 + r - 1;
      int const wy = ripple_wrap(my - a.s.g.oy, R);

      float const e = tile[r][lx + 1];
      float const eL = ripple_wall_neighbour(wx != 0, flag[r][lx] != 0, e, tile[r][lx]);
      float const eR = ripple_wall_neighbour(wx != R - 1, flag[r][lx + 2] != 0, e, tile[r][lx + 2]);
      float const eD = ripple_wall_neighbour(wy != 0, flag[r - 1][lx + 1] != 0, e, tile[r - 1][lx + 1]);
      float const eU = ripple_wall_neighbour(wy != R - 1, flag[r + 1][lx + 1] != 0, e, tile[r + 1][lx + 1]);

      float const f = a.s.f[ripple_sponge(wx, wy, R, a.s.B)];

      RippleCell const c = ripple_wall_pin(bwall[s] != 0, ripple_update(e, body[s].y, eL, eR, eD, eU, a.s.h, a.s.c2s2, f));

      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ c.eta, c.rate }, rout, (my * R + x0 + lx) * (int)sizeof(float2), 0);
    }
  }

  inline hipError_t launch_ripple_step_walls(RippleWallStepArgs &a, bool first, hipStream_t stream)
  {
    void *args[] = { &a };

    void const *kernel = first ? reinterpret_cast<void const*>(&ocean_ripple_step_walls_kernel<true>) : reinterpret_cast<void const*>(&ocean_ripple_step_walls_kernel<false>);

    return hipLaunchKernel(kernel, dim3((unsigned)(a.s.g.R / RIPPLE_TX), (unsigned)(a.s.g.R / RIPPLE_TY)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // the DEEP sub-step with walls: ocean_ripple_deep_step_kernel's form
  struct RippleWallDeepStepArgs
  {
    RippleDeepStepArgs d;
    unsigned char const *wall;
  };

  template<bool FIRST>
  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_deep_step_walls_kernel(RippleWallDeepStepArgs a)
  {
    __shared__ float tile[RIPPLE_DEEP_LY][RIPPLE_DEEP_LX];
    __shared__ unsigned int flag[RIPPLE_DEEP_LY][RIPPLE_DEEP_LX];

    int const R = a.d.s.g.R;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * RIPPLE_TX;
    int const y0 = (int)blockIdx.y * RIPPLE_TY;

    size_t const cells = (size_t)R * R;

    __amdgpu_buffer_rsrc_t const rin = make_rsrc(a.d.s.in, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rout = make_rsrc(a.d.s.out, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rsrc = make_rsrc(a.d.s.src, cells * sizeof(int));
    __amdgpu_buffer_rsrc_t const rwall = make_rsrc(a.wall, cells);

    int const lx = t & (RIPPLE_TX - 1);
    int const wave = __builtin_amdgcn_readfirstlane(t / RIPPLE_TX);
    int const row0 = wave * RIPPLE_PER_THREAD;

    // the image: cell k of 2128 is image row k / 76, column k % 76, memory cell (x0 - 6 + column, y0 - 6 + row) wrapped
    float img[RIPPLE_DEEP_ROUNDS];
    int isrc[RIPPLE_DEEP_ROUNDS];
    unsigned int iwall[RIPPLE_DEEP_ROUNDS];

    #pragma unroll
    for(int i = 0; i < RIPPLE_DEEP_ROUNDS; ++i)
    {
      int const k = t + RIPPLE_THREADS * i;

      img[i] = 0.0f;
      isrc[i] = 0;
      iwall[i] = 0;

      if (k < RIPPLE_DEEP_IMAGE)
      {
        int const iy = k / RIPPLE_DEEP_LX, ix = k - iy * RIPPLE_DEEP_LX;
        int const cell = ripple_wrap(y0 - RIPPLE_DEEP_P + iy, R) * R + ripple_wrap(x0 - RIPPLE_DEEP_P + ix, R);

        img[i] = buf_load_f32(rin, cell * (int)sizeof(float2), 0);
        isrc[i] = FIRST ? (int)buf_load_u32(rsrc, cell * (int)sizeof(int), 0) : 0;
        iwall[i] = buf_load_u8(rwall, cell, 0);
      }
    }

    float rate[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
      rate[s] = buf_load_f32(rin, ((y0 + row0 + s) * R + x0 + lx) * (int)sizeof(float2), (int)sizeof(float));

    #pragma unroll
    for(int i = 0; i < RIPPLE_DEEP_ROUNDS; ++i)
    {
      int const k = t + RIPPLE_THREADS * i;

      if (k < RIPPLE_DEEP_IMAGE)
      {
        (&tile[0][0])[k] = ripple_wall_height(iwall[i] != 0, img[i], isrc[i], FIRST);
        (&flag[0][0])[k] = iwall[i];
      }
    }

    __syncthreads();

    int const wx = ripple_wrap(x0 + lx - a.d.s.g.ox, R);

    int wy[RIPPLE_PER_THREAD];
    float acc[RIPPLE_PER_THREAD];
    float own[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      wy[s] = ripple_wrap(y0 + row0 + s - a.d.s.g.oy, R);
      acc[s] = 0.0f;
      own[s] = 0.0f;
    }

    // image row row0 + r is the row dj = r - 6 - s of the wave's cell s
    #pragma unroll
    for(int r = 0; r < RIPPLE_DEEP_WAVE_ROWS; ++r)
    {
      float e[RIPPLE_DEEP_SPAN];

      #pragma unroll
      for(int i = 0; i < RIPPLE_DEEP_SPAN; ++i)
      {
        float const v = tile[row0 + r][lx + i];

        e[i] = (unsigned int)(wx + i - RIPPLE_DEEP_P) < (unsigned int)R ? v : 0.0f;
      }

      #pragma unroll
      for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
      {
        int const dj = r - RIPPLE_DEEP_P - s;

        if (dj < -RIPPLE_DEEP_P || dj > RIPPLE_DEEP_P)
          continue;

        if (dj == 0)
          own[s] = e[RIPPLE_DEEP_P];

        if ((unsigned int)(wy[s] + dj) < (unsigned int)R)
          acc[s] = ripple_deep_row(acc[s], a.d.G + RIPPLE_DEEP_Q * ripple_deep_abs(dj), [&](int di) { return e[di + RIPPLE_DEEP_P]; });
      }
    }

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const my = y0 + row0 + s;

      float const f = a.d.s.f[ripple_sponge(wx, wy[s], R, a.d.s.B)];

      bool const wall = flag[row0 + s + RIPPLE_DEEP_P][lx + RIPPLE_DEEP_P] != 0;

      RippleCell const c = ripple_wall_pin(wall, ripple_deep_update(own[s], rate[s], acc[s], a.d.s.h, a.d.gs, f));

      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ c.eta, c.rate }, rout, (my * R + x0 + lx) * (int)sizeof(float2), 0);
    }
  }

  inline hipError_t launch_ripple_deep_step_walls(RippleWallDeepStepArgs &a, bool first, hipStream_t stream)
  {
    void *args[] = { &a };

    void const *kernel = first ? reinterpret_cast<void const*>(&ocean_ripple_deep_step_walls_kernel<true>) : reinterpret_cast<void const*>(&ocean_ripple_deep_step_walls_kernel<false>);

    return hipLaunchKernel(kernel, dim3((unsigned)(a.d.s.g.R / RIPPLE_TX), (unsigned)(a.d.s.g.R / RIPPLE_TY)), dim3(RIPPLE_THREADS), args, 0, stream);
  }
}
