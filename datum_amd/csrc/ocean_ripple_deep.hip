// ocean_ripple_deep.hip -- the ripple layer's DEEP step (include/datum_ocean_hip.h: "dispersive ripples"): the sub-step whose restoring
// term is g sqrt(-Laplacian) eta, the operator a 13 x 13 convolution.  The arithmetic is ocean_ripple_deep.h's (a CPU walks the same
// functions); this file is how the cells reach it.
//
// ocean_ripple_deep_step_kernel, one sub-step, in the form of ocean_ripple_step_kernel:
//   * one 256-thread workgroup per 64 x 16 tile aligned in MEMORY coordinates; window coordinates are derived per cell, (mx - ox) mod R;
//   * the tile's heights and a six-cell halo, corners included, wrapped on the torus, are staged in LDS as floats, the first sub-step's
//     deposits already added: 28 x 76 x 4 = 8512 bytes, loaded in a loop of nine rounds (2128 cells, 256 threads).  The lanes of a wave
//     read consecutive floats of one row -- at the Makefile's flags 96 ds_read2_b32 (two neighbouring floats per lane) and 16 ds_read_b32
//     per lane, 208 floats.  Both are banked modulo 32 dwords, and consecutive lanes read consecutive dwords at either offset, so NO
//     CONFLICT IS EXPECTED at any pitch and the pitch is the image's own 76; the conflict counter was not read;
//   * a wave owns FOUR CONSECUTIVE rows of the tile, a lane one column of them: each of the 16 image rows a wave needs is read once, 13
//     floats per lane, and serves up to four cells -- 208 LDS reads for four cells, not 676.  Every cell still sums dj outer, di inner
//     from 0.0f: its accumulator meets the rows in rising dj and a row's cells in rising di (ripple_deep_row);
//   * a cell outside the WINDOW is 0 whatever memory holds there: a column by select on the lane's window coordinate, a row -- the same
//     for all of a wave -- by leaving the row's thirteen terms out, which adds nothing bit for bit (ocean_ripple_deep.h);
//   * the rate is the cell's own and stays in registers; the 49 weights come in the kernel arguments (scalar registers);
//   * the new state is written through (sc0 sc1), as the wave step's: the next sub-step's tile runs on any XCD;
//   * every access goes through a buffer resource over exactly the plane: no index can reach outside it.
// No scratch (make resource-usage).

#pragma once

#include "ocean_ripple_deep.h"
#include "ocean_ripple.hip"

namespace ocean
{
  constexpr int RIPPLE_DEEP_LX = RIPPLE_TX + 2 * RIPPLE_DEEP_P;                   // 76
  constexpr int RIPPLE_DEEP_LY = RIPPLE_TY + 2 * RIPPLE_DEEP_P;                   // 28
  constexpr int RIPPLE_DEEP_IMAGE = RIPPLE_DEEP_LX * RIPPLE_DEEP_LY;              // 2128 cells
  constexpr int RIPPLE_DEEP_ROUNDS = (RIPPLE_DEEP_IMAGE + RIPPLE_THREADS - 1) / RIPPLE_THREADS;   // 9
  constexpr int RIPPLE_DEEP_SPAN = 2 * RIPPLE_DEEP_P + 1;                         // 13
  constexpr int RIPPLE_DEEP_WAVE_ROWS = RIPPLE_PER_THREAD + 2 * RIPPLE_DEEP_P;    // 16 image rows serve a wave's four

  static_assert(RIPPLE_PER_THREAD * (RIPPLE_THREADS / RIPPLE_TX) == RIPPLE_TY, "a wave owns RIPPLE_PER_THREAD consecutive rows of the tile");

  struct RippleDeepStepArgs
  {
    RippleStepArgs s;       // in, out, src, the grid, B, h and the sponge table: the wave step's, c2s2 unused
    float gs;               // g / s
    float G[RIPPLE_DEEP_WEIGHTS];   // the quadrant table [l][k]
  };

  template<bool FIRST>
  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_deep_step_kernel(RippleDeepStepArgs a)
  {
    __shared__ float tile[RIPPLE_DEEP_LY][RIPPLE_DEEP_LX];

    int const R = a.s.g.R;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * RIPPLE_TX;
    int const y0 = (int)blockIdx.y * RIPPLE_TY;

    size_t const cells = (size_t)R * R;

    __amdgpu_buffer_rsrc_t const rin = make_rsrc(a.s.in, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rout = make_rsrc(a.s.out, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rsrc = make_rsrc(a.s.src, cells * sizeof(int));

    int const lx = t & (RIPPLE_TX - 1);
    int const wave = __builtin_amdgcn_readfirstlane(t / RIPPLE_TX);      // the same for all of a wave: its rows' tests are scalar
    int const row0 = wave * RIPPLE_PER_THREAD;                           // the wave's first row in the tile

    // the image: cell k of 2128 is image row k / 76, column k % 76, memory cell (x0 - 6 + column, y0 - 6 + row) wrapped
    float img[RIPPLE_DEEP_ROUNDS];
    int isrc[RIPPLE_DEEP_ROUNDS];

    #pragma unroll
    for(int i = 0; i < RIPPLE_DEEP_ROUNDS; ++i)
    {
      int const k = t + RIPPLE_THREADS * i;

      img[i] = 0.0f;
      isrc[i] = 0;

      if (k < RIPPLE_DEEP_IMAGE)
      {
        int const iy = k / RIPPLE_DEEP_LX, ix = k - iy * RIPPLE_DEEP_LX;
        int const cell = ripple_wrap(y0 - RIPPLE_DEEP_P + iy, R) * R + ripple_wrap(x0 - RIPPLE_DEEP_P + ix, R);

        img[i] = buf_load_f32(rin, cell * (int)sizeof(float2), 0);
        isrc[i] = FIRST ? (int)buf_load_u32(rsrc, cell * (int)sizeof(int), 0) : 0;
      }
    }

    // the rates of this lane's four cells: memory cell (x0 + lx, y0 + row0 + s)
    float rate[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
      rate[s] = buf_load_f32(rin, ((y0 + row0 + s) * R + x0 + lx) * (int)sizeof(float2), (int)sizeof(float));

    #pragma unroll
    for(int i = 0; i < RIPPLE_DEEP_ROUNDS; ++i)
    {
      int const k = t + RIPPLE_THREADS * i;

      if (k < RIPPLE_DEEP_IMAGE)
        (&tile[0][0])[k] = ripple_height(img[i], isrc[i], FIRST);
    }

    __syncthreads();

    // window coordinates: this lane's column, and the wave's four rows
    int const wx = ripple_wrap(x0 + lx - a.s.g.ox, R);

    int wy[RIPPLE_PER_THREAD];
    float acc[RIPPLE_PER_THREAD];
    float own[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      wy[s] = ripple_wrap(y0 + row0 + s - a.s.g.oy, R);
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
          acc[s] = ripple_deep_row(acc[s], a.G + RIPPLE_DEEP_Q * ripple_deep_abs(dj), [&](int di) { return e[di + RIPPLE_DEEP_P]; });
      }
    }

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const my = y0 + row0 + s;

      float const f = a.s.f[ripple_sponge(wx, wy[s], R, a.s.B)];

      RippleCell const c = ripple_deep_update(own[s], rate[s], acc[s], a.s.h, a.gs, f);

      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ c.eta, c.rate }, rout, (my * R + x0 + lx) * (int)sizeof(float2), 0);
    }
  }

  inline hipError_t launch_ripple_deep_step(RippleDeepStepArgs &a, bool first, hipStream_t stream)
  {
    void *args[] = { &a };

    void const *kernel = first ? reinterpret_cast<void const*>(&ocean_ripple_deep_step_kernel<true>) : reinterpret_cast<void const*>(&ocean_ripple_deep_step_kernel<false>);

    return hipLaunchKernel(kernel, dim3((unsigned)(a.s.g.R / RIPPLE_TX), (unsigned)(a.s.g.R / RIPPLE_TY)), dim3(RIPPLE_THREADS), args, 0, stream);
  }
}
