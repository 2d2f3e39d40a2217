// ocean_ripple_bed.hip -- the ripple bed (include/datum_ocean_hip.h: "ripple bed"): still-water depth under the ripple layer as two planes on
// the layer's torus -- R x R floats of effective depth, +0 where the cell is solid, and R x R bytes of surf level -- and the WAVE sub-step
// with a per-face coefficient that shoals, refracts and breaks on it.  The arithmetic is ocean_ripple_bed.h's (a CPU walks the same
// functions); this file is how the cells reach it.
//
// ocean_ripple_bed_raster_kernel: ocean_ripple_wall_raster_kernel's form -- one thread per memory cell, whole memory rows per wave, the
// WHOLE of both planes on every launch (they are a function of the map, the parameters, the wall plane and the world cell, so a rebuild
// gives the values that writing only the entered cells would).  The map is read through a buffer resource over exactly its bytes, four
// texels per cell that lies on it; the wall byte is read while walls are on; d, q and with `zero` the (+0, +0) of a solid cell in both
// state buffers are written through.
//
// ocean_ripple_bed_step_kernel, one sub-step, is ocean_ripple_step_walls_kernel restated with the depths -- that kernel and its parents
// are not touched and keep their instructions:
//   * the same 256 threads over a 64 x 16 tile aligned in memory coordinates, the same halo, rates in registers, write-through, a
//     resource per plane;
//   * the depths of the tile and its halo are staged beside the heights as a second image of floats with the heights' own pitch: a wave
//     reads a depth as it reads a height, 64 consecutive dwords, so NO CONFLICT IS EXPECTED by the parent's argument (the conflict
//     counter was not read);
//   * the surf level is read once per cell from memory, a byte; no neighbour's is needed, so it has no halo and no image;
//   * a sub-step reads 8 + 4 + 1 bytes per cell and 4 + 4 per halo cell (src besides, in a first sub-step), and writes the parent's 8.
// Walls are in d already: the kernel runs whether walls are on or off.  No scratch (make resource-usage).

#pragma once

#include "ocean_ripple_bed.h"
#include "ocean_ripple_wall.hip"

namespace ocean
{
  struct RippleBedRasterArgs
  {
    float *depth;                               // [R][R], memory order
    unsigned char *surf;                        // [R][R]
    float2 *state[2];
    float const *map;                           // [height][width], device
    unsigned char const *wall;                  // the wall plane, null while walls are off
    int zero;                                   // solid cells become (+0, +0) in both state buffers (datum_ocean_set_ripple_bed)
    RippleGrid g;
    float s;                                    // the cell side
    RippleBed b;
  };

  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_bed_raster_kernel(RippleBedRasterArgs a)
  {
    int const R = a.g.R;
    int const mx = (int)blockIdx.x * RIPPLE_TX + ((int)threadIdx.x & (RIPPLE_TX - 1));
    int const my = (int)blockIdx.y * RIPPLE_ROWSTEP + (int)threadIdx.x / RIPPLE_TX;

    size_t const cells = (size_t)R * R;
    int const cell = my * R + mx;

    __amdgpu_buffer_rsrc_t const rmap = make_rsrc(a.map, (size_t)a.b.width * a.b.height * sizeof(float));

    bool const wall = a.wall ? buf_load_u8(make_rsrc(a.wall, cells), cell, 0) != 0 : false;

    RippleBedCell const c = ripple_bed_cell(a.b, ripple_world(mx, a.g.ox, R), ripple_world(my, a.g.oy, R), a.s, wall, [&](int index) { return buf_load_f32(rmap, index * (int)sizeof(float), 0); });

    buf_store_f32_aux<RIPPLE_STORE_AUX>(c.d, make_rsrc(a.depth, cells * sizeof(float)), cell * (int)sizeof(float), 0);
    buf_store_u8_aux<RIPPLE_STORE_AUX>(c.q, make_rsrc(a.surf, cells), cell, 0);

    if (a.zero && c.d == 0.0f)
    {
      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ 0.0f, 0.0f }, make_rsrc(a.state[0], cells * sizeof(float2)), cell * (int)sizeof(float2), 0);
      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ 0.0f, 0.0f }, make_rsrc(a.state[1], cells * sizeof(float2)), cell * (int)sizeof(float2), 0);
    }
  }

  inline hipError_t launch_ripple_bed_raster(RippleBedRasterArgs &a, hipStream_t stream)
  {
    void *args[] = { &a };

    return hipLaunchKernel(reinterpret_cast<void const*>(&ocean_ripple_bed_raster_kernel), dim3((unsigned)(a.g.R / RIPPLE_TX), (unsigned)(a.g.R / RIPPLE_ROWSTEP)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // the WAVE sub-step over a bed: ocean_ripple_step_walls_kernel's form.  s.c2s2 is not read
  struct RippleBedStepArgs
  {
    RippleStepArgs s;
    float const *depth;
    unsigned char const *surf;
    float gs2;                                  // g / s^2, rounded once from double
    float fsurf[RIPPLE_SURF_LEVELS + 1];        // the surf table for this h
  };

  template<bool FIRST>
  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_bed_step_kernel(RippleBedStepArgs a)
  {
    __shared__ float tile[RIPPLE_TY + 2][RIPPLE_LX];
    __shared__ float bed[RIPPLE_TY + 2][RIPPLE_LX];

    int const R = a.s.g.R;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * RIPPLE_TX;
    int const y0 = (int)blockIdx.y * RIPPLE_TY;

    size_t const cells = (size_t)R * R;

    __amdgpu_buffer_rsrc_t const rin = make_rsrc(a.s.in, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rout = make_rsrc(a.s.out, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rsrc = make_rsrc(a.s.src, cells * sizeof(int));
    __amdgpu_buffer_rsrc_t const rbed = make_rsrc(a.depth, cells * sizeof(float));
    __amdgpu_buffer_rsrc_t const rsurf = make_rsrc(a.surf, cells);

    int const lx = t & (RIPPLE_TX - 1);
    int const ly = t / RIPPLE_TX;

    // body: memory cell (x0 + lx, y0 + ly + 4 s)
    float2 body[RIPPLE_PER_THREAD];
    int bsrc[RIPPLE_PER_THREAD];
    float bbed[RIPPLE_PER_THREAD];
    unsigned int bsurf[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const cell = (y0 + ly + RIPPLE_ROWSTEP * s) * R + x0 + lx;

      body[s] = buf_load_f32x2(rin, cell * (int)sizeof(float2), 0);
      bsrc[s] = FIRST ? (int)buf_load_u32(rsrc, cell * (int)sizeof(int), 0) : 0;
      bbed[s] = buf_load_f32(rbed, cell * (int)sizeof(float), 0);
      bsurf[s] = buf_load_u8(rsurf, cell, 0);
    }

    // halo: the rows above and below, then the columns left and right, wrapped on the torus; the height and the depth
    float halo = 0.0f;
    int hsrc = 0;
    float hbed = 0.0f;
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
      hbed = buf_load_f32(rbed, cell * (int)sizeof(float), 0);
    }

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      tile[ly + RIPPLE_ROWSTEP * s + 1][lx + 1] = ripple_height(body[s].x, bsrc[s], FIRST);
      bed[ly + RIPPLE_ROWSTEP * s + 1][lx + 1] = bbed[s];
    }

    if (t < RIPPLE_HALO)
    {
      tile[hy][hx] = ripple_height(halo, hsrc, FIRST);
      bed[hy][hx] = hbed;
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
      float const dc = bbed[s];

      float const tL = ripple_bed_flux(wx != 0, dc, bed[r][lx], e, tile[r][lx]);
      float const tR = ripple_bed_flux(wx != R - 1, dc, bed[r][lx + 2], e, tile[r][lx + 2]);
      float const tD = ripple_bed_flux(wy != 0, dc, bed[r - 1][lx + 1], e, tile[r - 1][lx + 1]);
      float const tU = ripple_bed_flux(wy != R - 1, dc, bed[r + 1][lx + 1], e, tile[r + 1][lx + 1]);

      // (a surf level above the table's end cannot come from the raster; the index is held to the table all the same)
      unsigned int const q = bsurf[s] < (unsigned int)RIPPLE_SURF_LEVELS ? bsurf[s] : (unsigned int)RIPPLE_SURF_LEVELS;

      RippleCell const c = ripple_bed_update(e, body[s].y, tL, tR, tD, tU, dc, a.s.h, a.gs2, a.s.f[ripple_sponge(wx, wy, R, a.s.B)], a.fsurf[q]);

      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ c.eta, c.rate }, rout, (my * R + x0 + lx) * (int)sizeof(float2), 0);
    }
  }

  inline hipError_t launch_ripple_bed_step(RippleBedStepArgs &a, bool first, hipStream_t stream)
  {
    void *args[] = { &a };

    void const *kernel = first ? reinterpret_cast<void const*>(&ocean_ripple_bed_step_kernel<true>) : reinterpret_cast<void const*>(&ocean_ripple_bed_step_kernel<false>);

    return hipLaunchKernel(kernel, dim3((unsigned)(a.s.g.R / RIPPLE_TX), (unsigned)(a.s.g.R / RIPPLE_TY)), dim3(RIPPLE_THREADS), args, 0, stream);
  }
}
