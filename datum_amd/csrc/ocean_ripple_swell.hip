// ocean_ripple_swell.hip -- ripple swell (include/datum_ocean_hip.h: "ripple swell"): the FFT swell as a source of the ripple layer at
// every solid face, so that the layer carries the reflection in front of a wall, the shadow behind it and the diffraction round its
// end.  One R x R float plane F on the layer's torus, and the two WAVE sub-steps that read it.  The arithmetic is ocean_ripple_swell.h's
// (a CPU walks the same functions); this file is how the cells reach it.
//
// ocean_ripple_swell_refresh_kernel, the plane's only writer, the WHOLE plane on every launch:
//   * the step kernels' 256 threads over a 64 x 16 tile aligned in memory coordinates, whole memory rows per wave, four rows a thread;
//   * the solid flags of the tile and its one-cell halo are staged in LDS as dwords with the heights' pitch, as the walled sub-step
//     stages its flags: the wall byte without a bed, d == +0 over one, nothing where neither plane is set;
//   * a WAVE none of whose 256 cells has a counting neighbour stores +0 and returns (a ballot: wave-uniform).  Most of a harbour is open
//     water, and that is all most waves do;
//   * in the other waves a lane with a counting neighbour runs the several-cascade query (ocean_query.hip: query_solve, query_height,
//     the blended sample's field 2 bit for bit) above its own centre and above each counting neighbour's, one point after the other in
//     a loop that is not unrolled; the other lanes of the wave idle through it.  CHOSEN for being the definition read aloud; what it
//     costs is lanes idle along a wall that crosses the rows (a wall along a row fills the wave).  NOT DONE AND NOT MEASURED: compacting
//     the (cell, neighbour) pairs of a tile into a list in LDS and dealing them out to all 256 lanes; sharing a height between the cells
//     that ask for the same centre through LDS (a solid cell's centre is asked for by up to four neighbours, a wet one's by itself
//     and never by another, so at most a factor 5 / 2 is there to take; a height is a function of its centre, the list and the set
//     alone, so a shared one has the bits of one computed again and every F keeps its bits);
//   * every access goes through a buffer resource over exactly its plane; F is written through like the other planes.
//
// ocean_ripple_step_walls_swell_kernel and ocean_ripple_bed_swell_step_kernel, one sub-step each, are ocean_ripple_step_walls_kernel and
// ocean_ripple_bed_step_kernel restated with one more load per cell -- F, the cell's own, no halo -- and ripple_swell_update or
// ripple_swell_bed_update at the end.  Those two kernels and their files are not touched and keep their instructions.  A sub-step with
// swell reads 4 bytes per cell more than its parent.
// No scratch, no atomics, no inline assembly (make resource-usage).

#pragma once

#include "ocean_ripple_swell.h"
#include "ocean_ripple_bed.hip"

namespace ocean
{
  struct RippleSwellRefreshArgs
  {
    float *swell;                               // [R][R], memory order: F
    unsigned char const *wall;                  // the wall plane, null while walls are off; not read over a bed
    float const *depth;                         // the bed's depth plane, null while the bed is off
    RippleGrid g;
    float s;                                    // the cell side
    QueryArgs q;                                // the summed surface (query_frame is the launch's)
  };

  template<int LAYOUT>
  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_swell_refresh_kernel(RippleSwellRefreshArgs a)
  {
    __shared__ unsigned int flag[RIPPLE_TY + 2][RIPPLE_LX];

    int const R = a.g.R;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * RIPPLE_TX;
    int const y0 = (int)blockIdx.y * RIPPLE_TY;

    size_t const cells = (size_t)R * R;

    __amdgpu_buffer_rsrc_t const rswell = make_rsrc(a.swell, cells * sizeof(float));
    __amdgpu_buffer_rsrc_t const rwall = make_rsrc(a.wall, a.wall ? cells : 0);
    __amdgpu_buffer_rsrc_t const rbed = make_rsrc(a.depth, a.depth ? cells * sizeof(float) : 0);

    bool const bed = a.depth != nullptr, walls = a.wall != nullptr;

    // the solid flag of a memory cell (kernel-uniform choice of the plane)
    auto solid = [&](int cell) -> unsigned int
    {
      if (bed)
        return ripple_swell_solid_bed(buf_load_f32(rbed, cell * (int)sizeof(float), 0)) ? 1u : 0u;

      return walls && ripple_swell_solid(buf_load_u8(rwall, cell, 0)) ? 1u : 0u;
    };

    int const lx = t & (RIPPLE_TX - 1);
    int const ly = t / RIPPLE_TX;

    // body: memory cell (x0 + lx, y0 + ly + 4 s)
    unsigned int bflag[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
      bflag[s] = solid((y0 + ly + RIPPLE_ROWSTEP * s) * R + x0 + lx);

    // halo: the rows above and below, then the columns left and right, wrapped on the torus
    unsigned int hflag = 0;
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

      hflag = solid(y * R + x);
    }

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
      flag[ly + RIPPLE_ROWSTEP * s + 1][lx + 1] = bflag[s];

    if (t < RIPPLE_HALO)
      flag[hy][hx] = hflag;

    __syncthreads();

    int const wx = ripple_wrap(x0 + lx - a.g.ox, R);

    // which of the four neighbours of each of the thread's cells count: bits 0 .. 3 are L R D U; none on a solid cell, whose F is +0
    unsigned int need[RIPPLE_PER_THREAD];
    unsigned int any = 0;

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const r = ly + RIPPLE_ROWSTEP * s + 1;
      int const wy = ripple_wrap(y0 + r - 1 - a.g.oy, R);

      unsigned int const cL = ripple_swell_counts(wx != 0, flag[r][lx] != 0) ? 1u : 0u;
      unsigned int const cR = ripple_swell_counts(wx != R - 1, flag[r][lx + 2] != 0) ? 2u : 0u;
      unsigned int const cD = ripple_swell_counts(wy != 0, flag[r - 1][lx + 1] != 0) ? 4u : 0u;
      unsigned int const cU = ripple_swell_counts(wy != R - 1, flag[r + 1][lx + 1] != 0) ? 8u : 0u;

      need[s] = bflag[s] != 0 ? 0u : (cL | cR) | (cD | cU);
      any |= need[s];
    }

    // open water, and the inside of the land: nothing to ask the surface
    if (__builtin_amdgcn_ballot_w64(any != 0) == 0)
    {
      #pragma unroll
      for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
        buf_store_f32_aux<RIPPLE_STORE_AUX>(0.0f, rswell, ((y0 + ly + RIPPLE_ROWSTEP * s) * R + x0 + lx) * (int)sizeof(float), 0);

      return;
    }

    int const I = ripple_world(x0 + lx, a.g.ox, R);

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const my = y0 + ly + RIPPLE_ROWSTEP * s;
      int const J = ripple_world(my, a.g.oy, R);

      float Hc = 0.0f, dL = 0.0f, dR = 0.0f, dD = 0.0f, dU = 0.0f;

      // point 0 is the cell's own centre, points 1 .. 4 its neighbours' L R D U; a lane takes a point it needs
      #pragma unroll 1
      for(int k = 0; k < 5; ++k)
      {
        bool const counts = k == 0 ? need[s] != 0 : ((need[s] >> (k - 1)) & 1u) != 0;

        if (counts)
        {
          int const di = k == 1 ? -1 : k == 2 ? 1 : 0;
          int const dj = k == 3 ? -1 : k == 4 ? 1 : 0;

          float2 const p = make_float2(ripple_swell_centre(I + di, a.s), ripple_swell_centre(J + dj, a.s));

          float const H = query_height<LAYOUT>(a.q, query_solve<LAYOUT>(a.q, p));

          float const d = ripple_swell_face(k != 0, Hc, H);

          Hc = k == 0 ? H : Hc;
          dL = k == 1 ? d : dL;
          dR = k == 2 ? d : dR;
          dD = k == 3 ? d : dD;
          dU = k == 4 ? d : dU;
        }
      }

      float const F = ripple_swell_force(bflag[s] != 0, dL, dR, dD, dU);

      buf_store_f32_aux<RIPPLE_STORE_AUX>(F, rswell, (my * R + x0 + lx) * (int)sizeof(float), 0);
    }
  }

  // a.q (but its frame) and the planes filled in
  inline hipError_t launch_ripple_swell_refresh(RippleSwellRefreshArgs &a, hipStream_t stream)
  {
    query_frame(a.q);

    void *args[] = { &a };

    return hipLaunchKernel(layout_kernel(a.q.N, &ocean_ripple_swell_refresh_kernel<GEN_PLAIN>, &ocean_ripple_swell_refresh_kernel<GEN_BANDED>), dim3((unsigned)(a.g.R / RIPPLE_TX), (unsigned)(a.g.R / RIPPLE_TY)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // the WAVE sub-step with walls and swell: ocean_ripple_step_walls_kernel's form
  struct RippleWallSwellStepArgs
  {
    RippleWallStepArgs w;
    float const *swell;
  };

  template<bool FIRST>
  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_step_walls_swell_kernel(RippleWallSwellStepArgs a)
  {
    __shared__ float tile[RIPPLE_TY + 2][RIPPLE_LX];
    __shared__ unsigned int flag[RIPPLE_TY + 2][RIPPLE_LX];

    RippleStepArgs const &p = a.w.s;

    int const R = p.g.R;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * RIPPLE_TX;
    int const y0 = (int)blockIdx.y * RIPPLE_TY;

    size_t const cells = (size_t)R * R;

    __amdgpu_buffer_rsrc_t const rin = make_rsrc(p.in, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rout = make_rsrc(p.out, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rsrc = make_rsrc(p.src, cells * sizeof(int));
    __amdgpu_buffer_rsrc_t const rwall = make_rsrc(a.w.wall, cells);
    __amdgpu_buffer_rsrc_t const rswell = make_rsrc(a.swell, cells * sizeof(float));

    int const lx = t & (RIPPLE_TX - 1);
    int const ly = t / RIPPLE_TX;

    // body: memory cell (x0 + lx, y0 + ly + 4 s)
    float2 body[RIPPLE_PER_THREAD];
    int bsrc[RIPPLE_PER_THREAD];
    unsigned int bwall[RIPPLE_PER_THREAD];
    float bswell[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const cell = (y0 + ly + RIPPLE_ROWSTEP * s) * R + x0 + lx;

      body[s] = buf_load_f32x2(rin, cell * (int)sizeof(float2), 0);
      bsrc[s] = FIRST ? (int)buf_load_u32(rsrc, cell * (int)sizeof(int), 0) : 0;
      bwall[s] = buf_load_u8(rwall, cell, 0);
      bswell[s] = buf_load_f32(rswell, cell * (int)sizeof(float), 0);
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

    int const wx = ripple_wrap(x0 + lx - p.g.ox, R);

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const r = ly + RIPPLE_ROWSTEP * s + 1;
      int const my = y0 + r - 1;
      int const wy = ripple_wrap(my - p.g.oy, R);

      float const e = tile[r][lx + 1];
      float const eL = ripple_wall_neighbour(wx != 0, flag[r][lx] != 0, e, tile[r][lx]);
      float const eR = ripple_wall_neighbour(wx != R - 1, flag[r][lx + 2] != 0, e, tile[r][lx + 2]);
      float const eD = ripple_wall_neighbour(wy != 0, flag[r - 1][lx + 1] != 0, e, tile[r - 1][lx + 1]);
      float const eU = ripple_wall_neighbour(wy != R - 1, flag[r + 1][lx + 1] != 0, e, tile[r + 1][lx + 1]);

      float const f = p.f[ripple_sponge(wx, wy, R, p.B)];

      RippleCell const c = ripple_swell_update(e, body[s].y, eL, eR, eD, eU, bswell[s], bwall[s] != 0, p.h, p.c2s2, f);

      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ c.eta, c.rate }, rout, (my * R + x0 + lx) * (int)sizeof(float2), 0);
    }
  }

  inline hipError_t launch_ripple_step_walls_swell(RippleWallSwellStepArgs &a, bool first, hipStream_t stream)
  {
    void *args[] = { &a };

    void const *kernel = first ? reinterpret_cast<void const*>(&ocean_ripple_step_walls_swell_kernel<true>) : reinterpret_cast<void const*>(&ocean_ripple_step_walls_swell_kernel<false>);

    return hipLaunchKernel(kernel, dim3((unsigned)(a.w.s.g.R / RIPPLE_TX), (unsigned)(a.w.s.g.R / RIPPLE_TY)), dim3(RIPPLE_THREADS), args, 0, stream);
  }

  // the WAVE sub-step over a bed with swell: ocean_ripple_bed_step_kernel's form
  struct RippleBedSwellStepArgs
  {
    RippleBedStepArgs b;
    float const *swell;
  };

  template<bool FIRST>
  __global__ void __launch_bounds__(RIPPLE_THREADS) ocean_ripple_bed_swell_step_kernel(RippleBedSwellStepArgs a)
  {
    __shared__ float tile[RIPPLE_TY + 2][RIPPLE_LX];
    __shared__ float bed[RIPPLE_TY + 2][RIPPLE_LX];

    RippleStepArgs const &p = a.b.s;

    int const R = p.g.R;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * RIPPLE_TX;
    int const y0 = (int)blockIdx.y * RIPPLE_TY;

    size_t const cells = (size_t)R * R;

    __amdgpu_buffer_rsrc_t const rin = make_rsrc(p.in, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rout = make_rsrc(p.out, cells * sizeof(float2));
    __amdgpu_buffer_rsrc_t const rsrc = make_rsrc(p.src, cells * sizeof(int));
    __amdgpu_buffer_rsrc_t const rbed = make_rsrc(a.b.depth, cells * sizeof(float));
    __amdgpu_buffer_rsrc_t const rsurf = make_rsrc(a.b.surf, cells);
    __amdgpu_buffer_rsrc_t const rswell = make_rsrc(a.swell, cells * sizeof(float));

    int const lx = t & (RIPPLE_TX - 1);
    int const ly = t / RIPPLE_TX;

    // body: memory cell (x0 + lx, y0 + ly + 4 s)
    float2 body[RIPPLE_PER_THREAD];
    int bsrc[RIPPLE_PER_THREAD];
    float bbed[RIPPLE_PER_THREAD];
    unsigned int bsurf[RIPPLE_PER_THREAD];
    float bswell[RIPPLE_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const cell = (y0 + ly + RIPPLE_ROWSTEP * s) * R + x0 + lx;

      body[s] = buf_load_f32x2(rin, cell * (int)sizeof(float2), 0);
      bsrc[s] = FIRST ? (int)buf_load_u32(rsrc, cell * (int)sizeof(int), 0) : 0;
      bbed[s] = buf_load_f32(rbed, cell * (int)sizeof(float), 0);
      bsurf[s] = buf_load_u8(rsurf, cell, 0);
      bswell[s] = buf_load_f32(rswell, cell * (int)sizeof(float), 0);
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

    int const wx = ripple_wrap(x0 + lx - p.g.ox, R);

    #pragma unroll
    for(int s = 0; s < RIPPLE_PER_THREAD; ++s)
    {
      int const r = ly + RIPPLE_ROWSTEP * s + 1;
      int const my = y0 + r - 1;
      int const wy = ripple_wrap(my - p.g.oy, R);

      float const e = tile[r][lx + 1];
      float const dc = bbed[s];

      float const tL = ripple_bed_flux(wx != 0, dc, bed[r][lx], e, tile[r][lx]);
      float const tR = ripple_bed_flux(wx != R - 1, dc, bed[r][lx + 2], e, tile[r][lx + 2]);
      float const tD = ripple_bed_flux(wy != 0, dc, bed[r - 1][lx + 1], e, tile[r - 1][lx + 1]);
      float const tU = ripple_bed_flux(wy != R - 1, dc, bed[r + 1][lx + 1], e, tile[r + 1][lx + 1]);

      // (a surf level above the table's end cannot come from the raster; the index is held to the table all the same)
      unsigned int const q = bsurf[s] < (unsigned int)RIPPLE_SURF_LEVELS ? bsurf[s] : (unsigned int)RIPPLE_SURF_LEVELS;

      RippleCell const c = ripple_swell_bed_update(e, body[s].y, tL, tR, tD, tU, dc, bswell[s], p.h, a.b.gs2, p.f[ripple_sponge(wx, wy, R, p.B)], a.b.fsurf[q]);

      buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ c.eta, c.rate }, rout, (my * R + x0 + lx) * (int)sizeof(float2), 0);
    }
  }

  inline hipError_t launch_ripple_bed_swell_step(RippleBedSwellStepArgs &a, bool first, hipStream_t stream)
  {
    void *args[] = { &a };

    void const *kernel = first ? reinterpret_cast<void const*>(&ocean_ripple_bed_swell_step_kernel<true>) : reinterpret_cast<void const*>(&ocean_ripple_bed_swell_step_kernel<false>);

    return hipLaunchKernel(kernel, dim3((unsigned)(a.b.s.g.R / RIPPLE_TX), (unsigned)(a.b.s.g.R / RIPPLE_TY)), dim3(RIPPLE_THREADS), args, 0, stream);
  }
}
