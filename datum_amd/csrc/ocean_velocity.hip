// ocean_velocity.hip -- the surface velocity plane of datum_ocean_displace and its several-cascade query (an extension: the reference
// computes no velocity; include/datum_ocean_hip.h, "surface velocity").
//
// (vx, vy, vz) = d/dt of map layer 0's (dx, dy, dz) at a fixed texel: the step's own 2-D transform of ocean_velocity.h's spectrum.
// Two kernels per cascade group, launched behind the group's column pass and foam launch.  The transform is separable and the PLANE is
// row-major, so the COLUMNS go first and the rows last: the kernel that writes the plane holds whole rows and stores whole lines at every N.
//
//   velocity column pass  W columns per workgroup.  Reads phase (4 B/pt), h0 (8, plus ocean.sim's mirror column through L2) and the
//                         dispersion quadrant; advances the phase by the dt's the step's row pass applied without storing
//                         (ocean_writeback.h) and stores nothing of it; forms ht and k^ once per point and transforms ht, htx, hty along
//                         the columns, one field after the other through the same LDS lines; writes them to a work buffer of its own,
//                         cf [slot][field] in blocks of BC columns x BR rows = one 128-byte line (24)
//   velocity row pass     whole rows; the three fields one after the other through one LDS line per row; keeps the real parts, applies
//                         (-1)^(x+y) and the choppiness, writes float4 (vx, vy, vz, 0) row-major [cascade][y][x] (16): consecutive lanes,
//                         consecutive texels, written through or streamed as the plan stores the maps
//
// = 76 bytes per point (4 + 8 + 24 + 24 + 16).  Three transforms, not the step's two packed ones: the packing pairs a line with its
// negated index in one workgroup and trades values through LDS (ocean_kernels.hip, "packed step"); the velocity is opt-in and not on the
// step's critical path, and the plain form has no trade.  The step's kernels are not touched: maps, phase and foam are the bits of
// a handle with velocity off.
// Every store instruction of both kernels fills 128-byte lines: the column pass's 64 lanes cover W columns x 64 / W rows = whole blocks of
// the work buffer, the row pass's lanes consecutive float4 of one row.  No scratch, no atomics (make resource-usage); every access goes
// through a buffer resource laid over the cascade's plane of the array.

#pragma once

#include "ocean_kernels.hip"
#include "ocean_blend.hip"
#include "ocean_velocity.h"

namespace ocean
{
  struct VelocityArgs
  {
    float2 const *h0;       // [cascade][N*N]
    float const *phase;     // [cascade][N*N] as stored: behind the step's phase by dt[0 .. ndt)
    float const *omega;     // [cascade][(N/2+1)^2]
    cf const *tw;           // [N]
    cf *work;               // [cascade - first][3][N*N], blocked (VelCfg::work_index): ht, htx, hty between the two passes
    float4 *vel;            // [cascade][N*N] (vx, vy, vz, 0)
    int ndt;                // the dt's the step's row pass applied to the stored phase without storing (0 where it stored)
    int wild;               // a phase may lie outside [0, 2 pi): the general advance
    int first;              // first cascade of this launch (blockIdx.y counts from it)
    float dt[MAX_PENDING];
    CascadeConst casc[DATUM_OCEAN_MAX_CASCADES];
  };

  template<int N>
  struct VelCfg
  {
    static constexpr int E = (N >= 1024) ? 16 : default_radix(N);          // points per thread, both passes
    static constexpr int T = Plan<N, E>::T;

    // column pass: W columns per workgroup, at most 512 threads (256 registers per lane: ht and k^ of 16 points wait beside a 16-point
    // transform; a 1024-thread tile's 128 registers spilled)
    static constexpr int W = (N >= 4096) ? 2 : ((N >= 2048) ? 4 : ((N >= 512) ? 8 : 16));
    static constexpr int COL_THREADS = W * T;
    static constexpr int COL_LINE = LineFFT<N, W, E>::LINE;
    static constexpr size_t COL_LDS = ((size_t)LineFFT<N, 1, E>::MIDTAB + (size_t)W * COL_LINE) * sizeof(cf);
    static constexpr int COL_TILES = N / W;

    // the work buffer between the passes: blocks of BC columns x BR rows of cf = 128 bytes, block rows one after the other.  A wave of the
    // column pass is W columns x 64 / W rows, column-fastest: whole blocks
    static constexpr int BC = (W >= 4) ? 4 : 2;
    static constexpr int BR = 16 / BC;

    static OC_HD constexpr int work_index(int y, int x) { return ((y / BR) * (N / BC) + x / BC) * 16 + (y % BR) * BC + x % BC; }

    // row pass: whole rows, 128 threads or one row
    static constexpr int ROWS = (T >= 128) ? 1 : 128 / T;
    static constexpr int ROW_THREADS = ROWS * T;
    static constexpr int ROW_LINE = LineFFT<N, 1, E>::LINE;
    static constexpr size_t ROW_LDS = ((size_t)LineFFT<N, 1, E>::MIDTAB + (size_t)ROWS * ROW_LINE) * sizeof(cf);
    static constexpr int ROW_GROUPS = N / ROWS;

    static_assert(COL_THREADS <= 512 && ROW_THREADS <= 512, "workgroup size");
    static_assert(ROW_LDS <= (size_t)160 * 1024 && COL_LDS <= (size_t)160 * 1024, "LDS of a CU");
    static_assert(N % ROWS == 0 && N % W == 0, "whole workgroups");
    static_assert(W % BC == 0 && (64 / W) % BR == 0 && T % BR == 0 && T % BC == 0 && (64 / W) >= 1, "a wave of the column pass stores whole blocks; slots are whole blocks apart");
    static_assert(T >= 8, "eight consecutive float4 of a row per store instruction at least: whole lines");
    static_assert((size_t)N * N * sizeof(float4) <= 0x7FFFFFFFull, "a cascade's plane fits one buffer resource and a signed offset");
  };

  template<int N>
  __global__ void OCEAN_LDS_UNPAIRED __launch_bounds__(VelCfg<N>::COL_THREADS) ocean_velocity_col_kernel(VelocityArgs a)
  {
    typedef VelCfg<N> C;
    typedef LineFFT<N, C::W, C::E> L;

    constexpr int E = C::E;
    constexpr int T = C::T;
    constexpr int W = C::W;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    cf *midtab = reinterpret_cast<cf*>(smem);
    cf *lines = midtab + LineFFT<N, 1, E>::MIDTAB;            // [COL_LINE][W]

    for(int i = threadIdx.x; i < L::MIDTAB; i += C::COL_THREADS)
      midtab[i] = L::midtab_entry(a.tw, i);

    int const cp = (int)threadIdx.x % W;
    int const t = (int)threadIdx.x / W;
    int const x = (int)blockIdx.x * W + cp;
    int const cascade = a.first + (int)blockIdx.y;

    constexpr size_t plane = (size_t)N * N;
    constexpr size_t QUAD = (size_t)(N / 2 + 1) * (N / 2 + 1);

    __amdgpu_buffer_rsrc_t const romega = make_rsrc(a.omega + cascade * QUAD, QUAD * sizeof(float));
    __amdgpu_buffer_rsrc_t const rphase = make_rsrc(a.phase + cascade * plane, plane * sizeof(float));
    __amdgpu_buffer_rsrc_t const rh0 = make_rsrc(a.h0 + cascade * plane, plane * sizeof(float2));

    CascadeConst const cc = a.casc[cascade];

    typename LineTw<N, E>::type w;
    LineTw<N, E>::load(a.tw, t, w);

    // slot s is row y = t + T s of column x: the phase and h0 there, ocean.sim's mirror (N-1-y, N-1-x) backwards (sim.comp:59), the
    // dispersion by (|y - N/2|, |x - N/2|)
    int const e0 = t * N + x;
    int const m0 = (N - 1 - t - T * (E - 1)) * N + (N - 1 - x);
    int const oj = abs(x - N / 2);

    cf ht[E];
    float knx[E], kny[E];

    {
      float ph[E], om[E];
      float2 hk[E], hm[E];

      #pragma unroll
      for(int s = 0; s < E; ++s)
      {
        ph[s] = buf_load_f32(rphase, e0 * 4, T * s * N * 4);
        hk[s] = buf_load_f32x2(rh0, e0 * 8, T * s * N * 8);
        hm[s] = buf_load_f32x2(rh0, m0 * 8, T * (E - 1 - s) * N * 8);
        om[s] = buf_load_f32(romega, (abs(t + T * s - N / 2) * (N / 2 + 1) + oj) * 4, 0);
      }

      // the phase the step's maps were formed from: the same dt's on the same stored value by the same operations (ocean_phase.h)
      for(int k = 0; k < a.ndt; ++k)
      {
        float const dt = a.dt[k];

        #pragma unroll
        for(int s = 0; s < E; ++s)
        {
          float const wdt = om[s] * dt;

          // (the general advance for a handle on the wild path.  Not reachable with a list today: every host path that makes a handle
          // wild -- an uploaded phase outside [0, 2 pi), a dt the fused advance cannot take -- stores the phase first, so ndt is 0 then
          // (ocean_capi.hip: datum_ocean_displace, flush_phase) and no test can reach it; it is here so that a host path that one day
          // retains a list on a wild handle gets fmod and not the one-subtraction form)
          if (a.wild)
            ph[s] = advance_phase(ph[s], wdt);
          else
          {
            float const sum = ph[s] + wdt;

            ph[s] = fused_advance_select(sum, sum - 6.2831855f);
          }
        }
      }

      #pragma unroll
      for(int s = 0; s < E; ++s)
      {
        float sn, cs;

        sincos_phase(ph[s], &sn, &cs);

        velocity_ht(hk[s].x, hk[s].y, hm[s].x, hm[s].y, sn, cs, om[s], &ht[s].x, &ht[s].y);
        velocity_khat(x, t + T * s, N, cc.scale, &knx[s], &kny[s]);
      }
    }

    __syncthreads();      // the table of the middle pass

    int const b0 = C::work_index(t, x);

    #pragma unroll
    for(int f = 0; f < 3; ++f)
    {
      // one field after the other
      OC_SCHED_FENCE();

      cf v[1][E];

      #pragma unroll
      for(int s = 0; s < E; ++s)
      {
        if (f == 0)
          v[0][s] = ht[s];
        else
        {
          float hk2[2];

          velocity_hk(ht[s].x, ht[s].y, (f == 1) ? knx[s] : kny[s], hk2);

          v[0][s] = cf{ hk2[0], hk2[1] };
        }
      }

      fft_lines<N, 1, W, E>(v, t, lines + cp, 0, midtab, w, true);

      __amdgpu_buffer_rsrc_t const rwork = make_rsrc(a.work + ((size_t)(cascade - a.first) * 3 + f) * plane, plane * sizeof(cf));

      // slot s is T s rows down: whole block rows, T s N elements on
      #pragma unroll
      for(int s = 0; s < E; ++s)
        buf_store_cf_aux<SPEC_STORE_AUX>(v[0][s], rwork, b0 * 8, T * s * N * 8);
    }
  }

  template<int N, bool STREAM>
  __global__ void OCEAN_LDS_UNPAIRED __launch_bounds__(VelCfg<N>::ROW_THREADS) ocean_velocity_row_kernel(VelocityArgs a)
  {
    typedef VelCfg<N> C;
    typedef LineFFT<N, 1, C::E> L;

    constexpr int E = C::E;
    constexpr int T = C::T;

    // (written through or streamed as the plan stores the maps: MAP_STORE_AUX / MAP_STORE_AUX_STREAM)
    constexpr int AUX = STREAM ? MAP_STORE_AUX_STREAM : MAP_STORE_AUX;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    cf *midtab = reinterpret_cast<cf*>(smem);

    for(int i = threadIdx.x; i < L::MIDTAB; i += C::ROW_THREADS)
      midtab[i] = L::midtab_entry(a.tw, i);

    int const r = (int)threadIdx.x / T;
    int const t = (int)threadIdx.x % T;
    int const y = (int)blockIdx.x * C::ROWS + r;
    int const cascade = a.first + (int)blockIdx.y;

    cf *line = midtab + L::MIDTAB + r * C::ROW_LINE;

    constexpr size_t plane = (size_t)N * N;

    CascadeConst const cc = a.casc[cascade];

    typename LineTw<N, E>::type w;
    LineTw<N, E>::load(a.tw, t, w);

    __syncthreads();      // the table of the middle pass

    // slot s is column x = t + T s of row y: T s / BC blocks on in the work buffer
    int const b0 = C::work_index(y, t);

    float out[3][E];

    #pragma unroll
    for(int f = 0; f < 3; ++f)
    {
      __amdgpu_buffer_rsrc_t const rwork = make_rsrc(a.work + ((size_t)(cascade - a.first) * 3 + f) * plane, plane * sizeof(cf));

      // one field after the other: the next field's loads are not requested under this field's transform
      OC_SCHED_FENCE();

      cf v[1][E];

      #pragma unroll
      for(int s = 0; s < E; ++s)
        v[0][s] = buf_load_cf(rwork, b0 * 8, T * s * C::BR * 8);

      fft_lines<N, 1, 1, E>(v, t, line, C::ROW_LINE, midtab, w, true);

      #pragma unroll
      for(int s = 0; s < E; ++s)
        out[f][s] = v[0][s].x;
    }

    __amdgpu_buffer_rsrc_t const rvel = make_rsrc(a.vel + cascade * plane, plane * sizeof(float4));

    // (-1)^(x + y), x = t + T s: T is even, the sign is the thread's
    float const sigma = ((y + t) & 1) ? -1.0f : 1.0f;

    static_assert(T % 2 == 0, "the sign does not depend on the slot");

    #pragma unroll
    for(int s = 0; s < E; ++s)
    {
      float const vz = out[0][s] * sigma;
      float const vx = (out[1][s] * sigma) * cc.choppiness;
      float const vy = (out[2][s] * sigma) * cc.choppiness;

      buf_store_f32x4_aux<AUX>(make_float4(vx, vy, vz, 0.0f), rvel, (y * N + t) * 16, T * s * 16);
    }
  }

  // the kernels at resolution N as the module launches them
  struct VelocityKernels
  {
    void const *col = nullptr;
    void const *row[2] = { nullptr, nullptr };      // [maps streamed]
    int rowthreads = 0, rowgroups = 0, colthreads = 0, coltiles = 0;
    size_t rowlds = 0, collds = 0;
  };

  template<int N>
  VelocityKernels velocity_kernels()
  {
    typedef VelCfg<N> C;

    VelocityKernels k;

    k.col = reinterpret_cast<void const*>(&ocean_velocity_col_kernel<N>);
    k.row[0] = reinterpret_cast<void const*>(&ocean_velocity_row_kernel<N, false>);
    k.row[1] = reinterpret_cast<void const*>(&ocean_velocity_row_kernel<N, true>);
    k.rowthreads = C::ROW_THREADS;
    k.rowgroups = C::ROW_GROUPS;
    k.rowlds = C::ROW_LDS;
    k.colthreads = C::COL_THREADS;
    k.coltiles = C::COL_TILES;
    k.collds = C::COL_LDS;

    return k;
  }

  //|---------------------- the query ------------------------------------------

  struct VelocityBlendArgs
  {
    QueryArgs q;                                          // q.list's foam planes are not read
    float2 const *points;
    float4 *samples;                                      // 2 float4 per point
    int count;
    float4 const *vel[DATUM_OCEAN_MAX_CASCADES];          // the listed cascades' velocity planes, in list order
  };

  // datum_ocean_sample_velocity_blend: the several-cascade query's solve and V(b) (ocean_query.hip: query_solve, bit for bit), then the
  // listed cascades' velocity planes at the same texture coordinates with the same fetch (query_velocity)
  template<int LAYOUT>
  __global__ void __launch_bounds__(SURFACE_THREADS) ocean_velocity_blend_kernel(VelocityBlendArgs vb)
  {
    query_each_point(vb.points, vb.samples, vb.count, [&](float2 q) { return query_velocity<LAYOUT>(vb.q, query_solve<LAYOUT>(vb.q, q), q, vb.vel); });
  }

  // vb.q (but its frame), points, samples, count (> 0) and vb.vel filled in
  inline hipError_t launch_velocity_blend(VelocityBlendArgs &vb, hipStream_t stream)
  {
    query_frame(vb.q);

    void *args[] = { &vb };

    return hipLaunchKernel(layout_kernel(vb.q.N, &ocean_velocity_blend_kernel<GEN_PLAIN>, &ocean_velocity_blend_kernel<GEN_BANDED>), dim3((unsigned)((vb.count + SURFACE_THREADS - 1) / SURFACE_THREADS)), dim3(SURFACE_THREADS), args, 0, stream);
  }
}
