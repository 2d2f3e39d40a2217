// ocean_foam.hip -- the Jacobian foam plane of datum_ocean_displace (an extension: the reference computes no foam).
//
// The mesh places each vertex at p - D(p), D = (dx, dy) of map layer 0 with the choppiness already applied (ocean_gen.hip; gen.comp:122-124).
// Per texel, with periodic central differences in world units (h = wavescale / N, the texel pitch; x = column, y = row):
//
//     J = (1 - a)(1 - d) - b c,   a = d/dx dx,  b = d/dy dx,  c = d/dx dy,  d = d/dy dy,   f' = (f[i+1] - f[i-1]) / (2 h)
//
// J < 0: the rendered mesh folds over at that texel; J = 1: undisturbed.  FOAM_JACOBIAN stores J; FOAM_ACCUMULATE stores
// max(clamp((threshold - J) gain, 0, 1), previous * fade).  One fp32 plane per cascade, row-major [cascade][y][x].
//
// One workgroup per 64 x 32 tile of a cascade: the tile's (dx, dy) and a one-texel periodic halo (64 above, 64 below, 32 left,
// 32 right; the corners are not needed) are staged in LDS, then every wave writes whole 256-byte rows of the plane.  The tile
// is whole patches of the map layout (map_compact_a: PW x PH = 16 texels, 64 and 32 are multiples of every PW and PH), so the
// body's loads take the two 128-byte lines of each patch's part A whole; the 192 halo texels are 9 % of what a tile loads.
// Bytes per point: 16 read (part A, of which dx, dy are used) + 4 written; FOAM_ACCUMULATE reads the previous 4 as well.
// The row-pass and column-pass kernels are not touched: the maps are bit-identical with foam on or off.

#pragma once

#include "ocean_layout.h"
#include "ocean_kernels.hip"

namespace ocean
{
  constexpr int FOAM_TX = 64, FOAM_TY = 32, FOAM_THREADS = 256;
  constexpr int FOAM_PER_THREAD = FOAM_TX * FOAM_TY / FOAM_THREADS;   // 8
  constexpr int FOAM_HALO = 2 * FOAM_TX + 2 * FOAM_TY;                // 192 texels

  static_assert(FOAM_TX == 64 && FOAM_THREADS % FOAM_TX == 0, "one wave per tile row in the compute / store phase");

  // per cascade: 1 / (2 h) = N / (2 wavescale), and the accumulation's parameters with fade = exp(-decay dt) rounded once on the host
  struct FoamCascade { float inv2h, threshold, gain, fade; };

  struct FoamArgs
  {
    float4 const *maps;   // [cascade] map blocks (map_cascade_bytes each)
    float *foam;          // [cascade][N][N]
    int first;            // first cascade of this launch (blockIdx.y counts from it)
    FoamCascade casc[DATUM_OCEAN_MAX_CASCADES];
  };

  template<int N> constexpr int foam_tiles() { return (N / FOAM_TX) * (N / FOAM_TY); }

  template<int N, bool ACCUM, bool STREAM>
  __global__ void __launch_bounds__(FOAM_THREADS) ocean_foam_kernel(FoamArgs a)
  {
    static_assert(N % FOAM_TX == 0 && N % FOAM_TY == 0 && band_cols(N) % FOAM_TX == 0, "a tile lies inside one band of the map layout");

    constexpr int PW = map_patch_cols(N), PH = map_patch_rows(N);
    constexpr int PPR = FOAM_TX / PW;                                  // patches per tile row of patches
    constexpr int LX = FOAM_TX + 2;

    static_assert(FOAM_TY % PH == 0, "a tile is whole patches");

    // (written through or streamed as the plan stores the maps: MAP_STORE_AUX / MAP_STORE_AUX_STREAM)
    constexpr int AUX = STREAM ? MAP_STORE_AUX_STREAM : MAP_STORE_AUX;

    __shared__ float2 tile[FOAM_TY + 2][LX];

    int const t = (int)threadIdx.x;
    int const cascade = a.first + (int)blockIdx.y;
    int const x0 = ((int)blockIdx.x % (N / FOAM_TX)) * FOAM_TX;
    int const y0 = ((int)blockIdx.x / (N / FOAM_TX)) * FOAM_TY;

    __amdgpu_buffer_rsrc_t rmaps = make_rsrc(reinterpret_cast<char const*>(a.maps) + (size_t)cascade * map_cascade_bytes(N), map_cascade_bytes(N));
    __amdgpu_buffer_rsrc_t rfoam = make_rsrc(a.foam + (size_t)cascade * N * N, (size_t)N * N * sizeof(float));

    // body: texel q = s * THREADS + t is texel q % 16 of the tile's patch q / 16, so 16 neighbouring lanes read one patch's part A
    float2 body[FOAM_PER_THREAD];

    #pragma unroll
    for(int s = 0; s < FOAM_PER_THREAD; ++s)
    {
      int const q = s * FOAM_THREADS + t;
      int const p = q >> 4, j = q & 15;
      int const x = x0 + (p % PPR) * PW + j % PW;
      int const y = y0 + (p / PPR) * PH + j / PW;

      body[s] = buf_load_f32x2(rmaps, (int)map_compact_a(N, y, x), 0);
    }

    // halo: the rows above and below, then the columns left and right, wrapped
    float2 halo = make_float2(0.0f, 0.0f);
    int hy = 0, hx = 0;

    if (t < FOAM_HALO)
    {
      int x, y;

      if (t < 2 * FOAM_TX)
      {
        bool const below = t >= FOAM_TX;
        hx = (t & (FOAM_TX - 1)) + 1;
        hy = below ? FOAM_TY + 1 : 0;
        x = x0 + hx - 1;
        y = (y0 + (below ? FOAM_TY : -1)) & (N - 1);
      }
      else
      {
        bool const right = t >= 2 * FOAM_TX + FOAM_TY;
        hy = ((t - 2 * FOAM_TX) & (FOAM_TY - 1)) + 1;
        hx = right ? FOAM_TX + 1 : 0;
        x = (x0 + (right ? FOAM_TX : -1)) & (N - 1);
        y = y0 + hy - 1;
      }

      halo = buf_load_f32x2(rmaps, (int)map_compact_a(N, y, x), 0);
    }

    // this thread's points in the store phase: column x0 + (t % 64), rows t / 64 + 4 s -- one wave per row of the tile
    constexpr int ROWSTEP = FOAM_THREADS / FOAM_TX;
    int const lx = t & (FOAM_TX - 1);
    int const ly = t / FOAM_TX;

    float prev[ACCUM ? FOAM_PER_THREAD : 1];

    if constexpr (ACCUM)
    {
      #pragma unroll
      for(int s = 0; s < FOAM_PER_THREAD; ++s)
        prev[s] = buf_load_f32(rfoam, ((y0 + ly + ROWSTEP * s) * N + x0 + lx) * 4, 0);
    }

    #pragma unroll
    for(int s = 0; s < FOAM_PER_THREAD; ++s)
    {
      int const q = s * FOAM_THREADS + t;
      int const p = q >> 4, j = q & 15;

      tile[(p / PPR) * PH + j / PW + 1][(p % PPR) * PW + j % PW + 1] = body[s];
    }

    if (t < FOAM_HALO)
      tile[hy][hx] = halo;

    __syncthreads();

    FoamCascade const fc = a.casc[cascade];

    #pragma unroll
    for(int s = 0; s < FOAM_PER_THREAD; ++s)
    {
      int const r = ly + ROWSTEP * s + 1;

      float2 const xm = tile[r][lx], xp = tile[r][lx + 2];
      float2 const ym = tile[r - 1][lx + 1], yp = tile[r + 1][lx + 1];

      // (built with -ffp-contract=off: every product and difference is rounded as written)
      float const da = (xp.x - xm.x) * fc.inv2h;      // d dx / dx
      float const db = (yp.x - ym.x) * fc.inv2h;      // d dx / dy
      float const dc = (xp.y - xm.y) * fc.inv2h;      // d dy / dx
      float const dd = (yp.y - ym.y) * fc.inv2h;      // d dy / dy

      float v = (1.0f - da) * (1.0f - dd) - db * dc;

      if constexpr (ACCUM)
        v = fmaxf(fminf(fmaxf((fc.threshold - v) * fc.gain, 0.0f), 1.0f), prev[s] * fc.fade);

      buf_store_f32_aux<AUX>(v, rfoam, ((y0 + r - 1) * N + x0 + lx) * 4, 0);
    }
  }

  // the four forms at resolution N: [ACCUMULATE][maps streamed]
  struct FoamKernels { void const *k[2][2]; };

  template<int N>
  FoamKernels foam_kernels()
  {
    FoamKernels f;

    f.k[0][0] = reinterpret_cast<void const*>(&ocean_foam_kernel<N, false, false>);
    f.k[0][1] = reinterpret_cast<void const*>(&ocean_foam_kernel<N, false, true>);
    f.k[1][0] = reinterpret_cast<void const*>(&ocean_foam_kernel<N, true, false>);
    f.k[1][1] = reinterpret_cast<void const*>(&ocean_foam_kernel<N, true, true>);

    return f;
  }
}
