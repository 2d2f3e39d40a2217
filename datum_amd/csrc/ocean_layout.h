// ocean_layout.h -- the module's two private memory layouts, stated once: the blocked work spectrum the row pass writes
// and the column pass reads, and the patched, banded displacement maps every other kernel reads or writes.
//
// Index arithmetic only, host/device neutral so that a CPU can walk every grid point of every resolution through it
// (tests/cpu/layout_emul.cpp, tests/test_layout_emul.py); the kernels that use it live in the .hip files beside it.

#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define OL_HD __host__ __device__ __forceinline__
#else
#define OL_HD inline
#endif

namespace ocean
{
  //|---------------------- work spectrum --------------------------------------
  // Per cascade, 8 x 8 blocks of 16-byte values (C, D), [y/8][x/8][y%8][x%8]: a row of a block is one 128-byte line; a
  // column-pass wave reads whole blocks.  The largest grids keep the columns one XCD works on at a time contiguous
  // ([x/B][...]: band_cols), for the maps too (map_compact_patch).

  constexpr int SBR = 8, SBC = 8;

  // columns per block, by the stored value's size.  The 8-byte values of the fp16-stored spectrum keep 8 columns (64-byte block rows): with 16 -- whole
  // lines per row-pass store -- the row pass gains 6-14 us at 4096^2 and 2048^2 x 4 and the column pass, whose narrow tiles then take 16 bytes of
  // every line they touch, loses as much or more (profiles/r06_spectrum_blocks.txt: 4096^2 with h0 as halves 5.2 -> 5.1 k grids/s)
  OL_HD constexpr int spec_block_cols(bool half) { return half ? 8 : SBC; }

  // Bands (large grids): the columns one XCD's column-pass workgroups work on at the same time are made contiguous in
  // memory -- [x / B][rows][x % B] -- for the work spectrum and for the maps alike, so that what is read and written
  // concurrently is a dense region instead of 2 KB pieces of rows 128 KB apart (4096^2).  B = band_cols(N), 0 = whole rows.
  // measured (profiles/r02_large_grids.txt): 4096^2 B = 64 (32 CUs x 2-column tiles): column pass 240 -> 226 us, with the
  // fp16-stored spectrum 202 -> 164 us; 2048^2 x 4 B = 128 (32 CUs x 4-column tiles): 181 -> 167 us; B = 512 at 4096^2: 270 us.
  // With the maps in 2 x 2 patches at 4096^2 (round 3's layout): B = 64 184-195 us, B = 128 176-183 us, B = 256 192 us, B = 512 / none 220 us
  OL_HD constexpr int band_cols(int N) { return (N >= 2048) ? 128 : N; }

  // element index of grid point (y, x) in the blocked work spectrum: per band, blocks of SBR rows x SBC columns, row-major inside
  OL_HD constexpr size_t blocked_at(int N, int y, int x, bool half = false)
  {
    int const B = band_cols(N);
    int const BC = spec_block_cols(half);

    return (size_t)(x / B) * N * B + ((size_t)(y / SBR) * (B / BC) + (x % B) / BC) * (SBR * BC) + (y % SBR) * BC + (x % BC);
  }

  template<int N, bool H16 = false>
  OL_HD constexpr size_t blocked(int y, int x) { return blocked_at(N, y, x, H16); }

  //|---------------------- displacement maps, texel -> byte offset ------------
  // Displacement map layout (private to this module: in the reference the map is a VK_IMAGE_TILING_OPTIMAL 2-layer image whose
  // only reader is ocean.gen's sampler, ocean.cpp:706, gen.comp:113-114; datum_ocean_read_maps / datum_ocean_export_maps hand out
  // the logical [layer][y][x] RGBA32F image).
  // 24 bytes per texel instead of 32 -- the two RGBA32F layers' .w channels are
  // constant zero (map.comp:79-80) and nothing reads them (gen.comp:113-114 takes .xyz), yet they were a quarter of what the
  // write-bound column pass stores.  Per cascade, bands as above; inside a band PATCHES of PW x PH = 16 texels, patch rows
  // one after the other; a patch is 384 bytes = three 128-byte lines:
  //     part A, 256 bytes: texel j = (y % PH) * PW + x % PW  ->  float4 (dx, dy, dz, nx)   at 16 j
  //     part B, 128 bytes: texel j                            ->  float2 (ny, nz)           at 256 + 8 j
  // PW = the column pass's tile width at that resolution (8 up to 256^2, 2 at 512^2, 4 at 1024^2 and 2048^2, 2 at 4096^2), so that the 16 texels of
  // a patch are 16 neighbouring lanes of a column-pass wave: one 16-byte and one 8-byte store instruction per thread and slot
  // write two whole lines and one whole line per patch -- no lane trades, no partial lines.  For ocean.gen a 4 x 4 patch holds
  // the four corners of a bilinear fetch more often than a 4 x 1 group did.
  constexpr int MAP_PATCH = 16, MAP_PATCH_LOG2 = 4;                // texels per patch
  constexpr int MAP_A_STRIDE = 16, MAP_B_STRIDE = 8;               // bytes of a texel's part A, (dx, dy, dz, nx), and part B, (ny, nz)
  constexpr int MAP_TEXEL_BYTES = MAP_A_STRIDE + MAP_B_STRIDE;     // 24
  constexpr int MAP_PART_B = MAP_PATCH * MAP_A_STRIDE;             // 256: where part B begins in its patch
  constexpr int MAP_PATCH_BYTES = MAP_PATCH * MAP_TEXEL_BYTES;     // 384

  static_assert((1 << MAP_PATCH_LOG2) == MAP_PATCH && MAP_PATCH_BYTES == 3 * 128, "a patch is three 128-byte lines, two of part A and one of part B");

  OL_HD constexpr int map_patch_cols(int N) { return N <= 256 ? 8 : (N == 512 ? 2 : (N <= 2048 ? 4 : 2)); }     // == ColCfg<N>::W (asserted there)
  OL_HD constexpr int map_patch_rows(int N) { return MAP_PATCH / map_patch_cols(N); }

  // bytes of one cascade's maps
  OL_HD constexpr size_t map_cascade_bytes(int N) { return (size_t)N * N * MAP_TEXEL_BYTES; }

  // byte offset of texel (x, y)'s patch inside its cascade's block; its part A is map_compact_a(...), part B map_compact_b(...)
  OL_HD constexpr size_t map_compact_patch(int N, int y, int x)
  {
    int const B = band_cols(N);
    int const PW = map_patch_cols(N), PH = map_patch_rows(N);

    return (size_t)(x / B) * MAP_TEXEL_BYTES * N * B + ((size_t)(y / PH) * (B / PW) + (x % B) / PW) * MAP_PATCH_BYTES;
  }

  OL_HD constexpr int map_compact_j(int N, int y, int x) { return (y % map_patch_rows(N)) * map_patch_cols(N) + x % map_patch_cols(N); }

  OL_HD constexpr size_t map_compact_a(int N, int y, int x) { return map_compact_patch(N, y, x) + MAP_A_STRIDE * map_compact_j(N, y, x); }
  OL_HD constexpr size_t map_compact_b(int N, int y, int x) { return map_compact_patch(N, y, x) + MAP_PART_B + MAP_B_STRIDE * map_compact_j(N, y, x); }

  // bytes from a texel's patch to the patch of the same column k * PH rows on
  OL_HD constexpr int map_compact_patchrow_bytes(int N) { return (band_cols(N) / map_patch_cols(N)) * MAP_PATCH_BYTES; }

  //|---------------------- displacement maps, the same as shifts ---------------
  // BYTE offset of a texel column's / row's part of the map layout; the two add up to the texel's
  // displacement: part A of its patch, (dx, dy, dz, nx) -- whose part B, (ny, nz), lies at A + MAP_PART_B - bcolumn(i) - brow(j).
  //   PLAIN   N <= 1024: whole rows
  //   BANDED  2048 and 4096: bands of band_cols(N) columns
  enum GenLayout { GEN_PLAIN = 0, GEN_BANDED = 1 };

  template<int LAYOUT> struct TexelIndex
  {
    int ln, lb, bmask;
    int lpw, lph;            // log2 of the patch's columns and rows

    OL_HD TexelIndex(int N) : ln(31 - __builtin_clz(N)), lb(31 - __builtin_clz(band_cols(N))), bmask(band_cols(N) - 1),
                              lpw(31 - __builtin_clz(map_patch_cols(N))), lph(31 - __builtin_clz(map_patch_rows(N))) { }

    OL_HD int column(int i) const
    {
      int const inband = ((i & bmask) >> lpw) * MAP_PATCH_BYTES + ((i & ((1 << lpw) - 1)) << 4);

      if constexpr (LAYOUT == GEN_PLAIN)
        return inband;
      else
        return (i >> lb) * (3 << (3 + ln + lb)) + inband;           // 24 N B bytes per band
    }

    OL_HD int row(int j) const
    {
      return (j >> lph) * (3 << (7 + lb - lpw)) + ((j & ((1 << lph) - 1)) << (4 + lpw));     // 384 B / PW bytes per patch row
    }

    // 8 * (the texel's index in its patch), column and row part
    OL_HD int bcolumn(int i) const { return (i & ((1 << lpw) - 1)) << 3; }
    OL_HD int brow(int j) const { return (j & ((1 << lph) - 1)) << (3 + lpw); }
  };

  inline GenLayout gen_layout(int N) { return (band_cols(N) != N) ? GEN_BANDED : GEN_PLAIN; }

  // of a kernel template's two instances, the one for N's layout, as hipLaunchKernel takes it
  template<class Kernel> inline void const *layout_kernel(int N, Kernel *plain, Kernel *banded)
  {
    return reinterpret_cast<void const*>(gen_layout(N) == GEN_PLAIN ? plain : banded);
  }

  //|---------------------- displacement maps, byte offset -> texel -------------
  // The layout read backwards, for the kernels that take the maps in the order they lie in memory (ocean_pack_kernel, ocean_export_kernel):
  // the layout's shape as shifts, and part number r of a cascade -- parts A (and B) counted patch after patch -- back to its texel.
  struct PackShape
  {
    int n2;                 // log2 N
    int pw2;                // log2 of a patch's width
    int bp2;                // log2 of the patches in a row of patches of one band (B / PW)
    int bandpatches2;       // log2 of the patches per band ((N / PH) * (B / PW))
    int b2;                 // log2 of the band's columns
  };

  inline PackShape pack_shape(int N)
  {
    auto log2of = [](int v) { int l = 0; while ((1 << l) < v) ++l; return l; };

    int const B = band_cols(N), PW = map_patch_cols(N), PH = map_patch_rows(N);

    PackShape sh;
    sh.n2 = log2of(N);
    sh.pw2 = log2of(PW);
    sh.bp2 = log2of(B / PW);
    sh.bandpatches2 = log2of((N / PH) * (B / PW));
    sh.b2 = log2of(B);

    return sh;
  }

  // part A number r of the block at `block` (a byte offset or a byte pointer), which needs no shape: block + map_part(sh, r).a
  template<typename Block>
  OL_HD constexpr Block map_part_a(Block block, size_t r) { return block + (r >> MAP_PATCH_LOG2) * MAP_PATCH_BYTES + (r & (MAP_PATCH - 1)) * MAP_A_STRIDE; }

  struct MapPart { int y, x; size_t a, b; };      // the texel, and map_compact_a / _b of it

  // texel j = r % 16 of patch P = r / 16 (map_compact_patch / map_compact_j read backwards)
  OL_HD MapPart map_part(PackShape const &sh, size_t r)
  {
    int const P = (int)(r >> MAP_PATCH_LOG2), j = (int)(r & (MAP_PATCH - 1));
    int const band = P >> sh.bandpatches2, pp = P & ((1 << sh.bandpatches2) - 1);

    MapPart m;
    m.y = ((pp >> sh.bp2) << (MAP_PATCH_LOG2 - sh.pw2)) + (j >> sh.pw2);
    m.x = (band << sh.b2) + ((pp & ((1 << sh.bp2) - 1)) << sh.pw2) + (j & ((1 << sh.pw2) - 1));
    m.a = (size_t)P * MAP_PATCH_BYTES + j * MAP_A_STRIDE;
    m.b = (size_t)P * MAP_PATCH_BYTES + MAP_PART_B + j * MAP_B_STRIDE;

    return m;
  }
}
