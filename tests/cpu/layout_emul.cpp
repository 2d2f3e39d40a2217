// The PRODUCT's layout arithmetic (datum_amd/csrc/ocean_layout.h) evaluated on the CPU at every grid point of a resolution,
// for tests/test_layout_emul.py to check: nothing here restates a formula, every number comes out of the header.
// Test harness only; built into libfft_core_emul.so.
#include <stdint.h>
#include "../../datum_amd/csrc/ocean_layout.h"

using namespace ocean;

static_assert(blocked<1024>(9, 17) == blocked_at(1024, 9, 17, false) && blocked<4096, true>(4095, 4095) == blocked_at(4096, 4095, 4095, true), "blocked<N, H16> is blocked_at");
static_assert(map_part_a((size_t)0, 17) == MAP_PATCH_BYTES + MAP_A_STRIDE, "part A number 17 is texel 1 of patch 1");

namespace
{
  bool supported(int N) { return N == 64 || N == 128 || N == 256 || N == 512 || N == 1024 || N == 2048 || N == 4096; }

  template<int LAYOUT>
  void shifts(int N, int64_t *a, int64_t *b)
  {
    TexelIndex<LAYOUT> const texel(N);

    for(int y = 0; y < N; ++y)
    {
      for(int x = 0; x < N; ++x)
      {
        int const oa = texel.column(x) + texel.row(y);

        a[(size_t)y * N + x] = oa;
        b[(size_t)y * N + x] = oa + MAP_PART_B - texel.bcolumn(x) - texel.brow(y);      // as ocean_gen.hip and ocean_surface.hip form it
      }
    }
  }
}

extern "C"
{

// the named numbers of the map layout and the work spectrum at N
int layout_constants(int N, int64_t *out)
{
  if (!supported(N))
    return 1;

  out[0] = (int64_t)map_cascade_bytes(N);
  out[1] = map_patch_cols(N);
  out[2] = map_patch_rows(N);
  out[3] = band_cols(N);
  out[4] = MAP_TEXEL_BYTES;
  out[5] = MAP_PATCH_BYTES;
  out[6] = MAP_PART_B;
  out[7] = MAP_A_STRIDE;
  out[8] = MAP_B_STRIDE;
  out[9] = MAP_PATCH;
  out[10] = map_compact_patchrow_bytes(N);
  out[11] = SBR;
  out[12] = spec_block_cols(false);
  out[13] = spec_block_cols(true);

  return 0;
}

// map_compact_a / map_compact_b of every texel, [y][x]
int layout_map_forward(int N, int64_t *a, int64_t *b, int64_t *patch, int32_t *j)
{
  if (!supported(N))
    return 1;

  for(int y = 0; y < N; ++y)
  {
    for(int x = 0; x < N; ++x)
    {
      a[(size_t)y * N + x] = (int64_t)map_compact_a(N, y, x);
      b[(size_t)y * N + x] = (int64_t)map_compact_b(N, y, x);
      patch[(size_t)y * N + x] = (int64_t)map_compact_patch(N, y, x);
      j[(size_t)y * N + x] = map_compact_j(N, y, x);
    }
  }

  return 0;
}

// the same two offsets through TexelIndex, in the layout gen_layout(N) picks (returned in *layout)
int layout_map_shifts(int N, int64_t *a, int64_t *b, int *layout)
{
  if (!supported(N))
    return 1;

  *layout = (int)gen_layout(N);

  switch(gen_layout(N))
  {
    case GEN_PLAIN: shifts<GEN_PLAIN>(N, a, b); break;
    default: shifts<GEN_BANDED>(N, a, b); break;
  }

  return 0;
}

// map_part of every part number r: its texel and the two offsets; a0[r] = map_part_a(0, r)
int layout_map_inverse(int N, int32_t *y, int32_t *x, int64_t *a, int64_t *b, int64_t *a0)
{
  if (!supported(N))
    return 1;

  PackShape const sh = pack_shape(N);

  for(size_t r = 0; r < (size_t)N * N; ++r)
  {
    MapPart const m = map_part(sh, r);

    y[r] = m.y;
    x[r] = m.x;
    a[r] = (int64_t)m.a;
    b[r] = (int64_t)m.b;
    a0[r] = (int64_t)map_part_a((size_t)0, r);
  }

  return 0;
}

// blocked_at of every grid point, [y][x]
int layout_blocked(int N, int half, int64_t *at)
{
  if (!supported(N))
    return 1;

  for(int y = 0; y < N; ++y)
    for(int x = 0; x < N; ++x)
      at[(size_t)y * N + x] = (int64_t)blocked_at(N, y, x, half != 0);

  return 0;
}

}
