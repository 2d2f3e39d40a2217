// ocean_gen_tile.inc -- the head of a mesh kernel (ocean_gen.hip), included as text by ocean_gen_kernel and ocean_gen_blend_kernel
// (ocean_blend.hip): which tile this workgroup owns, which rows this wave, which columns this thread.  Text, not a function: the kernel
// keeps its registers only as one function over local arrays (ocean_gen.hip, "the kernel").
// In scope before: GenArgs const &g; constexpr int PH; template parameter LAYOUT.
// Leaves: p, f, tid, lane, wave, tile, tilex, tiley, x0, ywave, xa, ip, texel, nmask.  Returns from the kernel for a padding workgroup.

    datum_ocean_set const &p = g.set;
    GenFrame const &f = g.frame;

    int const tid = threadIdx.x;
    int const lane = tid & 63;
    int const wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // Workgroup b runs on XCD b % 8.  A map that does not fit an XCD's 4 MB L2 is sampled in chunks of whole tile rows
    // dealt to the XCDs in turn: neighbouring tiles share an L2 (1024^2 maps: 36.4 -> 31.0 us), and every XCD gets its
    // share of the cheap rows above the horizon (one contiguous run of tiles per XCD: 43 us).  Small maps sit in every
    // L2 anyway; there the launch order is kept (64^2 maps: 16.5 against 17.1 us).
    int tile = (int)blockIdx.x + g.block0;

    if (g.chunk)
    {
      int const slot = tile >> 3;

      tile = ((slot / g.chunk) * 8 + (tile & 7)) * g.chunk + slot % g.chunk;

      if (tile >= g.tiles)
        return;
    }

    int const tilex = tile % g.tilesx, tiley = tile / g.tilesx;

    int const x0 = tilex * GEN_TILE_X;
    int const ywave = tiley * GEN_TILE_Y + 4 * PH * wave;          // first of this wave's 4 * PH rows

    int const xa = x0 + (lane & 15);

    float const *ip = p.invproj;

    TexelIndex<LAYOUT> const texel(g.N);

    int const nmask = g.N - 1;
