// ocean_gen_texel.inc -- the texel addressing of a mesh kernel (ocean_gen.hip), included as text by ocean_gen_kernel and, once per
// cascade, by ocean_gen_blend_kernel (ocean_blend.hip): texture(sampler2DArray, REPEAT, linear, lod 0) of both layers at
// (position.xy * scale), texel centres at (i + 0.5) / N -- the weights, the fract wrap, the byte offsets of the four corners in the map
// layout, zero-weight corners pushed out of the buffer.
// In scope before: ocean_gen_tile.inc's names; ph; position[ph]; OCEAN_GEN_TEXEL_SCALE, the cascade's texcoord scale (1 / wavescale);
// v2 w00[PH] .. w11[PH]; int o00[PH][2] .. o11[PH][2], q00[PH][2] .. q11[PH][2]; bool near[PH].
// Leaves: those, near[ph] wave-uniform.

      v2 const fx = (position[ph].x * OCEAN_GEN_TEXEL_SCALE) * f.fn - 0.5f;
      v2 const fy = (position[ph].y * OCEAN_GEN_TEXEL_SCALE) * f.fn - 0.5f;

      v2 const flx = pfloor(fx), fly = pfloor(fy);

      v2 const ax = fx - flx, ay = fy - fly;

      // floor(coordinate) mod N: N is a power of two, so coordinate / N, its fractional part and the product with N are exact
      v2 const wx = flx * f.rfn, wy = fly * f.rfn;
      v2 const mx = v2{ __builtin_amdgcn_fractf(wx.x), __builtin_amdgcn_fractf(wx.y) } * f.fn;
      v2 const my = v2{ __builtin_amdgcn_fractf(wy.x), __builtin_amdgcn_fractf(wy.y) } * f.fn;

      v2 const bx = 1.0f - ax, by = 1.0f - ay;

      w00[ph] = bx * by; w10[ph] = ax * by; w01[ph] = bx * ay; w11[ph] = ax * ay;

      near[ph] = false;                        // some weight other than w00 is not zero

      #pragma unroll
      for(int i = 0; i < 2; ++i)
      {
        int const i0 = (int)mx[i], j0 = (int)my[i];

        int const i1 = (i0 + 1) & nmask, j1 = (j0 + 1) & nmask;

        int const c0 = texel.column(i0), c1 = texel.column(i1);
        int const r0 = texel.row(j0), r1 = texel.row(j1);

        // A zero weight along an axis (beyond |coordinate| = 2^23 texels: every ray above the horizon): the second texel of
        // that axis is not needed (0 * finite adds nothing).  Its offset is pushed out of the buffer's range: zeros come
        // back without a memory access, and no branch -- hence no wait -- separates the fetches.
        bool const wantx = ax[i] != 0.0f, wanty = ay[i] != 0.0f;

        o00[ph][i] = r0 + c0; o10[ph][i] = wantx ? r0 + c1 : -256; o01[ph][i] = wanty ? r1 + c0 : -256; o11[ph][i] = (wantx && wanty) ? r1 + c1 : -256;

        int const bc0 = texel.bcolumn(i0), bc1 = texel.bcolumn(i1);
        int const br0 = MAP_PART_B - texel.brow(j0), br1 = MAP_PART_B - texel.brow(j1);

        q00[ph][i] = o00[ph][i] + br0 - bc0; q10[ph][i] = wantx ? o10[ph][i] + br0 - bc1 : -256; q01[ph][i] = wanty ? o01[ph][i] + br1 - bc0 : -256; q11[ph][i] = (wantx && wanty) ? o11[ph][i] + br1 - bc1 : -256;

        near[ph] = near[ph] || wantx || wanty;
      }

      near[ph] = __builtin_amdgcn_ballot_w64(near[ph]) != 0;
