// ocean_gen_store.inc -- the tail of a mesh kernel (ocean_gen.hip), included as text by ocean_gen_kernel, ocean_gen_blend_kernel
// (ocean_blend.hip) and ocean_gen_blend_rippled_kernel (ocean_rippled.hip): the tangent, the vertex and its way through LDS into the mesh.
// In scope before: ocean_gen_tile.inc's names; ph; position[ph]; p3 displacement, tbn2; float4 *mine (the wave's 6 KB of LDS).

      // tbn[0] = normalize((1, 0, 0) - tbn[2].x * tbn[2])
      p3 const tbn0 = normalize3(p3{ pfma(-tbn2.x, tbn2.x, 1.0f), -tbn2.x * tbn2.y, -tbn2.x * tbn2.z });

      OCEAN_STAMP(3);

      //-- Mesh::Vertex { position3, texcoord2, normal3, tangent4 } = 48 bytes (src/renderer/mesh.h:20-26) -----------
      // The wave's 4 rows x 32 vertices = 4 x 96 float4 go through its 6 KB of LDS: lane i then stores float4 number
      // i, 64 + i, ... 320 + i of the wave's 384 (three 16-byte stores per vertex at a 48-byte stride touch every line three times).

      // (OCEAN_GEN_STORE_LIFT, where the including kernel defines it: a v2 added to the finished height, one more fp32 addition)
#ifdef OCEAN_GEN_STORE_LIFT
      v2 const px = position[ph].x - displacement.x, py = position[ph].y - displacement.y, pz = (position[ph].z + displacement.z) + OCEAN_GEN_STORE_LIFT;
#else
      v2 const px = position[ph].x - displacement.x, py = position[ph].y - displacement.y, pz = position[ph].z + displacement.z;
#endif
      v2 const tu = 0.1f * position[ph].x, tv = 0.1f * position[ph].y;

      #pragma unroll
      for(int i = 0; i < 2; ++i)
      {
        float4 *vtx = mine + 3 * ((lane >> 4) * 32 + 16 * i + (lane & 15));

        vtx[0] = make_float4(px[i], py[i], pz[i], tu[i]);
        vtx[1] = make_float4(tv[i], tbn2.x[i], tbn2.y[i], tbn2.z[i]);
        vtx[2] = make_float4(tbn0.x[i], tbn0.y[i], tbn0.z[i], -1.0f);
      }

      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

      int const y0 = ywave + 4 * ph;
      int const rowlen = min(GEN_TILE_X, g.sizex - x0) * 3;                                // float4 of this tile in one mesh row

      // (the wave's part of the address is uniform: a scalar base and a 32-bit offset per lane)
      float4 *out = reinterpret_cast<float4*>(g.vertices) + ((size_t)y0 * g.sizex + x0) * 3;

      #pragma unroll
      for(int k = 0; k < 6; ++k)
      {
        int const j = 64 * k + lane;
        int const r = j / 96, c = j % 96;

        if (c < rowlen && y0 + r < g.sizey)
          store_vertex_float4(out + (unsigned)(r * g.sizex * 3 + c), mine[j]);
      }
