// ocean_gen_cascades.inc -- one listed cascade's share of a several-cascade mesh kernel, included as text inside the loop over the list by
// ocean_gen_blend_kernel (ocean_blend.hip) and ocean_gen_blend_rippled_kernel (ocean_rippled.hip): gen's three fetch patterns, its blend,
// the displacement summed in list order and the normal as slopes.
// In scope before: ocean_gen_texel.inc's names for this cascade (w00 .. w11, o00 .. o11, q00 .. q11, near) and the corner registers a00 .. a11,
// b00 .. b11; rmap; c; ph; bool const shaded; p3 displacement; v2 slopex, slopey.
// Leaves: displacement, slopex, slopey with this cascade added.

      // gen's three fetch patterns (ocean_gen.hip), the normal right behind its displacement, and gen's blend
      // w11 a11 + (w01 a01 + (w10 a10 + w00 a00)) in FMAs, each pattern blended where it is fetched: only the cascade's sample leaves the branch
      #define OCEAN_GEN_FETCH_A(C) a##C[ph][i] = buf_load_f32x4_aux<0>(rmap, o##C[ph][i], 0)
      #define OCEAN_GEN_FETCH_B(C) b##C[ph][i] = GenNormal::load(rmap, q##C[ph][i])
      #define OCEAN_GEN_BLEND(T, C) pfma(w11[ph], v2{ T##11[ph][0].C, T##11[ph][1].C }, pfma(w01[ph], v2{ T##01[ph][0].C, T##01[ph][1].C }, pfma(w10[ph], v2{ T##10[ph][0].C, T##10[ph][1].C }, w00[ph] * v2{ T##00[ph][0].C, T##00[ph][1].C })))
      #define OCEAN_GEN_BLENDN(F) pfma(w11[ph], v2{ F(a11[ph][0], b11[ph][0]), F(a11[ph][1], b11[ph][1]) }, pfma(w01[ph], v2{ F(a01[ph][0], b01[ph][0]), F(a01[ph][1], b01[ph][1]) }, pfma(w10[ph], v2{ F(a10[ph][0], b10[ph][0]), F(a10[ph][1], b10[ph][1]) }, w00[ph] * v2{ F(a00[ph][0], b00[ph][0]), F(a00[ph][1], b00[ph][1]) })))

      p3 d;

      if (shaded)
      {
        #pragma unroll
        for(int i = 0; i < 2; ++i)
        {
          OCEAN_GEN_FETCH_A(00); OCEAN_GEN_FETCH_B(00);
          OCEAN_GEN_FETCH_A(10); OCEAN_GEN_FETCH_B(10);
          OCEAN_GEN_FETCH_A(01); OCEAN_GEN_FETCH_B(01);
          OCEAN_GEN_FETCH_A(11); OCEAN_GEN_FETCH_B(11);
        }

        d = { OCEAN_GEN_BLEND(a, x), OCEAN_GEN_BLEND(a, y), OCEAN_GEN_BLEND(a, z) };

        v2 const mx_ = OCEAN_GEN_BLENDN(GenNormal::x), my_ = OCEAN_GEN_BLENDN(GenNormal::y), mz_ = OCEAN_GEN_BLENDN(GenNormal::z);

        // slopes add, unit normals do not: m.z > 0 in every texel (v_rcp_f32, 1 ulp: the shading frame amplifies nothing)
        v2 const rz = prcp(mz_);

        slopex = pfma(mx_, rz, slopex);
        slopey = pfma(my_, rz, slopey);
      }
      else if (near[ph])
      {
        #pragma unroll
        for(int i = 0; i < 2; ++i)
        {
          OCEAN_GEN_FETCH_A(00);
          OCEAN_GEN_FETCH_A(10);
          OCEAN_GEN_FETCH_A(01);
          OCEAN_GEN_FETCH_A(11);
        }

        d = { OCEAN_GEN_BLEND(a, x), OCEAN_GEN_BLEND(a, y), OCEAN_GEN_BLEND(a, z) };
      }
      else
      {
        // every ray of the wave is beyond 2^23 texels of this cascade along both axes: one texel per vertex, its weight (1 - 0) * (1 - 0)
        #pragma unroll
        for(int i = 0; i < 2; ++i)
          OCEAN_GEN_FETCH_A(00);

        d = { w00[ph] * v2{ a00[ph][0].x, a00[ph][1].x }, w00[ph] * v2{ a00[ph][0].y, a00[ph][1].y }, w00[ph] * v2{ a00[ph][0].z, a00[ph][1].z } };
      }

      #undef OCEAN_GEN_FETCH_A
      #undef OCEAN_GEN_FETCH_B
      #undef OCEAN_GEN_BLEND
      #undef OCEAN_GEN_BLENDN

      // the first cascade as it is (a one-element list gives gen's bits), each further one added: one rounding per component
      if (c == 0)
        displacement = d;
      else
        displacement = { displacement.x + d.x, displacement.y + d.y, displacement.z + d.z };
