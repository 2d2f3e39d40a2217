// ocean_gen_ray.inc -- the ray stage of a mesh kernel (ocean_gen.hip), included as text by ocean_gen_kernel and ocean_gen_blend_kernel
// (ocean_blend.hip): view ray, plane hit, swell phase, position before the displacement, distance smoothing (gen.comp:81-99,116).
// In scope before: ocean_gen_tile.inc's names; ph; p3 position[PH]; v2 smoothing[PH], st[PH], ct[PH].
// Leaves: position[ph], st[ph], ct[ph], smoothing[ph] (and the stage's locals: yy, xx, u, v, viewvec, len, rlen, worlddir, costheta, hit,
// dist, basex, basey, theta, cl).

      int const yy = ywave + 4 * ph + (lane >> 4);

      //-- view ray, plane hit, swell phase: the shader's expressions and roundings (gen.comp:81-99) ----------------

      v2 const xx = { (float)xa, (float)(xa + 16) };

      v2 const u = (div_exact(2.0f * xx, splat(f.sxm1)) - 1.0f) * f.margin;

      // (one row per thread: its v is the first half of a packed division whose second half repeats it)
      float const v = ((1.0f - div_exact(splat(2.0f * (float)yy), splat(f.sym1))) * f.margin).x;

      p3 viewvec = { ((ip[0] * u + ip[1] * v) + f.viewz[0]) + f.vieww[0],
                     ((ip[4] * u + ip[5] * v) + f.viewz[1]) + f.vieww[1],
                     ((ip[8] * u + ip[9] * v) + f.viewz[2]) + f.vieww[2] };

      v2 const len = sqrt_exact(dot3(viewvec, viewvec));
      v2 const rlen = refined_rcp(len);

      p3 const worlddir = rotate(p.camera_real, p3{ div_exact(viewvec.x, len, rlen), div_exact(viewvec.y, len, rlen), div_exact(viewvec.z, len, rlen) });

      v2 const costheta = worlddir.x * f.negplane[0] + worlddir.y * f.negplane[1] + worlddir.z * f.negplane[2];

      v2 const hit = div_exact(splat(f.cameraheight), costheta);

      v2 const dist = { (costheta.x > 0) ? hit.x : 1e6f, (costheta.y > 0) ? hit.y : 1e6f };

      v2 const basex = f.camerapos[0] + dist * worlddir.x;
      v2 const basey = f.camerapos[1] + dist * worlddir.y;

      v2 const theta = f.frequency * (p.swelldirection[0] * basex + p.swelldirection[1] * basey) + p.swellphase;

      // (ocean_phase.h, no copy here: always the software form -- the swell phase reaches 1e5 .. 1e6 at the horizon, far outside
      // v_sin_f32's domain -- and pinned against float64 up to |x| = 2^21 by tests/test_gen64.py)
      sincos_phase_pair_poly(theta, st[ph], ct[ph]);

      position[ph] = { basex + f.gx * ct[ph], basey + f.gy * ct[ph], f.basez + p.swellamplitude * st[ph] };

      v2 cl = dist * p.smoothing - 0.35f;

      #pragma unroll
      for(int i = 0; i < 2; ++i)       // pow(clamp(cl, 0, 1), 0.2): 0 -> 0, 1 -> 1 exactly
        smoothing[ph][i] = __builtin_amdgcn_exp2f(0.2f * __builtin_amdgcn_logf(__builtin_amdgcn_fmed3f(cl[i], 0.0f, 1.0f)));
