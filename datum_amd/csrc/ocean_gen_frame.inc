// ocean_gen_frame.inc -- the shading frame of a mesh kernel (ocean_gen.hip, gen.comp:101-120), included as text by ocean_gen_kernel and
// ocean_gen_blend_kernel (ocean_blend.hip): the Gerstner frame times the sampled normal, mixed towards the plane normal.
// In scope before: f, ph, st[ph], ct[ph], smoothing[ph]; p3 const dn (displacementnormal), p3 const planen; p3 tbn2.
// Leaves: tbn2.

        // tbn[2] = normalize(-normal.xy, 1 - normal.z), tbn[0] = normalize(1 - tangent.x, -tangent.y, tangent.z), tbn[1] = tbn[0] x tbn[2]
        p3 const t2 = normalize3(p3{ -f.nx * ct[ph], -f.ny * ct[ph], pfma(-f.nz, st[ph], 1.0f) });
        p3 const t0 = normalize3(p3{ pfma(-f.tx, st[ph], 1.0f), -f.ty * st[ph], f.tz * ct[ph] });
        p3 const t1 = { t0.y * t2.z - t0.z * t2.y, t0.z * t2.x - t0.x * t2.z, t0.x * t2.y - t0.y * t2.x };

        // tbn * displacementnormal, mixed towards the plane normal with the distance smoothing
        p3 const tn = { pfma(dn.z, t2.x, pfma(dn.y, t1.x, dn.x * t0.x)), pfma(dn.z, t2.y, pfma(dn.y, t1.y, dn.x * t0.y)), pfma(dn.z, t2.z, pfma(dn.y, t1.z, dn.x * t0.z)) };

        v2 const keep = 1.0f - smoothing[ph];

        tbn2 = normalize3(p3{ pfma(keep, tn.x, smoothing[ph] * planen.x), pfma(keep, tn.y, smoothing[ph] * planen.y), pfma(keep, tn.z, smoothing[ph] * planen.z) });
