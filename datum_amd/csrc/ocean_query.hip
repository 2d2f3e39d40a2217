// ocean_query.hip -- one point of the several-cascade surface query (include/datum_ocean_hip.h: datum_ocean_sample_surface_blend), stated
// once for every kernel that asks the summed surface something: the blended sample (ocean_blend.hip), body buoyancy (ocean_body.hip), the
// ray casts (ocean_ray.hip, ocean_bounds.hip) and the velocity query (ocean_velocity.hip).
//
//   * QueryArgs is what they all pass: the set and its frame, the cascade list, N and the iterations;
//   * query_solve: `iterations` updates b <- b + (q - V(b).xy) from b = q, V(b) summed over the list in list order (the first cascade
//     taken as it is, one fp32 addition per component for each further one), then the swell terms of the final evaluation at b;
//   * QueryCorners: one cascade at one position -- the resource over its map, gen's REPEAT bilinear fetch (SurfaceTexel) and part A of
//     the four corners.  Nothing else in the five kernels makes a SurfaceTexel or loads from a map;
//   * three final evaluations over it: query_height (part A alone: what a ray's search needs), query_record (parts A and B and the foam
//     planes: the record's eight fields; query_sums is its loop and query_finish what follows it, so that the rippled record of
//     ocean_rippled.hip puts the layer's slopes between the two) and query_velocity (part A and the velocity planes).  Each is the same operations in the same
//     order on what it shares with the others, so a height has the record's bits;
//   * query_each_point: the prologue of the one-point-per-thread kernels.
// Every fetch goes through a buffer resource sized to what it reads; a zero bilinear weight pushes its corner out of range (-256).

#pragma once

#include "ocean_surface.hip"

namespace ocean
{
  struct BlendCascade
  {
    float4 const *map;      // the cascade's displacement map, map_cascade_bytes(N) bytes
    float const *foam;      // the cascade's foam plane, N * N floats; nullptr while foam is OFF
    float scale;            // the handle's 1 / wavescale of the cascade
    int pad;
  };

  struct BlendList
  {
    int count;
    int foammode;           // DATUM_OCEAN_FOAM_*: how the queries combine the planes
    BlendCascade casc[DATUM_OCEAN_MAX_CASCADES];
  };

  struct QueryArgs
  {
    datum_ocean_set set;    // set.scale is not read: every cascade has its own in the list
    GenFrame frame;         // query_frame
    BlendList list;
    int N;
    int iterations;
  };

  // set and N filled in; every launch_* of a query calls it
  inline void query_frame(QueryArgs &a)
  {
    a.frame = make_gen_frame(a.set, a.N, 2, 2);      // the camera's terms are not read
  }

  // the final base point b: sin and cos of its swell phase and P(b).xy
  struct QueryBase
  {
    float st, ct, px, py;
  };

  // a sample as it is stored
  struct QueryRecord
  {
    float4 v;               // V(b).xyz, |V(b).xy - q|
    float4 m;               // query_record: the shading normal, the foam; query_velocity: the summed velocity, 0
  };

  template<int LAYOUT>
  struct QueryCorners
  {
    TexelIndex<LAYOUT> texel;
    __amdgpu_buffer_rsrc_t rmap;
    SurfaceTexel<LAYOUT> t;
    float4 a00, a10, a01, a11;

    __device__ __forceinline__ QueryCorners(QueryArgs const &a, BlendCascade const &bc, float px, float py)
      : texel(a.N), rmap(make_rsrc(bc.map, map_cascade_bytes(a.N))), t(texel, a.frame, bc.scale, a.N - 1, px, py)
    {
      a00 = buf_load_f32x4_aux<0>(rmap, t.o00, 0);
      a10 = buf_load_f32x4_aux<0>(rmap, t.o10, 0);
      a01 = buf_load_f32x4_aux<0>(rmap, t.o01, 0);
      a11 = buf_load_f32x4_aux<0>(rmap, t.o11, 0);
    }

    __device__ __forceinline__ float x() const { return t.blend(a00.x, a10.x, a01.x, a11.x); }
    __device__ __forceinline__ float y() const { return t.blend(a00.y, a10.y, a01.y, a11.y); }
    __device__ __forceinline__ float z() const { return t.blend(a00.z, a10.z, a01.z, a11.z); }
    __device__ __forceinline__ float w() const { return t.blend(a00.w, a10.w, a01.w, a11.w); }

    // a row-major plane of N * N elements of BYTES bytes at the corners' texels: the byte offsets, a zero-weight corner out of range
    template<int BYTES>
    __device__ __forceinline__ void plane(int &p00, int &p10, int &p01, int &p11) const
    {
      p00 = ((t.j0 << texel.ln) + t.i0) * BYTES;
      p10 = t.wantx ? ((t.j0 << texel.ln) + t.i1) * BYTES : -256;
      p01 = t.wanty ? ((t.j1 << texel.ln) + t.i0) * BYTES : -256;
      p11 = (t.wantx && t.wanty) ? ((t.j1 << texel.ln) + t.i1) * BYTES : -256;
    }
  };

  // the sum over the list: the first cascade as it is (a one-element list gives that cascade's bits), each further one added
  __device__ __forceinline__ float query_sum(int c, float sum, float x)
  {
    return (c == 0) ? x : sum + x;
  }

  __device__ __forceinline__ QueryBase query_base(QueryArgs const &a, float bx, float by)
  {
    datum_ocean_set const &p = a.set;
    GenFrame const &f = a.frame;

    float const theta = f.frequency * (p.swelldirection[0] * bx + p.swelldirection[1] * by) + p.swellphase;

    QueryBase b;

    sincos_phase(theta, &b.st, &b.ct);

    b.px = bx + f.gx * b.ct;
    b.py = by + f.gy * b.ct;

    return b;
  }

  template<int LAYOUT>
  __device__ __forceinline__ QueryBase query_solve(QueryArgs const &a, float2 q)
  {
    float bx = q.x, by = q.y;

    // the updates b <- b + (q - V(b).xy): part A of every listed cascade's four corners, D.xy summed in list order
    for(int it = 0; it < a.iterations; ++it)
    {
      QueryBase const b = query_base(a, bx, by);

      float dx = 0.0f, dy = 0.0f;

      for(int c = 0; c < a.list.count; ++c)
      {
        QueryCorners<LAYOUT> const k(a, a.list.casc[c], b.px, b.py);

        dx = query_sum(c, dx, k.x());
        dy = query_sum(c, dy, k.y());
      }

      float const vx = b.px - dx;
      float const vy = b.py - dy;

      bx = bx + (q.x - vx);
      by = by + (q.y - vy);
    }

    return query_base(a, bx, by);
  }

  // V(b) from the summed displacement, and the distance of V(b).xy from q
  __device__ __forceinline__ float4 query_position(QueryArgs const &a, QueryBase const &b, float2 q, float dx, float dy, float dz)
  {
    float const vx = b.px - dx, vy = b.py - dy, vz = (a.frame.basez + a.set.swellamplitude * b.st) + dz;

    float const rx = vx - q.x, ry = vy - q.y;

    return make_float4(vx, vy, vz, __builtin_sqrtf(fmaf(ry, ry, rx * rx)));
  }

  // gen's frame m.x t0 + m.y t1 + m.z t2 normalised (ocean_surface.hip, gen.comp:101-120 with smoothing = 0), for dn = normalize(sx, sy, 1)
  __device__ __forceinline__ void blend_surface_normal(GenFrame const &f, float st, float ct, float sx, float sy, float &mx, float &my, float &mz)
  {
    float nx = sx, ny = sy, nz = 1.0f;

    normalize3(nx, ny, nz);

    float t2x = -f.nx * ct, t2y = -f.ny * ct, t2z = fmaf(-f.nz, st, 1.0f);
    float t0x = fmaf(-f.tx, st, 1.0f), t0y = -f.ty * st, t0z = f.tz * ct;

    normalize3(t2x, t2y, t2z);
    normalize3(t0x, t0y, t0z);

    float const t1x = t0y * t2z - t0z * t2y, t1y = t0z * t2x - t0x * t2z, t1z = t0x * t2y - t0y * t2x;

    mx = fmaf(nz, t2x, fmaf(ny, t1x, nx * t0x));
    my = fmaf(nz, t2y, fmaf(ny, t1y, nx * t0y));
    mz = fmaf(nz, t2z, fmaf(ny, t1z, nx * t0z));

    normalize3(mx, my, mz);
  }

  // V(b).z alone, the record's bits: parts B and the foam planes are not fetched
  template<int LAYOUT>
  __device__ __forceinline__ float query_height(QueryArgs const &a, QueryBase const &b)
  {
    float dz = 0.0f;

    for(int c = 0; c < a.list.count; ++c)
    {
      QueryCorners<LAYOUT> const k(a, a.list.casc[c], b.px, b.py);

      dz = query_sum(c, dz, k.z());
    }

    return (a.frame.basez + a.set.swellamplitude * b.st) + dz;
  }

  // the record's sums over the list: the displacement, the slopes (m.x / m.z, m.y / m.z) and the foam as the record stores it
  struct QuerySums
  {
    float dx, dy, dz, sx, sy, foam;
  };

  // parts A and B and the foam plane of every listed cascade: the one loop behind every record
  template<int LAYOUT>
  __device__ __forceinline__ QuerySums query_sums(QueryArgs const &a, QueryBase const &b)
  {
    float dx = 0.0f, dy = 0.0f, dz = 0.0f, sx = 0.0f, sy = 0.0f, foam = 0.0f;

    for(int c = 0; c < a.list.count; ++c)
    {
      BlendCascade const &bc = a.list.casc[c];

      QueryCorners<LAYOUT> const k(a, bc, b.px, b.py);

      SurfaceTexel<LAYOUT> const &t = k.t;

      int const bc0 = k.texel.bcolumn(t.i0), bc1 = k.texel.bcolumn(t.i1);
      int const br0 = MAP_PART_B - k.texel.brow(t.j0), br1 = MAP_PART_B - k.texel.brow(t.j1);

      float2 const b00 = buf_load_f32x2(k.rmap, t.o00 + br0 - bc0, 0);
      float2 const b10 = buf_load_f32x2(k.rmap, t.wantx ? t.o10 + br0 - bc1 : -256, 0);
      float2 const b01 = buf_load_f32x2(k.rmap, t.wanty ? t.o01 + br1 - bc0 : -256, 0);
      float2 const b11 = buf_load_f32x2(k.rmap, (t.wantx && t.wanty) ? t.o11 + br1 - bc1 : -256, 0);

      if (bc.foam)
      {
        __amdgpu_buffer_rsrc_t const rfoam = make_rsrc(bc.foam, (size_t)a.N * a.N * sizeof(float));

        int p00, p10, p01, p11;

        k.template plane<4>(p00, p10, p01, p11);

        float const g00 = buf_load_f32(rfoam, p00, 0);
        float const g10 = buf_load_f32(rfoam, p10, 0);
        float const g01 = buf_load_f32(rfoam, p01, 0);
        float const g11 = buf_load_f32(rfoam, p11, 0);

        float const fc = t.blend(g00, g10, g01, g11);

        // ACCUMULATE: the largest coverage; JACOBIAN: 1 + sum (J_c - 1), the summed displacement's Jacobian without the cross terms
        if (a.list.foammode == DATUM_OCEAN_FOAM_JACOBIAN)
          foam = foam + (fc - 1.0f);
        else
          foam = (c == 0) ? fc : fmaxf(foam, fc);
      }

      dx = query_sum(c, dx, k.x());
      dy = query_sum(c, dy, k.y());
      dz = query_sum(c, dz, k.z());

      // slopes add, unit normals do not (ocean_blend.hip)
      float const nx = k.w();
      float const ny = t.blend(b00.x, b10.x, b01.x, b11.x);
      float const nz = t.blend(b00.y, b10.y, b01.y, b11.y);

      float const rz = __builtin_amdgcn_rcpf(nz);

      sx = fmaf(nx, rz, sx);
      sy = fmaf(ny, rz, sy);
    }

    if (a.list.foammode == DATUM_OCEAN_FOAM_JACOBIAN)
      foam = 1.0f + foam;

    return QuerySums{ dx, dy, dz, sx, sy, foam };
  }

  // the record of the sums: V(b) and the residual, the shading normal of the summed slopes, the foam
  __device__ __forceinline__ QueryRecord query_finish(QueryArgs const &a, QueryBase const &b, float2 q, QuerySums const &s)
  {
    QueryRecord r;

    r.v = query_position(a, b, q, s.dx, s.dy, s.dz);

    blend_surface_normal(a.frame, b.st, b.ct, s.sx, s.sy, r.m.x, r.m.y, r.m.z);

    r.m.w = s.foam;

    return r;
  }

  // the record: parts A and B and the foam plane of every listed cascade
  template<int LAYOUT>
  __device__ __forceinline__ QueryRecord query_record(QueryArgs const &a, QueryBase const &b, float2 q)
  {
    return query_finish(a, b, q, query_sums<LAYOUT>(a, b));
  }

  // the record's first half, and the listed cascades' velocity planes (`vel`, in list order) sampled with the same fetch and summed in
  // list order; parts B and the foam planes are not fetched
  template<int LAYOUT>
  __device__ __forceinline__ QueryRecord query_velocity(QueryArgs const &a, QueryBase const &b, float2 q, float4 const *const *vel)
  {
    float dx = 0.0f, dy = 0.0f, dz = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f;

    for(int c = 0; c < a.list.count; ++c)
    {
      __amdgpu_buffer_rsrc_t const rvel = make_rsrc(vel[c], (size_t)a.N * a.N * sizeof(float4));

      QueryCorners<LAYOUT> const k(a, a.list.casc[c], b.px, b.py);

      int p00, p10, p01, p11;

      k.template plane<16>(p00, p10, p01, p11);

      float4 const u00 = buf_load_f32x4_aux<0>(rvel, p00, 0);
      float4 const u10 = buf_load_f32x4_aux<0>(rvel, p10, 0);
      float4 const u01 = buf_load_f32x4_aux<0>(rvel, p01, 0);
      float4 const u11 = buf_load_f32x4_aux<0>(rvel, p11, 0);

      dx = query_sum(c, dx, k.x());
      dy = query_sum(c, dy, k.y());
      dz = query_sum(c, dz, k.z());

      ux = query_sum(c, ux, k.t.blend(u00.x, u10.x, u01.x, u11.x));
      uy = query_sum(c, uy, k.t.blend(u00.y, u10.y, u01.y, u11.y));
      uz = query_sum(c, uz, k.t.blend(u00.z, u10.z, u01.z, u11.z));
    }

    QueryRecord r;

    r.v = query_position(a, b, q, dx, dy, dz);
    r.m = make_float4(ux, uy, uz, 0.0f);

    return r;
  }

  // one point per thread: thread k of the grid takes points[k] and writes samples[2k], samples[2k + 1] -- the QueryRecord `record` returns
  // for a finite point, quiet NaNs for any other
  template<class Record>
  __device__ __forceinline__ void query_each_point(float2 const *points, float4 *samples, int count, Record &&record)
  {
    int const k = (int)blockIdx.x * SURFACE_THREADS + (int)threadIdx.x;

    if (k >= count)
      return;

    float2 const q = points[k];

    float4 *out = samples + 2 * (size_t)k;

    if (!__builtin_isfinite(q.x) || !__builtin_isfinite(q.y))
    {
      float const nan = __builtin_nanf("");

      out[0] = make_float4(nan, nan, nan, nan);
      out[1] = make_float4(nan, nan, nan, nan);
      return;
    }

    QueryRecord const r = record(q);

    out[0] = r.v;
    out[1] = r.m;
  }
}
