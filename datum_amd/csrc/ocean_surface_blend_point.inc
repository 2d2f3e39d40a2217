// ocean_surface_blend_point.inc -- one point of the several-cascade surface query (include/datum_ocean_hip.h: datum_ocean_sample_surface_blend),
// the text ocean_surface_blend_kernel and ocean_body_kernel share as gen's stages are shared: `iterations` updates b <- b + (q - V(b).xy)
// from b = q, then the final evaluation at b.
//   in scope: SurfaceArgs const &s (N, iterations), datum_ocean_set const &p, GenFrame const &f, BlendList const &list, float2 q (finite)
//   leaves:   vx, vy, vz, residual, mx, my, mz, foam -- the record's eight fields
// With OCEAN_SURFACE_BLEND_POINT_HEIGHT defined by the includer (ocean_ray.hip's search) the final evaluation keeps to part A and leaves vz
// alone, the same operations in the same order: the height has the record's bits, parts B and the foam planes are not fetched.
// With OCEAN_SURFACE_BLEND_POINT_VELOCITY defined as the array of the listed cascades' velocity planes (ocean_velocity.hip) the final
// evaluation leaves vx, vy, vz and residual with the record's bits, and ux, uy, uz: the planes sampled at t_c with the same fetch, summed
// in list order; parts B and the foam planes are not fetched.
TexelIndex<LAYOUT> const texel(s.N);

int const nmask = s.N - 1;
int const count = list.count;

size_t const mapbytes = map_cascade_bytes(s.N);

float const dirx = p.swelldirection[0], diry = p.swelldirection[1];

float bx = q.x, by = q.y;

float st, ct, px, py;

// the updates b <- b + (q - V(b).xy): part A of every listed cascade's four corners, D.xy summed in list order
for(int it = 0; it < s.iterations; ++it)
{
  float const theta = f.frequency * (dirx * bx + diry * by) + p.swellphase;

  sincos_phase(theta, &st, &ct);

  px = bx + f.gx * ct;
  py = by + f.gy * ct;

  float dx = 0.0f, dy = 0.0f;

  for(int c = 0; c < count; ++c)
  {
    BlendCascade const &bc = list.casc[c];

    __amdgpu_buffer_rsrc_t const rmap = make_rsrc(bc.map, mapbytes);

    SurfaceTexel<LAYOUT> const t(texel, f, bc.scale, nmask, px, py);

    float4 const a00 = buf_load_f32x4_aux<0>(rmap, t.o00, 0);
    float4 const a10 = buf_load_f32x4_aux<0>(rmap, t.o10, 0);
    float4 const a01 = buf_load_f32x4_aux<0>(rmap, t.o01, 0);
    float4 const a11 = buf_load_f32x4_aux<0>(rmap, t.o11, 0);

    float const cx = t.blend(a00.x, a10.x, a01.x, a11.x);
    float const cy = t.blend(a00.y, a10.y, a01.y, a11.y);

    dx = (c == 0) ? cx : dx + cx;
    dy = (c == 0) ? cy : dy + cy;
  }

  float const vx = px - dx;
  float const vy = py - dy;

  bx = bx + (q.x - vx);
  by = by + (q.y - vy);
}

// the final evaluation at b: parts A and B and the foam plane of every listed cascade
float const theta = f.frequency * (dirx * bx + diry * by) + p.swellphase;

sincos_phase(theta, &st, &ct);

px = bx + f.gx * ct;
py = by + f.gy * ct;

#ifdef OCEAN_SURFACE_BLEND_POINT_HEIGHT

float dz = 0.0f;

for(int c = 0; c < count; ++c)
{
  BlendCascade const &bc = list.casc[c];

  __amdgpu_buffer_rsrc_t const rmap = make_rsrc(bc.map, mapbytes);

  SurfaceTexel<LAYOUT> const t(texel, f, bc.scale, nmask, px, py);

  float4 const a00 = buf_load_f32x4_aux<0>(rmap, t.o00, 0);
  float4 const a10 = buf_load_f32x4_aux<0>(rmap, t.o10, 0);
  float4 const a01 = buf_load_f32x4_aux<0>(rmap, t.o01, 0);
  float4 const a11 = buf_load_f32x4_aux<0>(rmap, t.o11, 0);

  float const cz = t.blend(a00.z, a10.z, a01.z, a11.z);

  dz = (c == 0) ? cz : dz + cz;
}

float const vz = (f.basez + p.swellamplitude * st) + dz;

#elif defined(OCEAN_SURFACE_BLEND_POINT_VELOCITY)

float dx = 0.0f, dy = 0.0f, dz = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f;

for(int c = 0; c < count; ++c)
{
  BlendCascade const &bc = list.casc[c];

  __amdgpu_buffer_rsrc_t const rmap = make_rsrc(bc.map, mapbytes);
  __amdgpu_buffer_rsrc_t const rvel = make_rsrc((OCEAN_SURFACE_BLEND_POINT_VELOCITY)[c], (size_t)s.N * s.N * sizeof(float4));

  SurfaceTexel<LAYOUT> const t(texel, f, bc.scale, nmask, px, py);

  float4 const a00 = buf_load_f32x4_aux<0>(rmap, t.o00, 0);
  float4 const a10 = buf_load_f32x4_aux<0>(rmap, t.o10, 0);
  float4 const a01 = buf_load_f32x4_aux<0>(rmap, t.o01, 0);
  float4 const a11 = buf_load_f32x4_aux<0>(rmap, t.o11, 0);

  float4 const u00 = buf_load_f32x4_aux<0>(rvel, ((t.j0 << texel.ln) + t.i0) * 16, 0);
  float4 const u10 = buf_load_f32x4_aux<0>(rvel, t.wantx ? ((t.j0 << texel.ln) + t.i1) * 16 : -256, 0);
  float4 const u01 = buf_load_f32x4_aux<0>(rvel, t.wanty ? ((t.j1 << texel.ln) + t.i0) * 16 : -256, 0);
  float4 const u11 = buf_load_f32x4_aux<0>(rvel, (t.wantx && t.wanty) ? ((t.j1 << texel.ln) + t.i1) * 16 : -256, 0);

  float const cx = t.blend(a00.x, a10.x, a01.x, a11.x);
  float const cy = t.blend(a00.y, a10.y, a01.y, a11.y);
  float const cz = t.blend(a00.z, a10.z, a01.z, a11.z);

  dx = (c == 0) ? cx : dx + cx;
  dy = (c == 0) ? cy : dy + cy;
  dz = (c == 0) ? cz : dz + cz;

  float const wx = t.blend(u00.x, u10.x, u01.x, u11.x);
  float const wy = t.blend(u00.y, u10.y, u01.y, u11.y);
  float const wz = t.blend(u00.z, u10.z, u01.z, u11.z);

  ux = (c == 0) ? wx : ux + wx;
  uy = (c == 0) ? wy : uy + wy;
  uz = (c == 0) ? wz : uz + wz;
}

float const vx = px - dx, vy = py - dy, vz = (f.basez + p.swellamplitude * st) + dz;

float const rx = vx - q.x, ry = vy - q.y;
float const residual = __builtin_sqrtf(fmaf(ry, ry, rx * rx));

#else

float dx = 0.0f, dy = 0.0f, dz = 0.0f, sx = 0.0f, sy = 0.0f, foam = 0.0f;

for(int c = 0; c < count; ++c)
{
  BlendCascade const &bc = list.casc[c];

  __amdgpu_buffer_rsrc_t const rmap = make_rsrc(bc.map, mapbytes);

  SurfaceTexel<LAYOUT> const t(texel, f, bc.scale, nmask, px, py);

  float4 const a00 = buf_load_f32x4_aux<0>(rmap, t.o00, 0);
  float4 const a10 = buf_load_f32x4_aux<0>(rmap, t.o10, 0);
  float4 const a01 = buf_load_f32x4_aux<0>(rmap, t.o01, 0);
  float4 const a11 = buf_load_f32x4_aux<0>(rmap, t.o11, 0);

  int const bc0 = texel.bcolumn(t.i0), bc1 = texel.bcolumn(t.i1);
  int const br0 = MAP_PART_B - texel.brow(t.j0), br1 = MAP_PART_B - texel.brow(t.j1);

  float2 const b00 = buf_load_f32x2(rmap, t.o00 + br0 - bc0, 0);
  float2 const b10 = buf_load_f32x2(rmap, t.wantx ? t.o10 + br0 - bc1 : -256, 0);
  float2 const b01 = buf_load_f32x2(rmap, t.wanty ? t.o01 + br1 - bc0 : -256, 0);
  float2 const b11 = buf_load_f32x2(rmap, (t.wantx && t.wanty) ? t.o11 + br1 - bc1 : -256, 0);

  if (bc.foam)
  {
    __amdgpu_buffer_rsrc_t const rfoam = make_rsrc(bc.foam, (size_t)s.N * s.N * sizeof(float));

    float const g00 = buf_load_f32(rfoam, ((t.j0 << texel.ln) + t.i0) * 4, 0);
    float const g10 = buf_load_f32(rfoam, t.wantx ? ((t.j0 << texel.ln) + t.i1) * 4 : -256, 0);
    float const g01 = buf_load_f32(rfoam, t.wanty ? ((t.j1 << texel.ln) + t.i0) * 4 : -256, 0);
    float const g11 = buf_load_f32(rfoam, (t.wantx && t.wanty) ? ((t.j1 << texel.ln) + t.i1) * 4 : -256, 0);

    float const fc = t.blend(g00, g10, g01, g11);

    // ACCUMULATE: the largest coverage; JACOBIAN: 1 + sum (J_c - 1), the summed displacement's Jacobian without the cross terms
    if (list.foammode == DATUM_OCEAN_FOAM_JACOBIAN)
      foam = foam + (fc - 1.0f);
    else
      foam = (c == 0) ? fc : fmaxf(foam, fc);
  }

  float const cx = t.blend(a00.x, a10.x, a01.x, a11.x);
  float const cy = t.blend(a00.y, a10.y, a01.y, a11.y);
  float const cz = t.blend(a00.z, a10.z, a01.z, a11.z);

  dx = (c == 0) ? cx : dx + cx;
  dy = (c == 0) ? cy : dy + cy;
  dz = (c == 0) ? cz : dz + cz;

  float const nx = t.blend(a00.w, a10.w, a01.w, a11.w);
  float const ny = t.blend(b00.x, b10.x, b01.x, b11.x);
  float const nz = t.blend(b00.y, b10.y, b01.y, b11.y);

  float const rz = __builtin_amdgcn_rcpf(nz);

  sx = fmaf(nx, rz, sx);
  sy = fmaf(ny, rz, sy);
}

if (list.foammode == DATUM_OCEAN_FOAM_JACOBIAN)
  foam = 1.0f + foam;

float const vx = px - dx, vy = py - dy, vz = (f.basez + p.swellamplitude * st) + dz;

float const rx = vx - q.x, ry = vy - q.y;
float const residual = __builtin_sqrtf(fmaf(ry, ry, rx * rx));

float mx, my, mz;

blend_surface_normal(f, st, ct, sx, sy, mx, my, mz);

#endif
