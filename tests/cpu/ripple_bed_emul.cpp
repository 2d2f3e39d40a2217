// ripple_bed_emul.cpp -- datum_amd/csrc/ocean_ripple_bed.h walked on the CPU (tests/test_ripple_bed_emul.py): the functions the kernels
// of ocean_ripple_bed.hip call, cell by cell over the torus in memory.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_ripple_bed.h"

using namespace ocean;

namespace
{
  // the bed as the host builds it from the record: 1 / texel and 1 / surf_depth rounded once from double
  RippleBed bed_of(datum_ocean_ripple_bed const &p)
  {
    RippleBed b;
    b.width = p.width;
    b.height = p.height;
    b.ox = p.origin[0];
    b.oy = p.origin[1];
    b.invt = (float)(1.0 / (double)p.texel);
    b.outside = p.outside;
    b.max_depth = p.max_depth;
    b.dry_depth = p.dry_depth;
    b.surf_depth = p.surf_depth;
    b.invsurf = p.surf_depth > 0.0f ? (float)(1.0 / (double)p.surf_depth) : 0.0f;
    return b;
  }
}

extern "C"
{

int ripple_bed_emul_sizeof(void) { return (int)sizeof(datum_ocean_ripple_bed); }

// both planes [R*R] in MEMORY order at the origin (ox, oy); wall [R*R] or null
void ripple_bed_emul_raster(datum_ocean_ripple_bed const *p, float const *map, unsigned char const *wall, float *depth, unsigned char *surf, int R, int ox, int oy, float s)
{
  RippleBed const b = bed_of(*p);

  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
    {
      int const i = my * R + mx;

      RippleBedCell const c = ripple_bed_cell(b, ox + ripple_wrap(mx - ox, R), oy + ripple_wrap(my - oy, R), s, wall && wall[i] != 0, [&](int index) { return map[index]; });

      depth[i] = c.d;
      surf[i] = c.q;
    }
}

// one sub-step over a bed, the layer in memory order: in, out [R*R][2], src [R*R], depth [R*R], surf [R*R], f [B + 1], fsurf [17]
void ripple_bed_emul_substep(float const *in, float *out, int const *src, float const *depth, unsigned char const *surf, int R, int ox, int oy, int B, float h, float gs2, float const *f, float const *fsurf, int first)
{
  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
    {
      int const wx = ripple_wrap(mx - ox, R), wy = ripple_wrap(my - oy, R);
      int const i = my * R + mx;

      float const e = ripple_height(in[2 * i], src[i], first != 0);
      float const dc = depth[i];

      auto flux = [&](int di, int dj, bool inside)
      {
        int const n = ripple_wrap(my + dj, R) * R + ripple_wrap(mx + di, R);

        return ripple_bed_flux(inside, dc, depth[n], e, ripple_height(in[2 * n], src[n], first != 0));
      };

      float const tL = flux(-1, 0, wx != 0), tR = flux(1, 0, wx != R - 1), tD = flux(0, -1, wy != 0), tU = flux(0, 1, wy != R - 1);

      RippleCell const c = ripple_bed_update(e, in[2 * i + 1], tL, tR, tD, tU, dc, h, gs2, f[ripple_sponge(wx, wy, R, B)], fsurf[surf[i]]);

      out[2 * i] = c.eta;
      out[2 * i + 1] = c.rate;
    }
}

}
