// ripple_wall_emul.cpp -- datum_amd/csrc/ocean_ripple_wall.h walked on the CPU (tests/test_ripple_wall_emul.py): the functions the
// kernels of ocean_ripple_wall.hip call, cell by cell over the torus in memory.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_ripple_wall.h"

using namespace ocean;

extern "C"
{

int ripple_wall_emul_sizeof(void) { return (int)sizeof(datum_ocean_ripple_wall); }

// the plane [R*R] in MEMORY order at the origin (ox, oy)
void ripple_wall_emul_raster(datum_ocean_ripple_wall const *walls, int count, unsigned char *plane, int R, int ox, int oy, float s)
{
  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
      plane[my * R + mx] = ripple_wall_cell(walls, count, ox + ripple_wrap(mx - ox, R), oy + ripple_wrap(my - oy, R), s);
}

// one walled WAVE sub-step over the layer in memory order: in, out [R*R][2], src [R*R], wall [R*R], f [B + 1]
void ripple_wall_emul_substep(float const *in, float *out, int const *src, unsigned char const *wall, int R, int ox, int oy, int B, float h, float c2s2, float const *f, int first)
{
  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
    {
      int const wx = ripple_wrap(mx - ox, R), wy = ripple_wrap(my - oy, R);
      int const i = my * R + mx;

      float const e = ripple_height(in[2 * i], src[i], first != 0);

      auto read = [&](int di, int dj, bool inside)
      {
        int const n = ripple_wrap(my + dj, R) * R + ripple_wrap(mx + di, R);

        return ripple_wall_neighbour(inside, wall[n] != 0, e, ripple_height(in[2 * n], src[n], first != 0));
      };

      float const eL = read(-1, 0, wx != 0), eR = read(1, 0, wx != R - 1), eD = read(0, -1, wy != 0), eU = read(0, 1, wy != R - 1);

      RippleCell const c = ripple_wall_pin(wall[i] != 0, ripple_update(e, in[2 * i + 1], eL, eR, eD, eU, h, c2s2, f[ripple_sponge(wx, wy, R, B)]));

      out[2 * i] = c.eta;
      out[2 * i + 1] = c.rate;
    }
}

// one walled DEEP sub-step, G [49]
void ripple_wall_emul_deep_substep(float const *in, float *out, int const *src, unsigned char const *wall, int R, int ox, int oy, int B, float h, float gs, float const *f, float const *G, int first)
{
  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
    {
      int const wx = ripple_wrap(mx - ox, R), wy = ripple_wrap(my - oy, R);

      auto height = [&](int di, int dj)
      {
        if ((unsigned int)(wx + di) >= (unsigned int)R || (unsigned int)(wy + dj) >= (unsigned int)R)
          return 0.0f;

        int const n = ripple_wrap(my + dj, R) * R + ripple_wrap(mx + di, R);

        return ripple_wall_height(wall[n] != 0, in[2 * n], src[n], first != 0);
      };

      float const acc = ripple_deep_conv(G, height);

      int const i = my * R + mx;

      RippleCell const c = ripple_wall_pin(wall[i] != 0, ripple_deep_update(height(0, 0), in[2 * i + 1], acc, h, gs, f[ripple_sponge(wx, wy, R, B)]));

      out[2 * i] = c.eta;
      out[2 * i + 1] = c.rate;
    }
}

}
