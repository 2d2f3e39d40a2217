// ripple_swell_emul.cpp -- datum_amd/csrc/ocean_ripple_swell.h walked on the CPU (tests/test_ripple_swell_emul.py): the functions the
// kernels of ocean_ripple_swell.hip call, cell by cell over the torus in memory.  The heights of the summed surface are the caller's: a
// plane H [R*R] in memory order, the height above each cell's centre (a neighbour that counts lies inside the window, so on the torus).

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_ripple_swell.h"

using namespace ocean;

extern "C"
{

// F [R*R] in MEMORY order at the origin (ox, oy); wall [R*R] or null, depth [R*R] or null (the bed on: the wall plane is not read)
void ripple_swell_emul_force(float const *H, unsigned char const *wall, float const *depth, float *F, int R, int ox, int oy)
{
  auto solid = [&](int i) { return depth ? ripple_swell_solid_bed(depth[i]) : wall ? ripple_swell_solid(wall[i]) : false; };

  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
    {
      int const wx = ripple_wrap(mx - ox, R), wy = ripple_wrap(my - oy, R);
      int const i = my * R + mx;

      auto face = [&](int di, int dj, bool inside)
      {
        int const n = ripple_wrap(my + dj, R) * R + ripple_wrap(mx + di, R);

        return ripple_swell_face(ripple_swell_counts(inside, solid(n)), H[i], H[n]);
      };

      float const dL = face(-1, 0, wx != 0), dR = face(1, 0, wx != R - 1), dD = face(0, -1, wy != 0), dU = face(0, 1, wy != R - 1);

      F[i] = ripple_swell_force(solid(i), dL, dR, dD, dU);
    }
}

// the centre of world cell I along one axis, as the refresh kernel hands it to the query
float ripple_swell_emul_centre(int I, float s) { return ripple_swell_centre(I, s); }

// one WAVE sub-step with walls and swell, the layer in memory order: in, out [R*R][2], src [R*R], wall [R*R] or null, F [R*R], f [B + 1]
void ripple_swell_emul_substep(float const *in, float *out, int const *src, unsigned char const *wall, float const *F, int R, int ox, int oy, int B, float h, float c2s2, float const *f, int first)
{
  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
    {
      int const wx = ripple_wrap(mx - ox, R), wy = ripple_wrap(my - oy, R);
      int const i = my * R + mx;

      float const e = ripple_height(in[2 * i], src[i], first != 0);

      auto neighbour = [&](int di, int dj, bool inside)
      {
        int const n = ripple_wrap(my + dj, R) * R + ripple_wrap(mx + di, R);

        return ripple_wall_neighbour(inside, wall && wall[n] != 0, e, ripple_height(in[2 * n], src[n], first != 0));
      };

      float const eL = neighbour(-1, 0, wx != 0), eR = neighbour(1, 0, wx != R - 1), eD = neighbour(0, -1, wy != 0), eU = neighbour(0, 1, wy != R - 1);

      RippleCell const c = ripple_swell_update(e, in[2 * i + 1], eL, eR, eD, eU, F[i], wall && wall[i] != 0, h, c2s2, f[ripple_sponge(wx, wy, R, B)]);

      out[2 * i] = c.eta;
      out[2 * i + 1] = c.rate;
    }
}

// one WAVE sub-step over a bed with swell: depth [R*R], surf [R*R], fsurf [17] besides
void ripple_swell_emul_bed_substep(float const *in, float *out, int const *src, float const *depth, unsigned char const *surf, float const *F, int R, int ox, int oy, int B, float h, float gs2, float const *f, float const *fsurf, int first)
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

      RippleCell const c = ripple_swell_bed_update(e, in[2 * i + 1], tL, tR, tD, tU, dc, F[i], h, gs2, f[ripple_sponge(wx, wy, R, B)], fsurf[surf[i]]);

      out[2 * i] = c.eta;
      out[2 * i + 1] = c.rate;
    }
}

}
