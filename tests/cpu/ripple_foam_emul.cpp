// ripple_foam_emul.cpp -- datum_amd/csrc/ocean_ripple_foam.h walked on the CPU (tests/test_ripple_foam_emul.py): the functions the kernels
// of ocean_ripple_foam.hip call, cell by cell over the torus in memory as ocean_ripple_foam_kernel reaches them, and point by point for
// the sampler.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_ripple_foam.h"

using namespace ocean;

extern "C"
{

float ripple_foam_emul_max(float a, float b) { return ripple_foam_max(a, b); }

// one update of the plane in MEMORY order, in place as the kernel does it: state [R*R][2], foam [R*R], p = hinv, t1, k1, t2, k2, fade
void ripple_foam_emul_update(float const *state, float *foam, int R, int ox, int oy, float const *p)
{
  RippleFoamParams q;
  q.hinv = p[0];
  q.t1 = p[1];
  q.k1 = p[2];
  q.t2 = p[3];
  q.k2 = p[4];
  q.fade = p[5];

  auto height = [&](int mx, int my) { return state[2 * ((my & (R - 1)) * R + (mx & (R - 1)))]; };

  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
    {
      int const wx = ripple_wrap(mx - ox, R), wy = ripple_wrap(my - oy, R);

      float const eL = wx == 0 ? 0.0f : height(mx - 1, my);
      float const eR = wx == R - 1 ? 0.0f : height(mx + 1, my);
      float const eD = wy == 0 ? 0.0f : height(mx, my - 1);
      float const eU = wy == R - 1 ? 0.0f : height(mx, my + 1);

      int const cell = my * R + mx;

      foam[cell] = ripple_foam_update(state[2 * cell + 1], eL, eR, eD, eU, foam[cell], q);
    }
}

// n samples of the plane [R*R] (memory order) at points [n][2]: out [n]; returns the cells fetched
long long ripple_foam_emul_sample(float const *foam, int R, int ox, int oy, float invs, float const *points, int n, float *out)
{
  RippleGrid g;
  g.R = R;
  g.ox = ox;
  g.oy = oy;
  g.invs = invs;

  long long fetched = 0;

  for(int i = 0; i < n; ++i)
    out[i] = ripple_foam_sample(g, points[2 * i], points[2 * i + 1], [&](int index) { ++fetched; return foam[index]; });

  return fetched;
}

}
