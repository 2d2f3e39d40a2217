// ripple_deep_emul.cpp -- datum_amd/csrc/ocean_ripple_deep.h walked on the CPU (tests/test_ripple_deep_emul.py): the functions the
// kernel of ocean_ripple_deep.hip calls, cell by cell over the torus in memory, and the host-only construction of the weights.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_ripple_deep.h"

using namespace ocean;

extern "C"
{

// the 49 weights [l][k] as the header builds them; returns Sum |F| over the 169
double ripple_deep_emul_weights(float *G) { return ripple_deep_weights(G); }

// one DEEP sub-step over the layer in MEMORY order: in, out [R*R][2], src [R*R], f [B + 1], G [49]
void ripple_deep_emul_substep(float const *in, float *out, int const *src, int R, int ox, int oy, int B, float h, float gs, float const *f, float const *G, int first)
{
  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
    {
      int const wx = ripple_wrap(mx - ox, R), wy = ripple_wrap(my - oy, R);

      auto height = [&](int di, int dj)
      {
        if ((unsigned int)(wx + di) >= (unsigned int)R || (unsigned int)(wy + dj) >= (unsigned int)R)
          return 0.0f;

        int const i = ripple_wrap(my + dj, R) * R + ripple_wrap(mx + di, R);

        return ripple_height(in[2 * i], src[i], first != 0);
      };

      float const acc = ripple_deep_conv(G, height);

      RippleCell const c = ripple_deep_update(height(0, 0), in[2 * (my * R + mx) + 1], acc, h, gs, f[ripple_sponge(wx, wy, R, B)]);

      out[2 * (my * R + mx)] = c.eta;
      out[2 * (my * R + mx) + 1] = c.rate;
    }
}

}
