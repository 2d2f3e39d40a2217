// ripple_emul.cpp -- datum_amd/csrc/ocean_ripple.h walked on the CPU (tests/test_ripple_emul.py): the functions the kernels of
// ocean_ripple.hip call, cell by cell over the torus in memory, with the src plane a plain array and the wave's 64 lanes as an array.  The
// velocity records of the wake are given (body b's probe k has record offsets[b] + k): the fetch and the solve are the several-cascade
// velocity query's and are pinned there.

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../datum_amd/csrc/ocean_ripple.h"

using namespace ocean;

namespace
{
  struct RippleWaveArray
  {
    BodyPartial p[BODY_LANES];

    template<int S>
    void step()
    {
      for(int l = 0; l < S; ++l)
        body_add(p[l], p[l + S]);
    }
  };

  RippleGrid grid(int R, int ox, int oy, float invs)
  {
    RippleGrid g;
    g.R = R;
    g.ox = ox;
    g.oy = oy;
    g.invs = invs;
    return g;
  }
}

extern "C"
{

int ripple_emul_index(int I, int J, int R) { return ripple_index(I, J, R); }
int ripple_emul_inside(int R, int ox, int oy, int I, int J) { return ripple_inside(grid(R, ox, oy, 1.0f), I, J) ? 1 : 0; }
int ripple_emul_sponge(int wx, int wy, int R, int B) { return ripple_sponge(wx, wy, R, B); }

// the window's rectangles in memory, rects [4][4]: from, to, w, h of each; returns their number
int ripple_emul_window(int ox, int oy, int R, int *rects)
{
  RippleRect rect[4];

  int const n = ripple_window(ox, oy, R, rect);

  for(int k = 0; k < n; ++k)
  {
    rects[4 * k] = rect[k].from;
    rects[4 * k + 1] = rect[k].to;
    rects[4 * k + 2] = rect[k].w;
    rects[4 * k + 3] = rect[k].h;
  }

  return n;
}

// one sub-step over the layer in MEMORY order, as the kernel walks it: in, out [R*R][2], src [R*R], f [B + 1]
void ripple_emul_substep(float const *in, float *out, int const *src, int R, int ox, int oy, int B, float h, float c2s2, float const *f, int first)
{
  auto height = [&](int mx, int my)
  {
    int const i = (my & (R - 1)) * R + (mx & (R - 1));

    return ripple_height(in[2 * i], src[i], first != 0);
  };

  for(int my = 0; my < R; ++my)
    for(int mx = 0; mx < R; ++mx)
    {
      int const wx = ripple_wrap(mx - ox, R), wy = ripple_wrap(my - oy, R);

      float const e = height(mx, my);
      float const eL = wx == 0 ? 0.0f : height(mx - 1, my);
      float const eR = wx == R - 1 ? 0.0f : height(mx + 1, my);
      float const eD = wy == 0 ? 0.0f : height(mx, my - 1);
      float const eU = wy == R - 1 ? 0.0f : height(mx, my + 1);

      RippleCell const c = ripple_update(e, in[2 * (my * R + mx) + 1], eL, eR, eD, eU, h, c2s2, f[ripple_sponge(wx, wy, R, B)]);

      out[2 * (my * R + mx)] = c.eta;
      out[2 * (my * R + mx) + 1] = c.rate;
    }
}

// n splats (x, y, V, 0) into src; returns the dropped quanta
long long ripple_emul_splat(int *src, int R, int ox, int oy, float invs, float const *impulses, int n)
{
  RippleGrid const g = grid(R, ox, oy, invs);

  long long dropped = 0;

  for(int i = 0; i < n; ++i)
    dropped += ripple_splat(g, impulses[4 * i], impulses[4 * i + 1], impulses[4 * i + 2], [&](int index, int q) { src[index] += q; });

  return dropped;
}

// n samples of the state [R*R][2] (memory order) at points [n][2]: out [n][4]
void ripple_emul_sample(float const *state, int R, int ox, int oy, float invs, float const *points, int n, float *out)
{
  RippleGrid const g = grid(R, ox, oy, invs);

  for(int i = 0; i < n; ++i)
  {
    RippleSample const s = ripple_sample(g, points[2 * i], points[2 * i + 1], [&](int index) { return RippleCell{ state[2 * index], state[2 * index + 1] }; });

    out[4 * i] = s.eta;
    out[4 * i + 1] = s.dx;
    out[4 * i + 2] = s.dy;
    out[4 * i + 3] = s.rate;
  }
}

// the wake kernel's walk with the velocity records given: records_out [nbodies][8], deposits into src
void ripple_emul_wake(datum_ocean_body const *bodies, datum_ocean_body_motion const *motions, int nbodies, float const *probes, int nprobes, int64_t const *offsets,
                      float const *recs, float dt, int *src, int R, int ox, int oy, float invs, float *records_out)
{
  RippleGrid const g = grid(R, ox, oy, invs);

  auto splat = [&](float x, float y, float V) { return ripple_splat(g, x, y, V, [&](int index, int q) { src[index] += q; }); };

  for(int b = 0; b < nbodies; ++b)
  {
    datum_ocean_body const &B = bodies[b];
    datum_ocean_body_motion const &M = motions[b];

    bool bad = body_range_bad(B, nprobes) || drag_motion_bad(M);

    int const n = bad ? 0 : B.count;

    RippleWaveArray wave;

    for(int l = 0; l < BODY_LANES; ++l)
    {
      wave.p[l] = body_zero();

      for(int k = 0; k < body_lane_probes(n, l); ++k)
      {
        int const i = body_lane_probe(0, l, k);

        BodyProbe const &pr = reinterpret_cast<BodyProbe const*>(probes)[B.first + i];
        BodyWorld const w = body_transform(B, pr);

        if (body_probe_bad(w, pr.a))
        {
          bad = true;
          continue;
        }

        body_add(wave.p[l], wake_terms(B, M, w, pr.a, recs + 8 * (offsets[b] + i), dt, splat));
      }
    }

    body_tree(wave);

    for(int f = 0; f < BODY_FIELDS; ++f)
      records_out[8 * b + f] = bad ? nanf("") : wave.p[0].f[f];
  }
}

}
