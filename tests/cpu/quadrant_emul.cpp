// The phase's quadrant table (datum_amd/csrc/ocean_quadrant.h) behind a C interface, for tests/test_quadrant_emul.py: the index rule, the
// expand map, the row pass's offsets and its single-writer rule, and the symmetry test, walked by the very functions the kernels call; the
// advance is ocean_phase.h's.

#include <stdint.h>

#include "../../datum_amd/csrc/ocean_phase.h"
#include "../../datum_amd/csrc/ocean_quadrant.h"

using namespace ocean;

extern "C"
{
  int quadrant_emul_side(int N) { return quadrant_side(N); }

  // the expand map over every plane element: hits[k] = plane elements that read table element k; returns the plane elements whose index
  // is out of the table or whose representative does not share it (0 = none)
  long quadrant_emul_expand(int N, int *hits)
  {
    long bad = 0;

    for(int y = 0; y < N; ++y)
    {
      for(int x = 0; x < N; ++x)
      {
        size_t const k = quadrant_index(N, y, x);

        if (k >= quadrant_count(N))
        {
          ++bad;
          continue;
        }

        hits[k] += 1;

        size_t const r = quadrant_representative(N, (int)(k / quadrant_side(N)), (int)(k % quadrant_side(N)));

        if (r >= (size_t)N * N || quadrant_index(N, (int)(r / N), (int)(r % N)) != k)
          ++bad;
      }
    }

    return bad;
  }

  // the row pass over one cascade, every (pair, half, thread, slot) with E slots per thread: writers[k] = threads whose store goes to table
  // element k; returns the slots whose LOAD offset is not the quadrant index of the point the slot holds (0 = none)
  long quadrant_emul_rowpass(int N, int E, int *writers)
  {
    int const T = N / E;
    long bad = 0;

    for(int p = 0; p < N / 2; ++p)
    {
      for(int half = 0; half < 2; ++half)
      {
        int const y = half ? (p == 0 ? N / 2 : N - p) : p;      // ocean_rowpass_kernel: row_of
        int const i = quadrant_abs(y - N / 2);

        for(int t = 0; t < T; ++t)
        {
          for(int s = 0; s < E; ++s)
          {
            int const k = quadrant_slot(N, T, E, i, t, s);

            if (k < 0 || (size_t)k >= quadrant_count(N) || (size_t)k != quadrant_index(N, y, t + T * s))
            {
              ++bad;
              continue;
            }

            if (quadrant_row_stores(p, half) && quadrant_slot_stores(E, t, s))
              writers[k] += 1;
          }
        }
      }
    }

    return bad;
  }

  // update_ocean on a whole plane, one dt: the fused advance where `fused` (the caller keeps to its range), the general one otherwise
  void quadrant_emul_advance(int N, float const *omega, float dt, int fused, float *phase)
  {
    for(int y = 0; y < N; ++y)
    {
      for(int x = 0; x < N; ++x)
      {
        float const w = omega[quadrant_index(N, y, x)] * dt;
        float &p = phase[(size_t)y * N + x];

        if (fused)
        {
          float const sum = p + w;
          p = fused_advance_select(sum, sum - 6.2831855f);
        }
        else
          p = advance_phase(p, w);
      }
    }
  }

  // ... and on the table alone (ocean_advance_kernel's quadrant branch)
  void quadrant_emul_advance_table(int N, float const *omega, float dt, int fused, float *q)
  {
    for(size_t k = 0; k < quadrant_count(N); ++k)
    {
      float const w = omega[k] * dt;

      if (fused)
      {
        float const sum = q[k] + w;
        q[k] = fused_advance_select(sum, sum - 6.2831855f);
      }
      else
        q[k] = advance_phase(q[k], w);
    }
  }

  // the symmetry test over a plane: the elements that differ from their representative
  long quadrant_emul_asymmetric(int N, float const *phase)
  {
    long bad = 0;

    for(size_t k = 0; k < (size_t)N * N; ++k)
      bad += quadrant_element_symmetric(phase, N, k) ? 0 : 1;

    return bad;
  }

  // compact and expand as the kernels index them
  void quadrant_emul_compact(int N, float const *phase, float *q)
  {
    for(size_t k = 0; k < quadrant_count(N); ++k)
      q[k] = phase[quadrant_representative(N, (int)(k / quadrant_side(N)), (int)(k % quadrant_side(N)))];
  }

  void quadrant_emul_fill(int N, float const *q, float *phase)
  {
    for(size_t k = 0; k < (size_t)N * N; ++k)
      phase[k] = q[quadrant_index(N, (int)(k / N), (int)(k % N))];
  }
}
