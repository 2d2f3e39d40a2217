// ocean_quadrant.h -- the phase's second home, stated once: a quadrant table per cascade, indexed like the dispersion table of
// ocean_omega_kernel, which holds the whole phase plane for as long as the plane is symmetric.
//
// update_ocean gives every point  p = fmod(p + omega(k) dt, 2 pi)  and omega(k) is a function of (|y - N/2|, |x - N/2|) alone, served from the
// (N/2 + 1)^2 table.  Points that share that index and start from the same bits are given the same fp32 instructions on the same operands
// for ever after: a phase that is a function of the quadrant index stays one -- under the fused advance and under the general one, whatever
// the sign of dt -- until somebody replaces it.  Zero, what every state without an uploaded phase starts from, is such a phase.
//
// Index arithmetic and the symmetry test only, host/device neutral so that a CPU can walk every resolution through it
// (tests/cpu/quadrant_emul.cpp, tests/test_quadrant_emul.py).  The kernels that use it are in ocean_kernels.hip, the host's record of where a
// cascade's phase lives in ocean_capi.hip (CascadeState::quadrant).
//
// WHERE THE TRUTH LIVES, the one rule: while CascadeState::quadrant is set the table is the cascade's phase and the plane is nobody's; every
// call that reads or copies the plane expands the table into it first (ocean_capi.hip: materialise) and the table STAYS the truth -- the
// plane is then a copy that is current until the next advance.  A call that replaces the phase decides anew (quadrant_symmetric), and a
// cascade that must take the plane kernel (a wild phase, an asymmetric cascade in the same handle, the plane mode) is expanded and its flag
// cleared: from then on the plane is the truth, as in builds before the table.

#pragma once

#include <stddef.h>
#include <string.h>

#if defined(__HIPCC__)
#define OQ_HD __host__ __device__ __forceinline__
#else
#define OQ_HD inline
#endif

namespace ocean
{
  //|---------------------- the table and the expand map -----------------------

  OQ_HD constexpr int quadrant_side(int N) { return N / 2 + 1; }
  OQ_HD constexpr size_t quadrant_count(int N) { return (size_t)quadrant_side(N) * quadrant_side(N); }

  OQ_HD constexpr int quadrant_abs(int v) { return v < 0 ? -v : v; }

  // the table element of grid point (y, x): phase[y][x] = q[|y - N/2|][|x - N/2|] (dispersion_lookup's index)
  OQ_HD constexpr size_t quadrant_index(int N, int y, int x)
  {
    return (size_t)quadrant_abs(y - N / 2) * quadrant_side(N) + quadrant_abs(x - N / 2);
  }

  // ... and the grid point that stands for table element (i, j) where the table is filled from a plane: the one with y, x >= N/2
  OQ_HD constexpr size_t quadrant_representative(int N, int i, int j)
  {
    return (size_t)(N / 2 + (i == N / 2 ? -i : i)) * N + (N / 2 + (j == N / 2 ? -j : j));
  }

  //|---------------------- the row pass's view ---------------------------------
  // A row-pass thread t of a row holds the E points x = t + T s (N = T E).  |x - N/2| is N/2 - t - T s in the lower half of the slots and
  // t + T (s - E/2) in the upper: two per-thread element offsets into table row i = |y - N/2| and compile-time steps.

  OQ_HD constexpr int quadrant_lower(int N, int T, int E, int i, int t) { return i * quadrant_side(N) + N / 2 - t - T * (E / 2 - 1); }   // slot E/2 - 1
  OQ_HD constexpr int quadrant_upper(int N, int i, int t) { return i * quadrant_side(N) + t; }                                           // slot E/2

  // elements from quadrant_lower / quadrant_upper to slot s
  OQ_HD constexpr int quadrant_step(int T, int E, int s) { return (s < E / 2) ? T * (E / 2 - 1 - s) : T * (s - E / 2); }

  OQ_HD constexpr int quadrant_slot(int N, int T, int E, int i, int t, int s)
  {
    return ((s < E / 2) ? quadrant_lower(N, T, E, i, t) : quadrant_upper(N, i, t)) + quadrant_step(T, E, s);
  }

  // THE SINGLE WRITER of a table element among the row pass's threads.  A workgroup's pair p (0 <= p < N/2) is rows p (half 0) and N - p
  // (half 1), which share table row N/2 - p: half 0 stores.  Pair 0 is rows 0 and N/2, table rows N/2 and 0, two distinct ones: both store.
  OQ_HD constexpr bool quadrant_row_stores(int p, int half) { return half == 0 || p == 0; }

  // In a row, x and N - x share an element: the upper half of the slots stores (x >= N/2, ascending addresses), and x = 0, whose element
  // j = N/2 has no twin, is stored by its thread as well.
  OQ_HD constexpr bool quadrant_slot_stores(int E, int t, int s) { return s >= E / 2 || (s == 0 && t == 0); }

  //|---------------------- is a plane symmetric? -------------------------------

  // one element against its representative, bit for bit (a NaN equals itself, +0 differs from -0: what is compared is what a load returns)
  OQ_HD bool quadrant_same_bits(float a, float b)
  {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(unsigned int, a) == __builtin_bit_cast(unsigned int, b);
#else
    unsigned int ua, ub;
    memcpy(&ua, &a, sizeof(ua));
    memcpy(&ub, &b, sizeof(ub));
    return ua == ub;
#endif
  }

  // element k = y N + x of a plane (ocean_phasecheck_kernel's body, a CPU's loop)
  OQ_HD bool quadrant_element_symmetric(float const *phase, int N, size_t k)
  {
    int const y = (int)(k / N), x = (int)(k % N);
    int const i = quadrant_abs(y - N / 2), j = quadrant_abs(x - N / 2);

    return quadrant_same_bits(phase[k], phase[quadrant_representative(N, i, j)]);
  }
}
