"""ref64.lit64 -- the literal transform mode's float64 reference -- pinned on the CPU, and the bars of
tests/test_gpu_literal_pointwise.py derived from the reference's own fp32 arithmetic.  Three properties:

  1. with accurately evaluated twiddles lit64 IS displace64 (the exact transform) to float64 rounding: its gathers, its lane / stage
     indexing and its map stage are not a restatement of a mistake in ocean_literal.hip;
  2. the fp32 oracle (oracle.displace with the literal table: the reference's arithmetic, libm's sin / cos, no contraction) against lit64
     on the GPU test's own inputs gives K_REF_*; the GPU's bars are 3 x that (tests/pointwise.py) and the oracle must stay within a
     third of them -- and not far below: the constants are the measured worst, not a roomy guess;
  3. the pointwise comparison at those bars fails on faults that the RMSE < 2e-6 of tests/test_gpu_parity.py lets through.
CPU only."""

import numpy as np
import pytest

import pointwise as pw
import ref64

CHOP = 1.35


def _oracle_channels(oracle, h0, phase, wavescale, N):
    return ref64.channels(oracle.displace(h0, phase.copy(), wavescale, CHOP, w=oracle.weights(N), mt=N >= 1024).astype(np.float64))


def _k_of_the_oracle(oracle, h0, phase, wavescale):
    N = phase.shape[0]
    scale = np.float32(1) / np.float32(wavescale)
    ref, ln = ref64.lit64(h0, phase, scale, CHOP, oracle.weights(N), return_len=True)
    kd, kn, _ = pw.pointwise(_oracle_channels(oracle, h0, phase, wavescale, N), ref, ln, N)
    return kd, kn


# -- 1. ties to the exact transform ---------------------------------------------------------------------------------------------------

# Float64 tolerance.  Both sides run 2 log2 N butterfly stages per texel (rows, then columns; pocketfft's are radix 4 / 2 on the same
# data), each stage one complex product with a twiddle that is itself rounded and one sum: <= 4 roundings of 2^-53 relative to the
# running magnitude, which max |channel| bounds.  Errors of the stages add like a random walk at worst linearly in log2 N, so
# |lit64 - displace64| <= TIE * 2^-53 * log2 N * max |channel| with TIE = 2 sides x 2 passes x 4 = 16 (measured: 2.1 .. 2.9).
# A normal is (dz_a - dz_b) / len with len >= nz: its error is that of two dz values over nz, so max |channel| is replaced by
# 2 max |dz| / nz where that is the larger (measured in those units: <= 6).
TIE = 16.0


@pytest.mark.parametrize("N", [64, 256])
def test_lit64_with_accurate_twiddles_is_displace64(oracle, N):
    ws = oracle.EXAMPLE["wavescale"]
    h0, phase = pw.lit_state(oracle, N), pw.lit_phase(oracle, N, ws, pw.LIT_STEPS)
    scale = np.float32(1) / np.float32(ws)
    want, wlen = ref64.displace64(h0, phase, scale, CHOP, return_len=True)
    got, glen = ref64.lit64(h0, phase, scale, CHOP, ref64.twiddles64(N), return_len=True)
    unit = 2.0 ** -53 * np.log2(N)
    nz = 4.0 / (float(scale) * N)
    for ch in range(6):
        big = float(np.abs(want[ch]).max())
        if ch >= 3:
            big = max(big, 2 * float(np.abs(want[2]).max()) / nz)
        worst = float(np.abs(got[ch] - want[ch]).max()) / (unit * big)
        print(f"lit64 vs displace64 N={N} channel {ch}: {worst:.2f} x 2^-53 log2 N max (bar {TIE:g})")
        assert worst <= TIE, (N, ch, worst)
    assert float(np.abs(glen - wlen).max()) <= TIE * unit * 2 * float(np.abs(want[2]).max())
    # and it is the table handed in that it uses: with the fp32 literal table it leaves the exact transform by far more than the GPU's
    # bar allows (the table's own error) -- a kernel with other twiddles than the reference's would not pass as literal
    lit, _ = ref64.lit64(h0, phase, scale, CHOP, oracle.weights(N), return_len=True)
    kd, kn, _ = pw.pointwise(lit, want, wlen, N)
    assert kd > 2 * pw.K_LIT_DISP, (N, kd)


def test_twiddles64_is_the_table_rounded_where_the_literal_angle_is_exact(oracle):
    # stage 0 (period 2) and every lane below a stage's period with a short angle: the fp32 table is the float64 one within fp32 rounding
    # of the angle; over the whole table the literal one drifts with the unreduced angle (up to pi N * 2^-24)
    N = 256
    w32 = oracle.weights(N).astype(np.float64)
    w64 = ref64.twiddles64(N)
    assert w32.shape == w64.shape == (N, 16)
    assert np.abs(w32[:8] - w64[:8]).max() < 4e-6                # lanes 0 .. 7: angles up to 7 pi
    assert np.abs(w32 - w64).max() < np.pi * N * 2.0 ** -23
    assert np.array_equal(w64[:, 0], np.where(np.arange(N) & 1, -1.0, 1.0))


# -- 2. the reference's own rounding noise sets the GPU's bars ------------------------------------------------------------------------


@pytest.fixture(scope="module")
def measured():
    return {}


@pytest.mark.parametrize("N", pw.LIT_SIZES)
def test_the_oracle_sets_the_bar(oracle, measured, N):
    ws = oracle.EXAMPLE["wavescale"]
    kd, kn = _k_of_the_oracle(oracle, pw.lit_state(oracle, N), pw.lit_phase(oracle, N, ws, pw.LIT_STEPS), ws)
    measured[N] = (kd, kn)
    print(f"K_REF N={N:4d}: disp {kd:.3f} (a third of the bar: {pw.K_LIT_DISP / 3:g}); normal {kn:.3f} ({pw.K_LIT_NORMAL / 3:g})")
    assert kd <= pw.K_LIT_DISP / 3 and kn <= pw.K_LIT_NORMAL / 3, (N, kd, kn)


def test_the_bars_are_three_times_the_measured_worst(oracle, measured):
    # the constants of tests/pointwise.py are what the cases above measure (rounded up in the third digit), not more
    for N in pw.LIT_SIZES:
        if N not in measured:
            test_the_oracle_sets_the_bar(oracle, measured, N)
    kd = max(v[0] for v in measured.values())
    kn = max(v[1] for v in measured.values())
    assert pw.K_LIT_DISP == 3 * pw.K_REF_DISP and pw.K_LIT_NORMAL == 3 * pw.K_REF_NORMAL and pw.K_LIT_EDGE == 3 * pw.K_REF_EDGE
    assert 0.98 * pw.K_REF_DISP <= kd <= pw.K_REF_DISP, kd
    assert 0.98 * pw.K_REF_NORMAL <= kn <= pw.K_REF_NORMAL, kn


def test_the_oracle_on_the_cascade_case(oracle):
    # other wave scales (the per-cascade scale enters k^, nz and the phase) stay under the same K_REF
    N = pw.LIT_CASCADES[0]
    for ws, h0 in pw.lit_cascade_states(oracle):
        kd, kn = _k_of_the_oracle(oracle, h0, pw.lit_phase(oracle, N, ws, pw.LIT_STEPS), ws)
        print(f"K_REF cascade case, wavescale {ws:g}: disp {kd:.3f}; normal {kn:.3f}")
        assert kd <= pw.K_LIT_DISP / 3 and kn <= pw.K_LIT_NORMAL / 3, (ws, kd, kn)


@pytest.mark.parametrize("N", pw.LIT_EDGE_SIZES)
def test_the_oracle_sets_the_edge_bar(oracle, N):
    # single bins: a pure tone adds the table's errors coherently -- its own constant for the displacement channels, obtained the same way
    ws = oracle.EXAMPLE["wavescale"]
    worst = [0.0, 0.0]
    for steps in pw.LIT_EDGE_STEPS:
        phase = pw.lit_phase(oracle, N, ws, steps)
        for b in pw.lit_edge_bins(N):
            kd, kn = _k_of_the_oracle(oracle, pw.lit_edge_h0(N, b), phase, ws)
            worst = [max(worst[0], kd), max(worst[1], kn)]
            assert kd <= pw.K_LIT_EDGE / 3 and kn <= pw.K_LIT_NORMAL / 3, (N, b, steps, kd, kn)
    print(f"K_REF single bins N={N:4d}: disp {worst[0]:.3f} (a third of the bar: {pw.K_LIT_EDGE / 3:g}); normal {worst[1]:.3f} ({pw.K_LIT_NORMAL / 3:g})")
    if N == max(pw.LIT_EDGE_SIZES):
        assert worst[0] >= 0.98 * pw.K_REF_EDGE, worst                  # the constant is this size's worst


def test_single_bin_at_k0_has_no_direction(oracle):
    # h0 only at (N/2, N/2): that bin is k = 0 and contributes a constant to dz and NOTHING to dx, dy; what moves is its partner
    # (N/2-1, N/2-1) -- the displacement is that one wave's.  lit64 keeps the two apart exactly where the phase is zero.
    N = 64
    h = N // 2
    h0 = pw.lit_edge_h0(N, (h, h))
    hh, hx, hy = ref64.sim64(h0, np.zeros((N, N), np.float32), np.float32(1) / np.float32(22.0))
    assert hx[h, h] == 0 and hy[h, h] == 0 and hh[h, h] != 0
    assert np.count_nonzero(hx) == 1 and hx[h - 1, h - 1] != 0


# -- 3. what the comparison finds and the RMSE does not -------------------------------------------------------------------------------


def _rmse(a, b):
    d = a - b
    return float(np.sqrt((d * d).mean()))


@pytest.fixture(scope="module")
def passing(oracle):
    """the fp32 oracle's channels at 256^2 (they pass), lit64's, its length and the displacement scales"""
    N = 256
    ws = oracle.EXAMPLE["wavescale"]
    h0, phase = pw.lit_state(oracle, N), pw.lit_phase(oracle, N, ws, pw.LIT_STEPS)
    ref, ln = ref64.lit64(h0, phase, np.float32(1) / np.float32(ws), CHOP, oracle.weights(N), return_len=True)
    got = _oracle_channels(oracle, h0, phase, ws, N)
    got.setflags(write=False)
    ref.setflags(write=False)
    return N, got, ref, ln, pw.disp_scales(ref), float(np.float32(4) / (np.float32(1) / np.float32(ws) * np.float32(N)))


def _without_wrap(dz, y, x, nz):
    """the normal at (y, x) from dz with the neighbours clamped to the grid instead of wrapped"""
    N = dz.shape[0]
    nx = dz[y, max(x - 1, 0)] - dz[y, min(x + 1, N - 1)]
    ny = dz[min(y + 1, N - 1), x] - dz[max(y - 1, 0), x]
    ln = np.sqrt(nx * nx + ny * ny + nz * nz)
    return nx / ln, ny / ln, nz / ln


FAULTS = ["interior texel of dz", "dz texel in column 0", "dz texel in row N-1", "one row of dx", "border normal without wrap"]


@pytest.mark.parametrize("fault", FAULTS)
def test_the_comparison_finds_what_rmse_does_not(passing, fault):
    N, clean, ref, ln, s, nz = passing
    L = np.log2(N)
    kd, kn, _ = pw.pointwise(clean, ref, ln, N)
    assert kd <= pw.K_LIT_DISP and kn <= pw.K_LIT_NORMAL                       # the oracle passes
    bad = clean.copy()
    step = 4 * pw.K_LIT_DISP * pw.EPS * L * s[2]
    if fault == "interior texel of dz":
        bad[2, 100, 57] += step
    elif fault == "dz texel in column 0":
        bad[2, 31, 0] -= step
    elif fault == "dz texel in row N-1":
        bad[2, N - 1, 200] += step
    elif fault == "one row of dx":
        bad[0, 77, :] += 2 * pw.K_LIT_DISP * pw.EPS * L * s[0]                 # one workgroup of the row transform
    else:
        y, x = 140, 0                                                          # x - 1 = -1
        bad[3, y, x], bad[4, y, x], bad[5, y, x] = _without_wrap(clean[2], y, x, nz)
    assert not np.array_equal(bad, clean)
    kd, kn, _ = pw.pointwise(bad, ref, ln, N)
    print(f"{fault}: disp K {kd:.2f} (bar {pw.K_LIT_DISP:g}), normal K {kn:.2f} (bar {pw.K_LIT_NORMAL:g}); "
          f"rmse vs lit64: disp {_rmse(bad[:3], ref[:3]):.2e} normal {_rmse(bad[3:], ref[3:]):.2e}")
    assert kd > pw.K_LIT_DISP or kn > pw.K_LIT_NORMAL, fault                   # the pointwise check fails
    if fault == "border normal without wrap":
        assert kn > pw.K_LIT_NORMAL and kd <= pw.K_LIT_DISP
    else:
        assert kd > pw.K_LIT_DISP
    # ... while the displacement RMSE of tests/test_gpu_parity.py's literal-mode tests (< 2e-6, against the fp32 oracle there; against
    # lit64 here as well) does not move
    assert _rmse(bad[:3], clean[:3]) < 2e-6 and _rmse(bad[:3], ref[:3]) < 2e-6, fault
    # The normal layer's RMSE stays put as well, except under the last fault: one unwrapped normal is off by ~2e-2 (K = 5e4), which at
    # 256^2 is 3.9e-5 of RMSE on that layer -- visible there at this size, 16 times smaller at 4096^2 (2.4e-6 against the 2e-6 bar).
    if fault != "border normal without wrap":
        assert _rmse(bad[3:], clean[3:]) < 2e-6 and _rmse(bad[3:], ref[3:]) < 2e-6, fault
