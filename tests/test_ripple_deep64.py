"""The DEEP step's definition (include/datum_ocean_hip.h: "dispersive ripples") held against what it claims, in numpy alone
(tests/ripple_deep64.py) and with the table the library returns:

  weights   the getter's 49 within 1e-6 G[0][0] of the float64 construction (one fp32 rounding plus libm); the 169 sum, in double, into
            [0, 2^-23 G[0][0]]; the symbol G^ >= 0 on a 256 x 256 grid of theta with its minimum at 0; |G^ - |theta|| / |theta| <= 0.08 on
            0.5 <= |theta| <= 1 and <= 0.02 on 1 <= |theta| <= 3, on the 512 x 512 grid; sum|F| bounds max G^;
  scheme    in the periodic box in float64 a single Fourier mode stays that mode and follows symplectic Euler's recurrence with
            omega^2 = gs G^(theta), to 1e-12, for three theta, one on the diagonal; with gamma = 0 the scheme's invariant
            <v, v> + gs <eta, G eta> - h gs <G eta, v> is conserved to 1e-12;
  mistakes  the four planted ones each fail the check that is there for it.
"""

import numpy as np
import pytest

import ripple_deep64 as rd

F = np.float32


@pytest.fixture(scope="module")
def table():
    from datum_amd import capi

    G = np.zeros((rd.Q, rd.Q), F)
    assert capi.load().datum_ocean_ripple_deep_weights(G.ctypes.data_as(capi.P)) == capi.OK
    return G


def _weights_close(G):
    want = rd.weights64()
    return np.abs(np.asarray(G, np.float64) - want).max() <= 1e-6 * want[0, 0]


def _sum_ok(G):
    s = float(rd.unfold(G).astype(np.float64).sum())
    return 0.0 <= s <= 2.0 ** -23 * float(G[0, 0])


def test_getter_against_float64(table):
    assert _weights_close(table) and _weights_close(rd.weights32())
    assert abs(float(table[0, 0]) - 2.403) < 0.001 and np.array_equal(table, table.T)


def test_sum_of_weights(table):
    assert _sum_ok(table) and _sum_ok(rd.weights32())
    # planted: the centre not corrected -- the rounded weights' sum misses the interval
    assert not _sum_ok(rd.weights32(mistake="centre"))


def test_symbol_not_negative(table):
    S, theta = rd.symbol(table, 256)
    assert S.min() >= 0.0
    assert np.unravel_index(np.argmin(S), S.shape) == (128, 128) and theta[128] == 0.0
    assert rd.symbol(rd.weights32(mistake="centre"), 256)[0].min() != S.min()


def _band(S, theta, lo, hi):
    r = np.sqrt(theta[:, None] ** 2 + theta[None, :] ** 2)
    m = (r >= lo) & (r <= hi)
    return float((np.abs(S - r)[m] / r[m]).max())


def test_band_errors(table):
    S, theta = rd.symbol(table, 512)
    low, mid, high = _band(S, theta, 0.5, 1.0), _band(S, theta, 1.0, 2.0), _band(S, theta, 2.0, 3.0)
    print(f"DEEP symbol: relative error {low:.4f} on [0.5, 1], {mid:.4f} on [1, 2], {high:.4f} on [2, 3]; max {S.max():.3f}, sum|F| {rd.mass(table):.3f}")
    assert low <= 0.08
    assert max(mid, high) <= 0.02


def test_mass_bounds_symbol(table):
    S, _ = rd.symbol(table, 512)
    assert S.max() <= rd.mass(table)
    assert abs(S.max() - 4.30) < 0.01 and abs(rd.mass(table) - 5.37) < 0.01


# -- the scheme, in the periodic box in float64

R, S_CELL, H, STEPS = 64, 0.5, 0.05, 40
MODES = [(3, 0), (5, 9), (7, 7)]                 # theta = 2 pi (m, n) / R; the last on the diagonal


def _box(G, gamma=0.0):
    return rd.Layer(R, S_CELL, np.float64, gamma=gamma, B=0, sponge_gamma=0.0, G=G, periodic=True)


def _mode_error(G, m, n, mistake=None, gamma=0.3):
    """the largest distance, over STEPS sub-steps, of the box started as cos(theta . x) from amplitude-times-that-mode with the amplitude
    following v1 = (v - h gs G^ a) f, a1 = a + h v1"""
    tx, ty = 2 * np.pi * m / R, 2 * np.pi * n / R
    j, i = np.mgrid[0:R, 0:R]
    mode = np.cos(tx * i + ty * j)
    lay = _box(G, gamma)
    lay.eta, lay.rate = mode.copy(), 0.25 * mode
    h, gs, f = rd.params(lay.g, lay.s, gamma, 0, 0.0, H, 1)
    h, gs, f0 = float(h), float(gs), float(f[0])
    w2 = gs * rd.symbol_at(G, tx, ty)
    a, v, worst = 1.0, 0.25, 0.0
    for _ in range(STEPS):
        lay.step(H, 1, mistake)
        v = (v - h * w2 * a) * f0
        a = a + h * v
        worst = max(worst, np.abs(lay.eta - a * mode).max(), np.abs(lay.rate - v * mode).max())
    assert abs(a) < 2 and abs(v) < 10                                           # (the recurrence itself is stable here)
    return worst


@pytest.mark.parametrize("m,n", MODES)
def test_single_mode_follows_the_recurrence(table, m, n):
    assert _mode_error(table, m, n) <= 1e-12


def _invariant(lay, h, gs):
    rest = rd.Layer(R, S_CELL, np.float64, gamma=0.0, B=0, sponge_gamma=0.0, G=lay.G, periodic=True)
    rest.eta = lay.eta.copy()
    # G eta by the restatement itself: one sub-step of length 1 with gs = 1 from rest turns eta into the rate -G eta
    _, minus = rd.substep(rest.eta, rest.rate, rest.src, rest.ox, rest.oy, 0, 1.0, 1.0, np.ones(1), lay.G, False, np.float64, None, True)
    Ge = -minus
    return float((lay.rate * lay.rate).sum() + gs * (lay.eta * Ge).sum() - h * gs * (Ge * lay.rate).sum())


def _invariant_drift(G, mistake=None):
    rng = np.random.default_rng(11)
    lay = _box(G)
    lay.eta, lay.rate = rng.normal(size=(R, R)), rng.normal(size=(R, R))
    h, gs, _ = rd.params(lay.g, lay.s, 0.0, 0, 0.0, H, 1)
    gs_used = float(rd.params(lay.g, lay.s, 0.0, 0, 0.0, H, 1, mistake)[1])
    q0 = _invariant(lay, float(h), float(gs))
    drift = 0.0
    for _ in range(STEPS):
        lay.step(H, 1, mistake)
        drift = max(drift, abs(_invariant(lay, float(h), float(gs)) - q0) / q0)
    assert gs_used > 0
    return drift


def test_invariant_is_conserved(table):
    assert _invariant_drift(table) <= 1e-12


# -- the planted mistakes


def test_planted_mistakes_fail(table):
    rng = np.random.default_rng(5)
    probe = (rng.normal(size=(rd.Q, rd.Q)) * 0.02).astype(F)                     # G[l][k] != G[k][l]
    probe[0, 0] = 1.0
    # [k][l] swapped: invisible with the symmetric table, seen by the asymmetric probe off the diagonal
    assert _mode_error(table, 5, 9, "swap") <= 1e-12
    assert _mode_error(probe, 5, 9) <= 1e-12 and _mode_error(probe, 5, 9, "swap") > 1e-6
    # the sign of acc: the mode grows instead of swinging
    assert _mode_error(table, 5, 9, "sign") > 1e-3
    # g s for g / s
    assert _mode_error(table, 5, 9, "gs_product") > 1e-3 and _invariant_drift(table, "gs_product") > 1e-6
    # the centre not corrected: see test_sum_of_weights
    assert not _sum_ok(rd.weights32(mistake="centre"))
