"""Wake foam's arithmetic (datum_amd/csrc/ocean_ripple_foam.h), the very functions the kernels of ocean_ripple_foam.hip call, walked on the
CPU (tests/cpu/ripple_foam_emul.cpp) against ripple_foam64's numpy float32 restatement, bit for bit:

  * the update: R = 64 and 128, origins (0, 0) and (37, -11) -- ox mod 64 = 37, oy mod 16 = 5, the window's edge inside a tile -- over
    states that a few ripple64 sub-steps make of random impulses, three updates in a row with different dt and a layer step between them;
  * the window's edge cells and corners; each source alone (the other gain 0); dt = 0; the plane stays in [0, 1];
  * fmaxf's open case: two zeros of opposite sign give +0;
  * the sampler, on every edge of the window, with non-finite and far points;
  * the planted mistakes of ripple_foam64.MISTAKES each change the plane.

The restatement's worst distance from its own float64 form over the update cases, in units of eps (k1 max q + k2 max|eta_t| + 1), is the
bar K_RFOAM (ripple_foam64.py): 3 x that measured value; test_k_rfoam checks that it still is at least that.
"""

import ctypes
import os

import numpy as np
import pytest

import ripple64
import ripple_foam64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
EPS = 2.0 ** -24
ORIGINS = ((0, 0), (37, -11))
CASES = [(R, o) for R in (64, 128) for o in ORIGINS]
DTS = (0.05, 0.016, 0.11)


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ripple_foam_emul_update.argtypes = [P, P, I, I, I, P]
    lib.ripple_foam_emul_sample.argtypes = [P, I, I, I, Fl, P, I, P]
    lib.ripple_foam_emul_sample.restype = ctypes.c_longlong
    lib.ripple_foam_emul_max.argtypes = [Fl, Fl]
    lib.ripple_foam_emul_max.restype = Fl
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def impulses(R, origin, s, seed, n=160):
    """random deposits over the window and a little beyond it, some on its very edge: (n, 4) float32"""
    rng = np.random.default_rng(seed)
    lo = np.array(origin, np.float64) * s
    xy = lo + rng.uniform(-2 * s, (R + 2) * s, (n, 2))
    xy[:8, 0] = lo[0] + rng.uniform(0, s, 8)                 # the left edge's cells
    xy[8:16, 1] = lo[1] + (R - rng.uniform(0, 1, 8)) * s     # the top edge's cells
    xy[16] = lo + 0.25 * s                                   # two corners
    xy[17] = lo + (R - 0.25) * s
    imp = np.zeros((n, 4), F)
    imp[:, :2] = xy
    imp[:, 2] = rng.uniform(-0.15, 0.15, n)
    return imp


def layer(R, origin, dtype, seed):
    """a layer a few sub-steps after random impulses"""
    lay = ripple64.Layer(R, 0.5, dtype)
    lay.move(*origin)
    lay.deposit(impulses(R, origin, 0.5, seed))
    lay.step(0.09, 3)
    return lay


def _emul_update(emul, lay, plane, dt, **kw):
    p = np.array(ripple_foam64.params(lay.invs, dt, **dict(ripple_foam64.DEFAULTS, **kw)), F)
    foam = np.ascontiguousarray(plane, F).copy()
    state = np.ascontiguousarray(lay.state(), F)
    emul.ripple_foam_emul_update(_p(state), _p(foam), lay.R, lay.ox, lay.oy, _p(p))
    return foam


def _run(emul, R, origin, **kw):
    """three updates with a layer step between them: the header's planes, the restatement's, the float64 form's, and max q, max |eta_t|"""
    lay, l64 = layer(R, origin, F, R + 1), layer(R, origin, np.float64, R + 1)
    pl, p64 = ripple_foam64.Plane(lay, F, **kw), ripple_foam64.Plane(l64, np.float64, **kw)
    got, want, wide = [], [], []
    foam = pl.f.copy()
    qmax = rmax = 0.0
    for dt in DTS:
        foam = _emul_update(emul, lay, foam, dt, **kw)
        pl.step(dt)
        _, q, et = ripple_foam64.update(l64.eta, l64.rate, p64.f, l64.ox, l64.oy, ripple_foam64.params(l64.invs, dt, **p64.kw), np.float64, parts=True)
        qmax, rmax = max(qmax, q.max()), max(rmax, np.abs(et).max())
        p64.step(dt)
        got.append(foam.copy()), want.append(pl.f.copy()), wide.append(p64.f.copy())
        lay.step(dt, 2)
        l64.step(dt, 2)
    return got, want, wide, qmax, rmax


@pytest.mark.parametrize("R,origin", CASES)
def test_update_bits(emul, R, origin):
    got, want, _, _, _ = _run(emul, R, origin)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(g), _bits(w)), (k, np.argwhere(_bits(g) != _bits(w))[:4])
        assert w.min() >= 0 and w.max() <= 1
        # the window's edge rows and columns, and its corners, on their own
        win = lambda a: np.roll(a, (-(origin[1] & (R - 1)), -(origin[0] & (R - 1))), (0, 1))
        for sl in ((0, slice(None)), (R - 1, slice(None)), (slice(None), 0), (slice(None), R - 1)):
            assert np.array_equal(_bits(win(g)[sl]), _bits(win(w)[sl]))
    # the cases are not idle: coverage strictly inside (0, 1), at 0 and at 1, and foam on the window's edge
    last = want[-1]
    assert np.any((last > 0) & (last < 1)) and np.any(last == 0) and any(np.any(w == 1) for w in want)
    edge = np.concatenate([win(last)[0], win(last)[-1], win(last)[:, 0], win(last)[:, -1]])
    assert np.any(edge > 0)


def test_k_rfoam(emul):
    """K_RFOAM is 3 x the restatement's worst distance from float64 over the cases above (measured here, not on the GPU)"""
    dist = {}
    k1, k2 = ripple_foam64.DEFAULTS["k1"], ripple_foam64.DEFAULTS["k2"]
    for case in CASES:
        _, want, wide, qmax, rmax = _run(emul, *case)
        unit = EPS * (k1 * qmax + k2 * rmax + 1)
        dist[case] = max(np.abs(w.astype(np.float64) - d).max() for w, d in zip(want, wide)) / unit
    worst = max(dist.values())
    print(f"wake foam restatement vs float64: worst {worst:.2f} eps (k1 max q + k2 max|eta_t| + 1) at {max(dist, key=dist.get)}; K_RFOAM = {ripple_foam64.K_RFOAM}")
    assert 3 * worst <= ripple_foam64.K_RFOAM <= 4.5 * worst


@pytest.mark.parametrize("kw", [dict(k1=0.0), dict(k2=0.0), dict(k1=0.0, k2=0.0)])
def test_each_source_alone(emul, kw):
    R, origin = 64, ORIGINS[1]
    got, want, _, _, _ = _run(emul, R, origin, **kw)
    both = _run(emul, R, origin)[1]
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w))
    if len(kw) == 2:
        assert all(np.all(_bits(w) == 0) for w in want)         # no source: no foam, and +0 everywhere
    else:
        assert np.any(want[0] > 0) and np.any(want[0] != both[0]) and np.all(want[0] <= both[0])


def test_dt_zero_and_fade(emul):
    R, origin = 64, ORIGINS[1]
    lay = layer(R, origin, F, 7)
    rng = np.random.default_rng(3)
    old = rng.uniform(0, 1, (R, R)).astype(F)
    p = ripple_foam64.params(lay.invs, 0.0)
    assert p[5] == F(1)
    got = _emul_update(emul, lay, old, 0.0)
    want = ripple_foam64.update(lay.eta, lay.rate, old, lay.ox, lay.oy, p)
    assert np.array_equal(_bits(got), _bits(want)) and np.all(want >= old)
    # water at rest: the plane only fades, by the host's factor
    lay.eta[:], lay.rate[:] = 0, 0
    got = _emul_update(emul, lay, old, 0.25)
    assert np.array_equal(_bits(got), _bits(old * ripple_foam64.params(lay.invs, 0.25)[5]))
    # a decay that underflows: fade = +0
    assert ripple_foam64.params(lay.invs, 1e4, decay=1e4)[5] == 0
    assert np.all(_bits(_emul_update(emul, lay, old, 1e4, decay=1e4)) == 0)


def test_max_of_zeros(emul):
    """fmaxf's open case is decided: +0 of two zeros of opposite sign, in either order; every other pair as fmaxf"""
    nz, pz = F(-0.0), F(0.0)
    vals = [nz, pz, F(-1), F(1), F(np.nan), F(np.inf), F(-np.inf), F(1e-45)]
    for a in vals:
        for b in vals:
            got = F(emul.ripple_foam_emul_max(float(a), float(b)))
            want = F(ripple_foam64.fmax(a, b))
            assert _bits(got) == _bits(want) or (np.isnan(got) and np.isnan(want)), (a, b)
    assert _bits(F(emul.ripple_foam_emul_max(-0.0, 0.0))) == 0 and _bits(F(emul.ripple_foam_emul_max(0.0, -0.0))) == 0
    assert _bits(F(emul.ripple_foam_emul_max(-0.0, -0.0))) == 0x80000000


def sample_points(R, origin, s, seed, n=400):
    """points over the window and a margin, on each of its edges, and the special ones: non-finite, beyond 2^30 cells"""
    rng = np.random.default_rng(seed)
    lo = np.array(origin, np.float64) * s
    pts = (lo + rng.uniform(-3 * s, (R + 3) * s, (n, 2))).astype(F)
    k = 0
    for edge in (0.0, 0.5, 1.0, R - 1.0, R - 0.5, R + 0.0):    # the outermost centres, the edges, half a cell either side
        for axis in (0, 1):
            pts[k:k + 6, axis] = F(lo[axis] + edge * s)
            k += 6
    pts[k] = (np.nan, 1.0)
    pts[k + 1] = (1.0, np.inf)
    pts[k + 2] = (-np.inf, np.nan)
    pts[k + 3] = (3e9, 1.0)            # |x invs| >= 2^30
    pts[k + 4] = (1.0, -3e9)
    pts[k + 5] = (5e8, 1.0)            # below 2^30 cells, outside the window
    return pts, k


@pytest.mark.parametrize("R,origin", CASES)
def test_sampler(emul, R, origin):
    lay = layer(R, origin, F, R)
    pl = ripple_foam64.Plane(lay)
    pl.step(0.05)
    pts, k = sample_points(R, origin, 0.5, R)
    out = np.full(len(pts), 7, F)
    foam = np.ascontiguousarray(pl.f, F)
    fetched = emul.ripple_foam_emul_sample(_p(foam), R, lay.ox, lay.oy, float(lay.invs), _p(pts), len(pts), _p(out))
    want = pl.sample(pts)
    assert np.array_equal(_bits(out[np.isfinite(want)]), _bits(want[np.isfinite(want)]))
    assert np.all(np.isnan(out[k:k + 3])) and np.all(np.isnan(want[k:k + 3])) and np.all(_bits(out[k + 3:k + 6]) == 0)
    assert np.any(out > 0) and np.nanmin(out) >= 0 and np.nanmax(out) <= 1
    # the special points fetch nothing: the same count without them
    rest = np.delete(pts, np.s_[k:k + 6], 0)
    assert emul.ripple_foam_emul_sample(_p(foam), R, lay.ox, lay.oy, float(lay.invs), _p(np.ascontiguousarray(rest)), len(rest), _p(out)) == fetched
    # at a cell's centre the sample is the cell
    i, j = np.unravel_index(np.argmax(pl.window()), (R, R))
    centre = np.array([[(lay.ox + j + 0.5) * 0.5, (lay.oy + i + 0.5) * 0.5]], F)
    assert pl.sample(centre)[0] == pl.window()[i, j]


@pytest.mark.parametrize("mistake", ripple_foam64.MISTAKES)
def test_planted_mistakes_fail(emul, mistake):
    R, origin = 64, ORIGINS[1]
    lay = layer(R, origin, F, 11)
    pl, bad = ripple_foam64.Plane(lay), ripple_foam64.Plane(lay)
    foam = pl.f.copy()
    for dt in DTS[:2]:
        foam = _emul_update(emul, lay, foam, dt)
        pl.step(dt)
        bad.step(dt, mistake)
        lay.step(dt, 2)             # (the sources move on: what is left behind only fades)
    assert np.array_equal(_bits(foam), _bits(pl.f))
    assert not np.array_equal(_bits(foam), _bits(bad.f)), mistake
