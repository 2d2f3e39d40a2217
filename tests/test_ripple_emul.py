"""The ripple layer's arithmetic (datum_amd/csrc/ocean_ripple.h), the very functions the kernels of ocean_ripple.hip call, walked on the
CPU (tests/cpu/ripple_emul.cpp) against ripple64's numpy float32 restatement, bit for bit:

  * the sub-step: R = 64 and 128, origins (0, 0) and (37, -21), 1, 3 and 16 sub-steps, the sponge on and off, random state and src;
  * the splat: 10^5 random deposits change the plane's sum by sum Q exactly; every edge of the window drops what lies outside;
    non-finite and out-of-range deposits; the clamp;
  * the surge pair cancels to zero where e.xy = 0;
  * wake_terms record for record, and the src plane it leaves; the sampler.

The restatement's worst distance from its own float64 form over the sub-step cases, in units of eps max|eta|, is the bar the device is
held to: K_RIP (ripple64.py) is 3 x that measured value, test_k_rip checks that it still is at least that.
"""

import ctypes
import os

import numpy as np
import pytest

import body64
import drag64
import ripple64
from test_body_emul import _case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
EPS = 2.0 ** -24
CASES = [(R, o, n, B) for R in (64, 128) for o in ((0, 0), (37, -21)) for n in (1, 3, 16) for B in (8, 0)]


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ripple_emul_substep.argtypes = [P, P, P, I, I, I, I, Fl, Fl, P, I]
    lib.ripple_emul_splat.argtypes = [P, I, I, I, Fl, P, I]
    lib.ripple_emul_splat.restype = ctypes.c_longlong
    lib.ripple_emul_sample.argtypes = [P, I, I, I, Fl, P, I, P]
    lib.ripple_emul_wake.argtypes = [P, P, I, P, I, P, P, Fl, P, I, I, I, Fl, P]
    lib.ripple_emul_window.argtypes = [I, I, I, P]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _emul_step(emul, lay, dt, substeps):
    h, c2s2, f = ripple64.params(lay.c, lay.s, lay.gamma, lay.B, lay.sponge_gamma, dt, substeps)
    state = np.ascontiguousarray(lay.state(), F)
    src = lay.src.copy()
    for i in range(substeps):
        out = np.empty_like(state)
        emul.ripple_emul_substep(_p(state), _p(out), _p(src), lay.R, lay.ox, lay.oy, lay.B, float(h), float(c2s2), _p(f), int(i == 0))
        state = out
        src[:] = 0
    return state


def _random_layer(R, origin, B, dtype, seed):
    rng = np.random.default_rng(seed)
    lay = ripple64.Layer(R, 0.5, dtype, B=B)
    lay.move(*origin)
    lay.set_window(rng.normal(size=(R, R)).astype(F), rng.normal(size=(R, R)).astype(F), rng.integers(-2 ** 21, 2 ** 21, (R, R)))
    return lay


def _step_case(emul, R, origin, substeps, B):
    """one case: the header's walk and the restatement's state after the call, and the restatement's distance from float64 in eps max|eta|"""
    lay = _random_layer(R, origin, B, F, R + substeps)
    l64 = _random_layer(R, origin, B, np.float64, R + substeps)
    got = _emul_step(emul, lay, 0.1 * substeps, substeps)
    lay.step(0.1 * substeps, substeps)
    l64.step(0.1 * substeps, substeps)
    return got, lay, np.abs(lay.eta.astype(np.float64) - l64.eta).max() / (EPS * np.abs(l64.eta).max())


@pytest.mark.parametrize("R,origin,substeps,B", CASES)
def test_substep_bits(emul, R, origin, substeps, B):
    got, lay, _ = _step_case(emul, R, origin, substeps, B)
    assert np.array_equal(_bits(got), _bits(lay.state())), np.argwhere(_bits(got) != _bits(lay.state()))[:4]
    assert np.all(lay.src == 0)


def test_k_rip(emul):
    """K_RIP is 3 x the restatement's worst distance from float64 over the cases above (measured here, not on the GPU)"""
    dist = {case: _step_case(emul, *case)[2] for case in CASES}
    worst = max(dist.values())
    print(f"ripple restatement vs float64: worst {worst:.2f} eps max|eta| at {max(dist, key=dist.get)}; K_RIP = {ripple64.K_RIP}")
    assert 3 * worst <= ripple64.K_RIP <= 4.5 * worst


def test_addressing(emul):
    R = 64
    for I, J in [(0, 0), (-1, -1), (63, 64), (-64, 65), (2 ** 30, -2 ** 30), (37, -21)]:
        assert emul.ripple_emul_index(I, J, R) == (J % R) * R + (I % R)
    for ox, oy in [(0, 0), (37, -21), (2 ** 30 - 10, -2 ** 30)]:
        for I, J, want in [(ox, oy, 1), (ox - 1, oy, 0), (ox, oy - 1, 0), (ox + R - 1, oy + R - 1, 1), (ox + R, oy, 0), (ox, oy + R, 0)]:
            assert emul.ripple_emul_inside(R, ox, oy, I, J) == want
    wx, wy = ripple64.window_coords(R, 0, 0)
    for B in (0, 1, 8, 64):
        k = ripple64.sponge_index(wx, wy, R, B)
        assert all(emul.ripple_emul_sponge(int(x), int(y), R, B) == k[y, x] for x in (0, 1, 7, 8, 31, 32, 56, 62, 63) for y in (0, 5, 8, 33, 63))


@pytest.mark.parametrize("R", (64, 128))
def test_window_rectangles(emul, R):
    """ripple_window, by whose rectangles the host copies a plane out in window order: with both coordinates of the origin from the list,
    the rectangles number at most four, none is empty, each lies within the rows it starts in, they are disjoint and cover R^2 cells, and
    a plane of cell indices scattered through them is plane[(J mod R), (I mod R)] at the window's (I, J)"""
    plane = np.arange(R * R).reshape(R, R)
    wy, wx = np.mgrid[0:R, 0:R]
    rects = np.zeros((4, 4), np.int32)
    for ox in (-R // 2, 0, 1, R // 2, R - 1, -1, -R - 3, 5 * R + 17):
        for oy in (-R // 2, 0, 1, R // 2, R - 1, -1, -R - 3, 5 * R + 17):
            n = emul.ripple_emul_window(ox, oy, R, _p(rects))
            assert 1 <= n <= 4, (ox, oy, n)
            window = np.full((R, R), -1)
            for src, dst, w, h in rects[:n].tolist():
                assert w > 0 and h > 0, (ox, oy, w, h)
                sy, sx, dy, dx = src // R, src % R, dst // R, dst % R
                assert 0 <= src and sx + w <= R and sy + h <= R and 0 <= dst and dx + w <= R and dy + h <= R, (ox, oy, src, dst, w, h)
                assert np.all(window[dy:dy + h, dx:dx + w] == -1), (ox, oy)          # disjoint
                window[dy:dy + h, dx:dx + w] = plane[sy:sy + h, sx:sx + w]
            assert sum(w * h for _, _, w, h in rects[:n].tolist()) == R * R
            assert np.array_equal(window, plane[(oy + wy) % R, (ox + wx) % R]), (ox, oy)


def _emul_splat(emul, lay, imp):
    src = lay.src.copy()
    dropped = emul.ripple_emul_splat(_p(src), lay.R, lay.ox, lay.oy, float(lay.invs), _p(np.ascontiguousarray(imp, F)), len(imp))
    return src, dropped


def test_splat_sum_exact(emul):
    """10^5 random deposits well inside the window: the plane's sum changes by sum Q exactly, and the plane is numpy's"""
    rng = np.random.default_rng(1)
    lay = ripple64.Layer(128, 0.5)
    lay.move(37, -21)
    n = 100000
    imp = np.zeros((n, 4), F)
    imp[:, 0] = rng.uniform((37 + 2) * 0.5, (37 + 126) * 0.5, n)
    imp[:, 1] = rng.uniform((-21 + 2) * 0.5, (-21 + 126) * 0.5, n)
    imp[:, 2] = rng.normal(size=n) * 1e-3
    src, dropped = _emul_splat(emul, lay, imp)
    assert dropped == 0 and lay.deposit(imp).sum() == 0
    assert np.array_equal(src, lay.src)
    Q = np.rint((imp[:, 2] * (lay.invs * lay.invs)) * ripple64.PER_METRE).astype(np.int64)
    assert np.abs(Q).max() > 1000 and int(src.astype(np.int64).sum()) == int(Q.sum())


def test_splat_edges_clamp_and_refusals(emul):
    R, s = 64, 0.5
    lay = ripple64.Layer(R, s)
    lay.move(37, -21)
    x0, y0, x1, y1 = 37 * s, -21 * s, (37 + R) * s, (-21 + R) * s
    mid = (x0 + x1) / 2, (y0 + y1) / 2
    # one deposit astride each edge (half its quanta outside) and each corner (three quarters outside); a cell centre on the very edge
    imp = [(x0, mid[1], 1), (x1, mid[1], 1), (mid[0], y0, 1), (mid[0], y1, 1), (x0, y0, 1), (x1, y0, 1), (x0, y1, 1), (x1, y1, 1),
           (x0 + 0.25, y0 + 0.25, 1), (x1 - 0.25, y1 - 0.25, 1), (x0 - 0.26, mid[1], 1), (x1 + 0.26, mid[1], 1)]
    imp = np.array([(x, y, v, 0) for x, y, v in imp], F)
    want_dropped = [2, 2, 2, 2, 3, 3, 3, 3, 0, 0, 4, 4]
    for k in range(len(imp)):
        one = ripple64.Layer(R, s)
        one.move(37, -21)
        src, dropped = _emul_splat(emul, one, imp[k:k + 1])
        d = one.deposit(imp[k:k + 1])
        assert np.array_equal(src, one.src) and dropped == d.sum()
        # astride an edge the weights are exact halves and quarters: the quanta outside are non-zero
        assert dropped == want_dropped[k], (k, dropped)
        Q = int(np.rint(np.float64(imp[k, 2]) * 4 * 2 ** 20))
        assert int(src.sum()) == Q * (4 - dropped) // 4
    # the clamp, and what deposits nothing
    big = np.array([(mid[0] + 0.25, mid[1] + 0.25, 1e30, 0), (mid[0] + 0.25, mid[1] + 0.25, -1e30, 0), (mid[0] + 1.25, mid[1] + 0.25, 1e30, 0)], F)
    src, dropped = _emul_splat(emul, lay, big)
    assert dropped == 0 and np.count_nonzero(src) == 1 and src.sum() == 2 ** 30
    none = np.array([(np.nan, 0, 1, 0), (0, np.inf, 1, 0), (mid[0], mid[1], np.nan, 0), (mid[0], mid[1], np.inf, 0), (2.0 ** 30 * s, mid[1], 1, 0),
                     (mid[0], -2.0 ** 30 * s, 1, 0), (3e38, 3e38, 1, 0), (mid[0], mid[1], 1e-9, 0)], F)
    src, dropped = _emul_splat(emul, lay, none)
    assert dropped == 0 and not src.any() and lay.deposit(none).sum() == 0 and not lay.src.any()


def test_sampler_bits(emul):
    rng = np.random.default_rng(2)
    for R, origin in [(64, (37, -21)), (128, (0, 0))]:
        lay = _random_layer(R, origin, 8, F, 5)
        s = 0.5
        x0, y0 = origin[0] * s, origin[1] * s
        p = np.stack([rng.uniform(x0 - 4, x0 + R * s + 4, 5000), rng.uniform(y0 - 4, y0 + R * s + 4, 5000)], 1).astype(F)
        p[::50] = np.floor(p[::50] * 2) / 2 + 0.25                                  # cell centres
        p[1::50, 0], p[2::50, 1] = x0, y0 + R * s                                   # the window's edges
        p[3::500, 0], p[4::500, 1], p[5::500, 0] = np.nan, np.inf, 1e30
        out = np.empty((len(p), 4), F)
        emul.ripple_emul_sample(_p(np.ascontiguousarray(lay.state(), F)), R, lay.ox, lay.oy, float(lay.invs), _p(p), len(p), _p(out))
        want = lay.sample(p)
        nan = np.isnan(want)
        assert nan.any() and np.array_equal(np.isnan(out), nan) and np.array_equal(_bits(out)[~nan], _bits(want)[~nan])
        assert np.all(want[5::500] == 0)
        # at a cell centre the sample is the cell
        c = p[::50]
        inside = (c[:, 0] > x0) & (c[:, 0] < x0 + R * s) & (c[:, 1] > y0) & (c[:, 1] < y0 + R * s) & np.isfinite(c).all(1)
        I, J = np.floor(c[inside, 0] * 2).astype(int), np.floor(c[inside, 1] * 2).astype(int)
        assert np.array_equal(_bits(want[::50][inside][:, 0]), _bits(lay.eta[J & (R - 1), I & (R - 1)]))


def _wake_case(seed, counts):
    rng = np.random.RandomState(seed)
    bodies, probes = _case(rng, counts)
    bodies["position"][:, :2] = rng.uniform(-15, 15, (len(bodies), 2))
    motions = drag64.make_motions(rng.uniform(-3, 3, (len(bodies), 3)), rng.uniform(-1, 1, (len(bodies), 3)), np.ones(len(bodies)), np.ones(len(bodies)))
    off, rows = body64.offsets(bodies, len(probes))
    recs = np.zeros((rows, 8), F)
    recs[:, 2] = rng.uniform(-4, 3, rows)
    recs[:, 3] = rng.uniform(0, 1e-3, rows)
    recs[:, 4:7] = rng.normal(size=(rows, 3)) * (2.0, 2.0, 1.0)
    return bodies, motions, probes, off, recs


def _emul_wake(emul, bodies, motions, probes, off, recs, dt, lay):
    src = lay.src.copy()
    out = np.empty((len(bodies), 8), F)
    emul.ripple_emul_wake(_p(bodies), _p(motions), len(bodies), _p(probes), len(probes), _p(np.ascontiguousarray(off, np.int64)), _p(recs), dt, _p(src), lay.R,
                          lay.ox, lay.oy, float(lay.invs), _p(out))
    return out, src


def _same(got, want):
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(_bits(got)[~gn], _bits(want)[~wn])


def test_wake_records_and_plane(emul):
    counts = [0, 1, 63, 64, 65, 129, 1000]
    bodies, motions, probes, off, recs = _wake_case(3, counts)
    for R, cell in [(128, 0.5), (64, 0.25)]:                                      # the second window is too small: quanta are dropped
        lay = ripple64.Layer(R, cell)
        got, src = _emul_wake(emul, bodies, motions, probes, off, recs, 0.05, lay)
        want = ripple64.wake32(bodies, motions, probes, recs, 0.05, lay.src, lay.ox, lay.oy, lay.invs)
        assert _same(got, want), np.argwhere(_bits(got) != _bits(want))[:4]
        assert np.array_equal(src, lay.src) and np.count_nonzero(src) > 100
        assert (want[:, 3] > 0).any() == (R == 64)
        assert np.array_equal(_bits(got[:, 6]), _bits(drag64.reduce32(bodies, motions, probes, recs)[:, 6]))
    # a bad motion and a bad range: NaNs, nothing deposited for them
    m2, b2 = motions.copy(), bodies.copy()
    m2["angular"][3, 0] = np.nan
    b2["cap"][5] = np.nan
    lay = ripple64.Layer(128, 0.5)
    got, src = _emul_wake(emul, b2, m2, probes, off, recs, 0.05, lay)
    live = body64._gather(bodies, probes)[0] != 5                                 # (a body with a bad range has no rows in the restatement)
    want = ripple64.wake32(b2, m2, probes, recs[live], 0.05, lay.src, lay.ox, lay.oy, lay.invs)
    assert np.isnan(got[[3, 5]]).all() and _same(got, want) and np.array_equal(src, lay.src)


def test_surge_pair_cancels_at_rest(emul):
    """e.xy = 0 (the hull moves with the water): the two surge splats have the same weights and cancel to the last unit; a probe that
    neither rises nor sinks adds no heave either"""
    bodies, motions, probes, off, recs = _wake_case(4, [64, 200])
    motions["angular"][:] = 0
    recs[:, 4:7] = motions["linear"][body64._gather(bodies, probes)[0]]
    lay = ripple64.Layer(128, 0.5)
    got, src = _emul_wake(emul, bodies, motions, probes, off, recs, 0.05, lay)
    assert not src.any() and np.all(got[:, :6] == 0) and got[:, 6].max() > 0
