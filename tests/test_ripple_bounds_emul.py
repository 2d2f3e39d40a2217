"""The ripple-layer bounds' arithmetic (datum_amd/csrc/ocean_ripple_bounds.h), the very functions the kernels of ocean_ripple_bounds.hip and
datum_ocean_surface_slab_rippled call, walked on the CPU (tests/cpu/ripple_bounds_emul.cpp):

  * the cell fold against ripple_bounds64.fold (numpy's fmin / fmax) by value, the counts exactly, on R = 64 states: random, all zero, one
    NaN, one +inf, one cell with only a rate; the merge under 20 shuffles of the partials;
  * the rippled slab bit for bit against ripple_bounds64.slab32, for lists of 1, 4 and 16, a NaN slab where a listed cascade or the layer
    has a non-finite value, and datum_ocean_surface_slab's own slab over a layer at rest;
  * ray_search_bounded over the rippled height with the rippled slab against ray_search over the same height: all twelve floats of every
    record as bits, on test_bounds_emul.py's ray families (restated here), with rays that graze etamax over the window and cross its edge;
  * each planted mistake of ripple_bounds64 changes the slab's bits, and the two that lower zhi put a height outside it and change a record.
"""

import ctypes
import os

import numpy as np
import pytest

import bounds64
import ripple64
import ripple_bounds64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
P, I, L, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float

# ray_height_waves with these: |h - 0.1| <= 0.9 + 0.35 (tests/test_ray_emul.py's surface)
WAVES = np.array([0.9, 0.21, 0.13, 0.3, 0.35, -0.8, 0.55, 1.7, 0.1], F)
# its "cascade": basez = 0.1 and one record with the amplitude's sum for extrema, nothing non-finite
BASEZ = F(0.1)
WAVE_RECORDS = np.array([[-1.25, 1.25, 0, 0, 0, 0, 0, 0]], F)
ORIGIN = (37, -21)


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    lib.ripple_bounds_fold.argtypes = [P, L, I, P, P]
    lib.ripple_bounds_slab_eval.argtypes = [P, P, I, Fl, Fl, Fl, Fl, P, P]
    lib.bounds_slab_eval.argtypes = [P, P, I, Fl, Fl, Fl, Fl, P]
    lib.ripple_bounds_heights.argtypes = [P, P, P, I, I, I, Fl, P, L, P]
    lib.ripple_bounds_cast.argtypes = [P, L, I, Fl, I, I, Fl, Fl, P, P, P, I, I, I, Fl, P, P]
    for f in (lib.ripple_bounds_fold, lib.ripple_bounds_slab_eval, lib.bounds_slab_eval, lib.ripple_bounds_heights, lib.ripple_bounds_cast):
        f.restype = None
    return lib


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _fold(emul, state, parts, order=None):
    st = np.ascontiguousarray(state, F).reshape(-1, 2)
    rec = np.full(8, -7.0, F)
    o = None if order is None else np.ascontiguousarray(order, np.int32)
    emul.ripple_bounds_fold(st.ctypes.data, len(st), parts, None if o is None else o.ctypes.data, rec.ctypes.data)
    return rec


def _same_record(got, want):
    return np.array_equal(got[:4], want[:4]) and _bits(got[4:]).tolist() == _bits(want[4:]).tolist()


def _states():
    """R = 64 states [4096, 2] by name, with the counts (nonfinite, active) each must give"""
    rng = np.random.RandomState(64)
    rand = np.stack([rng.uniform(-0.3, 0.3, 4096), rng.uniform(-1, 1, 4096)], 1).astype(F)
    zero = np.zeros((4096, 2), F)
    zero[::3] = -0.0
    nan = rand.copy()
    nan[1234, 0] = np.nan
    inf = rand.copy()
    inf[4095, 0] = np.inf
    rate = np.zeros((4096, 2), F)
    rate[77, 1] = -2.5
    nanrest = np.zeros((4096, 2), F)
    nanrest[0, 1] = np.nan
    return {"random": (rand, 0, 4096), "zero": (zero, 0, 0), "nan": (nan, 1, 4096), "inf": (inf, 1, 4096), "rate_only": (rate, 0, 1),
            "nan_at_rest": (nanrest, 1, 1)}


def test_record_floats(emul):
    from datum_amd import capi

    assert emul.ripple_bounds_record_floats() == capi.RIPPLE_BOUNDS_RECORD_FLOATS == ripple_bounds64.RECORD_FLOATS == 8


@pytest.mark.parametrize("parts", [1, 8, 170, 2048])
def test_fold(emul, parts):
    for name, (st, nonfinite, active) in _states().items():
        got, want = _fold(emul, st, parts), ripple_bounds64.fold(st)
        assert _same_record(got, want), (name, parts, got, want)
        assert got[4] == nonfinite and got[5] == active and got[6] == 0 and got[7] == 0, (name, got)
    st = _states()
    assert np.all(_fold(emul, st["zero"][0], parts)[:4] == 0)
    got = _fold(emul, st["nan"][0], parts)
    assert np.isfinite(got[:4]).all() and got[0] == np.nanmin(st["nan"][0][:, 0])
    assert _fold(emul, st["inf"][0], parts)[1] == np.inf
    got = _fold(emul, st["rate_only"][0], parts)
    assert got[2] == F(-2.5) and got[3] == 0 and got[0] == 0 and got[1] == 0
    # planted extrema at the ends and inside
    for pos in (0, 4095, 511, 2049):
        for v in (5.0, -5.0):
            for ch in (0, 1):
                t = st["random"][0].copy()
                t[pos, ch] = v
                assert _fold(emul, t, parts)[2 * ch + (1 if v > 0 else 0)] == F(v)
    # nothing but NaNs: the identity
    got = _fold(emul, np.full((64, 2), np.nan, F), parts)
    assert np.all(got[[0, 2]] == np.inf) and np.all(got[[1, 3]] == -np.inf) and got[4] == 64 and got[5] == 64


def test_merge_order(emul):
    rng = np.random.RandomState(20)
    for name, (st, _, _) in _states().items():
        want = _fold(emul, st, 8)
        for k in range(20):
            assert _same_record(_fold(emul, st, 8, rng.permutation(8)), want), (name, k)


def _slab(emul, records, cascades, basez, A, gx, gy, layer):
    records, layer = np.ascontiguousarray(records, F), np.ascontiguousarray(layer, F)
    cascades = np.ascontiguousarray(cascades, np.int32)
    out = np.full(4, -7.0, F)
    emul.ripple_bounds_slab_eval(records.ctypes.data, cascades.ctypes.data, len(cascades), basez, A, gx, gy, layer.ctypes.data, out.ctypes.data)
    return out


@pytest.mark.parametrize("count", [1, 4, 16])
def test_slab(emul, count):
    rng = np.random.RandomState(count)
    for trial in range(200):
        records = np.zeros((16, 8), F)
        lo, hi = -rng.uniform(0, 3, (16, 3)), rng.uniform(0, 3, (16, 3))
        if trial % 5 == 0:
            lo, hi = np.minimum(lo, hi) + 1.0, np.maximum(lo, hi) + 1.0
        records[:, 0:6:2], records[:, 1:6:2] = lo, hi
        if trial % 7 == 3:
            records[rng.randint(16), 6] = 1
        e = np.sort(rng.uniform(-0.5, 0.5, 2))
        if trial % 4 == 1:
            e = -np.abs(e)[::-1]                                  # all negative
        if trial % 4 == 2:
            e = np.abs(e)                                         # all positive
        layer = np.array([e[0], e[1], -1, 1, 0, 4096, 0, 0], F)
        if trial % 11 == 5:
            layer[4] = 2
        if trial % 13 == 6:
            layer[:] = 0                                          # at rest
        cascades = rng.randint(0, 16, count).astype(np.int32)
        basez, A, gx, gy = F(rng.uniform(-2, 2)), F(rng.uniform(-1, 1)), F(rng.uniform(-1, 1)), F(rng.uniform(-1, 1))
        out = _slab(emul, records, cascades, basez, A, gx, gy, layer)
        zlo, zhi, rx, ry, pad = ripple_bounds64.slab32(records, cascades, basez, A, gx, gy, layer)
        assert _bits(out).tolist() == _bits(np.array([zlo, zhi, rx, ry], F)).tolist(), (count, trial)
        bad = bool(records[cascades, 6].any()) or layer[4] > 0
        assert np.isnan(out[:2]).all() == bad and np.isnan(out[:2]).any() == bad
        # the parent's slab: the same reach, and over a layer at rest the same bits
        parent = np.full(4, -7.0, F)
        emul.bounds_slab_eval(records.ctypes.data, cascades.ctypes.data, count, basez, A, gx, gy, parent.ctypes.data)
        assert _bits(parent[2:]).tolist() == _bits(out[2:]).tolist()
        assert _bits(parent).tolist() == _bits(np.array(bounds64.slab32(records, cascades, basez, A, gx, gy)[:4], F)).tolist()
        if trial % 13 == 6:
            assert np.array_equal(parent, out, equal_nan=True), (count, trial)
        elif not bad:
            assert out[0] <= parent[0] and parent[1] <= out[1] and np.isfinite(out).all()


def _layer(R, cell, seed, lo=-0.3, hi=0.3):
    """tests/test_rippled_emul.py's layer state: the window at ORIGIN, wrapped round the torus in memory"""
    lay = ripple64.Layer(R, cell)
    lay.move(*ORIGIN)
    rng = np.random.RandomState(seed)
    lay.set_window(rng.uniform(lo, hi, (R, R)).astype(F), rng.uniform(-1, 1, (R, R)).astype(F))
    return lay


def _rays(seed, n):
    """tests/test_ray_emul.py's general rays: origins a few metres above or below the surface, any slope, up-going and down-going"""
    rng = np.random.RandomState(seed)
    r = np.empty((n, 8), F)
    r[:, 0:2] = rng.uniform(-40, 40, (n, 2))
    r[:, 2] = rng.uniform(-3, 3.5, n)
    az = rng.uniform(0, 2 * np.pi, n)
    el = np.radians(rng.uniform(2, 90, n)) * rng.choice([-1, 1], n)
    length = rng.uniform(0.3, 3.0, n)
    r[:, 4], r[:, 5], r[:, 6] = length * np.cos(el) * np.cos(az), length * np.cos(el) * np.sin(az), length * np.sin(el)
    r[:, 3] = rng.uniform(-1, 1, n)
    r[:, 7] = r[:, 3] + rng.uniform(0.5, 12, n) / length
    return r


def _ray_set(seed, lay, zlo, zhi, top):
    """tests/test_bounds_emul.py's families -- general rays, rays wholly inside the slab, wholly above, wholly below, a fan from far above,
    bad rays, rays whose parameter range overflows -- and nearly level rays that graze the highest water over the window (`top`: from 40 cm
    below it to 5 cm above) and cross the window's edge"""
    rng = np.random.RandomState(seed)
    general = _rays(seed, 2048)
    zlo, zhi = float(zlo), float(zhi)

    def segment(n, z0, z1):
        r = np.zeros((n, 8), F)
        r[:, 0:2] = rng.uniform(-40, 40, (n, 2))
        r[:, 2] = z0
        az, run = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 30, n)
        r[:, 4], r[:, 5], r[:, 6] = run * np.cos(az), run * np.sin(az), z1 - z0
        r[:, 3], r[:, 7] = 0.0, 1.0
        return r

    inside = segment(256, rng.uniform(zlo + 0.1, zhi - 0.1, 256), rng.uniform(zlo + 0.1, zhi - 0.1, 256))
    above = segment(128, rng.uniform(zhi + 0.1, 30, 128), rng.uniform(zhi + 0.1, 30, 128))
    below = segment(128, rng.uniform(-30, zlo - 0.1, 128), rng.uniform(-30, zlo - 0.1, 128))
    fan = segment(256, rng.uniform(20, 60, 256), rng.uniform(-5, zlo - 0.1, 256))
    bad = _rays(seed + 1, 16)
    for k in range(8):
        bad[2 * k, k] = np.nan
        bad[2 * k + 1, k] = np.inf
    overflow = np.array([[0, 0, 1, -3.0e38, 0, 0, -1e-38, 3.0e38], [0, 0, -1, -3.0e38, 0, 0, -1e-38, 3.0e38],
                         [0, 0, 50, -3.0e38, 1e-38, 0, -1e-37, 3.0e38], [0, 0, -50, -3.0e38, 0, 1e-38, 1e-37, 3.0e38]], F)
    # grazing: nearly level rays from outside the window across its left or lower edge, next to the slab's top
    n = 256
    graze = np.zeros((n, 8), F)
    cell = float(lay.s)
    x0, y0 = lay.ox * cell, lay.oy * cell
    side = rng.randint(0, 2, n)
    along = rng.uniform(0, 40, n)
    graze[:, 0] = np.where(side == 0, x0 - rng.uniform(1, 20, n), x0 + along)
    graze[:, 1] = np.where(side == 0, y0 + along, y0 - rng.uniform(1, 20, n))
    graze[:, 2] = top + rng.uniform(-0.4, 0.05, n)
    graze[:, 4] = np.where(side == 0, rng.uniform(25, 60, n), rng.uniform(-5, 5, n))
    graze[:, 5] = np.where(side == 0, rng.uniform(-5, 5, n), rng.uniform(25, 60, n))
    graze[:, 6] = rng.uniform(-0.08, 0.08, n)
    graze[:, 3], graze[:, 7] = 0.0, 1.0
    sets = (general, inside, above, below, fan, bad, overflow, graze)
    return np.concatenate(sets), np.concatenate([np.full(len(a), k) for k, a in enumerate(sets)])


def _cast(emul, lay, rays, S, R, slab=None):
    rays = np.ascontiguousarray(rays, F)
    state = np.ascontiguousarray(lay.state(), F)
    out = np.full((len(rays), 12), -7.0, F)
    calls = np.zeros(len(rays), np.int32)
    zlo, zhi = (F(0), F(0)) if slab is None else slab
    fn = ctypes.cast(emul.ray_height_waves, P)
    emul.ripple_bounds_cast(rays.ctypes.data, len(rays), S, F(1.0) / F(S), R, 0 if slab is None else 1, zlo, zhi, fn, WAVES.ctypes.data,
                            state.ctypes.data, lay.R, lay.ox, lay.oy, float(lay.invs), out.ctypes.data, calls.ctypes.data)
    return out, calls


def _heights(emul, lay, points, waves=WAVES):
    q = np.ascontiguousarray(points, F)
    state = np.ascontiguousarray(lay.state(), F)
    out = np.zeros(len(q), F)
    emul.ripple_bounds_heights(ctypes.cast(emul.ray_height_waves, P), waves.ctypes.data, state.ctypes.data, lay.R, lay.ox, lay.oy, float(lay.invs), q.ctypes.data, len(q), out.ctypes.data)
    return out


def _top(emul, lay):
    """the highest rippled water at the window's cell centres"""
    cell = float(lay.s)
    j, i = np.mgrid[0:lay.R, 0:lay.R]
    return float(_heights(emul, lay, np.stack([(lay.ox + i.ravel() + 0.5) * cell, (lay.oy + j.ravel() + 0.5) * cell], 1)).max())


def _wave_slab(emul, lay, mistake=None):
    layer = _fold(emul, lay.state(), 8)
    if mistake is None:
        out = _slab(emul, WAVE_RECORDS, [0], BASEZ, F(0), F(0), F(0), layer)
        return out[0], out[1], layer
    zlo, zhi, _, _, _ = ripple_bounds64.slab32(WAVE_RECORDS, [0], BASEZ, 0, 0, 0, layer, mistake)
    return zlo, zhi, layer


@pytest.mark.parametrize("S", [1, 7, 32, 1024])
def test_bounded_search_is_the_search(emul, S):
    lay = _layer(64, 1.0, 64)
    zlo, zhi, layer = _wave_slab(emul, lay)
    assert layer[0] < -0.29 and layer[1] > 0.29 and zlo < -1.44 and zhi > 1.64
    rays, kinds = _ray_set(S, lay, zlo, zhi, _top(emul, lay))
    zstart = (rays[:, 2] + rays[:, 3] * rays[:, 6]).astype(F)
    for R in (0, 12, 24):
        want, calls = _cast(emul, lay, rays, S, R)
        got, bcalls = _cast(emul, lay, rays, S, R, (zlo, zhi))
        assert np.array_equal(_bits(got), _bits(want)), (S, R, np.argwhere(_bits(got) != _bits(want))[:4], kinds[np.argwhere(_bits(got) != _bits(want))[:4, 0]])
        assert np.isnan(got[kinds == 5]).all() and np.all(bcalls[kinds == 5] == 0)
        assert np.all(bcalls <= calls)
        good = kinds != 5
        starts_above = good & (zstart > zhi) & (kinds != 6)
        assert starts_above.sum() > 300 and np.all(bcalls[starts_above] < calls[starts_above])
        assert np.array_equal(bcalls[kinds == 1], calls[kinds == 1])
        assert np.all(bcalls[kinds == 2] == 1) and np.all(bcalls[kinds == 3] == 1)
        assert np.all(got[kinds == 2, 3] == 0) and np.all(got[kinds == 3, 3] == 0) and np.all(got[kinds == 3, 2] < 0)
        assert np.all(got[kinds == 4, 3] == 1)
        for v in (0, 1, 2):
            assert (got[good, 3] == v).sum() > 40
        # the grazing rays: hits and misses both, and the layer decides some of them
        if S >= 32:
            assert (got[kinds == 7, 3] > 0).sum() > 10 and (got[kinds == 7, 3] == 0).sum() > 10
    # the layer is in the height: a layer at rest gives other records
    rest = ripple64.Layer(64, 1.0)
    rest.move(*ORIGIN)
    other, _ = _cast(emul, rest, rays, S, 12)
    assert (_bits(other) != _bits(_cast(emul, lay, rays, S, 12)[0])).any(1).mean() > 0.05


def test_a_nan_slab_skips_nothing(emul):
    lay = _layer(64, 1.0, 64)
    lay.eta[5, 9] = np.nan
    zlo, zhi, layer = _wave_slab(emul, lay)
    assert layer[4] == 1 and np.isnan(zlo) and np.isnan(zhi)
    rays, _ = _ray_set(3, lay, -1.5, 1.7, 1.6)
    want, calls = _cast(emul, lay, rays, 32, 8)
    got, bcalls = _cast(emul, lay, rays, 32, 8, (zlo, zhi))
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(bcalls, calls)


@pytest.mark.parametrize("mistake", ripple_bounds64.MISTAKES)
def test_planted_mistakes_are_seen(emul, mistake):
    """an all-negative layer over the window: outside it the water stands at the waves' own height, which the window's lowered top does not
    cover unless 0 is taken into the layer's interval"""
    lay = _layer(64, 1.0, 7, lo=-0.3, hi=-0.1)
    zlo, zhi, layer = _wave_slab(emul, lay)
    assert layer[1] < -0.09
    mlo, mhi, _ = _wave_slab(emul, lay, mistake)
    assert _bits(np.array([zlo, zhi], F)).tolist() != _bits(np.array([mlo, mhi], F)).tolist(), mistake
    rng = np.random.RandomState(8)
    q = rng.uniform(-200, 200, (20000, 2)).astype(F)
    h = _heights(emul, lay, q)
    assert np.all(h > zlo) and np.all(h < zhi)
    if mistake == "no_mag":
        # the pad alone is smaller: over this surface the bits of the slab tell, its heights do not.  Where the missing term matters: a
        # level sea at 0 -- no other magnitude -- under one raised cell.  Without the layer's term mag is 0 and so is the pad: zhi is etamax
        # itself, and the height at that cell's centre IS etamax, not strictly inside
        assert mhi < zhi and mlo > zlo
        bump = ripple64.Layer(64, 1.0)
        bump.move(*ORIGIN)
        eta = np.zeros((64, 64), F)
        eta[9, 7] = 1.0
        bump.set_window(eta, np.zeros((64, 64), F))
        level, none = np.zeros(9, F), np.zeros((1, 8), F)
        top = _heights(emul, bump, [[ORIGIN[0] + 7.5, ORIGIN[1] + 9.5]], level)[0]
        rec = _fold(emul, bump.state(), 8)
        good = _slab(emul, none, [0], F(0), F(0), F(0), F(0), rec)
        bad = ripple_bounds64.slab32(none, [0], 0, 0, 0, 0, rec, mistake)
        assert top == F(1.0) == rec[1] and good[0] < 0 < top < good[1]
        assert not top < bad[1], (top, bad[1])
        return
    assert (h > mhi).any(), (mistake, float(h.max()), float(mhi))
    rays, kinds = _ray_set(5, lay, zlo, zhi, _top(emul, lay))
    want, _ = _cast(emul, lay, rays, 32, 8)
    assert np.array_equal(_bits(_cast(emul, lay, rays, 32, 8, (zlo, zhi))[0]), _bits(want))
    assert (_bits(_cast(emul, lay, rays, 32, 8, (mlo, mhi))[0]) != _bits(want)).any(), mistake
