"""The surface bounds' arithmetic (datum_amd/csrc/ocean_bounds.h), the very functions the kernels of ocean_bounds.hip call, walked on the
CPU (tests/cpu/bounds_emul.cpp):

  * the texel fold, as one run and as strided partials merged, over arrays with planted extrema, zeros of both signs, NaNs and infinities:
    the six extrema equal bounds64.fold's (numpy's fmin / fmax) by value, nonfinite exactly;
  * the slab bit for bit against bounds64.slab32, for lists of 1, 4 and 16, a NaN slab where a listed cascade has a non-finite texel;
  * ray_search_bounded against ray_search over ray_emul.cpp's two sinusoids with a slab that truly bounds them: all twelve floats of every
    record as bits -- bad rays and rays with NaN samples among them --, never more height evaluations, strictly fewer for a ray that
    starts above zhi, as many for a ray that lies wholly inside the slab;
  * a wrong slab (zhi below a crest) changes some record: the comparison can see a wrong skip.
"""

import ctypes
import os

import numpy as np
import pytest

import bounds64
from test_ray_emul import WAVES, _bits, _cast, _fn, _rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
P, I = ctypes.c_void_p, ctypes.c_int

# ray_height_waves with WAVES: |h - 0.1| <= 0.9 + 0.35
ZLO, ZHI = F(-1.2), F(1.4)


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    lib.ray_cast.argtypes = [P, ctypes.c_int64, I, ctypes.c_float, I, P, P, P, P]
    lib.bounds_fold.argtypes = [P, ctypes.c_int64, I, P]
    lib.bounds_slab_eval.argtypes = [P, P, I, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, P]
    lib.bounds_cast.argtypes = [P, ctypes.c_int64, I, ctypes.c_float, I, ctypes.c_float, ctypes.c_float, P, P, P, P]
    return lib


def _fold(emul, texels, parts):
    t = np.ascontiguousarray(texels, F)
    rec = np.full(8, -7.0, F)
    emul.bounds_fold(t.ctypes.data, len(t), parts, rec.ctypes.data)
    return rec


def _same_record(got, want):
    return np.array_equal(got[:6], want[:6]) and _bits(got[6:]).tolist() == _bits(want[6:]).tolist()


def test_record_floats(emul):
    from datum_amd import capi

    assert emul.bounds_record_floats() == capi.BOUNDS_RECORD_FLOATS == bounds64.RECORD_FLOATS == 8


@pytest.mark.parametrize("parts", [1, 4, 170, 1024])
def test_fold(emul, parts):
    rng = np.random.RandomState(parts)
    n = 4096
    base = rng.uniform(-1, 1, (n, 4)).astype(F)
    base[:, 3] = np.nan                                        # nx is not read

    def check(t, nonfinite):
        got, want = _fold(emul, t, parts), bounds64.fold(t[:, 0], t[:, 1], t[:, 2])
        assert _same_record(got, want), (parts, got, want)
        assert got[6] == nonfinite and got[7] == 0
        return got

    got = check(base, 0)
    assert got[0] == base[:, 2].min() and got[3] == base[:, 0].max()

    # a planted maximum and a planted minimum of each component, at the ends and inside
    for ch, k in ((0, 2), (1, 4), (2, 0)):
        for pos in (0, n - 1, 15, 2049):
            for v in (5.0, -5.0):
                t = base.copy()
                t[pos, ch] = v
                got = check(t, 0)
                assert got[k + (1 if v > 0 else 0)] == F(v)

    # zeros of both signs alone: the extrema are zero whatever the sign
    z = np.zeros((n, 4), F)
    z[::3, :3] = -0.0
    got = check(z, 0)
    assert np.all(got[:6] == 0)

    # NaNs enter no extremum, infinities do; both are counted, a texel once
    t = base.copy()
    t[7, 0] = np.nan
    t[7, 1] = np.inf
    t[100, 2] = np.nan
    t[4095, 1] = -np.inf
    t[2000, 0] = np.inf
    got = check(t, 4)
    assert got[3] == np.inf and got[4] == -np.inf and got[5] == np.inf and np.isfinite(got[:3]).all()

    # nothing but NaNs: the identity
    t = np.full((64, 4), np.nan, F)
    got = check(t, 64)
    assert np.all(got[[0, 2, 4]] == np.inf) and np.all(got[[1, 3, 5]] == -np.inf)


@pytest.mark.parametrize("count", [1, 4, 16])
def test_slab(emul, count):
    rng = np.random.RandomState(count)
    for trial in range(200):
        records = np.zeros((16, 8), F)
        lo, hi = -rng.uniform(0, 3, (16, 3)), rng.uniform(0, 3, (16, 3))
        if trial % 5 == 0:
            lo, hi = np.minimum(lo, hi) + 1.0, np.maximum(lo, hi) + 1.0          # both extrema on one side of zero
        records[:, 0:6:2], records[:, 1:6:2] = lo, hi
        if trial % 7 == 3:
            records[rng.randint(16), 6] = 1                                       # a non-finite texel somewhere (listed or not)
        if trial == 11:
            records[:] = 0
        cascades = rng.randint(0, 16, count).astype(np.int32)                    # cascades may repeat
        basez, A, gx, gy = F(rng.uniform(-2, 2)), F(rng.uniform(-1, 1)), F(rng.uniform(-1, 1)), F(rng.uniform(-1, 1))
        if trial == 11:
            basez = A = F(0)
        out = np.full(4, -7.0, F)
        emul.bounds_slab_eval(records.ctypes.data, cascades.ctypes.data, count, basez, A, gx, gy, out.ctypes.data)
        zlo, zhi, rx, ry, pad = bounds64.slab32(records, cascades, basez, A, gx, gy)
        assert _bits(out).tolist() == _bits(np.array([zlo, zhi, rx, ry], F)).tolist(), (count, trial)
        listed_bad = bool(records[cascades, 6].any())
        assert np.isnan(out[:2]).all() == listed_bad and np.isnan(out[:2]).any() == listed_bad
        if not listed_bad:
            assert out[0] <= out[1] and np.isfinite(out).all()
        if trial == 11:
            assert np.all(out[:2] == 0) and out[2] == abs(gx) and out[3] == abs(gy)      # mag = 0: no pad


def _cast_bounded(emul, fn, user, rays, S, R, zlo, zhi):
    rays = np.ascontiguousarray(rays, F)
    out = np.full((len(rays), 12), -7.0, F)
    calls = np.zeros(len(rays), np.int32)
    emul.bounds_cast(rays.ctypes.data, len(rays), S, F(1.0) / F(S), R, zlo, zhi, fn, user.ctypes.data, out.ctypes.data, calls.ctypes.data)
    return out, calls


def _ray_set(seed):
    """test_ray_emul's rays (origins from 3 below to 3.5 above), then rays wholly inside the slab, wholly above, wholly below, from far
    above down through it, bad rays, and rays whose parameter range overflows (NaN samples)"""
    rng = np.random.RandomState(seed)
    general = _rays(seed, 2048)

    def segment(n, z0, z1):
        r = np.zeros((n, 8), F)
        r[:, 0:2] = rng.uniform(-40, 40, (n, 2))
        r[:, 2] = z0
        az, run = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 30, n)
        r[:, 4], r[:, 5], r[:, 6] = run * np.cos(az), run * np.sin(az), z1 - z0
        r[:, 3], r[:, 7] = 0.0, 1.0
        return r

    inside = segment(256, rng.uniform(-1.1, 1.3, 256), rng.uniform(-1.1, 1.3, 256))
    above = segment(128, rng.uniform(1.5, 30, 128), rng.uniform(1.5, 30, 128))
    below = segment(128, rng.uniform(-30, -1.3, 128), rng.uniform(-30, -1.3, 128))
    fan = segment(256, rng.uniform(20, 60, 256), rng.uniform(-5, -1.3, 256))
    bad = _rays(seed + 1, 16)
    for k in range(8):
        bad[2 * k, k] = np.nan
        bad[2 * k + 1, k] = np.inf
    overflow = np.array([[0, 0, 1, -3.0e38, 0, 0, -1e-38, 3.0e38], [0, 0, -1, -3.0e38, 0, 0, -1e-38, 3.0e38],
                         [0, 0, 50, -3.0e38, 1e-38, 0, -1e-37, 3.0e38], [0, 0, -50, -3.0e38, 0, 1e-38, 1e-37, 3.0e38]], F)
    rays = np.concatenate([general, inside, above, below, fan, bad, overflow])
    kinds = np.concatenate([np.full(len(a), k) for k, a in enumerate((general, inside, above, below, fan, bad, overflow))])
    return rays, kinds


@pytest.mark.parametrize("S", [1, 7, 32, 1024])
def test_bounded_search_is_the_search(emul, S):
    fn = _fn(emul, "ray_height_waves")
    rays, kinds = _ray_set(S)
    r64 = rays.astype(np.float64)
    zstart = (rays[:, 2] + rays[:, 3] * rays[:, 6]).astype(F)                    # point(tmin).z as the walk forms it
    for R in (0, 12, 24):
        want, calls = _cast(emul, fn, WAVES, rays, S, R)
        got, bcalls = _cast_bounded(emul, fn, WAVES, rays, S, R, ZLO, ZHI)
        assert np.array_equal(_bits(got), _bits(want)), (S, R, np.argwhere(_bits(got) != _bits(want))[:4], kinds[np.argwhere(_bits(got) != _bits(want))[:4, 0]])
        assert np.isnan(got[kinds == 5]).all() and np.all(bcalls[kinds == 5] == 0)
        assert np.all(bcalls <= calls)
        good = kinds != 5
        starts_above = good & (zstart > ZHI) & (kinds != 6)
        assert starts_above.sum() > 300 and np.all(bcalls[starts_above] < calls[starts_above])
        assert np.array_equal(bcalls[kinds == 1], calls[kinds == 1])
        # wholly above, wholly below: the record's evaluation alone
        assert np.all(bcalls[kinds == 2] == 1) and np.all(bcalls[kinds == 3] == 1)
        assert np.all(got[kinds == 2, 3] == 0) and np.all(got[kinds == 3, 3] == 0) and np.all(got[kinds == 3, 2] < 0)
        # the fan crosses: ENTER for every ray, with far fewer evaluations at a long march
        assert np.all(got[kinds == 4, 3] == 1)
        if S >= 32 and R == 0:                              # (the slab is at most 2.6 of the 21.3 or more the ray descends)
            assert bcalls[kinds == 4].sum() * 4 < calls[kinds == 4].sum()
        for v in (0, 1, 2):
            assert (got[good, 3] == v).sum() > 40
    assert np.isfinite(r64[kinds != 5]).all()


def test_a_nan_slab_skips_nothing(emul):
    fn = _fn(emul, "ray_height_waves")
    rays, _ = _ray_set(3)
    want, calls = _cast(emul, fn, WAVES, rays, 32, 8)
    for zlo, zhi in ((np.nan, np.nan), (np.nan, ZHI), (ZLO, np.nan)):
        got, bcalls = _cast_bounded(emul, fn, WAVES, rays, 32, 8, F(zlo), F(zhi))
        assert np.array_equal(_bits(got), _bits(want))
        if np.isnan(zlo) and np.isnan(zhi):
            assert np.array_equal(bcalls, calls)


def test_a_wrong_slab_is_seen(emul):
    fn = _fn(emul, "ray_height_waves")
    rays, kinds = _ray_set(5)
    want, _ = _cast(emul, fn, WAVES, rays, 32, 8)
    got, _ = _cast_bounded(emul, fn, WAVES, rays, 32, 8, ZLO, F(0.5))            # crests reach 1.35
    differ = (_bits(got) != _bits(want)).any(1)
    assert differ.any() and not differ[kinds == 5].any()
    got, _ = _cast_bounded(emul, fn, WAVES, rays, 32, 8, F(-0.3), ZHI)           # troughs reach -1.15
    assert (_bits(got) != _bits(want)).any()
