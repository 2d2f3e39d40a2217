"""The ray cast's arithmetic (datum_amd/csrc/ocean_ray.h), the very functions ocean_ray_kernel calls, walked on the CPU
(tests/cpu/ray_emul.cpp) over an analytic surface:

  * against ray64.cast32, the definition of include/datum_ocean_hip.h in numpy float32: all twelve floats bit for bit, on a plane and on
    two superposed sinusoids, 4096 random rays with every status among them, S in {1, 7, 32, 1024} and R in {0, 1, 12, 24}.  Both sides
    take the height from the SAME C function (ray_height_eval), so what is compared is the cast and nothing else;
  * the bad-ray rule on every field, on tmax < tmin and on end points that overflow;
  * t_S is tmax itself; tmin == tmax is a miss with lo = hi = tmax; a miss is not refined; a ray costs at most S + R + 2 evaluations.
"""

import ctypes
import os

import numpy as np
import pytest

import ray64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
P, I = ctypes.c_void_p, ctypes.c_int
HEIGHT_FN = ctypes.CFUNCTYPE(None, ctypes.c_float, ctypes.c_float, P, ctypes.POINTER(ctypes.c_float))

PLANE = np.array([0.05, -0.03, 0.4], F)
WAVES = np.array([0.9, 0.21, 0.13, 0.3, 0.35, -0.8, 0.55, 1.7, 0.1], F)


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    lib.ray_sizeof.restype = ctypes.c_size_t
    lib.ray_height_eval.argtypes = [P, P, P, ctypes.c_int64, P]
    lib.ray_bad_flags.argtypes = [P, ctypes.c_int64, P]
    lib.ray_samples.argtypes = [P, ctypes.c_int64, I, ctypes.c_float, P]
    lib.ray_cast.argtypes = [P, ctypes.c_int64, I, ctypes.c_float, I, P, P, P, P]
    return lib


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _fn(emul, name):
    return ctypes.cast(getattr(emul, name), P)


def _height(emul, fn, user):
    """ray64's height_fn over a C callback: records [M, 8] above points [M, 2]"""
    def height(q):
        q = np.ascontiguousarray(q, F)
        out = np.empty((len(q), 8), F)
        emul.ray_height_eval(fn, user.ctypes.data, q.ctypes.data, len(q), out.ctypes.data)
        return out
    return height


def _cast(emul, fn, user, rays, S, R):
    rays = np.ascontiguousarray(rays, F)
    out = np.full((len(rays), 12), -7.0, F)
    calls = np.zeros(len(rays), np.int32)
    emul.ray_cast(rays.ctypes.data, len(rays), S, F(1.0) / F(S), R, fn, user.ctypes.data if user is not None else None, out.ctypes.data, calls.ctypes.data)
    return out, calls


def _rays(seed, n=4096):
    """origins a few metres above or below the surface, slopes from vertical to 2 degrees off horizontal, up-going and down-going"""
    rng = np.random.RandomState(seed)
    r = np.empty((n, 8), F)
    r[:, 0:2] = rng.uniform(-40, 40, (n, 2))
    r[:, 2] = rng.uniform(-3, 3.5, n)
    az = rng.uniform(0, 2 * np.pi, n)
    el = np.radians(rng.uniform(2, 90, n)) * rng.choice([-1, 1], n)
    length = rng.uniform(0.3, 3.0, n)                          # the direction need not be normalised
    r[:, 4], r[:, 5], r[:, 6] = length * np.cos(el) * np.cos(az), length * np.cos(el) * np.sin(az), length * np.sin(el)
    r[:, 3] = rng.uniform(-1, 1, n)
    r[:, 7] = r[:, 3] + rng.uniform(0.5, 12, n) / length
    return r


@pytest.mark.parametrize("surface,user", [("ray_height_plane", PLANE), ("ray_height_waves", WAVES)])
@pytest.mark.parametrize("S", [1, 7, 32, 1024])
def test_emulation_is_the_definition(emul, surface, user, S):
    fn = _fn(emul, surface)
    rays = _rays(S)
    assert len(rays) >= 4000
    for R in (0, 1, 12, 24):
        got, calls = _cast(emul, fn, user, rays, S, R)
        want = ray64.cast32(_height(emul, fn, user), rays, S, R)
        assert not want.bad.any() and np.isfinite(got).all()
        assert np.array_equal(_bits(got), _bits(want.records)), (surface, S, R, np.argwhere(_bits(got) != _bits(want.records))[:4])
        status = got[:, 3]
        for v in (ray64.MISS, ray64.ENTER, ray64.LEAVE):
            assert (status == v).sum() > 40, (surface, S, R, v)
        miss = status == ray64.MISS
        assert (got[miss, 2] < 0).any() and (got[miss, 2] > 0).any()
        # a bracketed ray: the march up to its i, R refinements and the record; a miss: S + 1 samples and the record
        assert np.array_equal(calls, np.where(miss, S + 2, want.index + 1 + R + 1))
        assert calls.max() <= S + R + 2
        # field 2 is g at hi and fields 4 ... 11 the record there
        assert np.array_equal(got[:, 4:6], (rays[:, 0:2] + got[:, 0:1] * rays[:, 4:6]).astype(F))
        assert np.array_equal(got[:, 2], (rays[:, 2] + got[:, 0] * rays[:, 6]) - got[:, 6])
        assert np.all(got[~miss, 1] < got[~miss, 0]) or R >= 12                 # (a deep refinement may close the bracket to one value)
        assert np.all(got[:, 1] <= got[:, 0])


def test_samples_and_the_last_one(emul):
    rays = _rays(3, 500)
    for S in (1, 7, 32, 1024):
        t = np.zeros((len(rays), S + 1), F)
        emul.ray_samples(rays.ctypes.data, len(rays), S, F(1.0) / F(S), t.ctypes.data)
        assert np.array_equal(_bits(t), _bits(ray64.samples32(rays, S)))
        assert np.array_equal(_bits(t[:, S]), _bits(rays[:, 7]))                     # t_S is tmax exactly ...
    # ... also where tmin + S * delta is not: the ray that ends under the surface by less than that rounding must still be seen to end there
    S = 7
    ray = np.array([[0, 0, 1, 0, 0, 0, -1, 0.6]], F)
    reached = F(0) + F(S) * ((F(0.6) - F(0)) * (F(1.0) / F(S)))
    assert reached != F(0.6)
    lo_t, hi_t = sorted([float(reached), float(F(0.6))])
    level = np.array([0, 0, 1.0 - 0.5 * (lo_t + hi_t)], F)                          # the surface between point(reached).z and point(tmax).z
    got, _ = _cast(emul, _fn(emul, "ray_height_plane"), level, ray, S, 0)
    want = ray64.cast32(_height(emul, _fn(emul, "ray_height_plane"), level), ray, S, 0)
    assert np.array_equal(_bits(got), _bits(want.records))
    below_at_tmax = (F(1) + F(0.6) * F(-1)) - level[2] < 0
    assert (got[0, 3] == ray64.ENTER) == bool(below_at_tmax)
    if got[0, 3] == ray64.ENTER:
        assert got[0, 0] == F(0.6) and want.index[0] == S


def test_empty_range_and_misses(emul):
    fn = _fn(emul, "ray_height_plane")
    rays = _rays(5, 64)
    rays[:, 7] = rays[:, 3]                                   # tmin == tmax
    for S, R in ((1, 0), (7, 12), (1024, 24)):
        got, calls = _cast(emul, fn, PLANE, rays, S, R)
        assert np.all(got[:, 3] == ray64.MISS)
        assert np.array_equal(_bits(got[:, 0]), _bits(rays[:, 7])) and np.array_equal(_bits(got[:, 1]), _bits(rays[:, 7]))
        assert np.array_equal(_bits(got), _bits(ray64.cast32(_height(emul, fn, PLANE), rays, S, R).records))
        assert np.all(calls == S + 2)                         # a miss is not refined
    # a ray that stays above, one that stays below: the sign of field 2
    rays = np.array([[0, 0, 5, 0, 1, 0, 0.01, 10], [0, 0, -5, 0, 1, 0, -0.01, 10]], F)
    got, _ = _cast(emul, fn, PLANE, rays, 32, 8)
    assert np.all(got[:, 3] == ray64.MISS) and got[0, 2] > 0 and got[1, 2] < 0 and np.all(got[:, 0] == 10) and np.all(got[:, 1] == 10)


def test_bad_rays(emul):
    fn = _fn(emul, "ray_height_plane")
    base = _rays(7, 40)
    rays = base.copy()
    victims = []
    for k in range(8):                                         # every field, a NaN and an infinity
        rays[2 * k, k] = np.nan
        rays[2 * k + 1, k] = np.inf if k % 2 else -np.inf
        victims += [2 * k, 2 * k + 1]
    rays[20, 3], rays[20, 7] = 2.0, 1.0                        # tmax < tmin
    rays[21, 7], rays[21, 4] = 3.0e38, 10.0                    # point(tmax) overflows: finite fields, a non-finite end point
    rays[22, 3], rays[22, 6] = -3.0e38, -10.0                  # point(tmin) overflows
    rays[23, 0], rays[23, 4], rays[23, 7] = 3.0e38, 3.0e38, 1.5
    victims += [20, 21, 22, 23]
    assert np.isfinite(rays[21]).all() and np.isfinite(rays[22]).all() and np.isfinite(rays[23]).all()
    flags = np.zeros(len(rays), np.uint8)
    emul.ray_bad_flags(rays.ctypes.data, len(rays), flags.ctypes.data)
    assert flags.nonzero()[0].tolist() == sorted(victims) == ray64.bad32(rays).nonzero()[0].tolist()

    # a bad ray evaluates nothing (the callback would raise) and gets twelve NaNs; the others are as without it
    seen = []

    def record(x, y, user, rec):
        seen.append((x, y))
        rec[2] = 0.0

    cb = HEIGHT_FN(record)
    got, calls = _cast(emul, ctypes.cast(cb, P), None, rays[victims], 7, 3)
    assert np.isnan(got).all() and not seen and np.all(calls == 0)
    got, _ = _cast(emul, fn, PLANE, rays, 32, 8)
    clean, _ = _cast(emul, fn, PLANE, base, 32, 8)
    keep = np.setdiff1d(np.arange(len(rays)), victims)
    assert np.isnan(got[victims]).all()
    assert np.array_equal(_bits(got[keep]), _bits(clean[keep]))
    assert np.array_equal(_bits(got), _bits(ray64.cast32(_height(emul, fn, PLANE), rays, 32, 8).records))


def test_a_parameter_range_that_overflows_is_not_a_fault(emul):
    # finite fields and end points, but tmax - tmin overflows: every t_i but t_S is a NaN, its q is not finite, the query's record there
    # is NaNs and a NaN is "not below".  The cast is still the definition's
    fn = _fn(emul, "ray_height_plane")
    rays = np.array([[0, 0, 1, -3.0e38, 0, 0, -1e-38, 3.0e38], [0, 0, -1, -3.0e38, 0, 0, -1e-38, 3.0e38]], F)
    assert not ray64.bad32(rays).any()
    level = np.array([0, 0, 0], F)
    for S, R in ((1, 0), (7, 3)):
        got, _ = _cast(emul, fn, level, rays, S, R)
        want = ray64.cast32(_height(emul, fn, level), rays, S, R)
        assert np.array_equal(_bits(got), _bits(want.records)), (S, R)
