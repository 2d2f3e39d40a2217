"""datum_amd/csrc/ocean_rippled.h walked on the CPU (tests/cpu/rippled_emul.cpp) against tests/rippled64.py's fp32 form, bit for bit: the
lift of a height and the layer's share of a slope at points on cell centres, on the window's seam in memory, half outside the window,
outside, beyond 2^30 cells and not finite; and a cast over an analytic surface plus a layer through ocean_ray.h against ray64.cast32
with the rippled height."""

import ctypes
import os

import numpy as np
import pytest

import ripple64
import rippled64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I, Fl, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    lib.rippled_emul_points.argtypes = [P, I, I, I, Fl, P, L, P, P, P]
    lib.rippled_emul_points.restype = None
    lib.rippled_emul_cast.argtypes = [P, L, I, Fl, I, P, P, I, I, I, Fl, P]
    lib.rippled_emul_cast.restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _layer(R, cell, seed, origin=(37, -21)):
    lay = ripple64.Layer(R, cell)
    lay.move(*origin)
    rng = np.random.RandomState(seed)
    lay.set_window(rng.uniform(-0.3, 0.3, (R, R)).astype(F), rng.uniform(-1, 1, (R, R)).astype(F))
    return lay


def _points(lay, seed):
    R, cell = lay.R, float(lay.s)
    rng = np.random.RandomState(seed)
    lo = np.array([lay.ox, lay.oy]) * cell
    centres = (lo + (rng.randint(0, R, (200, 2)) + 0.5) * cell)
    inside = lo + rng.uniform(0, 1, (400, 2)) * R * cell
    seam = np.array([-(-lay.ox // R) * R, -(-lay.oy // R) * R]) * cell + rng.uniform(-1.5, 1.5, (200, 2)) * cell
    half = np.stack([lo[0] + rng.uniform(-1.5, 1.5, 200) * cell, lo[1] + rng.uniform(0, 1, 200) * R * cell], 1)
    far = lo + (R + rng.uniform(0, 1, (100, 2))) * R * cell
    out = lo - rng.uniform(1.6, 40, (100, 2)) * cell
    beyond = np.array([[2.0 ** 31 * cell, 0.0], [0.0, -(2.0 ** 30) * cell * 1.01], [3e38, 1.0]])
    bad = np.array([[np.nan, 1.0], [1.0, np.inf], [-np.inf, np.nan]])
    return np.concatenate([centres, inside, seam, half, far, out, beyond, bad]).astype(F)


@pytest.mark.parametrize("R,cell", [(64, 1.0), (128, 0.5)])
def test_points_bit_for_bit(lib, R, cell):
    lay = _layer(R, cell, R)
    q = _points(lay, 5)
    rng = np.random.RandomState(6)
    height = rng.uniform(-2, 2, len(q)).astype(F)
    slopes = rng.uniform(-0.7, 0.7, (len(q), 2)).astype(F)
    state = np.ascontiguousarray(lay.state(), F)
    got = np.zeros((len(q), 4), F)
    lib.rippled_emul_points(_ptr(state), R, lay.ox, lay.oy, float(lay.invs), _ptr(q), len(q), _ptr(height), _ptr(slopes), _ptr(got))
    smp = lay.sample(q)
    want = np.stack([rippled64.lift32(height, smp), rippled64.slope32(slopes[:, 0], smp[:, 1]), rippled64.slope32(slopes[:, 1], smp[:, 2]), smp[:, 3]], 1)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan[-3:].all() and not nan[:-3].any()
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    # beyond 2^30 cells: zeros from the layer, the height and the slopes as they came
    assert np.array_equal(_bits(got[-6:-3, 0]), _bits(height[-6:-3] + F(0))) and np.array_equal(got[-6:-3, 1:3], slopes[-6:-3] + F(0))
    # the planted mistakes differ in bits
    assert (got[:-3, 0] != rippled64.lift32(height, smp, "rate")[:-3]).mean() > 0.5
    for m in ("sign", "no_half"):
        assert (got[:-3, 1] != rippled64.slope32(slopes[:, 0], smp[:, 1], m)[:-3]).mean() > 0.5, m


def test_cast_over_plane_and_layer(lib):
    R, cell = 64, 1.0
    lay = _layer(R, cell, 9)
    lo = np.array([lay.ox, lay.oy]) * cell
    rng = np.random.RandomState(10)
    n = 600
    origin = np.concatenate([lo + rng.uniform(-0.3, 1.3, (n, 2)) * R * cell, rng.uniform(-0.5, 4.0, (n, 1))], 1)
    d = rng.normal(size=(n, 3))
    d[:, 2] = -np.abs(d[:, 2]) * rng.choice([1, -0.2], n)
    rays = np.concatenate([origin, np.zeros((n, 1)), d, rng.uniform(1, 40, (n, 1))], 1).astype(F)
    rays[0, 4] = np.nan
    rays[1, 7] = -1.0
    rays[2, 4:7] = 3e38
    plane = np.array([0.01, -0.02, 0.1], F)
    state = np.ascontiguousarray(lay.state(), F)
    fn = rippled64.analytic32(lambda x, y: (plane[0] * x + plane[1] * y) + plane[2], lay)
    for S, Rf in ((1, 0), (7, 12), (32, 12)):
        got = np.zeros((n, 12), F)
        lib.rippled_emul_cast(_ptr(rays), n, S, float(F(1) / F(S)), Rf, _ptr(plane), _ptr(state), R, lay.ox, lay.oy, float(lay.invs), _ptr(got))
        c = rippled64.cast32(fn, rays, S, Rf)
        want = c.records.copy()
        want[:, [4, 5]] = np.where(np.isnan(want[:, [6]]), np.nan, np.stack([rays[:, 0] + want[:, 0] * rays[:, 4], rays[:, 1] + want[:, 0] * rays[:, 5]], 1))
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and nan[:3].all(), (S, Rf)
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), (S, Rf)
    assert (c.records[3:, 3] > 0).mean() > 0.3 and (c.records[3:, 3] == 0).any()
    # the layer decides hits: the same rays over the plane alone give other records
    rest = ripple64.Layer(R, cell)
    rest.move(lay.ox, lay.oy)
    other = rippled64.cast32(rippled64.analytic32(lambda x, y: (plane[0] * x + plane[1] * y) + plane[2], rest), rays, 32, 12).records
    assert (other[3:, 0] != c.records[3:, 0]).mean() > 0.05
