"""CPU tests of the surface queries' interface (include/datum_ocean_hip.h: datum_ocean_sample_surface): the header declares both entry points
and states the definition, the libraries export them, both bindings have their methods, and the argument checks that need no device answer.
Plus the float64 helper's own identities (tests/surface64.py)."""

import ctypes
import math
import os
import re

import numpy as np

import surface64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

SURFACE_SYMBOLS = ("datum_ocean_sample_surface", "datum_ocean_read_surface")


def _header():
    return open(HEADER, encoding="utf-8").read()


def _set(A=0.0, steep=0.0, length=40.0, phase=0.0, direction=(0.780869, 0.624695), wavescale=22.0, plane_w=0.0):
    from datum_amd import capi

    s = capi.OceanSet()
    s.swellamplitude, s.swellsteepness, s.swelllength, s.swellphase = A, steep, length, phase
    s.swelldirection[:] = direction
    s.scale = 1.0 / wavescale
    s.plane[:] = (0.0, 0.0, 1.0, plane_w)
    return s


def test_header_declares_and_library_exports_surface():
    from datum_amd import capi

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    for name in SURFACE_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name


def test_header_states_definition():
    from datum_amd import capi

    text = _header()
    for line in ("θ     = frequency · (swelldirection · b) + swellphase",
                 "P(b)  = b + qi · A · swelldirection · cos θ",
                 "V(b)  = ( P.x − D.x,  P.y − D.y,  −plane.w + A · sin θ + D.z )",
                 "b ← b + (q − V(b).xy)",
                 "residual = |V(b).xy − q|"):
        assert line in text, line
    consts = {k: int(v) for k, v in re.findall(r"#define\s+DATUM_OCEAN_SURFACE_(\w+)\s+(\d+)", text)}
    assert consts == {"SAMPLE_FLOATS": capi.SURFACE_SAMPLE_FLOATS, "MAX_ITERATIONS": capi.SURFACE_MAX_ITERATIONS} == {"SAMPLE_FLOATS": 8, "MAX_ITERATIONS": 16}
    # added without a version bump: the binding, the header and the library still say 9
    assert capi.ABI_VERSION == capi.header_abi_version() == capi.load().datum_ocean_abi_version() == 9


def test_bindings_have_surface_methods():
    from datum_amd import capi, host_api

    for name in ("sample_surface", "read_surface"):
        assert callable(getattr(capi.Ocean, name)), name
    assert callable(host_api.OceanContext.query_ocean_surface)
    assert hasattr(host_api.load(), "datum_host_query_ocean_surface")


def test_surface_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    pts = np.zeros((4, 2), np.float32)
    out = np.zeros((4, 8), np.float32)
    P = capi.P
    for name in SURFACE_SYMBOLS:
        fn = getattr(lib, name)
        assert fn(None, 0, ctypes.byref(s), 4, pts.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
        assert fn(None, 0, None, 4, pts.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert fn(None, 0, ctypes.byref(s), 4, None, 0, None) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)


def test_missing_symbol_is_a_rebuild_error(monkeypatch, tmp_path):
    # a library without an entry point the binding declares is refused like a version mismatch (OSError naming the rebuild)
    from datum_amd import capi

    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setitem(capi.SYMBOLS, "datum_ocean_no_such_entry_point", (capi.I, []))
    try:
        capi.load()
    except OSError as e:
        assert "datum_ocean_no_such_entry_point" in str(e) and "rebuild the HIP module" in str(e)
    else:
        raise AssertionError("load() accepted a library without a declared symbol")


def test_surface64_flat_without_swell_is_exact():
    N = 64
    maps = np.zeros((2, N, N, 4))
    maps[1, ..., 2] = 1.0                                # a flat ocean's normal layer
    s = _set(A=0.0, plane_w=-1.5)
    q = np.array([[0.0, 0.0], [-1e6, 1e6], [12.34, -5.6], [1e5, -3.0]])
    for it in (0, 1, 4, 16):
        r = surface64.surface64(maps, None, s, q, it)
        want = np.column_stack([q, np.full(len(q), 1.5), np.zeros(len(q)), np.zeros((len(q), 2)), np.ones(len(q)), np.zeros(len(q))])
        assert np.array_equal(r, want), (it, r)


def test_surface64_swell_height_against_scalar_root_finder():
    # swell only (flat map): the Gerstner surface above q; the base point solves b + g cos(k (d . b) + phi) d = q along d, a scalar problem
    N = 64
    maps = np.zeros((2, N, N, 4))
    maps[1, ..., 2] = 1.0
    L, A, steep, phase = 40.0, 0.8, 0.6, 0.3
    d = np.array([0.6, 0.8])
    s = _set(A=A, steep=steep, length=L, phase=phase, direction=tuple(d))
    f = surface64.frame64(s)
    k, g = f["frequency"], f["qi"] * A
    rs = np.random.RandomState(3)
    q = rs.uniform(-200, 200, (40, 2))
    r = surface64.surface64(maps, None, s, q, 16)
    for qi_, rec in zip(q, r):
        u = float(d @ qi_)                               # along d: u_b + g cos(k u_b + phase) = u_q (monotone while k g < 1)
        assert k * g < 1
        lo, hi = u - g - 1, u + g + 1
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid + g * math.cos(k * mid + phase) < u:
                lo = mid
            else:
                hi = mid
        height = A * math.sin(k * lo + phase)
        assert abs(rec[2] - height) < 1e-6, (rec[2], height)
        assert rec[3] < 1e-6


def _smooth_random_maps(N, amp, seed):
    # a few low-frequency waves per channel: smooth, periodic, no fold (|gradient| well below one per metre of the map)
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:N, 0:N] / N
    maps = np.zeros((2, N, N, 4))
    for c in range(3):
        for _ in range(4):
            kx, ky = rs.randint(-3, 4, 2)
            maps[0, ..., c] += amp * rs.uniform(-1, 1) * np.cos(2 * np.pi * (kx * x + ky * y) + rs.uniform(0, 2 * np.pi))
    maps[1, ..., 2] = 1.0
    return maps


def test_surface64_residual_shrinks_with_iterations():
    N, ws = 64, 40.0
    maps = _smooth_random_maps(N, 0.3, 5)
    s = _set(A=0.5, steep=0.3, length=35.0, wavescale=ws)
    q = np.random.RandomState(9).uniform(-100, 100, (500, 2))
    res = [surface64.surface64(maps, None, s, q, it)[:, 3].max() for it in (0, 1, 2, 4, 8, 16)]
    assert all(b < a for a, b in zip(res, res[1:])), res
    assert res[0] > 0.05 and res[-1] < 1e-9, res


def test_surface64_zero_iterations_is_a_direct_sample():
    N, ws = 64, 30.0
    maps = _smooth_random_maps(N, 0.4, 11)
    foam = np.random.RandomState(2).uniform(0, 1, (N, N))
    s = _set(A=0.0, wavescale=ws, plane_w=0.25)
    q = np.random.RandomState(4).uniform(-500, 500, (300, 2))
    r = surface64.surface64(maps, foam, s, q, 0)
    sc = float(s.scale)                                  # 1 / wavescale as the set's float32
    D = surface64.bilinear64(maps[0].transpose(2, 0, 1)[:3], q[:, 0] * sc, q[:, 1] * sc)
    assert np.allclose(r[:, 0], q[:, 0] - D[0], rtol=0, atol=1e-12)
    assert np.allclose(r[:, 1], q[:, 1] - D[1], rtol=0, atol=1e-12)
    assert np.allclose(r[:, 2], -0.25 + D[2], rtol=0, atol=1e-12)
    assert np.allclose(r[:, 3], np.hypot(D[0], D[1]), rtol=0, atol=1e-12)
    assert np.allclose(r[:, 7], surface64.bilinear64(foam, q[:, 0] * sc, q[:, 1] * sc), rtol=0, atol=1e-12)
    # a point on a texel centre reads that texel
    i, j = 5, 9
    c = np.array([[(i + 0.5) / N / sc, (j + 0.5) / N / sc]])
    rc = surface64.surface64(maps, foam, s, c, 0)[0]
    assert abs(rc[2] - (-0.25 + maps[0, j, i, 2])) < 1e-12 and abs(rc[7] - foam[j, i]) < 1e-12


def test_surface64_nonfinite_points_give_nan_records():
    N = 64
    maps = _smooth_random_maps(N, 0.2, 1)
    q = np.array([[np.nan, 0.0], [1.0, 2.0], [np.inf, -np.inf], [0.0, -np.inf]])
    r = surface64.surface64(maps, None, _set(A=0.3, steep=0.2), q, 4)
    assert np.isnan(r[[0, 2, 3]]).all() and np.isfinite(r[1]).all()
