"""CPU tests of the foam plane's interface (ABI 9): the header declares the entry points and states the definition, the library
exports them, the binding matches, and the argument checks that need no device answer.  Plus the float64 helper's own identities."""

import ctypes
import math
import os
import re

import numpy as np

import foam64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

FOAM_SYMBOLS = (
    "datum_ocean_set_foam",
    "datum_ocean_set_foam_params",
    "datum_ocean_reset_foam",
    "datum_ocean_bind_foam",
    "datum_ocean_foam_device",
    "datum_ocean_read_foam",
    "datum_ocean_upload_height",
)


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_foam():
    from datum_amd import capi

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    for name in FOAM_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name


def test_abi_version_9():
    from datum_amd import capi

    assert capi.ABI_VERSION == capi.header_abi_version() == capi.load().datum_ocean_abi_version() == 9


def test_header_states_definition_and_modes():
    from datum_amd import capi

    text = _header()
    assert "J = (1 − a)(1 − d) − b·c" in text
    assert "a = ∂x dx,  b = ∂y dx,  c = ∂x dy,  d = ∂y dy" in text
    modes = {k: int(v) for k, v in re.findall(r"#define\s+DATUM_OCEAN_FOAM_(\w+)\s+(\d+)", text)}
    assert modes == {"OFF": capi.FOAM_OFF, "JACOBIAN": capi.FOAM_JACOBIAN, "ACCUMULATE": capi.FOAM_ACCUMULATE} == {"OFF": 0, "JACOBIAN": 1, "ACCUMULATE": 2}


def test_foam_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    p, n = capi.P(), ctypes.c_size_t()
    out = np.zeros(16, np.float32)
    assert lib.datum_ocean_set_foam(None, capi.FOAM_JACOBIAN) == capi.EINVAL
    assert b"datum_ocean_set_foam" in lib.datum_ocean_last_error(None)
    assert lib.datum_ocean_set_foam_params(None, 0, 0.5, 2.0, 1.0) == capi.EINVAL
    assert lib.datum_ocean_reset_foam(None, 0) == capi.EINVAL
    assert lib.datum_ocean_bind_foam(None, None, 0) == capi.EINVAL
    assert lib.datum_ocean_foam_device(None, ctypes.byref(p), ctypes.byref(n)) == capi.EINVAL
    assert lib.datum_ocean_read_foam(None, 0, out.ctypes.data_as(capi.P)) == capi.EINVAL
    assert b"datum_ocean_read_foam" in lib.datum_ocean_last_error(None)
    assert lib.datum_ocean_upload_height(None, 0, out.ctypes.data_as(capi.P)) == capi.EINVAL


def test_ocean_binding_has_foam_methods():
    from datum_amd import capi, host_api

    for name in ("set_foam", "set_foam_params", "reset_foam", "bind_foam", "foam_device", "read_foam", "upload_height"):
        assert callable(getattr(capi.Ocean, name)), name
    for name in ("set_foam", "set_foam_params", "read_foam"):
        assert callable(getattr(host_api.OceanContext, name)), name
    lib = host_api.load()
    for name in ("datum_host_set_ocean_foam", "datum_host_set_ocean_foam_params", "datum_host_read_ocean_foam"):
        assert hasattr(lib, name), name


def test_jacobian64_identities():
    # periodic central differences commute and are anti-self-adjoint: sum(a + d) = 0 and sum(a d - b c) = 0, so mean(J) = 1
    N, ws = 64, 37.0
    rs = np.random.RandomState(7)
    maps = rs.standard_normal((6, N, N))
    J = foam64.jacobian64(maps, ws, N)
    assert abs(J.mean() - 1.0) < 1e-12 * foam64.scale64(maps, ws, N).mean()
    # with two derivatives swapped the identity fails: what the device's mean(J) = 1 test catches
    a, b, c, d = foam64.parts64(maps, ws, N)
    assert abs(((1 - b) * (1 - d) - a * c).mean() - 1.0) > 1e-3
    # flat: exactly one
    assert np.array_equal(foam64.jacobian64(np.zeros((6, N, N)), ws, N), np.ones((N, N)))
    # a plane wave along x: 1 - J is a sinusoid of amplitude A sin(2 pi p / N) N / wavescale, constant along y
    p, A = 3, 0.7
    x = np.arange(N)
    dx = np.tile(A * np.cos(2 * math.pi * p * x / N + 0.3), (N, 1))
    J = foam64.jacobian64(np.stack([dx, np.zeros((N, N))]), ws, N)
    assert np.allclose(J, J[:1])
    assert abs(np.abs(1 - J).max() - A * math.sin(2 * math.pi * p / N) * N / ws) < 1e-2 * A * N / ws
