"""CPU tests of body buoyancy's interface (include/datum_ocean_hip.h: datum_ocean_reduce_bodies): the header declares the entry points and
states the definition, the library exports them, the binding has its methods, signatures and the body's layout, the argument checks that
need no device answer, and the per-point text of the several-cascade query is included once by each of its two kernels."""

import ctypes
import os
import re

import numpy as np

import body64
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

BODY_SYMBOLS = ("datum_ocean_reduce_bodies", "datum_ocean_read_bodies")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_bodies():
    from datum_amd import capi, host_api

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    for name in BODY_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    # added without a version bump
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    assert callable(host_api.OceanContext.reduce_ocean_bodies)
    assert hasattr(host_api.load(), "datum_host_reduce_ocean_bodies")


def test_header_states_definition():
    text = _header()
    for line in ("w.x = ((R[0]·x + R[1]·y) + R[2]·z) + T.x", "d   = min(max(rec.z − w.z, 0), cap)", "m   = a · d", "τy = −(r.x · m)",
                 "wet = (d > 0 ? a : 0)", "s = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + s] for l < s", "first + l, first + l + 64",
                 "count == 0 gives eight zeros", "eight quiet NaNs", "#define DATUM_OCEAN_BODY_RECORD_FLOATS 8"):
        assert line in text, line


def test_body_layout_and_signatures():
    from datum_amd import capi

    emul = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    emul.body_sizeof.restype = emul.body_offsetof.restype = ctypes.c_size_t
    assert emul.body_sizeof() == ctypes.sizeof(capi.Body) == capi.BODY_DTYPE.itemsize == body64.BODY.itemsize == 64
    want = {"rotation": 0, "position": 36, "first": 48, "count": 52, "cap": 56, "pad": 60}
    for i, (name, off) in enumerate(want.items()):
        assert emul.body_offsetof(i) == off, name
        assert getattr(capi.Body, name).offset == off, name
        assert capi.BODY_DTYPE.fields[name][1] == off and body64.BODY.fields[name][1] == off, name
    assert capi.BODY_RECORD_FLOATS == 8 and capi.BODY_PROBE_FLOATS == 4

    I, P, S, Z = capi.I, capi.P, ctypes.POINTER(capi.OceanSet), ctypes.c_size_t
    L = ctypes.POINTER(I)
    for name in BODY_SYMBOLS:
        assert capi.SYMBOLS[name] == (I, [P, L, I, S, I, P, Z, P, Z, P]), name
    for name in ("reduce_bodies", "read_bodies"):
        assert callable(getattr(capi.Ocean, name)), name


def test_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    bodies = np.zeros(2, capi.BODY_DTYPE)
    probes = np.zeros((4, 4), np.float32)
    out = np.zeros((2, 8), np.float32)
    arr = (capi.I * 2)(0, 0)
    P = capi.P
    for name in BODY_SYMBOLS:
        fn = getattr(lib, name)
        assert fn(None, arr, 2, ctypes.byref(s), 4, bodies.ctypes.data_as(P), 2, probes.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
        assert fn(None, None, 0, None, 4, None, 0, None, 0, None) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)


def test_the_point_evaluation_is_stated_once():
    # the fixed-point solve and the final evaluation of the several-cascade query: one text, included by the query and by the body kernel
    csrc = os.path.join(ROOT, "datum_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name), encoding="utf-8").read()
    blend, body, point = read("ocean_blend.hip"), read("ocean_body.hip"), read("ocean_surface_blend_point.inc")
    inc = '#include "ocean_surface_blend_point.inc"'
    assert blend.count(inc) == 1 and body.count(inc) == 1
    assert len(point) > 0
