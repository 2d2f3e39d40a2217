"""CPU tests of body buoyancy's interface (include/datum_ocean_hip.h: datum_ocean_reduce_bodies): the header declares the entry points and
states the definition, the library exports them, the binding has its methods, signatures and the body's layout, the argument checks that
need no device answer, and the per-point functions of the several-cascade query are defined once and are what its kernels call."""

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


CSRC = os.path.join(ROOT, "datum_amd", "csrc")
QUERY_FUNCTIONS = ("query_solve", "query_height", "query_record", "query_velocity")


def read_csrc(name):
    return open(os.path.join(CSRC, name), encoding="utf-8").read()


def assert_query_is_stated_once():
    """the fixed-point solve and each final evaluation of the several-cascade query: functions of ocean_query.hip, defined once in the whole
    module, over one corner fetch (the only place beside the single-cascade kernel that makes a SurfaceTexel); the text they replace is gone"""
    assert not os.path.exists(os.path.join(CSRC, "ocean_surface_blend_point.inc"))
    assert "ocean_surface_" not in open(os.path.join(ROOT, "Makefile"), encoding="utf-8").read().replace("ocean_surface.hip", "")
    sources = {name: read_csrc(name) for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h", ".inc"))}
    for fn in QUERY_FUNCTIONS:
        defined = {name: len(re.findall(r"__device__ __forceinline__ \w+ %s\(" % fn, text)) for name, text in sources.items()}
        assert defined.pop("ocean_query.hip") == 1 and not any(defined.values()), (fn, defined)
    assert sum(text.count("struct QueryCorners") for text in sources.values()) == 1
    assert sum(text.count("void query_each_point(") for text in sources.values()) == 1
    users = sorted(name for name, text in sources.items() if re.search(r"SurfaceTexel<LAYOUT>\s+(const\s+)?&?\w", text))
    assert users == ["ocean_query.hip", "ocean_surface.hip"], users
    assert sources["ocean_query.hip"].count("buf_load_f32x4_aux<0>(rmap") == 4           # the four corners' part A, once


def test_the_point_evaluation_is_stated_once():
    # the query kernel and the body kernel reach their records through the functions alone: neither makes a texel or loads from a map
    assert_query_is_stated_once()
    blend, body = read_csrc("ocean_blend.hip"), read_csrc("ocean_body.hip")
    kernel = blend.split("ocean_surface_blend_kernel(SurfaceBlendArgs b)")[1].split("inline hipError_t launch_gen_blend(")[0]
    for text in (kernel, body):
        assert text.count("query_record<LAYOUT>(") == 1 and text.count("query_solve<LAYOUT>(") == 1
        assert "SurfaceTexel" not in text and "rmap" not in text and ".map" not in text
    assert "buf_load" not in kernel and "query_each_point(" in kernel
    assert re.findall(r"buf_load\w*(?:<\d+>)?\((\w+)", body) == ["rprobes"]
