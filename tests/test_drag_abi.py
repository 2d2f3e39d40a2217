"""CPU tests of body drag's interface (include/datum_ocean_hip.h: datum_ocean_reduce_body_drag): the header declares the entry points and
states the definition, the library exports them, the binding has its methods, signatures and the motion's layout, the argument checks that
need no device answer, and the kernel reaches its record through the velocity query's functions and the body walk alone."""

import ctypes
import os
import re

import numpy as np

import drag64
from test_body_abi import assert_query_is_stated_once, read_csrc
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

DRAG_SYMBOLS = ("datum_ocean_reduce_body_drag", "datum_ocean_read_body_drag")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_drag():
    from datum_amd import capi, host_api

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    note = _header().split("#define DATUM_OCEAN_ABI_VERSION")[0]
    for name in DRAG_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
        assert name in note, name
    # added without a version bump
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    assert callable(host_api.OceanContext.reduce_ocean_body_drag)
    assert hasattr(host_api.load(), "datum_host_reduce_ocean_body_drag")
    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    for name in ("reduce_ocean_body_drag", "sizeof(OceanDragRecord) == 32"):
        assert name in shim, name


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- body drag (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("u.x = v.x + (ω.y·r.z − ω.z·r.y)", "u.y = v.y + (ω.z·r.x − ω.x·r.z)", "u.z = v.z + (ω.x·r.y − ω.y·r.x)",
                 "s   = sqrt((e.x·e.x + e.y·e.y) + e.z·e.z)", "k   = m · (cl + cq · s)", "τz = r.x·f.y − r.y·f.x",
                 "Fx, Fy, Fz, τx, τy, τz, Σ m, max residual", "field 6 is datum_ocean_reduce_bodies' field 0", "count == 0 gives eight zeros",
                 "eight quiet NaNs", "THE SWELL IS NOT INCLUDED", "#define DATUM_OCEAN_DRAG_RECORD_FLOATS 8",
                 "DATUM_OCEAN_ESTATE exactly where datum_ocean_sample_velocity_blend returns it"):
        assert line in section, line
    # the section comes after the surface velocity's, and that one points here
    velocity = text.split("/* -- surface velocity (added at ABI 9")[1].split("/* -- body drag")[0]
    assert "datum_ocean_reduce_body_drag" in velocity


def test_motion_layout_and_signatures():
    from datum_amd import capi

    emul = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    emul.drag_motion_sizeof.restype = emul.drag_motion_offsetof.restype = ctypes.c_size_t
    assert emul.drag_motion_sizeof() == ctypes.sizeof(capi.BodyMotion) == capi.BODY_MOTION_DTYPE.itemsize == drag64.MOTION.itemsize == 32
    want = {"linear": 0, "angular": 12, "cl": 24, "cq": 28}
    for i, (name, off) in enumerate(want.items()):
        assert emul.drag_motion_offsetof(i) == off, name
        assert getattr(capi.BodyMotion, name).offset == off, name
        assert capi.BODY_MOTION_DTYPE.fields[name][1] == off and drag64.MOTION.fields[name][1] == off, name
    assert capi.DRAG_RECORD_FLOATS == capi.BODY_RECORD_FLOATS == 8

    I, P, S, Z = capi.I, capi.P, ctypes.POINTER(capi.OceanSet), ctypes.c_size_t
    L = ctypes.POINTER(I)
    for name in DRAG_SYMBOLS:
        assert capi.SYMBOLS[name] == (I, [P, L, I, S, I, P, P, Z, P, Z, P]), name
    for name in ("reduce_body_drag", "read_body_drag"):
        assert callable(getattr(capi.Ocean, name)), name


def test_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    bodies = np.zeros(2, capi.BODY_DTYPE)
    motions = np.zeros(2, capi.BODY_MOTION_DTYPE)
    probes = np.zeros((4, 4), np.float32)
    out = np.zeros((2, 8), np.float32)
    arr = (capi.I * 2)(0, 0)
    P = capi.P
    for name in DRAG_SYMBOLS:
        fn = getattr(lib, name)
        assert fn(None, arr, 2, ctypes.byref(s), 4, bodies.ctypes.data_as(P), motions.ctypes.data_as(P), 2, probes.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
        assert fn(None, None, 0, None, 4, None, None, 0, None, 0, None) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)


def test_the_drag_kernel_states_no_fetch_of_its_own():
    # the record comes from the velocity query's two functions, once each; the probe load is the shared walk's, in ocean_body.hip
    assert_query_is_stated_once()
    drag, body = read_csrc("ocean_drag.hip"), read_csrc("ocean_body.hip")
    assert drag.count("query_solve<LAYOUT>(") == 1 and drag.count("query_velocity<LAYOUT>(") == 1 and drag.count("query_record<LAYOUT>(") == 0
    for word in ("SurfaceTexel", "buf_load", "buf_store", "rmap", ".map", "make_rsrc", "__shared__", "__syncthreads"):
        assert word not in drag, word
    assert not re.search(r"\batomic\w*\s*\(", drag)
    # one walk, two kernels
    assert body.count("void body_each_probe(") == 1 and body.count("body_each_probe(") == 2 and drag.count("body_each_probe(") == 1
    assert re.findall(r"buf_load\w*(?:<\d+>)?\((\w+)", body) == ["rprobes"]
    # the arithmetic is ocean_drag.h's, which the CPU walks
    header = read_csrc("ocean_drag.h")
    assert "drag_terms(" in drag and "drag_motion_bad(" in drag
    assert len(re.findall(r"OB_HD \w+ drag_terms\(", header)) == 1 and len(re.findall(r"OB_HD \w+ drag_motion_bad\(", header)) == 1
    assert "fmaf" not in header
    emul = open(os.path.join(ROOT, "tests", "cpu", "drag_emul.cpp"), encoding="utf-8").read()
    assert "ocean_drag.h" in emul and "drag_terms(" in emul and "body_tree(" in emul
