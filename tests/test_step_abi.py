"""CPU tests of body stepping's interface (include/datum_ocean_hip.h: datum_ocean_step_bodies): the header declares the entry points and
states the definition, the library exports them, the binding has its methods, signatures and the props' layout, the argument checks that
need no device answer, and the kernel reaches its sums through the velocity query's functions and the shared walk alone."""

import ctypes
import os
import re

import numpy as np

import step64
from test_body_abi import assert_query_is_stated_once, read_csrc
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

STEP_SYMBOLS = ("datum_ocean_step_bodies", "datum_ocean_step_bodies_host")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_step():
    from datum_amd import capi, host_api

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    note = _header().split("#define DATUM_OCEAN_ABI_VERSION")[0]
    for name in STEP_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
        assert name in note, name
    # added without a version bump
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    assert callable(host_api.OceanContext.step_ocean_bodies)
    assert hasattr(host_api.load(), "datum_host_step_ocean_bodies")
    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    for name in ("step_ocean_bodies", "sizeof(OceanStepRecord) == 32"):
        assert name in shim, name


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- body stepping (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("inv = 1.0f / (float)substeps", "h = dt · inv", "F = (D.Fx, D.Fy, buoyancy·M + D.Fz)", "τ = (buoyancy·bx + D.τx, buoyancy·by + D.τy, D.τz)",
                 "v'.z = v.z + h·(F.z·invmass − gravity)", "T' = T + h·v'", "τb_j = (R[j]·τ.x + R[3+j]·τ.y) + R[6+j]·τ.z", "αb_j = τb_j · invinertia[j]",
                 "ω' = ω + h·α", "THE GYROSCOPIC TERM ω × Iω IS LEFT OUT", "x = c_0' / |c_0'|", "y0 = c_1' − (x·c_1')·x", "z = x × y",
                 "THE SWELL IS NOT INCLUDED", "eight quiet NaNs", "left exactly as", "#define DATUM_OCEAN_STEP_RECORD_FLOATS 8",
                 "#define DATUM_OCEAN_STEP_MAX_SUBSTEPS 16", "DATUM_OCEAN_ESTATE exactly where datum_ocean_reduce_body_drag returns it",
                 "nbodies == 0 enqueues"):
        assert line in section, line
    velocity = text.split("/* -- surface velocity (added at ABI 9")[1].split("/* -- body drag")[0]
    assert "datum_ocean_step_bodies" in velocity and "two consumers" in velocity


def test_props_layout_defines_and_signatures():
    from datum_amd import capi

    emul = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    emul.step_props_sizeof.restype = emul.step_props_offsetof.restype = ctypes.c_size_t
    assert emul.step_props_sizeof() == ctypes.sizeof(capi.BodyProps) == capi.BODY_PROPS_DTYPE.itemsize == step64.PROPS.itemsize == 32
    want = {"invmass": 0, "invinertia": 4, "gravity": 16, "buoyancy": 20, "pad": 24}
    for i, (name, off) in enumerate(want.items()):
        assert emul.step_props_offsetof(i) == off, name
        assert getattr(capi.BodyProps, name).offset == off, name
        assert capi.BODY_PROPS_DTYPE.fields[name][1] == off and step64.PROPS.fields[name][1] == off, name
    assert emul.step_record_floats() == capi.STEP_RECORD_FLOATS == step64.RECORD_FLOATS == 8
    assert emul.step_max_substeps() == capi.STEP_MAX_SUBSTEPS == step64.MAX_SUBSTEPS == 16
    assert emul.step_fields() == 10

    I, P, S, Z, F = capi.I, capi.P, ctypes.POINTER(capi.OceanSet), ctypes.c_size_t, capi.F
    L = ctypes.POINTER(I)
    for name in STEP_SYMBOLS:
        assert capi.SYMBOLS[name] == (I, [P, L, I, S, I, P, P, P, Z, P, Z, F, I, P]), name
    for name in ("step_bodies", "step_bodies_host"):
        assert callable(getattr(capi.Ocean, name)), name


def test_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    bodies = np.zeros(2, capi.BODY_DTYPE)
    motions = np.zeros(2, capi.BODY_MOTION_DTYPE)
    props = np.zeros(2, capi.BODY_PROPS_DTYPE)
    probes = np.zeros((4, 4), np.float32)
    out = np.zeros((2, 8), np.float32)
    arr = (capi.I * 2)(0, 0)
    P = capi.P
    ptr = lambda a: a.ctypes.data_as(P)
    for name in STEP_SYMBOLS:
        fn = getattr(lib, name)
        # no handle: EINVAL whatever else is said, the substeps and dt among it
        for dt, sub in ((1 / 60, 1), (1 / 60, 0), (1 / 60, 17), (float("nan"), 1), (float("inf"), 2)):
            assert fn(None, arr, 2, ctypes.byref(s), 4, ptr(bodies), ptr(motions), ptr(props), 2, ptr(probes), 4, dt, sub, ptr(out)) == capi.EINVAL
            assert name.encode() in lib.datum_ocean_last_error(None)
        assert fn(None, None, 0, None, 4, None, None, None, 0, None, 0, 0.0, 1, None) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
    assert np.all(bodies.view(np.uint8) == 0) and np.all(motions.view(np.uint8) == 0)


def test_the_step_kernel_states_no_fetch_and_no_arithmetic_of_its_own():
    # the record comes from the velocity query's two functions, once each; the probe load is the shared walk's, in ocean_body.hip
    assert_query_is_stated_once()
    step, body = read_csrc("ocean_step.hip"), read_csrc("ocean_body.hip")
    assert step.count("query_solve<LAYOUT>(") == 1 and step.count("query_velocity<LAYOUT>(") == 1 and step.count("query_record<LAYOUT>(") == 0
    for word in ("SurfaceTexel", "buf_load", "rmap", ".map", "__shared__", "__syncthreads"):
        assert word not in step, word
    assert not re.search(r"\batomic\w*\s*\(", step)
    # one walk, three kernels; stores only through resources over the body's own slots
    assert body.count("bool body_walk(") == 1 and step.count("body_walk(") == 1 and "body_tree(" in step and "readfirstlane" in step
    assert set(re.findall(r"buf_store\w*(?:<\d+>)?\([^;]*?, (r\w+), \d+, 0\);", step)) == {"rrecord", "rbody", "rmotion"}
    # the arithmetic is ocean_step.h's, built on body_terms and drag_terms, which the CPU walks
    header = read_csrc("ocean_step.h")
    for fn in ("step_terms(", "step_integrate(", "step_state_finite(", "step_props_bad("):
        assert fn in step, fn
        assert len(re.findall(r"OB_HD \w+ " + re.escape(fn), header)) == 1, fn
    assert "body_terms(" in header and "drag_terms(" in header and "fmaf" not in header
    emul = open(os.path.join(ROOT, "tests", "cpu", "step_emul.cpp"), encoding="utf-8").read()
    assert "ocean_step.h" in emul and "step_terms(" in emul and "step_integrate(" in emul and "body_tree(" in emul
