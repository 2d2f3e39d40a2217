"""CPU tests of the ripple layer's interface (include/datum_ocean_hip.h: "ripple layer"): the header declares the entry points and states
the definition, the library exports them, the binding has its methods and signatures, the argument checks that need no device answer,
and the kernels reach their arithmetic through ocean_ripple.h alone.  (The refusals that need a handle, and ESTATE while the layer is
off, are in tests/test_gpu_ripples.py: a handle needs a device.)"""

import ctypes
import os
import re

import numpy as np

import ripple64
from test_body_abi import read_csrc
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

RIPPLE_SYMBOLS = ("datum_ocean_set_ripples", "datum_ocean_set_ripple_params", "datum_ocean_center_ripples", "datum_ocean_reset_ripples",
                  "datum_ocean_ripples_device", "datum_ocean_read_ripples", "datum_ocean_step_ripples", "datum_ocean_deposit_ripples",
                  "datum_ocean_deposit_body_ripples", "datum_ocean_sample_ripples", "datum_ocean_query_ripples", "datum_ocean_deposit_ripples_host",
                  "datum_ocean_deposit_body_ripples_host")

SHIM = ("set_ocean_ripples", "center_ocean_ripples", "deposit_ocean_ripples", "deposit_ocean_body_ripples", "step_ocean_ripples", "query_ocean_ripples")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_ripples():
    from datum_amd import capi

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    note = _header().split("#define DATUM_OCEAN_ABI_VERSION")[0]
    for name in RIPPLE_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
        assert name in note, name
    # added without a version bump
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    for name in ("set_ripples", "set_ripple_params", "center_ripples", "reset_ripples", "ripples_device", "read_ripples", "step_ripples", "deposit_ripples",
                 "deposit_body_ripples", "sample_ripples", "query_ripples", "deposit_ripples_host", "deposit_body_ripples_host"):
        assert callable(getattr(capi.Ocean, name)), name
    # the C++ shim and its binding
    from datum_amd import host_api

    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    for name in SHIM:
        assert callable(getattr(host_api.OceanContext, name)), name
        assert hasattr(host_api.load(), "datum_host_" + name), name
        assert "void " + name + "(OceanContext &context" in shim, name
    for name in ("sizeof(OceanWakeRecord) == 32", "sizeof(OceanRippleImpulse) == 16 && sizeof(OceanRippleSample) == 16"):
        assert name in shim, name


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- ripple layer (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("(J mod R)·R + (I mod R)", "a torus in memory", "zeroes the cells that entered", "no cell is copied", "h = dt · inv",
                 "e = η + (float)src · 2^-20", "lap = ((eL + eR) + (eD + eU)) − 4·e", "v1  = (η_t + h · (c2s2 · lap)) · f[k]", "e1  = e + h · v1",
                 "a neighbour outside the window is 0", "f[k] = 1 / (1 + h (γ + γe (k/B)²))", "refuses c·h/s > 0.7", "1/√2",
                 "Q   = rint((V · (invs·invs)) · 2^20) clamped to ±2^30", "q11 = Q − ((q00 + q10) + q01)", "cell centres stand at (I + ½)·s",
                 "is dropped", "deposits nothing", "heave   if 0 < d and d < cap", "Vh = (a · (−e.z)) · dt", "surge   if d > 0", "sx = −(e.x·dt)",
                 "KINEMATIC SOURCE, NOT A RADIATION SOLUTION", "only through its probes", "THE SWELL IS NOT INCLUDED", "eight quiet NaNs",
                 "THE POINTER ALTERNATES", "[j][i][2]", "∂xη = (a0 + wy·(a1 − a0))·invs", "DATUM_OCEAN_ESTATE while the layer is off",
                 "(−R/2, −R/2)", "dt < 0 or not finite is DATUM_OCEAN_EINVAL", "deposit_ripples_host, deposit_body_ripples_host", "#define DATUM_OCEAN_RIPPLE_RECORD_FLOATS 8", "#define DATUM_OCEAN_RIPPLE_MAX_SUBSTEPS 16",
                 "#define DATUM_OCEAN_RIPPLE_MAX_SPONGE 64"):
        assert line in section, line


def test_defines_and_signatures():
    from datum_amd import capi

    assert capi.RIPPLE_SIZES == (64, 128, 256, 512, 1024)
    assert capi.RIPPLE_RECORD_FLOATS == 8 and capi.RIPPLE_MAX_SUBSTEPS == 16 and capi.RIPPLE_MAX_SPONGE == ripple64.MAX_SPONGE == 64
    I, P, S, Z, F = capi.I, capi.P, ctypes.POINTER(capi.OceanSet), ctypes.c_size_t, capi.F
    L = ctypes.POINTER(I)
    want = {"datum_ocean_set_ripples": [P, I, F], "datum_ocean_set_ripple_params": [P, F, F, I, F], "datum_ocean_center_ripples": [P, F, F],
            "datum_ocean_reset_ripples": [P], "datum_ocean_ripples_device": [P, ctypes.POINTER(P), ctypes.POINTER(Z), L, L],
            "datum_ocean_read_ripples": [P, P], "datum_ocean_step_ripples": [P, F, I], "datum_ocean_deposit_ripples": [P, P, Z],
            "datum_ocean_deposit_body_ripples": [P, L, I, S, I, P, P, Z, P, Z, F, P], "datum_ocean_sample_ripples": [P, P, Z, P],
            "datum_ocean_query_ripples": [P, P, Z, P], "datum_ocean_deposit_ripples_host": [P, P, Z],
            "datum_ocean_deposit_body_ripples_host": [P, L, I, S, I, P, P, Z, P, Z, F, P]}
    assert set(want) == set(RIPPLE_SYMBOLS)
    for name, args in want.items():
        assert capi.SYMBOLS[name] == (I, args), name


def test_argument_errors_without_gpu():
    """no handle: EINVAL with the call's name in the text, whatever else is said"""
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    P = capi.P
    ptr = lambda a: a.ctypes.data_as(P)
    buf = np.zeros((4, 8), np.float32)
    arr = (capi.I * 1)(0)
    dev, nbytes, ox, oy = P(), ctypes.c_size_t(), capi.I(), capi.I()
    calls = {
        "datum_ocean_set_ripples": [(64, 0.5), (0, 0.0), (65, 0.5), (64, -1.0), (64, float("nan"))],
        "datum_ocean_set_ripple_params": [(2.0, 0.05, 8, 4.0), (0.0, 0.05, 8, 4.0), (2.0, -1.0, 8, 4.0), (2.0, 0.05, 65, 4.0), (2.0, 0.05, 8, float("inf"))],
        "datum_ocean_center_ripples": [(0.0, 0.0), (float("nan"), 0.0)],
        "datum_ocean_reset_ripples": [()],
        "datum_ocean_ripples_device": [(ctypes.byref(dev), ctypes.byref(nbytes), ctypes.byref(ox), ctypes.byref(oy))],
        "datum_ocean_read_ripples": [(ptr(buf),)],
        "datum_ocean_step_ripples": [(0.1, 1), (0.1, 0), (float("nan"), 17), (-0.1, 1)],
        "datum_ocean_deposit_ripples_host": [(ptr(buf), 2), (None, 0)],
        "datum_ocean_deposit_body_ripples_host": [(arr, 1, ctypes.byref(s), 4, ptr(buf), ptr(buf), 1, ptr(buf), 2, 0.05, ptr(buf))],
        "datum_ocean_deposit_ripples": [(ptr(buf), 2), (None, 0)],
        "datum_ocean_deposit_body_ripples": [(arr, 1, ctypes.byref(s), 4, ptr(buf), ptr(buf), 1, ptr(buf), 2, 0.05, ptr(buf)), (None, 0, None, 4, None, None, 0, None, 0, 0.0, None)],
        "datum_ocean_sample_ripples": [(ptr(buf), 2, ptr(buf))],
        "datum_ocean_query_ripples": [(ptr(buf), 2, ptr(buf)), (None, 0, None)],
    }
    assert set(calls) == set(RIPPLE_SYMBOLS)
    for name, cases in calls.items():
        for args in cases:
            assert getattr(lib, name)(None, *args) == capi.EINVAL, (name, args)
            assert name.encode() in lib.datum_ocean_last_error(None), name
    assert dev.value is None and np.all(buf == 0)


def test_the_kernels_call_the_header():
    """the arithmetic stands once, in ocean_ripple.h, which the CPU walks: the kernels hold no copy of it, the deposits are plain vector
    atomics in C++, every launch and memset goes on the handle's stream, and the walk and the drag header stay as they were"""
    kernels, header, host = read_csrc("ocean_ripple.hip"), read_csrc("ocean_ripple.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_ripple.h"' in kernels and "fmaf(" not in header and "fmaf(" not in kernels
    for fn in ("ripple_index(", "ripple_inside(", "ripple_sponge(", "ripple_height(", "ripple_update(", "ripple_splat(", "ripple_sample(", "wake_terms("):
        assert len(re.findall(r"OB_HD \w+ " + re.escape(fn), header)) == 1, fn
    for fn in ("ripple_sponge(", "ripple_height(", "ripple_update(", "ripple_splat(", "ripple_sample(", "wake_terms(", "ripple_wrap("):
        assert fn in kernels, fn
    for copy in ("4.0f *", "rintf(", "floorf(", "9.5367431640625e-07f", "1048576.0f"):
        assert copy not in kernels, copy
    assert kernels.count("atomicAdd(") == 1 and "asm" not in kernels
    assert kernels.count("query_solve<LAYOUT>(") == 1 and kernels.count("query_velocity<LAYOUT>(") == 1 and kernels.count("body_each_probe(") == 1
    emul = open(os.path.join(ROOT, "tests", "cpu", "ripple_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_ripple.h", "ripple_update(", "ripple_splat(", "ripple_sample(", "wake_terms(", "body_tree("):
        assert fn in emul, fn
    section = host.split("/* -- the ripple layer (ocean_ripple.hip)")[1].split("/* -- ray casts")[0]
    # (the read-back's copies are read_ripple_window's, ahead of the section; the two state buffers' fills name the stream here)
    assert section.count("hipMemsetAsync(") == 4 and section.count(", ctx->stream)") == 12
    assert section.count("read_ripple_window(ctx, ") == 1 and section.count(".allocate(cells, ctx->stream)") == 2
    # (the wake's host twin copies its arrays in and out through the body calls' shared staging, which names the handle's stream as well)
    staging = host.split("/* -- body buoyancy (ocean_body.hip)")[1].split("/* -- body drag")[0]
    assert section.count("stage_batch(") == 1 and section.count("fetch_batch(") == 1 and len(re.findall(r"hipMemcpyAsync\([^;]*, ctx->stream\)\);", staging)) == staging.count("hipMemcpyAsync(") == 4
    for word in ("hipMemset(", "hipMemcpy(", "hipDeviceSynchronize", ", 0)", "nullptr)"):
        assert word not in section.replace("fail(nullptr", ""), word


def test_guarded_planes_and_the_window_read_stand_once():
    """ocean_capi.hip: a plane between its 0xCD guards is GuardedPlane, stated once beside the bounds block's own guards; the window-order
    read is read_ripple_window, the file's one user of the 2D copy; the helpers the layer's section calls stand ahead of it, so nothing is
    declared ahead of its definition; and a refusal under a shared check's name is fail(ctx, code, name, text)"""
    host, header = read_csrc("ocean_capi.hip"), read_csrc("ocean_ripple.h")
    assert host.count("hipMemcpy2DAsync(") == 1 and host.count("int read_ripple_window(") == 1 and host.count("read_ripple_window(ctx, ") == 5
    assert len(re.findall(r"hipMemsetAsync\([^;]*0xCD[^;]*\)", host)) == 2
    assert re.findall(r"constexpr \w+ (\w*GUARD\w*) =", host) == ["RIPPLE_GUARD_BYTES", "RIPPLE_BOUNDS_GUARD"] and "RIPPLE_GUARD_BYTES = 256;" in host
    assert host.count("struct GuardedPlane") == 1 and len(re.findall(r"GuardedPlane<[\w ]+> ripple(state\[2\]|foam|wall|bed|surf);", host)) == 5
    assert len(re.findall(r"\.allocate\(\w+\(?\w*\)?, ctx->stream\)", host)) == 6 and host.count(".release()") == 12
    for gone in ("(what + ", "std::string(name) +", "ripplestateblock", "ripplefoamblock", "ripplewallblock", "ripplebedblock", "ripplesurfblock"):
        assert gone not in host, gone
    assert host.count("int fail(datum_ocean_ctx *ctx, int code, char const *name, char const *text)") == 1
    # the shared helpers: ahead of the layer's section, each defined once and declared nowhere else, everything on the handle's stream
    planes = host.split("/* -- the ripple layer's planes")[1].split("/* -- the ripple layer (ocean_ripple.hip)")[0]
    for fn in ("int free_ripple_foam(", "int clear_ripple_foam(", "int scroll_ripple_foam(", "int free_ripple_walls(", "int raster_ripple_walls(",
               "int free_ripple_bed(", "int raster_ripple_bed(", "void fill_ripple_surf(", "void fill_ripple_raster(", "size_t ripple_cells("):
        assert planes.count(fn) == 1 and host.count(fn) == 1, fn
    assert "alloc_ripple_state(" not in host and "free_ripple_state(" not in host
    assert planes.count("fill_ripple_raster(ctx, g, zero, a);") == 2 and host.count("ctx->rippleboundscurrent && !zero") == 1
    assert planes.count("hipMemsetAsync(") == 1 and planes.count(", ctx->stream)") == 5
    for word in ("hipMemset(", "hipMemcpy(", "hipDeviceSynchronize", ", 0)", "nullptr)"):
        assert word not in planes, word
    # the rectangles are ocean_ripple.h's, which the CPU walks (tests/test_ripple_emul.py); no kernel file names them
    assert header.count("inline int ripple_window(") == 1 and host.count("ripple_window(ctx->rippleox, ctx->rippleoy, ctx->rippleR, rect)") == 1
    for kernels in ("ocean_ripple.hip", "ocean_ripple_deep.hip", "ocean_ripple_foam.hip", "ocean_ripple_wall.hip", "ocean_ripple_bed.hip", "ocean_ripple_bounds.hip", "ocean_rippled.hip"):
        assert "ripple_window(" not in read_csrc(kernels), kernels
    assert "ripple_window(" in open(os.path.join(ROOT, "tests", "cpu", "ripple_emul.cpp"), encoding="utf-8").read()
