"""CPU tests of coupled stepping's interface (include/datum_ocean_hip.h: datum_ocean_step_bodies_coupled): the header declares the entry
points and states the definition, the library exports them, the bindings have their methods and signatures, the argument check that needs
no device answers, the kernel reaches its arithmetic through ocean_couple.h alone, and the files it builds on stayed as they were."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import couple64
from test_body_abi import read_csrc
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

COUPLE_SYMBOLS = ("datum_ocean_step_bodies_coupled", "datum_ocean_step_bodies_coupled_host")
UNCHANGED = ("ocean_step.hip", "ocean_ripple.hip", "ocean_step.h", "ocean_ripple.h", "ocean_drag.h")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_coupled_stepping():
    from datum_amd import capi, host_api

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    note = _header().split("#define DATUM_OCEAN_ABI_VERSION")[0]
    for name in COUPLE_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
        assert name in note, name
    # added without a version bump
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    for name in ("step_bodies_coupled", "step_bodies_coupled_host"):
        assert callable(getattr(capi.Ocean, name)), name
    assert callable(host_api.OceanContext.step_ocean_bodies_coupled)
    assert hasattr(host_api.load(), "datum_host_step_ocean_bodies_coupled")
    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    for name in ("void step_ocean_bodies_coupled(OceanContext &context", "struct OceanCoupledRecord", "sizeof(OceanCoupledRecord) == 48"):
        assert name in shim, name


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- coupled stepping (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("inv = 1.0f / (float)substeps", "h = dt · inv", "rec'[2] = rec[2] + s.η", "rec'[6] = rec[6] + s.η_t", "one fp32 addition each",
                 "pending deposits are not", "cells outside the window read 0", "fourteen fields", "at the START of the sub-step",
                 "in the step's FIRST form", "datum_ocean_step_ripples(h, 1)", "Every sub-step is a launch of its own",
                 "DATUM_OCEAN_COUPLED_RECORD_FLOATS = 12 floats (48 bytes)", "the dropped quanta summed over all sub-steps",
                 "LAST GOOD SUB-STEP", "has deposited its other probes", "has deposited ALL its probes", "The layer is looked at first", "that drag AND probes", "twelve quiet NaNs", "a NaN in field 0", "STABILITY OF A BODY'S OWN WAKE",
                 "THE FFT SURFACE IS FROZEN", "THE SWELL IS NOT INCLUDED", "DATUM_OCEAN_ESTATE exactly where datum_ocean_reduce_body_drag returns it",
                 "while the layer is off", "dt < 0 or not finite", "c·h/s > 0.7", "A refused call enqueues nothing", "nbodies == 0 still steps the water",
                 "LEFT OUT", "#define DATUM_OCEAN_COUPLED_RECORD_FLOATS 12"):
        assert line in section, line
    ripples = text.split("/* -- ripple layer (added at ABI 9; nothing in the reference)")[1].split("/* -- coupled stepping")[0]
    assert "the one call that" in ripples and "datum_ocean_step_bodies_coupled" in ripples


def test_defines_and_signatures():
    from datum_amd import capi

    emul = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    assert emul.couple_record_floats() == capi.COUPLED_RECORD_FLOATS == couple64.RECORD_FLOATS == 12
    assert emul.couple_fields() == 14
    I, P, S, Z, F = capi.I, capi.P, ctypes.POINTER(capi.OceanSet), ctypes.c_size_t, capi.F
    L = ctypes.POINTER(I)
    for name in COUPLE_SYMBOLS:
        assert capi.SYMBOLS[name] == (I, [P, L, I, S, I, P, P, P, Z, P, Z, F, I, P]), name
        assert capi.SYMBOLS[name] == capi.SYMBOLS["datum_ocean_step_bodies"], name


def test_argument_errors_without_gpu():
    """no handle: EINVAL with the call's name in the text, whatever else is said"""
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    bodies = np.zeros(2, capi.BODY_DTYPE)
    motions = np.zeros(2, capi.BODY_MOTION_DTYPE)
    props = np.zeros(2, capi.BODY_PROPS_DTYPE)
    probes = np.zeros((4, 4), np.float32)
    out = np.zeros((2, 12), np.float32)
    arr = (capi.I * 2)(0, 0)
    ptr = lambda a: a.ctypes.data_as(capi.P)
    for name in COUPLE_SYMBOLS:
        fn = getattr(lib, name)
        for dt, sub in ((1 / 60, 1), (1 / 60, 0), (1 / 60, 17), (float("nan"), 1), (-0.1, 2)):
            assert fn(None, arr, 2, ctypes.byref(s), 4, ptr(bodies), ptr(motions), ptr(props), 2, ptr(probes), 4, dt, sub, ptr(out)) == capi.EINVAL
            assert name.encode() in lib.datum_ocean_last_error(None)
        assert fn(None, None, 0, None, 4, None, None, None, 0, None, 0, 0.0, 1, None) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
    assert np.all(bodies.view(np.uint8) == 0) and np.all(motions.view(np.uint8) == 0) and np.all(out == 0)


def test_the_kernel_calls_the_headers():
    """the arithmetic stands once: ocean_couple.h calls ocean_step.h and ocean_ripple.h, the kernel calls ocean_couple.h, the CPU walks the
    same header; the deposits are one plain atomic in C++; the host code has a section of its own and shares the ripple step's parameters"""
    kernel, header, host = read_csrc("ocean_couple.hip"), read_csrc("ocean_couple.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_couple.h"' in kernel and '#include "ocean_step.hip"' in kernel and '#include "ocean_ripple.hip"' in kernel
    assert "fmaf(" not in header and "fmaf(" not in kernel and "asm" not in kernel and kernel.count("atomicAdd(") == 1
    for word in ("__shared__", "__syncthreads", "SurfaceTexel", ".map"):
        assert word not in kernel, word
    for fn in ("couple_record(", "couple_terms(", "couple_fold(", "couple_zero(", "couple_was_bad("):
        assert fn in kernel, fn
        assert len(re.findall(r"OB_HD \w+ " + re.escape(fn), header)) == 1, fn
    for fn in ("step_terms(", "wake_terms(", "step_zero(", "body_add(p.s, t.s)"):
        assert fn in header, fn
    for fn in ("ripple_sample(", "ripple_splat(", "step_integrate(", "step_state_finite(", "body_walk(", "body_tree(", "readfirstlane"):
        assert fn in kernel, fn
    # no copy of the parents' arithmetic
    for copy in ("sqrtf(", "rintf(", "floorf(", "fminf(", "4.0f *", "1048576.0f"):
        assert copy not in header and copy not in kernel, copy
    assert kernel.count("query_solve<LAYOUT>(") == 1 and kernel.count("query_velocity<LAYOUT>(") == 1 and kernel.count("body_walk(") == 1
    assert set(re.findall(r"buf_store\w*(?:<\d+>)?\([^;]*?, (r\w+), \d+, 0\);", kernel)) == {"rrecord", "rbody", "rmotion"}
    assert set(re.findall(r"buf_load\w*\((r\w+),", kernel)) == {"rstate"}
    emul = open(os.path.join(ROOT, "tests", "cpu", "couple_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_couple.h", "couple_record(", "couple_terms(", "couple_fold(", "step_integrate(", "body_tree("):
        assert fn in emul, fn
    section = host.split("/* -- coupled stepping (ocean_couple.hip)")[1].split("// a cascade's maps as the reference's")[0]
    assert section.count("ripple_step_args(ctx, h)") == 1 and section.count("hipMemsetAsync(") == 1 and section.count("launch_ripple_step(r, true, ctx->stream)") == 1
    for word in ("hipMemset(", "hipMemcpy(", "hipDeviceSynchronize", "1.0 / (1.0 +"):
        assert word not in section, word
    ripple = host.split("/* -- the ripple layer (ocean_ripple.hip)")[1].split("/* -- ray casts")[0]
    assert ripple.count("1.0 / (1.0 +") == 1 and ripple.count("ripple_step_args(ctx, h)") == 1


def _less_window(text):
    """ocean_ripple.h less ripple_window and its record, the host-only function beside ripple_wrap that no kernel calls
    (tests/test_ripple_emul.py walks it): a file that does not hold it yet is returned whole"""
    start, end = text.find(b"  // The window at origin (ox, oy) as it lies in memory"), text.find(b"  // ox <= I < ox + R and the same for J")
    return text if start < 0 else text[:start] + text[end:]


def test_parent_files_are_byte_identical():
    """the coupled kernel includes the step's and the ripple layer's files and edits none of them (every byte of ocean_ripple.h but
    ripple_window's block, which the kernels do not read)"""
    assert _less_window(b"a\n  // The window at origin (ox, oy) as it lies in memory b\n  // ox <= I < ox + R and the same for J c") == b"a\n  // ox <= I < ox + R and the same for J c"
    for name in UNCHANGED:
        path = "datum_amd/csrc/" + name
        try:
            shown = subprocess.run(["git", "-C", ROOT, "show", "HEAD~:" + path], capture_output=True)
        except OSError:
            pytest.skip("no git to ask for the parent commit")
        if shown.returncode != 0:
            pytest.skip("no parent commit that holds " + name)
        assert _less_window(shown.stdout) == _less_window(open(os.path.join(ROOT, path), "rb").read()), name
