"""CPU tests of wake foam's interface (include/datum_ocean_hip.h: "wake foam"): the header declares the entry points and states the
definition, the library exports them, the binding has its methods and signatures, the ABI stays 9, a null handle is EINVAL on every call,
the kernels reach the arithmetic through ocean_ripple_foam.h and restate nothing, and the C++ shim declares its calls.  (The refusals that
need a handle are in tests/test_gpu_ripple_foam.py: a handle needs a device.)"""

import ctypes
import os
import re

import numpy as np

from test_body_abi import read_csrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

SYMBOLS = ("datum_ocean_set_ripple_foam", "datum_ocean_set_ripple_foam_params", "datum_ocean_step_ripple_foam", "datum_ocean_reset_ripple_foam",
           "datum_ocean_ripple_foam_device", "datum_ocean_read_ripple_foam", "datum_ocean_sample_ripple_foam", "datum_ocean_query_ripple_foam")

SHIM = ("set_ocean_ripple_foam", "step_ocean_ripple_foam", "query_ocean_ripple_foam", "read_ocean_ripple_foam")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports():
    from datum_amd import capi

    text = _header()
    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", text))
    history = text[text.index("Later added at 9 without a bump"):text.index("#define DATUM_OCEAN_ABI_VERSION")]
    lib = capi.load()
    for name in SYMBOLS:
        assert name in declared and name in history, name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
        assert callable(getattr(capi.Ocean, name[len("datum_ocean_"):])), name
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    I, P, Z, F = capi.I, capi.P, ctypes.c_size_t, capi.F
    L = ctypes.POINTER(I)
    want = {"datum_ocean_set_ripple_foam": [P, I], "datum_ocean_set_ripple_foam_params": [P, F, F, F, F, F], "datum_ocean_step_ripple_foam": [P, F],
            "datum_ocean_reset_ripple_foam": [P], "datum_ocean_ripple_foam_device": [P, ctypes.POINTER(P), ctypes.POINTER(Z), L, L],
            "datum_ocean_read_ripple_foam": [P, P], "datum_ocean_sample_ripple_foam": [P, P, Z, P], "datum_ocean_query_ripple_foam": [P, P, Z, P]}
    assert set(want) == set(SYMBOLS)
    for name, args in want.items():
        assert capi.SYMBOLS[name] == (I, args), name
    # the sampler's and the device call's argument lists are the layer's, word for word
    args = lambda n: re.sub(r"\s+", " ", re.search(r"\bint " + n + r"\(([^;]*)\);", text).group(1))
    for mine, parent in (("datum_ocean_sample_ripple_foam", "datum_ocean_sample_ripples"), ("datum_ocean_query_ripple_foam", "datum_ocean_query_ripples"),
                         ("datum_ocean_ripple_foam_device", "datum_ocean_ripples_device")):
        assert args(mine) == args(parent), mine


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- wake foam (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("hx  = (eR − eL) · hinv", "hinv = 0.5f · invs", "hy  = (eU − eD) · hinv", "q   = hx·hx + hy·hy", "g1  = (q − t1) · k1",
                 "g2  = (fabsf(η_t) − t2) · k2", "g   = fminf(fmaxf(fmaxf(g1, g2), 0.0f), 1.0f)", "new = fmaxf(g, old · fade)",
                 "fade = (float)exp(−(double)decay · (double)dt), on the host", "FOAM_ACCUMULATE's rule with two sources", "CURRENT state buffer",
                 "pending deposits are not seen", "a neighbour outside\n * the window is 0", "of two zeros of opposite sign fmaxf gives +0",
                 "Off by default", "nothing is allocated or launched", "the state buffers, src, the FFT foam plane, the maps and\n * every record keep their bits",
                 "DESIGN CHOICES, NOT MEASUREMENTS", "t1 = 0.04 (a slope of 0.2), k1 = 10, t2 = 0.5 m/s, k2 = 2,\n *                            decay = 0.5 1/s",
                 "A gain of 0\n *                            switches its source off", "Works while the foam is off", "DATUM_OCEAN_ESTATE while the layer is off",
                 "datum_ocean_set_ripples with any R, 0 included", "Waits for\n *                            the stream", "enqueues one launch on the handle's stream and returns",
                 "dt < 0 or not finite is DATUM_OCEAN_EINVAL", "dt = 0 is\n *                            legal and gives fade = 1", "It writes the plane only",
                 "The pointer does not alternate", "[j][i] for cell (ox + i, oy + j); blocking", "one float, 4-byte aligned",
                 "f0 = f00 + wx·(f10 − f00)     f1 = f01 + wx·(f11 − f01)     f = f0 + wy·(f1 − f0)", "Cells outside the window read 0",
                 "A non-finite point gives NaN and fetches nothing", "2^30 cells gives 0", "datum_ocean_center_ripples also zeroes the plane's cells that entered",
                 "a jump of R\n * cells or more clears the plane", "datum_ocean_reset_ripples also clears the plane", "The layer is looked at first",
                 "with the call's name in the error text", "A refused call enqueues nothing", "LEFT OUT", "fusing the update into the last ripple sub-step",
                 "advection of the foam by the water's velocity", "a direct source from src", "field 7 of the rippled query's record",
                 "a bounds/`active` record for the plane", "INTEGRATION.md 5a"):
        assert line in section, line
    # "foam from the layer" is no longer left out of the rippled reads: a pointer to this block stands there
    rippled = text.split("/* -- rippled reads (added at ABI 9; nothing in the reference)")[1].split("/* -- ripple-layer bounds")[0]
    left = rippled.split("LEFT OUT:")[1]
    assert "foam from the layer is no longer left out" in left and '"wake foam"' in left


def test_argument_errors_without_gpu():
    """no handle: EINVAL with the call's name in the text, whatever else is said"""
    from datum_amd import capi

    lib = capi.load()
    P = capi.P
    buf = np.zeros((4, 8), np.float32)
    ptr = buf.ctypes.data_as(P)
    dev, nbytes, ox, oy = P(), ctypes.c_size_t(), capi.I(), capi.I()
    calls = {
        "datum_ocean_set_ripple_foam": [(1,), (0,)],
        "datum_ocean_set_ripple_foam_params": [(0.04, 10.0, 0.5, 2.0, 0.5), (0.04, -1.0, 0.5, 2.0, 0.5), (float("nan"), 10.0, 0.5, 2.0, 0.5)],
        "datum_ocean_step_ripple_foam": [(0.1,), (-0.1,), (float("nan"),)],
        "datum_ocean_reset_ripple_foam": [()],
        "datum_ocean_ripple_foam_device": [(ctypes.byref(dev), ctypes.byref(nbytes), ctypes.byref(ox), ctypes.byref(oy))],
        "datum_ocean_read_ripple_foam": [(ptr,)],
        "datum_ocean_sample_ripple_foam": [(ptr, 2, ptr), (None, 0, None)],
        "datum_ocean_query_ripple_foam": [(ptr, 2, ptr), (None, 0, None)],
    }
    assert set(calls) == set(SYMBOLS)
    for name, cases in calls.items():
        for args in cases:
            assert getattr(lib, name)(None, *args) == capi.EINVAL, (name, args)
            assert name.encode() in lib.datum_ocean_last_error(None), name
    assert dev.value is None and np.all(buf == 0)


def test_the_kernels_call_the_header():
    """the arithmetic stands once, in ocean_ripple_foam.h, which the CPU walks: the kernel file holds no copy of it and no assembly, every
    launch and memset of the host section names the handle's stream, and the ripple layer's files keep their text"""
    kernels, header, host = read_csrc("ocean_ripple_foam.hip"), read_csrc("ocean_ripple_foam.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_ripple_foam.h"' in kernels and '#include "ocean_ripple.hip"' in kernels and '#include "ocean_ripple.h"' in header
    assert '#include "ocean_ripple_foam.hip"' in host
    code = kernels.split("#pragma once")[1]
    assert "fmaf" not in header and "fmaf(" not in kernels and "asm" not in code and "atomic" not in code
    for fn in ("ripple_foam_max(", "ripple_foam_update(", "ripple_foam_sample("):
        assert len(re.findall(r"OB_HD float " + re.escape(fn), header)) == 1, fn
    for fn in ("ripple_foam_update(", "ripple_foam_sample(", "ripple_wrap(", "ripple_world("):
        assert fn in code, fn
    # nothing restated: the extrema, the products, the axis and the window test are called
    for copy in ("fminf(", "fmaxf(", "fabsf(", "hinv *", "* a.p", "floorf(", "ripple_axis(", "ripple_inside(", "exp("):
        assert copy not in code, copy
    # the step's form and constants, not a second set
    for text in ("__shared__ float tile[RIPPLE_TY + 2][RIPPLE_LX]", "__launch_bounds__(RIPPLE_THREADS)", "buf_store_f32_aux<RIPPLE_STORE_AUX>(f, rfoam",
                 "make_rsrc(a.foam, cells * sizeof(float))", "make_rsrc(a.state, cells * sizeof(float2))"):
        assert text in code, text
    assert "constexpr" not in code
    emul = open(os.path.join(ROOT, "tests", "cpu", "ripple_foam_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_ripple_foam.h", "ripple_foam_update(", "ripple_foam_sample(", "ripple_foam_max("):
        assert fn in emul, fn
    make = open(os.path.join(ROOT, "Makefile"), encoding="utf-8").read()
    assert "tests/cpu/ripple_foam_emul.cpp" in make and "datum_amd/csrc/ocean_ripple_foam.hip datum_amd/csrc/ocean_ripple_foam.h" in make
    # the host section: ahead of the ripple bounds', on the handle's stream, the layer's check shared
    section = host.split("/* -- wake foam: a coverage plane beside the ripple layer (ocean_ripple_foam.hip)")[1].split("/* -- bounds of the ripple layer")[0]
    assert section.count("check_ripples(ctx, ") == 2 and section.count("check_ripple_foam(ctx, ") == 5 and section.count("check_ripple_foam_points(ctx, ") == 2
    # (the section fills nothing itself: the guards' fill is GuardedPlane's, the plane's the one memset of clear_ripple_foam, which stands
    # with the other two hooks ahead of the ripple layer's section)
    hooks = host.split("/* -- the ripple layer's planes")[1].split("/* -- the ripple layer (ocean_ripple.hip)")[0]
    assert section.count("hipMemsetAsync(") == 0 and hooks.count("hipMemsetAsync(") == 1 and section.count("ctx->ripplefoam.allocate(ripple_cells(ctx), ctx->stream)") == 1
    assert "hipMemsetAsync(ctx->ripplefoam.get(), 0, ripple_cells(ctx) * sizeof(float), ctx->stream)" in hooks.split("int clear_ripple_foam(")[1].split("\n  }\n")[0]
    assert section.count("read_staged(ctx, ") == 1 and section.count("(float)std::exp(-(double)ctx->ripplefoamdecay * (double)dt)") == 1
    for word in ("hipMemset(", "hipMemcpy(", "hipDeviceSynchronize", "rippleboundscurrent"):
        assert word not in section, word
    launches = re.findall(r"launch_ripple_foam\w*\([^;]*\)\);", section + hooks)
    assert len(launches) == 3
    for launch in launches:
        assert launch.endswith(", ctx->stream));"), launch
    # the three hooks are called from the ripple layer's section
    ripple = host.split("/* -- the ripple layer (ocean_ripple.hip)")[1].split("/* -- ray casts")[0]
    for hook in ("free_ripple_foam(ctx)", "clear_ripple_foam(ctx)", "scroll_ripple_foam(ctx, a.g, a.oldx, a.oldy)"):
        assert hook in ripple, hook


def test_shim_declarations_present():
    from datum_amd import host_api

    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    code = open(os.path.join(ROOT, "datum_amd", "host", "ocean.cpp"), encoding="utf-8").read()
    for name in ("void set_ocean_ripple_foam(OceanContext &context, bool on)", "void step_ocean_ripple_foam(OceanContext &context, float dt)",
                 "void query_ocean_ripple_foam(OceanContext &context, lml::Vec2 const *positions, std::size_t count, float *coverage)",
                 "void read_ocean_ripple_foam(OceanContext &context, float *plane)"):
        assert name in shim, name
    lib = host_api.load()
    for name in SHIM:
        assert hasattr(lib, "datum_host_" + name) and callable(getattr(host_api.OceanContext, name)), name
        # each throws before prepare_ocean_context
        assert f'throw runtime_error("{name}: the context is not prepared (prepare_ocean_context)")' in code, name
