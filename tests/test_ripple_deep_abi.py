"""CPU tests of the DEEP step's interface (include/datum_ocean_hip.h: "dispersive ripples"): the header declares the two entry points and
states the definition, the library exports them, the binding has its methods and signatures, the ABI stays 9, the EINVALs that need no
device answer, the getter returns the table without a GPU, the kernel reaches its arithmetic through ocean_ripple_deep.h and restates
nothing of ocean_ripple.h, the mode is one decision in the host code, and the C++ shim declares its call.  (The refusals that need a handle
are in tests/test_gpu_ripple_deep.py: a handle needs a device.)"""

import ctypes
import os
import re

import numpy as np

import ripple_deep64 as rd
from test_body_abi import read_csrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

SYMBOLS = ("datum_ocean_set_ripple_dispersion", "datum_ocean_ripple_deep_weights")


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
    assert callable(capi.Ocean.set_ripple_dispersion)
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    assert capi.SYMBOLS["datum_ocean_set_ripple_dispersion"] == (capi.I, [capi.P, capi.I, capi.F])
    assert capi.SYMBOLS["datum_ocean_ripple_deep_weights"] == (capi.I, [capi.P])
    assert "int datum_ocean_set_ripple_dispersion(datum_ocean_t ctx, int mode, float g);" in text
    assert "int datum_ocean_ripple_deep_weights(float *quadrant49);" in text
    for define, value in (("DATUM_OCEAN_RIPPLE_WAVE", 0), ("DATUM_OCEAN_RIPPLE_DEEP", 1), ("DATUM_OCEAN_RIPPLE_DEEP_RADIUS", rd.P), ("DATUM_OCEAN_RIPPLE_DEEP_WEIGHTS", rd.Q * rd.Q)):
        assert re.search(r"#define\s+" + define + r"\s+" + str(value) + r"\s", text), define
    assert (capi.RIPPLE_WAVE, capi.RIPPLE_DEEP) == (rd.WAVE, rd.DEEP) == (0, 1)
    # the stepping calls keep their signatures: the mode is the layer's, not an argument
    assert "int datum_ocean_step_ripples(datum_ocean_t ctx, float dt, int substeps);" in text


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- dispersive ripples (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("ω² = g·|k|", "19.47°", "OPT-IN", "13 × 13 convolution", "The default mode is DATUM_OCEAN_RIPPLE_WAVE", "every call keeps its bits",
                 "P = 6", "G[l][k], 0 <= k, l <= 6", "built once on the host in double",
                 "G0[l][k] = (1/M²) Σ_a Σ_b |θ_ab| cos(k θ_a) cos(l θ_b)", "M = 1024, θ_a = 2π(a − M/2)/M, |θ_ab| = √(θ_a² + θ_b²)",
                 "F(di, dj) = G0[|dj|][|di|], subtract ΣF / 169 from every one, and round each to fp32",
                 "the smallest value >= 0", "one nextafterf upward if needed", "Ĝ(θ) = Σ F(di, dj) cos(di·θx) cos(dj·θy)", "Dirichlet kernel",
                 "<= 0.08 for 0.5 <= |θ| <= 1 and <= 0.02 for 1 <= |θ| <= 3", "max Ĝ = 4.30, Σ|F| = 5.37",
                 "BELOW |θ| ≈ 0.45 (WAVELENGTHS ABOVE 14 CELLS) THE SYMBOL IS QUADRATIC AND SUCH WAVES RUN SLOW", "The FFT surface\n * owns those wavelengths",
                 "are exactly datum_ocean_step_ripples'", "acc = 0.0f",
                 "for dj = −6 .. 6 (outer), di = −6 .. 6 (inner):   acc = acc + G[|dj|][|di|] · e(I + di, J + dj)     a cell outside the window is 0.0f",
                 "v1  = (η_t − h · (gs · acc)) · f[k]", "gs = g / s, rounded once on the host from double", "e1  = e + h · v1",
                 "h·Ω < 2, and Ω² <= gs · Σ|F|", "h · √(g · Σ|F| / s) in double", "refuses a value above 1.9 with DATUM_OCEAN_EINVAL",
                 "replaces the c·h/s > 0.7 check in this mode only", "dt < 0 and a dt that is not finite stay",
                 "g finite and > 0, default 9.81", "Works while the layer is off, survives\n *                           datum_ocean_set_ripples, writes no state",
                 "leaves the ripple bounds' CURRENT mark alone", "takes NO HANDLE and needs no GPU", "A null pointer is DATUM_OCEAN_EINVAL",
                 "datum_ocean_step_ripples, datum_ocean_step_bodies_coupled and its host twin take the layer's mode",
                 "then datum_ocean_step_ripples(h, 1)", "its refusal\n * uses the DEEP bound", "behaves as two layers would",
                 "LEFT OUT: temporal blocking; finite-depth dispersion", "radii other than 6; obstacles"):
        assert line in section, line


def test_argument_errors_and_getter_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    for args in [(0, 9.81), (1, 9.81), (2, 9.81), (1, float("nan"))]:
        assert lib.datum_ocean_set_ripple_dispersion(None, *args) == capi.EINVAL
        assert b"datum_ocean_set_ripple_dispersion" in lib.datum_ocean_last_error(None)
    assert lib.datum_ocean_ripple_deep_weights(None) == capi.EINVAL and b"datum_ocean_ripple_deep_weights" in lib.datum_ocean_last_error(None)
    guarded = np.full(rd.Q * rd.Q + 2, np.float32(-7.0))
    assert lib.datum_ocean_ripple_deep_weights(guarded[1:].ctypes.data_as(capi.P)) == capi.OK
    G = guarded[1:-1].reshape(rd.Q, rd.Q)
    assert guarded[0] == -7.0 and guarded[-1] == -7.0 and np.isfinite(G).all()
    # the table: [l][k], symmetric, the numpy construction to one fp32 rounding plus libm, and the same on a second call
    assert np.array_equal(G, G.T) and np.abs(G.astype(np.float64) - rd.weights64()).max() <= 1e-6 * rd.weights64()[0, 0]
    assert G[0, 0] == np.abs(G).max() and G[0, 1] < 0
    again = np.zeros((rd.Q, rd.Q), np.float32)
    assert lib.datum_ocean_ripple_deep_weights(again.ctypes.data_as(capi.P)) == capi.OK and np.array_equal(again.view(np.uint32), G.view(np.uint32))


def test_the_kernel_calls_the_header():
    """the arithmetic stands once, in ocean_ripple_deep.h, which the CPU walks; the window, the sponge, the height and the cell are
    ocean_ripple.h's; the host code chooses the kernel in one place; the wave step's files keep their text"""
    kernel, header, host = read_csrc("ocean_ripple_deep.hip"), read_csrc("ocean_ripple_deep.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_ripple_deep.h"' in kernel and '#include "ocean_ripple.hip"' in kernel and '#include "ocean_ripple.h"' in header
    assert '#include "ocean_ripple_deep.hip"' in host
    code = kernel.split("#pragma once")[1]
    assert "fmaf" not in header and "fmaf(" not in kernel and "asm" not in code and "atomic" not in code
    for fn in ("ripple_deep_row(", "ripple_deep_conv(", "ripple_deep_update("):
        assert len(re.findall(r"OB_HD \w+ " + re.escape(fn), header)) == 1, fn
    for fn in ("ripple_deep_row(", "ripple_deep_update(", "ripple_height(", "ripple_sponge(", "ripple_wrap("):
        assert fn in code, fn
    # no second copy of the layer's helpers, and the update's products stand in the header alone
    for copy in ("OB_HD int ripple_wrap", "OB_HD int ripple_sponge", "OB_HD float ripple_height", "struct RippleCell", "RIPPLE_UNIT"):
        assert copy not in header and copy not in code, copy
    for copy in ("a.gs *", "a.s.h *", "* a.G"):
        assert copy not in code, copy
    for text in ("__shared__ float tile[RIPPLE_DEEP_LY][RIPPLE_DEEP_LX]", "__launch_bounds__(RIPPLE_THREADS)", "buf_store_cf_aux<RIPPLE_STORE_AUX>(cf{ c.eta, c.rate }, rout",
                 "make_rsrc(a.s.in, cells * sizeof(float2))", "make_rsrc(a.s.out, cells * sizeof(float2))", "make_rsrc(a.s.src, cells * sizeof(int))"):
        assert text in code, text
    assert set(re.findall(r"buf_load\w*\((r\w+),", code)) == {"rin", "rsrc"} and set(re.findall(r"buf_store\w*(?:<\w+>)?\([^;]*?, (r\w+), ", code)) == {"rout"}
    emul = open(os.path.join(ROOT, "tests", "cpu", "ripple_deep_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_ripple_deep.h", "ripple_deep_conv(", "ripple_deep_update(", "ripple_deep_weights(", "ripple_height(", "ripple_sponge("):
        assert fn in emul, fn
    make = open(os.path.join(ROOT, "Makefile"), encoding="utf-8").read()
    assert "tests/cpu/ripple_deep_emul.cpp" in make and "datum_amd/csrc/ocean_ripple_deep.hip datum_amd/csrc/ocean_ripple_deep.h" in make
    # the mode is one decision: one place launches either kernel, one builds the arguments, one holds the bound
    assert host.count("launch_ripple_deep_step(") == 1 and host.count("ocean::launch_ripple_step(r.a.s, first, stream)") == 1
    assert host.count("ripple_deep_bound(ctx, h) > 1.9") == 1 and host.count("ripple_courant(ctx, h) > 0.7") == 1
    assert host.count("check_ripple_stability(ctx, ") == 2 and host.count("ripple_deep_weights(G)") == 1
    setter = host.split("int datum_ocean_set_ripple_dispersion(")[1].split("int datum_ocean_ripple_deep_weights(")[0]
    for word in ("hip", "rippleboundscurrent", "ripplestate", "stream"):
        assert word not in setter, word


def test_shim_declaration_present():
    from datum_amd import host_api

    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    code = open(os.path.join(ROOT, "datum_amd", "host", "ocean.cpp"), encoding="utf-8").read()
    assert "void set_ocean_ripple_dispersion(OceanContext &context, OceanRippleDispersion mode, float g = 9.81f)" in shim
    assert "Wave = 0" in shim and "Deep = 1" in shim
    assert hasattr(host_api.load(), "datum_host_set_ocean_ripple_dispersion") and callable(host_api.OceanContext.set_ocean_ripple_dispersion)
    assert 'throw runtime_error("set_ocean_ripple_dispersion: the context is not prepared (prepare_ocean_context)")' in code
