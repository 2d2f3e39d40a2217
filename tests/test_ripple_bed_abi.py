"""CPU tests of the ripple bed's interface (include/datum_ocean_hip.h: "ripple bed"): the header declares the three entry points and the
40-byte record and states the definition, the library exports them, the bindings have their methods and signatures, the ABI stays 9, every
new call answers a null handle with EINVAL, the kernels reach their arithmetic through ocean_ripple_bed.h and leave the parents' files
alone, the bed's kernel is chosen in launch_ripple_step, and the C++ shim declares its calls.  (The refusals that need a handle are in
tests/test_gpu_ripple_bed.py: a handle needs a device.)"""

import ctypes
import os
import re

import numpy as np

import ripple_bed64 as rb
from test_body_abi import read_csrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

SYMBOLS = ("datum_ocean_set_ripple_bed", "datum_ocean_ripple_bed_device", "datum_ocean_read_ripple_bed")


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
    for method in ("set_ripple_bed", "ripple_bed_device", "read_ripple_bed"):
        assert callable(getattr(capi.Ocean, method)), method
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    assert capi.SYMBOLS["datum_ocean_set_ripple_bed"] == (capi.I, [capi.P, capi.P, capi.P])
    assert capi.SYMBOLS["datum_ocean_ripple_bed_device"] == (capi.I, [capi.P, ctypes.POINTER(capi.P), ctypes.POINTER(capi.P), ctypes.POINTER(ctypes.c_size_t)])
    assert capi.SYMBOLS["datum_ocean_read_ripple_bed"] == (capi.I, [capi.P, capi.P, capi.P])
    assert "int datum_ocean_set_ripple_bed(datum_ocean_t ctx, datum_ocean_ripple_bed const *bed, float const *depths_host);" in text
    assert "int datum_ocean_ripple_bed_device(datum_ocean_t ctx, void **depth, void **surf, size_t *cells);" in text
    assert "int datum_ocean_read_ripple_bed(datum_ocean_t ctx, float *depth, unsigned char *surf);" in text
    for define, value in (("DATUM_OCEAN_RIPPLE_SURF_LEVELS", 16), ("DATUM_OCEAN_RIPPLE_BED_MAX_SIDE", 4096)):
        assert re.search(r"#define\s+" + define + r"\s+" + str(value) + r"\s", text), define
    assert (capi.RIPPLE_SURF_LEVELS, capi.RIPPLE_BED_MAX_SIDE) == (rb.SURF_LEVELS, rb.MAX_SIDE) == (16, 4096)
    # the stepping calls keep their signatures: the bed is the layer's, not an argument
    assert "int datum_ocean_step_ripples(datum_ocean_t ctx, float dt, int substeps);" in text
    assert "int datum_ocean_center_ripples(datum_ocean_t ctx, float x, float y);" in text


def test_record_is_40_bytes_with_its_offsets():
    from datum_amd import capi

    text = _header()
    struct = text.split("typedef struct datum_ocean_ripple_bed\n{")[1].split("} datum_ocean_ripple_bed;")[0]
    fields = re.findall(r"^\s*(float|int) ([\w, ]+?)(?:\[(\d)\])?;", struct, re.M)
    assert fields == [("int", "width, height", ""), ("float", "origin", "2"), ("float", "texel", ""), ("float", "outside", ""), ("float", "max_depth", ""),
                      ("float", "dry_depth", ""), ("float", "surf_depth", ""), ("float", "surf_gamma", "")]
    for dt in (capi.RIPPLE_BED, rb.BED):
        assert dt.itemsize == 40
        assert [(n, dt.fields[n][1]) for n in dt.names] == [("width", 0), ("height", 4), ("origin", 8), ("texel", 16), ("outside", 20), ("max_depth", 24),
                                                            ("dry_depth", 28), ("surf_depth", 32), ("surf_gamma", 36)]
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    assert lib.ripple_bed_emul_sizeof() == 40
    # the compiled record, field by field: a 3 x 2 map that only the right offsets put over the cells (0 .. 2, 0 .. 1) of a 64 x 64 window, with
    # every parameter doing its work there: the clamp, the dry cell, the surf level, `outside`
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ripple_bed_emul_raster.argtypes = [P, P, P, P, P, I, I, I, Fl]
    b = np.array([rb.bed(3, 2, (0.25, 0.25), 0.5, outside=3.5, max_depth=4.0, dry_depth=0.5, surf_depth=2.0, surf_gamma=1.0)], rb.BED)
    depths = np.array([[9.0, 0.25, 1.0], [3.0, 2.0, 1.5]], np.float32)
    d, q = np.zeros((64, 64), np.float32), np.zeros((64, 64), np.uint8)
    lib.ripple_bed_emul_raster(b.ctypes.data_as(P), depths.ctypes.data_as(P), None, d.ctypes.data_as(P), q.ctypes.data_as(P), 64, -32, -32, 0.5)
    assert d[:2, :3].tolist() == [[4.0, 0.0, 1.0], [3.0, 2.0, 1.5]] and q[:2, :3].tolist() == [[0, 0, 8], [0, 0, 4]]
    assert (d == 3.5).sum() == 64 * 64 - 6 and not q[d == 3.5].any()


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- ripple bed (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("OPT-IN", "the parents' kernels are launched, and every call keeps its bits in both step modes", "POSITIVE DOWN",
                 "2 <= width, height <= DATUM_OCEAN_RIPPLE_BED_MAX_SIDE = 4096", "`outside` is the depth that a cell off the map reads",
                 "The handle keeps a device copy of the map", "+0.0f where the cell is SOLID", "0 .. DATUM_OCEAN_RIPPLE_SURF_LEVELS = 16",
                 "a function of (map, parameters, wall plane, world cell) only", "a jump of R cells or more included", "no\n * division",
                 "invt = (float)(1.0 / texel) and invsurf = (float)(1.0 / surf_depth) are rounded once on the host from double",
                 "x = ((float)I + 0.5f) · s", "u = (x − origin[0]) · invt", "u < 0 or u > width − 1 or v < 0 or v > height − 1:   raw = outside",
                 "i = min((int)floorf(u), width − 2)", "a0 = c1 − c0, a1 = c3 − c2, e0 = c0 + wu·a0, e1 = c2 + wu·a1, raw = e0 + wv·(e1 − e0)",
                 "d = fminf(fmaxf(raw, 0), max_depth);   d < dry_depth -> d = +0;   the cell's wall byte is 1 (walls on) -> d = +0",
                 "q = 0 where d == 0 or surf_depth == 0 or d >= surf_depth, else min(16, (int)floorf((1 − d·invsurf)·16))",
                 "t = dc·(0 − e)", "the neighbour is solid (dn == 0):", "t = (0.5f·(dc + dn))·(en − e)",
                 "div = (tL + tR) + (tD + tU);   f = fsponge[k]·fsurf[q];   v1 = (η_t + h·(gs2·div))·f;   η' = e + h·v1;   η_t' = v1",
                 "gs2 = (float)(g / s²)", "fsurf[q] = (float)(1 / (1 + h·surf_gamma·(q/16)²))", "With surf_depth == 0 the factor is exactly 1.0f",
                 "A solid cell's new state is (+0.0f, +0.0f)", "is lost, uncounted, as on a wall", "c IS NOT USED BY THE STEP",
                 "symmetric on the wet cells", "4·max_depth", "c := sqrt(g·max_depth)", "above 0.7", "DO NOT COMBINE", "a variable depth is not a convolution",
                 "Uniform finite depth for DEEP stays left out", "a null `bed` turns the bed off and frees everything", "in BOTH state buffers",
                 "the ripple bounds' CURRENT mark\n *                          is cleared", "a map value that is not finite (checked on the host)",
                 "DATUM_OCEAN_ESTATE while the layer is off\n *                          or its mode is DEEP", "datum_ocean_set_ripples with any R drops the bed",
                 "datum_ocean_reset_ripples keeps it", "datum_ocean_center_ripples rebuilds both planes whole, in one launch",
                 "datum_ocean_set_ripple_walls rasters the bed again", "null and 0 while\n *                          the bed is off",
                 "as datum_ocean_read_ripple_walls", "LEFT OUT: the bed in DEEP, as tanh(k·d) weights", "wetting and drying, run-up and non-linear steepening",
                 "foam from the surf zone", "the FFT swell feeling the\n * bed", "writing only the entered cells on a scroll; temporal blocking"):
        assert line in section, line


def test_null_handle_is_einval():
    from datum_amd import capi

    lib = capi.load()
    b = np.array([rb.bed(2, 2, (0, 0), 1.0)], rb.BED)
    depths, plane = np.ones(4, np.float32), np.zeros(4, np.float32)
    ptr, cells = capi.P(), ctypes.c_size_t(5)
    for name, args in (("datum_ocean_set_ripple_bed", (b.ctypes.data_as(capi.P), depths.ctypes.data_as(capi.P))), ("datum_ocean_set_ripple_bed", (None, None)),
                       ("datum_ocean_ripple_bed_device", (ctypes.byref(ptr), None, ctypes.byref(cells))), ("datum_ocean_read_ripple_bed", (plane.ctypes.data_as(capi.P), None))):
        assert getattr(lib, name)(None, *args) == capi.EINVAL, name
        assert name.encode() in lib.datum_ocean_last_error(None), name
    assert ptr.value is None and cells.value == 5 and not plane.any()


def test_the_kernels_call_the_header():
    """the arithmetic stands once, in ocean_ripple_bed.h, which the CPU walks; the parents' files keep their text; the bed's kernel is chosen
    in launch_ripple_step and nowhere else"""
    kernel, header, host = read_csrc("ocean_ripple_bed.hip"), read_csrc("ocean_ripple_bed.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_ripple_bed.h"' in kernel and '#include "ocean_ripple_wall.hip"' in kernel and '#include "ocean_ripple_wall.h"' in header
    assert '#include "ocean_ripple_bed.hip"' in host
    code = kernel.split("#pragma once")[1]
    body = header.split("#pragma once")[1]
    assert "fmaf" not in header and "fmaf" not in kernel and "asm" not in code and "atomic" not in code and "/" not in re.sub(r"//.*", "", body).replace('"', "")
    for word in ("sinf", "cosf", "sqrt", "tanh"):
        assert word not in body and word not in code, word
    for fn in ("ripple_bed_raw(", "ripple_bed_depth(", "ripple_bed_surf(", "ripple_bed_cell(", "ripple_bed_flux(", "ripple_bed_update("):
        assert len(re.findall(r"OB_HD [\w ]+ " + re.escape(fn), header)) == 1, fn
    for fn in ("ripple_bed_cell(", "ripple_bed_flux(", "ripple_bed_update(", "ripple_height(", "ripple_sponge(", "ripple_wrap(", "ripple_world("):
        assert fn in code, fn
    # no second copy of the layer's helpers or of the update's products
    for copy in ("OB_HD int ripple_wrap", "OB_HD int ripple_sponge", "OB_HD float ripple_height", "struct RippleCell ", "RIPPLE_UNIT", "OB_HD RippleCell ripple_update"):
        assert copy not in header and copy not in code, copy
    for copy in ("a.gs2 *", "a.s.h *", "* a.fsurf", "0.5f"):
        assert copy not in code, copy
    for name in ("ocean_ripple_bed_raster_kernel", "ocean_ripple_bed_step_kernel"):
        assert re.search(r"__global__ void __launch_bounds__\(RIPPLE_THREADS\) " + name + r"\(", code), name
    assert set(re.findall(r"buf_load\w*\((r\w+),", code)) == {"rin", "rsrc", "rbed", "rsurf", "rmap"}
    assert set(re.findall(r"buf_store\w*(?:<\w+>)?\([^;]*?, (r\w+), ", code)) == {"rout"}
    for text in ("__shared__ float tile[RIPPLE_TY + 2][RIPPLE_LX]", "__shared__ float bed[RIPPLE_TY + 2][RIPPLE_LX]",
                 "make_rsrc(a.map, (size_t)a.b.width * a.b.height * sizeof(float))", "make_rsrc(a.depth, cells * sizeof(float))", "make_rsrc(a.surf, cells)"):
        assert text in code, text
    # the parents: no word of the bed in their files
    for parent in ("ocean_ripple.hip", "ocean_ripple.h", "ocean_ripple_deep.hip", "ocean_ripple_deep.h", "ocean_ripple_wall.hip", "ocean_ripple_wall.h"):
        assert "bed" not in read_csrc(parent).lower(), parent
    emul = open(os.path.join(ROOT, "tests", "cpu", "ripple_bed_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_ripple_bed.h", "ripple_bed_cell(", "ripple_bed_flux(", "ripple_bed_update(", "ripple_height(", "ripple_sponge("):
        assert fn in emul, fn
    make = open(os.path.join(ROOT, "Makefile"), encoding="utf-8").read()
    assert "tests/cpu/ripple_bed_emul.cpp" in make and make.count("datum_amd/csrc/ocean_ripple_bed.h ") == 2 and "datum_amd/csrc/ocean_ripple_bed.hip" in make
    # one place launches the bed's kernel; the stepping loops read as before; the rasters' call sites
    assert host.count("launch_ripple_bed_step(") == 1
    chooser = host.split("hipError_t launch_ripple_step(RippleStep &r, bool first, hipStream_t stream)")[1].split("\n  }\n")[0]
    assert "launch_ripple_bed_step(" in chooser
    step = host.split("int datum_ocean_step_ripples(")[1].split("int datum_ocean_deposit_ripples(")[0]
    coupled = host.split("int run_step_bodies_coupled(")[1].split('extern "C"')[0]
    assert "bed" not in step.lower() and "bed" not in coupled.lower()
    assert host.count("raster_ripple_bed(ctx, ") == 4 and host.count("free_ripple_bed(ctx)") == 3
    assert host.count("ctx->ripplebed.get() ? std::sqrt(ctx->rippleg * (double)ctx->ripplebedparams.max_depth) : ctx->ripplec") == 1
    setter = host.split("int datum_ocean_set_ripple_dispersion(")[1].split("int datum_ocean_ripple_deep_weights(")[0]
    assert "mode == DATUM_OCEAN_RIPPLE_DEEP && ctx->ripplebed" in setter and "DATUM_OCEAN_ESTATE" in setter


def test_shim_declarations_present():
    from datum_amd import host_api

    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    code = open(os.path.join(ROOT, "datum_amd", "host", "ocean.cpp"), encoding="utf-8").read()
    assert "typedef datum_ocean_ripple_bed OceanRippleBed;" in shim
    assert "void set_ocean_ripple_bed(OceanContext &context, OceanRippleBed const *bed, float const *depths);" in shim
    assert "void read_ocean_ripple_bed(OceanContext &context, float *depth" in shim
    lib = host_api.load()
    assert hasattr(lib, "datum_host_set_ocean_ripple_bed") and hasattr(lib, "datum_host_read_ocean_ripple_bed")
    assert callable(host_api.OceanContext.set_ocean_ripple_bed) and callable(host_api.OceanContext.read_ocean_ripple_bed)
    assert 'throw runtime_error("set_ocean_ripple_bed: the context is not prepared (prepare_ocean_context)")' in code
