"""CPU tests of ripple walls' interface (include/datum_ocean_hip.h: "ripple walls"): the header declares the three entry points and the
32-byte record and states the definition, the library exports them, the bindings have their methods and signatures, the ABI stays 9, every
new call answers a null handle with EINVAL, the kernels reach their arithmetic through ocean_ripple_wall.h and leave the parents' files
alone, every wall decision of the host stands in launch_ripple_step, and the C++ shim declares its calls.  (The refusals that need a handle
are in tests/test_gpu_ripple_walls.py: a handle needs a device.)"""

import ctypes
import os
import re

import numpy as np

import ripple_wall64 as rw
from test_body_abi import read_csrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

SYMBOLS = ("datum_ocean_set_ripple_walls", "datum_ocean_ripple_walls_device", "datum_ocean_read_ripple_walls")


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
    for method in ("set_ripple_walls", "ripple_walls_device", "read_ripple_walls"):
        assert callable(getattr(capi.Ocean, method)), method
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    assert capi.SYMBOLS["datum_ocean_set_ripple_walls"] == (capi.I, [capi.P, capi.P, capi.I])
    assert capi.SYMBOLS["datum_ocean_ripple_walls_device"] == (capi.I, [capi.P, ctypes.POINTER(capi.P)])
    assert capi.SYMBOLS["datum_ocean_read_ripple_walls"] == (capi.I, [capi.P, capi.P])
    assert "int datum_ocean_set_ripple_walls(datum_ocean_t ctx, datum_ocean_ripple_wall const *walls, int count);" in text
    assert "int datum_ocean_ripple_walls_device(datum_ocean_t ctx, unsigned char const **plane);" in text
    assert "int datum_ocean_read_ripple_walls(datum_ocean_t ctx, unsigned char *host);" in text
    for define, value in (("DATUM_OCEAN_RIPPLE_WALL_BOX", 0), ("DATUM_OCEAN_RIPPLE_WALL_ELLIPSE", 1), ("DATUM_OCEAN_RIPPLE_MAX_WALLS", 256)):
        assert re.search(r"#define\s+" + define + r"\s+" + str(value) + r"\s", text), define
    assert (capi.RIPPLE_WALL_BOX, capi.RIPPLE_WALL_ELLIPSE, capi.RIPPLE_MAX_WALLS) == (rw.BOX, rw.ELLIPSE, rw.MAX_WALLS) == (0, 1, 256)
    # the stepping calls keep their signatures: walls are the layer's, not an argument
    assert "int datum_ocean_step_ripples(datum_ocean_t ctx, float dt, int substeps);" in text
    assert "int datum_ocean_center_ripples(datum_ocean_t ctx, float x, float y);" in text


def test_record_is_32_bytes_with_its_offsets():
    from datum_amd import capi

    text = _header()
    struct = text.split("typedef struct datum_ocean_ripple_wall\n{")[1].split("} datum_ocean_ripple_wall;")[0]
    fields = re.findall(r"^\s*(float|int) (\w+)(?:\[(\d)\])?;", struct, re.M)
    assert fields == [("float", "center", "2"), ("float", "axis", "2"), ("float", "half", "2"), ("int", "kind", ""), ("int", "reserved", "")]
    for dt in (capi.RIPPLE_WALL, rw.WALL):
        assert dt.itemsize == 32
        assert [(n, dt.fields[n][1]) for n in dt.names] == [("center", 0), ("axis", 8), ("half", 16), ("kind", 24), ("reserved", 28)]
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    assert lib.ripple_wall_emul_sizeof() == 32
    # the compiled record, field by field: a box that only the right offsets make cover the cell (0, 0) and no other of a 64 x 64 window
    w = rw.box(0.25, 0.25, 0.1, 0.1)
    plane = np.zeros((64, 64), np.uint8)
    lib.ripple_wall_emul_raster.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float]
    lib.ripple_wall_emul_raster(w.ctypes.data_as(ctypes.c_void_p), 1, plane.ctypes.data_as(ctypes.c_void_p), 64, -32, -32, 0.5)
    assert plane.sum() == 1 and plane[0, 0] == 1


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- ripple walls (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("OPT-IN", "every call keeps its bits in both step modes", "R × R bytes, 0 water, 1 wall", "(J mod R)·R + (I mod R)",
                 "GIVEN BY THE CALLER AS (cosine, sine)", "DOES NOT NORMALISE", "a non-unit axis scales the shape",
                 "x  = ((float)I + 0.5f) · s", "u  = dx·axis[0] + dy·axis[1]        v  = dy·axis[0] − dx·axis[1]",
                 "BOX:      |u| <= half[0] && |v| <= half[1]", "ELLIPSE:  a = u·half[1], b = v·half[0], r = half[0]·half[1];   a·a + b·b <= r·r",
                 "no division", "A cell is wall if any record covers its centre", "a function of (list, world cell) only",
                 "a jump of R cells or more included", "rasterises the whole plane again behind the scroll",
                 "(+0.0f, +0.0f) in both modes", "its src is ignored", "the wall flag of the torus-aliased cell is not consulted",
                 "a wall neighbour reads as the cell's own e", "a wall cell reads 0.0f in the convolution, the pending deposit of a first sub-step included",
                 "No new stability refusal", "graph Laplacian of the open cells", "principal submatrix",
                 "`walls` is a HOST pointer", "the handle keeps its own copy", "count == 0 turns walls off", "in BOTH state buffers",
                 "the ripple bounds' CURRENT mark is cleared", "DATUM_OCEAN_ESTATE while\n *                          the layer is off",
                 "datum_ocean_set_ripples with any R drops the walls", "datum_ocean_reset_ripples keeps them", "null while walls are off",
                 "as datum_ocean_read_ripple_foam", "LEFT OUT: moving walls and hull footprints as walls", "fractional obstruction",
                 "a count of deposits lost on wall cells; finite depth; a shoreline"):
        assert line in section, line


def test_null_handle_is_einval():
    from datum_amd import capi

    lib = capi.load()
    one = rw.box(0, 0, 1, 1)
    ptr, plane = capi.P(), np.zeros(4, np.uint8)
    for name, args in (("datum_ocean_set_ripple_walls", (one.ctypes.data_as(capi.P), 1)), ("datum_ocean_set_ripple_walls", (None, 0)),
                       ("datum_ocean_ripple_walls_device", (ctypes.byref(ptr),)), ("datum_ocean_read_ripple_walls", (plane.ctypes.data_as(capi.P),))):
        assert getattr(lib, name)(None, *args) == capi.EINVAL, name
        assert name.encode() in lib.datum_ocean_last_error(None), name
    assert ptr.value is None and not plane.any()


def test_the_kernels_call_the_header():
    """the arithmetic stands once, in ocean_ripple_wall.h, which the CPU walks; the parents' files keep their text; every wall decision of
    the host stands in launch_ripple_step"""
    kernel, header, host = read_csrc("ocean_ripple_wall.hip"), read_csrc("ocean_ripple_wall.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_ripple_wall.h"' in kernel and '#include "ocean_ripple_deep.hip"' in kernel and '#include "ocean_ripple_deep.h"' in header
    assert '#include "ocean_ripple_wall.hip"' in host
    code = kernel.split("#pragma once")[1]
    body = header.split("#pragma once")[1]
    assert "fmaf" not in body and "fmaf(" not in code and "asm" not in code and "atomic" not in code and "/" not in re.sub(r"//.*", "", body).replace('"', "")
    for word in ("sinf", "cosf", "sincos", "sqrt"):
        assert word not in body and word not in code, word
    for fn in ("ripple_wall_covers(", "ripple_wall_cell(", "ripple_wall_neighbour(", "ripple_wall_height(", "ripple_wall_pin("):
        assert len(re.findall(r"OB_HD [\w ]+ " + re.escape(fn), header)) == 1 and fn in code or fn == "ripple_wall_covers(", fn
    for fn in ("ripple_update(", "ripple_deep_row(", "ripple_deep_update(", "ripple_height(", "ripple_sponge(", "ripple_wrap(", "ripple_world("):
        assert fn in code, fn
    for copy in ("OB_HD int ripple_wrap", "OB_HD int ripple_sponge", "OB_HD float ripple_height", "struct RippleCell", "RIPPLE_UNIT", "OB_HD RippleCell ripple_update"):
        assert copy not in header and copy not in code, copy
    for name in ("ocean_ripple_wall_raster_kernel", "ocean_ripple_step_walls_kernel", "ocean_ripple_deep_step_walls_kernel"):
        assert re.search(r"__global__ void __launch_bounds__\(RIPPLE_THREADS\) " + name + r"\(", code), name
    assert set(re.findall(r"buf_load\w*\((r\w+),", code)) == {"rin", "rsrc", "rwall"} and "make_rsrc(a.wall, cells)" in code
    # the parents: no word of walls in their files
    for parent in ("ocean_ripple.hip", "ocean_ripple.h", "ocean_ripple_deep.hip", "ocean_ripple_deep.h"):
        assert "wall" not in read_csrc(parent).lower(), parent
    emul = open(os.path.join(ROOT, "tests", "cpu", "ripple_wall_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_ripple_wall.h", "ripple_wall_cell(", "ripple_wall_neighbour(", "ripple_wall_height(", "ripple_wall_pin(", "ripple_update(", "ripple_deep_conv("):
        assert fn in emul, fn
    make = open(os.path.join(ROOT, "Makefile"), encoding="utf-8").read()
    assert "tests/cpu/ripple_wall_emul.cpp" in make and make.count("datum_amd/csrc/ocean_ripple_wall.h ") == 2 and "datum_amd/csrc/ocean_ripple_wall.hip" in make
    # one place launches the walled kernels; the stepping loops read as before
    assert host.count("launch_ripple_step_walls(") == 1 and host.count("launch_ripple_deep_step_walls(") == 1
    chooser = host.split("hipError_t launch_ripple_step(RippleStep &r, bool first, hipStream_t stream)")[1].split("\n  }\n")[0]
    assert "launch_ripple_step_walls(" in chooser and "launch_ripple_deep_step_walls(" in chooser
    step = host.split("int datum_ocean_step_ripples(")[1].split("int datum_ocean_deposit_ripples(")[0]
    coupled = host.split("int run_step_bodies_coupled(")[1].split('extern "C"')[0]
    assert "wall" not in step.lower() and "wall" not in coupled.lower()
    assert host.count("raster_ripple_walls(ctx, ") == 2 and host.count("free_ripple_walls(ctx)") == 3


def test_shim_declarations_present():
    from datum_amd import host_api

    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    code = open(os.path.join(ROOT, "datum_amd", "host", "ocean.cpp"), encoding="utf-8").read()
    assert "typedef datum_ocean_ripple_wall OceanRippleWall;" in shim
    assert "void set_ocean_ripple_walls(OceanContext &context, OceanRippleWall const *walls, size_t count);" in shim
    assert "void read_ocean_ripple_walls(OceanContext &context, unsigned char *plane" in shim
    lib = host_api.load()
    assert hasattr(lib, "datum_host_set_ocean_ripple_walls") and hasattr(lib, "datum_host_read_ocean_ripple_walls")
    assert callable(host_api.OceanContext.set_ocean_ripple_walls) and callable(host_api.OceanContext.read_ocean_ripple_walls)
    assert 'throw runtime_error("set_ocean_ripple_walls: the context is not prepared (prepare_ocean_context)")' in code
