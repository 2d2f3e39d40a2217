"""CPU tests of ripple swell's interface (include/datum_ocean_hip.h: "ripple swell"): the header declares the entry points and states the
definition, the library exports them, the bindings have their methods and signatures, a null handle is EINVAL, the kernels reach their
arithmetic through ocean_ripple_swell.h alone, the parents' kernel files keep their text, and the swell's kernels are chosen in
launch_ripple_step and nowhere else.  (The refusals that need a handle are in tests/test_gpu_ripple_swell.py: a handle needs a device.)"""

import ctypes
import os
import re

import numpy as np

import ripple_swell64 as rs
from test_body_abi import read_csrc
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

SYMBOLS = ("datum_ocean_set_ripple_swell", "datum_ocean_refresh_ripple_swell", "datum_ocean_ripple_swell_device", "datum_ocean_read_ripple_swell")


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
    for method in ("set_ripple_swell", "refresh_ripple_swell", "ripple_swell_device", "read_ripple_swell"):
        assert callable(getattr(capi.Ocean, method)), method
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    I, P = capi.I, capi.P
    assert capi.SYMBOLS["datum_ocean_set_ripple_swell"] == (I, [P, I])
    assert capi.SYMBOLS["datum_ocean_refresh_ripple_swell"] == (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(capi.OceanSet), I])
    assert capi.SYMBOLS["datum_ocean_ripple_swell_device"] == (I, [P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(I)])
    assert capi.SYMBOLS["datum_ocean_read_ripple_swell"] == (I, [P, P])
    assert "int datum_ocean_set_ripple_swell(datum_ocean_t ctx, int on);" in text
    assert "int datum_ocean_refresh_ripple_swell(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations);" in text
    assert "int datum_ocean_ripple_swell_device(datum_ocean_t ctx, void **plane, size_t *bytes, int *current);" in text
    assert "int datum_ocean_read_ripple_swell(datum_ocean_t ctx, float *plane);" in text
    # the stepping calls keep their signatures: the swell is the layer's, not an argument
    assert "int datum_ocean_step_ripples(datum_ocean_t ctx, float dt, int substeps);" in text
    assert (rs.WAVE, rs.DEEP) == (capi.RIPPLE_WAVE, capi.RIPPLE_DEEP)


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- ripple swell (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("OPT-IN", "SCATTERED FIELD", "nothing is allocated, the parents' kernels are launched, and every call\n * keeps its bits",
                 "the renderer changes nothing", "(J mod R)·R + (I mod R)", "by its wall byte while the bed is off (no walls: nothing is solid)",
                 "by d == +0 while the bed is on", "a neighbour outside the window never counts", "dX = (neighbour X counts) ? (Hc − Hn) : +0.0f",
                 "F  = (dL + dR) + (dD + dU)", "for a solid cell, and (the sum of four +0) for a cell none of whose neighbours count",
                 "x = ((float)I + 0.5f) · s", "FIELD 2 OF datum_ocean_sample_surface_blend's record", "no contraction",
                 "lap = (((eL + eR) + (eD + eU)) − 4.0f·e) + F", "div = ((tL + tR) + (tD + tU)) + dc·F", "THE FACE AT A SOLID NEIGHBOUR CARRIES THE CELL'S OWN DEPTH",
                 "F IS FROZEN OVER THE SUB-STEPS OF A CALL", "its only\n * writer", "datum_ocean_center_ripples when the origin moves",
                 "datum_ocean_set_ripple_walls, datum_ocean_set_ripple_bed, datum_ocean_set_ripples and datum_ocean_set_ripple_swell",
                 "WHILE THE MARK IS\n * CLEAR THE PARENTS' KERNELS ARE LAUNCHED", "displace -> center_ripples -> refresh_ripple_swell -> step_ripples or\n * step_bodies_coupled",
                 "datum_ocean_reset_ripples keeps the plane and the mark", "DO NOT COMBINE", "a mask, not a face flux", "256-byte guards of 0xCD",
                 "`on`\n *                          outside {0, 1}", "DATUM_OCEAN_ESTATE while the layer is off or its mode is DEEP",
                 "ONE launch on the handle's stream writes F WHOLE", "null, 0 and 0 while swell is\n *                          off",
                 "IN MEMORY ORDER", "LEFT OUT: swell in DEEP", "H itself shoaling or breaking over the bed",
                 "a swell that\n * changes within a call's sub-steps", "datum_ocean_sample_velocity_blend", "walls in the bilinear sample's patch"):
        assert line in section, line
    # the bed's "left out" is struck in part only
    bed = text.split("/* -- ripple bed (added at ABI 9; nothing in the reference)")[1].split("/* -- ripple swell")[0]
    assert "is struck in part" in bed and "H\n * itself still does not shoal" in bed


def test_null_handle_is_einval():
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    arr = (capi.I * 1)(0)
    plane = np.zeros(4, np.float32)
    ptr, nbytes, cur = capi.P(), ctypes.c_size_t(5), capi.I(7)
    for name, args in (("datum_ocean_set_ripple_swell", (1,)), ("datum_ocean_set_ripple_swell", (0,)), ("datum_ocean_set_ripple_swell", (2,)),
                       ("datum_ocean_refresh_ripple_swell", (arr, 1, ctypes.byref(s), 4)), ("datum_ocean_refresh_ripple_swell", (None, 0, None, 0)),
                       ("datum_ocean_ripple_swell_device", (ctypes.byref(ptr), ctypes.byref(nbytes), ctypes.byref(cur))),
                       ("datum_ocean_read_ripple_swell", (plane.ctypes.data_as(capi.P),))):
        assert getattr(lib, name)(None, *args) == capi.EINVAL, name
        assert name.encode() in lib.datum_ocean_last_error(None), name
    assert ptr.value is None and nbytes.value == 5 and cur.value == 7 and not plane.any()


def test_the_kernels_call_the_header():
    """the arithmetic stands once, in ocean_ripple_swell.h, which the CPU walks; the parents' files keep their text; the swell's kernels are
    chosen in launch_ripple_step and nowhere else"""
    kernel, header, host = read_csrc("ocean_ripple_swell.hip"), read_csrc("ocean_ripple_swell.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_ripple_swell.h"' in kernel and '#include "ocean_ripple_bed.hip"' in kernel and '#include "ocean_ripple_bed.h"' in header
    assert '#include "ocean_ripple_swell.hip"' in host
    code = kernel.split("#pragma once")[1]
    body = header.split("#pragma once")[1]
    assert "fmaf" not in header and "fmaf" not in kernel and "asm" not in code and "atomic" not in code and "/" not in re.sub(r"//.*", "", body).replace('"', "")
    for word in ("sinf", "cosf", "sqrt", "tanh"):
        assert word not in body and word not in code, word
    for fn in ("ripple_swell_solid(", "ripple_swell_solid_bed(", "ripple_swell_counts(", "ripple_swell_face(", "ripple_swell_force(", "ripple_swell_centre(",
               "ripple_swell_update(", "ripple_swell_bed_update("):
        assert len(re.findall(r"OB_HD [\w ]+ " + re.escape(fn), header)) == 1, fn
        assert fn in code, fn
    # the parents' functions are called as they stand, and none is copied
    for fn in ("ripple_wall_pin(", "ripple_wall_neighbour(", "ripple_bed_flux(", "ripple_height(", "ripple_sponge(", "ripple_wrap(", "ripple_world("):
        assert fn in code or fn in body, fn
    for copy in ("OB_HD int ripple_wrap", "OB_HD int ripple_sponge", "OB_HD float ripple_height", "struct RippleCell ", "RIPPLE_UNIT", "OB_HD RippleCell ripple_update",
                 "OB_HD float ripple_bed_flux", "OB_HD float ripple_wall_neighbour", "OB_HD RippleCell ripple_wall_pin", "OB_HD RippleCell ripple_bed_update"):
        assert copy not in header and copy not in code, copy
    for copy in ("4.0f *", "0.5f", "a.b.gs2 *", "p.h *", "p.c2s2 *", "Hc - ", "+ F"):
        assert copy not in code, copy
    # the heights are the several-cascade query's, asked once in the file
    assert code.count("query_height<LAYOUT>(a.q, query_solve<LAYOUT>(a.q, p))") == 1 and code.count("query_frame(a.q)") == 1
    for name, tmpl in (("ocean_ripple_swell_refresh_kernel", "int LAYOUT"), ("ocean_ripple_step_walls_swell_kernel", "bool FIRST"), ("ocean_ripple_bed_swell_step_kernel", "bool FIRST")):
        assert re.search(r"template<" + tmpl + r">\s+__global__ void __launch_bounds__\(RIPPLE_THREADS\) " + name + r"\(", code), name
    assert set(re.findall(r"buf_load\w*\((r\w+),", code)) == {"rin", "rsrc", "rwall", "rbed", "rsurf", "rswell"}
    assert set(re.findall(r"buf_store\w*(?:<\w+>)?\([^;]*?, (r\w+), ", code)) == {"rout", "rswell"}
    for text in ("__shared__ unsigned int flag[RIPPLE_TY + 2][RIPPLE_LX]", "__shared__ float bed[RIPPLE_TY + 2][RIPPLE_LX]", "make_rsrc(a.swell, cells * sizeof(float))",
                 "__builtin_amdgcn_ballot_w64(any != 0) == 0", "#pragma unroll 1"):
        assert text in code, text
    assert code.count("buf_store_f32_aux<RIPPLE_STORE_AUX>(") == 2 and code.count("buf_load_f32(rswell, ") == 2
    # the parents: no word of ripple swell in their files
    for parent in ("ocean_ripple.hip", "ocean_ripple.h", "ocean_ripple_deep.hip", "ocean_ripple_deep.h", "ocean_ripple_wall.hip", "ocean_ripple_wall.h",
                   "ocean_ripple_bed.hip", "ocean_ripple_bed.h", "ocean_ripple_foam.hip", "ocean_ripple_bounds.hip", "ocean_rippled.hip", "ocean_query.hip"):
        text = read_csrc(parent).lower()
        assert "ripple_swell" not in text and "ripple swell" not in text and "rippleswell" not in text, parent
    emul = open(os.path.join(ROOT, "tests", "cpu", "ripple_swell_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_ripple_swell.h", "ripple_swell_force(", "ripple_swell_face(", "ripple_swell_counts(", "ripple_swell_update(", "ripple_swell_bed_update(", "ripple_bed_flux(",
               "ripple_wall_neighbour("):
        assert fn in emul, fn
    make = open(os.path.join(ROOT, "Makefile"), encoding="utf-8").read()
    assert "tests/cpu/ripple_swell_emul.cpp" in make and make.count("datum_amd/csrc/ocean_ripple_swell.h ") == 2 and "datum_amd/csrc/ocean_ripple_swell.hip" in make
    # one place launches the swell's step kernels; the stepping loops read as before
    assert host.count("launch_ripple_step_walls_swell(") == 1 and host.count("launch_ripple_bed_swell_step(") == 1 and host.count("launch_ripple_swell_refresh(") == 1
    chooser = host.split("hipError_t launch_ripple_step(RippleStep &r, bool first, hipStream_t stream)")[1].split("\n  }\n")[0]
    assert "launch_ripple_step_walls_swell(" in chooser and "launch_ripple_bed_swell_step(" in chooser and chooser.count("if (r.swell") == 2
    step = host.split("int datum_ocean_step_ripples(")[1].split("int datum_ocean_deposit_ripples(")[0]
    coupled = host.split("int run_step_bodies_coupled(")[1].split('extern "C"')[0]
    assert "swell" not in step.lower() and "swell" not in coupled.lower().replace("swell terms", "")
    # the mark: one writer sets it; the five calls clear it (set_ripples through the plane's release); a sub-step reads the plane through it
    assert host.count("ctx->rippleswell.current = true") == 1 and host.count("ctx->rippleswell.current = false") == 3
    assert host.count("ctx->rippleswell.off()") == 4 and host.count("ctx->rippleswell.fresh()") == 1
    section = host.split("/* -- ripple swell: a forcing plane beside the ripple layer (ocean_ripple_swell.hip)")[1].split("/* -- wake foam:")[0]
    assert section.count("check_ripple_swell(ctx, ") == 2 and section.count("check_query(ctx, q, ") == 1 and section.count("check_ripples(ctx, ") == 2
    for word in ("hipMemset(", "hipMemcpy(", "hipDeviceSynchronize", "read_ripple_window"):
        assert word not in section, word
    setter = host.split("int datum_ocean_set_ripple_dispersion(")[1].split("int datum_ocean_ripple_deep_weights(")[0]
    assert "mode == DATUM_OCEAN_RIPPLE_DEEP && ctx->rippleswell" in setter and setter.count("DATUM_OCEAN_ESTATE") == 2


def test_shim_declarations_present():
    from datum_amd import host_api

    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    code = open(os.path.join(ROOT, "datum_amd", "host", "ocean.cpp"), encoding="utf-8").read()
    assert "void set_ocean_ripple_swell(OceanContext &context, bool on);" in shim
    assert "void refresh_ocean_ripple_swell(OceanContext &context, OceanParams const &params, int iterations = 4);" in shim
    assert "void read_ocean_ripple_swell(OceanContext &context, float *plane" in shim
    lib = host_api.load()
    for name in ("set_ocean_ripple_swell", "refresh_ocean_ripple_swell", "read_ocean_ripple_swell"):
        assert hasattr(lib, "datum_host_" + name) and callable(getattr(host_api.OceanContext, name)), name
        assert 'throw runtime_error("' + name + ': the context is not prepared (prepare_ocean_context)")' in code, name
    assert "datum_ocean_refresh_ripple_swell(context.hip, &cascade, 1, &set, iterations)" in code
