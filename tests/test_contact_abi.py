"""CPU tests of body contact's interface (include/datum_ocean_hip.h: datum_ocean_step_bodies_contact): the header declares the entry points
and states the definition, the library exports them, the bindings have their methods, struct sizes and signatures, the argument checks
that need no device answer, and the kernel reaches its arithmetic through ocean_contact.h alone.  The refusals that need a handle (a null
contact struct, bad rates, unknown flags, a flag without its bed or walls, and that each leaves poses, motions, records and the layer
untouched) are tests/test_gpu_contact.py's: a handle needs the device."""

import ctypes
import os
import re

import numpy as np

import contact64
from test_body_abi import read_csrc
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")
SYMBOLS = ("datum_ocean_step_bodies_contact", "datum_ocean_step_bodies_contact_host")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_body_contact():
    from datum_amd import capi, host_api

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    for name in SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    for name in ("step_bodies_contact", "step_bodies_contact_host"):
        assert callable(getattr(capi.Ocean, name)), name
    assert callable(host_api.OceanContext.step_ocean_bodies_contact) and hasattr(host_api.load(), "datum_host_step_ocean_bodies_contact")
    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    for name in ("void step_ocean_bodies_contact(OceanContext &context", "struct OceanContactRecord", "sizeof(OceanContactRecord) == 64"):
        assert name in shim, name


def test_sizes_and_signatures():
    from datum_amd import capi

    emul = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    assert emul.contact_struct_bytes() == ctypes.sizeof(capi.BodyContact) == contact64.CONTACT.itemsize == 32
    assert emul.contact_record_floats() == capi.CONTACT_RECORD_FLOATS == contact64.RECORD_FLOATS == 16 and emul.contact_fields() == 22
    assert (capi.CONTACT_BED, capi.CONTACT_WALLS) == (contact64.BED, contact64.WALLS) == (1, 2)
    assert [(n, capi.BodyContact.__dict__[n].offset) for n, _ in capi.BodyContact._fields_] == [("stiffness", 0), ("damping", 4), ("friction", 8), ("flags", 12), ("reserved", 16)]
    for name in SYMBOLS:
        assert capi.SYMBOLS[name] == (capi.SYMBOLS["datum_ocean_step_bodies_coupled"][0], capi.SYMBOLS["datum_ocean_step_bodies_coupled"][1] + [capi.P]), name
    text = _header()
    for line in ("#define DATUM_OCEAN_CONTACT_RECORD_FLOATS 16", "#define DATUM_OCEAN_CONTACT_BED 1u", "#define DATUM_OCEAN_CONTACT_WALLS 2u", "float reserved[4];"):
        assert line in text, line


def test_header_states_definition():
    section = _header().split("/* -- body contact (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("zg = 0 − raw", "p  = zg − w.z", "TOUCHES when p > 0", "gx = (a0 + wv·(a1 − a0))·invt", "gy = (e1 − e0)·invt", "n = (0, 0, 1)", "UNCLAMPED",
                 "px = half[0] − |u|", "px <= py", "ρ = sqrt(eu·eu + ev·ev)", "q = (1 − ρ)·fminf(half[0], half[1])", "ρ == 0:  m = (1, 0)", "IN LIST ORDER",
                 "inv2 = (float)(1.0 / (axis[0]² + axis[1]²))", "DOES NOT NORMALISE THE AXIS", "NOT THE BYTE PLANE", "thinner than a cell",
                 "fn = fmaxf(a·(k·p − c·vn), 0)", "F  = fn·n − g·(u − vn·n)", "τ  = r × F", "twenty-two fields", "A body whose count is 0",
                 "DATUM_OCEAN_CONTACT_RECORD_FLOATS = 16 floats (64 bytes)", "sixteen quiet NaNs", "h·sqrt(k·Σa·invmass) < 2", "THE BOUND IS NOT CHECKED",
                 "a null\n * contact struct", "unknown flag bits", "flag BED with no bed set", "flag WALLS with no walls set", "A refused call enqueues nothing",
                 "Coulomb friction", "contact between bodies", "wall tops", "moving walls", "contact outside the coupled step"):
        assert line in section, line


def test_argument_errors_without_gpu():
    """no handle: EINVAL with the call's name in the text, and nothing written"""
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    bodies, motions, props = np.zeros(2, capi.BODY_DTYPE), np.zeros(2, capi.BODY_MOTION_DTYPE), np.zeros(2, capi.BODY_PROPS_DTYPE)
    probes, out = np.zeros((4, 4), np.float32), np.zeros((2, 16), np.float32)
    arr = (capi.I * 2)(0, 0)
    ptr = lambda a: a.ctypes.data_as(capi.P)
    con = capi.BodyContact(1.0, 1.0, 1.0, 0)
    for name in SYMBOLS:
        fn = getattr(lib, name)
        for c in (ctypes.cast(ctypes.byref(con), capi.P), None):
            assert fn(None, arr, 2, ctypes.byref(s), 4, ptr(bodies), ptr(motions), ptr(props), 2, ptr(probes), 4, 1 / 60, 1, ptr(out), c) == capi.EINVAL
            assert name.encode() in lib.datum_ocean_last_error(None)
    assert np.all(bodies.view(np.uint8) == 0) and np.all(motions.view(np.uint8) == 0) and np.all(out == 0)


def test_the_kernel_calls_the_headers():
    """the arithmetic stands once: ocean_contact.h calls the coupled step's, the step's, the bed's and the walls' headers and restates none;
    the kernel calls ocean_contact.h, the CPU walks the same header; the host loop is the coupled call's, stated once"""
    kernel, header, host = read_csrc("ocean_contact.hip"), read_csrc("ocean_contact.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_contact.h"' in kernel and '#include "ocean_couple.hip"' in kernel
    assert '#include "ocean_couple.h"' in header and '#include "ocean_ripple_bed.h"' in header
    assert "fmaf(" not in header and "fmaf(" not in kernel and "asm" not in kernel and kernel.count("atomicAdd(") == 1
    for word in ("__shared__", "__syncthreads"):
        assert word not in kernel, word
    for fn in ("contact_terms(", "contact_integrate(", "contact_fold(", "contact_zero("):
        assert fn in kernel, fn
        assert len(re.findall(r"OB_HD \w+ " + re.escape(fn), header)) == 1, fn
    for fn in ("ripple_bed_patch(", "ripple_wall_covers(", "step_integrate(", "couple_fold(", "step_norm(", "body_add(p.c, t.c)"):
        assert fn in header, fn
    # no copy of the integrator, of the patch or of the cover test
    for copy in ("floorf(", "p.invmass", "invinertia", "p.gravity", "half[1];\n\n    return a * a"):
        assert copy not in header and copy not in kernel, copy
    assert kernel.count("query_solve<LAYOUT>(") == 1 and kernel.count("query_velocity<LAYOUT>(") == 1 and kernel.count("body_walk(") == 2
    assert set(re.findall(r"buf_store\w*(?:<\d+>)?\([^;]*?, (r\w+), \d+, 0\);", kernel)) == {"rrecord", "rbody", "rmotion"}
    assert set(re.findall(r"buf_load\w*\((r\w+),", kernel)) == {"rstate", "rmap"}
    assert "make_rsrc(ca.map, (size_t)ca.s.bed.width * ca.s.bed.height * sizeof(float))" in kernel
    emul = open(os.path.join(ROOT, "tests", "cpu", "contact_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_contact.h", "contact_terms(", "contact_integrate(", "contact_fold(", "body_tree("):
        assert fn in emul, fn
    # one loop for both calls: one layer sub-step, one memset, one stability check
    assert host.count("launch_ripple_step(r, true, ctx->stream)") == 1 and host.count("int run_step_bodies_coupled(") == 1
    section = host.split("/* -- body contact (ocean_contact.hip)")[1].split("/* -- rippled reads")[0]
    assert section.count("check_coupled_args(") == 2 and section.count("run_step_bodies_coupled(") == 2 and "hipMemsetAsync" not in section and "launch_" not in section
    # ripple_bed_raw is stated through the patch
    bed = read_csrc("ocean_ripple_bed.h")
    assert "return ripple_bed_patch(b, x, y, texel).raw;" in bed and bed.count("floorf(u)") == 1
