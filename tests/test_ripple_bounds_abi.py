"""CPU tests of the ripple-layer bounds' interface (include/datum_ocean_hip.h: "ripple-layer bounds"): the header declares the entry points
and states the definition, the library exports them with their parents' signatures, the ABI stays 9, the argument check that needs no
device answers, and the kernels reach the arithmetic through ocean_ripple_bounds.h and restate nothing."""

import ctypes
import os
import re

import numpy as np

from test_body_abi import read_csrc
from test_rippled_abi import assert_ray_calls_are_stated_once
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

PARENTS = {"datum_ocean_reduce_ripple_bounds": "datum_ocean_reduce_bounds",
           "datum_ocean_ripple_bounds_device": "datum_ocean_bounds_device",
           "datum_ocean_read_ripple_bounds": "datum_ocean_read_bounds",
           "datum_ocean_surface_slab_rippled": "datum_ocean_surface_slab",
           "datum_ocean_cast_rays_rippled_bounded": "datum_ocean_cast_rays_rippled",
           "datum_ocean_read_rays_rippled_bounded": "datum_ocean_read_rays_rippled"}


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports():
    from datum_amd import capi

    text = _header()
    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", text))
    note = text.split("#define DATUM_OCEAN_ABI_VERSION")[0]
    lib = capi.load()
    args = lambda n: re.sub(r"\s+", " ", re.search(r"\bint " + n + r"\(([^;]*)\);", text).group(1))
    for name, parent in PARENTS.items():
        assert name in declared and name in note, name
        assert hasattr(lib, name), name
        assert capi.SYMBOLS[name] == capi.SYMBOLS[parent], name
        assert callable(getattr(capi.Ocean, name[len("datum_ocean_"):])), name
        # the declaration's argument list is the parent's, but for the name of the record
        mine = args(name) + ")"
        assert mine.replace("float *record)", "float *records)") == args(parent) + ")", name
    assert "#define DATUM_OCEAN_RIPPLE_BOUNDS_RECORD_FLOATS 8" in text and capi.RIPPLE_BOUNDS_RECORD_FLOATS == 8
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- ripple-layer bounds, the rippled slab and the bounded rippled cast (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("0, 1   etamin, etamax     2, 3   ratemin, ratemax     4   nonfinite     5   active     6, 7   0", "CURRENT state buffer",
                 "pending deposits are not seen", "a NaN enters no extremum, an infinity", "compare them by value", "η != 0 || rate != 0 (a NaN counts)",
                 "R² ≤ 2^20", "active == 0 is the test for a layer at rest", "elo  = fminf(etamin, 0)", "ehi = fmaxf(etamax, 0)",
                 "mag  = mag + fmaxf(|elo|, |ehi|)", "hi  = hi + ehi", "lo = lo + elo", "pad  = mag · 2^-16", "zhi = hi + pad", "zlo = lo − pad",
                 "strictly between zlo and zhi", "pad ≥ 128 ulp(mag)", "zlo = zhi = NaN", "datum_ocean_surface_slab keeps its results",
                 "below'(t) = point(t).z > zhi ? false : point(t).z < zlo ? true : below(t)", "marks it\n *                              CURRENT",
                 "datum_ocean_step_ripples", "datum_ocean_step_bodies_coupled and its host twin", "datum_ocean_center_ripples", "datum_ocean_reset_ripples",
                 "datum_ocean_set_ripples", "The deposit calls", "datum_ocean_set_ripple_params and every read leave it", "32 bytes, handle-owned",
                 "unless BOTH marks are current", "BIT FOR\n *                              BIT, all twelve floats of every ray",
                 "datum_ocean_ripples_device's pointer behind the module's back", "The layer is looked at first", "A refused call enqueues nothing",
                 "LEFT OUT", "a single-launch reduction", "bounds per tile of the window"):
        assert line in section, line
    rippled = text.split("/* -- rippled reads (added at ABI 9; nothing in the reference)")[1].split("/* -- ripple-layer bounds")[0]
    left = rippled.split("LEFT OUT:")[1]
    assert "bounded cast" not in left and "slab" not in left and "No longer left out" not in rippled


def test_argument_errors_without_gpu():
    """no handle: EINVAL with the call's name in the text, whatever else is said"""
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    arr = (capi.I * 2)(0, 0)
    buf = np.zeros(64, np.float32)
    ptr = buf.ctypes.data_as(capi.P)
    p, n = capi.P(), ctypes.c_size_t()
    calls = {"datum_ocean_reduce_ripple_bounds": (),
             "datum_ocean_ripple_bounds_device": (ctypes.byref(p), ctypes.byref(n)),
             "datum_ocean_read_ripple_bounds": (ptr,),
             "datum_ocean_surface_slab_rippled": (arr, 2, ctypes.byref(s), ptr, ptr, ptr, ptr),
             "datum_ocean_cast_rays_rippled_bounded": (arr, 2, ctypes.byref(s), 4, 8, 4, ptr, 1, ptr),
             "datum_ocean_read_rays_rippled_bounded": (arr, 2, ctypes.byref(s), 4, 8, 4, ptr, 1, ptr)}
    assert set(calls) == set(PARENTS)
    for name, args in calls.items():
        assert getattr(lib, name)(None, *args) == capi.EINVAL, name
        assert name.encode() in lib.datum_ocean_last_error(None), name
    assert np.all(buf == 0)


def test_the_kernels_call_the_header():
    kernel, header, host = read_csrc("ocean_ripple_bounds.hip"), read_csrc("ocean_ripple_bounds.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_ripple_bounds.h"' in kernel and '#include "ocean_bounds.h"' in header and '#include "ocean_rippled.h"' in header
    assert '#include "ocean_ripple_bounds.hip"' in host
    code = kernel.split("#pragma once")[1]
    assert "fmaf" not in header and "fmaf(" not in kernel and "asm" not in code and "atomic" not in code
    for fn in ("ripple_bounds_identity(", "ripple_bounds_cell(", "ripple_bounds_merge(", "ripple_bounds_slab("):
        assert fn in code, fn
        assert len(re.findall(r"OR_HD \w+ " + re.escape(fn), header)) == 1, fn
    assert len(re.findall(r"OR_HD void ripple_bounds_record\(", header)) == 1
    # nothing restated: the extrema, the search, the rippled height and the cast's loads and stores are called
    for copy in ("fminf(", "fmaxf(", "ray_mid(", "ray_sample(", "ripple_sample(", "ray_bad("):
        assert copy not in code, copy
    for text in ("ray_search_bounded(", "ray_cast_rippled<LAYOUT>(", "body_tree(wave)", "body_lane_up<S>("):
        assert text in code, text
    # bounds_slab keeps its text; the bounded search has one definition
    bounds = read_csrc("ocean_bounds.h")
    assert bounds.count("OR_HD BoundsSlab bounds_slab(") == 1 and bounds.count("ray_search_bounded(") == 1 and "ripple" not in bounds
    # the parents' checks are shared, not copied
    section = host.split("/* -- bounds of the ripple layer, the rippled slab and the bounded rippled cast (ocean_ripple_bounds.hip)")[1]
    # (the four calls that are the layer's own check it themselves; the two casts are the shared cast with both flags, checked in its order)
    assert section.count("check_ripples(ctx, ") == 4 and section.count("check_blend_list(") == 1 and "check_ray" not in section and "run_rays" not in section
    assert section.count("read_rays(ctx, ") == 1 and section.count("cast_rays(ctx, ") == 1 and section.count("ReadVariant{ true, true }") == 2
    assert_ray_calls_are_stated_once(host)
    # the mark: set in one place, cleared by the calls that write a state buffer
    assert host.count("ctx->rippleboundscurrent = true") == 1 and host.count("ctx->rippleboundscurrent = false") == 5
    emul = open(os.path.join(ROOT, "tests", "cpu", "ripple_bounds_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_ripple_bounds.h", "ripple_bounds_cell(", "ripple_bounds_merge(", "ripple_bounds_record(", "ripple_bounds_slab(", "ray_search_bounded(", "rippled_height(", "ripple_sample("):
        assert fn in emul, fn
    assert "tests/cpu/ripple_bounds_emul.cpp" in open(os.path.join(ROOT, "Makefile"), encoding="utf-8").read()


def test_shim_declarations_present():
    from datum_amd import host_api

    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    code = open(os.path.join(ROOT, "datum_amd", "host", "ocean.cpp"), encoding="utf-8").read()
    for name in ("struct OceanRippleBounds", "OceanRippleBounds reduce_ocean_ripple_bounds(OceanContext &context)",
                 "OceanSurfaceSlab ocean_surface_slab_rippled(OceanContext &context, OceanParams const &params)", "void cast_ocean_rays_rippled_bounded(OceanContext &context"):
        assert name in shim, name
    lib = host_api.load()
    for name in ("reduce_ocean_ripple_bounds", "ocean_surface_slab_rippled", "cast_ocean_rays_rippled_bounded"):
        assert hasattr(lib, "datum_host_" + name) and callable(getattr(host_api.OceanContext, name)), name
        # all three throw before prepare_ocean_context
        assert f'throw runtime_error("{name}: the context is not prepared (prepare_ocean_context)")' in code, name
