"""CPU tests of the rippled reads' interface (include/datum_ocean_hip.h: "rippled reads"): the header declares the entry points and states
the definition, the library exports them with their parents' signatures, the ABI stays 9, the argument check that needs no device answers,
and the kernels reach what is new through ocean_rippled.h and restate nothing."""

import ctypes
import os
import re

import numpy as np

from test_body_abi import read_csrc
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

PARENTS = {"datum_ocean_gen_blend_rippled": "datum_ocean_gen_blend",
           "datum_ocean_sample_surface_blend_rippled": "datum_ocean_sample_surface_blend",
           "datum_ocean_read_surface_blend_rippled": "datum_ocean_read_surface_blend",
           "datum_ocean_cast_rays_rippled": "datum_ocean_cast_rays",
           "datum_ocean_read_rays_rippled": "datum_ocean_read_rays"}


def _header():
    return open(HEADER, encoding="utf-8").read()


def entry_points(text):
    """the C entry points defined in a stretch of ocean_capi.hip: {name: body}, in the text's order"""
    return dict(re.findall(r"^int (datum_ocean_\w+)\([^{;]*\)\n\{\n(.*?)^\}\n", text, re.S | re.M))


RAY_VARIANTS = {"": "false, false", "_bounded": "false, true", "_rippled": "true, false", "_rippled_bounded": "true, true"}


def assert_ray_calls_are_stated_once(host):
    """ocean_capi.hip: the eight casts build the query, the call and the variant and name one shared function once; that function's check
    and run are defined once; no entry point refuses, copies or launches by itself"""
    entries = entry_points(host)
    for suffix, flags in RAY_VARIANTS.items():
        for shared in ("cast_rays", "read_rays"):
            name = "datum_ocean_" + shared + suffix
            body = entries[name]
            assert re.findall(r"\b(\w+)\(ctx, ", body) == [shared], name
            assert '%s(ctx, q, call, ReadVariant{ %s }, "%s");' % (shared, flags, name) in body, name
            assert "Query const q = { cascades, count, set, iterations };" in body and "RayCall const call = { steps, refine, rays" in body, name
            for word in ("fail(", "hipMemcpy", "hipSetDevice", "check_", "launch_"):
                assert word not in body, (name, word)
    for fn in ("int check_rays(", "int run_rays(", "int cast_rays(", "int read_rays(", "RayBatch ray_batch(", "void list_cascades("):
        assert host.count(fn) == 1, fn
    assert host.count("check_rays(ctx, q, call, v, name)") == 2 and host.count("run_rays(ctx, q, ") == 2 and host.count("list_cascades(q, ") == 2
    # the refusals in their order: the layer, the query, the cast's own, the maps' mark, the layer's mark
    check = host.split("int check_rays(")[1].split("RayBatch ray_batch(")[0]
    order = ["v.rippled ? check_ripples(ctx, name)", "check_query(ctx, q, name)", "steps outside", "refine outside", "null rays or records", "16-byte aligned", "n above INT32_MAX",
             "v.bounded && !ctx->boundscurrent", "v.bounded && v.rippled && !ctx->rippleboundscurrent"]
    assert [check.count(text) for text in order] == [1] * len(order) and sorted(order, key=check.index) == order
    assert host.count("!ctx->boundscurrent") == 1 and host.count("!ctx->rippleboundscurrent") == 1
    for gone in ("check_ray_args(", "check_ray_bounded_args(", "check_ray_rippled_bounded_args(", "run_rays_bounded(", "run_rays_rippled(", "run_rays_rippled_bounded("):
        assert gone not in host, gone


def test_header_declares_and_library_exports():
    from datum_amd import capi

    text = _header()
    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", text))
    note = text.split("#define DATUM_OCEAN_ABI_VERSION")[0]
    lib = capi.load()
    for name, parent in PARENTS.items():
        assert name in declared and name in note, name
        assert hasattr(lib, name), name
        assert capi.SYMBOLS[name] == capi.SYMBOLS[parent], name
        assert callable(getattr(capi.Ocean, name[len("datum_ocean_"):])), name
        # the declaration's argument list is the parent's, word for word
        args = lambda n: re.sub(r"\s+", " ", re.search(r"\bint " + n + r"\(([^;]*)\);", text).group(1))
        assert args(name) == args(parent), name
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9


def test_header_states_definition():
    text = _header()
    section = text.split("/* -- rippled reads (added at ABI 9; nothing in the reference)")[1].split("/* -- the tile farm")[0]
    for line in ("rec'[2] = rec[2] + s.η", "fields 0, 1, 3 and 7 are rec's bits", "p' = (p.x + (−0.5f · s.∂xη), p.y + (−0.5f · s.∂yη))",
                 "dn = normalize(p'.x, p'.y, 1)", "m.x / m.z = −½ ∂z/∂x", "the ASKED point", "the layer displaces nothing horizontally",
                 "eight quiet NaNs", "THE RIPPLED HEIGHT", "one fp32 addition", "(px, py) = position.xy − displacement.xy", "pz' = pz + s.η",
                 "Unshaded waves keep the plane normal", "THE RIPPLED CAST", "g taken from its field 2", "CURRENT state buffer",
                 "writes nothing into the layer", "pending deposits are not seen", "cells outside the window read 0", "The layer is looked at first",
                 "n == 0", "A refused call enqueues nothing", "LEFT OUT", "the bounded cast", "datum_ocean_sample_velocity_blend",
                 "foam from the layer", "anything on the displace path"):
        assert line in section, line
    ripples = text.split("/* -- ripple layer (added at ABI 9; nothing in the reference)")[1].split("/* -- coupled stepping")[0]
    assert "the one call that" in ripples and "rippled reads" in ripples
    coupled = text.split("/* -- coupled stepping (added at ABI 9; nothing in the reference)")[1].split("/* -- rippled reads")[0]
    assert "LEFT OUT" in coupled and "the layer in the surface queries, gen_blend and the ray casts" not in coupled


def test_argument_errors_without_gpu():
    """no handle: EINVAL with the call's name in the text, whatever else is said"""
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    arr = (capi.I * 2)(0, 0)
    buf = np.zeros(64, np.float32)
    ptr = buf.ctypes.data_as(capi.P)
    calls = {"datum_ocean_gen_blend_rippled": (arr, 2, ctypes.byref(s), 4, 4, ptr),
             "datum_ocean_sample_surface_blend_rippled": (arr, 2, ctypes.byref(s), 4, ptr, 2, ptr),
             "datum_ocean_read_surface_blend_rippled": (arr, 2, ctypes.byref(s), 4, ptr, 2, ptr),
             "datum_ocean_cast_rays_rippled": (arr, 2, ctypes.byref(s), 4, 8, 4, ptr, 1, ptr),
             "datum_ocean_read_rays_rippled": (arr, 2, ctypes.byref(s), 4, 8, 4, ptr, 1, ptr)}
    for name, args in calls.items():
        assert getattr(lib, name)(None, *args) == capi.EINVAL, name
        assert name.encode() in lib.datum_ocean_last_error(None), name
    assert np.all(buf == 0)


def test_the_kernels_call_the_headers():
    kernel, header, host = read_csrc("ocean_rippled.hip"), read_csrc("ocean_rippled.h"), read_csrc("ocean_capi.hip")
    assert '#include "ocean_rippled.h"' in kernel and '#include "ocean_ripple.h"' in header
    assert "fmaf" not in header and "fmaf(" not in kernel and "asm" not in kernel and "atomic" not in kernel.split("#pragma once")[1]
    for fn in ("rippled_height(", "rippled_slope("):
        assert fn in kernel, fn
        assert len(re.findall(r"OB_HD \w+ " + re.escape(fn), header)) == 1, fn
    # nothing restated: the sample, the query's loop, the march and the mesh stages are called or included
    for copy in ("floorf(", "sqrtf(", "SurfaceTexel", "rcpf(", "ray_mid(", "-0.5f", "fmaxf("):
        assert copy not in kernel, copy
    for text in ("ripple_sample(", "query_sums<LAYOUT>(", "query_finish(", "query_height<LAYOUT>(", "ray_search(", '"ocean_gen_cascades.inc"', '"ocean_gen_texel.inc"',
                 '"ocean_gen_tile.inc"', '"ocean_gen_ray.inc"', '"ocean_gen_frame.inc"', '"ocean_gen_store.inc"'):
        assert text in kernel, text
    assert set(re.findall(r"buf_load\w*(?:<\d+>)?\((r\w+),", kernel)) == {"rstate", "rrays"}
    # query_record's sums stand once, and the parents are that one loop
    query = read_csrc("ocean_query.hip")
    assert query.count("sx = fmaf(nx, rz, sx);") == 1 and "return query_finish(a, b, q, query_sums<LAYOUT>(a, b));" in query
    assert read_csrc("ocean_blend.hip").count('#include "ocean_gen_cascades.inc"') == 1
    # the parents' checks are shared, not copied: each call here is its parent's one function with the layer on top, and that function
    # is defined once, the layer's check ahead of the parent's own
    section = host.split("/* -- rippled reads:")[1].split("// a cascade's maps as the reference's")[0]
    assert "fail(" not in section and "hipMemcpy" not in section and "check_" not in section and "launch_" not in section
    entries = entry_points(section)
    assert list(entries) == ["datum_ocean_gen_blend_rippled", "datum_ocean_sample_surface_blend_rippled", "datum_ocean_read_surface_blend_rippled",
                             "datum_ocean_cast_rays_rippled", "datum_ocean_read_rays_rippled"]
    for name, body in entries.items():
        parent = name[len("datum_ocean_"):-len("_rippled")]
        assert re.findall(r"\b(\w+)\(ctx, ", body) == [parent], name
        assert ('ReadVariant{ true, false }, "%s");' % name if "rays" in name else 'true, "%s");' % name) in body, name
    for fn in ("int gen_blend(", "int check_surface_read(", "int run_surface_blend(", "int sample_surface_blend(", "int read_surface_blend("):
        assert host.count(fn) == 1, fn
    assert host.count("int rc = rippled ? check_ripples(ctx, name) : DATUM_OCEAN_OK;") == 2 and host.count("check_gen_blend_args(ctx, ") == 1 and host.count("check_surface_read(ctx, ") == 2
    assert_ray_calls_are_stated_once(host)
    emul = open(os.path.join(ROOT, "tests", "cpu", "rippled_emul.cpp"), encoding="utf-8").read()
    for fn in ("ocean_rippled.h", "ocean_ray.h", "rippled_height(", "rippled_slope(", "ripple_sample(", "ray_search("):
        assert fn in emul, fn


def test_shim_declarations_present():
    from datum_amd import host_api

    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    code = open(os.path.join(ROOT, "datum_amd", "host", "ocean.cpp"), encoding="utf-8").read()
    for name in ("void query_ocean_surface_rippled(OceanContext &context", "void cast_ocean_rays_rippled(OceanContext &context", "void gen_ocean_surface_rippled(OceanContext &context, Ocean const *target, Camera const &camera, OceanParams const &params)"):
        assert name in shim, name
    lib = host_api.load()
    for name in ("query_ocean_surface_rippled", "cast_ocean_rays_rippled", "gen_ocean_surface_rippled"):
        assert hasattr(lib, "datum_host_" + name) and callable(getattr(host_api.OceanContext, name)), name
        # all three throw before prepare_ocean_context
        assert f'throw runtime_error("{name}: the context is not prepared (prepare_ocean_context)")' in code, name
