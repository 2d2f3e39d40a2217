"""CPU tests of the surface velocity's interface: the header declares the entry points and states the definition, the library exports
them, the binding matches, the record size, and every argument check that needs no device."""

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

VELOCITY_SYMBOLS = (
    "datum_ocean_set_velocity",
    "datum_ocean_bind_velocity",
    "datum_ocean_velocity_device",
    "datum_ocean_read_velocity",
    "datum_ocean_sample_velocity_blend",
    "datum_ocean_read_velocity_blend",
)


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_velocity():
    from datum_amd import capi

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    for name in VELOCITY_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name


def test_abi_version_stays_9_and_the_note_names_the_calls():
    from datum_amd import capi

    assert capi.ABI_VERSION == capi.header_abi_version() == capi.load().datum_ocean_abi_version() == 9
    note = _header().split("#define DATUM_OCEAN_ABI_VERSION")[0]
    for name in VELOCITY_SYMBOLS:
        assert name in note, name


def test_header_states_definition_modes_and_sizes():
    from datum_amd import capi

    text = _header()
    assert "ht.re = omega · ( −(a.x + m.x) sin phase − (a.y + m.y) cos phase )" in text
    assert "ht.im = omega · (  (a.x − m.x) cos phase − (a.y − m.y) sin phase )" in text
    assert "THE SWELL IS NOT INCLUDED" in text
    modes = {k: int(v) for k, v in re.findall(r"#define\s+DATUM_OCEAN_VELOCITY_(OFF|ON)\s+(\d+)", text)}
    assert modes == {"OFF": capi.VELOCITY_MODES["off"], "ON": capi.VELOCITY_MODES["on"]} == {"OFF": 0, "ON": 1}
    floats = int(re.search(r"#define\s+DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS\s+(\d+)", text).group(1))
    assert floats == capi.VELOCITY_SAMPLE_FLOATS == capi.SURFACE_SAMPLE_FLOATS == 8
    assert ctypes.sizeof(capi.OceanSet) == 216


def test_velocity_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    p, n = capi.P(), ctypes.c_size_t()
    out = np.zeros(16, np.float32)
    pts = np.zeros(2, np.float32)
    lst = (ctypes.c_int * 1)(0)
    s = capi.OceanSet()
    assert lib.datum_ocean_set_velocity(None, 1) == capi.EINVAL
    assert b"datum_ocean_set_velocity" in lib.datum_ocean_last_error(None)
    assert lib.datum_ocean_bind_velocity(None, None, 0) == capi.EINVAL
    assert b"datum_ocean_bind_velocity" in lib.datum_ocean_last_error(None)
    assert lib.datum_ocean_velocity_device(None, ctypes.byref(p), ctypes.byref(n)) == capi.EINVAL
    assert lib.datum_ocean_read_velocity(None, 0, out.ctypes.data_as(capi.P)) == capi.EINVAL
    assert b"datum_ocean_read_velocity" in lib.datum_ocean_last_error(None)
    assert lib.datum_ocean_sample_velocity_blend(None, lst, 1, ctypes.byref(s), 0, None, 0, None) == capi.EINVAL
    assert b"datum_ocean_sample_velocity_blend" in lib.datum_ocean_last_error(None)
    assert lib.datum_ocean_read_velocity_blend(None, lst, 1, ctypes.byref(s), 0, pts.ctypes.data_as(capi.P), 1, out.ctypes.data_as(capi.P)) == capi.EINVAL
    assert b"datum_ocean_read_velocity_blend" in lib.datum_ocean_last_error(None)


def test_ocean_binding_has_velocity_methods():
    from datum_amd import capi, host_api

    for name in ("set_velocity", "bind_velocity", "velocity_device", "read_velocity", "sample_velocity_blend", "read_velocity_blend"):
        assert callable(getattr(capi.Ocean, name)), name
    for name in ("set_velocity", "read_velocity", "query_ocean_velocity"):
        assert callable(getattr(host_api.OceanContext, name)), name
    lib = host_api.load()
    for name in ("datum_host_set_ocean_velocity", "datum_host_read_ocean_velocity", "datum_host_query_ocean_velocity"):
        assert hasattr(lib, name), name
    shim = open(os.path.join(ROOT, "datum_amd", "host", "ocean.h"), encoding="utf-8").read()
    for name in ("set_ocean_velocity", "read_ocean_velocity", "query_ocean_velocity", "sizeof(OceanVelocitySample) == 32"):
        assert name in shim, name


def test_the_blend_point_text_is_guarded():
    # the velocity query is the several-cascade query's prologue and solve with a final evaluation of its own beside the record's and the
    # height's, each a function defined once; the query kernel states no texel and no load itself
    from test_body_abi import assert_query_is_stated_once, read_csrc as read

    assert_query_is_stated_once()
    kernel = read("ocean_velocity.hip").split("struct VelocityBlendArgs")[1]
    assert kernel.count("query_velocity<LAYOUT>(") == 1 and kernel.count("query_solve<LAYOUT>(") == 1 and kernel.count("query_each_point(") == 1
    for word in ("SurfaceTexel", "buf_load", "rmap", ".map"):
        assert word not in kernel, word
