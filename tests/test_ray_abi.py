"""CPU tests of the ray casts' interface (include/datum_ocean_hip.h: datum_ocean_cast_rays): the header declares the entry points, states
the definition and names the calls in its history, the library exports them, the binding has its methods, signatures and sizes, the
argument checks that need no device answer, and the search's height comes from the several-cascade query's own text."""

import ctypes
import os
import re

import numpy as np

import ray64
from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

RAY_SYMBOLS = ("datum_ocean_cast_rays", "datum_ocean_read_rays")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_rays():
    from datum_amd import capi, host_api

    text = _header()
    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", text))
    lib = capi.load()
    for name in RAY_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    # added without a version bump, and the header's history says so
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    history = text[text.index("Later added at 9 without a bump"):text.index("#define DATUM_OCEAN_ABI_VERSION")]
    assert all(name in history for name in RAY_SYMBOLS)
    assert callable(host_api.OceanContext.cast_ocean_rays)
    assert hasattr(host_api.load(), "datum_host_cast_ocean_rays")


def test_header_states_definition():
    text = _header()
    for line in ("point(t) = ( ox + t·dx,  oy + t·dy,  oz + t·dz )", "g(t)     = point(t).z − rec(t).z", "below(t) = g(t) < 0",
                 "inv      = 1.0f / (float)S", "Δ        = (tmax − tmin) · inv", "t_i      = tmin + (float)i · Δ", "t_S = tmax",
                 "mid = 0.5f · (lo + hi)", "lo = hi = tmax", "twelve\n * quiet NaNs", "#define DATUM_OCEAN_RAY_RECORD_FLOATS 12",
                 "#define DATUM_OCEAN_RAY_MAX_STEPS 1024", "#define DATUM_OCEAN_RAY_MAX_REFINE 24"):
        assert line in text, line


def test_sizes_and_signatures():
    from datum_amd import capi

    emul = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    emul.ray_sizeof.restype = ctypes.c_size_t
    assert emul.ray_sizeof() == 4 * capi.RAY_FLOATS == 4 * ray64.RAY_FLOATS == 32
    assert emul.ray_record_floats() == capi.RAY_RECORD_FLOATS == ray64.RECORD_FLOATS == 12
    assert (capi.RAY_MAX_STEPS, capi.RAY_MAX_REFINE) == (1024, 24)
    assert (capi.RAY_MISS, capi.RAY_ENTER, capi.RAY_LEAVE) == (ray64.MISS, ray64.ENTER, ray64.LEAVE) == (0, 1, 2)

    I, P, S, Z = capi.I, capi.P, ctypes.POINTER(capi.OceanSet), ctypes.c_size_t
    L = ctypes.POINTER(I)
    for name in RAY_SYMBOLS:
        assert capi.SYMBOLS[name] == (I, [P, L, I, S, I, I, I, P, Z, P]), name
    for name in ("cast_rays", "read_rays"):
        assert callable(getattr(capi.Ocean, name)), name


def test_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    rays = np.zeros((4, 8), np.float32)
    out = np.zeros((4, 12), np.float32)
    arr = (capi.I * 2)(0, 0)
    P = capi.P
    for name in RAY_SYMBOLS:
        fn = getattr(lib, name)
        assert fn(None, arr, 2, ctypes.byref(s), 4, 32, 8, rays.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
        assert fn(None, None, 0, None, 4, 0, -1, None, 0, None) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)


def test_the_height_is_the_query_text():
    # the search's height and the record at hi: the several-cascade query's functions, each called once by the one ray-cast body; the
    # kernel loads its rays and nothing of a map
    from test_body_abi import assert_query_is_stated_once, read_csrc as read

    assert_query_is_stated_once()
    ray = read("ocean_ray.hip")
    assert ray.count("query_height<LAYOUT>(") == 1 and ray.count("query_record<LAYOUT>(") == 1 and ray.count("query_solve<LAYOUT>(") == 2
    assert "SurfaceTexel" not in ray and "rmap" not in ray and ".map" not in ray
    assert re.findall(r"buf_load\w*(?:<\d+>)?\((\w+)", ray) == ["rrays", "rrays"]
    assert ray.count("void ray_cast(") == 1 and ray.count("ray_cast<LAYOUT>(") == 1 and "ray_search(ray," in ray
    assert "fmaf" not in read("ocean_ray.h").replace("there is no fmaf here", "")
    assert '#include "ocean_ray.hip"' in read("ocean_capi.hip")
