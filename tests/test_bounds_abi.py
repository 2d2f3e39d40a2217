"""CPU tests of the surface bounds' interface (include/datum_ocean_hip.h: datum_ocean_reduce_bounds): the header declares the entry points,
states the definition and names the calls in its history, the library exports them, the binding has its methods, signatures and sizes, the
argument checks that need no device answer, and the bounded cast takes its heights from the several-cascade query's own text."""

import ctypes
import os
import re

import numpy as np

from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

BOUNDS_SYMBOLS = ("datum_ocean_reduce_bounds", "datum_ocean_bounds_device", "datum_ocean_read_bounds", "datum_ocean_surface_slab",
                  "datum_ocean_cast_rays_bounded", "datum_ocean_read_rays_bounded")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_bounds():
    from datum_amd import capi, host_api

    text = _header()
    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", text))
    lib = capi.load()
    for name in BOUNDS_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    # added without a version bump, and the header's history says so
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9
    history = text[text.index("Later added at 9 without a bump"):text.index("#define DATUM_OCEAN_ABI_VERSION")]
    assert all(name in history for name in BOUNDS_SYMBOLS)
    host = host_api.load()
    for method, symbol in (("reduce_ocean_bounds", "datum_host_reduce_ocean_bounds"), ("ocean_surface_slab", "datum_host_ocean_surface_slab"),
                           ("cast_ocean_rays_bounded", "datum_host_cast_ocean_rays_bounded")):
        assert callable(getattr(host_api.OceanContext, method)), method
        assert hasattr(host, symbol), symbol


def test_header_states_definition():
    text = _header()
    for line in ("0, 1   zmin, zmax     2, 3   xmin, xmax     4, 5   ymin, ymax     6   nonfinite     7   0",
                 "mag  = (|basez| + |A|) + Σ_c max(|zmin_c|, |zmax_c|)", "pad  = mag · 2^-16", "zhi  = ((basez + |A|) + Σ_c zmax_c) + pad",
                 "zlo  = ((basez − |A|) + Σ_c zmin_c) − pad", "reach.x = |gx| + Σ_c max(|xmin_c|, |xmax_c|)", "zlo = zhi = NaN",
                 "below'(t) = point(t).z > zhi ? false : point(t).z < zlo ? true : below(t)", "BIT FOR BIT", "forfeits that guarantee",
                 "#define DATUM_OCEAN_BOUNDS_RECORD_FLOATS 8"):
        assert line in text, line


def test_sizes_and_signatures():
    from datum_amd import capi

    I, P, S, Z = capi.I, capi.P, ctypes.POINTER(capi.OceanSet), ctypes.c_size_t
    L = ctypes.POINTER(I)
    assert capi.BOUNDS_RECORD_FLOATS == 8
    assert capi.SYMBOLS["datum_ocean_reduce_bounds"] == (I, [P])
    assert capi.SYMBOLS["datum_ocean_bounds_device"] == (I, [P, ctypes.POINTER(P), ctypes.POINTER(Z)])
    assert capi.SYMBOLS["datum_ocean_read_bounds"] == (I, [P, P])
    assert capi.SYMBOLS["datum_ocean_surface_slab"] == (I, [P, L, I, S, P, P, P, P])
    for name in ("datum_ocean_cast_rays_bounded", "datum_ocean_read_rays_bounded"):
        assert capi.SYMBOLS[name] == capi.SYMBOLS["datum_ocean_cast_rays"] == (I, [P, L, I, S, I, I, I, P, Z, P]), name
    for name in ("reduce_bounds", "bounds_device", "read_bounds", "surface_slab", "cast_rays_bounded", "read_rays_bounded"):
        assert callable(getattr(capi.Ocean, name)), name


def test_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    rays = np.zeros((4, 8), np.float32)
    out = np.zeros((4, 12), np.float32)
    rec = np.zeros((16, 8), np.float32)
    arr = (capi.I * 2)(0, 0)
    P = capi.P
    for name in ("datum_ocean_cast_rays_bounded", "datum_ocean_read_rays_bounded"):
        fn = getattr(lib, name)
        assert fn(None, arr, 2, ctypes.byref(s), 4, 32, 8, rays.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
        assert fn(None, None, 0, None, 4, 0, -1, None, 0, None) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
    p, n = P(), ctypes.c_size_t()
    slab = np.zeros(4, np.float32)
    sp = [P(slab.ctypes.data + 4 * k) for k in range(4)]
    for name, args in (("datum_ocean_reduce_bounds", (None,)), ("datum_ocean_bounds_device", (None, ctypes.byref(p), ctypes.byref(n))),
                       ("datum_ocean_read_bounds", (None, rec.ctypes.data_as(P))), ("datum_ocean_surface_slab", (None, arr, 2, ctypes.byref(s), *sp))):
        assert getattr(lib, name)(*args) == capi.EINVAL, name
        assert name.encode() in lib.datum_ocean_last_error(None)


def test_the_height_is_the_query_text():
    # the bounded kernel is the ray kernel's one body (ray_cast, ocean_ray.hip) around a search of its own: it states no height, record,
    # texel or load itself; the search is ocean_bounds.h's, which has no fmaf and leaves ray_search to ocean_ray.h
    from test_body_abi import assert_query_is_stated_once, read_csrc as read

    assert_query_is_stated_once()
    rays = read("ocean_bounds.hip").split("struct RayBoundedArgs")[1]
    assert rays.count("ray_cast<LAYOUT>(") == 1 and read("ocean_ray.hip").count("void ray_cast(") == 1
    for word in ("SurfaceTexel", "buf_load", "buf_store", "query_", "rmap", ".map"):
        assert word not in rays, word
    assert "amdgpu_waves_per_eu(8, 8)" in rays
    assert "ray_search_bounded(" in rays and "ray_search_bounded" not in read("ocean_ray.hip") + read("ocean_ray.h")
    assert "fmaf" not in read("ocean_bounds.h").replace("there is no fmaf here", "")
    assert "LAYOUT" not in read("ocean_bounds.hip").split("ocean_bounds_partial_kernel(BoundsArgs a)")[1].split("struct RayBoundedArgs")[0]
    assert '#include "ocean_bounds.hip"' in read("ocean_capi.hip")
