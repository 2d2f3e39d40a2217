"""CPU tests of the several-cascade calls' interface (include/datum_ocean_hip.h: datum_ocean_gen_blend): the header declares the entry
points and states the definition, the library exports them, the binding has its methods and signatures, and the argument checks that need
no device answer."""

import ctypes
import os
import re

import numpy as np

from test_surface_abi import _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")

BLEND_SYMBOLS = ("datum_ocean_gen_blend", "datum_ocean_sample_surface_blend", "datum_ocean_read_surface_blend")


def _header():
    return open(HEADER, encoding="utf-8").read()


def test_header_declares_and_library_exports_blend():
    from datum_amd import capi

    declared = set(re.findall(r"\b(datum_ocean_[a-z_]+)\s*\(", _header()))
    lib = capi.load()
    for name in BLEND_SYMBOLS:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    # added without a version bump
    assert capi.ABI_VERSION == capi.header_abi_version() == lib.datum_ocean_abi_version() == 9


def test_header_states_definition():
    text = _header()
    for line in ("t_c      = P.xy · scale_c", "p_c      = ( m_c.x / m_c.z,  m_c.y / m_c.z )", "p        = Σ p_c  in list order",
                 "dn       = normalize(p.x, p.y, 1)", "1 + Σ (J_c − 1)", "cross terms", "set->scale is ignored", "height\n * field"):
        assert line in text, line


def test_ctypes_signatures_and_methods():
    from datum_amd import capi

    I, P, S = capi.I, capi.P, ctypes.POINTER(capi.OceanSet)
    L = ctypes.POINTER(I)
    assert capi.SYMBOLS["datum_ocean_gen_blend"] == (I, [P, L, I, S, I, I, P])
    assert capi.SYMBOLS["datum_ocean_sample_surface_blend"] == (I, [P, L, I, S, I, P, ctypes.c_size_t, P])
    assert capi.SYMBOLS["datum_ocean_read_surface_blend"] == (I, [P, L, I, S, I, P, ctypes.c_size_t, P])
    for name in ("gen_blend", "sample_surface_blend", "read_surface_blend"):
        assert callable(getattr(capi.Ocean, name)), name


def test_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    s = _set()
    pts = np.zeros((4, 2), np.float32)
    out = np.zeros((4, 8), np.float32)
    arr = (capi.I * 2)(0, 0)
    P = capi.P
    for name in BLEND_SYMBOLS[1:]:
        fn = getattr(lib, name)
        assert fn(None, arr, 2, ctypes.byref(s), 4, pts.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
        assert fn(None, None, 0, None, 4, None, 0, None) == capi.EINVAL
        assert name.encode() in lib.datum_ocean_last_error(None)
    assert lib.datum_ocean_gen_blend(None, arr, 2, ctypes.byref(s), 4, 4, out.ctypes.data_as(P)) == capi.EINVAL
    assert b"datum_ocean_gen_blend" in lib.datum_ocean_last_error(None)


def test_the_shared_mesh_stages_are_stated_once():
    # the mesh kernels share their stages as text (ocean_gen_*.inc): both include every stage, neither keeps a copy of the ray stage, and
    # what tests/test_gen64.py pins for ocean_gen.hip holds for the included text as well -- the header's sin / cos, no copy of its constants
    csrc = os.path.join(ROOT, "datum_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name), encoding="utf-8").read()
    # (the blend kernels with the per-point query functions they include: ocean_query.hip holds the queries' frame)
    gen, blend = read("ocean_gen.hip"), read("ocean_query.hip") + read("ocean_blend.hip")
    for stage in ("tile", "ray", "texel", "frame", "store"):
        inc = f'#include "ocean_gen_{stage}.inc"'
        assert gen.count(inc) == 1 and blend.count(inc) == 1, stage
        text = read(f"ocean_gen_{stage}.inc")
        for copy in ("1.57079637050628662109375f", "4.37113900018624283e-8f", "0.636619772367581343f", "1.9515295891e-4f"):
            assert copy not in text, (stage, copy)
    assert read("ocean_gen_ray.inc").count("sincos_phase_pair_poly(theta, st[ph], ct[ph]);") == 1
    for once in ("div_exact(splat(f.cameraheight), costheta)", "__builtin_amdgcn_fractf(wx.x)"):
        assert once not in gen and once not in blend, once
    assert "make_gen_frame" in blend and "struct GenFrame" not in blend and "struct TexelIndex" not in blend
