"""datum_amd/csrc/ocean_velocity.h walked on the CPU (tests/cpu/velocity_emul.cpp) against the numpy fp32 restatement of the
definition (tests/vel64.py: khat32, spectrum32), bit for bit; and that the kernels call the header's functions."""

import ctypes
import os

import numpy as np
import pytest

import pointwise as pw
import vel64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p


def _lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    lib.velocity_emul_walk.restype = None
    lib.velocity_emul_walk.argtypes = [ctypes.c_int, ctypes.c_float] + [P] * 9
    return lib


def _ptr(a):
    return a.ctypes.data_as(P)


@pytest.mark.parametrize("N,ws", [(64, 22.0), (128, 64.0), (256, 176.0)])
def test_header_walk_matches_the_restatement_bit_for_bit(oracle, N, ws):
    h0 = pw.lit_state(oracle, N, ws, 77 + N)
    rs = np.random.RandomState(N)
    phase = (rs.random_sample((N, N)) * 31.4 - 10.0).astype(np.float32)
    sn, cs = np.ascontiguousarray(np.sin(phase)), np.ascontiguousarray(np.cos(phase))
    om = vel64.omega32(N, ws)
    scale = np.float32(1) / np.float32(ws)
    out = [np.empty((N, N, 2), np.float32) for _ in range(3)] + [np.empty((N, N), np.float32) for _ in range(2)]
    _lib().velocity_emul_walk(N, scale, _ptr(h0), _ptr(sn), _ptr(cs), _ptr(om), *[_ptr(a) for a in out])
    knx, kny = vel64.khat32(N, scale)
    assert np.array_equal(out[3], knx) and np.array_equal(out[4], kny)
    for got, want in zip(out[:3], vel64.spectrum32(h0, sn, cs, om, knx, kny)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_kernels_call_the_header():
    src = open(os.path.join(ROOT, "datum_amd", "csrc", "ocean_velocity.hip"), encoding="utf-8").read()
    hdr = open(os.path.join(ROOT, "datum_amd", "csrc", "ocean_velocity.h"), encoding="utf-8").read()
    assert '#include "ocean_velocity.h"' in src
    # the kernel calls the three parts; velocity_spectrum, which the CPU walks, is those same parts and nothing else
    for call in ("velocity_ht(", "velocity_hk(", "velocity_khat("):
        assert call in src, call
    body = hdr[hdr.index("OV_HD VelocitySpectrum velocity_spectrum("):]
    assert body.count("velocity_ht(") == 1 and body.count("velocity_hk(") == 2 and "*" not in body.split("{", 1)[1].replace("&v", "")
    assert ".x * k" not in src and ".y * k" not in src          # no htx / hty formed beside the header
    assert "fmaf" not in hdr and "fma(" not in hdr
