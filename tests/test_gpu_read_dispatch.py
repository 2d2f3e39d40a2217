"""The reads of the summed surface as the C ABI dispatches them (ocean_capi.hip): the eight ray casts -- cast_rays / read_rays, plain, _bounded,
_rippled, _rippled_bounded -- and the four blended point reads, interleaved on one handle with ray counts on either side of one 256-thread
workgroup and the empty call, return what the same calls return one at a time on a fresh handle, bit for bit, and every device call returns
what its host twin returns.  Once in the PLAIN map layout and once at the smallest resolution gen_layout makes BANDED.  Then the order of
the refusals per variant: the layer, the cast's own arguments, the maps' bounds, the layer's bounds, each under the call's own name."""

import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
ITERATIONS, STEPS, REFINE = 4, 16, 4
COUNTS = (1, 255, 257, 0)
R, CELL, DT = 64, 0.5, F(1 / 60)
IMPULSE = (1.0, 2.0, 0.05, 0.0)
LEVEL = 0.3
SIZES = (64, 128, 256, 512, 1024, 2048, 4096)
VARIANTS = ("", "_bounded", "_rippled", "_rippled_bounded")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _set(capi):
    s = capi.OceanSet()
    s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, 0.8, 0.5, 1.1
    s.swelldirection[:] = (0.780869, 0.624695)
    s.plane[:] = (0.0, 0.0, 1.0, -LEVEL)
    s.scale = F(1.0)
    return s


def _points(rs, n):
    """inside and outside the layer's window; the first is the impulse's cell"""
    p = rs.uniform(-24, 24, (n, 2)).astype(F)
    p[:1] = IMPULSE[:2]
    return p


def _rays(rs, n):
    """up-going rays from below and down-going from above; the first falls straight onto the impulse's cell"""
    r = np.empty((n, 8), F)
    el = np.radians(rs.uniform(2, 90, n)) * rs.choice([-1, 1], n)
    az = rs.uniform(0, 2 * np.pi, n)
    r[:, 0:2] = rs.uniform(-24, 24, (n, 2))
    r[:, 2] = LEVEL - np.sign(el) * rs.uniform(0.5, 4.0, n)
    r[:, 4], r[:, 5], r[:, 6] = np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)
    r[:, 3] = 0.0
    r[:, 7] = rs.uniform(4.0, 8.0, n) / np.abs(np.sin(el))
    r[:1] = (IMPULSE[0], IMPULSE[1], LEVEL + 3.0, 0.0, 0.0, 0.0, -1.0, 8.0)
    return r


def _banded_size():
    """the smallest resolution for which ocean_layout.h's gen_layout gives GEN_BANDED (1), read from the header through the CPU walk"""
    emul = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    for N in SIZES:
        a, b = np.empty((N, N), np.int64), np.empty((N, N), np.int64)
        layout = ctypes.c_int(-1)
        assert emul.layout_map_shifts(N, a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), ctypes.byref(layout)) == 0
        if layout.value == 1:
            return N
        assert layout.value == 0, N
    raise AssertionError("no BANDED resolution")


def _ocean(capi, N, scales):
    """one displace, the layer on with one impulse taken in by one step, both bounds current: every handle made here holds the same state"""
    oc = capi.Ocean(N, len(scales))
    rs = np.random.RandomState(5)
    for c, ws in enumerate(scales):
        oc.set_cascade(c, ws, 1.0)
        oc.upload_state(c, (rs.standard_normal((N, N, 2)) * (0.4 / N)).astype(F))
    oc.set_foam("accumulate")
    oc.update(DT)
    oc.displace()
    oc.set_ripples(R, CELL)
    oc.deposit_ripples_host([IMPULSE])
    oc.step_ripples(DT, 1)
    oc.reduce_bounds()
    oc.reduce_ripple_bounds()
    return oc


def _calls(oc, s, cascades):
    """the twelve calls on `oc`, each a function of (points, rays) that returns the call's records as a host array"""
    import torch

    def device(host, floats, launch):
        """a device-array call: `host` as a torch tensor, `floats` floats of result per row"""
        src = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(-1)).cuda()
        out = torch.zeros(len(host) * floats, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        launch(src.data_ptr() if len(host) else 0, len(host), out.data_ptr() if len(host) else 0)
        oc.sync()
        return out.cpu().numpy().reshape(len(host), floats)

    calls = {}
    for v in VARIANTS:
        cast, read = getattr(oc, "cast_rays" + v), getattr(oc, "read_rays" + v)
        calls["cast_rays" + v] = lambda pts, rays, cast=cast: device(rays, 12, lambda r, n, o: cast(cascades, s, r, n, o, ITERATIONS, STEPS, REFINE))
        calls["read_rays" + v] = lambda pts, rays, read=read: read(cascades, s, rays, ITERATIONS, STEPS, REFINE)
    for v in ("", "_rippled"):
        sample, read = getattr(oc, "sample_surface_blend" + v), getattr(oc, "read_surface_blend" + v)
        calls["sample_surface_blend" + v] = lambda pts, rays, sample=sample: device(pts, 8, lambda p, n, o: sample(cascades, s, p, n, o, ITERATIONS))
        calls["read_surface_blend" + v] = lambda pts, rays, read=read: read(cascades, s, pts, ITERATIONS)
    return calls


@pytest.mark.parametrize("layout", ["plain", "banded"])
def test_reads_interleaved_are_a_fresh_handles_bits_and_their_twins(layout):
    from datum_amd import capi

    capi.load()
    N, scales, cascades = (64, (22.0, 64.0, 150.0), [2, 0]) if layout == "plain" else (_banded_size(), (64.0,), [0])
    s = _set(capi)
    rs = np.random.RandomState(13)
    inputs = {n: (_points(rs, n), _rays(rs, n)) for n in COUNTS}

    with _ocean(capi, N, scales) as oc:
        calls = _calls(oc, s, cascades)
        got = {(name, n): call(*inputs[n]) for n in COUNTS for name, call in calls.items()}                  # interleaved
    with _ocean(capi, N, scales) as fresh:
        want = {(name, n): call(*inputs[n]) for name, call in _calls(fresh, s, cascades).items() for n in COUNTS}      # one at a time

    assert set(got) == set(want) and len(got) == 12 * len(COUNTS)
    for (name, n), w in want.items():
        g = got[name, n]
        assert g.shape == w.shape == (n, 12 if "rays" in name else 8), (name, n)
        assert np.array_equal(_bits(g), _bits(w)), (name, n)
        # (answers, not the NaNs of refused input, which would compare equal as well)
        assert np.isfinite(g[:, 3] if "rays" in name else g).all(), (name, n)
    for n in COUNTS:
        for v in VARIANTS:
            assert np.array_equal(_bits(got["cast_rays" + v, n]), _bits(got["read_rays" + v, n])), (v, n)
        for v in ("", "_rippled"):
            assert np.array_equal(_bits(got["sample_surface_blend" + v, n]), _bits(got["read_surface_blend" + v, n])), (v, n)
        # the bounded casts are their parents' records (include/datum_ocean_hip.h: BIT FOR BIT)
        assert np.array_equal(_bits(got["read_rays_bounded", n]), _bits(got["read_rays", n])), n
        assert np.array_equal(_bits(got["read_rays_rippled_bounded", n]), _bits(got["read_rays_rippled", n])), n
        # the layer is on top where the call says so: the impulse's cell stands at another height
        if n > 0:
            assert got["read_surface_blend_rippled", n][0, 2] != got["read_surface_blend", n][0, 2], n
            assert got["read_rays_rippled", n][0, 6] != got["read_rays", n][0, 6], n          # (the record's height at hi, above the same x, y)


def test_refusals_keep_their_order_per_variant():
    """every call here returns before any launch: it is refused, or its n is 0"""
    from datum_amd import capi

    lib = capi.load()
    s = _set(capi)
    arr = (capi.I * 1)(0)

    with capi.Ocean(64, 1) as oc:
        oc.set_cascade(0, 22.0, 1.0)
        oc.upload_state(0, (np.random.RandomState(5).standard_normal((64, 64, 2)) * (0.4 / 64)).astype(F))
        oc.update(DT)
        oc.displace()

        def rays(name, steps):
            return getattr(lib, "datum_ocean_" + name)(oc.h, arr, 1, ctypes.byref(s), ITERATIONS, steps, REFINE, None, 0, None)

        def refused(rc, code, name, text):
            message = lib.datum_ocean_last_error(oc.h).decode()
            assert rc == code and ("datum_ocean_" + name + ":") in message and text in message, (name, rc, message)

        # the layer is off: ESTATE from the rippled variants ahead of a bad steps' EINVAL, and the others go on to theirs
        for call in ("cast_rays", "read_rays"):
            for v in ("_rippled", "_rippled_bounded"):
                refused(rays(call + v, 0), capi.ESTATE, call + v, "")
            refused(rays(call, 0), capi.EINVAL, call, "steps outside")
            assert rays(call, STEPS) == 0
        for call in ("sample_surface_blend_rippled", "read_surface_blend_rippled"):
            rc = getattr(lib, "datum_ocean_" + call)(oc.h, arr, 1, ctypes.byref(s), 99, None, 0, None)
            refused(rc, capi.ESTATE, call, "")
        for call in ("sample_surface_blend", "read_surface_blend"):
            rc = getattr(lib, "datum_ocean_" + call)(oc.h, arr, 1, ctypes.byref(s), 99, None, 0, None)
            refused(rc, capi.EINVAL, call, "iterations outside")
        refused(lib.datum_ocean_gen_blend_rippled(oc.h, arr, 1, ctypes.byref(s), 1, 1, None), capi.ESTATE, "gen_blend_rippled", "")
        refused(lib.datum_ocean_gen_blend(oc.h, arr, 1, ctypes.byref(s), 1, 1, None), capi.EINVAL, "gen_blend", "null argument")

        # no bounds yet: a bad steps' EINVAL ahead of the stale bounds' ESTATE
        for call in ("cast_rays_bounded", "read_rays_bounded"):
            refused(rays(call, 0), capi.EINVAL, call, "steps outside")
            refused(rays(call, STEPS), capi.ESTATE, call, "the bounds are not current")

        # the layer on, neither bounds current: the cast's own arguments, then the maps' bounds, then the layer's
        oc.set_ripples(R, CELL)
        for call in ("cast_rays_rippled_bounded", "read_rays_rippled_bounded"):
            refused(rays(call, 0), capi.EINVAL, call, "steps outside")
            refused(rays(call, STEPS), capi.ESTATE, call, "the bounds are not current")
        for call in ("cast_rays_rippled", "read_rays_rippled"):
            refused(rays(call, 0), capi.EINVAL, call, "steps outside")
            assert rays(call, STEPS) == 0
        oc.reduce_ripple_bounds()
        for call in ("cast_rays_rippled_bounded", "read_rays_rippled_bounded"):
            refused(rays(call, STEPS), capi.ESTATE, call, "the bounds are not current")
        oc.reduce_bounds()
        oc.step_ripples(DT, 1)
        for call in ("cast_rays_rippled_bounded", "read_rays_rippled_bounded"):
            refused(rays(call, 0), capi.EINVAL, call, "steps outside")
            refused(rays(call, STEPS), capi.ESTATE, call, "the ripple bounds are not current")
        for call in ("cast_rays_bounded", "read_rays_bounded"):
            assert rays(call, STEPS) == 0
        oc.reduce_ripple_bounds()
        for call in ("cast_rays_rippled_bounded", "read_rays_rippled_bounded"):
            assert rays(call, STEPS) == 0
