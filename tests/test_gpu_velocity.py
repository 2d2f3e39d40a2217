"""The surface velocity on the device (datum_ocean_set_velocity; ocean_velocity.hip), against tests/vel64.py.

  * pointwise           every texel of read_velocity within K_VEL eps log2 N (relative to the channel's RMS, pointwise.pointwise's units)
                        of vel64, at every N that instantiates a kernel form; after a negative dt and from uploaded phases outside
                        [0, 2 pi); with one cascade per launch; single bins against the closed form (vel64.single_bin64); the flat ocean
  * nothing else moves  two handles in lockstep, velocity on and off: maps, foam and phase bit for bit, in every spectrum format, the literal
                        mode and at write-back intervals 1 and 8; the plane bit for bit between the two intervals
  * queries             fields 0-3 are read_surface_blend's bits, fields 4-6 the fp32 restatement over the read_velocity planes, bit for bit
K_VEL comes from CPU arithmetic (tests/vel64.py, tests/test_vel64.py).  Each case prints its measured K beside the bar."""

import ctypes

import numpy as np
import pytest

import pointwise as pw
import vel64

pytestmark = pytest.mark.gpu

F = np.float32
DT = pw.DT
SCALES = (22.0, 64.0, 176.0)


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _channels(plane):
    assert np.all(plane[..., 3] == 0), ".w"
    assert np.isfinite(plane).all()
    return np.moveaxis(plane[..., :3], -1, 0).astype(np.float64)


def _check(report, label, plane, h0, phase, ws, chop, N):
    ref = vel64.vel64(h0, phase, F(1) / F(ws), chop, vel64.omega32(N, ws))
    k = vel64.k_of(_channels(plane), ref, N)
    line = f"velocity pointwise {label}: K {k:.3g} (bar {vel64.K_VEL:.3g})"
    print(line)
    report(line)
    assert k <= vel64.K_VEL, (label, k)


def _set(capi, N, scale):
    s = capi.OceanSet()
    s.plane[2], s.plane[3] = 1.0, 0.5
    s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 10.0, 0.0, 0.0, 0.3
    s.swelldirection[0], s.swelldirection[1] = 0.6, 0.8
    s.scale = float(scale)
    s.size = N
    return s


# 1 -- pointwise

@pytest.mark.parametrize("N,C", [(64, 3), (128, 1), (256, 1), (512, 1), (1024, 2), (2048, 1), (4096, 1)])
def test_every_kernel_form_against_vel64(capi, oracle, report, N, C):
    chop = oracle.EXAMPLE["choppiness"]
    scales = SCALES[:C] if C > 1 else (oracle.EXAMPLE["wavescale"],)
    states = [pw.lit_state(oracle, N, ws, 1000 + N + c) for c, ws in enumerate(scales)]
    with capi.Ocean(N, C) as oc:
        for c, ws in enumerate(scales):
            oc.set_cascade(c, ws, chop)
            oc.upload_state(c, states[c])
        oc.set_velocity("on")
        for _ in range(3):
            oc.update(DT)
            oc.displace()
        planes = [oc.read_velocity(c) for c in range(C)]
        phases = [oc.read_state(c) for c in range(C)]
    for c, ws in enumerate(scales):
        want = pw.lit_phase(oracle, N, ws, 3)
        assert np.array_equal(phases[c], want), (N, c, "phase")
        _check(report, f"N={N} x {C} cascade {c}", planes[c], states[c], want, ws, chop, N)


@pytest.mark.parametrize("group", [0, 1])
def test_wild_phases_negative_dt_and_one_cascade_per_launch(capi, oracle, report, group):
    N, chop = 64, 1.3
    states = [pw.lit_state(oracle, N, ws, 500 + c) for c, ws in enumerate(SCALES)]
    rs = np.random.RandomState(11)
    up = [(rs.random_sample((N, N)) * 31.4 - 10.0).astype(F) for _ in SCALES]
    with capi.Ocean(N, 3) as oc:
        for c, ws in enumerate(SCALES):
            oc.set_cascade(c, ws, chop)
            oc.upload_state(c, states[c], up[c])
        oc.set_cascade_group(group)
        oc.set_velocity("on")
        oc.update(DT)
        oc.update(-F(0.4))
        oc.displace()
        oc.update(DT)
        oc.displace()
        planes = [oc.read_velocity(c) for c in range(3)]
        phases = [oc.read_state(c) for c in range(3)]
    for c, ws in enumerate(SCALES):
        want = up[c].copy()
        for dt in (DT, -F(0.4), DT):
            oracle.update(want, ws, dt)
        assert np.array_equal(phases[c], want), (c, "phase")
        _check(report, f"uploaded phases, negative dt, group {group}, cascade {c}", planes[c], states[c], want, ws, chop, N)


@pytest.mark.parametrize("N", [64, 1024])
def test_single_bins_and_the_flat_ocean(capi, oracle, report, N):
    ws, chop = 22.0, 1.3
    h = N // 2
    bins = [(0, 0), (N - 1, N - 1), (h, h + 1), (0, h), (h, 0), (h, h)]
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, ws, chop)
        oc.set_velocity("on")
        for b in bins:
            h0 = pw.lit_edge_h0(N, b)
            oc.upload_state(0, h0)
            oc.update(DT)
            oc.displace()
            plane, phase = oc.read_velocity(0), oc.read_state(0)
            ref = vel64.single_bin64(N, b, pw.LIT_EDGE_AMP, phase, F(1) / F(ws), chop, vel64.omega32(N, ws))
            k = vel64.k_of(_channels(plane), ref, N)
            print(f"velocity single bin N={N} {b} against the closed form: K {k:.3g} (bar {vel64.K_VEL:.3g})")
            assert k <= vel64.K_VEL, (N, b, k)
        oc.upload_state(0, np.zeros((N, N, 2), F))
        oc.update(DT)
        oc.displace()
        assert np.all(oc.read_velocity(0) == 0)


# 2 -- nothing else moves

QUEUES = ((1,), (0,), (2, 1), (1,), (3,), (1, 1, 1), (), (2,), (1,), (1, 2), (1,), (0, 1), (4,), (1,), (), (1, 1), (2,))


@pytest.mark.parametrize("mode", ["fp32", "fp16", "fp16h0", "literal"])
def test_maps_phase_and_foam_are_those_of_velocity_off(capi, oracle, mode):
    N, C, chop = 128, 2, 1.3
    assert len(QUEUES) == 17
    states = [pw.lit_state(oracle, N, ws, 300 + c) for c, ws in enumerate(SCALES[:C])]
    handles = []
    try:
        for vel, every in ((False, 1), (True, 1), (True, 8)):
            oc = capi.Ocean(N, C)
            handles.append(oc)
            for c, ws in enumerate(SCALES[:C]):
                oc.set_cascade(c, ws, chop)
                oc.upload_state(c, states[c])
            if mode == "literal":
                oc.set_literal_transform(True)
            else:
                oc.set_spectrum_format(mode)
            oc.set_phase_writeback(every)
            oc.set_foam("accumulate")
            if vel:
                oc.set_velocity("on")
        off, on1, on8 = handles
        for step, queue in enumerate(QUEUES):
            for oc in handles:
                for q in queue:
                    oc.update(F(q) * DT * F(0.37 + 0.11 * step))
                oc.displace()
            for c in range(C):
                want = off.read_maps(c)
                foam = off.read_foam(c)
                for oc in (on1, on8):
                    assert np.array_equal(_bits(oc.read_maps(c)), _bits(want)), (mode, step, c, "maps")
                    assert np.array_equal(_bits(oc.read_foam(c)), _bits(foam)), (mode, step, c, "foam")
                assert np.array_equal(_bits(on1.read_velocity(c)), _bits(on8.read_velocity(c))), (mode, step, c, "velocity")
        for c in range(C):
            want = off.read_state(c)
            for oc in (on1, on8):
                assert np.array_equal(_bits(oc.read_state(c)), _bits(want)), (mode, c, "phase")
            # the velocity kernels read fp32 h0 and the phase whatever the format: the plane is held to the same bar in every mode
            ref = vel64.vel64(states[c], want, F(1) / F(SCALES[c]), chop, vel64.omega32(N, SCALES[c]))
            k = vel64.k_of(_channels(on1.read_velocity(c)), ref, N)
            print(f"velocity pointwise mode {mode} cascade {c}: K {k:.3g} (bar {vel64.K_VEL:.3g})")
            assert k <= vel64.K_VEL, (mode, c, k)
    finally:
        for oc in handles:
            oc.close()


# 3 -- queries

def _points(M, seed):
    rs = np.random.RandomState(seed)
    return ((rs.random_sample((M, 2)) - 0.5) * 300.0).astype(F)


@pytest.mark.parametrize("N,C", [(64, 3), (2048, 2)])
def test_queries_bit_for_bit(capi, oracle, N, C):
    import torch

    chop = 1.3
    scales = SCALES[:C]
    pts = _points(3000, N)
    with capi.Ocean(N, C) as oc:
        for c, ws in enumerate(scales):
            oc.set_cascade(c, ws, chop)
            oc.upload_state(c, pw.lit_state(oracle, N, ws, 700 + c))
        s = _set(capi, N, F(1) / F(scales[0]))
        oc.update(DT)
        oc.displace()
        # ESTATE while velocity is off, and while no displace has run since it was switched on
        lst = (ctypes.c_int * 1)(0)
        out = np.zeros((pts.shape[0], 8), F)
        args = (oc.h, lst, 1, ctypes.byref(s), 0, pts.ctypes.data_as(capi.P), pts.shape[0], out.ctypes.data_as(capi.P))
        assert oc.lib.datum_ocean_read_velocity_blend(*args) == capi.ESTATE
        assert oc.lib.datum_ocean_read_velocity(oc.h, 0, out.ctypes.data_as(capi.P)) == capi.ESTATE
        oc.set_velocity("on")
        assert oc.lib.datum_ocean_read_velocity_blend(*args) == capi.ESTATE
        oc.update(DT)
        oc.displace()
        maps = [oc.read_maps(c) for c in range(C)]
        planes = [oc.read_velocity(c) for c in range(C)]
        lists = [[C - 1], [0, 0]] + ([[0, 1, 2]] if C >= 3 else [[1, 0]])
        for cascades in lists:
            sc = [F(1) / F(scales[c]) for c in cascades]
            for it in (0, 4):
                got = oc.read_velocity_blend(cascades, s, pts, it)
                want = oc.read_surface_blend(cascades, s, pts, it)
                assert np.array_equal(_bits(got[:, :4]), _bits(want[:, :4])), (N, cascades, it, "V(b), residual")
                assert np.all(got[:, 7] == 0)
                vel = vel64.sample32([maps[c] for c in cascades], [planes[c] for c in cascades], sc, pts, it)
                assert np.array_equal(_bits(got[:, 4:7]), _bits(vel)), (N, cascades, it, "velocity")
                assert np.abs(got[:, 4:7]).max() > 0
        # a non-finite point: quiet NaNs, its neighbours untouched
        bad = pts[:8].copy()
        bad[3, 0] = np.inf
        bad[5, 1] = np.nan
        got = oc.read_velocity_blend(lists[-1], s, bad, 4)
        ok = oc.read_velocity_blend(lists[-1], s, pts[:8], 4)
        assert np.isnan(got[[3, 5]]).all()
        keep = [0, 1, 2, 4, 6, 7]
        assert np.array_equal(_bits(got[keep]), _bits(ok[keep]))
        # device pointers, and a bound plane: the same bits from caller-owned memory
        P = N * N * 4 * C
        mine = torch.zeros(P, dtype=torch.float32, device="cuda:0")
        oc.bind_velocity(mine.data_ptr(), P * 4)
        assert oc.lib.datum_ocean_read_velocity_blend(*args) == capi.ESTATE
        oc.displace()
        ptr, nbytes = oc.velocity_device()
        assert ptr == mine.data_ptr() and nbytes == P * 4
        dpts = torch.from_numpy(pts).to("cuda:0")
        dout = torch.zeros(pts.shape[0] * 8, dtype=torch.float32, device="cuda:0")
        oc.sample_velocity_blend(lists[-1], s, dpts.data_ptr(), pts.shape[0], dout.data_ptr(), 4)
        oc.sync()
        want = oc.read_velocity_blend(lists[-1], s, pts, 4)
        assert np.array_equal(_bits(dout.cpu().numpy().reshape(-1, 8)), _bits(want))
        bound = mine.cpu().numpy().reshape(C, N, N, 4)
        for c in range(C):
            assert np.array_equal(_bits(bound[c]), _bits(planes[c])), (c, "bound plane")
        oc.bind_velocity(None, 0)
        oc.set_velocity("off")
        assert oc.lib.datum_ocean_read_velocity(oc.h, 0, out.ctypes.data_as(capi.P)) == capi.ESTATE


# 4 -- the C++ shim

def test_cpp_shim(oracle, report):
    from datum_amd import host_api

    N = 256
    e = oracle.EXAMPLE
    params = host_api.OceanParams(N, **host_api.EXAMPLE_TUNABLES)
    params.seed_ocean(1000)
    h0 = params.height.copy()
    pts = _points(500, 5)
    with host_api.OceanContext(N, device=0) as ctx:
        with pytest.raises(Exception):
            ctx.read_velocity()
        ctx.set_velocity("on")
        for _ in range(3):
            params.update_ocean(DT)
            ctx.displace_ocean_surface(params)
        ctx.fetch_ocean_state(params)
        plane = ctx.read_velocity()
        got = ctx.query_ocean_velocity(params, pts, 4)
        want = ctx.query_ocean_surface(params, pts, 4)
        ctx.set_velocity("off")
        with pytest.raises(Exception):
            ctx.query_ocean_velocity(params, pts, 4)
    _check(report, "C++ shim N=256", plane, h0, params.phase, e["wavescale"], e["choppiness"], N)
    assert np.array_equal(_bits(got[:, :4]), _bits(want[:, :4]))
    assert np.all(got[:, 7] == 0) and np.abs(got[:, 4:7]).max() > 0
