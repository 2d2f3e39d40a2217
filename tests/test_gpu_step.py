"""Body stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies) on the MI355X.

  1  bits, one sub-step: step_bodies_host against step64.integrate32 of the records read_bodies and read_body_drag give for the same pose
     and motion -- bodies, motions and records, no tolerance: the two calls' records are pinned by tests/test_gpu_body.py and
     tests/test_gpu_drag.py, the integrator is the definition's.  The same comparison holds the device's division and sqrt to the
     correctly rounded ones (numpy's);
  2  bits, several sub-steps: against a host loop of the two calls plus integrate32 per sub-step, and against K calls of one sub-step;
  3  known answers on the flat ocean: a box at its equilibrium draught stays, a box released above it settles (the damped spring);
  4  edges; 5  the device entry point and the C++ shim.
"""

import ctypes

import numpy as np
import pytest

import body64
import drag64
import step64
from test_gpu_body import COUNTS, _box, _fleet, _step
from test_gpu_drag import _motions, _moving
from test_gpu_surface import DT, EPS, _set, _setup

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _props(seed, nb):
    """masses of 200 kg to 5 t, moments to match, g and rho g of water; every sixth body is not accelerated linearly (invmass 0), every
    seventh does not spin up about its second axis"""
    rng = np.random.RandomState(seed)
    b = np.arange(nb)
    p = step64.make_props(1.0 / rng.uniform(200, 5000, nb), 1.0 / rng.uniform(100, 5000, (nb, 3)), 9.81, 1000 * 9.81)
    p["invmass"][b % 6 == 2] = 0
    p["invinertia"][b % 7 == 4, 1] = 0
    return p


def _host_substep(oc, cascades, s, bodies, motions, props, probes, it, h):
    """the definition through the two existing calls: (bodies', motions', records, bad)"""
    lift = oc.read_bodies(cascades, s, bodies, probes, it)
    drag = oc.read_body_drag(cascades, s, bodies, motions, probes, it)
    return step64.integrate32(lift, drag, bodies, motions, props, h)


def _same(got, want, what):
    gb, gm, gr = got
    wb, wm, wr = want
    assert np.array_equal(_bytes(gb), _bytes(wb)), (what, "bodies", np.argwhere((_bytes(gb) != _bytes(wb)).any(1))[:4].ravel())
    assert np.array_equal(_bytes(gm), _bytes(wm)), (what, "motions", np.argwhere((_bytes(gm) != _bytes(wm)).any(1))[:4].ravel())
    assert np.array_equal(_bits(gr), _bits(wr)), (what, "records", np.argwhere(_bits(gr) != _bits(wr))[:4])


# 1 -- bits, one sub-step


@pytest.mark.parametrize("N,C,lists", [(64, 3, ([1], [0, 1, 2])), (2048, 2, ([1], [0, 1]))])
def test_bits_one_substep(capi, oracle, N, C, lists):
    bodies, probes = _fleet(N)
    motions, props = _motions(N, len(bodies)), _props(N, len(bodies))
    assert set(bodies["count"].tolist()) == set(COUNTS) and len(bodies) % 4 == 1
    assert (props["invmass"] == 0).any()
    h = step64.step_size(DT, 1)
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        for cascades in lists:
            for swell in (True, False):
                s = _set(capi, 0, swell)
                for it in (0, 4):
                    wb, wm, wr, bad = _host_substep(oc, cascades, s, bodies, motions, props, probes, it, h)
                    assert not bad.any()
                    gb, gm = bodies.copy(), motions.copy()
                    gr = oc.step_bodies_host(cascades, s, gb, gm, props, probes, float(DT), 1, it)
                    assert np.isfinite(gr).all()
                    _same((gb, gm, gr), (wb, wm, wr), (N, cascades, swell, it))
        # something happened: forces and torques, poses that moved and turned; dry bodies fall freely, pinned ones keep their place
        assert np.abs(gr[:, :3]).max() > 1 and np.abs(gr[:, 3:6]).max() > 1
        assert (gb["position"] != bodies["position"]).any() and (gb["rotation"] != bodies["rotation"]).any()
        dry = (gr[:, 6] == 0) & (bodies["count"] > 0)
        assert dry.any() and np.all(gr[dry, :6] == 0)
        pinned = props["invmass"] == 0
        assert np.array_equal(_bits(gm["linear"][pinned][:, :2]), _bits(motions["linear"][pinned][:, :2]))


# 2 -- bits, several sub-steps


@pytest.mark.parametrize("N,C,cascades", [(64, 3, [0, 1, 2]), (2048, 2, [0, 1])])
def test_bits_several_substeps(capi, oracle, N, C, cascades):
    bodies, probes = _fleet(N + 2)
    motions, props = _motions(N + 2, len(bodies)), _props(N + 2, len(bodies))
    K, it = 3, 4
    dt = float(DT)
    h = step64.step_size(dt, K)
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        s = _set(capi, 0)
        # the host loop: K rounds of the two calls and the integrator, the same h each
        wb, wm, res = bodies, motions, np.zeros(len(bodies), F)
        for _ in range(K):
            wb, wm, wr, bad = _host_substep(oc, cascades, s, wb, wm, props, probes, it, h)
            assert not bad.any()
            res = np.fmax(res, wr[:, 7])
        wr[:, 7] = res
        gb, gm = bodies.copy(), motions.copy()
        gr = oc.step_bodies_host(cascades, s, gb, gm, props, probes, dt, K, it)
        _same((gb, gm, gr), (wb, wm, wr), (N, "host loop"))

        # K calls of one sub-step of length h: the same poses and motions; field 7 is the largest of the calls'
        cb, cm, res = bodies.copy(), motions.copy(), np.zeros(len(bodies), F)
        for _ in range(K):
            cr = oc.step_bodies_host(cascades, s, cb, cm, props, probes, float(h), 1, it)
            res = np.fmax(res, cr[:, 7])
        cr[:, 7] = res
        _same((gb, gm, gr), (cb, cm, cr), (N, "K calls"))
        assert (gb["rotation"] != bodies["rotation"]).any() and res.max() >= 0


# 3 -- known answers on the flat ocean


def _flat(capi, N=64):
    oc = capi.Ocean(N, 1)
    oc.set_cascade(0, 22.0, 1.35)
    oc.upload_state(0, np.zeros((N, N, 2), F))
    oc.set_velocity("on")
    oc.update(DT)
    oc.displace()
    return oc


def test_known_answers(capi):
    probes = _box()
    n = len(probes)
    sa = float(probes[:, 3].sum())                     # 20.25 m^2 of water plane
    # water at z = 0.25 (plane.w = -0.25, no swell, h0 = 0: the velocity plane is zeros).  Box 0: every product exact -- rho g = 8192,
    # M = 81 * (0.25 * 0.5) = 10.125, invmass = 2^-13, gravity = 10.125 -- so the net force is +0.0 and nothing moves, bit for bit.
    # Boxes 1, 2: 10125 kg in water of rho g = 9810, so the equilibrium draught is 0.5 m; 1 starts there, 2 starts 0.2 m higher with
    # a linear drag that damps it (water at rest: f = -m cl v)
    z_eq, lift = -0.25, 0.2
    bodies = body64.make_bodies([np.eye(3)] * 3, [[10, -20, z_eq], [3, 4, z_eq], [-7, 2, z_eq + lift]], [0] * 3, [n] * 3, [np.inf] * 3)
    motions = drag64.make_motions(np.zeros((3, 3)), np.zeros((3, 3)), [0.0, 0.0, 2000.0], [0.0] * 3)
    props = step64.make_props([2.0 ** -13, 1.0 / 10125, 1.0 / 10125], np.full((3, 3), 1.0e-4), [10.125, 9.81, 9.81], [8192.0, 9810.0, 9810.0])
    calls, sub = 90, 2
    h = float(step64.step_size(DT, sub))
    with _flat(capi) as oc:
        assert np.all(oc.read_velocity(0) == 0)
        s = _set(capi, 0, swell=False, plane_w=-0.25)
        b, m = bodies.copy(), motions.copy()
        vz = []
        for _ in range(calls):
            r = oc.step_bodies_host([0], s, b, m, props, probes, float(DT), sub, 4)
            assert np.isfinite(r).all()
            vz.append(m["linear"][:, 2].copy())
    vz = np.abs(np.array(vz, np.float64))

    # box 0: exactly at rest
    assert np.array_equal(_bytes(b[:1]), _bytes(bodies[:1])) and np.array_equal(_bytes(m[:1]), _bytes(motions[:1]))
    assert r[0, 2] == F(8192.0 * 10.125) and r[0, 6] == F(10.125) and r[0, 7] == 0

    # box 1: the spring z'' = -w2 (z - z_eq) + a0 with w2 = rho g sa / mass, driven by the residual acceleration a0 of the fp32 parameters
    # (float64 of the given numbers) and by the roundings of the acceleration -- two products and a difference of values near 9.81 -- so
    # |a| <= |a0| + 3 eps 9.81.  From rest at z_eq the undamped spring stays within 2 |a| / w2 of it, the semi-implicit Euler step within
    # (1 + w h) of that (its conserved energy differs by the factor 1 +- w h / 2); on top, every sub-step rounds T.z + h v (half an ulp
    # of |z| < 0.5) and v + h a (v below w times the excursion: smaller than the first by w h)
    w2 = 9810.0 * sa * float(props["invmass"][1])
    a0 = abs(9810.0 * (sa * 0.5) * float(props["invmass"][1]) - float(props["gravity"][1]))
    a = a0 + 3 * EPS * 9.81
    wh = np.sqrt(w2) * h
    bar = 2 * a / w2 * (1 + wh) + calls * sub * EPS * 0.5 * (1 + wh)
    assert abs(float(b["position"][1, 2]) - z_eq) <= bar, (float(b["position"][1, 2]) - z_eq, bar)
    assert np.array_equal(_bits(b["position"][1, :2]), _bits(bodies["position"][1, :2]))

    # box 2: damped -- closer to equilibrium than it started, slower than at its peak
    assert abs(float(b["position"][2, 2]) - z_eq) < lift
    assert vz[:, 2].max() > 0 and vz[-1, 2] < vz[:, 2].max()


# 4 -- edges


def test_edges(capi, oracle, torch):
    N, cascades = 64, [1, 0]
    C = ctypes
    nb = 41
    counts = [(7, 64, 65, 130, 1, 0, 200)[b % 7] for b in range(nb)]
    bodies, probes = _fleet(5, nbodies=nb, nprobes=600, counts=counts)
    motions, props = _motions(5, nb), _props(5, nb)
    dt, sub = float(DT), 2
    with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
        _step(oc, 1)
        s = _set(capi, 0)
        lib = capi.load()
        arr = (capi.I * 2)(*cascades)
        P = capi.P
        rec = np.zeros((nb, 8), F)
        hb, hm = bodies.copy(), motions.copy()
        bp, mp, qp, pp, rp = hb.ctypes.data_as(P), hm.ctypes.data_as(P), props.ctypes.data_as(P), probes.ctypes.data_as(P), rec.ctypes.data_as(P)
        head = (arr, 2, C.byref(s), 4)
        good = head + (bp, mp, qp, nb, pp, 600, dt, sub, rp)
        names = ("datum_ocean_step_bodies_host", "datum_ocean_step_bodies")

        # ESTATE while velocity is off, and while no displace has run since it was switched on; nothing is written
        for name in names:
            assert getattr(lib, name)(oc.h, *good) == capi.ESTATE, name
            assert name.encode() in lib.datum_ocean_last_error(oc.h)
        oc.set_velocity("on")
        for name in names:
            assert getattr(lib, name)(oc.h, *good) == capi.ESTATE, name
        assert np.array_equal(_bytes(hb), _bytes(bodies)) and np.array_equal(_bytes(hm), _bytes(motions))
        _step(oc, 1)

        before = [oc.read_maps(c).copy() for c in (0, 1)], [oc.read_foam(c).copy() for c in (0, 1)], [oc.read_velocity(c).copy() for c in (0, 1)]
        cb, cm = bodies.copy(), motions.copy()
        clean = oc.step_bodies_host(cascades, s, cb, cm, props, probes, dt, sub, 4)
        assert np.isfinite(clean).all() and np.abs(clean[:, :3]).max() > 0

        # bad bodies: pose and motion bytes untouched, NaN records, the neighbours as without them
        bad, mb, qb = bodies.copy(), motions.copy(), props.copy()
        bad["first"][3], bad["count"][10] = -1, -2
        bad["first"][11], bad["count"][11] = 600 - 63, 64
        bad["cap"][17] = np.nan
        bad["position"][20, 0] = np.inf                     # count 0 or not: the integrated pose is not finite
        bad["rotation"][24].reshape(3, 3)[:, 0] = 0         # a first column of length zero: x = 0 / 0
        mb["angular"][24] = 0
        qb["invinertia"][24] = 0
        mb["linear"][27, 1], mb["cq"][28] = np.inf, np.nan
        qb["invmass"][30], qb["invinertia"][31, 2], qb["gravity"][32], qb["buoyancy"][33] = np.nan, np.inf, -np.inf, np.nan
        victims = [3, 10, 11, 17, 20, 24, 27, 28, 30, 31, 32, 33]
        gb, gm = bad.copy(), mb.copy()
        r = oc.step_bodies_host(cascades, s, gb, gm, qb, probes, dt, sub, 4)
        assert np.isnan(r[victims]).all()
        assert np.array_equal(_bytes(gb[victims]), _bytes(bad[victims])) and np.array_equal(_bytes(gm[victims]), _bytes(mb[victims]))
        keep = np.setdiff1d(np.arange(nb), victims)
        _same((gb[keep], gm[keep], r[keep]), (cb[keep], cm[keep], clean[keep]), "neighbours")
        # a bad probe spoils exactly the bodies whose range holds it
        pb = probes.copy()
        pb[300, 3] = np.nan
        gb, gm = bodies.copy(), motions.copy()
        r = oc.step_bodies_host(cascades, s, gb, gm, props, pb, dt, sub, 4)
        f, c = bodies["first"].astype(int), bodies["count"].astype(int)
        hit = (f <= 300) & (300 < f + c)
        assert hit.any() and not hit.all() and np.isnan(r[hit]).all()
        assert np.array_equal(_bytes(gb[hit]), _bytes(bodies[hit])) and np.array_equal(_bytes(gm[hit]), _bytes(motions[hit]))
        _same((gb[~hit], gm[~hit], r[~hit]), (cb[~hit], cm[~hit], clean[~hit]), "beside a bad probe")

        # nbodies == 0
        assert oc.step_bodies_host(cascades, s, bodies[:0].copy(), motions[:0].copy(), props[:0], probes, dt, sub, 4).shape == (0, 8)
        assert lib.datum_ocean_step_bodies(oc.h, *head, None, None, None, 0, None, 0, dt, sub, None) == capi.OK

        # argument errors with a live handle: body drag's, then the props pointer, substeps and dt
        mis = lambda a, k: P(a.ctypes.data + k)
        calls = [
            (None, 2, C.byref(s), 4, bp, mp, qp, nb, pp, 600, dt, sub, rp), (arr, 0, C.byref(s), 4, bp, mp, qp, nb, pp, 600, dt, sub, rp),
            (arr, 2, None, 4, bp, mp, qp, nb, pp, 600, dt, sub, rp), (arr, 2, C.byref(s), 17, bp, mp, qp, nb, pp, 600, dt, sub, rp),
            head + (None, mp, qp, nb, pp, 600, dt, sub, rp), head + (bp, None, qp, nb, pp, 600, dt, sub, rp), head + (bp, mp, qp, nb, None, 600, dt, sub, rp),
            head + (bp, mp, qp, nb, pp, 600, dt, sub, None), head + (mis(hb, 4), mp, qp, nb - 1, pp, 600, dt, sub, rp),
            head + (bp, mis(hm, 8), qp, nb - 1, pp, 600, dt, sub, rp), head + (bp, mp, qp, nb, mis(probes, 8), 599, dt, sub, rp),
            head + (bp, mp, qp, nb, pp, 600, dt, sub, mis(rec, 4)), head + (bp, mp, qp, 1 << 31, pp, 600, dt, sub, rp),
            head + (bp, mp, None, nb, pp, 600, dt, sub, rp), head + (bp, mp, mis(props, 4), nb - 1, pp, 600, dt, sub, rp),
            head + (bp, mp, qp, nb, pp, 600, dt, 0, rp), head + (bp, mp, qp, nb, pp, 600, dt, -1, rp),
            head + (bp, mp, qp, nb, pp, 600, dt, capi.STEP_MAX_SUBSTEPS + 1, rp),
            head + (bp, mp, qp, nb, pp, 600, float("nan"), sub, rp), head + (bp, mp, qp, nb, pp, 600, float("inf"), sub, rp),
        ]
        assert all(a.ctypes.data % 16 == 0 for a in (hb, hm, props, probes, rec))
        for args in calls:
            for name in names:
                assert getattr(lib, name)(oc.h, *args) == capi.EINVAL, (name, args[1:4], args[7], args[9:12])
                assert name.encode() in lib.datum_ocean_last_error(oc.h)
        assert np.array_equal(_bytes(hb), _bytes(bodies)) and np.array_equal(_bytes(hm), _bytes(motions))
        # a negative dt follows the arithmetic
        gb, gm = bodies.copy(), motions.copy()
        assert np.isfinite(oc.step_bodies_host(cascades, s, gb, gm, props, probes, -dt, sub, 4)).all()

        # the calls left the maps, the foam planes and the velocity planes as they were
        for c in (0, 1):
            assert np.array_equal(_bits(before[0][c]), _bits(oc.read_maps(c)))
            assert np.array_equal(_bits(before[1][c]), _bits(oc.read_foam(c)))
            assert np.array_equal(_bits(before[2][c]), _bits(oc.read_velocity(c)))


# 5 -- the device entry point and the C++ shim


def test_device_arrays_match_host_and_keep_canaries(capi, oracle, torch):
    N, cascades = 64, [0, 1]
    bodies, probes = _fleet(21, nbodies=45, nprobes=700, counts=[(0, 1, 63, 64, 65, 300)[b % 6] for b in range(45)])
    nb = len(bodies)
    motions, props = _motions(21, nb), _props(21, nb)
    bodies["cap"][7] = np.nan                               # one bad body: its slots are not written on the device either
    dt, sub, G, CAN = float(DT), 3, 64, F(-3.0e38)
    with _moving(capi, oracle, N, 2) as oc:
        _step(oc)
        s = _set(capi, 0)
        hb, hm = bodies.copy(), motions.copy()
        hr = oc.step_bodies_host(cascades, s, hb, hm, props, probes, dt, sub, 4)
        assert np.isnan(hr[7]).all() and np.isfinite(np.delete(hr, 7, 0)).all()

        def guarded(a):
            flat = np.ascontiguousarray(a).view(F).ravel()
            t = torch.full((len(flat) + 2 * G,), float(CAN), dtype=torch.float32, device="cuda")
            t[G:G + len(flat)] = torch.from_numpy(flat.copy()).cuda()
            return t

        db, dm, dr = guarded(bodies), guarded(motions), guarded(np.zeros((nb, 8), F))
        dq = torch.from_numpy(props.view(F).reshape(nb, 8).copy()).cuda()
        dp = torch.from_numpy(probes).cuda()
        torch.cuda.synchronize()
        off = G * 4
        oc.step_bodies(cascades, s, db.data_ptr() + off, dm.data_ptr() + off, dq.data_ptr(), nb, dp.data_ptr(), len(probes), dt, sub, dr.data_ptr() + off, 4)
        oc.sync()
        for t, want in ((db, hb), (dm, hm), (dr, hr)):
            raw = t.cpu().numpy()
            assert np.all(raw[:G] == CAN) and np.all(raw[-G:] == CAN)
            assert np.array_equal(raw[G:-G].view(np.uint32), np.ascontiguousarray(want).view(np.uint32).ravel())
        assert np.array_equal(dq.cpu().numpy().view(np.uint32), props.view(np.uint32).reshape(nb, 8))
        assert np.array_equal(_bits(dp.cpu().numpy()), _bits(probes))


def test_cpp_shim_matches_capi(capi):
    from datum_amd import host_api

    N = 256
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.4))
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    bodies, probes = _fleet(13, nbodies=77, nprobes=500, counts=[(0, 1, 64, 65, 200)[b % 5] for b in range(77)])
    motions, props = _motions(13, 77), _props(13, 77)
    with host_api.OceanContext(N) as ctx:
        with pytest.raises(Exception):
            ctx.step_ocean_bodies(params, bodies.copy(), motions.copy(), props, probes, float(DT), 2, 4)
        ctx.set_velocity("on")
        for _ in range(2):
            params.update_ocean(DT)
            ctx.displace_ocean_surface(params)
        lib = capi.load()
        h = ctx.lib.datum_host_context_handle(ctx.c)
        one = (capi.I * 1)(0)
        P = capi.P
        for sub in (1, 4):
            gb, gm = bodies.copy(), motions.copy()
            got = ctx.step_ocean_bodies(params, gb, gm, props, probes, float(DT), sub, 4)
            s = params.oceanset(camera)
            wb, wm, want = bodies.copy(), motions.copy(), np.empty_like(got)
            assert lib.datum_ocean_step_bodies_host(h, one, 1, ctypes.byref(s), 4, wb.ctypes.data_as(P), wm.ctypes.data_as(P), props.ctypes.data_as(P), len(bodies),
                                                    probes.ctypes.data_as(P), len(probes), float(DT), sub, want.ctypes.data_as(P)) == capi.OK
            _same((gb, gm, got), (wb, wm, want), sub)
            assert np.isfinite(got).all() and np.abs(got[:, :3]).max() > 0 and (gb["position"] != bodies["position"]).any()
