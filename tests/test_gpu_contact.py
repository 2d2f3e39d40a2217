"""GPU tests of body contact (include/datum_ocean_hip.h: datum_ocean_step_bodies_contact) against tests/contact64.py, bit for bit.  The
velocity records and the layer's samples are read from the device (calls pinned by their own tests); everything behind them -- the rippled
record, the twenty-two sums, the contact's totals, the integrator, the record's fold -- is the numpy restatement's.  The whole call of
one and of three sub-steps is held against contact64's fp32 loop over ripple_bed64's layer with the same walls, bed and deposits (only
the velocity records are the device's); beside that, a call of K sub-steps against K calls of one, each against the restatement from
the device's samples of the layer as it then lies, and the layer after a call against the coupled call's, which deposits the same wake.

N = 64 x 3 cascades, velocity on, R = 64, s = 0.5; 1, 4, 5 and 9 bodies (the last workgroup partly empty) of 1, 63, 64, 65 and 130 probes."""

import ctypes

import numpy as np
import pytest

import body64
import contact64
import couple64
import drag64
import ripple64
import ripple_bed64
import step64
from test_gpu_body import _step
from test_gpu_drag import _moving
from test_gpu_step import _bits, _bytes
from test_gpu_surface import DT, _set

pytestmark = pytest.mark.gpu

F = np.float32
N, C, CASCADES, R, CELL, IT = 64, 3, [0, 1, 2], 64, 0.5, 4
PROBES = [1, 63, 64, 65, 130, 64, 65, 1, 130]
LO = -R // 2 * CELL                                    # the window of a fresh layer: [-16, 16) m both ways


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


def _fleet(nb, seed=3, z=(-1.6, -0.4)):
    """nb bodies of PROBES[b] probes over the window, rotated, moving, with drag; low enough for many hulls to reach the ground"""
    rng = np.random.RandomState(seed)
    counts = PROBES[:nb]
    rot = []
    for _ in range(nb):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        rot.append(q * np.sign(np.linalg.det(q)))
    pos = np.stack([rng.uniform(LO + 3, -LO - 3, nb), rng.uniform(LO + 3, -LO - 3, nb), rng.uniform(z[0], z[1], nb)], 1)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    bodies = body64.make_bodies(rot, pos, first, counts, [np.inf] * nb)
    probes = np.concatenate([rng.uniform(-1.5, 1.5, (sum(counts), 3)), rng.uniform(0.02, 0.06, (sum(counts), 1))], 1).astype(F)
    motions = drag64.make_motions(rng.uniform(-1, 1, (nb, 3)), rng.uniform(-0.3, 0.3, (nb, 3)), rng.uniform(50, 500, nb), rng.uniform(0, 50, nb))
    props = step64.make_props(1.0 / rng.uniform(500, 5000, nb), 1.0 / rng.uniform(500, 5000, (nb, 3)), 9.81, 9810.0)
    return bodies, motions, props, probes


def _harbour(capi, oc, flags, k=2.0e4, c=400.0, ct=60.0, walls=None, seed=4):
    """the handle's layer with a bed whose map covers x < 8 (off it `outside`, 1.2 m deep: ground contact off the map too) and rises to
    land towards -x, and a wall list: a rotated box and an ellipse with non-unit axes, and two boxes that overlap.  Returns the scene of
    the restatement and the ctypes parameters"""
    rng = np.random.RandomState(seed)
    oc.set_ripples(0)
    oc.set_ripple_params(2.0, 0.05, 8, 4.0)
    oc.set_ripples(R, CELL)
    W, H, texel = 25, 33, 1.0
    x = np.arange(W)[None, :] / (W - 1)
    depths = (2.5 * x - 0.5 + 0.15 * rng.normal(size=(H, W))).astype(F)
    bed = dict(origin=(LO + 0.25, LO - 0.125), texel=texel, outside=1.2)
    rows = walls if walls is not None else [
        (-6.0, 5.0, 0.7 * np.cos(0.6), 0.7 * np.sin(0.6), 2.5, 1.0, contact64.BOX),
        (6.0, -5.0, 1.6 * np.cos(-0.5), 1.6 * np.sin(-0.5), 5.0, 3.0, contact64.ELLIPSE),
        (3.0, 7.0, 1.0, 0.0, 3.0, 2.0, contact64.BOX),
        (5.0, 8.0, 0.0, 1.0, 2.0, 2.5, contact64.BOX),
    ]
    wl = contact64.make_walls(rows)
    gw = np.zeros(len(wl), capi.RIPPLE_WALL)
    for f in ("center", "axis", "half", "kind"):
        gw[f] = wl[f]
    oc.set_ripple_walls(gw)
    gb = np.zeros(1, capi.RIPPLE_BED)
    gb["width"], gb["height"], gb["origin"], gb["texel"], gb["outside"] = W, H, bed["origin"], texel, bed["outside"]
    gb["max_depth"], gb["dry_depth"], gb["surf_depth"], gb["surf_gamma"] = 3.0, 0.05, 0.5, 2.0
    oc.set_ripple_bed(gb[0], depths)
    # a layer that is not at rest
    imp = np.zeros((200, 4), F)
    imp[:, :2] = rng.uniform(LO, -LO, (200, 2))
    imp[:, 2] = rng.normal(size=200) * 0.01
    oc.deposit_ripples_host(imp)
    oc.step_ripples(0.02, 2)
    oc.deposit_ripples_host(imp[:50])
    scene = contact64.make_scene(k, c, ct, flags, bed, depths, wl)
    con = capi.BodyContact(k, c, ct, flags)
    # the model's layer through the same calls: scene["layer"] is the restatement of the handle's layer as it now lies
    lay = ripple_bed64.Layer(R, CELL, F, 2.0, 0.05, 8, 4.0)
    lay.set_walls(gw)
    lay.set_bed(gb[0], depths)
    lay.deposit(imp)
    lay.step(0.02, 2)
    lay.deposit(imp[:50])
    scene["layer"] = lay
    return scene, con


def _same(got, want, what):
    gb, gm, gr = got
    wb, wm, wr = want
    assert np.array_equal(_bytes(gb), _bytes(wb)), (what, "bodies", np.argwhere((_bytes(gb) != _bytes(wb)).any(1))[:4].ravel())
    assert np.array_equal(_bytes(gm), _bytes(wm)), (what, "motions", np.argwhere((_bytes(gm) != _bytes(wm)).any(1))[:4].ravel())
    gn, wn = np.isnan(gr), np.isnan(wr)
    assert np.array_equal(gn, wn) and np.array_equal(_bits(gr)[~gn], _bits(wr)[~wn]), (what, "records", np.argwhere(_bits(gr) != _bits(wr))[:4])


def _want(oc, s, bodies, motions, props, probes, h, scene, old=None):
    """the restatement's sub-step from the device's velocity records and the device's samples of the layer as it lies"""
    pts = couple64.points32(bodies, probes)
    recs = oc.read_velocity_blend(CASCADES, s, pts, IT)
    return contact64.substep32(ripple64.Layer(R, CELL), bodies, motions, props, probes, recs, h, scene, samples=oc.query_ripples(pts), old=old)


@pytest.mark.parametrize("nb", (1, 4, 5, 9))
def test_bits_one_and_three_substeps(capi, oracle, nb):
    bodies, motions, props, probes = _fleet(nb)
    flags = contact64.BED | contact64.WALLS
    dt, K = float(DT), 3
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        s = _set(capi, 0)
        # one sub-step
        scene, con = _harbour(capi, oc, flags)
        wb, wm, wr, bad = _want(oc, s, bodies, motions, props, probes, step64.step_size(dt, 1), scene)
        assert not bad.any()
        gb, gm = bodies.copy(), motions.copy()
        gr = oc.step_bodies_contact_host(CASCADES, s, gb, gm, props, probes, dt, con, 1, IT)
        assert gr.shape == (nb, 16)
        _same((gb, gm, gr), (wb, wm, wr), (nb, "one"))
        state1 = oc.read_ripples().copy()
        # ... and the layer is the coupled call's: the same wake, the same sub-step
        _harbour(capi, oc, flags)
        cb, cm = bodies.copy(), motions.copy()
        oc.step_bodies_coupled_host(CASCADES, s, cb, cm, props, probes, dt, 1, IT)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(state1))
        if nb >= 5:
            assert np.count_nonzero(gr[:, 15]) >= 2 and np.abs(gr[:, 12:15]).max() > 1 and (gb["position"] != cb["position"]).any()

        # K calls of one sub-step of length h against the restatement, each from the layer as it lies; fields 7, 11 and 15 fold
        h = step64.step_size(dt, K)
        _harbour(capi, oc, flags)
        kb, km = bodies.copy(), motions.copy()
        wb, wm, wr = bodies, motions, None
        res, dropped, deep = np.zeros(nb, F), np.zeros(nb, F), np.zeros(nb, F)
        for i in range(K):
            wb, wm, wr, bad = _want(oc, s, wb, wm, props, probes, h, scene, old=wr)
            assert not bad.any()
            kr = oc.step_bodies_contact_host(CASCADES, s, kb, km, props, probes, float(h), con, 1, IT)
            res, dropped, deep = np.fmax(res, kr[:, 7]), dropped + kr[:, 11], np.fmax(deep, kr[:, 15])
        kr[:, 7], kr[:, 11], kr[:, 15] = res, dropped, deep
        _same((kb, km, kr), (wb, wm, wr), (nb, "K calls"))
        stateK = oc.read_ripples().copy()
        # one call of K sub-steps: the same bytes and the same layer
        _harbour(capi, oc, flags)
        gb, gm = bodies.copy(), motions.copy()
        gr = oc.step_bodies_contact_host(CASCADES, s, gb, gm, props, probes, dt, con, K, IT)
        _same((gb, gm, gr), (kb, km, kr), (nb, "one call"))
        assert np.array_equal(_bits(oc.read_ripples()), _bits(stateK))


@pytest.mark.parametrize("case", ("ground", "off_map", "box", "ellipse", "overlap"))
def test_bits_case_by_case(capi, oracle, case):
    """one kind of contact at a time: a flat hull of 64 probes set down where only that contact is met"""
    rng = np.random.RandomState(12)
    n = 64
    probes = np.concatenate([rng.uniform(-0.6, 0.6, (n, 2)), np.zeros((n, 1)), np.full((n, 1), 0.05)], 1).astype(F)
    where = dict(ground=(-12.0, -8.0, -0.3), off_map=(12.0, -12.0, -1.3), box=(-6.0, 5.0, 5.0), ellipse=(6.0, -5.0, 5.0), overlap=(4.5, 7.5, 5.0))[case]
    flags = contact64.BED if case in ("ground", "off_map") else contact64.WALLS
    bodies = body64.make_bodies([np.eye(3)], [where], [0], [n], [np.inf])
    motions = drag64.make_motions([[0.4, -0.3, -0.5]], [[0.05, -0.02, 0.1]], [100.0], [5.0])
    props = step64.make_props([1.0 / 800], [[1.0e-3] * 3], 9.81, 9810.0)
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        s = _set(capi, 0)
        scene, con = _harbour(capi, oc, flags)
        want = _want(oc, s, bodies, motions, props, probes, step64.step_size(float(DT), 1), scene)
        gb, gm = bodies.copy(), motions.copy()
        gr = oc.step_bodies_contact_host(CASCADES, s, gb, gm, props, probes, float(DT), con, 1, IT)
        _same((gb, gm, gr), want[:3], case)
        assert gr[0, 15] > 0 and np.abs(gr[0, 12:15]).max() > 0
        if flags == contact64.BED:
            assert gr[0, 14] > 0                                                # the ground pushes up
        k = contact64.reduce32(bodies, probes, contact64.terms(F, bodies, motions, probes, scene))
        assert k[0, 6] >= (2 * n if case == "overlap" else 1)


def test_nothing_touching_is_the_coupled_call(capi, oracle):
    """bed and walls set, every probe clear of both; and flags = 0 among the obstacles: pose, motion, fields 0-11 and the layer are
    step_bodies_coupled's bit for bit, fields 12-15 are +0"""
    bodies, motions, props, probes = _fleet(9, z=(3.0, 6.0))
    clear = bodies.copy()
    clear["position"][:, :2] = np.random.RandomState(2).uniform(11.0, 13.0, (9, 2)) * [1, -1]          # no shape stands there
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        s = _set(capi, 0)
        for flags, b0 in ((contact64.BED | contact64.WALLS, clear), (0, _fleet(9)[0])):
            for K in (1, 3):
                scene, con = _harbour(capi, oc, flags)
                cb, cm = b0.copy(), motions.copy()
                cr = oc.step_bodies_coupled_host(CASCADES, s, cb, cm, props, probes, float(DT), K, IT)
                cstate = oc.read_ripples().copy()
                _harbour(capi, oc, flags)
                gb, gm = b0.copy(), motions.copy()
                gr = oc.step_bodies_contact_host(CASCADES, s, gb, gm, props, probes, float(DT), con, K, IT)
                _same((gb, gm, gr[:, :12]), (cb, cm, cr), (flags, K))
                assert np.all(_bits(gr[:, 12:]) == 0) and np.array_equal(_bits(oc.read_ripples()), _bits(cstate))


def test_canaries_bad_bodies_and_entry_points(capi, oracle, torch):
    nb = 9
    bodies, motions, props, probes = _fleet(nb)
    flags = contact64.BED | contact64.WALLS
    dt, K = float(DT), 3
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        s = _set(capi, 0)
        # a bad body among good ones of its workgroup: sixteen NaNs, its pose alone, the neighbours as without it
        _harbour(capi, oc, flags)
        cb, cm = bodies.copy(), motions.copy()
        clean = oc.step_bodies_contact_host(CASCADES, s, cb, cm, props, probes, dt, capi.BodyContact(2.0e4, 400.0, 60.0, flags), K, IT)
        clean_state = oc.read_ripples().copy()
        assert np.isfinite(clean).all()
        scene, con = _harbour(capi, oc, flags)
        ob, om = bodies.copy(), motions.copy()
        one = oc.step_bodies_contact_host(CASCADES, s, ob, om, props, probes, dt, con, 1, IT)
        _harbour(capi, oc, flags)
        bad = bodies.copy()
        bad["cap"][5] = np.nan
        gb, gm = bad.copy(), motions.copy()
        gr = oc.step_bodies_contact_host(CASCADES, s, gb, gm, props, probes, dt, con, 1, IT)
        assert np.isnan(gr[5]).all() and gr[5].shape == (16,) and _bytes(gb)[5].tobytes() == _bytes(bad)[5].tobytes() and _bytes(gm)[5].tobytes() == _bytes(motions)[5].tobytes()
        keep = np.arange(nb) != 5
        # (within one sub-step no body sees another: the neighbours in body 5's workgroup have the bytes they have without it)
        assert np.array_equal(_bits(gr[keep]), _bits(one[keep])) and np.array_equal(_bytes(gb[keep]), _bytes(ob[keep])) and np.array_equal(_bytes(gm[keep]), _bytes(om[keep]))

        # the device entry point: the host twin's bytes, canaries round every array
        G, CAN = 64, F(-3.0e38)

        def guarded(a):
            flat = np.ascontiguousarray(a).view(F).ravel()
            t = torch.full((len(flat) + 2 * G,), float(CAN), dtype=torch.float32, device="cuda")
            t[G:G + len(flat)] = torch.from_numpy(flat.copy()).cuda()
            return t

        _harbour(capi, oc, flags)
        db, dm, dr = guarded(bodies), guarded(motions), guarded(np.zeros((nb, 16), F))
        dq, dp = guarded(props.view(F).reshape(nb, 8)), guarded(probes)
        torch.cuda.synchronize()
        off = G * 4
        oc.step_bodies_contact(CASCADES, s, db.data_ptr() + off, dm.data_ptr() + off, dq.data_ptr() + off, nb, dp.data_ptr() + off, len(probes), dt, K, dr.data_ptr() + off, con, IT)
        oc.sync()
        for t, want in ((db, cb), (dm, cm), (dr, clean), (dq, props), (dp, probes)):
            raw = t.cpu().numpy()
            assert np.all(raw[:G] == CAN) and np.all(raw[-G:] == CAN)
            assert np.array_equal(raw[G:-G].view(np.uint32), np.ascontiguousarray(want).view(np.uint32).ravel())
        assert np.array_equal(_bits(oc.read_ripples()), _bits(clean_state))


def test_cpp_shim_matches_capi(capi):
    from datum_amd import host_api

    Nh = 256
    params = host_api.OceanParams(Nh, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.4))
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    bodies, motions, props, probes = _fleet(5)
    con = capi.BodyContact(2.0e4, 400.0, 60.0, 0)
    with host_api.OceanContext(Nh) as ctx:
        ctx.set_velocity("on")
        for _ in range(2):
            params.update_ocean(DT)
            ctx.displace_ocean_surface(params)
        with pytest.raises(Exception):
            ctx.step_ocean_bodies_contact(params, bodies.copy(), motions.copy(), props, probes, float(DT), con, 2, 4)           # the layer is off
        lib = capi.load()
        h = ctx.lib.datum_host_context_handle(ctx.c)
        one = (capi.I * 1)(0)
        P = capi.P
        # the shim has no call for walls or a bed: they are set through the handle, as a renderer that owns it would
        wall = np.zeros(1, capi.RIPPLE_WALL)
        wall["center"], wall["axis"], wall["half"], wall["kind"] = (0.0, 0.0), (1.0, 0.0), (40.0, 40.0), contact64.BOX
        for sub in (1, 3):
            res = []
            for shim in (True, False):
                ctx.set_ocean_ripples(R, CELL)
                assert lib.datum_ocean_set_ripple_walls(h, wall.ctypes.data_as(P), 1) == capi.OK
                cw = capi.BodyContact(2.0e4, 400.0, 60.0, contact64.WALLS)
                gb, gm = bodies.copy(), motions.copy()
                if shim:
                    got = ctx.step_ocean_bodies_contact(params, gb, gm, props, probes, float(DT), cw, sub, 4)
                else:
                    s = params.oceanset(camera)
                    got = np.empty((len(bodies), 16), F)
                    assert lib.datum_ocean_step_bodies_contact_host(h, one, 1, ctypes.byref(s), 4, gb.ctypes.data_as(P), gm.ctypes.data_as(P), props.ctypes.data_as(P), len(bodies),
                                                                    probes.ctypes.data_as(P), len(probes), float(DT), sub, got.ctypes.data_as(P), ctypes.cast(ctypes.byref(cw), P)) == capi.OK
                res.append((gb, gm, got))
            _same(res[0], res[1], sub)
            assert np.isfinite(res[0][2]).all() and np.all(res[0][2][:, 15] > 0)


def test_refusals_change_nothing(capi, oracle):
    """every refusal the contact call adds to the coupled call's, from both entry points: the status, the call's name in the text, and
    poses, motions, records and the layer untouched"""
    nb = 4
    bodies, motions, props, probes = _fleet(nb)
    dt = float(DT)
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        s = _set(capi, 0)
        lib, P = capi.load(), capi.P
        arr = (capi.I * 3)(*CASCADES)
        rec = np.zeros((nb, 16), F)
        hb, hm = bodies.copy(), motions.copy()
        args = (arr, 3, ctypes.byref(s), IT, hb.ctypes.data_as(P), hm.ctypes.data_as(P), props.ctypes.data_as(P), nb, probes.ctypes.data_as(P), len(probes))
        names = ("datum_ocean_step_bodies_contact_host", "datum_ocean_step_bodies_contact")
        both = contact64.BED | contact64.WALLS

        def refused(con, dt_, sub, status, what):
            ptr0, state0 = oc.ripples_device()[0], oc.read_ripples().copy()
            c = None if con is None else ctypes.cast(ctypes.byref(con), P)
            for name in names:
                assert getattr(lib, name)(oc.h, *args, dt_, sub, rec.ctypes.data_as(P), c) == status, (name, what)
                assert name.encode() in lib.datum_ocean_last_error(oc.h)
            assert np.array_equal(_bytes(hb), _bytes(bodies)) and np.array_equal(_bytes(hm), _bytes(motions)) and np.all(rec == 0), what
            assert oc.ripples_device()[0] == ptr0 and np.array_equal(_bits(oc.read_ripples()), _bits(state0)), what

        _harbour(capi, oc, both)
        B = capi.BodyContact
        refused(None, dt, 1, capi.EINVAL, "null contact")
        for bad in (float("nan"), float("inf"), -1.0):
            refused(B(bad, 1.0, 1.0, both), dt, 1, capi.EINVAL, ("stiffness", bad))
            refused(B(1.0, bad, 1.0, both), dt, 1, capi.EINVAL, ("damping", bad))
            refused(B(1.0, 1.0, bad, both), dt, 1, capi.EINVAL, ("friction", bad))
        refused(B(1.0, 1.0, 1.0, 4), dt, 1, capi.EINVAL, "unknown flag")
        refused(B(1.0, 1.0, 1.0, both | 0x80000000), dt, 1, capi.EINVAL, "unknown flag")
        # what the coupled call refuses, with a good contact struct
        refused(B(1.0, 1.0, 1.0, both), dt, 0, capi.EINVAL, "substeps")
        refused(B(1.0, 1.0, 1.0, both), -dt, 1, capi.EINVAL, "dt")
        refused(B(1.0, 1.0, 1.0, both), 10.0, 1, capi.EINVAL, "stability")
        # a flag without its object
        oc.set_ripple_bed(None)
        refused(B(1.0, 1.0, 1.0, contact64.BED), dt, 1, capi.ESTATE, "no bed")
        refused(B(1.0, 1.0, 1.0, both), dt, 1, capi.ESTATE, "no bed")
        oc.set_ripple_walls(None)
        refused(B(1.0, 1.0, 1.0, contact64.WALLS), dt, 1, capi.ESTATE, "no walls")
        # ... and with neither flag the call goes through
        for name in names[:1]:
            assert getattr(lib, name)(oc.h, *args, dt, 1, rec.ctypes.data_as(P), ctypes.cast(ctypes.byref(B(1.0, 1.0, 1.0, 0)), P)) == capi.OK
        assert np.isfinite(rec).all() and np.all(_bits(rec[:, 12:]) == 0) and not np.array_equal(_bytes(hb), _bytes(bodies))
        # the layer off: ESTATE first, whatever else is said
        oc.set_ripples(0)
        for name in names:
            assert getattr(lib, name)(oc.h, *args, dt, 1, rec.ctypes.data_as(P), None) == capi.ESTATE


@pytest.mark.parametrize("K", (1, 3))
def test_bits_against_the_fp32_loop_over_the_model_layer(capi, oracle, K):
    """the whole call against contact64.call32 over ripple_bed64's layer with the same walls and bed: only the velocity records are the
    device's; the samples, the deposits and the layer's sub-steps between the bodies' are the model's"""
    nb = 9
    bodies, motions, props, probes = _fleet(nb)
    flags = contact64.BED | contact64.WALLS
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        s = _set(capi, 0)
        scene, con = _harbour(capi, oc, flags)
        lay = scene["layer"]
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())) and np.abs(lay.eta).max() > 0 and np.count_nonzero(lay.src) > 20
        recs_of = lambda b: oc.read_velocity_blend(CASCADES, s, couple64.points32(b, probes), IT)
        wb, wm, wr = contact64.call32(lay, bodies, motions, props, probes, recs_of, float(DT), K, scene)
        gb, gm = bodies.copy(), motions.copy()
        gr = oc.step_bodies_contact_host(CASCADES, s, gb, gm, props, probes, float(DT), con, K, IT)
        _same((gb, gm, gr), (wb, wm, wr), ("model layer", K))
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))
        assert np.count_nonzero(gr[:, 15]) >= 2
