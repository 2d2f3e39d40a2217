"""GPU tests of coupled stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies_coupled) against tests/couple64.py, bit for bit: the
velocity records and the layer's samples are read from the device (calls that are pinned by their own tests), everything behind them --
the rippled record, the fourteen sums, the integrator, the record's fold, the wake's deposits and the layer's sub-step -- is the numpy
restatement's.  N = 64 x 3 cascades is the PLAIN map layout, 2048^2 x 2 the BANDED one; R = 64 and 128 with the origin (37, -21) wrap the
window round the torus in memory and span more than one tile of the ripple step."""

import ctypes

import numpy as np
import pytest

import body64
import couple64
import drag64
import ripple64
import step64
from test_gpu_body import _box, _fleet, _step
from test_gpu_drag import _motions, _moving
from test_gpu_ripples import ORIGIN, _impulses, _layer
from test_gpu_step import _bits, _bytes, _flat, _props
from test_gpu_surface import DT, _set, _setup

pytestmark = pytest.mark.gpu

F = np.float32
NB = 29                       # the last workgroup holds one body
SEAM, HALF, OUT = 3, 4, 5     # bodies of 64, 65 and 129 probes


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


def _same(got, want, what):
    gb, gm, gr = got
    wb, wm, wr = want
    assert np.array_equal(_bytes(gb), _bytes(wb)), (what, "bodies", np.argwhere((_bytes(gb) != _bytes(wb)).any(1))[:4].ravel())
    assert np.array_equal(_bytes(gm), _bytes(wm)), (what, "motions", np.argwhere((_bytes(gm) != _bytes(wm)).any(1))[:4].ravel())
    gn, wn = np.isnan(gr), np.isnan(wr)
    assert np.array_equal(gn, wn) and np.array_equal(_bits(gr)[~gn], _bits(wr)[~wn]), (what, "records", np.argwhere(_bits(gr) != _bits(wr))[:4])


def _bodies(seed, R, cell, origin=ORIGIN, nb=NB):
    """a fleet inside the window: one body on the window's seam in memory, one on the window's edge, one outside"""
    bodies, probes = _fleet(seed, nbodies=nb, nprobes=1500)
    rng = np.random.RandomState(seed)
    lo = np.array(origin) * cell
    bodies["position"][:, :2] = lo + rng.uniform(0.2, 0.8, (nb, 2)) * R * cell
    bodies["position"][:, 2] = rng.uniform(-1.0, 0.5, nb)
    bodies["position"][SEAM, :2] = np.array([-(-origin[0] // R) * R, -(-origin[1] // R) * R]) * cell
    bodies["position"][HALF, :2] = (lo[0], lo[1] + 0.5 * R * cell)
    bodies["position"][OUT, :2] = lo - 60.0
    bodies["position"][[SEAM, HALF, OUT], 2] = -0.5                             # in the water: they have a wake
    return bodies, probes, _motions(seed, nb), _props(seed, nb)


def _prime(oc, R, cell, seed=9):
    """the handle's layer and its restatement in the same non-trivial state: a few hundred impulses stepped a few times, and more pending"""
    oc.set_ripples(0)
    lay = _layer(oc, R, cell, 8)
    rng = np.random.RandomState(seed)
    for n, step in ((300, True), (100, False)):
        imp = _impulses(rng, lay, n, 0.05 * cell * cell)
        oc.deposit_ripples_host(imp)
        lay.deposit(imp)
        if step:
            oc.step_ripples(0.1 * cell, 3)
            lay.step(0.1 * cell, 3)
    assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())) and np.abs(lay.eta).max() > 0 and np.count_nonzero(lay.src) > 50
    return lay


def _host_substep(oc, lay, cascades, s, bodies, motions, props, probes, it, h, old=None):
    """the restatement's sub-step from the device's velocity records; in a call's first sub-step the samples are the device's too (the
    handle's layer is in the restatement's state then; later the host loop has stepped only the restatement, which samples itself)"""
    pts = couple64.points32(bodies, probes)
    recs = oc.read_velocity_blend(cascades, s, pts, it)
    samples = oc.query_ripples(pts) if old is None else None
    return couple64.substep32(lay, bodies, motions, props, probes, recs, h, samples=samples, old=old)


# 1 -- bits, one sub-step, a moving ocean, a layer that is not at rest


@pytest.mark.parametrize("N,C,lists,R,cell", [(64, 3, ([1], [0, 1, 2]), 64, 1.0), (2048, 2, ([1], [0, 1]), 128, 0.5)])
def test_bits_one_substep(capi, oracle, N, C, lists, R, cell):
    bodies, probes, motions, props = _bodies(N, R, cell)
    h = step64.step_size(DT, 1)
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        for cascades in lists:
            for swell in (True, False):
                s = _set(capi, 0, swell)
                for it in (0, 4):
                    lay = _prime(oc, R, cell)
                    before = lay.window().copy()
                    wb, wm, wr, bad = _host_substep(oc, lay, cascades, s, bodies, motions, props, probes, it, h)
                    assert not bad.any()
                    gb, gm = bodies.copy(), motions.copy()
                    gr = oc.step_bodies_coupled_host(cascades, s, gb, gm, props, probes, float(DT), 1, it)
                    _same((gb, gm, gr), (wb, wm, wr), (N, cascades, swell, it))
                    state = oc.read_ripples()
                    assert np.array_equal(_bits(state), _bits(lay.window())), (N, cascades, swell, it)
        # something happened: the layer changed under the hulls, a wake, forces, dropped quanta only where the window ends
        assert np.count_nonzero(state[..., 0] != before[..., 0]) > 100
        assert np.count_nonzero(gr[:, 8]) > 3 and np.abs(gr[:, :3]).max() > 1 and gr[OUT, 11] > 0 and gr[HALF, 11] > 0 and gr[SEAM, 11] == 0
        # ... and the layer was felt: step_bodies gives other poses
        sb, sm = bodies.copy(), motions.copy()
        oc.step_bodies_host(cascades, s, sb, sm, props, probes, float(DT), 1, it)
        assert (sm["linear"] != gm["linear"]).any()


# 2 -- several sub-steps: one call, K calls, and the host loop


@pytest.mark.parametrize("N,C,cascades,R,cell", [(64, 3, [0, 1, 2], 128, 0.5), (2048, 2, [0, 1], 64, 1.0)])
def test_bits_several_substeps(capi, oracle, N, C, cascades, R, cell):
    bodies, probes, motions, props = _bodies(N + 2, R, cell)
    K, it = 3, 4
    dt = float(DT)
    h = step64.step_size(dt, K)
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        s = _set(capi, 0)
        lay = _prime(oc, R, cell)
        wb, wm, wr = bodies, motions, None
        for _ in range(K):
            wb, wm, wr, bad = _host_substep(oc, lay, cascades, s, wb, wm, props, probes, it, h, old=wr)
            assert not bad.any()
        want_state = lay.window().copy()

        _prime(oc, R, cell)
        gb, gm = bodies.copy(), motions.copy()
        gr = oc.step_bodies_coupled_host(cascades, s, gb, gm, props, probes, dt, K, it)
        _same((gb, gm, gr), (wb, wm, wr), (N, "host loop"))
        assert np.array_equal(_bits(oc.read_ripples()), _bits(want_state))

        # K calls of one sub-step of length h: the same poses, motions and layer; fields 7 and 11 fold over the calls
        _prime(oc, R, cell)
        cb, cm, res, dropped = bodies.copy(), motions.copy(), np.zeros(len(bodies), F), np.zeros(len(bodies), F)
        for _ in range(K):
            cr = oc.step_bodies_coupled_host(cascades, s, cb, cm, props, probes, float(h), 1, it)
            res, dropped = np.fmax(res, cr[:, 7]), dropped + cr[:, 11]
        cr[:, 7], cr[:, 11] = res, dropped
        _same((gb, gm, gr), (cb, cm, cr), (N, "K calls"))
        assert np.array_equal(_bits(oc.read_ripples()), _bits(want_state))
        assert gr[OUT, 11] > cr[OUT, 11] / K and (gb["rotation"] != bodies["rotation"]).any()


# 3 -- flat ocean: the whole loop without reading anything back


def _two_boxes(gap=3.0):
    """two 4 m boxes of 81 probes (a = 0.25 m^2 each, half a metre apart: a / s^2 = 1 on cells of 0.5 m), `gap` metres between their
    sides; 10125 kg in water of rho g = 9810: the equilibrium draught is 0.5 m.  The first is dropped from 0.3 m above it, the second rests"""
    probes = _box()
    n = len(probes)
    x = 2.0 + gap / 2
    bodies = body64.make_bodies([np.eye(3)] * 2, [[-x, 0.0, -0.25 + 0.3], [x, 0.0, -0.25]], [0] * 2, [n] * 2, [np.inf] * 2)
    motions = drag64.make_motions(np.zeros((2, 3)), np.zeros((2, 3)), [500.0, 500.0], [0.0] * 2)
    props = step64.make_props([1.0 / 10125] * 2, np.full((2, 3), 1.0e-4), [9.81] * 2, [9810.0] * 2)
    return bodies, motions, props, probes


def test_flat_ocean_whole_loop(capi):
    bodies, motions, props, probes = _two_boxes()
    R, cell, K, calls, dt = 64, 0.5, 16, 4, 0.8
    with _flat(capi) as oc:
        s = _set(capi, 0, swell=False, plane_w=-0.25)
        oc.set_ripples(R, cell)
        lay = ripple64.Layer(R, cell)
        # zero maps and velocity: every record is (.., .., 0.25, 0, 0, 0, 0, ..) exactly, wherever it is taken
        pts = couple64.points32(bodies, probes)
        first = oc.read_velocity_blend([0], s, pts, 4)
        assert np.all(first[:, 2] == F(0.25)) and np.all(first[:, 3:7] == 0)
        recs = np.zeros((len(pts), 8), F)
        recs[:, 2] = 0.25
        wb, wm = bodies, motions
        gb, gm = bodies.copy(), motions.copy()
        for _ in range(calls):
            wb, wm, wr = couple64.call32(lay, wb, wm, props, probes, lambda b: recs, dt, K)
            gr = oc.step_bodies_coupled_host([0], s, gb, gm, props, probes, dt, K, 4)
            _same((gb, gm, gr), (wb, wm, wr), "flat")
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())) and np.abs(lay.eta).max() > 1e-3
        # the coupling: without it the second box, at rest in its equilibrium, stays where it is for ever
        sb, sm = bodies.copy(), motions.copy()
        for _ in range(calls):
            oc.step_bodies_host([0], s, sb, sm, props, probes, dt, K, 4)
        assert abs(float(sb["position"][1, 2]) + 0.25) < 1e-5 and np.all(sb["position"][1, :2] == bodies["position"][1, :2])
        assert gb["position"][1, 2] != sb["position"][1, 2] and abs(float(gm["linear"][1, 2])) > 1e-4
        assert np.isfinite(gr).all() and gr[1, 11] == 0


# 4 -- a layer at rest that no deposit reaches: step_bodies' poses by value


def test_outside_the_window_equals_step_bodies(capi, oracle):
    N, cascades, R, cell = 64, [0, 1, 2], 64, 1.0
    bodies, probes, motions, props = _bodies(31, R, cell)
    bodies["position"][:, 0] += 500.0
    with _moving(capi, oracle, N, 3) as oc:
        _step(oc)
        s = _set(capi, 0)
        oc.set_ripples(R, cell)
        gb, gm = bodies.copy(), motions.copy()
        gr = oc.step_bodies_coupled_host(cascades, s, gb, gm, props, probes, float(DT), 3, 4)
        sb, sm = bodies.copy(), motions.copy()
        sr = oc.step_bodies_host(cascades, s, sb, sm, props, probes, float(DT), 3, 4)
        # (== and not the bits: rec + 0 turns a -0 into +0)
        for f in ("rotation", "position"):
            assert np.array_equal(gb[f], sb[f]), f
        for f in ("linear", "angular"):
            assert np.array_equal(gm[f], sm[f]), f
        assert np.array_equal(gr[:, :8], sr) and np.all(oc.read_ripples() == 0)
        assert gr[:, 11].max() > 0 and np.all(gr[:, 11] == np.rint(gr[:, 11]))


# 5 -- repeats


def test_repeats_give_identical_bytes(capi, oracle):
    N, cascades, R, cell = 64, [0, 1, 2], 64, 1.0
    bodies, probes, motions, props = _bodies(17, R, cell)
    with _moving(capi, oracle, N, 3) as oc:
        _step(oc)
        s = _set(capi, 0)
        runs = []
        for _ in range(3):
            _prime(oc, R, cell)
            gb, gm = bodies.copy(), motions.copy()
            gr = oc.step_bodies_coupled_host(cascades, s, gb, gm, props, probes, float(DT), 4, 4)
            runs.append((gb.tobytes(), gm.tobytes(), gr.tobytes(), oc.read_ripples().tobytes()))
        assert runs[0] == runs[1] == runs[2]


# 6 -- isolation and edges; 7 -- the device entry point against the host twin


def test_isolation_edges_and_device_arrays(capi, oracle, torch):
    N, cascades, R, cell = 64, [1, 0], 64, 1.0
    C = ctypes
    bodies, probes, motions, props = _bodies(5, R, cell)
    nb, npr = len(bodies), len(probes)
    dt, sub = float(DT), 3
    with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
        _step(oc, 1)
        s = _set(capi, 0)
        lib = capi.load()
        P = capi.P
        arr = (capi.I * 2)(*cascades)
        rec = np.zeros((nb, 12), F)
        hb, hm = bodies.copy(), motions.copy()
        bp, mp, qp, pp, rp = hb.ctypes.data_as(P), hm.ctypes.data_as(P), props.ctypes.data_as(P), probes.ctypes.data_as(P), rec.ctypes.data_as(P)
        head = (arr, 2, C.byref(s), 4)
        good = head + (bp, mp, qp, nb, pp, npr, dt, sub, rp)
        names = ("datum_ocean_step_bodies_coupled_host", "datum_ocean_step_bodies_coupled")

        def unchanged(ptr0, state0):
            assert np.array_equal(_bytes(hb), _bytes(bodies)) and np.array_equal(_bytes(hm), _bytes(motions)) and np.all(rec == 0)
            assert oc.ripples_device()[0] == ptr0 and np.array_equal(_bits(oc.read_ripples()), _bits(state0))

        # ESTATE exactly where body drag returns it, the layer on: velocity off, and no displace since it was switched on; and while the
        # layer is off (that first: with the layer off nothing else is looked at).  Nothing is enqueued or written
        _prime(oc, R, cell)
        ptr0, state0 = oc.ripples_device()[0], oc.read_ripples().copy()
        for switch in (False, True):
            if switch:
                oc.set_velocity("on")
            for name in names:
                assert getattr(lib, name)(oc.h, *good) == capi.ESTATE, (name, switch)
                assert name.encode() in lib.datum_ocean_last_error(oc.h)
            unchanged(ptr0, state0)
        _step(oc, 1)
        oc.set_ripples(0)
        for name in names:
            assert getattr(lib, name)(oc.h, *good) == capi.ESTATE, name
            assert name.encode() in lib.datum_ocean_last_error(oc.h)
            assert getattr(lib, name)(oc.h, None, 0, None, 99, None, None, None, 5, None, 0, float("nan"), 0, None) == capi.ESTATE, name
        assert np.array_equal(_bytes(hb), _bytes(bodies)) and np.array_equal(_bytes(hm), _bytes(motions)) and np.all(rec == 0)

        lay = _prime(oc, R, cell)
        before = ([oc.read_maps(c).copy() for c in (0, 1)], [oc.read_velocity(c).copy() for c in (0, 1)], [oc.read_state(c).copy() for c in (0, 1)],
                  [oc.read_foam(c).copy() for c in (0, 1)])
        sb, sm = bodies.copy(), motions.copy()
        step_before = oc.step_bodies_host(cascades, s, sb, sm, props, probes, dt, sub, 4)

        # every refusal leaves the layer, its pointer and the arrays as they were
        ptr0, state0 = oc.ripples_device()[0], oc.read_ripples().copy()
        mis = lambda a, k: P(a.ctypes.data + k)
        calls = [
            (None, 2, C.byref(s), 4, bp, mp, qp, nb, pp, npr, dt, sub, rp), head + (None, mp, qp, nb, pp, npr, dt, sub, rp),
            head + (bp, mp, None, nb, pp, npr, dt, sub, rp), head + (bp, mp, qp, nb, pp, npr, dt, sub, None),
            head + (bp, mp, qp, nb, pp, npr, dt, sub, mis(rec, 4)), head + (bp, mis(hm, 8), qp, nb - 1, pp, npr, dt, sub, rp),
            head + (bp, mp, qp, nb, pp, npr, dt, 0, rp), head + (bp, mp, qp, nb, pp, npr, dt, capi.STEP_MAX_SUBSTEPS + 1, rp),
            head + (bp, mp, qp, nb, pp, npr, float("nan"), sub, rp), head + (bp, mp, qp, nb, pp, npr, float("inf"), sub, rp),
            head + (bp, mp, qp, nb, pp, npr, -dt, sub, rp),
            head + (bp, mp, qp, nb, pp, npr, 0.36 * cell * sub, sub, rp),                              # c h / s = 0.72
            head + (None, None, None, 0, None, 0, -dt, sub, None),
        ]
        for args in calls:
            for name in names:
                assert getattr(lib, name)(oc.h, *args) == capi.EINVAL, (name, args[7], args[10:12])
                assert name.encode() in lib.datum_ocean_last_error(oc.h)
        assert np.array_equal(_bytes(hb), _bytes(bodies)) and np.array_equal(_bytes(hm), _bytes(motions)) and np.all(rec == 0)
        assert oc.ripples_device()[0] == ptr0 and np.array_equal(_bits(oc.read_ripples()), _bits(state0))

        # nbodies == 0 still steps the water: step_ripples(h, 1) x substeps, from the device entry point and from the host twin
        h = step64.step_size(dt, sub)
        for name in names:
            lay = _prime(oc, R, cell)
            assert getattr(lib, name)(oc.h, *head, None, None, None, 0, None, 0, dt, sub, None) == capi.OK
            for _ in range(sub):
                lay.step(h, 1)
            assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))

        # the clean call, from host arrays
        lay = _prime(oc, R, cell)
        cb, cm = bodies.copy(), motions.copy()
        clean = oc.step_bodies_coupled_host(cascades, s, cb, cm, props, probes, dt, sub, 4)
        clean_state = oc.read_ripples().copy()
        assert np.isfinite(clean).all()

        # the device entry point: the same bytes, canaries before and after every array
        G, CAN = 64, F(-3.0e38)

        def guarded(a):
            flat = np.ascontiguousarray(a).view(F).ravel()
            t = torch.full((len(flat) + 2 * G,), float(CAN), dtype=torch.float32, device="cuda")
            t[G:G + len(flat)] = torch.from_numpy(flat.copy()).cuda()
            return t

        _prime(oc, R, cell)
        db, dm, dr = guarded(bodies), guarded(motions), guarded(np.zeros((nb, 12), F))
        dq, dp = guarded(props.view(F).reshape(nb, 8)), guarded(probes)
        torch.cuda.synchronize()
        off = G * 4
        oc.step_bodies_coupled(cascades, s, db.data_ptr() + off, dm.data_ptr() + off, dq.data_ptr() + off, nb, dp.data_ptr() + off, npr, dt, sub, dr.data_ptr() + off, 4)
        oc.sync()
        for t, want in ((db, cb), (dm, cm), (dr, clean), (dq, props), (dp, probes)):
            raw = t.cpu().numpy()
            assert np.all(raw[:G] == CAN) and np.all(raw[-G:] == CAN)
            assert np.array_equal(raw[G:-G].view(np.uint32), np.ascontiguousarray(want).view(np.uint32).ravel())
        assert np.array_equal(_bits(oc.read_ripples()), _bits(clean_state))

        # bad bodies: a bad range, motion and props keep pose and motion, give twelve NaNs and deposit nothing; a count of 0 is good
        bad, mb, qb = bodies.copy(), motions.copy(), props.copy()
        bad["cap"][8] = np.nan
        mb["linear"][10, 1] = np.inf
        qb["gravity"][12] = np.nan
        bad["count"][14] = 0
        victims = [8, 10, 12]
        lay = _prime(oc, R, cell)
        wb, wm, wr = bad, mb, None
        for _ in range(sub):
            wb, wm, wr, _bad = _host_substep(oc, lay, cascades, s, wb, wm, qb, probes, 4, h, old=wr)
        _prime(oc, R, cell)
        gb, gm = bad.copy(), mb.copy()
        gr = oc.step_bodies_coupled_host(cascades, s, gb, gm, qb, probes, dt, sub, 4)
        _same((gb, gm, gr), (wb, wm, wr), "bad bodies")
        assert np.isnan(gr[victims]).all() and np.isfinite(np.delete(gr, victims, 0)).all() and gr[14, 6] == 0
        assert np.array_equal(_bytes(gb[victims]), _bytes(bad[victims])) and np.array_equal(_bytes(gm[victims]), _bytes(mb[victims]))
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())) and not np.array_equal(_bits(lay.window()), _bits(clean_state))

        # a bad probe: its body is bad from the first sub-step on, has deposited its other probes once, and nothing after
        pb = probes.copy()
        k = int(bodies["first"][9]) + 1
        pb[k, 3] = np.nan
        f, c = bodies["first"].astype(int), bodies["count"].astype(int)
        hit = (f <= k) & (k < f + c)
        assert hit[9] and not hit.all()
        lay = _prime(oc, R, cell)
        wb, wm, wr = bodies, motions, None
        for _ in range(sub):
            pts = np.nan_to_num(couple64.points32(wb, pb))
            recs = oc.read_velocity_blend(cascades, s, pts, 4)
            wb, wm, wr, _bad = couple64.substep32(lay, wb, wm, props, pb, recs, h, samples=lay.sample(pts), old=wr)
        _prime(oc, R, cell)
        gb, gm = bodies.copy(), motions.copy()
        gr = oc.step_bodies_coupled_host(cascades, s, gb, gm, props, pb, dt, sub, 4)
        _same((gb, gm, gr), (wb, wm, wr), "bad probe")
        assert np.isnan(gr[hit]).all() and np.array_equal(_bytes(gb[hit]), _bytes(bodies[hit]))
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))

        # a body that turns bad in its second sub-step, in the middle of the window, three sub-steps.  It moves at 2 m/s with a huge
        # quadratic drag and a mass sized from its own drag record so that the first sub-step throws it back at about 1500 m/s (8 m:
        # still inside the window); in the second the drag of that speed is not a float any more, the state is not finite, and memory
        # keeps the first sub-step's pose.  In both it has deposited; in the third it walks nothing and deposits nothing
        k = 2
        late_b, late_m, qb = bodies.copy(), motions.copy(), props.copy()
        centre = (np.array(ORIGIN) + R // 2) * cell
        late_b["rotation"][k], late_b["position"][k] = np.eye(3).ravel(), (centre[0], centre[1], -0.5)
        late_m["linear"][k], late_m["angular"][k], late_m["cl"][k], late_m["cq"][k] = (2.0, 0, 0), 0, 0, 1.0e34
        force = oc.read_body_drag(cascades, s, late_b, late_m, probes, 4)[k, :3].astype(np.float64)
        assert np.isfinite(force).all() and np.linalg.norm(force) > 1e34
        qb["invmass"][k], qb["invinertia"][k] = 1500.0 / (float(h) * np.linalg.norm(force)), 0.0
        for revive in (False, True):
            lay = _prime(oc, R, cell)
            wb, wm, wr, bads = late_b, late_m, None, []
            for i in range(sub):
                if revive and i == 2:
                    wr = wr.copy()
                    wr[k] = 0                                            # (planted: the third sub-step does not see that the body went bad)
                wb, wm, wr, wbad = _host_substep(oc, lay, cascades, s, wb, wm, qb, probes, 4, h, old=wr)
                bads.append(bool(wbad[k]))
                if i == 0:
                    first_pose = wb[k].copy()
            if revive:
                revived = lay.window().copy()
            else:
                want = (wb, wm, wr, lay.window().copy())
                assert bads == [False, True, True], bads
        assert np.abs(first_pose["position"][:2] - centre).max() < R * cell / 2 - 8 and first_pose["position"][0] != late_b["position"][k, 0]
        _prime(oc, R, cell)
        gb, gm = late_b.copy(), late_m.copy()
        gr = oc.step_bodies_coupled_host(cascades, s, gb, gm, qb, probes, dt, sub, 4)
        _same((gb, gm, gr), want[:3], "bad in sub-step 2")
        assert np.isnan(gr[k]).all() and _bytes(gb)[k].tobytes() == first_pose.tobytes()
        state = oc.read_ripples()
        assert np.array_equal(_bits(state), _bits(want[3])) and not np.array_equal(_bits(state), _bits(revived))

        # the calls left the maps, the velocity planes, the phase and step_bodies' own results as they were
        for c in (0, 1):
            assert np.array_equal(_bits(before[0][c]), _bits(oc.read_maps(c)))
            assert np.array_equal(_bits(before[1][c]), _bits(oc.read_velocity(c)))
            assert np.array_equal(_bits(before[2][c]), _bits(oc.read_state(c)))
            assert np.array_equal(_bits(before[3][c]), _bits(oc.read_foam(c)))
        sb2, sm2 = bodies.copy(), motions.copy()
        step_after = oc.step_bodies_host(cascades, s, sb2, sm2, props, probes, dt, sub, 4)
        assert np.array_equal(_bits(step_after), _bits(step_before)) and np.array_equal(_bytes(sb2), _bytes(sb)) and np.array_equal(_bytes(sm2), _bytes(sm))


# 7 -- the C++ shim


def test_cpp_shim_matches_capi(capi):
    from datum_amd import host_api

    N, R, cell = 256, 64, 1.0
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.4))
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    bodies, probes, motions, props = _bodies(13, R, cell, origin=(-R // 2, -R // 2))
    with host_api.OceanContext(N) as ctx:
        ctx.set_velocity("on")
        for _ in range(2):
            params.update_ocean(DT)
            ctx.displace_ocean_surface(params)
        with pytest.raises(Exception):
            ctx.step_ocean_bodies_coupled(params, bodies.copy(), motions.copy(), props, probes, float(DT), 2, 4)      # the layer is off
        lib = capi.load()
        h = ctx.lib.datum_host_context_handle(ctx.c)
        one = (capi.I * 1)(0)
        P = capi.P
        state = np.empty((R, R, 2), F)
        for sub in (1, 4):
            ctx.set_ocean_ripples(R, cell)
            gb, gm = bodies.copy(), motions.copy()
            got = ctx.step_ocean_bodies_coupled(params, gb, gm, props, probes, float(DT), sub, 4)
            assert lib.datum_ocean_read_ripples(h, state.ctypes.data_as(P)) == capi.OK
            got_state = state.copy()
            ctx.set_ocean_ripples(R, cell)
            s = params.oceanset(camera)
            wb, wm, want = bodies.copy(), motions.copy(), np.empty_like(got)
            assert lib.datum_ocean_step_bodies_coupled_host(h, one, 1, ctypes.byref(s), 4, wb.ctypes.data_as(P), wm.ctypes.data_as(P), props.ctypes.data_as(P), len(bodies),
                                                            probes.ctypes.data_as(P), len(probes), float(DT), sub, want.ctypes.data_as(P)) == capi.OK
            assert lib.datum_ocean_read_ripples(h, state.ctypes.data_as(P)) == capi.OK
            _same((gb, gm, got), (wb, wm, want), sub)
            assert np.array_equal(_bits(got_state), _bits(state)) and np.abs(state).max() > 0
            assert got.shape == (len(bodies), 12) and np.isfinite(got).all() and np.abs(got[:, :3]).max() > 0
