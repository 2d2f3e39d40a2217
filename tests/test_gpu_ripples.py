"""The ripple layer (include/datum_ocean_hip.h: "ripple layer") on the MI355X, against tests/ripple64.py.

R = 64 is one tile of the step kernel across and four down, R = 128 two across and eight down; with the origin (37, -21) the window wraps
the torus inside a tile, in both directions.  The layer has no entry point that writes its state or reads its src plane, and the tests
need none: a state is made by deposits and steps, and a step of dt = 0 turns src into heights exactly (e = 0 + float(src) 2^-20, the rate
and the height's increment are products with 0), so read_ripples after it IS the src plane while |src| < 2^24.

  step      bit for bit against the fp32 restatement after 1, 3 and 16 sub-steps, from a state that earlier random deposits and steps left
            and with random deposits pending, the sponge on (B = 8) and off; one leg with a single cell in each corner and on each edge;
            a second step without deposits (src was cleared); within K_RIP eps max|eta| of float64;
  scroll    center by (+5, -3) cells, by exactly R, and back; a layer whose centre moves every step against one that never moves: a
            sub-step carries a disturbance one cell (the stencil reaches the four neighbours), so after n sub-steps two runs agree bit for
            bit in every cell further than n cells from every border cell that ever differed -- the n-cell light cone;
  deposits  impulses and the wake: the src plane exact, the records bit for bit; sampler; isolation; canaries.
"""

import ctypes

import numpy as np
import pytest

import body64
import drag64
import ripple64
from test_gpu_body import _fleet, _step
from test_gpu_surface import DT, _set, _setup

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -24
ORIGIN = (37, -21)
CANARY = 0x7FC0DEAD


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


def _plain(capi, N=64):
    oc = capi.Ocean(N, 1)
    oc.set_cascade(0, 22.0, 1.35)
    oc.upload_state(0, np.zeros((N, N, 2), F))
    return oc


def _layer(oc, R, s, B, origin=ORIGIN, dtype=F, gamma=0.05):
    """the handle's layer and its restatement, both with the window's origin at `origin`"""
    oc.set_ripple_params(2.0, gamma, B, 4.0)
    oc.set_ripples(R, s)
    lay = ripple64.Layer(R, s, dtype, 2.0, gamma, B, 4.0)
    x, y = (origin[0] + R // 2 + 0.5) * s, (origin[1] + R // 2 + 0.5) * s
    oc.center_ripples(x, y)
    lay.center(x, y)
    assert (lay.ox, lay.oy) == origin and oc.ripples_device()[2:] == origin
    return lay


def _impulses(rng, lay, n, volume=0.02):
    """n deposits over the window and a margin of four cells round it"""
    s, R = float(lay.s), lay.R
    imp = np.zeros((n, 4), F)
    imp[:, 0] = rng.uniform((lay.ox - 4) * s, (lay.ox + R + 4) * s, n)
    imp[:, 1] = rng.uniform((lay.oy - 4) * s, (lay.oy + R + 4) * s, n)
    imp[:, 2] = rng.normal(size=n) * volume
    return imp


def _deposit(oc, torch, imp):
    d = torch.from_numpy(np.ascontiguousarray(imp, F)).cuda()
    oc.deposit_ripples(d.data_ptr(), len(imp))
    return d


def _src_plane(oc):
    """the pending deposits in window order: a step of dt = 0 from rest (module docstring)"""
    st = oc.read_ripples()
    assert np.all(st == 0)
    oc.step_ripples(0.0, 1)
    st = oc.read_ripples()
    assert np.all(st[..., 1] == 0)
    q = st[..., 0].astype(np.float64) * 2.0 ** 20
    assert np.all(q == np.rint(q)) and np.abs(q).max() < 2 ** 24
    return q.astype(np.int64)


# -- step


@pytest.mark.parametrize("R,B", [(64, 8), (64, 0), (128, 8), (128, 0)])
def test_step_bits(capi, torch, report, R, B):
    rng = np.random.default_rng(R + B)
    s = 0.5
    with _plain(capi) as oc:
        lay = _layer(oc, R, s, B)
        l64 = ripple64.Layer(R, s, np.float64, 2.0, 0.05, B, 4.0)
        l64.move(*ORIGIN)
        keep = []
        worst = 0.0
        for substeps in (1, 3, 16):
            imp = _impulses(rng, lay, 4 * R * R)
            keep.append(_deposit(oc, torch, imp))
            lay.deposit(imp)
            # (K_RIP bounds one call from a common fp32 state: float64 starts where the restatement stands)
            l64.eta, l64.rate, l64.src = lay.eta.astype(np.float64), lay.rate.astype(np.float64), lay.src.copy()
            assert np.count_nonzero(lay.src) > 0.9 * R * R
            oc.step_ripples(0.1 * substeps, substeps)
            lay.step(0.1 * substeps, substeps)
            l64.step(0.1 * substeps, substeps)
            got = oc.read_ripples()
            assert np.array_equal(_bits(got), _bits(lay.window())), (R, B, substeps, np.argwhere(_bits(got) != _bits(lay.window()))[:4])
            # a second step without deposits: src was cleared behind the first sub-step
            err = np.abs(got[..., 0].astype(np.float64) - l64.window()[..., 0]).max() / (EPS * np.abs(l64.eta).max())
            worst = max(worst, err)
            oc.step_ripples(0.1, 2)
            lay.step(0.1, 2)
            got = oc.read_ripples()
            assert np.array_equal(_bits(got), _bits(lay.window())), (R, B, substeps, "second")
        line = f"ripples R={R} B={B}: |device - float64| / (eps max|eta|) = {worst:.2f}, K_RIP = {ripple64.K_RIP}"
        print(line)
        report(line)
        assert np.abs(got[..., 0]).max() > 1e-3
        assert worst <= ripple64.K_RIP


@pytest.mark.parametrize("R", [64, 128])
def test_step_corners_and_edges(capi, torch, R):
    s = 0.5
    ox, oy = ORIGIN
    cells = [(0, 0), (R - 1, 0), (0, R - 1), (R - 1, R - 1), (R // 2, 0), (R // 2, R - 1), (0, R // 3), (R - 1, R // 3)]
    with _plain(capi) as oc:
        lay = _layer(oc, R, s, 8)
        imp = np.zeros((len(cells), 4), F)
        for k, (i, j) in enumerate(cells):
            imp[k] = ((ox + i + 0.5) * s, (oy + j + 0.5) * s, 0.25 * (k + 1), 0)
        d = _deposit(oc, torch, imp)
        assert lay.deposit(imp).sum() == 0 and np.count_nonzero(lay.src) == len(cells)
        for substeps in (1, 3, 16):
            oc.step_ripples(0.1 * substeps, substeps)
            lay.step(0.1 * substeps, substeps)
            got = oc.read_ripples()
            assert np.array_equal(_bits(got), _bits(lay.window())), (R, substeps, np.argwhere(_bits(got) != _bits(lay.window()))[:4])
        assert np.count_nonzero(got[..., 0]) > 8 * len(cells)
        del d


# -- scroll


@pytest.mark.parametrize("R", [64, 128])
def test_scroll(capi, torch, R):
    rng = np.random.default_rng(R)
    s = 0.5
    with _plain(capi) as oc:
        lay = _layer(oc, R, s, 8)
        keep = [_deposit(oc, torch, imp) for imp in [_impulses(rng, lay, 2 * R * R)]]
        lay.deposit(np.asarray(keep[0].cpu()))
        oc.step_ripples(0.2, 2)
        lay.step(0.2, 2)
        cx, cy = (lay.ox + R // 2 + 0.5) * s, (lay.oy + R // 2 + 0.5) * s
        for dx, dy in [(5, -3), (R, 0), (-5, 3)]:
            before = oc.read_ripples()
            ox0, oy0 = oc.ripples_device()[2:]
            cx, cy = cx + dx * s, cy + dy * s
            oc.center_ripples(cx, cy)
            lay.center(cx, cy)
            ox1, oy1 = oc.ripples_device()[2:]
            assert (ox1 - ox0, oy1 - oy0) == (dx, dy) and (lay.ox, lay.oy) == (ox1, oy1)
            after = oc.read_ripples()
            # surviving cells keep their bits, entered cells are zero
            world = np.zeros((R, R, 2), F)
            i = np.arange(R)
            si, sj = i + ox1 - ox0, i + oy1 - oy0                      # the cell's index in the old window
            okx, oky = (si >= 0) & (si < R), (sj >= 0) & (sj < R)
            world[np.ix_(oky, okx)] = before[np.ix_(sj[oky], si[okx])]
            assert np.array_equal(_bits(after), _bits(world)), (dx, dy)
            assert np.array_equal(_bits(after), _bits(lay.window()))
            if abs(dx) < R:
                assert np.count_nonzero(after) > 0
            else:
                assert np.count_nonzero(after) == 0
            imp = _impulses(rng, lay, R * R)
            keep.append(_deposit(oc, torch, imp))
            lay.deposit(imp)
            oc.step_ripples(0.3, 3)
            lay.step(0.3, 3)
            assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())), (dx, dy, "stepped")


def test_moving_centre_equals_fixed_inside_the_light_cone(capi, torch):
    """B = 0, one deposit pattern in the middle; layer A never moves, layer B's centre moves one cell right every step.  The windows'
    contents differ only through the border (the zero neighbour stands one cell further right for B, and B lost a column on the left and
    gained one at rest), so after n sub-steps in all a cell can differ only within n cells of a border: everywhere else the bits agree"""
    R, s, steps, sub = 64, 0.5, 6, 2
    rng = np.random.default_rng(3)
    imp = np.zeros((64, 4), F)
    imp[:, 0] = rng.uniform(-4, 4, 64)
    imp[:, 1] = rng.uniform(-4, 4, 64)
    imp[:, 2] = rng.normal(size=64)
    out = []
    for moving in (False, True):
        with _plain(capi) as oc:
            oc.set_ripple_params(2.0, 0.05, 0, 0.0)
            oc.set_ripples(R, s)
            d = _deposit(oc, torch, imp)
            for k in range(steps):
                oc.step_ripples(0.2, sub)
                if moving:
                    oc.center_ripples((k + 1.5) * s, 0.25)
            out.append((oc.read_ripples(), oc.ripples_device()[2:]))
            del d
    (a, (ax, ay)), (b, (bx, by)) = out
    assert (bx - ax, by - ay) == (steps, 0)
    n = steps * sub
    # world cells further than n from both windows' borders
    i0, i1 = bx + n + 1, ax + R - n - 1
    j0, j1 = ay + n + 1, ay + R - n - 1
    A = a[j0 - ay:j1 - ay, i0 - ax:i1 - ax]
    B = b[j0 - by:j1 - by, i0 - bx:i1 - bx]
    assert A.size > 0 and np.abs(A).max() > 1e-4
    assert np.array_equal(_bits(A), _bits(B))


# -- deposits


def test_impulses_exact_and_repeatable(capi, torch):
    R, s, n = 64, 0.5, 4096
    rng = np.random.default_rng(9)
    planes = []
    for run in range(3):
        with _plain(capi) as oc:
            lay = _layer(oc, R, s, 8)
            if run == 0:
                imp = _impulses(rng, lay, n, volume=0.05)
                imp[::7, :2] = imp[3, :2]                                # many on the same cell
                imp[5::97, 0] = (lay.ox - 40) * s                        # some well outside
                imp[11::101, 0], imp[13::103, 1], imp[17::107, 2] = np.nan, np.inf, np.nan
                imp[19::109, 0] = 3e30
                imp[23, 2] = 1e30                                        # clamped to 2^30 units
                imp[23, :2] = ((lay.ox + 0.5) * s, (lay.oy + 0.5) * s)
            dropped = lay.deposit(imp)
            assert dropped.sum() > 0
            # (the third run through the host twin)
            d = _deposit(oc, torch, imp) if run < 2 else oc.deposit_ripples_host(imp)
            st0 = oc.read_ripples()
            assert np.all(st0 == 0)
            oc.step_ripples(0.0, 1)
            got = oc.read_ripples()
            del d
            want = np.roll(lay.src, (-(lay.oy & (R - 1)), -(lay.ox & (R - 1))), (0, 1))
            assert want[0, 0] >= 2 ** 29
            # (float(src) 2^-20 is one rounding of an integer: compared as such, and exactly where |src| < 2^24)
            assert np.array_equal(_bits(got[..., 0]), _bits(want.astype(F) * ripple64.UNIT))
            assert np.all(got[..., 1] == 0)
            planes.append(got)
    assert np.array_equal(_bits(planes[0]), _bits(planes[1])) and np.array_equal(_bits(planes[0]), _bits(planes[2]))


def _bodies_inside(seed, nb=8, per=64):
    """nb bodies of `per` probes each, within 20 m of the origin: well inside a 128-cell window of 1 m cells round it"""
    bodies, probes = _fleet(seed, nbodies=nb, nprobes=nb * per, counts=[per] * nb)
    rng = np.random.RandomState(seed)
    bodies["position"][:, :2] = rng.uniform(-20, 20, (nb, 2))
    bodies["position"][:, 2] = rng.uniform(-1.0, 0.5, nb)
    motions = drag64.make_motions(rng.uniform(-3, 3, (nb, 3)), rng.uniform(-1, 1, (nb, 3)), np.ones(nb), np.ones(nb))
    return bodies, motions, probes


G = 16                       # guard floats before and after every device output array (64 bytes: the arrays keep their alignment)


def _guarded(torch, floats):
    """a device array of `floats` floats with G canary words before and after it: (tensor, pointer to the array)"""
    t = torch.zeros(floats + 2 * G, dtype=torch.float32, device="cuda")
    t.view(torch.int32)[:] = CANARY
    torch.cuda.synchronize()
    return t, t.data_ptr() + 4 * G


def _unguard(t, floats):
    raw = t.cpu().numpy()
    assert np.all(raw[:G].view(np.int32) == CANARY) and np.all(raw[G + floats:].view(np.int32) == CANARY)
    return raw[G:G + floats]


def _wake(oc, torch, cascades, s, bodies, motions, probes, dt, it=4):
    nb = len(bodies)
    db = torch.from_numpy(bodies.view(np.uint8).reshape(nb, 64).copy()).cuda()
    dm = torch.from_numpy(motions.view(np.uint8).reshape(nb, 32).copy()).cuda()
    dp = torch.from_numpy(np.ascontiguousarray(probes, F)).cuda()
    rec, ptr = _guarded(torch, nb * 8)
    oc.deposit_body_ripples(cascades, s, db.data_ptr(), dm.data_ptr(), nb, dp.data_ptr(), len(probes), dt, ptr, it)
    oc.read_ripples()                                                    # waits for the handle's stream
    return _unguard(rec, nb * 8).reshape(nb, 8).copy()


def test_body_wake(capi, oracle, torch):
    N, cascades, R, cell, dt = 64, [0, 1], 128, 1.0, 0.05
    bodies, motions, probes = _bodies_inside(4)
    with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
        s = _set(capi, 0)
        oc.set_ripples(R, cell)
        lib = capi.load()
        # ESTATE exactly where body drag returns it: velocity off, and no displace since it was switched on
        P, C = capi.P, ctypes
        rec = np.zeros((8, 8), F)
        args = ((capi.I * 2)(*cascades), 2, C.byref(s), 4, bodies.ctypes.data_as(P), motions.ctypes.data_as(P), 8, probes.ctypes.data_as(P), len(probes), dt, rec.ctypes.data_as(P))
        _step(oc, 1)
        assert lib.datum_ocean_deposit_body_ripples(oc.h, *args) == capi.ESTATE
        assert b"datum_ocean_deposit_body_ripples" in lib.datum_ocean_last_error(oc.h)
        oc.set_velocity("on")
        assert lib.datum_ocean_deposit_body_ripples(oc.h, *args) == capi.ESTATE
        _step(oc)

        lay = ripple64.Layer(R, cell)
        w, _, bad = body64.world32(bodies, probes)
        assert not bad.any() and np.abs(w[:, :2]).max() < 40
        recs = oc.read_velocity_blend(cascades, s, np.ascontiguousarray(w[:, :2]), 4)
        want = ripple64.wake32(bodies, motions, probes, recs, dt, lay.src, lay.ox, lay.oy, lay.invs)
        got = _wake(oc, torch, cascades, s, bodies, motions, probes, dt)
        assert np.isfinite(got).all() and np.abs(got[:, 0]).max() > 0 and np.abs(got[:, 1:3]).max() > 0 and np.all(got[:, 3:6] == 0)
        assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:4]
        lift = oc.read_bodies(cascades, s, bodies, probes, 4)
        assert np.array_equal(_bits(got[:, 6]), _bits(lift[:, 0]))
        plane = _src_plane(oc)
        assert np.count_nonzero(plane) > 100
        assert np.array_equal(plane, lay.window(lay.src).astype(np.int64))

        # the host twin: the same records and the same plane
        oc.reset_ripples()
        host = oc.deposit_body_ripples_host(cascades, s, bodies, motions, probes, dt)
        assert np.array_equal(_bits(host), _bits(got)) and np.array_equal(_src_plane(oc), plane)

        # one bad body and one bad motion deposit nothing and give NaNs; the others as before
        oc.reset_ripples()
        b2, m2 = bodies.copy(), motions.copy()
        b2["cap"][2] = np.nan
        m2["linear"][5, 1] = np.inf
        lay2 = ripple64.Layer(R, cell)
        live = body64._gather(bodies, probes)[0] != 2                      # (a body with a bad range has no rows in the restatement)
        want2 = ripple64.wake32(b2, m2, probes, recs[live], dt, lay2.src, lay2.ox, lay2.oy, lay2.invs)
        got2 = _wake(oc, torch, cascades, s, b2, m2, probes, dt)
        assert np.isnan(got2[[2, 5]]).all() and np.isnan(want2[[2, 5]]).all()
        rest = [0, 1, 3, 4, 6, 7]
        assert np.array_equal(_bits(got2[rest]), _bits(got[rest]))
        plane2 = _src_plane(oc)
        assert np.array_equal(plane2, lay2.window(lay2.src).astype(np.int64)) and not np.array_equal(plane2, plane)


def test_body_at_rest_on_flat_water_deposits_nothing(capi, torch):
    N, R = 64, 128
    bodies, motions, probes = _bodies_inside(6)
    motions["linear"][:], motions["angular"][:] = 0, 0
    with _plain(capi, N) as oc:
        oc.set_velocity("on")
        oc.update(DT)
        oc.displace()
        oc.set_ripples(R, 1.0)
        s = _set(capi, 0, swell=False, plane_w=-0.25)
        got = _wake(oc, torch, [0], s, bodies, motions, probes, 0.05)
        assert np.all(got[:, :6] == 0) and got[:, 6].max() > 0
        assert np.all(_src_plane(oc) == 0)


# -- sampler


@pytest.mark.parametrize("R", [64, 128])
def test_sampler(capi, torch, R):
    rng = np.random.default_rng(R + 1)
    s = 0.5
    with _plain(capi) as oc:
        lay = _layer(oc, R, s, 8)
        imp = _impulses(rng, lay, 2 * R * R)
        d = _deposit(oc, torch, imp)
        lay.deposit(imp)
        oc.step_ripples(0.3, 3)
        lay.step(0.3, 3)
        x0, y0, x1, y1 = lay.ox * s, lay.oy * s, (lay.ox + R) * s, (lay.oy + R) * s
        pts = [np.stack([rng.uniform(x0 - 3, x1 + 3, 2000), rng.uniform(y0 - 3, y1 + 3, 2000)], 1)]
        ci = rng.integers(0, R, (200, 2))
        pts.append(np.stack([(lay.ox + ci[:, 0] + 0.5) * s, (lay.oy + ci[:, 1] + 0.5) * s], 1))                  # cell centres
        t = rng.uniform(y0, y1, 50)
        pts += [np.stack([np.full(50, v), t], 1) for v in (x0, x1, x0 + 0.25, x1 - 0.25)]                       # the window's edges
        pts += [np.stack([rng.uniform(x0, x1, 50), np.full(50, v)], 1) for v in (y0, y1, y0 + 0.25, y1 - 0.25)]
        pts.append(np.array([[1e6, 0], [0, -1e6], [3e30, 0], [np.nan, 0], [0, np.inf], [-np.inf, np.nan]]))
        p = np.concatenate(pts).astype(F)
        want = lay.sample(p)
        got = oc.query_ripples(p)
        nan = np.isnan(want)
        assert nan[-3:].all() and not nan[:-3].any() and np.all(want[-6:-3] == 0)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), np.argwhere(_bits(got) != _bits(want))[:4]
        centres = got[2000:2200]
        assert np.array_equal(_bits(centres[:, 0]), _bits(lay.window()[ci[:, 1], ci[:, 0], 0]))
        # device arrays, canaries before and after the samples
        dp = torch.from_numpy(p).cuda()
        out, ptr = _guarded(torch, len(p) * 4)
        oc.sample_ripples(dp.data_ptr(), len(p), ptr)
        oc.read_ripples()
        o = _unguard(out, len(p) * 4)
        assert np.array_equal(_bits(o.reshape(-1, 4))[~nan], _bits(want)[~nan])
        del d


# -- isolation


def test_isolation(capi, oracle, torch):
    """with the layer on, fed and stepped, every map, phase, foam and velocity value and a step_bodies result are those of a handle
    without it"""
    N, cascades = 64, [0, 1]
    bodies, motions, probes = _bodies_inside(8)
    props = np.zeros(len(bodies), capi.BODY_PROPS_DTYPE)
    props["invmass"], props["invinertia"], props["gravity"], props["buoyancy"] = 0.01, 0.01, 9.81, 9810.0
    out = []
    for on in (False, True):
        with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
            oc.set_velocity("on")
            s = _set(capi, 0)
            if on:
                oc.set_ripples(128, 1.0)
            for k in range(3):
                _step(oc, 1)
                if on:
                    _wake(oc, torch, cascades, s, bodies, motions, probes, 0.05)
                    oc.step_ripples(0.05, 2)
                    oc.center_ripples(float(k), 0.0)
            b, m = bodies.copy(), motions.copy()
            rec = oc.step_bodies_host(cascades, s, b, m, props, probes, 0.02, 2)
            out.append([oc.read_maps(c) for c in cascades] + [oc.read_foam(c) for c in cascades] + [oc.read_velocity(c) for c in cascades]
                       + [oc.read_state(c) for c in cascades] + [rec, b.view(np.uint8), m.view(np.uint8)])
            if on:
                assert np.abs(oc.read_ripples()).max() > 0
    for x, y in zip(*out):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


# -- the off state and the refusals that need a device


def test_off_and_refusals(capi):
    with _plain(capi) as oc:
        lib = capi.load()
        s = _set(capi, 0)
        bodies, motions, probes = _bodies_inside(1, nb=2, per=4)
        # every call that needs the layer, its host twins among them, whatever else holds (here velocity is off as well: the layer first)
        for call in (lambda: oc.center_ripples(0, 0), oc.reset_ripples, oc.ripples_device, oc.read_ripples, lambda: oc.step_ripples(0.1, 1),
                     lambda: oc.deposit_ripples(None, 0), lambda: oc.deposit_ripples_host(np.zeros((1, 4), F)), lambda: oc.sample_ripples(None, 0, None),
                     lambda: oc.query_ripples(np.zeros((1, 2), F)), lambda: oc.deposit_body_ripples([0], s, None, None, 0, None, 0, 0.05, None),
                     lambda: oc.deposit_body_ripples_host([0], s, bodies, motions, probes, 0.05)):
            with pytest.raises(capi.OceanError) as e:
                call()
            assert e.value.code == capi.ESTATE and "ripple layer is off" in str(e.value)
        for R, s in [(63, 0.5), (2048, 0.5), (-64, 0.5), (64, 0.0), (64, -1.0), (64, float("inf")), (64, float("nan"))]:
            assert lib.datum_ocean_set_ripples(oc.h, R, s) == capi.EINVAL and b"datum_ocean_set_ripples" in lib.datum_ocean_last_error(oc.h)
        for args in [(0.0, 0.05, 8, 4.0), (-1.0, 0.05, 8, 4.0), (float("nan"), 0.05, 8, 4.0), (2.0, -0.1, 8, 4.0), (2.0, float("inf"), 8, 4.0), (2.0, 0.05, -1, 4.0),
                     (2.0, 0.05, 65, 4.0), (2.0, 0.05, 8, -1.0), (2.0, 0.05, 8, float("nan"))]:
            assert lib.datum_ocean_set_ripple_params(oc.h, *args) == capi.EINVAL and b"datum_ocean_set_ripple_params" in lib.datum_ocean_last_error(oc.h)
        oc.set_ripple_params(2.0, 0.0, 0, 0.0)
        oc.set_ripple_params(2.0, 0.05, 64, 4.0)
        oc.set_ripple_params()
        with pytest.raises(capi.OceanError) as e:
            oc.read_ripples()
        assert e.value.code == capi.ESTATE
        oc.set_ripples(64, 0.5)
        assert oc.ripples_device()[1:] == (64 * 64 * 8, -32, -32) and np.all(oc.read_ripples() == 0)
        assert lib.datum_ocean_step_ripples(oc.h, 0.2, 1) == capi.EINVAL and b"stability" in lib.datum_ocean_last_error(oc.h)   # c h / s = 0.8
        oc.step_ripples(0.2, 2)
        for dt, sub in [(0.1, 0), (0.1, 17), (np.nan, 1), (np.inf, 1), (-0.1, 1), (-1e-9, 4)]:
            assert lib.datum_ocean_step_ripples(oc.h, float(dt), sub) == capi.EINVAL and b"datum_ocean_step_ripples" in lib.datum_ocean_last_error(oc.h)
        assert lib.datum_ocean_center_ripples(oc.h, float('nan'), 0.0) == capi.EINVAL and lib.datum_ocean_center_ripples(oc.h, 0.0, 1e30) == capi.EINVAL
        a, b = oc.ripples_device()[0], None
        oc.step_ripples(0.1, 1)
        b = oc.ripples_device()[0]
        oc.step_ripples(0.1, 1)
        assert a != b and oc.ripples_device()[0] == a                    # the pointer alternates
        oc.set_ripples(0)
        with pytest.raises(capi.OceanError):
            oc.read_ripples()


# -- the C++ shim


def test_cpp_shim_reaches_the_same_bits(capi, torch):
    """set, center, the two deposits, step and query through datum_amd/host against the same sequence through the C ABI's device-array
    calls on the same handle: the state, the wake's records and the samples, bit for bit; the impulse leg against the restatement too"""
    from datum_amd import host_api

    N, R, cell, dt = 256, 128, 0.5, 0.05
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.4))
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    bodies, motions, probes = _bodies_inside(12)
    rng = np.random.default_rng(12)
    pts = rng.uniform(-40, 40, (500, 2)).astype(F)
    with host_api.OceanContext(N) as ctx:
        with pytest.raises(Exception):
            ctx.step_ocean_ripples(dt, 2)                                # the layer is off
        ctx.set_velocity("on")
        for _ in range(2):
            params.update_ocean(DT)
            ctx.displace_ocean_surface(params)
        # the shim's own handle behind a capi.Ocean that does not own it
        oc = capi.Ocean.__new__(capi.Ocean)
        oc.lib, oc.h, oc.N, oc.cascades = capi.load(), ctx.lib.datum_host_context_handle(ctx.c), N, 1
        try:
            _shim_legs(capi, torch, ctx, oc, params.oceanset(camera), params, R, cell, dt, bodies, motions, probes, rng, pts)
        finally:
            oc.h = None


def _shim_legs(capi, torch, ctx, oc, s, params, R, cell, dt, bodies, motions, probes, rng, pts):
    if True:

        ctx.set_ocean_ripples(R, cell)
        ctx.center_ocean_ripples(3.3, -2.2)
        lay = ripple64.Layer(R, cell)
        lay.center(3.3, -2.2)
        assert oc.ripples_device()[2:] == (lay.ox, lay.oy)
        imp = _impulses(rng, lay, 2000)
        ctx.deposit_ocean_ripples(imp)
        lay.deposit(imp)
        ctx.step_ocean_ripples(dt * 3, 3)
        lay.step(dt * 3, 3)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))
        rec = ctx.deposit_ocean_body_ripples(params, bodies, motions, probes, dt)
        ctx.step_ocean_ripples(dt * 2, 2)
        state = oc.read_ripples()
        samples = ctx.query_ocean_ripples(pts)
        assert np.isfinite(rec).all() and np.abs(rec[:, :3]).max() > 0 and np.abs(samples).max() > 0

        # the same through the C ABI's device calls
        oc.reset_ripples()
        d = _deposit(oc, torch, imp)
        oc.step_ripples(dt * 3, 3)
        want_rec = _wake(oc, torch, [0], s, bodies, motions, probes, dt)
        oc.step_ripples(dt * 2, 2)
        assert np.array_equal(_bits(rec), _bits(want_rec))
        assert np.array_equal(_bits(state), _bits(oc.read_ripples()))
        assert np.array_equal(_bits(samples), _bits(oc.query_ripples(pts)))
        del d
        ctx.set_ocean_ripples(0, 0.0)
        with pytest.raises(Exception):
            ctx.query_ocean_ripples(pts)
