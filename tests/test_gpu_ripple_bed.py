"""The ripple bed (include/datum_ocean_hip.h: "ripple bed") on the MI355X, through the C ABI, against tests/ripple_bed64.py.

R = 64 is one tile of the step kernel across, R = 128 has tile seams in both directions (memory x 63|64, y 15|16 ...); with the origin
(37, -21) the window wraps the torus inside a tile, with (0, 0) on a tile's edge.  The bed is tests/test_ripple_bed_emul.py's `shore`: a
map smaller than the window, a beach whose shoreline crosses the torus seam, an island, a surf zone; `piers` are walls over it.

  planes    both bit for bit against numpy after set_ripple_bed, a center_ripples of a few cells, one of R cells or more, set_ripple_walls
            after the bed (it rasters the bed again), walls off again; a null bed -> the getter returns nulls; guards whole;
  steps     bit for bit against the fp32 restatement after 1, 3 and 16 sub-steps, B = 8 with the surf zone and B = 0 without, walls on
            and off, within K_RIP_BED of float64; deposits on solid cells and on the water beside them (those on solid cells are lost);
            the buffer a sub-step reads and both planes keep their bits (and a raster from the map afterwards gives them again: the map
            is untouched); the planes' four guards and the state buffers' four stay whole;
  zeroing   set_ripple_bed leaves +0 in both state buffers at every solid cell and every other cell as it was;
  off       a bed set and removed gives the bits of a handle that never had one, in both modes;
  coupled   step_bodies_coupled over a bed against couple64's loop over the restatement, nbodies == 0 included;
  bounds    the CURRENT mark is cleared by set_ripple_bed; maps, wake foam and src are untouched by the new calls;
  refusals  the stability bound at sqrt(g max_depth), the two DEEP refusals, a non-finite map value, the record's ranges; the C++ shim.
"""

import numpy as np
import pytest

import couple64
import ripple_bed64 as rb
import ripple_deep64 as rd
import ripple_wall64 as rw
from test_gpu_couple import _same, _two_boxes
from test_gpu_ripple_deep import _both_guards_whole, _guards_whole
from test_gpu_ripple_foam import _peek
from test_gpu_ripple_walls import _plane_guards_whole
from test_gpu_ripples import ORIGIN, _deposit, _impulses, _plain
from test_gpu_step import _flat
from test_gpu_surface import _set
from test_ripple_bed_emul import piers, shore

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -24
S = 0.5
H = 0.1
BGUARD = 64                   # 32-bit words of 0xCD bytes the handle keeps before and after each of the bed's planes


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


@pytest.fixture(scope="module")
def table(capi):
    G = np.zeros((rd.Q, rd.Q), F)
    assert capi.load().datum_ocean_ripple_deep_weights(G.ctypes.data_as(capi.P)) == capi.OK
    return G


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _layer(oc, table, R, B, origin, dtype=F, mode=rb.WAVE):
    oc.set_ripple_params(2.0, 0.05, B, 4.0)
    oc.set_ripple_dispersion(mode, 9.81)
    oc.set_ripples(R, S)
    lay = rb.Layer(R, S, dtype, 2.0, 0.05, B, 4.0, mode=mode, g=9.81, G=table)
    x, y = (origin[0] + R // 2 + 0.5) * S, (origin[1] + R // 2 + 0.5) * S
    oc.center_ripples(x, y)
    lay.center(x, y)
    assert (lay.ox, lay.oy) == origin and oc.ripples_device()[2:] == origin
    return lay


def _bed_memory(oc, torch):
    """(d, q) in MEMORY order, straight from the device planes"""
    oc.read_ripple_bed()                                                 # waits for the handle's stream
    dptr, qptr, cells = oc.ripple_bed_device()
    R = int(round(cells ** 0.5))
    return _peek(torch, dptr, cells).view(np.float32).reshape(R, R), _peek(torch, qptr, cells // 4).view(np.uint8).reshape(R, R)


def _bed_guards_whole(oc, torch):
    oc.read_ripple_bed()
    dptr, qptr, cells = oc.ripple_bed_device()
    whole = lambda ptr, nbytes: bool(np.all(_peek(torch, ptr - 4 * BGUARD, BGUARD) == 0xCDCDCDCD) and np.all(_peek(torch, ptr + nbytes, BGUARD) == 0xCDCDCDCD))
    return whole(dptr, 4 * cells) and whole(qptr, cells)


def _same_planes(oc, torch, lay, what):
    d, q = oc.read_ripple_bed()
    wd, wq = lay.bed_window()
    assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(q, wq), (what, np.argwhere(_bits(d) != _bits(wd))[:4], np.argwhere(q != wq)[:4])
    md, mq = _bed_memory(oc, torch)
    assert np.array_equal(_bits(md), _bits(lay.d)) and np.array_equal(mq, lay.q), what


def _shore_impulses(lay, rng):
    """a deposit on the centre of every solid cell that has water within one cell, and on that water: the shoreline, the island, the piers"""
    solid = lay.window(lay.d) == 0
    near = np.zeros_like(solid)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            near |= np.roll(~solid, (dj, di), (0, 1))
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            near |= np.roll(solid & near, (dj, di), (0, 1))
    j, i = np.nonzero(near)
    imp = np.zeros((len(i), 4), F)
    imp[:, 0], imp[:, 1] = (lay.ox + i + 0.5) * S, (lay.oy + j + 0.5) * S
    imp[:, 2] = rng.uniform(0.005, 0.03, len(i)) * rng.choice([-1, 1], len(i))
    return imp


# -- the planes


@pytest.mark.parametrize("R,origin", [(R, o) for R in (64, 128) for o in ((0, 0), ORIGIN)])
def test_plane_bits(capi, torch, table, R, origin):
    with _plain(capi) as oc:
        lay = _layer(oc, table, R, 8, origin)
        assert oc.ripple_bed_device() == (None, None, 0)
        b, depths = shore(R, *origin)
        oc.set_ripple_bed(b, depths)
        lay.set_bed(b, depths)
        dptr, qptr, cells = oc.ripple_bed_device()
        assert dptr and qptr and cells == R * R and 0 < (lay.d == 0).sum() < 3 * R * R // 4 and lay.q.max() >= 14
        _same_planes(oc, torch, lay, "set")
        # a few cells, then R cells or more (everything off the map reads `outside`), then back over the map
        for dx, dy in ((3, -2), (-5, 7), (R + 9, 0), (-(R + 9), -3 * R), (2, 3 * R + 1), (0, -6)):
            x, y = (lay.ox + dx + R // 2 + 0.5) * S, (lay.oy + dy + R // 2 + 0.5) * S
            oc.center_ripples(x, y)
            lay.center(x, y)
            assert oc.ripples_device()[2:] == (lay.ox, lay.oy)
            _same_planes(oc, torch, lay, (dx, dy))
        assert (lay.d == 0).any() and _bed_guards_whole(oc, torch)
        # walls after the bed: the bed is rastered again, a wall cell is solid; walls off: it is water again
        wl = piers(R, lay.ox, lay.oy)
        wet = (lay.d != 0).sum()
        oc.set_ripple_walls(wl)
        lay.set_walls(wl)
        assert (lay.d != 0).sum() < wet - 10 and not lay.d[lay.wall != 0].any()
        _same_planes(oc, torch, lay, "walls after the bed")
        x, y = (lay.ox + 7 + R // 2 + 0.5) * S, (lay.oy - 4 + R // 2 + 0.5) * S
        oc.center_ripples(x, y)
        lay.center(x, y)
        _same_planes(oc, torch, lay, "a scroll with walls")
        assert np.array_equal(oc.read_ripple_walls(), lay.wall_window())
        oc.set_ripple_walls(None)
        lay.set_walls(None)
        _same_planes(oc, torch, lay, "walls off")
        assert _bed_guards_whole(oc, torch) and _both_guards_whole(oc, torch)
        # reset keeps the bed; a new bed replaces it; a null bed -> nulls; set_ripples drops it
        oc.reset_ripples()
        _same_planes(oc, torch, lay, "reset")
        b2, depths2 = shore(R, lay.ox, lay.oy, surf=False, seed=9)
        oc.set_ripple_bed(b2, depths2)
        lay.set_bed(b2, depths2)
        _same_planes(oc, torch, lay, "a new bed")
        assert not lay.q.any()
        oc.set_ripple_bed(None)
        assert oc.ripple_bed_device() == (None, None, 0)
        oc.set_ripple_bed(b, depths)
        oc.set_ripples(R, S)
        assert oc.ripple_bed_device() == (None, None, 0)


# -- the steps


@pytest.mark.parametrize("walls", [False, True])
@pytest.mark.parametrize("R,B,origin", [(64, 8, ORIGIN), (64, 0, (0, 0)), (128, 8, (0, 0)), (128, 0, ORIGIN)])
def test_step_bits(capi, torch, table, report, R, B, origin, walls):
    rng = np.random.default_rng(R + B + walls)
    with _plain(capi) as oc:
        lay = _layer(oc, table, R, B, origin)
        l64 = _layer(oc, table, R, B, origin, np.float64)
        b, depths = shore(R, *origin, surf=B > 0)
        if walls:
            wl = piers(R, *origin)
            oc.set_ripple_walls(wl)
            lay.set_walls(wl)
            l64.set_walls(wl)
        oc.set_ripple_bed(b, depths)
        lay.set_bed(b, depths)
        l64.set_bed(b, depths)
        _same_planes(oc, torch, lay, "before the steps")
        planes = [p.copy() for p in _bed_memory(oc, torch)]
        assert (lay.q > 0).any() == (B > 0) and (lay.d == 0).sum() > R
        keep, worst = [], 0.0
        for substeps in (1, 3, 16):
            imp = np.concatenate([_shore_impulses(lay, rng), _impulses(rng, lay, R * R // 4)])
            keep.append(_deposit(oc, torch, imp))
            lay.deposit(imp)
            assert np.any(lay.src[lay.d == 0] != 0)
            l64.eta, l64.rate, l64.src = lay.eta.astype(np.float64), lay.rate.astype(np.float64), lay.src.copy()
            oc.step_ripples(H * substeps, substeps)
            lay.step(H * substeps, substeps)
            l64.step(H * substeps, substeps)
            got = oc.read_ripples()
            assert np.array_equal(_bits(got), _bits(lay.window())), (R, B, origin, walls, substeps, np.argwhere(_bits(got) != _bits(lay.window()))[:4])
            # a solid cell holds (+0, +0) whatever was deposited on it
            assert not _bits(got)[lay.window(lay.d) == 0].any()
            worst = max(worst, np.abs(got[..., 0].astype(np.float64) - l64.window()[..., 0]).max() / (EPS * np.abs(l64.eta).max()))
            # one more sub-step without deposits: the buffer it reads and both planes keep their bits
            ptr, nbytes = oc.ripples_device()[:2]
            oc.step_ripples(H, 1)
            lay.step(H, 1)
            after = oc.read_ripples()
            assert np.array_equal(_bits(after), _bits(lay.window())), (R, B, origin, walls, substeps, "second")
            read = _peek(torch, ptr, nbytes // 4).view(np.float32).reshape(R, R, 2)
            assert np.array_equal(_bits(lay.window(read)), _bits(got)), "the sub-step wrote the buffer it reads"
            now = _bed_memory(oc, torch)
            assert np.array_equal(_bits(now[0]), _bits(planes[0])) and np.array_equal(now[1], planes[1]), "the sub-step wrote a plane"
            cur = oc.ripples_device()[0]
            assert cur != ptr and _guards_whole(torch, ptr, nbytes) and _guards_whole(torch, cur, nbytes) and _bed_guards_whole(oc, torch)
            assert not walls or _plane_guards_whole(oc, torch)
        line = f"ripple bed R={R} B={B} origin={origin} walls={walls}: |device - float64| / (eps max|eta|) = {worst:.2f}, K_RIP_BED = {rb.K_RIP_BED}"
        print(line)
        report(line)
        assert np.abs(after[..., 0]).max() > 1e-3 and np.isfinite(after).all()
        assert worst <= rb.K_RIP_BED
        # the map is untouched: a scroll away and back rasters the same planes from it
        for dx in (R + 3, 0):
            oc.center_ripples((lay.ox + dx + R // 2 + 0.5) * S, (lay.oy + R // 2 + 0.5) * S)
        now = _bed_memory(oc, torch)
        assert oc.ripples_device()[2:] == origin and np.array_equal(_bits(now[0]), _bits(planes[0])) and np.array_equal(now[1], planes[1])


# -- zeroing, and the bed off


def test_zeroing(capi, torch, table):
    R, B = 128, 8
    rng = np.random.default_rng(31)
    with _plain(capi) as oc:
        lay = _layer(oc, table, R, B, ORIGIN)
        imp = _impulses(rng, lay, R * R)
        oc.deposit_ripples_host(imp)
        oc.step_ripples(H * 3, 3)
        a, nbytes = oc.ripples_device()[:2]
        oc.step_ripples(0.0, 1)
        b_ = oc.ripples_device()[0]
        oc.read_ripples()
        before = [_peek(torch, p, nbytes // 4).copy() for p in (a, b_)]
        bed, depths = shore(R, *ORIGIN)
        lay.set_bed(bed, depths)
        oc.set_ripple_bed(bed, depths)
        oc.read_ripple_bed()
        mask = np.repeat(lay.d.reshape(-1) == 0, 2)
        for p, old in zip((a, b_), before):
            new = _peek(torch, p, nbytes // 4)
            assert not new[mask].any() and np.array_equal(new[~mask], old[~mask]) and old[mask].any() and mask.sum() > R
        assert oc.ripples_device()[0] == b_ and _both_guards_whole(oc, torch) and _bed_guards_whole(oc, torch)


@pytest.mark.parametrize("mode", [rb.WAVE, rb.DEEP])
def test_bed_off_keeps_the_parents_bits(capi, torch, table, mode):
    R, B = 128, 8
    rng = np.random.default_rng(41 + mode)
    with _plain(capi) as oc, _plain(capi) as never:
        lay = _layer(oc, table, R, B, ORIGIN)
        ref = _layer(never, table, R, B, ORIGIN, mode=mode)
        bed, depths = shore(R, *ORIGIN)
        oc.set_ripple_bed(bed, depths)
        oc.set_ripple_bed(None)
        oc.set_ripple_dispersion(mode, 9.81)
        lay.mode = mode
        # (the bed zeroed nothing that was not zero: both start from rest)
        imp = _impulses(rng, lay, R * R)
        for o, l in ((oc, lay), (never, ref)):
            o.deposit_ripples_host(imp)
            l.deposit(imp)
            o.step_ripples(H * 3, 3)
            l.step(H * 3, 3)
        got = oc.read_ripples()
        assert np.count_nonzero(got) > R * R and np.array_equal(_bits(got), _bits(never.read_ripples())) and np.array_equal(_bits(got), _bits(lay.window()))
        # and with walls alone, the walled kernels' bits
        wl = piers(R, *ORIGIN)
        for o, l in ((oc, lay), (never, ref)):
            o.set_ripple_walls(wl)
            l.set_walls(wl)
            o.deposit_ripples_host(imp)
            l.deposit(imp)
            o.step_ripples(H * 2, 2)
            l.step(H * 2, 2)
        got = oc.read_ripples()
        assert np.array_equal(_bits(got), _bits(never.read_ripples())) and np.array_equal(_bits(got), _bits(lay.window()))


# -- coupled stepping


def test_coupled_with_bed(capi, torch, table):
    bodies, motions, props, probes = _two_boxes()
    R, K, dt = 64, 2, 0.1
    with _flat(capi) as oc:
        s = _set(capi, 0, swell=False, plane_w=-0.25)
        oc.set_ripples(R, S)
        lay = rb.Layer(R, S, G=table)
        pts = couple64.points32(bodies, probes)
        # a shelf that shoals towards +x with land beyond the boxes, and a pile (a wall) under one of their probes
        W = 40
        X = -16.0 + 0.8 * np.arange(W)
        depths = np.broadcast_to(np.clip(1.1 - 0.12 * (X - float(pts[:, 0].min())), -0.5, 2.0), (W, W)).astype(F)
        bed = rb.bed(W, W, (-16.0, -16.0), 0.8, outside=1.0, max_depth=1.2, dry_depth=0.05, surf_depth=0.5, surf_gamma=2.0)
        wl = rw.box(float(pts[0, 0]), float(pts[0, 1]), 0.3, 0.3)
        oc.set_ripple_walls(wl)
        lay.set_walls(wl)
        oc.set_ripple_bed(bed, depths)
        lay.set_bed(bed, depths)
        assert (lay.d == 0).sum() > R and (lay.q > 0).sum() > R and lay.wall.sum() > 0
        _same_planes(oc, torch, lay, "coupled")
        recs = np.zeros((len(pts), 8), F)
        recs[:, 2] = 0.25
        wb, wm = bodies, motions
        gb, gm = bodies.copy(), motions.copy()
        for _ in range(2):
            wb, wm, wr = couple64.call32(lay, wb, wm, props, probes, lambda b: recs, dt, K)
            gr = oc.step_bodies_coupled_host([0], s, gb, gm, props, probes, dt, K, 4)
            _same((gb, gm, gr), (wb, wm, wr), "bed, host twin")
        state = oc.read_ripples()
        assert np.array_equal(_bits(state), _bits(lay.window())) and np.abs(lay.eta).max() > 1e-3
        assert not _bits(state)[lay.window(lay.d) == 0].any()
        # nbodies == 0: step_ripples(h, 1) x substeps, the bed on
        for coupled in (True, False):
            oc.reset_ripples()
            imp = _impulses(np.random.default_rng(2), lay, 500)
            oc.deposit_ripples_host(imp)
            if coupled:
                oc.step_bodies_coupled([0], s, None, None, None, 0, None, 0, dt, 3, None, 4)
                alone = oc.read_ripples()
            else:
                h = F(dt) * (F(1) / F(3))
                for _ in range(3):
                    oc.step_ripples(float(h), 1)
                assert np.array_equal(_bits(oc.read_ripples()), _bits(alone)) and np.abs(alone).max() > 0
        assert _both_guards_whole(oc, torch) and _bed_guards_whole(oc, torch)


# -- bounds, isolation, refusals


def test_bounds_mark_and_isolation(capi, torch, table):
    R = 64
    with _plain(capi) as oc:
        lay = _layer(oc, table, R, 8, ORIGIN)
        oc.set_ripple_foam(True)
        imp = _impulses(np.random.default_rng(8), lay, 400)
        oc.deposit_ripples_host(imp)
        lay.deposit(imp)
        oc.step_ripples(H, 1)
        lay.step(H, 1)
        oc.step_ripple_foam(0.1)
        oc.deposit_ripples_host(imp)                                     # pending while the bed is set
        lay.deposit(imp)
        foam, maps, state = oc.read_ripple_foam(), oc.read_maps(0), oc.read_state(0)
        first = oc.read_ripple_bounds()
        ptr = oc.ripple_bounds_device()[0]
        w = lay.window()
        assert first[0] == w[..., 0].min() and first[1] == w[..., 0].max()
        # the mark: a reduce leaves the record CURRENT; set_ripple_bed clears it, so the next read reduces again and sees the zeroed cells
        b, depths = shore(R, *ORIGIN)
        oc.set_ripple_bed(b, depths)
        lay.set_bed(b, depths)
        stale = _peek(torch, ptr, 8).view(np.float32)
        assert np.array_equal(stale, first)                              # nothing reduced yet
        got = oc.read_ripple_bounds()
        w = lay.window()
        assert got[0] == w[..., 0].min() and got[1] == w[..., 0].max() and got[2] == w[..., 1].min() and got[3] == w[..., 1].max()
        assert np.array_equal(_bits(oc.read_ripples()), _bits(w))
        # src, wake foam and the maps are untouched: the pending deposits arrive in the next step, on water only
        assert np.array_equal(_bits(oc.read_ripple_foam()), _bits(foam))
        assert np.array_equal(_bits(oc.read_maps(0)), _bits(maps)) and np.array_equal(_bits(oc.read_state(0)), _bits(state))
        oc.step_ripples(H * 2, 2)
        lay.step(H * 2, 2)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())) and np.abs(lay.eta).max() > 1e-4
        oc.set_ripple_bed(None)
        assert np.array_equal(_bits(oc.read_ripple_foam()), _bits(foam))


def test_refusals(capi):
    with _plain(capi) as oc:
        lib = capi.load()
        p = lambda a: a.ctypes.data_as(capi.P)
        err = lambda: lib.datum_ocean_last_error(oc.h)
        depths = np.full((3, 4), 1.0, F)
        rec = lambda **kw: np.array([rb.bed(4, 3, (0.0, 0.0), 1.0, **kw)], rb.BED)
        good = rec(max_depth=1.2)
        # the layer is off
        assert lib.datum_ocean_set_ripple_bed(oc.h, p(good), p(depths)) == capi.ESTATE and b"datum_ocean_set_ripple_bed" in err()
        assert lib.datum_ocean_set_ripple_bed(oc.h, None, None) == capi.ESTATE
        assert lib.datum_ocean_read_ripple_bed(oc.h, p(np.zeros(4, F)), None) == capi.ESTATE
        assert oc.ripple_bed_device() == (None, None, 0)
        oc.set_ripples(64, S)
        assert lib.datum_ocean_read_ripple_bed(oc.h, p(np.zeros(64 * 64, F)), None) == capi.ESTATE and b"the bed is off" in err()
        # the record's ranges
        bad = [rec(max_depth=0.0), rec(max_depth=np.inf), rec(max_depth=np.nan), rec(dry_depth=0.0), rec(dry_depth=11.0), rec(dry_depth=np.nan),
               rec(surf_depth=-1.0), rec(surf_depth=np.nan), rec(surf_gamma=-1.0), rec(surf_gamma=np.inf), rec(outside=np.nan)]
        for field, v in (("width", 1), ("width", 4097), ("height", 1), ("height", 4097), ("texel", 0.0), ("texel", -1.0), ("texel", np.inf), ("texel", np.nan)):
            r = good.copy()
            r[field] = v
            bad.append(r)
        for k, v in ((0, np.nan), (1, np.inf)):
            r = good.copy()
            r["origin"][0, k] = v
            bad.append(r)
        big = np.full(4097 * 2, 1.0, F)
        for r in bad:
            assert lib.datum_ocean_set_ripple_bed(oc.h, p(r), p(big)) == capi.EINVAL and b"datum_ocean_set_ripple_bed" in err(), r
        assert lib.datum_ocean_set_ripple_bed(oc.h, p(good), None) == capi.EINVAL and b"depths_host" in err()
        # a map value that is not finite, anywhere
        for k, v in ((0, np.nan), (5, np.inf), (11, -np.inf)):
            m = depths.copy()
            m.reshape(-1)[k] = v
            assert lib.datum_ocean_set_ripple_bed(oc.h, p(good), p(m)) == capi.EINVAL and b"not finite" in err()
        assert oc.ripple_bed_device() == (None, None, 0)                  # a refusal changes nothing
        # the stability bound: c = 2 passes at dt = 0.1, the bed's sqrt(g max_depth) decides once it is on, whatever c is
        assert rb.stable(9.81, 1.2, S, 0.1, 1) and not rb.stable(9.81, 1.3, S, 0.1, 1)
        oc.set_ripple_params(2.0, 0.05, 8, 4.0)
        oc.step_ripples(0.1, 1)
        oc.set_ripple_bed(rec(max_depth=1.3)[0], depths)
        assert lib.datum_ocean_step_ripples(oc.h, 0.1, 1) == capi.EINVAL and b"0.7" in err()
        assert lib.datum_ocean_step_ripples(oc.h, 0.2, 2) == capi.EINVAL
        assert lib.datum_ocean_step_ripples(oc.h, 0.2, 3) == capi.OK
        oc.set_ripple_bed(good[0], depths)
        oc.set_ripple_params(100.0, 0.05, 8, 4.0)                        # c is not used while the bed is on
        assert lib.datum_ocean_step_ripples(oc.h, 0.1, 1) == capi.OK
        oc.set_ripple_bed(None)
        assert lib.datum_ocean_step_ripples(oc.h, 0.1, 1) == capi.EINVAL
        oc.set_ripple_params(2.0, 0.05, 8, 4.0)
        # the bed and DEEP do not combine
        oc.set_ripple_bed(good[0], depths)
        assert lib.datum_ocean_set_ripple_dispersion(oc.h, rb.DEEP, 9.81) == capi.ESTATE and b"bed" in err()
        oc.set_ripple_dispersion(rb.WAVE, 9.81)
        oc.set_ripple_bed(None)
        oc.set_ripple_dispersion(rb.DEEP, 9.81)
        assert lib.datum_ocean_set_ripple_bed(oc.h, p(good), p(depths)) == capi.ESTATE and b"DEEP" in err()
        assert oc.ripple_bed_device() == (None, None, 0)
        assert lib.datum_ocean_set_ripple_bed(oc.h, None, None) == capi.OK
        oc.set_ripple_dispersion(rb.WAVE, 9.81)
        oc.set_ripple_bed(good[0], depths)
        d, q = oc.read_ripple_bed()
        assert d.shape == (64, 64) and lib.datum_ocean_read_ripple_bed(oc.h, None, None) == capi.OK
        assert lib.datum_ocean_ripple_bed_device(oc.h, None, None, None) == capi.OK


# -- the C++ shim


def test_cpp_shim_reaches_the_same_bits(capi, torch, table):
    from datum_amd import host_api

    N, R = 256, 128
    rng = np.random.default_rng(12)
    with host_api.OceanContext(N) as ctx:
        oc = capi.Ocean.__new__(capi.Ocean)
        oc.lib, oc.h, oc.N, oc.cascades = capi.load(), ctx.lib.datum_host_context_handle(ctx.c), N, 1
        try:
            b0, d0 = shore(R, 0, 0)
            with pytest.raises(Exception):
                ctx.set_ocean_ripple_bed(b0, d0)                         # the layer is off
            ctx.set_ocean_ripples(R, S)
            ctx.center_ocean_ripples(3.3, -2.2)
            lay = rb.Layer(R, S, G=table)
            lay.center(3.3, -2.2)
            b, depths = shore(R, lay.ox, lay.oy)
            ctx.set_ocean_ripple_bed(b, depths)
            lay.set_bed(b, depths)
            d, q = ctx.read_ocean_ripple_bed(R)
            wd, wq = lay.bed_window()
            assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(q, wq)
            _same_planes(oc, torch, lay, "shim")
            imp = _impulses(rng, lay, 2000)
            ctx.deposit_ocean_ripples(imp)
            lay.deposit(imp)
            ctx.step_ocean_ripples(H * 3, 3)
            lay.step(H * 3, 3)
            state = oc.read_ripples()
            assert np.array_equal(_bits(state), _bits(lay.window())) and np.abs(state).max() > 0
            # the same through the C ABI on the same handle
            oc.reset_ripples()
            oc.set_ripple_bed(b, depths)
            oc.deposit_ripples_host(imp)
            oc.step_ripples(H * 3, 3)
            assert np.array_equal(_bits(oc.read_ripples()), _bits(state))
            with pytest.raises(Exception):
                ctx.set_ocean_ripple_bed(rb.bed(4, 3, (0, 0), -1.0), np.ones((3, 4), F))
            ctx.set_ocean_ripple_bed(None)
            assert oc.ripple_bed_device() == (None, None, 0)
            ctx.set_ocean_ripples(0, 0.0)
        finally:
            oc.h = None
