"""Ripple walls (include/datum_ocean_hip.h: "ripple walls") on the MI355X, through the C ABI, against tests/ripple_wall64.py.

R = 64 is one tile of the step kernels across, R = 128 has tile seams in both directions (memory x 63|64, y 15|16 ...); with the origin
(37, -21) the window's seam falls inside a tile, with (0, 0) on a tile's edge.

  plane     bit for bit against numpy after set_ripple_walls, a center_ripples of a few cells, one of R cells or more, a new list;
            count == 0 -> the getter returns null;
  steps     both modes bit for bit against the fp32 restatement after 1, 3 and 16 sub-steps, B = 8 and 0, within K_RIP_WALL of float64;
            the walls: a one-cell line crossing the tile seams, cells in a tile's halo row and column, a cell at every window corner and on
            every edge, walls on both sides of the torus seam; deposits on wall cells and on the water beside them; the buffer a sub-step
            reads and the plane keep their bits; the plane's two guards and the state buffers' four stay whole;
  zeroing   set_ripple_walls leaves +0 in both state buffers at every wall cell and every other cell as it was;
  off       walls set and removed, and a list that covers no cell centre, give the bits of a handle that never had walls;
  coupled   step_bodies_coupled with walls in both modes against couple64's loop over the walled restatement, nbodies == 0 included;
  bounds    the CURRENT mark is cleared by set_ripple_walls, and the record after a walled step is numpy's;
  isolation maps, wake foam and src are untouched by the new calls; refusals; read_ripple_walls and the C++ shim.
"""

import ctypes

import numpy as np
import pytest

import couple64
import ripple64
import ripple_deep64 as rd
import ripple_wall64 as rw
from test_gpu_couple import _same, _two_boxes
from test_gpu_ripple_deep import _both_guards_whole, _guards_whole
from test_gpu_ripple_foam import _peek
from test_gpu_ripples import ORIGIN, _deposit, _impulses, _plain
from test_gpu_step import _flat
from test_gpu_surface import _set

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -24
S = 0.5
H = 0.1
WGUARD = 64                   # 32-bit words of 0xCD bytes the handle keeps before and after the wall plane


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


def _layer(oc, table, R, B, origin, mode, dtype=F):
    oc.set_ripple_params(2.0, 0.05, B, 4.0)
    oc.set_ripple_dispersion(mode, 9.81)
    oc.set_ripples(R, S)
    lay = rw.Layer(R, S, dtype, 2.0, 0.05, B, 4.0, mode=mode, g=9.81, G=table)
    x, y = (origin[0] + R // 2 + 0.5) * S, (origin[1] + R // 2 + 0.5) * S
    oc.center_ripples(x, y)
    lay.center(x, y)
    assert (lay.ox, lay.oy) == origin and oc.ripples_device()[2:] == origin
    return lay


def _cell(lay, i, j, hx=0.25, hy=0.25):
    """a box round the centre of window cell (i, j), `hx` x `hy` cells half extents"""
    return rw.box((lay.ox + i + 0.5) * S, (lay.oy + j + 0.5) * S, hx * S, hy * S)


def _seam_walls(lay):
    """the issue's wall set for a window at lay's origin, by WINDOW coordinates of the MEMORY places that matter"""
    R, ox, oy = lay.R, lay.ox, lay.oy
    wx = lambda m: (m - ox) & (R - 1)                      # window coordinate of memory column / row m
    wy = lambda m: (m - oy) & (R - 1)
    recs = []
    # a one-cell line across the tile seams: memory row 20 over memory columns 40 .. 90 (x 63|64 at R = 128), memory column 30 over rows 8 .. 40 (y 15|16, 31|32)
    recs += [_cell(lay, wx(m), wy(20)) for m in range(40, min(R, 91))]
    recs += [_cell(lay, wx(30), wy(m)) for m in range(8, 41)]
    # cells in a tile's halo row and halo column: memory rows 15 and 16, 31 and 32; memory columns 63 and 0 (the halo of the tile beside them)
    recs += [_cell(lay, wx(5), wy(15)), _cell(lay, wx(6), wy(16)), _cell(lay, wx(50), wy(31)), _cell(lay, wx(51), wy(32))]
    recs += [_cell(lay, wx(63), wy(3)), _cell(lay, wx(0), wy(4)), _cell(lay, wx(R - 1), wy(47)), _cell(lay, wx(64 & (R - 1)), wy(46))]
    # every window corner and edge
    recs += [_cell(lay, i, j) for i in (0, R - 1) for j in (0, R - 1)]
    recs += [_cell(lay, R // 2, 0, 2.25), _cell(lay, R // 2 + 3, R - 1, 1.25), _cell(lay, 0, R // 2 - 5, 0.25, 2.25), _cell(lay, R - 1, R // 2 + 7, 0.25, 1.25)]
    # both sides of the torus seam (memory column / row R - 1 | 0), a rotated box and an ellipse in open water
    recs += [_cell(lay, wx(R - 1), wy(R - 9)), _cell(lay, wx(0), wy(R - 9)), _cell(lay, wx(R - 12), wy(R - 1)), _cell(lay, wx(R - 12), wy(0))]
    recs += [rw.box((ox + R // 2) * S, (oy + R // 3) * S, 5.3 * S, 1.1 * S, 0.6, 0.8), rw.ellipse((ox + R // 4) * S, (oy + 3 * R // 4) * S, 4.2 * S, 2.6 * S, 0.8, -0.6)]
    return rw.walls(*recs)


def _wall_impulses(lay, rng):
    """a deposit on the centre of every wall cell's 3 x 3 neighbourhood that lies in the window: wall cells and the water beside them"""
    R = lay.R
    w = lay.wall_window() != 0
    near = w.copy()
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            near |= np.roll(w, (dj, di), (0, 1))
    j, i = np.nonzero(near)
    imp = np.zeros((len(i), 4), F)
    imp[:, 0], imp[:, 1] = (lay.ox + i + 0.5) * S, (lay.oy + j + 0.5) * S
    imp[:, 2] = rng.uniform(0.005, 0.03, len(i)) * rng.choice([-1, 1], len(i))
    return imp


def _plane_guards_whole(oc, torch):
    ptr = oc.ripple_walls_device()
    R = oc.read_ripple_walls().shape[0]                                   # waits for the handle's stream
    return bool(np.all(_peek(torch, ptr - 4 * WGUARD, WGUARD) == 0xCDCDCDCD) and np.all(_peek(torch, ptr + R * R, WGUARD) == 0xCDCDCDCD))


def _plane_memory(oc, torch):
    R = oc.read_ripple_walls().shape[0]
    return _peek(torch, oc.ripple_walls_device(), R * R // 4).view(np.uint8).reshape(R, R)


# -- the plane


@pytest.mark.parametrize("R,origin", [(R, o) for R in (64, 128) for o in ((0, 0), ORIGIN)])
def test_plane_bits(capi, torch, table, R, origin):
    with _plain(capi) as oc:
        lay = _layer(oc, table, R, 8, origin, rw.WAVE)
        assert oc.ripple_walls_device() is None
        wl = _seam_walls(lay)
        oc.set_ripple_walls(wl)
        lay.set_walls(wl)
        assert oc.ripple_walls_device() is not None and 0 < lay.wall.sum() < R * R // 8
        assert np.array_equal(oc.read_ripple_walls(), lay.wall_window()) and np.array_equal(_plane_memory(oc, torch), lay.wall)
        # a few cells, then R cells or more, then back over the walls
        for dx, dy in ((3, -2), (-5, 7), (R + 9, 0), (-(R + 9), -3 * R), (2, 3 * R + 1)):
            x, y = (lay.ox + dx + R // 2 + 0.5) * S, (lay.oy + dy + R // 2 + 0.5) * S
            oc.center_ripples(x, y)
            lay.center(x, y)
            assert oc.ripples_device()[2:] == (lay.ox, lay.oy)
            assert np.array_equal(oc.read_ripple_walls(), lay.wall_window()), (dx, dy)
            assert np.array_equal(_plane_memory(oc, torch), lay.wall), (dx, dy)
        assert lay.wall.sum() > 0 and _plane_guards_whole(oc, torch)
        # a new list, 256 records
        rng = np.random.default_rng(R)
        many = np.zeros(rw.MAX_WALLS, rw.WALL)
        ang = rng.uniform(0, 2 * np.pi, len(many))
        many["center"] = (np.array([lay.ox, lay.oy]) + rng.uniform(-8, R + 8, (len(many), 2))) * S
        many["axis"] = np.stack([np.cos(ang), np.sin(ang)], 1)
        many["half"] = rng.uniform(0.2, 2.5, (len(many), 2))
        many["kind"] = rng.integers(0, 2, len(many))
        oc.set_ripple_walls(many)
        lay.set_walls(many)
        assert np.array_equal(oc.read_ripple_walls(), lay.wall_window()) and lay.wall.sum() > 100
        assert _plane_guards_whole(oc, torch) and _both_guards_whole(oc, torch)
        # reset keeps them; count == 0 -> null; set_ripples drops them
        oc.reset_ripples()
        assert np.array_equal(oc.read_ripple_walls(), lay.wall_window())
        oc.set_ripple_walls(None)
        assert oc.ripple_walls_device() is None
        oc.set_ripple_walls(wl)
        oc.set_ripples(R, S)
        assert oc.ripple_walls_device() is None


# -- the steps


@pytest.mark.parametrize("mode", [rw.WAVE, rw.DEEP])
@pytest.mark.parametrize("R,B,origin", [(64, 8, ORIGIN), (64, 0, (0, 0)), (128, 8, (0, 0)), (128, 0, ORIGIN)])
def test_step_bits(capi, torch, table, report, mode, R, B, origin):
    rng = np.random.default_rng(R + B + mode)
    with _plain(capi) as oc:
        lay = _layer(oc, table, R, B, origin, mode)
        l64 = _layer(oc, table, R, B, origin, mode, np.float64)
        wl = _seam_walls(lay)
        oc.set_ripple_walls(wl)
        lay.set_walls(wl)
        l64.set_walls(wl)
        plane = _plane_memory(oc, torch)
        assert np.array_equal(plane, lay.wall)
        keep, worst = [], 0.0
        for substeps in (1, 3, 16):
            imp = np.concatenate([_wall_impulses(lay, rng), _impulses(rng, lay, R * R // 4)])
            keep.append(_deposit(oc, torch, imp))
            lay.deposit(imp)
            assert np.any(lay.src[lay.wall != 0] != 0)
            l64.eta, l64.rate, l64.src = lay.eta.astype(np.float64), lay.rate.astype(np.float64), lay.src.copy()
            oc.step_ripples(H * substeps, substeps)
            lay.step(H * substeps, substeps)
            l64.step(H * substeps, substeps)
            got = oc.read_ripples()
            assert np.array_equal(_bits(got), _bits(lay.window())), (mode, R, B, origin, substeps, np.argwhere(_bits(got) != _bits(lay.window()))[:4])
            assert not _bits(got)[lay.wall_window() != 0].any()
            worst = max(worst, np.abs(got[..., 0].astype(np.float64) - l64.window()[..., 0]).max() / (EPS * np.abs(l64.eta).max()))
            # one more sub-step without deposits: the buffer it reads and the plane keep their bits
            ptr, nbytes = oc.ripples_device()[:2]
            oc.step_ripples(H, 1)
            lay.step(H, 1)
            after = oc.read_ripples()
            assert np.array_equal(_bits(after), _bits(lay.window())), (mode, R, B, origin, substeps, "second")
            read = _peek(torch, ptr, nbytes // 4).view(np.float32).reshape(R, R, 2)
            assert np.array_equal(_bits(lay.window(read)), _bits(got)), "the sub-step wrote the buffer it reads"
            assert np.array_equal(_plane_memory(oc, torch), plane), "the sub-step wrote the plane"
            cur = oc.ripples_device()[0]
            assert cur != ptr and _guards_whole(torch, ptr, nbytes) and _guards_whole(torch, cur, nbytes) and _plane_guards_whole(oc, torch)
        K = rw.K_RIP_WALL[mode]
        line = f"walled ripples mode={mode} R={R} B={B} origin={origin}: |device - float64| / (eps max|eta|) = {worst:.2f}, K_RIP_WALL = {K}"
        print(line)
        report(line)
        assert np.abs(after[..., 0]).max() > 1e-3 and np.isfinite(after).all()
        assert worst <= K


# -- zeroing, and walls off


@pytest.mark.parametrize("mode", [rw.WAVE, rw.DEEP])
def test_zeroing_and_walls_off(capi, torch, table, mode):
    R, B = 128, 8
    rng = np.random.default_rng(21 + mode)
    with _plain(capi) as oc, _plain(capi) as never:
        lay = _layer(oc, table, R, B, ORIGIN, mode)
        ref = _layer(never, table, R, B, ORIGIN, mode)
        imp = _impulses(rng, lay, R * R)
        for o, l in ((oc, lay), (never, ref)):
            o.deposit_ripples_host(imp)
            l.deposit(imp)
            o.step_ripples(H * 3, 3)
            l.step(H * 3, 3)
        filled = oc.read_ripples()
        assert np.count_nonzero(filled) > R * R and np.array_equal(_bits(filled), _bits(never.read_ripples()))
        # an empty plane (a shape between four cell centres), then no walls: the bits of the handle that never had any
        between = rw.box((lay.ox + 40) * S, (lay.oy + 40) * S, 0.4 * S, 0.4 * S)
        oc.set_ripple_walls(between)
        assert not oc.read_ripple_walls().any() and np.array_equal(_bits(oc.read_ripples()), _bits(filled))
        for o in (oc, never):
            o.deposit_ripples_host(imp)
            o.step_ripples(H * 2, 2)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(never.read_ripples()))
        oc.set_ripple_walls(_seam_walls(lay))
        oc.set_ripple_walls(None)
        # (that zeroed the wall cells: the comparison goes on from a common state)
        oc.reset_ripples()
        never.reset_ripples()
        for o in (oc, never):
            o.deposit_ripples_host(imp)
            o.step_ripples(H * 2, 2)
        filled = oc.read_ripples()
        assert np.array_equal(_bits(filled), _bits(never.read_ripples())) and np.count_nonzero(filled) > R * R
        # zeroing: +0 in BOTH buffers at every wall cell, every other cell as it was
        a, nbytes = oc.ripples_device()[:2]
        oc.step_ripples(0.0, 1)
        b = oc.ripples_device()[0]
        oc.read_ripples()
        before = [_peek(torch, p, nbytes // 4).copy() for p in (a, b)]
        lay.move(*ORIGIN)
        wl = _seam_walls(lay)
        lay.set_walls(wl)
        oc.set_ripple_walls(wl)
        oc.read_ripple_walls()
        mask = np.repeat(lay.wall.reshape(-1) != 0, 2)
        for p, old in zip((a, b), before):
            new = _peek(torch, p, nbytes // 4)
            assert not new[mask].any() and np.array_equal(new[~mask], old[~mask]) and old[mask].any()
        assert oc.ripples_device()[0] == b and _both_guards_whole(oc, torch) and _plane_guards_whole(oc, torch)


# -- coupled stepping


@pytest.mark.parametrize("mode", [rw.WAVE, rw.DEEP])
def test_coupled_with_walls(capi, torch, table, mode):
    bodies, motions, props, probes = _two_boxes()
    R, K, dt = 64, 2, 0.1
    with _flat(capi) as oc:
        s = _set(capi, 0, swell=False, plane_w=-0.25)
        oc.set_ripple_dispersion(mode, 9.81)
        oc.set_ripples(R, S)
        lay = rw.Layer(R, S, mode=mode, G=table)
        pts = couple64.points32(bodies, probes)
        # a quay beside the boxes and a pile under one of their probes
        wl = rw.walls(rw.box(float(pts[:, 0].max()) + 2.0, 0.0, 0.5, 6.0), rw.box(float(pts[0, 0]), float(pts[0, 1]), 0.3, 0.3))
        oc.set_ripple_walls(wl)
        lay.set_walls(wl)
        assert lay.wall.sum() > 10 and np.array_equal(oc.read_ripple_walls(), lay.wall_window())
        recs = np.zeros((len(pts), 8), F)
        recs[:, 2] = 0.25
        wb, wm = bodies, motions
        gb, gm = bodies.copy(), motions.copy()
        for _ in range(2):
            wb, wm, wr = couple64.call32(lay, wb, wm, props, probes, lambda b: recs, dt, K)
            gr = oc.step_bodies_coupled_host([0], s, gb, gm, props, probes, dt, K, 4)
            _same((gb, gm, gr), (wb, wm, wr), "walls, host twin")
        state = oc.read_ripples()
        assert np.array_equal(_bits(state), _bits(lay.window())) and np.abs(lay.eta).max() > 1e-3
        assert not _bits(state)[lay.wall_window() != 0].any()
        # nbodies == 0: step_ripples(h, 1) x substeps, walls on
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
        assert _both_guards_whole(oc, torch) and _plane_guards_whole(oc, torch)


# -- bounds, isolation, refusals


def test_bounds_mark_and_isolation(capi, torch, table):
    R = 64
    with _plain(capi) as oc:
        lay = _layer(oc, table, R, 8, ORIGIN, rw.WAVE)
        oc.set_ripple_foam(True)
        imp = _impulses(np.random.default_rng(8), lay, 400)
        oc.deposit_ripples_host(imp)
        lay.deposit(imp)
        oc.step_ripples(H, 1)
        lay.step(H, 1)
        oc.step_ripple_foam(0.1)
        oc.deposit_ripples_host(imp)                                     # pending while the walls are set
        lay.deposit(imp)
        foam, maps, state = oc.read_ripple_foam(), oc.read_maps(0), oc.read_state(0)
        first = oc.read_ripple_bounds()
        ptr = oc.ripple_bounds_device()[0]
        w = lay.window()
        assert first[0] == w[..., 0].min() and first[1] == w[..., 0].max()
        # the mark: a reduce leaves the record CURRENT; set_ripple_walls clears it, so the next read reduces again and sees the zeroed cells
        wl = rw.walls(_cell(lay, *np.unravel_index(np.argmax(w[..., 0]), w.shape[:2])[::-1], 1.25, 1.25), _cell(lay, *np.unravel_index(np.argmin(w[..., 0]), w.shape[:2])[::-1], 1.25, 1.25))
        oc.set_ripple_walls(wl)
        lay.set_walls(wl)
        stale = _peek(torch, ptr, 8).view(np.float32)
        assert np.array_equal(stale, first)                              # nothing reduced yet
        got = oc.read_ripple_bounds()
        w = lay.window()
        assert got[0] == w[..., 0].min() and got[1] == w[..., 0].max() and got[1] < first[1] and got[0] > first[0]
        # src, wake foam and the maps are untouched: the pending deposits arrive in the next step, on water only
        assert np.array_equal(_bits(oc.read_ripple_foam()), _bits(foam))
        assert np.array_equal(_bits(oc.read_maps(0)), _bits(maps)) and np.array_equal(_bits(oc.read_state(0)), _bits(state))
        oc.step_ripples(H * 2, 2)
        lay.step(H * 2, 2)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))
        got = oc.read_ripple_bounds()
        w = lay.window()
        assert got[0] == w[..., 0].min() and got[1] == w[..., 0].max() and got[2] == w[..., 1].min() and got[3] == w[..., 1].max()
        oc.set_ripple_walls(None)
        assert np.array_equal(_bits(oc.read_ripple_foam()), _bits(foam))


def test_refusals(capi):
    with _plain(capi) as oc:
        lib = capi.load()
        one = rw.box(0.0, 0.0, 1.0, 1.0)
        p = lambda a: a.ctypes.data_as(capi.P)
        err = lambda: lib.datum_ocean_last_error(oc.h)
        # the layer is off
        assert lib.datum_ocean_set_ripple_walls(oc.h, p(one), 1) == capi.ESTATE and b"datum_ocean_set_ripple_walls" in err()
        assert lib.datum_ocean_read_ripple_walls(oc.h, p(np.zeros(4, np.uint8))) == capi.ESTATE
        assert oc.ripple_walls_device() is None
        oc.set_ripples(64, S)
        assert lib.datum_ocean_read_ripple_walls(oc.h, p(np.zeros(64 * 64, np.uint8))) == capi.ESTATE and b"walls are off" in err()
        many = np.repeat(one, rw.MAX_WALLS + 1)
        for walls, count in ((one, -1), (many, rw.MAX_WALLS + 1), (None, 1)):
            assert lib.datum_ocean_set_ripple_walls(oc.h, p(walls) if walls is not None else None, count) == capi.EINVAL and b"datum_ocean_set_ripple_walls" in err()
        for field, k, v in [("center", 0, np.nan), ("center", 1, np.inf), ("axis", 0, -np.inf), ("axis", 1, np.nan), ("half", 0, np.nan), ("half", 1, np.inf),
                            ("half", 0, 0.0), ("half", 1, -1.0), ("half", 0, -0.0)]:
            bad = np.repeat(one, 3)
            bad[field][2, k] = v
            assert lib.datum_ocean_set_ripple_walls(oc.h, p(bad), 3) == capi.EINVAL, (field, k, v)
        for kind in (2, -1):
            bad = one.copy()
            bad["kind"] = kind
            assert lib.datum_ocean_set_ripple_walls(oc.h, p(bad), 1) == capi.EINVAL and b"kind" in err()
        assert oc.ripple_walls_device() is None                          # a refusal changes nothing
        oc.set_ripple_walls(np.repeat(one, rw.MAX_WALLS))
        assert oc.ripple_walls_device() is not None
        assert lib.datum_ocean_read_ripple_walls(oc.h, None) == capi.EINVAL
        assert lib.datum_ocean_ripple_walls_device(oc.h, None) == capi.EINVAL
        assert lib.datum_ocean_set_ripple_walls(oc.h, None, 0) == capi.OK and oc.ripple_walls_device() is None


# -- the C++ shim


def test_cpp_shim_reaches_the_same_bits(capi, torch, table):
    from datum_amd import host_api

    N, R = 256, 128
    rng = np.random.default_rng(12)
    with host_api.OceanContext(N) as ctx:
        oc = capi.Ocean.__new__(capi.Ocean)
        oc.lib, oc.h, oc.N, oc.cascades = capi.load(), ctx.lib.datum_host_context_handle(ctx.c), N, 1
        try:
            with pytest.raises(Exception):
                ctx.set_ocean_ripple_walls(rw.box(0, 0, 1, 1))           # the layer is off
            ctx.set_ocean_ripples(R, S)
            ctx.center_ocean_ripples(3.3, -2.2)
            lay = rw.Layer(R, S, G=table)
            lay.center(3.3, -2.2)
            wl = _seam_walls(lay)
            ctx.set_ocean_ripple_walls(wl)
            lay.set_walls(wl)
            assert np.array_equal(ctx.read_ocean_ripple_walls(R), lay.wall_window()) and np.array_equal(oc.read_ripple_walls(), lay.wall_window())
            imp = _impulses(rng, lay, 2000)
            ctx.deposit_ocean_ripples(imp)
            lay.deposit(imp)
            ctx.step_ocean_ripples(H * 3, 3)
            lay.step(H * 3, 3)
            state = oc.read_ripples()
            assert np.array_equal(_bits(state), _bits(lay.window())) and np.abs(state).max() > 0
            # the same through the C ABI on the same handle
            oc.reset_ripples()
            oc.set_ripple_walls(wl)
            oc.deposit_ripples_host(imp)
            oc.step_ripples(H * 3, 3)
            assert np.array_equal(_bits(oc.read_ripples()), _bits(state))
            with pytest.raises(Exception):
                ctx.set_ocean_ripple_walls(rw.box(0, 0, -1, 1))
            ctx.set_ocean_ripple_walls(None)
            assert oc.ripple_walls_device() is None
            ctx.set_ocean_ripples(0, 0.0)
        finally:
            oc.h = None
