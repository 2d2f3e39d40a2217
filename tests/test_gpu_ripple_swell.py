"""Ripple swell (include/datum_ocean_hip.h: "ripple swell") on the MI355X, through the C ABI, against tests/ripple_swell64.py.

The maps are the golden 64 x 64 ones, three cascades (and 128 x 128 once).  R = 64 is one tile of the kernels across, R = 128 has tile seams
in both directions; at both origins the window wraps the torus inside a tile.  The solids are tests/test_ripple_swell_emul.py's `harbour`
(walls that touch the window's edge, a box across the torus seam, an ellipse, a one-cell pillar) and, over a bed, test_ripple_bed_emul's
`shore` (an island and a beach) with `piers` and the harbour on top.

  plane     F after refresh bit for bit against the restatement fed with datum_ocean_read_surface_blend's heights at the same centres, lists
            of 1 and 3; whole and +0 with nothing solid; read and device agree; the guards; state, src, foam, walls, bed and maps untouched;
  steps     1, 3 and 16 sub-steps bit for bit against the restatement and within K_RIP_SWELL of float64, both variants;
  currency  center_ripples, set_ripple_walls and set_ripple_bed clear the mark: the step is the parent's bit for bit, and the swell's again
            after a new refresh; with swell off every step has the bits of a handle that never had it;
  coupled   step_bodies_coupled's layer share runs the swell kernels;
  refusals  ESTATE / EINVAL, both directions with DEEP; the C++ shim.
"""

import ctypes

import numpy as np
import pytest

import ripple_bed64 as rb
import ripple_swell64 as rs
import ripple_wall64 as rw
from test_gpu_body import _step
from test_gpu_ripple_foam import _peek
from test_gpu_ripples import _deposit, _impulses
from test_gpu_surface import _set, _setup
from test_ripple_bed_emul import piers, shore
from test_ripple_swell_emul import ORIGINS, harbour

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -24
S = 0.5
H = 0.1
GUARD = 64                    # 32-bit words of 0xCD bytes the handle keeps before and after the plane


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


def _scene(oc, R, origin, bed, walls=True, B=8, dtype=F, swell=True, like=None):
    """the handle's layer and its restatement: the origin, the harbour, the bed, swell on (not current); `like` gives another layer's walls and bed"""
    oc.set_ripple_params(2.0, 0.05, B, 4.0)
    oc.set_ripple_dispersion(rs.WAVE, 9.81)
    oc.set_ripples(R, S)
    lay = rs.Layer(R, S, dtype, 2.0, 0.05, B, 4.0, g=9.81)
    x, y = (origin[0] + R // 2 + 0.5) * S, (origin[1] + R // 2 + 0.5) * S
    oc.center_ripples(x, y)
    lay.center(x, y)
    assert (lay.ox, lay.oy) == origin and oc.ripples_device()[2:] == origin
    if walls:
        wl = like.list if like is not None else rw.walls(harbour(R, *origin), piers(R, *origin)) if bed else harbour(R, *origin)
        oc.set_ripple_walls(wl)
        lay.set_walls(wl)
    if bed:
        b, depths = (like.bed, like.depths) if like is not None else shore(R, *origin)
        oc.set_ripple_bed(b, depths)
        lay.set_bed(b, depths)
    if swell:
        oc.set_ripple_swell(True)
        lay.set_swell(True)
    return lay


def _heights(oc, lay, cascades, s, it):
    """the summed surface above every cell's centre, memory order: field 2 of the blended sample's record"""
    return oc.read_surface_blend(cascades, s, lay.points(), it)[:, 2].reshape(lay.R, lay.R)


def _refresh(oc, lay, cascades, s, it=4):
    oc.refresh_ripple_swell(cascades, s, it)
    lay.refresh(_heights(oc, lay, cascades, s, it))


def _plane_memory(oc, torch):
    got = oc.read_ripple_swell()                                          # waits for the handle's stream
    ptr, nbytes, _ = oc.ripple_swell_device()
    assert nbytes == got.size * 4
    mem = _peek(torch, ptr, nbytes // 4)
    whole = bool(np.all(_peek(torch, ptr - 4 * GUARD, GUARD) == 0xCDCDCDCD) and np.all(_peek(torch, ptr + nbytes, GUARD) == 0xCDCDCDCD))
    return got, mem.reshape(got.shape), whole


# -- the plane


@pytest.mark.parametrize("N,R,origin,bed", [(64, 64, ORIGINS[0], False), (64, 64, ORIGINS[1], True), (64, 128, ORIGINS[0], True), (64, 128, ORIGINS[1], False), (128, 128, ORIGINS[0], True)])
def test_plane_bits(capi, torch, oracle, N, R, origin, bed):
    with _setup(capi, oracle, N, 3) as oc:
        _step(oc)
        assert oc.ripple_swell_device() == (None, 0, False)
        lay = _scene(oc, R, origin, bed)
        oc.set_ripple_foam(True)
        imp = _impulses(np.random.default_rng(R), lay, 600)
        oc.deposit_ripples_host(imp)
        oc.step_ripples(H, 1)
        oc.step_ripple_foam(0.1)
        oc.deposit_ripples_host(imp)                                     # pending through the refreshes
        state, foam, wall = oc.read_ripples(), oc.read_ripple_foam(), oc.read_ripple_walls()
        planes = oc.read_ripple_bed() if bed else None
        maps = [oc.read_maps(c) for c in range(3)]
        ptr, nbytes, current = oc.ripple_swell_device()
        got, mem, whole = _plane_memory(oc, torch)
        assert ptr and nbytes == R * R * 4 and not current and whole and not _bits(got).any()        # allocated zeroed, the mark clear
        for cascades in ([1], [0, 1, 2]):
            for swell, it in ((True, 4), (False, 0)):
                s = _set(capi, 0, swell)
                _refresh(oc, lay, cascades, s, it)
                got, mem, whole = _plane_memory(oc, torch)
                tag = (N, R, origin, bed, cascades, swell, it)
                assert np.array_equal(_bits(got), _bits(lay.F)), (tag, np.argwhere(_bits(got) != _bits(lay.F))[:4])
                assert np.array_equal(mem, _bits(got)) and whole and oc.ripple_swell_device() == (ptr, nbytes, True), tag
                sol = lay.solid()
                nb = sum(n.astype(int) for n in rw._neighbours(sol))
                assert not _bits(got)[sol].any() and not _bits(got)[~sol & (nb == 0)].any() and (got != 0).sum() > 60, tag
        # refresh wrote the plane alone
        assert np.array_equal(_bits(oc.read_ripples()), _bits(state)) and np.array_equal(_bits(oc.read_ripple_foam()), _bits(foam))
        assert np.array_equal(oc.read_ripple_walls(), wall) and all(np.array_equal(_bits(oc.read_maps(c)), _bits(maps[c])) for c in range(3))
        if bed:
            now = oc.read_ripple_bed()
            assert np.array_equal(_bits(now[0]), _bits(planes[0])) and np.array_equal(now[1], planes[1])
        # the pending deposits were left alone: they arrive with the next step, which is the swell's
        lay.set_window(state[..., 0], state[..., 1])
        lay.deposit(imp)
        oc.step_ripples(H, 1)
        lay.step(H, 1)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))
        # reset_ripples keeps the plane and the mark; set_ripples drops both
        oc.reset_ripples()
        assert oc.ripple_swell_device() == (ptr, nbytes, True) and np.array_equal(_bits(oc.read_ripple_swell()), _bits(lay.F))
        oc.set_ripples(R, S)
        assert oc.ripple_swell_device() == (None, 0, False)


def test_nothing_solid_is_zero(capi, torch, oracle):
    R = 128
    with _setup(capi, oracle, 64, 3) as oc:
        _step(oc)
        lay = _scene(oc, R, ORIGINS[0], False, walls=False)
        s = _set(capi, 0)
        # (the plane starts as zeroes: make it something else first, from a harbour, so that the refresh is seen to write it whole)
        wl = harbour(R, *ORIGINS[0])
        oc.set_ripple_walls(wl)
        oc.refresh_ripple_swell([0, 1, 2], s)
        assert np.count_nonzero(oc.read_ripple_swell()) > 60
        oc.set_ripple_walls(None)
        assert oc.ripple_swell_device()[2] is False
        oc.refresh_ripple_swell([0, 1, 2], s)
        got, mem, whole = _plane_memory(oc, torch)
        assert not _bits(got).any() and not mem.any() and whole and oc.ripple_swell_device()[2] is True
        # and a step with it is the plain parent: nothing is solid (the restatement falls through as the library does)
        lay.refresh(np.zeros((R, R), F))
        imp = _impulses(np.random.default_rng(4), lay, 900)
        oc.deposit_ripples_host(imp)
        lay.deposit(imp)
        oc.step_ripples(H * 3, 3)
        lay.step(H * 3, 3)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())) and np.abs(lay.eta).max() > 1e-4


# -- the steps


@pytest.mark.parametrize("R,origin,bed,B", [(64, ORIGINS[0], False, 8), (64, ORIGINS[1], True, 0), (128, ORIGINS[1], False, 0), (128, ORIGINS[0], True, 8)])
def test_step_bits(capi, torch, oracle, report, R, origin, bed, B):
    rng = np.random.default_rng(R + B)
    with _setup(capi, oracle, 64, 3) as oc:
        _step(oc)
        lay = _scene(oc, R, origin, bed, B=B)
        l64 = rs.Layer(R, S, np.float64, 2.0, 0.05, B, 4.0, g=9.81)
        l64.move(*origin)
        l64.set_walls(lay.list)
        if bed:
            l64.set_bed(lay.bed, lay.depths)
        s = _set(capi, 0)
        keep, worst = [], 0.0
        for substeps, cascades in ((1, [0, 1, 2]), (3, [1]), (16, [0, 1, 2])):
            _refresh(oc, lay, cascades, s)
            l64.F, l64.current = lay.F.astype(np.float64), True
            imp = _impulses(rng, lay, R * R // 4)
            keep.append(_deposit(oc, torch, imp))
            lay.deposit(imp)
            l64.eta, l64.rate, l64.src = lay.eta.astype(np.float64), lay.rate.astype(np.float64), lay.src.copy()
            oc.step_ripples(H * substeps, substeps)
            lay.step(H * substeps, substeps)
            l64.step(H * substeps, substeps)
            got = oc.read_ripples()
            assert np.array_equal(_bits(got), _bits(lay.window())), (R, origin, bed, substeps, np.argwhere(_bits(got) != _bits(lay.window()))[:4])
            assert not _bits(got)[lay.window(lay.solid())].any()
            worst = max(worst, np.abs(got[..., 0].astype(np.float64) - l64.window()[..., 0]).max() / (EPS * np.abs(l64.eta).max()))
            # one more sub-step without deposits (FIRST with an empty src), the plane unchanged behind it
            before = oc.read_ripple_swell()
            oc.step_ripples(H, 1)
            lay.step(H, 1)
            assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())), (R, origin, bed, substeps, "second")
            got2, mem, whole = _plane_memory(oc, torch)
            assert np.array_equal(_bits(got2), _bits(before)) and whole
        line = f"ripple swell R={R} B={B} origin={origin} bed={bed}: |device - float64| / (eps max|eta|) = {worst:.2f}, K_RIP_SWELL = {rs.K_RIP_SWELL}"
        print(line)
        report(line)
        assert np.abs(lay.eta).max() > 1e-3 and np.isfinite(lay.eta).all()
        assert worst <= rs.K_RIP_SWELL


# -- currency, and swell off


@pytest.mark.parametrize("bed", [False, True])
def test_currency(capi, torch, oracle, bed):
    R, origin = 128, ORIGINS[0]
    rng = np.random.default_rng(7 + bed)
    with _setup(capi, oracle, 64, 3) as oc, _setup(capi, oracle, 64, 3) as never:
        _step(oc)
        _step(never)
        lay = _scene(oc, R, origin, bed)
        ref = _scene(never, R, origin, bed, swell=False)
        s = _set(capi, 0)

        def both(what, swell):
            """the same deposits and three sub-steps on both handles: the bits agree exactly when the swell's kernels did not run"""
            imp = _impulses(rng, lay, 800)
            never.set_ripples(R, S)                                       # the other handle starts from this one's state: rest, the planes again
            _scene(never, R, (lay.ox, lay.oy), bed, swell=False, like=lay)
            oc.reset_ripples()
            lay.set_window(np.zeros((R, R), F), np.zeros((R, R), F))
            for o in (oc, never):
                o.deposit_ripples_host(imp)
                o.step_ripples(H * 3, 3)
            lay.deposit(imp)
            lay.step(H * 3, 3)
            got = oc.read_ripples()
            assert np.array_equal(_bits(got), _bits(lay.window())), what
            assert np.array_equal(_bits(got), _bits(never.read_ripples())) == (not swell), what
            assert oc.ripple_swell_device()[2] is swell and lay.current is swell, what

        both("on, never refreshed", False)
        _refresh(oc, lay, [0, 1, 2], s)
        both("refreshed", True)
        # center_ripples by a few cells clears the mark; to the same cell it does not
        oc.center_ripples((lay.ox + R // 2 + 0.5) * S, (lay.oy + R // 2 + 0.5) * S)
        assert oc.ripple_swell_device()[2] is True
        x, y = (lay.ox + 3 + R // 2 + 0.5) * S, (lay.oy - 2 + R // 2 + 0.5) * S
        oc.center_ripples(x, y)
        lay.center(x, y)
        both("moved", False)
        _refresh(oc, lay, [1], s)
        both("refreshed after the move", True)
        # set_ripple_walls, the same list
        oc.set_ripple_walls(lay.list)
        lay.set_walls(lay.list)
        both("walls set", False)
        _refresh(oc, lay, [0, 1, 2], s)
        both("refreshed after the walls", True)
        if bed:
            oc.set_ripple_bed(lay.bed, lay.depths)
            lay.set_bed(lay.bed, lay.depths)
            both("bed set", False)
            _refresh(oc, lay, [0, 1, 2], s)
            both("refreshed after the bed", True)
        # set_ripple_swell: on again starts from zeroes and a clear mark; off frees it
        oc.set_ripple_swell(True)
        lay.set_swell(True)
        assert oc.ripple_swell_device()[2] is False and not _bits(oc.read_ripple_swell()).any()
        both("on again", False)
        oc.set_ripple_swell(False)
        lay.set_swell(False)
        assert oc.ripple_swell_device() == (None, 0, False)
        both("off", False)


# -- coupled stepping


@pytest.mark.parametrize("bed", [False, True])
def test_coupled_steps_with_swell(capi, torch, oracle, bed):
    """nbodies == 0: the layer's share of a coupled call is step_ripples(h, 1) x substeps, through launch_ripple_step -- the swell's kernels"""
    R, origin, dt = 64, ORIGINS[1], 0.3
    with _setup(capi, oracle, 64, 3) as oc:
        oc.set_velocity("on")
        _step(oc)
        lay = _scene(oc, R, origin, bed)
        s = _set(capi, 0)
        _refresh(oc, lay, [0, 1, 2], s)
        imp = _impulses(np.random.default_rng(2), lay, 500)
        out = []
        for coupled in (True, False):
            oc.reset_ripples()
            oc.deposit_ripples_host(imp)
            if coupled:
                oc.step_bodies_coupled([0, 1, 2], s, None, None, None, 0, None, 0, dt, 3, None, 4)
            else:
                h = F(dt) * (F(1) / F(3))
                for _ in range(3):
                    oc.step_ripples(float(h), 1)
            out.append(oc.read_ripples())
        lay.deposit(imp)
        h = F(dt) * (F(1) / F(3))
        for _ in range(3):
            lay.step(float(h), 1)
        assert np.array_equal(_bits(out[0]), _bits(out[1])) and np.array_equal(_bits(out[0]), _bits(lay.window()))
        lay.current = False
        lay.set_window(np.zeros((R, R), F), np.zeros((R, R), F))
        lay.deposit(imp)
        for _ in range(3):
            lay.step(float(h), 1)
        assert not np.array_equal(_bits(out[0]), _bits(lay.window()))      # and not the parent's


# -- refusals


def test_refusals(capi, oracle):
    with _setup(capi, oracle, 64, 3) as oc:
        _step(oc)
        lib = capi.load()
        err = lambda: lib.datum_ocean_last_error(oc.h)
        s = _set(capi, 0)
        arr = (capi.I * 3)(0, 1, 2)
        plane = np.zeros(64 * 64, F)
        p = plane.ctypes.data_as(capi.P)
        # the layer is off
        assert lib.datum_ocean_set_ripple_swell(oc.h, 1) == capi.ESTATE and b"datum_ocean_set_ripple_swell" in err()
        assert lib.datum_ocean_set_ripple_swell(oc.h, 0) == capi.ESTATE
        assert lib.datum_ocean_set_ripple_swell(oc.h, 2) == capi.EINVAL and lib.datum_ocean_set_ripple_swell(oc.h, -1) == capi.EINVAL
        assert lib.datum_ocean_refresh_ripple_swell(oc.h, arr, 3, ctypes.byref(s), 4) == capi.ESTATE and b"layer is off" in err()
        assert lib.datum_ocean_read_ripple_swell(oc.h, p) == capi.ESTATE
        assert oc.ripple_swell_device() == (None, 0, False)
        oc.set_ripples(64, S)
        # swell is off
        assert lib.datum_ocean_refresh_ripple_swell(oc.h, arr, 3, ctypes.byref(s), 4) == capi.ESTATE and b"swell is off" in err()
        assert lib.datum_ocean_read_ripple_swell(oc.h, p) == capi.ESTATE and b"swell is off" in err()
        assert lib.datum_ocean_set_ripple_swell(oc.h, 0) == capi.OK
        oc.set_ripple_swell(True)
        # the blended sample's checks
        bad = (capi.I * 3)(0, 3, 1)
        for args in ((None, 3, ctypes.byref(s), 4), (arr, 0, ctypes.byref(s), 4), (arr, capi.MAX_CASCADES + 1, ctypes.byref(s), 4), (bad, 3, ctypes.byref(s), 4),
                     (arr, 3, None, 4), (arr, 3, ctypes.byref(s), -1), (arr, 3, ctypes.byref(s), capi.SURFACE_MAX_ITERATIONS + 1)):
            assert lib.datum_ocean_refresh_ripple_swell(oc.h, *args) == capi.EINVAL and b"datum_ocean_refresh_ripple_swell" in err(), args
            assert oc.ripple_swell_device()[2] is False
        assert lib.datum_ocean_read_ripple_swell(oc.h, None) == capi.EINVAL
        assert lib.datum_ocean_ripple_swell_device(oc.h, None, None, None) == capi.OK
        # swell and DEEP do not combine, either way round
        assert lib.datum_ocean_set_ripple_dispersion(oc.h, rs.DEEP, 9.81) == capi.ESTATE and b"swell" in err()
        oc.set_ripple_dispersion(rs.WAVE, 9.81)
        oc.set_ripple_swell(False)
        oc.set_ripple_dispersion(rs.DEEP, 9.81)
        assert lib.datum_ocean_set_ripple_swell(oc.h, 1) == capi.ESTATE and b"DEEP" in err()
        assert lib.datum_ocean_set_ripple_swell(oc.h, 0) == capi.OK and oc.ripple_swell_device() == (None, 0, False)
        oc.set_ripple_dispersion(rs.WAVE, 9.81)
        oc.set_ripple_swell(True)
        oc.refresh_ripple_swell([0, 1, 2], s, 0)
        assert oc.ripple_swell_device()[2] is True


# -- the C++ shim


def test_cpp_shim_agrees(capi, torch):
    from datum_amd import host_api

    N, R = 256, 128
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.8))
    params.seed_ocean(1000)
    with host_api.OceanContext(N) as ctx:
        oc = capi.Ocean.__new__(capi.Ocean)
        oc.lib, oc.h, oc.N, oc.cascades = capi.load(), ctx.lib.datum_host_context_handle(ctx.c), N, 1
        try:
            mesh = ctx.create_ocean(16, 16)
            params.update_ocean(np.float32(1.0 / 60.0))
            ctx.render_ocean_surface(mesh, params, host_api.example_camera())
            with pytest.raises(Exception):
                ctx.set_ocean_ripple_swell(True)                         # the layer is off
            ctx.set_ocean_ripples(R, S)
            ctx.center_ocean_ripples(3.3, -2.2)
            lay = rs.Layer(R, S)
            lay.center(3.3, -2.2)
            with pytest.raises(Exception):
                ctx.refresh_ocean_ripple_swell(params)                   # swell is off
            wl = harbour(R, lay.ox, lay.oy)
            ctx.set_ocean_ripple_walls(wl)
            lay.set_walls(wl)
            ctx.set_ocean_ripple_swell(True)
            lay.set_swell(True)
            ctx.refresh_ocean_ripple_swell(params, 4)
            s = params.oceanset(host_api.example_camera())                # (a query reads none of the camera's terms)
            lay.refresh(oc.read_surface_blend([0], s, lay.points(), 4)[:, 2].reshape(R, R))
            got = ctx.read_ocean_ripple_swell(R)
            assert np.array_equal(_bits(got), _bits(lay.F)) and np.count_nonzero(got) > 60
            assert np.array_equal(_bits(got), _bits(oc.read_ripple_swell())) and oc.ripple_swell_device()[2] is True
            # the same through the C ABI on the same handle
            oc.set_ripple_swell(True)
            oc.refresh_ripple_swell([0], s, 4)
            assert np.array_equal(_bits(oc.read_ripple_swell()), _bits(got))
            imp = _impulses(np.random.default_rng(12), lay, 2000)
            ctx.deposit_ocean_ripples(imp)
            lay.deposit(imp)
            ctx.step_ocean_ripples(H * 3, 3)
            lay.step(H * 3, 3)
            assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())) and np.abs(lay.eta).max() > 0
            ctx.set_ocean_ripple_swell(False)
            assert oc.ripple_swell_device() == (None, 0, False)
            ctx.set_ocean_ripples(0, 0.0)
        finally:
            oc.h = None
