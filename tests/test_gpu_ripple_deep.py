"""The ripple layer's DEEP step (include/datum_ocean_hip.h: "dispersive ripples") on the MI355X, against tests/ripple_deep64.py with the
table datum_ocean_ripple_deep_weights returns.

R = 64 is one tile of the step kernel across -- the six-cell halo wraps onto the tile itself -- and four down, R = 128 two across and eight
down; with the origin (37, -21) the window's seam falls inside a tile, in both directions, with (0, 0) on a tile's edge.

  step      bit for bit against the fp32 restatement after 1, 3 and 16 sub-steps, the sponge on (B = 8) and off, from deposits within six
            cells of every window edge and corner and on both sides of the torus seam plus random ones; a second step without deposits;
            within K_RIP_DEEP eps max|eta| of float64; the buffer a sub-step reads keeps its bits; the 0xCD guards the handle keeps
            before and after BOTH state buffers stay whole, in every case;
  modes     WAVE after a round trip through DEEP gives ripple64's bits; a switch between two calls behaves as two layers would; the
            setting survives set_ripples and works while the layer is off;
  refusals  the bound at 1.9 on both sides, dt < 0, ESTATE while the layer is off, in step_ripples and in step_bodies_coupled;
  coupled   step_bodies_coupled in DEEP against the manual sequence bit for bit (the host twin and the device call); nbodies == 0 equals
            step_ripples(h, 1) x substeps;
  bounds    a read_ripple_bounds after a DEEP step reflects the new state;
  shim      set_ocean_ripple_dispersion and step_ocean_ripples through datum_amd/host against the C ABI on the same handle.
"""

import numpy as np
import pytest

import couple64
import ripple64
import ripple_deep64 as rd
from test_gpu_couple import _same, _two_boxes
from test_gpu_ripple_foam import _peek
from test_gpu_ripples import ORIGIN, _deposit, _impulses, _plain
from test_gpu_step import _flat
from test_gpu_surface import _set

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -24
S = 0.5
H = 0.1                       # a sub-step: h sqrt(g sum|F| / s) = 1.03 at s = 0.5
GUARD = 64                    # 32-bit words of 0xCD bytes the handle keeps before and after each state buffer


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


def _guards_whole(torch, ptr, nbytes):
    """the canaries before and after the state buffer at `ptr`"""
    return bool(np.all(_peek(torch, ptr - 4 * GUARD, GUARD) == 0xCDCDCDCD) and np.all(_peek(torch, ptr + nbytes, GUARD) == 0xCDCDCDCD))


def _both_guards_whole(oc, torch):
    """both state buffers: the current one, and the other, which a step of dt = 0 from here makes current (and one more puts back)"""
    a, nbytes = oc.ripples_device()[:2]
    oc.step_ripples(0.0, 1)
    b = oc.ripples_device()[0]
    oc.read_ripples()                                                    # waits for the handle's stream
    return a != b and _guards_whole(torch, a, nbytes) and _guards_whole(torch, b, nbytes)


def _layer(oc, table, R, B, origin, dtype=F, mode=rd.DEEP, g=9.81):
    """the handle's layer and its restatement, both in `mode` with the window's origin at `origin`"""
    oc.set_ripple_params(2.0, 0.05, B, 4.0)
    oc.set_ripple_dispersion(mode, g)
    oc.set_ripples(R, S)
    lay = rd.Layer(R, S, dtype, 2.0, 0.05, B, 4.0, mode=mode, g=g, G=table)
    x, y = (origin[0] + R // 2 + 0.5) * S, (origin[1] + R // 2 + 0.5) * S
    oc.center_ripples(x, y)
    lay.center(x, y)
    assert (lay.ox, lay.oy) == origin and oc.ripples_device()[2:] == origin
    return lay


def _edge_impulses(lay):
    """a deposit on a cell centre within six cells of every window edge and corner, and on both sides of the torus seam in memory"""
    R, ox, oy = lay.R, lay.ox, lay.oy
    near = (0, 2, 5, R - 6, R - 3, R - 1)
    cells = [(i, j) for i in near for j in near]                                            # the four corners' 6 x 6 neighbourhoods, sampled
    cells += [(i, R // 2) for i in near] + [(R // 3, j) for j in near]                       # the four edges
    sx, sy = (-ox) & (R - 1), (-oy) & (R - 1)                                               # window coordinates of memory column / row 0
    cells += [((sx + d) & (R - 1), R // 4) for d in (-3, -1, 0, 2)] + [(R // 4 + 1, (sy + d) & (R - 1)) for d in (-3, -1, 0, 2)]
    imp = np.zeros((len(cells), 4), F)
    for k, (i, j) in enumerate(cells):
        imp[k] = ((ox + i + 0.5) * S, (oy + j + 0.5) * S, 0.01 * (1 + k % 7) * (-1) ** k, 0)
    return imp


# -- step


@pytest.mark.parametrize("R,B,origin", [(R, B, o) for R in (64, 128) for B in (8, 0) for o in ((0, 0), ORIGIN)])
def test_step_bits(capi, torch, table, report, R, B, origin):
    rng = np.random.default_rng(R + B)
    with _plain(capi) as oc:
        lay = _layer(oc, table, R, B, origin)
        l64 = rd.Layer(R, S, np.float64, 2.0, 0.05, B, 4.0, G=table)
        l64.move(*origin)
        keep, worst = [], 0.0
        for substeps in (1, 3, 16):
            imp = np.concatenate([_edge_impulses(lay), _impulses(rng, lay, R * R // 4)])
            keep.append(_deposit(oc, torch, imp))
            lay.deposit(imp)
            # (K_RIP_DEEP bounds one call from a common fp32 state: float64 starts where the restatement stands)
            l64.eta, l64.rate, l64.src = lay.eta.astype(np.float64), lay.rate.astype(np.float64), lay.src.copy()
            oc.step_ripples(H * substeps, substeps)
            lay.step(H * substeps, substeps)
            l64.step(H * substeps, substeps)
            got = oc.read_ripples()
            assert np.array_equal(_bits(got), _bits(lay.window())), (R, B, origin, substeps, np.argwhere(_bits(got) != _bits(lay.window()))[:4])
            err = np.abs(got[..., 0].astype(np.float64) - l64.window()[..., 0]).max() / (EPS * np.abs(l64.eta).max())
            worst = max(worst, err)
            # a second step without deposits (src was cleared behind the first sub-step); the buffer its one sub-step reads keeps its bits
            ptr, nbytes = oc.ripples_device()[:2]
            oc.step_ripples(H, 1)
            lay.step(H, 1)
            after = oc.read_ripples()
            assert np.array_equal(_bits(after), _bits(lay.window())), (R, B, origin, substeps, "second")
            assert oc.ripples_device()[0] != ptr
            read = _peek(torch, ptr, nbytes // 4).view(np.float32).reshape(R, R, 2)
            assert np.array_equal(_bits(lay.window(read)), _bits(got)), "the sub-step wrote the buffer it reads"
            # canaries before and after both state buffers (`ptr` is the other one now)
            cur = oc.ripples_device()[0]
            assert _guards_whole(torch, ptr, nbytes) and _guards_whole(torch, cur, nbytes), (R, B, origin, substeps, "guards")
        line = f"DEEP ripples R={R} B={B} origin={origin}: |device - float64| / (eps max|eta|) = {worst:.2f}, K_RIP_DEEP = {rd.K_RIP_DEEP}"
        print(line)
        report(line)
        assert np.abs(after[..., 0]).max() > 1e-3 and np.isfinite(after).all()
        assert worst <= rd.K_RIP_DEEP


# -- modes


def test_mode_round_trip_and_switch(capi, torch, table):
    R, B = 64, 8
    rng = np.random.default_rng(4)
    with _plain(capi) as oc:
        oc.set_ripple_dispersion(capi.RIPPLE_DEEP, 5.0)                  # while the layer is off; survives set_ripples
        oc.set_ripple_params(2.0, 0.05, B, 4.0)
        oc.set_ripples(R, S)
        oc.set_ripple_dispersion(capi.RIPPLE_WAVE, 5.0)
        lay = _layer(oc, table, R, B, ORIGIN, mode=rd.WAVE)
        wave = ripple64.Layer(R, S, F, 2.0, 0.05, B, 4.0)
        wave.move(*ORIGIN)
        imp = _impulses(rng, lay, R * R)
        d = _deposit(oc, torch, imp)
        lay.deposit(imp)
        wave.deposit(imp)
        # WAVE after a round trip through DEEP: ripple64's own bits
        oc.set_ripple_dispersion(capi.RIPPLE_DEEP)
        oc.set_ripple_dispersion(capi.RIPPLE_WAVE)
        oc.step_ripples(0.3, 3)
        wave.step(0.3, 3)
        lay.step(0.3, 3)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(wave.window())) and np.array_equal(_bits(lay.state()), _bits(wave.state()))
        # a switch between two calls: the state is common, each call steps in its own mode; g is taken as given
        for mode, g in ((rd.DEEP, 9.81), (rd.WAVE, 9.81), (rd.DEEP, 3.0)):
            oc.set_ripple_dispersion(mode, g)
            lay.mode, lay.g = mode, g
            oc.step_ripples(0.2, 2)
            lay.step(0.2, 2)
            assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window())), (mode, g)
        # the setting survives set_ripples: the new layer steps in DEEP with g = 3
        oc.set_ripples(R, S)
        fresh = rd.Layer(R, S, F, 2.0, 0.05, B, 4.0, g=3.0, G=table)
        imp = _impulses(rng, fresh, R * R)
        oc.deposit_ripples_host(imp)
        fresh.deposit(imp)
        oc.step_ripples(0.2, 2)
        fresh.step(0.2, 2)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(fresh.window())) and np.abs(fresh.eta).max() > 0
        assert _both_guards_whole(oc, torch)
        del d


# -- refusals


def test_refusals(capi, table):
    with _plain(capi) as oc:
        lib = capi.load()
        oc.set_ripple_dispersion(capi.RIPPLE_DEEP)
        with pytest.raises(capi.OceanError) as e:
            oc.step_ripples(0.1, 1)
        assert e.value.code == capi.ESTATE and "ripple layer is off" in str(e.value)
        for mode, g in [(2, 9.81), (-1, 9.81), (1, 0.0), (1, -9.81), (1, float("nan")), (1, float("inf")), (0, 0.0)]:
            assert lib.datum_ocean_set_ripple_dispersion(oc.h, mode, g) == capi.EINVAL and b"datum_ocean_set_ripple_dispersion" in lib.datum_ocean_last_error(oc.h)
        oc.set_ripples(64, S)
        # the bound: h sqrt(g sum|F| / s) against 1.9, on both sides; c h / s = 0.74 would be refused in WAVE and is not looked at here
        k = np.sqrt(float(F(9.81)) * rd.mass(table) / S)
        lo, hi = F(1.899 / k), F(1.901 / k)
        assert rd.stable(9.81, S, lo, 1, table) and not rd.stable(9.81, S, hi, 1, table) and 2.0 * float(lo) / S > 0.7
        oc.step_ripples(float(lo), 1)
        oc.step_ripples(float(lo) * 4, 4)
        assert lib.datum_ocean_step_ripples(oc.h, float(hi), 1) == capi.EINVAL
        assert b"datum_ocean_step_ripples" in lib.datum_ocean_last_error(oc.h) and b"1.9" in lib.datum_ocean_last_error(oc.h)
        assert lib.datum_ocean_step_ripples(oc.h, float(hi) * 4, 4) == capi.EINVAL
        # a larger g tightens it; WAVE does not know it
        oc.set_ripple_dispersion(capi.RIPPLE_DEEP, 4 * 9.81)
        assert lib.datum_ocean_step_ripples(oc.h, float(lo), 1) == capi.EINVAL
        oc.step_ripples(float(lo), 2)
        for dt, sub in [(-0.01, 1), (-1e-9, 4), (np.nan, 1), (np.inf, 1), (0.01, 0), (0.01, 17)]:
            assert lib.datum_ocean_step_ripples(oc.h, float(dt), sub) == capi.EINVAL and b"datum_ocean_step_ripples" in lib.datum_ocean_last_error(oc.h)
        oc.step_ripples(0.0, 1)
        oc.set_ripple_dispersion(capi.RIPPLE_WAVE)
        assert lib.datum_ocean_step_ripples(oc.h, float(lo), 1) == capi.EINVAL and b"0.7" in lib.datum_ocean_last_error(oc.h)
        assert np.all(oc.read_ripples() == 0)


# -- coupled stepping


def test_coupled_in_deep(capi, torch, table):
    bodies, motions, props, probes = _two_boxes()
    R, K, dt = 64, 2, 0.1
    with _flat(capi) as oc:
        s = _set(capi, 0, swell=False, plane_w=-0.25)
        oc.set_ripple_dispersion(capi.RIPPLE_DEEP)
        # ESTATE while the layer is off, then the DEEP bound in the coupled call's name
        with pytest.raises(capi.OceanError) as e:
            oc.step_bodies_coupled_host([0], s, bodies.copy(), motions.copy(), props, probes, dt, K, 4)
        assert e.value.code == capi.ESTATE
        oc.set_ripples(R, S)
        with pytest.raises(capi.OceanError) as e:
            oc.step_bodies_coupled_host([0], s, bodies.copy(), motions.copy(), props, probes, 0.4, 2, 4)      # h = 0.2: 2.05
        assert e.value.code == capi.EINVAL and "datum_ocean_step_bodies_coupled_host" in str(e.value) and "1.9" in str(e.value)
        assert np.all(oc.read_ripples() == 0)
        oc.step_bodies_coupled_host([0], s, bodies.copy(), motions.copy(), props, probes, 0.36, 2, 4)        # h = 0.18: 1.85; c h / s = 0.72
        oc.reset_ripples()

        lay = rd.Layer(R, S, G=table)
        recs = np.zeros((len(couple64.points32(bodies, probes)), 8), F)
        recs[:, 2] = 0.25
        wb, wm = bodies, motions
        gb, gm = bodies.copy(), motions.copy()
        for _ in range(2):
            wb, wm, wr = couple64.call32(lay, wb, wm, props, probes, lambda b: recs, dt, K)
            gr = oc.step_bodies_coupled_host([0], s, gb, gm, props, probes, dt, K, 4)
            _same((gb, gm, gr), (wb, wm, wr), "DEEP, host twin")
        state = oc.read_ripples()
        assert np.array_equal(_bits(state), _bits(lay.window())) and np.abs(lay.eta).max() > 1e-3

        # the manual sequence in WAVE gives another layer: the mode was felt
        oc.reset_ripples()
        oc.set_ripple_dispersion(capi.RIPPLE_WAVE)
        hb, hm = bodies.copy(), motions.copy()
        for _ in range(2):
            oc.step_bodies_coupled_host([0], s, hb, hm, props, probes, dt, K, 4)
        assert not np.array_equal(_bits(oc.read_ripples()), _bits(state))

        # the device call against the host twin
        oc.reset_ripples()
        oc.set_ripple_dispersion(capi.RIPPLE_DEEP)
        nb = len(bodies)
        dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(nb, -1).copy()).cuda() for a in (bodies, motions, props)]
        dp = torch.from_numpy(np.ascontiguousarray(probes, F)).cuda()
        rec = torch.zeros(nb * 12, dtype=torch.float32, device="cuda")
        for _ in range(2):
            oc.step_bodies_coupled([0], s, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), nb, dp.data_ptr(), len(probes), dt, K, rec.data_ptr(), 4)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(state))
        assert np.array_equal(dev[0].cpu().numpy().ravel(), gb.view(np.uint8).ravel()) and np.array_equal(dev[1].cpu().numpy().ravel(), gm.view(np.uint8).ravel())
        assert np.array_equal(_bits(rec.cpu().numpy().reshape(nb, 12)), _bits(gr))
        assert _both_guards_whole(oc, torch)

        # nbodies == 0: step_ripples(h, 1) x substeps
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


# -- the bounds' mark


def test_bounds_mark_is_cleared(capi, torch, table):
    R = 64
    with _plain(capi) as oc:
        lay = _layer(oc, table, R, 8, ORIGIN)
        imp = _impulses(np.random.default_rng(8), lay, 400)
        d = _deposit(oc, torch, imp)
        lay.deposit(imp)
        before = oc.read_ripple_bounds()
        assert before[0] == 0 and before[1] == 0
        oc.set_ripple_dispersion(capi.RIPPLE_DEEP)                        # the setter leaves the mark alone: the record stays usable
        oc.step_ripples(H * 2, 2)
        lay.step(H * 2, 2)
        got = oc.read_ripple_bounds()
        w = lay.window()
        assert got[0] == w[..., 0].min() and got[1] == w[..., 0].max() and got[2] == w[..., 1].min() and got[3] == w[..., 1].max()
        assert got[1] > 0 > got[0]
        del d


# -- the C++ shim


def test_cpp_shim_reaches_the_same_bits(capi, torch, table):
    from datum_amd import host_api

    N, R = 256, 128
    rng = np.random.default_rng(12)
    with host_api.OceanContext(N) as ctx:
        oc = capi.Ocean.__new__(capi.Ocean)
        oc.lib, oc.h, oc.N, oc.cascades = capi.load(), ctx.lib.datum_host_context_handle(ctx.c), N, 1
        try:
            ctx.set_ocean_ripple_dispersion(1, 9.81)                     # while the layer is off
            with pytest.raises(Exception):
                ctx.set_ocean_ripple_dispersion(2, 9.81)
            with pytest.raises(Exception):
                ctx.set_ocean_ripple_dispersion(1, 0.0)
            ctx.set_ocean_ripples(R, S)
            ctx.center_ocean_ripples(3.3, -2.2)
            lay = rd.Layer(R, S, G=table)
            lay.center(3.3, -2.2)
            imp = _impulses(rng, lay, 2000)
            ctx.deposit_ocean_ripples(imp)
            lay.deposit(imp)
            ctx.step_ocean_ripples(H * 3, 3)
            lay.step(H * 3, 3)
            state = oc.read_ripples()
            assert np.array_equal(_bits(state), _bits(lay.window())) and np.abs(state).max() > 0
            # the same through the C ABI on the same handle
            oc.reset_ripples()
            d = _deposit(oc, torch, imp)
            oc.set_ripple_dispersion(capi.RIPPLE_DEEP, 9.81)
            oc.step_ripples(H * 3, 3)
            assert np.array_equal(_bits(oc.read_ripples()), _bits(state))
            ctx.set_ocean_ripple_dispersion(0)
            oc.reset_ripples()
            oc.deposit_ripples_host(imp)
            ctx.step_ocean_ripples(H * 3, 3)
            wave = ripple64.Layer(R, S)
            wave.center(3.3, -2.2)
            wave.deposit(imp)
            wave.step(H * 3, 3)
            assert np.array_equal(_bits(oc.read_ripples()), _bits(wave.window()))
            del d
            ctx.set_ocean_ripples(0, 0.0)
        finally:
            oc.h = None
