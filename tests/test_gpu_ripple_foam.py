"""Wake foam (include/datum_ocean_hip.h: "wake foam") on the MI355X, against tests/ripple_foam64.py, bit for bit.

R = 64 is one tile of the update kernel across and four down -- the torus wrap and the window's edge meet in one tile -- R = 128 two across
and eight down; with the origin (37, -11), ox mod 64 = 37 and oy mod 16 = 5, the window's edge lies inside a tile in both directions.

  plane      after 1 and after 3 updates interleaved with step_ripples, from states that impulses made, and from the state one
             step_bodies_coupled call on a handful of bodies left (read back, so that the restatement starts from the device's bits);
             the 0xCD guards the handle keeps before and after the plane stay whole;
  scroll     center_ripples: entered cells read 0, kept cells keep their bits, a jump of R cells clears the plane; reset_ripples,
             reset_ripple_foam, set_ripples (the foam is off afterwards);
  isolation  a handle with the foam on against its twin with it off over the same calls: both state buffers, src (through a dt = 0 step),
             the FFT foam plane, the maps, step_bodies_coupled's records, bodies and motions, byte for byte;
  sampler    host twin and device call against the restatement, points on every edge, outside, non-finite and far; canaries round the output;
  shim       the C++ shim's four calls against the C ABI on the same handle;
  refusals   every ESTATE and EINVAL of the header; a refused call leaves the plane's bits.
"""

import numpy as np
import pytest

import ripple64
import ripple_foam64
from test_gpu_body import _step
from test_gpu_ripples import _bits, _bodies_inside, _guarded, _impulses, _layer, _plain, _unguard
from test_gpu_surface import _set, _setup
from test_ripple_foam_emul import DTS, ORIGINS, sample_points

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64                    # floats of 0xCD bytes the handle keeps before and after the plane


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


def _peek(torch, ptr, words):
    """`words` 32-bit words of device memory at `ptr`, as uint32 (no copy on the device: __cuda_array_interface__ of a raw pointer)"""

    class _Raw:
        pass

    r = _Raw()
    r.__cuda_array_interface__ = {"shape": (words,), "typestr": "<i4", "data": (ptr, False), "version": 2}
    return torch.as_tensor(r, device="cuda:0").cpu().numpy().view(np.uint32)


def _guards_whole(oc, torch):
    ptr, nbytes, _, _ = oc.ripple_foam_device()
    oc.read_ripple_foam()                                                # waits for the handle's stream
    return np.all(_peek(torch, ptr - 4 * GUARD, GUARD) == 0xCDCDCDCD) and np.all(_peek(torch, ptr + nbytes, GUARD) == 0xCDCDCDCD)


def _foamy(oc, torch, R, origin, seed, s=0.5):
    """a handle's layer and plane, and their restatements, a few sub-steps after random impulses strong enough to foam"""
    rng = np.random.default_rng(seed)
    lay = _layer(oc, R, s, 8, origin)
    oc.set_ripple_foam(True)
    pl = ripple_foam64.Plane(lay)
    imp = _impulses(rng, lay, 3 * R, 0.1)
    oc.deposit_ripples_host(imp)
    lay.deposit(imp)
    oc.step_ripples(0.09, 3)
    lay.step(0.09, 3)
    return lay, pl


def _same_plane(oc, pl, what):
    got, want = oc.read_ripple_foam(), pl.window()
    assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:4])
    return got


# -- the plane


@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("origin", ORIGINS)
def test_plane_bits(capi, torch, R, origin):
    with _plain(capi) as oc:
        lay, pl = _foamy(oc, torch, R, origin, R + origin[0])
        assert oc.ripple_foam_device()[1:] == (R * R * 4, *origin) and np.all(_bits(oc.read_ripple_foam()) == 0)
        for k, dt in enumerate(DTS):
            oc.step_ripple_foam(dt)
            pl.step(dt)
            if k != 1:
                got = _same_plane(oc, pl, (R, origin, k))
                assert got.min() >= 0 and got.max() <= 1
            # it wrote the plane only: the layer's state is the restatement's, before and after a step
            assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))
            oc.step_ripples(dt, 2)
            lay.step(dt, 2)
        assert np.any((got > 0) & (got < 1)) and np.any(got == 0) and np.any(got == 1)
        edge = np.concatenate([got[0], got[-1], got[:, 0], got[:, -1]])
        assert np.any(edge > 0)
        assert _guards_whole(oc, torch)


def test_plane_after_coupled_step(capi, oracle, torch):
    """the state one step_bodies_coupled call leaves under a handful of hulls; other parameters than the defaults"""
    R, cell, origin, cascades = 128, 1.0, (-27, -59), [0, 1]             # ox mod 64 = 37, oy mod 16 = 5; the hulls lie within 20 m of (0, 0)
    bodies, motions, probes = _bodies_inside(5, nb=6, per=32)
    props = np.zeros(len(bodies), capi.BODY_PROPS_DTYPE)
    props["invmass"], props["invinertia"], props["gravity"], props["buoyancy"] = 0.01, 0.01, 9.81, 9810.0
    kw = dict(t1=1e-4, k1=60.0, t2=0.02, k2=4.0, decay=1.5)
    with _setup(capi, oracle, 64, 2) as oc:
        oc.set_velocity("on")
        _step(oc, 1)
        lay = _layer(oc, R, cell, 8, origin)
        oc.set_ripple_foam(True)
        oc.set_ripple_foam_params(**kw)
        pl = ripple_foam64.Plane(lay, **kw)
        for k, dt in enumerate((0.05, 0.03)):
            oc.step_bodies_coupled_host(cascades, _set(capi, 0), bodies, motions, props, probes, dt, 2, 4)
            state = oc.read_ripples()
            lay.set_window(state[..., 0], state[..., 1])
            oc.step_ripple_foam(dt)
            pl.step(dt)
            got = _same_plane(oc, pl, k)
        assert np.abs(state).max() > 0 and np.count_nonzero(got) > 20 and np.any((got > 0) & (got < 1))
        assert _guards_whole(oc, torch)


# -- scroll, reset, set


def test_scroll_reset_and_set(capi, torch):
    R, s, origin = 64, 0.5, ORIGINS[1]
    with _plain(capi) as oc:
        lay, pl = _foamy(oc, torch, R, origin, 21)
        oc.step_ripple_foam(0.05)
        pl.step(0.05)
        before = _same_plane(oc, pl, "before")
        assert np.count_nonzero(before) > 50

        def center(di, dj):
            x, y = (lay.ox + di + R // 2 + 0.5) * s, (lay.oy + dj + R // 2 + 0.5) * s
            oc.center_ripples(x, y)
            pl.move(lay.ox + di, lay.oy + dj)
            lay.center(x, y)
            assert oc.ripple_foam_device()[2:] == (lay.ox, lay.oy)

        center(5, -3)
        got = _same_plane(oc, pl, "moved")
        # kept cells keep their bits, entered cells read 0: window cell (i, j) was (i + 5, j - 3)
        assert np.array_equal(_bits(got[3:, :R - 5]), _bits(before[:R - 3, 5:])) and np.all(_bits(got[:3]) == 0) and np.all(_bits(got[:, R - 5:]) == 0)
        assert np.count_nonzero(got) > 20
        # an update on the moved window: the new edge is the border now
        oc.step_ripple_foam(0.02)
        pl.step(0.02)
        _same_plane(oc, pl, "moved, updated")
        center(-5, 3)
        assert np.count_nonzero(_same_plane(oc, pl, "back")) > 10
        center(R, 0)                                                     # a jump of R cells clears the plane
        assert np.all(_bits(_same_plane(oc, pl, "jump")) == 0)
        assert _guards_whole(oc, torch)

        # reset_ripple_foam leaves the layer, reset_ripples clears both
        lay2, pl2 = _foamy(oc, torch, R, origin, 22)                      # (set_ripples again: the foam was off, and is on again)
        oc.step_ripple_foam(0.05)
        assert np.count_nonzero(oc.read_ripple_foam()) > 50
        state = oc.read_ripples()
        oc.reset_ripple_foam()
        assert np.all(_bits(oc.read_ripple_foam()) == 0) and np.array_equal(_bits(oc.read_ripples()), _bits(state))
        oc.step_ripple_foam(0.05)
        assert np.count_nonzero(oc.read_ripple_foam()) > 50
        oc.reset_ripples()
        assert np.all(_bits(oc.read_ripple_foam()) == 0) and np.all(_bits(oc.read_ripples()) == 0)
        # set_ripple_foam(True) a second time zero-fills; set_ripples switches the foam off, with any R
        imp = _impulses(np.random.default_rng(5), lay2, 100, 0.1)
        oc.deposit_ripples_host(imp)
        oc.step_ripples(0.09, 3)
        oc.step_ripple_foam(0.05)
        assert np.count_nonzero(oc.read_ripple_foam()) > 20
        oc.set_ripple_foam(True)
        assert np.all(_bits(oc.read_ripple_foam()) == 0) and np.abs(oc.read_ripples()).max() > 0
        for R2 in (64, 128, 0):
            if R2:
                oc.set_ripple_foam(True)
            oc.set_ripples(R2, s)
            with pytest.raises(capi.OceanError) as e:
                oc.read_ripple_foam()
            assert e.value.code == capi.ESTATE and ("wake foam is off" if R2 else "ripple layer is off") in str(e.value)


# -- isolation


def test_isolation(capi, oracle, torch):
    """with the foam on, updated, scrolled and sampled, every other output of the handle is that of a handle without it"""
    N, R, cascades = 64, 128, [0, 1]
    bodies, motions, probes = _bodies_inside(8, nb=6, per=32)
    props = np.zeros(len(bodies), capi.BODY_PROPS_DTYPE)
    props["invmass"], props["invinertia"], props["gravity"], props["buoyancy"] = 0.01, 0.01, 9.81, 9810.0
    rng = np.random.default_rng(8)
    lay = ripple64.Layer(R, 1.0)
    imps = [_impulses(rng, lay, 300, 0.3) for _ in range(3)]
    pts = rng.uniform(-70, 70, (256, 2)).astype(F)
    out = []
    for on in (False, True):
        with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
            oc.set_velocity("on")
            s = _set(capi, 0)
            oc.set_ripples(R, 1.0)
            foam = (lambda dt: oc.step_ripple_foam(dt)) if on else (lambda dt: None)
            if on:
                oc.set_ripple_foam(True)
            ptrs = set()
            for k in range(3):
                _step(oc, 1)
                oc.deposit_ripples_host(imps[k])
                foam(0.05)
                ptrs.add(oc.ripples_device()[0])
                oc.step_ripples(0.05, 1)
                ptrs.add(oc.ripples_device()[0])
                foam(0.05)
                oc.center_ripples(3.0 * k, -2.0 * k)
                foam(0.0)
            b, m = bodies.copy(), motions.copy()
            rec = oc.step_bodies_coupled_host(cascades, s, b, m, props, probes, 0.04, 2, 4)
            foam(0.04)
            if on:
                cover = oc.query_ripple_foam(pts)
                assert np.count_nonzero(oc.read_ripple_foam()) > 50 and np.count_nonzero(cover) > 5
            current = oc.read_ripples()
            assert len(ptrs) == 2 and np.abs(current).max() > 0
            both = [_peek(torch, p, R * R * 2) for p in sorted(ptrs, key=lambda p: p != oc.ripples_device()[0])]   # the current buffer first
            # src: pending deposits become heights in a dt = 0 step
            oc.deposit_ripples_host(imps[0])
            foam(0.05)
            oc.step_ripples(0.0, 1)
            after = oc.read_ripples()
            assert not np.array_equal(after, current)
            out.append([oc.read_maps(c) for c in cascades] + [oc.read_foam(c) for c in cascades] + [oc.read_state(c) for c in cascades]
                       + [current, after, rec, b.view(np.uint8), m.view(np.uint8)] + both)
            if on:
                assert _guards_whole(oc, torch)
    for k, (x, y) in enumerate(zip(*out)):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), k


# -- the sampler, its host twin


@pytest.mark.parametrize("R", [64, 128])
def test_sampler(capi, torch, R):
    origin = ORIGINS[1]
    with _plain(capi) as oc:
        lay, pl = _foamy(oc, torch, R, origin, R + 3)
        oc.step_ripple_foam(0.05)
        pl.step(0.05)
        _same_plane(oc, pl, R)
        pts, k = sample_points(R, origin, 0.5, R, 600)
        want = pl.sample(pts)
        nan = np.isnan(want)
        assert nan[k:k + 3].all() and nan.sum() == 3 and np.all(_bits(want[k + 3:k + 6]) == 0) and np.count_nonzero(want[~nan]) > 20
        got = oc.query_ripple_foam(pts)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), np.argwhere(_bits(got) != _bits(want))[:4]
        # device arrays, canaries before and after the output; an odd count, and one point alone
        dp = torch.from_numpy(pts).cuda()
        for n in (len(pts), 257, 1):
            out, ptr = _guarded(torch, n)
            oc.sample_ripple_foam(dp.data_ptr(), n, ptr)
            oc.read_ripple_foam()
            o = _unguard(out, n)
            assert np.array_equal(np.isnan(o), nan[:n]) and np.array_equal(_bits(o)[~nan[:n]], _bits(want[:n])[~nan[:n]]), n
        # n == 0 enqueues nothing, whatever the pointers
        oc.sample_ripple_foam(None, 0, None)
        assert len(oc.query_ripple_foam(np.zeros((0, 2), F))) == 0
        assert _guards_whole(oc, torch)


# -- the C++ shim


def test_cpp_shim_reaches_the_same_bits(capi, torch):
    from datum_amd import host_api

    N, R, cell, origin = 256, 64, 0.5, ORIGINS[1]
    rng = np.random.default_rng(31)
    with host_api.OceanContext(N) as ctx:
        with pytest.raises(Exception):
            ctx.set_ocean_ripple_foam(True)                              # the layer is off
        # the shim's own handle behind a capi.Ocean that does not own it
        oc = capi.Ocean.__new__(capi.Ocean)
        oc.lib, oc.h, oc.N, oc.cascades = capi.load(), ctx.lib.datum_host_context_handle(ctx.c), N, 1
        try:
            ctx.set_ocean_ripples(R, cell)
            with pytest.raises(Exception):
                ctx.step_ocean_ripple_foam(0.05)                         # the foam is off
            x, y = (origin[0] + R // 2 + 0.5) * cell, (origin[1] + R // 2 + 0.5) * cell
            ctx.center_ocean_ripples(x, y)
            lay = ripple64.Layer(R, cell)
            lay.center(x, y)
            pl = ripple_foam64.Plane(lay)
            ctx.set_ocean_ripple_foam(True)
            imp = _impulses(rng, lay, 3 * R, 0.1)
            ctx.deposit_ocean_ripples(imp)
            lay.deposit(imp)
            for dt in DTS[:2]:
                ctx.step_ocean_ripples(dt * 2, 2)
                lay.step(dt * 2, 2)
                ctx.step_ocean_ripple_foam(dt)
                pl.step(dt)
            pts, _ = sample_points(R, origin, cell, 5)
            plane, cover = ctx.read_ocean_ripple_foam(R), ctx.query_ocean_ripple_foam(pts)
            assert np.array_equal(_bits(plane), _bits(oc.read_ripple_foam())) and np.array_equal(_bits(plane), _bits(pl.window()))
            assert np.array_equal(_bits(cover), _bits(oc.query_ripple_foam(pts))) and np.count_nonzero(plane) > 50
            ctx.set_ocean_ripple_foam(False)
            with pytest.raises(Exception):
                ctx.read_ocean_ripple_foam(R)
        finally:
            oc.h = None


# -- the off states and the refusals that need a device


def test_off_and_refusals(capi, torch):
    R, origin = 64, ORIGINS[1]
    pts = np.zeros((4, 2), F)
    with _plain(capi) as oc:
        lib = capi.load()
        needs = (oc.reset_ripple_foam, oc.ripple_foam_device, oc.read_ripple_foam, lambda: oc.step_ripple_foam(0.1), lambda: oc.sample_ripple_foam(None, 0, None),
                 lambda: oc.query_ripple_foam(pts))
        # the layer is off: every call but the parameters', the layer looked at first
        for call in needs + (lambda: oc.set_ripple_foam(True), lambda: oc.set_ripple_foam(False)):
            with pytest.raises(capi.OceanError) as e:
                call()
            assert e.value.code == capi.ESTATE and "ripple layer is off" in str(e.value)
        nan, inf = float("nan"), float("inf")
        for args in [(nan, 10.0, 0.5, 2.0, 0.5), (0.04, 10.0, inf, 2.0, 0.5), (0.04, -1.0, 0.5, 2.0, 0.5), (0.04, nan, 0.5, 2.0, 0.5), (0.04, 10.0, 0.5, -1e-9, 0.5),
                     (0.04, 10.0, 0.5, inf, 0.5), (0.04, 10.0, 0.5, 2.0, -0.5), (0.04, 10.0, 0.5, 2.0, nan)]:
            assert lib.datum_ocean_set_ripple_foam_params(oc.h, *args) == capi.EINVAL and b"datum_ocean_set_ripple_foam_params" in lib.datum_ocean_last_error(oc.h)
        oc.set_ripple_foam_params(-1.0, 0.0, -1.0, 0.0, 0.0)             # thresholds of any sign, gains and decay of 0
        oc.set_ripple_foam_params()
        # the layer is on, the foam is off
        lay, pl = _foamy(oc, torch, R, origin, 41)
        oc.set_ripple_foam(False)
        for call in needs:
            with pytest.raises(capi.OceanError) as e:
                call()
            assert e.value.code == capi.ESTATE and "wake foam is off" in str(e.value)
        oc.set_ripple_foam(False)                                        # off twice is fine
        oc.set_ripple_foam(True)
        ptr = oc.ripple_foam_device()[0]
        oc.step_ripple_foam(0.05)
        pl.step(0.05)
        before = _same_plane(oc, pl, "before")
        assert np.count_nonzero(before) > 50
        # refused calls leave the plane's bits
        dp = torch.zeros(16, dtype=torch.float32, device="cuda")
        Pn = capi.P
        for dt in (-0.1, -1e-9, nan, inf, -inf):
            assert lib.datum_ocean_step_ripple_foam(oc.h, dt) == capi.EINVAL and b"datum_ocean_step_ripple_foam" in lib.datum_ocean_last_error(oc.h)
        for name in ("datum_ocean_sample_ripple_foam", "datum_ocean_query_ripple_foam"):
            fn = getattr(lib, name)
            for args in [(None, 2, Pn(dp.data_ptr())), (Pn(dp.data_ptr()), 2, None), (Pn(dp.data_ptr() + 4), 2, Pn(dp.data_ptr())), (Pn(dp.data_ptr()), 2, Pn(dp.data_ptr() + 2)),
                         (Pn(dp.data_ptr()), 2 ** 31, Pn(dp.data_ptr()))]:
                assert fn(oc.h, *args) == capi.EINVAL and name.encode() in lib.datum_ocean_last_error(oc.h), (name, args)
        assert lib.datum_ocean_ripple_foam_device(oc.h, None, None, None, None) == capi.EINVAL and lib.datum_ocean_read_ripple_foam(oc.h, None) == capi.EINVAL
        assert np.array_equal(_bits(oc.read_ripple_foam()), _bits(before)) and np.all(dp.cpu().numpy() == 0)
        # dt = 0 is legal: fade = 1, the plane can only grow; the pointer does not alternate
        oc.step_ripples(0.05, 1)
        lay.step(0.05, 1)
        oc.step_ripple_foam(0.0)
        pl.step(0.0)
        got = _same_plane(oc, pl, "dt = 0")
        assert np.all(got >= before) and oc.ripple_foam_device()[0] == ptr
        assert _guards_whole(oc, torch)
        oc.set_ripples(0)
        with pytest.raises(capi.OceanError) as e:
            oc.step_ripple_foam(0.1)
        assert e.value.code == capi.ESTATE and "ripple layer is off" in str(e.value)
