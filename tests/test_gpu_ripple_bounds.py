"""GPU tests of the ripple layer's bounds, the rippled slab and the bounded rippled cast (include/datum_ocean_hip.h: "ripple-layer bounds"):
the record against numpy over read_ripples (by value, the counts exactly), the CURRENT mark through every call the header lists, the
bounded rippled cast against cast_rays_rippled bit for bit, the slab against tests/ripple_bounds64.py bit for bit, and that nothing else
moved.  N = 64 x 3 cascades is the PLAIN map layout, 2048^2 x 2 the BANDED one; R = 64 and 128 with the origin (37, -21) wrap the window
round the torus in memory; R = 1024 is the reduction's grid-stride loop and the cap on its workgroups.
"""

import ctypes

import numpy as np
import pytest

import bounds64
import ripple_bounds64
from test_gpu_body import _step
from test_gpu_couple import _bodies, _prime
from test_gpu_rays import _rays
from test_gpu_ripples import ORIGIN, _impulses, _plain
from test_gpu_surface import DT, _set, _setup

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 0xCDCDCDCD            # the module fills the guards round the partials and the record with 0xCD bytes once


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


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_record(got, want):
    return np.array_equal(got[:4], want[:4]) and _bits(got[4:]).tolist() == _bits(want[4:]).tolist()


def _groups(R):
    return min(256, R * R // 512)


def _device(capi, oc, ptr, nbytes):
    out = np.zeros(nbytes // 4, np.uint32)
    assert capi.load().datum_ocean_device_read(oc.h, out.ctypes.data_as(capi.P), capi.P(ptr), nbytes) == capi.OK
    return out


def _guards_whole(capi, oc, R):
    """the 32 bytes before the partials, between them and the record, and behind the record"""
    rec, n = oc.ripple_bounds_device()
    assert n == 32
    G = _groups(R)
    for at in (rec - 32 - G * 32 - 32, rec - 32, rec + 32):
        assert np.all(_device(capi, oc, at, 32) == GUARD), (R, at - rec)


def _check_record(capi, oc, R, tag):
    got = oc.read_ripple_bounds()
    want = ripple_bounds64.fold(oc.read_ripples())
    assert _same_record(got, want), (tag, got, want)
    _guards_whole(capi, oc, R)
    # the record on the device is the one that was read
    rec, _ = oc.ripple_bounds_device()
    assert np.array_equal(_device(capi, oc, rec, 32), _bits(got)), tag
    return got


# 1 -- the record


@pytest.mark.parametrize("R,cell", [(64, 1.0), (128, 0.5)])
def test_record(capi, oracle, R, cell):
    cascades = [0, 1, 2]
    with _setup(capi, oracle, 64, 3) as oc:
        oc.set_velocity("on")                                                    # (coupled stepping reads the water's velocity)
        _step(oc)
        s = _set(capi, 0)
        lay = _prime(oc, R, cell)
        got = _check_record(capi, oc, R, "primed")
        assert got[4] == 0 and 0 < got[5] <= R * R and got[0] < 0 < got[1] and got[2] < 0 < got[3]
        # pending deposits are not seen: the state alone
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))
        bodies, probes, motions, props = _bodies(R, R, cell)
        oc.step_bodies_coupled_host(cascades, s, bodies, motions, props, probes, float(DT), 2, 4)
        after = _check_record(capi, oc, R, "coupled")
        assert not np.array_equal(after[:4], got[:4])
        for substeps in (1, 16):
            oc.step_ripples(0.05 * cell * substeps, substeps)
            now = _check_record(capi, oc, R, substeps)
            assert not np.array_equal(now[:4], after[:4])
            after = now
        oc.reset_ripples()
        rest = _check_record(capi, oc, R, "rest")
        assert np.all(rest == 0)


def _plant(capi, oc, cell, field, value):
    """one float of the current state buffer in MEMORY order, written behind the module's back"""
    ptr = oc.ripples_device()[0]
    v = np.array([value], F)
    assert capi.load().datum_ocean_device_write(oc.h, capi.P(ptr + 8 * cell + 4 * field), v.ctypes.data_as(capi.P), 4) == capi.OK


def test_record_of_the_largest_layer(capi):
    R = 1024
    with _plain(capi) as oc:
        oc.set_ripples(R, 1.0)
        assert np.all(oc.read_ripple_bounds() == 0)
        _guards_whole(capi, oc, R)
        _plant(capi, oc, R * R - 1, 0, 7.0)                                       # the last cell in memory
        assert oc.read_ripple_bounds().tolist() == [0, 7, 0, 0, 0, 1, 0, 0]
        _plant(capi, oc, 0, 1, -3.0)                                              # the first: a rate alone
        assert oc.read_ripple_bounds().tolist() == [0, 7, -3, 0, 0, 2, 0, 0]
        _plant(capi, oc, 300 * R + 513, 0, np.nan)
        got = oc.read_ripple_bounds()
        assert got.tolist() == [0, 7, -3, 0, 1, 3, 0, 0]
        _plant(capi, oc, 777 * R + 2, 1, -np.inf)
        assert oc.read_ripple_bounds().tolist() == [0, 7, -np.inf, 0, 2, 4, 0, 0]
        assert _same_record(oc.read_ripple_bounds(), ripple_bounds64.fold(oc.read_ripples()))
        _guards_whole(capi, oc, R)
        # another size: the block is the new layer's
        oc.set_ripples(256, 1.0)
        with pytest.raises(capi.OceanError) as e:
            oc.ripple_bounds_device()
        assert e.value.code == capi.ESTATE
        _plant(capi, oc, 256 * 256 - 1, 0, -2.0)
        assert oc.read_ripple_bounds().tolist() == [-2, 0, 0, 0, 0, 1, 0, 0]
        _guards_whole(capi, oc, 256)


# 2 -- the mark


def test_mark(capi, oracle, torch):
    N, C, R, cell = 64, 2, 64, 1.0
    lib = capi.load()
    with _setup(capi, oracle, N, C) as oc:
        oc.set_velocity("on")                                                    # (coupled stepping reads the water's velocity)
        _step(oc)
        s = _set(capi, 0)
        arr = (capi.I * 2)(0, 1)
        call = lambda fn, *a: fn(oc.h, arr, 2, ctypes.byref(s), *a)
        bounded = lambda: call(lib.datum_ocean_cast_rays_rippled_bounded, 4, 32, 8, None, 0, None)
        out = np.zeros(8, F)

        # the layer is off: ESTATE from every call, whatever else is said
        p, n = capi.P(), ctypes.c_size_t()
        assert lib.datum_ocean_reduce_ripple_bounds(oc.h) == capi.ESTATE
        assert lib.datum_ocean_ripple_bounds_device(oc.h, ctypes.byref(p), ctypes.byref(n)) == capi.ESTATE
        assert lib.datum_ocean_read_ripple_bounds(oc.h, None) == capi.ESTATE
        assert lib.datum_ocean_surface_slab_rippled(oc.h, arr, 99, None, None, None, None, None) == capi.ESTATE
        assert call(lib.datum_ocean_cast_rays_rippled_bounded, 4, 0, 99, None, 0, None) == capi.ESTATE
        assert call(lib.datum_ocean_read_rays_rippled_bounded, 4, 0, 99, None, 0, None) == capi.ESTATE
        assert b"datum_ocean_read_rays_rippled_bounded" in lib.datum_ocean_last_error(oc.h)

        lay = _prime(oc, R, cell)
        assert lib.datum_ocean_ripple_bounds_device(oc.h, ctypes.byref(p), ctypes.byref(n)) == capi.ESTATE
        # neither mark, then one of the two, either way round
        assert bounded() == capi.ESTATE
        oc.reduce_bounds()
        assert bounded() == capi.ESTATE and b"ripple bounds are not current" in lib.datum_ocean_last_error(oc.h)
        oc.reduce_ripple_bounds()
        assert bounded() == capi.OK
        oc.displace()
        assert bounded() == capi.ESTATE and b"the bounds are not current" in lib.datum_ocean_last_error(oc.h)
        oc.reduce_bounds()
        assert bounded() == capi.OK
        # an argument error comes first, as in cast_rays_rippled
        assert call(lib.datum_ocean_cast_rays_rippled_bounded, 4, 0, 8, None, 0, None) == capi.EINVAL
        assert lib.datum_ocean_read_ripple_bounds(oc.h, None) == capi.EINVAL
        assert lib.datum_ocean_ripple_bounds_device(oc.h, None, None) == capi.EINVAL
        assert lib.datum_ocean_surface_slab_rippled(oc.h, arr, 2, None, None, None, None, None) == capi.EINVAL
        assert lib.datum_ocean_surface_slab_rippled(oc.h, arr, 17, ctypes.byref(s), None, None, None, None) == capi.EINVAL

        # what leaves the mark: deposits (there are pending ones already), the parameters, every read
        imp = _impulses(np.random.RandomState(1), lay, 50, 0.05)
        oc.deposit_ripples_host(imp)
        oc.set_ripple_params(2.0, 0.05, 8, 4.0)
        oc.read_ripples()
        oc.query_ripples(np.zeros((4, 2), F))
        oc.read_surface_blend_rippled([0, 1], s, np.zeros((4, 2), F), 4)
        oc.ripple_bounds_device()
        assert bounded() == capi.OK

        # what clears it
        bodies, probes, motions, props = _bodies(3, R, cell)
        x, y = (ORIGIN[0] + R // 2 + 3.5) * cell, (ORIGIN[1] + R // 2 + 0.5) * cell
        dev = [torch.from_numpy(np.ascontiguousarray(a).view(F).ravel().copy()).cuda() for a in (bodies, motions, props, probes)]
        drec = torch.zeros(len(bodies) * 12, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        clearing = (("step_ripples", lambda: oc.step_ripples(0.1, 2)),
                    ("step_bodies_coupled", lambda: oc.step_bodies_coupled([0, 1], s, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(bodies),
                                                                           dev[3].data_ptr(), len(probes), float(DT), 1, drec.data_ptr(), 4)),
                    ("step_bodies_coupled_host", lambda: oc.step_bodies_coupled_host([0, 1], s, bodies, motions, props, probes, float(DT), 1, 4)),
                    ("center_ripples", lambda: oc.center_ripples(x, y)),
                    ("reset_ripples", oc.reset_ripples),
                    ("set_ripples", lambda: oc.set_ripples(R, cell)))
        for name, fn in clearing:
            assert bounded() == capi.OK, name
            fn()
            assert bounded() == capi.ESTATE, name
            with pytest.raises(capi.OceanError) as e:
                oc.read_rays_rippled_bounded([0, 1], s, _rays(1, 8), 4, 32, 8)
            assert e.value.code == capi.ESTATE, name
            # either way of making it current again
            if name in ("center_ripples", "set_ripples"):
                oc.surface_slab_rippled([0], s)
            else:
                oc.read_ripple_bounds()
        assert bounded() == capi.OK
        # a refused clearing call changes nothing
        with pytest.raises(capi.OceanError):
            oc.step_ripples(-1.0, 1)
        with pytest.raises(capi.OceanError):
            oc.center_ripples(np.nan, 0.0)
        assert bounded() == capi.OK


# 3 -- the bounded rippled cast is the rippled cast


def _ray_set(seed, R, cell, zlo, zhi, n=4096):
    """4096 rays: test_gpu_rays' segments around the level over and beside the window; a camera fan from 40-120 m above the window; segments
    wholly inside the slab; nearly level segments inside the slab's upper part that cross the window's edge; test_gpu_rays' degenerate rays"""
    rng = np.random.RandomState(seed)
    lo = np.array(ORIGIN) * cell
    side = R * cell
    zlo, zhi = float(zlo), float(zhi)

    def segment(m, start, z0, z1, run):
        r = np.zeros((m, 8), F)
        r[:, 0:2] = start
        r[:, 2] = z0
        az, d = rng.uniform(0, 2 * np.pi, m), rng.uniform(*run, m)
        r[:, 4], r[:, 5], r[:, 6] = d * np.cos(az), d * np.sin(az), z1 - z0
        r[:, 3], r[:, 7] = 0.0, 1.0
        return r

    m = n // 4
    eye = lo + 0.5 * side
    fan = segment(m, eye, 0.3 + rng.uniform(40, 120), rng.uniform(-30, -8, m), (5, 400))
    mid = lambda k: rng.uniform(0.9 * zlo + 0.1 * zhi, 0.1 * zlo + 0.9 * zhi, k)
    inside = segment(m // 2, lo + rng.uniform(-0.3, 1.3, (m // 2, 2)) * side, mid(m // 2), mid(m // 2), (0, 60))
    edge = segment(m // 2, lo + np.stack([rng.uniform(-0.4, 0.0, m // 2), rng.uniform(0, 1, m // 2)], 1) * side, 0, 0, (0, 1))
    edge[:, 2] = rng.uniform(0.5 * (zlo + zhi), zhi, m // 2)
    edge[:, 4], edge[:, 5], edge[:, 6] = rng.uniform(0.5, 1.0, m // 2) * side, rng.uniform(-0.2, 0.2, m // 2) * side, rng.uniform(-0.3, 0.1, m // 2)
    general = _rays(seed, n - 2 * m, spread=45.0)
    general[:, 0:2] += lo + 0.25 * side
    # the degenerate rays: a NaN component, tmax < tmin, an overflowing direction, an infinite origin, an overflowing parameter range, tmin == tmax
    general[:6] = general[6:12]
    general[0, 4] = np.nan
    general[1, 7] = general[1, 3] - 1.0
    general[2, 4:7] = 3e38
    general[3, 0] = np.inf
    general[4, 3], general[4, 7], general[4, 4:7] = -3e38, 3e38, (2.0, 2.0, -2.0)
    general[5, 7] = general[5, 3]
    rays = np.concatenate([general, fan, inside, edge]).astype(F)
    assert len(rays) == n
    return rays


@pytest.mark.parametrize("N,C,lists,R,cell", [(64, 3, ([1], [0, 1, 2]), 64, 1.0), (2048, 2, ([1], [0, 1]), 128, 0.5)])
def test_cast_bits(capi, oracle, N, C, lists, R, cell):
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        lay = _prime(oc, R, cell)
        oc.reduce_bounds()
        oc.reduce_ripple_bounds()
        for cascades in lists:
            for swell in (True, False):
                s = _set(capi, 0, swell)
                zlo, zhi, _, _ = oc.surface_slab_rippled(cascades, s)
                rays = _ray_set(N + R, R, cell, zlo, zhi)
                start, end = rays[:, 2] + rays[:, 3] * rays[:, 6], rays[:, 2] + rays[:, 7] * rays[:, 6]
                with np.errstate(invalid="ignore"):
                    assert (start > zhi).sum() > 1000 and ((start > zlo) & (start < zhi) & (end > zlo) & (end < zhi)).sum() > 500
                for S, Rf in ((7, 12), (32, 8)):
                    want = oc.read_rays_rippled(cascades, s, rays, 4, S, Rf)
                    got = oc.read_rays_rippled_bounded(cascades, s, rays, 4, S, Rf)
                    assert _same(got, want), (N, cascades, swell, S, Rf, np.argwhere(_bits(got) != _bits(want))[:4])
                    assert np.isnan(got[:5]).all() and np.isfinite(got[5:]).all()
                    assert all((got[:, 3] == v).sum() > 100 for v in (0, 1, 2)), (N, cascades, swell, S, Rf)
                # the layer is in the records: the parents' bounded cast (the same steps and bisections) gives others
                plain = oc.read_rays_bounded(cascades, s, rays, 4, 32, 8)
                assert (plain[6:, 0] != got[6:, 0]).mean() > 0.02
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))

        # a non-finite cell in the layer: a NaN slab, which decides nothing -- and still the rippled cast's bits
        s = _set(capi, 0)
        cascades = lists[-1]
        # (one row of cells in memory, right across the window: rays meet it)
        ptr = oc.ripples_device()[0]
        v = np.full(2 * R, np.nan, F)
        assert capi.load().datum_ocean_device_write(oc.h, capi.P(ptr + 8 * R * (R // 2)), v.ctypes.data_as(capi.P), 8 * R) == capi.OK
        rec = oc.read_ripple_bounds()
        assert rec[4] == R and rec[5] >= R
        slab = oc.surface_slab_rippled(cascades, s)
        assert np.isnan(slab[0]) and np.isnan(slab[1]) and np.isfinite(slab[2]) and np.isfinite(slab[3])
        want = oc.read_rays_rippled(cascades, s, rays, 4, 32, 8)
        assert _same(oc.read_rays_rippled_bounded(cascades, s, rays, 4, 32, 8), want)
        assert np.isnan(want[6:, 6]).any()


# 4 -- the slab


@pytest.mark.parametrize("N,C,lists", [(64, 3, ([1], [0, 1, 2], [2, 2, 0]))])
def test_slab(capi, oracle, N, C, lists):
    with _setup(capi, oracle, N, C) as oc:
        _step(oc)
        for R, cell in ((64, 1.0), (128, 0.5)):
            _prime(oc, R, cell)
            records, layer = oc.read_bounds(), oc.read_ripple_bounds()
            for cascades in lists:
                for swell in (True, False):
                    s = _set(capi, 0, swell)
                    got = np.array(oc.surface_slab_rippled(cascades, s), F)
                    want = ripple_bounds64.slab32(records, cascades, *bounds64.frame32(s), layer)
                    assert _same(got, np.array(want[:4], F)), (R, cascades, swell, got, want)
                    parent = np.array(oc.surface_slab(cascades, s), F)
                    assert got[0] < parent[0] and parent[1] < got[1] and _same(got[2:], parent[2:])
                    # every height of the rippled query lies inside
                    rng = np.random.RandomState(R)
                    q = (np.array(ORIGIN) * cell + rng.uniform(-0.2, 1.2, (4000, 2)) * R * cell).astype(F)
                    z = oc.read_surface_blend_rippled(cascades, s, q, 4)[:, 2]
                    assert np.all(z > got[0]) and np.all(z < got[1])
            # over a layer at rest: the parent's slab
            oc.reset_ripples()
            for cascades in lists:
                s = _set(capi, 0)
                assert np.array_equal(np.array(oc.surface_slab_rippled(cascades, s), F), np.array(oc.surface_slab(cascades, s), F))


# 5 -- isolation, the device arrays and the host twin


def test_isolation_and_device_arrays(capi, oracle, torch):
    N, cascades, R, cell = 64, [1, 0, 2], 64, 1.0
    with _setup(capi, oracle, N, 3, foam="accumulate") as oc:
        _step(oc)
        lay = _prime(oc, R, cell)
        s = _set(capi, 0)
        rays = _ray_set(7, R, cell, -2.0, 3.0, 1024)
        n = len(rays)
        oc.reduce_bounds()
        before = {"ripples": oc.read_ripples().copy(), "maps": [oc.read_maps(c).copy() for c in range(3)], "foam": [oc.read_foam(c).copy() for c in range(3)],
                  "bounds": oc.read_bounds().copy(), "rays": oc.read_rays(cascades, s, rays, 4, 32, 8), "bounded": oc.read_rays_bounded(cascades, s, rays, 4, 32, 8),
                  "rippled": oc.read_rays_rippled(cascades, s, rays, 4, 32, 8), "slab": np.array(oc.surface_slab(cascades, s), F)}

        oc.reduce_ripple_bounds()
        oc.read_ripple_bounds()
        oc.surface_slab_rippled(cascades, s)
        host = oc.read_rays_rippled_bounded(cascades, s, rays, 4, 32, 8)
        dr = torch.from_numpy(rays).cuda()
        out = torch.full((n * 12 + 128,), -3.0e38, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        # n = 0 enqueues nothing
        oc.cast_rays_rippled_bounded(cascades, s, dr.data_ptr(), 0, out.data_ptr() + 256, 4, 32, 8)
        oc.sync()
        assert bool((out == -3.0e38).all())
        oc.cast_rays_rippled_bounded(cascades, s, dr.data_ptr(), n, out.data_ptr() + 256, 4, 32, 8)
        oc.sync()
        raw = out.cpu().numpy()
        assert np.all(raw[:64] == F(-3.0e38)) and np.all(raw[64 + n * 12:] == F(-3.0e38))      # canaries before and behind the records
        assert _same(raw[64:64 + n * 12].reshape(n, 12), host) and _same(host, before["rippled"])
        assert oc.read_rays_rippled_bounded(cascades, s, rays[:0], 4, 32, 8).shape == (0, 12)
        assert _same(oc.read_rays_rippled_bounded(cascades, s, rays[:257], 4, 32, 8), host[:257])
        # the parents' refusals under the new names
        for bad in (lambda: oc.read_rays_rippled_bounded([3], s, rays, 4, 32, 8), lambda: oc.read_rays_rippled_bounded(cascades, s, rays, 4, 0, 8),
                    lambda: oc.read_rays_rippled_bounded(cascades, s, rays, 65, 32, 8), lambda: oc.cast_rays_rippled_bounded(cascades, s, dr.data_ptr() + 8, n, out.data_ptr(), 4, 32, 8)):
            with pytest.raises(capi.OceanError) as e:
                bad()
            assert e.value.code == capi.EINVAL and "rippled_bounded" in str(e.value)

        assert _same(oc.read_ripples(), before["ripples"])
        for c in range(3):
            assert _same(oc.read_maps(c), before["maps"][c]) and _same(oc.read_foam(c), before["foam"][c])
        assert _same(oc.read_rays(cascades, s, rays, 4, 32, 8), before["rays"]) and _same(oc.read_rays_rippled(cascades, s, rays, 4, 32, 8), before["rippled"])
        assert _same(np.array(oc.surface_slab(cascades, s), F), before["slab"]) and _same(oc.read_bounds(), before["bounds"])
        assert _same(oc.read_rays_bounded(cascades, s, rays, 4, 32, 8), before["bounded"])
        # the pending deposits too: a step shows them
        oc.step_ripples(0.1 * cell, 2)
        lay.step(0.1 * cell, 2)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))


# 6 -- the C++ shim


def test_cpp_shim_matches_capi(capi):
    from datum_amd import host_api

    N, R, cell = 64, 64, 1.0
    params = host_api.OceanParams(N, **host_api.EXAMPLE_TUNABLES)
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    rng = np.random.RandomState(5)
    lib = capi.load()
    P = capi.P
    with host_api.OceanContext(N, device=0) as ctx:
        mesh = ctx.create_ocean(33, 17)
        ctx.render_ocean_surface(mesh, params, camera)
        rays = _ray_set(3, R, cell, -1.0, 1.5, 512)
        for call in (ctx.reduce_ocean_ripple_bounds, lambda: ctx.ocean_surface_slab_rippled(params), lambda: ctx.cast_ocean_rays_rippled_bounded(params, rays)):
            with pytest.raises(host_api.HostError, match="the ripple layer is off"):
                call()
        ctx.set_ocean_ripples(R, cell)
        ctx.center_ocean_ripples((ORIGIN[0] + R // 2 + 0.5) * cell, (ORIGIN[1] + R // 2 + 0.5) * cell)
        imp = np.zeros((300, 4), F)
        imp[:, :2] = np.array(ORIGIN) * cell + rng.uniform(0.05, 0.95, (300, 2)) * R * cell
        imp[:, 2] = rng.normal(size=300) * 0.05
        ctx.deposit_ocean_ripples(imp)
        ctx.step_ocean_ripples(0.1 * cell, 3)
        ctx.reduce_ocean_bounds()
        with pytest.raises(host_api.HostError, match="ripple bounds are not current"):
            ctx.cast_ocean_rays_rippled_bounded(params, rays, 4, 32, 8)
        b = ctx.reduce_ocean_ripple_bounds()
        h = ctx.lib.datum_host_context_handle(ctx.c)
        rec = np.zeros(8, F)
        assert lib.datum_ocean_read_ripple_bounds(h, rec.ctypes.data_as(P)) == capi.OK
        assert _same(np.array([b.etamin, b.etamax, b.ratemin, b.ratemax], F), rec[:4]) and (b.nonfinite, b.active) == (int(rec[4]), int(rec[5]))
        assert b.nonfinite == 0 and b.active > 0 and b.etamin < 0 < b.etamax
        one = (capi.I * 1)(0)
        s = params.oceanset(camera)
        got = ctx.cast_ocean_rays_rippled_bounded(params, rays, 4, 32, 8)
        want = np.empty_like(got)
        assert lib.datum_ocean_read_rays_rippled_bounded(h, one, 1, ctypes.byref(s), 4, 32, 8, rays.ctypes.data_as(P), len(rays), want.ctypes.data_as(P)) == capi.OK
        assert _same(got, want) and _same(got, ctx.cast_ocean_rays_rippled(params, rays, 4, 32, 8))
        slab = np.array(ctx.ocean_surface_slab_rippled(params), F)
        out = np.zeros(4, F)
        assert lib.datum_ocean_surface_slab_rippled(h, one, 1, ctypes.byref(s), *[P(out.ctypes.data + 4 * k) for k in range(4)]) == capi.OK
        assert _same(slab, out) and np.isfinite(slab).all() and slab[0] < slab[1]
        parent = np.array(ctx.ocean_surface_slab(params), F)
        assert slab[0] < parent[0] and parent[1] < slab[1]
