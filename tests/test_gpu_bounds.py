"""Surface bounds per cascade and the bounded ray casts (include/datum_ocean_hip.h: datum_ocean_reduce_bounds) on the MI355X.

  1  records: the six extrema equal numpy's over datum_ocean_read_maps by value, nonfinite = 0, at 64^2 x 3, 128^2, 512^2 and 2048^2 x 2
     (fewer patches than lanes of the launch, each patch width, the banded layout); the slab is bounds64.slab32's bit for bit;
  2  single texels planted through a bound map buffer (datum_ocean_device_write at the layout's offsets): the first and the last texel,
     the last of the first patch and, at 2048^2, the first of the last band, each as a new maximum and a new minimum of dx, dy and dz;
     a NaN and an infinity: counted, the NaN in no extremum, the slab a NaN;
  3  the flat ocean; 4  currency: ESTATE before a reduce, after a displace and after bind_maps;
  5  bits: read_rays_bounded against read_rays, all twelve floats of every ray, no ray excluded; also under a NaN slab;
  6  the C++ shim's three calls against the C ABI's.
"""

import ctypes

import numpy as np
import pytest

import bounds64
from test_gpu_body import _step
from test_gpu_rays import _flat, _rays
from test_gpu_surface import DT, _set, _setup

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


def _same(a, b):
    """equal as bits, NaNs as NaNs"""
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _slab_matches(capi, oc, cascades, s, records):
    got = np.array(oc.surface_slab(cascades, s), F)
    zlo, zhi, rx, ry, _ = bounds64.slab32(records, cascades, *bounds64.frame32(s))
    want = np.array([zlo, zhi, rx, ry], F)
    return _same(got, want), got, want


# 1 -- records


@pytest.mark.parametrize("N,C", [(64, 3), (128, 1), (512, 1), (2048, 2)])
def test_records(capi, oracle, N, C):
    with _setup(capi, oracle, N, C) as oc:
        _step(oc)
        got = oc.read_bounds()
        assert got.shape == (C, 8)
        want = np.stack([bounds64.fold_maps(oc.read_maps(c)) for c in range(C)])
        assert np.array_equal(got[:, :6], want[:, :6]), (N, got, want)
        assert np.all(got[:, 6] == 0) and np.all(got[:, 7] == 0)
        assert np.all(got[:, 0:6:2] < 0) and np.all(got[:, 1:6:2] > 0)
        # a second reduce gives the same records, and the device buffer holds them
        assert np.array_equal(_bits(got), _bits(oc.read_bounds()))
        ptr, nbytes = oc.bounds_device()
        assert nbytes == C * 32
        raw = np.zeros((C, 8), F)
        assert capi.load().datum_ocean_device_read(oc.h, raw.ctypes.data_as(capi.P), capi.P(ptr), nbytes) == capi.OK
        assert np.array_equal(_bits(raw), _bits(got))
        for cascades in ([0], list(range(C)), [C - 1, 0, C - 1]):
            for swell in (True, False):
                ok, a, b = _slab_matches(capi, oc, cascades, _set(capi, 0, swell), got)
                assert ok and np.isfinite(a).all() and a[0] < a[1], (N, cascades, swell, a, b)


# 2 -- planted texels through a bound buffer


def _offset(capi, N, cascade, x, y):
    """byte offset of texel (x, y)'s part A in the handle's map buffer (include/datum_ocean_hip.h: datum_ocean_bind_maps)"""
    PW, PH, B, TB = capi.map_layout(N)
    patch = (x // B) * TB * N * B + ((y // PH) * (B // PW) + (x % B) // PW) * 16 * TB
    return cascade * N * N * TB + patch + ((y % PH) * PW + x % PW) * 16


def _bound(capi, oracle, torch, N, C):
    oc = _setup(capi, oracle, N, C)
    nbytes = oc.maps_device()[1]
    buf = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    oc.bind_maps(buf.data_ptr(), nbytes)
    return oc, buf


def _write(capi, oc, buf, offset, value):
    v = np.array([value], F)
    assert capi.load().datum_ocean_device_write(oc.h, capi.P(buf.data_ptr() + offset), v.ctypes.data_as(capi.P), 4) == capi.OK


@pytest.mark.parametrize("N,C", [(64, 3), (2048, 2)])
def test_planted_texels(capi, oracle, torch, N, C):
    PW, PH, B, _ = capi.map_layout(N)
    cascade = C - 1
    oc, buf = _bound(capi, oracle, torch, N, C)
    with oc:
        _step(oc)
        base = oc.read_bounds()
        host = buf.cpu().numpy()
        positions = [(0, 0), (N - 1, N - 1), (PW - 1, PH - 1)] + ([(N - B, 0)] if B != N else [])
        assert _offset(capi, N, 0, N - 1, N - 1) == N * N * 24 - 384 + 240 and _offset(capi, N, 0, PW - 1, PH - 1) == 240
        for x, y in positions:
            for ch, k in ((0, 2), (1, 4), (2, 0)):                                   # dx, dy, dz -> the record's fields
                off = _offset(capi, N, cascade, x, y) + 4 * ch
                for sign in (1, -1):
                    value = F(base[cascade, k + 1] + 1) if sign > 0 else F(base[cascade, k] - 1)
                    _write(capi, oc, buf, off, value)
                    got = oc.read_bounds()
                    want = base.copy()
                    want[cascade, k + (1 if sign > 0 else 0)] = value
                    # (where the overwritten texel was itself the old extremum of the other end, that end moves inwards, never out;
                    # everywhere else the whole record is as before but for the planted field)
                    other = k + (0 if sign > 0 else 1)
                    assert got[cascade, k + (1 if sign > 0 else 0)] == value, (N, x, y, ch, sign)
                    if host[off // 4] == base[cascade, other]:
                        assert (got[cascade, other] >= base[cascade, other]) if sign > 0 else (got[cascade, other] <= base[cascade, other])
                        want[cascade, other] = got[cascade, other]
                    assert np.array_equal(got, want), (N, x, y, ch, sign, got, want)
                    assert np.array_equal(got[:cascade], base[:cascade])
                    _write(capi, oc, buf, off, host[off // 4])
        assert np.array_equal(_bits(oc.read_bounds()), _bits(base))

        # a NaN and an infinity in one cascade
        nan_at, inf_at = _offset(capi, N, cascade, 5, 3) + 8, _offset(capi, N, cascade, N - 2, N - 7) + 0
        _write(capi, oc, buf, nan_at, np.nan)
        _write(capi, oc, buf, inf_at, np.inf)
        got = oc.read_bounds()
        assert got[cascade, 6] == 2 and np.all(got[:cascade, 6] == 0)
        assert got[cascade, 3] == np.inf and np.isfinite(got[cascade, [0, 1, 2, 4, 5]]).all()
        want = bounds64.fold_maps(oc.read_maps(cascade))
        assert np.array_equal(got[cascade, :7], want[:7])
        s = _set(capi, 0)
        zlo, zhi, rx, ry = oc.surface_slab([0, cascade], s)
        assert np.isnan(zlo) and np.isnan(zhi) and rx == np.inf and np.isfinite(ry)
        zlo, zhi, rx, ry = oc.surface_slab([0], s)
        assert np.isfinite([zlo, zhi, rx, ry]).all()

        # 5b -- under the NaN slab the bounded cast is still the cast
        _write(capi, oc, buf, inf_at, host[inf_at // 4])
        rays = _ray_set(N + 2, 600)
        oc.reduce_bounds()
        a, b = oc.read_rays([0, cascade], s, rays, 4, 32, 8), oc.read_rays_bounded([0, cascade], s, rays, 4, 32, 8)
        assert _same(a, b), (N, np.argwhere(_bits(a) != _bits(b))[:4])
        assert np.isnan(oc.surface_slab([0, cascade], s)[0])


# 3 -- the flat ocean


def test_flat_ocean(capi):
    with _flat(capi) as oc:
        rec = oc.read_bounds()
        assert rec.shape == (1, 8) and np.all(rec == 0)
        # mag = 0: no pad, the slab is the level itself
        s = _set(capi, 0, swell=False, plane_w=0.0)
        assert np.all(np.array(oc.surface_slab([0], s)) == 0)
        # otherwise zlo = (basez - |A|) - pad with pad = (|basez| + |A|) 2^-16, each rounded once
        s = _set(capi, 0, swell=True, plane_w=-0.25)
        s.swellamplitude = -0.5                                                       # |A|
        zlo, zhi, rx, ry = oc.surface_slab([0], s)
        pad = F(F(0.75) * F(2.0 ** -16))
        assert zlo == F(F(0.25) - F(0.5)) - pad and zhi == F(0.75) + pad
        ok, a, b = _slab_matches(capi, oc, [0], s, rec)
        assert ok, (a, b)
        # s.swellsteepness = 0: a height field between the bounds, strictly
        s.swellsteepness = 0.0
        z = oc.read_surface_blend([0], s, np.random.RandomState(1).uniform(-100, 100, (4000, 2)).astype(F), 4)[:, 2]
        assert np.all(z > zlo) and np.all(z < zhi) and z.max() - z.min() > 0.99


# 4 -- currency


def test_currency(capi, oracle, torch):
    N, C = 64, 2
    lib = capi.load()
    rays = _rays(3, 64)
    with _setup(capi, oracle, N, C) as oc:
        s = _set(capi, 0)
        arr = (capi.I * 2)(0, 1)

        def bounded():
            return lib.datum_ocean_cast_rays_bounded(oc.h, arr, 2, ctypes.byref(s), 4, 32, 8, None, 0, None)

        p, n = capi.P(), ctypes.c_size_t()
        assert lib.datum_ocean_bounds_device(oc.h, ctypes.byref(p), ctypes.byref(n)) == capi.ESTATE
        _step(oc)
        assert bounded() == capi.ESTATE and b"datum_ocean_cast_rays_bounded" in lib.datum_ocean_last_error(oc.h)
        with pytest.raises(capi.OceanError):
            oc.read_rays_bounded([0, 1], s, rays, 4, 32, 8)
        # an argument error comes first, as in cast_rays
        assert lib.datum_ocean_cast_rays_bounded(oc.h, arr, 2, ctypes.byref(s), 4, 0, 8, None, 0, None) == capi.EINVAL
        oc.reduce_bounds()
        assert bounded() == capi.OK
        assert lib.datum_ocean_bounds_device(oc.h, ctypes.byref(p), ctypes.byref(n)) == capi.OK and n.value == C * 32
        want = oc.read_rays([0, 1], s, rays, 4, 32, 8)
        assert _same(oc.read_rays_bounded([0, 1], s, rays, 4, 32, 8), want)
        # queries, casts, an update and bind_foam leave the records current
        oc.update(DT)
        foambuf = torch.zeros(C * N * N, dtype=torch.float32, device="cuda")
        oc.bind_foam(foambuf.data_ptr(), C * N * N * 4)
        assert bounded() == capi.OK
        oc.bind_foam(0, 0)
        oc.displace()
        assert bounded() == capi.ESTATE
        oc.read_bounds()
        assert bounded() == capi.OK
        nbytes = oc.maps_device()[1]
        buf = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        oc.bind_maps(buf.data_ptr(), nbytes)
        assert bounded() == capi.ESTATE
        oc.surface_slab([0], s)
        assert bounded() == capi.OK
        oc.bind_maps(0, 0)
        assert bounded() == capi.ESTATE
        # an argument error of the bounded calls with a live handle
        assert lib.datum_ocean_surface_slab(oc.h, arr, 17, ctypes.byref(s), None, None, None, None) == capi.EINVAL
        assert lib.datum_ocean_surface_slab(oc.h, (capi.I * 2)(0, 2), 2, ctypes.byref(s), None, None, None, None) == capi.EINVAL
        assert lib.datum_ocean_surface_slab(oc.h, arr, 2, None, None, None, None, None) == capi.EINVAL
        assert lib.datum_ocean_read_bounds(oc.h, None) == capi.EINVAL
        assert lib.datum_ocean_surface_slab(oc.h, arr, 2, ctypes.byref(s), None, None, None, None) == capi.OK


def test_release_memory_that_unbinds_the_maps_ends_currency(capi, oracle):
    # maps bound at an offset inside an imported block, reduced, then the block released by its base pointer: the handle's own maps are in
    # use again, other texels than the records', and a bounded cast must be refused until the next reduce
    import os

    class ExtMem(ctypes.Structure):
        _fields_ = [("handle", ctypes.c_void_p), ("va", ctypes.c_void_p), ("bytes", ctypes.c_size_t)]

    helper = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu", "libextmem_helper.so"))
    helper.extmem_create.argtypes = [ctypes.c_size_t, ctypes.POINTER(ExtMem), ctypes.POINTER(ctypes.c_int)]
    helper.extmem_destroy.argtypes = [ctypes.POINTER(ExtMem)]
    N, C, offset = 64, 2, 4096
    lib = capi.load()
    rays = _rays(4, 300)
    nbytes = C * N * N * 24
    mem, fd = ExtMem(), ctypes.c_int(-1)
    assert helper.extmem_create(nbytes + offset, ctypes.byref(mem), ctypes.byref(fd)) == 0
    try:
        with _setup(capi, oracle, N, C) as oc:
            assert oc.maps_device()[1] == nbytes
            s = _set(capi, 0)
            arr = (capi.I * 2)(0, 1)

            def bounded():
                return lib.datum_ocean_cast_rays_bounded(oc.h, arr, 2, ctypes.byref(s), 4, 32, 8, None, 0, None)

            ptr = oc.import_memory_fd(fd.value, mem.bytes)
            oc.bind_maps(ptr + offset, nbytes)
            _step(oc)
            inside = oc.read_bounds()
            assert bounded() == capi.OK
            oc.release_memory(ptr)                                               # the maps were bound at ptr + offset
            assert oc.maps_device()[0] != ptr + offset
            assert bounded() == capi.ESTATE
            with pytest.raises(capi.OceanError):
                oc.read_rays_bounded([0, 1], s, rays, 4, 32, 8)
            # the own maps hold other texels (nothing was displaced into them): the old records were not theirs
            own = oc.read_bounds()
            assert not np.array_equal(own[:, :6], inside[:, :6])
            assert bounded() == capi.OK
            # displaced into, reduced: the bounded cast is the cast again
            _step(oc)
            assert bounded() == capi.ESTATE
            oc.reduce_bounds()
            assert _same(oc.read_rays_bounded([0, 1], s, rays, 4, 32, 8), oc.read_rays([0, 1], s, rays, 4, 32, 8))
    finally:
        assert helper.extmem_destroy(ctypes.byref(mem)) == 0


# 5 -- bits


def _ray_set(seed, n=2000, level=0.3, slab=None):
    """test_gpu_rays' segments around the level, then: a camera fan from 40-120 m above, segments wholly above the slab, wholly below it
    and wholly inside it, segments that leave the water upwards from far below to far above, bad rays and rays with an overflowing sample"""
    rng = np.random.RandomState(seed)
    general = _rays(seed, n)

    def segment(m, z0, z1, run=(0, 60)):
        r = np.zeros((m, 8), F)
        r[:, 0:2] = rng.uniform(-150, 150, (m, 2))
        r[:, 2] = level + z0
        az, d = rng.uniform(0, 2 * np.pi, m), rng.uniform(*run, m)
        r[:, 4], r[:, 5], r[:, 6] = d * np.cos(az), d * np.sin(az), z1 - z0
        r[:, 3], r[:, 7] = 0.0, 1.0
        return r

    m = n // 8
    eye = np.array([10.0, -20.0, level + rng.uniform(40, 120)])
    fan = segment(2 * m, eye[2] - level, rng.uniform(-30, -8, 2 * m), run=(5, 400))
    fan[:, 0:2] = eye[:2]
    above = segment(m, rng.uniform(6, 50, m), rng.uniform(6, 50, m))
    below = segment(m, rng.uniform(-50, -6, m), rng.uniform(-50, -6, m))
    # (inside a slab known to the caller: its middle four fifths; otherwise 0.3 m around the level)
    lo, hi = (-0.3, 0.3) if slab is None else (0.9 * slab[0] + 0.1 * slab[1] - level, 0.1 * slab[0] + 0.9 * slab[1] - level)
    inside = segment(m, rng.uniform(lo, hi, m), rng.uniform(lo, hi, m))
    leaving = segment(m, rng.uniform(-40, -6, m), rng.uniform(6, 40, m))
    bad = _rays(seed + 1, 16)
    for k in range(8):
        bad[2 * k, k] = np.nan
        bad[2 * k + 1, k] = -np.inf
    bad = np.concatenate([bad, np.array([[0, 0, 1, 2.0, 1, 0, -1, 1.0], [0, 0, 1, 0, 10.0, 0, -1, 3.0e38]], F)])
    overflow = np.array([[0, 0, 1, -3.0e38, 0, 0, -1e-38, 3.0e38], [0, 0, -1, -3.0e38, 0, 0, -1e-38, 3.0e38],
                         [0, 0, 50, -3.0e38, 1e-38, 0, -1e-37, 3.0e38], [0, 0, -50, -3.0e38, 0, 1e-38, 1e-37, 3.0e38]], F)
    return np.concatenate([general, fan, above, below, inside, leaving, bad, overflow]).astype(F)


@pytest.mark.parametrize("N,C,lists,cases", [(64, 3, ([1], [0, 1, 2]), ((1, 0), (32, 8), (1024, 24))), (2048, 2, ([0, 1],), ((32, 8),))])
def test_bits(capi, oracle, N, C, lists, cases):
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        oc.reduce_bounds()
        for cascades in lists:
            for swell in (True, False):
                s = _set(capi, 0, swell)
                zlo, zhi, _, _ = oc.surface_slab(cascades, s)
                rays = _ray_set(N, slab=(float(zlo), float(zhi)))
                start, end = rays[:, 2] + rays[:, 3] * rays[:, 6], rays[:, 2] + rays[:, 7] * rays[:, 6]
                with np.errstate(invalid="ignore"):
                    assert (start > zhi).sum() > 500 and (start < zlo).sum() > 400 and ((start > zlo) & (start < zhi) & (end > zlo) & (end < zhi)).sum() > 200
                for S, R in cases:
                    want = oc.read_rays(cascades, s, rays, 4, S, R)
                    got = oc.read_rays_bounded(cascades, s, rays, 4, S, R)
                    assert _same(got, want), (N, cascades, swell, S, R, np.argwhere(_bits(got) != _bits(want))[:4])
                    assert np.isnan(got).all(1).sum() == 18
                    status = got[:, 3]
                    assert all((status == v).sum() > 100 for v in (0, 1, 2)), (N, cascades, swell, S, R)
        # no iteration, as well
        s = _set(capi, 0)
        assert _same(oc.read_rays_bounded(lists[-1], s, rays, 0, 32, 8), oc.read_rays(lists[-1], s, rays, 0, 32, 8))


def test_device_arrays_and_edges(capi, oracle, torch):
    N, cascades = 64, [1, 0]
    rays = _ray_set(7, 512)
    n = len(rays)
    with _setup(capi, oracle, N, 2) as oc:
        _step(oc)
        oc.reduce_bounds()
        s = _set(capi, 0)
        want = oc.read_rays(cascades, s, rays, 4, 32, 8)
        dr = torch.from_numpy(rays).cuda()
        out = torch.full((n * 12 + 64,), -3.0e38, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        oc.cast_rays_bounded(cascades, s, dr.data_ptr(), n, out.data_ptr(), 4, 32, 8)
        oc.sync()
        raw = out.cpu().numpy()
        assert _same(raw[: n * 12].reshape(n, 12), want)
        assert np.all(raw[n * 12:] == F(-3.0e38))                                 # a canary behind the records left alone
        assert oc.read_rays_bounded(cascades, s, rays[:0], 4, 32, 8).shape == (0, 12)
        assert _same(oc.read_rays_bounded(cascades, s, rays[:1], 4, 32, 8), want[:1])
        assert _same(oc.read_rays_bounded(cascades, s, rays[:257], 4, 32, 8), want[:257])


# 6 -- the C++ shim


def test_cpp_shim_matches_capi(capi):
    from datum_amd import host_api

    N = 256
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.4))
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    rays = _ray_set(13, 500, level=0.0)
    with host_api.OceanContext(N) as ctx:
        mesh = ctx.create_ocean(32, 32)
        for _ in range(2):
            params.update_ocean(DT)
            ctx.render_ocean_surface(mesh, params, camera)
        lib = capi.load()
        h = ctx.lib.datum_host_context_handle(ctx.c)
        one = (capi.I * 1)(0)
        s = params.oceanset(camera)
        P = capi.P
        with pytest.raises(host_api.HostError):
            ctx.cast_ocean_rays_bounded(params, rays, 4, 32, 8)                   # no reduce since the last displace
        ctx.reduce_ocean_bounds()
        got = ctx.cast_ocean_rays_bounded(params, rays, 4, 32, 8)
        want = np.empty_like(got)
        assert lib.datum_ocean_read_rays_bounded(h, one, 1, ctypes.byref(s), 4, 32, 8, rays.ctypes.data_as(P), len(rays), want.ctypes.data_as(P)) == capi.OK
        assert _same(got, want) and _same(got, ctx.cast_ocean_rays(params, rays, 4, 32, 8))
        slab = np.array(ctx.ocean_surface_slab(params), F)
        out = np.zeros(4, F)
        assert lib.datum_ocean_surface_slab(h, one, 1, ctypes.byref(s), *[P(out.ctypes.data + 4 * k) for k in range(4)]) == capi.OK
        assert _same(slab, out) and np.isfinite(slab).all() and slab[0] < slab[1]
        rec = np.zeros((1, 8), F)
        assert lib.datum_ocean_read_bounds(h, rec.ctypes.data_as(P)) == capi.OK
        assert np.array_equal(rec[0, :7], bounds64.fold_maps(ctx.read_displacement())[:7])
