"""Ray casts (include/datum_ocean_hip.h: datum_ocean_cast_rays) on the MI355X.

  1  bits: read_rays against ray64.cast32 driven by read_surface_blend on the same handle, all twelve floats -- no tolerance: the query is
     held to float64 by tests/test_gpu_blend.py, the sequence of evaluations is the definition's;
  2  against ray64.cast64 as a property.  Per ray the fp32 g(t) differs from float64 by at most
       h = K_POS eps S  +  6 eps reach (1 + 2 G)
     -- the height bar of tests/test_gpu_blend.py (K_POS imported; S = (1 + max |q|)(1 + G) over the segment, G = sum_c N scale_c max|D_c|;
     two texels differ by at most 2 max|D|, so 2 G bounds the gradient) and the roundings of t and point(t): inv, the product with Δ's
     difference, i Δ and the sum, then the product and the sum of a component, six in all, each relative to reach = |o| + |t||d| at most;
     they move point.z directly and the height through point.xy by the gradient.  A ray one of whose march samples up to its bracket has
     a float64 |g| within h is excluded (its side there is not decided); the ray set keeps those to at most 5 %, asserted;
  3  known answers on the flat ocean; 4  edges; 5  the C++ shim.
"""

import ctypes

import numpy as np
import pytest

import ray64
import surface64
from test_gpu_blend import K_POS
from test_gpu_body import _scale, _step
from test_gpu_surface import DT, EPS, _set, _setup

pytestmark = pytest.mark.gpu

F = np.float32
NRAYS = 2000
LEVEL = 0.3                  # _set's plane: the mean level


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


def _rays(seed, n=NRAYS, spread=150.0, level=LEVEL):
    """Segments around the mean level, the summed surface within 2.7 m of it: 30 % from 2.7 ... 4 m above to as far below (ENTER), 30 % the
    other way (LEAVE), 12 % that stay above and 12 % that stay below (MISS), 16 % with both ends within 2.5 m of the level (whatever the
    waves make of them).  Slopes from vertical (a few exactly so) to 2 degrees off horizontal, up- and down-going; directions not unit."""
    rng = np.random.RandomState(seed)
    kind = rng.choice(5, n, p=[0.30, 0.30, 0.12, 0.12, 0.16])
    far = lambda: rng.uniform(2.7, 4.0, n)
    z0 = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [far(), -far(), far(), -far()], rng.uniform(-2.5, 2.5, n))
    z1 = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [-far(), far(), far() + rng.uniform(0, 1, n), -far()], rng.uniform(-2.5, 2.5, n))
    z1 = np.where(np.abs(z1 - z0) < 0.05, z0 + 0.05, z1)
    el = np.radians(rng.uniform(2, 90, n))
    el[::97] = np.pi / 2
    az = rng.uniform(0, 2 * np.pi, n)
    run = np.abs(z1 - z0) / np.tan(el)
    run[::97] = 0
    length = rng.uniform(0.3, 3.0, n)                          # |direction|
    tmin = rng.uniform(-1, 1, n)
    span = np.hypot(run, z1 - z0) / length                     # tmax - tmin
    r = np.empty((n, 8), F)
    d = np.stack([run * np.cos(az), run * np.sin(az), z1 - z0], 1) / span[:, None]
    start = np.concatenate([rng.uniform(-spread, spread, (n, 2)), (level + z0)[:, None]], 1)
    r[:, 4:7] = d
    r[:, 0:3] = start - tmin[:, None] * d                      # point(tmin) is the start
    r[:, 3], r[:, 7] = tmin, tmin + span
    assert not ray64.bad32(r).any()
    return r


def _query(oc, cascades, s, it):
    return lambda q: oc.read_surface_blend(cascades, s, np.ascontiguousarray(q, F), it)


def _mix(rec):
    """the batch shows something: every status on at least 10 % of it, and a segment under water throughout"""
    status = rec[:, 3]
    share = [float((status == v).mean()) for v in (ray64.MISS, ray64.ENTER, ray64.LEAVE)]
    return min(share) >= 0.10 and bool(((status == ray64.MISS) & (rec[:, 2] < 0)).any()), share


# 1 -- bits


@pytest.mark.parametrize("N,C,lists", [(64, 3, ([1], [0, 2], [0, 1, 2])), (2048, 2, ([1], [0, 1]))])
def test_bits(capi, oracle, N, C, lists):
    rays = _rays(N)
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        for cascades in lists:
            for swell in (True, False):
                s = _set(capi, 0, swell)
                for it in (0, 4):
                    for S, R in ((8, 0), (32, 8), (1, 24)):
                        got = oc.read_rays(cascades, s, rays, it, S, R)
                        want = ray64.cast32(_query(oc, cascades, s, it), rays, S, R)
                        assert want.calls <= S + R + 2
                        assert np.isfinite(got).all()
                        assert np.array_equal(_bits(got), _bits(want.records)), (N, cascades, swell, it, S, R, np.argwhere(_bits(got) != _bits(want.records))[:4])
                        ok, share = _mix(got)
                        assert ok, (N, cascades, swell, it, S, R, share)


# 2 -- against float64, as a property


@pytest.mark.parametrize("N,C,cascades", [(64, 3, [0, 1, 2]), (2048, 2, [0, 1])])
def test_against_cast64(capi, oracle, report, N, C, cascades):
    S, R, it = 16, 8, 4
    rays = _rays(N + 1, spread=15.0)
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        # (float64 once: blend64 would convert the maps again at each of cast64's S + R + 2 calls)
        maps_list, scales = [oc.read_maps(c).astype(np.float64) for c in cascades], [_scale(c) for c in cascades]
        foams = [oc.read_foam(c).astype(np.float64) for c in cascades]
        s = _set(capi, 0)
        march = oc.read_rays(cascades, s, rays, it, S, 0).astype(np.float64)
        got = oc.read_rays(cascades, s, rays, it, S, R).astype(np.float64)

    r = rays.astype(np.float64)
    tmin, tmax = r[:, 3], r[:, 7]
    delta = (tmax - tmin) / S
    G = sum(N * float(sc) * float(np.abs(m[0, ..., :3]).max()) for m, sc in zip(maps_list, scales))
    tabs = np.maximum(np.abs(tmin), np.abs(tmax))
    reach = (np.abs(r[:, 0:3]) + tabs[:, None] * np.abs(r[:, 4:7])).max(1)
    ends = np.maximum(np.abs(r[:, 0:2] + tmin[:, None] * r[:, 4:6]), np.abs(r[:, 0:2] + tmax[:, None] * r[:, 4:6])).max(1)
    h = K_POS * EPS * (1.0 + ends) * (1.0 + G) + 6 * EPS * reach * (1.0 + 2.0 * G)

    height = ray64.height64(maps_list, foams, "accumulate", scales, s, it)
    want = ray64.cast64(height, rays, S, R, bar=h)
    near = want.gmin <= 1.0
    share = float(near.mean())
    keep = ~near

    def g64(t):
        return (r[:, 2] + t * r[:, 6]) - height(np.stack([r[:, 0] + t * r[:, 4], r[:, 1] + t * r[:, 5]], 1))[:, 2]

    status = got[:, 3]
    hit = status != ray64.MISS
    side = want.side
    # the march interval: hi of the unrefined cast is t_i
    index = np.where(march[:, 3] != ray64.MISS, np.rint((march[:, 0] - tmin) / delta), 0).astype(np.int64)
    width = got[:, 0] - got[:, 1]
    ulp = np.spacing(np.abs(got[:, 0]).astype(F)).astype(np.float64)
    ghi, glo = g64(got[:, 0]), g64(got[:, 1])
    rhi = np.where((ghi < 0) != side, 0.0, np.abs(ghi) / h)
    rlo = np.where((glo < 0) == side, 0.0, np.abs(glo) / h)
    k = keep & hit
    report(f"rays vs cast64 N={N} list={cascades} S={S} R={R}: excluded (a march sample within the height bar) {share:.4%}; of the rest: "
           f"status differs {int((status != want.records[:, 3])[keep].sum())}, march interval differs {int((index != want.index)[keep].sum())}, "
           f"width / (delta 2^-R + 2 ulp) {float((width[k] / (delta[k] * 2.0 ** -R + 2 * ulp[k])).max()):.3f}, "
           f"wrong-side |g64(hi)| / h {float(rhi[k].max()):.3f}, |g64(lo)| / h {float(rlo[k].max()):.3f}")
    assert share <= 0.05, share
    assert _mix(got.astype(F))[0]
    assert np.array_equal(status[keep], want.records[keep, 3])
    assert np.array_equal(march[keep, 3], status[keep])
    assert np.array_equal(index[keep], want.index[keep])
    assert np.all(march[k, 1] <= got[k, 1]) and np.all(got[k, 0] <= march[k, 0])
    miss = keep & ~hit
    assert np.array_equal(got[miss, 0], tmax[miss]) and np.array_equal(got[miss, 1], tmax[miss])
    assert np.all(width[k] <= delta[k] * 2.0 ** -R + 2 * ulp[k])
    assert np.all(rhi[k] <= 1.0)
    assert np.all(rlo[k] <= 1.0)


# 3 -- known answers on the flat ocean


def _flat(capi, N=64):
    oc = capi.Ocean(N, 1)
    oc.set_cascade(0, 22.0, 1.35)
    oc.upload_state(0, np.zeros((N, N, 2), F))
    oc.update(DT)
    oc.displace()
    return oc


def test_known_answers_flat(capi):
    S, R = 32, 8
    z0 = 0.25
    rays = _rays(11, 600, spread=40.0, level=z0)
    rays = rays[np.abs(rays[:, 2] + rays[:, 3] * rays[:, 6] - z0) > 1e-3]          # the start is not in the water line
    with _flat(capi) as oc:
        s = _set(capi, 0, swell=False, plane_w=-z0)
        got = oc.read_rays([0], s, rays, 4, S, R).astype(np.float64)
    r = rays.astype(np.float64)
    tmin, tmax = r[:, 3], r[:, 7]
    delta = (tmax - tmin) / S
    tstar = (r[:, 2] - z0) / (-r[:, 6])
    zs, ze = r[:, 2] + tmin * r[:, 6], r[:, 2] + tmax * r[:, 6]
    # (point.z rounds by two ulps of |oz| + |t dz| at most: ends that close to the level are left out)
    clear = (np.abs(ze - z0) > 1e-4)
    crosses = (zs < z0) != (ze < z0)
    status = got[:, 3]
    assert np.array_equal(status[clear & crosses & (zs > z0)], np.full((clear & crosses & (zs > z0)).sum(), ray64.ENTER))
    assert np.array_equal(status[clear & crosses & (zs < z0)], np.full((clear & crosses & (zs < z0)).sum(), ray64.LEAVE))       # starting below: LEAVE
    stays = clear & ~crosses
    assert np.all(status[stays] == ray64.MISS) and np.all(got[stays, 0] == tmax[stays]) and np.all(got[stays, 1] == tmax[stays])
    assert np.all((got[stays, 2] < 0) == (ze[stays] < z0)) and (got[stays, 2] < 0).any() and (got[stays, 2] > 0).any()
    k = clear & crosses
    assert k.sum() > 200
    # hi lies above t* by at most the final bracket; t*'s own fp32 image moves by the rounding of point.z over |dz|
    slack = 4 * EPS * (np.abs(r[:, 2]) + np.abs(tstar * r[:, 6])) / np.abs(r[:, 6]) + 4 * EPS * np.abs(tstar)
    assert np.all(got[k, 1] <= tstar[k] + slack[k]) and np.all(tstar[k] <= got[k, 0] + slack[k])
    assert np.all(got[k, 0] - tstar[k] <= delta[k] * 2.0 ** -R + slack[k])
    # the record at hi: the flat surface
    assert np.all(got[k, 6] == F(z0)) and np.all(got[k, 7] == 0) and np.all(got[k, 10] > 0.999)


def test_known_answers_swell(capi):
    S, R = 32, 12
    z0 = 0.25
    rays = _rays(12, 600, spread=40.0, level=z0)
    with _flat(capi) as oc:
        s = _set(capi, 0, swell=True, plane_w=-z0)
        s.swellsteepness = 0.0                                   # a height field: z0 + A sin(theta(x, y))
        got = oc.read_rays([0], s, rays, 4, S, R).astype(np.float64)
    f = surface64.frame64(s)
    r = rays.astype(np.float64)

    def g(t):
        x, y, z = r[:, 0] + t * r[:, 4], r[:, 1] + t * r[:, 5], r[:, 2] + t * r[:, 6]
        return z - (z0 + f["A"] * np.sin(f["frequency"] * (f["dirx"] * x + f["diry"] * y) + f["phase"]))

    # rays steeper than the swell (|dz| > 1.5 A k |d.xy|): g is monotonic along them, one root at most
    steep = np.abs(r[:, 6]) > 1.5 * f["A"] * f["frequency"] * np.hypot(r[:, 4], r[:, 5])
    tmin, tmax = r[:, 3], r[:, 7]
    g0, g1 = g(tmin), g(tmax)
    crosses = steep & ((g0 < 0) != (g1 < 0)) & (np.abs(g0) > 1e-3) & (np.abs(g1) > 1e-3)
    assert crosses.sum() > 150
    lo, hi = tmin.copy(), tmax.copy()
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        same = (g(mid) < 0) == (g0 < 0)
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    root = 0.5 * (lo + hi)
    delta = (tmax - tmin) / S
    slope = np.abs(r[:, 6]) - f["A"] * f["frequency"] * np.hypot(r[:, 4], r[:, 5])
    # fp32 against float64 in g: the phase (|theta| eps A, and sincos's own few ulps) and point(t), over the least slope of g
    reach = (np.abs(r[:, 0:3]) + np.maximum(np.abs(tmin), np.abs(tmax))[:, None] * np.abs(r[:, 4:7])).max(1)
    slack = (16 * EPS * (1 + f["frequency"] * reach) * f["A"] + 8 * EPS * reach) / slope + 4 * EPS * np.abs(root)
    k = crosses
    assert np.array_equal(got[k, 3], np.where(g0[k] < 0, ray64.LEAVE, ray64.ENTER))
    assert np.all(got[k, 1] <= root[k] + slack[k]) and np.all(root[k] <= got[k, 0] + slack[k])
    assert np.all(got[k, 0] - root[k] <= delta[k] * 2.0 ** -R + slack[k])
    away = steep & ((g0 < 0) == (g1 < 0)) & (np.abs(g0) > 1e-3) & (np.abs(g1) > 1e-3)
    assert away.sum() > 50 and np.all(got[away, 3] == ray64.MISS) and np.all((got[away, 2] < 0) == (g1[away] < 0))


# 4 -- edges


def test_edges(capi, oracle, torch):
    N, cascades = 64, [1, 0]
    C = ctypes
    S, R, it = 32, 8, 4
    rays = _rays(5, 257)
    with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
        _step(oc)
        s = _set(capi, 0)
        lib = capi.load()
        before = [oc.read_maps(c).copy() for c in (0, 1)], [oc.read_foam(c).copy() for c in (0, 1)]
        clean = oc.read_rays(cascades, s, rays, it, S, R)
        assert np.isfinite(clean).all()
        assert np.array_equal(_bits(clean), _bits(oc.read_rays(cascades, s, rays, it, S, R)))                  # the same on a second call

        # a bad ray of each kind: NaNs, the neighbours as without it
        bad = rays.copy()
        victims = []
        for k in range(8):
            bad[10 + 3 * k, k] = np.nan if k % 2 else np.inf
            victims.append(10 + 3 * k)
        bad[40, 3], bad[40, 7] = 2.0, 1.0                       # tmax < tmin
        bad[43, 7], bad[43, 4] = 3.0e38, 10.0                   # point(tmax) overflows
        bad[46, 3], bad[46, 6] = -3.0e38, -10.0                 # point(tmin) overflows
        bad[255, 0] = -np.inf                                   # the last ray of the first workgroup
        bad[256, 6] = np.nan                                    # the second workgroup's only ray
        victims += [40, 43, 46, 255, 256]
        assert ray64.bad32(bad).nonzero()[0].tolist() == sorted(victims)
        got = oc.read_rays(cascades, s, bad, it, S, R)
        keep = np.setdiff1d(np.arange(len(rays)), victims)
        assert np.isnan(got[victims]).all()
        assert np.array_equal(_bits(got[keep]), _bits(clean[keep]))

        # n in {0, 1, 257}
        assert oc.read_rays(cascades, s, rays[:0], it, S, R).shape == (0, 12)
        assert np.array_equal(_bits(oc.read_rays(cascades, s, rays[:1], it, S, R)), _bits(clean[:1]))
        arr = (capi.I * 2)(*cascades)
        assert lib.datum_ocean_cast_rays(oc.h, arr, 2, C.byref(s), it, S, R, None, 0, None) == capi.OK

        # device arrays: the same bits, a canary behind the records left alone
        n = len(rays)
        dr = torch.from_numpy(rays).cuda()
        out = torch.full((n * 12 + 64,), -3.0e38, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        oc.cast_rays(cascades, s, dr.data_ptr(), n, out.data_ptr(), it, S, R)
        oc.sync()
        raw = out.cpu().numpy()
        assert np.array_equal(_bits(raw[: n * 12].reshape(n, 12)), _bits(clean))
        assert np.all(raw[n * 12:] == F(-3.0e38))
        assert np.array_equal(dr.cpu().numpy().view(np.uint32), rays.view(np.uint32))

        # argument errors with a live handle
        P = capi.P
        rec = np.zeros((n, 12), F)
        rp, op = rays.ctypes.data_as(P), rec.ctypes.data_as(P)
        sp = C.byref(s)
        calls = [
            (None, 2, sp, it, S, R, rp, n, op), (arr, 0, sp, it, S, R, rp, n, op), (arr, 17, sp, it, S, R, rp, n, op),
            ((capi.I * 2)(0, 2), 2, sp, it, S, R, rp, n, op), (arr, 2, None, it, S, R, rp, n, op),
            (arr, 2, sp, -1, S, R, rp, n, op), (arr, 2, sp, 17, S, R, rp, n, op),
            (arr, 2, sp, it, 0, R, rp, n, op), (arr, 2, sp, it, 1025, R, rp, n, op), (arr, 2, sp, it, S, -1, rp, n, op), (arr, 2, sp, it, S, 25, rp, n, op),
            (arr, 2, sp, it, S, R, None, n, op), (arr, 2, sp, it, S, R, rp, n, None),
            (arr, 2, sp, it, S, R, P(rays.ctypes.data + 8), n - 1, op), (arr, 2, sp, it, S, R, rp, n, P(rec.ctypes.data + 4)),
            (arr, 2, sp, it, S, R, rp, 1 << 31, op),
        ]
        assert rays.ctypes.data % 16 == 0 and rec.ctypes.data % 16 == 0
        for args in calls:
            for name in ("datum_ocean_read_rays", "datum_ocean_cast_rays"):
                assert getattr(lib, name)(oc.h, *args) == capi.EINVAL, (name, args[1], args[3:6], args[7])
                assert name.encode() in lib.datum_ocean_last_error(oc.h)
        # the ends of the ranges are inside
        assert np.isfinite(oc.read_rays(cascades, s, rays[:3], it, 1024, 24)).all()

        # the calls left the maps and the foam planes as they were
        for c in (0, 1):
            assert np.array_equal(_bits(before[0][c]), _bits(oc.read_maps(c)))
            assert np.array_equal(_bits(before[1][c]), _bits(oc.read_foam(c)))


def test_bound_maps_give_the_same_bits(capi, oracle, torch):
    N, cascades = 64, [1, 0]
    rays = _rays(9, 700)
    own = _setup(capi, oracle, N, 2, foam="accumulate")
    bound = _setup(capi, oracle, N, 2)
    nbytes = own.maps_device()[1]
    buf = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    foambuf = torch.zeros(2 * N * N, dtype=torch.float32, device="cuda")
    with own, bound:
        bound.bind_maps(buf.data_ptr(), nbytes)
        bound.bind_foam(foambuf.data_ptr(), 2 * N * N * 4)
        bound.set_foam("accumulate")
        for oc in (own, bound):
            _step(oc)
        s = _set(capi, 0)
        a, b = own.read_rays(cascades, s, rays, 4, 32, 8), bound.read_rays(cascades, s, rays, 4, 32, 8)
        assert np.isfinite(a).all() and _mix(a)[0]
        assert np.array_equal(_bits(a), _bits(b))


# 5 -- the C++ shim


def test_cpp_shim_matches_capi(capi):
    from datum_amd import host_api

    N = 256
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.4))
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    rays = _rays(13, 500, level=0.0)
    with host_api.OceanContext(N) as ctx:
        mesh = ctx.create_ocean(32, 32)
        for _ in range(2):
            params.update_ocean(DT)
            ctx.render_ocean_surface(mesh, params, camera)
        lib = capi.load()
        h = ctx.lib.datum_host_context_handle(ctx.c)
        one = (capi.I * 1)(0)
        for it, S, R in ((0, 8, 0), (4, 32, 8)):
            got = ctx.cast_ocean_rays(params, rays, it, S, R)
            s = params.oceanset(camera)
            want = np.empty_like(got)
            P = capi.P
            assert lib.datum_ocean_read_rays(h, one, 1, ctypes.byref(s), it, S, R, rays.ctypes.data_as(P), len(rays), want.ctypes.data_as(P)) == capi.OK
            assert np.array_equal(_bits(got), _bits(want)), (it, S, R)
            assert np.isfinite(got).all() and (got[:, 3] == ray64.ENTER).any() and (got[:, 3] == ray64.LEAVE).any()
