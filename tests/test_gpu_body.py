"""Body buoyancy (include/datum_ocean_hip.h: datum_ocean_reduce_bodies) on the MI355X.

  1  bits: read_bodies against body64.reduce32 of the records read_surface_blend gives at body64.world32's points -- no tolerance: the
     per-probe records are held to float64 by tests/test_gpu_blend.py, the sum's order is the definition's;
  2  against body64 end to end, a cross-check that the chain closes.  Per probe the height differs from float64 by at most
       h_i = K_POS eps S_i  +  3 eps (|R||x| + |T|) (1 + 2 G)
     -- the height bar of tests/test_gpu_blend.py (K_POS imported; S_i = (1 + |q_i|)(1 + G), G = sum_c N scale_c max|D_c|; two texels
     differ by at most 2 max|D|, so 2 G bounds the gradient) and the transform's three roundings per component, which move w.z directly and
     the height through w.xy by the gradient.  min / max are 1-Lipschitz, so a body's Fz lies within sum a_i h_i, tau within
     sum a_i (|r_i| h_i + d_i 2 * 3 eps (|R||x| + |T|)), plus 3 eps sum |term| for the roundings inside a term (d, a d, r m) and the bound
     of the stated order (body64.bound64).  `wet` may differ by the weights of the probes whose float64 |rec.z - w.z| is inside h_i:
     the poses keep those to at most 2 % of the probes, asserted;
  3  known answers on the flat ocean; 4  edges; 5  the C++ shim.
"""

import ctypes

import numpy as np
import pytest

import body64
from test_gpu_blend import K_POS
from test_gpu_surface import DT, EPS, SCALES, _set, _setup

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = (0, 1, 63, 64, 65, 129, 1000)
NBODIES = 301                # the last workgroup holds one body
NPROBES = 1500


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


def _scale(c):
    return F(1.0) / F(SCALES[c % 4])


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _fleet(seed, nbodies=NBODIES, nprobes=NPROBES, counts=None):
    """bodies of random poses (every fifth the identity) around the water line, their ranges anywhere in a shared probe array; the counts
    cycle through COUNTS with 1000 kept to every 43rd body"""
    rng = np.random.RandomState(seed)
    if counts is None:
        small = [c for c in COUNTS if c != 1000]
        counts = [1000 if b % 43 == 7 else small[b % len(small)] for b in range(nbodies)]
    rot = [np.eye(3) if b % 5 == 0 else _rotation(rng) for b in range(nbodies)]
    pos = rng.uniform(-200, 200, (nbodies, 3))
    pos[:, 2] = rng.uniform(-1.5, 2.5, nbodies)
    firsts = [int(rng.randint(0, nprobes - c + 1)) for c in counts]
    caps = np.where(rng.uniform(size=nbodies) < 0.3, np.inf, rng.uniform(0.3, 2.0, nbodies))
    probes = rng.uniform(-3, 3, (nprobes, 4)).astype(F)
    probes[:, 3] = rng.uniform(0.05, 2.0, nprobes)
    return body64.make_bodies(rot, pos, firsts, counts, caps), probes


def _step(oc, steps=2):
    for _ in range(steps):
        oc.update(DT)
        oc.displace()


def _want32(oc, cascades, s, bodies, probes, it):
    w, _, bad = body64.world32(bodies, probes)
    assert not bad.any()
    recs = oc.read_surface_blend(cascades, s, np.ascontiguousarray(w[:, :2]), it)
    return body64.reduce32(bodies, probes, recs), recs


# 1 -- bits


@pytest.mark.parametrize("N,C,lists", [(64, 3, ([1], [0, 2], [0, 1, 2])), (2048, 2, ([1], [0, 1]))])
def test_bits(capi, oracle, N, C, lists):
    bodies, probes = _fleet(N)
    assert set(bodies["count"].tolist()) == set(COUNTS) and len(bodies) % 4 == 1
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        for cascades in lists:
            for swell in (True, False):
                s = _set(capi, 0, swell)
                for it in (0, 4, 16):
                    got = oc.read_bodies(cascades, s, bodies, probes, it)
                    want, _ = _want32(oc, cascades, s, bodies, probes, it)
                    assert np.isfinite(got).all()
                    assert np.array_equal(_bits(got), _bits(want)), (N, cascades, swell, it, np.argwhere(_bits(got) != _bits(want))[:4])
        assert got[:, 0].max() > 1 and (got[:, 3] == 0).any()


# 2 -- against body64 end to end


@pytest.mark.parametrize("N,C,cascades", [(64, 3, [0, 1, 2]), (2048, 2, [0, 1])])
def test_against_body64(capi, oracle, report, N, C, cascades):
    bodies, probes = _fleet(N + 1)
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        maps_list, scales = [oc.read_maps(c) for c in cascades], [_scale(c) for c in cascades]
        foams = [oc.read_foam(c) for c in cascades]
        s = _set(capi, 0)
        it = 4
        got = oc.read_bodies(cascades, s, bodies, probes, it).astype(np.float64)
        want, pp = body64.body64(bodies, probes, maps_list, foams, "accumulate", scales, s, it)

    G = sum(N * float(sc) * float(np.abs(m[0, ..., :3]).max()) for m, sc in zip(maps_list, scales))
    bi, w, a = pp["body"], pp["w"], pp["a"]
    R, T = np.abs(bodies["rotation"][bi].astype(np.float64)), np.abs(bodies["position"][bi].astype(np.float64))
    x = np.abs(probes[body64._gather(bodies, probes)[1], :3].astype(np.float64))
    reach = (R.reshape(-1, 3, 3) * x[:, None, :]).sum(2).max(1) + T.max(1)               # |R||x| + |T|, the largest component
    S = (1.0 + np.abs(w[:, :2]).max(1)) * (1.0 + G)
    tr = 3 * EPS * reach
    h = K_POS * EPS * S + tr * (1.0 + 2.0 * G)
    d = np.minimum(np.maximum(pp["d"], 0.0), bodies["cap"][bi].astype(np.float64))
    arm = np.hypot(w[:, 0] - bodies["position"][bi, 0], w[:, 1] - bodies["position"][bi, 1])

    def per_body(v):
        out = np.zeros(len(bodies))
        np.add.at(out, bi, v)
        return out

    mag = np.zeros((len(bodies), 8))
    for k, v in enumerate((a * d, a * d * arm, a * d * arm, a)):
        mag[:, k] = per_body(v)
    order = body64.bound64(bodies, mag)
    bar_f = per_body(a * h) + order[:, 0] + 3 * EPS * mag[:, 0]
    bar_t = per_body(a * (arm * h + d * 2 * tr)) + order[:, 1] + 3 * EPS * mag[:, 1]
    near = np.abs(pp["d"]) <= h
    share = float(near.mean())
    bar_w = per_body(np.where(near, a, 0.0)) + order[:, 3]

    err = np.abs(got - want)
    rf, rt = float((err[:, 0] / np.maximum(bar_f, 1e-300)).max()), float((err[:, 1:3].max(1) / np.maximum(bar_t, 1e-300)).max())
    report(f"body vs body64 N={N} list={cascades}: Fz error / bar {rf:.3f}, tau error / bar {rt:.3f}, probes within the height bar of the water line {share:.4%}")
    assert share <= 0.02, share
    assert np.all(err[:, 0] <= bar_f), rf
    assert np.all(err[:, 1] <= bar_t) and np.all(err[:, 2] <= bar_t), rt
    assert np.all(err[:, 3] <= bar_w)
    res_bar = per_body(np.zeros(len(bi)))
    np.maximum.at(res_bar, bi, K_POS * EPS * S + 2 * tr)
    assert np.all(err[:, 7] <= res_bar)


# 3 -- known answers on the flat ocean


def _box(n=9, half=2.0):
    g = np.linspace(-half, half, n)
    xx, yy = np.meshgrid(g, g)
    p = np.zeros((n * n, 4), F)
    p[:, 0], p[:, 1], p[:, 3] = xx.ravel(), yy.ravel(), 0.25
    return p


def test_known_answers(capi):
    N = 64
    probes = _box()
    n = len(probes)
    sa = float(probes[:, 3].sum())
    phi = 0.25
    c, sn = np.cos(phi), np.sin(phi)
    roll = [[1, 0, 0], [0, c, -sn], [0, sn, c]]
    # water at z = 0.25 (plane.w = -0.25, no swell, h0 = 0); body origins at depth 0.5, in the water line, 5 m above
    bodies = body64.make_bodies([np.eye(3), np.eye(3), np.eye(3), roll], [[10, -20, -0.25], [10, -20, -0.25], [3, 4, 5.25], [-7, 2, -1.25]],
                                [0] * 4, [n] * 4, [np.inf, 0.125, np.inf, np.inf])
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, 22.0, 1.35)
        oc.upload_state(0, np.zeros((N, N, 2), F))
        oc.update(DT)
        oc.displace()
        s = _set(capi, 0, swell=False, plane_w=-0.25)
        r = oc.read_bodies([0], s, bodies, probes, 4).astype(np.float64)
    eps_order = (n // 64 + 1 + 6) * EPS

    # level box at depth h = 0.5: every d = 0.5 exactly, Fz = h sum a, tau = 0 -- to the bound of the order
    assert abs(r[0, 0] - 0.5 * sa) <= eps_order * 0.5 * sa
    lever = float((np.abs(probes[:, 1]) * probes[:, 3] * 0.5).sum())
    # (the lever arm: w = x + T rounds by half an ulp of |w| < 32, 16 eps; the products a d and r m by eps each)
    tol = eps_order * lever + 16 * EPS * 0.5 * sa + 2 * EPS * lever
    assert abs(r[0, 1]) <= tol and abs(r[0, 2]) <= tol
    assert r[0, 3] == sa and r[0, 7] == 0
    assert abs(r[0, 6] - r[0, 0]) <= eps_order * r[0, 0] and r[0, 4] == 0 and r[0, 5] == 0                               # the normal is (0, 0, 1)

    # cap saturates
    assert abs(r[1, 0] - 0.125 * sa) <= eps_order * 0.125 * sa and r[1, 3] == sa

    # above the water: zeros
    assert np.all(r[2] == 0)

    # rolled by phi about x, origin at depth h0 = 1.5: d = h0 - y sin(phi) > 0 for every probe, r.y = y cos(phi), so
    # tau x = sum a y cos (h0 - y sin) = -a sin cos sum y^2 on a symmetric box, Fz = h0 sum a, tau y = sum -(x m) = 0
    y = probes[:, 1].astype(np.float64)
    av = probes[:, 3].astype(np.float64)
    taux = float((av * y * c * (1.5 - y * sn)).sum())
    assert abs(taux - (-0.25 * sn * c * float((y * y).sum()))) < 1e-12
    mags = float((av * np.abs(y) * c * (1.5 - y * sn)).sum())
    # beyond the order: sin and cos rounded to fp32 (eps each), three roundings in w.y and w.z against |T| + |y| <= 9.25, one in d and in r.y
    slack = 8 * EPS * mags + float((av * (np.abs(y) * 4 * EPS * 9.25 + 2.0 * 4 * EPS * 9.25)).sum())
    assert abs(r[3, 1] - taux) <= eps_order * mags + slack, (r[3, 1], taux)
    assert abs(r[3, 0] - 1.5 * sa) <= eps_order * 1.5 * sa + 2 * EPS * 1.5 * sa + float((av * 4 * EPS * 9.25).sum())
    magx = float((av * np.abs(probes[:, 0]) * (1.5 - y * sn)).sum())
    assert abs(r[3, 2]) <= eps_order * magx + 8 * EPS * magx + float((av * (np.abs(probes[:, 0]) + 2.0) * 4 * EPS * 9.25).sum())
    assert r[3, 3] == sa


# 4 -- edges


def test_edges(capi, oracle, torch):
    N, cascades = 64, [1, 0]
    C = ctypes
    bodies, probes = _fleet(5, nbodies=41, nprobes=600, counts=[(7, 64, 65, 130, 1, 0, 200)[b % 7] for b in range(41)])
    with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
        _step(oc)
        s = _set(capi, 0)
        lib = capi.load()
        before = [oc.read_maps(c).copy() for c in (0, 1)], [oc.read_foam(c).copy() for c in (0, 1)]
        clean = oc.read_bodies(cascades, s, bodies, probes, 4)
        assert np.isfinite(clean).all()
        assert np.array_equal(_bits(clean), _bits(oc.read_bodies(cascades, s, bodies, probes, 4)))             # the same on a second call

        # bad bodies: NaN records, the others as without them
        bad = bodies.copy()
        pb = probes.copy()
        bad["first"][3], bad["count"][10] = -1, -2
        bad["first"][11], bad["count"][11] = 600 - 63, 64
        bad["first"][12], bad["count"][12] = 2 ** 31 - 1, 2 ** 31 - 1
        bad["cap"][17] = np.nan
        bad["position"][20, 0] = np.inf
        bad["rotation"][24, 8] = np.nan
        victims = [3, 10, 11, 12, 17, 20, 24]
        counted = [b for b in (20, 24) if bad["count"][b] > 0]
        r = oc.read_bodies(cascades, s, bad, pb, 4)
        nanrows = [b for b in victims if b not in (20, 24) or b in counted]
        assert np.isnan(r[nanrows]).all()
        keep = np.setdiff1d(np.arange(len(bodies)), victims)
        assert np.array_equal(_bits(r[keep]), _bits(clean[keep]))
        # a bad probe spoils exactly the bodies whose range holds it
        pb[300, 3] = np.nan
        pb[301, 1] = -np.inf
        r = oc.read_bodies(cascades, s, bodies, pb, 4)
        f, c = bodies["first"].astype(int), bodies["count"].astype(int)
        hit = ((f <= 300) & (300 < f + c)) | ((f <= 301) & (301 < f + c))
        assert hit.any() and not hit.all()
        assert np.isnan(r[hit]).all()
        assert np.array_equal(_bits(r[~hit]), _bits(clean[~hit]))

        # device arrays: the same bits, a guard tail behind the records left alone
        nb = len(bodies)
        db = torch.from_numpy(bodies.view(np.uint8).reshape(nb, 64).copy()).cuda()
        dp = torch.from_numpy(probes).cuda()
        out = torch.full((nb * 8 + 64,), -3.0e38, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        oc.reduce_bodies(cascades, s, db.data_ptr(), nb, dp.data_ptr(), len(probes), out.data_ptr(), 4)
        oc.sync()
        raw = out.cpu().numpy()
        assert np.array_equal(_bits(raw[: nb * 8].reshape(nb, 8)), _bits(clean))
        assert np.all(raw[nb * 8:] == F(-3.0e38))

        # nbodies == 0
        assert oc.read_bodies(cascades, s, bodies[:0], probes, 4).shape == (0, 8)
        arr = (capi.I * 2)(*cascades)
        assert lib.datum_ocean_reduce_bodies(oc.h, arr, 2, C.byref(s), 4, None, 0, None, 0, None) == capi.OK
        # no probes at all: bodies of count 0 give zeros
        empty = body64.make_bodies([np.eye(3)] * 2, np.zeros((2, 3)), [0, 0], [0, 0], [1.0, np.inf])
        assert np.all(_bits(oc.read_bodies(cascades, s, empty, probes[:0], 4)) == 0)

        # argument errors with a live handle
        P = capi.P
        rec = np.zeros((nb, 8), F)
        bp, pp, rp = bodies.ctypes.data_as(P), probes.ctypes.data_as(P), rec.ctypes.data_as(P)
        calls = [
            (None, 2, C.byref(s), 4, bp, nb, pp, 600, rp), (arr, 0, C.byref(s), 4, bp, nb, pp, 600, rp), (arr, 17, C.byref(s), 4, bp, nb, pp, 600, rp),
            ((capi.I * 2)(0, 2), 2, C.byref(s), 4, bp, nb, pp, 600, rp), (arr, 2, None, 4, bp, nb, pp, 600, rp),
            (arr, 2, C.byref(s), -1, bp, nb, pp, 600, rp), (arr, 2, C.byref(s), 17, bp, nb, pp, 600, rp),
            (arr, 2, C.byref(s), 4, None, nb, pp, 600, rp), (arr, 2, C.byref(s), 4, bp, nb, None, 600, rp), (arr, 2, C.byref(s), 4, bp, nb, pp, 600, None),
            (arr, 2, C.byref(s), 4, P(bodies.ctypes.data + 4), nb - 1, pp, 600, rp), (arr, 2, C.byref(s), 4, bp, nb, P(probes.ctypes.data + 8), 599, rp),
            (arr, 2, C.byref(s), 4, bp, nb, pp, 600, P(rec.ctypes.data + 4)),
            (arr, 2, C.byref(s), 4, bp, 1 << 31, pp, 600, rp), (arr, 2, C.byref(s), 4, bp, nb, pp, 1 << 31, rp),
        ]
        assert bodies.ctypes.data % 16 == 0 and probes.ctypes.data % 16 == 0 and rec.ctypes.data % 16 == 0
        for args in calls:
            for name in ("datum_ocean_read_bodies", "datum_ocean_reduce_bodies"):
                assert getattr(lib, name)(oc.h, *args) == capi.EINVAL, (name, args[1:4], args[5], args[7])
                assert name.encode() in lib.datum_ocean_last_error(oc.h)

        # the calls left the maps and the foam planes as they were
        for c in (0, 1):
            assert np.array_equal(_bits(before[0][c]), _bits(oc.read_maps(c)))
            assert np.array_equal(_bits(before[1][c]), _bits(oc.read_foam(c)))


def test_bound_maps_give_the_same_bits(capi, oracle, torch):
    N, cascades = 64, [1, 0]
    bodies, probes = _fleet(9, nbodies=50, nprobes=400, counts=[(5, 64, 129)[b % 3] for b in range(50)])
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
        a, b = own.read_bodies(cascades, s, bodies, probes, 4), bound.read_bodies(cascades, s, bodies, probes, 4)
        assert np.isfinite(a).all() and a[:, 0].max() > 0
        assert np.array_equal(_bits(a), _bits(b))


# 5 -- the C++ shim


def test_cpp_shim_matches_capi(capi):
    from datum_amd import host_api

    N = 256
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.4))
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    bodies, probes = _fleet(13, nbodies=77, nprobes=500, counts=[(0, 1, 64, 65, 200)[b % 5] for b in range(77)])
    with host_api.OceanContext(N) as ctx:
        mesh = ctx.create_ocean(32, 32)
        for _ in range(2):
            params.update_ocean(DT)
            ctx.render_ocean_surface(mesh, params, camera)
        lib = capi.load()
        h = ctx.lib.datum_host_context_handle(ctx.c)
        one = (capi.I * 1)(0)
        for it in (0, 4):
            got = ctx.reduce_ocean_bodies(params, bodies, probes, it)
            s = params.oceanset(camera)
            want = np.empty_like(got)
            P = capi.P
            assert lib.datum_ocean_read_bodies(h, one, 1, ctypes.byref(s), it, bodies.ctypes.data_as(P), len(bodies), probes.ctypes.data_as(P), len(probes),
                                               want.ctypes.data_as(P)) == capi.OK
            assert np.array_equal(_bits(got), _bits(want)), it
            assert np.isfinite(got).all() and got[:, 0].max() > 0
