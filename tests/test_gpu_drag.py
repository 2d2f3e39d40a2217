"""Body drag (include/datum_ocean_hip.h: datum_ocean_reduce_body_drag) on the MI355X.

  1  bits: read_body_drag against drag64.reduce32 of the records read_velocity_blend gives at body64.world32's points -- no tolerance: the
     per-probe records are pinned by tests/test_gpu_velocity.py, the sum's order is the definition's.  The same comparison holds the
     device's sqrt to the correctly rounded one (numpy's).  Field 6 is read_bodies' field 0, bit for bit;
  2  against drag64 end to end, from the maps and planes read back: a cross-check that the chain closes.  With eps = 2^-24, per probe i
     (tests/test_gpu_body.py's symbols: reach_i = |R||x| + |T|, S_i = (1 + |q_i|)(1 + G), G = sum_c N scale_c max|D_c|):
       tr_i  = 3 eps reach_i                               a component of w: the transform's three roundings
       h_i   = K_POS eps S_i + tr_i (1 + 2 G)              the submersion d (test_gpu_body's height bar; min / max are 1-Lipschitz), so
       dm_i  = a_i h_i                                     the weight m
       dr_i  = tr_i + eps |r_i|                            a component of r = w - T: w's error and one rounding
       p_i   = K_POS eps S_i + tr_i                        the position the planes are sampled at: the query's position bar and q's own error
       dv_i  = (5 + C) eps sum_c max|U_c| + 2 GU p_i       a component of the velocity sample: bilinear rounding of the plane -- a weight
                                                           is two roundings (1 - a, the product), the blend a product and three fmas, against
                                                           weights that sum to 1; C - 1 additions over the list -- plus the plane's gradient,
                                                           two texels' difference <= 2 max|U_c| per texel, N scale_c texels per metre
                                                           (GU = sum_c N scale_c max|U_c|), times the position bar
       du_i  = 2 |omega| dr_i + 3 eps (|v| + 2 |omega| |r_i|)     a component of u = v + omega x r: r's error, and three roundings (product,
                                                           difference, sum) of a value below |v| + 2 |omega| |r_i|   (|.| of a vector here: its
                                                           largest component)
       E_i   = sqrt(3) (dv_i + du_i + eps |e_i|)           |delta e| as a vector: the three above and e's own subtraction
       DF_i  = dm_i c_i s_i + m_i (cl + 2 cq s_i) E_i + 9 eps |f_i|       |delta f|, c_i = cl + cq s_i: the weight's error; |delta(s e)| <= 2 s
                                                           |delta e| for the quadratic term and |delta e| for the linear one; nine roundings
                                                           inside a term (d, a d; s: two products' sum, a sum, the root = three; cq s, cl +, m (),
                                                           k e)
       DT_i  = sqrt(3) dr_i |f_i| + |r_i|_2 DF_i + 3 sqrt(3) eps |r_i|_2 |f_i|    |delta tau|: r's error, f's error, and three roundings per
                                                           component (two products, a difference) of values below |r||f|
     A body's F lies within sum DF_i, tau within sum DT_i, field 6 within sum dm_i + 2 eps sum m_i, each plus the bound of the stated
     order (body64.bound64 on the sums of the terms' magnitudes); field 7 within the residual bar of test_gpu_body.  m_i, s_i, e_i, f_i, r_i
     are float64's.  No constant is free: K_POS is imported, every other figure counts roundings;
  3  known answers on the flat ocean; 4  edges; 5  a bound velocity plane; 6  the C++ shim.
"""

import ctypes

import numpy as np
import pytest

import body64
import drag64
from test_gpu_blend import K_POS
from test_gpu_body import COUNTS, _box, _fleet, _scale, _step
from test_gpu_surface import DT, EPS, _set, _setup

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


def _motions(seed, nb):
    """linear within 3 m/s, angular within 1 rad/s, cl and cq in [0, 2]; every fourth body without cq, every fifth without cl, every
    seventh fully at rest"""
    rng = np.random.RandomState(seed)
    b = np.arange(nb)
    m = drag64.make_motions(rng.uniform(-3, 3, (nb, 3)), rng.uniform(-1, 1, (nb, 3)), rng.uniform(0, 2, nb), rng.uniform(0, 2, nb))
    m["cq"][b % 4 == 1] = 0
    m["cl"][b % 5 == 2] = 0
    rest = b % 7 == 3
    m["linear"][rest], m["angular"][rest] = 0, 0
    return m


def _moving(capi, oracle, N, C, foam="accumulate"):
    oc = _setup(capi, oracle, N, C, foam=foam)
    oc.set_velocity("on")
    return oc


def _want32(oc, cascades, s, bodies, motions, probes, it):
    w, _, bad = body64.world32(bodies, probes)
    assert not bad.any()
    recs = oc.read_velocity_blend(cascades, s, np.ascontiguousarray(w[:, :2]), it)
    return drag64.reduce32(bodies, motions, probes, recs)


# 1 -- bits


@pytest.mark.parametrize("N,C,lists", [(64, 3, ([1], [0, 2], [0, 1, 2])), (2048, 2, ([1], [0, 1]))])
def test_bits(capi, oracle, N, C, lists):
    bodies, probes = _fleet(N)
    motions = _motions(N, len(bodies))
    assert set(bodies["count"].tolist()) == set(COUNTS) and len(bodies) % 4 == 1
    assert (motions["cq"] == 0).any() and (motions["cl"] == 0).any() and (np.abs(motions["linear"]).max(1) == 0).any()
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        for cascades in lists:
            for swell in (True, False):
                s = _set(capi, 0, swell)
                for it in (0, 4, 16):
                    got = oc.read_body_drag(cascades, s, bodies, motions, probes, it)
                    want = _want32(oc, cascades, s, bodies, motions, probes, it)
                    assert np.isfinite(got).all()
                    assert np.array_equal(_bits(got), _bits(want)), (N, cascades, swell, it, np.argwhere(_bits(got) != _bits(want))[:4])
                    lift = oc.read_bodies(cascades, s, bodies, probes, it)
                    assert np.array_equal(_bits(got[:, 6]), _bits(lift[:, 0])), (N, cascades, swell, it)
        force = np.sqrt((got[:, :3].astype(np.float64) ** 2).sum(1))
        assert force.max() > 1 and np.abs(got[:, 3:6]).max() > 1
        dry = (got[:, 6] == 0) & (bodies["count"] > 0)
        assert dry.any() and np.all(got[dry, :6] == 0)


# 2 -- against drag64 end to end


@pytest.mark.parametrize("N,C,cascades", [(64, 3, [0, 1, 2]), (2048, 2, [0, 1])])
def test_against_drag64(capi, oracle, report, N, C, cascades):
    bodies, probes = _fleet(N + 1)
    motions = _motions(N + 1, len(bodies))
    with _moving(capi, oracle, N, C) as oc:
        _step(oc)
        maps_list, scales = [oc.read_maps(c) for c in cascades], [_scale(c) for c in cascades]
        planes = [oc.read_velocity(c) for c in cascades]
        s = _set(capi, 0)
        it = 4
        got = oc.read_body_drag(cascades, s, bodies, motions, probes, it).astype(np.float64)
        want, pp = drag64.drag64(bodies, motions, probes, maps_list, planes, scales, s, it)

    nl = len(cascades)
    G = sum(N * float(sc) * float(np.abs(m[0, ..., :3]).max()) for m, sc in zip(maps_list, scales))
    umax = [float(np.abs(pl[..., :3]).max()) for pl in planes]
    GU = sum(N * float(sc) * u for sc, u in zip(scales, umax))
    assert min(umax) > 0
    bi, w, a = pp["body"], pp["w"], pp["a"]
    R, T = np.abs(bodies["rotation"][bi].astype(np.float64)), np.abs(bodies["position"][bi].astype(np.float64))
    x = np.abs(probes[body64._gather(bodies, probes)[1], :3].astype(np.float64))
    reach = (R.reshape(-1, 3, 3) * x[:, None, :]).sum(2).max(1) + T.max(1)               # |R||x| + |T|, the largest component
    S = (1.0 + np.abs(w[:, :2]).max(1)) * (1.0 + G)
    tr = 3 * EPS * reach
    h = K_POS * EPS * S + tr * (1.0 + 2.0 * G)

    r, e, sp, f, m = pp["r"], pp["e"], pp["s"], pp["f"], pp["m"]
    v, om = np.abs(motions["linear"][bi].astype(np.float64)).max(1), np.abs(motions["angular"][bi].astype(np.float64)).max(1)
    cl, cq = motions["cl"][bi].astype(np.float64), motions["cq"][bi].astype(np.float64)
    rmax, r2, f2 = np.abs(r).max(1), np.sqrt((r * r).sum(1)), np.sqrt((f * f).sum(1))
    dm = a * h
    dr = tr + EPS * rmax
    p = K_POS * EPS * S + tr
    dv = (5 + nl) * EPS * sum(umax) + 2.0 * GU * p
    du = 2.0 * om * dr + 3 * EPS * (v + 2.0 * om * rmax)
    E = np.sqrt(3.0) * (dv + du + EPS * np.abs(e).max(1))
    DF = dm * (cl + cq * sp) * sp + m * (cl + 2.0 * cq * sp) * E + 9 * EPS * f2
    DT_ = np.sqrt(3.0) * dr * f2 + r2 * DF + 3 * np.sqrt(3.0) * EPS * r2 * f2

    def per_body(val):
        out = np.zeros(len(bodies))
        np.add.at(out, bi, val)
        return out

    mag = np.zeros((len(bodies), 8))
    mag[:, 0] = mag[:, 1] = mag[:, 2] = per_body(f2)
    mag[:, 3] = mag[:, 4] = mag[:, 5] = per_body(r2 * f2)
    mag[:, 6] = per_body(m)
    order = body64.bound64(bodies, mag)
    bar_f = per_body(DF) + order[:, 0]
    bar_t = per_body(DT_) + order[:, 3]
    bar_m = per_body(dm) + 2 * EPS * mag[:, 6] + order[:, 6]
    res_bar = per_body(np.zeros(len(bi)))
    np.maximum.at(res_bar, bi, K_POS * EPS * S + 2 * tr)

    err = np.abs(got - want)
    ratios = [float((err[:, k] / np.maximum(bar, 1e-300)).max()) for k, bar in enumerate([bar_f] * 3 + [bar_t] * 3 + [bar_m, res_bar])]
    line = f"drag vs drag64 N={N} list={cascades}: error / bar per field " + " ".join(f"{x:.3f}" for x in ratios)
    print(line)
    report(line)
    assert np.isfinite(got).all() and np.sqrt((got[:, :3] ** 2).sum(1)).max() > 1
    for k in range(3):
        assert np.all(err[:, k] <= bar_f), (k, ratios[k])
        assert np.all(err[:, 3 + k] <= bar_t), (3 + k, ratios[3 + k])
    assert np.all(err[:, 6] <= bar_m), ratios[6]
    assert np.all(err[:, 7] <= res_bar), ratios[7]


# 3 -- known answers on the flat ocean


def test_known_answers(capi):
    N = 64
    probes = _box()
    n = len(probes)
    x, y = probes[:, 0].astype(np.float64), probes[:, 1].astype(np.float64)
    sa = float(probes[:, 3].sum())
    Lx, Ly, Q = float(np.abs(x).sum()), float(np.abs(y).sum()), float((x * x + y * y).sum())
    # water at z = 0.25 (plane.w = -0.25, no swell, h0 = 0: the velocity plane is zeros); body origins at depth 0.5, and 5 m above
    deep, high = [10, -20, -0.25], [3, 4, 5.25]
    bodies = body64.make_bodies([np.eye(3)] * 4, [deep, deep, high, deep], [0] * 4, [n] * 4, [np.inf] * 4)
    v = np.array([1.5, -2.0, 0.5], F).astype(np.float64)
    cl0, cq0, cl1, Om = (float(F(t)) for t in (0.8, 0.6, 1.3, 0.7))
    motions = drag64.make_motions([v, [0, 0, 0], [1, 2, 3], v], [[0, 0, 0], [0, 0, Om], [0.1, 0.2, 0.3], [0.3, -0.2, 0.1]], [cl0, cl1, 1.0, 0.0], [cq0, 0.0, 1.0, 0.0])
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, 22.0, 1.35)
        oc.upload_state(0, np.zeros((N, N, 2), F))
        oc.set_velocity("on")
        oc.update(DT)
        oc.displace()
        assert np.all(oc.read_velocity(0) == 0)
        s = _set(capi, 0, swell=False, plane_w=-0.25)
        raw = oc.read_body_drag([0], s, bodies, motions, probes, 4)
        lift = oc.read_bodies([0], s, bodies, probes, 4)
    r = raw.astype(np.float64)
    eps_order = (n // 64 + 1 + 6) * EPS
    m = 0.25 * 0.5                      # every probe: a = 0.25, d = 0.5, exactly
    # (the lever arm: w = x + T rounds by half an ulp of |w| < 32, 16 eps; r = w - T is exact; r.z = 0 exactly)
    arm = 16 * EPS

    # translating, omega = 0: u = v and e = -v exactly, every probe the same f = -m (cl + cq |v|) v -- seven roundings (|v|: three; cq s,
    # cl +, m (), k e) -- and F = n f to the bound of the order; tau = (sum r) x f = 0 on the symmetric box
    f = -m * (cl0 + cq0 * np.linalg.norm(v)) * v
    af = np.abs(f)
    assert np.all(np.abs(r[0, :3] - n * f) <= (eps_order + 7 * EPS) * n * af), (r[0, :3], n * f)
    rnd = eps_order + 10 * EPS           # f's seven, and a torque's two products and difference
    assert abs(r[0, 3]) <= af[2] * (arm * n + rnd * Ly)
    assert abs(r[0, 4]) <= af[2] * (arm * n + rnd * Lx)
    assert abs(r[0, 5]) <= (af[1] * Lx + af[0] * Ly) * rnd + arm * n * (af[0] + af[1])
    assert abs(r[0, 6] - 0.5 * sa) <= eps_order * 0.5 * sa and r[0, 7] == 0

    # yawing, v = 0, cq = 0: u = Om (-r.y, r.x, 0), k = m cl (cq s = 0), f = m cl Om (r.y, -r.x, 0): three roundings (Om r, m cl, k e);
    # F = 0 on the symmetric box, F z and tau x, tau y are zero exactly (r.z = 0), tau z = -cl Om m sum (x^2 + y^2): two more roundings
    g = m * cl1 * Om
    assert abs(r[1, 0]) <= g * (arm * n + (eps_order + 3 * EPS) * Ly)
    assert abs(r[1, 1]) <= g * (arm * n + (eps_order + 3 * EPS) * Lx)
    assert r[1, 2] == 0 and r[1, 3] == 0 and r[1, 4] == 0
    assert abs(r[1, 5] - (-g * Q)) <= g * (2 * arm * (Lx + Ly) + (eps_order + 5 * EPS) * Q), (r[1, 5], -g * Q)

    # above the water: zeros
    assert np.all(r[2] == 0)

    # cl = cq = 0: no force whatever the motion; field 6 is the buoyancy's Fz
    assert np.all(r[3, :6] == 0) and r[3, 6] > 0
    assert np.array_equal(_bits(raw[:, 6]), _bits(lift[:, 0]))


# 4 -- edges


def test_edges(capi, oracle, torch):
    N, cascades = 64, [1, 0]
    C = ctypes
    counts = [(7, 64, 65, 130, 1, 0, 200)[b % 7] for b in range(41)]
    bodies, probes = _fleet(5, nbodies=41, nprobes=600, counts=counts)
    motions = _motions(5, 41)
    with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
        _step(oc, 1)
        s = _set(capi, 0)
        lib = capi.load()
        arr = (capi.I * 2)(*cascades)
        P = capi.P
        nb = len(bodies)
        rec = np.zeros((nb, 8), F)
        bp, mp, pp, rp = bodies.ctypes.data_as(P), motions.ctypes.data_as(P), probes.ctypes.data_as(P), rec.ctypes.data_as(P)
        good = (arr, 2, C.byref(s), 4, bp, mp, nb, pp, 600, rp)
        names = ("datum_ocean_read_body_drag", "datum_ocean_reduce_body_drag")

        # ESTATE while velocity is off, and while no displace has run since it was switched on
        for name in names:
            assert getattr(lib, name)(oc.h, *good) == capi.ESTATE, name
            assert name.encode() in lib.datum_ocean_last_error(oc.h)
        oc.set_velocity("on")
        for name in names:
            assert getattr(lib, name)(oc.h, *good) == capi.ESTATE, name
            assert name.encode() in lib.datum_ocean_last_error(oc.h)
        _step(oc, 1)

        before = [oc.read_maps(c).copy() for c in (0, 1)], [oc.read_foam(c).copy() for c in (0, 1)], [oc.read_velocity(c).copy() for c in (0, 1)]
        clean = oc.read_body_drag(cascades, s, bodies, motions, probes, 4)
        assert np.isfinite(clean).all() and np.abs(clean[:, :3]).max() > 0
        assert np.array_equal(_bits(clean), _bits(oc.read_body_drag(cascades, s, bodies, motions, probes, 4)))         # the same on a second call

        # bad bodies and bad motions: NaN records, the others as without them
        bad, mb = bodies.copy(), motions.copy()
        pb = probes.copy()
        bad["first"][3], bad["count"][10] = -1, -2
        bad["first"][11], bad["count"][11] = 600 - 63, 64
        bad["first"][12], bad["count"][12] = 2 ** 31 - 1, 2 ** 31 - 1
        bad["cap"][17] = np.nan
        bad["position"][20, 0] = np.inf
        bad["rotation"][24, 8] = np.nan
        fields = [("linear", 0), ("linear", 1), ("linear", 2), ("angular", 0), ("angular", 1), ("angular", 2), ("cl", None), ("cq", None)]
        values = [np.nan, np.inf, -np.inf, np.nan, -np.inf, np.inf, np.nan, np.inf]
        spoiled = list(range(26, 34))                         # one motion field each; bodies 26 and 33 have no probes and are NaN all the same
        for b, ((name, k), val) in zip(spoiled, zip(fields, values)):
            if k is None:
                mb[name][b] = val
            else:
                mb[name][b, k] = val
        victims = [3, 10, 11, 12, 17, 20, 24]
        counted = [b for b in (20, 24) if bad["count"][b] > 0]
        r = oc.read_body_drag(cascades, s, bad, mb, pb, 4)
        nanrows = [b for b in victims if b not in (20, 24) or b in counted] + spoiled
        assert np.isnan(r[nanrows]).all()
        keep = np.setdiff1d(np.arange(nb), victims + spoiled)
        assert np.array_equal(_bits(r[keep]), _bits(clean[keep]))
        # a bad probe spoils exactly the bodies whose range holds it
        pb[300, 3] = np.nan
        pb[301, 1] = -np.inf
        r = oc.read_body_drag(cascades, s, bodies, motions, pb, 4)
        f, c = bodies["first"].astype(int), bodies["count"].astype(int)
        hit = ((f <= 300) & (300 < f + c)) | ((f <= 301) & (301 < f + c))
        assert hit.any() and not hit.all()
        assert np.isnan(r[hit]).all()
        assert np.array_equal(_bits(r[~hit]), _bits(clean[~hit]))

        # device arrays: the same bits, a guard tail behind the records left alone
        db = torch.from_numpy(bodies.view(np.uint8).reshape(nb, 64).copy()).cuda()
        dm = torch.from_numpy(motions.view(np.uint8).reshape(nb, 32).copy()).cuda()
        dp = torch.from_numpy(probes).cuda()
        out = torch.full((nb * 8 + 64,), -3.0e38, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        oc.reduce_body_drag(cascades, s, db.data_ptr(), dm.data_ptr(), nb, dp.data_ptr(), len(probes), out.data_ptr(), 4)
        oc.sync()
        raw = out.cpu().numpy()
        assert np.array_equal(_bits(raw[: nb * 8].reshape(nb, 8)), _bits(clean))
        assert np.all(raw[nb * 8:] == F(-3.0e38))

        # nbodies == 0
        assert oc.read_body_drag(cascades, s, bodies[:0], motions[:0], probes, 4).shape == (0, 8)
        assert lib.datum_ocean_reduce_body_drag(oc.h, arr, 2, C.byref(s), 4, None, None, 0, None, 0, None) == capi.OK
        # no probes at all: bodies of count 0 give zeros
        empty = body64.make_bodies([np.eye(3)] * 2, np.zeros((2, 3)), [0, 0], [0, 0], [1.0, np.inf])
        assert np.all(_bits(oc.read_body_drag(cascades, s, empty, motions[:2], probes[:0], 4)) == 0)

        # argument errors with a live handle: test_gpu_body's list with the motions beside the bodies, then the motions pointer itself
        calls = [
            (None, 2, C.byref(s), 4, bp, mp, nb, pp, 600, rp), (arr, 0, C.byref(s), 4, bp, mp, nb, pp, 600, rp), (arr, 17, C.byref(s), 4, bp, mp, nb, pp, 600, rp),
            ((capi.I * 2)(0, 2), 2, C.byref(s), 4, bp, mp, nb, pp, 600, rp), (arr, 2, None, 4, bp, mp, nb, pp, 600, rp),
            (arr, 2, C.byref(s), -1, bp, mp, nb, pp, 600, rp), (arr, 2, C.byref(s), 17, bp, mp, nb, pp, 600, rp),
            (arr, 2, C.byref(s), 4, None, mp, nb, pp, 600, rp), (arr, 2, C.byref(s), 4, bp, mp, nb, None, 600, rp), (arr, 2, C.byref(s), 4, bp, mp, nb, pp, 600, None),
            (arr, 2, C.byref(s), 4, P(bodies.ctypes.data + 4), mp, nb - 1, pp, 600, rp), (arr, 2, C.byref(s), 4, bp, mp, nb, P(probes.ctypes.data + 8), 599, rp),
            (arr, 2, C.byref(s), 4, bp, mp, nb, pp, 600, P(rec.ctypes.data + 4)),
            (arr, 2, C.byref(s), 4, bp, mp, 1 << 31, pp, 600, rp), (arr, 2, C.byref(s), 4, bp, mp, nb, pp, 1 << 31, rp),
            (arr, 2, C.byref(s), 4, bp, None, nb, pp, 600, rp), (arr, 2, C.byref(s), 4, bp, P(motions.ctypes.data + 4), nb - 1, pp, 600, rp),
            (arr, 2, C.byref(s), 4, bp, P(motions.ctypes.data + 8), nb - 1, pp, 600, rp),
        ]
        assert bodies.ctypes.data % 16 == 0 and probes.ctypes.data % 16 == 0 and rec.ctypes.data % 16 == 0 and motions.ctypes.data % 16 == 0
        for args in calls:
            for name in names:
                assert getattr(lib, name)(oc.h, *args) == capi.EINVAL, (name, args[1:4], args[6], args[8])
                assert name.encode() in lib.datum_ocean_last_error(oc.h)

        # the calls left the maps, the foam planes and the velocity planes as they were
        for c in (0, 1):
            assert np.array_equal(_bits(before[0][c]), _bits(oc.read_maps(c)))
            assert np.array_equal(_bits(before[1][c]), _bits(oc.read_foam(c)))
            assert np.array_equal(_bits(before[2][c]), _bits(oc.read_velocity(c)))


# 5 -- a bound velocity plane


def test_bound_velocity_plane_gives_the_same_bits(capi, oracle, torch):
    N, cascades = 64, [1, 0]
    bodies, probes = _fleet(9, nbodies=50, nprobes=400, counts=[(5, 64, 129)[b % 3] for b in range(50)])
    motions = _motions(9, 50)
    own = _moving(capi, oracle, N, 2, foam=None)
    bound = _setup(capi, oracle, N, 2)
    P = 2 * N * N * 4
    plane = torch.zeros(P, dtype=torch.float32, device="cuda")
    with own, bound:
        bound.bind_velocity(plane.data_ptr(), P * 4)
        bound.set_velocity("on")
        for oc in (own, bound):
            _step(oc)
        s = _set(capi, 0)
        a, b = own.read_body_drag(cascades, s, bodies, motions, probes, 4), bound.read_body_drag(cascades, s, bodies, motions, probes, 4)
        assert np.isfinite(a).all() and np.abs(a[:, :3]).max() > 0
        assert np.array_equal(_bits(a), _bits(b))
        mine = plane.cpu().numpy().reshape(2, N, N, 4)
        assert np.abs(mine).max() > 0
        for c in (0, 1):
            assert np.array_equal(_bits(mine[c]), _bits(own.read_velocity(c)))
        bound.bind_velocity(None, 0)


# 6 -- the C++ shim


def test_cpp_shim_matches_capi(capi):
    from datum_amd import host_api

    N = 256
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.4))
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    bodies, probes = _fleet(13, nbodies=77, nprobes=500, counts=[(0, 1, 64, 65, 200)[b % 5] for b in range(77)])
    motions = _motions(13, 77)
    with host_api.OceanContext(N) as ctx:
        with pytest.raises(Exception):
            ctx.reduce_ocean_body_drag(params, bodies, motions, probes, 4)
        ctx.set_velocity("on")
        for _ in range(2):
            params.update_ocean(DT)
            ctx.displace_ocean_surface(params)
        lib = capi.load()
        h = ctx.lib.datum_host_context_handle(ctx.c)
        one = (capi.I * 1)(0)
        for it in (0, 4):
            got = ctx.reduce_ocean_body_drag(params, bodies, motions, probes, it)
            s = params.oceanset(camera)
            want = np.empty_like(got)
            P = capi.P
            assert lib.datum_ocean_read_body_drag(h, one, 1, ctypes.byref(s), it, bodies.ctypes.data_as(P), motions.ctypes.data_as(P), len(bodies),
                                                  probes.ctypes.data_as(P), len(probes), want.ctypes.data_as(P)) == capi.OK
            assert np.array_equal(_bits(got), _bits(want)), it
            assert np.isfinite(got).all() and np.abs(got[:, :3]).max() > 0
