"""Several cascades at once (include/datum_ocean_hip.h: datum_ocean_gen_blend, datum_ocean_sample_surface_blend) on the MI355X: a
one-element list against the single-cascade calls bit for bit, lists against the float64 restatement of tests/blend64.py on the device's
own maps, the mesh's sample stage against its derived bar, the store pattern, order and neutrality, foam, configurations and edges.

Bars of the queries, eps = 2^-24, per point q, the form of tests/test_gpu_surface.py's with the list's terms summed:
  position, height, residual   |Δ| <= K_POS * eps * S,   S = (1 + |q|) (1 + Σ_c N scale_c max|D_c|)
  normal                       |Δ| <= K_NRM * eps * tex, tex = 1 + |q| N max_c scale_c
  foam                         |Δ| <= K_FOAM * eps * tex * max|foam|
"""

import ctypes

import numpy as np
import pytest

import blend64
import foam64
import gen64
import gen_cases
import surface64
from test_gpu_surface import CHOPS, DT, EPS, SCALES, _h0, _phase, _points, _set, _setup

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = np.float32(-3.0e38)
GUARD = 64

# Measured on the MI355X (profiles/blend_gpu_suite.txt), each at least 3x the worst value seen against blend64, the convention of
# tests/test_gpu_surface.py; tests/test_blend64.py keeps a loose constant from hiding a wrong term (a planted mistake moves the result by
# at least 1300 of these bars).  The two large worsts belong to lists whose SUMMED surface folds, where b <- b + (q - V(b).xy) does not
# contract and carries a rounding forward by |grad D| per iteration: [1, 1] doubles the choppiness-2.2 cascade (float64 on the oracle's
# maps: max |grad D| 1.33, min J -0.27, and ONE rounding of the start alone moves the float64 result by 9.75 of the position bar after 16
# iterations), the 16-cascade list sums four choppinesses four times.  Every other list stays below 2.3 / 0.7.
K_POS = 50.0         # position / height / residual: measured 16.63 (64^2, [1, 1], swell, 16 iterations); 2.29 on the other lists
K_NRM = 36.0         # unit normal: measured 11.69 (256^2 x 16, swell, 16 iterations); 5.80 for [1, 1], 0.69 on the other lists
K_FOAM = 1.5         # foam sample: measured 0.27 (512^2 x 2, accumulate)
K_FRAME = 8 * EPS    # mesh normal and tangent against staged_blend64, absolute: measured 1.46e-7 (64^2 x 4, grazing)
K_MESH = 8.0e-5      # |height - vertex z| and the residual in metres, choppiness 0.3 x 4, 8 iterations: measured 3.8e-6 / 2.50e-5


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


def _scale(c):
    return F(1.0) / F(SCALES[c % 4])             # what the handle holds: 1 / wavescale in fp32 (datum_ocean_set_cascade)


def _step(oc, steps=1):
    for _ in range(steps):
        oc.update(DT)
        oc.displace()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _mesh(capi, torch, oc, cascades, s, sx, sy, single=None):
    """one launch into a sentinel-filled buffer with a guard tail: [sy, sx, 12] after the store pattern's checks"""
    verts = torch.full((sx * sy * 12 + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    if single is None:
        oc.gen_blend(cascades, s, sx, sy, verts.data_ptr())
    else:
        oc.gen(single, s, sx, sy, verts.data_ptr())
    oc.sync()
    raw = verts.cpu().numpy()
    sentinel = np.array([SENTINEL], F).view(np.uint32)[0]
    assert np.all(raw[sx * sy * 12:].view(np.uint32) == sentinel), "the guard tail was written"
    got = raw[: sx * sy * 12].reshape(sy, sx, 12)
    left = np.argwhere(got.view(np.uint32) == sentinel)
    assert left.size == 0, ("vertices not written", sx, sy, left[:4])
    assert np.all(got[..., 11] == -1)
    return got


def _header(capi, oracle, N, case, cascade, **over):
    s = capi.OceanSet.from_buffer_copy(bytes(gen_cases.oceanset(oracle, N, case, wavescale=SCALES[cascade % 4])))
    s.scale = _scale(cascade)
    for k, v in over.items():
        setattr(s, k, v)
    return s


# 1 -- a one-element list is the single-cascade call


@pytest.mark.parametrize("N", [64, 2048])
def test_one_element_list_is_the_single_call(capi, oracle, torch, N):
    with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
        _step(oc, 2)
        c = 1
        for case in ("example", "above_horizon", "grazing"):
            for sx, sy in ((33, 17), (200, 150)):
                s = _header(capi, oracle, N, case, c)
                want = _mesh(capi, torch, oc, None, s, sx, sy, single=c)
                s.scale = 123.0                                  # ignored: the handle's scale is used
                got = _mesh(capi, torch, oc, [c], s, sx, sy)
                assert np.array_equal(_bits(got[..., :5]), _bits(want[..., :5])), (N, case, sx, sy)
        q = _points(4000, 300.0, N)
        for swell in (True, False):
            s = _set(capi, c, swell)
            for it in (0, 4, 16):
                want = oc.read_surface(c, s, q, it)
                s2 = capi.OceanSet.from_buffer_copy(bytes(s))
                s2.scale = 0.5
                got = oc.read_surface_blend([c], s2, q, it)
                assert np.array_equal(_bits(got[:, :4]), _bits(want[:, :4])), (N, swell, it)
                assert np.array_equal(_bits(got[:, 7]), _bits(want[:, 7])), (N, swell, it)


# 2 -- against blend64 on the device's own maps


def _errors(got, want, q, maps_list, scales, N, foams=None):
    qa = np.abs(q.astype(np.float64)).max(1)
    slope = sum(N * float(sc) * float(np.abs(m[0, ..., :3]).max()) for m, sc in zip(maps_list, scales))
    tex = 1.0 + qa * N * max(float(sc) for sc in scales)
    S = (1.0 + qa) * (1.0 + slope)
    d = np.abs(got.astype(np.float64) - want)
    kp = float((d[:, :4].max(1) / (EPS * S)).max())
    kn = float((d[:, 4:7].max(1) / (EPS * tex)).max())
    if foams is None:
        return kp, kn, float(d[:, 7].max())
    fmax = max(float(np.abs(fp).max()) for fp in foams)
    return kp, kn, float((d[:, 7] / (EPS * tex * max(fmax, 1e-30))).max())


def _check(report, tag, got, want, q, maps_list, scales, N, foams=None):
    kp, kn, kf = _errors(got, want, q, maps_list, scales, N, foams)
    report(f"blend {tag}: K_POS {kp:.2f} (bar {K_POS}), K_NRM {kn:.2f} (bar {K_NRM}), K_FOAM {kf:.2f} (bar {K_FOAM})")
    assert np.isfinite(got).all(), tag
    assert kp <= K_POS, (tag, kp)
    assert kn <= K_NRM, (tag, kn)
    if foams is not None:
        assert kf <= K_FOAM, (tag, kf)
    else:
        assert np.all(got[:, 7] == 0), tag


LISTS = [(64, 4, [0, 1, 2, 3]), (64, 4, [2, 0]), (64, 4, [1, 1]), (256, 16, list(range(16))), (2048, 2, [0, 1])]


@pytest.mark.parametrize("N,C,cascades", LISTS)
def test_against_blend64(capi, oracle, report, N, C, cascades):
    with _setup(capi, oracle, N, C) as oc:
        _step(oc)
        own = {c: oc.read_maps(c) for c in sorted(set(cascades))}
        maps_list, scales = [own[c] for c in cascades], [_scale(c) for c in cascades]
        q = _points(4000, 300.0, N + len(cascades))
        for swell in (True, False):
            s = _set(capi, 0, swell)
            for it in (0, 1, 4, 16):
                got = oc.read_surface_blend(cascades, s, q, it)
                want = blend64.surface_blend64(maps_list, None, "off", scales, s, q, it)
                _check(report, f"N={N} list={cascades} swell={swell} it={it}", got, want, q, maps_list, scales, N)


# 3 -- the mesh's sample stage


@pytest.mark.parametrize("N,C", [(64, 4), (2048, 2)])
def test_mesh_sample_stage(capi, oracle, torch, report, N, C):
    sx, sy = 200, 150
    cascades = list(range(C))
    with capi.Ocean(N, C) as oc:
        for c in cascades:
            oc.set_cascade(c, SCALES[c], CHOPS[c])
            oc.upload_state(c, gen64.band_limited_h0(N, 7 + c))
        _step(oc)
        maps_list, scales = [oc.read_maps(c) for c in cascades], [_scale(c) for c in cascades]
        for case in ("pitched_steep", "above_horizon", "grazing"):
            # swellamplitude = swellsteepness = 0: position = (base.xy, basez) exactly, so vertex.xyz - position is the summed sample alone
            s = _header(capi, oracle, N, case, 0, swellsteepness=0.0, swellamplitude=0.0)
            got = _mesh(capi, torch, oc, cascades, s, sx, sy).astype(np.float64)
            ray = gen64.ray32(s, sx, sy)
            ref = blend64.staged_blend64(s, maps_list, scales, ray)
            want = ref.vertices
            assert float(np.abs(ref.displacement).max()) > 0.02
            err = np.abs(got[..., 0:3] - want[..., 0:3])
            # derived: every cascade's blend (8 roundings of values up to its largest corner texel), one rounding per addition of the
            # list's sum, the final subtraction from the position (blend_bar's 2 |want|)
            bar = sum(gen64.blend_bar(t.corner, 0.0) for t in ref.terms) + gen64.EPS * (C - 1) * np.abs(ref.displacement) + gen64.blend_bar(0.0, want[..., 0:3])
            frame = float(np.abs(got[..., 5:11] - want[..., 5:11]).max())
            report(f"blend mesh {case} N={N} x {C}: vertex.xyz error / bar {float((err / bar).max()):.3f}, frame vs float64 {frame:.2e} (bar {K_FRAME})")
            bad = np.argwhere(err > bar)
            assert bad.size == 0, (case, N, bad.shape[0], bad[:4], err[tuple(bad[0])], bar[tuple(bad[0])])
            assert frame <= K_FRAME, (case, N, frame)


# 4 -- the store pattern; 5 -- order and neutrality


def test_store_pattern_order_and_neutrality(capi, oracle, torch):
    N = 64
    with _setup(capi, oracle, N, 4) as oc:
        oc.upload_state(3, np.zeros((N, N, 2), np.float32))          # cascade 3: a flat ocean
        _step(oc)
        assert np.all(oc.read_maps(3)[0] == 0)
        s = _header(capi, oracle, N, "pitched_steep", 0)
        for sx, sy in ((2, 2), (17, 3), (31, 15)):
            _mesh(capi, torch, oc, [0, 1, 2], s, sx, sy)                # (_mesh: no sentinel left inside, none touched behind)
        ab = _mesh(capi, torch, oc, [0, 2], s, 200, 150)
        ba = _mesh(capi, torch, oc, [2, 0], s, 200, 150)
        assert np.all(ab[..., :5] == ba[..., :5])
        flat = _mesh(capi, torch, oc, [0, 2, 3], s, 200, 150)
        assert np.all(flat[..., :5] == ab[..., :5])
        q = _points(4000, 300.0, 3)
        sq = _set(capi, 0)
        for it in (0, 8):
            a, b, z = (oc.read_surface_blend(l, sq, q, it) for l in ([0, 2], [2, 0], [0, 2, 3]))
            assert np.all(a[:, :4] == b[:, :4]), it
            assert np.all(a[:, :4] == z[:, :4]), it


# 6 -- the mesh and the query describe the same surface


def _summed_jacobian64(maps_list, wavescales, scales, N, px, py):
    """float64 Jacobian of x -> x - sum_c D_c(x scale_c).xy at (px, py): every cascade's four central-difference derivatives
    (foam64.parts64) resampled as blend64 resamples the maps, summed over the list"""
    a = b = c = d = 0.0
    for maps, ws, sc in zip(maps_list, wavescales, scales):
        r = surface64.bilinear64(np.stack(foam64.parts64(maps, np.float32(ws), N)), px * float(sc), py * float(sc))
        a, b, c, d = a + r[0], b + r[1], c + r[2], d + r[3]
    return (1.0 - a) * (1.0 - d) - b * c


def test_agrees_with_blend_mesh(capi, oracle, report, torch):
    N, W, chop = 256, 96, 0.3                  # 0.3 per cascade: the summed Jacobian of these four spectra stays above 0.6 (0.6 gives 0.33)
    cascades = [0, 1, 2, 3]
    with capi.Ocean(N, 4) as oc:
        for c in cascades:
            oc.set_cascade(c, SCALES[c], chop)
            oc.upload_state(c, _h0(oracle, N, 1000 + c, SCALES[c]), _phase(N, 77 + c))
        _step(oc)
        maps_list, scales = [oc.read_maps(c) for c in cascades], [_scale(c) for c in cascades]
        s0 = oracle.oceanset(N, position=(3, -2, 6), target=(3 + 0.8660254, -2, 6 - 0.5),
                             params=dict(wavescale=SCALES[0], choppiness=chop, swellsteepness=0.3), swellphase=0.7)
        s = capi.OceanSet.from_buffer_copy(bytes(s0))
        v = _mesh(capi, torch, oc, cascades, s, W, W).reshape(-1, 12)
        near = np.hypot(v[:, 0] - 3, v[:, 1] + 2) < 200.0                # beyond, a vertex's texel spacing dwarfs the map
        q = np.ascontiguousarray(v[near, :2])
        assert len(q) > 1000

        # the precondition: a height field everywhere probed, at the float64 base points' P(b) and at the vertices themselves
        qq = q.astype(np.float64).T
        b = qq.copy()
        for _ in range(8):
            b = b + (qq - blend64.evaluate_blend64(maps_list, scales, s, b)[0][:2])
        _, _, (px, py) = blend64.evaluate_blend64(maps_list, scales, s, b)
        J = min(float(_summed_jacobian64(maps_list, SCALES, scales, N, x, y).min()) for x, y in ((px, py), (qq[0], qq[1])))
        assert J > 0.3, J

        r = oc.read_surface_blend(cascades, s, q, 8)
        dz = float(np.abs(r[:, 2] - v[near, 2]).max())
        res = float(r[:, 3].max())
        report(f"blend surface vs mesh (N={N} x 4, {len(q)} vertices, 8 iterations, summed J >= {J:.2f}): max |height - z| {dz:.3e} m, max residual {res:.3e} m (bar {K_MESH})")
        assert dz <= K_MESH and res <= K_MESH, (dz, res)


# 7 -- foam


@pytest.mark.parametrize("mode", ["jacobian", "accumulate"])
def test_foam(capi, oracle, report, mode):
    N, cascades = 512, [0, 1]
    with _setup(capi, oracle, N, 2, foam=mode) as oc:
        _step(oc, 3)
        maps_list, foams, scales = [oc.read_maps(c) for c in cascades], [oc.read_foam(c) for c in cascades], [_scale(c) for c in cascades]
        q = _points(4000, 200.0, 8)
        s = _set(capi, 0)
        for it in (0, 4):
            got = oc.read_surface_blend(cascades, s, q, it)
            want = blend64.surface_blend64(maps_list, foams, mode, scales, s, q, it)
            _check(report, f"foam {mode} it={it}", got, want, q, maps_list, scales, N, foams=foams)
        oc.set_foam("off")
        assert np.all(oc.read_surface_blend(cascades, s, q, 4)[:, 7] == 0)


# 8 -- configurations and edges


def test_bound_maps_and_foam_give_the_same_bits(capi, oracle, torch):
    N, cascades = 256, [1, 0]
    own = _setup(capi, oracle, N, 2, foam="jacobian")
    bound = _setup(capi, oracle, N, 2)
    nbytes = own.maps_device()[1]
    buf = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    foambuf = torch.zeros(2 * N * N, dtype=torch.float32, device="cuda")
    with own, bound:
        bound.bind_maps(buf.data_ptr(), nbytes)
        bound.bind_foam(foambuf.data_ptr(), 2 * N * N * 4)
        bound.set_foam("jacobian")
        for oc in (own, bound):
            _step(oc)
        q = _points(5000, 400.0, 31)
        s = _set(capi, 0)
        a, b = own.read_surface_blend(cascades, s, q, 4), bound.read_surface_blend(cascades, s, q, 4)
        assert np.array_equal(_bits(a), _bits(b))
        sm = _header(capi, oracle, N, "pitched_steep", 0)
        assert np.array_equal(_bits(_mesh(capi, torch, own, cascades, sm, 33, 17)), _bits(_mesh(capi, torch, bound, cascades, sm, 33, 17)))


def test_fp16_format(capi, oracle, report):
    N, cascades = 256, [0, 1]
    with _setup(capi, oracle, N, 2, "fp16") as oc:
        _step(oc)
        maps_list, scales = [oc.read_maps(c) for c in cascades], [_scale(c) for c in cascades]
        q = _points(3000, 250.0, 21)
        s = _set(capi, 0)
        got = oc.read_surface_blend(cascades, s, q, 4)
        _check(report, f"N={N} fp16", got, blend64.surface_blend64(maps_list, None, "off", scales, s, q, 4), q, maps_list, scales, N)


def test_edges(capi, oracle, torch):
    N, cascades = 512, [1, 0]
    with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
        _step(oc, 2)
        s = _set(capi, 0)
        C = ctypes
        lib = capi.load()
        before = [oc.read_maps(c).copy() for c in (0, 1)], [oc.read_foam(c).copy() for c in (0, 1)]
        arr = (capi.I * 2)(*cascades)

        for M in (0, 1, 1037):
            q = _points(M, 500.0, M)
            host = oc.read_surface_blend(cascades, s, q, 4)
            assert host.shape == (M, 8)
            if M == 0:
                assert lib.datum_ocean_sample_surface_blend(oc.h, arr, 2, C.byref(s), 4, None, 0, None) == capi.OK
                continue
            pts = torch.from_numpy(q).cuda()
            out = torch.full((M * 8,), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            oc.sample_surface_blend(cascades, s, pts.data_ptr(), M, out.data_ptr(), 4)
            oc.sync()
            assert np.array_equal(_bits(host), _bits(out.cpu().numpy().reshape(M, 8))), M

        # non-finite inputs: NaN records, neighbours as without them
        q = _points(256, 100.0, 5)
        clean = oc.read_surface_blend(cascades, s, q, 4)
        bad = q.copy()
        idx = [3, 64, 65, 200]
        bad[3, 0], bad[64, 1], bad[65] = np.nan, np.inf, (-np.inf, np.nan)
        bad[200, 0] = -np.inf
        r = oc.read_surface_blend(cascades, s, bad, 4)
        assert np.isnan(r[idx]).all()
        keep = np.setdiff1d(np.arange(256), idx)
        assert np.array_equal(_bits(r[keep]), _bits(clean[keep]))

        # argument errors with a live handle
        pts = np.zeros((4, 2), np.float32)
        out = np.zeros((4, 8), np.float32)
        P = capi.P
        verts = torch.zeros(4 * 4 * 12, dtype=torch.float32, device="cuda")
        lists = [(None, 2), (arr, 0), (arr, 17), (arr, -1), ((capi.I * 2)(0, 2), 2), ((capi.I * 2)(-1, 0), 2)]
        for lst, n in lists:
            assert lib.datum_ocean_read_surface_blend(oc.h, lst, n, C.byref(s), 4, pts.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
            assert b"datum_ocean_read_surface_blend" in lib.datum_ocean_last_error(oc.h)
            assert lib.datum_ocean_sample_surface_blend(oc.h, lst, n, C.byref(s), 4, pts.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
            assert b"datum_ocean_sample_surface_blend" in lib.datum_ocean_last_error(oc.h)
            assert lib.datum_ocean_gen_blend(oc.h, lst, n, C.byref(s), 4, 4, P(verts.data_ptr())) == capi.EINVAL
            assert b"datum_ocean_gen_blend" in lib.datum_ocean_last_error(oc.h)
        for it in (-1, 17):
            assert lib.datum_ocean_read_surface_blend(oc.h, arr, 2, C.byref(s), it, pts.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert lib.datum_ocean_read_surface_blend(oc.h, arr, 2, C.byref(s), 4, P(pts.ctypes.data + 4), 2, out.ctypes.data_as(P)) == capi.EINVAL
        assert lib.datum_ocean_sample_surface_blend(oc.h, arr, 2, C.byref(s), 4, None, 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert lib.datum_ocean_gen_blend(oc.h, arr, 2, C.byref(s), 1, 4, P(verts.data_ptr())) == capi.EINVAL
        assert lib.datum_ocean_gen_blend(oc.h, arr, 2, C.byref(s), 4, 4, P(verts.data_ptr() + 4)) == capi.EINVAL
        assert lib.datum_ocean_gen_blend(oc.h, arr, 2, None, 4, 4, P(verts.data_ptr())) == capi.EINVAL

        # the calls left the maps and the foam planes as they were
        for c in (0, 1):
            assert np.array_equal(_bits(before[0][c]), _bits(oc.read_maps(c)))
            assert np.array_equal(_bits(before[1][c]), _bits(oc.read_foam(c)))
