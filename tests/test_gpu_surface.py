"""Surface queries (include/datum_ocean_hip.h: datum_ocean_sample_surface) on the MI355X, against the float64 restatement of
tests/surface64.py, against ocean.gen's mesh, and through every configuration of the handle.

Bars, with eps = 2^-24, per point q and per record field, on the device's own maps (read_maps) as surface64's input:
  position, height, residual   |Δ| <= K_POS * eps * S,  S = (1 + |q|) (1 + N scale max|D|)   -- the texture coordinate's rounding
                               (|q| N scale texels) times the map's slope, and |q| itself
  normal                       |Δ| <= K_NRM * eps * (1 + |q| N scale)
  foam                         |Δ| <= K_FOAM * eps * (1 + |q| N scale) * max|foam|
The fixed-point iteration carries the rounding of one evaluation into the next (where the surface nearly folds, with a factor near 1),
so the bars hold for the iteration counts tested.  Each test reports the measured worst value next to its bar (tests/conftest.py: report).
"""

import ctypes

import numpy as np
import pytest

import foam64
import surface64

pytestmark = pytest.mark.gpu

DT = np.float32(1.0 / 60.0)
EPS = 2.0 ** -24

# at least 3x the worst value measured on the MI355X (the measured worst beside each)
K_POS = 6.0        # position / height / residual against surface64: measured 1.95 (64^2, swell, 16 iterations)
K_NRM = 1.0        # unit normal: measured 0.33 (64^2, swell, 16 iterations)
K_FOAM = 1.5       # foam sample: measured 0.39 (256^2, bound maps and foam plane)
K_GEN = 1.5e-4     # |height - vertex z| and the residual, in metres, for a mesh of choppiness 0.6, 8 iterations: measured 1.3e-5 / 4.3e-5


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


def _h0(oracle, N, rngseed, wavescale):
    p = oracle.EXAMPLE
    _, h0 = oracle.seed(N, rngseed, wavescale, p["waveamplitude"], p["windspeed"], p["winddirection"], sanitize=True)
    return h0


def _phase(N, rngseed):
    return np.random.RandomState(rngseed).uniform(0, 2 * np.pi, (N, N)).astype(np.float32)


SCALES = [22.0, 64.0, 9.5, 140.0]
CHOPS = [1.35, 2.2, 0.8, 1.0]


def _setup(capi, oracle, N, C, fmt="fp32", foam=None, policy=None):
    oc = capi.Ocean(N, C)
    if fmt == "literal":
        oc.set_literal_transform(True)
    elif fmt != "fp32":
        oc.set_spectrum_format(fmt)
    if policy:
        oc.set_map_store_policy(policy)
    for c in range(C):
        oc.set_cascade(c, SCALES[c % 4], CHOPS[c % 4])
        oc.upload_state(c, _h0(oracle, N, 1000 + c, SCALES[c % 4]), _phase(N, 77 + c))
    if foam:
        oc.set_foam(foam)
    return oc


def _set(capi, cascade, swell=True, plane_w=-0.3, phase=1.1):
    s = capi.OceanSet()
    s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, (0.8 if swell else 0.0), (0.5 if swell else 0.0), phase
    s.swelldirection[:] = (0.780869, 0.624695)
    s.scale = np.float32(1.0) / np.float32(SCALES[cascade % 4])
    s.plane[:] = (0.0, 0.0, 1.0, plane_w)
    return s


def _points(M, R, seed):
    return np.random.RandomState(seed).uniform(-R, R, (M, 2)).astype(np.float32)


def _errors(got, want, q, maps, N, scale, foam=None):
    """worst (position, normal, foam) error in units of their bars' eps * scale terms"""
    qa = np.abs(q.astype(np.float64)).max(1)
    dmax = float(np.abs(maps[0, ..., :3]).max())
    tex = 1.0 + qa * N * scale
    S = (1.0 + qa) * (1.0 + N * scale * dmax)
    d = np.abs(got.astype(np.float64) - want)
    kp = float((d[:, :4].max(1) / (EPS * S)).max())
    kn = float((d[:, 4:7].max(1) / (EPS * tex)).max())
    fmax = float(np.abs(foam).max()) if foam is not None else 0.0
    kf = float((d[:, 7] / (EPS * tex * max(fmax, 1e-30))).max()) if foam is not None else float(d[:, 7].max())
    return kp, kn, kf


def _check(report, tag, got, want, q, maps, N, scale, foam=None):
    kp, kn, kf = _errors(got, want, q, maps, N, scale, foam)
    report(f"surface {tag}: K_POS {kp:.2f} (bar {K_POS}), K_NRM {kn:.2f} (bar {K_NRM}), K_FOAM {kf:.2f} (bar {K_FOAM})")
    assert np.isfinite(got).all(), tag
    assert kp <= K_POS, (tag, kp)
    assert kn <= K_NRM, (tag, kn)
    if foam is not None:
        assert kf <= K_FOAM, (tag, kf)
    else:
        assert np.all(got[:, 7] == 0), tag


# 1 -- a flat ocean without swell: every record exact


def test_flat_ocean_is_exact(capi):
    N = 256
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, 22.0, 1.35)
        oc.upload_state(0, np.zeros((N, N, 2), np.float32))
        oc.update(DT)
        oc.displace()
        m = oc.read_maps(0)
        assert np.all(m[0] == 0) and np.all(m[1][..., :2] == 0)
        q = np.concatenate([_points(5000, 1e6, 1), _points(5000, 100, 2), -np.abs(_points(100, 3e5, 3)),
                            np.array([[0, 0], [-1e6, -1e6], [1e6, -1e6], [-0.5, 1e-30]], np.float32)])
        s = _set(capi, 0, swell=False, plane_w=-2.5)
        for it in (0, 1, 4, 16):
            r = oc.read_surface(0, s, q, it)
            assert np.array_equal(r[:, :2], q), it
            assert np.all(r[:, 2] == np.float32(2.5)) and np.all(r[:, 3] == 0) and np.all(r[:, 4:6] == 0) and np.all(r[:, 7] == 0), it
            if np.all(m[1][..., 2] == 1):
                assert np.all(r[:, 6] == 1), it
            else:                                    # the map's own normal rounds (tests/test_gpu_parity.py: test_flat_ocean)
                assert np.all(np.abs(r[:, 6] - 1) <= 2 ** -22), it


# 2 -- against surface64 on random displaced states


CASES = [(N, 1, 0) for N in (64, 256, 1024, 2048, 4096)] + [(1024, 4, 2)]


@pytest.mark.parametrize("N,C,cascade", CASES)
def test_against_surface64(capi, oracle, report, N, C, cascade):
    with _setup(capi, oracle, N, C) as oc:
        oc.update(DT)
        oc.displace()
        maps = oc.read_maps(cascade)
        q = _points(4000, 300.0, N + cascade)
        for swell in (True, False):
            s = _set(capi, cascade, swell)
            for it in (0, 1, 4, 16):
                got = oc.read_surface(cascade, s, q, it)
                want = surface64.surface64(maps, None, s, q, it)
                _check(report, f"N={N} C={C} c={cascade} swell={swell} it={it}", got, want, q, maps, N, float(s.scale))


# 3 -- agreement with ocean.gen's mesh


def test_agrees_with_gen_mesh(capi, oracle, report, torch):
    N, W = 256, 96
    ws, chop = 22.0, 0.6
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, ws, chop)
        oc.upload_state(0, _h0(oracle, N, 1000, ws), _phase(N, 5))
        oc.update(DT)
        oc.displace()
        maps = oc.read_maps(0)
        J = foam64.jacobian64(maps, np.float32(ws), N)
        assert J.min() > 0.3, J.min()                            # a height field everywhere: the query has one answer
        s0 = oracle.oceanset(N, position=(3, -2, 6), target=(3 + 0.8660254, -2, 6 - 0.5),
                             params=dict(wavescale=ws, choppiness=chop, swellsteepness=0.3), swellphase=0.7)
        s = capi.OceanSet.from_buffer_copy(bytes(s0))
        verts = torch.zeros(W * W * 12, dtype=torch.float32, device="cuda")
        oc.gen(0, s, W, W, verts.data_ptr())
        oc.sync()
        v = verts.cpu().numpy().reshape(-1, 12)
        near = np.hypot(v[:, 0] - 3, v[:, 1] + 2) < 200.0                # beyond, a vertex's texel spacing dwarfs the map
        q = np.ascontiguousarray(v[near, :2])
        r = oc.read_surface(0, s, q, 8)
        dz = float(np.abs(r[:, 2] - v[near, 2]).max())
        res = float(r[:, 3].max())
        report(f"surface vs gen (N={N}, {len(q)} vertices, 8 iterations): max |height - z| {dz:.3e} m, max residual {res:.3e} m (bar {K_GEN})")
        assert len(q) > 1000
        assert dz <= K_GEN and res <= K_GEN, (dz, res)


# 4 -- foam


@pytest.mark.parametrize("mode", ["jacobian", "accumulate"])
def test_foam_field(capi, oracle, report, mode):
    N = 512
    with _setup(capi, oracle, N, 1, foam=mode) as oc:
        for _ in range(3):
            oc.update(DT)
            oc.displace()
        maps, fp = oc.read_maps(0), oc.read_foam(0)
        q = _points(4000, 200.0, 8)
        s = _set(capi, 0)
        for it in (0, 4):
            got = oc.read_surface(0, s, q, it)
            want = surface64.surface64(maps, fp, s, q, it)
            _check(report, f"foam {mode} it={it}", got, want, q, maps, N, float(s.scale), foam=fp)
        oc.set_foam("off")
        assert np.all(oc.read_surface(0, s, q, 4)[:, 7] == 0)


# 5 -- configurations


@pytest.mark.parametrize("N,fmt,policy", [(256, "fp16", None), (1024, "fp16h0", None), (256, "literal", None), (1024, "fp32", "streamed"),
                                          (2048, "fp32", "streamed")])
def test_configurations(capi, oracle, report, N, fmt, policy):
    with _setup(capi, oracle, N, 1, fmt, policy=policy) as oc:
        oc.update(DT)
        oc.displace()
        maps = oc.read_maps(0)
        q = _points(3000, 250.0, 21)
        s = _set(capi, 0)
        got = oc.read_surface(0, s, q, 4)
        _check(report, f"N={N} {fmt} {policy or ''}", got, surface64.surface64(maps, None, s, q, 4), q, maps, N, float(s.scale))


@pytest.mark.parametrize("N", [256, 4096])
def test_bound_maps_give_the_same_bits(capi, oracle, report, torch, N):
    own = _setup(capi, oracle, N, 1, foam="jacobian")
    bound = _setup(capi, oracle, N, 1)
    nbytes = own.maps_device()[1]
    buf = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    foambuf = torch.zeros(N * N, dtype=torch.float32, device="cuda")
    with own, bound:
        bound.bind_maps(buf.data_ptr(), nbytes)
        bound.bind_foam(foambuf.data_ptr(), N * N * 4)
        bound.set_foam("jacobian")
        for oc in (own, bound):
            oc.update(DT)
            oc.displace()
        q = _points(5000, 400.0, 31)
        s = _set(capi, 0)
        a, b = own.read_surface(0, s, q, 4), bound.read_surface(0, s, q, 4)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        maps = bound.read_maps(0)
        _check(report, f"N={N} bound maps", b, surface64.surface64(maps, bound.read_foam(0), s, q, 4), q, maps, N, float(s.scale), foam=bound.read_foam(0))


# 6 -- stream order


def test_stream_order(capi, oracle, report, torch):
    N, M = 1024, 1 << 16
    q = _points(M, 300.0, 41)
    s = _set(capi, 0)
    pts = torch.from_numpy(q).cuda()
    out1 = torch.zeros(M * 8, dtype=torch.float32, device="cuda")
    out2 = torch.zeros(M * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with _setup(capi, oracle, N, 1) as oc, _setup(capi, oracle, N, 1) as twin:
        oc.update(DT)
        oc.displace()
        oc.sample_surface(0, s, pts.data_ptr(), M, out1.data_ptr(), 4)
        oc.update(DT)
        oc.displace()
        oc.sample_surface(0, s, pts.data_ptr(), M, out2.data_ptr(), 4)
        oc.sync()
        twin.update(DT)
        twin.displace()
        mapsA = twin.read_maps(0)
        twin.update(DT)
        twin.displace()
        mapsB = twin.read_maps(0)
        assert np.array_equal(mapsB, oc.read_maps(0))
        r1, r2 = out1.cpu().numpy().reshape(M, 8), out2.cpu().numpy().reshape(M, 8)
        _check(report, "stream order, first", r1, surface64.surface64(mapsA, None, s, q, 4), q, mapsA, N, float(s.scale))
        _check(report, "stream order, second", r2, surface64.surface64(mapsB, None, s, q, 4), q, mapsB, N, float(s.scale))
        assert np.array_equal(twin.read_surface(0, s, q, 4), r2)


# 7 -- edges


def test_edges(capi, oracle, torch):
    N = 512
    with _setup(capi, oracle, N, 2, foam="accumulate") as oc:
        for _ in range(2):
            oc.update(DT)
            oc.displace()
        s = _set(capi, 1)
        C = ctypes
        lib = capi.load()
        hb = oc.read_maps(1).copy(), oc.read_foam(1).copy()

        for M in (0, 1, 37, 1000 + 37, 1 << 20):
            q = _points(M, 500.0, M)
            host = oc.read_surface(1, s, q, 4)
            assert host.shape == (M, 8)
            if M == 0:
                assert lib.datum_ocean_sample_surface(oc.h, 1, C.byref(s), 4, None, 0, None) == capi.OK
                continue
            pts = torch.from_numpy(q).cuda()
            out = torch.full((M * 8,), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            oc.sample_surface(1, s, pts.data_ptr(), M, out.data_ptr(), 4)
            oc.sync()
            dev = out.cpu().numpy().reshape(M, 8)
            assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)), M

        # non-finite inputs: NaN records, neighbours as without them
        q = _points(256, 100.0, 5)
        clean = oc.read_surface(1, s, q, 4)
        bad = q.copy()
        idx = [3, 64, 65, 200]
        bad[3, 0], bad[64, 1], bad[65] = np.nan, np.inf, (-np.inf, np.nan)
        bad[200, 0] = -np.inf
        r = oc.read_surface(1, s, bad, 4)
        assert np.isnan(r[idx]).all()
        keep = np.setdiff1d(np.arange(256), idx)
        assert np.array_equal(r[keep].view(np.uint32), clean[keep].view(np.uint32))

        # argument errors with a live handle
        pts = np.zeros((4, 2), np.float32)
        out = np.zeros((4, 8), np.float32)
        P = capi.P
        for it in (-1, 17):
            assert lib.datum_ocean_read_surface(oc.h, 0, C.byref(s), it, pts.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert lib.datum_ocean_read_surface(oc.h, 2, C.byref(s), 4, pts.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert lib.datum_ocean_read_surface(oc.h, -1, C.byref(s), 4, pts.ctypes.data_as(P), 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert lib.datum_ocean_read_surface(oc.h, 0, C.byref(s), 4, P(pts.ctypes.data + 4), 2, out.ctypes.data_as(P)) == capi.EINVAL
        assert lib.datum_ocean_read_surface(oc.h, 0, C.byref(s), 4, pts.ctypes.data_as(P), 2, P(out.ctypes.data + 8)) == capi.EINVAL
        assert lib.datum_ocean_sample_surface(oc.h, 0, C.byref(s), 4, pts.ctypes.data_as(P), 1 << 31, out.ctypes.data_as(P)) == capi.EINVAL
        assert lib.datum_ocean_sample_surface(oc.h, 0, C.byref(s), 4, None, 4, out.ctypes.data_as(P)) == capi.EINVAL
        assert b"datum_ocean_sample_surface" in lib.datum_ocean_last_error(oc.h)

        # the queries left the maps and the foam plane as they were
        ha = oc.read_maps(1), oc.read_foam(1)
        assert np.array_equal(hb[0].view(np.uint32), ha[0].view(np.uint32))
        assert np.array_equal(hb[1].view(np.uint32), ha[1].view(np.uint32))


# 8 -- the C++ mirror


def test_cpp_mirror_matches_capi(capi, torch):
    from datum_amd import host_api

    N = 256
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, swellsteepness=0.4))
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    with host_api.OceanContext(N) as ctx:
        mesh = ctx.create_ocean(32, 32)
        for _ in range(2):
            params.update_ocean(DT)
            ctx.render_ocean_surface(mesh, params, camera)
        q = _points(5000, 200.0, 51)
        for it in (0, 4, 16):
            got = ctx.query_ocean_surface(params, q, it)
            s = params.oceanset(camera)
            want = np.empty_like(got)
            lib = capi.load()
            h = ctx.lib.datum_host_context_handle(ctx.c)
            assert lib.datum_ocean_read_surface(h, 0, ctypes.byref(s), it, q.ctypes.data_as(capi.P), len(q), want.ctypes.data_as(capi.P)) == capi.OK
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), it
            assert np.isfinite(got).all()
