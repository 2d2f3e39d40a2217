"""GPU tests of the rippled reads (include/datum_ocean_hip.h: datum_ocean_gen_blend_rippled, datum_ocean_sample_surface_blend_rippled,
datum_ocean_cast_rays_rippled and the host twins) against tests/rippled64.py.  What the header states bit for bit is asserted bit for bit
from calls that their own tests pin (read_surface_blend, gen_blend, query_ripples): the lifted height, the untouched fields, the mesh's
x, y, z, u, v and the cast over read_surface_blend_rippled.  The normals are compared with the float64 form under the bar rippled64 derives.
N = 64 x 3 cascades is the PLAIN map layout, 2048^2 x 2 the BANDED one; R = 64 and 128 with the origin (37, -21) wrap the window round the
torus in memory; a second origin follows a center_ripples.
"""

import numpy as np
import pytest

import blend64
import ray64
import rippled64
from test_gpu_blend import K_NRM, SENTINEL, GUARD, _header, _mesh
from test_gpu_body import _scale, _step
from test_gpu_couple import _prime
from test_gpu_rays import _flat, _rays
from test_gpu_ripples import ORIGIN, _impulses
from test_gpu_surface import EPS, _set, _setup

pytestmark = pytest.mark.gpu

F = np.float32
FOLD = 1e-3                   # a folded point: the un-rippled residual in metres after the solve


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


def _points(R, cell, seed, origin=ORIGIN, n=1500):
    """inside the window, round its seam in memory, across its edge, outside, and three that are not finite"""
    rng = np.random.RandomState(seed)
    lo = np.array(origin) * cell
    inside = lo + rng.uniform(0, 1, (n, 2)) * R * cell
    seam = np.array([-(-origin[0] // R) * R, -(-origin[1] // R) * R]) * cell + rng.uniform(-1.5, 1.5, (200, 2)) * cell
    half = np.stack([lo[0] + rng.uniform(-1.5, 1.5, 200) * cell, lo[1] + rng.uniform(0, 1, 200) * R * cell], 1)
    out = lo - rng.uniform(2, 60, (200, 2))
    bad = np.array([[np.nan, 1.0], [1.0, np.inf], [-np.inf, np.nan]])
    return np.concatenate([inside, seam, half, out, bad]).astype(F)


def _same_record_bits(got, plain, smp, tag):
    nan = np.isnan(plain[:, 0])
    assert nan[-3:].all() and not nan[:-3].any() and np.isnan(got[nan]).all() and np.isfinite(got[~nan]).all(), tag
    g, p = got[~nan], plain[~nan]
    assert np.array_equal(_bits(g[:, 2]), _bits(p[:, 2] + smp[~nan, 0])), (tag, "height")
    for k in (0, 1, 3, 7):
        assert np.array_equal(_bits(g[:, k]), _bits(p[:, k])), (tag, k)


# 1 -- the query: bits of what is stated bit for bit, the normals under their bar


@pytest.mark.parametrize("N,C,lists,R,cell,foam", [(64, 3, ([1], [0, 1, 2]), 64, 1.0, "accumulate"), (2048, 2, ([1], [0, 1]), 128, 0.5, "jacobian"), (64, 4, ([2], [2, 3]), 128, 0.5, None)])
def test_query(capi, oracle, report, N, C, lists, R, cell, foam):
    worst = tight = 0.0
    with _setup(capi, oracle, N, C, foam=foam) as oc:
        _step(oc)
        lay = _prime(oc, R, cell)
        for origin in (ORIGIN, None):
            if origin is None:
                x, y = (ORIGIN[0] + R // 2 + 9.5) * cell, (ORIGIN[1] + R // 2 - 6.5) * cell
                oc.center_ripples(x, y)
                lay.center(x, y)
                origin = (lay.ox, lay.oy)
                assert origin != ORIGIN and oc.ripples_device()[2:] == origin
            q = _points(R, cell, N + R, origin)
            smp = oc.query_ripples(q)
            assert np.array_equal(_bits(smp[:-3]), _bits(lay.sample(q)[:-3])) and np.abs(smp[:-3, 0]).max() > 1e-3
            for cascades in lists:
                for swell in (True, False):
                    s = _set(capi, 0, swell)
                    for it in (0, 4):
                        tag = (N, R, origin, cascades, swell, it)
                        plain = oc.read_surface_blend(cascades, s, q, it)
                        got = oc.read_surface_blend_rippled(cascades, s, q, it)
                        _same_record_bits(got, plain, smp, tag)
                        assert np.array_equal(_bits(oc.read_surface_blend(cascades, s, q, it)), _bits(plain)), tag
                        # the layer is in the normal where it has a slope, and only there
                        moved = (got[:-3, 4:7] != plain[:-3, 4:7]).any(1)
                        sloped = (smp[:-3, 1:3] != 0).any(1)
                        assert not moved[~sloped].any() and moved[sloped].mean() > 0.5, tag
                        if not swell:
                            # the tight bar: without swell the frame is constant, and the rippled normal follows from the parent's own
                            # normal and the layer's sample (rippled64.relift64); no point is left out
                            want, pp = rippled64.relift64(plain[:-3, 4:7], smp[:-3])
                            tight = max(tight, float((np.abs(got[:-3, 4:7] - want).max(1) / (EPS * (1 + pp))).max()))
                            assert tight <= rippled64.K_RIPN, (tag, tight)
                        if N == 64 and it == 4 and set(cascades) <= {2, 3}:          # choppiness <= 1: the summed surface does not fold
                            maps = [oc.read_maps(c) for c in cascades]
                            scales = [_scale(c) for c in cascades]
                            # (16 iterations: a point that is not folded has converged, so the residual tells the two apart)
                            plain, got = oc.read_surface_blend(cascades, s, q, 16), oc.read_surface_blend_rippled(cascades, s, q, 16)
                            want = rippled64.record64(maps, None, "off", scales, s, lay, q[:-3], 16)
                            keep = plain[:-3, 3] <= FOLD
                            assert (~keep).mean() <= 0.05, (tag, (~keep).mean())
                            tex = 1.0 + np.abs(q[:-3].astype(np.float64)).max(1) * N * max(float(x) for x in scales)
                            ratio = np.abs(got[:-3, 4:7] - want[:, 4:7]).max(1) / (EPS * (K_NRM * tex + rippled64.K_RIPN))
                            worst = max(worst, float(ratio[keep].max()))
                            assert ratio[keep].max() <= 1.0, (tag, float(ratio[keep].max()))
        # nothing of the layer was written
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))
    report(f"rippled query normals N={N} R={R}: against the parent's own normal re-lifted, worst {tight:.2f} eps (1 + |p'|^2) (bar K_RIPN = {rippled64.K_RIPN}); "
           f"against float64, worst share of K_NRM eps tex + K_RIPN eps: {worst:.3f}")


# 2 -- known answer over the flat ocean; the layer at rest gives the parents' values; a ripple alone is hit


def test_flat_ocean_known_answers(capi, torch):
    R, cell, z0 = 64, 1.0, 0.25
    with _flat(capi) as oc:
        s = _set(capi, 0, swell=False, plane_w=-z0)
        lay = _prime(oc, R, cell)
        q = _points(R, cell, 3)[:-3]
        smp = oc.query_ripples(q)
        got = oc.read_surface_blend_rippled([0], s, q, 4)
        assert np.array_equal(_bits(got[:, 2]), _bits(F(z0) + smp[:, 0]))
        want = rippled64.flat_normal64(smp)
        assert np.abs(got[:, 4:7] - want).max() <= 4 * EPS, np.abs(got[:, 4:7] - want).max()
        assert np.abs(want[:, :2]).max() > 1e-3

        # a ray that passes 5 cm above the level sea misses it and enters the highest ripple; one that dips under the sea well outside
        # the window hits the FFT surface where there is no layer
        e = lay.window()[..., 0]
        j, i = np.unravel_index(np.argmax(e), e.shape)
        top = float(e[j, i])
        cx, cy = (lay.ox + i + 0.5) * cell, (lay.oy + j + 0.5) * cell
        assert top > 0.01
        zr = z0 + 0.5 * top
        far = (lay.ox - 500) * cell
        rays = np.array([[cx - 0.75 * cell, cy, zr, 0.0, 1.0, 0.0, 0.0, 0.75 * cell],
                         [far, cy, z0 + 1.0, 0.0, 0.0, 0.0, -1.0, 2.0]], F)
        hit = oc.read_rays_rippled([0], s, rays, 4, 32, 12)
        miss = oc.read_rays([0], s, rays, 4, 32, 12)
        assert miss[0, 3] == ray64.MISS and hit[0, 3] != ray64.MISS and abs(hit[0, 6] - zr) < 1e-2
        assert hit[1, 3] == ray64.ENTER and np.array_equal(_bits(hit[1]), _bits(miss[1]))

        # the layer at rest: the parents' outputs, equal by value (-0 and +0 compare equal)
        oc.reset_ripples()
        pts = _points(R, cell, 4)
        assert np.array_equal(oc.read_surface_blend_rippled([0], s, pts, 4)[:-3], oc.read_surface_blend([0], s, pts, 4)[:-3])
        rr = _rays(5, 500, spread=40.0, level=z0)
        assert np.array_equal(oc.read_rays_rippled([0], s, rr, 4, 32, 8), oc.read_rays([0], s, rr, 4, 32, 8))


@pytest.mark.parametrize("N,C,cascades", [(64, 3, [0, 1, 2]), (2048, 2, [0, 1])])
def test_layer_at_rest_is_the_parent(capi, oracle, torch, N, C, cascades):
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        _prime(oc, 64, 1.0)
        oc.reset_ripples()
        s = _set(capi, 0)
        q = _points(64, 1.0, 8)
        a, b = oc.read_surface_blend_rippled(cascades, s, q, 4), oc.read_surface_blend(cascades, s, q, 4)
        assert np.array_equal(a[:-3], b[:-3]) and np.isnan(a[-3:]).all()
        # ray_cast_rippled is ray_cast's sibling: with the layer at rest the two agree on every record, bad rays and rays that leave the
        # finite range included, for every set of steps and bisections
        rays = _rays(N)
        rays[:6] = rays[6:12]
        rays[0, 4] = np.nan
        rays[1, 7] = rays[1, 3] - 1.0
        rays[2, 4:7] = 3e38
        rays[3, 0] = np.inf
        rays[4, 3], rays[4, 7], rays[4, 4:7] = -3e38, 3e38, (2.0, 2.0, -2.0)
        rays[5, 7] = rays[5, 3]
        for S, Rf in ((1, 0), (7, 12), (32, 8), (32, 0), (64, 24)):
            a, b = oc.read_rays_rippled(cascades, s, rays, 4, S, Rf), oc.read_rays(cascades, s, rays, 4, S, Rf)
            assert np.array_equal(a, b, equal_nan=True) and np.isnan(a[:5]).all() and np.isfinite(a[5:]).all(), (N, S, Rf)
        h = _header(capi, oracle, N, "example", 0)
        assert np.array_equal(_rippled_mesh(capi, torch, oc, cascades, h, 33, 17), _mesh(capi, torch, oc, cascades, h, 33, 17))


# 3 -- the mesh


def _rippled_mesh(capi, torch, oc, cascades, s, sx, sy):
    """_mesh of tests/test_gpu_blend.py for the rippled call: a sentinel-filled buffer with a guard tail"""
    verts = torch.full((sx * sy * 12 + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    oc.gen_blend_rippled(cascades, s, sx, sy, verts.data_ptr())
    oc.sync()
    raw = verts.cpu().numpy()
    sentinel = np.array([SENTINEL], F).view(np.uint32)[0]
    assert np.all(raw[sx * sy * 12:].view(np.uint32) == sentinel), "the guard tail was written"
    got = raw[: sx * sy * 12].reshape(sy, sx, 12)
    assert not np.any(got.view(np.uint32) == sentinel), ("vertices not written", sx, sy)
    assert np.all(got[..., 11] == -1)
    return got


@pytest.mark.parametrize("N,C,cascades", [(64, 3, [0, 1, 2]), (2048, 2, [0, 1])])
def test_mesh(capi, oracle, torch, report, N, C, cascades):
    worst = 0.0
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        for case, sx, sy, R, cell in (("example", 33, 17, 128, 0.5), ("example", 200, 150, 64, 1.0), ("grazing", 45, 37, 64, 1.0), ("above_horizon", 33, 17, 64, 1.0)):
            s = _header(capi, oracle, N, case, cascades[0])
            plain = _mesh(capi, torch, oc, cascades, s, sx, sy)
            lay = _prime(oc, R, cell)
            # the window over the mesh's nearest vertices (a jump that clears the layer: it is disturbed again there)
            gap = np.hypot(*np.moveaxis(np.diff(plain[..., :2].astype(np.float64), axis=1), -1, 0))
            near = plain[np.unravel_index(np.argmin(gap), gap.shape)][:2]                  # where the mesh is densest: next to the camera
            oc.center_ripples(float(near[0]), float(near[1]))
            lay.center(float(near[0]), float(near[1]))
            imp = _impulses(np.random.RandomState(sx), lay, 300, 0.05 * cell * cell)
            oc.deposit_ripples_host(imp)
            lay.deposit(imp)
            oc.step_ripples(0.1 * cell, 3)
            lay.step(0.1 * cell, 3)
            got = _rippled_mesh(capi, torch, oc, cascades, s, sx, sy)
            fin = np.isfinite(plain[..., :3]).all(-1)
            at = np.where(fin[..., None], plain[..., :2], F(0)).reshape(-1, 2)
            smp = oc.query_ripples(at).reshape(sy, sx, 4)
            tag = (N, case, sx, sy, R)
            for k in (0, 1, 3, 4):
                assert np.array_equal(_bits(got[..., k]), _bits(plain[..., k])), (tag, k)
            assert np.array_equal(_bits(got[..., 2][fin]), _bits((plain[..., 2] + smp[..., 0])[fin])), tag
            # a vertex whose stored x or y is not finite has the sample's NaNs for a height
            assert np.isnan(got[..., 2][~np.isfinite(plain[..., :2]).all(-1)]).all(), tag
            touched = (smp[..., 0] != 0) & fin
            if case == "example":
                assert touched.any() and (~touched).any(), (tag, touched.mean())
            if N == 64 and case != "above_horizon":
                maps = [oc.read_maps(c) for c in cascades]
                import gen64
                ray = gen64.ray32(s, sx, sy)
                want = rippled64.mesh64(s, maps, [_scale(c) for c in cascades], ray, lay)
                # the frame's bar of tests/test_gpu_blend.py (K_FRAME = 8 eps, absolute) and the layer's one eps with its factor 3
                d = np.abs(got[..., 5:11] - want.vertices[..., 5:11])[fin].max()
                worst = max(worst, float(d / ((8 + rippled64.K_RIPN) * EPS)))
            assert np.array_equal(_bits(_mesh(capi, torch, oc, cascades, s, sx, sy)), _bits(plain)), tag
    report(f"rippled mesh normals and tangents N={N}: worst share of (8 + K_RIPN) eps: {worst:.3f}")
    assert worst <= 1.0, worst


# 4 -- the cast: bit for bit against ray64.cast32 over read_surface_blend_rippled, no ray excluded


@pytest.mark.parametrize("N,C,lists,R,cell", [(64, 3, ([1], [0, 1, 2]), 128, 0.5), (2048, 2, ([0, 1],), 64, 1.0)])
def test_cast_bits(capi, oracle, N, C, lists, R, cell):
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        lay = _prime(oc, R, cell)
        rays = _rays(N, 1200, spread=45.0)
        rays[:3] = rays[3:6]
        rays[0, 4] = np.nan
        rays[1, 7] = rays[1, 3] - 1.0
        rays[2, 4:7] = 3e38
        for cascades in lists:
            for swell in (True, False):
                s = _set(capi, 0, swell)
                query = lambda q: oc.read_surface_blend_rippled(cascades, s, np.ascontiguousarray(q, F), 4)
                for S, Rf in ((1, 0), (7, 12), (32, 12), (32, 0)):
                    got = oc.read_rays_rippled(cascades, s, rays, 4, S, Rf)
                    want = rippled64.cast32(query, rays, S, Rf).records
                    nan = np.isnan(want)
                    assert np.array_equal(np.isnan(got), nan) and nan[:3].all() and not nan[3:].any(), (N, cascades, swell, S, Rf)
                    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), (N, cascades, swell, S, Rf, np.argwhere(_bits(got) != _bits(want))[:4])
                # the layer decides brackets: the same cast without it gives other parameters
                plain, rippled = oc.read_rays(cascades, s, rays, 4, 32, 12), oc.read_rays_rippled(cascades, s, rays, 4, 32, 12)
                assert (plain[3:, 0] != rippled[3:, 0]).mean() > 0.02, (N, cascades, swell)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))


# 5 -- edges and isolation


def test_edges(capi, oracle, torch):
    N, C, R, cell = 64, 3, 64, 1.0
    cascades = [0, 1, 2]
    with _setup(capi, oracle, N, C, foam="accumulate") as oc:
        _step(oc)
        s = _set(capi, 0)
        q = _points(R, cell, 2)
        rays = _rays(3, 300)
        mesh = torch.zeros(33 * 17 * 12, dtype=torch.float32, device="cuda:0")

        # the layer is off: ESTATE from every call, whatever else is said
        def refused(code, fn, *a, **k):
            with pytest.raises(capi.OceanError) as e:
                fn(*a, **k)
            assert e.value.code == code, (fn.__name__, e.value.code)
            assert ("datum_ocean_" + fn.__name__) in str(e.value), str(e.value)

        oc.set_ripples(0)
        refused(capi.ESTATE, oc.read_surface_blend_rippled, cascades, s, q, 4)
        refused(capi.ESTATE, oc.read_surface_blend_rippled, [7], s, q, 99)
        refused(capi.ESTATE, oc.read_rays_rippled, cascades, s, rays, 4, 32, 8)
        refused(capi.ESTATE, oc.gen_blend_rippled, cascades, s, 33, 17, mesh.data_ptr())
        refused(capi.ESTATE, oc.sample_surface_blend_rippled, cascades, s, 0, 0, 0)
        refused(capi.ESTATE, oc.cast_rays_rippled, cascades, s, 0, 0, 0)

        lay = _prime(oc, R, cell)
        before = oc.read_ripples().copy()
        maps = [oc.read_maps(c).copy() for c in cascades]
        foam = [oc.read_foam(c).copy() for c in cascades]

        # every refusal of the parents
        refused(capi.EINVAL, oc.read_surface_blend_rippled, [3], s, q, 4)
        refused(capi.EINVAL, oc.read_surface_blend_rippled, [], s, q, 4)
        refused(capi.EINVAL, oc.read_surface_blend_rippled, cascades, s, q, -1)
        refused(capi.EINVAL, oc.read_surface_blend_rippled, cascades, s, q, 65)
        refused(capi.EINVAL, oc.read_rays_rippled, cascades, s, rays, 4, 0, 8)
        refused(capi.EINVAL, oc.read_rays_rippled, cascades, s, rays, 4, 32, 99)
        refused(capi.EINVAL, oc.read_rays_rippled, [-1], s, rays, 4, 32, 8)
        refused(capi.EINVAL, oc.gen_blend_rippled, cascades, s, 1, 17, mesh.data_ptr())
        refused(capi.EINVAL, oc.gen_blend_rippled, cascades, s, 33, 17, mesh.data_ptr() + 4)
        refused(capi.EINVAL, oc.gen_blend_rippled, [9], s, 33, 17, mesh.data_ptr())
        dq = torch.from_numpy(q).cuda()
        out = torch.zeros(len(q) * 8 + 16, dtype=torch.float32, device="cuda:0")
        refused(capi.EINVAL, oc.sample_surface_blend_rippled, cascades, s, dq.data_ptr(), len(q), out.data_ptr() + 4)
        dr = torch.from_numpy(rays).cuda()
        rec = torch.zeros(len(rays) * 12 + 16, dtype=torch.float32, device="cuda:0")
        refused(capi.EINVAL, oc.cast_rays_rippled, cascades, s, dr.data_ptr() + 8, len(rays), rec.data_ptr())

        # n = 0 enqueues nothing; canaries before and after the device outputs; the device calls against the host twins
        CAN = 12345.0
        out.fill_(CAN)
        rec.fill_(CAN)
        oc.sample_surface_blend_rippled(cascades, s, 0, 0, 0)
        oc.cast_rays_rippled(cascades, s, 0, 0, 0)
        oc.sample_surface_blend_rippled(cascades, s, dq.data_ptr(), 0, out.data_ptr())
        oc.sync()
        assert bool((out == CAN).all()) and bool((rec == CAN).all())
        oc.sample_surface_blend_rippled(cascades, s, dq.data_ptr(), len(q), out.data_ptr() + 32)
        oc.cast_rays_rippled(cascades, s, dr.data_ptr(), len(rays), rec.data_ptr() + 32, 4, 32, 8)
        oc.sync()
        o, r = out.cpu().numpy(), rec.cpu().numpy()
        assert np.all(o[:8] == CAN) and np.all(o[8 + len(q) * 8:] == CAN) and np.all(r[:8] == CAN) and np.all(r[8 + len(rays) * 12:] == CAN)
        host = oc.read_surface_blend_rippled(cascades, s, q, 4)
        assert np.array_equal(_bits(o[8:8 + len(q) * 8].reshape(-1, 8)[:-3]), _bits(host[:-3])) and np.isnan(o[8:8 + len(q) * 8].reshape(-1, 8)[-3:]).all()
        assert np.array_equal(_bits(r[8:8 + len(rays) * 12].reshape(-1, 12)), _bits(oc.read_rays_rippled(cascades, s, rays, 4, 32, 8)))

        # nothing but the outputs was written: both state buffers and src (a step shows them), the maps, the foam planes
        assert np.array_equal(_bits(oc.read_ripples()), _bits(before))
        for c, m in zip(cascades, maps):
            assert np.array_equal(_bits(oc.read_maps(c)), _bits(m))
        for c, fo in zip(cascades, foam):
            assert np.array_equal(_bits(oc.read_foam(c)), _bits(fo))
        oc.step_ripples(0.1 * cell, 2)
        lay.step(0.1 * cell, 2)
        assert np.array_equal(_bits(oc.read_ripples()), _bits(lay.window()))


# 6 -- the C++ shim against both bindings


def test_cpp_shim_matches_capi(capi, torch):
    from datum_amd import host_api

    N, R, cell = 64, 64, 1.0
    params = host_api.OceanParams(N, **host_api.EXAMPLE_TUNABLES)
    params.seed_ocean(1000)
    camera = host_api.example_camera()
    rng = np.random.RandomState(5)
    with host_api.OceanContext(N, device=0) as ctx:
        mesh = ctx.create_ocean(33, 17)
        ctx.render_ocean_surface(mesh, params, camera)
        plain = ctx.read_vertices(mesh).copy()
        # the layer is off: the shim raises with the C ABI's text
        for call in (lambda: ctx.query_ocean_surface_rippled(params, np.zeros((2, 2), F)), lambda: ctx.cast_ocean_rays_rippled(params, _rays(1, 4)),
                     lambda: ctx.gen_ocean_surface_rippled(mesh, params, camera)):
            with pytest.raises(host_api.HostError, match="the ripple layer is off"):
                call()
        gap = np.hypot(*np.moveaxis(np.diff(plain[..., :2].astype(np.float64), axis=1), -1, 0))
        near = plain[np.unravel_index(np.argmin(gap), gap.shape)][:2]
        ctx.set_ocean_ripples(R, cell)
        ctx.center_ocean_ripples(float(near[0]), float(near[1]))
        imp = np.zeros((300, 4), F)
        imp[:, :2] = near + rng.uniform(-0.45, 0.45, (300, 2)) * R * cell
        imp[:, 2] = rng.normal(size=300) * 0.05
        ctx.deposit_ocean_ripples(imp)
        ctx.step_ocean_ripples(0.1 * cell, 3)
        q = (near + rng.uniform(-0.6, 0.6, (500, 2)) * R * cell).astype(F)
        smp = ctx.query_ocean_ripples(q)
        assert np.abs(smp[:, 0]).max() > 1e-4
        # the query: the shim's parent plus the shim's sample, and nothing else moved
        base, got = ctx.query_ocean_surface(params, q), ctx.query_ocean_surface_rippled(params, q)
        assert np.array_equal(_bits(got[:, 2]), _bits(base[:, 2] + smp[:, 0]))
        assert np.array_equal(_bits(got[:, [0, 1, 3, 7]]), _bits(base[:, [0, 1, 3, 7]])) and (got[:, 4:7] != base[:, 4:7]).any()
        # the cast: ray64.cast32 over the shim's rippled query, bit for bit
        rays = _rays(3, 300, spread=20.0)
        rays[:, :2] += near
        rec = ctx.cast_ocean_rays_rippled(params, rays, 4, 16, 6)
        want = rippled64.cast32(lambda p: ctx.query_ocean_surface_rippled(params, np.ascontiguousarray(p, F)), rays, 16, 6).records
        assert np.array_equal(_bits(rec), _bits(want))
        # the mesh: the rendered vertices' x, y, u, v, z lifted by the sample at the stored (x, y); nothing was displaced
        ctx.gen_ocean_surface_rippled(mesh, params, camera)
        verts = ctx.read_vertices(mesh)
        lift = ctx.query_ocean_ripples(plain[..., :2].reshape(-1, 2))[:, 0].reshape(plain.shape[:2])
        assert np.array_equal(_bits(verts[..., [0, 1, 3, 4]]), _bits(plain[..., [0, 1, 3, 4]]))
        assert np.array_equal(_bits(verts[..., 2]), _bits(plain[..., 2] + lift)) and (lift != 0).any()

