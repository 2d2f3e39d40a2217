"""The host twins' device staging (ocean_capi.hip: Staging, read_staged): the six read_* queries of one handle, interleaved, with counts that
grow, shrink and regrow every staging buffer and cross one 256-thread workgroup.  Each result is the same query's device-array twin on
torch tensors, bit for bit."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
N, LIST, ITERATIONS, STEPS, REFINE = 64, [0, 1], 4, 16, 4
SCALES = (22.0, 64.0)
COUNTS = (3, 300, 1, 700, 2)
PROBES_PER_BODY = 3


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _set(capi):
    s = capi.OceanSet()
    s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, 0.8, 0.5, 1.1
    s.swelldirection[:] = (0.780869, 0.624695)
    s.plane[:] = (0.0, 0.0, 1.0, -0.3)
    s.scale = F(1.0) / F(SCALES[1])                                          # the single-cascade query's (cascade 1)
    return s


def _points(rs, n):
    return rs.uniform(-200, 200, (n, 2)).astype(F)


def _rays(rs, n):
    r = np.empty((n, 8), F)
    el = np.radians(rs.uniform(2, 90, n)) * rs.choice([-1, 1], n)
    az = rs.uniform(0, 2 * np.pi, n)
    r[:, 0:2] = rs.uniform(-200, 200, (n, 2))
    r[:, 2] = 0.3 - np.sign(el) * rs.uniform(0.5, 4.0, n)                    # up-going rays start below, down-going above
    r[:, 4], r[:, 5], r[:, 6] = np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)
    r[:, 3] = 0.0
    r[:, 7] = rs.uniform(4.0, 8.0, n) / np.abs(np.sin(el))
    return r


def _bodies(capi, rs, n):
    b = np.zeros(n, capi.BODY_DTYPE)
    angle = rs.uniform(0, 2 * np.pi, n)
    rot = np.zeros((n, 3, 3), F)
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = np.cos(angle), -np.sin(angle), np.sin(angle), np.cos(angle), 1.0
    b["rotation"] = rot.reshape(n, 9)
    b["position"] = np.concatenate([rs.uniform(-200, 200, (n, 2)), rs.uniform(-0.5, 0.5, (n, 1))], 1).astype(F)
    b["first"] = np.arange(n) * PROBES_PER_BODY
    b["count"] = PROBES_PER_BODY
    b["cap"] = 2.0
    probes = np.concatenate([rs.uniform(-1, 1, (n * PROBES_PER_BODY, 3)), rs.uniform(0.1, 1.0, (n * PROBES_PER_BODY, 1))], 1).astype(F)
    return b, probes


def test_read_twins_interleaved_are_the_device_twins_bits():
    import torch

    from datum_amd import capi

    capi.load()
    rs = np.random.RandomState(7)
    s = _set(capi)

    def device(host, floats, launch):
        """the device-array twin: `host` arrays as torch tensors, `floats` floats of result per row of the first"""
        tensors = [torch.from_numpy(np.ascontiguousarray(h).view(np.uint8).reshape(-1)).cuda() for h in host]
        out = torch.zeros(len(host[0]) * floats, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        launch(*[t.data_ptr() for t in tensors], out.data_ptr())
        oc.sync()
        return out.cpu().numpy().reshape(len(host[0]), floats)

    with capi.Ocean(N, len(SCALES)) as oc:
        for c, ws in enumerate(SCALES):
            oc.set_cascade(c, ws, 1.0)
            oc.upload_state(c, (rs.standard_normal((N, N, 2)) * (0.4 / N)).astype(F))
        oc.set_foam("accumulate")
        oc.set_velocity("on")
        oc.update(F(1 / 60))
        oc.displace()
        oc.reduce_bounds()

        for n in COUNTS:
            pts, rays = _points(rs, n), _rays(rs, n)
            bodies, probes = _bodies(capi, rs, n)
            got = {
                "surface": oc.read_surface(1, s, pts, ITERATIONS),
                "rays": oc.read_rays(LIST, s, rays, ITERATIONS, STEPS, REFINE),
                "surface_blend": oc.read_surface_blend(LIST, s, pts, ITERATIONS),
                "bodies": oc.read_bodies(LIST, s, bodies, probes, ITERATIONS),
                "velocity_blend": oc.read_velocity_blend(LIST, s, pts, ITERATIONS),
                "rays_bounded": oc.read_rays_bounded(LIST, s, rays, ITERATIONS, STEPS, REFINE),
            }
            want = {
                "surface": device([pts], 8, lambda p, o: oc.sample_surface(1, s, p, n, o, ITERATIONS)),
                "surface_blend": device([pts], 8, lambda p, o: oc.sample_surface_blend(LIST, s, p, n, o, ITERATIONS)),
                "velocity_blend": device([pts], 8, lambda p, o: oc.sample_velocity_blend(LIST, s, p, n, o, ITERATIONS)),
                "bodies": device([bodies, probes], 8, lambda b, p, o: oc.reduce_bodies(LIST, s, b, n, p, len(probes), o, ITERATIONS)),
                "rays": device([rays], 12, lambda r, o: oc.cast_rays(LIST, s, r, n, o, ITERATIONS, STEPS, REFINE)),
                "rays_bounded": device([rays], 12, lambda r, o: oc.cast_rays_bounded(LIST, s, r, n, o, ITERATIONS, STEPS, REFINE)),
            }
            for name in want:
                assert got[name].shape == want[name].shape, (n, name)
                assert np.array_equal(_bits(got[name]), _bits(want[name])), (n, name)
            # (the records are answers, not the NaNs of refused input, which would compare equal as well)
            for name in want:
                answers = got[name][:, 3] if name.startswith("rays") else got[name]          # (a ray's status)
                assert np.isfinite(answers).all(), (n, name)
