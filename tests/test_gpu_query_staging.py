"""The host twins' device staging (ocean_capi.hip: Staging, read_staged): the six read_* queries of one handle, interleaved, with counts that
grow, shrink and regrow every staging buffer and cross one 256-thread workgroup.  Each result is the same query's device-array twin on
torch tensors, bit for bit.  The five body host twins share one pair of helpers (stage_batch, fetch_batch): interleaved on one handle with
stagings that grow, shrink and go to zero, each returns what the same call returns on a fresh handle, bit for bit."""

import ctypes

import numpy as np
import pytest

import body64
import drag64
import step64

pytestmark = pytest.mark.gpu

F = np.float32
N, LIST, ITERATIONS, STEPS, REFINE = 64, [0, 1], 4, 16, 4
SCALES = (22.0, 64.0)
COUNTS = (3, 300, 1, 700, 2)
PROBES_PER_BODY = 3
BODY_COUNTS, PROBE_COUNTS = (1, 3, 2, 0), (4, 16, 0, 8)
R, CELL, DT, SUBSTEPS = 64, 0.5, F(1 / 60), 2


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


def _body_ocean(capi):
    """N = 64, one cascade, velocity on, one displace, the layer on and at rest: every handle made here holds the same state"""
    oc = capi.Ocean(N, 1)
    oc.set_cascade(0, SCALES[0], 1.0)
    oc.upload_state(0, (np.random.RandomState(3).standard_normal((N, N, 2)) * (0.4 / N)).astype(F))
    oc.set_velocity("on")
    oc.update(DT)
    oc.displace()
    oc.set_ripples(R, CELL)
    return oc


def _batch(rs, nb, npr):
    """nb bodies inside the layer's window that all walk the same npr probes, with their motions and props"""
    pos = np.concatenate([rs.uniform(-8, 8, (nb, 2)), rs.uniform(-0.5, 0.5, (nb, 1))], 1)
    bodies = body64.make_bodies([np.eye(3)] * nb, pos, [0] * nb, [npr] * nb, [2.0] * nb)
    motions = drag64.make_motions(rs.uniform(-1, 1, (nb, 3)), rs.uniform(-0.3, 0.3, (nb, 3)), [1.0] * nb, [0.5] * nb)
    props = step64.make_props(np.full(nb, 1e-3), np.full((nb, 3), 1e-3), 9.81, 9810.0)
    probes = np.concatenate([rs.uniform(-1, 1, (npr, 3)), rs.uniform(0.1, 1.0, (npr, 1))], 1).astype(F)
    return bodies, motions, props, probes


def _body_calls(oc, s, batch):
    """the five body host twins on `oc`, from the layer at rest with one impulse pending: all they return, the layer before and after"""
    bodies, motions, props, probes = batch
    oc.deposit_ripples_host([[1.0, 2.0, 0.05, 0.0]])
    out = {"lift": oc.read_bodies([0], s, bodies, probes, ITERATIONS),
           "drag": oc.read_body_drag([0], s, bodies, motions, probes, ITERATIONS),
           "wake": oc.deposit_body_ripples_host([0], s, bodies, motions, probes, DT, ITERATIONS)}
    for name, step in (("step", oc.step_bodies_host), ("coupled", oc.step_bodies_coupled_host)):
        b, m = bodies.copy(), motions.copy()
        out["before " + name] = oc.read_ripples()
        out[name] = step([0], s, b, m, props, probes, DT, SUBSTEPS, ITERATIONS)
        out[name + " bodies"], out[name + " motions"] = b.view(np.uint8), m.view(np.uint8)
    out["after"] = oc.read_ripples()
    return out


def test_body_twins_interleaved_are_a_fresh_handles_bits():
    from datum_amd import capi

    capi.load()
    rs = np.random.RandomState(11)
    s = _set(capi)
    with _body_ocean(capi) as oc:
        for nb, npr in zip(BODY_COUNTS, PROBE_COUNTS):
            batch = _batch(rs, nb, npr)
            oc.reset_ripples()
            got = _body_calls(oc, s, batch)
            with _body_ocean(capi) as fresh:
                want = _body_calls(fresh, s, batch)
            for name in want:
                assert got[name].shape == want[name].shape, (nb, npr, name)
                assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint8), np.ascontiguousarray(want[name]).view(np.uint8)), (nb, npr, name)
            for name in ("lift", "drag", "wake", "step", "coupled"):
                assert got[name].shape[0] == nb and np.isfinite(got[name]).all(), (nb, npr, name)
            # the coupled twin steps the layer, with bodies or without: the pending impulse is in the state after it, and not before
            assert not got["before coupled"].any() and got["after"].any(), (nb, npr)
            if nb > 0:
                assert got["step bodies"].tobytes() != batch[0].tobytes() and got["coupled motions"].tobytes() != batch[1].tobytes(), (nb, npr)
        # nbodies == 0 with arrays that are there: step_bodies_host returns before it stages or writes anything
        b, m, p, pr = _batch(rs, 2, 4)
        keep, rec = (b.tobytes(), m.tobytes()), np.full((2, 8), 7.0, F)
        ptr = lambda a: a.ctypes.data_as(capi.P)
        assert oc.lib.datum_ocean_step_bodies_host(oc.h, (capi.I * 1)(0), 1, ctypes.byref(s), ITERATIONS, ptr(b), ptr(m), ptr(p), 0, ptr(pr), 4, DT, SUBSTEPS, ptr(rec)) == 0
        assert (b.tobytes(), m.tobytes()) == keep and np.all(rec == 7.0)
