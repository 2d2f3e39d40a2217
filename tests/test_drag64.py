"""The references of body drag (tests/drag64.py) against answers known in closed form, on hand-made velocity records; and the sensitivity
of the fp32 restatement: every planted mistake changes reduce32's bits on the fleet the GPU test uses."""

import numpy as np

import body64
import drag64
from test_gpu_body import _box, _fleet

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _sum64(bodies, motions, probes, recs):
    """the definition in float64 on given records: drag64.terms64 summed per body (the part of drag64.drag64 behind the query)"""
    bi, pi = body64._gather(bodies, probes)
    R, T = bodies["rotation"][bi].astype(np.float64), bodies["position"][bi].astype(np.float64)
    pr = np.asarray(probes, np.float64)[pi]
    w = np.stack([R[:, 3 * r] * pr[:, 0] + R[:, 3 * r + 1] * pr[:, 1] + R[:, 3 * r + 2] * pr[:, 2] + T[:, r] for r in range(3)], 1)
    d = np.minimum(np.maximum(recs[:, 2] - w[:, 2], 0.0), bodies["cap"][bi].astype(np.float64))
    m = pr[:, 3] * d
    mo = {k: motions[k][bi].astype(np.float64) for k in ("linear", "angular", "cl", "cq")}
    f, tau, _, _ = drag64.terms64(w - T, mo["linear"], mo["angular"], mo["cl"], mo["cq"], m, recs[:, 4:7])
    out = np.zeros((len(bodies), 7))
    np.add.at(out, bi, np.concatenate([f, tau, m[:, None]], 1))
    return out


def _flat_records(n, height, velocity):
    r = np.zeros((n, 8))
    r[:, 2] = height
    r[:, 4:7] = velocity
    return r


def test_closed_forms():
    probes = _box()
    n = len(probes)
    sa = float(probes[:, 3].sum())
    x, y, a = (probes[:, k].astype(np.float64) for k in (0, 1, 3))
    # a level box with its origin 0.5 under flat water: d = 0.5 for every probe, sum m = 0.5 sum a
    bodies = body64.make_bodies([np.eye(3)] * 3, [[10, -20, -0.5]] * 3, [0] * 3, [n] * 3, [np.inf] * 3)
    v, Om, cur = np.array([1.5, -2.0, 0.5]), 0.7, np.array([0.3, 0.4, 0.0])
    motions = drag64.make_motions([v, [0, 0, 0], [0, 0, 0]], [[0, 0, 0], [0, 0, Om], [0, 0, 0]], [0.8, 1.3, 0.5], [0.6, 0.0, 2.0])
    recs = np.concatenate([_flat_records(n, 0.0, 0.0), _flat_records(n, 0.0, 0.0), _flat_records(n, 0.0, cur)])
    for got in (_sum64(bodies, motions, probes, recs), drag64.reduce32(bodies, motions, probes, recs.astype(F)).astype(np.float64)[:, :7]):
        tol = 1e-5                       # (a check of the formulas, fp32's eps times a few dozen terms at the most: not a precision bar)
        sm = 0.5 * sa
        assert np.allclose(got[:, 6], sm, rtol=tol, atol=0)
        # translating through still water: F = -(sum m)(cl + cq |v|) v, no torque on the symmetric box
        assert np.allclose(got[0, :3], -sm * (0.8 + 0.6 * np.linalg.norm(v)) * v, rtol=tol, atol=tol)
        assert np.allclose(got[0, 3:6], 0, atol=2e-4)
        # yawing, cq = 0: u = Om (-y, x, 0), F = 0 on the symmetric box, tau z = -cl Om sum m (x^2 + y^2)
        assert np.allclose(got[1, :3], 0, atol=2e-4)
        assert np.allclose(got[1, 5], -1.3 * Om * float((a * 0.5 * (x * x + y * y)).sum()), rtol=tol)
        assert np.allclose(got[1, 3:5], 0, atol=2e-4)
        # at rest in a current: F = (sum m)(cl + cq |c|) c, carried along; no torque
        assert np.allclose(got[2, :3], sm * (0.5 + 2.0 * 0.5) * cur, rtol=tol, atol=tol)
        assert np.allclose(got[2, 3:6], 0, atol=2e-4)


def test_dry_and_capped_and_the_tilted_arm():
    probes = _box()
    n = len(probes)
    c, sn = np.cos(0.25), np.sin(0.25)
    roll = [[1, 0, 0], [0, c, -sn], [0, sn, c]]
    # above the water; capped at 0.125; rolled: the arm has a z part, and the drag of a sideways motion a torque about x
    bodies = body64.make_bodies([np.eye(3), np.eye(3), roll], [[0, 0, 5.0], [0, 0, -0.5], [0, 0, -1.5]], [0] * 3, [n] * 3, [np.inf, 0.125, np.inf])
    motions = drag64.make_motions([[1, 2, 3], [1, 0, 0], [0, 2, 0]], [[0.1, 0.2, 0.3], [0, 0, 0], [0, 0, 0]], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0])
    recs = _flat_records(3 * n, 0.0, 0.0)
    got = _sum64(bodies, motions, probes, recs)
    a, y = probes[:, 3].astype(np.float64), probes[:, 1].astype(np.float64)
    assert np.all(got[0] == 0)
    assert np.isclose(got[1, 6], 0.125 * a.sum()) and np.isclose(got[1, 0], -0.125 * a.sum())
    # rolled: w.z = -1.5 + y sin, d = 1.5 - y sin, r = (x, y cos, y sin); f = -m (0, 2, 0): tau x = -r.z f.y = 2 m y sin
    m = a * (1.5 - y * sn)
    assert np.isclose(got[2, 1], -2 * m.sum()) and np.isclose(got[2, 3], float((2 * m * y * sn).sum()))
    got32 = drag64.reduce32(bodies, motions, probes, recs.astype(F))
    assert np.allclose(got32[:, :7], got, rtol=1e-5, atol=1e-4)
    assert np.all(_bits(got32[0]) == 0)


def _fleet_motions(seed, nb):
    from test_drag_emul import _motions

    return _motions(np.random.RandomState(seed), nb)


def test_every_mistake_changes_the_bits():
    bodies, probes = _fleet(64)
    motions = _fleet_motions(64, len(bodies))
    rng = np.random.RandomState(5)
    rows = body64.offsets(bodies, len(probes))[1]
    w, _, _ = body64.world32(bodies, probes)
    recs = np.zeros((rows, 8), F)
    recs[:, 2] = w[:, 2] + rng.uniform(-1.0, 1.5, rows)
    recs[:, 3] = rng.uniform(0, 1e-3, rows)
    recs[:, 4:7] = rng.normal(size=(rows, 3)) * (2.0, 2.0, 1.0)
    right = drag64.reduce32(bodies, motions, probes, recs)
    assert np.isfinite(right).all() and np.array_equal(_bits(right), _bits(drag64.reduce32(bodies, motions, probes, recs)))
    assert drag64.MISTAKES == ("omega_sign", "no_rz", "wet_switch", "s_no_z", "fma", "tau_transposed")
    for mistake in drag64.MISTAKES:
        wrong = drag64.reduce32(bodies, motions, probes, recs, mistake)
        changed = (_bits(wrong) != _bits(right)).any(1)
        assert changed.sum() >= len(bodies) // 4, (mistake, int(changed.sum()))
        # the weight and the residual are no part of any of them
        assert np.array_equal(_bits(wrong[:, 6:]), _bits(right[:, 6:])), mistake
