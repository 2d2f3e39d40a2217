"""ray64.cast64, the float64 restatement of the ray cast the GPU tests compare against, held to answers known without it:

  * on a plane the bracket holds the closed-form parameter, and hi lies within Δ·2^-R of it;
  * on two superposed sinusoids hi is within Δ·2^-R above the first root a dense float64 scan (64 points per march step) finds, wherever
    the scan sees no second change of side inside the march step of the first (there a bisection may keep either root);
  * the comparison discriminates: a cast that takes the last crossing, one that returns lo for hi and one that skips t_S each fail it.
"""

import numpy as np

import ray64

F = np.float32
S, R = 32, 12


def _plane(a, b, c):
    def height(q):
        q = np.asarray(q, np.float64)
        rec = np.zeros((len(q), 8))
        rec[:, 0:2], rec[:, 2], rec[:, 6] = q, a * q[:, 0] + b * q[:, 1] + c, 1.0
        return rec
    return height


def _waves(q):
    q = np.asarray(q, np.float64)
    rec = np.zeros((len(q), 8))
    rec[:, 0:2], rec[:, 6] = q, 1.0
    rec[:, 2] = 0.9 * np.sin(0.21 * q[:, 0] + 0.13 * q[:, 1] + 0.3) + 0.35 * np.sin(-0.8 * q[:, 0] + 0.55 * q[:, 1] + 1.7) + 0.1
    return rec


def _rays(seed, n=3000):
    rng = np.random.RandomState(seed)
    r = np.empty((n, 8), F)
    r[:, 0:2] = rng.uniform(-40, 40, (n, 2))
    r[:, 2] = rng.uniform(-3, 3.5, n)
    az = rng.uniform(0, 2 * np.pi, n)
    el = np.radians(rng.uniform(2, 90, n)) * rng.choice([-1, 1], n)
    length = rng.uniform(0.3, 3.0, n)
    r[:, 4], r[:, 5], r[:, 6] = length * np.cos(el) * np.cos(az), length * np.cos(el) * np.sin(az), length * np.sin(el)
    r[:, 3] = rng.uniform(-1, 1, n)
    r[:, 7] = r[:, 3] + rng.uniform(0.5, 12, n) / length
    return r


def _plane_failures(c, rays, a, b, c0):
    """rays whose record disagrees with the closed form t* = (a ox + b oy + c0 - oz) / (dz - a dx - b dy)"""
    r = rays.astype(np.float64)
    tstar = (a * r[:, 0] + b * r[:, 1] + c0 - r[:, 2]) / (r[:, 6] - a * r[:, 4] - b * r[:, 5])
    inside = (tstar > r[:, 3]) & (tstar <= r[:, 7])
    delta = (r[:, 7] - r[:, 3]) / S
    hi, lo, status = c.records[:, 0], c.records[:, 1], c.records[:, 3]
    g0 = r[:, 2] + r[:, 3] * r[:, 6] - (a * (r[:, 0] + r[:, 3] * r[:, 4]) + b * (r[:, 1] + r[:, 3] * r[:, 5]) + c0)
    want = np.where(inside, np.where(g0 < 0, ray64.LEAVE, ray64.ENTER), ray64.MISS)
    tol = delta * 2.0 ** -R + 1e-12 * (1 + np.abs(tstar))
    wrong = status != want
    wrong |= inside & ~((lo <= tstar + 1e-12) & (tstar <= hi + 1e-12) & (hi - tstar <= tol))
    wrong |= ~inside & ((hi != r[:, 7]) | (lo != r[:, 7]))
    return wrong, inside


def test_plane_closed_form():
    a, b, c0 = 0.05, -0.03, 0.4
    rays = _rays(1)
    c = ray64.cast64(_plane(a, b, c0), rays, S, R)
    wrong, inside = _plane_failures(c, rays, a, b, c0)
    assert inside.mean() > 0.2 and (~inside).mean() > 0.2
    assert not wrong.any(), wrong.nonzero()[0][:5]
    assert c.calls <= S + R + 2
    for v in (ray64.MISS, ray64.ENTER, ray64.LEAVE):
        assert (c.records[:, 3] == v).mean() > 0.1


def _scan(rays, per_step=64):
    """(first root by a dense scan with linear interpolation, the march step it lies in, whether that step holds another change of side)"""
    r = rays.astype(np.float64)
    n = len(r)
    m = S * per_step
    u = np.arange(m + 1) / m
    t = r[:, 3:4] + (r[:, 7:8] - r[:, 3:4]) * u
    x, y, z = r[:, 0:1] + t * r[:, 4:5], r[:, 1:2] + t * r[:, 5:6], r[:, 2:3] + t * r[:, 6:7]
    g = z - _waves(np.stack([x.ravel(), y.ravel()], 1))[:, 2].reshape(n, m + 1)
    change = (g[:, 1:] < 0) != (g[:, :-1] < 0)
    any_ = change.any(1)
    k = change.argmax(1)
    rows = np.arange(n)
    g0, g1 = g[rows, k], g[rows, k + 1]
    root = t[rows, k] + (t[rows, k + 1] - t[rows, k]) * g0 / (g0 - g1)
    step = k // per_step
    counts = np.add.reduceat(change, np.arange(0, m, per_step), axis=1)
    # the march sees a change in a step only if the step's ends differ: an even count hides it
    crowded = any_ & (counts[rows, step] != 1)
    hidden = ((counts[:, :] % 2 == 0) & (counts > 0)).any(1)
    return root, step, any_, crowded | hidden, (t[:, 1] - t[:, 0])


def _waves_failures(c, rays):
    root, step, any_, unclear, fine = _scan(rays)
    r = rays.astype(np.float64)
    delta = (r[:, 7] - r[:, 3]) / S
    hi, lo, status = c.records[:, 0], c.records[:, 1], c.records[:, 3]
    ok = ~unclear
    wrong = ok & ((status != ray64.MISS) != any_)
    hit = ok & any_
    # hi lies above the root by at most the final bracket; the scan's own root is good to its spacing squared times the curvature
    slack = fine * 0.05 + 1e-9
    wrong |= hit & ~((c.index == step + 1) & (lo <= root + slack) & (root <= hi + slack) & (hi - root <= delta * 2.0 ** -R + slack))
    return wrong, ok, hit


def test_sinusoid_first_root():
    rays = _rays(2)
    c = ray64.cast64(_waves, rays, S, R)
    wrong, ok, hit = _waves_failures(c, rays)
    assert ok.mean() > 0.8 and hit.mean() > 0.3
    assert not wrong.any(), wrong.nonzero()[0][:5]


def test_the_comparison_discriminates():
    a, b, c0 = 0.05, -0.03, 0.4
    rays = _rays(3)
    # on the plane: lo for hi puts field 0 below the root; a skipped t_S loses the rays that cross in the last step
    for mistake in ("lo_for_hi", "skip_tS"):
        wrong, _ = _plane_failures(ray64.cast64(_plane(a, b, c0), rays, S, R, mistake), rays, a, b, c0)
        assert wrong.sum() >= 5, mistake                     # (the tests above take a single wrong ray as a failure)
    # on the sinusoids: the last crossing is not the first wherever a ray crosses twice (lo for hi is below what the scan resolves there)
    for mistake in ("last", "skip_tS"):
        wrong, _, _ = _waves_failures(ray64.cast64(_waves, rays, S, R, mistake), rays)
        assert wrong.sum() >= 5, mistake                     # (the tests above take a single wrong ray as a failure)
    # and float32 follows float64 except where a sample grazes: the two restatements are one definition
    c32 = ray64.cast32(lambda q: _waves(q).astype(F), rays, S, R)
    c64 = ray64.cast64(_waves, rays, S, R)
    assert (c32.records[:, 3] == c64.records[:, 3]).mean() > 0.99
