"""Body stepping's sub-step (tests/step64.py: integrate32, integrate64) against closed forms, and the planted mistakes each caught.

  * zero sums: a body in free fall, v.z' = v.z + h (0 - g), exactly one product, one difference and one sum in fp32;
  * zero torque and no spin: R is reproduced -- an exact rotation to the roundings of the re-orthonormalisation: with eps = 2^-24, c_j' = c_j,
    the norm of a unit column carries its own |c| - 1 (up to 3 ulp of the entries: 3 eps) and four roundings, the division one: a column
    moves by at most 8 eps; y also by x's error through the projection (2 x 8 eps) and five roundings of the projection: 29 eps;
    z = x X y by 2 (8 + 29) eps and three roundings: 77 eps.  BAR_R = 77 eps for every entry;
  * constant omega about z, K sub-steps: the columns stay orthonormal.  After the Gram-Schmidt step, whatever came in: |x|^2 - 1 within
    2 (5 eps) (norm's four roundings and the division, doubled by the square) + 3 eps (the check's own sum in float64 is exact: 0) -> 10 eps;
    x.y within (5 + 5) eps for the projection's roundings relative to |c_1'| <= 1 + h |omega| and the division by n1 >= 1 / 2, i.e.
    2 (1 + h |omega|) 10 eps; |y|^2 - 1 within 10 eps; z against x, y: products of values below 1, three roundings per component -> 3 eps each,
    |z|^2 - 1 within 2 sqrt(3) 3 eps + the defects above.  BAR_ORTHO = 40 eps covers each of them for h |omega| <= 1 / 2, and does
    not grow with K: every sub-step orthonormalises anew;
  * invmass = 0 and gravity = 0: T' = T + h v, v unchanged bit for bit, whatever the sums; with v = 0 too, T is unchanged bit for bit;
  * the planted mistakes of step64.MISTAKES each move a result by far more than rounding.
"""

import numpy as np

import body64
import drag64
import step64

F = np.float32
EPS = 2.0 ** -24
BAR_R = 77 * EPS
BAR_ORTHO = 40 * EPS


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _bodies(seed, n):
    rng = np.random.RandomState(seed)
    rot = [np.eye(3) if b % 5 == 0 else _rot(rng) for b in range(n)]
    return body64.make_bodies(rot, rng.uniform(-200, 200, (n, 3)), [0] * n, [0] * n, [np.inf] * n), rng


def _zero(n):
    return np.zeros((n, 8), F), np.zeros((n, 8), F)


def test_free_fall():
    n = 16
    bodies, rng = _bodies(1, n)
    motions = drag64.make_motions(rng.uniform(-3, 3, (n, 3)), np.zeros((n, 3)), np.full(n, 0.5), np.full(n, 0.5))
    props = step64.make_props(rng.uniform(1e-4, 1e-2, n), np.full((n, 3), 1e-3), 9.81, 9810.0)
    lift, drag = _zero(n)
    h = step64.step_size(1 / 60, 2)
    nb, nm, rec, bad = step64.integrate32(lift, drag, bodies, motions, props, h)
    assert not bad.any() and np.all(rec == 0)
    g = props["gravity"]
    v = motions["linear"]
    assert np.array_equal(_bits(nm["linear"][:, 2]), _bits(v[:, 2] + h * (F(0) * props["invmass"] - g)))
    assert np.array_equal(_bits(nm["linear"][:, :2]), _bits(v[:, :2]))
    assert np.array_equal(_bits(nb["position"]), _bits(bodies["position"] + h * nm["linear"]))          # the NEW velocity
    assert np.array_equal(_bits(nm["angular"]), _bits(motions["angular"]))


def test_no_torque_reproduces_the_rotation():
    n = 64
    bodies, rng = _bodies(2, n)
    motions = drag64.make_motions(rng.uniform(-3, 3, (n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n))
    props = step64.make_props(np.full(n, 1e-3), np.full((n, 3), 1e-3), 9.81, 9810.0)
    lift, drag = _zero(n)
    lift[:, 0], drag[:, :3] = 50.0, rng.uniform(-10, 10, (n, 3))                    # forces but no torque
    nb, nm, _, bad = step64.integrate32(lift, drag, bodies, motions, props, step64.step_size(1 / 60, 1))
    assert not bad.any() and np.all(nm["angular"] == 0)
    assert np.abs(nb["rotation"].astype(np.float64) - bodies["rotation"]).max() <= BAR_R
    ident = np.arange(n) % 5 == 0
    assert np.array_equal(_bits(nb["rotation"][ident]), _bits(bodies["rotation"][ident]))        # the identity exactly


def test_constant_yaw_keeps_the_columns_orthonormal():
    n, K = 32, 16
    bodies, rng = _bodies(3, n)
    om = rng.uniform(-3, 3, n)
    motions = drag64.make_motions(np.zeros((n, 3)), np.stack([np.zeros(n), np.zeros(n), om], 1), np.zeros(n), np.zeros(n))
    props = step64.make_props(np.zeros(n), np.zeros((n, 3)), np.zeros(n), np.zeros(n))
    lift, drag = _zero(n)
    h = step64.step_size(0.1, 1)
    assert abs(float(h)) * np.abs(om).max() <= 0.5
    b, m = bodies, motions
    for _ in range(K):
        b, m, _, bad = step64.integrate32(lift, drag, b, m, props, h)
        assert not bad.any()
        R = b["rotation"].astype(np.float64).reshape(-1, 3, 3)
        gram = np.einsum("nij,nik->njk", R, R)
        assert np.abs(gram - np.eye(3)).max() <= BAR_ORTHO
        assert np.all(np.linalg.det(R) > 0.5)
    assert np.array_equal(_bits(m["angular"]), _bits(motions["angular"]))
    # it turns: x's heading moved by about K h omega (first order in h: within (h omega)^2 K)
    body = np.arange(n) % 5 == 0
    ang = np.arctan2(b["rotation"][body, 3].astype(np.float64), b["rotation"][body, 0])
    want = K * np.arctan(float(h) * om[body].astype(F).astype(np.float64))
    assert np.abs(np.angle(np.exp(1j * (ang - want)))).max() <= K * 8 * EPS * 4


def test_no_mass_no_gravity_leaves_the_velocity_and_moves_with_it():
    n = 16
    bodies, rng = _bodies(4, n)
    motions = drag64.make_motions(rng.uniform(-3, 3, (n, 3)), rng.uniform(-1, 1, (n, 3)), np.ones(n), np.ones(n))
    motions["linear"][::2] = 0
    props = step64.make_props(np.zeros(n), rng.uniform(1e-4, 1e-3, (n, 3)), 0.0, 9810.0)
    lift, drag = rng.uniform(-50, 50, (n, 8)).astype(F), rng.uniform(-50, 50, (n, 8)).astype(F)
    h = step64.step_size(1 / 60, 3)
    nb, nm, rec, bad = step64.integrate32(lift, drag, bodies, motions, props, h)
    assert not bad.any() and np.abs(rec[:, :6]).min() > 0
    assert np.array_equal(_bits(nm["linear"]), _bits(motions["linear"]))
    assert np.array_equal(_bits(nb["position"][::2]), _bits(bodies["position"][::2]))
    assert np.array_equal(_bits(nb["position"]), _bits(bodies["position"] + h * motions["linear"]))
    assert (nm["angular"] != motions["angular"]).any()


def test_planted_mistakes_are_caught():
    n = 40
    bodies, rng = _bodies(5, n)
    motions = drag64.make_motions(rng.uniform(-3, 3, (n, 3)), rng.uniform(-1, 1, (n, 3)), np.ones(n), np.ones(n))
    props = step64.make_props(rng.uniform(1e-3, 5e-3, n), rng.uniform(1e-3, 1e-2, (n, 3)), 9.81, 9810.0)
    lift, drag = rng.uniform(-5, 5, (n, 8)).astype(F), rng.uniform(-500, 500, (n, 8)).astype(F)
    lift[:, 0] = np.abs(lift[:, 0])
    h = step64.step_size(1 / 30, 1)
    right = step64.integrate32(lift, drag, bodies, motions, props, h)
    w64 = step64.integrate64(lift, drag, bodies, motions, props, h)
    # the right answer is near float64's, each mistake is far from it
    near = 1e-4
    assert np.abs(right[0]["rotation"] - w64["rotation"]).max() < near and np.abs(right[1]["angular"] - w64["angular"]).max() < near
    assert np.abs(right[0]["position"] - w64["position"]).max() < near * 200
    moved = {
        "explicit": lambda r: np.abs(r[0]["position"].astype(np.float64) - w64["position"]).max(),
        "transposed": lambda r: np.abs(r[1]["angular"].astype(np.float64) - w64["angular"]).max(),
        "by_sign": lambda r: np.abs(r[1]["angular"].astype(np.float64) - w64["angular"]).max(),
        "gs_order": lambda r: np.abs(r[0]["rotation"].astype(np.float64) - w64["rotation"]).max(),
    }
    floor = {"explicit": 1e-2, "transposed": 1e-2, "by_sign": 1e-2, "gs_order": 1e-4}
    assert set(moved) == set(step64.MISTAKES)
    for name in step64.MISTAKES:
        wrong = step64.integrate32(lift, drag, bodies, motions, props, h, mistake=name)
        assert moved[name](wrong) > floor[name], (name, moved[name](wrong))
        assert moved[name](right) < floor[name] / 10, (name, moved[name](right))
    # the flat-water box of tests/test_gpu_step.py: the step size and record layout it relies on
    assert step64.step_size(1 / 60, 2) == F(1 / 60) * (F(1) / F(2)) and step64.RECORD_FLOATS == 8 and step64.MAX_SUBSTEPS == 16
