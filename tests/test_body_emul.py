"""Body buoyancy's arithmetic (datum_amd/csrc/ocean_body.h), the very functions ocean_body_kernel calls, walked on the CPU
(tests/cpu/body_emul.cpp) on random records, poses and ranges:

  * against body64.reduce32, the definition of include/datum_ocean_hip.h in numpy float32: bit for bit, for every count in 0 ... 200 and
    for 1000, for ranges that share probes and for every rule that makes a body bad;
  * against the float64 sum of the same fp32 terms: within (ceil(count / 64) + 6) 2^-24 sum |term|, the bound of the stated order (a
    lane's chain of ceil(count / 64) additions, then the tree's six), not a measured figure;
  * planted mistakes (body64's `mistake`) break that comparison by far more than the bound.
"""

import ctypes
import os

import numpy as np
import pytest

import body64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.body_world.argtypes = [P, I, P, I, P, P, P]
    lib.body_reduce.argtypes = [P, I, P, I, P, P, P]
    return lib


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _probes(rng, n):
    p = rng.uniform(-3, 3, (n, 4)).astype(F)
    p[:, 3] = rng.uniform(0.05, 2.0, n)
    return p


def _case(rng, counts, nprobes=1400, caps=None):
    """bodies with random poses whose ranges start anywhere they fit (so they overlap), the identity pose among them"""
    nb = len(counts)
    rot = [np.eye(3) if b % 5 == 0 else _rotation(rng) for b in range(nb)]
    pos = rng.uniform(-50, 50, (nb, 3))
    pos[:, 2] = rng.uniform(-2, 1, nb)
    firsts = [int(rng.randint(0, nprobes - c + 1)) for c in counts]
    if caps is None:
        caps = np.where(rng.uniform(size=nb) < 0.3, np.inf, rng.uniform(0.2, 2.0, nb))
    return body64.make_bodies(rot, pos, firsts, counts, caps), _probes(rng, nprobes)


def _records(rng, rows):
    """surface records as a query could give them: height near the probes' depths, a residual, a unit normal, foam"""
    r = np.empty((rows, 8), F)
    r[:, :2] = rng.uniform(-60, 60, (rows, 2))
    r[:, 2] = rng.uniform(-4, 3, rows)
    r[:, 3] = rng.uniform(0, 1e-3, rows)
    n = rng.normal(size=(rows, 3)) * (0.3, 0.3, 0) + (0, 0, 1)
    r[:, 4:7] = n / np.linalg.norm(n, axis=1, keepdims=True)
    r[:, 7] = rng.uniform(0, 1, rows)
    return r


def _emul(emul, bodies, probes, recs):
    off, rows = body64.offsets(bodies, len(probes))
    assert len(recs) == rows
    bodies, probes, recs = np.ascontiguousarray(bodies), np.ascontiguousarray(probes, F), np.ascontiguousarray(recs, F)
    out = np.full((len(bodies), 8), -7.0, F)
    emul.body_reduce(bodies.ctypes.data, len(bodies), probes.ctypes.data, len(probes), off.ctypes.data, recs.ctypes.data, out.ctypes.data)
    return out


def test_transform_is_the_definition(emul):
    rng = np.random.RandomState(1)
    bodies, probes = _case(rng, [0, 1, 63, 64, 65, 129, 1000])
    off, rows = body64.offsets(bodies, len(probes))
    w, bad = np.zeros((rows, 3), F), np.ones(rows, np.uint8)
    emul.body_world(bodies.ctypes.data, len(bodies), probes.ctypes.data, len(probes), off.ctypes.data, w.ctypes.data, bad.ctypes.data)
    want, _, wbad = body64.world32(bodies, probes)
    assert np.array_equal(_bits(w), _bits(want))
    assert not bad.any() and not wbad.any()


def test_every_count_bit_for_bit(emul):
    rng = np.random.RandomState(2)
    counts = list(range(201)) + [1000]
    bodies, probes = _case(rng, counts)
    recs = _records(rng, body64.offsets(bodies, len(probes))[1])
    got = _emul(emul, bodies, probes, recs)
    want = body64.reduce32(bodies, probes, recs)
    assert np.isfinite(got).all()
    assert np.all(got[0] == 0) and not np.signbit(got[0]).any()            # count == 0: eight +0.0
    assert np.array_equal(_bits(got), _bits(want))
    # ranges overlap: the same probe under two poses
    f, c = bodies["first"].astype(int), bodies["count"].astype(int)
    assert any(f[i] < f[j] + c[j] and f[j] < f[i] + c[i] for i in range(100, 110) for j in range(110, 120))


def test_bad_bodies(emul):
    rng = np.random.RandomState(3)
    counts = [10, 64, 70, 5, 130, 7, 64, 20, 9, 65, 3]
    bodies, probes = _case(rng, counts, nprobes=600)
    bodies["first"][:] = np.arange(len(counts)) * 40
    bodies["first"][1], bodies["first"][2] = -1, 600 - 69                   # first < 0; first + count = nprobes + 1
    bodies["count"][3] = -5
    bodies["cap"][4] = np.nan
    bodies["first"][5], bodies["count"][5] = 2 ** 31 - 1, 2 ** 31 - 1       # first + count overflows an int
    probes[6 * 40 + 63, 3] = np.nan                                         # a weight
    probes[7 * 40 + 2, 0] = np.inf                                          # a coordinate: w not finite
    bodies["position"][8, 2] = -np.inf
    bodies["rotation"][9, 4] = np.nan
    expect_bad = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert body64.range_bad(bodies, len(probes)).nonzero()[0].tolist() == [1, 2, 3, 4, 5]
    recs = _records(rng, body64.offsets(bodies, len(probes))[1])
    got = _emul(emul, bodies, probes, recs)
    want = body64.reduce32(bodies, probes, recs)
    assert np.isnan(got[expect_bad]).all()
    good = np.setdiff1d(np.arange(len(counts)), expect_bad)
    # body 6's bad probes (280 + 63 and body 7's 282) lie inside bodies 6 and 7 only: first = 40 b, so bodies 5 ... cover them too
    good = [b for b in good if np.isfinite(want[b]).all()]
    assert 0 in good and 10 in good
    assert np.isfinite(got[good]).all()
    assert np.array_equal(_bits(got), _bits(want))
    # a cap of +inf is none, a cap of 0 leaves nothing
    bodies2, probes2 = _case(rng, [100, 100], caps=[np.inf, 0.0])
    recs2 = _records(rng, 200)
    r = _emul(emul, bodies2, probes2, recs2)
    assert r[0, 0] > 0 and np.all(r[1, :7] == 0)
    assert np.array_equal(_bits(r), _bits(body64.reduce32(bodies2, probes2, recs2)))


def _ratio(got, want, bar):
    """worst |got - want| / bar over the summed fields, where the bar is not zero"""
    d = np.abs(got.astype(np.float64)[:, :7] - want[:, :7])
    ok = bar[:, :7] > 0
    if np.any(d[~ok] != 0):
        return np.inf                              # off where every term is zero
    return float((d[ok] / bar[:, :7][ok]).max())


def test_against_float64_and_planted_mistakes(emul, report):
    rng = np.random.RandomState(4)
    counts = [1, 2, 31, 33, 63, 64, 65, 100, 128, 129, 200, 640, 1000] * 3
    bodies, probes = _case(rng, counts, nprobes=1400, caps=rng.uniform(0.5, 1.5, len(counts)))
    bodies["first"][:] = np.maximum(bodies["first"], 3)                    # "no_first" must move every range
    bodies["first"][:] = np.minimum(bodies["first"], 1400 - bodies["count"])
    recs = _records(rng, body64.offsets(bodies, len(probes))[1])
    got = _emul(emul, bodies, probes, recs)
    want, mag = body64.sum64(bodies, probes, recs)
    bar = body64.bound64(bodies, mag)
    worst = _ratio(got, want, bar)
    report(f"body: header against the float64 sum of the same terms: worst |error| / bound {worst:.3f}")
    assert worst <= 1.0
    assert np.array_equal(got[:, 7].astype(np.float64), want[:, 7])          # a maximum does not round

    # each planted mistake, against the same float64 sums, in units of the same bound
    multi = bodies["count"] > 32
    for mistake in ("tau_sign", "no_clamp", "no_cap", "world_arm", "no_first", "stride32"):
        wrong = body64.reduce32(bodies, probes, recs, mistake)
        sel = multi if mistake == "stride32" else np.ones(len(bodies), bool)
        r = _ratio(wrong[sel], want[sel], bar[sel])
        report(f"body: planted {mistake}: {r:.3g} bounds")
        assert r > 1000.0, (mistake, r)
