"""Body drag's arithmetic (datum_amd/csrc/ocean_drag.h), the very functions ocean_drag_kernel calls, walked on the CPU
(tests/cpu/drag_emul.cpp) on random velocity records, poses, motions and ranges:

  * against drag64.reduce32, the definition of include/datum_ocean_hip.h in numpy float32: bit for bit, for the counts 0, 1, 63, 64, 65,
    129 and 1000, with water velocities of 1e-20 and 1e18 among the records and submersions on both clamps;
  * field 6 is body buoyancy's field 0 (body64.reduce32 on the same records), bit for bit;
  * every rule that makes a body bad, the eight motion fields among them, gives eight NaNs and leaves the other bodies alone;
  * against the float64 sum of the same fp32 terms: within body64.bound64, the bound of the stated order.

Where a huge record overflows a sum the definition says "what fp32 gives": an infinity has one bit pattern and is compared as such; a NaN
(inf - inf) is compared as a NaN, its payload and sign are the processor's.
"""

import ctypes
import os

import numpy as np
import pytest

import body64
import drag64
from test_body_emul import _case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
COUNTS = [0, 1, 63, 64, 65, 129, 1000]


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.drag_reduce.argtypes = [P, P, I, P, I, P, P, P]
    return lib


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, want):
    """bit for bit; a NaN against a NaN"""
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(_bits(got)[~gn], _bits(want)[~wn])


def _motions(rng, nb):
    """linear within 3 m/s, angular within 1 rad/s, cl and cq in [0, 2]; every fourth body without cq, every fifth without cl, every
    seventh fully at rest"""
    b = np.arange(nb)
    m = drag64.make_motions(rng.uniform(-3, 3, (nb, 3)), rng.uniform(-1, 1, (nb, 3)), rng.uniform(0, 2, nb), rng.uniform(0, 2, nb))
    m["cq"][b % 4 == 1] = 0
    m["cl"][b % 5 == 2] = 0
    rest = b % 7 == 3
    m["linear"][rest], m["angular"][rest] = 0, 0
    return m


def _records(rng, rows, extremes=True):
    """velocity records as a query could give them: position, height near the probes' depths, a residual, the water's velocity, 0; with
    `extremes` every 53rd a velocity of 1e-20 (its square is not an fp32 number), every 97th one of 1e18 (its square is near the top)"""
    r = np.zeros((rows, 8), F)
    r[:, :2] = rng.uniform(-60, 60, (rows, 2))
    r[:, 2] = rng.uniform(-4, 3, rows)
    r[:, 3] = rng.uniform(0, 1e-3, rows)
    r[:, 4:7] = rng.normal(size=(rows, 3)) * (2.0, 2.0, 1.0)
    if extremes:
        r[::53, 4:7] = rng.choice([-1.0, 1.0], (len(r[::53]), 3)) * 1e-20
        r[::97, 4:7] = rng.choice([-1.0, 1.0], (len(r[::97]), 3)) * 1e18
    return r


def _emul(emul, bodies, motions, probes, recs):
    off, rows = body64.offsets(bodies, len(probes))
    assert len(recs) == rows and len(motions) == len(bodies)
    bodies, motions = np.ascontiguousarray(bodies), np.ascontiguousarray(motions)
    probes, recs = np.ascontiguousarray(probes, F), np.ascontiguousarray(recs, F)
    out = np.full((len(bodies), 8), -7.0, F)
    emul.drag_reduce(bodies.ctypes.data, motions.ctypes.data, len(bodies), probes.ctypes.data, len(probes), off.ctypes.data, recs.ctypes.data, out.ctypes.data)
    return out


def test_counts_bit_for_bit(emul):
    rng = np.random.RandomState(21)
    counts = COUNTS * 6
    bodies, probes = _case(rng, counts)
    motions = _motions(rng, len(counts))
    # bodies at rest in water of 1e-20: nothing but the tiny velocity in e
    still = (np.arange(len(counts)) % 7 == 3)
    recs = _records(rng, body64.offsets(bodies, len(probes))[1])
    got = _emul(emul, bodies, motions, probes, recs)
    want = drag64.reduce32(bodies, motions, probes, recs)
    assert _same(got, want), np.argwhere(_bits(got) != _bits(want))[:6]
    assert np.all(got[0] == 0) and not np.signbit(got[0]).any()            # count == 0: eight +0.0
    assert still.any() and (motions["cq"] == 0).any() and (motions["cl"] == 0).any()

    # both clamps are met: dry probes (d = 0), capped ones (d = cap) and some between
    bi, _ = body64._gather(bodies, probes)
    w, _, _ = body64.world32(bodies, probes)
    raw = recs[:, 2] - w[:, 2]
    cap = bodies["cap"][bi]
    assert (raw <= 0).any() and (raw >= cap).any() and ((raw > 0) & (raw < cap)).any()
    # the tiny velocity is not flushed: a body at rest, cq = 0, feels cl m 1e-20
    t = drag64.terms32(bodies, motions, probes, recs)
    tiny = np.zeros(len(recs), bool)
    tiny[::53] = True
    sel = tiny & still[bi] & (t[:, 6] > 0) & (motions["cl"][bi] > 0)
    assert sel.any() and np.all(np.abs(t[sel, :3]) > 0) and np.all(np.abs(t[sel, :3]) < 1e-18)
    # ... and the huge one is felt, its force finite (m cq s e < 20 * 2 * 1.8e18 * 1e18)
    huge = np.zeros(len(recs), bool)
    huge[::97] = True
    sel = huge & (t[:, 6] > 0) & (motions["cq"][bi] > 0)
    assert sel.any() and np.isfinite(t[sel, :3]).all() and np.abs(t[sel, :3]).max() > 1e30

    # field 6 is buoyancy's field 0 on the same records (only rec[2] is read for it)
    assert np.array_equal(_bits(got[:, 6]), _bits(body64.reduce32(bodies, probes, recs)[:, 0]))


def test_bad_bodies_and_bad_motions(emul):
    rng = np.random.RandomState(22)
    counts = [10, 64, 70, 5, 130, 7, 64, 20, 9, 65, 3, 40, 40, 40, 40, 40, 40, 40, 40, 12]
    bodies, probes = _case(rng, counts, nprobes=900)
    bodies["first"][:] = np.arange(len(counts)) * 40
    motions = _motions(rng, len(counts))
    recs = _records(rng, body64.offsets(bodies, len(probes))[1], extremes=False)
    clean = _emul(emul, bodies, motions, probes, recs)
    assert np.isfinite(clean).all()

    bad, mb = bodies.copy(), motions.copy()
    bad["first"][1] = -1
    bad["count"][3] = -5
    bad["cap"][4] = np.nan
    bad["position"][8, 2] = -np.inf
    bad["rotation"][9, 4] = np.nan
    fields = [("linear", 0), ("linear", 1), ("linear", 2), ("angular", 0), ("angular", 1), ("angular", 2), ("cl", None), ("cq", None)]
    values = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf, np.nan]
    for b, ((name, k), v) in zip(range(11, 19), zip(fields, values)):
        if k is None:
            mb[name][b] = v
        else:
            mb[name][b, k] = v
    victims = [1, 3, 4, 8, 9] + list(range(11, 19))
    # the per-probe rows move where a range is bad: records by body from the clean layout
    off0, _ = body64.offsets(bodies, len(probes))
    off1, rows1 = body64.offsets(bad, len(probes))
    recs1 = np.zeros((rows1, 8), F)
    for b in range(len(counts)):
        if not body64.range_bad(bad, len(probes))[b]:
            recs1[off1[b]:off1[b] + counts[b]] = recs[off0[b]:off0[b] + counts[b]]
    got = _emul(emul, bad, mb, probes, recs1)
    assert np.isnan(got[victims]).all()
    keep = np.setdiff1d(np.arange(len(counts)), victims)
    assert np.array_equal(_bits(got[keep]), _bits(clean[keep]))
    assert _same(got, drag64.reduce32(bad, mb, probes, recs1))
    assert drag64.motion_bad(mb).nonzero()[0].tolist() == list(range(11, 19))

    # a bad probe spoils exactly the bodies whose range holds it
    pb = probes.copy()
    pb[6 * 40 + 63, 3] = np.nan
    got = _emul(emul, bodies, motions, pb, recs)
    f, c = bodies["first"].astype(int), bodies["count"].astype(int)
    hit = (f <= 303) & (303 < f + c)
    assert hit.any() and not hit.all()
    assert np.isnan(got[hit]).all() and np.array_equal(_bits(got[~hit]), _bits(clean[~hit]))


def test_against_the_float64_sum_of_the_same_terms(emul, report):
    rng = np.random.RandomState(23)
    counts = [1, 2, 31, 33, 63, 64, 65, 100, 128, 129, 200, 640, 1000] * 3
    bodies, probes = _case(rng, counts, nprobes=1400, caps=rng.uniform(0.5, 1.5, len(counts)))
    motions = _motions(rng, len(counts))
    recs = _records(rng, body64.offsets(bodies, len(probes))[1], extremes=False)
    got = _emul(emul, bodies, motions, probes, recs).astype(np.float64)
    t = drag64.terms32(bodies, motions, probes, recs).astype(np.float64)
    bi, _ = body64._gather(bodies, probes)
    want, mag = np.zeros((len(bodies), 8)), np.zeros((len(bodies), 8))
    np.add.at(want[:, :7], bi, t[:, :7])
    np.add.at(mag[:, :7], bi, np.abs(t[:, :7]))
    np.maximum.at(want[:, 7], bi, t[:, 7])
    bar = body64.bound64(bodies, mag)
    err = np.abs(got - want)
    ok = bar[:, :7] > 0
    assert np.all(err[:, :7][~ok] == 0)
    worst = float((err[:, :7][ok] / bar[:, :7][ok]).max())
    report(f"drag: header against the float64 sum of the same terms: worst |error| / bound {worst:.3f}")
    assert worst <= 1.0
    assert np.array_equal(got[:, 7], want[:, 7])                           # a maximum does not round
