"""datum_amd/csrc/ocean_couple.h walked on the CPU (tests/cpu/couple_emul.cpp) against tests/couple64.py, bit for bit: the rippled record, the
fourteen sums, the integrator behind them, the record's fold over a call's sub-steps and the layer after each of them.  The restatement is
built from body64, drag64, step64 and ripple64, which are pinned against their own headers; the velocity records are given.

The fleet: probe counts 0, 1, 63, 64, 65 and 200; layers of R = 64 and 128 at two origins, one body standing on the window's seam in
memory, one half outside the window (its outside probes sample 0 and drop their quanta), one wholly outside; pending deposits that a
sample must not see.  Bad bodies: a NaN cap, a NaN motion, NaN props, a NaN probe, and one that turns bad in its second sub-step (its
velocity records hold a NaN there) and so walks and deposits nothing in its third."""

import ctypes
import os

import numpy as np
import pytest

import body64
import couple64
import drag64
import ripple64
import step64
from test_body_emul import _case
from test_drag_emul import _records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
COUNTS = [0, 1, 63, 64, 65, 200, 64, 64, 30, 30, 30, 30, 30]
SEAM, HALF, OUT, BADCAP, BADMOTION, BADPROPS, BADPROBE, LATE = 5, 6, 7, 8, 9, 10, 11, 12
CELL = 0.5
CASES = [(R, o) for R in (64, 128) for o in ((37, -21), (-75, 50))]


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.couple_emul_substep.argtypes = [P, P, P, I, P, I, P, P, P, P, I, I, I, Fl, Fl, I, P]
    lib.ripple_emul_substep.argtypes = [P, P, P, I, I, I, I, Fl, Fl, P, I]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _same(got, want):
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(_bits(got)[~gn], _bits(want)[~wn])


def _fleet(R, origin, seed=11):
    rng = np.random.RandomState(seed)
    nprobes = 1400
    bodies, probes = _case(rng, COUNTS, nprobes, caps=np.where(np.arange(len(COUNTS)) % 3 == 0, np.inf, 1.5))
    # non-overlapping ranges, so that one body's bad probe is its own
    bodies["first"] = np.concatenate([[0], np.cumsum(COUNTS)[:-1]])
    ox, oy = origin
    lo = np.array([ox, oy]) * CELL
    bodies["position"][:, :2] = lo + rng.uniform(0.25, 0.75, (len(COUNTS), 2)) * R * CELL
    bodies["position"][:, 2] = rng.uniform(-0.6, 0.3, len(COUNTS))
    seam = np.array([-(-ox // R) * R, -(-oy // R) * R]) * CELL                 # the multiple of R inside the window, per axis
    assert np.all(seam > lo) and np.all(seam < lo + R * CELL)
    bodies["position"][SEAM, :2] = seam
    bodies["position"][HALF, :2] = (lo[0], lo[1] + 0.5 * R * CELL)
    bodies["position"][OUT, :2] = lo - 40.0
    bodies["cap"][BADCAP] = np.nan
    motions = drag64.make_motions(rng.uniform(-2, 2, (len(COUNTS), 3)), rng.uniform(-0.5, 0.5, (len(COUNTS), 3)), rng.uniform(0, 2, len(COUNTS)), rng.uniform(0, 2, len(COUNTS)))
    motions["angular"][BADMOTION, 1] = np.nan
    props = step64.make_props(1.0 / rng.uniform(200, 5000, len(COUNTS)), 1.0 / rng.uniform(100, 5000, (len(COUNTS), 3)), 9.81, 9810.0)
    props["gravity"][BADPROPS] = np.inf
    probes = probes.copy()
    probes[bodies["first"][BADPROBE] + 7, 1] = np.nan
    return bodies, motions, props, probes


def _layer(R, origin, seed=5):
    rng = np.random.RandomState(seed)
    lay = ripple64.Layer(R, CELL)
    lay.move(*origin)
    lay.set_window(rng.normal(size=(R, R)).astype(F) * 0.2, rng.normal(size=(R, R)).astype(F) * 0.5, rng.randint(-2 ** 18, 2 ** 18, (R, R)))
    return lay


def _recs_of(bodies, probes):
    """velocity records per sub-step: a fixed stream, the same for both sides; body LATE's hold a NaN velocity in the second sub-step"""
    rng = np.random.RandomState(77)
    off, rows = body64.offsets(bodies, len(probes))
    late = slice(int(off[LATE]), int(off[LATE]) + COUNTS[LATE])
    calls = []

    def recs(_bodies):
        r = _records(rng, rows, extremes=False)
        r[:, 2] = rng.uniform(-1.5, 1.0, rows)
        if len(calls) == 1:
            r[late, 4] = np.nan
        calls.append(1)
        return r
    return recs


def _emul_call(emul, lay, bodies, motions, props, probes, recs_of, dt, substeps):
    h, c2s2, f = ripple64.params(lay.c, lay.s, lay.gamma, lay.B, lay.sponge_gamma, dt, substeps)
    assert h == step64.step_size(dt, substeps)
    state, src = np.ascontiguousarray(lay.state(), F), lay.src.copy()
    b, m, pp, pr = bodies.copy(), motions.copy(), np.ascontiguousarray(props), np.ascontiguousarray(probes, F)
    off, _ = body64.offsets(bodies, len(probes))
    off = np.ascontiguousarray(off, np.int64)
    records = np.full((len(b), couple64.RECORD_FLOATS), -7.0, F)
    for i in range(substeps):
        recs = np.ascontiguousarray(recs_of(b), F)
        emul.couple_emul_substep(_p(b), _p(m), _p(pp), len(b), _p(pr), len(pr), _p(off), _p(recs), _p(state), _p(src), lay.R, lay.ox, lay.oy, float(lay.invs),
                                 float(h), int(i == 0), _p(records))
        out = np.empty_like(state)
        emul.ripple_emul_substep(_p(state), _p(out), _p(src), lay.R, lay.ox, lay.oy, lay.B, float(h), float(c2s2), _p(f), 1)
        state = out
        src[:] = 0
    return b, m, records, state


def _both(emul, R, origin, substeps, mistake=None, dt=None):
    bodies, motions, props, probes = _fleet(R, origin)
    dt = 0.02 * substeps if dt is None else dt
    got = _emul_call(emul, _layer(R, origin), bodies, motions, props, probes, _recs_of(bodies, probes), dt, substeps)
    lay = _layer(R, origin)
    wb, wm, wrec = couple64.call32(lay, bodies, motions, props, probes, _recs_of(bodies, probes), dt, substeps, mistake=mistake)
    return got, (wb, wm, wrec, lay.state()), (bodies, motions)


@pytest.mark.parametrize("R,origin", CASES)
@pytest.mark.parametrize("substeps", (1, 3, 16))
def test_coupled_call_bits(emul, R, origin, substeps):
    assert emul.couple_record_floats() == couple64.RECORD_FLOATS == 12 and emul.couple_fields() == 14
    (b, m, rec, state), (wb, wm, wrec, wstate), (b0, m0) = _both(emul, R, origin, substeps)
    assert np.array_equal(_bytes(b), _bytes(wb)), np.argwhere((_bytes(b) != _bytes(wb)).any(1)).ravel()
    assert np.array_equal(_bytes(m), _bytes(wm)), np.argwhere((_bytes(m) != _bytes(wm)).any(1)).ravel()
    assert _same(rec, wrec), np.argwhere(_bits(rec) != _bits(wrec))[:6]
    assert np.array_equal(_bits(state), _bits(wstate))
    # the bad ones, and only they
    bad = np.isnan(rec[:, 0])
    want = [BADCAP, BADMOTION, BADPROPS, BADPROBE] + ([LATE] if substeps > 1 else [])
    assert sorted(np.flatnonzero(bad)) == want and np.isnan(rec[bad]).all()
    for k in (BADCAP, BADMOTION, BADPROPS, BADPROBE):
        assert _bytes(b)[k].tobytes() == _bytes(b0)[k].tobytes() and _bytes(m)[k].tobytes() == _bytes(m0)[k].tobytes()
    if substeps > 1:
        # its pose is the one its last good sub-step wrote
        one = _both(emul, R, origin, 1, dt=step64.step_size(0.02 * substeps, substeps))[0]
        assert not np.isnan(one[2][LATE]).any() and _bytes(b)[LATE].tobytes() == _bytes(one[0])[LATE].tobytes() != _bytes(b0)[LATE].tobytes()
    # something happened: forces, a wake, dropped quanta at the window's edge and outside it, none inside
    good = ~bad
    assert np.abs(rec[good, :3]).max() > 1.0 and np.count_nonzero(rec[good, 8]) >= 2
    assert rec[HALF, 11] > 0 and rec[OUT, 11] > 0
    if substeps == 1:                                                          # (over many sub-steps of random water some bodies leave)
        assert rec[SEAM, 11] == 0 and rec[3, 11] == 0
    assert rec[0, 6] == 0 and np.all(rec[0, 8:] == 0)                          # no probes: no sums
    assert not np.array_equal(b["position"][good][1:], b0["position"][good][1:])


@pytest.mark.parametrize("mistake", couple64.MISTAKES)
def test_planted_mistakes_change_the_bits(emul, mistake):
    """each of the restatement's planted mistakes shows in the poses, the records or the layer (three sub-steps, so that a fold exists)"""
    (b, m, rec, state), (wb, wm, wrec, wstate), _ = _both(emul, 64, (37, -21), 3, mistake)
    differs = (not np.array_equal(_bytes(b), _bytes(wb)), not _same(rec, wrec), not np.array_equal(_bits(state), _bits(wstate)))
    assert any(differs), mistake
    if mistake == "dropped_last":
        assert differs == (False, True, False) and np.all(rec[:, :11][~np.isnan(rec[:, 0])] == wrec[:, :11][~np.isnan(wrec[:, 0])])
    else:
        assert differs[0] or differs[2], mistake


def test_fold_fields(emul):
    """field 7 is the largest residual and field 11 the sum of the dropped quanta over the call, fields 0-6 and 8-10 the last sub-step's"""
    R, origin = 64, (37, -21)
    bodies, motions, props, probes = _fleet(R, origin)
    lay = _layer(R, origin)
    recs_of = _recs_of(bodies, probes)
    singles = []
    couple64.call32(lay, bodies, motions, props, probes, recs_of, 0.02 * 3, 3, trace=singles)
    got = _both(emul, R, origin, 3)[0][2]
    good = ~np.isnan(got[:, 0])
    assert good[HALF] and not np.isnan(singles[2][good]).any()
    assert np.array_equal(got[good][:, 7], np.max([s[good][:, 7] for s in singles], 0))
    assert np.array_equal(got[good][:, 11], sum(s[good][:, 11] for s in singles)) and got[HALF, 11] > singles[2][HALF, 11]
    for k in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10):
        assert np.array_equal(_bits(got[good][:, k]), _bits(singles[2][good][:, k])), k
