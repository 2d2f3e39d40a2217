"""The CPU half of the step side's sequence tests (tests/step_seq.py; the GPU half is tests/test_gpu_step_sequences.py): the sequences
are shown to have teeth before any of them runs on a GPU.

  determinism   sequence(seed, n) twice gives the same list, and a model run twice the same observables;
  coverage      over the committed seeds, from the TRUE model's log alone: every call family in three seeds, every refusal the header names
                three times, every row-pass form in three seeds, more than 32 updates without a displace three times, a displace between
                changes of the format, the literal mode, velocity and the phase store pairwise, a resume into another cascade, a parked
                and resumed state outside the range, every mark set and cleared by the calls that should and by no other;
  refusals      a refused call leaves every observable as it was;
  teeth         every planted mistake of step_seq.MISTAKES parts from the true model on a committed seed;
  the bars      the fp32 oracle on the model's state at every displace stays within a third of the bar the GPU test holds the device to.
"""

import functools
import itertools

import numpy as np
import pytest

import pointwise as pw
import ref64
import step_seq as sq
from oracle import oracle
from test_gpu_pointwise import K_MAP, K_NORMAL

F32 = np.float32
SIZES = (64, 128)
CHANGES = {"set_spectrum_format": "format", "set_literal_transform": "literal", "set_velocity": "velocity", "set_phase_store": "store"}


def _marks(m):
    return dict(bounds=m.bounds_current, velocity=m.velocity_current, **{f"quadrant{c}": s.quadrant for c, s in enumerate(m.casc)})


def _reference_k(m):
    """worst (displacement K, normal K) of the fp32 oracle against float64 over the cascades of a model that has just displaced"""
    kd = kn = 0.0
    for c, s in enumerate(m.casc):
        got = ref64.channels(m.oracle_maps(c))
        scale = F32(1) / F32(s.wavescale)
        if m.literal:
            ref, ln = ref64.lit64(s.h0, s.phase, scale, s.chop, oracle.weights(m.N), return_len=True)
        else:
            ref, ln = ref64.displace64(s.h0, s.phase, scale, s.chop, return_len=True)
        d, n, _ = pw.pointwise(got, ref, ln, m.N)
        kd, kn = max(kd, d), max(kn, n)
    return kd, kn


def run(seed, N=64, mistake=None, reference=False, ops=None):
    """the sequence on a model: one record per operation"""
    ops = sq.sequence(seed, sq.LENGTH) if ops is None else ops
    m, log = sq.Model(N, mistake=mistake), []
    for k, op in enumerate(ops):
        rec = dict(k=k, name=op[0], args=op[1], marks_before=_marks(m))
        keep = (sq.observe(m), sq.hidden(m)) if mistake is None else None
        n, flushes = len(m.trace), m.update_flushes
        rec["code"] = sq.apply(m, op)
        rec["refused"] = m.refused
        rec["trace"] = tuple(m.trace[n:])
        rec["update_flushed"] = m.update_flushes > flushes
        rec["marks_after"] = _marks(m)
        rec["observed"] = sq.observe(m)
        rec["unchanged"] = keep is None or rec["code"] == sq.OK or (rec["observed"], sq.hidden(m)) == keep
        rec["state"] = dict(literal=m.literal, format=m.format, profile=m.profile, foam=m.foam_mode, velocity=m.velocity, seed=m.seed_held, store=m.store)
        if op[0] == "park_state" and rec["code"] == sq.OK:
            rec["parked"] = (op[1][0], m.parked[op[1][1]][2])
        if reference and op[0] == "displace" and rec["code"] == sq.OK:
            rec["ref_k"] = _reference_k(m)
        log.append(rec)
    return log


@functools.lru_cache(maxsize=None)
def true_log(seed, N=64, reference=False):
    return run(seed, N, reference=reference)


def _refusal(r, before):
    """the header's name for a refusal, from the call and the state it met"""
    name, a = r["name"], r["args"]
    if name == "displace":
        return "displace without a state"
    if name == "upload_height":
        return "upload_height without a state"
    if name == "park_state":
        return "park_state without a state"
    if name == "rebuild_height":
        if a[0] >= 3:
            return "rebuild_height cascade out of range"
        if not before["seed"]:
            return "rebuild_height without a seed"
        return "rebuild_height wavescale" if not a[1] > 0 else "rebuild_height amplitude" if not (0 <= a[2] < sq.INF) else "rebuild_height wind"
    if name == "set_spectrum_format":
        return "set_spectrum_format while profiling" if before["profile"] else "set_spectrum_format in the literal mode"
    if name == "set_literal_transform":
        return "set_literal_transform while profiling" if before["profile"] else "set_literal_transform with an fp16 spectrum"
    if name in ("set_phase_writeback", "set_phase_store", "set_cascade_group", "set_map_store_policy"):
        return "a launch-plan setter while profiling"
    if name == "set_foam_params":
        return "set_foam_params not finite" if sq.INF in a else "set_foam_params negative"
    if name == "reset_foam":
        return "reset_foam while foam is off"
    if name == "profile_end":
        return "profile_end without a profile"
    if name == "profile_begin":
        return "profile_begin in the literal mode"
    return "unexpected " + name


# the refusals the header names for these calls (park_state's and profile_begin's are the code's: allowed, not required)
REFUSALS = ("displace without a state", "upload_height without a state", "rebuild_height cascade out of range", "rebuild_height without a seed",
            "rebuild_height wavescale", "rebuild_height amplitude", "rebuild_height wind", "set_spectrum_format while profiling",
            "set_spectrum_format in the literal mode", "set_literal_transform while profiling", "set_literal_transform with an fp16 spectrum",
            "a launch-plan setter while profiling", "set_foam_params not finite", "set_foam_params negative", "reset_foam while foam is off",
            "profile_end without a profile")
ALLOWED = ("park_state without a state", "profile_begin in the literal mode")

# who sets and who clears each mark: the header ("surface bounds", "surface velocity", datum_ocean_set_phase_store) and, for the quadrant
# bits, the comments of ocean_capi.hip (zero_phase, inspect_phase, settle_phase_store) as step_seq's docstring restates them
MAKES = {"bounds": {"reduce_bounds"}, "velocity": {"displace"}, "quadrant": {"upload_state", "resume_state", "set_phase_store", "rebuild_height"}}
CLEARS = {"bounds": {"displace", "bind_maps"}, "velocity": {"set_velocity", "bind_velocity"},
          "quadrant": {"displace", "set_phase_store", "upload_state", "resume_state"}}


def coverage(logs):
    families, forms, refusals = {}, {}, dict.fromkeys(REFUSALS, 0)
    made, cleared = {k: set() for k in MAKES}, {k: set() for k in CLEARS}
    bits = {}
    pairs = set()
    long_queues = update_flushes = other_cascade = wild_roundtrip = 0
    for seed, log in logs.items():
        before = dict(literal=False, format=sq.FP32, profile=False, foam=sq.FOAM_OFF, velocity=False, seed=False, store=sq.AUTO)
        parked = {}
        since = 0
        last_change = {}                                                           # kind -> displaces seen when it last changed
        displaces = 0
        for r in log:
            name, code = r["name"], r["code"]
            families.setdefault(name, set()).add(seed)
            for first, form in r["trace"]:
                forms.setdefault(form, set()).add(seed)
                if first:
                    forms.setdefault("advance first", set()).add(seed)
            if code != sq.OK:
                what = _refusal(r, before)
                refusals[what] = refusals.get(what, 0) + 1
            if name == "update":
                since += r["args"][1]
                update_flushes += r["update_flushed"]
            if name == "displace" and code == sq.OK:
                long_queues += since > 32
                since = 0
                displaces += 1
            for mark, b in r["marks_before"].items():
                a = r["marks_after"][mark]
                kind = "quadrant" if mark.startswith("quadrant") else mark
                if a != b:
                    (made if a else cleared)[kind].add(name)
                    bits.setdefault(mark, set()).add(a)
            if name in CHANGES and code == sq.OK and r["state"] != before:
                kind = CHANGES[name]
                for other, at in last_change.items():
                    if other != kind and displaces > at:
                        pairs.add(frozenset((kind, other)))
                last_change[kind] = displaces
            if "parked" in r:
                parked[r["args"][1]] = r["parked"]
            if name == "resume_state" and code == sq.OK:
                c, flags = parked[r["args"][1]]
                other_cascade += c != r["args"][0]
                wild_roundtrip += flags & 1
            before = r["state"]
    return dict(families=families, forms=forms, refusals=refusals, made=made, cleared=cleared, bits=bits, pairs=pairs, long_queues=long_queues,
                update_flushes=update_flushes, other_cascade=other_cascade, wild_roundtrip=wild_roundtrip)


FAMILIES = ("update", "displace", "set_cascade", "upload_state", "upload_height", "upload_seed", "rebuild_height", "park_state", "resume_state", "read_state",
            "read_height", "set_spectrum_format", "set_literal_transform", "set_phase_store", "set_phase_writeback", "set_cascade_group", "set_map_store_policy",
            "set_foam", "set_foam_params", "reset_foam", "bind_foam", "set_velocity", "bind_velocity", "bind_maps", "reduce_bounds", "profile_begin",
            "profile_end", "set_stream")


def check(c):
    """the coverage conditions, as a list of what is missing"""
    missing = [f"family {f}: {sorted(c['families'].get(f, ()))}" for f in FAMILIES if len(c["families"].get(f, ())) < 3]
    missing += [f"form {f}: {sorted(c['forms'].get(f, ()))}" for f in sq.FORMS + ("advance first",) if len(c["forms"].get(f, ())) < 3]
    missing += [f"refusal {k}: {n}" for k, n in c["refusals"].items() if (n < 3 if k in REFUSALS else k not in ALLOWED)]
    for mark in MAKES:
        if c["made"][mark] != MAKES[mark]:
            missing.append(f"{mark} set by {sorted(c['made'][mark])}")
        if c["cleared"][mark] != CLEARS[mark]:
            missing.append(f"{mark} cleared by {sorted(c['cleared'][mark])}")
    missing += [f"{m} never {'set' if v else 'cleared'}" for m in ("bounds", "velocity", "quadrant0", "quadrant1", "quadrant2") for v in (True, False) if v not in c["bits"].get(m, ())]
    missing += [f"no displace between {a} and {b}" for a, b in itertools.combinations(sorted(set(CHANGES.values())), 2) if frozenset((a, b)) not in c["pairs"]]
    missing += [f"{k}: {c[k]}" for k, n in (("long_queues", 3), ("update_flushes", 3), ("other_cascade", 1), ("wild_roundtrip", 1)) if c[k] < n]
    return missing


def test_determinism():
    for seed in sq.SEEDS[:3]:
        a, b = sq.sequence(seed, sq.LENGTH), sq.sequence(seed, sq.LENGTH)
        assert a == b and len(a) >= sq.LENGTH
        np.random.seed(seed + 1)                                              # the global generator is not what it draws from
        assert sq.sequence(seed, sq.LENGTH) == a
        assert [r["observed"] for r in run(seed)] == [r["observed"] for r in true_log(seed)]
    assert sq.sequence(sq.SEEDS[0], sq.LENGTH) != sq.sequence(sq.SEEDS[1], sq.LENGTH)
    assert len(set(sq.SEEDS)) == len(sq.SEEDS) == 12
    for seed in sq.PLAN_SEEDS:
        ops = sq.sequence(seed, sq.PLAN_LENGTH, C=2, plan_only=True)
        assert ops == sq.sequence(seed, sq.PLAN_LENGTH, C=2, plan_only=True)
        assert {o[0] for o in ops} <= set(sq.PLAN) | {"set_cascade", "upload_state", "update", "displace"}
        assert len(ops) == 4 + sq.PLAN_LENGTH or (len(ops) <= 4 + sq.PLAN_LENGTH + 2 and ops[-1][0] == "displace")


def test_coverage():
    c = coverage({seed: true_log(seed) for seed in sq.SEEDS})
    print({k: (sorted(map(sorted, v)) if k == "pairs" else v) for k, v in c.items() if k not in ("families", "forms")})
    print({f: len(s) for f, s in c["families"].items()}, {f: len(s) for f, s in c["forms"].items()})
    assert not check(c), check(c)


def test_a_refused_call_changes_nothing():
    refused = [(seed, r["k"], r["name"]) for seed in sq.SEEDS for r in true_log(seed) if r["code"] != sq.OK]
    assert len(refused) >= 3 * len(REFUSALS)
    assert not [(seed, r["k"], r["name"]) for seed in sq.SEEDS for r in true_log(seed) if not r["unchanged"]]
    for seed in sq.SEEDS:
        for r in true_log(seed):
            assert (r["code"] == sq.OK) == (r["refused"] is None) and (r["refused"] is None or r["refused"] == "datum_ocean_" + r["name"]), (seed, r["k"])


@pytest.mark.parametrize("mistake", sq.MISTAKES)
def test_teeth(mistake):
    """the mistaken model and the true one run the same sequence; the first operation behind which an observable or the trace differs"""
    seen = {}
    for seed in sq.SEEDS:
        for t, r in zip(true_log(seed), run(seed, mistake=mistake)):
            what = [k for k in t["observed"] if t["observed"][k] != r["observed"][k]] + (["trace"] if t["trace"] != r["trace"] else []) + (["code"] if t["code"] != r["code"] else [])
            if what:
                seen[seed] = (r["k"], r["name"], what)
                break
    print(mistake, seen)
    assert seen, f"no committed seed sees the planted mistake {mistake!r}"


@functools.lru_cache(maxsize=None)
def _reference_worst():
    worst = {"fused": [0.0, 0.0], "literal": [0.0, 0.0]}
    n = 0
    for N in SIZES:
        for seed in sq.SEEDS:
            for r in true_log(seed, N, True):
                if "ref_k" in r:
                    w = worst["literal" if r["state"]["literal"] else "fused"]
                    w[0], w[1] = max(w[0], r["ref_k"][0]), max(w[1], r["ref_k"][1])
                    n += 1
    print(f"reference worst K over {n} displaces: fused disp {worst['fused'][0]:.3f} (bar {K_MAP} / 3), normal {worst['fused'][1]:.3f} (bar {K_NORMAL} / 3); "
          f"literal disp {worst['literal'][0]:.3f} (bar {pw.K_LIT_DISP:.2f} / 3), normal {worst['literal'][1]:.3f} (bar {pw.K_LIT_NORMAL:.2f} / 3)")
    return worst, n


def test_the_reference_sets_the_literal_bars():
    """oracle.displace with oracle.weights(N) on the model's state against lit64 at every literal displace of every committed seed and both
    sizes: the worst K at or below a third of K_LIT_DISP / K_LIT_NORMAL, the bars tests/test_gpu_step_sequences.py holds the device to.
    Measured: displacement 2.17 of 2.24, normals 1.40 of 2.17"""
    worst, n = _reference_worst()
    assert n >= 60 and worst["literal"][0] > 0
    assert worst["literal"][0] <= pw.K_LIT_DISP / 3 and worst["literal"][1] <= pw.K_LIT_NORMAL / 3, worst


def test_the_reference_sets_the_fused_bars():
    """The same for the fused step: oracle.displace on the table's exact values rounded to fp32 (step_seq.Model.oracle_maps says why not
    oracle.weights(N, reduced=True)) against displace64, a third of K_MAP / K_NORMAL.  Measured: displacement 2.68 of 3, normals 1.52 of 2.
    The reference's own worst texel varies from sea to sea, 1.7 to 3.1: step_seq.SCALES and step_seq.H0_SEEDS say what sequence draws for
    that reason; the bars are as tests/test_gpu_pointwise.py states them"""
    worst, _ = _reference_worst()
    assert worst["fused"][0] <= K_MAP / 3 and worst["fused"][1] <= K_NORMAL / 3, worst
