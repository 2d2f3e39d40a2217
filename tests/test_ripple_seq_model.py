"""The CPU half of the ripple layer's sequence tests (tests/ripple_seq.py; the GPU half is tests/test_gpu_ripple_sequences.py): the
sequences are shown to have teeth before any of them runs on a GPU.

  determinism   sequence(seed, n) twice gives the same list, and reads nothing but its arguments;
  coverage      over the committed seeds, from the TRUE model's trace alone (no device code is consulted): every step family in three
                seeds, stale-swell steps, swell with nothing solid, every mark set and cleared by every call the header names, every
                documented refusal twice, set_ripples to another R under walls, bed, swell and foam, a seam-wrapping scroll under walls
                and over a bed;
  refusals      a refused call leaves every observable and every parameter as it was;
  teeth         every planted mistake of ripple_seq.MISTAKES parts from the true model in its observables on a committed seed;
  float64       every step of every sequence stays within its family's K of the float64 form started from the same fp32 state.
"""

import functools

import numpy as np
import pytest

import ripple_seq as rq

WAVE, DEEP = rq.WAVE, rq.DEEP
STEPS = ("step_ripples", "step_bodies_coupled_host")


def _flags(m):
    L = m.layer
    if L is None:
        return dict(R=0, walls=False, bed=False, swell=False, foam=False, mode=m.mode, origin=None)
    return dict(R=L.R, walls=L.wall is not None, bed=L.bed is not None, swell=L.F is not None, foam=m.foam is not None, mode=L.mode, origin=(L.ox, L.oy))


def _params(m):
    L = m.layer
    return (m.c, m.gamma, m.B, m.sponge_gamma, m.mode, m.g) + (() if L is None else (L.c, L.gamma, L.B, L.sponge_gamma, L.mode, L.g, L.ox, L.oy, L.src.tobytes()))


def run(seed, length=None, mistake=None, distances=False):
    """the sequence on a model: a list of one record per operation"""
    ops = rq.sequence(seed, rq.LENGTH if length is None else length)
    m, sea, log = rq.Model(mistake=mistake), rq.Sea(), []
    for k, op in enumerate(ops):
        rec = dict(k=k, name=op[0], args=op[1], before=_flags(m), marks_before=m.marks())
        if distances and op[0] in STEPS and m.layer is not None and m.stable(op[1][-2], op[1][-1]) and (op[0] == "step_ripples" or not op[1][1]):
            rec["distance"] = m.distance64(op[1][-2], op[1][-1], every_first=op[0] != "step_ripples")
        keep = (rq.observe(m), _params(m)) if mistake is None else None
        n = len(m.families)
        rec["code"], _ = rq.apply(m, op, sea)
        rec["families"] = tuple(m.families[n:])
        rec["after"], rec["marks_after"] = _flags(m), m.marks()
        rec["observed"] = rq.observe(m)
        rec["unchanged"] = keep is None or rec["code"] == rq.OK or (rq.observe(m), _params(m)) == keep
        log.append(rec)
    return log


@functools.lru_cache(maxsize=None)
def true_log(seed):
    return run(seed, distances=True)


def coverage(logs):
    """the coverage figures of {seed: log}, every one from the model's own trace and switches"""
    fam = {f: set() for f in rq.FAMILIES}
    cleared = {"bounds": set(), "swell": set(), "fft": set()}
    made = {"bounds": set(), "swell": set(), "fft": set()}
    refusals = dict.fromkeys(("deep_with_bed", "deep_with_swell", "bed_in_deep", "swell_in_deep", "unstable_wave", "unstable_deep", "unstable_bed"), 0)
    other_R = dict.fromkeys(("walls", "bed", "swell", "foam"), 0)
    wrap = dict.fromkeys(("walls", "bed"), 0)
    stale = unsolid = unexpected = 0
    for seed, log in logs.items():
        for r in log:
            b, a, name, code = r["before"], r["after"], r["name"], r["code"]
            for f in r["families"]:
                fam[f].add(seed)
            for k, mark in enumerate(("bounds", "swell", "fft")):
                if r["marks_before"][k] and not r["marks_after"][k]:
                    cleared[mark].add(name)
                if not r["marks_before"][k] and r["marks_after"][k]:
                    made[mark].add(name)
            if name in STEPS and code == rq.OK and b["swell"]:
                stale += (not r["marks_before"][1]) and (b["walls"] or b["bed"])
                unsolid += r["marks_before"][1] and not (b["walls"] or b["bed"])
            if code != rq.OK:
                if name == "set_ripple_dispersion" and code == rq.ESTATE:
                    refusals["deep_with_bed" if b["bed"] else "deep_with_swell"] += 1
                elif name == "set_ripple_bed" and code == rq.ESTATE:
                    refusals["bed_in_deep"] += 1
                elif name == "set_ripple_swell" and code == rq.ESTATE:
                    refusals["swell_in_deep"] += 1
                elif name in STEPS and code == rq.EINVAL:
                    refusals["unstable_deep" if b["mode"] == DEEP else "unstable_bed" if b["bed"] else "unstable_wave"] += 1
                else:
                    unexpected += 1
            if name == "set_ripples" and b["R"] and a["R"] != b["R"]:
                for what in other_R:
                    other_R[what] += b[what]
            if name == "center_ripples" and a["origin"] != b["origin"] and a["origin"][0] % 64 and a["origin"][1] % 16:
                for what in wrap:
                    wrap[what] += b[what]
    return dict(families=fam, cleared=cleared, made=made, refusals=refusals, other_R=other_R, wrap=wrap, stale=stale, unsolid=unsolid, unexpected=unexpected)


# what the header says sets and clears each mark ("ripple-layer bounds": reduce_ripple_bounds; "ripple walls" and "ripple bed": the zeroing
# rasters; "ripple swell": CURRENCY; "surface bounds": reduce_bounds and displace)
CLEARS = {"bounds": {"step_ripples", "step_bodies_coupled_host", "center_ripples", "reset_ripples", "set_ripples", "set_ripple_walls", "set_ripple_bed"},
          "swell": {"center_ripples", "set_ripple_walls", "set_ripple_bed", "set_ripples", "set_ripple_swell"},
          "fft": {"displace"}}
MAKES = {"bounds": {"reduce_ripple_bounds"}, "swell": {"refresh_ripple_swell"}, "fft": {"reduce_bounds"}}


def test_determinism():
    for seed in rq.SEEDS[:3]:
        a, b = rq.sequence(seed, rq.LENGTH), rq.sequence(seed, rq.LENGTH)
        assert a == b and len(a) >= rq.LENGTH
        np.random.seed(seed + 1)                                              # the global generator is not what it draws from
        assert rq.sequence(seed, rq.LENGTH) == a
    assert rq.sequence(rq.SEEDS[0], rq.LENGTH) != rq.sequence(rq.SEEDS[1], rq.LENGTH)
    assert len(set(rq.SEEDS)) == len(rq.SEEDS)


def test_coverage():
    c = coverage({seed: true_log(seed) for seed in rq.SEEDS})
    print(c)
    for f in rq.FAMILIES:
        assert len(c["families"][f]) >= 3, (f, c["families"][f])
    assert c["stale"] >= 3 and c["unsolid"] >= 1, (c["stale"], c["unsolid"])
    for mark in CLEARS:
        assert c["cleared"][mark] == CLEARS[mark], (mark, c["cleared"][mark] ^ CLEARS[mark])         # every one that should, and no other
        assert c["made"][mark] == MAKES[mark], (mark, c["made"][mark])
    assert all(n >= 2 for n in c["refusals"].values()) and c["unexpected"] == 0, (c["refusals"], c["unexpected"])
    assert all(n >= 1 for n in c["other_R"].values()), c["other_R"]
    assert all(n >= 1 for n in c["wrap"].values()), c["wrap"]


def test_a_refused_call_changes_nothing():
    refused = [(seed, r["k"], r["name"]) for seed in rq.SEEDS for r in true_log(seed) if r["code"] != rq.OK]
    assert len(refused) >= 14
    assert not [(seed, r["k"], r["name"]) for seed in rq.SEEDS for r in true_log(seed) if not r["unchanged"]]


@pytest.mark.parametrize("mistake", rq.MISTAKES)
def test_teeth(mistake):
    """the mistaken model and the true one run the same sequence; the first operation behind which an observable differs, per seed"""
    seen = {}
    for seed in rq.SEEDS:
        for t, r in zip(true_log(seed), run(seed, mistake=mistake)):
            what = [k for k in t["observed"] if t["observed"][k] != r["observed"][k]] + (["families"] if t["families"] != r["families"] else [])
            if what:
                seen[seed] = (r["k"], r["name"], what)
                break
    print(mistake, seen)
    assert seen, f"no committed seed sees the planted mistake {mistake!r}"
    if mistake != "swell_unsolid":                                            # (its plane is +0 everywhere: ripple_seq's docstring)
        assert any(w != ["families"] for _, _, w in seen.values()), (mistake, seen)


def test_float64_self_consistency():
    worst = dict.fromkeys(rq.FAMILIES, 0.0)
    n = 0
    for seed in rq.SEEDS:
        for r in true_log(seed):
            if "distance" in r:
                d, fam = r["distance"]
                worst[fam] = max(worst[fam], d)
                n += 1
                assert d <= rq.K[fam], (seed, r["k"], r["name"], fam, d, rq.K[fam])
    print({f: round(v, 2) for f, v in worst.items()}, n)
    assert n >= 40 and all(v > 0 for v in worst.values())                     # every family was measured on water that moves
