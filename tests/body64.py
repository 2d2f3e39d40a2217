"""Body buoyancy (include/datum_ocean_hip.h: datum_ocean_reduce_bodies) restated twice:

  body32   the definition in numpy float32, every operation one rounding as written: the pose transform, the per-probe terms from given
           surface records, the lane order and the tree;
  body64   the same in float64 on top of blend64.surface_blend64 (plain sums: the order does not matter there).

Bodies are a structured array (BODY, 64 bytes, the header's datum_ocean_body), probes an (n, 4) float32 array (x, y, z, a).  A body's
probe k has row offsets(bodies)[b] + k of the per-probe arrays (world positions, records); bodies whose range is bad have no rows.
`mistake` plants the errors tests/test_body_emul.py names: "tau_sign", "no_clamp", "no_cap", "world_arm", "no_first", "stride32".
"""

import numpy as np

import blend64

F = np.float32
LANES = 64

BODY = np.dtype([("rotation", F, 9), ("position", F, 3), ("first", np.int32), ("count", np.int32), ("cap", F), ("pad", np.int32)], align=False)
assert BODY.itemsize == 64


def make_bodies(rotations, positions, firsts, counts, caps):
    b = np.zeros(len(firsts), BODY)
    b["rotation"] = np.asarray(rotations, F).reshape(-1, 9)
    b["position"] = np.asarray(positions, F).reshape(-1, 3)
    b["first"], b["count"], b["cap"] = firsts, counts, caps
    return b


def range_bad(bodies, nprobes):
    f, c = bodies["first"].astype(np.int64), bodies["count"].astype(np.int64)
    return (f < 0) | (c < 0) | (f + c > nprobes) | np.isnan(bodies["cap"])


def offsets(bodies, nprobes):
    """(row offset of every body's first probe in the per-probe arrays, total rows); bad ranges take no rows"""
    n = np.where(range_bad(bodies, nprobes), 0, bodies["count"]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)])
    return off[:-1].copy(), int(off[-1])


def _gather(bodies, probes, mistake=None):
    """(body index, probe row) of every per-probe row"""
    bad = range_bad(bodies, len(probes))
    n = np.where(bad, 0, bodies["count"]).astype(np.int64)
    bi = np.repeat(np.arange(len(bodies)), n)
    off, _ = offsets(bodies, len(probes))
    k = np.arange(int(n.sum())) - off[bi]
    first = 0 if mistake == "no_first" else bodies["first"][bi].astype(np.int64)
    return bi, first + k


def world32(bodies, probes, mistake=None):
    """(w [rows, 3] float32, a [rows] float32, bad [rows]) of every probe of every body: ((R0 x + R1 y) + R2 z) + T"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    bi, pi = _gather(bodies, probes, mistake)
    R, T = bodies["rotation"][bi], bodies["position"][bi]
    x, y, z, a = (probes[pi, j] for j in range(4))
    with np.errstate(all="ignore"):
        w = np.stack([((R[:, 3 * r] * x + R[:, 3 * r + 1] * y) + R[:, 3 * r + 2] * z) + T[:, r] for r in range(3)], 1)
    assert w.dtype == F
    bad = ~(np.isfinite(w).all(1) & np.isfinite(a))
    return w, a, bad


def terms32(bodies, probes, recs, mistake=None):
    """[rows, 8] float32 terms of every probe from its surface record [rows, 8]"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    recs = np.asarray(recs, F).reshape(-1, 8)
    bi, _ = _gather(bodies, probes, mistake)
    w, a, _ = world32(bodies, probes, mistake)
    T, cap = bodies["position"][bi], bodies["cap"][bi]
    with np.errstate(all="ignore"):
        d = recs[:, 2] - w[:, 2]
        if mistake != "no_clamp":
            d = np.fmax(d, F(0))
        if mistake != "no_cap":
            d = np.fmin(d, cap)
        m = a * d
        rx, ry = (w[:, 0], w[:, 1]) if mistake == "world_arm" else (w[:, 0] - T[:, 0], w[:, 1] - T[:, 1])
        ty = rx * m if mistake == "tau_sign" else -(rx * m)
        t = np.stack([m, ry * m, ty, np.where(d > 0, a, F(0)), m * recs[:, 4], m * recs[:, 5], m * recs[:, 6], recs[:, 3]], 1)
    assert t.dtype == F
    return t


def _combine(p, t):
    """p + t per field, field 7 the maximum (fmaxf)"""
    with np.errstate(all="ignore"):
        return np.concatenate([p[..., :7] + t[..., :7], np.fmax(p[..., 7:], t[..., 7:])], -1)


def reduce32(bodies, probes, recs, mistake=None):
    """[nbodies, 8] float32 records: lane l adds the terms of probes l, l + 64, ... in order; then p[l] += p[l + s] for s = 32 ... 1"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    t = terms32(bodies, probes, recs, mistake)
    _, _, pbad = world32(bodies, probes, mistake)
    off, _ = offsets(bodies, len(probes))
    rbad = range_bad(bodies, len(probes))
    stride = 32 if mistake == "stride32" else LANES          # (planted: lane l takes l, l + 32, ...: probes from 32 on are taken twice)
    out = np.empty((len(bodies), 8), F)
    for b in range(len(bodies)):
        n = 0 if rbad[b] else int(bodies["count"][b])
        rows = slice(int(off[b]), int(off[b]) + n)
        if rbad[b] or pbad[rows].any():
            out[b] = np.nan
            continue
        tb = t[rows]
        p = np.zeros((LANES, 8), F)
        for k in range(0, n, stride):
            chunk = tb[k:k + LANES]
            p[:len(chunk)] = _combine(p[:len(chunk)], chunk)
        s = LANES // 2
        while s >= 1:
            p[:s] = _combine(p[:s], p[s:2 * s])
            s //= 2
        out[b] = p[0]
    return out


def sum64(bodies, probes, recs):
    """([nbodies, 8] float64 sums of the same fp32 terms, [nbodies, 8] sums of their magnitudes); field 7 the maximum"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    t = terms32(bodies, probes, recs).astype(np.float64)
    off, _ = offsets(bodies, len(probes))
    rbad = range_bad(bodies, len(probes))
    out, mag = np.zeros((len(bodies), 8)), np.zeros((len(bodies), 8))
    for b in range(len(bodies)):
        n = 0 if rbad[b] else int(bodies["count"][b])
        tb = t[int(off[b]):int(off[b]) + n]
        out[b, :7], mag[b, :7] = tb[:, :7].sum(0), np.abs(tb[:, :7]).sum(0)
        out[b, 7] = mag[b, 7] = tb[:, 7].max() if n else 0.0
    return out, mag


def bound64(bodies, mag):
    """|record - float64 sum of the same terms| <= (ceil(count / 64) + 6) 2^-24 sum |term|: a lane's chain and the six tree steps"""
    n = np.maximum(bodies["count"].astype(np.int64), 0)
    return ((n + 63) // 64 + 6)[:, None] * 2.0 ** -24 * mag


def body64(bodies, probes, maps_list, foams, mode, scales, s, iterations):
    """([nbodies, 8] float64 records of the definition in float64, per-probe dict: w, a, rec (float64 records), d (unclamped rec.z - w.z),
    body (index per row)) on top of blend64.surface_blend64"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    bi, pi = _gather(bodies, probes)
    R, T = bodies["rotation"][bi].astype(np.float64), bodies["position"][bi].astype(np.float64)
    pr = probes[pi].astype(np.float64)
    w = np.stack([R[:, 3 * r] * pr[:, 0] + R[:, 3 * r + 1] * pr[:, 1] + R[:, 3 * r + 2] * pr[:, 2] + T[:, r] for r in range(3)], 1)
    a = pr[:, 3]
    rec = blend64.surface_blend64(maps_list, foams, mode, scales, s, w[:, :2], iterations)
    raw = rec[:, 2] - w[:, 2]
    d = np.minimum(np.maximum(raw, 0.0), bodies["cap"][bi].astype(np.float64))
    m = a * d
    rx, ry = w[:, 0] - T[:, 0], w[:, 1] - T[:, 1]
    t = np.stack([m, ry * m, -(rx * m), np.where(d > 0, a, 0.0), m * rec[:, 4], m * rec[:, 5], m * rec[:, 6], rec[:, 3]], 1)
    out = np.zeros((len(bodies), 8))
    np.add.at(out[:, :7], bi, t[:, :7])
    np.maximum.at(out[:, 7], bi, t[:, 7])
    return out, dict(w=w, a=a, rec=rec, d=raw, body=bi)
