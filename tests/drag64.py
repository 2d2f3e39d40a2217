"""Body drag (include/datum_ocean_hip.h: datum_ocean_reduce_body_drag) restated twice, beside body64.py and on top of it:

  terms32 / reduce32   the definition in numpy float32, every operation one rounding as written: the per-probe force and torque terms from
                       given velocity records (datum_ocean_read_velocity_blend's), the lane order and the tree (body64's);
  drag64               the same in float64 end to end, from the maps and the velocity planes (plain sums: the order does not matter there).

Bodies and probes are body64's; motions are a structured array (MOTION, 32 bytes, the header's datum_ocean_body_motion), one per body.  A
body's probe k has row body64.offsets(bodies)[b] + k of the per-probe arrays; bodies whose range is bad have no rows.
`mistake` plants the errors tests/test_drag64.py names:
  "omega_sign"   u = v - omega x r                       "no_rz"       r.z left out of the lever arm (a planar arm)
  "wet_switch"   the weight a (d > 0) instead of m       "s_no_z"      s without the e.z term
  "fma"          cl + cq s contracted into one fma       "tau_transposed"   f x r instead of r x f
"""

import numpy as np

import blend64
import body64
import surface64
import vel64

F = np.float32
LANES = body64.LANES

MOTION = np.dtype([("linear", F, 3), ("angular", F, 3), ("cl", F), ("cq", F)], align=False)
assert MOTION.itemsize == 32

MISTAKES = ("omega_sign", "no_rz", "wet_switch", "s_no_z", "fma", "tau_transposed")


def make_motions(linear, angular, cl, cq):
    n = len(np.asarray(cl).reshape(-1))
    m = np.zeros(n, MOTION)
    m["linear"] = np.asarray(linear, F).reshape(-1, 3)
    m["angular"] = np.asarray(angular, F).reshape(-1, 3)
    m["cl"], m["cq"] = cl, cq
    return m


def motion_bad(motions):
    return ~(np.isfinite(motions["linear"]).all(1) & np.isfinite(motions["angular"]).all(1) & np.isfinite(motions["cl"]) & np.isfinite(motions["cq"]))


def terms32(bodies, motions, probes, recs, mistake=None):
    """[rows, 8] float32 terms of every probe from its velocity record [rows, 8]: Fx, Fy, Fz, tau x, tau y, tau z, m, residual"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    recs = np.asarray(recs, F).reshape(-1, 8)
    bi, _ = body64._gather(bodies, probes)
    w, a, _ = body64.world32(bodies, probes)
    T, cap = bodies["position"][bi], bodies["cap"][bi]
    v, o, cl, cq = motions["linear"][bi], motions["angular"][bi], motions["cl"][bi], motions["cq"][bi]
    with np.errstate(all="ignore"):
        d = np.fmin(np.fmax(recs[:, 2] - w[:, 2], F(0)), cap)
        m = a * d
        rx, ry, rz = w[:, 0] - T[:, 0], w[:, 1] - T[:, 1], w[:, 2] - T[:, 2]
        if mistake == "no_rz":
            rz = np.zeros_like(rz)
        cx, cy, cz = o[:, 1] * rz - o[:, 2] * ry, o[:, 2] * rx - o[:, 0] * rz, o[:, 0] * ry - o[:, 1] * rx
        if mistake == "omega_sign":
            ux, uy, uz = v[:, 0] - cx, v[:, 1] - cy, v[:, 2] - cz
        else:
            ux, uy, uz = v[:, 0] + cx, v[:, 1] + cy, v[:, 2] + cz
        ex, ey, ez = recs[:, 4] - ux, recs[:, 5] - uy, recs[:, 6] - uz
        s = np.sqrt(ex * ex + ey * ey) if mistake == "s_no_z" else np.sqrt((ex * ex + ey * ey) + ez * ez)
        c = vel64.fma32(cq, s, cl) if mistake == "fma" else cl + cq * s
        k = (np.where(d > 0, a, F(0)) if mistake == "wet_switch" else m) * c
        fx, fy, fz = k * ex, k * ey, k * ez
        tx, ty, tz = ry * fz - rz * fy, rz * fx - rx * fz, rx * fy - ry * fx
        if mistake == "tau_transposed":
            tx, ty, tz = fy * rz - fz * ry, fz * rx - fx * rz, fx * ry - fy * rx
        t = np.stack([fx, fy, fz, tx, ty, tz, m, recs[:, 3]], 1)
    assert t.dtype == F
    return t


def reduce32(bodies, motions, probes, recs, mistake=None):
    """[nbodies, 8] float32 records: body64.reduce32's walk (lane l adds probes l, l + 64, ... in order; then p[l] += p[l + s] for
    s = 32 ... 1, field 7 the maximum) over terms32; NaN records for body64's bad bodies and for a non-finite motion"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    t = terms32(bodies, motions, probes, recs, mistake)
    _, _, pbad = body64.world32(bodies, probes)
    off, _ = body64.offsets(bodies, len(probes))
    rbad = body64.range_bad(bodies, len(probes))
    mbad = motion_bad(motions)
    out = np.empty((len(bodies), 8), F)
    for b in range(len(bodies)):
        n = 0 if rbad[b] else int(bodies["count"][b])
        rows = slice(int(off[b]), int(off[b]) + n)
        if rbad[b] or mbad[b] or pbad[rows].any():
            out[b] = np.nan
            continue
        tb = t[rows]
        p = np.zeros((LANES, 8), F)
        for k in range(0, n, LANES):
            chunk = tb[k:k + LANES]
            p[:len(chunk)] = body64._combine(p[:len(chunk)], chunk)
        s = LANES // 2
        while s >= 1:
            p[:s] = body64._combine(p[:s], p[s:2 * s])
            s //= 2
        out[b] = p[0]
    return out


def terms64(r, v, o, cl, cq, m, vel):
    """the definition's force and torque of one probe in float64, arrays [rows, ...]: lever arm r [rows, 3], the body's v and omega
    [rows, 3], cl, cq, the weight m and the water's velocity vel [rows, 3].  Returns (f [rows, 3], tau [rows, 3], e, s)"""
    e = vel - (v + np.cross(o, r))
    s = np.sqrt((e * e).sum(1))
    f = (m * (cl + cq * s))[:, None] * e
    return f, np.cross(r, f), e, s


def velocity_blend64(maps_list, planes, scales, s, points, iterations):
    """(M, 8) float64 records of datum_ocean_sample_velocity_blend: blend64's solve and V(b), the listed planes' REPEAT bilinear samples at
    the same texture coordinates, summed"""
    scales = [float(x) for x in scales]
    q = np.asarray(points, np.float64).reshape(-1, 2).T.copy()
    b = q.copy()
    for _ in range(iterations):
        V, _, _ = blend64.evaluate_blend64(maps_list, scales, s, b)
        b = b + (q - V[:2])
    V, _, (px, py) = blend64.evaluate_blend64(maps_list, scales, s, b)
    u = sum(surface64.bilinear64(np.asarray(pl, np.float64).transpose(2, 0, 1)[:3], px * sc, py * sc) for pl, sc in zip(planes, scales))
    return np.concatenate([V, np.hypot(V[0] - q[0], V[1] - q[1])[None], u, np.zeros_like(px)[None]]).T


def drag64(bodies, motions, probes, maps_list, planes, scales, s, iterations):
    """([nbodies, 8] float64 records of the definition in float64, per-probe dict: w, a, rec (float64 velocity records), d (unclamped
    rec[2] - w.z), m, r, e, s, f, body (index per row))"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    bi, pi = body64._gather(bodies, probes)
    R, T = bodies["rotation"][bi].astype(np.float64), bodies["position"][bi].astype(np.float64)
    pr = probes[pi].astype(np.float64)
    w = np.stack([R[:, 3 * r] * pr[:, 0] + R[:, 3 * r + 1] * pr[:, 1] + R[:, 3 * r + 2] * pr[:, 2] + T[:, r] for r in range(3)], 1)
    a = pr[:, 3]
    rec = velocity_blend64(maps_list, planes, scales, s, w[:, :2], iterations)
    raw = rec[:, 2] - w[:, 2]
    d = np.minimum(np.maximum(raw, 0.0), bodies["cap"][bi].astype(np.float64))
    m = a * d
    r = w - T
    mo = {k: motions[k][bi].astype(np.float64) for k in ("linear", "angular", "cl", "cq")}
    f, tau, e, sp = terms64(r, mo["linear"], mo["angular"], mo["cl"], mo["cq"], m, rec[:, 4:7])
    t = np.concatenate([f, tau, m[:, None], rec[:, 3:4]], 1)
    out = np.zeros((len(bodies), 8))
    np.add.at(out[:, :7], bi, t[:, :7])
    np.maximum.at(out[:, 7], bi, t[:, 7])
    return out, dict(w=w, a=a, rec=rec, d=raw, m=m, r=r, e=e, s=sp, f=f, body=bi)
