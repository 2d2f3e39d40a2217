"""Body contact (include/datum_ocean_hip.h: datum_ocean_step_bodies_contact) restated beside couple64.py:

  terms         the eight contact terms of every probe in the dtype asked for: numpy float32 reproduces datum_amd/csrc/ocean_contact.h
                operation for operation (the bits of the device), float64 is the same formulas in double.  With `mag` the same walk
                over magnitudes -- every difference the sum of the absolute values -- for the bar of tests/test_contact_emul.py;
  reduce32      the lanes' chains and the tree over the eight fields (seven sums and a maximum: body64's shape);
  substep32     one contact sub-step in float32: couple64's rippled records, body64.reduce32, drag64.reduce32, ripple64.wake32, the
                contact's totals, step64's integrator, then layer.step(h, 1);
  call32        `substeps` of them, the record folded;
  Land64        bodies under gravity and contact alone in float64 (no water), for the closed forms of tests/test_contact64.py.

A scene is make_scene(...): the parameters, the bed (its map is the handle's: raw depths, positive down) and the wall list with inv2.
`mistake` plants the errors tests/test_contact64.py names:
  "normal_sign"   the normal points into the ground / the shape      "no_clamp"      fn is not clamped at 0
  "no_inv2"       the shape's penetration is not scaled by inv2       "origin_arm"    r is the world point, not w - T
  "deepest_sum"   the deepest penetration is summed, not folded by the maximum
"""

import numpy as np

import body64
import couple64
import drag64
import ripple64
import step64

F = np.float32
D = np.float64

RECORD_FLOATS = 16
FIELDS = 8
BED, WALLS = 1, 2
BOX, ELLIPSE = 0, 1
MISTAKES = ("normal_sign", "no_clamp", "no_inv2", "origin_arm", "deepest_sum")

CONTACT = np.dtype([("stiffness", F), ("damping", F), ("friction", F), ("flags", np.uint32), ("reserved", F, 4)], align=False)
WALL = np.dtype([("center", F, 2), ("axis", F, 2), ("half", F, 2), ("kind", np.int32), ("reserved", np.int32)], align=False)
assert CONTACT.itemsize == 32 and WALL.itemsize == 32


def make_contact(k, c, ct, flags):
    p = np.zeros(1, CONTACT)
    p["stiffness"], p["damping"], p["friction"], p["flags"] = k, c, ct, flags
    return p


def make_walls(rows):
    """rows of (cx, cy, ax, ay, hx, hy, kind)"""
    w = np.zeros(len(rows), WALL)
    for i, (cx, cy, ax, ay, hx, hy, kind) in enumerate(rows):
        w[i]["center"], w[i]["axis"], w[i]["half"], w[i]["kind"] = (cx, cy), (ax, ay), (hx, hy), kind
    return w


def inv2(walls):
    """(float)(1.0 / (ax^2 + ay^2)), formed in double from the fp32 axis and rounded once"""
    a = walls["axis"].astype(D)
    with np.errstate(all="ignore"):
        return (1.0 / (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])).astype(F)


def make_scene(k, c, ct, flags, bed=None, depths=None, walls=None):
    """bed: dict(origin, texel, outside) with depths [height, width]; walls: make_walls(...)"""
    s = dict(k=F(k), c=F(c), ct=F(ct), flags=int(flags), bed=None, walls=None)
    if bed is not None:
        depths = np.ascontiguousarray(depths, F)
        s["bed"] = dict(width=depths.shape[1], height=depths.shape[0], ox=F(bed["origin"][0]), oy=F(bed["origin"][1]), invt=F(1.0 / D(F(bed["texel"]))),
                        outside=F(bed["outside"]), map=depths)
    if walls is not None:
        s["walls"] = walls
        s["inv2"] = inv2(walls)
    return s


def _sub(mag, x, y):
    return np.abs(x) + np.abs(y) if mag else x - y


def _ground(t, bed, w, mag, true):
    """(p, n[3], inside) of the ground under the world points w [rows, 3]"""
    S = lambda x, y: _sub(mag, x, y)
    c = lambda v: t(v)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    W, H = bed["width"], bed["height"]
    # (which texels and whether on the map: decided by the real walk, in magnitudes too)
    xr, yr, _ = true["w"].T if mag else (x, y, z)
    ur, vr = (xr - c(bed["ox"])) * c(bed["invt"]), (yr - c(bed["oy"])) * c(bed["invt"])
    inside = (ur >= 0) & (ur <= t(W - 1)) & (vr >= 0) & (vr <= t(H - 1))
    uc, vc = np.where(inside, ur, 0), np.where(inside, vr, 0)
    i = np.minimum(np.floor(uc).astype(np.int64), W - 2)
    j = np.minimum(np.floor(vc).astype(np.int64), H - 2)
    u, v = S(x, c(bed["ox"])) * c(bed["invt"]), S(y, c(bed["oy"])) * c(bed["invt"])
    wu, wv = S(u, i.astype(t)), S(v, j.astype(t))
    m = bed["map"].astype(t)
    if mag:
        m = np.abs(m)
    c0, c1, c2, c3 = m[j, i], m[j, i + 1], m[j + 1, i], m[j + 1, i + 1]
    a0, a1 = S(c1, c0), S(c3, c2)
    e0, e1 = c0 + wu * a0, c2 + wu * a1
    raw = e0 + wv * S(e1, e0)
    gx = (a0 + wv * S(a1, a0)) * c(bed["invt"])
    gy = S(e1, e0) * c(bed["invt"])
    if mag:
        l = true["l"]
    else:
        l = np.sqrt((gx * gx + gy * gy) + t(1) * t(1))
        true["l"] = l
    one = np.ones_like(gx)
    n = [np.where(inside, gx / l, 0), np.where(inside, gy / l, 0), np.where(inside, one / l, one)]
    raw = np.where(inside, raw, np.abs(c(bed["outside"])) if mag else c(bed["outside"]))
    zg = S(t(0), raw)
    p = S(zg, z)
    return p.astype(t), [a.astype(t) for a in n], inside


def _wall(t, shape, i2, w, mag, true, key, mistake):
    """(p, n[3], covers) of one shape at the world points w"""
    S = lambda x, y: _sub(mag, x, y)
    cx, cy = t(shape["center"][0]), t(shape["center"][1])
    ax, ay = t(shape["axis"][0]), t(shape["axis"][1])
    hx, hy = t(shape["half"][0]), t(shape["half"][1])
    if mag:
        cx, cy, ax, ay = abs(cx), abs(cy), abs(ax), abs(ay)
    x, y = w[:, 0], w[:, 1]
    dx, dy = S(x, cx), S(y, cy)
    u = dx * ax + dy * ay
    v = S(dy * ax, dx * ay)
    if mag:
        tu, tv, covers = true[key + "u"], true[key + "v"], true[key + "covers"]
    else:
        tu, tv = u, v
    zero, one = np.zeros_like(u), np.ones_like(u)
    if int(shape["kind"]) == BOX:
        if not mag:
            covers = (np.abs(u) <= hx) & (np.abs(v) <= hy)
        px, py = S(hx, np.abs(u)), S(hy, np.abs(v))
        tpx, tpy = hx - np.abs(tu), hy - np.abs(tv)
        first = tpx <= tpy
        q = np.where(first, px, py)
        sx, sy = np.where(tu >= 0, one, -one), np.where(tv >= 0, one, -one)
        if mag:
            sx, sy = one, one
        mx, my = np.where(first, sx, zero), np.where(first, zero, sy)
    else:
        if not mag:
            a, b, r = u * hy, v * hx, hx * hy
            covers = a * a + b * b <= r * r
        eu, ev = u / hx, v / hy
        rho = np.sqrt(eu * eu + ev * ev)
        q = S(t(1), rho) * min(hx, hy)
        lx, ly = eu / hx, ev / hy
        if mag:
            l, trho = true[key + "l"], true[key + "rho"]
        else:
            with np.errstate(all="ignore"):
                l = np.sqrt(lx * lx + ly * ly)
            true[key + "l"], true[key + "rho"], trho = l, rho, rho
        with np.errstate(all="ignore"):
            mx, my = np.where(trho == 0, one, lx / l), np.where(trho == 0, zero, ly / l)
    if not mag:
        true[key + "u"], true[key + "v"], true[key + "covers"] = u, v, covers
    p = q if mistake == "no_inv2" else q * t(i2)
    n = [S(mx * ax, my * ay), mx * ay + my * ax, zero]
    return p.astype(t), [a.astype(t) for a in n], covers


def _force(t, scene, r, vel, omega, a, p, n, mag, mistake):
    """the eight terms [rows, 8] of one contact (p, n) of every row: drag_terms' u, the clamped normal force, the viscous tangential one"""
    S = lambda x, y: _sub(mag, x, y)
    k, c, ct = t(scene["k"]), t(scene["c"]), t(scene["ct"])
    if mistake == "normal_sign":
        n = [-x for x in n]
    rx, ry, rz = r
    ux = vel[0] + S(omega[1] * rz, omega[2] * ry)
    uy = vel[1] + S(omega[2] * rx, omega[0] * rz)
    uz = vel[2] + S(omega[0] * ry, omega[1] * rx)
    vn = (ux * n[0] + uy * n[1]) + uz * n[2]
    fn = a * S(k * p, c * vn)
    if mistake != "no_clamp":
        fn = np.fmax(fn, t(0))
    g = a * ct
    f = [S(fn * n[j], g * S(u, vn * n[j])) for j, u in enumerate((ux, uy, uz))]
    tau = [S(ry * f[2], rz * f[1]), S(rz * f[0], rx * f[2]), S(rx * f[1], ry * f[0])]
    out = np.stack(f + tau + [np.ones_like(p), p], 1)
    assert out.dtype == t
    return out


def terms(t, bodies, motions, probes, scene, mistake=None, world=None, mag=False, true=None):
    """[rows, 8] contact terms of every probe of every body in the dtype t (np.float32: the header's bits).  world: (w, a, body index) to
    use in place of the pose transform (float64 poses).  mag: the walk over magnitudes, with the decisions and the denominators of the
    real walk `true` (a dict a real walk filled)"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    if world is None:
        bi, _ = body64._gather(bodies, probes)
        w, a, _ = body64.world32(bodies, probes)
        w, a = w.astype(t), a.astype(t)
        T = bodies["position"][bi].astype(t)
        vel, omega = motions["linear"][bi].astype(t), motions["angular"][bi].astype(t)
    else:
        w, a, T, vel, omega = (np.asarray(x, t) for x in world)
    true = {} if true is None else true
    if mag:
        w, a, T, vel, omega = (np.abs(x) for x in (w, a, T, vel, omega))
    else:
        true["w"] = w
    S = lambda x, y: _sub(mag, x, y)
    with np.errstate(all="ignore"):
        r = [w[:, j] if mistake == "origin_arm" else S(w[:, j], T[:, j]) for j in range(3)]
        vel, omega = [vel[:, j] for j in range(3)], [omega[:, j] for j in range(3)]
        total = np.zeros((len(w), FIELDS), t)

        def add(touch, one):
            nonlocal total
            s = total + one
            s[:, 7] = s[:, 7] if mistake == "deepest_sum" else np.fmax(total[:, 7], one[:, 7])
            total = np.where(touch[:, None], s, total).astype(t)

        if scene["flags"] & BED:
            p, n, _ = _ground(t, scene["bed"], w, mag, true)
            touch = true["gtouch"] if mag else p > 0
            true["gtouch"] = touch
            add(touch, _force(t, scene, r, vel, omega, a, p, n, mag, mistake))
        if scene["flags"] & WALLS:
            for i, shape in enumerate(scene["walls"]):
                key = f"s{i}"
                p, n, covers = _wall(t, shape, scene["inv2"][i], w, mag, true, key, mistake)
                touch = true[key + "touch"] if mag else covers & (p > 0)
                true[key + "touch"] = touch
                add(touch, _force(t, scene, r, vel, omega, a, p, n, mag, mistake))
    assert total.dtype == t
    return total


def reduce32(bodies, probes, t):
    """[nbodies, 8] float32: lane l adds the terms of probes l, l + 64, ... in order, then the tree; NaNs for a body with a bad range or probe"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    _, _, pbad = body64.world32(bodies, probes)
    off, _ = body64.offsets(bodies, len(probes))
    rbad = body64.range_bad(bodies, len(probes))
    out = np.empty((len(bodies), FIELDS), F)
    for b in range(len(bodies)):
        n = 0 if rbad[b] else int(bodies["count"][b])
        rows = slice(int(off[b]), int(off[b]) + n)
        if rbad[b] or pbad[rows].any():
            out[b] = np.nan
            continue
        tb = t[rows]
        p = np.zeros((body64.LANES, FIELDS), F)
        for k in range(0, n, body64.LANES):
            chunk = tb[k:k + body64.LANES]
            p[:len(chunk)] = body64._combine(p[:len(chunk)], chunk)
        s = body64.LANES // 2
        while s >= 1:
            p[:s] = body64._combine(p[:s], p[s:2 * s])
            s //= 2
        out[b] = p[0]
    return out


def fold32(rec, old, first):
    """couple64.fold32 for the first twelve fields, field 15 by fmaxf"""
    out = rec.copy()
    out[:, :12] = couple64.fold32(rec[:, :12], None if first else old[:, :12], first)
    if not first:
        with np.errstate(all="ignore"):
            out[:, 15] = np.fmax(old[:, 15], rec[:, 15])
        out[np.isnan(old[:, 0]) | np.isnan(rec[:, 0])] = np.nan
    return out


def substep32(layer, bodies, motions, props, probes, recs, h, scene, samples=None, old=None, trace=None):
    """couple64.substep32 with contact: returns (bodies', motions', records [n, 16], bad [n])"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    h = F(h)
    first = old is None
    if samples is None:
        samples = layer.sample(couple64.points32(bodies, probes))
    rr = couple64.ripple32(recs, samples)
    wasbad = np.zeros(len(bodies), bool) if first else np.isnan(old[:, 0])
    dead = wasbad | step64.props_bad(props)
    mo = motions.copy()
    mo["linear"][dead] = np.nan
    lift = body64.reduce32(bodies, probes, rr)
    drag = drag64.reduce32(bodies, motions, probes, rr)
    wake = ripple64.wake32(bodies, mo, probes, rr, h, layer.src, layer.ox, layer.oy, layer.invs)
    k = reduce32(bodies, probes, terms(F, bodies, motions, probes, scene))
    # untouched bodies: step64's sub-step as it stands.  Touched ones: its totals with the contact's share, handed back to it as a drag
    # under no buoyancy (0 * 0 + F.z)
    nb, nm, rec8, bad = step64.integrate32(lift, drag, bodies, motions, props, h)
    touched = k[:, 6] != 0
    with np.errstate(all="ignore"):
        tot = (rec8[:, :6] + k[:, :6]).astype(F)
    zl = np.zeros_like(lift)
    dr = np.zeros_like(drag)
    dr[:, :6] = np.where(np.isnan(tot), 0, tot)
    pz = props.copy()
    pz["buoyancy"] = 0
    tb, tm, trec, tbad = step64.integrate32(zl, dr, bodies, motions, pz, h)
    tbad = tbad | np.isnan(tot).any(1)
    nb[touched], nm[touched], bad[touched] = tb[touched], tm[touched], tbad[touched]
    tot = np.where(touched[:, None], trec[:, :6], rec8[:, :6]).astype(F)
    bad = bad | dead | np.isnan(lift).any(1) | np.isnan(drag).any(1) | np.isnan(k).any(1)
    rec = np.concatenate([tot, lift[:, :1], drag[:, 7:8], wake[:, :4], k[:, :3], k[:, 7:8]], 1).astype(F)
    nb[bad], nm[bad], rec[bad] = bodies[bad], motions[bad], np.nan
    if trace is not None:
        trace.append(rec.copy())
    rec = fold32(rec, old, first)
    assert rec.dtype == F and rec.shape[1] == RECORD_FLOATS
    layer.step(h, 1)
    return nb, nm, rec, bad


def call32(layer, bodies, motions, props, probes, recs_of, dt, substeps, scene, trace=None):
    """datum_ocean_step_bodies_contact: recs_of(bodies) gives the velocity records [rows, 8] for the poses of a sub-step"""
    h = step64.step_size(dt, substeps)
    rec = None
    for _ in range(substeps):
        bodies, motions, rec, _ = substep32(layer, bodies, motions, props, probes, recs_of(bodies), h, scene, old=rec, trace=trace)
    return bodies, motions, rec


class Land64:
    """Bodies under gravity and contact alone, in float64: no water (buoyancy and drag are nothing), the contact's sums plain, step64's
    integrator in float64.  deepest is the largest per-probe term 7 of the last sub-step; count the touching contacts"""

    def __init__(self, bodies, motions, props, probes, scene, mistake=None):
        self.props, self.scene, self.mistake = props, scene, mistake
        self.probes = np.asarray(probes, D).reshape(-1, 4)
        self.bi, self.pi = body64._gather(bodies, self.probes)
        self.R = bodies["rotation"].astype(D).reshape(-1, 3, 3)
        self.T = bodies["position"].astype(D)
        self.v = motions["linear"].astype(D)
        self.o = motions["angular"].astype(D)

    def contact(self):
        bi = self.bi
        p = self.probes[self.pi]
        w = np.einsum("nij,nj->ni", self.R[bi], p[:, :3]) + self.T[bi]
        t = terms(D, None, None, self.probes, self.scene, self.mistake, world=(w, p[:, 3], self.T[bi], self.v[bi], self.o[bi]))
        n = len(self.T)
        k = np.zeros((n, FIELDS))
        np.add.at(k[:, :7], bi, t[:, :7])
        if self.mistake == "deepest_sum":
            np.add.at(k[:, 7], bi, t[:, 7])
        else:
            np.maximum.at(k[:, 7], bi, t[:, 7])
        return k

    def substep(self, h):
        k = self.contact()
        n = len(self.T)
        lift, drag = np.zeros((n, 8)), np.zeros((n, 8))
        drag[:, :6] = k[:, :6]
        b64 = np.zeros(n, np.dtype([("rotation", D, 9), ("position", D, 3)]))
        b64["rotation"], b64["position"] = self.R.reshape(-1, 9), self.T
        m64 = np.zeros(n, np.dtype([("linear", D, 3), ("angular", D, 3)]))
        m64["linear"], m64["angular"] = self.v, self.o
        out = step64.integrate64(lift, drag, b64, m64, self.props, D(h))
        self.R, self.T, self.v, self.o = out["rotation"].reshape(-1, 3, 3), out["position"], out["linear"], out["angular"]
        self.force, self.count, self.deepest = k[:, :3], k[:, 6], k[:, 7]
        return out
