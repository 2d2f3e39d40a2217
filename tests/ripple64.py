"""The ripple layer (include/datum_ocean_hip.h: "ripple layer") restated, beside drag64.py and on top of it:

  params            what datum_ocean_step_ripples rounds on the host: h, c2s2 and the sponge table f[0 .. B];
  substep           one sub-step over the layer in MEMORY order, in numpy float32 -- every operation one rounding as written, the bits of
                    datum_amd/csrc/ocean_ripple.h -- or, with dtype=np.float64, the same arithmetic in float64 from the same rounded
                    parameters;
  Layer             the layer as the handle keeps it: the torus in memory, the origin, center, step, deposit, window;
  splat32           the integer splat; sample32 the bilinear sample; wake32 the wake's per-probe terms, deposits and per-body records
                    from given velocity records (datum_ocean_read_velocity_blend's).

`mistake` plants the errors tests/test_ripple64.py names:
  "explicit"        the height moves with the OLD rate           "wrap"            neighbours wrap round instead of a zero border
  "src_own_only"    the first sub-step's neighbours lack src     "sponge_off_one"  the sponge index starts one cell further in
"""

import numpy as np

import body64
import drag64

F = np.float32
LANES = body64.LANES

UNIT = F(2.0 ** -20)
PER_METRE = F(2.0 ** 20)
QMAX = F(2.0 ** 30)
MAX_SPONGE = 64

MISTAKES = ("explicit", "wrap", "src_own_only", "sponge_off_one")

# The device against float64, for one datum_ocean_step_ripples call (up to 16 sub-steps) from a common fp32 state: |eta - eta64| <= K_RIP eps
# max|eta64|.  3 x the worst distance of THIS restatement from its float64 form over tests/test_ripple_emul.py's cases (measured on the
# CPU: 5.88, at R = 128, 16 sub-steps, no sponge); the device is the restatement bit for bit, so the figure is not taken from the GPU
K_RIP = 18.0


def params(c, s, gamma, B, sponge_gamma, dt, substeps):
    """(h, c2s2, f): h = dt * (1 / substeps) in fp32; c2s2 and f[0 .. B] in double from the fp32 c, s, gamma, sponge_gamma, rounded once"""
    c, s, gamma, sponge_gamma = (float(F(v)) for v in (c, s, gamma, sponge_gamma))
    h = F(dt) * (F(1) / F(substeps))
    k = np.arange(B + 1, dtype=np.float64)
    u = k / B if B > 0 else np.zeros(1)
    f = (1.0 / (1.0 + float(h) * (gamma + sponge_gamma * (u * u)))).astype(F)
    return h, F(c * c / (s * s)), f


def stable(c, s, dt, substeps):
    """what the call accepts: dt >= 0 and c h / s <= 0.7 (the scheme's bound is 1 / sqrt 2)"""
    h = F(dt) * (F(1) / F(substeps))
    return float(h) >= 0 and float(F(c)) * float(h) / float(F(s)) <= 0.7


def window_coords(R, ox, oy):
    """window coordinates (wx [R], wy [R]) of memory columns and rows"""
    m = np.arange(R)
    return (m - ox) & (R - 1), (m - oy) & (R - 1)


def sponge_index(wx, wy, R, B):
    d = np.minimum(np.minimum(wx[None, :], R - 1 - wx[None, :]), np.minimum(wy[:, None], R - 1 - wy[:, None]))
    return np.maximum(0, B - d)


def substep(eta, rate, src, ox, oy, B, h, c2s2, f, first, dtype=F, mistake=None):
    """(eta, rate) [R, R] in memory order after one sub-step; src [R, R] int32 is read by a step's first sub-step only"""
    R = eta.shape[0]
    T = dtype
    eta, rate = eta.astype(T), rate.astype(T)
    h, c2s2, f = T(h), T(c2s2), np.asarray(f).astype(T)
    e = eta + src.astype(T) * T(UNIT) if first else eta
    en = eta if (first and mistake == "src_own_only") else e
    wx, wy = window_coords(R, ox, oy)
    zero = T(0)
    eL, eR = np.roll(en, 1, 1), np.roll(en, -1, 1)
    eD, eU = np.roll(en, 1, 0), np.roll(en, -1, 0)
    if mistake != "wrap":
        eL = np.where(wx[None, :] == 0, zero, eL)
        eR = np.where(wx[None, :] == R - 1, zero, eR)
        eD = np.where(wy[:, None] == 0, zero, eD)
        eU = np.where(wy[:, None] == R - 1, zero, eU)
    k = sponge_index(wx, wy, R, B - 1 if (mistake == "sponge_off_one" and B > 0) else B)
    lap = ((eL + eR) + (eD + eU)) - T(4) * e
    v1 = (rate + h * (c2s2 * lap)) * f[k]
    e1 = e + h * (rate if mistake == "explicit" else v1)
    assert e1.dtype == T and v1.dtype == T
    return e1, v1


def _ok(x, invs):
    with np.errstate(all="ignore"):
        return np.isfinite(x) & (np.abs(x * invs) < QMAX)


def _axis(x, invs):
    u = x * invs - F(0.5)
    fl = np.floor(u)
    return fl.astype(np.int64), u - fl


def _inside(I, J, R, ox, oy):
    return (I >= ox) & (I < ox + R) & (J >= oy) & (J < oy + R)


def _index(I, J, R):
    return (J & (R - 1)) * R + (I & (R - 1))


def splat32(src, ox, oy, invs, x, y, V):
    """adds the splats of volumes V at (x, y) to src [R, R] int32 (memory order) in place; returns the dropped non-zero quanta of each"""
    R = src.shape[0]
    invs = F(invs)
    x, y, V = (np.atleast_1d(np.asarray(v, F)) for v in (x, y, V))
    ok = _ok(x, invs) & _ok(y, invs) & np.isfinite(V)
    dropped = np.zeros(len(x), np.int64)
    xs, ys, Vs = x[ok], y[ok], V[ok]
    with np.errstate(all="ignore"):
        units = (Vs * (invs * invs)) * PER_METRE
        Q = np.rint(np.fmin(np.fmax(units, -QMAX), QMAX)).astype(np.int64)
        (I0, wx), (J0, wy) = _axis(xs, invs), _axis(ys, invs)
        ux, uy = F(1) - wx, F(1) - wy
        fq = Q.astype(np.int32).astype(F)
        q0 = np.rint(fq * (ux * uy)).astype(np.int64)
        q1 = np.rint(fq * (wx * uy)).astype(np.int64)
        q2 = np.rint(fq * (ux * wy)).astype(np.int64)
        q3 = Q - ((q0 + q1) + q2)
    flat = src.reshape(-1)
    d = np.zeros(len(xs), np.int64)
    for k, q in enumerate((q0, q1, q2, q3)):
        I, J = I0 + (k & 1), J0 + (k >> 1)
        nz = (q != 0) & (Q != 0)
        ins = _inside(I, J, R, ox, oy)
        np.add.at(flat, _index(I, J, R)[nz & ins], q[nz & ins].astype(np.int32))
        d += nz & ~ins
    dropped[ok] = d
    return dropped


def sample32(state, ox, oy, invs, points):
    """[n, 4] float32 samples (height, d/dx, d/dy, rate) of the state [R, R, 2] (memory order) at points [n, 2]"""
    R = state.shape[0]
    invs = F(invs)
    p = np.asarray(points, F).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    out = np.zeros((len(p), 4), F)
    fin = np.isfinite(x) & np.isfinite(y)
    out[~fin] = np.nan
    ok = fin & _ok(x, invs) & _ok(y, invs)
    xs, ys = x[ok], y[ok]
    (I0, wx), (J0, wy) = _axis(xs, invs), _axis(ys, invs)
    flat = state.reshape(-1, 2)
    c = []
    for k in range(4):
        I, J = I0 + (k & 1), J0 + (k >> 1)
        ins = _inside(I, J, R, ox, oy)
        c.append(np.where(ins[:, None], flat[_index(I, J, R)], F(0)).astype(F))
    a0, a1 = c[1][:, 0] - c[0][:, 0], c[3][:, 0] - c[2][:, 0]
    e0, e1 = c[0][:, 0] + wx * a0, c[2][:, 0] + wx * a1
    r0, r1 = c[0][:, 1] + wx * (c[1][:, 1] - c[0][:, 1]), c[2][:, 1] + wx * (c[3][:, 1] - c[2][:, 1])
    res = np.stack([e0 + wy * (e1 - e0), (a0 + wy * (a1 - a0)) * invs, (e1 - e0) * invs, r0 + wy * (r1 - r0)], 1)
    assert res.dtype == F
    out[ok] = res
    return out


class Layer:
    """the layer as the handle keeps it; dtype float32 (the bits) or float64 (the same arithmetic, wider)"""

    def __init__(self, R, s, dtype=F, c=2.0, gamma=0.05, B=8, sponge_gamma=4.0):
        self.R, self.s, self.T = R, F(s), dtype
        self.invs = F(1.0 / float(F(s)))
        self.ox = self.oy = -R // 2
        self.eta, self.rate = np.zeros((R, R), dtype), np.zeros((R, R), dtype)
        self.src = np.zeros((R, R), np.int32)
        self.c, self.gamma, self.B, self.sponge_gamma = c, gamma, B, sponge_gamma

    def cell_of(self, x):
        return int(np.floor(F(x) * self.invs))

    def center(self, x, y):
        self.move(self.cell_of(x) - self.R // 2, self.cell_of(y) - self.R // 2)

    def move(self, ox, oy):
        """the cells that entered are water at rest: a memory cell whose world cell changed"""
        R, m = self.R, np.arange(self.R)
        world = lambda o: o + ((m - o) & (R - 1))
        ent = (world(ox) != world(self.ox))[None, :] | (world(oy) != world(self.oy))[:, None]
        self.eta[ent], self.rate[ent], self.src[ent] = 0, 0, 0
        self.ox, self.oy = ox, oy

    def step(self, dt, substeps=1, mistake=None):
        h, c2s2, f = params(self.c, self.s, self.gamma, self.B, self.sponge_gamma, dt, substeps)
        for i in range(substeps):
            self.eta, self.rate = substep(self.eta, self.rate, self.src, self.ox, self.oy, self.B, h, c2s2, f, i == 0, self.T, mistake)
            if i == 0:
                self.src = np.zeros_like(self.src)

    def deposit(self, impulses):
        imp = np.asarray(impulses, F).reshape(-1, 4)
        return splat32(self.src, self.ox, self.oy, self.invs, imp[:, 0], imp[:, 1], imp[:, 2])

    def window(self, a=None):
        """memory order -> window order: [j][i] is cell (ox + i, oy + j)"""
        a = np.stack([self.eta, self.rate], 2) if a is None else a
        return np.roll(a, (-(self.oy & (self.R - 1)), -(self.ox & (self.R - 1))), (0, 1))

    def set_window(self, eta, rate, src=None):
        """window order -> memory order"""
        sh = (self.oy & (self.R - 1), self.ox & (self.R - 1))
        self.eta, self.rate = np.roll(np.asarray(eta, self.T), sh, (0, 1)), np.roll(np.asarray(rate, self.T), sh, (0, 1))
        if src is not None:
            self.src = np.roll(np.asarray(src, np.int32), sh, (0, 1))

    def state(self):
        return np.stack([self.eta, self.rate], 2)

    def sample(self, points):
        return sample32(self.state().astype(F), self.ox, self.oy, self.invs, points)


def wake_terms32(bodies, motions, probes, recs, dt):
    """per probe row: (terms [rows, 8] without field 3, splats: list of (x, y, V, mask) in the order the kernel issues them)"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    recs = np.asarray(recs, F).reshape(-1, 8)
    dt = F(dt)
    bi, _ = body64._gather(bodies, probes)
    w, a, _ = body64.world32(bodies, probes)
    T, cap = bodies["position"][bi], bodies["cap"][bi]
    v, o = motions["linear"][bi], motions["angular"][bi]
    with np.errstate(all="ignore"):
        d = np.fmin(np.fmax(recs[:, 2] - w[:, 2], F(0)), cap)
        m = a * d
        rx, ry, rz = w[:, 0] - T[:, 0], w[:, 1] - T[:, 1], w[:, 2] - T[:, 2]
        ux = v[:, 0] + (o[:, 1] * rz - o[:, 2] * ry)
        uy = v[:, 1] + (o[:, 2] * rx - o[:, 0] * rz)
        uz = v[:, 2] + (o[:, 0] * ry - o[:, 1] * rx)
        ex, ey, ez = recs[:, 4] - ux, recs[:, 5] - uy, recs[:, 6] - uz
        sx, sy = -(ex * dt), -(ey * dt)
        heave = (F(0) < d) & (d < cap)
        wet = d > 0
        Vh = (a * -ez) * dt
        z = np.zeros_like(m)
        t = np.stack([np.where(heave, Vh, z), np.where(wet, m * sx, z), np.where(wet, m * sy, z), z, z, z, m, recs[:, 3]], 1)
    assert t.dtype == F
    splats = [(w[:, 0], w[:, 1], Vh, heave), (w[:, 0], w[:, 1], -m, wet), (w[:, 0] + sx, w[:, 1] + sy, m, wet)]
    return t, splats


def wake32(bodies, motions, probes, recs, dt, src, ox, oy, invs):
    """[nbodies, 8] float32 records of datum_ocean_deposit_body_ripples from given velocity records, and the deposits added to src in place:
    body64.reduce32's walk over wake_terms32.  A body with a bad range or motion walks no probe; a body with a bad probe deposits its
    other probes and has a NaN record, as the kernel"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    t, splats = wake_terms32(bodies, motions, probes, recs, dt)
    _, _, pbad = body64.world32(bodies, probes)
    off, _ = body64.offsets(bodies, len(probes))
    rbad = body64.range_bad(bodies, len(probes))
    mbad = drag64.motion_bad(motions)
    bi, _ = body64._gather(bodies, probes)
    live = ~pbad & ~mbad[bi]
    for x, y, V, mask in splats:
        sel = live & mask
        dropped = np.zeros(len(t), np.int64)
        dropped[sel] = splat32(src, ox, oy, invs, x[sel], y[sel], V[sel])
        t[:, 3] += dropped.astype(F)
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
