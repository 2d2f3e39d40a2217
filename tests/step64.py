"""Body stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies) restated twice, beside body64.py and drag64.py:

  integrate32   one sub-step in numpy float32, every operation one rounding as written, from the records of the two existing calls for the
                same pose and motion: datum_ocean_reduce_bodies' (fields 0-2: M, bx, by) and datum_ocean_reduce_body_drag's (fields 0-5: the
                drag's force and torque, 7: the residual).  Bad bodies (a NaN record, non-finite props, a non-finite integrated state) keep
                pose and motion and get a NaN record;
  integrate64   the same formulas in float64, without the bad-body rules.

Bodies and motions are body64's and drag64's structured arrays; props are PROPS below (32 bytes, the header's datum_ocean_body_props).
`mistake` plants the errors tests/test_step64.py names:
  "explicit"    T' = T + h v  with the OLD velocity            "transposed"   R and its transpose swapped in the angular step
  "by_sign"     tau.y = -buoyancy by + D.tau y                 "gs_order"     Gram-Schmidt with the second column first
"""

import numpy as np

import body64
import drag64

F = np.float32

PROPS = np.dtype([("invmass", F), ("invinertia", F, 3), ("gravity", F), ("buoyancy", F), ("pad", F, 2)], align=False)
assert PROPS.itemsize == 32

RECORD_FLOATS = 8
MAX_SUBSTEPS = 16

MISTAKES = ("explicit", "transposed", "by_sign", "gs_order")


def make_props(invmass, invinertia, gravity, buoyancy):
    n = len(np.asarray(invmass).reshape(-1))
    p = np.zeros(n, PROPS)
    p["invmass"] = invmass
    p["invinertia"] = np.asarray(invinertia, F).reshape(-1, 3)
    p["gravity"], p["buoyancy"] = gravity, buoyancy
    return p


def props_bad(props):
    return ~(np.isfinite(props["invmass"]) & np.isfinite(props["invinertia"]).all(1) & np.isfinite(props["gravity"]) & np.isfinite(props["buoyancy"]))


def step_size(dt, substeps):
    """h = dt * (1.0f / (float)substeps), two fp32 operations"""
    return F(dt) * (F(1) / F(substeps))


def _norm(a):
    return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(o, c):
    """drag_terms' u: (o.y c.z - o.z c.y, o.z c.x - o.x c.z, o.x c.y - o.y c.x)"""
    return [o[1] * c[2] - o[2] * c[1], o[2] * c[0] - o[0] * c[2], o[0] * c[1] - o[1] * c[0]]


def _substep(t, sums, R, T, v, o, P, h, mistake=None):
    """the sub-step in the dtype t on lists of [n] arrays: sums = (M, bx, by, D0..D5); R 9 entries row-major, T, v, o 3 each; P = (invmass,
    invinertia x 3, gravity, buoyancy).  Returns (R', T', v', o', force, torque)"""
    assert all(a.dtype == t for a in list(sums) + R + T + v + o + list(P)) and type(h) is t
    M, bx, by = sums[:3]
    D = sums[3:9]
    invmass, ii, g, rho = P[0], P[1:4], P[4], P[5]
    with np.errstate(all="ignore"):
        force = [D[0], D[1], rho * M + D[2]]
        torque = [rho * bx + D[3], (-(rho * by) if mistake == "by_sign" else rho * by) + D[4], D[5]]

        vn = [v[0] + h * (force[0] * invmass), v[1] + h * (force[1] * invmass), v[2] + h * (force[2] * invmass - g)]
        Tn = [T[k] + h * (v[k] if mistake == "explicit" else vn[k]) for k in range(3)]

        if mistake == "transposed":
            ab = [((R[3 * j] * torque[0] + R[3 * j + 1] * torque[1]) + R[3 * j + 2] * torque[2]) * ii[j] for j in range(3)]
            al = [(R[k] * ab[0] + R[3 + k] * ab[1]) + R[6 + k] * ab[2] for k in range(3)]
        else:
            ab = [((R[j] * torque[0] + R[3 + j] * torque[1]) + R[6 + j] * torque[2]) * ii[j] for j in range(3)]
            al = [(R[3 * k] * ab[0] + R[3 * k + 1] * ab[1]) + R[3 * k + 2] * ab[2] for k in range(3)]
        on = [o[k] + h * al[k] for k in range(3)]

        c = []
        for j in range(2):
            col = [R[j], R[3 + j], R[6 + j]]
            w = _cross(on, col)
            c.append([col[k] + h * w[k] for k in range(3)])
        if mistake == "gs_order":
            n1 = _norm(c[1])
            y = [c[1][k] / n1 for k in range(3)]
            d = _dot(y, c[0])
            x0 = [c[0][k] - d * y[k] for k in range(3)]
            n0 = _norm(x0)
            x = [x0[k] / n0 for k in range(3)]
        else:
            n0 = _norm(c[0])
            x = [c[0][k] / n0 for k in range(3)]
            d = _dot(x, c[1])
            y0 = [c[1][k] - d * x[k] for k in range(3)]
            n1 = _norm(y0)
            y = [y0[k] / n1 for k in range(3)]
        z = _cross(x, y)
        Rn = [None] * 9
        for k in range(3):
            Rn[3 * k], Rn[3 * k + 1], Rn[3 * k + 2] = x[k], y[k], z[k]
    out = Rn + Tn + vn + on + force + torque
    assert all(a.dtype == t for a in out)
    return Rn, Tn, vn, on, force, torque


def _unpack(t, lift, drag, bodies, motions, props):
    lift, drag = np.asarray(lift, t).reshape(-1, 8), np.asarray(drag, t).reshape(-1, 8)
    sums = [lift[:, 0], lift[:, 1], lift[:, 2]] + [drag[:, k] for k in range(6)]
    R = [bodies["rotation"][:, k].astype(t) for k in range(9)]
    T = [bodies["position"][:, k].astype(t) for k in range(3)]
    v = [motions["linear"][:, k].astype(t) for k in range(3)]
    o = [motions["angular"][:, k].astype(t) for k in range(3)]
    P = [props["invmass"].astype(t)] + [props["invinertia"][:, k].astype(t) for k in range(3)] + [props["gravity"].astype(t), props["buoyancy"].astype(t)]
    return sums, R, T, v, o, P


def integrate32(lift, drag, bodies, motions, props, h, mistake=None):
    """(bodies', motions', records [n, 8] float32, bad [n]) after one sub-step of length h (a float32) from the two calls' records"""
    lift, drag = np.asarray(lift, F).reshape(-1, 8), np.asarray(drag, F).reshape(-1, 8)
    Rn, Tn, vn, on, force, torque = _substep(F, *_unpack(F, lift, drag, bodies, motions, props), F(h), mistake)
    nb, nm = bodies.copy(), motions.copy()
    nb["rotation"], nb["position"] = np.stack(Rn, 1), np.stack(Tn, 1)
    nm["linear"], nm["angular"] = np.stack(vn, 1), np.stack(on, 1)
    rec = np.stack(force + torque + [lift[:, 0], drag[:, 7]], 1)
    assert rec.dtype == F
    finite = np.isfinite(nb["rotation"]).all(1) & np.isfinite(nb["position"]).all(1) & ~drag64.motion_bad(nm)
    bad = np.isnan(lift).any(1) | np.isnan(drag).any(1) | props_bad(props) | ~finite
    nb[bad], nm[bad], rec[bad] = bodies[bad], motions[bad], np.nan
    return nb, nm, rec, bad


def integrate64(lift, drag, bodies, motions, props, h, mistake=None):
    """dict of float64 arrays after the same sub-step in float64: rotation [n, 9], position, linear, angular, force, torque [n, 3]"""
    t = np.float64
    Rn, Tn, vn, on, force, torque = _substep(t, *_unpack(t, lift, drag, bodies, motions, props), t(h), mistake)
    return dict(rotation=np.stack(Rn, 1), position=np.stack(Tn, 1), linear=np.stack(vn, 1), angular=np.stack(on, 1), force=np.stack(force, 1),
                torque=np.stack(torque, 1))


def sums32(lift, drag):
    """[n, 10] float32: the ten sums of ocean_step.h's StepPartial from the two calls' records"""
    lift, drag = np.asarray(lift, F).reshape(-1, 8), np.asarray(drag, F).reshape(-1, 8)
    return np.concatenate([lift[:, :3], drag[:, :6], drag[:, 7:8]], 1)
