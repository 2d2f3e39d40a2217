"""Float64 reference of the surface queries (include/datum_ocean_hip.h: datum_ocean_sample_surface).

For a base point b in the plane, with gen's own constants (ocean_gen.hip: make_gen_frame):
    theta = frequency (swelldirection . b) + swellphase,            frequency = 2 pi / swelllength
    P(b)  = b + qi A swelldirection cos(theta),                      qi = swellsteepness / (frequency A 4 + 1e-6), A = swellamplitude
    t     = P(b) scale                                               REPEAT bilinear, texel centres at (i + 0.5) / N
    V(b)  = (P.x - D.x, P.y - D.y, -plane.w + A sin(theta) + D.z)    D = layer 0 of the map at t
The query of q starts at b = q, applies `iterations` updates b <- b + (q - V(b).xy) and evaluates once more.  Record: V, |V.xy - q|,
gen's tbn[2] with smoothing = 0, the foam plane at t.  Inputs are the logical maps ([2][N][N][4], read_maps / capi.map_layers), the foam
plane ([N][N] or None), a datum_ocean_set (capi.OceanSet or anything with its fields), the points and the iteration count.
"""

import math

import numpy as np


def frame64(s):
    """gen's per-launch swell constants in float64 from the set's fields"""
    A = float(s.swellamplitude)
    frequency = 2.0 * math.pi / float(s.swelllength)
    qi = float(s.swellsteepness) / (frequency * A * 4.0 + 1e-6)
    phi = frequency * A
    return dict(A=A, frequency=frequency, qi=qi, phi=phi, phase=float(s.swellphase), dirx=float(s.swelldirection[0]),
                diry=float(s.swelldirection[1]), scale=float(s.scale), basez=-float(s.plane[3]))


def bilinear64(planes, tx, ty):
    """REPEAT bilinear fetch of [..., N, N] planes (row y, column x) at texture coordinates (tx, ty): texel centres at (i + 0.5) / N"""
    N = planes.shape[-1]
    fx, fy = tx * N - 0.5, ty * N - 0.5
    flx, fly = np.floor(fx), np.floor(fy)
    ax, ay = fx - flx, fy - fly
    i0, j0 = np.mod(flx, N).astype(np.int64), np.mod(fly, N).astype(np.int64)
    i1, j1 = (i0 + 1) % N, (j0 + 1) % N
    return ((1 - ax) * (1 - ay) * planes[..., j0, i0] + ax * (1 - ay) * planes[..., j0, i1]
            + (1 - ax) * ay * planes[..., j1, i0] + ax * ay * planes[..., j1, i1])


def _normalize(v):
    return v / np.sqrt((v * v).sum(0))


def evaluate64(maps, s, b):
    """(V [3][M], theta, texcoord (tx, ty)) at base points b [2][M]"""
    f = frame64(s)
    m0 = np.asarray(maps, np.float64)[0].transpose(2, 0, 1)[:3]             # (dx, dy, dz) planes
    theta = f["frequency"] * (f["dirx"] * b[0] + f["diry"] * b[1]) + f["phase"]
    g = f["qi"] * f["A"] * np.cos(theta)
    px, py = b[0] + g * f["dirx"], b[1] + g * f["diry"]
    tx, ty = px * f["scale"], py * f["scale"]
    D = bilinear64(m0, tx, ty)
    V = np.stack([px - D[0], py - D[1], f["basez"] + f["A"] * np.sin(theta) + D[2]])
    return V, theta, (tx, ty)


def surface64(maps, foam, s, points, iterations):
    """(M, 8) float64 records of the definition"""
    q = np.asarray(points, np.float64).reshape(-1, 2).T.copy()
    ok = np.isfinite(q).all(0)
    qq = np.where(ok, q, 0.0)
    b = qq.copy()
    for _ in range(iterations):
        V, _, _ = evaluate64(maps, s, b)
        b = b + (qq - V[:2])
    V, theta, (tx, ty) = evaluate64(maps, s, b)
    f = frame64(s)
    m1 = np.asarray(maps, np.float64)[1].transpose(2, 0, 1)[:3]
    m = bilinear64(m1, tx, ty)
    st, ct = np.sin(theta), np.cos(theta)
    phi, qi, dx, dy = f["phi"], f["qi"], f["dirx"], f["diry"]
    t2 = _normalize(np.stack([-(phi * dx / 6) * ct, -(phi * dy / 6) * ct, 1 - qi * phi * st]))
    t0 = _normalize(np.stack([1 - qi * phi * dx * dx * st, -qi * phi * dy * dx * st, (phi * dx / 6) * ct]))
    t1 = np.cross(t0.T, t2.T).T
    n = _normalize(t0 * m[0] + t1 * m[1] + t2 * m[2])
    fo = bilinear64(np.asarray(foam, np.float64), tx, ty) if foam is not None else np.zeros_like(tx)
    res = np.hypot(V[0] - qq[0], V[1] - qq[1])
    out = np.concatenate([V, res[None], n, fo[None]]).T
    out[~ok] = np.nan
    return out


def texcoord64(maps, s, points, iterations):
    """the converged texture coordinate (tx, ty) of each point (where the foam is sampled)"""
    q = np.asarray(points, np.float64).reshape(-1, 2).T.copy()
    b = q.copy()
    for _ in range(iterations):
        V, _, _ = evaluate64(maps, s, b)
        b = b + (q - V[:2])
    return evaluate64(maps, s, b)[2]
