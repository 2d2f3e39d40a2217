"""Float64 reference of the several-cascade calls (include/datum_ocean_hip.h: datum_ocean_gen_blend, datum_ocean_sample_surface_blend),
on top of surface64.py and gen64.py.

At a position P every listed cascade c is sampled at P.xy * scale_c (REPEAT bilinear); the displacements add, the normals add as slopes
p_c = (m_c.x / m_c.z, m_c.y / m_c.z), dn = normalize(sum p_c.x, sum p_c.y, 1).  Foam: the largest coverage (accumulate), 1 + sum (J_c - 1)
(jacobian), 0 (off).  `mistake` plants the errors the sensitivity test names: "swap" (the first two scales exchanged), "drop" (the last
cascade left out), "normals" (unit normals summed instead of slopes), "min" (min instead of max of the coverage).
"""

from types import SimpleNamespace

import numpy as np

import gen64
import surface64


def _plan(maps_list, scales, mistake):
    maps_list, scales = list(maps_list), [float(x) for x in scales]
    if mistake == "swap":
        scales[0], scales[1] = scales[1], scales[0]
    if mistake == "drop":
        maps_list, scales = maps_list[:-1], scales[:-1]
    return maps_list, scales


def evaluate_blend64(maps_list, scales, s, b):
    """(V [3][M], theta, P (px, py)) of the summed surface at base points b [2][M]"""
    f = surface64.frame64(s)
    theta = f["frequency"] * (f["dirx"] * b[0] + f["diry"] * b[1]) + f["phase"]
    g = f["qi"] * f["A"] * np.cos(theta)
    px, py = b[0] + g * f["dirx"], b[1] + g * f["diry"]
    D = None
    for maps, sc in zip(maps_list, scales):
        m0 = np.asarray(maps, np.float64)[0].transpose(2, 0, 1)[:3]
        Dc = surface64.bilinear64(m0, px * sc, py * sc)
        D = Dc if D is None else D + Dc
    V = np.stack([px - D[0], py - D[1], f["basez"] + f["A"] * np.sin(theta) + D[2]])
    return V, theta, (px, py)


def slopes64(samples, mistake=None):
    """dn [3][...] from the list of sampled normals m_c [3][...]"""
    if mistake == "normals":
        n = sum(samples)
        return n / np.sqrt((n * n).sum(0))
    px = sum(m[0] / m[2] for m in samples)
    py = sum(m[1] / m[2] for m in samples)
    n = np.stack([px, py, np.ones_like(px)])
    return n / np.sqrt((n * n).sum(0))


def surface_blend64(maps_list, foams, mode, scales, s, points, iterations, mistake=None):
    """(M, 8) float64 records.  `foams`: the planes [N][N] in list order or None; `mode`: "off", "accumulate" or "jacobian";
    `scales`: 1 / wavescale per listed cascade (the handle's fp32 values)."""
    foams = None if foams is None or mode == "off" else list(foams)
    if mistake == "drop" and foams is not None:
        foams = foams[:-1]
    maps_list, scales = _plan(maps_list, scales, mistake)
    q = np.asarray(points, np.float64).reshape(-1, 2).T.copy()
    ok = np.isfinite(q).all(0)
    qq = np.where(ok, q, 0.0)
    b = qq.copy()
    for _ in range(iterations):
        V, _, _ = evaluate_blend64(maps_list, scales, s, b)
        b = b + (qq - V[:2])
    V, theta, (px, py) = evaluate_blend64(maps_list, scales, s, b)
    f = surface64.frame64(s)
    samples = [surface64.bilinear64(np.asarray(maps, np.float64)[1].transpose(2, 0, 1)[:3], px * sc, py * sc) for maps, sc in zip(maps_list, scales)]
    dn = slopes64(samples, mistake)
    st, ct = np.sin(theta), np.cos(theta)
    phi, qi, dx, dy = f["phi"], f["qi"], f["dirx"], f["diry"]
    t2 = surface64._normalize(np.stack([-(phi * dx / 6) * ct, -(phi * dy / 6) * ct, 1 - qi * phi * st]))
    t0 = surface64._normalize(np.stack([1 - qi * phi * dx * dx * st, -qi * phi * dy * dx * st, (phi * dx / 6) * ct]))
    t1 = np.cross(t0.T, t2.T).T
    n = surface64._normalize(t0 * dn[0] + t1 * dn[1] + t2 * dn[2])
    fo = np.zeros_like(px)
    if foams is not None:
        planes = [surface64.bilinear64(np.asarray(fp, np.float64), px * sc, py * sc) for fp, sc in zip(foams, scales)]
        if mode == "accumulate":
            fo = np.minimum.reduce(planes) if mistake == "min" else np.maximum.reduce(planes)
        else:
            fo = 1.0 + sum(p - 1.0 for p in planes)
    res = np.hypot(V[0] - qq[0], V[1] - qq[1])
    out = np.concatenate([V, res[None], n, fo[None]]).T
    out[~ok] = np.nan
    return out


def _with_scale(s, scale):
    c = type(s).from_buffer_copy(bytes(s))
    c.scale = float(scale)
    return c


def staged_blend64(s, maps_list, scales, ray, st=None, ct=None, mistake=None):
    """gen.comp:93-137 of the summed surface in float64 downstream of gen64.ray32's fp32 values, as gen64.staged64 is for one cascade (each
    cascade's texel coordinate in fp32 from the fp32 position, with ITS scale).  Returns a namespace: vertices [sizey, sizex, 12],
    position, displacement (the sum), terms (per cascade: its displacement and the largest |corner texel|), dn."""
    maps_list, scales = _plan(maps_list, scales, mistake)
    first, terms, normals = None, [], []
    for maps, sc in zip(maps_list, scales):
        sc_set = _with_scale(s, sc)
        r = gen64.staged64(sc_set, maps, ray, st, ct)
        first = r if first is None else first
        terms.append(SimpleNamespace(displacement=r.displacement, corner=r.corner))
        # staged64 samples layer 0 into .displacement: layer 1 put in its place gives the cascade's sampled normal
        normals.append(np.moveaxis(gen64.staged64(sc_set, np.stack([maps[1], maps[1]]), ray, st, ct).displacement, -1, 0))
    disp = sum(t.displacement for t in terms)
    dn = np.moveaxis(slopes64(normals, mistake), 0, -1)

    stv, ctv = first.st, first.ct
    plane = np.array(list(s.plane), np.float64)
    nc, tc = ray.normal_c.astype(np.float64), ray.tangent_c.astype(np.float64)
    normal = np.stack([nc[0] * ctv, nc[1] * ctv, nc[2] * stv], -1)
    tangent = np.stack([tc[0] * stv, tc[1] * stv, tc[2] * ctv], -1)
    tbn2 = gen64._unit(np.stack([-normal[..., 0], -normal[..., 1], 1 - normal[..., 2]], -1))
    tbn0 = gen64._unit(np.stack([1 - tangent[..., 0], -tangent[..., 1], tangent[..., 2]], -1))
    tbn1 = np.cross(tbn0, tbn2)
    smoothing = first.smoothing[..., None]
    tn = dn[..., 0:1] * tbn0 + dn[..., 1:2] * tbn1 + dn[..., 2:3] * tbn2
    tbn2 = gen64._unit(tn * (1 - smoothing) + plane[:3] * smoothing)
    tbn0 = gen64._unit(np.array([1.0, 0.0, 0.0]) - tbn2[..., 0:1] * tbn2)

    position = first.position
    out = np.empty(position.shape[:2] + (12,))
    out[..., 0] = position[..., 0] - disp[..., 0]
    out[..., 1] = position[..., 1] - disp[..., 1]
    out[..., 2] = position[..., 2] + disp[..., 2]
    out[..., 3:5] = float(np.float32(0.1)) * position[..., :2]
    out[..., 5:8] = tbn2
    out[..., 8:11] = tbn0
    out[..., 11] = -1
    return SimpleNamespace(vertices=out, position=position, displacement=disp, terms=terms, dn=dn)
