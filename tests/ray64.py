"""Ray casts on the summed surface (include/datum_ocean_hip.h: datum_ocean_cast_rays) restated twice:

  cast32   the definition in numpy float32, every operation one rounding as written, vectorised over the rays: the march's samples, the
           first change of side, the refinement and the record.  `height_fn(points [M, 2]) -> records [M, 8]` is the several-cascade
           query (oc.read_surface_blend on a device, an analytic surface on a CPU); it is called at most S + R + 2 times;
  cast64   the same in float64 over a float64 height_fn (blend64.surface_blend64 through height64).

Rays are an (n, 8) array (ox, oy, oz, tmin, dx, dy, dz, tmax), records (n, 12): hi, lo, g(hi), status, the query's record at hi.  Both
return a namespace: records, index (the march's i of the bracket, 0 for a miss and for a bad ray), side (below(t_0)), bad, calls (how often
height_fn was called) and gmin (the smallest |g| over the march samples t_0 ... t_index, t_S for a miss; in units of `bar` where a per-ray
bar is given: the float64 side's measure of how close a ray's march came to the surface).
`mistake` plants the errors tests/test_ray64.py names: "last" (the last crossing of the march instead of the first), "lo_for_hi" (the
record's field 0 and its sample taken at lo), "skip_tS" (the march ends at t_(S-1)).
"""

from types import SimpleNamespace

import numpy as np

import blend64

F = np.float32
MISS, ENTER, LEAVE = 0, 1, 2
RAY_FLOATS, RECORD_FLOATS = 8, 12


def bad32(rays):
    """the bad-ray rule, in float32 as the header writes it: a non-finite field, tmax < tmin, a non-finite point(tmin) or point(tmax)"""
    r = np.asarray(rays, F).reshape(-1, RAY_FLOATS)
    with np.errstate(all="ignore"):
        ends = [r[:, j] + r[:, t] * r[:, 4 + j] for t in (3, 7) for j in range(3)]
        return ~np.isfinite(r).all(1) | (r[:, 7] < r[:, 3]) | ~np.isfinite(np.stack(ends, 1)).all(1)


def _point(r, t):
    return r[:, 0] + t * r[:, 4], r[:, 1] + t * r[:, 5], r[:, 2] + t * r[:, 6]


def _cast(height_fn, rays, S, R, T, mistake=None, bar=None):
    r32 = np.asarray(rays, F).reshape(-1, RAY_FLOATS)
    n = len(r32)
    bad = bad32(r32)
    # a bad ray takes no part: a harmless stand-in is marched in its place and its record overwritten
    r = np.where(bad[:, None], np.array([0, 0, 0, 0, 0, 0, 0, 0], F), r32).astype(T)
    tmin, tmax = r[:, 3], r[:, 7]
    calls = [0]

    def g_of(t):
        """(g(t), the records at point(t)); a non-finite q has the query's NaN record"""
        x, y, z = _point(r, t)
        calls[0] += 1
        rec = np.asarray(height_fn(np.stack([x, y], 1)), T).reshape(n, 8)
        return z - rec[:, 2], rec

    unit = T(1.0) if bar is None else np.asarray(bar, np.float64)

    with np.errstate(all="ignore"):
        inv = T(1.0) / T(S)
        delta = (tmax - tmin) * inv
        assert delta.dtype == T

        g, _ = g_of(tmin + T(0) * delta)
        side = g < 0
        open_ = np.ones(n, bool)                     # still marching
        lo, hi = tmax.copy(), tmax.copy()
        index = np.zeros(n, np.int64)
        gmin = np.abs(g) / unit
        last = tmin + T(0) * delta
        gprev = g
        end = S - 1 if mistake == "skip_tS" else S
        for i in range(1, end + 1):
            if not open_.any():
                break
            t = tmax.copy() if i == S else tmin + T(i) * delta
            g, _ = g_of(t)
            if mistake == "last":
                cross = (g < 0) != (gprev < 0)       # every change of side along the march: the last one is kept
            else:
                cross = open_ & ((g < 0) != side)
                gmin = np.where(open_, np.fmin(gmin, np.abs(g) / unit), gmin)
                open_ &= ~cross
            lo, hi, index = np.where(cross, last, lo), np.where(cross, t, hi), np.where(cross, i, index)
            gprev, last = g, t
        hit = index > 0

        for _ in range(R):
            if not hit.any():
                break
            mid = T(0.5) * (lo + hi)
            g, _ = g_of(mid)
            same = (g < 0) == side
            lo, hi = np.where(hit & same, mid, lo), np.where(hit & ~same, mid, hi)

        at = lo if mistake == "lo_for_hi" else hi
        g, rec = g_of(at)
        status = np.where(hit, np.where(side, LEAVE, ENTER), MISS).astype(T)
        out = np.concatenate([np.stack([at, lo, g, status], 1), rec], 1)
    assert out.dtype == T
    out[bad] = np.nan
    index[bad] = 0
    return SimpleNamespace(records=out, index=index, side=side, bad=bad, calls=calls[0], gmin=gmin)


def cast32(height_fn, rays, S, R, mistake=None):
    """the definition in float32; .records is what datum_ocean_read_rays gives, bit for bit, where height_fn is the query"""
    c = _cast(height_fn, rays, S, R, F, mistake)
    assert c.calls <= S + R + 2
    return c


def cast64(height_fn, rays, S, R, mistake=None, bar=None):
    """the definition in float64 on the same fp32 rays"""
    return _cast(height_fn, rays, S, R, np.float64, mistake, bar)


def height64(maps_list, foams, mode, scales, s, iterations):
    """cast64's height_fn over blend64.surface_blend64"""
    return lambda q: blend64.surface_blend64(maps_list, foams, mode, scales, s, q, iterations)


def samples32(rays, S):
    """t_i [n, S + 1] in float32"""
    r = np.asarray(rays, F).reshape(-1, RAY_FLOATS)
    with np.errstate(all="ignore"):
        delta = (r[:, 7] - r[:, 3]) * (F(1.0) / F(S))
        t = np.stack([r[:, 3] + F(i) * delta for i in range(S)] + [r[:, 7]], 1)
    assert t.dtype == F
    return t
