"""Float64 reference of the Jacobian foam plane (include/datum_ocean_hip.h: datum_ocean_set_foam).

The mesh places each vertex at p - D(p), D = (dx, dy) of map layer 0.  Per texel
    J = (1 - a)(1 - d) - b c,  a = d/dx dx,  b = d/dy dx,  c = d/dx dy,  d = d/dy dy
with periodic central differences in world units, (f[i+1] - f[i-1]) / (2 h), h = wavescale / N; x = column, y = row.
"""

import numpy as np


def _dxdy(maps):
    """(dx, dy) in float64 from read_maps' [2][N][N][4] image or from ref64.displace64's [6][N][N] channels"""
    m = np.asarray(maps)
    if m.ndim == 4:
        return m[0, ..., 0].astype(np.float64), m[0, ..., 1].astype(np.float64)
    return m[0].astype(np.float64), m[1].astype(np.float64)


def parts64(maps, wavescale, N):
    """(a, b, c, d): the four derivatives in float64"""
    dx, dy = _dxdy(maps)
    assert dx.shape == (N, N)
    inv2h = N / (2.0 * float(wavescale))

    def ddx(f):
        return (np.roll(f, -1, axis=1) - np.roll(f, 1, axis=1)) * inv2h

    def ddy(f):
        return (np.roll(f, -1, axis=0) - np.roll(f, 1, axis=0)) * inv2h

    return ddx(dx), ddy(dx), ddx(dy), ddy(dy)


def jacobian64(maps, wavescale, N):
    """J per texel, float64 [N][N]"""
    a, b, c, d = parts64(maps, wavescale, N)
    return (1.0 - a) * (1.0 - d) - b * c


def scale64(maps, wavescale, N):
    """|(1 - a)(1 - d)| + |b c| + 1: the magnitude the kernel's fp32 arithmetic is measured against"""
    a, b, c, d = parts64(maps, wavescale, N)
    return np.abs((1.0 - a) * (1.0 - d)) + np.abs(b * c) + 1.0


def coverage64(J, threshold, gain):
    """clamp((threshold - J) gain, 0, 1)"""
    return np.clip((threshold - np.asarray(J, np.float64)) * gain, 0.0, 1.0)
