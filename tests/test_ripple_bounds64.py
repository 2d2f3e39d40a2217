"""The rippled slab's margin without a GPU (include/datum_ocean_hip.h: datum_ocean_surface_slab_rippled): over the committed maps of
tests/golden/ocean_n64.npz and the R = 64 and R = 128 layer states of tests/test_rippled_emul.py (origin (37, -21)), the float64 rippled
height -- blend64's height of the summed surface plus the layer's bilinear height in float64 -- at every cell centre, at 10^4 random
points inside and outside the window, and with the layer's extreme cells placed over the maps' extreme texels, lies strictly inside
(zlo, zhi) of ripple_bounds64's restatement and no nearer to either bound than half of pad.  Each planted mistake of ripple_bounds64 that
moves a bound puts a height outside it.
"""

import os

import numpy as np
import pytest

import blend64
import bounds64
import ripple64
import ripple_bounds64
from test_surface_abi import _set

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ocean_n64.npz")
ORIGIN = (37, -21)
SCALE = F(1) / F(22)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _layer(R, cell, seed, lo=-0.3, hi=0.3, origin=ORIGIN):
    """tests/test_rippled_emul.py's layer state"""
    lay = ripple64.Layer(R, cell)
    lay.move(*origin)
    rng = np.random.RandomState(seed)
    lay.set_window(rng.uniform(lo, hi, (R, R)).astype(F), rng.uniform(-1, 1, (R, R)).astype(F))
    return lay


def _centres(lay):
    cell = float(lay.s)
    j, i = np.mgrid[0:lay.R, 0:lay.R]
    return np.stack([(lay.ox + i.ravel() + 0.5) * cell, (lay.oy + j.ravel() + 0.5) * cell], 1)


def _random(lay, n, seed):
    """inside the window, across its edge and well outside it"""
    cell, R = float(lay.s), lay.R
    lo = np.array([lay.ox, lay.oy]) * cell
    return lo + np.random.RandomState(seed).uniform(-0.5, 1.5, (n, 2)) * R * cell


def _heights(maps, cascades, scales, s, lay, points, iterations=4):
    q = np.asarray(points, F)
    return blend64.surface_blend64([maps] * len(cascades), None, "off", scales, s, q, iterations)[:, 2] + ripple_bounds64.eta64(lay, q)


@pytest.mark.parametrize("R,cell", [(64, 1.0), (128, 0.5)])
@pytest.mark.parametrize("steps", [1, 600])
def test_heights_lie_inside_the_rippled_slab(golden, steps, R, cell):
    maps = golden[f"maps_{steps}"]
    records = bounds64.fold_maps(maps)[None]
    lay = _layer(R, cell, R)
    layer = ripple_bounds64.fold(lay.state())
    assert layer[4] == 0 and layer[5] == R * R and layer[0] < -0.29 and layer[1] > 0.29
    points = np.concatenate([_centres(lay), _random(lay, 10000, R + steps)])
    worst = np.inf
    for cascades, scales in (([0], [SCALE]), ([0, 0, 0], [SCALE, F(1) / F(7), F(1) / F(3)])):
        for swell in (True, False):
            s = _set(A=0.6 if swell else 0.0, steep=0.5 if swell else 0.0, plane_w=-0.3)
            zlo, zhi, _, _, pad = ripple_bounds64.slab32(records, cascades, *bounds64.frame32(s), layer)
            z = _heights(maps, cascades, scales, s, lay, points)
            assert np.isfinite(z).all() and pad > 0
            assert np.all(z > float(zlo)) and np.all(z < float(zhi))
            nearest = min(float(z.min()) - float(zlo), float(zhi) - float(z.max())) / float(pad)
            print(f"rippled slab margin steps={steps} R={R} list={cascades} swell={swell}: [{float(zlo):.6f}, {float(zhi):.6f}], heights [{z.min():.6f}, {z.max():.6f}], "
                  f"nearest {nearest:.1f} pad")
            assert nearest >= 0.5
            worst = min(worst, nearest)
            # the fp32 sums against the same lines in float64: the slab's own rounding is a small share of pad
            lo64, hi64, _, _, pad64 = ripple_bounds64.slab64(records, cascades, *bounds64.frame32(s), layer)
            assert abs(float(zlo) - lo64) < 0.1 * pad64 and abs(float(zhi) - hi64) < 0.1 * pad64
            # the planted mistakes that lower the top: over an all-negative layer the water outside the window is not covered
            low = _layer(R, cell, R + 1, lo=-0.3, hi=-0.1)
            lowrec = ripple_bounds64.fold(low.state())
            zl = _heights(maps, cascades, scales, s, low, points)
            good = ripple_bounds64.slab32(records, cascades, *bounds64.frame32(s), lowrec)
            assert np.all(zl > float(good[0])) and np.all(zl < float(good[1]))
    print(f"rippled slab: nearest approach over the random points and the cell centres {worst:.3f} pad")


@pytest.mark.parametrize("steps", [1, 600])
def test_extreme_cells_over_extreme_texels(golden, steps):
    """cells of the maps' texel size (22 / 64 m) stand centre over centre with the texels: the layer's highest cell over the highest texel
    and its lowest over the lowest, no swell, no iteration -- the heights there are the un-padded sums, one pad inside"""
    maps = golden[f"maps_{steps}"]
    records = bounds64.fold_maps(maps)[None]
    R, cell = 64, 22.0 / 64.0
    s = _set(A=0.0, steep=0.0, plane_w=-0.3)
    dz = maps[0, ..., 2]
    (jl, il), (jh, ih) = np.unravel_index(dz.argmin(), dz.shape), np.unravel_index(dz.argmax(), dz.shape)
    for R in (64, 128):
        lay = _layer(R, cell, R)
        eta = lay.window()[..., 0].copy()
        rate = lay.window()[..., 1].copy()
        # window cell (i, j) is world cell (ox + i, oy + j), over texel ((ox + i) mod 64, (oy + j) mod 64)
        at = lambda it, jt: ((it - lay.ox) % 64, (jt - lay.oy) % 64)
        (i0, j0), (i1, j1) = at(il, jl), at(ih, jh)
        a, b = np.unravel_index(eta.argmin(), eta.shape), np.unravel_index(eta.argmax(), eta.shape)
        eta[a], eta[j0, i0] = eta[j0, i0], eta[a]
        b = np.unravel_index(eta.argmax(), eta.shape)
        eta[b], eta[j1, i1] = eta[j1, i1], eta[b]
        lay.set_window(eta, rate)
        layer = ripple_bounds64.fold(lay.state())
        assert eta[j0, i0] == layer[0] and eta[j1, i1] == layer[1]
        zlo, zhi, _, _, pad = ripple_bounds64.slab32(records, [0], *bounds64.frame32(s), layer)
        q = np.array([[(lay.ox + i0 + 0.5) * cell, (lay.oy + j0 + 0.5) * cell], [(lay.ox + i1 + 0.5) * cell, (lay.oy + j1 + 0.5) * cell]])
        ze = _heights(maps, [0], [SCALE], s, lay, q, iterations=0)
        edge = min(float(ze[0]) - float(zlo), float(zhi) - float(ze[1])) / float(pad)
        print(f"rippled slab at the extremes steps={steps} R={R}: heights {ze[0]:.6f}, {ze[1]:.6f} in [{float(zlo):.6f}, {float(zhi):.6f}], nearest {edge:.3f} pad")
        assert abs(ze[0] - (0.3 + float(records[0, 0]) + float(layer[0]))) < 2e-6 and abs(ze[1] - (0.3 + float(records[0, 1]) + float(layer[1]))) < 2e-6
        assert float(zlo) < ze[0] and ze[1] < float(zhi) and edge >= 0.5


@pytest.mark.parametrize("mistake", ripple_bounds64.MISTAKES)
def test_planted_mistakes_put_a_height_outside(golden, mistake):
    maps = golden["maps_60"]
    records = bounds64.fold_maps(maps)[None]
    R, cell = 64, 22.0 / 64.0
    s = _set(A=0.0, steep=0.0, plane_w=-0.3)
    lay = _layer(R, cell, 5, lo=-0.3, hi=-0.1)                                  # all negative
    layer = ripple_bounds64.fold(lay.state())
    dz = maps[0, ..., 2]
    jh, ih = np.unravel_index(dz.argmax(), dz.shape)
    # the highest texel's centre, one period outside the window: the water there stands at basez + zmax, the layer reads 0
    far = np.array([[(ih + 0.5) * cell + 22.0 * 40, (jh + 0.5) * cell]])
    z = _heights(maps, [0], [SCALE], s, lay, far, iterations=0)
    good = ripple_bounds64.slab32(records, [0], *bounds64.frame32(s), layer)
    bad = ripple_bounds64.slab32(records, [0], *bounds64.frame32(s), layer, mistake)
    assert float(good[0]) < z[0] < float(good[1])
    assert (good[0], good[1]) != (bad[0], bad[1]), mistake
    if mistake == "no_mag":
        # over these maps the smaller pad still covers the roundings.  Where the missing term matters: a level sea at 0 -- no other
        # magnitude -- under one raised cell: mag and the pad are 0, zhi is etamax itself, and the height at that cell's centre IS etamax
        assert bad[4] < good[4]
        level = np.zeros_like(maps)
        level[1, ..., 2] = 1.0
        none = bounds64.fold_maps(level)[None]
        s0 = _set(A=0.0, steep=0.0, plane_w=0.0)
        bump = ripple64.Layer(64, 1.0)
        bump.move(*ORIGIN)
        eta = np.zeros((64, 64), F)
        eta[9, 7] = 1.0
        bump.set_window(eta, np.zeros((64, 64), F))
        rec = ripple_bounds64.fold(bump.state())
        top = _heights(level, [0], [SCALE], s0, bump, np.array([[ORIGIN[0] + 7.5, ORIGIN[1] + 9.5]]), iterations=0)[0]
        g = ripple_bounds64.slab32(none, [0], *bounds64.frame32(s0), rec)
        b = ripple_bounds64.slab32(none, [0], *bounds64.frame32(s0), rec, mistake)
        assert top == 1.0 and float(g[0]) < 0 < top < float(g[1]) and b[4] == 0
        assert not top < float(b[1]), (top, b[1])
    else:
        assert z[0] > float(bad[1]), (mistake, z[0], bad[1])
