"""Ripple walls' arithmetic (datum_amd/csrc/ocean_ripple_wall.h), the very functions the kernels of ocean_ripple_wall.hip call, walked on
the CPU (tests/cpu/ripple_wall_emul.cpp) against ripple_wall64's numpy float32 restatement, bit for bit:

  * the raster: rotated boxes and ellipses, shapes partly outside the window, shapes across the torus seam, negative origins, cell
    centres exactly on a shape's edge with exactly representable numbers (so that <= is tested), overlapping shapes, 256 records;
  * the walled sub-steps in both modes on tests/test_ripple_emul.py's cases -- R = 64 and 128, origins (0, 0) and (37, -21), 1, 3 and
    16 sub-steps, the sponge on and off, random state and src -- with a wall list added.

The restatement's worst distance from its own float64 form over the sub-step cases, in units of eps max|eta|, is the bar the device is held
to: K_RIP_WALL (ripple_wall64.py, one per mode) is 3 x that measured value, and test_k_rip_wall checks that it still is.
"""

import ctypes
import os

import numpy as np
import pytest

import ripple64
import ripple_deep64 as rd
import ripple_wall64 as rw
from test_ripple_emul import CASES, EPS, F, ROOT, _bits, _p

DT = 0.1
S = 0.5
C, SN = 0.8, 0.6                       # an exactly representable rotation would need 0.8f, 0.6f: they are what they round to, on both sides


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ripple_wall_emul_raster.argtypes = [P, I, P, I, I, I, Fl]
    lib.ripple_wall_emul_substep.argtypes = [P, P, P, P, I, I, I, I, Fl, Fl, P, I]
    lib.ripple_wall_emul_deep_substep.argtypes = [P, P, P, P, I, I, I, I, Fl, Fl, P, P, I]
    lib.ripple_deep_emul_weights.argtypes = [P]
    lib.ripple_deep_emul_weights.restype = ctypes.c_double
    return lib


@pytest.fixture(scope="module")
def table(emul):
    G = np.zeros((rd.Q, rd.Q), F)
    emul.ripple_deep_emul_weights(_p(G))
    return G


def _emul_raster(emul, wl, R, ox, oy, s=S):
    wl = np.ascontiguousarray(wl, rw.WALL)
    plane = np.full((R, R), 7, np.uint8)
    emul.ripple_wall_emul_raster(_p(wl), len(wl), _p(plane), R, ox, oy, s)
    return plane


def harbour(R, ox, oy, s=S):
    """a list for a window at (ox, oy): a rotated box and a rotated ellipse inside, a box across the window's lower-left corner (partly
    outside), an ellipse over the torus seam (memory column and row 0), two overlapping boxes, a one-cell line"""
    x = lambda i: (ox + i + 0.5) * s
    y = lambda j: (oy + j + 0.5) * s
    sx, sy = (-ox) & (R - 1), (-oy) & (R - 1)          # window coordinates of memory column / row 0
    return rw.walls(
        rw.box(x(R // 3), y(R // 4), 4.3 * s, 1.2 * s, C, SN),
        rw.ellipse(x(2 * R // 3), y(R // 2), 5.1 * s, 2.4 * s, SN, -C),
        rw.box(x(0), y(0), 3.0 * s, 2.0 * s),
        rw.ellipse(x(sx), y(sy), 3.7 * s, 3.2 * s),
        rw.box(x(R // 2), y(3 * R // 4), 3.0 * s, 1.0 * s),
        rw.box(x(R // 2 + 2), y(3 * R // 4 + 1), 1.0 * s, 3.0 * s),
        rw.box(x(R - 4), y(R // 2), 0.25 * s, 6.25 * s),
    )


RASTER = [(R, o) for R in (64, 128) for o in ((0, 0), (37, -21), (-64, -64), (-1000003, 77))]


@pytest.mark.parametrize("R,origin", RASTER)
def test_raster_bits(emul, R, origin):
    wl = harbour(R, *origin)
    got = _emul_raster(emul, wl, R, *origin)
    want = rw.raster(wl, R, *origin, S)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert 0 < want.sum() < R * R // 4 and set(np.unique(got)) == {0, 1}
    # every record marks something, and the plane differs from the one with the sine negated
    for k in range(len(wl)):
        assert rw.raster(wl[k:k + 1], R, *origin, S).sum() > 0, k
    assert not np.array_equal(want, rw.raster(wl, R, *origin, S, mistake="sine"))
    # the plane is a function of the world cell: the same list at another origin agrees wherever the windows overlap
    o2 = (origin[0] + 5, origin[1] - 9)
    a = np.roll(want, (-(origin[1] & (R - 1)), -(origin[0] & (R - 1))), (0, 1))
    b = np.roll(_emul_raster(emul, wl, R, *o2), (-(o2[1] & (R - 1)), -(o2[0] & (R - 1))), (0, 1))
    assert np.array_equal(a[:R - 9, 5:], b[9:, :R - 5])


def test_edges_are_inside(emul):
    """s = 0.5, centres at multiples of 0.25: a box and a circle whose edges pass exactly through cell centres, all numbers exact"""
    R, o = 64, (-32, -32)
    cases = [
        (rw.box(0.25, 0.25, 1.0, 0.5), lambda I, J: (abs(I) <= 2) & (abs(J) <= 1)),                     # centres (I + .5) / 2: |I / 2| <= 1
        (rw.box(0.25, 0.25, 1.0, 0.5, 0.0, 1.0), lambda I, J: (abs(J) <= 2) & (abs(I) <= 1)),           # a quarter turn
        (rw.ellipse(0.25, 0.25, 2.5, 2.5), lambda I, J: I * I + J * J <= 25),                           # (3, 4), (5, 0) lie on it
        (rw.ellipse(0.25, 0.25, 1.0, 0.5, 2.0, 0.0), lambda I, J: (4 * I * I + 16 * J * J) <= 4),      # a non-unit axis scales the shape: u = 2 dx
    ]
    m = np.arange(R)
    I, J = np.meshgrid(o[0] + ((m - o[0]) & (R - 1)), o[1] + ((m - o[1]) & (R - 1)))
    for wl, rule in cases:
        got = _emul_raster(emul, wl, R, *o)
        assert np.array_equal(got, rw.raster(wl, R, *o, S))
        assert np.array_equal(got != 0, rule(I, J)), wl
    on = _emul_raster(emul, cases[2][0], R, *o)
    assert on[4, 3] == 1 and on[0, 5] == 1 and on[-4 & 63, -3 & 63] == 1 and on[4, 4] == 0         # memory cell [J mod R][I mod R]


def test_many_records_and_none(emul):
    R, o = 128, (37, -21)
    rng = np.random.default_rng(3)
    wl = np.zeros(rw.MAX_WALLS, rw.WALL)
    ang = rng.uniform(0, 2 * np.pi, len(wl))
    wl["center"] = (np.array(o) + rng.uniform(-8, R + 8, (len(wl), 2))) * S
    wl["axis"] = np.stack([np.cos(ang), np.sin(ang)], 1)
    wl["half"] = rng.uniform(0.2, 2.5, (len(wl), 2))
    wl["kind"] = rng.integers(0, 2, len(wl))
    got = _emul_raster(emul, wl, R, *o)
    assert np.array_equal(got, rw.raster(wl, R, *o, S)) and got.sum() > 256
    assert not _emul_raster(emul, wl[:0], R, *o).any()
    # fp32 against float64: a disagreement needs a centre within rounding of an edge; random shapes have none
    assert np.array_equal(got, rw.raster(wl, R, *o, S, np.float64))


# -- the walled sub-steps


def _random_layer(table, R, origin, B, dtype, seed, mode):
    rng = np.random.default_rng(seed)
    lay = rw.Layer(R, S, dtype, B=B, mode=mode, G=table)
    lay.move(*origin)
    lay.set_window(rng.normal(size=(R, R)).astype(F), rng.normal(size=(R, R)).astype(F), rng.integers(-2 ** 21, 2 ** 21, (R, R)))
    lay.set_walls(harbour(R, *origin))
    return lay


def _emul_step(emul, lay, dt, substeps):
    state = np.ascontiguousarray(lay.state(), F)
    src = lay.src.copy()
    wall = np.ascontiguousarray(lay.wall)
    G = np.ascontiguousarray(lay.G, F)
    if lay.mode == rw.WAVE:
        h, c2s2, f = ripple64.params(lay.c, lay.s, lay.gamma, lay.B, lay.sponge_gamma, dt, substeps)
    else:
        h, gs, f = rd.params(lay.g, lay.s, lay.gamma, lay.B, lay.sponge_gamma, dt, substeps)
    for i in range(substeps):
        out = np.empty_like(state)
        if lay.mode == rw.WAVE:
            emul.ripple_wall_emul_substep(_p(state), _p(out), _p(src), _p(wall), lay.R, lay.ox, lay.oy, lay.B, float(h), float(c2s2), _p(f), int(i == 0))
        else:
            emul.ripple_wall_emul_deep_substep(_p(state), _p(out), _p(src), _p(wall), lay.R, lay.ox, lay.oy, lay.B, float(h), float(gs), _p(f), _p(G), int(i == 0))
        state = out
        src[:] = 0
    return state


@pytest.fixture(scope="module")
def cases(emul, table):
    """every case once per mode: (the header's walk, the restatement, the restatement's distance from float64 in eps max|eta|)"""
    out = {}
    for mode in (rw.WAVE, rw.DEEP):
        for R, origin, substeps, B in CASES:
            lay = _random_layer(table, R, origin, B, F, R + substeps, mode)
            l64 = _random_layer(table, R, origin, B, np.float64, R + substeps, mode)
            assert np.array_equal(lay.wall, l64.wall)
            got = _emul_step(emul, lay, DT * substeps, substeps)
            lay.step(DT * substeps, substeps)
            l64.step(DT * substeps, substeps)
            out[mode, R, origin, substeps, B] = got, lay, np.abs(lay.eta.astype(np.float64) - l64.eta).max() / (EPS * np.abs(l64.eta).max())
    return out


@pytest.mark.parametrize("mode", [rw.WAVE, rw.DEEP])
@pytest.mark.parametrize("R,origin,substeps,B", CASES)
def test_substep_bits(cases, mode, R, origin, substeps, B):
    got, lay, _ = cases[mode, R, origin, substeps, B]
    want = lay.state()
    assert np.abs(want).max() > 1 and np.isfinite(want).all() and np.all(lay.src == 0)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:4]
    # a wall cell holds (+0, +0): the bits, not only the value
    assert not _bits(got)[lay.wall != 0].any() and np.abs(got[lay.wall == 0]).min() > 0


def test_k_rip_wall(cases):
    """K_RIP_WALL is 3 x the restatement's worst distance from float64 over the cases above, per mode (measured here, not on the GPU), and
    DESIGN.md states that measurement"""
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    for mode, name in ((rw.WAVE, "WAVE"), (rw.DEEP, "DEEP")):
        dist = {case: v[2] for case, v in cases.items() if case[0] == mode}
        worst = max(dist.values())
        K = rw.K_RIP_WALL[mode]
        print(f"walled {name} restatement vs float64: worst {worst:.2f} eps max|eta| at {max(dist, key=dist.get)[1:]}; K_RIP_WALL = {K}")
        assert 3 * worst <= K <= 3.3 * worst
        assert f"{name} worst {worst:.2f} eps" in design and f"`K_RIP_WALL[{name}]` = {K}" in design
