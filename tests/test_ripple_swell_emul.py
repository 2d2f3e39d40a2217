"""Ripple swell's arithmetic (datum_amd/csrc/ocean_ripple_swell.h), the very functions the kernels of ocean_ripple_swell.hip call, walked on
the CPU (tests/cpu/ripple_swell_emul.cpp) against ripple_swell64's numpy float32 restatement, bit for bit:

  * the forcing plane from a plane of heights: R = 64 and 128; two origins at which the window wraps the torus inside a tile; walls that
    touch the window's edge, a box across the torus seam, an ellipse, a one-cell pillar with four neighbours' worth of faces; an island
    and a beach with walls on top; the bed on and off; nothing solid;
  * the two sub-steps over those scenes, 1, 3 and 16 of them, with and without a first sub-step's deposits.

The restatement's worst distance from its own float64 form over the sub-step cases, in units of eps max|eta|, is the bar the device is held
to: K_RIP_SWELL (ripple_swell64.py) is 3 x that measured value, and test_k_rip_swell checks that it still is.
"""

import ctypes
import os

import numpy as np
import pytest

import ripple64
import ripple_bed64 as rb
import ripple_swell64 as rs
import ripple_wall64 as rw
from test_ripple_bed_emul import piers, shore
from test_ripple_emul import EPS, F, ROOT, _bits, _p

DT = 0.1
S = 0.5
ORIGINS = ((37, -21), (-70, 9))         # memory column 0 is window column 27 or 6: the window wraps inside the first tile
CASES = [(R, o, n, bed, src) for R in (64, 128) for o in ORIGINS for n in (1, 3, 16) for bed in (False, True) for src in (True, False)]


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ripple_swell_emul_force.argtypes = [P, P, P, P, I, I, I]
    lib.ripple_swell_emul_centre.argtypes = [I, Fl]
    lib.ripple_swell_emul_centre.restype = Fl
    lib.ripple_swell_emul_substep.argtypes = [P, P, P, P, P, I, I, I, I, Fl, Fl, P, I]
    lib.ripple_swell_emul_bed_substep.argtypes = [P, P, P, P, P, P, I, I, I, I, Fl, Fl, P, P, I]
    return lib


def harbour(R, ox, oy, s=S):
    """the walls of the issue's list: two that touch the window's edge (one runs along it, one ends on it), a box across the torus seam,
    an ellipse, a one-cell pillar"""
    x = lambda i: (ox + i + 0.5) * s
    y = lambda j: (oy + j + 0.5) * s
    sx, sy = (-ox) & (R - 1), (-oy) & (R - 1)
    return rw.walls(rw.box(x(R // 2), y(0), 9.0 * s, 1.2 * s), rw.box(x(R - 2), y(R // 2), 3.2 * s, 0.7 * s),
                    rw.box(x(sx), y(sy), 3.2 * s, 2.2 * s), rw.ellipse(x(R // 4), y(3 * R // 4), 5.3 * s, 2.6 * s, 0.8, 0.6),
                    rw.box(x(3 * R // 4), y(R // 4), 0.3 * s, 0.3 * s))


def heights(R, ox, oy, seed, s=S):
    """a plane of heights above the cells' centres in memory order: two swells and noise, fp32"""
    rng = np.random.default_rng(seed)
    x, y = rs.centres(R, ox, oy, s)
    X, Y = x.astype(np.float64)[None, :], y.astype(np.float64)[:, None]
    return (0.8 * np.sin(0.31 * X + 0.17 * Y + 1.0) + 0.3 * np.cos(0.9 * Y - 0.4 * X) + 0.05 * rng.normal(size=(R, R))).astype(F)


def scene(R, origin, bed, dtype=F, B=8, seed=3, src=True, walls=True):
    rng = np.random.default_rng(seed)
    lay = rs.Layer(R, S, dtype, B=B)
    lay.move(*origin)
    lay.set_window(rng.normal(size=(R, R)).astype(F), rng.normal(size=(R, R)).astype(F), rng.integers(-2 ** 21, 2 ** 21, (R, R)) if src else np.zeros((R, R), np.int64))
    if walls:
        lay.set_walls(rw.walls(harbour(R, *origin), piers(R, *origin)) if bed else harbour(R, *origin))
    if bed:
        lay.set_bed(*shore(R, *origin, surf=True))
    lay.set_swell(True)
    return lay


def _emul_force(emul, H, wall, d, R, ox, oy):
    out = np.full((R, R), 7, F)
    emul.ripple_swell_emul_force(_p(np.ascontiguousarray(H, F)), _p(np.ascontiguousarray(wall)) if wall is not None else None,
                                 _p(np.ascontiguousarray(d, F)) if d is not None else None, _p(out), R, ox, oy)
    return out


@pytest.mark.parametrize("bed", [False, True])
@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("R", [64, 128])
def test_force_bits(emul, R, origin, bed):
    lay = scene(R, origin, bed)
    H = heights(R, *origin, seed=R)
    got = _emul_force(emul, H, lay.wall, lay.d, R, *origin)
    lay.refresh(H)
    assert np.array_equal(_bits(got), _bits(lay.F)), np.argwhere(_bits(got) != _bits(lay.F))[:4]
    sol = lay.solid()
    # +0, the bits, on every solid cell and on every cell none of whose neighbours count; something on the others
    nb = sum(n.astype(int) for n in rw._neighbours(sol))
    assert not _bits(got)[sol].any() and not _bits(got)[~sol & (nb == 0)].any()
    wx, wy = ripple64.window_coords(R, *origin)
    interior = (wx[None, :] > 0) & (wx[None, :] < R - 1) & (wy[:, None] > 0) & (wy[:, None] < R - 1)
    boundary = ~sol & (nb > 0) & interior
    assert boundary.sum() > 60 and (got[boundary] != 0).mean() > 0.95
    # the scene has what it claims: solid cells in window row 0 and in window column R - 1 (the edge), in memory row 0 and column 0
    # both (the seam), and a pillar: a solid cell whose four neighbours are wet and each have exactly its face
    win = lay.window(sol)
    assert win[0].sum() >= 18 and win[:, R - 1].sum() >= 1 and sol[0, 0] and sol[0, R - 1] and sol[R - 1, 0]
    pj, pi = R // 4, 3 * R // 4
    if not bed:
        assert win[pj, pi] and not (win[pj, pi - 1] or win[pj, pi + 1] or win[pj - 1, pi] or win[pj + 1, pi])
        Hw, Fw = lay.window(H), lay.window(got)
        assert Fw[pj, pi - 1] == Hw[pj, pi - 1] - Hw[pj, pi] and Fw[pj + 1, pi] == Hw[pj + 1, pi] - Hw[pj, pi]
    else:
        assert (lay.d[lay.wall != 0] == 0).all() and (sol & (lay.wall == 0)).sum() > R        # land besides the walls
    # the centre the kernel hands to the query is the restatement's
    x, y = rs.centres(R, *origin, S)
    m = np.arange(R)
    I = origin[0] + ((m - origin[0]) & (R - 1))
    assert all(_bits(F(emul.ripple_swell_emul_centre(int(i), S))) == _bits(v) for i, v in zip(I[::7], x[::7]))


def test_nothing_solid_and_no_alias(emul):
    """no walls and no bed: F is +0 everywhere.  A wall on the window's last column is the torus neighbour of the first column's cells in
    memory, but lies outside the window for them: they do not count it"""
    R, origin = 64, (37, -21)
    H = heights(R, *origin, seed=1)
    got = _emul_force(emul, H, None, None, R, *origin)
    assert not _bits(got).any()
    lay = scene(R, origin, False, walls=False)
    x = lambda i: (origin[0] + i + 0.5) * S
    y = lambda j: (origin[1] + j + 0.5) * S
    lay.set_walls(rw.box(x(R - 1), y(R // 2), 0.3 * S, 40 * S))
    assert lay.window(lay.wall)[:, R - 1].all() and lay.wall.sum() == R
    got = _emul_force(emul, H, lay.wall, None, R, *origin)
    lay.refresh(H)
    assert np.array_equal(_bits(got), _bits(lay.F))
    Fw = lay.window(got)
    assert not Fw[:, 0].any() and (Fw[:, R - 2] != 0).all() and not Fw[:, 1:R - 2].any()


def _emul_step(emul, lay, dt, substeps):
    state = np.ascontiguousarray(lay.state(), F)
    src = lay.src.copy()
    Fp = np.ascontiguousarray(lay.F, F)
    if lay.bed is not None:
        d, q = np.ascontiguousarray(lay.d, F), np.ascontiguousarray(lay.q)
        h, gs2, f, fsurf = rb.params(lay.g, lay.s, lay.gamma, lay.B, lay.sponge_gamma, lay.bed["surf_gamma"], dt, substeps)
    else:
        wall = np.ascontiguousarray(lay.wall)
        h, c2s2, f = ripple64.params(lay.c, lay.s, lay.gamma, lay.B, lay.sponge_gamma, dt, substeps)
    for i in range(substeps):
        out = np.empty_like(state)
        if lay.bed is not None:
            emul.ripple_swell_emul_bed_substep(_p(state), _p(out), _p(src), _p(d), _p(q), _p(Fp), lay.R, lay.ox, lay.oy, lay.B, float(h), float(gs2), _p(f), _p(fsurf), int(i == 0))
        else:
            emul.ripple_swell_emul_substep(_p(state), _p(out), _p(src), _p(wall), _p(Fp), lay.R, lay.ox, lay.oy, lay.B, float(h), float(c2s2), _p(f), int(i == 0))
        state = out
        src[:] = 0
    return state


@pytest.fixture(scope="module")
def cases(emul):
    """every case once: (the header's walk, the restatement, the restatement's distance from float64 in eps max|eta|)"""
    out = {}
    for R, origin, substeps, bed, src in CASES:
        lay = scene(R, origin, bed, F, seed=R + substeps, src=src)
        l64 = scene(R, origin, bed, np.float64, seed=R + substeps, src=src)
        H = heights(R, *origin, seed=substeps)
        lay.refresh(H)
        l64.F, l64.current = lay.F.astype(np.float64), True                    # a common fp32 plane
        got = _emul_step(emul, lay, DT * substeps, substeps)
        lay.step(DT * substeps, substeps)
        l64.step(DT * substeps, substeps)
        out[R, origin, substeps, bed, src] = got, lay, np.abs(lay.eta.astype(np.float64) - l64.eta).max() / (EPS * np.abs(l64.eta).max())
    return out


@pytest.mark.parametrize("R,origin,substeps,bed,src", CASES)
def test_substep_bits(cases, R, origin, substeps, bed, src):
    got, lay, _ = cases[R, origin, substeps, bed, src]
    want = lay.state()
    assert np.abs(want).max() > 1 and np.isfinite(want).all() and np.all(lay.src == 0)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:4]
    # a solid cell holds (+0, +0): the bits, not only the value
    assert not _bits(got)[lay.solid()].any()
    # the swell is in the step: the parent's step from the same state differs on the boundary cells
    assert (lay.F != 0).sum() > 60


def test_swell_off_or_stale_is_the_parent(emul):
    """with the mark clear the layer steps as ripple_bed64's and ripple_wall64's do, bit for bit"""
    for bed in (False, True):
        lay, par = scene(64, ORIGINS[0], bed), scene(64, ORIGINS[0], bed)
        lay.refresh(heights(64, *ORIGINS[0], seed=9))
        lay.move(ORIGINS[0][0] + 3, ORIGINS[0][1] - 2)
        par.move(ORIGINS[0][0] + 3, ORIGINS[0][1] - 2)
        par.set_swell(False)
        assert not lay.current
        lay.step(0.3, 3)
        rb.Layer.step(par, 0.3, 3)
        assert np.array_equal(_bits(lay.state()), _bits(par.state()))


def test_k_rip_swell(cases):
    """K_RIP_SWELL is 3 x the restatement's worst distance from float64 over the cases above (measured here, not on the GPU), and
    DESIGN.md states that measurement"""
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    dist = {case: v[2] for case, v in cases.items()}
    worst = max(dist.values())
    print(f"swell restatement vs float64: worst {worst:.2f} eps max|eta| at {max(dist, key=dist.get)}; K_RIP_SWELL = {rs.K_RIP_SWELL}")
    assert 3 * worst <= rs.K_RIP_SWELL <= 3.3 * worst
    assert f"worst {worst:.2f} eps" in design and f"`K_RIP_SWELL` = {rs.K_RIP_SWELL}" in design
