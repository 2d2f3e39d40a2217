"""The ripple bed's arithmetic (datum_amd/csrc/ocean_ripple_bed.h), the very functions the kernels of ocean_ripple_bed.hip call, walked on
the CPU (tests/cpu/ripple_bed_emul.cpp) against ripple_bed64's numpy float32 restatement, bit for bit:

  * the raster: maps smaller than the window, a map edge exactly on a cell centre, negative origins, a beach across the torus seam, the
    dry_depth and max_depth clamps, every surf level, walls on;
  * the sub-step on tests/test_ripple_emul.py's cases -- R = 64 and 128, origins (0, 0) and (37, -21), 1, 3 and 16 sub-steps, the
    sponge on and off, random state and src -- over a bed with a beach, an island, a surf zone and walls.

The restatement's worst distance from its own float64 form over the sub-step cases, in units of eps max|eta|, is the bar the device is held
to: K_RIP_BED (ripple_bed64.py) is 3 x that measured value, and test_k_rip_bed checks that it still is.
"""

import ctypes
import os

import numpy as np
import pytest

import ripple_bed64 as rb
import ripple_wall64 as rw
from test_ripple_emul import CASES, EPS, F, ROOT, _bits, _p

DT = 0.1
S = 0.5
TEXEL = 0.75                           # no multiple of the cell side: the patch's weights vary from cell to cell


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ripple_bed_emul_raster.argtypes = [P, P, P, P, P, I, I, I, Fl]
    lib.ripple_bed_emul_substep.argtypes = [P, P, P, P, P, I, I, I, I, Fl, Fl, P, P, I]
    return lib


def _emul_raster(emul, b, depths, wall, R, ox, oy, s=S):
    rec = np.array([b], rb.BED)
    depths = np.ascontiguousarray(depths, F)
    d, q = np.full((R, R), 7, F), np.full((R, R), 77, np.uint8)
    emul.ripple_bed_emul_raster(_p(rec), _p(depths), _p(np.ascontiguousarray(wall)) if wall is not None else None, _p(d), _p(q), R, ox, oy, s)
    return d, q


def seam(R, ox, oy):
    """the window cell the shoreline of `shore` passes through: the one memory cell (0, 0) holds, where it lies well on the map"""
    sx, sy = (-ox) & (R - 1), (-oy) & (R - 1)
    return (sx if 8 <= sx < R - 8 else R // 4), (sy if 8 <= sy < R - 8 else R // 4)


def shore(R, ox, oy, s=S, surf=True, seed=5):
    """a bed for a window at (ox, oy): a map SMALLER than the window (a margin of six cells reads `outside`) that falls from max_depth
    to land along a diagonal through the window cell that memory cell (0, 0) holds -- the shoreline crosses the torus seam -- where that
    cell lies on the map, else through (R/4, R/4); an island in the water beside it; small random relief.  (record, depths)"""
    rng = np.random.default_rng(seed)
    x0, y0 = (ox + 6) * s, (oy + 6.5) * s                      # the map's texel (0, 0): a cell edge in x, a cell centre in y
    W = H = int((R - 12) * s / TEXEL)
    X, Y = x0 + TEXEL * np.arange(W)[None, :], y0 + TEXEL * np.arange(H)[:, None]
    px, py = seam(R, ox, oy)
    depth = 0.06 * ((X - (ox + px + 0.5) * s) + 0.5 * (Y - (oy + py + 0.5) * s))
    cx, cy = (ox + px + 12.5) * s, (oy + py + 6.5) * s
    depth -= 2.0 * np.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / (2 * 1.5 ** 2))
    depth += 0.02 * rng.normal(size=(H, W))
    b = rb.bed(W, H, (x0, y0), TEXEL, outside=0.9, max_depth=1.2, dry_depth=0.02, surf_depth=0.6 if surf else 0.0, surf_gamma=3.0 if surf else 0.0)
    return b, depth.astype(F)


def piers(R, ox, oy, s=S):
    """walls over the bed: a rotated box in deep water, a box across the shoreline, an ellipse over the torus seam"""
    x = lambda i: (ox + i + 0.5) * s
    y = lambda j: (oy + j + 0.5) * s
    sx, sy = (-ox) & (R - 1), (-oy) & (R - 1)
    return rw.walls(rw.box(x(3 * R // 4), y(3 * R // 4), 4.3 * s, 1.2 * s, 0.8, 0.6), rw.box(x(R // 4), y(R // 3), 6.0 * s, 0.7 * s), rw.ellipse(x(sx), y(sy), 2.7 * s, 2.2 * s))


RASTER = [(R, o) for R in (64, 128) for o in ((0, 0), (37, -21), (-64, -64), (-1000003, 77))]


@pytest.mark.parametrize("walls", [False, True])
@pytest.mark.parametrize("R,origin", RASTER)
def test_raster_bits(emul, R, origin, walls):
    b, depths = shore(R, *origin)
    wall = rw.raster(piers(R, *origin), R, *origin, S) if walls else None
    d, q = _emul_raster(emul, b, depths, wall, R, *origin)
    wd, wq = rb.raster(depths, b, wall, R, *origin, S)
    assert np.array_equal(_bits(d), _bits(wd)), np.argwhere(_bits(d) != _bits(wd))[:4]
    assert np.array_equal(q, wq), np.argwhere(q != wq)[:4]
    # the scene has what it claims: land, a beach, clamped deep water, the margin that reads `outside`, most surf levels
    solid = d == 0
    assert R * R // 50 < solid.sum() < 3 * R * R // 4 and not _bits(d)[solid].any()
    assert d[~solid].min() >= b["dry_depth"] and d.max() == b["max_depth"] and (d == b["outside"]).sum() >= 12 * R
    assert set(np.unique(q)) >= set(range(15)) and q.max() <= rb.SURF_LEVELS and not q[solid].any()
    if walls:
        assert solid[wall != 0].all() and (wall != 0).sum() > 20
    # where memory cell (0, 0) lies on the map the shoreline crosses memory column 0 and memory row 0 (the torus seam): land and water
    # on the map's part of both
    if seam(R, *origin) == ((-origin[0]) & (R - 1), (-origin[1]) & (R - 1)):
        onmap = (d != b["outside"]) | solid
        for line, on in ((solid[:, 0], onmap[:, 0]), (solid[0, :], onmap[0, :])):
            assert 4 < line[on].sum() < on.sum() - 4
    # an island: a solid cell whose row has water on both sides of it on the map (at a million cells out fp32 centres are too coarse to say)
    isl = np.roll(solid, (-(origin[1] & (R - 1)), -(origin[0] & (R - 1))), (0, 1))[seam(R, *origin)[1] + 6]
    if abs(origin[0]) < 1000:
        assert isl[seam(R, *origin)[0] + 12] and not isl[seam(R, *origin)[0] + 5] and not isl[seam(R, *origin)[0] + 19]
    # the planes are a function of the world cell: the same bed at another origin agrees wherever the windows overlap
    o2 = (origin[0] + 5, origin[1] - 9)
    wall2 = rw.raster(piers(R, *origin), R, *o2, S) if walls else None
    d2, q2 = _emul_raster(emul, b, depths, wall2, R, *o2)
    unroll = lambda a, o: np.roll(a, (-(o[1] & (R - 1)), -(o[0] & (R - 1))), (0, 1))
    assert np.array_equal(unroll(d, origin)[:R - 9, 5:], unroll(d2, o2)[9:, :R - 5]) and np.array_equal(unroll(q, origin)[:R - 9, 5:], unroll(q2, o2)[9:, :R - 5])


def test_map_edge_on_a_cell_centre(emul):
    """s = 0.5, texel = 0.5, texel (0, 0) on the centre of cell (-3, -2): u and v are whole numbers, every value exact.  The map covers
    the cells -3 .. 1 by -2 .. 1, its last column and row exactly on cell centres (u == width - 1 is ON the map: the clamped lower index,
    weight 1); one cell further reads `outside`"""
    R, o = 64, (-32, -32)
    W, H = 5, 4
    depths = (1.0 + np.arange(W)[None, :] + 10.0 * np.arange(H)[:, None]).astype(F)
    b = rb.bed(W, H, (-1.25, -0.75), 0.5, outside=77.0, max_depth=100.0, dry_depth=0.5)
    d, q = _emul_raster(emul, b, depths, None, R, *o)
    wd, wq = rb.raster(depths, b, None, R, *o, S)
    assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(q, wq) and not q.any()
    at = lambda I, J: float(d[J & (R - 1), I & (R - 1)])
    for j in range(H):
        for i in range(W):
            assert at(-3 + i, -2 + j) == depths[j, i], (i, j)
    assert at(-4, 0) == 77.0 and at(2, 0) == 77.0 and at(0, -3) == 77.0 and at(0, 2) == 77.0 and (d == 77.0).sum() == R * R - W * H
    # half a cell off: the patch between texels, and the last half cell is off the map
    b2 = rb.bed(W, H, (-1.0, -0.75), 0.5, outside=77.0, max_depth=100.0, dry_depth=0.5)
    d2, _ = _emul_raster(emul, b2, depths, None, R, *o)
    assert np.array_equal(_bits(d2), _bits(rb.raster(depths, b2, None, R, *o, S)[0]))
    assert d2[-2 & 63, -2 & 63] == 1.5 and d2[-2 & 63, -3 & 63] == 77.0 and d2[-2 & 63, 1] == 4.5 and d2[-2 & 63, 2] == 77.0


def test_clamps_and_every_surf_level(emul):
    """a map aligned with the cells (exact values): negative depths and depths below dry_depth are solid +0, depths above max_depth are
    max_depth, -0 stays +0; with surf_depth = 1 a depth of 1 - (k + 1/2) / 16 has level k, a depth below 2^-25 level 16"""
    R, o = 64, (-32, -32)
    levels = [1.0 - (k + 0.5) / 16 for k in range(16)] + [1e-9]
    row = np.array([-3.0, -0.0, 0.0, 0.009, 0.01, 0.5, 7.0, 8.0, 9.0, 1e30, 1.0, 0.99999994] + levels, F)
    depths = np.stack([row, row])
    b = rb.bed(len(row), 2, (-1.25 - 4.0, 0.25), 0.5, outside=-5.0, max_depth=8.0, dry_depth=0.01, surf_depth=0.0)
    d, q = _emul_raster(emul, b, depths, None, R, *o)
    wd, wq = rb.raster(depths, b, None, R, *o, S)
    assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(q, wq) and not q.any()
    got = d[0, (np.arange(len(row)) - 11) & 63]
    assert np.array_equal(_bits(got[:10]), _bits(np.array([0, 0, 0, 0, 0.01, 0.5, 7, 8, 8, 8], F)))
    assert (d != 0).sum() == 2 * (len(row) - 5)                  # `outside` is negative: everything off the map is land
    b = rb.bed(len(row), 2, (-1.25 - 4.0, 0.25), 0.5, outside=-5.0, max_depth=8.0, dry_depth=1e-12, surf_depth=1.0, surf_gamma=1.0)
    d, q = _emul_raster(emul, b, depths, None, R, *o)
    wd, wq = rb.raster(depths, b, None, R, *o, S)
    assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(q, wq)
    got = q[0, (np.arange(len(row)) - 11) & 63]
    assert list(got[12:]) == list(range(17)) and list(got[:12]) == [0, 0, 0, 15, 15, 8, 0, 0, 0, 0, 0, 0]


# -- the sub-step over a bed


def _random_layer(R, origin, B, dtype, seed):
    rng = np.random.default_rng(seed)
    lay = rb.Layer(R, S, dtype, B=B)
    lay.move(*origin)
    lay.set_window(rng.normal(size=(R, R)).astype(F), rng.normal(size=(R, R)).astype(F), rng.integers(-2 ** 21, 2 ** 21, (R, R)))
    lay.set_walls(piers(R, *origin))
    lay.set_bed(*shore(R, *origin, surf=B > 0))                # (the surf zone on with the sponge and off without it)
    return lay


def _emul_step(emul, lay, dt, substeps):
    state = np.ascontiguousarray(lay.state(), F)
    src = lay.src.copy()
    d, q = np.ascontiguousarray(lay.d, F), np.ascontiguousarray(lay.q)
    h, gs2, f, fsurf = rb.params(lay.g, lay.s, lay.gamma, lay.B, lay.sponge_gamma, lay.bed["surf_gamma"], dt, substeps)
    for i in range(substeps):
        out = np.empty_like(state)
        emul.ripple_bed_emul_substep(_p(state), _p(out), _p(src), _p(d), _p(q), lay.R, lay.ox, lay.oy, lay.B, float(h), float(gs2), _p(f), _p(fsurf), int(i == 0))
        state = out
        src[:] = 0
    return state


@pytest.fixture(scope="module")
def cases(emul):
    """every case once: (the header's walk, the restatement, the restatement's distance from float64 in eps max|eta|)"""
    out = {}
    for R, origin, substeps, B in CASES:
        lay = _random_layer(R, origin, B, F, R + substeps)
        l64 = _random_layer(R, origin, B, np.float64, R + substeps)
        assert np.array_equal(lay.d, l64.d) and np.array_equal(lay.q, l64.q) and rb.stable(lay.g, lay.bed["max_depth"], S, DT * substeps, substeps)
        got = _emul_step(emul, lay, DT * substeps, substeps)
        lay.step(DT * substeps, substeps)
        l64.step(DT * substeps, substeps)
        out[R, origin, substeps, B] = got, lay, np.abs(lay.eta.astype(np.float64) - l64.eta).max() / (EPS * np.abs(l64.eta).max())
    return out


@pytest.mark.parametrize("R,origin,substeps,B", CASES)
def test_substep_bits(cases, R, origin, substeps, B):
    got, lay, _ = cases[R, origin, substeps, B]
    want = lay.state()
    assert np.abs(want).max() > 1 and np.isfinite(want).all() and np.all(lay.src == 0)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:4]
    # a solid cell holds (+0, +0): the bits, not only the value
    assert not _bits(got)[lay.d == 0].any() and np.abs(got[lay.d != 0]).min() > 0
    assert (lay.q > 0).any() == (B > 0)


def test_k_rip_bed(cases):
    """K_RIP_BED is 3 x the restatement's worst distance from float64 over the cases above (measured here, not on the GPU), and DESIGN.md
    states that measurement"""
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    dist = {case: v[2] for case, v in cases.items()}
    worst = max(dist.values())
    print(f"bed restatement vs float64: worst {worst:.2f} eps max|eta| at {max(dist, key=dist.get)}; K_RIP_BED = {rb.K_RIP_BED}")
    assert 3 * worst <= rb.K_RIP_BED <= 3.3 * worst
    assert f"worst {worst:.2f} eps" in design and f"`K_RIP_BED` = {rb.K_RIP_BED}" in design
