"""CPU tests of the rippled reads' restatement (tests/rippled64.py): the closed forms over a flat FFT surface, a ray through a single raised
cell, the share of folded points on the lists the GPU test uses, and the planted mistakes, each of which moves a result by far more than
any bar of tests/test_gpu_rippled.py."""

import numpy as np
import pytest

import blend64
import gen64
import gen_cases
import ripple64
import rippled64
from test_blend64 import WS, _maps
from test_surface_abi import _set

F = np.float32
EPS = 2.0 ** -24


def _rough(R, cell, seed):
    lay = ripple64.Layer(R, cell)
    lay.move(37, -21)
    rng = np.random.RandomState(seed)
    lay.set_window(rng.uniform(-0.2, 0.2, (R, R)).astype(F), rng.uniform(-1, 1, (R, R)).astype(F))
    return lay


def _flat_maps(N):
    m = np.zeros((2, N, N, 4))
    m[1, ..., 2] = 1.0
    return m


def _inside_points(lay, n, seed):
    lo = np.array([lay.ox, lay.oy]) * float(lay.s)
    return (lo + np.random.RandomState(seed).uniform(0.1, 0.9, (n, 2)) * lay.R * float(lay.s)).astype(F)


def test_flat_surface_closed_forms():
    """over a flat FFT surface without swell the rippled normal is normalize(-1/2 dx, -1/2 dy, 1) and the height the bilinear patch"""
    lay = _rough(64, 0.5, 3)
    s = _set(A=0.0, steep=0.0, length=35.0, wavescale=WS[0], plane_w=0.25)
    q = _inside_points(lay, 400, 5)
    smp = lay.sample(q)
    got = rippled64.record64([_flat_maps(64)], None, "off", [1 / WS[0]], s, lay, q, 4)
    level = blend64.surface_blend64([_flat_maps(64)], None, "off", [1 / WS[0]], s, q, 4)[:, 2]
    assert np.abs(got[:, 4:7] - rippled64.flat_normal64(smp)).max() < 1e-14
    assert np.abs(got[:, 2] - (level + smp[:, 0])).max() < 1e-14 and np.abs(smp[:, 0]).max() > 0.05
    # the patch is bilinear between the four centres: at a centre it is the cell's height, between two the mean
    I, J = lay.ox + 7, lay.oy + 9
    c = np.array([[(I + 0.5) * 0.5, (J + 0.5) * 0.5], [(I + 1.0) * 0.5, (J + 0.5) * 0.5]], F)
    e = lay.window()[..., 0]
    h = lay.sample(c)[:, 0]
    assert h[0] == e[9, 7] and abs(h[1] - 0.5 * (float(e[9, 7]) + float(e[9, 8]))) < 4 * EPS
    # the bit-for-bit part: one fp32 addition
    rec = got.astype(F)
    assert np.array_equal(rippled64.record32(rec, smp)[:, 2], rec[:, 2] + smp[:, 0])


def test_ray_through_a_raised_cell():
    """a level sea at 0 and one cell raised by H: a vertical ray above the cell's centre hits at z = H, one two cells away at z = 0, and a
    horizontal ray at z = H / 2 enters the bump where the bilinear patch reaches H / 2: half a cell before the centre"""
    lay = ripple64.Layer(64, 1.0)
    b = rippled64.bump(lay, 3, -5, F(0.5))
    fn = rippled64.analytic32(lambda x, y: np.zeros_like(x), lay)
    rays = np.array([[b.x, b.y, 2.0, 0.0, 0.0, 0.0, -1.0, 4.0],
                     [b.x + 2.0, b.y, 2.0, 0.0, 0.0, 0.0, -1.0, 4.0],
                     [b.x - 3.0, b.y, 0.25, 0.0, 1.0, 0.0, 0.0, 3.0]], F)
    c = rippled64.cast32(fn, rays, 32, 20).records
    assert np.all(c[:, 3] == 1)
    assert abs(c[0, 0] - 1.5) < 1e-5 and abs(c[1, 0] - 2.0) < 1e-5
    assert abs(c[2, 0] - 2.5) < 1e-5 and abs(c[2, 6] - 0.25) < 1e-5
    # without the layer the horizontal ray at 0.25 m misses the level sea
    flat = ripple64.Layer(64, 1.0)
    assert rippled64.cast32(rippled64.analytic32(lambda x, y: np.zeros_like(x), flat), rays, 32, 20).records[2, 3] == 0


def _case():
    N = 64
    maps = [_maps(N, 0.02, 5 + k, WS[k]) for k in range(3)]
    scales = [1 / WS[k] for k in range(3)]
    s = _set(A=0.5, steep=0.3, length=35.0, wavescale=WS[0], plane_w=0.25)
    lay = _rough(64, 1.0, 11)
    return maps, scales, s, lay, _inside_points(lay, 600, 13)


def test_folded_share():
    """the lists of the float64 comparisons stay within 5 % of folded points (residual above 1e-3 m after 4 iterations)"""
    maps, scales, s, lay, q = _case()
    res = blend64.surface_blend64(maps, None, "off", scales, s, q, 4)[:, 3]
    assert (res > 1e-3).mean() <= 0.05


@pytest.mark.parametrize("mistake", ["at_b", "sign", "no_half", "rate"])
def test_planted_mistakes_fail_the_query(mistake):
    maps, scales, s, lay, q = _case()
    want = rippled64.record64(maps, None, "off", scales, s, lay, q, 4)
    got = rippled64.record64(maps, None, "off", scales, s, lay, q, 4, mistake=mistake)
    bar = (36.0 * (1 + np.abs(q).max() * 64 * max(scales)) + rippled64.K_RIPN) * EPS
    moved = np.abs(got - want)
    if mistake == "rate":
        assert moved[:, 2].max() > 0.1 and moved[:, 4:7].max() == 0
        smp = lay.sample(q)
        assert (rippled64.lift32(want[:, 2].astype(F), smp, mistake) != rippled64.lift32(want[:, 2].astype(F), smp)).mean() > 0.9
    else:
        assert moved[:, 4:7].max() > 20 * bar, (mistake, moved[:, 4:7].max(), bar)
    if mistake == "at_b":
        assert moved[:, 2].max() > 1e-3


def test_planted_mistake_fails_the_mesh(oracle):
    N = 64
    maps = [_maps(N, 0.3, 5 + k, WS[k]).astype(F) for k in range(2)]
    scales = [float(F(1) / F(WS[k])) for k in range(2)]
    s = gen_cases.oceanset(oracle, N, "example", wavescale=WS[0])
    ray = gen64.ray32(s, 33, 17)
    plain = blend64.staged_blend64(s, maps, scales, ray)
    lay = ripple64.Layer(128, 0.5)
    lay.center(float(plain.vertices[-1, 16, 0]), float(plain.vertices[-1, 16, 1]))
    rng = np.random.RandomState(4)
    lay.set_window(rng.uniform(-0.2, 0.2, (128, 128)).astype(F), np.zeros((128, 128), F))
    want = rippled64.mesh64(s, maps, scales, ray, lay)
    assert np.array_equal(want.vertices[..., [0, 1, 3, 4]], plain.vertices[..., [0, 1, 3, 4]])
    assert np.abs(want.vertices[..., 2] - plain.vertices[..., 2]).max() > 1e-3
    got = rippled64.mesh64(s, maps, scales, ray, lay, mistake="at_position")
    assert np.abs(got.vertices[..., 2] - want.vertices[..., 2]).max() > 1e-3
    v32 = plain.vertices.astype(F)
    a, b = rippled64.vertex32(v32, lay), rippled64.vertex32(v32, lay, "at_position", plain.position)
    assert (a[..., 2] != b[..., 2]).any()


def test_the_bar_of_the_normals():
    """K_RIPN, taken as K_LIT and K_RIP were: the fp32 restatement against the float64 form over slopes of the tests' range and the tests'
    layer samples, the reciprocal square root off by up to an ulp either way; three times the worst ratio is the constant"""
    lay = _rough(64, 1.0, 11)
    smp = lay.sample(_inside_points(lay, 20000, 17))
    rng = np.random.RandomState(18)
    p = rng.uniform(-1.5, 1.5, (len(smp), 2)).astype(F)
    worst = 0.0
    for ulp in (-1, 0, 1):
        plain = rippled64.normal32(p[:, 0], p[:, 1], ulp)
        got = rippled64.normal32(rippled64.slope32(p[:, 0], smp[:, 1]), rippled64.slope32(p[:, 1], smp[:, 2]), ulp)
        want, pp = rippled64.relift64(plain, smp)
        worst = max(worst, float((np.abs(got - want).max(1) / (EPS * (1 + pp))).max()))
    print(f"K_RIPN: worst ratio {worst:.3f}")
    assert worst <= rippled64.K_RIPN / 3 <= 1.5 * worst, worst
    # the bar tells a wrong slope term: each planted mistake misses it by far
    plain = rippled64.normal32(p[:, 0], p[:, 1])
    want, pp = rippled64.relift64(plain, smp)
    for m in ("sign", "no_half"):
        bad = rippled64.normal32(rippled64.slope32(p[:, 0], smp[:, 1], m), rippled64.slope32(p[:, 1], smp[:, 2], m))
        assert (np.abs(bad - want).max(1) / (EPS * (1 + pp))).max() > 1000 * rippled64.K_RIPN, m


def test_folded_share_on_the_golden_cascades(oracle):
    """the float64 comparison of tests/test_gpu_rippled.py::test_query runs on cascades 2 and 3 of its 64^2 x 4 handle (choppiness 0.8 and
    1.0 on the golden spectra) at 16 iterations: on those maps, one step old as there, blend64 alone leaves at most 5 % of the test's point
    set with a residual above the fold threshold"""
    from datum_amd import capi
    from test_gpu_rippled import FOLD, _points
    from test_gpu_surface import CHOPS, DT, SCALES, _h0, _phase
    from test_gpu_surface import _set as device_set

    capi.load()
    N, R, cell = 64, 128, 0.5
    maps = {}
    for c in (2, 3):
        phase = _phase(N, 77 + c)
        maps[c] = oracle.displace(_h0(oracle, N, 1000 + c, SCALES[c]), phase, SCALES[c], CHOPS[c], dt=float(DT), w=oracle.weights(N, reduced=True))
        assert CHOPS[c] <= 1.0
    q = _points(R, cell, N + R)[:-3]
    for cascades in ([2], [2, 3]):
        for swell in (True, False):
            res = blend64.surface_blend64([maps[c] for c in cascades], None, "off", [float(F(1) / F(SCALES[c])) for c in cascades], device_set(capi, 0, swell), q, 16)[:, 3]
            assert (res > FOLD).mean() <= 0.05, (cascades, swell, float((res > FOLD).mean()))
