"""CPU tests of the several-cascade reference (tests/blend64.py): its one-cascade identities against surface64 and gen64, neutrality of a
zero map, slopes against the summed height on plane waves, and the sensitivity of the GPU suite's bars (tests/test_gpu_blend.py) to the
mistakes a wrong kernel would make."""

import numpy as np

import blend64
import gen64
import gen_cases
import surface64
from test_surface_abi import _set, _smooth_random_maps

EPS = 2.0 ** -24


def _maps(N, amp, seed, wavescale):
    """smooth displacement maps with the normal layer ocean.map.comp derives from dz: normalize(l.z - r.z, b.z - t.z, 4 wavescale / N)"""
    m = _smooth_random_maps(N, amp, seed)
    z = m[0, ..., 2]
    n = np.stack([np.roll(z, 1, 1) - np.roll(z, -1, 1), np.roll(z, 1, 0) - np.roll(z, -1, 0), np.full_like(z, 4 * wavescale / N)], -1)
    m[1, ..., :3] = n / np.sqrt((n * n).sum(-1, keepdims=True))
    return m


WS = [22.0, 64.0, 9.5, 140.0]


def test_one_cascade_is_surface64():
    N = 64
    maps = _maps(N, 0.3, 5, WS[0])
    foam = np.random.RandomState(2).uniform(0, 1, (N, N))
    s = _set(A=0.5, steep=0.3, length=35.0, wavescale=WS[0], plane_w=0.25)
    q = np.random.RandomState(9).uniform(-300, 300, (500, 2))
    for it in (0, 1, 4, 16):
        want = surface64.surface64(maps, foam, s, q, it)
        got = blend64.surface_blend64([maps], [foam], "accumulate", [float(s.scale)], s, q, it)
        assert np.abs(got - want).max() < 1e-12, it
        # the normal is scale-invariant in m: any positive multiple of the normal layer gives the same slopes
        scaled = maps.copy()
        scaled[1] *= 3.7
        again = blend64.surface_blend64([scaled], [foam], "accumulate", [float(s.scale)], s, q, it)
        assert np.abs(again - got).max() < 1e-12, it
        jac = blend64.surface_blend64([maps], [foam], "jacobian", [float(s.scale)], s, q, it)
        assert np.abs(jac[:, 7] - want[:, 7]).max() < 1e-12, it
        assert np.all(blend64.surface_blend64([maps], [foam], "off", [float(s.scale)], s, q, it)[:, 7] == 0)


def test_one_cascade_is_staged64(oracle):
    N = 64
    maps = _maps(N, 0.3, 5, WS[0]).astype(np.float32)
    for case in ("pitched_steep", "above_horizon"):
        s = gen_cases.oceanset(oracle, N, case, wavescale=WS[0])
        ray = gen64.ray32(s, 33, 17)
        want = gen64.staged64(s, maps, ray)
        got = blend64.staged_blend64(s, [maps], [float(s.scale)], ray)
        assert np.array_equal(got.vertices[..., :5], want.vertices[..., :5]), case
        # (the normal differs by definition: gen mixes the blended, unnormalised m with the plane normal, the blend normalises the slopes)


def test_a_zero_map_is_neutral():
    N = 64
    maps = _maps(N, 0.3, 5, WS[0])
    zero = np.zeros_like(maps)
    zero[1, ..., 2] = 1.0
    s = _set(A=0.5, steep=0.3, length=35.0, wavescale=WS[0])
    q = np.random.RandomState(1).uniform(-300, 300, (500, 2))
    one = blend64.surface_blend64([maps], None, "off", [1 / WS[0]], s, q, 4)
    two = blend64.surface_blend64([maps, zero], None, "off", [1 / WS[0], 1 / WS[1]], s, q, 4)
    assert np.abs(one - two).max() < 1e-12


def test_slope_sum_is_the_slope_of_the_summed_height():
    # one plane wave z_c = a_c cos(k_c . x) per cascade, sampled on texel centres so that the bilinear fetch reads a texel: the map's
    # m.x / m.z is the central difference -(z(x + h) - z(x - h)) / (4 wavescale / N) = -1/2 dz/dx up to O(h^2), and the sums agree
    N = 256
    samples = []
    s = _set(A=0.0, wavescale=WS[0])
    rs = np.random.RandomState(4)
    q = rs.uniform(-100, 100, (300, 2))
    dzdx = np.zeros(len(q))
    dzdy = np.zeros(len(q))
    for c, (a, kx, ky) in enumerate([(0.4, 2, 1), (0.2, -3, 2), (0.7, 1, -1)]):
        ws = WS[c]
        y, x = np.mgrid[0:N, 0:N]
        phase = 2 * np.pi * (kx * (x + 0.5) + ky * (y + 0.5)) / N
        m = np.zeros((2, N, N, 4))
        m[0, ..., 2] = a * np.cos(phase)
        z = m[0, ..., 2]
        n = np.stack([np.roll(z, 1, 1) - np.roll(z, -1, 1), np.roll(z, 1, 0) - np.roll(z, -1, 0), np.full_like(z, 4 * ws / N)], -1)
        m[1, ..., :3] = n / np.sqrt((n * n).sum(-1, keepdims=True))
        samples.append(surface64.bilinear64(m[1].transpose(2, 0, 1)[:3], q[:, 0] / ws, q[:, 1] / ws))
        # the bilinear interpolation of the texels' central differences against the analytic gradient: second order in 2 pi k / N
        ph = 2 * np.pi * (kx * q[:, 0] + ky * q[:, 1]) / ws
        dzdx += -a * np.sin(ph) * 2 * np.pi * kx / ws
        dzdy += -a * np.sin(ph) * 2 * np.pi * ky / ws
    dn = blend64.slopes64(samples)
    got = np.stack([dn[0] / dn[2], dn[1] / dn[2]])
    want = np.stack([-0.5 * dzdx, -0.5 * dzdy])
    scale = np.abs(want).max()
    assert np.abs(got - want).max() < 5e-3 * scale, (np.abs(got - want).max(), scale)
    # and summing unit normals instead is off by far more
    wrong = blend64.slopes64(samples, "normals")
    assert np.abs(np.stack([wrong[0] / wrong[2], wrong[1] / wrong[2]]) - want).max() > 0.3 * scale


def test_planted_mistakes_are_far_outside_the_bars():
    import test_gpu_blend as g

    N = 64
    cascades = [0, 1, 2]
    maps_list = [_maps(N, 0.3, 5 + c, WS[c]) for c in cascades]
    foams = [np.random.RandomState(20 + c).uniform(0, 1, (N, N)) for c in cascades]
    scales = [1 / WS[c] for c in cascades]
    s = _set(A=0.5, steep=0.3, length=35.0, wavescale=WS[0])
    q = np.random.RandomState(9).uniform(-300, 300, (2000, 2))
    want = blend64.surface_blend64(maps_list, foams, "accumulate", scales, s, q, 4)
    for mistake, fields in (("swap", "pos"), ("drop", "pos"), ("normals", "nrm"), ("min", "foam")):
        got = blend64.surface_blend64(maps_list, foams, "accumulate", scales, s, q, 4, mistake=mistake)
        kp, kn, kf = g._errors(got, want, q, maps_list, scales, N, foams)
        moved = {"pos": kp / g.K_POS, "nrm": kn / g.K_NRM, "foam": kf / g.K_FOAM}[fields]
        assert moved >= 100, (mistake, moved)
