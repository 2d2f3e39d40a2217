"""The staged reference of the mesh kernel (tests/gen64.py) and the cases of tests/test_gpu_gen_pointwise.py, validated on the CPU against
the fp32 oracle alone -- the oracle is itself a valid "kernel" for every bar the GPU test asserts, so no bar is tighter than fp32 allows:

  * ray32 is the oracle's ray stage bit for bit (texcoords at steepness 0), for every camera and mesh size of the GPU test;
  * the cases meet the kernel's documented precondition for its division and square root (operands and quotients in the normal range);
  * staged64 agrees with oracle.gen within the GPU test's bars, on a flat ocean and on oracle-made maps;
  * the bars notice a texel off by one and swapped weights far from the camera;
  * sin / cos of ocean_phase.h (the mesh kernel's, the row pass's and the surface queries') against float64 up to |x| = 2^21, the swell
    phase of a ray at the horizon, with a bar derived from the header's constants.
"""

import os

import numpy as np
import pytest

import gen64
import gen_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

CAMERAS = ["example", "pitched_steep", "above_horizon", "rolled", "high", "plane_w", "grazing", "nadir", "altitude"]
MESHES = [(2, 2), (17, 3), (31, 15), (33, 17), (200, 150)]
STEEP = ["pitched_steep", "above_horizon", "rolled", "high", "plane_w"]
SAMPLED = ["pitched_steep", "above_horizon", "grazing"]


def flat_maps(N):
    m = np.zeros((2, N, N, 4), np.float32)
    m[1, ..., 2] = 1
    return m


def header(oracle, N, case, steepness=None, amplitude=None, wavescale=None):
    s = gen_cases.oceanset(oracle, N, case, wavescale=wavescale)
    if steepness is not None:
        s.swellsteepness = steepness
    if amplitude is not None:
        s.swellamplitude = amplitude
    return s


_MAPS = {}


def oracle_maps(oracle, N, kind):
    """oracle-made maps, computed once: a seeded ocean after a few steps, or the band-limited spectrum the GPU test uploads"""
    if (N, kind) not in _MAPS:
        p = oracle.EXAMPLE
        if kind == "seeded":
            _, h0 = oracle.seed(N, 1000, p["wavescale"], p["waveamplitude"], p["windspeed"], p["winddirection"], sanitize=True)
        else:
            h0 = gen64.band_limited_h0(N, 7)
        phase = np.zeros((N, N), np.float32)
        for _ in range(2):
            oracle.update(phase, p["wavescale"], np.float32(1.0 / 60.0))
        m = oracle.displace(h0, phase, p["wavescale"], p["choppiness"], w=oracle.weights(N, reduced=True))
        m.setflags(write=False)
        _MAPS[(N, kind)] = m
    return _MAPS[(N, kind)]


def test_the_mesh_kernel_calls_the_header():
    # the sin / cos pinned below is the mesh kernel's: ocean_gen.hip keeps no copy of the reduction or the polynomials
    gen = open(os.path.join(ROOT, "datum_amd", "csrc", "ocean_gen.hip"), encoding="utf-8").read()
    assert "sincos_phase_pair_poly(theta" in gen
    for copy in ("1.57079637050628662109375f", "4.37113900018624283e-8f", "0.636619772367581343f", "1.9515295891e-4f"):
        assert copy not in gen, copy


@pytest.mark.parametrize("case", CAMERAS)
def test_ray32_is_the_oracle_ray_bit_for_bit(oracle, case):
    for sx, sy in MESHES:
        s = header(oracle, 64, case, steepness=0.0)
        ray = gen64.ray32(s, sx, sy)
        want = oracle.gen(s, flat_maps(64), sx, sy)
        tex = (F(0.1) * ray.base).astype(F)
        bad = np.argwhere(tex.view(np.uint32) != want[..., 3:5].view(np.uint32))
        assert bad.size == 0, (case, sx, sy, bad[:4])
        assert np.all(want[..., 11] == -1)


@pytest.mark.parametrize("case", CAMERAS)
def test_cases_meet_the_normal_range_precondition(oracle, case):
    # ocean_gen.hip: div_exact / sqrt_exact leave out v_div_scale / v_div_fixup "for operands in the normal range".  A condition on the
    # inputs: every operand and quotient of gen.comp:75-91 within [2^-100, 2^100], at both steepness settings the GPU test uses
    for sx, sy in MESHES:
        for steepness in (0.0, None):
            ray = gen64.ray32(header(oracle, 64, case, steepness=steepness), sx, sy)
            assert float(ray.cameraheight) > 0
            for name, lo, hi in gen64.normal_range(ray):
                assert gen64.NORMAL_LO <= lo and hi <= gen64.NORMAL_HI, (case, sx, sy, name, lo, hi)
            assert np.isfinite(ray.base).all() and np.isfinite(ray.theta).all()


def test_the_new_cameras_are_what_they_claim(oracle):
    sx, sy = 200, 150
    g = gen64.ray32(header(oracle, 64, "grazing"), sx, sy)
    assert 0.4 < g.hit.mean() < 0.6 and g.hit[: sy // 2 - 2].all() and not g.hit[sy // 2 + 2:].any()         # the sign change crosses the middle rows
    g2 = gen64.ray32(header(oracle, 64, "grazing"), 33, 17)                                                     # (a row at v = 0 exactly)
    assert float(g2.dist[g2.hit].max()) > 1e5 and float(g2.cameraheight) == pytest.approx(0.3, rel=1e-5)
    n = gen64.ray32(header(oracle, 64, "nadir"), sx, sy)
    assert n.hit.all()
    for c in range(2):                                                                                          # components through zero
        assert (n.worlddir[..., c] < 0).any() and (n.worlddir[..., c] > 0).any()
    assert (n.viewvec[..., 0] == 0).any() or ((n.viewvec[..., 0] < 0).any() and (n.viewvec[..., 0] > 0).any())
    a = gen64.ray32(header(oracle, 64, "altitude"), sx, sy)
    assert float(a.cameraheight) == pytest.approx(2e4, rel=1e-5) and a.hit.mean() > 0.9 and float(a.margin) < 1.02


@pytest.mark.parametrize("case", STEEP)
def test_staged64_agrees_with_the_oracle_on_a_flat_ocean(oracle, case):
    # test_gpu_gen_pointwise.py (b) with the oracle in the kernel's place: libm's sinf / cosf are within the bar of the header's
    sx, sy, N = 200, 150, 64
    s = header(oracle, N, case)
    assert s.swellsteepness > 0
    ray = gen64.ray32(s, sx, sy)
    assert float(np.abs(ray.theta).max()) <= 2.0 ** 21
    ref = gen64.staged64(s, flat_maps(N), ray)
    got = oracle.gen(s, flat_maps(N), sx, sy).astype(np.float64)
    bar = gen64.sin_bar(ray.theta)
    want = ref.vertices
    assert np.all(np.abs(got[..., 2] - want[..., 2]) <= float(ray.amplitude) * bar + 2.0 ** -23 * np.abs(want[..., 2]))
    for c, g in ((0, float(ray.gx)), (1, float(ray.gy))):
        assert np.all(np.abs(got[..., 3 + c] - want[..., 3 + c]) <= 0.1 * (abs(g) * bar + 2.0 ** -22 * np.abs(ref.position[..., c]))), (case, c)
    # the frame: the oracle is the yardstick there; it has to be a small one (a few ulp) for 8 x yardstick to mean anything
    assert np.abs(got[..., 5:11] - want[..., 5:11]).max() < 16 * gen64.EPS, case


@pytest.mark.parametrize("N,kind", [(64, "seeded"), (256, "seeded"), (64, "band"), (256, "band")])
@pytest.mark.parametrize("case", SAMPLED)
def test_staged64_agrees_with_the_oracle_on_real_maps(oracle, case, N, kind):
    # test_gpu_gen_pointwise.py (c) with the oracle in the kernel's place
    sx, sy = 200, 150
    s = header(oracle, N, case, steepness=0.0, amplitude=0.0)
    maps = oracle_maps(oracle, N, kind)
    ray = gen64.ray32(s, sx, sy)
    ref = gen64.staged64(s, maps, ray)
    got = oracle.gen(s, maps, sx, sy).astype(np.float64)
    assert np.array_equal(got[..., 3:5], (F(0.1) * ray.base).astype(np.float64))
    err = np.abs(got[..., 0:3] - ref.vertices[..., 0:3])
    bar = gen64.blend_bar(ref.corner, ref.vertices[..., 0:3])
    bad = np.argwhere(err > bar)
    assert bad.size == 0, (case, N, bad[:4], err[tuple(bad[0])], bar[tuple(bad[0])])
    assert np.abs(got[..., 5:11] - ref.vertices[..., 5:11]).max() < 16 * gen64.EPS
    assert float(np.abs(ref.displacement).max()) > 0.05             # the maps are not flat


@pytest.mark.parametrize("N,kind", [(64, "seeded"), (256, "seeded"), (64, "band"), (256, "band")])
@pytest.mark.parametrize("case", ["pitched_steep", "above_horizon", "high"])
def test_the_blend_bar_notices_a_wrong_texel_far_from_the_camera(oracle, case, N, kind):
    # a texel off by one in x or in y, and ax / ay swapped, at the vertices beyond 500 m: the error is over the bar (in some component of
    # vertex.xyz) at 90 % of them and more.  A swap of two EQUAL weights is no mistake -- beyond 2^23 texels both are exactly zero -- so
    # the swap is counted where ax != ay.
    sx, sy = 200, 150
    s = header(oracle, N, case, steepness=0.0, amplitude=0.0)
    maps = oracle_maps(oracle, N, kind)
    ray = gen64.ray32(s, sx, sy)
    ref = gen64.staged64(s, maps, ray)
    far = np.hypot(ref.vertices[..., 0], ref.vertices[..., 1]) > 500.0
    assert far.mean() >= 0.1
    bar = gen64.blend_bar(ref.corner, ref.vertices[..., 0:3])
    for what, kw, among in (("i0 + 1", dict(shift=(1, 0)), far), ("j0 + 1", dict(shift=(0, 1)), far), ("i0 - 1", dict(shift=(-1, 0)), far),
                            ("ax <-> ay", dict(swap_weights=True), far & (ref.ax != ref.ay))):
        wrong = gen64.staged64(s, maps, ray, **kw)
        seen = (np.abs(wrong.vertices[..., 0:3] - ref.vertices[..., 0:3]) > bar).any(-1)
        assert among.mean() >= 0.05, (what, among.mean())
        assert seen[among].mean() >= 0.9, (case, N, kind, what, seen[among].mean())


@pytest.mark.parametrize("N,wavescale", [(N, None) for N in (64, 256, 1024, 2048, 4096)] + [(4096, 1.5), (1024, 0.25)])
def test_sampled_cases_reach_the_wrap_and_the_far_field(oracle, N, wavescale):
    # conditions on the cases of test_gpu_gen_pointwise.py (c): under every camera a tenth of the mesh lies beyond 500 m; in every map
    # layout the wrap column and row i0 = N - 1 and j0 = N - 1 occur with a non-zero weight on their second texel (column / row 0) --
    # under some camera of the layout: a 200 x 150 mesh looking along +x does not land in a 5 mm column of a 4096^2 map, one looking
    # sideways does
    sx, sy = 200, 150
    wrapx = wrapy = 0
    for case in SAMPLED if wavescale is None else ["above_horizon"]:
        s = header(oracle, N, case, steepness=0.0, amplitude=0.0, wavescale=wavescale)
        ray = gen64.ray32(s, sx, sy)
        i0, j0, ax, ay = gen64.texel32(s, ray, N, ray.base[..., 0], ray.base[..., 1])
        assert (np.hypot(ray.base[..., 0], ray.base[..., 1]) > 500.0).mean() >= 0.1, case
        assert i0.min() >= 0 and i0.max() < N and j0.min() >= 0 and j0.max() < N
        wrapx += int(((i0 == N - 1) & (ax != 0)).sum())
        wrapy += int(((j0 == N - 1) & (ay != 0)).sum())
        if wavescale is not None:
            # texel coordinates beyond 2^31, where an int32 conversion saturates, and weights that are exactly zero (the skipped fetches)
            assert (np.abs(ray.base[..., 0].astype(np.float64)) * float(s.scale) * N > 2.0 ** 31).mean() > 0.1
            assert ((ax == 0) & (ay == 0)).mean() > 0.1 and ((ax != 0) & (ay != 0)).mean() > 0.1
    assert wrapx > 0 and wrapy > 0, (N, wrapx, wrapy)


def test_sincos_constants_and_the_bar():
    # c of the bar 4 * 2^-24 + |x| * c, from the header's own constants: |HEAD + TAIL - pi/2| * 2/pi
    hdr = open(os.path.join(ROOT, "datum_amd", "csrc", "ocean_phase.h"), encoding="utf-8").read()
    assert "-1.57079637050628662109375f" in hdr and "4.37113900018624283e-8f" in hdr
    d = gen64.pio2_representation_error()
    assert 1.70e-15 < d < 1.73e-15
    assert gen64.SINCOS_C == pytest.approx(2 / np.pi * d)
    assert 2.0 ** -50 < gen64.SINCOS_C < 2.0 ** -49.5          # "about 2^-50 per unit of x": 2^-49.70
    # at the top of the range the pi/2 term is a hundredth of the rounding term
    assert gen64.sin_bar(2.0 ** 21) - gen64.sin_bar(0.0) < 0.01 * gen64.sin_bar(0.0)


def test_header_sincos_against_float64_up_to_2_to_the_21():
    rng = np.random.default_rng(20261)
    n = 1 << 20
    sign = rng.choice([-1.0, 1.0], n)
    x = [sign * np.exp(rng.uniform(np.log(1e-3), np.log(2.0 ** 21), n)),                 # log-spaced
         sign * np.exp(rng.uniform(np.log(2.0 ** 17), np.log(2.0 ** 21), n)),            # the horizon's decades
         rng.uniform(-2.0 ** 21, 2.0 ** 21, 2 * n),                                      # uniform: half of it beyond 2^20
         [0.0, -0.0, 2.0 ** 21, -2.0 ** 21, 2.0 ** 20, 1e5, 1e6]]
    # the fp32 neighbours (+-2 ulp) of k pi/2 for 2^16 counts up to 2^21 * 2/pi: where the reduction cancels most
    k = np.unique(np.concatenate([rng.integers(-1335088, 1335089, 1 << 16), [1335088, -1335088, 1, 0]])).astype(np.float64)
    centre = (k * (np.pi / 2)).astype(F)
    lo = hi = centre
    near = [centre]
    for _ in range(2):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        near += [lo, hi]
    # ... and of (k + 1/2) pi/2, the quadrant boundaries, where the quarter-turn count is decided
    edge = ((k + 0.5) * (np.pi / 2)).astype(F)
    x = np.concatenate([np.asarray(a, np.float64) for a in x] + [np.concatenate(near).astype(np.float64), edge.astype(np.float64)]).astype(F)
    x = x[np.abs(x) <= F(2.0 ** 21)]
    assert x.size >= (1 << 22)
    sn, cs, sn2, cs2 = gen64.header_sincos(x)
    assert np.array_equal(sn.view(np.uint32), sn2.view(np.uint32)) and np.array_equal(cs.view(np.uint32), cs2.view(np.uint32))     # scalar and packed form
    x64 = x.astype(np.float64)
    es = np.abs(sn.astype(np.float64) - np.sin(x64))
    ec = np.abs(cs.astype(np.float64) - np.cos(x64))
    bar = gen64.sin_bar(x64)
    edges = [0.0, 1e4, 1e5, 2.0 ** 19, 2.0 ** 20, np.inf]
    for a, b in zip(edges[:-1], edges[1:]):
        m = (np.abs(x64) >= a) & (np.abs(x64) < b)
        print(f"sincos_phase, {a:.6g} <= |x| < {b:.6g}, {int(m.sum())} arguments: max |sin error| {es[m].max():.3e}, max |cos error| {ec[m].max():.3e}, "
              f"bar {bar[m].min():.3e} .. {bar[m].max():.3e}")
    worst = int(np.argmax(np.maximum(es, ec) / bar))
    assert np.all(es <= bar) and np.all(ec <= bar), (x[worst], es[worst], ec[worst], bar[worst])
    assert float(np.abs(sn).max()) <= 1.0 and float(np.abs(cs).max()) <= 1.0
    # (for the record: a correctly reduced fp32 libm over the same arguments)
    print(f"numpy float32 sin over the same arguments: {float(np.abs(np.sin(x).astype(np.float64) - np.sin(x64)).max()):.3e}")
