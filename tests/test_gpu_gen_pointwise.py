"""The projected-grid mesh kernel (datum_amd/csrc/ocean_gen.hip) stage by stage, point by point, against the staged reference of
tests/gen64.py (validated against the fp32 oracle alone by tests/test_gen64.py, which also checks the conditions on the cases):

  a. the ray stage bit for bit and the store pattern: with swellsteepness = 0 texcoord = 0.1f * base.xy is a function of the view ray,
     the plane hit and nothing else, and the oracle's ray stage is the same IEEE fp32 expression tree -- every texcoord bit of every
     vertex has to match, for nine cameras and five mesh sizes (one column, one tile, one vertex past a tile); no sentinel is left
     inside the mesh, none is touched behind it;
  b. the swell's sin / cos and the Gerstner frame on a flat ocean: vertex.z = basez + amplitude * sin(theta) and texcoord =
     0.1 (base + gx cos(theta)) per vertex from the fp32 theta, within the bar of ocean_phase.h's sin / cos; the frame within 8 x the
     oracle's own distance to the same float64 evaluation;
  c. the bilinear sample on real maps in every map layout: vertex.xyz - position is the four-texel blend alone, within a few ulp of the
     largest corner texel -- at 1000 m from the camera as next to it.

Every bar is derived in tests/gen64.py or taken from the oracle as the yardstick; none is fitted to the kernel's output.
"""

import numpy as np
import pytest

import gen64
import gen_cases

pytestmark = pytest.mark.gpu

F = np.float32
DT = np.float32(1.0 / 60.0)
SENTINEL = np.float32(-3.0e38)           # no vertex component comes near it
GUARD = 64

CAMERAS = ["example", "pitched_steep", "above_horizon", "rolled", "high", "plane_w", "grazing", "nadir", "altitude"]
MESHES = [(2, 2), (17, 3), (31, 15), (33, 17), (200, 150)]
STEEP = ["pitched_steep", "above_horizon", "rolled", "high", "plane_w"]
SAMPLED = ["pitched_steep", "above_horizon", "grazing"]


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


def header(oracle, N, case, steepness=None, amplitude=None, wavescale=None):
    s = gen_cases.oceanset(oracle, N, case, wavescale=wavescale)
    if steepness is not None:
        s.swellsteepness = steepness
    if amplitude is not None:
        s.swellamplitude = amplitude
    return s


def ocean(capi, oracle, N, h0, wavescale=None, steps=1):
    oc = capi.Ocean(N, 1)
    oc.set_cascade(0, oracle.EXAMPLE["wavescale"] if wavescale is None else wavescale, oracle.EXAMPLE["choppiness"])
    oc.upload_state(0, h0)
    for _ in range(steps):
        oc.update(DT)
    oc.displace()
    return oc


def mesh(capi, torch, oc, s, sx, sy):
    """one launch into a sentinel-filled buffer with a guard tail: the mesh [sy, sx, 12], after the store pattern's checks"""
    verts = torch.full((sx * sy * 12 + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()              # torch's stream and the handle's own are not ordered
    oc.gen(0, capi.OceanSet.from_buffer_copy(bytes(s)), sx, sy, verts.data_ptr())
    oc.sync()
    raw = verts.cpu().numpy()
    sentinel = np.array([SENTINEL], F).view(np.uint32)[0]
    assert np.all(raw[sx * sy * 12:].view(np.uint32) == sentinel), "the guard tail was written"
    got = raw[: sx * sy * 12].reshape(sy, sx, 12)
    left = np.argwhere(got.view(np.uint32) == sentinel)
    assert left.size == 0, ("vertices not written", sx, sy, left[:4])
    assert np.isfinite(got).all()
    assert np.all(got[..., 11] == -1)
    return got


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_texcoord_bits(got, ray, label):
    want = (F(0.1) * ray.base).astype(F)
    bad = np.argwhere(bits(got[..., 3:5]) != bits(want))
    assert bad.size == 0, (label, bad.shape[0], bad[:4], got[..., 3:5][tuple(bad[0])], want[tuple(bad[0])])


# -- a. the ray stage bit for bit, the store pattern ----------------------------------------------------------------------------------


@pytest.mark.parametrize("case", CAMERAS)
def test_ray_stage_bits_and_store_pattern(capi, oracle, torch, report, case):
    N = 64
    with ocean(capi, oracle, N, gen64.band_limited_h0(N, 7)) as oc:
        maps = oc.read_maps(0)
        for sx, sy in MESHES:
            s = header(oracle, N, case, steepness=0.0)
            got = mesh(capi, torch, oc, s, sx, sy)
            ray = gen64.ray32(s, sx, sy)
            want = oracle.gen(s, maps, sx, sy)
            same = float((bits(got) == bits(want)).mean())
            tex = float((bits(got[..., 3:5]) == bits(want[..., 3:5])).mean())
            report(f"genpw a {case} mesh {sx}x{sy}: texcoord bits equal {tex:.4f}, identical floats of the whole vertex {same:.3f}, "
                   f"rays hitting the plane {ray.hit.mean():.2f}, largest dist of a hit {float(ray.dist[ray.hit].max()) if ray.hit.any() else 0:.3g}")
            assert_texcoord_bits(got, ray, (case, sx, sy))
            assert np.array_equal(bits(got[..., 3:5]), bits(want[..., 3:5])), (case, sx, sy)


# -- b. swell and Gerstner frame on a flat ocean --------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", STEEP)
def test_swell_and_frame_on_a_flat_ocean(capi, oracle, torch, report, case):
    N, sx, sy = 64, 200, 150
    s = header(oracle, N, case)
    assert s.swellsteepness > 0
    with ocean(capi, oracle, N, np.zeros((N, N, 2), np.float32)) as oc:
        maps = oc.read_maps(0)
        got = mesh(capi, torch, oc, s, sx, sy).astype(np.float64)
    # what test_flat_ocean allows: zero displacement, normals along z up to the reciprocal square root's rounding
    assert np.all(maps[0] == 0) and np.all(maps[1][..., :2] == 0) and np.all(maps[1][..., 3] == 0) and np.abs(maps[1][..., 2] - 1).max() < 1e-6
    ray = gen64.ray32(s, sx, sy)
    assert float(np.abs(ray.theta).max()) <= 2.0 ** 21
    ref = gen64.staged64(s, maps, ray)
    want = ref.vertices
    bar = gen64.sin_bar(ray.theta)
    amplitude = float(ray.amplitude)

    ez = np.abs(got[..., 2] - want[..., 2])
    bz = amplitude * bar + 2.0 ** -23 * np.abs(want[..., 2])
    et = np.abs(got[..., 3:5] - want[..., 3:5])
    bt = np.stack([0.1 * (abs(float(g)) * bar + 2.0 ** -22 * np.abs(ref.position[..., c])) for c, g in ((0, ray.gx), (1, ray.gy))], -1)

    # for the record: the floats that the header's own sin / cos (walked on the CPU) predict bit for bit
    hs, hc, _, _ = gen64.header_sincos(ray.theta)
    with np.errstate(all="ignore"):
        pz = ray.basez + ray.amplitude * hs
        px, py = ray.base[..., 0] + ray.gx * hc, ray.base[..., 1] + ray.gy * hc
        ptex = np.stack([F(0.1) * px, F(0.1) * py], -1)
    same = (float((bits(got[..., 2].astype(F)) == bits(pz)).mean()), float((bits(got[..., 3:5].astype(F)) == bits(ptex)).mean()))

    ours = float(np.abs(got[..., 5:11] - want[..., 5:11]).max())
    yard = float(np.abs(oracle.gen(s, maps, sx, sy).astype(np.float64)[..., 5:11] - want[..., 5:11]).max())
    report(f"genpw b {case}: z error / bar {float((ez / bz).max()):.3f} (worst {float(ez.max()):.2e}), texcoord error / bar {float((et / bt).max()):.3f} "
           f"(worst {float(et.max()):.2e}), largest |theta| {float(np.abs(ray.theta).max()):.3g}; predicted by the header's sin / cos bit for bit: "
           f"z {same[0]:.4f}, texcoords {same[1]:.4f}; frame vs float64: kernel {ours:.2e}, oracle {yard:.2e}, bar {gen64.frame_bar(yard):.2e}")
    assert np.all(ez <= bz), (case, float((ez / bz).max()))
    assert np.all(et <= bt), (case, float((et / bt).max()))
    assert ours <= gen64.frame_bar(yard), (case, ours, yard)


# -- c. bilinear sampling on real maps ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("N,wavescale", [(64, None), (256, None), (1024, None), (2048, None), (4096, None), (4096, 1.5), (1024, 0.25)])
def test_bilinear_sample_on_real_maps(capi, oracle, torch, report, N, wavescale):
    # N = 1024: the map is beyond an XCD's L2, the tiles are dealt in chunks and the last set of chunks is ragged; 2048, 4096: banded maps.
    # The two wave scales put the far texel coordinates beyond 2^31 (test_gen_texel_coordinates_beyond_int32).  swellamplitude = 0 as well
    # as swellsteepness: position = (base.xy, basez) exactly, verified by the texcoord bits of the same launch, so that z - basez is the
    # bilinear sample alone as x and y are.
    sx, sy = 200, 150
    with ocean(capi, oracle, N, gen64.band_limited_h0(N, 7), wavescale=wavescale) as oc:
        maps = oc.read_maps(0)
        assert np.isfinite(maps).all()
        for case in SAMPLED if wavescale is None else ["above_horizon"]:
            s = header(oracle, N, case, steepness=0.0, amplitude=0.0, wavescale=wavescale)
            got = mesh(capi, torch, oc, s, sx, sy)
            ray = gen64.ray32(s, sx, sy)
            assert_texcoord_bits(got, ray, (case, N))
            got = got.astype(np.float64)
            ref = gen64.staged64(s, maps, ray)
            want = ref.vertices
            assert float(np.abs(ref.displacement).max()) > 0.02             # the maps are not flat
            err = np.abs(got[..., 0:3] - want[..., 0:3])
            bar = gen64.blend_bar(ref.corner, want[..., 0:3])
            far = np.hypot(want[..., 0], want[..., 1]) > 500.0
            ours = float(np.abs(got[..., 5:11] - want[..., 5:11]).max())
            yard = float(np.abs(oracle.gen(s, maps, sx, sy).astype(np.float64)[..., 5:11] - want[..., 5:11]).max())
            # (the sample itself in units of the largest corner texel: position cancels)
            sample = np.abs((got[..., 0:3] - want[..., 0:3])) / np.maximum(ref.corner, 1e-30)
            report(f"genpw c {case} N={N} wavescale {22.0 if wavescale is None else wavescale}: vertex.xyz error / bar {float((err / bar).max()):.3f} "
                   f"(beyond 500 m, {far.mean():.2f} of the mesh: {float((err / bar)[far].max()):.3f}), worst |error| x {float(err[..., 0].max()):.2e} "
                   f"y {float(err[..., 1].max()):.2e} z {float(err[..., 2].max()):.2e}, z error / largest corner texel {float(sample[..., 2].max()) / gen64.EPS:.2f} eps; "
                   f"frame vs float64: kernel {ours:.2e}, oracle {yard:.2e}, bar {gen64.frame_bar(yard):.2e}")
            bad = np.argwhere(err > bar)
            assert bad.size == 0, (case, N, bad.shape[0], bad[:4], err[tuple(bad[0])], bar[tuple(bad[0])])
            assert ours <= gen64.frame_bar(yard), (case, N, ours, yard)
