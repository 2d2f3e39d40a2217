"""The slab's margin without a GPU (include/datum_ocean_hip.h: datum_ocean_surface_slab): over the committed maps of
tests/golden/ocean_n64.npz after 1 / 60 / 600 steps, blend64's float64 height of the summed surface at 10^4 random points -- lists [0] and
[0, 0, 0], swell on and off -- lies strictly inside [zlo, zhi] of bounds64's restatement, and no nearer to either bound than half of pad.
"""

import os

import numpy as np
import pytest

import blend64
import bounds64
from test_surface_abi import _set

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ocean_n64.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def points():
    return np.random.RandomState(64).uniform(-150, 150, (10000, 2))


@pytest.mark.parametrize("steps", [1, 60, 600])
def test_heights_lie_inside_the_slab(golden, points, steps):
    maps = golden[f"maps_{steps}"]
    records = bounds64.fold_maps(maps)[None]
    assert records[0, 6] == 0 and records[0, 0] < 0 < records[0, 1]
    for cascades, scales in (([0], [F(1) / F(22)]), ([0, 0, 0], [F(1) / F(22), F(1) / F(7), F(1) / F(3)])):
        for swell in (True, False):
            s = _set(A=0.6 if swell else 0.0, steep=0.5 if swell else 0.0, plane_w=-0.3)
            zlo, zhi, _, _, pad = bounds64.slab32(records, cascades, *bounds64.frame32(s))
            z = blend64.surface_blend64([maps] * len(cascades), None, "off", scales, s, points, 4)[:, 2]
            assert np.isfinite(z).all() and pad > 0
            assert np.all(z > float(zlo)) and np.all(z < float(zhi))
            nearest = min(float(z.min()) - float(zlo), float(zhi) - float(z.max())) / float(pad)
            print(f"slab margin steps={steps} list={cascades} swell={swell}: [{float(zlo):.6f}, {float(zhi):.6f}], heights [{z.min():.6f}, {z.max():.6f}], "
                  f"nearest {nearest:.1f} pad")
            assert nearest >= 0.5
            if not swell and len(cascades) == 1:
                # the extreme texels' centres, no iteration: the heights there are basez + zmin and basez + zmax, one pad inside
                dz = maps[0, ..., 2]
                (jl, il), (jh, ih) = np.unravel_index(dz.argmin(), dz.shape), np.unravel_index(dz.argmax(), dz.shape)
                centres = (np.array([[il, jl], [ih, jh]], np.float64) + 0.5) / (64 * float(scales[0]))
                ze = blend64.surface_blend64([maps], None, "off", scales, s, centres, 0)[:, 2]
                edge = min(float(ze[0]) - float(zlo), float(zhi) - float(ze[1])) / float(pad)
                print(f"   at the extreme texels: heights {ze[0]:.6f}, {ze[1]:.6f}, nearest {edge:.3f} pad")
                assert abs(ze[0] - (0.3 + float(records[0, 0]))) < 1e-6 and abs(ze[1] - (0.3 + float(records[0, 1]))) < 1e-6
                assert float(zlo) < ze[0] and ze[1] < float(zhi) and edge >= 0.5
            # the slab is no wider than the extrema and the swell make it, but for the pad
            assert float(zhi) - float(zlo) <= 2 * 0.6 * swell + len(cascades) * float(records[0, 1] - records[0, 0]) + 2.5 * float(pad)
