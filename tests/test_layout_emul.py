"""The product's two private memory layouts (datum_amd/csrc/ocean_layout.h: the blocked work spectrum and the patched,
banded displacement maps) evaluated on the CPU at EVERY grid point of every resolution (tests/cpu/layout_emul.cpp) and
checked here: the texel -> offset formula is a bijection onto the cascade's block, the offset -> texel function undoes it,
the shift form the mesh and surface kernels use equals it, the work spectrum's index is a bijection with whole lines per
block row.  Exact integer checks, no tolerance.  (tests/test_golden_and_abi.py restates the documented map layout in numpy
on its own; nothing here is derived from it or the other way round.)"""

import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [64, 128, 256, 512, 1024, 2048, 4096]

# what the layout's description promises per resolution: the patch is as wide as the column pass's tile (8 up to 256^2, 2 at
# 512^2, 4 at 1024^2 and 2048^2, 2 at 4096^2), 16 texels in all; bands of 128 columns from 2048^2 up, whole rows below
PATCH_COLS = {64: 8, 128: 8, 256: 8, 512: 2, 1024: 4, 2048: 4, 4096: 2}
BAND_COLS = {64: 64, 128: 128, 256: 256, 512: 512, 1024: 1024, 2048: 128, 4096: 128}


@pytest.fixture(scope="module")
def emul():
    return ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _constants(emul, N):
    out = np.zeros(14, np.int64)
    assert emul.layout_constants(N, _p(out)) == 0
    names = ["bytes", "pw", "ph", "band", "texel", "patch_bytes", "part_b", "a_stride", "b_stride", "patch", "patchrow", "sbr", "bc32", "bc16"]
    return dict(zip(names, (int(v) for v in out)))


def _forward(emul, N):
    a, b, patch = (np.empty((N, N), np.int64) for _ in range(3))
    j = np.empty((N, N), np.int32)
    assert emul.layout_map_forward(N, _p(a), _p(b), _p(patch), _p(j)) == 0
    return a, b, patch, j


def _is_permutation(idx, count):
    idx = idx.ravel()
    if idx.size != count or idx.min() < 0 or idx.max() >= count:
        return False
    seen = np.zeros(count, bool)
    seen[idx] = True
    return bool(seen.all())


@pytest.mark.parametrize("N", SIZES)
def test_named_numbers(emul, N):
    c = _constants(emul, N)
    assert (c["texel"], c["patch_bytes"], c["part_b"], c["a_stride"], c["b_stride"], c["patch"]) == (24, 384, 256, 16, 8, 16)
    assert c["bytes"] == N * N * 24
    assert (c["pw"], c["ph"]) == (PATCH_COLS[N], 16 // PATCH_COLS[N])
    assert c["band"] == BAND_COLS[N]
    assert c["patchrow"] == (c["band"] // c["pw"]) * 384
    assert (c["sbr"], c["bc32"], c["bc16"]) == (8, 8, 8)


@pytest.mark.parametrize("N", SIZES)
def test_maps_forward_is_a_bijection_onto_the_block(emul, N):
    c = _constants(emul, N)
    a, b, patch, j = _forward(emul, N)

    assert not (a % 16).any() and not (b % 8).any()
    assert a.min() >= 0 and b.min() >= 0
    assert (a + 16).max() <= c["bytes"] and (b + 8).max() <= c["bytes"]

    # every range is whole 8-byte units: the 3 N^2 units of all parts A and B are each unit of the block exactly once
    units = c["bytes"] // 8
    assert units == 3 * N * N
    seen = np.zeros(units, bool)
    taken = 0
    for first in (a // 8, a // 8 + 1, b // 8):
        idx = first.ravel()
        assert not seen[idx].any()                      # no unit taken by an earlier part ...
        seen[idx] = True
        taken += idx.size
        assert int(np.count_nonzero(seen)) == taken     # ... and none twice within this one
    assert seen.all()

    # a patch is PW x PH neighbouring texels, part A then part B
    pw, ph = c["pw"], c["ph"]
    y, x = np.indices((N, N))
    assert (j == (y % ph) * pw + x % pw).all()
    assert (a == patch + 16 * j).all() and (b == patch + 256 + 8 * j).all()
    assert not (patch % 384).any()
    corner = patch[::ph, ::pw]
    assert (patch == np.repeat(np.repeat(corner, ph, axis=0), pw, axis=1)).all()
    assert _is_permutation(corner // 384, N * N // 16)

    # k patch rows down the same column: patchrow bytes per row of patches, inside the band
    assert (patch[ph:, :] - patch[:-ph, :] == c["patchrow"]).all()


@pytest.mark.parametrize("N", SIZES)
def test_maps_inverse_undoes_forward(emul, N):
    a, b, _, _ = _forward(emul, N)

    ry, rx = (np.empty(N * N, np.int32) for _ in range(2))
    ra, rb, ra0 = (np.empty(N * N, np.int64) for _ in range(3))
    assert emul.layout_map_inverse(N, _p(ry), _p(rx), _p(ra), _p(rb), _p(ra0)) == 0

    # part number r = 16 * patch + texel of the patch, patches in the order they lie in memory
    r = np.arange(N * N, dtype=np.int64)
    assert (ra == (r // 16) * 384 + (r % 16) * 16).all()
    assert (ra0 == ra).all()

    # forward after inverse
    assert ry.min() >= 0 and ry.max() < N and rx.min() >= 0 and rx.max() < N
    assert (a[ry, rx] == ra).all() and (b[ry, rx] == rb).all()

    # inverse after forward
    part = (a // 384) * 16 + (a % 384) // 16
    assert (ry[part] == np.arange(N)[:, None]).all() and (rx[part] == np.arange(N)[None, :]).all()
    assert _is_permutation(ry.astype(np.int64) * N + rx, N * N)


@pytest.mark.parametrize("N", SIZES)
def test_texel_index_shifts_equal_the_formula(emul, N):
    a, b, _, _ = _forward(emul, N)

    sa, sb = (np.empty((N, N), np.int64) for _ in range(2))
    layout = ctypes.c_int(-1)
    assert emul.layout_map_shifts(N, _p(sa), _p(sb), ctypes.byref(layout)) == 0

    assert layout.value == (1 if BAND_COLS[N] != N else 0)       # GEN_BANDED where there are bands, else GEN_PLAIN
    assert (sa == a).all()
    assert (sb == b).all()


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("N", SIZES)
def test_work_spectrum_blocks(emul, N, half):
    c = _constants(emul, N)
    bc = c["bc16"] if half else c["bc32"]

    at = np.empty((N, N), np.int64)
    assert emul.layout_blocked(N, half, _p(at)) == 0

    assert _is_permutation(at, N * N)

    # a row of a block is contiguous, a block is its SBR rows one after the other
    x = np.arange(N)
    inrow = (x % bc) != bc - 1
    assert (at[:, 1:][:, inrow[:-1]] - at[:, :-1][:, inrow[:-1]] == 1).all()
    y = np.arange(N)
    inblock = (y % c["sbr"]) != c["sbr"] - 1
    assert (at[1:, :][inblock[:-1], :] - at[:-1, :][inblock[:-1], :] == bc).all()

    if not half:
        # sixteen-byte values: a block row is one whole 128-byte line
        assert bc * 16 == 128
        assert not ((at[:, ::bc] * 16) % 128).any()
