"""The DEEP step's arithmetic (datum_amd/csrc/ocean_ripple_deep.h), the very functions the kernel of ocean_ripple_deep.hip calls, walked on
the CPU (tests/cpu/ripple_deep_emul.cpp) against ripple_deep64's numpy float32 restatement, bit for bit, on tests/test_ripple_emul.py's
cases: R = 64 and 128, origins (0, 0) and (37, -21), 1, 3 and 16 sub-steps, the sponge on and off, random state and src.  The weights are
the header's own (its builder is walked too and held against numpy's float64 construction).

The restatement's worst distance from its own float64 form over those cases, in units of eps max|eta|, is the bar the device is held to:
K_RIP_DEEP (ripple_deep64.py) is 3 x that measured value, and test_k_rip_deep checks that it still is.
"""

import ctypes
import os

import numpy as np
import pytest

import ripple_deep64 as rd
from test_ripple_emul import CASES, EPS, F, ROOT, _bits, _p

DT = 0.1                     # per sub-step, as tests/test_ripple_emul.py has it: h sqrt(g sum|F| / s) = 1.03 at s = 0.5


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ripple_deep_emul_weights.argtypes = [P]
    lib.ripple_deep_emul_weights.restype = ctypes.c_double
    lib.ripple_deep_emul_substep.argtypes = [P, P, P, I, I, I, I, Fl, Fl, P, P, I]
    return lib


@pytest.fixture(scope="module")
def table(emul):
    G = np.zeros((rd.Q, rd.Q), F)
    total = emul.ripple_deep_emul_weights(_p(G))
    return G, total


def test_builder_against_numpy(table):
    G, total = table
    want = rd.weights64()
    assert np.abs(G.astype(np.float64)[1:, :] - want[1:, :]).max() <= 1e-6 * want[0, 0]
    assert np.abs(G.astype(np.float64) - want).max() <= 1e-6 * want[0, 0]
    s = float(rd.unfold(G).astype(np.float64).sum())
    assert 0.0 <= s <= 2.0 ** -23 * float(G[0, 0])
    assert total == rd.mass(G) and np.array_equal(G, G.T)
    # numpy's own rounding of the same construction differs by an fp32 rounding at the most
    assert np.abs(G.astype(np.float64) - rd.weights32().astype(np.float64)).max() <= 2.0 ** -23 * float(G[0, 0])


def _random_layer(G, R, origin, B, dtype, seed):
    rng = np.random.default_rng(seed)
    lay = rd.Layer(R, 0.5, dtype, B=B, G=G)
    lay.move(*origin)
    lay.set_window(rng.normal(size=(R, R)).astype(F), rng.normal(size=(R, R)).astype(F), rng.integers(-2 ** 21, 2 ** 21, (R, R)))
    return lay


def _emul_step(emul, lay, dt, substeps):
    h, gs, f = rd.params(lay.g, lay.s, lay.gamma, lay.B, lay.sponge_gamma, dt, substeps)
    state = np.ascontiguousarray(lay.state(), F)
    src = lay.src.copy()
    G = np.ascontiguousarray(lay.G, F)
    for i in range(substeps):
        out = np.empty_like(state)
        emul.ripple_deep_emul_substep(_p(state), _p(out), _p(src), lay.R, lay.ox, lay.oy, lay.B, float(h), float(gs), _p(f), _p(G), int(i == 0))
        state = out
        src[:] = 0
    return state


@pytest.fixture(scope="module")
def cases(emul, table):
    """every case once: (the header's walk, the restatement's state, the restatement's distance from float64 in eps max|eta|)"""
    out = {}
    for R, origin, substeps, B in CASES:
        lay = _random_layer(table[0], R, origin, B, F, R + substeps)
        l64 = _random_layer(table[0], R, origin, B, np.float64, R + substeps)
        got = _emul_step(emul, lay, DT * substeps, substeps)
        lay.step(DT * substeps, substeps)
        l64.step(DT * substeps, substeps)
        assert np.all(lay.src == 0) and rd.stable(lay.g, lay.s, DT * substeps, substeps, lay.G)
        out[R, origin, substeps, B] = got, lay.state(), np.abs(lay.eta.astype(np.float64) - l64.eta).max() / (EPS * np.abs(l64.eta).max())
    return out


@pytest.mark.parametrize("R,origin,substeps,B", CASES)
def test_substep_bits(cases, R, origin, substeps, B):
    got, want, _ = cases[R, origin, substeps, B]
    assert np.abs(want).max() > 1 and np.isfinite(want).all()
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:4]


def test_asymmetric_probe_bits(emul):
    """a table with G[l][k] != G[k][l]: the header indexes [|dj|][|di|] as the restatement does, and the swap is seen"""
    rng = np.random.default_rng(5)
    G = rng.normal(size=(rd.Q, rd.Q)).astype(F) * F(0.1)
    lay = _random_layer(G, 64, (37, -21), 8, F, 9)
    swapped = _random_layer(G, 64, (37, -21), 8, F, 9)
    got = _emul_step(emul, lay, DT, 1)
    lay.step(DT, 1)
    swapped.step(DT, 1, mistake="swap")
    assert np.array_equal(_bits(got), _bits(lay.state())) and not np.array_equal(_bits(got), _bits(swapped.state()))


def test_k_rip_deep(cases):
    """K_RIP_DEEP is 3 x the restatement's worst distance from float64 over the cases above (measured here, not on the GPU), and DESIGN.md
    states that measurement"""
    dist = {case: v[2] for case, v in cases.items()}
    worst = max(dist.values())
    print(f"DEEP restatement vs float64: worst {worst:.2f} eps max|eta| at {max(dist, key=dist.get)}; K_RIP_DEEP = {rd.K_RIP_DEEP}")
    assert 3 * worst <= rd.K_RIP_DEEP <= 3.3 * worst
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    assert f"worst {worst:.2f} eps" in design and f"`K_RIP_DEEP` = {rd.K_RIP_DEEP}" in design
