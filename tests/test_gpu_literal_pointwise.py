"""The literal transform mode (datum_ocean_set_literal_transform: ocean_literal.hip's sim / radix-2 Stockham / map kernels) pinned
texel by texel: every texel of all six channels against ref64.lit64 -- the reference's algorithm in float64 on the fp32 twiddle
table the module serves -- where tests/test_gpu_parity.py holds the mode to a displacement RMSE only.  Nothing is masked or sampled.

  * every loop shape     64^2 (fewer lanes than the 256 threads of literal_fft_kernel), 256^2 (one lane per thread), 1024^2 (four lanes
                         per thread; the grid-stride loops of sim and map take more than one trip) against lit64
  * large sizes          2048^2, 4096^2 (banded map layout, 32 / 64 KB of LDS per line, 8 / 16 lanes per thread) against the fp32 oracle
                         at twice the bar: both sides carry the noise of the same arithmetic, each within one bar of the float64 value
  * single bins          one nonzero h0 bin at the corners, at k = 0 and on one row / column of the transforms, phase zero and not
  * cascades             three cascades of one handle, each against lit64 with its own scale (the per-cascade LiteralArgs)

Bars (tests/pointwise.py): K_LIT_DISP, K_LIT_NORMAL, K_LIT_EDGE = 3 x the error of the reference's own fp32 arithmetic against lit64 on
these same inputs, measured and asserted on the CPU by tests/test_lit64.py; the error forms are those of tests/test_gpu_pointwise.py.
The table itself (datum_ocean_reference_weights == oracle.weights, bit for bit, at every N used here) is
tests/test_golden_and_abi.py::test_reference_weights_match_oracle; that literal -> fused -> literal on one state gives the first
literal maps back bit for bit is tests/test_gpu_parity.py::test_literal_transform_mode_against_the_literal_oracle, at every N used
here (1024^2 included).  Each case reports its measured K beside the bar (profiles/literal_pointwise_table.txt keeps them)."""

import numpy as np
import pytest

import pointwise as pw
import ref64

pytestmark = pytest.mark.gpu

DT = pw.DT


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


def _read(oc, c, want_phase, label):
    """cascade c's channels [6][N][N] after the checks that need no reference: phase bit for bit, .w == 0, everything finite"""
    maps = oc.read_maps(c)
    assert np.array_equal(oc.read_state(c), want_phase), (label, "phase")
    assert np.all(maps[..., 3] == 0), (label, ".w")
    assert np.isfinite(maps).all(), label
    return ref64.channels(maps).astype(np.float64)


def _line(what, kd, kn, bd, bn):
    return (f"literal pointwise {what}: disp K {kd:.3g} (bar {bd:.3g}, margin {bd / kd if kd > 0 else float('inf'):.1f}x); "
            f"normal K {kn:.3g} (bar {bn:.3g}, margin {bn / kn if kn > 0 else float('inf'):.1f}x)")


@pytest.mark.parametrize("N", pw.LIT_SIZES)
def test_every_loop_shape_against_lit64(capi, oracle, report, N):
    p = oracle.EXAMPLE
    ws, chop = p["wavescale"], p["choppiness"]
    h0 = pw.lit_state(oracle, N)
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, ws, chop)
        oc.upload_state(0, h0)
        oc.set_literal_transform(True)
        for _ in range(pw.LIT_STEPS):                # every displace overwrites every texel of the one before
            oc.update(DT)
            oc.displace()
        phase = pw.lit_phase(oracle, N, ws, pw.LIT_STEPS)
        got = _read(oc, 0, phase, N)
    ref, ln = ref64.lit64(h0, phase, np.float32(1) / np.float32(ws), chop, capi.reference_weights(N), return_len=True)
    kd, kn, _ = pw.pointwise(got, ref, ln, N)
    report(_line(f"N={N:4d} vs lit64", kd, kn, pw.K_LIT_DISP, pw.K_LIT_NORMAL))
    assert kd <= pw.K_LIT_DISP and kn <= pw.K_LIT_NORMAL, (N, kd, kn)


@pytest.mark.parametrize("N", pw.LIT_LARGE)
def test_large_sizes_against_the_fp32_oracle(capi, oracle, report, N):
    p = oracle.EXAMPLE
    ws, chop = p["wavescale"], p["choppiness"]
    h0 = pw.lit_state(oracle, N)
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, ws, chop)
        oc.upload_state(0, h0)
        oc.set_literal_transform(True)
        for _ in range(pw.LIT_STEPS):
            oc.update(DT)
            oc.displace()
        phase = pw.lit_phase(oracle, N, ws, pw.LIT_STEPS)
        got = _read(oc, 0, phase, N)
    ref = ref64.channels(oracle.displace(h0, phase.copy(), ws, chop, w=oracle.weights(N), mt=True)).astype(np.float64)
    ln = ref64.normal_len(ref[2], np.float32(1) / np.float32(ws))
    kd, kn, _ = pw.pointwise(got, ref, ln, N)
    report(_line(f"N={N:4d} vs the fp32 oracle", kd, kn, 2 * pw.K_LIT_DISP, 2 * pw.K_LIT_NORMAL))
    assert kd <= 2 * pw.K_LIT_DISP and kn <= 2 * pw.K_LIT_NORMAL, (N, kd, kn)


@pytest.mark.parametrize("N", pw.LIT_EDGE_SIZES)
def test_single_bins_against_lit64(capi, oracle, report, N):
    # one bin per cascade of one handle; the maps at phase zero, then after one update
    p = oracle.EXAMPLE
    ws, chop = p["wavescale"], p["choppiness"]
    scale = np.float32(1) / np.float32(ws)
    bins = pw.lit_edge_bins(N)
    w = capi.reference_weights(N)
    got = {}
    with capi.Ocean(N, len(bins)) as oc:
        for c, b in enumerate(bins):
            oc.set_cascade(c, ws, chop)
            oc.upload_state(c, pw.lit_edge_h0(N, b))
        oc.set_literal_transform(True)
        done = 0
        for steps in pw.LIT_EDGE_STEPS:
            for _ in range(steps - done):
                oc.update(DT)
            done = steps
            oc.displace()
            phase = pw.lit_phase(oracle, N, ws, steps)
            for c, b in enumerate(bins):
                got[b, steps] = _read(oc, c, phase, (N, b, steps))
    worst = [0.0, 0.0]
    every = []
    for (b, steps), g in got.items():
        ref, ln = ref64.lit64(pw.lit_edge_h0(N, b), pw.lit_phase(oracle, N, ws, steps), scale, chop, w, return_len=True)
        assert float(np.abs(ref[2]).max()) > 0.1, (b, steps)
        kd, kn, _ = pw.pointwise(g, ref, ln, N)
        worst = [max(worst[0], kd), max(worst[1], kn)]
        every.append((b, steps, kd, kn))
    report(_line(f"N={N:4d} single bins ({len(every)} maps) vs lit64", worst[0], worst[1], pw.K_LIT_EDGE, pw.K_LIT_NORMAL))
    for b, steps, kd, kn in every:
        assert kd <= pw.K_LIT_EDGE and kn <= pw.K_LIT_NORMAL, (N, b, steps, kd, kn)


def test_cascades_against_lit64(capi, oracle, report):
    chop = oracle.EXAMPLE["choppiness"]
    N = pw.LIT_CASCADES[0]
    states = pw.lit_cascade_states(oracle)
    w = capi.reference_weights(N)
    with capi.Ocean(N, len(states)) as oc:
        for c, (ws, h0) in enumerate(states):
            oc.set_cascade(c, ws, chop)
            oc.upload_state(c, h0)
        oc.set_literal_transform(True)
        for _ in range(pw.LIT_STEPS):
            oc.update(DT)
            oc.displace()
        phases = [pw.lit_phase(oracle, N, ws, pw.LIT_STEPS) for ws, _ in states]
        got = [_read(oc, c, phases[c], c) for c in range(len(states))]
    every = []
    for c, (ws, h0) in enumerate(states):
        ref, ln = ref64.lit64(h0, phases[c], np.float32(1) / np.float32(ws), chop, w, return_len=True)
        kd, kn, _ = pw.pointwise(got[c], ref, ln, N)
        report(_line(f"N={N:4d} cascade {c} of {len(states)} (wavescale {ws:g}) vs lit64", kd, kn, pw.K_LIT_DISP, pw.K_LIT_NORMAL))
        every.append((c, kd, kn))
    for c, kd, kn in every:
        assert kd <= pw.K_LIT_DISP and kn <= pw.K_LIT_NORMAL, (c, kd, kn)
    # the scale is the cascade's own: with its neighbour's (which enters nz) the normals of cascade 0 are far outside the bar
    ref, ln = ref64.lit64(states[0][1], phases[0], np.float32(1) / np.float32(states[1][0]), chop, w, return_len=True)
    assert pw.pointwise(got[0], ref, ln, N)[1] > 100 * pw.K_LIT_NORMAL
