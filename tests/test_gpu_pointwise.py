"""Pointwise pins of the displacement maps against the float64 reference of tests/ref64.py, in every kernel form the module
instantiates (row pass: 4 / 8 / 16 points per thread and the sequential 4096^2 form; column pass: written through, streamed,
streamed with walking workgroups) and every spectrum format (fp32, fp16, fp16 with h0 as halves).

Three comparisons per case, each from exactly the input the stage saw:
  * end to end   maps vs displace64(h0, phase) -- every point in fp32; RMSE in the fp16 formats, whose halves are pinned below
  * row pass     datum_ocean_debug_rowpass vs rowpass64 -- fp32: every element within fp32 noise of its row's RMS; fp16 formats:
                 every value times 2^e is a half, and it is the half nearest the float64 value (ties to even) unless that value
                 lies within the fp32 noise band of a rounding midpoint, where either neighbour is accepted
  * column pass  maps vs colpass64(the GPU's own row-pass output) -- every point, at fp32 precision in all three formats
and, from 1024^2 up, the shape of the error: no column, row or border ring of the grid stands out from the rest.

Bars, with eps = 2^-24 and L = log2 N (one constant per family for every N):
  displacement channel ch   |got - ref| <= K_MAP * eps * L * s_ch,  s_ch = max(rms(ch), rms(dx, dy, dz) / 4)
  normal channels           |got - ref| <= K_NORMAL * eps * (L * (r_n + s_dz) / len + 1), len = |(nx, ny, nz)| of the reference
                            before normalisation at that point, r_n the RMS of its slopes (the slopes' error is divided by len)
  row pass, per element     |got - ref| <= K_ROW * eps * L * rms(row); in the fp16 formats the stored half must be the rounding of
                            some value within K_BAND * eps * L * rms(row) of the float64 one
  single-bin known answers  as the displacement channels, with K_EDGE
Each test reports the measured worst value next to its bar (tests/conftest.py: report); profiles/r07_pointwise_table.txt keeps them.
Against the RMSE < 1e-5 bars of tests/test_gpu_parity.py, which allow one value off by ~1e-5 * sqrt(3) * N, these bars are more
than 1000 times tighter at every N.
"""

import numpy as np
import pytest

import ref64
from pointwise import EPS, pointwise as _pointwise, rms as _rms          # the error forms, shared with the literal mode's tests
from pointwise import BORDER, FP16_DISP_RMSE, FP16_NORMAL_RMSE, K_BAND, K_EDGE, K_MAP, K_NORMAL, K_ROW, STRUCT   # the bars, and the check of
from pointwise import check as _check                                    # one cascade: shared with tests/test_gpu_step_sequences.py

pytestmark = pytest.mark.gpu

DT = np.float32(1.0 / 60.0)

@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


def _state(oracle, N, rngseed, wavescale):
    p = oracle.EXAMPLE
    _, h0 = oracle.seed(N, rngseed, wavescale, p["waveamplitude"], p["windspeed"], p["winddirection"], sanitize=True)
    return h0


# every map form x every spectrum format: (N, map store policy, whether that policy streams)
FORMS = [(64, "auto", False), (128, "auto", False), (256, "auto", False), (512, "auto", False),
         (1024, "written through", False), (1024, "streamed", True), (2048, "written through", False), (2048, "streamed", True),
         (4096, "auto", True)]


@pytest.mark.parametrize("fmt", ["fp32", "fp16", "fp16h0"])
@pytest.mark.parametrize("N,policy,streamed", FORMS)
def test_pointwise_every_form(capi, oracle, report, N, policy, streamed, fmt):
    p = oracle.EXAMPLE
    wavescale, chop = p["wavescale"], p["choppiness"]
    h0 = _state(oracle, N, 1000 + N, wavescale)
    phase = np.zeros((N, N), np.float32)
    with capi.Ocean(N, 1) as oc:
        oc.set_spectrum_format(fmt)
        oc.set_map_store_policy(policy)
        assert oc.map_store_policy()[1] == streamed
        oc.set_cascade(0, wavescale, chop)
        oc.upload_state(0, h0)
        for _ in range(2):                       # the second displace overwrites every texel of the first (a skipped store shows)
            oc.update(DT)
            oc.displace()
            oracle.update(phase, wavescale, DT, mt=True)
        _check(capi, oracle, report, oc, 0, h0, wavescale, chop, fmt, f"N={N:4d} {fmt:6s} {policy}", phase)


@pytest.mark.parametrize("N,C,fmt,group,later", [(1024, 6, "fp16", 4, (3, 5)), (256, 5, "fp32", 2, (3, 4))])
def test_pointwise_later_cascade(capi, oracle, report, N, C, fmt, group, later):
    # multi-cascade handles launched in groups (4 + 2 and 2 + 2 + 1 cascades per launch), checked at later cascades and in the ragged last group
    p = oracle.EXAMPLE
    ws = [22.0 * 2.2 ** c for c in range(C)]
    h0 = [_state(oracle, N, 3000 + c, ws[c]) for c in range(C)]
    phases = [np.zeros((N, N), np.float32) for _ in range(C)]
    with capi.Ocean(N, C) as oc:
        oc.set_spectrum_format(fmt)
        oc.set_cascade_group(group)
        for c in range(C):
            oc.set_cascade(c, ws[c], p["choppiness"])
            oc.upload_state(c, h0[c])
        assert oc.cascade_group()[1] > 1                 # really more than one launch per pass
        for _ in range(2):
            oc.update(DT)
            oc.displace()
            for c in range(C):
                oracle.update(phases[c], ws[c], DT)
        for c in later:
            _check(capi, oracle, report, oc, c, h0[c], ws[c], p["choppiness"], fmt, f"N={N:4d} {fmt:6s} {C} cascades, group {group}, cascade {c}", phases[c])


def _edge_bins(capi, N):
    """single-bin cases: the corners, k = 0 (N/2, N/2) and its partner (N/2-1, N/2-1), the DC / Nyquist rows and columns, and waves
    whose sign flips every patch (and every band, where the maps are banded) of datum_ocean_map_layout"""
    PW, PH, B, _ = capi.map_layout(N)
    h = N // 2
    bins = [(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1), (h, h), (h - 1, h - 1), (0, h), (h, 0),
            (h + N // (2 * PH), h + N // (2 * PW))]
    if B < N:
        bins.append((h + 1, h + N // (2 * B)))
    return bins


@pytest.mark.parametrize("N", [64, 1024, 2048, 4096])
def test_known_answers_at_the_edges(capi, oracle, report, N):
    # one nonzero h0 bin per cascade of one handle, every channel against displace64
    wavescale, chop = 22.0, 1.35
    bins = _edge_bins(capi, N)
    amp = (0.3, -0.2)
    phases = [np.zeros((N, N), np.float32) for _ in bins]
    worst = [0.0, 0.0]
    every = []
    with capi.Ocean(N, len(bins)) as oc:
        for c, (y, x) in enumerate(bins):
            h0 = np.zeros((N, N, 2), np.float32)
            h0[y, x] = amp
            oc.set_cascade(c, wavescale, chop)
            oc.upload_state(c, h0)
        for _ in range(3):
            oc.update(DT)
            for ph in phases:
                oracle.update(ph, wavescale, DT)
        oc.displace()
        for c, (y, x) in enumerate(bins):
            h0 = np.zeros((N, N, 2), np.float32)
            h0[y, x] = amp
            assert np.array_equal(oc.read_state(c), phases[c])
            got = ref64.channels(oc.read_maps(c))
            ref, ln = ref64.displace64(h0, phases[c], np.float32(1) / np.float32(wavescale), chop, return_len=True)
            assert float(np.abs(ref[2]).max()) > 0.1, (y, x)
            kd, kn, _ = _pointwise(got, ref, ln, N, False)
            del got, ref, ln
            worst = [max(worst[0], kd), max(worst[1], kn)]
            every.append(((y, x), kd, kn))
    report(f"pointwise edges N={N:4d} ({len(bins)} single-bin cascades): disp K {worst[0]:.3g} (bar {K_EDGE:g}, margin {K_EDGE / worst[0]:.1f}x); "
           f"normal K {worst[1]:.3g} (bar {K_NORMAL:g}, margin {K_NORMAL / worst[1]:.1f}x)")
    for b, kd, kn in every:
        assert kd <= K_EDGE and kn <= K_NORMAL, (b, kd, kn)


@pytest.mark.parametrize("fmt", ["fp32", "fp16", "fp16h0"])
def test_debug_rowpass_refuses_a_cascade_without_state(capi, oracle, fmt):
    # datum_ocean_debug_rowpass, like datum_ocean_displace, refuses a cascade nobody uploaded (it used to run the row pass over unwritten
    # h0 and phase: in FP16_H0 a spurious "NaN or an infinity"); an uploaded cascade of the same handle still answers
    N = 64
    p = oracle.EXAMPLE
    with capi.Ocean(N, 2) as oc:
        oc.set_spectrum_format(fmt)
        oc.set_cascade(0, p["wavescale"], p["choppiness"])
        for c in (0, 1):
            with pytest.raises(capi.OceanError) as e:
                oc.debug_rowpass(c)
            assert e.value.code == capi.ESTATE, c
        oc.upload_state(0, _state(oracle, N, 1000, p["wavescale"]))
        c, d = oc.debug_rowpass(0)
        assert np.isfinite(c).all() and float(np.abs(c).max()) > 0
        with pytest.raises(capi.OceanError) as e:
            oc.debug_rowpass(1)
        assert e.value.code == capi.ESTATE
