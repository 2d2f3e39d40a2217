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

pytestmark = pytest.mark.gpu

DT = np.float32(1.0 / 60.0)

# Bars: at least 3x the worst value measured on the MI355X over every case of this file (the measured worst beside each).
K_MAP = 9.0             # random fields, every form, format and N, end to end (fp32) and column pass: measured 2.89 (512^2 fp32, e2e)
K_EDGE = 30.0           # single-bin known answers (a pure tone: the twiddles' errors add coherently): measured 9.73 (4096^2)
K_NORMAL = 6.0          # every case, the single bins included: measured 1.94 (4096^2)
K_ROW = 24.0            # fp32 row pass: measured 7.63 (4096^2); grows faster than L because a row's small elements carry the sim's error
K_BAND = 18.0           # fp16 formats, the band around a rounding midpoint: measured 5.59 (4096^2 fp16h0; 1e-4 .. 4e-3 of the halves are not the nearest)
STRUCT = 7.5            # worst column / row RMS of the normalised error over the median one: measured 2.42 (4096^2 column pass, rows)
BORDER = 4.0            # RMS of the error on the grid's border ring over the interior's: measured 1.22 (1024^2 column pass)
FP16_DISP_RMSE = 3.5e-4  # fp16 formats, end to end: displacement RMSE / max |displacement|: measured 1.11e-4 (128^2 fp16h0)
FP16_NORMAL_RMSE = 2e-3  # fp16 formats, end to end: normal RMSE (absolute): measured 6.17e-4 (4096^2 fp16)


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


def _state(oracle, N, rngseed, wavescale):
    p = oracle.EXAMPLE
    _, h0 = oracle.seed(N, rngseed, wavescale, p["waveamplitude"], p["windspeed"], p["winddirection"], sanitize=True)
    return h0


def _structure(energy):
    """(worst column / median column, worst row / median row, border ring / interior) of the RMS of the normalised error"""
    cols = np.sqrt(energy.mean(axis=0))
    rows = np.sqrt(energy.mean(axis=1))
    ring = np.concatenate([energy[0], energy[-1], energy[1:-1, 0], energy[1:-1, -1]])
    inner = float(np.sqrt(energy[1:-1, 1:-1].mean()))
    return float(cols.max() / np.median(cols)), float(rows.max() / np.median(rows)), float(np.sqrt(ring.mean()) / inner)


def _rowpass_fp32(got, want, N):
    """worst |got - want| per element over eps * L * rms(row)"""
    g = ref64.as_complex(got)
    rows = np.sqrt(np.mean(np.abs(want) ** 2, axis=1, keepdims=True))
    return float((np.abs(g - want) / (EPS * np.log2(N) * np.maximum(rows, 1e-37))).max())


def _rowpass_fp16(got, want, N, e):
    """(halves: every value times 2^e is one, K: the smallest band k * eps * L * rms(row) around the float64 value within which the
    kernel's fp32 value must lie for its half to be what it is, share of values that are not the half nearest the float64 value).
    A stored half h is RN(v) of the kernel's fp32 value v; |v - ref| <= band means RN(ref - band) <= h <= RN(ref + band): it is the
    nearest half unless ref lies within the band of a rounding midpoint (of several, where the band spans more than a half's spacing,
    as it does for the small values of a row).  Both components of each element are checked on their own."""
    unit = EPS * np.log2(N) * np.sqrt(np.mean(np.abs(want) ** 2, axis=1, keepdims=True)) * np.ldexp(1.0, e)
    halves = True
    need = 0.0
    off = 0
    for g, w in ((got[..., 0], want.real), (got[..., 1], want.imag)):
        g = g.astype(np.float64) * np.ldexp(1.0, e)                 # exact: a power of two
        w = w * np.ldexp(1.0, e)
        g16 = g.astype(np.float16)
        halves = halves and bool(np.array_equal(g16.astype(np.float64), g))
        rn = w.astype(np.float16)                                   # round to nearest even from float64
        miss = g16 != rn
        off += int(miss.sum())
        if miss.any():
            gm, wm = g16[miss], w[miss]
            um = np.broadcast_to(unit, w.shape)[miss]
            up = gm > rn[miss]
            below = (gm.astype(np.float64) + np.nextafter(gm, np.float16(-np.inf)).astype(np.float64)) / 2   # midpoints next to the half
            above = (gm.astype(np.float64) + np.nextafter(gm, np.float16(np.inf)).astype(np.float64)) / 2
            k = np.where(up, below - wm, wm - above) / um
            need = max(need, float(k.max()))
    return halves, need, off / got.size


def _check(capi, oracle, report, oc, c, h0, wavescale, chop, fmt, label, want_phase):
    """the three comparisons (and the structure check from 1024^2 up) for cascade c of a handle that has just displaced"""
    N = h0.shape[0]
    scale = np.float32(1) / np.float32(wavescale)
    maps = oc.read_maps(c)
    phase = oc.read_state(c)
    assert np.array_equal(phase, want_phase), label
    assert np.all(maps[..., 3] == 0) and np.isfinite(maps).all(), label
    got = ref64.channels(maps)
    del maps
    rp = oc.debug_rowpass(c)
    again = oc.debug_rowpass(c)
    same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(rp, again))
    del again
    checks = []                    # (what, measured, bar): measured <= bar
    structure = N >= 1024
    energies = []

    # 1. end to end
    ref, ln = ref64.displace64(h0, phase, scale, chop, return_len=True)
    if fmt == "fp32":
        kd, kn, en = _pointwise(got, ref, ln, N, structure)
        checks += [("e2e disp K", kd, K_MAP), ("e2e normal K", kn, K_NORMAL)]
        if structure:
            energies.append(("e2e", en))
    else:
        big = float(np.abs(ref[:3]).max())
        ed = _rms(got[:3] - ref[:3]) / big
        en_ = _rms(got[3:] - ref[3:])
        checks += [("e2e fp16 disp rmse/max", ed, FP16_DISP_RMSE), ("e2e fp16 normal rmse", en_, FP16_NORMAL_RMSE)]
        assert ed > 1e-7, label                                     # really went through halves
    del ref, ln

    # 2. row pass
    if fmt == "fp32":
        c64, d64 = ref64.rowpass64(h0, phase, scale)
        kr = max(_rowpass_fp32(rp[0], c64, N), _rowpass_fp32(rp[1], d64, N))
        checks += [("row K", kr, K_ROW)]
        off = None
    else:
        e, eh = ref64.fp16_scales(h0, N)
        c64, d64 = ref64.rowpass64(ref64.h0_as_halves(h0, eh) if fmt == "fp16h0" else h0, phase, scale)
        hc, kc, oc_ = _rowpass_fp16(rp[0], c64, N, e)
        hd, kd_, od = _rowpass_fp16(rp[1], d64, N, e)
        assert hc and hd, (label, "a row-pass value times 2^e is not a half")
        checks += [("row midpoint band K", max(kc, kd_), K_BAND)]
        off = (oc_ + od) / 2
    del c64, d64

    # 3. column pass from the GPU's own row-pass output
    ref, ln = ref64.colpass64(rp[0], rp[1], scale, chop, return_len=True)
    del rp
    kd, kn, en = _pointwise(got, ref, ln, N, structure)
    checks += [("col disp K", kd, K_MAP), ("col normal K", kn, K_NORMAL)]
    if structure:
        energies.append(("col", en))
    del ref, ln, got

    # 4. structure
    for what, en in energies:
        cr, rr, br = _structure(en)
        checks += [(f"{what} worst col/median", cr, STRUCT), (f"{what} worst row/median", rr, STRUCT), (f"{what} border/interior", br, BORDER)]
    del energies

    text = "; ".join(f"{w} {m:.3g} (bar {b:g}, margin {b / m if m > 0 else float('inf'):.1f}x)" for w, m, b in checks)
    extra = f"; halves not the nearest {off:.2e}" if off is not None else ""
    report(f"pointwise {label}: {text}{extra}")
    assert same, (label, "two debug_rowpass calls differ")
    for w, m, b in checks:
        assert m <= b, (label, w, m, b)


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
