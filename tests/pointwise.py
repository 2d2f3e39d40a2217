"""What the pointwise tests share: the error forms of tests/test_gpu_pointwise.py (one copy, used by that file, by
tests/test_lit64.py on the CPU and by tests/test_gpu_literal_pointwise.py on the GPU), and the bars and cases of the literal
transform mode.  Not a test module; pure numpy.

Error forms, with eps = 2^-24 and L = log2 N:
  displacement channel ch   |got - ref| / (eps * L * s_ch),  s_ch = max(rms(ch), rms(dx, dy, dz) / 4)
  normal channels           |got - ref| / (eps * (L * (r_n + s_dz) / len + 1)),  len = |(nx, ny, nz)| of the reference before
                            normalisation at that point, r_n the RMS of its slopes
`pointwise` returns the worst of each over every texel: the smallest constant K that would pass.
"""

import numpy as np

import ref64

EPS = 2.0 ** -24
DT = np.float32(1.0 / 60.0)


def rms(a):
    return float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))


def pointwise(got, ref, ln, N, structure=False):
    """(K of the displacement channels, K of the normal channels, normalised error energy per point or None): K is the worst
    |got - ref| over the bar's scale, i.e. the smallest K_MAP / K_NORMAL that passes"""
    L = np.log2(N)
    s = [rms(ref[ch]) for ch in range(3)]
    sall = float(np.sqrt(np.mean(np.square(s))))
    s = [max(v, 0.25 * sall, 1e-30) for v in s]
    energy = np.zeros((N, N)) if structure else None
    kd = 0.0
    for ch in range(3):
        e = np.abs(got[ch] - ref[ch]) / (EPS * L * s[ch])
        kd = max(kd, float(e.max()))
        if structure:
            energy += e * e
    rn = float(np.sqrt(np.mean(np.square(ref[3] * ln) + np.square(ref[4] * ln)) / 2))
    den = EPS * (L * (rn + s[2]) / ln + 1.0)
    kn = 0.0
    for ch in range(3, 6):
        e = np.abs(got[ch] - ref[ch]) / den
        kn = max(kn, float(e.max()))
        if structure:
            energy += e * e
    return kd, kn, energy


def disp_scales(ref):
    """s_ch of the three displacement channels, as `pointwise` forms them"""
    s = [rms(ref[ch]) for ch in range(3)]
    sall = float(np.sqrt(np.mean(np.square(s))))
    return [max(v, 0.25 * sall, 1e-30) for v in s]


# -- the literal transform mode (datum_ocean_set_literal_transform, ocean_literal.hip) ------------------------------------------------
#
# Reference: ref64.lit64, the reference's algorithm in float64 on the fp32 twiddle table the module serves.  The bars are NOT taken from
# the GPU: K_REF_* is the worst error of the reference's own fp32 arithmetic on the CPU (oracle.displace with oracle.weights(N)) against
# lit64 on the inputs below, measured by tests/test_lit64.py (which asserts that it stays so), and every bar is 3 x that -- the device's
# sinf / cosf and the compiler's FMA contraction differ from the host's libm and uncontracted arithmetic by a few ulps per operation;
# 3 x is the factor every other bar of this suite carries.
#
# Measured on the CPU (tests/test_lit64.py::test_the_oracle_sets_the_bar reports them), disp K / normal K:
#   one cascade, example parameters, seed 1000 + N, three updates     N = 64: 2.235 / 0.896    256: 1.733 / 1.355    1024: 1.765 / 2.170
#   the cascade case (256^2; wave scales 22, 64, 176; seeds 500 + c)  2.081 / 1.934    2.040 / 1.829    2.088 / 0.881
#   single bins (five bins, phase zero and one update), worst         N = 64: 1.607 / 0.844    1024: 1.623 / 1.464
K_REF_DISP = 2.24           # the worst of the three sizes (64^2), rounded up
K_REF_NORMAL = 2.17         # the worst of the three sizes (1024^2); the cascade case and the single bins stay below both
K_REF_EDGE = 1.63           # displacement channels of the single bins (a pure tone: the table's errors add coherently), 1024^2 bin (N/2, N/2+1)
K_LIT_DISP = 3 * K_REF_DISP             # 6.72
K_LIT_NORMAL = 3 * K_REF_NORMAL         # 6.51; the single bins' normals are held to it too
K_LIT_EDGE = 3 * K_REF_EDGE             # 4.89

LIT_SIZES = (64, 256, 1024)             # against lit64: fewer lanes than threads, one lane per thread, four lanes per thread
LIT_LARGE = (2048, 4096)                # against the fp32 oracle, 2 x the bar (float64 radix-2 stages cost minutes of numpy there)
LIT_STEPS = 3
LIT_CASCADES = (256, (22.0, 64.0, 176.0))
LIT_EDGE_SIZES = (64, 1024)
LIT_EDGE_AMP = (0.3, -0.2)
LIT_EDGE_STEPS = (0, 1)                 # phase zero, and after one update


def lit_state(oracle, N, wavescale=None, rngseed=None):
    """h0 of the literal-mode cases: the example parameters, seed 1000 + N unless given"""
    p = oracle.EXAMPLE
    ws = p["wavescale"] if wavescale is None else wavescale
    _, h0 = oracle.seed(N, 1000 + N if rngseed is None else rngseed, ws, p["waveamplitude"], p["windspeed"], p["winddirection"], sanitize=True)
    return h0


def lit_phase(oracle, N, wavescale, steps):
    """the phase after `steps` updates by DT from zero, as oracle.update advances it"""
    phase = np.zeros((N, N), np.float32)
    for _ in range(steps):
        oracle.update(phase, wavescale, DT, mt=N >= 1024)
    return phase


def lit_cascade_states(oracle):
    """[(wavescale, h0)] of the cascade case: one handle, three cascades with scales of their own"""
    N, scales = LIT_CASCADES
    return [(ws, lit_state(oracle, N, ws, 500 + c)) for c, ws in enumerate(scales)]


def lit_edge_bins(N):
    """single-bin inputs: (0, 0) and (N-1, N-1) are each other's mirror at k = -N/2; (N/2, N/2) is k = 0 (no direction: hx = hy = 0
    there); (N/2, N/2+1) and (0, N/2) put the energy on a single row / column of the transforms"""
    h = N // 2
    return [(0, 0), (N - 1, N - 1), (h, h), (h, h + 1), (0, h)]


def lit_edge_h0(N, b):
    h0 = np.zeros((N, N, 2), np.float32)
    h0[b] = LIT_EDGE_AMP
    return h0


# -- the fused step's bars and the check of one cascade (tests/test_gpu_pointwise.py, where the bars are explained; shared with
# tests/test_gpu_step_sequences.py) ---------------------------------------------------------------------------------------------------

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


def check(capi, oracle, report, oc, c, h0, wavescale, chop, fmt, label, want_phase):
    """the three comparisons (and the structure check from 1024^2 up) for cascade c of a handle that has just displaced"""
    maps = oc.read_maps(c)
    phase = oc.read_state(c)
    assert np.array_equal(phase, want_phase), label
    rp = oc.debug_rowpass(c)
    again = oc.debug_rowpass(c)
    same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(rp, again))
    del again
    return compare(report, maps, phase, rp, same, h0, wavescale, chop, fmt, label)


def compare(report, maps, phase, rp, same, h0, wavescale, chop, fmt, label, scales=None):
    """`check` from what it read: the maps, the phase they were formed from, debug_rowpass's pair and whether a second call gave the same
    bits.  scales: the fp16 exponents (e, eh) the handle should be using (default: ref64.fp16_scales of this h0).  Returns the checks"""
    N = h0.shape[0]
    scale = np.float32(1) / np.float32(wavescale)
    assert np.all(maps[..., 3] == 0) and np.isfinite(maps).all(), label
    got = ref64.channels(maps)
    del maps
    checks = []                    # (what, measured, bar): measured <= bar
    structure = N >= 1024
    energies = []

    # 1. end to end
    ref, ln = ref64.displace64(h0, phase, scale, chop, return_len=True)
    if fmt == "fp32":
        kd, kn, en = pointwise(got, ref, ln, N, structure)
        checks += [("e2e disp K", kd, K_MAP), ("e2e normal K", kn, K_NORMAL)]
        if structure:
            energies.append(("e2e", en))
    else:
        big = float(np.abs(ref[:3]).max())
        ed = rms(got[:3] - ref[:3]) / big
        en_ = rms(got[3:] - ref[3:])
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
        e, eh = ref64.fp16_scales(h0, N) if scales is None else scales
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
    kd, kn, en = pointwise(got, ref, ln, N, structure)
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
    return checks


