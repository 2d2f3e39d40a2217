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
