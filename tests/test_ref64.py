"""The float64 reference of tests/ref64.py pinned against things that are not itself: a direct centred-k Fourier sum, its own
two-field packing (rowpass64 + colpass64 must give displace64 back), the golden fixtures and the CPU oracle.  CPU only."""

import os

import numpy as np
import pytest

import ref64

DT = np.float32(1.0 / 60.0)


def _state(oracle, N, rngseed, steps=3, wavescale=22.0):
    p = oracle.EXAMPLE
    _, h0 = oracle.seed(N, rngseed, wavescale, p["waveamplitude"], p["windspeed"], p["winddirection"], sanitize=True)
    phase = np.zeros((N, N), np.float32)
    for _ in range(steps):
        oracle.update(phase, wavescale, DT)
    return h0, phase, np.float32(1) / np.float32(wavescale)


@pytest.mark.parametrize("N", [16, 32])
def test_displace64_is_the_centred_fourier_sum(N):
    # dz(x, y) = Re sum_k h~(k) e^{i k . x} with k = 2 pi (m - N/2, n - N/2) / N -- no FFT, no (-1)^(x+y) trick
    rng = np.random.default_rng(N)
    h0 = rng.standard_normal((N, N, 2)).astype(np.float32)
    h0[N // 2, N // 2] = (0.7, -0.4)                                    # k = 0 with a nonzero h0
    phase = (rng.random((N, N)) * 6.28).astype(np.float32)
    scale, chop = np.float32(1 / 22.0), 1.35
    h, hx, hy = ref64.sim64(h0, phase, scale)
    got = ref64.displace64(h0, phase, scale, chop)
    kc = np.arange(N) - N // 2
    pos = np.arange(N)
    ex = np.exp(2j * np.pi * np.outer(kc, pos) / N)                     # [k][x]
    want = [(ex.T @ f @ ex).real for f in (hx, hy, h)]                  # [y][x] = sum_{ky,kx} f[ky][kx] e^{i(kx x + ky y)}
    want[0], want[1] = want[0] * chop, want[1] * chop
    dz = want[2]
    nx = np.roll(dz, 1, axis=1) - np.roll(dz, -1, axis=1)
    ny = np.roll(dz, -1, axis=0) - np.roll(dz, 1, axis=0)
    nz = float(np.float32(4) / (scale * np.float32(N)))
    ln = np.sqrt(nx * nx + ny * ny + nz * nz)
    want += [nx / ln, ny / ln, nz / ln]
    for ch in range(6):
        assert np.abs(got[ch] - want[ch]).max() <= 1e-12 * max(1.0, np.abs(want[ch]).max()), ch
    # the k = 0 guard: no slope at k = 0 (hx, hy vanish there), the partner's own
    assert hx[N // 2, N // 2] == 0 and hy[N // 2, N // 2] == 0
    assert h[N // 2, N // 2] != 0


@pytest.mark.parametrize("N", [64, 256])
def test_rowpass_then_colpass_is_displace64(oracle, N):
    # the packing identities of include/datum_ocean_hip.h (C = h_S + i hx_S, D = hy_S + 2 sin(2 pi x / N) h_S) and the column kernel's
    # map stage (halving, sign, nx = -Im(D) from the x slope carried by D) reproduce the plain three-field path exactly
    h0, phase, scale = _state(oracle, N, 1000 + N)
    want = ref64.displace64(h0, phase, scale, 1.35)
    c, d = ref64.rowpass64(h0, phase, scale)
    got = ref64.colpass64(c, d, scale, 1.35)
    for ch in range(6):
        assert np.abs(got[ch] - want[ch]).max() <= 1e-12 * max(1.0, np.abs(want[ch]).max()), ch
    # specinv is a plain factor on the input scale: the fp16 formats' power of two comes out again
    got2 = ref64.colpass64(c * 2.0 ** 7, d * 2.0 ** 7, scale, 1.35, specinv=2.0 ** -7)
    assert np.abs(got2 - got).max() <= 1e-12
    # and the fp32 [N][N][2] form debug_rowpass hands back is accepted as it is
    c32 = np.stack([c.real, c.imag], -1).astype(np.float32)
    d32 = np.stack([d.real, d.imag], -1).astype(np.float32)
    got3 = ref64.colpass64(c32, d32, scale, 1.35)
    assert np.abs(got3[:3] - got[:3]).max() < 1e-5 * np.abs(got[:3]).max()


def test_rowpass64_matches_the_oracle_row_transform(oracle):
    # rowpass64's packed fields are the fields tests/test_gpu_parity.py builds from the oracle's own ocean.sim (fp32) within fp32 noise
    N = 128
    h0, phase, scale = _state(oracle, N, 7)
    c, d = ref64.rowpass64(h0, phase, scale)
    fields = oracle.sim(h0, phase, scale)
    h, hx, hy = (ref64.as_complex(f) for f in fields)
    C, D = ref64.packed64(h, hx, hy)
    for want, F in ((c, C), (d, D)):
        got = np.fft.ifft(F, axis=1) * N
        assert np.abs(got - want).max() < 1e-6 * np.abs(want).max()


def test_displace64_on_the_golden_inputs():
    # tests/golden/ocean_n64.npz: the reference's h0 and the phases after 1 / 60 / 600 steps, the maps of the reference's arithmetic (fp32)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ocean_n64.npz"))
    scale = np.float32(1) / np.float32(22.0)
    for steps in (1, 60, 600):
        want = ref64.channels(g[f"maps_{steps}"].astype(np.float64))
        got = ref64.displace64(g["h0"], g[f"phase_{steps}"], scale, 1.35)
        for ch in range(6):
            # the fixtures carry the literal twiddle table's fp32 error: measured RMSE <= 1.8e-6, max 6.9e-6
            d = got[ch] - want[ch]
            assert np.sqrt((d * d).mean()) < 4e-6, (steps, ch)
            assert np.abs(d).max() < 2e-5, (steps, ch)


@pytest.mark.parametrize("N", [64, 256, 512])
def test_displace64_against_the_oracle(oracle, N):
    h0, phase, scale = _state(oracle, N, 2000 + N)
    want = ref64.channels(oracle.displace(h0, phase.copy(), 22.0, 1.35, w=oracle.weights(N, reduced=True)).astype(np.float64))
    got, ln = ref64.displace64(h0, phase, scale, 1.35, return_len=True)
    for ch in range(6):
        d = got[ch] - want[ch]
        assert np.sqrt((d * d).mean()) < 1e-6, ch
        assert np.abs(d).max() < 1e-5 * max(1.0, 1.0 / float(ln.min())), ch


def test_fp16_scales_follow_size_spectrum_scale():
    # the rule of ocean_capi.hip (size_spectrum_scale): 12 N sqrt(2) m 2^e < 60000 <= 2 * that, and m 2^eh just under 2^15
    rng = np.random.default_rng(3)
    for N in (64, 4096):
        for m in (1e-21, 3.7e-3, 0.11, 1.0, 4.0e8):
            h0 = (rng.standard_normal((8, 8, 2)) * m).astype(np.float32)
            e, eh = ref64.fp16_scales(h0, N)
            a = float(np.abs(h0).max())
            b = 12.0 * N * 1.41421356 * a
            assert b * 2.0 ** e <= 60000.0 < b * 2.0 ** (e + 1)
            assert 16384.0 <= a * 2.0 ** eh < 32768.0
            halves = ref64.h0_as_halves(h0, eh)
            assert np.array_equal((halves * np.float32(2.0 ** eh)).astype(np.float16).astype(np.float32), halves * np.float32(2.0 ** eh))
