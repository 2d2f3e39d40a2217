"""Float64 restatement of the displacement path, written from the operations (data/ocean.{sim,fftx,ffty,map}.comp as
oracle/ocean_oracle.cpp restates them, and the two-field packing of include/datum_ocean_hip.h), not by calling the oracle.

  sim64       ocean.sim from the fp32 inputs: partner h0 at (N-1-y, N-1-x) with only the bin's own phase, k = 0 guarded
  displace64  the exact 2-D inverse transform of sim64's three fields, (-1)^(x+y), ocean.map's six channels
  lit64       the same channels through the reference's LITERAL algorithm (log2 N radix-2 Stockham stages per line, twiddles read
              from a table handed in): what datum_ocean_set_literal_transform runs (ocean_literal.hip), in float64
  rowpass64   the packed fields C, D (datum_ocean_debug_rowpass) and their exact row transform
  colpass64   from any row-pass output (the GPU's own included): the exact column transform and the column kernel's map stage
  fp16_scales the power-of-two exponents the fp16 formats pick from max |h0| (ocean_capi.hip: size_spectrum_scale)

A transform is out[n] = sum_k in[k] e^{+2 pi i k n / N} (the reference's Stockham lines conjugate in and out), i.e. N * ifft.
Channels come back as one float64 array [6][N][N] in the order dx, dy, dz, nx, ny, nz: maps[0][..., :3] then maps[1][..., :3].
At 4096^2 a complex128 plane is 256 MB: the fields are built and transformed one at a time and freed as soon as they are used.
"""

import numpy as np

TWO_PI = 2 * np.pi


def _k(N, scale):
    """centred wave vector components (sim.comp:48) in float64 from the fp32 scale = 1 / wavescale"""
    k = TWO_PI * (np.arange(N, dtype=np.float64) - 0.5 * N) * float(scale)
    return k[None, :], k[:, None]


def _unit_k(N, scale):
    kx, ky = _k(N, scale)
    ln = np.hypot(kx, ky)
    ln[N // 2, N // 2] = 1.0                     # the k = 0 guard: k^ = 0 there (kx = ky = 0)
    return kx / ln, ky / ln


def sim64(h0, phase, scale):
    """ocean.sim in float64: (h, hx, hy) complex128 [N][N] from h0 [N][N][2] and phase [N][N] (fp32 arrays)."""
    N = phase.shape[0]
    a = h0[..., 0].astype(np.float64) + 1j * h0[..., 1].astype(np.float64)
    m = a[::-1, ::-1]                            # the partner bin (N-1-y, N-1-x), sim.comp:59
    ph = phase.astype(np.float64)
    c, s = np.cos(ph), np.sin(ph)
    hre = (a.real + m.real) * c - (a.imag + m.imag) * s
    him = (a.real - m.real) * s + (a.imag - m.imag) * c
    h = hre + 1j * him
    del a, m, ph, c, s, hre, him
    knx, kny = _unit_k(N, scale)
    hx = -1j * knx * h                           # (him, -hre) * knx
    hy = -1j * kny * h
    return h, hx, hy


def _sign(N):
    i = np.arange(N)
    return np.where((i[:, None] + i[None, :]) & 1, -1.0, 1.0)


def _nz(N, scale):
    """nz = 4 / (scale * N), the fp32 constant both ocean.map and the column kernel use (map.comp:77)"""
    return float(np.float32(4) / (np.float32(scale) * np.float32(N)))


def _normals(out, nx, ny, nz):
    ln = np.sqrt(nx * nx + ny * ny + nz * nz)
    out[3] = nx / ln
    out[4] = ny / ln
    out[5] = nz / ln
    return ln


def transform2(f):
    """exact 2-D transform: N^2 ifft2 (complex128)"""
    N = f.shape[0]
    return np.fft.ifft2(f) * (N * N)


def displace64(h0, phase, scale, chop, return_len=False):
    """ocean.sim + ocean.fftx + ocean.ffty + ocean.map in float64: [6][N][N] (dx, dy, dz, nx, ny, nz).
    The normals are the map stage's central differences of dz with wrap-around, nz = 4 / (scale N).
    return_len: also the float64 length |(nx, ny, nz)| before normalisation [N][N]."""
    N = phase.shape[0]
    sg = _sign(N)
    out = np.empty((6, N, N), np.float64)
    h, hx, hy = sim64(h0, phase, scale)
    out[2] = transform2(h).real * sg
    del h
    out[0] = transform2(hx).real * sg * float(chop)
    del hx
    out[1] = transform2(hy).real * sg * float(chop)
    del hy, sg
    ln = _map_normals(out, scale)
    return (out, ln) if return_len else out


def _map_normals(out, scale):
    """ocean.map's normal from out[2] = dz into out[3:6]: central differences with wrap-around, nz = 4 / (scale N) (map.comp:58-78);
    returns the length before normalisation"""
    dz = out[2]
    nx = np.roll(dz, 1, axis=1) - np.roll(dz, -1, axis=1)      # dz(x-1) - dz(x+1)
    ny = np.roll(dz, -1, axis=0) - np.roll(dz, 1, axis=0)      # dz(y+1) - dz(y-1)
    return _normals(out, nx, ny, _nz(dz.shape[0], scale))


def normal_len(dz, scale):
    """|(nx, ny, nz)| before normalisation [N][N] in float64, from any dz [N][N] (ocean.map's differences, as displace64's return_len)"""
    dz = np.asarray(dz, np.float64)
    nx = np.roll(dz, 1, axis=1) - np.roll(dz, -1, axis=1)
    ny = np.roll(dz, -1, axis=0) - np.roll(dz, 1, axis=0)
    nz = _nz(dz.shape[0], scale)
    return np.sqrt(nx * nx + ny * ny + nz * nz)


def twiddles64(N):
    """the table of ocean.cpp:686-700 in its layout [N][2 log2 N] (cos, sin per stage s of lane i), evaluated accurately: the angle
    -2 pi i / 2^(s+1) with the lane index reduced modulo the stage's period 2^(s+1) first, in float64"""
    stages = N.bit_length() - 1
    i = np.arange(N)
    w = np.empty((N, 2 * stages), np.float64)
    for s in range(stages):
        period = 2 << s
        a = -TWO_PI * (i % period) / period
        w[:, 2 * s] = np.cos(a)
        w[:, 2 * s + 1] = np.sin(a)
    return w


def stockham64(f, w, axis):
    """one dispatch of ocean.fftx (axis = 1: every row) or ocean.ffty (axis = 0: every column) on a complex128 plane [N][N]:
    conjugate, log2 N stages dst[i] = src[i0] + (t0 + i t1) src[i0 + N/2] with i0 = (i / n) (n / 2) + i % (n / 2), n = 2, 4 .. N
    and (t0, t1) = w[i][2 s], w[i][2 s + 1] -- the twiddle of the FULL lane index i --, conjugate (fftx.comp:55-99).
    One gather per stage over the whole plane; w is used value for value (float64)."""
    N = f.shape[0]
    stages = N.bit_length() - 1
    assert 1 << stages == N and w.shape == (N, 2 * stages)
    i = np.arange(N)
    src = np.conj(f if axis == 1 else f.T)
    for s in range(stages):
        n = 2 << s
        i0 = (i // n) * (n // 2) + i % (n // 2)
        t = w[:, 2 * s] + 1j * w[:, 2 * s + 1]
        src = src[:, i0] + t[None, :] * src[:, i0 + N // 2]
    src = np.conj(src)
    return src if axis == 1 else np.ascontiguousarray(src.T)


def lit64(h0, phase, scale, chop, w, return_len=False):
    """The literal transform mode in float64: ocean.sim (sim64), for each of the three planes ocean.fftx then ocean.ffty as radix-2
    Stockham stages reading the table w [N][2 log2 N] (the fp32 table the module serves, datum_ocean_reference_weights, converted value
    for value; or any other), then ocean.map: (-1)^(x+y), choppiness on dx and dy, the central-difference normal with wrap-around and
    nz = 4 / (scale N).  [6][N][N] (dx, dy, dz, nx, ny, nz) like displace64; it is not an FFT and inherits the table's error."""
    N = phase.shape[0]
    w = np.asarray(w, np.float64)
    sg = _sign(N)
    out = np.empty((6, N, N), np.float64)
    h, hx, hy = sim64(h0, phase, scale)
    out[2] = stockham64(stockham64(h, w, 1), w, 0).real * sg
    del h
    out[0] = stockham64(stockham64(hx, w, 1), w, 0).real * sg * float(chop)
    del hx
    out[1] = stockham64(stockham64(hy, w, 1), w, 0).real * sg * float(chop)
    del hy, sg
    ln = _map_normals(out, scale)
    return (out, ln) if return_len else out


def packed64(h, hx, hy):
    """the two fields the module transforms (include/datum_ocean_hip.h, datum_ocean_debug_rowpass): with F_S = F + conj(F[-y][-x]),
    C = h_S + i hx_S and D = hy_S + 2 sin(2 pi x / N) h_S (complex128)"""
    N = h.shape[0]
    idx = (-np.arange(N)) % N

    def herm(f):
        return f + np.conj(f[idx][:, idx])

    hs = herm(h)
    C = hs + 1j * herm(hx)
    D = herm(hy) + (2 * np.sin(TWO_PI * np.arange(N) / N))[None, :] * hs
    return C, D


def rowpass64(h0, phase, scale):
    """(c, d) complex128 [N][N]: the row transform of the packed fields built from sim64 -- what datum_ocean_debug_rowpass returns"""
    N = phase.shape[0]
    h, hx, hy = sim64(h0, phase, scale)
    C, D = packed64(h, hx, hy)
    del h, hx, hy
    c = np.fft.ifft(C, axis=1) * N
    del C
    d = np.fft.ifft(D, axis=1) * N
    return c, d


def as_complex(a):
    """[N][N][2] float array -> complex128"""
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def colpass64(c, d, scale, chop, specinv=1.0, return_len=False):
    """The column kernel's work in float64 from a row-pass output (complex128, or [N][N][2] floats such as datum_ocean_debug_rowpass's):
    exact column transforms Fc, Fd, then the map stage as the kernel forms it (ocean_kernels.hip, column pass):
      sig = (-1)^(x+y) / 2 * specinv,  dz = Re Fc sig,  dx = Im Fc sig chop,  dy = Re Fd sig chop,
      nx = -Im Fd sig (the x slope carried by D, not a difference of dz),  ny = dz(y+1) - dz(y-1),  nz = 4 / (scale N)."""
    if np.isrealobj(c):
        c = as_complex(c)
    if np.isrealobj(d):
        d = as_complex(d)
    N = c.shape[0]
    sig = _sign(N) * (0.5 * float(specinv))
    out = np.empty((6, N, N), np.float64)
    f = np.fft.ifft(c, axis=0) * N
    out[2] = f.real * sig
    out[0] = f.imag * sig * float(chop)
    f = np.fft.ifft(d, axis=0) * N
    out[1] = f.real * sig * float(chop)
    nx = -f.imag * sig
    del f, sig
    dz = out[2]
    ny = np.roll(dz, -1, axis=0) - np.roll(dz, 1, axis=0)
    ln = _normals(out, nx, ny, _nz(N, scale))
    return (out, ln) if return_len else out


def fp16_scales(h0, N):
    """(e, eh): the fp16 work spectrum is stored as halves of value * 2^e, FP16_H0 reads h0 as halves of h0 * 2^eh -- the exponents
    ocean_capi.hip's size_spectrum_scale picks from m = max |component of h0|"""
    m = float(np.abs(h0).max())
    bound = 12.0 * N * (1.41421356 * m)
    e = int(np.floor(np.log2(60000.0 / bound))) if bound > 0 else 0
    e = max(-100, min(100, e))
    eh = int(np.floor(np.log2(32768.0 / m))) if m > 0 else 0
    if m > 0 and np.ldexp(m, eh) >= 32768.0:
        eh -= 1
    eh = max(-120, min(120, eh))
    return e, eh


def h0_as_halves(h0, eh):
    """h0 as FP16_H0 holds it: h0 * 2^eh rounded to the nearest half (ties to even), times 2^-eh (fp32 holds it exactly)"""
    s = np.float32(np.ldexp(1.0, eh))
    return (((h0 * s).astype(np.float16)).astype(np.float32) / s).astype(np.float32)


def channels(maps):
    """a cascade's maps [2][N][N][4] (datum_ocean_read_maps) as [6][N][N] in displace64's channel order"""
    return np.concatenate([np.moveaxis(maps[0, ..., :3], -1, 0), np.moveaxis(maps[1, ..., :3], -1, 0)])
