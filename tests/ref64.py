"""Float64 restatement of the displacement path, written from the operations (data/ocean.{sim,fftx,ffty,map}.comp as
oracle/ocean_oracle.cpp restates them, and the two-field packing of include/datum_ocean_hip.h), not by calling the oracle.

  sim64       ocean.sim from the fp32 inputs: partner h0 at (N-1-y, N-1-x) with only the bin's own phase, k = 0 guarded
  displace64  the exact 2-D inverse transform of sim64's three fields, (-1)^(x+y), ocean.map's six channels
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
    dz = out[2]
    nx = np.roll(dz, 1, axis=1) - np.roll(dz, -1, axis=1)      # dz(x-1) - dz(x+1)
    ny = np.roll(dz, -1, axis=0) - np.roll(dz, 1, axis=0)      # dz(y+1) - dz(y-1)
    ln = _normals(out, nx, ny, _nz(N, scale))
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
