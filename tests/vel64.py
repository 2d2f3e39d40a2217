"""References of the surface velocity (include/datum_ocean_hip.h, "surface velocity"), beside ref64.sim64 / displace64.  Pure numpy.

  omega32    the handle's dispersion table in its own fp32 arithmetic (ocean_kernels.hip: dispersion_at), [N][N]
  single_bin64  one nonzero bin in closed form: two plane waves, amplitude omega |h|, a quarter period ahead of the displacement
  vel64      the definition in float64: [3][N][N] (vx, vy, vz) = d/dt of displace64's (dx, dy, dz) at a fixed texel
  spectrum32 the definition's spectrum in fp32, operation for operation as datum_amd/csrc/ocean_velocity.h states it
  vel32      the fp32 restatement: spectrum32, the oracle's radix-2 transforms (oracle.fftx / ffty), sigma and the choppiness
  sample32   the query's velocity sample over planes in fp32 (ocean_query.hip: query_velocity), FMAs rounded once

`mistake` plants the errors tests/test_vel64.py's sensitivity test names: "mirror" (the mirror term's sign), "omega" (omega taken at
the mirrored index), "chop" (choppiness left off vx, vy).

The bar.  K_VEL = 3 x the worst error of vel32 against vel64 at 64^2, 256^2 and 1024^2 (example parameters, seed 1000 + N, three
updates), in pointwise.pointwise's units (eps log2 N relative to the channel's RMS, disp_scales) -- CPU arithmetic only, as K_LIT was
made; tests/test_vel64.py::test_the_restatement_sets_the_bar measures it again and asserts that it stays so.
Measured:  N = 64: 7.21    256: 8.22    1024: 10.53   (the spectrum is weighted by omega: the fine bins, whose phase has gone round most
often and whose products carry the largest roundings, dominate the velocity where they hardly show in the displacement)
"""

import numpy as np

import pointwise as pw
import ref64

K_REF_VEL = 10.53           # the worst of the three sizes (1024^2)
K_VEL = 3 * K_REF_VEL       # 31.59

VEL_SIZES = (64, 256, 1024)
VEL_STEPS = 3

F = np.float32
TWO_PI = 2 * np.pi


def omega32(N, wavescale):
    """dispersion(k) as update_ocean forms it (ocean.cpp:225-233) in fp32, [N][N] by (row y, column x)"""
    i = np.arange(N, dtype=np.float32)
    k = (F(6.2831855) * (i - F(0.5) * F(N))) / F(wavescale)
    k2 = (k * k)[None, :] + (k * k)[:, None]
    return np.sqrt((F(9.81) * np.sqrt(k2)) * (F(1.0) + k2 / F(136900.0))).astype(np.float32)


def vel64(h0, phase, scale, chop, omega=None, mistake=None):
    """[3][N][N] float64 (vx, vy, vz).  omega: the fp32 table [N][N] (default: omega32 at wavescale = 1 / scale in fp32)"""
    N = phase.shape[0]
    if omega is None:
        omega = omega32(N, F(1) / F(scale))
    om = np.asarray(omega, np.float64)
    if mistake == "omega":
        om = om[::-1, ::-1]
    a = h0[..., 0].astype(np.float64) + 1j * h0[..., 1].astype(np.float64)
    m = a[::-1, ::-1]
    if mistake == "mirror":
        m = -m
    ph = phase.astype(np.float64)
    c, s = np.cos(ph), np.sin(ph)
    re = om * (-(a.real + m.real) * s - (a.imag + m.imag) * c)
    im = om * ((a.real - m.real) * c - (a.imag - m.imag) * s)
    ht = re + 1j * im
    knx, kny = ref64._unit_k(N, scale)
    sg = ref64._sign(N)
    ch = 1.0 if mistake == "chop" else float(chop)
    out = np.empty((3, N, N), np.float64)
    out[2] = ref64.transform2(ht).real * sg
    out[0] = ref64.transform2(-1j * knx * ht).real * sg * ch
    out[1] = ref64.transform2(-1j * kny * ht).real * sg * ch
    return out


def single_bin64(N, b, a, phase, scale, chop, omega):
    """One nonzero bin h0[b] = a (b = (row, column)) in closed form, [3][N][N] float64.  ocean.sim puts a e^{i phase[b]} at b and, at the
    mirror texel M = (N-1-row, N-1-column), conj(a) e^{-i phase[M]}: two plane waves, each moving with the omega of ITS texel.  With
    psi_b = 2 pi (b . x) / N + phase[b] + arg a and psi_M = 2 pi (M . x) / N - phase[M] - arg a:
        dz = sigma |a| (cos psi_b + cos psi_M)                    vz = sigma |a| (-omega_b sin psi_b + omega_M sin psi_M)
        dx = sigma chop |a| (k^x_b sin psi_b + k^x_M sin psi_M)   vx = sigma chop |a| (omega_b k^x_b cos psi_b - omega_M k^x_M cos psi_M)
    the amplitude of either wave's velocity is omega |a|, a quarter period ahead of its displacement."""
    M = (N - 1 - b[0], N - 1 - b[1])
    ax, ay = float(F(a[0])), float(F(a[1]))                # the fp32 values h0 holds
    amp, arg = float(np.hypot(ax, ay)), float(np.arctan2(ay, ax))
    i = np.arange(N, dtype=np.float64)
    X, Y = i[None, :], i[:, None]
    knx, kny = ref64._unit_k(N, scale)
    psi_b = TWO_PI * (b[1] * X + b[0] * Y) / N + float(phase[b]) + arg
    psi_m = TWO_PI * (M[1] * X + M[0] * Y) / N - float(phase[M]) - arg
    wb, wm = float(omega[b]), float(omega[M])
    sg = ref64._sign(N)
    out = np.empty((3, N, N), np.float64)
    out[2] = sg * amp * (-wb * np.sin(psi_b) + wm * np.sin(psi_m))
    out[0] = sg * float(chop) * amp * (wb * knx[b] * np.cos(psi_b) - wm * knx[M] * np.cos(psi_m))
    out[1] = sg * float(chop) * amp * (wb * kny[b] * np.cos(psi_b) - wm * kny[M] * np.cos(psi_m))
    return out


def khat32(N, scale):
    """k^ of sim.comp:52-54 in fp32 as ocean_velocity.h's velocity_khat forms it: ([N][N] knx, kny)"""
    i = np.arange(N, dtype=np.float32)
    k = (F(6.28318530717958647692) * (i - F(0.5) * F(N))) * F(scale)
    kx, ky = np.broadcast_to(k[None, :], (N, N)), np.broadcast_to(k[:, None], (N, N))
    ln = np.sqrt(kx * kx + ky * ky)
    zero = ln == 0
    ln = np.where(zero, F(1), ln)
    return np.where(zero, F(0), kx / ln).astype(np.float32), np.where(zero, F(0), ky / ln).astype(np.float32)


def spectrum32(h0, sn, cs, omega, knx, kny):
    """(ht, htx, hty) [N][N][2] fp32 from h0 [N][N][2], sin and cos of the phase, omega and k^ (all fp32), every operation rounded as
    ocean_velocity.h: velocity_spectrum writes it"""
    ax, ay = h0[..., 0], h0[..., 1]
    mx, my = ax[::-1, ::-1], ay[::-1, ::-1]
    re = omega * (-(ax + mx) * sn - (ay + my) * cs)
    im = omega * ((ax - mx) * cs - (ay - my) * sn)
    return (np.stack([re, im], -1).astype(np.float32), np.stack([im * knx, -re * knx], -1).astype(np.float32),
            np.stack([im * kny, -re * kny], -1).astype(np.float32))


def vel32(oracle, h0, phase, omega, scale, chop, w=None):
    """the fp32 restatement [3][N][N] (vx, vy, vz): spectrum32 with numpy's fp32 sin / cos, the oracle's radix-2 transforms on the table w
    (default: the reduced-argument table), sigma, choppiness"""
    N = phase.shape[0]
    h0, phase = np.asarray(h0, np.float32), np.asarray(phase, np.float32)
    knx, kny = khat32(N, scale)
    ht, htx, hty = spectrum32(h0, np.sin(phase), np.cos(phase), np.asarray(omega, np.float32), knx, kny)
    w = oracle.weights(N, reduced=True) if w is None else w
    sg = ref64._sign(N).astype(np.float32)
    t = [oracle.ffty(oracle.fftx(f, w), w)[..., 0] for f in (htx, hty, ht)]
    return np.stack([(t[0] * sg) * F(chop), (t[1] * sg) * F(chop), t[2] * sg]).astype(np.float32)


def k_of(got, ref, N):
    """worst |got - ref| over the three channels in pointwise.pointwise's displacement units: the smallest K that passes"""
    s = pw.disp_scales(ref)
    L = np.log2(N)
    return max(float((np.abs(got[ch] - ref[ch]) / (pw.EPS * L * s[ch])).max()) for ch in range(3))


# -- the query's velocity sample -------------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 arrays, rounded once: the product is exact in float64; the float64 sum is rounded to odd (TwoSum's error
    term), so that the final rounding to fp32 is that of the exact value"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


class Texel32:
    """SurfaceTexel (ocean_surface.hip) in fp32 at positions (px, py) for a cascade of scale `scale`"""

    def __init__(self, N, scale, px, py):
        fn, rfn = F(N), F(1) / F(N)
        fx = (px * F(scale)) * fn - F(0.5)
        fy = (py * F(scale)) * fn - F(0.5)
        flx, fly = np.floor(fx), np.floor(fy)
        ax, ay = fx - flx, fy - fly
        tx, ty = flx * rfn, fly * rfn
        mx, my = (tx - np.floor(tx)) * fn, (ty - np.floor(ty)) * fn
        bx, by = F(1) - ax, F(1) - ay
        self.w00, self.w10, self.w01, self.w11 = bx * by, ax * by, bx * ay, ax * ay
        self.i0, self.j0 = mx.astype(np.int64), my.astype(np.int64)
        self.i1, self.j1 = (self.i0 + 1) % N, (self.j0 + 1) % N
        self.wantx, self.wanty = ax != 0, ay != 0

    def blend(self, plane):
        """gen's blend order w11 a11 + (w01 a01 + (w10 a10 + w00 a00)) in FMAs; a zero-weight corner is not fetched (0)"""
        a00 = plane[self.j0, self.i0]
        a10 = np.where(self.wantx, plane[self.j0, self.i1], F(0))
        a01 = np.where(self.wanty, plane[self.j1, self.i0], F(0))
        a11 = np.where(self.wantx & self.wanty, plane[self.j1, self.i1], F(0))
        return fma32(self.w11, a11, fma32(self.w01, a01, fma32(self.w10, a10, self.w00 * a00)))


def sample32(maps_list, planes, scales, points, iterations):
    """Fields 4-6 of datum_ocean_read_velocity_blend, (M, 3) fp32, for a set WITHOUT swell (swellamplitude = 0: P(b) = b exactly).
    maps_list: the listed cascades' logical maps [2][N][N][4] (read_maps); planes: their velocity planes [N][N][4] (read_velocity);
    scales: the handle's fp32 1 / wavescale per listed cascade; points (M, 2) fp32, finite."""
    q = np.asarray(points, np.float32).reshape(-1, 2)
    N = planes[0].shape[0]
    qx, qy = q[:, 0].copy(), q[:, 1].copy()
    bx, by = qx.copy(), qy.copy()
    for _ in range(iterations):
        dx = dy = None
        for maps, sc in zip(maps_list, scales):
            t = Texel32(N, sc, bx, by)
            cx, cy = t.blend(maps[0][..., 0]), t.blend(maps[0][..., 1])
            dx = cx if dx is None else dx + cx
            dy = cy if dy is None else dy + cy
        bx, by = bx + (qx - (bx - dx)), by + (qy - (by - dy))
    out = None
    for pl, sc in zip(planes, scales):
        t = Texel32(N, sc, bx, by)
        u = np.stack([t.blend(pl[..., ch]) for ch in range(3)], -1)
        out = u if out is None else out + u
    return out.astype(np.float32)
