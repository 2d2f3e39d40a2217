"""A staged reference of data/ocean.gen.comp:67-137 for the pointwise pins of the mesh kernel (tests/test_gen64.py on the CPU,
tests/test_gpu_gen_pointwise.py on the device).

gen.comp has two kinds of arithmetic.  The view ray, the plane hit and the swell phase (gen.comp:75-99) AMPLIFY a rounding: one ulp of
the ray moves a grazing vertex by dist / costheta ulps, the swell phase turns metres into radians.  A float64 evaluation of these lines
says nothing about an fp32 implementation there (gen_cases.well_conditioned masks such vertices out).  Everything after them -- the
Gerstner frame, the bilinear sample, the mix, the normalisations -- is well conditioned in its inputs.  So the reference is cut there:

  * ray32() restates gen.comp:75-99 in numpy float32, operation for operation as the shader writes them.  numpy's float32 + - * / sqrt
    are correctly rounded and never contracted, so this is the IEEE fp32 value of every intermediate: an implementation that promises the
    shader's roundings has to return these bits.
  * staged64() evaluates everything downstream in float64 FROM those fp32 values, and takes sin / cos of the swell phase as arguments:
    whatever it returns differs from an exact evaluation of the shader's remaining lines by float64 roundings only.

Three facts make the stages observable in the kernel's output (the tests lean on them):
  1. swellsteepness = 0: position.xy = base.xy exactly, texcoord = 0.1f * base.xy is a function of the ray stage alone;
  2. a flat ocean (h0 = 0): vertex.z = basez + amplitude * sin(theta), the frame is the Gerstner frame alone;
  3. with both known, vertex.xyz - position on real maps is the bilinear sample alone.
"""

from types import SimpleNamespace

import numpy as np

F = np.float32

# The normal range the kernel's division and square root are exact in without range scaling and fix-up (ocean_gen.hip: div_exact,
# sqrt_exact): every operand, every quotient and every intermediate of the refinement stays a normal number well inside this
NORMAL_LO, NORMAL_HI = 2.0 ** -100, 2.0 ** 100


def _f(a):
    return np.array(list(a), F)


def ray32(s, sizex, sizey):
    """gen.comp:75-99 in float32 from the 216-byte OceanSet header `s`: every value as an fp32 scalar or a [sizey, sizex] fp32 array."""
    ip = _f(s.invproj)
    rw, ri, rj, rk = _f(s.camera_real)
    dw, di, dj, dk = _f(s.camera_dual)
    plane = _f(s.plane)
    amplitude, steepness, length, phase0 = F(s.swellamplitude), F(s.swellsteepness), F(s.swelllength), F(s.swellphase)
    dirx, diry = _f(s.swelldirection)
    two = F(2)

    with np.errstate(all="ignore"):
        # camerapos = 2 * (dual * conjugate(real)).yzw   (gen.comp:75; the Hamilton product's summation order of transform.inc:22-25)
        bw, bi, bj, bk = rw, -ri, -rj, -rk
        camerapos = np.array([two * (dw * bi + di * bw + dj * bk - dk * bj),
                              two * (dw * bj + dj * bw + dk * bi - di * bk),
                              two * (dw * bk + dk * bw + di * bj - dj * bi)], F)
        cameraheight = (plane[0] * camerapos[0] + plane[1] * camerapos[1] + plane[2] * camerapos[2]) + plane[3]
        margin_arg = (two * amplitude + F(0.5)) / cameraheight
        margin = F(1) + np.sqrt(margin_arg)

        xx = np.arange(sizex, dtype=F)[None, :]
        yy = np.arange(sizey, dtype=F)[:, None]
        uq = two * xx / F(sizex - 1)
        vq = two * yy / F(sizey - 1)
        u = np.broadcast_to((uq - F(1)) * margin, (sizey, sizex))
        v = np.broadcast_to((F(1) - vq) * margin, (sizey, sizex))

        # viewvec = invproj * vec4(u, v, 0, 1), row_major: the * 0.0f and * 1.0f terms are the shader's
        viewvec = np.stack([((ip[4 * r + 0] * u + ip[4 * r + 1] * v) + ip[4 * r + 2] * F(0.0)) + ip[4 * r + 3] * F(1.0) for r in range(3)], -1)
        vx, vy, vz = viewvec[..., 0], viewvec[..., 1], viewvec[..., 2]
        dotvv = (vx * vx + vy * vy) + vz * vz
        length_ = np.sqrt(dotvv)
        nx, ny, nz = vx / length_, vy / length_, vz / length_

        # qrot (transform.inc:32-37): t = 2 * cross(q.yzw, v); v + q.x * t + cross(q.yzw, t)
        ux, uy, uz = ri, rj, rk
        tx, ty, tz = two * (uy * nz - uz * ny), two * (uz * nx - ux * nz), two * (ux * ny - uy * nx)
        wx = (nx + rw * tx) + (uy * tz - uz * ty)
        wy = (ny + rw * ty) + (uz * tx - ux * tz)
        wz = (nz + rw * tz) + (ux * ty - uy * tx)

        costheta = (wx * -plane[0] + wy * -plane[1]) + wz * -plane[2]
        hit = costheta > 0
        quotient = cameraheight / np.where(hit, costheta, F(1))
        dist = np.where(hit, quotient, F(1e6)).astype(F)

        basex = camerapos[0] + dist * wx
        basey = camerapos[1] + dist * wy
        basez = -plane[3]

        frequency = two * F(3.14159265358979323846) / length
        qi = steepness / (frequency * amplitude * F(4) + F(1e-6))
        phi = frequency * amplitude
        theta = frequency * (dirx * basex + diry * basey) + phase0
        cl = dist * F(s.smoothing) - F(0.35)

        # the constants of the Gerstner terms as gen.comp:97-105 rounds them (left to right)
        gx, gy = qi * amplitude * dirx, qi * amplitude * diry
        normal_c = np.array([phi * dirx / F(6), phi * diry / F(6), qi * phi], F)                                  # * (ct, ct, st)
        tangent_c = np.array([qi * phi * dirx * dirx, qi * phi * diry * dirx, phi * dirx / F(6)], F)              # * (st, st, ct)

    for a in (u, v, viewvec, dotvv, length_, costheta, dist, basex, basey, theta, cl):
        assert a.dtype == F
    return SimpleNamespace(sizex=sizex, sizey=sizey, camerapos=camerapos, cameraheight=F(cameraheight), margin=F(margin), margin_arg=F(margin_arg),
                           u=u, v=v, uq=uq, vq=vq, viewvec=viewvec, dotvv=dotvv, len=length_, viewdir=np.stack([nx, ny, nz], -1),
                           worlddir=np.stack([wx, wy, wz], -1), costheta=costheta, hit=hit, quotient=quotient, dist=dist,
                           base=np.stack([basex, basey], -1), basez=F(basez), theta=theta, cl=cl, frequency=F(frequency), qi=F(qi), phi=F(phi),
                           gx=F(gx), gy=F(gy), normal_c=normal_c, tangent_c=tangent_c, amplitude=amplitude)


def normal_range(ray):
    """The precondition of the kernel's division and square root, as a condition on the case: (name, smallest |value|, largest |value|)
    of every operand and result of a division or a square root in gen.comp:75-91."""
    out = []
    hit = ray.hit

    def add(name, a, where=None, zero_ok=False):
        a = np.abs(np.asarray(a, np.float64))
        if where is not None:
            a = a[where]
        if zero_ok:
            a = a[a != 0]               # 0 / b = 0 exactly in every division sequence, range scaling or not
        if a.size:
            out.append((name, float(a.min()), float(a.max())))

    add("cameraheight", ray.cameraheight)
    add("(2 amplitude + 0.5) / cameraheight", ray.margin_arg)
    add("2 x / (sizex - 1)", ray.uq, zero_ok=True)
    add("2 y / (sizey - 1)", ray.vq, zero_ok=True)
    add("dot(viewvec, viewvec)", ray.dotvv)
    add("len", ray.len)
    add("viewvec / len", ray.viewdir, zero_ok=True)
    add("viewvec", ray.viewvec, zero_ok=True)
    add("costheta > 0", ray.costheta, hit)
    add("cameraheight / costheta", ray.quotient, hit)
    return out


def _unit(a):
    return a / np.sqrt((a * a).sum(-1, keepdims=True))


def texel32(s, ray, N, px, py):
    """gen.comp:113-114's addressing in float32 from an fp32 position: (i0, j0, ax, ay), the unnormalised coordinate
    (p * scale) * N - 0.5, its floor, the weights and the floor wrapped to [0, N)."""
    scale, fn = F(s.scale), F(N)
    with np.errstate(all="ignore"):
        fx = (px.astype(F) * scale) * fn - F(0.5)
        fy = (py.astype(F) * scale) * fn - F(0.5)
        flx, fly = np.floor(fx), np.floor(fy)
        ax, ay = fx - flx, fy - fly
    assert ax.dtype == F and ay.dtype == F
    # floor(coordinate) mod N: the floats are integers, fmod is exact (up to 2^31 and beyond: dist = 1e6 at small wave scales)
    i0 = np.mod(flx.astype(np.float64), N).astype(np.int64)
    j0 = np.mod(fly.astype(np.float64), N).astype(np.int64)
    return i0, j0, ax, ay


def staged64(s, maps, ray, st=None, ct=None, shift=(0, 0), swap_weights=False):
    """gen.comp:93-137 in float64 downstream of ray32's fp32 values.  `maps` [2, N, N, 4]; `st`, `ct`: sin / cos of the swell phase
    ([sizey, sizex], default: of float64(theta32)).  `shift` moves the sampled texel, `swap_weights` exchanges ax and ay: the two
    mistakes the sensitivity test plants.  Returns a namespace: vertices [sizey, sizex, 12] float64, position [.., 3] (before the
    displacement), displacement [.., 3], corner [.., 3] (the largest |texel component| of the four corners), i0, j0, ax, ay."""
    N = maps.shape[1]
    theta = ray.theta.astype(np.float64)
    st = np.sin(theta) if st is None else np.asarray(st, np.float64)
    ct = np.cos(theta) if ct is None else np.asarray(ct, np.float64)
    plane = np.array(list(s.plane), np.float64)
    base = ray.base.astype(np.float64)
    gx, gy, amplitude = float(ray.gx), float(ray.gy), float(ray.amplitude)

    position = np.stack([base[..., 0] + gx * ct, base[..., 1] + gy * ct, float(ray.basez) + amplitude * st], -1)

    # the texel coordinate is amplified by N / wavescale: from the fp32 position, in fp32 (with steepness 0 that is base.xy itself)
    with np.errstate(all="ignore"):
        px32 = ray.base[..., 0] + (ray.gx * ct.astype(F))
        py32 = ray.base[..., 1] + (ray.gy * ct.astype(F))
    i0, j0, ax32, ay32 = texel32(s, ray, N, px32, py32)
    i0, j0 = (i0 + shift[0]) % N, (j0 + shift[1]) % N
    i1, j1 = (i0 + 1) % N, (j0 + 1) % N
    ax, ay = ax32.astype(np.float64)[..., None], ay32.astype(np.float64)[..., None]
    if swap_weights:
        ax, ay = ay, ax

    def sample(layer):
        t00, t10, t01, t11 = (layer[j, i, :3].astype(np.float64) for j, i in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)))
        blend = (1 - ax) * (1 - ay) * t00 + ax * (1 - ay) * t10 + (1 - ax) * ay * t01 + ax * ay * t11
        return blend, np.maximum(np.maximum(np.abs(t00), np.abs(t10)), np.maximum(np.abs(t01), np.abs(t11)))

    disp, corner = sample(maps[0])
    dn, _ = sample(maps[1])

    nc, tc = ray.normal_c.astype(np.float64), ray.tangent_c.astype(np.float64)
    normal = np.stack([nc[0] * ct, nc[1] * ct, nc[2] * st], -1)
    tangent = np.stack([tc[0] * st, tc[1] * st, tc[2] * ct], -1)
    tbn2 = _unit(np.stack([-normal[..., 0], -normal[..., 1], 1 - normal[..., 2]], -1))
    tbn0 = _unit(np.stack([1 - tangent[..., 0], -tangent[..., 1], tangent[..., 2]], -1))
    tbn1 = np.cross(tbn0, tbn2)

    smoothing = (np.clip(ray.cl.astype(np.float64), 0.0, 1.0) ** float(F(0.2)))[..., None]
    tn = dn[..., 0:1] * tbn0 + dn[..., 1:2] * tbn1 + dn[..., 2:3] * tbn2
    tbn2 = _unit(tn * (1 - smoothing) + plane[:3] * smoothing)
    tbn0 = _unit(np.array([1.0, 0.0, 0.0]) - tbn2[..., 0:1] * tbn2)

    out = np.empty(base.shape[:2] + (12,))
    out[..., 0] = position[..., 0] - disp[..., 0]
    out[..., 1] = position[..., 1] - disp[..., 1]
    out[..., 2] = position[..., 2] + disp[..., 2]
    out[..., 3:5] = float(F(0.1)) * position[..., :2]
    out[..., 5:8] = tbn2
    out[..., 8:11] = tbn0
    out[..., 11] = -1
    return SimpleNamespace(vertices=out, position=position, displacement=disp, corner=corner, i0=i0, j0=j0, ax=ax32, ay=ay32,
                           smoothing=smoothing[..., 0], st=st, ct=ct)


# -- the bars ------------------------------------------------------------------------------------------------------------------------

EPS = 2.0 ** -24

# sincos_phase (ocean_phase.h) reduces x by k = rint(x * 2/pi) quarter turns with pi/2 = HEAD + TAIL, two fp32 constants:
PIO2_HEAD = float(F(1.57079637050628662109375))
PIO2_TAIL = -float(F(4.37113900018624283e-8))


def pio2_representation_error():
    """|HEAD + TAIL - pi/2|, exactly (rational arithmetic against 40 digits of pi): what every quarter turn of the reduction is off by."""
    from fractions import Fraction

    pi = Fraction(31415926535897932384626433832795028841971, 10 ** 40)
    return float(abs(Fraction(PIO2_HEAD) + Fraction(PIO2_TAIL) - pi / 2))


# Error of the reduced argument per unit of x.  r = x - k HEAD - k TAIL is evaluated by two FMAs; the first is exact (k HEAD is a
# multiple of ulp(HEAD) = 2^-23 below 2^22 ulps of it and |x - k HEAD| < 1), so the reduced argument is off from x - k pi/2 by
#   |k| * |HEAD + TAIL - pi/2|  +  one rounding of r (inside the 4 * 2^-24 term),
# with |k| <= |x| * 2/pi + 1/2.  HEAD + TAIL - pi/2 = 1.7151e-15 = 2^-49.05 (TAIL is pi/2 - HEAD rounded to fp32: half an ulp of TAIL
# is 2^-49), so c = 2/pi * 1.7151e-15 = 1.092e-15 = 2^-49.70 per unit of x: the issue's estimate of "about 2^-50" is right to a
# quarter of a bit.  |d sin / d r| <= 1, so the same c bounds the error of sin and cos.
SINCOS_C = 2 / np.pi * pio2_representation_error()


def sin_bar(x):
    """|sincos_phase(x) - sin / cos (float64(x))| <= 4 * 2^-24 + |x| * c.  The first term is tests/test_phase_emul.py's: the rounding
    of the reduced argument, the ~1 ulp minimax polynomials; the second the two-constant pi/2 (SINCOS_C above)."""
    return 4 * EPS + np.abs(np.asarray(x, np.float64)) * SINCOS_C


def blend_bar(corner, want):
    """vertex.xyz = position -+ bilinear sample: 2^-24 * (8 max|corner texel| + 2 |want|) -- 8 for the roundings of the weights
    (1 - ax, 1 - ay, four products) and of the four-term blend, each at most one ulp of a value no larger than the largest corner;
    2 for the final subtraction."""
    return EPS * (8 * corner + 2 * np.abs(want))


def frame_bar(oracle_distance):
    """normal and tangent: 8 x the fp32 restatement's own worst distance to staged64 on the same case + 8 * 2^-24.  The oracle's / and
    sqrt are correctly rounded and its pow is libm's (0.5 .. 1 ulp each); the kernel uses v_rsq / v_exp / v_log (1 ulp each) through
    three normalisations.  A wrong term or texel is >= 1e3 ulp."""
    return 8 * oracle_distance + 8 * EPS


def band_limited_h0(N, seed, amplitude=8e-3, kmax=12):
    """A cheap band-limited spectrum [N, N, 2]: random complex amplitudes on |k| <= kmax (both signs), zero elsewhere -- the maps it
    makes vary over a few texels to a few dozen, like a seeded ocean's, without a seeded ocean's 2 N^2 draws."""
    rng = np.random.default_rng(seed)
    h0 = np.zeros((N, N, 2), np.float32)
    k = np.arange(-kmax, kmax + 1)
    idx = k % N
    a = rng.standard_normal((k.size, k.size, 2)) / (1.0 + np.hypot(k[:, None], k[None, :]))[..., None]
    h0[np.ix_(idx, idx)] = (amplitude * a).astype(np.float32)
    h0[0, 0] = 0
    return h0


def header_sincos(x):
    """sin and cos of fp32 arguments by datum_amd/csrc/ocean_phase.h itself, walked on the CPU (tests/cpu/phase_emul.cpp): (sin, cos, sin
    and cos of the packed form), float32, the shape of x."""
    import ctypes
    import os

    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu", "libfft_core_emul.so"))
    lib.phase_sincos.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 4
    x = np.ascontiguousarray(x, F)
    flat = x.ravel()
    if flat.size % 2:
        flat = np.concatenate([flat, flat[:1]])
    out = [np.empty_like(flat) for _ in range(4)]
    lib.phase_sincos(flat.ctypes.data, flat.size, *(o.ctypes.data for o in out))
    return [o[: x.size].reshape(x.shape) for o in out]
