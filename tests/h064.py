"""The device-side spectrum build (ocean_kernels.hip: ocean_height_kernel, the h0 loop of ocean.cpp:89-107 / :194-211) as an interval walk
in float64, beside body64.py, drag64.py and vel64.py.  Pure numpy.

  inputs32    dk = 6.2831855f / wavescale and kx[n], ky[m] = dk * ((float)n - 0.5f * N) in numpy float32, one rounding each as written
  walk        (lo, hi, mid) float64 [rows, N] for amp = dk * sqrt(P / 2): every fp32 result the kernel's expression can give lies in
              [lo, hi]; mid is the plain float64 value of the formula from the same float32 kx, ky and the float32 constants
  amp32       the formula in numpy float32, operation for operation; `mistake` plants the errors tests/test_h064.py names (MISTAKES)
  CASES       the cases both tests use, with case_rows / case_seed / case_walk (the walk is made once per case and shared)

Why an interval and not a value with a bar.  P = a * d * expf(-1 / (k2 L2)) / (k2 k2 k2) * (kdotw kdotw) * expf(-k2 l2): an exponential
carries its argument's error times the argument (thousands at a long wavescale, tens of thousands under a strong wind at a short one);
either exponential and any running product can fall into the subnormals, lose its bits there and come back into the normal range through
the division by a tiny k2^3; and kdotw = kx wx + ky wy cancels near the line across the wind, where its sign picks d.  A relative bar of
"roundings x eps" fails on correct code at thousands of points; the walk gives each point the width its own operands earn.

The rules of the walk:
  * dk, kx, ky (inputs32), L2, l2 (scalars32) and the arguments are exact inputs: a mistake in the kernel's version of them shows as an error;
  * every later operation is evaluated on an interval, in the kernel's order and association (ocean.cpp:89-107), each end rounded outward
    in float64 (np.nextafter);
  * each + - * / and sqrt widens its result by one relative EPS = 2^-24: correctly rounded under -ffp-contract=off -fno-fast-math
    (the build's flags; the disassembly shows v_div_scale / v_div_fmas / v_div_fixup and the v_sqrt_f32 fix-up sequence, no v_rcp shortcut);
  * each expf widens by EXP_ULPS = 3 ulp (3 x 2^-23 relative): OCML is held to the OpenCL full-profile bound for exp, 3 ulp; HIP's own
    math table states 1.  3 is used here;
  * every operation also widens downwards by an absolute TINY = 2^-126 and upwards by 2^-150: a subnormal result, kept or flushed to zero
    (below: "where this walk says more");
  * a result of non-negative operands is non-negative (rounding keeps the sign): such lower ends are clamped at 0;
  * where the kdotw interval contains 0, d is [0.2f, 1] and the lower end of kdotw^2 is 0;
  * kx == 0 && ky == 0 gives exactly [0, 0].
No other constant is written down.  h0 = seed * amp is one more rounding (bounds_for_product; 2^-149 is the floor of a kept subnormal).

*Loose* point: hi > 2^-120 and hi - lo > 1e-3 hi.  tests/test_h064.py requires of the walk alone: loose <= 5 % of the plane; <= 1 % of
the points with mid > 1e-6 max(mid); median (hi - lo) / hi over hi > 2^-120 at most 1e-5.  Measured (shares of the case's points; "amb"
the points whose d is ambiguous; "tiny" those with hi <= 2^-120; widths relative to hi over hi > 2^-120):

  case      N  points   loose     loose among   median    wider than  amb   hi == 0   largest |x - mid| / (hi - lo) of
                                  mid > 1e-6 max  width     1e-5              (= tiny)  the oracle's float32   the MI355X
  A        64    4096   2.9e-3    0             2.09e-6   1.22 %        0   0.02 %    0.363                  0.363
  B       256   65536   9.6e-4    0             2.12e-6   1.11 %       63   0.00 %    0.340                  0.341
  C        64    4096   5.9e-3    0             2.97e-6   3.76 %       63   3.27 %    0.192                  0.192
  D       512  262144   0         0             3.08e-6   0           511   0.20 %    0.439                  0.439
  E      1024 1048576   4.7e-4    0             9.32e-6   0.07 %      255   99.84 %   0.427                  0.427
  F      2048 4194304   9.7e-5    0             2.09e-6   1.19 %        0   0.00 %    0.459                  0.459
  H      4096  262144   8.8e-5    0             2.14e-6   1.02 %       16   0.00 %    0.382                  0.382
(1/2 in the last columns would be an end of an interval whose middle is mid.  No point of the oracle, of the host shim, of numpy's float32
or of the device lay outside.  The loose points lie along the line across the wind, where kdotw cancels, and in the underflow rings;
none carries energy.)

Where this walk says more than "one eps and 2^-126 at every operation", and why.  Taken literally that rule leaves case E hollow: sqrt
brings an absolute 2^-126 on P back to 2^-63 on amp, so every point where the second exponential underflows would be loose (99.9 % of E;
its median width 1) and a wrong non-zero value there would pass.  Three statements about correctly rounded fp32 arithmetic, each at least
as strict, close that:
  * the absolute term is one-sided.  A flush lowers a magnitude, by less than 2^-126: that is the lower end.  Upwards a result moves by its
    rounding alone, inside the subnormals by at most HALF_SUB = 2^-150 (half the spacing 2^-149); for expf, EXP_ULPS spacings;
  * a correctly rounded result whose exact value lies under HALF_SUB is 0, kept or flushed: [0, 0].  (Not so for expf, which is not
    correctly rounded: where exp underflows its interval is [0, 3 x 2^-149], and the product that follows is what rounds to 0);
  * L2 and l2 (scalars32) are, like dk, correctly rounded operations on the arguments alone and are taken as exact inputs in float32.
    Walked as intervals they add 5 eps to the argument of the second exponential at every point alike; E's median width is then 2.56e-5
    and no case of its kind (the survivors fill the disc x2 < 104 evenly, so their median x2 is about 52) can meet the 1e-5 condition.
"""

import functools

import numpy as np

F = np.float32
EPS = 2.0 ** -24
TINY = 2.0 ** -126
HALF_SUB = 2.0 ** -150        # half the smallest subnormal, 2^-149
EXP_ULPS = 3
FLOOR = 2.0 ** -120          # below it a point's interval is compared as |got| <= hi only (the loose rule above)
F32_MAX = float(np.finfo(np.float32).max)

MISTAKES = ("g_9.8", "against_0.25", "no_half", "damping_0.002", "swap_k", "wind_negated", "centre_off_by_one", "k2_squared", "second_trip_stride")

# name: N, wavescale, waveamplitude, windspeed, (windx, windy)
CASES = {
    "A": (64, 22.0, 0.0025, 7.9, (0.780869, 0.624695)),          # oracle.EXAMPLE
    "B": (256, 30.0, 0.004, 12.0, (0.6, 0.8)),
    "C": (64, 2000.0, 0.0025, 7.9, (1.0, 0.0)),                  # the first exponential underflows in a ring round the centre; column N/2 is zero
    "D": (512, 0.5, 0.01, 3.0, (0.0, -1.0)),                     # x2 matters; exactly one trip of the grid-stride loop (1024 x 256 threads)
    "E": (1024, 1.5, 0.004, 30.0, (-0.6, 0.8)),                  # the second exponential underflows over most of the plane; four trips
    "F": (2048, 400.0, 0.0025, 7.9, (0.780869, -0.624695)),
    "H": (4096, 1000.0, 0.0025, 20.0, (0.6, 0.8)),               # 64 rows only (case_rows)
}
H_ROWS = 64
WALK_BLOCK = 1 << 15
TRIP = 1024 * 256            # the kernel's grid: points per trip of its grid-stride loop


def inputs32(N, wavescale, rows=None):
    """(dk, kx [N], ky [rows]) in float32, each one correctly rounded operation as the kernel writes it"""
    dk = F(6.2831855) / F(wavescale)
    n = np.arange(N, dtype=F)
    m = n if rows is None else np.asarray(rows).astype(F)
    half = F(0.5) * F(N)
    kx, ky = dk * (n - half), dk * (m - half)
    assert dk.dtype == F and kx.dtype == F and ky.dtype == F
    return dk, kx, ky


def scalars32(windspeed):
    """(L2, l2) in float32: L = v * v / 9.81f, L2 = L * L, l2 = L2 * 0.001f * 0.001f, each operation correctly rounded as written"""
    v = F(windspeed)
    L = v * v / F(9.81)
    L2 = L * L
    l2 = L2 * F(0.001) * F(0.001)
    assert L2.dtype == F and l2.dtype == F
    return L2, l2


# -- interval arithmetic on pairs (lo, hi) of float64 arrays -----------------------------------------------------------------------------

def _out(lo, hi):
    return np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)


def _round(lo, hi, rel=EPS):
    """one fp32 operation's result of either sign: widened by `rel` relative and TINY absolute, outward in float64"""
    return _out(lo - np.abs(lo) * rel - TINY, hi + np.abs(hi) * rel + TINY)


def _round_nn(lo, hi, rel=EPS, sub=HALF_SUB, correctly_rounded=True):
    """one fp32 operation's non-negative result.  Below: `rel` and TINY, clamped at 0 (a subnormal kept or flushed).  Above: `rel` and
    `sub`, the rounding error inside the subnormals, where a flush only lowers; and a correctly rounded result whose exact value lies under
    half the smallest subnormal is 0 itself, flushed or not"""
    lo = np.nextafter(lo - lo * rel - TINY, -np.inf)
    up = np.nextafter(hi + hi * rel + sub, np.inf)
    if correctly_rounded:
        up = np.where(hi < HALF_SUB, 0.0, up)
    return np.maximum(lo, 0.0), up


def _pt(x):
    x = np.asarray(x, np.float64)
    return x, x


def _add(a, b):
    return _round(*_out(a[0] + b[0], a[1] + b[1]))


def _add_nn(a, b):
    return _round_nn(*_out(a[0] + b[0], a[1] + b[1]))


def _mul_nn(a, b):
    """product of two non-negative intervals"""
    return _round_nn(*_out(a[0] * b[0], a[1] * b[1]))


def _div_nn(a, b):
    """quotient of a non-negative interval by a non-negative one (an end of b at 0 gives +inf)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where((a[0] == 0) | np.isinf(b[1]), 0.0, a[0] / b[1])
        hi = np.where(b[0] > 0, a[1] / np.where(b[0] > 0, b[0], 1.0), np.inf)
    return _round_nn(*_out(lo, hi))


def _exp_neg(a):
    """expf(-a) of a non-negative interval"""
    with np.errstate(under="ignore"):
        return _round_nn(*_out(np.exp(-a[1]), np.exp(-a[0])), rel=EXP_ULPS * 2 * EPS, sub=EXP_ULPS * 2 * HALF_SUB, correctly_rounded=False)


def _sqrt_nn(a):
    return _round_nn(*_out(np.sqrt(a[0]), np.sqrt(a[1])))


def walk(N, wavescale, waveamplitude, windspeed, windx, windy, rows=None, detail=False):
    """(lo, hi, mid) float64 [rows, N] of amp = dk * sqrtf(phillips / 2.0f); with detail also the mask of the points whose d is ambiguous.
    The arguments are the float32 values the C ABI receives; waveamplitude >= 0 and everything finite."""
    a, v, wx, wy = (float(F(x)) for x in (waveamplitude, windspeed, windx, windy))
    assert a >= 0 and np.isfinite([a, v, wx, wy]).all() and F(wavescale) > 0
    dk, kx32, ky32 = inputs32(N, wavescale, rows)
    kx, ky = kx32.astype(np.float64)[None, :], ky32.astype(np.float64)[:, None]
    g, against, damping = float(F(9.81)), float(F(0.2)), float(F(0.001))
    # L = v * v / 9.81f;   L2 = L * L;   l2 = L2 * 0.001f * 0.001f: scalars of the arguments alone
    L2s, l2s = scalars32(windspeed)

    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        # float kdotw = kx * wx + ky * wy;   d = (kdotw < 0) ? 0.2f : 1
        kd = _add(_round(*_pt(kx * wx)), _round(*_pt(ky * wy)))   # the products of two floats are exact in float64
        neg, pos = kd[1] < 0, kd[0] >= 0
        d = np.where(pos, 1.0, against), np.where(neg, against, 1.0)
        kd2 = _round_nn(*_out(np.where(neg | pos, np.minimum(kd[0] * kd[0], kd[1] * kd[1]), 0.0), np.maximum(kd[0] * kd[0], kd[1] * kd[1])))

        L2, l2 = _pt(float(L2s)), _pt(float(l2s))

        k2 = _add_nn(_mul_nn(_pt(np.abs(kx)), _pt(np.abs(kx))), _mul_nn(_pt(np.abs(ky)), _pt(np.abs(ky))))

        # a * d * expf(-1 / (k2 * L2)) / (k2 * k2 * k2) * (kdotw * kdotw) * expf(-k2 * l2), left to right
        e1 = _exp_neg(_div_nn(_pt(1.0), _mul_nn(k2, L2)))
        e2 = _exp_neg(_mul_nn(k2, l2))
        p = _mul_nn(_pt(a), d)
        p = _mul_nn(p, e1)
        p = _div_nn(p, _mul_nn(_mul_nn(k2, k2), k2))
        p = _mul_nn(p, kd2)
        p = _mul_nn(p, e2)
        lo, hi = _mul_nn(_pt(float(dk)), _sqrt_nn(_div_nn(p, _pt(2.0))))

        # the plain value
        kdm = kx * wx + ky * wy
        Lm = v * v / g
        k2m = kx * kx + ky * ky
        with np.errstate(divide="ignore", invalid="ignore"):
            pm = a * np.where(kdm < 0, against, 1.0) * np.exp(-1.0 / (k2m * (Lm * Lm))) / (k2m * k2m * k2m) * (kdm * kdm) * np.exp(-k2m * (Lm * Lm * damping * damping))
        mid = float(dk) * np.sqrt(pm / 2.0)

    centre = (kx == 0) & (ky == 0)
    lo, hi, mid = (np.where(centre, 0.0, x) for x in (lo, hi, mid))
    assert np.all(lo <= hi) and np.all(lo >= 0) and np.all(hi < F32_MAX), "an intermediate leaves fp32's range: not a case for this walk"
    return (lo, hi, mid, ~(neg | pos) & ~centre) if detail else (lo, hi, mid)


def bounds_for_product(lo, hi, s):
    """(lo, hi) of |fl32(s * amp)| for amp in [lo, hi]: one more rounding, and 2^-149 for a subnormal product"""
    s = np.abs(np.asarray(s, np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        plo, phi = _out(lo * s, hi * s)
        plo, phi = _out(plo - plo * EPS - 2.0 ** -149, phi + phi * EPS + 2.0 ** -149)
    return np.maximum(plo, 0.0), np.where(hi == 0, 0.0, phi)


def amp32(N, wavescale, waveamplitude, windspeed, windx, windy, rows=None, mistake=None):
    """amp [rows, N] in numpy float32, every operation one rounding in the kernel's order; `mistake` one of MISTAKES"""
    assert mistake is None or mistake in MISTAKES
    a, v, wx, wy = F(waveamplitude), F(windspeed), F(windx), F(windy)
    dk = F(6.2831855) / F(wavescale)
    n = np.arange(N, dtype=np.int64)[None, :]
    m = (np.arange(N, dtype=np.int64) if rows is None else np.asarray(rows, np.int64))[:, None]
    if mistake == "second_trip_stride":          # the m and n of point i + N from the second trip on
        i = m * N + n
        i = np.where(i >= TRIP, i + N, i)
        m, n = i // N, i % N
    m, n = np.broadcast_arrays(m, n)
    half = F(0.5) * F(N) - F(1) if mistake == "centre_off_by_one" else F(0.5) * F(N)
    ky, kx = dk * (m.astype(F) - half), dk * (n.astype(F) - half)
    if mistake == "swap_k":
        kx, ky = ky, kx
    if mistake == "wind_negated":
        wx, wy = -wx, -wy
    with np.errstate(all="ignore"):
        kd = kx * wx + ky * wy
        d = np.where(kd < 0, F(0.25 if mistake == "against_0.25" else 0.2), F(1))
        L = v * v / F(9.8 if mistake == "g_9.8" else 9.81)
        L2 = L * L
        damping = F(0.002 if mistake == "damping_0.002" else 0.001)
        l2 = L2 * damping * damping
        k2 = kx * kx + ky * ky
        k6 = k2 * k2 if mistake == "k2_squared" else k2 * k2 * k2
        p = a * d * np.exp(F(-1) / (k2 * L2)) / k6 * (kd * kd) * np.exp(-k2 * l2)
        p = np.where((kx == 0) & (ky == 0), F(0), p)
        amp = dk * np.sqrt(p if mistake == "no_half" else p / F(2))
    assert amp.dtype == F
    return amp


# -- the cases ---------------------------------------------------------------------------------------------------------------------------

def case_args(name):
    N, ws, a, v, (wx, wy) = CASES[name]
    return N, F(ws), F(a), F(v), F(wx), F(wy)


def case_rows(name):
    """None (the whole plane), or case H's 64 rows: first, last, N/2 - 1 ... N/2 + 1, the rest drawn"""
    if name != "H":
        return None
    N = CASES[name][0]
    fixed = [0, N - 1, N // 2 - 1, N // 2, N // 2 + 1]
    rest = np.setdiff1d(np.arange(N), fixed)
    return np.sort(np.concatenate([fixed, np.random.RandomState(4096).choice(rest, H_ROWS - len(fixed), replace=False)]))


def case_seed(name):
    """[N, N, 2] float32: random normal with 0, -0.0, 1e30 and 1e-30 planted (and their negatives), the same on every call"""
    N = CASES[name][0]
    rng = np.random.RandomState(sum(map(ord, name)) + N)
    s = rng.standard_normal((N, N, 2)).astype(F)
    flat = s.reshape(-1)
    at = rng.choice(flat.size, 8 * max(16, N // 4), replace=False).reshape(8, -1)
    for k, val in enumerate((0.0, -0.0, 1e30, -1e30, 1e-30, -1e-30)):
        flat[at[k]] = F(val)
    rows = case_rows(name)
    r = np.arange(N) if rows is None else rows
    # some of each on the lines the cases are about: the centre row and column (whichever rows are compared)
    for k, val in enumerate((0.0, -0.0, 1e30, 1e-30)):
        s[r[(3 + 5 * k) % len(r)], N // 2 + 3 + k, :] = F(val)
        s[N // 2, (7 + 11 * k) % N, :] = F(val)
    return s


@functools.lru_cache(maxsize=None)
def case_walk(name):
    """(lo, hi, mid, ambiguous) of the case, over case_rows(name); made once"""
    N = CASES[name][0]
    rows = np.arange(N) if case_rows(name) is None else case_rows(name)
    # in blocks of rows that stay in the cache: the walk is some sixty passes over its arrays
    parts = [walk(*case_args(name), rows=rows[k:k + WALK_BLOCK // N], detail=True) for k in range(0, len(rows), WALK_BLOCK // N)]
    out = tuple(np.concatenate(x) for x in zip(*parts))
    for x in out:
        x.setflags(write=False)
    return out


def shares(lo, hi, mid, amb):
    """the measured figures of a walk: dict of shares (of all points) and widths"""
    big = hi > FLOOR
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(big, (hi - lo) / hi, 0.0)
    loose = big & (w > 1e-3)
    carrying = mid > 1e-6 * mid.max()
    return dict(points=hi.size, loose=loose.mean(), loose_carrying=(loose & carrying).sum() / max(1, carrying.sum()), median=float(np.median(w[big])) if big.any() else 0.0,
                wider_1e5=(big & (w > 1e-5)).mean(), ambiguous=int(amb.sum()), tiny=(~big).mean(), zero=(hi == 0).mean())


def outside(got, seed, lo, hi):
    """mask [rows, N, 2] of the components of h0 = seed * amp that no amp in [lo, hi] explains: the magnitude outside bounds_for_product,
    not exactly zero where hi == 0, the sign not the seed's (amp >= +0, so a zero product carries the seed's sign too), or not finite"""
    got, seed = np.asarray(got), np.asarray(seed)
    plo, phi = bounds_for_product(lo[..., None], hi[..., None], seed)
    mag = np.abs(got.astype(np.float64))
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(got) | (mag < plo) | (mag > phi) | (np.signbit(got) != np.signbit(seed))


def ratio(got, seed, lo, hi, mid):
    """the largest |got / seed - mid| / (hi - lo) over the components whose seed is an ordinary number and whose interval is above FLOOR"""
    s = np.asarray(seed, np.float64)
    use = ((hi > FLOOR) & (lo > 0))[..., None] & (np.abs(s) > 1e-3) & (np.abs(s) < 1e3)
    with np.errstate(all="ignore"):
        r = np.abs(np.asarray(got, np.float64) / s - mid[..., None]) / (hi - lo)[..., None]
    return float(r[use].max()) if use.any() else 0.0
