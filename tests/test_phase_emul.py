"""The phase arithmetic the row pass's dispatch rests on (datum_amd/csrc/ocean_phase.h), the very functions the kernels and the host
code call, walked on the CPU (tests/cpu/phase_emul.cpp):

  * the fused advance (phase + w, - 2 pi, select) is fmod, bit for bit, over the whole range the host admits to it -- 0 <= phase < 2 pi
    (phase_in_range) and 0 <= w < 2 pi -- densely and on every edge of that range; the reference is fmod in float64 of the fp32 sum,
    which is exact;
  * the range predicate admits exactly [0, 2 pi), -0.0 included;
  * the polynomial sin / cos (the any-phase row pass) against numpy's float64 sin / cos of the same fp32 argument over |x| <= 1e4, at
    random arguments and at every fp32 neighbour of every multiple of pi/2 there; scalar and packed form bit-identical;
  * the host's decision (which dt's the fused advance may take, which leave a cascade "wild") under a model of datum_ocean_displace.
"""

import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
TWO_PI = F(6.2831855)                       # the constant of ocean_phase.h
BELOW = np.nextafter(TWO_PI, F(0))          # the largest phase inside
TINY = F(1e-45)                             # the smallest subnormal

# Largest |error| of sincos_phase against float64 over |x| <= 1e4, measured by test_polynomial_sincos_against_float64 itself (a
# deterministic CPU computation: g++ 11, glibc 2.35; profiles/pointwise_phase_table.txt): sin 9.22e-08, cos 9.24e-08, i.e. 1.55 * 2^-24,
# under the 4 * 2^-24 the two fused multiply-adds of the reduction and the ~1 ulp polynomials allow.  The bar is twice the measured
# value; the margin covers another host's libm or compiler, nothing else.
SINCOS_MEASURED = 9.24e-8
SINCOS_BAR = 2 * SINCOS_MEASURED


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, Z, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.phase_advance.argtypes = [P, P, Z, P, P]
    lib.phase_in_range.argtypes = [P, Z, P]
    lib.phase_sincos.argtypes = [P, Z, P, P, P, P]
    lib.phase_dt_fusable.argtypes = [ctypes.c_float, ctypes.c_float]
    lib.phase_dt_keeps_range.argtypes = [ctypes.c_float]
    lib.phase_host_step.argtypes = [P, I, P, P, I]
    return lib


def _advance(emul, phase, w):
    phase, w = np.ascontiguousarray(phase, F), np.ascontiguousarray(w, F)
    assert phase.shape == w.shape and phase.ndim == 1
    fused, general = np.empty_like(phase), np.empty_like(phase)
    emul.phase_advance(phase.ctypes.data, w.ctypes.data, phase.size, fused.ctypes.data, general.ctypes.data)
    return fused, general


def _fmod64(phase, w):
    """update_ocean's fmod(phase + w, 2 pi): the sum rounded to fp32 as the kernels round it, the remainder in float64, where it is exact
    (and an fp32 number: it has no bit below the sum's last)"""
    s = (phase.astype(F) + w.astype(F)).astype(np.float64)
    r = np.fmod(s, np.float64(TWO_PI))
    assert np.array_equal(r.astype(F).astype(np.float64), r, equal_nan=True)
    return r.astype(F)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _inside(emul, phase):
    phase = np.ascontiguousarray(phase, F)
    out = np.empty(phase.size, np.uint8)
    emul.phase_in_range(phase.ctypes.data, phase.size, out.ctypes.data)
    return out.astype(bool)


def _neighbours(x, n):
    """x and its n fp32 neighbours on either side"""
    out = [F(x)]
    lo = hi = F(x)
    for _ in range(n):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return out


def test_the_product_calls_the_header():
    # what is walked here is the product's text: the kernels and the host code include the header and keep no copy of its pieces
    kernels = open(os.path.join(ROOT, "datum_amd", "csrc", "ocean_kernels.hip"), encoding="utf-8").read()
    host = open(os.path.join(ROOT, "datum_amd", "csrc", "ocean_capi.hip"), encoding="utf-8").read()
    assert '#include "ocean_phase.h"' in kernels
    for call in ("phase_in_range(", "fused_advance_pair(", "advance_phase(", "sincos_phase(", "sincos_phase_pair_poly("):
        assert call in kernels, call
    for copy in ("fmodf(", "1.57079637050628662109375f", "4.37113900018624283e-8f", ">= 6.2831855f", "< 6.2831855f"):
        assert copy not in kernels, copy
    assert "dt_fusable(" in host and "dt_keeps_range(" in host
    for copy in ("< 6.0f", ">= 0.0f)"):
        assert copy not in host, copy


def test_fused_advance_is_fmod_on_random_pairs(emul):
    # 1.2e7 pairs over the admitted range, in four distributions: both uniform; small steps (a frame's w is far below 2 pi); phases
    # crowded against 2 pi; sums crowded around 2 pi
    rng = np.random.default_rng(20251)
    n = 3_000_000
    total = 0
    for what in ("uniform", "small w", "phase near 2 pi", "sum near 2 pi"):
        phase = (rng.random(n) * float(TWO_PI)).astype(F)
        w = (rng.random(n) * float(TWO_PI)).astype(F)
        if what == "small w":
            w = np.exp(rng.uniform(np.log(1e-30), np.log(6.0), n)).astype(F)
        elif what == "phase near 2 pi":
            phase = (float(TWO_PI) - np.exp(rng.uniform(np.log(1e-7), np.log(1.0), n))).astype(F)
        elif what == "sum near 2 pi":
            w = (TWO_PI - phase + (rng.integers(-40, 41, n) * 4.7683716e-7).astype(F)).astype(F)
        phase = np.minimum(phase, BELOW)
        w = np.clip(w, F(0), BELOW)
        assert _inside(emul, phase).all() and _inside(emul, w).all()
        fused, general = _advance(emul, phase, w)
        want = _fmod64(phase, w)
        assert np.array_equal(_bits(general), _bits(want)), what
        bad = np.flatnonzero(_bits(fused) != _bits(want))
        assert bad.size == 0, (what, phase[bad[:4]], w[bad[:4]], fused[bad[:4]], want[bad[:4]])
        assert _inside(emul, fused).all(), what                 # ... and the next fused step may take it
        total += n
    assert total >= 10_000_000


def test_fused_advance_is_fmod_on_every_edge(emul):
    phases = [F(0), F(-0.0), TINY, BELOW, F(1e-30), F(1.0), F(3.1415927), F(6.0)] + _neighbours(F(0.28318548), 2)
    ws = [F(0), F(-0.0), TINY, F(1e-30)] + _neighbours(F(6.0), 1) + [BELOW, F(3.1415927)]
    # sums within 2 ulp of 2 pi: w = target - phase and its neighbours, for every phase above
    for p in list(phases):
        for t in _neighbours(TWO_PI, 2):
            w = F(t) - F(p)
            ws += [x for x in _neighbours(w, 2) if F(0) <= x < TWO_PI]
    ws = sorted(set(float(x) for x in ws)) + [-0.0]
    pp, ww = np.meshgrid(np.array(phases, F), np.array(ws, F), indexing="ij")
    pp, ww = pp.ravel(), ww.ravel()
    assert _inside(emul, pp).all() and _inside(emul, ww).all()
    fused, general = _advance(emul, pp, ww)
    want = _fmod64(pp, ww)
    sums = pp + ww
    assert (sums == TWO_PI).sum() >= 8 and (sums == BELOW).sum() >= 8 and (sums > TWO_PI).sum() >= 8      # the select's own edge is in
    assert np.array_equal(_bits(general), _bits(want))
    bad = np.flatnonzero(_bits(fused) != _bits(want))
    assert bad.size == 0, (pp[bad[:4]], ww[bad[:4]], fused[bad[:4]], want[bad[:4]])
    # a fused step from -0.0 in particular (the predicate admits it)
    z = np.full(len(ws), -0.0, F)
    fused, _ = _advance(emul, z, np.array(ws, F))
    assert np.array_equal(_bits(fused), _bits(_fmod64(z, np.array(ws, F))))


def test_range_predicate(emul):
    inside = [F(0), F(-0.0), TINY, F(1.0), BELOW]
    outside = [TWO_PI, np.nextafter(TWO_PI, F(np.inf)), -TINY, F(-1e-30), F(-1.0), F(20.0), F(np.nan), F(np.inf), F(-np.inf)]
    assert _inside(emul, np.array(inside, F)).all()
    assert not _inside(emul, np.array(outside, F)).any()
    # the predicate is needed: from outside it the fused advance is not fmod
    fused, general = _advance(emul, np.array([20.0, -1.0], F), np.array([0.5, 0.25], F))
    assert not np.array_equal(_bits(fused), _bits(general))
    assert np.array_equal(_bits(general), _bits(_fmod64(np.array([20.0, -1.0], F), np.array([0.5, 0.25], F))))


def test_general_advance_is_fmod_anywhere(emul):
    # advance_phase takes any operands: negative and large ones, the sign of the sum kept as fmod keeps it
    rng = np.random.default_rng(20252)
    n = 2_000_000
    phase = rng.uniform(-1e4, 1e4, n).astype(F)
    w = (rng.uniform(-50, 50, n) * np.exp(rng.uniform(-20, 3, n))).astype(F)
    _, general = _advance(emul, phase, w)
    assert np.array_equal(_bits(general), _bits(_fmod64(phase, w)))
    assert (general < 0).any() and (general > 0).any()


def _sincos(emul, x):
    x = np.ascontiguousarray(x, F)
    assert x.size % 2 == 0
    out = [np.empty_like(x) for _ in range(4)]
    emul.phase_sincos(x.ctypes.data, x.size, *(o.ctypes.data for o in out))
    return out


def test_polynomial_sincos_against_float64(emul):
    rng = np.random.default_rng(20253)
    x = [rng.uniform(-1e4, 1e4, 4_000_000).astype(F), rng.uniform(0, float(TWO_PI), 1_000_000).astype(F),
         rng.uniform(-10, 21.4, 1_000_000).astype(F), np.array([0.0, -0.0, 1e4, -1e4, float(BELOW), float(TWO_PI)], F)]
    # every fp32 neighbour (+-2 ulp) of k pi/2, |k| <= 6400: where the reduction cancels most and the quadrant changes
    k = np.arange(-6400, 6401, dtype=np.float64)
    centre = (k * (np.pi / 2)).astype(F)
    lo, hi = centre, centre
    near = [centre]
    for _ in range(2):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        near += [lo, hi]
    near = np.concatenate(near)
    assert near.size == 5 * 12801 and float(np.abs(near).max()) > 1e4
    x = np.concatenate(x + [near])
    if x.size % 2:
        x = np.concatenate([x, x[:1]])
    sn, cs, sn2, cs2 = _sincos(emul, x)
    assert np.array_equal(_bits(sn), _bits(sn2)) and np.array_equal(_bits(cs), _bits(cs2))      # scalar and packed form
    x64 = x.astype(np.float64)
    es = float(np.abs(sn.astype(np.float64) - np.sin(x64)).max())
    ec = float(np.abs(cs.astype(np.float64) - np.cos(x64)).max())
    print(f"sincos_phase over |x| <= 1e4, {x.size} arguments: max |sin error| {es:.3e}, max |cos error| {ec:.3e} (bar {SINCOS_BAR:.3e})")
    assert max(es, ec) <= 4 * 2.0 ** -24, (es, ec)              # beyond this the reduction is wrong, not the margin too small
    assert es <= SINCOS_BAR and ec <= SINCOS_BAR, (es, ec)
    assert max(es, ec) >= SINCOS_MEASURED / 2, (es, ec)         # the constant above is what this test measures
    # |sin|, |cos| <= 1 and sin^2 + cos^2 = 1 at fp32 precision, everywhere
    assert float(np.abs(sn).max()) <= 1.0 and float(np.abs(cs).max()) <= 1.0
    assert float(np.abs(sn.astype(np.float64) ** 2 + cs.astype(np.float64) ** 2 - 1).max()) < 4e-7


class Host:
    """the wild flags of a handle's cascades across displace calls (tests/cpu/phase_emul.cpp: phase_host_step)"""

    def __init__(self, emul, omegamax):
        self.emul = emul
        self.omegamax = np.array(omegamax, F)
        self.wild = np.zeros(len(omegamax), np.uint8)

    def new_state(self, c, wild=False):
        self.wild[c] = 1 if wild else 0

    def displace(self, dts):
        dt = np.array(dts, F)
        return bool(self.emul.phase_host_step(dt.ctypes.data, dt.size, self.omegamax.ctypes.data, self.wild.ctypes.data, self.wild.size))


def test_host_rules(emul):
    om = [F(20.0), F(300.0), F(3.0)]
    h = Host(emul, om)
    assert h.displace([1 / 60, 1 / 60]) and not h.wild.any()
    assert h.displace([]) and h.displace([0.0]) and h.displace([-0.0]) and not h.wild.any()
    # omegamax * dt < 6 for every cascade: the largest dispersion decides
    assert h.displace([0.0199]) and not h.displace([0.0201]) and not h.wild.any()       # too large a dt: general path, nobody wild
    assert h.displace([1 / 60])
    # the boundary itself, in fp32: the product as the host rounds it
    for c, o in enumerate(om):
        for dt in _neighbours(F(6.0) / o, 3):
            assert bool(emul.phase_dt_fusable(dt, o)) == bool(F(o * dt) < F(6.0)), (o, dt)
    # one negative dt makes every cascade wild, whatever comes with it
    assert not h.displace([1 / 60, -1e-6, 1 / 60]) and h.wild.all()
    # wild is cleared only by a new state: not by updates, not by a displace without one
    assert not h.displace([1 / 60]) and not h.displace([]) and h.wild.all()
    h.new_state(0)
    assert not h.displace([1 / 60]) and list(h.wild) == [0, 1, 1]
    h.new_state(1)
    h.new_state(2)
    assert h.displace([1 / 60]) and not h.wild.any()
    # an uploaded phase outside the range: that cascade alone, and the whole handle leaves the fused path
    h.new_state(1, wild=True)
    assert not h.displace([1 / 60]) and list(h.wild) == [0, 1, 0]
    assert not h.displace([])
    h.new_state(1)
    assert h.displace([])
    # a NaN dt is not fusable and leaves every cascade wild; an infinite one is not fusable
    assert not emul.phase_dt_fusable(F(np.nan), F(1.0)) and not emul.phase_dt_keeps_range(F(np.nan))
    assert not emul.phase_dt_fusable(F(np.inf), F(1.0)) and not emul.phase_dt_fusable(F(1.0), F(np.nan))
    assert not emul.phase_dt_fusable(F(-1e-45), F(1.0)) and emul.phase_dt_fusable(F(-0.0), F(1.0)) and emul.phase_dt_keeps_range(F(-0.0))
    assert not h.displace([float("nan")]) and h.wild.all()


def test_fusable_dt_keeps_the_fused_range(emul):
    # what the rule is for: with dt fusable against omegamax, every w = omega * dt of the table (omega <= omegamax) is inside [0, 2 pi)
    rng = np.random.default_rng(20254)
    n = 1_000_000
    omax = np.exp(rng.uniform(np.log(0.1), np.log(5000.0), n)).astype(F)
    dt = (F(6.0) / omax * rng.uniform(0.999999, 1.000001, n).astype(F)).astype(F)
    fus = np.array([emul.phase_dt_fusable(float(d), float(o)) for d, o in zip(dt[:20000], omax[:20000])], bool)
    assert fus.any() and not fus.all()
    assert np.array_equal(fus, (omax[:20000] * dt[:20000]) < F(6.0))
    omega = (omax * rng.random(n).astype(F)).astype(F)
    omega[::7] = omax[::7]
    ok = (omax * dt) < F(6.0)
    w = (omega * dt)[ok]
    assert _inside(emul, w).all() and float(w.max()) < 6.0
