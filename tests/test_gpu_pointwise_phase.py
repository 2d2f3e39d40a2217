"""The other side of the row pass's dispatch, pinned as tests/test_gpu_pointwise.py pins the fast one: the any-phase instantiations
(ocean_rowpass_kernel<N, H16, true, H0H>: the phase-only fmod kernel first, sin / cos by reduction and polynomials) pointwise against
the float64 reference of tests/ref64.py at every size and format, and the dispatch itself -- which uploads, dt's and resumed states put
a handle on which path, and that the stored phase is update_ocean's bit for bit on either.

The comparisons and the bars are test_gpu_pointwise's own (_check and its constants, imported, not copied): the polynomial sin / cos is
at least as accurate as the hardware's (tests/test_phase_emul.py: 9.2e-8 against 4.8e-7), so what holds the fast path holds this one.
Every case asserts the path it is on through the flag datum_ocean_park_state returns (1: a phase outside [0, 2 pi), the general path;
0: the fused one) and reports it with its measured worst values (tests/conftest.py: report); profiles/pointwise_phase_table.txt keeps them.
"""

import numpy as np
import pytest

from test_gpu_pointwise import DT, FORMS, _check, _state

pytestmark = pytest.mark.gpu

F = np.float32
TWO_PI = F(6.2831855)                       # the constant of ocean_phase.h
BELOW = np.nextafter(TWO_PI, F(0))          # the largest phase the fused path takes

SIZES = sorted({N for N, _, _ in FORMS})    # one store policy per size: the policy does not reach the row pass
STRIDE = 262144                             # threads of one sweep of ocean_phaserange_kernel (1024 workgroups of 256)


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


def _flag(torch, oc, c=0):
    """the path cascade c is on: the flag datum_ocean_park_state hands out (1 = its phase may lie outside [0, 2 pi))"""
    slot = torch.empty(oc.state_bytes(), dtype=torch.uint8, device="cuda:0")
    flag = oc.park_state(c, slot.data_ptr(), oc.state_bytes())
    oc.sync()
    del slot
    return flag


def _neighbours(x):
    x = F(x)
    return [np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))]


def _wild_phase(N, seed):
    return np.random.default_rng(seed).uniform(-10.0, 21.4, (N, N)).astype(F)


def _circle_phase(N, seed):
    """uniform over [0, 2 pi) with 0, -0.0, the largest phase inside and the fp32 neighbours of pi/2, pi and 3 pi/2 at scattered places"""
    rng = np.random.default_rng(seed)
    phase = np.minimum((rng.random((N, N)) * float(TWO_PI)).astype(F), BELOW)
    special = [F(0), F(-0.0), BELOW] + _neighbours(np.pi / 2) + _neighbours(np.pi) + _neighbours(3 * np.pi / 2)
    flat = phase.reshape(-1)
    at = rng.choice(flat.size, 4 * len(special), replace=False)
    for i, j in enumerate(at):
        flat[j] = special[i % len(special)]
    flat[0], flat[-1] = F(0), BELOW
    assert float(phase.min()) >= 0 and float(phase.max()) < float(TWO_PI)
    return phase


def _open(capi, oracle, N, fmt, policy="auto", cascades=1):
    p = oracle.EXAMPLE
    oc = capi.Ocean(N, cascades)
    oc.set_spectrum_format(fmt)
    oc.set_map_store_policy(policy)
    for c in range(cascades):
        oc.set_cascade(c, p["wavescale"], p["choppiness"])
    return oc


# a. the any-phase row pass behind the phase-only kernel, every size x every format
@pytest.mark.parametrize("fmt", ["fp32", "fp16", "fp16h0"])
@pytest.mark.parametrize("N", SIZES)
def test_any_phase_every_form(capi, oracle, report, torch, N, fmt):
    p = oracle.EXAMPLE
    wavescale, chop = p["wavescale"], p["choppiness"]
    h0 = _state(oracle, N, 1000 + N, wavescale)
    phase = _wild_phase(N, 5000 + N)
    assert float(phase.min()) < -9 and float(phase.max()) > 20
    with _open(capi, oracle, N, fmt) as oc:
        oc.upload_state(0, h0, phase)
        for _ in range(2):
            oc.update(DT)
            oc.displace()
            oracle.update(phase, wavescale, DT, mt=True)
        flag = _flag(torch, oc)
        assert flag == 1
        _check(capi, oracle, report, oc, 0, h0, wavescale, chop, fmt, f"phase a N={N:4d} {fmt:6s} uploaded in [-10, 21.4), flag {flag}", phase)


# b. large arguments: the reduction's whole claimed range, nothing queued
@pytest.mark.parametrize("fmt", ["fp32", "fp16h0"])
@pytest.mark.parametrize("N", [64, 1024, 4096])
def test_any_phase_large_arguments(capi, oracle, report, torch, N, fmt):
    p = oracle.EXAMPLE
    wavescale, chop = p["wavescale"], p["choppiness"]
    h0 = _state(oracle, N, 1000 + N, wavescale)
    phase = np.random.default_rng(6000 + N).uniform(-1e4, 1e4, (N, N)).astype(F)
    with _open(capi, oracle, N, fmt) as oc:
        oc.upload_state(0, h0, phase)
        oc.displace()
        flag = _flag(torch, oc)
        assert flag == 1
        # (_check asserts the stored phase against the uploaded one, bit for bit: untouched)
        _check(capi, oracle, report, oc, 0, h0, wavescale, chop, fmt, f"phase b N={N:4d} {fmt:6s} uploaded in [-1e4, 1e4], no update, flag {flag}", phase)


# c. the fast path over the whole circle (test_gpu_pointwise starts at phase 0 and stays in the first quadrant up to 1024^2)
@pytest.mark.parametrize("N,fmt", [(N, "fp32") for N in SIZES] + [(64, "fp16"), (1024, "fp16")])
def test_full_circle_on_the_fast_path(capi, oracle, report, torch, N, fmt):
    p = oracle.EXAMPLE
    wavescale, chop = p["wavescale"], p["choppiness"]
    h0 = _state(oracle, N, 1000 + N, wavescale)
    phase = _circle_phase(N, 7000 + N)
    with _open(capi, oracle, N, fmt) as oc:
        oc.upload_state(0, h0, phase)
        assert _flag(torch, oc) == 0
        for _ in range(2):
            oc.update(DT)
            oc.displace()
            oracle.update(phase, wavescale, DT, mt=True)
        flag = _flag(torch, oc)
        assert flag == 0
        _check(capi, oracle, report, oc, 0, h0, wavescale, chop, fmt, f"phase c N={N:4d} {fmt:6s} uploaded over [0, 2 pi), flag {flag}", phase)


# d. gone wild by a negative dt, at the large forms (16 points per thread, banded, sequential)
@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_wild_by_a_negative_dt(capi, oracle, report, torch, N, fmt):
    p = oracle.EXAMPLE
    wavescale, chop = p["wavescale"], p["choppiness"]
    h0 = _state(oracle, N, 1000 + N, wavescale)
    phase = np.zeros((N, N), F)
    with _open(capi, oracle, N, fmt) as oc:
        oc.upload_state(0, h0)
        assert _flag(torch, oc) == 0
        for dt in (DT, F(-0.1), DT):
            oc.update(dt)
            oc.displace()
            oracle.update(phase, wavescale, dt, mt=True)
        assert float(phase.min()) < 0                           # the negative dt really left phases below zero
        flag = _flag(torch, oc)
        assert flag == 1
        _check(capi, oracle, report, oc, 0, h0, wavescale, chop, fmt, f"phase d N={N:4d} {fmt:6s} from 0 by dt 1/60, -0.1, 1/60, flag {flag}", phase)


# e. one wild cascade in a grouped handle: the whole launch plan goes over, the in-range cascades with it
@pytest.mark.parametrize("N,C,fmt,group,others", [(1024, 6, "fp16", 4, (3, 5)), (256, 5, "fp32", 2, (0, 4))])
def test_one_wild_cascade_in_a_grouped_handle(capi, oracle, report, torch, N, C, fmt, group, others):
    p = oracle.EXAMPLE
    ws = [22.0 * 2.2 ** c for c in range(C)]
    h0 = [_state(oracle, N, 3000 + c, ws[c]) for c in range(C)]
    phases = [np.zeros((N, N), F) for _ in range(C)]
    phases[1] = _wild_phase(N, 8000 + N)
    with capi.Ocean(N, C) as oc:
        oc.set_spectrum_format(fmt)
        oc.set_cascade_group(group)
        for c in range(C):
            oc.set_cascade(c, ws[c], p["choppiness"])
            oc.upload_state(c, h0[c], phases[c] if c == 1 else None)
        assert oc.cascade_group()[1] > 1
        for _ in range(2):
            oc.update(DT)
            oc.displace()
            for c in range(C):
                oracle.update(phases[c], ws[c], DT)
        flags = [_flag(torch, oc, c) for c in range(C)]
        assert flags == [1 if c == 1 else 0 for c in range(C)]
        for c in (1,) + tuple(others):
            _check(capi, oracle, report, oc, c, h0[c], ws[c], p["choppiness"], fmt,
                   f"phase e N={N:4d} {fmt:6s} {C} cascades, group {group}, cascade 1 wild, cascade {c}, flag {flags[c]}", phases[c])


# f. detection: one element outside [0, 2 pi), wherever it lies
@pytest.mark.parametrize("N", [64, 1024, 4096])
def test_one_element_out_of_range_is_found(capi, oracle, report, torch, N):
    p = oracle.EXAMPLE
    wavescale = p["wavescale"]
    rng = np.random.default_rng(9000 + N)
    h0 = (rng.standard_normal((N, N, 2)) * 1e-3).astype(F)
    base = np.minimum((rng.random((N, N)) * float(TWO_PI)).astype(F), BELOW)
    places = [(0, 0), (N - 1, N - 1), (N // 2, N // 2)]
    if N * N > STRIDE:
        i = (N * N // STRIDE - 1) * STRIDE - 1                  # the last thread of the kernel's last sweep but one ...
        j = 2 * STRIDE - 1                                      # ... and of its second
        assert i >= STRIDE and i % STRIDE == STRIDE - 1 and j % STRIDE == STRIDE - 1
        places += [divmod(i, N), divmod(j, N)]
    values = [TWO_PI, F(-1e-30), F(20.0), F(np.nan)]
    with _open(capi, oracle, N, "fp32") as oc:
        oc.upload_state(0, h0, base)
        assert _flag(torch, oc) == 0                            # the same array without the replacement
        found = 0
        for y, x in places:
            for v in values:
                phase = base.copy()
                phase[y, x] = v
                oc.upload_state(0, h0, phase)
                assert _flag(torch, oc) == 1, (y, x, v)
                for _ in range(3):
                    oc.update(DT)
                    oracle.update(phase, wavescale, DT, mt=True)
                oc.displace()
                got = oc.read_state(0)
                if np.isnan(v):
                    assert np.isnan(got[y, x]) and np.isnan(phase[y, x]), (y, x)
                    got[y, x] = phase[y, x] = 0
                assert np.array_equal(got.view(np.uint32), phase.view(np.uint32)), (y, x, v)
                assert _flag(torch, oc) == 1, (y, x, v)
                found += 1
        oc.upload_state(0, h0, base)
        assert _flag(torch, oc) == 0                            # ... and back
    report(f"phase f N={N:4d} one element of {{2 pi, -1e-30, 20, NaN}} at {len(places)} places: {found} of {found} uploads flag 1, phase bit-exact after 3 updates; without it flag 0")


def _run3(oc, oracle, phase, wavescale):
    for _ in range(3):
        oc.update(DT)
        oracle.update(phase, wavescale, DT, mt=True)
    oc.displace()


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# g. back to the fast path: a new in-range state, by upload or by resume with flag 0, runs the fused kernels again
@pytest.mark.parametrize("N,fmt", [(256, "fp32"), (1024, "fp16")])
def test_back_to_the_fast_path(capi, oracle, report, torch, N, fmt):
    p = oracle.EXAMPLE
    wavescale, chop = p["wavescale"], p["choppiness"]
    h0 = _state(oracle, N, 1000 + N, wavescale)
    s = _circle_phase(N, 7100 + N)
    nbytes = 12 * N * N

    # B: fresh, the in-range state S
    want = s.copy()
    with _open(capi, oracle, N, fmt) as ob:
        ob.upload_state(0, h0, s)
        _run3(ob, oracle, want, wavescale)
        assert _flag(torch, ob) == 0
        maps_b, phase_b = ob.read_maps(0), ob.read_state(0)
    assert np.array_equal(phase_b, want)

    # A: wild first, then S uploaded over it
    with _open(capi, oracle, N, fmt) as oa:
        oa.upload_state(0, h0, _wild_phase(N, 5000 + N))
        oa.update(DT)
        oa.displace()
        assert _flag(torch, oa) == 1
        oa.upload_state(0, h0, s)
        assert _flag(torch, oa) == 0
        _run3(oa, oracle, s.copy(), wavescale)
        assert _flag(torch, oa) == 0
        assert _same_bits(oa.read_maps(0), maps_b) and _same_bits(oa.read_state(0), phase_b)

    # D: S parked (flag 0), the handle wild meanwhile, S resumed with its flag
    with _open(capi, oracle, N, fmt) as od:
        slot = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        od.upload_state(0, h0, s)
        f = od.park_state(0, slot.data_ptr(), nbytes)
        assert f == 0
        od.upload_state(0, h0, _wild_phase(N, 5001 + N))
        od.update(F(-0.05))
        od.displace()
        assert _flag(torch, od) == 1
        od.resume_state(0, slot.data_ptr(), nbytes, f)
        assert _flag(torch, od) == 0
        _run3(od, oracle, s.copy(), wavescale)
        assert _flag(torch, od) == 0
        assert _same_bits(od.read_maps(0), maps_b) and _same_bits(od.read_state(0), phase_b)

    # C: a wild state parked and resumed with its flag into ANOTHER cascade of a handle that is otherwise in range: the general path
    w = _wild_phase(N, 5002 + N)
    with _open(capi, oracle, N, fmt, cascades=2) as oc:
        slot = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        oc.upload_state(0, h0, w)
        oc.upload_state(1, h0, s)
        oc.update(DT)
        oc.displace()
        oracle.update(w, wavescale, DT, mt=True)
        f = oc.park_state(0, slot.data_ptr(), nbytes)
        assert f == 1 and _flag(torch, oc, 1) == 0
        oc.upload_state(0, h0, s)                               # nobody wild now
        assert [_flag(torch, oc, c) for c in (0, 1)] == [0, 0]
        oc.resume_state(1, slot.data_ptr(), nbytes, f)
        assert [_flag(torch, oc, c) for c in (0, 1)] == [0, 1]
        oc.update(DT)
        oc.displace()
        oracle.update(w, wavescale, DT, mt=True)
        flag = _flag(torch, oc, 1)
        assert flag == 1
        _check(capi, oracle, report, oc, 1, h0, wavescale, chop, fmt, f"phase g N={N:4d} {fmt:6s} wild state resumed into cascade 1, flag {flag}", w)
    report(f"phase g N={N:4d} {fmt:6s} in-range state over a wild one (upload; resume with flag 0): flag 0, maps and phase bit-equal to a fresh handle's")


def _omega_corner(N, wavescale):
    """the largest dispersion of a cascade in fp32, as ocean_capi.hip forms it (ensure_omega: omegamax)"""
    kc = (F(6.2831855) * (F(0.5) * F(N))) / F(wavescale)
    k2 = kc * kc + kc * kc
    return np.sqrt((F(9.81) * np.sqrt(k2)) * (F(1.0) + k2 / F(136900.0)))


# h. the dispatch's boundaries, phase only: queue lengths around MAX_PENDING and dt's around the fusable threshold
@pytest.mark.parametrize("every", [1, 0])
@pytest.mark.parametrize("N", [64, 1024, 2048, 4096])
def test_dispatch_boundaries_keep_the_phase_bit_exact(capi, oracle, report, torch, N, every):
    p = oracle.EXAMPLE
    wavescale = p["wavescale"]
    rng = np.random.default_rng(9500 + N)
    h0 = (rng.standard_normal((N, N, 2)) * 1e-3).astype(F)
    base = _circle_phase(N, 7200 + N)
    assert (base.view(np.uint32) == 0x80000000).any() and (base == BELOW).any() and (base.view(np.uint32) == 0).any()
    om = _omega_corner(N, wavescale)
    assert om.dtype == F
    edge = [F(F(6.0) / om * F(1.0 + j * 2.0 ** -20)) for j in range(-2, 3)]
    fus = [bool(F(om * dt) < F(6.0)) for dt in edge]
    assert fus[0] and not fus[-1], fus                          # they straddle the host's threshold
    runs = 0
    with _open(capi, oracle, N, "fp32") as oc:
        oc.set_phase_writeback(every)
        for queued in (8, 9, 16, 17):
            phase = base.copy()
            oc.upload_state(0, h0, phase)
            for i in range(queued):
                dt = F(DT * F(1 + 0.03 * i))
                oc.update(dt)
                oracle.update(phase, wavescale, dt, mt=True)
            oc.displace()
            assert _same_bits(oc.read_state(0), phase), (queued, every)
            assert _flag(torch, oc) == 0
            runs += 1
        # each threshold dt decides a displace call of its own, an ordinary step in between
        phase = base.copy()
        oc.upload_state(0, h0, phase)
        for dt in edge:
            for d in (dt, DT):
                oc.update(d)
                oc.displace()
                oracle.update(phase, wavescale, d, mt=True)
        assert _same_bits(oc.read_state(0), phase), ("threshold", every)
        assert _flag(torch, oc) == 0
        # ... and all five queued for one call
        for dt in edge:
            oc.update(dt)
            oracle.update(phase, wavescale, dt, mt=True)
        oc.displace()
        assert _same_bits(oc.read_state(0), phase), ("threshold, queued", every)
        assert _flag(torch, oc) == 0
        interval = oc.phase_writeback()
    report(f"phase h N={N:4d} write-back every {interval}: 8 / 9 / 16 / 17 queued updates and dt = 6 / {float(om):.6g} * (1 + j 2^-20), j = -2 .. 2 "
           f"(fusable {''.join('y' if f else 'n' for f in fus)}): phase bit-exact in {runs + 2} of {runs + 2} runs, flag 0")
