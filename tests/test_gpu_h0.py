"""The device-side spectrum build (datum_ocean_upload_seed / datum_ocean_rebuild_height / datum_ocean_read_height; ocean_kernels.hip:
ocean_height_kernel) point by point against tests/h064.py's interval walk of the kernel's own expression.

  * intervals      every case of h064.CASES: each component of h0 within [lo, hi] times the seed's component (one more rounding, the 2^-149
                   floor), exactly 0 where hi == 0, the seed's sign (a zero product's too), everything finite; the seed is random normal
                   with 0, -0.0, 1e30 and 1e-30 planted.  The 4096^2 case compares 64 rows.  The rules of the walk: h064's docstring
                   (each + - * / sqrt one eps = 2^-24, expf 3 ulp, a subnormal kept or flushed at every operation, d = [0.2, 1] where
                   the sign of kdotw is open, dk, kx, ky and the wind's scalars exact float32 inputs)
  * known zeros    the centre; column N/2 of case C; windspeed = 0; waveamplitude = 0; a cascade whose seed was never uploaded
  * independence   one NaN in the seed is one NaN in h0 and no other bit moves; a second rebuild gives the same bits; rebuilding cascade 1
                   of three leaves cascades 0 and 2 alone (h0, phase, the maps of the next step)
  * installed = read   in every spectrum format a handle given read_height() through upload_state / upload_height steps bit for bit as
                   the handle that rebuilt on the device, also after a second rebuild (a stale fp16 scale or half copy of h0 shows here)
  * arguments      a refused call (include/datum_ocean_hip.h: datum_ocean_rebuild_height) changes nothing

Measured on the MI355X, the largest |got / seed - mid| / (hi - lo) per case (1/2 would be an end of the interval):
  A 0.363   B 0.341   C 0.192   D 0.439   E 0.427   F 0.459   H 0.382      no component outside, at the first run of the unchanged kernel
(the oracle's float32 gives 0.363 0.340 0.192 0.439 0.427 0.459 0.382: tests/h064.py has the table of shares and widths per case).
"""

import numpy as np
import pytest

import h064

pytestmark = pytest.mark.gpu

F = np.float32
DT = F(1.0 / 60.0)
CHOP = 1.35


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rows(a, name):
    rows = h064.case_rows(name)
    return a if rows is None else a[rows]


def _args(name):
    N, ws, a, v, wx, wy = h064.case_args(name)
    return N, (ws, a, v, (wx, wy))


def _seed(N, rngseed):
    return np.random.RandomState(rngseed).standard_normal((N, N, 2)).astype(F)


# 1 -- intervals

@pytest.mark.parametrize("name", tuple(h064.CASES))
def test_every_point_inside_its_interval(capi, report, name):
    N, args = _args(name)
    lo, hi, mid, _ = h064.case_walk(name)
    seed = h064.case_seed(name)
    with capi.Ocean(N, 1) as oc:
        oc.upload_seed(0, seed)
        oc.rebuild_height(0, *args)
        got = oc.read_height(0)
    assert np.isfinite(got).all()
    assert np.all(_bits(got[N // 2, N // 2]) == _bits(seed[N // 2, N // 2]) & 0x80000000)        # the centre: zero, with the seed's sign
    g, s = _rows(got, name), _rows(seed, name)
    r = h064.ratio(g, s, lo, hi, mid)
    bad = h064.outside(g, s, lo, hi)
    line = f"h0 intervals {name} N={N}: {g.size} components, outside {int(bad.sum())}, largest (got - mid) / (hi - lo) {r:.3f}"
    print(line)
    report(line)
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:8].tolist())
    assert np.all(g[hi == 0] == 0)


# 2 -- known zeros

def test_known_zeros(capi):
    N, args = _args("C")
    seed = h064.case_seed("C")
    with capi.Ocean(N, 2) as oc:
        oc.upload_seed(1, seed)
        oc.rebuild_height(1, *args)
        got = oc.read_height(1)
        assert np.all(got[:, N // 2] == 0) and np.all(got[N // 2, N // 2] == 0)
        assert np.count_nonzero(got) > N * N                  # and the plane is not empty
        ws, a, v, w = args
        oc.rebuild_height(1, ws, a, F(0), w)
        assert np.all(oc.read_height(1) == 0)
        oc.rebuild_height(1, ws, F(0), v, w)
        assert np.all(oc.read_height(1) == 0)
        oc.rebuild_height(1, *_args("A")[1])
        assert np.count_nonzero(oc.read_height(1)) > N * N
        # cascade 0's seed was never uploaded: the buffer is zero-filled
        oc.rebuild_height(0, *_args("A")[1])
        assert np.all(_bits(oc.read_height(0)) == 0)


# 3 -- independence

def test_one_nan_in_the_seed_is_one_nan_in_h0(capi):
    N, args = _args("B")
    seed = _seed(N, 7)
    poisoned = seed.copy()
    poisoned[17, 201, 0] = np.nan
    poisoned[N // 2 + 1, 3, :] = np.nan
    with capi.Ocean(N, 1) as oc:
        oc.upload_seed(0, seed)
        oc.rebuild_height(0, *args)
        clean = oc.read_height(0)
        oc.rebuild_height(0, *args)
        assert _same(oc.read_height(0), clean)                 # the same arguments, the same bits
        oc.upload_seed(0, poisoned)
        oc.rebuild_height(0, *args)
        got = oc.read_height(0)
    assert np.array_equal(np.isnan(got), np.isnan(poisoned)) and np.isnan(got).sum() == 3
    assert np.array_equal(_bits(got)[~np.isnan(poisoned)], _bits(clean)[~np.isnan(poisoned)])


def test_rebuilding_one_cascade_leaves_the_others(capi):
    N = 64
    first = [(22.0, 0.0025, 7.9, (0.780869, 0.624695)), (64.0, 0.001, 9.0, (0.6, 0.8)), (176.0, 0.0005, 11.0, (0.0, 1.0))]

    def make():
        oc = capi.Ocean(N, 3)
        for c, a in enumerate(first):
            oc.set_cascade(c, a[0], CHOP)
            oc.upload_seed(c, _seed(N, 30 + c))
            oc.rebuild_height(c, *a)
        oc.update(DT)
        oc.displace()
        oc.update(DT)               # queued when cascade 1 is rebuilt
        return oc

    with make() as x, make() as y:
        x.rebuild_height(1, 40.0, 0.002, 14.0, (-0.8, 0.6))
        for c in (0, 2):
            assert _same(x.read_height(c), y.read_height(c)) and _same(x.read_state(c), y.read_state(c))
        assert not _same(x.read_height(1), y.read_height(1))
        for oc in (x, y):
            oc.update(DT)
            oc.displace()
        for c in (0, 2):
            assert _same(x.read_maps(c), y.read_maps(c)) and _same(x.read_state(c), y.read_state(c)) and _same(x.read_height(c), y.read_height(c))
        assert not _same(x.read_maps(1), y.read_maps(1))


# 4 -- what is installed is what is read

@pytest.mark.parametrize("fmt", ["fp32", "fp16", "fp16h0"])
@pytest.mark.parametrize("how", ["upload_state", "upload_height"])
def test_a_read_height_installed_elsewhere_steps_the_same(capi, fmt, how):
    N = 256
    seed = _seed(N, 11)
    one, two = _args("B")[1], (5.0, 1e-6, 21.0, (-0.28, 0.96))

    def steps():
        for _ in range(2):
            for oc in (x, y):
                oc.update(DT)
                oc.displace()
        assert _same(x.read_maps(0), y.read_maps(0)) and _same(x.read_state(0), y.read_state(0))
        assert np.isfinite(x.read_maps(0)).all() and float(np.abs(x.read_maps(0)[0]).max()) > 0

    with capi.Ocean(N, 1) as x, capi.Ocean(N, 1) as y:
        for oc in (x, y):
            oc.set_spectrum_format(fmt)
            oc.set_cascade(0, 22.0, CHOP)
        x.upload_seed(0, seed)
        x.rebuild_height(0, *one)
        y.set_cascade(0, one[0], CHOP)
        y.upload_state(0, x.read_height(0))
        steps()
        large = float(np.abs(x.read_height(0)).max())
        # the second rebuild's h0 is smaller by orders of magnitude (by the parameters: 1.5e-3) and under another wave scale
        x.rebuild_height(0, *two)
        y.set_cascade(0, two[0], CHOP)
        if how == "upload_height":
            y.upload_height(0, x.read_height(0))
        else:
            y.upload_state(0, x.read_height(0), x.read_state(0))
        assert 0 < float(np.abs(x.read_height(0)).max()) < 1e-2 * large
        steps()


# 5 -- arguments

def test_a_refused_rebuild_changes_nothing(capi):
    N = 64
    good = _args("A")[1]

    def make():
        oc = capi.Ocean(N, 2)
        for c in range(2):
            oc.set_cascade(c, good[0], CHOP)
            oc.upload_seed(c, _seed(N, 50 + c))
            oc.rebuild_height(c, *good)
        oc.update(DT)
        oc.displace()
        oc.update(DT)               # queued: a wave scale installed by a refused call would flush it under the wrong dispersion
        return oc

    nan, inf = F(np.nan), F(np.inf)
    ws = 30.0                       # a new wave scale in every refused call
    refused = [(0, ws, nan, 7.9, (0.6, 0.8)), (0, ws, inf, 7.9, (0.6, 0.8)), (0, ws, -0.001, 7.9, (0.6, 0.8)),
               (1, ws, 0.0025, nan, (0.6, 0.8)), (1, ws, 0.0025, -inf, (0.6, 0.8)), (0, ws, 0.0025, 7.9, (nan, 0.8)), (0, ws, 0.0025, 7.9, (0.6, inf)),
               (0, 0.0, 0.0025, 7.9, (0.6, 0.8)), (1, -ws, 0.0025, 7.9, (0.6, 0.8)), (0, nan, 0.0025, 7.9, (0.6, 0.8)),
               (-1, ws, 0.0025, 7.9, (0.6, 0.8)), (2, ws, 0.0025, 7.9, (0.6, 0.8))]

    with make() as x, make() as y:
        before = x.cascade_group(), [x.read_height(c) for c in range(2)]
        for call in refused:
            with pytest.raises(capi.OceanError) as e:
                x.rebuild_height(*call)
            assert e.value.code == capi.EINVAL and "datum_ocean_rebuild_height" in str(e.value), call
        assert x.cascade_group() == before[0] == y.cascade_group()
        for c in range(2):
            assert _same(x.read_height(c), before[1][c]) and _same(x.read_height(c), y.read_height(c))
            assert np.isfinite(x.read_height(c)).all()
        for oc in (x, y):
            oc.update(DT)
            oc.displace()
        for c in range(2):
            assert _same(x.read_state(c), y.read_state(c)) and _same(x.read_maps(c), y.read_maps(c))
            assert np.isfinite(x.read_maps(c)).all()

    # no seed on the device: ESTATE, whatever else the call asks for
    with capi.Ocean(N, 1) as oc:
        for call in [(0,) + good, (0, ws, nan, 7.9, (0.6, 0.8))]:
            with pytest.raises(capi.OceanError) as e:
                oc.rebuild_height(*call)
            assert e.value.code == capi.ESTATE and "datum_ocean_rebuild_height" in str(e.value)
