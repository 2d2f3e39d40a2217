"""The phase's quadrant table (include/datum_ocean_hip.h: datum_ocean_set_phase_store; datum_amd/csrc/ocean_quadrant.h) changes nothing a
caller can see.

Every case drives two handles in lockstep through the same calls on the same seeds -- one in the automatic mode, which keeps a symmetric
cascade's phase as an (N/2 + 1)^2 table and lets the row pass read it there, one held to the plane as builds before the table were -- and
compares BIT FOR BIT, no tolerance, after every step: the maps (the handles' map blocks, bound to torch tensors, torch.equal), the
downloaded phase and the foam plane (numpy.array_equal).  The arithmetic is the same instructions on the same values; only the array they
are loaded from differs.  Each case also asserts, through datum_ocean_phase_store, which row pass ran."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
FORMATS = ["fp32", "fp16", "fp16h0"]
STARTS = ["zero", "symmetric", "asymmetric"]


@functools.lru_cache(maxsize=None)
def _h0(N, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((N, N, 2)) * 1e-3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _phase(N, seed, start):
    """None (zero), a non-zero phase in [0, 2 pi) that is a function of (|y - N/2|, |x - N/2|), or the same with one element's lowest bit flipped"""
    if start == "zero":
        return None
    rs = np.random.RandomState(seed)
    q = rs.uniform(0.0, 6.28, (N // 2 + 1, N // 2 + 1)).astype(np.float32)
    i = np.abs(np.arange(N) - N // 2)
    phase = np.ascontiguousarray(q[np.ix_(i, i)])
    if start == "asymmetric":
        phase.view(np.uint32)[N // 2 + 3, 5] ^= np.uint32(1)
    return phase


class Pair:
    """`auto` and `plane`, two handles given the same calls"""

    def __init__(self, N, cascades=2, fmt="fp32", every=None, starts=("zero", "zero"), foam="accumulate"):
        import torch

        from datum_amd import capi

        self.torch = torch
        self.N, self.cascades = N, cascades
        self.auto = capi.Ocean(N, cascades)
        self.plane = capi.Ocean(N, cascades)
        self.plane.set_phase_store("plane")
        assert self.auto.phase_store() == ("auto", (1 << cascades) - 1)        # a new handle's zero phase lives in the tables
        assert self.plane.phase_store() == ("plane", 0)
        self.tensors = []
        for oc in (self.auto, self.plane):
            oc.set_spectrum_format(fmt)
            if every is not None:
                oc.set_phase_writeback(every)
            for c in range(cascades):
                oc.set_cascade(c, 64.0 + 23.0 * c, 1.35)                       # two wave scales: two dispersion tables
                oc.upload_state(c, _h0(N, 100 + c), _phase(N, 200 + c, starts[c % len(starts)]))
            if foam:
                oc.set_foam(foam)
            _, nbytes = oc.maps_device()
            t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            oc.bind_maps(t.data_ptr(), nbytes)
            self.tensors.append(t)
        self.foam = foam
        self.all = (1 << cascades) - 1

    def both(self, fn):
        fn(self.auto)
        fn(self.plane)

    def close(self):
        self.both(lambda oc: oc.close())

    def quadrants(self):
        assert self.plane.phase_store() == ("plane", 0)
        mode, mask = self.auto.phase_store()
        assert mode == "auto"
        return mask

    def step(self, dts=(DT,), expect=None, phase=True):
        """queue the dt's, displace, compare every map, the downloaded phase and the foam plane; `expect`: the cascades in their tables afterwards
        (all of them: the row pass read the tables; anything else: it read the plane)"""
        for dt in dts:
            self.both(lambda oc: oc.update(dt))
        self.both(lambda oc: oc.displace())
        if expect is not None:
            assert self.quadrants() == expect
        self.both(lambda oc: oc.sync())
        assert self.torch.equal(self.tensors[0], self.tensors[1])
        if self.foam:
            for c in range(self.cascades):
                assert np.array_equal(self.auto.read_foam(c), self.plane.read_foam(c))
        if phase:
            self.check_phase()
        if expect is not None:
            assert self.quadrants() == expect                                  # a download leaves the truth where it was

    def check_phase(self):
        for c in range(self.cascades):
            a, b = self.auto.read_state(c), self.plane.read_state(c)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _expected(starts, cascades=2):
    return (1 << cascades) - 1 if "asymmetric" not in starts else 0


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("every", [1, 8])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024])
def test_lockstep_every_form_format_interval_and_start(N, fmt, every, start):
    starts = (start, "symmetric" if start == "asymmetric" else start)          # the asymmetric case: one such cascade beside a symmetric one
    p = Pair(N, 2, fmt, every, starts)
    try:
        want = _expected(starts)
        if start == "asymmetric":
            assert p.quadrants() == 0b10                                        # the upload's test told them apart; the first displace settles on the plane
        else:
            assert p.quadrants() == 0b11
        for n in (1, 1, 8, 1, 9, 0, 17, 1, 1):                                  # irregular queues: 1, 8, 9 and 17 pending
            p.step((DT,) * n, expect=want)
        assert bool(p.tensors[0].any())
    finally:
        p.close()


@pytest.mark.parametrize("N,fmt", [(2048, "fp32"), (4096, "fp16h0")])
def test_two_steps_at_the_large_sizes(N, fmt):
    p = Pair(N, 1, fmt, None, ("zero",), foam=None)
    try:
        p.step(expect=1, phase=False)
        p.step(expect=1)
    finally:
        p.close()


def _download(p, want):
    p.check_phase()
    assert p.quadrants() == want


def _park_and_adopt(p, want):
    slots = [p.torch.empty(p.auto.state_bytes(), dtype=p.torch.uint8, device="cuda:0") for _ in range(2)]
    flags = [oc.park_state(0, s.data_ptr(), oc.state_bytes()) for oc, s in zip((p.auto, p.plane), slots)]
    p.both(lambda oc: oc.sync())
    assert p.torch.equal(slots[0], slots[1])                                    # the parked h0 and phase themselves
    assert p.quadrants() == want
    p.both(lambda oc: oc.upload_state(0, _h0(p.N, 7), _phase(p.N, 8, "symmetric")))
    for _ in range(3):
        p.step(expect=want)
    for oc, s, f in zip((p.auto, p.plane), slots, flags):
        oc.resume_state(0, s.data_ptr(), oc.state_bytes(), f)
    assert p.quadrants() == want                                                # the adopted phase is as symmetric as the parked one was


def _velocity(p, want):
    p.both(lambda oc: oc.set_velocity("on"))
    for _ in range(2):
        p.step(expect=0)                                                        # the velocity passes read the stored plane in every step
        for c in range(p.cascades):
            assert np.array_equal(p.auto.read_velocity(c), p.plane.read_velocity(c))
    p.both(lambda oc: oc.set_velocity("off"))
    # a new state brings the cascades back to their tables
    for c in range(p.cascades):
        p.both(lambda oc: oc.upload_state(c, _h0(p.N, 100 + c), _phase(p.N, 300 + c, "symmetric")))
    assert p.quadrants() == p.all


def _upload_height(p, want):
    p.both(lambda oc: oc.upload_height(1, _h0(p.N, 11)))
    assert p.quadrants() == want


def _negative_dt_and_new_state(p, want):
    p.step((DT, -0.25), expect=0)                                               # wild: expanded, the row pass whose sin / cos take any phase
    p.step(expect=0)
    for c in range(p.cascades):
        p.both(lambda oc: oc.upload_state(c, _h0(p.N, 100 + c), _phase(p.N, 400 + c, "symmetric")))
    assert p.quadrants() == p.all
    p.step(expect=p.all)


def _mode_switch(p, want):
    p.auto.set_phase_store("plane")
    assert p.auto.phase_store() == ("plane", 0)
    p.both(lambda oc: oc.update(DT))
    p.both(lambda oc: oc.displace())
    p.both(lambda oc: oc.sync())
    assert p.torch.equal(p.tensors[0], p.tensors[1])
    p.auto.set_phase_store("auto")                                              # the planes are tested again and move back
    assert p.quadrants() == want


OPS = [_download, _park_and_adopt, _velocity, _upload_height, _negative_dt_and_new_state, _mode_switch]


@pytest.mark.parametrize("every", [1, 8])
@pytest.mark.parametrize("op", OPS, ids=[f.__name__.strip("_") for f in OPS])
def test_plane_touching_calls_in_the_middle_of_an_interval(op, every):
    p = Pair(256, 2, "fp32", every, ("symmetric", "zero"))
    try:
        for _ in range(3):
            p.step(expect=p.all, phase=False)                                   # three dt's retained at interval 8
        op(p, p.all)
        after = p.quadrants()
        for _ in range(10):
            p.step(expect=after)
        for _ in range(2):
            p.step(expect=after, phase=False)
        op(p, after)
        p.step((), expect=p.quadrants())
    finally:
        p.close()


def test_mixed_handle_takes_the_plane_and_returns_with_a_symmetric_state():
    p = Pair(128, 2, "fp32", None, ("symmetric", "asymmetric"))
    try:
        assert p.quadrants() == 0b01
        for _ in range(4):
            p.step(expect=0)
        p.both(lambda oc: oc.upload_state(1, _h0(128, 5), None))
        assert p.quadrants() == 0b10                                            # cascade 0 was expanded for good, cascade 1 is new
        p.step(expect=0)
        p.both(lambda oc: oc.upload_state(0, _h0(128, 6), _phase(128, 9, "symmetric")))
        assert p.quadrants() == 0b01                                            # ... and cascade 1 went to the plane with that displace
        p.both(lambda oc: oc.upload_state(1, _h0(128, 5), None))
        assert p.quadrants() == 0b11
        for _ in range(9):
            p.step(expect=0b11)
    finally:
        p.close()


def test_setter_getter_and_estate_under_an_open_profile():
    from datum_amd import capi

    with capi.Ocean(64, 1) as oc:
        assert oc.phase_store() == ("auto", 1)
        with pytest.raises(capi.OceanError) as e:
            oc.set_phase_store(2)
        assert e.value.code == capi.EINVAL
        oc.upload_state(0, np.zeros((64, 64, 2), np.float32))
        oc.profile_begin(4)
        with pytest.raises(capi.OceanError) as e:
            oc.set_phase_store("plane")
        assert e.value.code == capi.ESTATE
        oc.profile_end()
        oc.set_phase_store("plane")
        assert oc.phase_store() == ("plane", 0)
        oc.set_phase_store("auto")
        assert oc.phase_store() == ("auto", 1)
