"""The lazy phase write-back (include/datum_ocean_hip.h: datum_ocean_set_phase_writeback) changes nothing a caller can see.

Every case drives two handles through the same calls on the same seeds -- one at the interval under test (the module's default, 2, 4, 8),
one at interval 1, which stores the phase on every row pass as builds before the write-back did -- and compares BIT FOR BIT, no tolerance:
the maps after every displace (the handles' map blocks, bound to torch tensors, with torch.equal), the phase wherever it is read
(numpy.array_equal) and the foam plane.  The arithmetic is the same instructions in the same order; only the store moves."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
INTERVALS = [None, 2, 4, 8]          # None: the module's default


@functools.lru_cache(maxsize=None)
def _state(N, seed):
    # any finite h0 and any phase in [0, 2 pi) will do: the comparison is between two handles, not against a sea
    rs = np.random.RandomState(seed)
    h0 = (rs.standard_normal((N, N, 2)) * 1e-3).astype(np.float32)
    phase = rs.uniform(0.0, 6.28, (N, N)).astype(np.float32)
    return h0, phase


def _make_pair(N, cascades=1, every=None, fmt="fp32", foam=None, wildphase=False):
    import torch

    from datum_amd import capi

    pair = _Pair()
    pair.torch = torch
    pair.N, pair.cascades = N, cascades
    pair.lazy = capi.Ocean(N, cascades)
    pair.eager = capi.Ocean(N, cascades)
    if every is not None:
        pair.lazy.set_phase_writeback(every)
        assert pair.lazy.phase_writeback() == every
    else:
        assert 1 <= pair.lazy.phase_writeback() <= 8
    pair.every = pair.lazy.phase_writeback()
    pair.eager.set_phase_writeback(1)
    assert pair.eager.phase_writeback() == 1
    pair.tensors = []
    for oc in (pair.lazy, pair.eager):
        oc.set_spectrum_format(fmt)
        for c in range(cascades):
            h0, phase = _state(N, 100 + c)
            if wildphase:
                phase = (phase * 5.0 - 10.0).astype(np.float32)      # [-10, 21.4): outside [0, 2 pi) on either side
            oc.set_cascade(c, 64.0 + 23.0 * c, 1.35)
            oc.upload_state(c, h0, phase)
        if foam:
            oc.set_foam(foam)
        _, nbytes = oc.maps_device()
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        oc.bind_maps(t.data_ptr(), nbytes)
        pair.tensors.append(t)
    pair.foam = foam
    return pair


class _Pair:
    def both(self, fn):
        fn(self.lazy)
        fn(self.eager)

    def close(self):
        self.both(lambda oc: oc.close())

    def step(self, dts=(DT,)):
        """queue the dt's, displace, compare the maps (and the foam plane)"""
        for dt in dts:
            self.both(lambda oc: oc.update(dt))
        self.both(lambda oc: oc.displace())
        self.check_maps()

    def check_maps(self):
        self.both(lambda oc: oc.sync())
        assert self.torch.equal(self.tensors[0], self.tensors[1])
        if self.foam:
            for c in range(self.cascades):
                assert np.array_equal(self.lazy.read_foam(c), self.eager.read_foam(c))

    def check_phase(self):
        for c in range(self.cascades):
            assert np.array_equal(self.lazy.read_state(c), self.eager.read_state(c))


Pair = _make_pair


# the row-pass forms of DESIGN.md section 0
FORMS = [(64, 1, "fp32"), (512, 1, "fp32"), (1024, 4, "fp32"), (2048, 1, "fp32"), (4096, 1, "fp16h0")]


@pytest.mark.parametrize("every", INTERVALS)
@pytest.mark.parametrize("N,cascades,fmt", FORMS)
def test_maps_and_phase_every_step(N, cascades, fmt, every):
    p = Pair(N, cascades, every, fmt)
    try:
        k = p.lazy.phase_writeback()
        for _ in range(3):
            p.step()
        p.check_phase()                  # inside an interval of 4 or 8 (and of 2: steps 1 and 3 retain); the read brings the phase up to date
        for _ in range(k):
            p.step()
        p.check_phase()                  # on the boundary: the k-th row pass since the read has just stored
        for i in range(max(14, 20 - 3 - k)):
            p.step((DT * (1 + i % 3),))
        p.check_phase()
        assert bool(p.tensors[0].any())
    finally:
        p.close()


@pytest.mark.parametrize("every", INTERVALS)
def test_irregular_queues(every):
    # 0, 1, 3 and 9 updates between displaces (9: more than one row pass takes, the phase-only kernel first), two displaces in a row
    p = Pair(256, 2, every)
    try:
        for n in [1, 0, 3, 1, 9, 1, 1, 0, 0, 3, 1, 1, 9, 9, 1, 1, 1, 1, 1, 3, 3, 3, 1, 0, 1]:
            p.step((DT,) * n)
        p.check_phase()
        # 40 updates and no displace: datum_ocean_update itself flushes the oldest
        for _ in range(40):
            p.both(lambda oc: oc.update(DT))
        p.step(())
        for _ in range(9):
            p.step()
        p.check_phase()
    finally:
        p.close()


def _park_and_resume(p):
    slots = [p.torch.empty(p.lazy.state_bytes(), dtype=p.torch.uint8, device="cuda:0") for _ in range(2)]
    flags = [oc.park_state(0, s.data_ptr(), oc.state_bytes()) for oc, s in zip((p.lazy, p.eager), slots)]
    p.both(lambda oc: oc.sync())
    assert p.torch.equal(slots[0], slots[1])                # the parked h0 and phase themselves
    h0, phase = _state(p.N, 7)
    p.both(lambda oc: oc.upload_state(0, h0, phase))
    for _ in range(3):
        p.step()
    for oc, s, f in zip((p.lazy, p.eager), slots, flags):
        oc.resume_state(0, s.data_ptr(), oc.state_bytes(), f)


def _new_wavescale(p):
    p.both(lambda oc: oc.set_cascade(1, 41.0, 1.2))


def _upload_state(p):
    h0, phase = _state(p.N, 9)
    p.both(lambda oc: oc.upload_state(0, h0, phase))


def _literal_and_back(p):
    p.both(lambda oc: oc.set_literal_transform(True))
    p.step()
    p.step(())
    p.step((DT, DT))
    p.both(lambda oc: oc.set_literal_transform(False))


def _rebuild_height(p):
    rs = np.random.RandomState(5)
    seed = rs.standard_normal((p.N, p.N, 2)).astype(np.float32)
    p.both(lambda oc: oc.upload_seed(1, seed))
    p.both(lambda oc: oc.rebuild_height(1, 50.0, 2e-4, 12.0, (0.8, 0.6)))


def _spectrum_format(p):
    p.both(lambda oc: oc.set_spectrum_format("fp16"))
    p.step()
    p.step()
    p.both(lambda oc: oc.set_spectrum_format("fp32"))


def _debug_entry_points(p):
    for c in range(p.cascades):
        for x, y in zip(p.lazy.debug_rowpass(c), p.eager.debug_rowpass(c)):
            assert np.array_equal(x, y)
    for x, y in zip(p.lazy.debug_sim(1), p.eager.debug_sim(1)):
        assert np.array_equal(x, y)


def _large_dt(p):
    # omega dt beyond the fused advance's one subtraction (the table corner at 256^2 and wavescale 64 is 13 rad/s): the general kernel
    p.step((DT, 2.0))
    p.step((3.5,))


def _profile(p):
    p.both(lambda oc: oc.profile_begin(4))
    for _ in range(5):
        p.step()
    p.both(lambda oc: oc.profile_end())


def _lower_interval(p):
    # retained dt's meet a shorter interval: the next row pass stores them
    p.lazy.set_phase_writeback(2)
    p.step(())
    p.lazy.set_phase_writeback(p.every)


MID_INTERVAL = [lambda p: p.check_phase(), _park_and_resume, _new_wavescale, _upload_state, _literal_and_back, _rebuild_height, _spectrum_format,
                _debug_entry_points, _large_dt, _profile, _lower_interval]
MID_INTERVAL_IDS = ["read", "park_resume", "wavescale", "upload_state", "literal", "rebuild_height", "spectrum_format", "debug", "large_dt", "profile",
                    "lower_interval"]


@pytest.mark.parametrize("every", [None, 4, 8])
@pytest.mark.parametrize("op", MID_INTERVAL, ids=MID_INTERVAL_IDS)
def test_calls_in_the_middle_of_an_interval(op, every):
    p = Pair(256, 2, every)
    try:
        for _ in range(3):
            p.step()
        op(p)
        for _ in range(10):
            p.step()
        p.check_phase()
        for _ in range(2):
            p.step()
        op(p)
        p.step(())
        p.check_phase()
    finally:
        p.close()


@pytest.mark.parametrize("every", INTERVALS)
def test_change_of_cascade_group(every):
    # 1024^2 x 6 in groups of 3 and of 6, changed in the middle of an interval
    p = Pair(1024, 6, every)
    try:
        for group in (3, 6, 3, 0):
            p.both(lambda oc: oc.set_cascade_group(group))
            for _ in range(3):
                p.step()
        for _ in range(8):
            p.step()
        p.check_phase()
    finally:
        p.close()


@pytest.mark.parametrize("every", INTERVALS)
def test_phase_outside_the_range_and_large_dt(every):
    # a phase outside [0, 2 pi) uploaded: the row pass whose sin / cos take any argument, the phase advanced by the general kernel
    p = Pair(512, 1, every, wildphase=True)
    try:
        for _ in range(6):
            p.step()
        p.check_phase()
        # back in range, then dt's whose omega dt leaves the one-subtraction range, in the middle of an interval
        h0, phase = _state(512, 3)
        p.both(lambda oc: oc.upload_state(0, h0, phase))
        for _ in range(3):
            p.step()
        p.step((DT, 1.0, DT))
        for _ in range(9):
            p.step()
        p.step((-0.25,))                 # a negative dt leaves phases below zero: the handle goes over to the general path for good
        for _ in range(4):
            p.step()
        p.check_phase()
    finally:
        p.close()


@pytest.mark.parametrize("every", INTERVALS)
def test_foam_accumulator_sees_each_dt_once(every):
    # ACCUMULATE fades by exp(-decay * sum of the dt's since the last displace): a retained dt is applied to the phase again, never to the foam
    p = Pair(256, 2, every, foam="accumulate")
    try:
        p.both(lambda oc: oc.set_foam_params(0, 0.9, 4.0, 3.0))
        for n in [1, 1, 1, 0, 3, 1, 1, 1, 9, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1]:
            p.step((DT,) * n)
        p.check_phase()
        assert p.lazy.read_foam(0).max() > 0
    finally:
        p.close()
