"""The host's bookkeeping of the lazy phase write-back (datum_amd/csrc/ocean_writeback.h), the struct the HIP module keeps in its handle,
walked on the CPU (tests/cpu/writeback_emul.cpp) under a model of datum_ocean_update / datum_ocean_displace's use of it: whatever the queue
lengths and the interval, the dt's stored into the phase plus the retained ones are exactly the dt's issued, in order, each once."""

import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    lib.writeback_new.restype = ctypes.c_void_p
    lib.writeback_delete.argtypes = [ctypes.c_void_p]
    lib.writeback_fits.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.writeback_clear.argtypes = [ctypes.c_void_p]
    lib.writeback_step.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.writeback_repeat.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


class Handle:
    """datum_ocean_update and datum_ocean_displace as ocean_capi.hip orders them (the fusable case), with lists of dt's for the phase"""

    def __init__(self, emul):
        self.emul = emul
        self.max = emul.writeback_max_pending()
        self.w = emul.writeback_new()
        self.pending = []
        self.stored = []        # the dt's the stored phase contains
        self.launches = []      # (dt's, store) of every row pass

    def close(self):
        self.emul.writeback_delete(self.w)

    def retained(self):
        dt = np.zeros(self.max, np.float32)
        store = ctypes.c_int(-1)
        n = self.emul.writeback_repeat(self.w, dt.ctypes.data, ctypes.byref(store))
        assert store.value == 0
        return [float(x) for x in dt[:n]]

    def flush_retained(self):                       # the phase-only kernel over the retained dt's
        self.stored += self.retained()
        self.emul.writeback_clear(self.w)

    def flush_pending(self, keep):                  # ... and over the oldest queued ones, behind the retained
        if len(self.pending) > keep:
            self.flush_retained()
            cut = len(self.pending) - keep
            self.stored += self.pending[:cut]
            self.pending = self.pending[cut:]

    def update(self, dt):
        self.pending.append(float(np.float32(dt)))
        if len(self.pending) > 4 * self.max:
            self.flush_pending(self.max)

    def displace(self, every):
        if self.pending:
            self.flush_pending(self.max)
            if not self.emul.writeback_fits(self.w, len(self.pending)):
                self.flush_retained()
        assert self.emul.writeback_fits(self.w, len(self.pending))
        pend = np.array(self.pending, np.float32)
        dt = np.zeros(self.max, np.float32)
        store = ctypes.c_int(-1)
        n = self.emul.writeback_step(self.w, pend.ctypes.data, len(pend), every, dt.ctypes.data, ctypes.byref(store))
        self.pending = []
        launch = [float(x) for x in dt[:n]]
        self.launches.append((launch, bool(store.value)))
        if store.value:
            self.stored += launch
        return launch, bool(store.value)


def test_max_pending_is_the_kernels(emul):
    text = open(os.path.join(ROOT, "datum_amd", "csrc", "ocean_kernels.hip"), encoding="utf-8").read()
    assert emul.writeback_max_pending() == 8
    assert '#include "ocean_writeback.h"' in text and "float dt[MAX_PENDING];" in text and "constexpr int MAX_PENDING" not in text


@pytest.mark.parametrize("every", range(1, 9))
def test_one_update_per_step_stores_every_kth(emul, every):
    h = Handle(emul)
    issued = []
    for i in range(40):
        dt = 0.001 * (i + 1)
        h.update(dt)
        issued.append(float(np.float32(dt)))
        launch, store = h.displace(every)
        assert store == ((i + 1) % every == 0)
        assert launch == issued[len(issued) - len(launch):] and len(launch) == (i % every) + 1
        assert h.stored + h.retained() == issued
    assert sum(s for _, s in h.launches) == 40 // every
    h.close()


@pytest.mark.parametrize("every", range(1, 9))
def test_irregular_queues_apply_every_dt_once_in_order(emul, every):
    rs = np.random.RandomState(every)
    h = Handle(emul)
    issued = []
    for step in range(400):
        n = int(rs.choice([0, 0, 1, 1, 1, 2, 3, 7, 8, 9, 17, 40]))
        for _ in range(n):
            dt = float(np.float32(rs.uniform(0, 0.05)))
            h.update(dt)
            issued.append(dt)
        before = list(h.stored)
        launch, store = h.displace(every)
        assert len(launch) <= h.max
        # the row pass loads the stored phase and must arrive at the phase after every dt issued
        stored_before_launch = h.stored[:len(h.stored) - len(launch)] if store else h.stored
        assert stored_before_launch + launch == issued
        assert stored_before_launch[:len(before)] == before
        assert store == (len(launch) >= every and len(launch) > 0)
        assert h.stored + h.retained() == issued
        # nothing queued: the same list again, the same maps
        again, store2 = h.displace(every)
        assert again == ([] if store else launch) and not store2
    h.close()


def test_a_shorter_interval_meets_retained_dts(emul):
    h = Handle(emul)
    for i in range(5):
        h.update(0.01)
        assert h.displace(8)[1] is False
    assert len(h.retained()) == 5
    launch, store = h.displace(2)
    assert store and len(launch) == 5 and h.retained() == [] and len(h.stored) == 5
    h.close()


def test_flush_in_the_middle_of_an_interval(emul):
    h = Handle(emul)
    for i in range(3):
        h.update(0.01 * (i + 1))
        h.displace(8)
    h.flush_retained()                              # a read, a state copy, a new wave scale ...
    assert len(h.stored) == 3 and h.retained() == []
    h.update(0.5)
    launch, store = h.displace(8)
    assert launch == [0.5] and not store
    h.close()
