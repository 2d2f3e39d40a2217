"""The FFT step side of one handle as ONE model, driven by seeded call sequences (include/datum_ocean_hip.h from "lifetime" to "foam", plus
"surface bounds", "surface velocity" and the profile).  Every kernel is pinned against float64 from a state its test sets up, and every
exactness claim by two handles that run the same host code; this module restates what the HOST decides between the kernels -- when queued
dt's are applied and under which wave scale, where the phase lives, which row-pass form runs, when a foam accumulator is zeroed and what
fade it sees, when the velocity plane and the bounds records count as current -- from the header, over long mixed orders of calls.

  Model       one method per C-ABI call, each returning OK, EINVAL or ESTATE; a refused call changes nothing.  The phase of every cascade
              is advanced by oracle.update one dt at a time AT THE MOMENT update is called, under the wave scale then in force: the header
              promises that every queue, every write-back interval and every phase store gives that phase bit for bit;
  sequence    (seed, length) -> a list of (name, args), a pure function of its arguments; args are numbers, strings and tuples of them;
  apply       one operation on a model;
  observe     what the GPU test can read back, as a dict of bytes and tuples: equal dicts are equal bits.

Where the header is silent the code's rule is taken, and named here:
  * the module's write-back interval (set_phase_writeback(0)) is 8; update itself brings the phase up to date, down to the newest 8 dt's, once
    more than 32 are queued; a row pass takes at most 8 dt's (the trace's "advance first": the phase-only kernel ran ahead of the row pass);
  * a dt may ride in the row pass while dt >= 0 and omegamax dt < 6 in every cascade, omegamax the fp32 dispersion of the table's corner;
  * a negative dt, once APPLIED (by any call that brings the phase up to date), makes EVERY cascade's phase count as outside [0, 2 pi)
    (park_state's flag word, bit 0) until the cascade gets a new state;
  * the quadrant word: a bit is set by a zero phase (create, upload_state without one, rebuild_height for a cascade without a state) and by an
    uploaded, resumed or -- on the switch to AUTO -- inspected phase that is symmetric bit for bit and in range, all only under AUTO; every
    bit is cleared by a displace that cannot read the tables (the literal mode, velocity on, a cascade outside the range or not symmetric)
    and by the switch to PLANE;
  * the checks of rebuild_height come in the order range, seed, wave scale, amplitude, wind; park_state refuses a cascade without a state;
  * cascade groups and the store policy as plan_step has them: grids below 1024^2 are written through in one launch per pass unless a group
    is set; 28 (20, 16 with h0 as halves) bytes per point against 240 MB size the module's group once 52 (44) bytes per point pass 300 MB;
  * set_cascade_group and set_map_store_policy refuse while a profile is open, as the four setters the header names do.

`mistake` plants one wrong host rule each (tests/test_step_seq_model.py shows that every one is seen by a committed seed):
  "new_scale_queue"      set_cascade with a new wave scale applies the queued and retained dt's under the NEW scale
  "resume_keeps_foam"    resume_state does not zero the cascade's foam accumulator
  "height_zeroes_foam"   upload_height zeroes it
  "height_resets_phase"  upload_height starts the phase from zero
  "foam_dt_queued"       foam's dt is the sum of the dt's still queued at displace, not of all since the previous displace
  "fade_negative"        fade is not held at 1 for a negative sum
  "negative_not_wild"    a negative dt leaves the park flag clear (and the row-pass form)
  "upload_keeps_wild"    an uploaded phase inside the range keeps the cascade's old flag
  "displace_keeps_bounds" displace leaves the bounds mark standing
  "bind_keeps_bounds"    bind_maps leaves it standing
  "velocity_keeps_current" set_velocity off and on again keeps the CURRENT mark
  "quadrant_survives"    the quadrant bits survive a displace that cannot read the tables
  "upload_keeps_phase"   upload_state without a phase keeps the old phase
  "refused_rebuild_installs" a rebuild_height refused for its amplitude or wind installs its wave scale
  "resume_ignores_flags" resume_state ignores the flag word
  "scale_not_resized"    the fp16 scale is not sized again after a new h0 (seen in the exponents `observe` carries, and in the maps)
"""

import functools
import math

import numpy as np

import foam64
import ref64
from oracle import oracle

F = np.float32
OK, EINVAL, ESTATE = 0, -1, -2
FP32, FP16, FP16_H0 = 0, 1, 2
FOAM_OFF, FOAM_JACOBIAN, FOAM_ACCUMULATE = 0, 1, 2
AUTO, PLANE = 0, 1
MAPS_AUTO, MAPS_WRITTEN_THROUGH, MAPS_STREAMED = 0, 1, 2
MAX_PENDING = 8
SLOTS = 4

FORMS = ("plane", "wild", "quadrant", "literal")
MISTAKES = ("new_scale_queue", "resume_keeps_foam", "height_zeroes_foam", "height_resets_phase", "foam_dt_queued", "fade_negative", "negative_not_wild",
            "upload_keeps_wild", "displace_keeps_bounds", "bind_keeps_bounds", "velocity_keeps_current", "quadrant_survives", "upload_keeps_phase",
            "refused_rebuild_installs", "resume_ignores_flags", "scale_not_resized")

WIND = (0.780869, 0.624695)
WINDSPEED = 7.9
AMPLITUDE = 0.0025


def _r(v):
    """a Python float that is an fp32 value: what reaches the model is what reaches the C ABI"""
    return float(F(v))


# -- the arrays an operation names by key


@functools.lru_cache(maxsize=64)
def _seeded(N, rngseed, wavescale):
    s, h0 = oracle.seed(N, int(rngseed), wavescale, AMPLITUDE, WINDSPEED, WIND, sanitize=True)
    s.setflags(write=False)
    h0.setflags(write=False)
    return s, h0


def make_h0(N, key):
    """key = (rngseed, wavescale the spectrum is made for)"""
    return _seeded(N, key[0], key[1])[1]


def make_seed(N, key):
    return _seeded(N, key[0], key[1])[0]


def make_phase(N, key):
    """key = None (no phase), ("sym", s): symmetric and in range, ("rand", s): in range, ("wild", s): some values outside [0, 2 pi)"""
    if key is None:
        return None
    kind, s = key
    rng = np.random.RandomState(int(s))
    if kind == "sym":
        q = rng.uniform(0.0, 6.28, (N // 2 + 1, N // 2 + 1)).astype(F)
        i = np.abs(np.arange(N) - N // 2)
        return np.ascontiguousarray(q[i][:, i])
    if kind == "rand":
        return rng.uniform(0.0, 6.28, (N, N)).astype(F)
    assert kind == "wild"
    return rng.uniform(-3.0, 9.0, (N, N)).astype(F)


@functools.lru_cache(maxsize=None)
def _table32(N):
    w = np.ascontiguousarray(ref64.twiddles64(N).astype(F))
    w.setflags(write=False)
    return w


def in_range(phase):
    return bool(np.all((phase >= F(0)) & (phase < F(6.2831855))))


def symmetric(phase):
    """ocean_quadrant.h: every element equals, bit for bit, the one with y, x >= N/2 that shares (|y - N/2|, |x - N/2|)"""
    N = phase.shape[0]
    i = np.abs(np.arange(N) - N // 2)
    rep = N // 2 + np.where(i == N // 2, -i, i)
    b = phase.view(np.uint32)
    return bool(np.array_equal(b, b[rep][:, rep]))


def omegamax(N, wavescale):
    """the fp32 dispersion of the table's corner, as ensure_omega forms it"""
    kc = (F(6.2831855) * (F(0.5) * F(N))) / F(wavescale)
    k2 = F(kc * kc) + F(kc * kc)
    return F(np.sqrt(F(F(9.81) * F(np.sqrt(k2))) * F(F(1.0) + F(k2 / F(136900.0)))))


def fusable(dt, N, wavescale):
    return dt >= 0.0 and float(F(omegamax(N, wavescale) * F(dt))) < 6.0


class Cascade:
    def __init__(self, N):
        self.h0 = np.zeros((N, N, 2), F)
        self.phase = np.zeros((N, N), F)
        self.base = self.phase.copy()          # (mistake "new_scale_queue" only: the phase as last brought up to date)
        self.wavescale, self.chop = 64.0, _r(1.35)
        self.seed = None
        self.held = self.wild = False
        self.quadrant = True
        self.threshold, self.gain, self.decay = 0.5, 2.0, 1.0
        self.foam = None                       # the plane, fp32, while foam is on and its contents are known
        self.foam_want = None                  # float64: what the last displace should have left
        self.dirty = False                     # the fp16 scale is to be sized again
        self.e = (0, 0)                        # ... and the exponents it was last sized to


class Model:
    """the handle's step side at resolution N with C cascades"""

    def __init__(self, N, C=3, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.N, self.C, self.mistake = N, C, mistake
        self.casc = [Cascade(N) for _ in range(C)]
        self.format, self.literal = FP32, False
        self.store, self.writeback, self.group, self.policy = AUTO, 0, 0, MAPS_AUTO
        self.foam_mode, self.velocity, self.velocity_current, self.bounds_current = FOAM_OFF, False, False, False
        self.foamdt = 0.0
        self.profile = False
        self.parked = [None] * SLOTS           # (h0, phase, flags)
        self.queue, self.retained = [], []
        self.bound = {"maps": False, "foam": False, "velocity": False}
        self.seed_held = False
        self.trace = []                        # one (advance first, form) per displace
        self.update_flushes = 0                # times update itself brought the phase up to date (more than 32 queued)
        self.refused = None
        self.maps = [None] * C                 # fp32 [2][N][N][4] of the last displace, where something asked for them

    # -- bookkeeping the bits do not show (the trace does)

    def _refuse(self, code, name):
        self.refused = "datum_ocean_" + name
        return code

    def _range(self, c, name):
        return None if 0 <= c < self.C else self._refuse(EINVAL, name)

    def _flush(self):
        """the stored phase brought up to every update: nothing queued, nothing retained"""
        done = bool(self.queue or self.retained)
        self._applied(self.queue)
        self.queue, self.retained = [], []
        if self.mistake == "new_scale_queue":
            for s in self.casc:
                s.base = s.phase.copy()
        return done

    def _applied(self, dts):
        """dt's that went through the phase-only kernel: a negative one leaves every cascade's phase outside the range (the header is silent
        on WHEN the flag rises; the code's rule: when the dt is applied, not when it is queued -- a queued dt can never ride in a row pass,
        so every call that shows the flag or acts on it has applied it first, except set_phase_store's inspection)"""
        if any(not dt >= 0 for dt in dts) and self.mistake != "negative_not_wild":
            for s in self.casc:
                s.wild = True

    def _flush_retained(self):
        done = bool(self.retained)
        if done and self.mistake == "new_scale_queue":
            for s in self.casc:
                for dt in self.retained:
                    oracle.update(s.base, s.wavescale, dt)
        self.retained = []
        return done

    def settled(self):
        """nothing queued and nothing retained: reading the phase changes nothing on the device"""
        return not self.queue and not self.retained

    def half(self):
        return self.format != FP32

    # -- the launch plan's getters

    def _beyond(self):
        N = self.N
        return N >= 4096 or (N >= 1024 and self.C * N * N * ((20.0 if self.half() else 28.0) + 24.0) > 300.0e6)

    def map_store_policy(self):
        N = self.N
        if N >= 4096 or N < 1024:
            return self.policy, N >= 4096
        if self.policy != MAPS_AUTO:
            return self.policy, self.policy == MAPS_STREAMED
        return self.policy, self._beyond()

    def cascade_group(self):
        C = self.C
        if self.group > 0:
            g = min(self.group, C)
        elif not self.map_store_policy()[1] or not self._beyond():
            g = C
        else:
            g = int(240.0e6 / (self.N * self.N * ((8.0 if self.format == FP16_H0 else 12.0) + (8.0 if self.half() else 16.0))))
            g = max(1, min(g, C))
            groups = (C + g - 1) // g
            g = (C + groups - 1) // groups
        return g, (C + g - 1) // g

    def phase_writeback(self):
        return self.writeback if self.writeback > 0 else MAX_PENDING

    def phase_store(self):
        return self.store, sum(int(s.quadrant) << c for c, s in enumerate(self.casc))

    # -- what the probes return

    def read_velocity_code(self):
        return OK if self.velocity and self.velocity_current else ESTATE

    def read_foam_code(self):
        return OK if self.foam_mode != FOAM_OFF else ESTATE

    def cast_bounded_code(self):
        return OK if self.bounds_current else ESTATE

    # -- state

    def set_cascade(self, c, wavescale, chop):
        if self._range(c, "set_cascade") or not wavescale > 0:
            return self._refuse(EINVAL, "set_cascade")
        s = self.casc[c]
        if wavescale != s.wavescale and not self.settled():
            if self.mistake == "new_scale_queue":
                s.phase = s.base.copy()
                for dt in self.retained + self.queue:
                    oracle.update(s.phase, wavescale, dt)
            self._flush()
        s.wavescale, s.chop = wavescale, chop
        return OK

    def _new_state(self, c, wild):
        s = self.casc[c]
        s.held, s.wild, s.dirty = True, wild, True
        if self.foam_mode == FOAM_ACCUMULATE and s.foam is not None:
            s.foam = np.zeros((self.N, self.N), F)

    def _inspect(self, c, wild):
        """a phase just written into the plane: symmetric and in range moves into the table under AUTO"""
        s = self.casc[c]
        s.quadrant = self.store == AUTO and not wild and symmetric(s.phase)

    def upload_state(self, c, h0, phase):
        if self._range(c, "upload_state"):
            return EINVAL
        self._flush()
        s = self.casc[c]
        s.h0 = np.array(h0, F)
        if phase is not None:
            s.phase = np.array(phase, F)
            wild = not in_range(s.phase)
            self._inspect(c, wild)
            if self.mistake == "upload_keeps_wild" and not wild:
                wild = s.wild
        else:
            if self.mistake != "upload_keeps_phase":
                s.phase = np.zeros((self.N, self.N), F)
            s.quadrant, wild = self.store == AUTO, False
        s.base = s.phase.copy()
        self._new_state(c, wild)
        return OK

    def _new_height(self, c):
        if self.mistake != "scale_not_resized":
            self.casc[c].dirty = True

    def upload_height(self, c, h0):
        if self._range(c, "upload_height"):
            return EINVAL
        s = self.casc[c]
        if not s.held:
            return self._refuse(ESTATE, "upload_height")
        s.h0 = np.array(h0, F)
        self._new_height(c)
        if self.mistake == "height_zeroes_foam" and s.foam is not None:
            s.foam = np.zeros((self.N, self.N), F)
        if self.mistake == "height_resets_phase":
            s.phase = np.zeros((self.N, self.N), F)
        return OK

    def upload_seed(self, c, seed):
        if self._range(c, "upload_seed"):
            return EINVAL
        self.casc[c].seed = np.array(seed, F)
        self.seed_held = True
        return OK

    def rebuild_height(self, c, wavescale, amplitude, windspeed, windx, windy, h0_of):
        """h0_of(seed, wavescale, amplitude, windspeed, (windx, windy)) gives the rebuilt h0: the oracle's on the CPU, the device's own in
        the GPU test (tests/test_gpu_h0.py holds the kernel to the expression)"""
        name = "rebuild_height"
        if self._range(c, name):
            return EINVAL
        if not self.seed_held:
            return self._refuse(ESTATE, name)
        if not wavescale > 0:
            return self._refuse(EINVAL, name)
        if not (amplitude >= 0 and math.isfinite(amplitude)) or not all(math.isfinite(v) for v in (windspeed, windx, windy)):
            if self.mistake == "refused_rebuild_installs":
                self.set_cascade(c, wavescale, self.casc[c].chop)
            return self._refuse(EINVAL, name)
        s = self.casc[c]
        self.set_cascade(c, wavescale, s.chop)
        seed = s.seed if s.seed is not None else np.zeros((self.N, self.N, 2), F)
        s.h0 = np.array(h0_of(seed, wavescale, amplitude, windspeed, (windx, windy)), F)
        self._new_height(c)
        if not s.held:
            # the header: a call that replaces the phase brings it up to date first -- the new state takes none of the dt's queued before it
            self._flush()
            s.phase = np.zeros((self.N, self.N), F)
            s.base = s.phase.copy()
            s.quadrant = self.store == AUTO
            s.held, s.wild, s.dirty = True, False, True
        return OK

    def read_height(self, c):
        return self._range(c, "read_height") or OK

    def read_state(self, c):
        if self._range(c, "read_state"):
            return EINVAL
        self._flush()
        return OK

    def park_state(self, c, slot):
        if self._range(c, "park_state"):
            return EINVAL
        s = self.casc[c]
        if not s.held:
            return self._refuse(ESTATE, "park_state")
        self._flush()
        self.parked[slot] = (s.h0.copy(), s.phase.copy(), 1 if s.wild else 0)
        return OK

    def resume_state(self, c, slot):
        if self._range(c, "resume_state"):
            return EINVAL
        self._flush()
        h0, phase, flags = self.parked[slot]
        s = self.casc[c]
        s.h0, s.phase = h0.copy(), phase.copy()
        s.base = s.phase.copy()
        wild = bool(flags & 1) and self.mistake != "resume_ignores_flags"
        self._inspect(c, wild)
        foam = s.foam
        self._new_state(c, wild)
        if self.mistake == "resume_keeps_foam":
            s.foam = foam
        return OK

    # -- the per-frame path

    def update(self, dt):
        for s in self.casc:
            oracle.update(s.phase, s.wavescale, dt)
        self.queue.append(dt)
        self.foamdt += float(dt)
        if len(self.queue) > 4 * MAX_PENDING:
            self._flush_retained()
            keep = self.queue[-MAX_PENDING:]
            self._applied(self.queue[:-MAX_PENDING])
            if self.mistake == "new_scale_queue":
                for s in self.casc:
                    for d in self.queue[:-MAX_PENDING]:
                        oracle.update(s.base, s.wavescale, d)
            self.queue = keep
            self.update_flushes += 1
        return OK

    def _maps(self, c, maps_of):
        if self.maps[c] is None:
            self.maps[c] = self.oracle_maps(c) if maps_of is None else maps_of(c)
        return self.maps[c]

    def oracle_maps(self, c):
        """the fp32 oracle on this cascade's state: on the literal table in the literal mode; otherwise on the table's exact values rounded
        to fp32 (ref64.twiddles64) -- oracle.weights(N, reduced=True) takes cos / sin of an fp32 ANGLE and is off by up to 6 ulp, which
        would be the table's error and not that of the fp32 arithmetic the device's bars are measured against"""
        s = self.casc[c]
        return oracle.displace(s.h0, s.phase.copy(), s.wavescale, s.chop, w=oracle.weights(self.N) if self.literal else _table32(self.N))

    def displace(self, maps_of=None):
        """maps_of(c): the maps the foam is formed from (the device's own in the GPU test; default: the fp32 oracle's)"""
        if not all(s.held for s in self.casc):
            return self._refuse(ESTATE, "displace")
        N = self.N
        first = False
        if self.literal:
            first = self._flush()
        elif self.queue:
            if not any(s.wild for s in self.casc) and all(fusable(dt, N, s.wavescale) for dt in self.queue for s in self.casc):
                if len(self.queue) > MAX_PENDING:
                    first = True
                    self._flush_retained()
                    self.queue = self.queue[-MAX_PENDING:]
            else:
                first = self._flush()
            if len(self.retained) + len(self.queue) > MAX_PENDING:
                first = self._flush_retained() or first
        if self.half():
            for s in self.casc:
                if s.dirty:
                    s.e, s.dirty = ref64.fp16_scales(s.h0, N), False
        tables = all(s.quadrant for s in self.casc) and not self.literal and not self.velocity and not any(s.wild for s in self.casc)
        if not tables and self.mistake != "quadrant_survives":
            for s in self.casc:
                s.quadrant = False
        form = "literal" if self.literal else "quadrant" if all(s.quadrant for s in self.casc) else "wild" if any(s.wild for s in self.casc) else "plane"
        self.trace.append((first, form))
        applied = self.retained + self.queue
        stored = len(applied) > 0 and len(applied) >= self.phase_writeback()
        if self.mistake == "new_scale_queue" and stored:
            for s in self.casc:
                s.base = s.phase.copy()
        self.retained = [] if stored else applied
        dt = sum(float(d) for d in self.queue) if self.mistake == "foam_dt_queued" else self.foamdt
        self.queue = []
        self.foamdt = 0.0
        self.maps = [None] * self.C
        if self.foam_mode != FOAM_OFF:
            for c, s in enumerate(self.casc):
                J = foam64.jacobian64(self._maps(c, maps_of), s.wavescale, N)
                if self.foam_mode == FOAM_JACOBIAN:
                    s.foam_want = J
                else:
                    fade = math.exp(-float(s.decay) * dt)
                    if self.mistake != "fade_negative":
                        fade = min(1.0, fade)
                    assert s.foam is not None, "an accumulator whose contents nobody defined"
                    s.foam_want = np.maximum(foam64.coverage64(J, s.threshold, s.gain), s.foam.astype(np.float64) * float(F(fade)))
                s.foam = s.foam_want.astype(F)
        if self.mistake != "displace_keeps_bounds":
            self.bounds_current = False
        if self.velocity:
            self.velocity_current = True
        return OK

    # -- modes

    def set_spectrum_format(self, fmt):
        name = "set_spectrum_format"
        if fmt not in (FP32, FP16, FP16_H0):
            return self._refuse(EINVAL, name)
        if self.profile or (fmt != FP32 and self.literal):
            return self._refuse(ESTATE, name)
        self.format = fmt
        for s in self.casc:
            s.dirty = self.half()
            if not self.half():
                s.e = (0, 0)
        return OK

    def set_literal_transform(self, on):
        if on and (self.profile or self.half()):
            return self._refuse(ESTATE, "set_literal_transform")
        self.literal = bool(on)
        return OK

    def _while_profiling(self, name):
        return self._refuse(ESTATE, name) if self.profile else None

    def set_phase_store(self, mode):
        if mode not in (AUTO, PLANE):
            return self._refuse(EINVAL, "set_phase_store")
        if self._while_profiling("set_phase_store"):
            return ESTATE
        if mode == self.store:
            return OK
        self.store = mode
        for c, s in enumerate(self.casc):
            if mode == PLANE:
                s.quadrant = False
            elif not s.wild:
                self._inspect(c, False)
        return OK

    def set_phase_writeback(self, every):
        if not 0 <= every <= MAX_PENDING:
            return self._refuse(EINVAL, "set_phase_writeback")
        if self._while_profiling("set_phase_writeback"):
            return ESTATE
        self.writeback = every
        return OK

    def set_cascade_group(self, n):
        if n < 0:
            return self._refuse(EINVAL, "set_cascade_group")
        if self._while_profiling("set_cascade_group"):
            return ESTATE
        self.group = n
        return OK

    def set_map_store_policy(self, policy):
        if policy not in (MAPS_AUTO, MAPS_WRITTEN_THROUGH, MAPS_STREAMED):
            return self._refuse(EINVAL, "set_map_store_policy")
        if self._while_profiling("set_map_store_policy"):
            return ESTATE
        self.policy = policy
        return OK

    # -- foam

    def set_foam(self, mode):
        if mode not in (FOAM_OFF, FOAM_JACOBIAN, FOAM_ACCUMULATE):
            return self._refuse(EINVAL, "set_foam")
        self.foam_mode = mode
        for s in self.casc:
            s.foam = None if mode == FOAM_OFF else np.zeros((self.N, self.N), F)
            s.foam_want = None
        return OK

    def set_foam_params(self, c, threshold, gain, decay):
        name = "set_foam_params"
        if self._range(c, name):
            return EINVAL
        if not all(math.isfinite(v) for v in (threshold, gain, decay)) or gain < 0 or decay < 0:
            return self._refuse(EINVAL, name)
        s = self.casc[c]
        s.threshold, s.gain, s.decay = threshold, gain, decay
        return OK

    def reset_foam(self, c):
        if self._range(c, "reset_foam"):
            return EINVAL
        if self.foam_mode == FOAM_OFF:
            return self._refuse(ESTATE, "reset_foam")
        self.casc[c].foam = np.zeros((self.N, self.N), F)
        return OK

    def bind_foam(self, on):
        """the plane in use changes: its contents are the caller's until reset_foam, set_foam or, in JACOBIAN mode, the next displace"""
        self.bound["foam"] = bool(on)
        for s in self.casc:
            s.foam = None
        return OK

    # -- velocity, maps, bounds, profile, stream

    def set_velocity(self, on):
        if on and self.velocity:
            return OK
        keep = self.velocity_current
        self.velocity, self.velocity_current = bool(on), False
        if self.mistake == "velocity_keeps_current":
            self.velocity_current = keep
        return OK

    def bind_velocity(self, on):
        self.bound["velocity"] = bool(on)
        self.velocity_current = False
        return OK

    def bind_maps(self, on):
        self.bound["maps"] = bool(on)
        if self.mistake != "bind_keeps_bounds":
            self.bounds_current = False
        return OK

    def reduce_bounds(self):
        self.bounds_current = True
        return OK

    def profile_begin(self, max_samples, stride):
        if max_samples < 1 or stride < 1:
            return self._refuse(EINVAL, "profile_begin")
        if self.literal:
            return self._refuse(ESTATE, "profile_begin")
        self._flush_retained()
        self.profile = True
        return OK

    def profile_end(self):
        if not self.profile:
            return self._refuse(ESTATE, "profile_end")
        self.profile = False
        return OK

    def set_stream(self, own):
        return OK


def observe(m):
    """the model's observables as a dict of bytes and tuples: what tests/test_gpu_step_sequences.py reads back, bit for bit (the maps'
    format and the fp16 exponents through the row pass's halves: "times 2^e is a half")"""
    out = {"phase": tuple(s.phase.tobytes() for s in m.casc), "h0": tuple(s.h0.tobytes() for s in m.casc),
           "parked": tuple(None if p is None else (p[0].tobytes(), p[1].tobytes(), p[2]) for p in m.parked),
           "phase_store": m.phase_store(), "phase_writeback": m.phase_writeback(), "cascade_group": m.cascade_group(),
           "map_store_policy": m.map_store_policy(), "probes": (m.read_velocity_code(), m.read_foam_code(), m.cast_bounded_code()),
           "foam": tuple(None if s.foam is None else s.foam.tobytes() for s in m.casc),
           "spectrum": (m.format, m.literal, tuple(s.e for s in m.casc) if m.half() and all(not s.dirty for s in m.casc) else None)}
    return out


def hidden(m):
    """what no call reads back but a refused call must not change either"""
    return {"wild": tuple(s.wild for s in m.casc), "held": tuple(s.held for s in m.casc),
            "scales": tuple((s.wavescale, s.chop, s.threshold, s.gain, s.decay) for s in m.casc), "queue": (tuple(m.queue), tuple(m.retained), m.foamdt),
            "modes": (m.foam_mode, m.velocity, m.profile, m.seed_held, tuple(sorted(m.bound.items())))}


def _oracle_h0(seed, wavescale, amplitude, windspeed, wind):
    return oracle.height_from_seed(seed, wavescale, amplitude, windspeed, wind)


def apply(m, op, h0_of=None, maps_of=None):
    """one operation on the model; returns the code"""
    name, a = op
    N = m.N
    m.refused = None
    if name == "update":
        dt, n = a
        for _ in range(n):
            m.update(dt)
        return OK
    if name == "displace":
        return m.displace(maps_of)
    if name == "upload_state":
        return m.upload_state(a[0], make_h0(N, a[1]), make_phase(N, a[2]))
    if name == "upload_height":
        return m.upload_height(a[0], make_h0(N, a[1]))
    if name == "upload_seed":
        return m.upload_seed(a[0], make_seed(N, a[1]))
    if name == "rebuild_height":
        return m.rebuild_height(*a, h0_of=h0_of or _oracle_h0)
    if name in ("bind_foam", "bind_velocity", "bind_maps", "set_velocity", "set_literal_transform", "set_stream"):
        return getattr(m, name)(a[0])
    return getattr(m, name)(*a)


def brief(op):
    name, a = op
    return f"{name}{tuple(a)}"


# -- the generator

# (wave scales at which a 64^2 or 128^2 grid resolves the spectrum's peak, k = g / windspeed^2 = 0.16 rad/m: at 9.5 and 140 m a handful of
# bins carries the sea, the transform's rounding errors add coherently as for a pure tone -- tests/test_gpu_pointwise.py holds single bins
# to K_EDGE, not K_MAP -- and the fp32 reference itself leaves a third of K_MAP, 3.07 at 140 m)
SCALES = (22.0, 64.0, 33.0, 45.0)
CHOPS = (0.0, 0.8, 1.35, 2.2)
# (the fp32 reference's worst texel against float64 varies from sea to sea, 1.7 to 3.1 in K_MAP's units over seeds 1000 .. 1099 at these
# scales and sizes, and a third of K_MAP is 3: these are the seeds that stay at or below 2.4 at every scale, at 64^2 and 128^2, with a zero,
# a random and a symmetric phase -- measured on the CPU reference alone, no device involved.  Three of them (1053, 1057, 1058) replace seeds whose
# LITERAL-mode reference left a third of K_LIT_DISP on a committed sequence: K_LIT_* is three times the reference's worst on the example state,
# so a third of it is the reference's own typical error (2.0 - 2.4 over ordinary seas), and that margin is fitted to the committed sequences
H0_SEEDS = (1004, 1005, 1007, 1011, 1053, 1058, 1029, 1057, 1038, 1039, 1042, 1046, 1047, 1048, 1050, 1052)
DTS = (1.0 / 60.0, 1.0 / 30.0, 0.25, 0.0, -1.0 / 60.0, 3.5)
PLAN = ("set_cascade_group", "set_map_store_policy", "set_phase_writeback", "set_phase_store")
INF = float("inf")


def sequence(seed, length, C=3, plan_only=False):
    """`length` operations (a few more where one choice emits several) from numpy.random.RandomState(seed) alone.  The generator keeps
    what it must know of the handle to make every operation valid or a documented refusal.  plan_only: the launch-plan families plus
    update and displace, on a handle of C cascades that all hold a state"""
    rng = np.random.RandomState(seed)
    ops = []
    ws = [64.0] * C
    held = [False] * C
    S = dict(seed=False, seeds=[False] * C, foam=FOAM_OFF, literal=False, fmt=FP32, profile=False, velocity=False, parked=[0.0] * SLOTS, queued=0)

    def pick(seq):
        return seq[int(rng.randint(len(seq)))]

    def h0_key(c):
        return (pick(H0_SEEDS), ws[c])

    def set_cascade(c=None):
        c = int(rng.randint(C)) if c is None else c
        kind = int(rng.randint(3))                                                 # a new scale, the choppiness alone, both
        scale = ws[c] if kind == 1 else pick([s for s in SCALES if s != ws[c]])
        fresh = scale != ws[c] and held[c]
        ws[c] = scale
        ops.append(("set_cascade", (c, scale, _r(pick(CHOPS)))))
        if fresh:                                                                  # a sea made for the new scale: the bars are for such seas
            ops.append(("upload_height", (c, h0_key(c))))

    def phase_key():
        return pick([None, None, ("sym", int(rng.randint(100))), ("sym", int(rng.randint(100))), ("rand", int(rng.randint(100))), ("wild", int(rng.randint(100)))])

    def upload_state(c=None, key=0):
        c = int(rng.randint(C)) if c is None else c
        held[c] = True
        S["queued"] = 0
        ops.append(("upload_state", (c, h0_key(c), phase_key() if key == 0 else key)))

    def update():
        n = 40 if rng.randint(8) == 0 else 1
        weights = np.array([6.0, 3.0, 2.0, 1.0, 1.0, 1.0])
        ops.append(("update", (_r(DTS[int(rng.choice(len(DTS), p=weights / weights.sum()))]), n)))
        S["queued"] += n

    def displace():
        ops.append(("displace", ()))
        S["queued"] = 0

    def step():
        update()
        displace()

    def upload_height():
        c = int(rng.randint(C))
        ops.append(("upload_height", (c, h0_key(c))))

    def upload_seed():
        c = int(rng.randint(C))
        S["seed"] = S["seeds"][c] = True
        ops.append(("upload_seed", (c, h0_key(c))))

    def rebuild_height():
        with_seed = [c for c in range(C) if S["seeds"][c]]
        c = pick(with_seed) if with_seed else int(rng.randint(C))
        kind = int(rng.randint(8))
        scale = ws[c] if rng.randint(2) else pick(SCALES)
        args = [c, scale, _r(AMPLITUDE * pick([0.5, 1.0, 2.0])), _r(pick([5.0, WINDSPEED, 12.0])), _r(WIND[0]), _r(WIND[1])]
        if kind == 0:
            args[0] = C                                                            # a cascade out of range
        elif kind == 1:
            args[1] = pick([0.0, -22.0])
        elif kind == 2:
            args[2] = pick([-1.0, INF])
        elif kind == 3:
            args[3 + int(rng.randint(3))] = INF
        elif S["seed"]:
            ws[c] = scale
            held[c] = True
        ops.append(("rebuild_height", tuple(args)))

    def park_state():
        c, slot = int(rng.randint(C)), int(rng.randint(SLOTS))
        if held[c]:
            S["parked"][slot] = ws[c]
            S["queued"] = 0
        ops.append(("park_state", (c, slot)))

    def resume_state():
        slots = [k for k in range(SLOTS) if S["parked"][k]]
        if not slots:
            return park_state()
        c, slot = int(rng.randint(C)), pick(slots)
        if ws[c] != S["parked"][slot]:                                             # the parked sea was made for its cascade's scale
            ws[c] = S["parked"][slot]
            ops.append(("set_cascade", (c, ws[c], _r(pick(CHOPS)))))
        held[c] = True
        S["queued"] = 0
        ops.append(("resume_state", (c, slot)))

    def set_format():
        fmt = pick([f for f in (FP32, FP16, FP16_H0) if f != S["fmt"]])
        if not S["profile"] and not (fmt != FP32 and S["literal"]):
            S["fmt"] = fmt
        ops.append(("set_spectrum_format", (fmt,)))

    def set_literal():
        on = 0 if S["literal"] else 1
        if not (on and (S["profile"] or S["fmt"] != FP32)):
            S["literal"] = bool(on)
        ops.append(("set_literal_transform", (on,)))

    def set_foam():
        S["foam"] = pick([m for m in (FOAM_OFF, FOAM_JACOBIAN, FOAM_ACCUMULATE) if m != S["foam"]])
        ops.append(("set_foam", (S["foam"],)))

    def set_foam_params():
        c = int(rng.randint(C))
        bad = int(rng.randint(6))
        args = [c, _r(pick([0.5, 0.9, 1.1])), _r(pick([2.0, 4.0])), _r(pick([0.0, 0.5, 1.0, 3.0]))]
        if bad == 0:
            args[1 + int(rng.randint(3))] = INF
        elif bad == 1:
            args[2 + int(rng.randint(2))] = -1.0
        ops.append(("set_foam_params", tuple(args)))

    def bind_foam():
        ops.append(("bind_foam", (int(rng.randint(2)),)))
        for c in range(C):                                                         # (the header: reset_foam to start from zero)
            ops.append(("reset_foam", (c,)))

    def profile():
        if S["profile"]:
            ops.append(("profile_end", ()))
            S["profile"] = False
        else:
            if rng.randint(6) == 0:
                ops.append(("profile_end", ()))                                    # refused: none is open
            ops.append(("profile_begin", (4, int(rng.choice([1, 2])))))
            S["profile"] = not S["literal"]
            if S["profile"]:                                                       # a setter that refuses while it is open
                pick([set_format, set_literal, lambda: plan("set_phase_writeback"), lambda: plan("set_phase_store")])()

    def plan(name=None):
        name = pick(PLAN) if name is None else name
        arg = {"set_cascade_group": lambda: int(rng.choice([0, 1, 2, C + 1])), "set_map_store_policy": lambda: int(rng.randint(3)),
               "set_phase_writeback": lambda: int(rng.choice([0, 1, 2, 3, 8])), "set_phase_store": lambda: int(rng.randint(2))}[name]()
        ops.append((name, (arg,)))

    if plan_only:
        for c in range(C):
            ws[c] = SCALES[c % 4]
            ops.append(("set_cascade", (c, ws[c], _r(CHOPS[1 + c % 3]))))
            upload_state(c, pick([None, ("rand", c)]))
        start = len(ops)                                                           # (the states are not counted)
        must = [("set_cascade_group", (1,)), ("set_map_store_policy", (MAPS_STREAMED,)), ("set_map_store_policy", (MAPS_WRITTEN_THROUGH,))]
        for k in rng.permutation(len(must)):                                       # each once, in the seed's order, a step behind each
            ops.append(must[int(k)])
            step()
        while len(ops) < start + length:
            pick([plan, plan, step])()
        if ops[-1][0] != "displace":
            step()
        return ops

    table = {"set_cascade": set_cascade, "upload_state": upload_state, "update": update, "displace": displace, "step": step, "upload_height": upload_height,
             "upload_seed": upload_seed, "rebuild_height": rebuild_height, "park_state": park_state, "resume_state": resume_state,
             "read_state": lambda: (ops.append(("read_state", (int(rng.randint(C)),))), S.update(queued=0)),
             "read_height": lambda: ops.append(("read_height", (int(rng.randint(C)),))),
             "set_format": set_format, "set_literal": set_literal, "plan": plan, "set_foam": set_foam, "set_foam_params": set_foam_params,
             "reset_foam": lambda: ops.append(("reset_foam", (int(rng.randint(C)),))), "bind_foam": bind_foam,
             "set_velocity": lambda: (S.update(velocity=not S["velocity"]), ops.append(("set_velocity", (int(S["velocity"]),)))),
             "bind_velocity": lambda: ops.append(("bind_velocity", (int(rng.randint(2)),))),
             "bind_maps": lambda: ops.append(("bind_maps", (int(rng.randint(2)),))),
             "reduce_bounds": lambda: ops.append(("reduce_bounds", ())), "profile": profile,
             "set_stream": lambda: ops.append(("set_stream", (int(rng.randint(2)),)))}

    # every sequence starts from a handle whose cascades have wave scales of their own; one cascade is sometimes left without a state
    for c in range(C):
        ws[c] = SCALES[(c + seed) % 4]
        ops.append(("set_cascade", (c, ws[c], _r(CHOPS[1 + (c + seed) % 3]))))
    late = int(rng.randint(C)) if rng.randint(3) == 0 else -1
    for c in range(C):
        if c != late:
            upload_state(c)
    if late >= 0 and rng.randint(2):
        # rebuild_height SETS a quadrant bit: a negative dt, applied, leaves the stateless cascade outside the range too; the switch to
        # PLANE clears its bit and the switch back to AUTO does not inspect it; its first state's zero phase is a table again
        ops.append(("update", (_r(DTS[4]), 1)))
        ops.append(("read_state", ((late + 1) % C,)))
        ops.append(("set_phase_store", (PLANE,)))
        ops.append(("set_phase_store", (AUTO,)))
        S["seed"] = S["seeds"][late] = True
        ops.append(("upload_seed", (late, h0_key(late))))
        held[late] = True
        ops.append(("rebuild_height", (late, ws[late], _r(AMPLITUDE), _r(WINDSPEED), _r(WIND[0]), _r(WIND[1]))))
    while len(ops) < length:
        w = {"set_cascade": 2.0, "upload_state": 2.0, "update": 3.0, "displace": 2.0, "step": 5.0, "upload_height": 1.5, "upload_seed": 1.5, "rebuild_height": 3.0,
             "park_state": 1.5, "resume_state": 1.5, "read_state": 1.0, "read_height": 0.7, "set_format": 1.5, "set_literal": 1.2, "plan": 3.0, "set_foam": 1.5,
             "set_foam_params": 1.0, "reset_foam": 0.7, "bind_foam": 0.5, "set_velocity": 1.2, "bind_velocity": 0.7, "bind_maps": 1.0, "reduce_bounds": 1.5,
             "profile": 1.6, "set_stream": 0.7}
        if not all(held):                                                          # a displace would be refused: sometimes, not mostly
            w["displace"], w["step"], w["rebuild_height"], w["upload_seed"], w["upload_state"], w["resume_state"], w["upload_height"] = 0.5, 0.5, 4.0, 3.0, 2.0, 2.0, 3.0
        if S["queued"]:
            w["displace"] = 5.0
        if S["profile"]:
            w["profile"] = 3.0
        names = sorted(w)
        p = np.array([w[n] for n in names])
        table[names[int(rng.choice(len(names), p=p / p.sum()))]]()
    return ops


# The committed sequences: twelve seeds of forty operations, picked out of 0 .. 399 for the coverage conditions and the teeth of
# tests/test_step_seq_model.py
LENGTH = 40
SEEDS = (1, 5, 117, 131, 144, 184, 220, 232, 281, 286, 359, 371)
PLAN_LENGTH = 12
PLAN_SEEDS = (0, 1)
