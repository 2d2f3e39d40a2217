"""The FFT step side of a handle on the MI355X under seeded call sequences (tests/step_seq.py), through the C ABI, against ONE model of what
the host code decides between the kernels.  tests/test_step_seq_model.py shows on the CPU that these sequences see every planted mistake
of that kind.

One case per committed seed at 64^2 x 3 and 128^2 x 3 (the smallest grids: the host code under test does not depend on N), and two short
cases at 1024^2 x 2, the smallest size at which the launch plan is not trivial (cascade groups, streamed or written-through maps).

Behind EVERY operation, bit for bit: the return code (and the call's name in a refusal's text); every held cascade's h0; park_state's flag
word and the parked h0 and phase; phase_store()'s mode and quadrant word, phase_writeback(), cascade_group()'s and map_store_policy()'s
pairs; whether read_velocity, read_foam / foam_device and the bounded cast of an empty ray list return OK or ESTATE; the foam planes against
the model's accumulator (the device's own plane as last checked, zeroed where the model's rules zero it).  Every cascade's PHASE bit for
bit whenever the model has nothing queued and nothing retained, every eighth operation and at the end -- not behind every update: read_state
brings the phase up to date, and a read behind every call would leave no displace a dt to apply and no interval a dt to retain, which are
the rules under test.
Behind every displace, by value: the maps of every cascade against displace64 (lit64 in the literal mode) on the model's state within
K_MAP / K_NORMAL (K_LIT_* in the literal mode); in the fp16 formats the per-format check of tests/test_gpu_pointwise.py (pointwise.compare:
the end-to-end RMSE bars and "really went through halves", every row-pass value times 2^e a half and the nearest one within K_BAND, the column
pass from the device's own row-pass output within K_MAP / K_NORMAL, two debug_rowpass calls equal) with the exponents the MODEL says the handle
sized -- debug_rowpass repeats the retained dt's without storing the phase, so it disturbs nothing under test; foam against jacobian64 / coverage64 of the
device's own maps with the header's fade from the model's double dt sum, within tests/test_gpu_foam.py's bars; velocity against vel64
within K_VEL.  Behind every reduce_bounds the records against bounds64.fold_maps(read_maps) as tests/test_gpu_bounds.py compares them.
A 555.0 canary lies behind every bound buffer.  No operation is retried.
"""

import ctypes
import time

import numpy as np
import pytest

import bounds64
import foam64
import pointwise as pw
import ref64
import step_seq as sq
import vel64
from test_gpu_foam import K_KERNEL, K_STEP
from pointwise import K_MAP, K_NORMAL
from test_gpu_surface import _set

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -24
IT = 4
CANARY = 555.0
FORMATS = {v: k for k, v in {"fp32": 0, "fp16": 1, "fp16h0": 2}.items()}


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _first(got, want):
    d = np.argwhere(_bits(got) != _bits(want))
    return None if not len(d) else (tuple(int(v) for v in d[0]), len(d))


class _Env:
    """the caller's side of a handle: parked states, the buffers that get bound (a canary behind each), a stream of the caller's"""

    def __init__(self, torch, oc):
        self.torch, self.oc = torch, oc
        N, C = oc.N, oc.cascades
        self.parked = [torch.zeros(oc.state_bytes() // 4, dtype=torch.float32, device="cuda") for _ in range(sq.SLOTS)]
        self.floats = {"maps": oc.maps_device()[1] // 4, "foam": C * N * N, "velocity": C * N * N * 4}
        self.buffers = {k: torch.full((n + 64,), CANARY, dtype=torch.float32, device="cuda") for k, n in self.floats.items()}
        for k, n in self.floats.items():
            self.buffers[k][:n] = 0
        self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()

    def bind(self, what, on):
        getattr(self.oc, "bind_" + what)(self.buffers[what].data_ptr() if on else None, self.floats[what] * 4 if on else 0)

    def canary(self, what):
        self.oc.sync()
        self.torch.cuda.synchronize()
        return bool((self.buffers[what][self.floats[what]:] == CANARY).all().item())


def _device(capi, oc, env, N, op):
    """the operation on the handle: (code, error text, what park_state returned)"""
    name, a = op
    out = None
    try:
        if name == "update":
            for _ in range(a[1]):
                oc.update(a[0])
        elif name == "upload_state":
            oc.upload_state(a[0], sq.make_h0(N, a[1]), sq.make_phase(N, a[2]))
        elif name == "upload_height":
            oc.upload_height(a[0], sq.make_h0(N, a[1]))
        elif name == "upload_seed":
            oc.upload_seed(a[0], sq.make_seed(N, a[1]))
        elif name == "rebuild_height":
            oc.rebuild_height(a[0], a[1], a[2], a[3], (a[4], a[5]))
        elif name == "park_state":
            out = oc.park_state(a[0], env.parked[a[1]].data_ptr(), oc.state_bytes())
        elif name == "resume_state":
            oc.resume_state(a[0], env.parked[a[1]].data_ptr(), oc.state_bytes(), env.flags[a[1]])
        elif name in ("bind_maps", "bind_foam", "bind_velocity"):
            env.bind(name[5:], a[0])
        elif name == "set_spectrum_format":
            oc.set_spectrum_format(FORMATS[a[0]])
        elif name == "set_velocity":
            oc.set_velocity("on" if a[0] else "off")
        elif name == "set_stream":
            oc.set_stream(None if a[0] else env.stream.cuda_stream)
        else:
            getattr(oc, name)(*a)
    except capi.OceanError as e:
        return e.code, str(e), None
    return capi.OK, "", out


def _check_maps(m, oc, c, where):
    """the maps of cascade c behind a displace against float64 on the model's state; returns the maps and the measured figures"""
    N, s = m.N, m.casc[c]
    maps = oc.read_maps(c)
    assert np.all(maps[..., 3] == 0) and np.isfinite(maps).all(), where("the maps' .w channels or finiteness")
    got = ref64.channels(maps)
    scale = F(1) / F(s.wavescale)
    if m.literal:
        ref, ln = ref64.lit64(s.h0, s.phase, scale, s.chop, oracle_weights(N), return_len=True)
        bars = ("literal", pw.K_LIT_DISP, pw.K_LIT_NORMAL)
    else:
        ref, ln = ref64.displace64(s.h0, s.phase, scale, s.chop, return_len=True)
        bars = ("fp32", K_MAP, K_NORMAL)
    if m.half():
        rp, again = oc.debug_rowpass(c), oc.debug_rowpass(c)
        same = all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(rp, again))
        lines = []
        try:
            checks = pw.compare(lines.append, maps, s.phase, rp, same, s.h0, s.wavescale, s.chop, FORMATS[m.format], where.tag + f" cascade {c}", scales=s.e)
        except AssertionError as e:
            raise AssertionError(where(f"cascade {c}'s per-format check in {FORMATS[m.format]} with the model's exponents {s.e} ({e}; {lines})")) from e
        print(lines[0])
        return maps, ("fp16",) + tuple(v for _, v, _ in checks[:3])
    kd, kn, _ = pw.pointwise(got, ref, ln, N)
    print(f"{where.tag} cascade {c} {bars[0]}: disp K {kd:.3g} (bar {bars[1]:g}), normal K {kn:.3g} (bar {bars[2]:g})")
    assert kd <= bars[1] and kn <= bars[2], where(f"cascade {c}'s maps ({bars[0]}: K {kd:.3g} / {kn:.3g} for {bars[1]:g} / {bars[2]:g})")
    return maps, (bars[0], kd, kn)


_WEIGHTS = {}


def oracle_weights(N):
    if N not in _WEIGHTS:
        from oracle import oracle as o

        _WEIGHTS[N] = o.weights(N)
    return _WEIGHTS[N]


def _run(capi, torch, report, label, N, C, ops):
    t0 = time.perf_counter()
    m = sq.Model(N, C)
    lib = capi.load()
    arr = (capi.I * C)(*range(C))
    s0 = _set(capi, 0)
    probe = np.empty((N, N, 4), F)
    worst = {}
    seen = None                                                   # the operation behind which the phases were last compared
    with capi.Ocean(N, C) as oc:
        env = _Env(torch, oc)
        env.flags = [0] * sq.SLOTS
        for k, op in enumerate(ops):
            name, a = op
            code, text, out = _device(capi, oc, env, N, op)
            device_maps = {}

            def maps_of(c):
                if c not in device_maps:
                    device_maps[c] = oc.read_maps(c)
                return device_maps[c]

            want_code = sq.apply(m, op, h0_of=lambda *_: oc.read_height(a[0]), maps_of=maps_of)

            def where(what, first=None):
                return (f"{label}, operation {k} {sq.brief(op)}: {what} differs; the model's row-pass form of the last displace {m.trace[-1] if m.trace else None}; "
                        f"first differing texel or word and count {first}; the operations so far: {[sq.brief(o) for o in ops[:k + 1]]}")

            where.tag = f"{label} op {k}"
            assert code == want_code, where(f"the return code ({code} for {want_code}, {text!r})")
            if code != capi.OK:
                assert m.refused in text, where(f"the refusal's text {text!r} (the model: {m.refused})")

            # the getters and the probes
            mode, word = oc.phase_store()
            assert (capi.PHASE_STORES[mode], word) == m.phase_store(), where(f"phase_store ({mode}, {word:#x} for {m.phase_store()})")
            assert oc.phase_writeback() == m.phase_writeback(), where("phase_writeback")
            assert oc.cascade_group() == m.cascade_group(), where(f"cascade_group ({oc.cascade_group()} for {m.cascade_group()})")
            policy, streamed = oc.map_store_policy()
            assert (capi.MAP_STORE_POLICIES[policy], streamed) == m.map_store_policy(), where("map_store_policy")
            assert lib.datum_ocean_read_velocity(oc.h, 0, probe.ctypes.data_as(capi.P)) == m.read_velocity_code(), where("read_velocity's code")
            assert lib.datum_ocean_read_foam(oc.h, 0, probe.ctypes.data_as(capi.P)) == m.read_foam_code(), where("read_foam's code")
            ptr, nbytes = capi.P(), ctypes.c_size_t()
            assert lib.datum_ocean_foam_device(oc.h, ctypes.byref(ptr), ctypes.byref(nbytes)) == m.read_foam_code(), where("foam_device's code")
            cast = lib.datum_ocean_read_rays_bounded(oc.h, arr, C, ctypes.byref(s0), IT, 32, 8, None, 0, None)
            assert cast == m.cast_bounded_code(), where(f"the bounded cast's code ({cast})")

            # h0, the parked states, the phase
            for c, s in enumerate(m.casc):
                if s.held:
                    h0 = oc.read_height(c)
                    assert np.array_equal(_bits(h0), _bits(s.h0)), where(f"cascade {c}'s h0", _first(h0, s.h0))
            if name == "park_state" and code == capi.OK:
                env.flags[a[1]] = out
                h0, phase, flags = m.parked[a[1]]
                assert out == flags, where(f"park_state's flag word ({out} for {flags})")
                oc.sync()
                raw = env.parked[a[1]].cpu().numpy()
                assert np.array_equal(_bits(raw[:2 * N * N]), _bits(h0).ravel()), where("the parked h0")
                assert np.array_equal(_bits(raw[2 * N * N:]), _bits(phase).ravel()), where("the parked phase", _first(raw[2 * N * N:].reshape(N, N), phase))
            if m.settled() or k % 8 == 7 or k == len(ops) - 1:
                for c, s in enumerate(m.casc):
                    phase = oc.read_state(c)
                    m.read_state(c)
                    assert np.array_equal(_bits(phase), _bits(s.phase)), where(f"cascade {c}'s phase (last compared behind operation {seen}: any call since may be the cause)", _first(phase, s.phase))
                seen = k

            # by value, behind a displace
            if name == "displace" and code == capi.OK:
                for c, s in enumerate(m.casc):
                    maps, fig = _check_maps(m, oc, c, where)
                    worst[fig[0]] = [max(x, y) for x, y in zip(worst.get(fig[0], (0.0, 0.0)), fig[1:])]
                    if m.foam_mode != sq.FOAM_OFF:
                        got = oc.read_foam(c)
                        bar = K_KERNEL * EPS * foam64.scale64(maps, s.wavescale, N)
                        if m.foam_mode == sq.FOAM_ACCUMULATE:
                            bar = s.gain * bar + K_STEP * EPS
                        err = float((np.abs(got.astype(np.float64) - s.foam_want) - bar).max())
                        assert err <= 0, where(f"cascade {c}'s foam plane (mode {m.foam_mode}; beyond the bar by {err / EPS:.3g} eps)")
                        s.foam = got                                      # the accumulator from here on: the device's own plane
                    if m.velocity:
                        plane = oc.read_velocity(c)
                        assert np.all(plane[..., 3] == 0) and np.isfinite(plane).all(), where("the velocity plane's .w or finiteness")
                        ref = vel64.vel64(s.h0, s.phase, F(1) / F(s.wavescale), s.chop, vel64.omega32(N, s.wavescale))
                        kv = vel64.k_of(np.moveaxis(plane[..., :3], -1, 0).astype(np.float64), ref, N)
                        worst["velocity"] = [max(worst.get("velocity", [0.0])[0], kv)]
                        assert kv <= vel64.K_VEL, where(f"cascade {c}'s velocity plane (K {kv:.3g} for {vel64.K_VEL:.3g})")
            elif m.foam_mode != sq.FOAM_OFF:
                for c, s in enumerate(m.casc):
                    if s.foam is not None:
                        got = oc.read_foam(c)
                        assert np.array_equal(_bits(got), _bits(s.foam)), where(f"cascade {c}'s foam accumulator", _first(got, s.foam))
            if name == "reduce_bounds" and code == capi.OK:
                rec = oc.read_bounds()
                want = np.stack([bounds64.fold_maps(oc.read_maps(c)) for c in range(C)])
                assert np.array_equal(rec[:, :6], want[:, :6]) and np.all(rec[:, 6:] == 0), where("read_bounds", (rec.tolist(), want.tolist()))
            if name.startswith("bind_") and not a[0]:
                assert env.canary(name[5:]), where(f"the canary behind the bound {name[5:]} buffer")
        for what in env.buffers:
            assert env.canary(what), f"{label}: the canary behind the {what} buffer at the end"
    line = f"step sequences: {label}, {len(ops)} operations, {len(m.trace)} displaces, worst {({k: [round(x, 4) for x in v] for k, v in worst.items()})}, {time.perf_counter() - t0:.2f} s"
    print(line)
    report(line)


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("seed", sq.SEEDS)
def test_sequence(capi, torch, report, seed, N):
    _run(capi, torch, report, f"seed {seed} at {N}^2 x 3", N, 3, sq.sequence(seed, sq.LENGTH))


@pytest.mark.parametrize("seed", sq.PLAN_SEEDS)
def test_launch_plan(capi, torch, report, seed):
    """1024^2 x 2 with set_cascade_group(1) and the STREAMED / WRITTEN_THROUGH policies: the getters' pairs against the model's
    restatement of the header's rule, the maps within the same bars"""
    ops = sq.sequence(seed, sq.PLAN_LENGTH, C=2, plan_only=True)
    _run(capi, torch, report, f"launch plan, seed {seed} at 1024^2 x 2", 1024, 2, ops)


def test_rebuild_height_gives_a_stateless_cascade_none_of_the_queued_updates(capi, torch, report):
    """the header: a call that replaces the phase brings it up to date first.  rebuild_height for a cascade without a state, at the wave
    scale the cascade already has, used to flush the retained dt's only: the new zero phase took the two updates queued before the call"""
    dt = sq._r(1.0 / 60.0)
    ops = [("set_cascade", (0, 22.0, sq._r(1.35))), ("set_cascade", (1, 33.0, sq._r(0.8))), ("upload_state", (0, (1004, 22.0), ("rand", 1))),
           ("upload_seed", (1, (1005, 33.0))), ("update", (dt, 2)), ("rebuild_height", (1, 33.0, sq._r(sq.AMPLITUDE), sq._r(sq.WINDSPEED), sq._r(sq.WIND[0]), sq._r(sq.WIND[1]))),
           ("displace", ()), ("read_state", (1,)), ("update", (dt, 1)), ("displace", ()), ("read_state", (0,))]
    _run(capi, torch, report, "rebuild_height of a stateless cascade behind two queued updates, 64^2 x 2", 64, 2, ops)
