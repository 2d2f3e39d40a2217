"""The Jacobian foam plane (include/datum_ocean_hip.h: datum_ocean_set_foam) on the MI355X, against the float64 reference of
tests/foam64.py.

Bars, with eps = 2^-24:
  against the device's own maps   |J - jacobian64(read_maps)| <= K_KERNEL * eps * (|(1-a)(1-d)| + |bc| + 1), every point: what the
                                  kernel's own fp32 arithmetic may add (two differences, four scalings, two products, a difference)
  end to end                      see test_end_to_end_against_displace64
  accumulation                    gain * K_KERNEL * eps * max_t(scale) + K_STEP * eps per point (clamp and max are 1-Lipschitz, fade <= 1)
Each test reports the measured worst value next to its bar (tests/conftest.py: report).
"""

import math

import numpy as np
import pytest

import foam64
import ref64

pytestmark = pytest.mark.gpu

DT = np.float32(1.0 / 60.0)
EPS = 2.0 ** -24

# at least 3x the worst value measured on the MI355X (the measured worst beside each)
K_KERNEL = 7.5     # kernel arithmetic against jacobian64 of the device's maps: measured 2.40 (4096^2 fp16h0); mean(J) - 1: 0.023
K_E2E = 9.0        # end to end, the maps' error (K_MAP of tests/test_gpu_pointwise.py) through the derivative: measured 0.74 (4096^2)
K_STEP = 32.0      # accumulation beyond the J bar, in eps (the fade's rounding over 20 steps): measured 0.00


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


def _h0(oracle, N, rngseed, wavescale, amplitude=None):
    p = oracle.EXAMPLE
    _, h0 = oracle.seed(N, rngseed, wavescale, amplitude or p["waveamplitude"], p["windspeed"], p["winddirection"], sanitize=True)
    return h0


def _phase(N, rngseed):
    return (np.random.RandomState(rngseed).uniform(0, 2 * np.pi, (N, N))).astype(np.float32)


def _setup(capi, oracle, N, C, fmt="fp32", chops=None, scales=None):
    """a handle of C cascades with distinct wave scales and choppiness, random phases, foam JACOBIAN; returns (handle, wavescales)"""
    scales = scales or [22.0, 64.0, 9.5, 140.0][:C] + [33.0] * max(0, C - 4)
    chops = chops or [1.35, 2.2, 0.8, 3.0][:C] + [1.0] * max(0, C - 4)
    oc = capi.Ocean(N, C)
    if fmt == "literal":
        oc.set_literal_transform(True)
    elif fmt != "fp32":
        oc.set_spectrum_format(fmt)
    for c in range(C):
        oc.set_cascade(c, scales[c], chops[c])
        oc.upload_state(c, _h0(oracle, N, 1000 + c, scales[c]), _phase(N, 77 + c))
    oc.set_foam("jacobian")
    return oc, [float(np.float32(s)) for s in scales]


def _kernel_k(J, maps, ws, N):
    return float((np.abs(J - foam64.jacobian64(maps, ws, N)) / (EPS * foam64.scale64(maps, ws, N))).max())


CASES = [(N, "fp32", 1) for N in (64, 128, 256, 512, 1024, 2048, 4096)]
CASES += [(N, f, 1) for N in (256, 1024, 4096) for f in ("fp16", "fp16h0")]
CASES += [(64, "literal", 1), (1024, "literal", 4), (256, "fp32", 4), (1024, "fp32", 4), (1024, "fp16h0", 4)]


@pytest.mark.parametrize("N,fmt,C", CASES)
def test_against_device_maps(capi, oracle, report, N, fmt, C):
    oc, ws = _setup(capi, oracle, N, C, fmt)
    with oc:
        oc.update(DT)
        oc.displace()
        worst, worst_mean = 0.0, 0.0
        for c in range(C):
            maps = oc.read_maps(c)
            J = oc.read_foam(c).astype(np.float64)
            k = _kernel_k(J, maps, ws[c], N)
            worst = max(worst, k)
            # area conservation: sum(a + d) = sum(ad - bc) = 0 for periodic central differences, so mean(J) = 1 up to the kernel's
            # rounding -- a sign or an axis swap moves it by the mean of a product of slopes
            km = abs(J.mean() - 1.0) / (EPS * foam64.scale64(maps, ws[c], N).mean())
            worst_mean = max(worst_mean, km)
            assert k <= K_KERNEL, (c, k)
            assert km <= K_KERNEL, (c, km)
            del maps, J
    report(f"foam vs jacobian64(device maps) N={N} {fmt} x{C}: K {worst:.3f} (bar {K_KERNEL}), mean(J)-1 K {worst_mean:.3f}")


@pytest.mark.parametrize("N", [64, 256, 1024, 4096])
def test_end_to_end_against_displace64(capi, oracle, report, N):
    """Derivation of the bar.  tests/test_gpu_pointwise.py bounds each displacement channel of the fp32 maps by
    |δ| <= K_MAP eps L s, L = log2 N, s = the channel scale there (max(rms(ch), rms(dx, dy, dz) / 4)).  A central difference over 2h
    takes two such errors: |δa| <= 2 |δ| / (2h) = |δ| N / wavescale, the same for b, c, d.  To first order
    δJ = -δa (1 - d) - δd (1 - a) - δb c - δc b, so |δJ| <= |δ| (N / wavescale) (|1 - a| + |1 - d| + |b| + |c|), plus the kernel's own
    rounding (K_KERNEL above).  The bar is K_E2E eps L s (N / wavescale) (|1 - a| + |1 - d| + |b| + |c|) + K_KERNEL eps scale64."""
    oc, ws = _setup(capi, oracle, N, 1)
    with oc:
        oc.update(DT)
        oc.displace()
        phase = oc.read_state(0)
        J = oc.read_foam(0).astype(np.float64)
        dev = oc.read_maps(0)
    h0 = _h0(oracle, N, 1000, 22.0)
    ref = ref64.displace64(h0, phase, float(np.float32(1.0 / np.float32(22.0))), 1.35)
    a, b, c, d = foam64.parts64(ref, ws[0], N)
    J64 = (1.0 - a) * (1.0 - d) - b * c
    L = math.log2(N)
    rms = [float(np.sqrt(np.mean(ref[ch] ** 2))) for ch in range(3)]
    sall = float(np.sqrt(np.mean(np.square(rms))))
    s = max(max(rms[0], 0.25 * sall), max(rms[1], 0.25 * sall))
    amp = EPS * L * s * (N / ws[0]) * (np.abs(1 - a) + np.abs(1 - d) + np.abs(b) + np.abs(c))
    kern = EPS * foam64.scale64(dev, ws[0], N)
    k = float(((np.abs(J - J64) - K_KERNEL * kern).clip(0) / amp).max())
    report(f"foam end to end vs displace64 N={N}: K {k:.3f} (bar {K_E2E}), folded {float((J < 0).mean()):.4f}")
    assert k <= K_E2E


@pytest.mark.parametrize("mode", ["jacobian", "accumulate"])
def test_exactly_one_when_undisturbed(capi, oracle, mode):
    N = 256
    with capi.Ocean(N, 2) as oc:
        oc.set_cascade(0, 22.0, 0.0)                       # choppiness 0: no horizontal displacement
        oc.upload_state(0, _h0(oracle, N, 5, 22.0), _phase(N, 5))
        oc.set_cascade(1, 22.0, 1.35)                      # a flat ocean
        oc.upload_state(1, np.zeros((N, N, 2), np.float32))
        oc.set_foam(mode)
        oc.set_foam_params(0, 1.5, 2.0, 1.0)
        oc.update(DT)
        oc.displace()
        want = np.ones((N, N), np.float32) if mode == "jacobian" else np.zeros((N, N), np.float32)
        if mode == "accumulate":
            want[:] = 1.0                                    # (threshold 1.5 - 1) * 2 = 1 exactly for cascade 0
        assert np.array_equal(oc.read_foam(0), want)
        want1 = np.ones((N, N), np.float32) if mode == "jacobian" else np.zeros((N, N), np.float32)
        assert np.array_equal(oc.read_foam(1), want1)


@pytest.mark.parametrize("N,p", [(64, 1), (256, 5), (1024, 37)])
def test_plane_wave_along_x(capi, report, N, p):
    ws = 48.0
    # one wave with k along x only.  The sim pairs h0[y][x] with h0[N-1-y][N-1-x] (sim.comp's mirror index), so a bin at row N/2
    # (k_y = 0) also feeds the point (N/2 - 1, N/2 - 1 - p) (k_y != 0): that point's h0 is set to the negated real part of the bin's
    # and its phase to 0, which makes its h~ exactly zero, while the bin's phase 0.7 keeps the k_y = 0 wave
    A = 0.3 * ws / N
    h0 = np.zeros((N, N, 2), np.float32)
    h0[N // 2, N // 2 + p] = (A, 0.5 * A)
    h0[N // 2 - 1, N // 2 - 1 - p] = (-A, 0.5 * A)
    phase = np.zeros((N, N), np.float32)
    phase[N // 2, N // 2 + p] = 0.7
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, ws, 1.35)
        oc.upload_state(0, h0, phase)
        oc.set_foam("jacobian")
        oc.displace()
        maps = oc.read_maps(0)
        J = oc.read_foam(0).astype(np.float64)
    dx, dy = maps[0, ..., 0].astype(np.float64), maps[0, ..., 1].astype(np.float64)
    assert np.abs(dy).max() <= 1e-5 * np.abs(dx).max()     # k_y = 0: dy is rounding noise of the packed transform
    x = np.arange(N)
    e = np.exp(-2j * np.pi * p * x / N)

    def coef(f):
        return 2.0 / N * (f.mean(axis=0) * e).sum()

    A = abs(coef(dx))
    want = A * math.sin(2 * math.pi * p / N) * N / float(np.float32(ws))
    noise = 64 * EPS * (1 + A * N / ws)
    # constant along y (up to the rounding of dx along a column)
    assert np.abs(J - J[:1]).max() <= noise
    # 1 - J is a sinusoid of that amplitude, and nothing else
    f = 1.0 - J
    z = coef(f)
    got = abs(z)
    resid = float(np.abs(f - f.mean() - (z * np.conj(e)).real[None, :]).max())
    report(f"foam plane wave N={N} p={p}: amplitude {got:.6g} want {want:.6g} rel {abs(got - want) / want:.2e}, residual {resid:.2e}")
    assert abs(got - want) <= 1e-5 * want + noise
    assert resid <= noise


def test_maps_do_not_move_and_foam_is_one_answer(capi, oracle):
    N, C = 1024, 4
    maps = {}
    foams = {}
    for mode in ("off", "jacobian", "accumulate"):
        oc, ws = _setup(capi, oracle, N, C)
        with oc:
            oc.set_foam(mode)
            oc.update(DT)
            oc.displace()
            maps[mode] = [oc.read_maps(c) for c in range(C)]
    for c in range(C):
        assert np.array_equal(maps["off"][c], maps["jacobian"][c])
        assert np.array_equal(maps["off"][c], maps["accumulate"][c])
    del maps
    # one answer for every cascade group and every map-store policy
    for group in (1, 2, 4):
        for policy in ("auto", "written through", "streamed"):
            oc, ws = _setup(capi, oracle, N, C)
            with oc:
                oc.set_cascade_group(group)
                oc.set_map_store_policy(policy)
                oc.update(DT)
                oc.displace()
                foams[(group, policy)] = [oc.read_foam(c) for c in range(C)]
    base = foams[(1, "auto")]
    for key, f in foams.items():
        for c in range(C):
            assert np.array_equal(f[c], base[c]), (key, c)


def test_bound_plane(capi, oracle):
    import torch

    N, C = 256, 2
    outs = []
    for bound in (False, True):
        oc, ws = _setup(capi, oracle, N, C)
        with oc:
            buf = torch.full((C * N * N,), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            oc.set_foam("accumulate")
            if bound:
                oc.bind_foam(buf.data_ptr(), buf.numel() * 4)
                assert oc.foam_device() == (buf.data_ptr(), C * N * N * 4)
                for c in range(C):
                    oc.reset_foam(c)
            for _ in range(3):
                oc.update(DT)
                oc.displace()
            outs.append([oc.read_foam(c) for c in range(C)])
            if bound:
                oc.sync()
                got = buf.cpu().numpy().reshape(C, N, N)
                for c in range(C):
                    assert np.array_equal(got[c], outs[-1][c])
                oc.bind_foam(None, 0)
                assert oc.foam_device()[0] != buf.data_ptr()
    for c in range(C):
        assert np.array_equal(outs[0][c], outs[1][c])


def test_plane_bound_while_off(capi, oracle):
    # bind_foam is allowed in any mode: a plane bound while foam is off becomes the plane in use (zero-filled) when foam is switched on,
    # stays bound through off and on again, and bind_foam(None, 0) returns to the handle's own plane
    import torch

    N, C = 64, 2
    nbytes = C * N * N * 4
    zero = np.zeros((C, N, N), np.float32)
    oc, ws = _setup(capi, oracle, N, C, chops=[2.5, 3.0])
    with oc:
        oc.set_foam("off")
        buf = torch.full((C * N * N,), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        oc.bind_foam(buf.data_ptr(), nbytes)
        with pytest.raises(capi.OceanError) as e:
            oc.foam_device()
        assert e.value.code == capi.ESTATE
        oc.update(DT)
        oc.displace()                                # foam off: the bound plane is not touched
        oc.sync()
        assert np.array_equal(buf.cpu().numpy(), np.full(C * N * N, 7.0, np.float32))

        oc.set_foam("accumulate")
        assert oc.foam_device() == (buf.data_ptr(), nbytes)
        assert np.array_equal(buf.cpu().numpy().reshape(C, N, N), zero)
        for c in range(C):
            oc.set_foam_params(c, 1.5, 1.0, 1.0)    # coverage 1.5 - J wherever J < 1.5: nonzero over much of the sea
        for _ in range(2):
            oc.update(DT)
            oc.displace()
        oc.sync()
        got = buf.cpu().numpy().reshape(C, N, N)
        assert np.any(got > 0)
        for c in range(C):
            assert np.array_equal(got[c], oc.read_foam(c))

        oc.set_foam("off")
        oc.set_foam("jacobian")
        assert oc.foam_device() == (buf.data_ptr(), nbytes)
        assert np.array_equal(buf.cpu().numpy().reshape(C, N, N), zero)
        oc.displace()
        oc.sync()
        jac = buf.cpu().numpy().reshape(C, N, N)
        assert not np.array_equal(jac, zero)

        oc.bind_foam(None, 0)
        own, n = oc.foam_device()
        assert own != buf.data_ptr() and n == nbytes
        oc.displace()                                # the same maps again: the same J, now in the handle's own plane
        for c in range(C):
            assert np.array_equal(oc.read_foam(c), jac[c])
        assert np.array_equal(buf.cpu().numpy().reshape(C, N, N), jac)


def test_accumulation(capi, oracle, report):
    N, C = 256, 2
    params = [(0.5, 2.0, 1.0), (0.9, 4.0, 0.5)]
    rs = np.random.RandomState(11)
    oc, ws = _setup(capi, oracle, N, C, chops=[2.5, 3.5])
    worst = 0.0
    with oc:
        oc.set_foam("accumulate")
        oc.set_foam_params(1, *params[1])
        F64 = [np.zeros((N, N)) for _ in range(C)]
        bars = [np.zeros((N, N)) for _ in range(C)]
        for step in range(20):
            dts = [np.float32(v) for v in rs.uniform(0.005, 0.05, rs.randint(1, 4))]
            for dt in dts:
                oc.update(dt)
            oc.displace()
            dtsum = sum(float(v) for v in dts)
            for c in range(C):
                thr, gain, decay = params[c]
                maps = oc.read_maps(c)
                J64 = foam64.jacobian64(maps, ws[c], N)
                fade = float(np.float32(math.exp(-decay * dtsum)))
                F64[c] = np.maximum(foam64.coverage64(J64, thr, gain), F64[c] * fade)
                bars[c] = np.maximum(bars[c], gain * K_KERNEL * EPS * foam64.scale64(maps, ws[c], N))
                got = oc.read_foam(c).astype(np.float64)
                err = np.abs(got - F64[c]) - bars[c]
                worst = max(worst, float(err.max()) / EPS)
                assert float(err.max()) <= K_STEP * EPS, (step, c)
        assert 0.01 < float((F64[0] > 0).mean()) < 0.99          # the case exercises both the clamp and the fade
        # displace without update: dt = 0, fade = 1, same maps -- the same plane bit for bit
        before = [oc.read_foam(c) for c in range(C)]
        oc.displace()
        for c in range(C):
            assert np.array_equal(oc.read_foam(c), before[c])
    report(f"foam accumulation 20 steps N={N}: worst beyond the J bar {worst:.2f} eps (bar {K_STEP})")


def test_decay_zero_holds_the_maximum(capi, oracle):
    N = 256
    oc, ws = _setup(capi, oracle, N, 1, chops=[2.5])
    with oc:
        oc.set_foam("accumulate")
        oc.set_foam_params(0, 0.5, 2.0, 0.0)
        prev = np.zeros((N, N), np.float32)
        for _ in range(10):
            oc.update(np.float32(0.1))
            oc.displace()
            cur = oc.read_foam(0)
            maps = oc.read_maps(0)
            cov = foam64.coverage64(foam64.jacobian64(maps, ws[0], N), 0.5, 2.0)
            assert np.all(cur >= prev)
            bar = 2.0 * K_KERNEL * EPS * foam64.scale64(maps, ws[0], N)
            assert np.all(np.abs(cur - np.maximum(prev, cov)) <= bar)
            prev = cur


def test_resets(capi, oracle):
    import torch

    N, C = 256, 2
    oc, ws = _setup(capi, oracle, N, C, chops=[2.5, 3.0])
    zero = np.zeros((N, N), np.float32)
    with oc:
        oc.set_foam("accumulate")
        oc.set_foam_params(0, 0.9, 2.0, 0.0)
        oc.set_foam_params(1, 0.9, 2.0, 0.0)

        def run():
            for _ in range(3):
                oc.update(DT)
                oc.displace()
            f = [oc.read_foam(c) for c in range(C)]
            assert all(np.any(v > 0) for v in f)
            return f

        f = run()
        oc.reset_foam(0)
        assert np.array_equal(oc.read_foam(0), zero)
        assert np.array_equal(oc.read_foam(1), f[1])
        f = run()
        oc.upload_state(1, _h0(oracle, N, 1001, ws[1]), _phase(N, 78))
        assert np.array_equal(oc.read_foam(1), zero)
        assert np.array_equal(oc.read_foam(0), f[0])
        f = run()
        park = torch.empty(oc.state_bytes(), dtype=torch.uint8, device="cuda")
        flags = oc.park_state(0, park.data_ptr(), oc.state_bytes())
        oc.resume_state(0, park.data_ptr(), oc.state_bytes(), flags)
        assert np.array_equal(oc.read_foam(0), zero)
        assert np.array_equal(oc.read_foam(1), f[1])
        f = run()
        seed, _ = oracle.seed(N, 1000, ws[0], oracle.EXAMPLE["waveamplitude"], oracle.EXAMPLE["windspeed"], oracle.EXAMPLE["winddirection"], sanitize=True)
        oc.upload_seed(0, seed)
        oc.rebuild_height(0, ws[0], 0.003, 8.5, oracle.EXAMPLE["winddirection"])
        for c in range(C):
            assert np.array_equal(oc.read_foam(c), f[c])


def test_errors_and_off(capi, oracle):
    N = 64
    with capi.Ocean(N, 2) as oc:
        with pytest.raises(capi.OceanError) as e:
            oc.read_foam(0)
        assert e.value.code == capi.ESTATE
        with pytest.raises(capi.OceanError) as e:
            oc.foam_device()
        assert e.value.code == capi.ESTATE
        with pytest.raises(capi.OceanError) as e:
            oc.reset_foam(0)
        assert e.value.code == capi.ESTATE
        for bad in ((0, float("nan"), 2.0, 1.0), (0, 0.5, float("inf"), 1.0), (0, 0.5, -1.0, 1.0), (0, 0.5, 2.0, -0.1), (2, 0.5, 2.0, 1.0)):
            with pytest.raises(capi.OceanError) as e:
                oc.set_foam_params(*bad)
            assert e.value.code == capi.EINVAL
        with pytest.raises(capi.OceanError) as e:
            oc.set_foam(3)
        assert e.value.code == capi.EINVAL
        oc.set_foam("jacobian")
        assert oc.foam_device()[1] == 2 * N * N * 4
        with pytest.raises(capi.OceanError) as e:
            oc.read_foam(2)
        assert e.value.code == capi.EINVAL
        with pytest.raises(capi.OceanError) as e:
            oc.bind_foam(oc.foam_device()[0], 2 * N * N * 4 - 4)
        assert e.value.code == capi.EINVAL
        oc.set_foam("off")
        with pytest.raises(capi.OceanError):
            oc.foam_device()


def test_host_shim_matches_c_abi(capi, oracle):
    from datum_amd import host_api

    N = 256
    e = oracle.EXAMPLE
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, choppiness=2.5))
    params.seed_ocean(1000)
    h0 = params.height.copy()
    with host_api.OceanContext(N, device=0) as ctx:
        mesh = ctx.create_ocean(64, 64)
        ctx.set_foam("jacobian")
        for _ in range(4):
            params.update_ocean(DT)
            ctx.render_ocean_surface(mesh, params)
        ctx.fetch_ocean_state(params)
        maps = ctx.read_displacement()
        foam = ctx.read_foam()
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, e["wavescale"], 2.5)
        oc.upload_state(0, h0, params.phase.copy())
        oc.set_foam("jacobian")
        oc.displace()
        assert np.array_equal(oc.read_maps(0), maps)
        assert np.array_equal(oc.read_foam(0), foam)
    assert _kernel_k(foam.astype(np.float64), maps, float(np.float32(e["wavescale"])), N) <= K_KERNEL


def test_bound_maps_and_a_running_farm(capi, oracle):
    # foam reads whatever maps the handle writes: bound to caller memory, or while a (one-rank) farm gathers every step
    import torch

    N, C = 256, 2
    ref = None
    for case in ("own", "bound maps", "farm"):
        oc, ws = _setup(capi, oracle, N, C)
        with oc:
            oc.set_foam("accumulate")
            if case == "bound maps":
                buf = torch.zeros(C * N * N * 6, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                oc.bind_maps(buf.data_ptr(), buf.numel() * 4)
            if case == "farm":
                oc.farm_init(capi.farm_unique_id(), 0, 1, capi.PAYLOAD_XYZ16, slots=2)
            for _ in range(3):
                oc.update(DT)
                oc.displace()
                if case == "farm":
                    slot = oc.farm_gather()
                    oc.farm_wait(slot)
            got = [oc.read_foam(c) for c in range(C)]
            if case == "farm":
                oc.farm_shutdown()
            if case == "bound maps":
                oc.bind_maps(None, 0)
        if ref is None:
            ref = got
        for c in range(C):
            assert np.array_equal(got[c], ref[c]), (case, c)


def test_release_memory_with_foam_bound_inside_the_block(capi, oracle):
    # as tests/test_gpu_interop.py does for the maps: a foam plane bound at an offset inside an imported block, then the block is
    # released by its base pointer -- the handle falls back to its own plane instead of writing into unmapped memory
    import ctypes
    import os

    class ExtMem(ctypes.Structure):
        _fields_ = [("handle", ctypes.c_void_p), ("va", ctypes.c_void_p), ("bytes", ctypes.c_size_t)]

    helper = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu", "libextmem_helper.so"))
    helper.extmem_create.argtypes = [ctypes.c_size_t, ctypes.POINTER(ExtMem), ctypes.POINTER(ctypes.c_int)]
    helper.extmem_destroy.argtypes = [ctypes.POINTER(ExtMem)]
    N = 64
    nbytes = N * N * 4
    offset = 4096
    mem, fd = ExtMem(), ctypes.c_int(-1)
    assert helper.extmem_create(nbytes + offset, ctypes.byref(mem), ctypes.byref(fd)) == 0
    try:
        oc, ws = _setup(capi, oracle, N, 1)
        with oc:
            ptr = oc.import_memory_fd(fd.value, mem.bytes)
            oc.bind_foam(ptr + offset, nbytes)
            assert oc.foam_device()[0] == ptr + offset
            oc.update(DT)
            oc.displace()
            inside = oc.read_foam(0)
            oc.release_memory(ptr)                       # the plane was bound at ptr + offset
            assert oc.foam_device()[0] != ptr + offset
            oc.displace()                                # ... and now lands in the handle's own plane: no fault
            oc.sync()
            assert np.array_equal(oc.read_foam(0), inside)
    finally:
        assert helper.extmem_destroy(ctypes.byref(mem)) == 0


def test_upload_height_keeps_phase_and_accumulator(capi, oracle):
    N = 256
    oc, ws = _setup(capi, oracle, N, 1, chops=[2.5])
    with oc:
        oc.set_foam("accumulate")
        oc.set_foam_params(0, 1.0, 2.0, 0.0)
        for _ in range(3):
            oc.update(DT)
            oc.displace()
        before = oc.read_foam(0)
        assert before.any()
        oc.update(DT)                                    # queued: applied by the next displace, under the new h0
        oc.upload_height(0, _h0(oracle, N, 1000, ws[0], amplitude=0.003))
        assert np.array_equal(oc.read_foam(0), before)
        oc.displace()
        after = oc.read_foam(0)
        assert np.all(after >= before)                  # decay 0: the coverage so far is held
        phase = oc.read_state(0)
    # the phase as a fresh upload of the same state would carry it
    with capi.Ocean(N, 1) as ref:
        ref.set_cascade(0, ws[0], 2.5)
        ref.upload_state(0, _h0(oracle, N, 1000, ws[0]), _phase(N, 77))
        for _ in range(4):
            ref.update(DT)
        assert np.array_equal(ref.read_state(0), phase)


def test_host_shim_lerp_keeps_accumulation(capi):
    # with OceanParams::deviceheight off (the default) lerp_ocean_waves recomputes h0 on the host and the context replaces the
    # device's h0 of the SAME state: the accumulated coverage is kept
    from datum_amd import host_api

    N = 256
    params = host_api.OceanParams(N, **dict(host_api.EXAMPLE_TUNABLES, choppiness=2.5))
    params.seed_ocean(1000)
    s = params.scalars()
    with host_api.OceanContext(N, device=0) as ctx:
        mesh = ctx.create_ocean(64, 64)
        ctx.set_foam("accumulate")
        ctx.set_foam_params(1.0, 2.0, 0.0)
        for _ in range(3):
            params.update_ocean(DT)
            ctx.render_ocean_surface(mesh, params)
        before = ctx.read_foam()
        assert before.any()
        for t in (0.5, 0.5):
            params.lerp_ocean_waves(s.wavescale, s.waveamplitude * 1.5, s.windspeed * 1.2, tuple(s.winddirection), t)
            params.update_ocean(DT)
            ctx.render_ocean_surface(mesh, params)
        after = ctx.read_foam()
    assert np.all(after >= before)
