"""The ripple layer on the MI355X under seeded call sequences (tests/ripple_seq.py), through the C ABI, against ONE model of the handle's
ripple side.  The features' own files pin each kernel from a state they set up; here forty mixed calls per seed decide who re-rasters
what, who zeroes which state buffer, who clears which mark and which of the seven step kernels runs next.  tests/test_ripple_seq_model.py
shows on the CPU that these sequences see every planted mistake of that kind.

N = 64 maps, three cascades, velocity on; the layer is R = 64 or 128 as the sequence says: the smallest shapes at which every step kernel
(tile 64 x 16) still has a tile seam, a torus wrap inside a tile and a halo.

Behind EVERY operation, bit for bit: the return code (and the call's name in a refusal's text); read_ripples; the wall, bed and swell
planes (or that they are gone); the swell's CURRENT flag; the foam plane; the bounded rippled cast on an empty ray list, which is OK
exactly when the model's two bounds marks stand.  Behind a coupled step the bodies, motions and records against couple64's loop over the
model's step, the velocity records read from the device; behind reduce_ripple_bounds the record against ripple_bounds64.fold by value;
every eighth operation query_ripples, query_ripple_foam and read_surface_blend_rippled at 16 points in and beside the window.  A
refresh feeds the model read_surface_blend's heights at Layer.points().  No operation is retried.
"""

import ctypes
import time

import numpy as np
import pytest

import ripple_bounds64
import ripple_deep64 as rd
import ripple_seq as rq
import rippled64
from test_gpu_body import _step
from test_gpu_surface import _set, _setup

pytestmark = pytest.mark.gpu

F = np.float32
IT = 4


@pytest.fixture(scope="module")
def capi():
    from datum_amd import capi as c

    c.load()
    return c


@pytest.fixture(scope="module")
def table(capi):
    G = np.zeros((rd.Q, rd.Q), F)
    assert capi.load().datum_ocean_ripple_deep_weights(G.ctypes.data_as(capi.P)) == capi.OK
    return G


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class _Sea:
    """ripple_seq's sea on the device: the heights and velocity records are the handle's own reads"""

    def __init__(self, oc, s):
        self.oc, self.s = oc, s

    def displace(self, dt):
        self.oc.update(dt)
        self.oc.displace()

    def reduce_bounds(self):
        self.oc.reduce_bounds()

    def heights(self, cascades, points):
        return self.oc.read_surface_blend(list(cascades), self.s, points, IT)[:, 2]

    def velocity(self, cascades, points):
        return self.oc.read_velocity_blend(list(cascades), self.s, points, IT)


def _device(capi, oc, s, op):
    """the operation on the handle: (code, error text, extra) -- extra is (bodies, motions, records) behind a coupled step with bodies"""
    name, a = op
    extra = None
    try:
        if name == "set_ripple_walls":
            oc.set_ripple_walls(rq.wall_records(a) if len(a) else None)
        elif name == "set_ripple_bed":
            oc.set_ripple_bed(*(rq.bed_record(a) if a is not None else (None, None)))
        elif name == "refresh_ripple_swell":
            oc.refresh_ripple_swell(list(a), s, IT)
        elif name == "deposit_ripples_host":
            oc.deposit_ripples_host(np.asarray(a, F))
        elif name == "step_bodies_coupled_host":
            cascades, positions, velocity, dt, substeps = a
            if len(positions):
                bodies, motions, props, probes = rq.fleet(positions, velocity)
                rec = oc.step_bodies_coupled_host(list(cascades), s, bodies, motions, props, probes, dt, substeps, IT)
                extra = (bodies, motions, rec)
            else:
                arr, n = oc._list(cascades)
                oc._check(oc.lib.datum_ocean_step_bodies_coupled_host(oc.h, arr, n, ctypes.byref(s), IT, None, None, None, 0, None, 0, dt, substeps, None))
        elif name == "displace":
            oc.update(a[0])
            oc.displace()
        else:
            getattr(oc, name)(*a)
    except capi.OceanError as e:
        return e.code, str(e), None
    return capi.OK, "", extra


def _first(got, want):
    d = np.argwhere(np.asarray(got) != np.asarray(want))
    return None if not len(d) else (tuple(int(v) for v in d[0]), len(d))


def _points(L, k):
    """16 points in and beside the window: cell centres, cell corners, the window's edges, one far outside"""
    rng = np.random.RandomState(k)
    lo, w = np.array([L.ox, L.oy]) * float(L.s), L.R * float(L.s)
    p = lo + rng.uniform(-0.1, 1.1, (16, 2)) * w
    p[0], p[1], p[2] = lo, lo + w, lo + 0.5 * float(L.s)
    p[3] = lo - 1000.0
    return p.astype(F)


@pytest.mark.parametrize("seed", rq.SEEDS)
def test_sequence(capi, oracle, report, table, seed):
    t0 = time.perf_counter()
    ops = rq.sequence(seed, rq.LENGTH)
    m = rq.Model(G=table)
    lib = capi.load()
    with _setup(capi, oracle, 64, 3) as oc:
        oc.set_velocity("on")
        _step(oc)
        s = _set(capi, 0)
        sea = _Sea(oc, s)
        arr = (capi.I * 3)(0, 1, 2)
        families = 0
        for k, op in enumerate(ops):
            n = len(m.families)
            # the model first where it reads the device (a refresh's heights, a coupled step's velocity records): the FFT surface is
            # frozen over the call, so the reads give what the kernels see
            want_code, want = rq.apply(m, op, sea) if op[0] not in ("displace", "reduce_bounds") else (getattr(m, op[0])(), None)
            code, text, got = _device(capi, oc, s, op)
            fam = sorted(set(m.families[n:]))
            families += len(m.families) - n

            def where(what, first=None):
                return (f"seed {seed}, operation {k} {rq.brief(op)}: {what} differs; the model's kernel family {fam or None}; first differing cell and count {first}; "
                        f"replay: ripple_seq.sequence({seed}, {rq.LENGTH})[:{k + 1}] = {[rq.brief(o) for o in ops[:k + 1]]}")

            assert code == want_code, where(f"the return code ({code} for {want_code}, {text!r})")
            if code != capi.OK:
                assert m.refused in text, where(f"the refusal's text {text!r}")
            L = m.layer
            if L is None:
                continue
            state = oc.read_ripples()
            assert np.array_equal(_bits(state), _bits(L.window())), where("read_ripples", _first(_bits(state), _bits(L.window())))
            assert oc.ripples_device()[2:] == (L.ox, L.oy), where("the origin")
            if L.wall is None:
                assert oc.ripple_walls_device() is None, where("walls off")
            else:
                wall = oc.read_ripple_walls()
                assert np.array_equal(wall, L.wall_window()), where("read_ripple_walls", _first(wall, L.wall_window()))
            if L.bed is None:
                assert oc.ripple_bed_device() == (None, None, 0), where("bed off")
            else:
                d, q = oc.read_ripple_bed()
                wd, wq = L.bed_window()
                assert np.array_equal(_bits(d), _bits(wd)), where("read_ripple_bed depth", _first(_bits(d), _bits(wd)))
                assert np.array_equal(q, wq), where("read_ripple_bed surf", _first(q, wq))
            if L.F is None:
                assert oc.ripple_swell_device() == (None, 0, False), where("swell off")
            else:
                assert oc.ripple_swell_device()[2] is bool(L.current), where("the swell's CURRENT flag")
                plane = oc.read_ripple_swell()
                assert np.array_equal(_bits(plane), _bits(L.F)), where("read_ripple_swell", _first(_bits(plane), _bits(L.F)))
            if m.foam is None:
                assert lib.datum_ocean_reset_ripple_foam(oc.h) == capi.ESTATE, where("foam off")
            else:
                foam = oc.read_ripple_foam()
                assert np.array_equal(_bits(foam), _bits(m.foam.window())), where("read_ripple_foam", _first(_bits(foam), _bits(m.foam.window())))
            if want is not None and got is not None:
                for what, g, w in zip(("bodies", "motions"), got, want):
                    assert g.tobytes() == w.tobytes(), where(f"the coupled step's {what}", _first(g.view(np.uint8), w.view(np.uint8)))
                gn, wn = np.isnan(got[2]), np.isnan(want[2])
                assert np.array_equal(gn, wn) and np.array_equal(_bits(got[2])[~gn], _bits(want[2])[~wn]), where("the coupled step's records", _first(_bits(got[2]), _bits(want[2])))
            # the marks: the bounded rippled cast takes an empty list exactly when both stand
            cast = lib.datum_ocean_read_rays_rippled_bounded(oc.h, arr, 3, ctypes.byref(s), IT, 32, 8, None, 0, None)
            assert cast == m.cast_bounded(), where(f"the bounded rippled cast's code ({cast}; the model's marks {m.marks()})")
            if cast != capi.OK:
                assert b"datum_ocean_read_rays_rippled_bounded" in lib.datum_ocean_last_error(oc.h), where("the bounded cast's refusal text")
            if op[0] == "reduce_ripple_bounds":
                rec = oc.read_ripple_bounds()
                assert np.array_equal(rec, ripple_bounds64.fold(L.state())) and np.array_equal(rec, m.bounds), where("read_ripple_bounds", (rec.tolist(), m.bounds.tolist()))
            if k % 8 == 7 or k == len(ops) - 1:
                p = _points(L, k)
                samples = oc.query_ripples(p)
                assert np.array_equal(_bits(samples), _bits(L.sample(p))), where("query_ripples", _first(_bits(samples), _bits(L.sample(p))))
                if m.foam is not None:
                    f = oc.query_ripple_foam(p)
                    assert np.array_equal(_bits(f), _bits(m.foam.sample(p))), where("query_ripple_foam", _first(_bits(f), _bits(m.foam.sample(p))))
                rippled = oc.read_surface_blend_rippled([0, 1, 2], s, p, IT)
                wr = rippled64.record32(oc.read_surface_blend([0, 1, 2], s, p, IT), samples)
                cols = [0, 1, 2, 3, 7]
                assert np.array_equal(_bits(rippled[:, cols]), _bits(wr[:, cols])), where("read_surface_blend_rippled", _first(_bits(rippled[:, cols]), _bits(wr[:, cols])))
        assert families > 0 and np.isfinite(m.layer.eta).all()
    line = f"ripple sequences: seed {seed}, {len(ops)} operations, {families} sub-steps, {time.perf_counter() - t0:.2f} s"
    print(line)
    report(line)
