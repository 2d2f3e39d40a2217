"""The ripple layer of one handle as ONE model, driven by seeded call sequences (include/datum_ocean_hip.h from "ripple layer" to "ripple
swell").  The per-feature restatements pin every kernel from a state their tests set up; this module uses them TOGETHER, over long mixed
orders of calls, where the host code decides who re-rasters what, who zeroes which state buffer, who clears which mark and which of the
seven step kernels runs next (launch_ripple_step in datum_amd/csrc/ocean_capi.hip).

  Layer       ripple_swell64.Layer with the choice of launch_ripple_step stated once (family) and every sub-step recorded in a trace;
  Model       the handle's ripple side: the layer, the wake-foam plane, the bounds record, the three CURRENT marks (the layer's bounds, the
              swell plane's -- Layer.current -- and the FFT maps' bounds, which the bounded rippled cast also needs), the parameters that
              survive set_ripples.  One method per C-ABI call, each returning OK, EINVAL or ESTATE; a refused call changes nothing;
  Sea         the FFT ocean as the CPU half has it: an analytic height and velocity that change with every displace;
  sequence    (seed, length) -> a list of (name, args), a pure function of its arguments; args are numbers, strings and tuples of them;
  apply       one operation on a model, the heights and velocity records coming from a `sea` (Sea here, the device in the GPU test);
  observe     what the GPU test can read back, as bytes: the state in window order, the wall, bed and swell planes, the foam plane, the
              bounds record, the three marks.

`mistake` plants one wrong rule each (tests/test_ripple_seq_model.py shows that every one is seen by a committed seed):
  "stale"              a center_ripples that moves the origin leaves the swell mark standing (ripple_swell64's "stale")
  "walls_keep_swell"   set_ripple_walls leaves the swell mark standing
  "bed_no_reraster"    set_ripple_walls does not raster the bed again: the depth plane lacks the new walls, or keeps the old ones
  "raster_no_zero"     set_ripple_walls and set_ripple_bed zero no state: a new solid cell keeps its height until the next step
  "zero_keeps_bounds"  a zeroing raster (set_ripple_walls with a list, set_ripple_bed with a bed) leaves the bounds mark standing
  "foam_no_scroll"     center_ripples does not zero the foam plane's cells that entered the window
  "coupled_keeps_bounds"  step_bodies_coupled leaves the bounds mark standing
  "stale_read"         a step reads the swell plane although its mark is clear
  "src_every"          the memset of src runs ahead of every sub-step's launch, the first included: the pending deposits are lost.  (The
                       literal "behind every sub-step, not only behind the first" cannot be seen: no sub-step but a call's first reads
                       src, and nothing deposits inside a call of step_ripples.  This is the nearest rule that can.)
  "src_first_only"     its counterpart in coupled stepping, where every sub-step is a first one and the wake deposits between them: src is
                       cleared behind the call's first sub-step only, and the later sub-steps take the earlier wakes in again
  "swell_unsolid"      swell that is current with nothing solid runs the walls+swell family.  Its plane is +0 everywhere, so no plane and no
                       state differs by a bit: only the trace of families sees it, which is why the trace is among the observables
"""

import numpy as np

import body64
import couple64
import drag64
import ripple64
import ripple_bed64 as rb
import ripple_bounds64
import ripple_deep64 as rd
import ripple_foam64 as rf
import ripple_swell64 as rs
import ripple_wall64 as rw
import step64

F = np.float32
OK, EINVAL, ESTATE = 0, -1, -2
WAVE, DEEP = rs.WAVE, rs.DEEP

FAMILIES = ("plain", "deep", "walls", "walls_deep", "walls_swell", "bed", "bed_swell")
MISTAKES = ("stale", "walls_keep_swell", "bed_no_reraster", "raster_no_zero", "zero_keeps_bounds", "foam_no_scroll", "coupled_keeps_bounds",
            "stale_read", "src_every", "src_first_only", "swell_unsolid")

# the float64 bound of each family for one call from a common fp32 state, |eta - eta64| <= K eps max|eta64|: the restatements' own
K = {"plain": ripple64.K_RIP, "deep": rd.K_RIP_DEEP, "walls": rw.K_RIP_WALL[WAVE], "walls_deep": rw.K_RIP_WALL[DEEP], "walls_swell": rs.K_RIP_SWELL,
     "bed": rb.K_RIP_BED, "bed_swell": rs.K_RIP_SWELL}

TEXEL = 0.75                  # the bed maps' texel: no multiple of either cell side
CASCADES = ((0, 1, 2), (1,))  # the lists a refresh and a coupled step take


class Layer(rs.Layer):
    """ripple_swell64.Layer; `trace` receives the family of every sub-step"""

    def __init__(self, R, s, dtype, c, gamma, B, sponge_gamma, mode, g, G, trace, mistake):
        super().__init__(R, s, dtype, c, gamma, B, sponge_gamma, mode=mode, g=g, G=G)
        self.trace, self.mistake, self.keep_src = trace, mistake, False

    def family(self):
        """launch_ripple_step's choice from the mode, the walls, the bed and the swell plane while it is fresh"""
        m = self.mistake
        fresh = self.F is not None and (self.current or m == "stale_read")
        if self.bed is not None:
            return "bed_swell" if fresh else "bed"
        if fresh and self.mode == WAVE and (self.wall is not None or m == "swell_unsolid"):
            return "walls_swell"
        if self.wall is not None:
            return "walls_deep" if self.mode == DEEP else "walls"
        return "deep" if self.mode == DEEP else "plain"

    def advance(self, dt, substeps, dtype, src=None, trace=None):
        """(eta, rate, family) after `substeps` sub-steps of this state in `dtype`; the layer is not changed"""
        fam = self.family()
        T, B, ox, oy = dtype, self.B, self.ox, self.oy
        eta, rate = self.eta, self.rate
        src = self.src if src is None else src
        if fam in ("bed", "bed_swell"):
            h, gs2, f, fsurf = rb.params(self.g, self.s, self.gamma, B, self.sponge_gamma, self.bed["surf_gamma"], dt, substeps)
        elif fam in ("deep", "walls_deep"):
            h, gs, f = rd.params(self.g, self.s, self.gamma, B, self.sponge_gamma, dt, substeps)
        else:
            h, c2s2, f = ripple64.params(self.c, self.s, self.gamma, B, self.sponge_gamma, dt, substeps)
        for i in range(substeps):
            first = i == 0
            if fam == "plain":
                eta, rate = ripple64.substep(eta, rate, src, ox, oy, B, h, c2s2, f, first, T)
            elif fam == "deep":
                eta, rate = rd.substep(eta, rate, src, ox, oy, B, h, gs, f, self.G, first, T)
            elif fam == "walls":
                eta, rate = rw.substep_wave(eta, rate, src, self.wall, ox, oy, B, h, c2s2, f, first, T)
            elif fam == "walls_deep":
                eta, rate = rw.substep_deep(eta, rate, src, self.wall, ox, oy, B, h, gs, f, self.G, first, T)
            elif fam == "walls_swell":
                eta, rate = rs.substep_wave(eta, rate, src, self.wall, self.F, ox, oy, B, h, c2s2, f, first, T)
            elif fam == "bed":
                eta, rate = rb.substep(eta, rate, src, self.d, self.q, ox, oy, B, h, gs2, f, fsurf, first, T)
            else:
                eta, rate = rs.substep_bed(eta, rate, src, self.d, self.q, self.F, ox, oy, B, h, gs2, f, fsurf, first, T)
            if trace is not None:
                trace.append(fam)
        return eta, rate, fam

    def step(self, dt, substeps=1, mistake=None):
        src = np.zeros_like(self.src) if self.mistake == "src_every" else self.src
        eta, rate, _ = self.advance(dt, substeps, self.T, src, self.trace)
        self.eta, self.rate = eta.astype(self.T), rate.astype(self.T)
        if not self.keep_src:
            self.src = np.zeros_like(self.src)

    def set_walls(self, wl):
        m = self.mistake
        eta, rate, current, d, q = self.eta.copy(), self.rate.copy(), self.current, self.d, self.q
        super().set_walls(wl)
        if m == "raster_no_zero":
            self.eta, self.rate = eta, rate
        if m == "walls_keep_swell":
            self.current = current
        if m == "bed_no_reraster" and self.bed is not None:
            self.d, self.q = d, q

    def set_bed(self, b, depths=None):
        eta, rate = self.eta.copy(), self.rate.copy()
        super().set_bed(b, depths)
        if self.mistake == "raster_no_zero":
            self.eta, self.rate = eta, rate

    def move(self, ox, oy, mistake=None):
        super().move(ox, oy, "stale" if self.mistake == "stale" else None)

    def origin_of(self, x, y):
        return self.cell_of(x) - self.R // 2, self.cell_of(y) - self.R // 2


def wall_records(walls):
    """the tuples (kind, cx, cy, hx, hy, cos, sin) of an operation as ripple_wall64.WALL records"""
    return rw.walls(*[np.array([((cx, cy), (co, si), (hx, hy), kind, 0)], rw.WALL) for kind, cx, cy, hx, hy, co, si in walls])


def bed_record(args):
    """(record, depths) of a set_ripple_bed operation's args (kind, W, H, x0, y0, ax, ay, max_depth, dry_depth, surf_depth, surf_gamma):
    a map that falls along a diagonal through (ax, ay) -- "beach": from water to land, so that the dry cells are solid; "shelf": a step
    from shallow to deep water with nothing dry -- with an analytic relief on top"""
    kind, W, H, x0, y0, ax, ay, max_depth, dry_depth, surf_depth, surf_gamma = args
    X, Y = x0 + TEXEL * np.arange(W)[None, :], y0 + TEXEL * np.arange(H)[:, None]
    t = (X - ax) + 0.5 * (Y - ay)
    depth = 0.06 * t if kind == "beach" else 0.35 + 0.7 * (t > 0)
    depth = depth + 0.02 * np.sin(1.3 * X) * np.cos(0.7 * Y)
    return rb.bed(W, H, (x0, y0), TEXEL, outside=0.9, max_depth=max_depth, dry_depth=dry_depth, surf_depth=surf_depth, surf_gamma=surf_gamma), depth.astype(F)


def fleet(positions, velocity):
    """(bodies, motions, props, probes) of a coupled step's args: boxes of 3 x 3 probes half a metre apart (a = 0.25 m^2 each) whose
    bottoms hang 0.25 m under their positions, all moving with `velocity`, with linear drag"""
    g = np.array([-0.5, 0.0, 0.5])
    xx, yy = np.meshgrid(g, g)
    probes = np.zeros((9, 4), F)
    probes[:, 0], probes[:, 1], probes[:, 2], probes[:, 3] = xx.ravel(), yy.ravel(), -0.25, 0.25
    n = len(positions)
    bodies = body64.make_bodies([np.eye(3)] * n, np.asarray(positions, F).reshape(n, 3), [0] * n, [9] * n, [np.inf] * n)
    motions = drag64.make_motions(np.tile(np.asarray(velocity, F), (n, 1)), np.zeros((n, 3)), [500.0] * n, [0.0] * n)
    props = step64.make_props([1.0 / 800.0] * n, np.full((n, 3), 1.0e-3), [9.81] * n, [9810.0] * n)
    return bodies, motions, props, probes


class Sea:
    """the FFT ocean of the CPU half: heights and velocity records that are analytic in the point and change with every displace"""

    def __init__(self):
        self.epoch = 0

    def displace(self, dt):
        self.epoch += 1

    def reduce_bounds(self):
        pass

    def heights(self, cascades, points):
        p = np.asarray(points, np.float64).reshape(-1, 2)
        a = 0.4 * len(cascades)
        return (a * np.sin(0.31 * p[:, 0] + 0.17 * p[:, 1] + 0.7 * self.epoch) + 0.1 * np.cos(0.9 * p[:, 1] - 0.4 * p[:, 0])).astype(F)

    def velocity(self, cascades, points):
        p = np.asarray(points, np.float64).reshape(-1, 2)
        recs = np.zeros((len(p), 8), F)
        recs[:, 2] = 0.25 * self.heights(cascades, p)
        recs[:, 4] = 0.2 * np.cos(0.31 * p[:, 0] + 0.7 * self.epoch)
        recs[:, 6] = 0.1 * np.sin(0.17 * p[:, 1] + 0.7 * self.epoch)
        return recs


class Model:
    """the handle's ripple side; `G` the DEEP table (the library's where a test has it), `dtype` float32 (the bits) or float64"""

    def __init__(self, G=None, dtype=F, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.G, self.T, self.mistake = G, dtype, mistake
        self.c, self.gamma, self.B, self.sponge_gamma = 2.0, 0.05, 8, 4.0
        self.mode, self.g = WAVE, float(F(9.81))
        self.layer = self.foam = self.bounds = None
        self.bounds_current = self.fft_current = False
        self.families = []            # one entry per sub-step since the model was made
        self.refused = None           # the call a refusal's error text names

    # -- what the checks read

    def _off(self, name):
        if self.layer is None:
            self.refused = name
            return True
        return False

    def _refuse(self, code, name):
        self.refused = name
        return code

    def swell_on(self):
        return self.layer is not None and self.layer.F is not None

    def marks(self):
        """(the layer's bounds, the swell plane, the FFT maps' bounds)"""
        return self.bounds_current, bool(self.layer is not None and self.layer.current), self.fft_current

    def stable(self, dt, substeps):
        L = self.layer
        if not (np.isfinite(dt) and dt >= 0):
            return False
        if L.mode == DEEP:
            return rd.stable(L.g, L.s, dt, substeps, L.G)
        if L.bed is not None:
            return rb.stable(L.g, L.bed["max_depth"], L.s, dt, substeps)
        return ripple64.stable(L.c, L.s, dt, substeps)

    # -- the calls

    def set_ripples(self, R, s):
        """everything of the old layer goes: walls, bed, swell, wake foam, the bounds record and both of the layer's marks; the step
        parameters, the mode and g, and the foam's parameters stay"""
        self.layer = Layer(R, s, self.T, self.c, self.gamma, self.B, self.sponge_gamma, self.mode, self.g, self.G, self.families, self.mistake)
        self.foam = self.bounds = None
        self.bounds_current = False
        return OK

    def set_ripple_params(self, c, gamma, B, sponge_gamma):
        self.c, self.gamma, self.B, self.sponge_gamma = c, gamma, B, sponge_gamma
        if self.layer is not None:
            L = self.layer
            L.c, L.gamma, L.B, L.sponge_gamma = c, gamma, B, sponge_gamma
        return OK

    def set_ripple_dispersion(self, mode, g):
        if mode == DEEP and self.layer is not None and (self.layer.bed is not None or self.layer.F is not None):
            return self._refuse(ESTATE, "datum_ocean_set_ripple_dispersion")
        self.mode, self.g = mode, float(F(g))
        if self.layer is not None:
            self.layer.mode, self.layer.g = self.mode, self.g
        return OK

    def set_ripple_walls(self, walls):
        if self._off("datum_ocean_set_ripple_walls"):
            return ESTATE
        self.layer.set_walls(wall_records(walls) if len(walls) else None)
        if len(walls) and self.mistake != "zero_keeps_bounds":
            self.bounds_current = False
        return OK

    def set_ripple_bed(self, args):
        if self._off("datum_ocean_set_ripple_bed"):
            return ESTATE
        if args is not None and self.layer.mode == DEEP:
            return self._refuse(ESTATE, "datum_ocean_set_ripple_bed")
        if args is None:
            self.layer.set_bed(None)
            return OK
        self.layer.set_bed(*bed_record(args))
        if self.mistake != "zero_keeps_bounds":
            self.bounds_current = False
        return OK

    def set_ripple_swell(self, on):
        if self._off("datum_ocean_set_ripple_swell"):
            return ESTATE
        if on and self.layer.mode == DEEP:
            return self._refuse(ESTATE, "datum_ocean_set_ripple_swell")
        self.layer.set_swell(bool(on))
        return OK

    def refresh_ripple_swell(self, H):
        """H: the summed surface above Layer.points(), [R * R] or [R, R] in memory order"""
        if self._off("datum_ocean_refresh_ripple_swell") or not self.swell_on():
            return self._refuse(ESTATE, "datum_ocean_refresh_ripple_swell")
        L = self.layer
        L.refresh(np.asarray(H, F).reshape(L.R, L.R))
        return OK

    def center_ripples(self, x, y):
        if self._off("datum_ocean_center_ripples"):
            return ESTATE
        L = self.layer
        ox, oy = L.origin_of(x, y)
        if (ox, oy) == (L.ox, L.oy):
            return OK
        if self.foam is not None and self.mistake != "foam_no_scroll":
            self.foam.move(ox, oy)
        L.move(ox, oy)
        self.bounds_current = False
        return OK

    def reset_ripples(self):
        if self._off("datum_ocean_reset_ripples"):
            return ESTATE
        L = self.layer
        L.eta, L.rate, L.src = np.zeros_like(L.eta), np.zeros_like(L.rate), np.zeros_like(L.src)
        self.bounds_current = False
        if self.foam is not None:
            self.foam.reset()
        return OK

    def deposit_ripples_host(self, impulses):
        if self._off("datum_ocean_deposit_ripples_host"):
            return ESTATE
        self.layer.deposit(np.asarray(impulses, F).reshape(-1, 4))
        return OK

    def step_ripples(self, dt, substeps):
        if self._off("datum_ocean_step_ripples"):
            return ESTATE
        if not self.stable(dt, substeps):
            return self._refuse(EINVAL, "datum_ocean_step_ripples")
        self.bounds_current = False
        self.layer.step(dt, substeps)
        return OK

    def step_bodies_coupled_host(self, bodies, motions, props, probes, recs_of, dt, substeps):
        """(code, bodies', motions', records): couple64's loop over this layer's step; recs_of(bodies) gives the velocity records at
        couple64.points32(bodies, probes)"""
        name = "datum_ocean_step_bodies_coupled_host"
        if self._off(name):
            return ESTATE, bodies, motions, None
        if not self.stable(dt, substeps):
            return self._refuse(EINVAL, name), bodies, motions, None
        if self.mistake != "coupled_keeps_bounds":
            self.bounds_current = False
        L = self.layer
        h = step64.step_size(dt, substeps)
        rec = None
        for i in range(substeps):
            L.keep_src = self.mistake == "src_first_only" and i > 0
            if len(bodies):
                bodies, motions, rec, _ = couple64.substep32(L, bodies, motions, props, probes, recs_of(bodies), h, old=rec)
            else:
                L.step(h, 1)
        L.keep_src = False
        return OK, bodies, motions, rec

    def set_ripple_foam(self, on):
        if self._off("datum_ocean_set_ripple_foam"):
            return ESTATE
        self.foam = rf.Plane(self.layer, self.T) if on else None
        return OK

    def _foam_off(self, name):
        if self._off(name) or self.foam is None:
            self.refused = name
            return True
        return False

    def step_ripple_foam(self, dt):
        if self._foam_off("datum_ocean_step_ripple_foam"):
            return ESTATE
        self.foam.step(dt)
        return OK

    def reset_ripple_foam(self):
        if self._foam_off("datum_ocean_reset_ripple_foam"):
            return ESTATE
        self.foam.reset()
        return OK

    def reduce_ripple_bounds(self):
        if self._off("datum_ocean_reduce_ripple_bounds"):
            return ESTATE
        self.bounds = ripple_bounds64.fold(self.layer.state())
        self.bounds_current = True
        return OK

    def reduce_bounds(self):
        self.fft_current = True
        return OK

    def displace(self):
        self.fft_current = False
        return OK

    def cast_bounded(self):
        """what the bounded rippled cast returns on an empty ray list"""
        if self._off("datum_ocean_read_rays_rippled_bounded"):
            return ESTATE
        return OK if (self.bounds_current and self.fft_current) else self._refuse(ESTATE, "datum_ocean_read_rays_rippled_bounded")

    # -- the float64 form of the next step from this fp32 state

    def distance64(self, dt, substeps, every_first=False):
        """(|eta - eta64| / (eps max|eta64|), family) of step_ripples(dt, substeps) -- with `every_first` of `substeps` calls of
        step_ripples(h, 1), a coupled step without bodies -- from the current state, the fp32 planes common to both"""
        L = self.layer
        out = []
        for T in (F, np.float64):
            if every_first:
                h = step64.step_size(dt, substeps)
                eta, rate, src = L.eta, L.rate, L.src
                keep = L.eta, L.rate
                for _ in range(substeps):
                    L.eta, L.rate = eta, rate
                    eta, rate, fam = L.advance(h, 1, T, src)
                    src = np.zeros_like(src)
                L.eta, L.rate = keep
            else:
                eta, _, fam = L.advance(dt, substeps, T)
            out.append(eta.astype(np.float64))
        top = np.abs(out[1]).max()
        return (float(np.abs(out[0] - out[1]).max() / (2.0 ** -24 * top)) if top > 0 else 0.0), fam


def observe(m):
    """the model's observables as a dict of bytes and tuples: equal dicts are equal bits"""
    L = m.layer
    out = {"marks": m.marks(), "bounds": None if m.bounds is None else m.bounds.tobytes()}
    if L is None:
        return out
    out["state"] = np.ascontiguousarray(L.window(), F).tobytes()
    out["walls"] = None if L.wall is None else L.wall_window().tobytes()
    out["bed"] = None if L.bed is None else (np.ascontiguousarray(L.window(L.d), F).tobytes(), L.window(L.q).tobytes())
    out["swell"] = None if L.F is None else np.ascontiguousarray(L.F, F).tobytes()
    out["foam"] = None if m.foam is None else np.ascontiguousarray(m.foam.window(), F).tobytes()
    return out


def apply(m, op, sea):
    """one operation on the model; returns (code, extra) -- extra is (bodies', motions', records) behind a coupled step, else None"""
    name, a = op
    if name == "set_ripple_walls":
        return m.set_ripple_walls(a), None
    if name == "set_ripple_bed":
        return m.set_ripple_bed(a), None
    if name == "refresh_ripple_swell":
        if m.layer is None or not m.swell_on():
            return m.refresh_ripple_swell(None), None
        return m.refresh_ripple_swell(sea.heights(a, m.layer.points())), None
    if name == "deposit_ripples_host":
        return m.deposit_ripples_host(a), None
    if name == "step_bodies_coupled_host":
        cascades, positions, velocity, dt, substeps = a
        bodies, motions, props, probes = fleet(positions, velocity)
        code, b, mo, rec = m.step_bodies_coupled_host(bodies, motions, props, probes, lambda b: sea.velocity(cascades, couple64.points32(b, probes)), dt, substeps)
        return code, (b, mo, rec)
    if name == "displace":
        sea.displace(*a)
        return m.displace(), None
    if name == "reduce_bounds":
        sea.reduce_bounds()
        return m.reduce_bounds(), None
    return getattr(m, name)(*a), None


def brief(op):
    """an operation in one short line, for an assertion's message"""
    name, a = op
    if name == "deposit_ripples_host":
        return f"{name}({len(a)} impulses)"
    if name == "set_ripple_walls":
        return f"{name}({len(a)} records)"
    if name == "set_ripple_bed":
        return f"{name}({a[0] if a else None})"
    if name == "step_bodies_coupled_host":
        return f"{name}({len(a[1])} bodies, dt={a[3]}, substeps={a[4]})"
    return f"{name}{tuple(a)}"


# -- the generator


class _Shadow:
    """what the generator has to know of the handle to keep every operation valid or a documented refusal: the switches, the origin, the
    parameters the stability bounds read, and whether the swell plane is current (to put a step behind a refresh often enough)"""

    def __init__(self):
        self.R = self.s = None
        self.ox = self.oy = 0
        self.c, self.g, self.mode = 2.0, 9.81, WAVE
        self.walls = self.swell = self.foam = self.current = False
        self.max_depth = None         # the bed's, None while it is off

    def hmax(self):
        """the longest sub-step the mode accepts"""
        if self.mode == DEEP:
            return 1.9 / np.sqrt(self.g * _MASS / self.s)
        if self.max_depth is not None:
            return 0.7 * self.s / np.sqrt(self.g * self.max_depth)
        return 0.7 * self.s / self.c


_MASS = rd.mass(rd.weights32())


def _r(v):
    """a Python float that is an fp32 value: what reaches the model is what reaches the C ABI"""
    return float(F(v))


def _wall_list(rng, S):
    R, s, ox, oy = S.R, S.s, S.ox, S.oy
    x = lambda i: _r((ox + i + 0.5) * s)
    y = lambda j: _r((oy + j + 0.5) * s)
    sx, sy = (-ox) & (R - 1), (-oy) & (R - 1)                  # the window cell memory cell (0, 0) holds: the torus seam
    shapes = {"box": (rw.BOX, x(R // 2), y(R // 3), _r(4.3 * s), _r(1.2 * s), 1.0, 0.0),
              "ellipse": (rw.ELLIPSE, x(R // 4), y(3 * R // 4), _r(5.3 * s), _r(2.6 * s), _r(0.8), _r(0.6)),
              "rotated": (rw.BOX, x(3 * R // 4), y(3 * R // 4), _r(4.3 * s), _r(1.2 * s), _r(0.6), _r(0.8)),
              "pillar": (rw.BOX, x(3 * R // 4), y(R // 4), _r(0.3 * s), _r(0.3 * s), 1.0, 0.0),
              "edge": (rw.BOX, x(R // 2), y(0), _r(9.0 * s), _r(1.2 * s), 1.0, 0.0),
              "seam": (rw.BOX, x(sx), y(sy), _r(3.2 * s), _r(2.2 * s), 1.0, 0.0)}
    names = sorted(shapes)
    pick = [names[k] for k in sorted(rng.choice(len(names), int(rng.randint(1, 4)), replace=False))]
    return tuple(shapes[n] for n in pick)


def _bed_args(rng, S, kind):
    R, s, ox, oy = S.R, S.s, S.ox, S.oy
    W = H = int((R - 12) * s / TEXEL)                          # smaller than the window: a margin of six cells reads `outside`
    px, py = int(rng.randint(R // 4, 3 * R // 4)), int(rng.randint(R // 4, 3 * R // 4))
    surf = bool(rng.randint(2))
    return (kind, W, H, _r((ox + 6) * s), _r((oy + 6.5) * s), _r((ox + px + 0.5) * s), _r((oy + py + 0.5) * s), _r(1.2), _r(0.02),
            _r(0.6 if surf else 0.0), _r(3.0 if surf else 0.0))


def _impulses(rng, S, n=48):
    lo = np.array([S.ox - 4, S.oy - 4]) * S.s
    p = lo + rng.uniform(0, 1, (n, 2)) * (S.R + 8) * S.s       # four cells beyond every edge: some land outside the window
    v = rng.uniform(0.005, 0.03, n) * rng.choice([-1.0, 1.0], n) * S.s * S.s
    return tuple((_r(p[k, 0]), _r(p[k, 1]), _r(v[k]), 0.0) for k in range(n))


def _dt(rng, S, substeps, over):
    """a step length well inside the mode's bound (0.3 .. 0.6 of it), or twice the bound"""
    return _r(S.hmax() * substeps * (2.0 if over else rng.uniform(0.3, 0.6)))


def sequence(seed, length):
    """`length` operations (a few more where one choice emits two) from numpy.random.RandomState(seed) alone"""
    rng = np.random.RandomState(seed)
    S = _Shadow()
    ops = []

    def set_ripples():
        S.R, S.s = int(rng.choice([64, 128])), float(rng.choice([0.5, 1.0]))
        S.ox = S.oy = -S.R // 2
        S.walls = S.swell = S.foam = S.current = False
        S.max_depth = None
        ops.append(("set_ripples", (S.R, S.s)))

    def set_params():
        S.c = float(rng.choice([1.5, 2.0, 3.0]))
        ops.append(("set_ripple_params", (S.c, float(rng.choice([0.0, 0.05])), int(rng.choice([0, 5, 8])), float(rng.choice([2.0, 4.0])))))

    def set_dispersion():
        mode, g = int(rng.randint(2)), _r(rng.choice([9.81, 4.0]))
        if not (mode == DEEP and (S.max_depth is not None or S.swell)):           # else refused: nothing changes
            S.mode, S.g = mode, g
        ops.append(("set_ripple_dispersion", (mode, g)))

    def set_walls():
        wl = () if (S.walls and rng.randint(3) == 0) else _wall_list(rng, S)
        S.walls, S.current = len(wl) > 0, False
        ops.append(("set_ripple_walls", wl))

    def set_bed():
        kind = ["shelf", "beach", "beach+walls"][int(rng.randint(3))]
        if S.max_depth is not None and rng.randint(5) < 2:
            kind = None
        if kind == "beach+walls":                                                  # a bed with walls on top
            set_walls()
            kind = "beach"
        args = None if kind is None else _bed_args(rng, S, kind)
        if args is None or S.mode == WAVE:                                         # else refused
            S.max_depth, S.current = (None if args is None else args[7]), False
        ops.append(("set_ripple_bed", args))

    def set_swell():
        on = 0 if (S.swell and rng.randint(3) == 0) else 1
        if not (on and S.mode == DEEP):
            S.swell, S.current = bool(on), False
        ops.append(("set_ripple_swell", (on,)))

    def refresh():
        S.current = True
        ops.append(("refresh_ripple_swell", CASCADES[int(rng.randint(2))]))

    def center():
        R, s = S.R, S.s
        kind = int(rng.randint(4))
        if kind == 0:                                                              # the same cell: no move
            ox, oy = S.ox, S.oy
        elif kind == 1:                                                            # a few cells
            ox, oy = S.ox + int(rng.randint(-5, 6)), S.oy + int(rng.randint(-5, 6))
        elif kind == 2:                                                            # the torus seam inside a 64 x 16 tile of the step
            ox, oy = S.ox + int(rng.randint(-20, 21)), S.oy + int(rng.randint(-20, 21))
            ox += 1 if ox % 64 == 0 else 0
            oy += 1 if oy % 16 == 0 else 0
        else:                                                                      # R cells or more: the layer is cleared
            ox, oy = S.ox + int(rng.choice([-1, 1])) * (R + int(rng.randint(0, 40))), S.oy + int(rng.randint(-R, R))
        if (ox, oy) != (S.ox, S.oy):
            S.current = False
        S.ox, S.oy = ox, oy
        ops.append(("center_ripples", (_r((ox + R // 2 + 0.5) * s), _r((oy + R // 2 + 0.5) * s))))

    def step():
        n = int(rng.choice([1, 3, 8]))
        ops.append(("step_ripples", (_dt(rng, S, n, rng.randint(12) == 0), n)))

    def coupled():
        nb, n = int(rng.choice([0, 3])), int(rng.randint(1, 4))
        lo, w = np.array([S.ox, S.oy]) * S.s, S.R * S.s
        # one body in open water, one on the window's edge, one that hangs over it
        pos = [(lo[0] + rng.uniform(0.3, 0.7) * w, lo[1] + rng.uniform(0.3, 0.7) * w), (lo[0] + 0.2, lo[1] + rng.uniform(0.2, 0.8) * w), (lo[0] + w - 0.1, lo[1] + w - 0.1)][:nb]
        positions = tuple((_r(p[0]), _r(p[1]), _r(-0.1)) for p in pos)
        velocity = (_r(rng.uniform(-1, 1)), _r(rng.uniform(-1, 1)), _r(rng.uniform(-0.3, 0.0)))
        ops.append(("step_bodies_coupled_host", (CASCADES[int(rng.randint(2))], positions, velocity, _dt(rng, S, n, rng.randint(12) == 0), n)))

    def set_foam():
        S.foam = not (S.foam and rng.randint(3) == 0)
        ops.append(("set_ripple_foam", (int(S.foam),)))

    plain = {"reset_ripples": lambda: ops.append(("reset_ripples", ())),
             "deposit": lambda: ops.append(("deposit_ripples_host", _impulses(rng, S))),
             "step_foam": lambda: ops.append(("step_ripple_foam", (_r(rng.choice([0.0, 0.1, 0.3])),))),
             "reset_foam": lambda: ops.append(("reset_ripple_foam", ())),
             "reduce_ripple_bounds": lambda: ops.append(("reduce_ripple_bounds", ())),
             "reduce_bounds": lambda: ops.append(("reduce_bounds", ())),
             "displace": lambda: ops.append(("displace", (_r(rng.choice([1.0 / 60.0, 0.05])),)))}
    table = dict(plain, set_ripples=set_ripples, set_params=set_params, set_dispersion=set_dispersion, set_walls=set_walls, set_bed=set_bed, set_swell=set_swell,
                 refresh=refresh, center=center, step=step, coupled=coupled, set_foam=set_foam)

    set_ripples()
    while len(ops) < length:
        solid = S.walls or S.max_depth is not None
        w = {"set_ripples": 1.0, "set_params": 1.0, "set_dispersion": 2.5, "set_walls": 3.0, "set_bed": 3.0, "set_swell": 3.0, "center": 3.5, "reset_ripples": 0.7,
             "deposit": 4.0, "step": 5.0, "coupled": 2.5, "set_foam": 1.5, "reduce_ripple_bounds": 4.0, "reduce_bounds": 1.5, "displace": 1.5}
        if S.swell:
            w["refresh"] = 1.0 if S.current else (6.0 if solid else 2.0)
            if S.current:                                                          # a fresh plane is there to be stepped with, or cleared
                w["step"], w["coupled"] = 9.0, 4.0
        if S.foam:
            w["step_foam"], w["reset_foam"] = 3.0, 0.5
        if S.mode == DEEP:                                                         # the bed and swell would be refused: sometimes, not mostly
            w["set_bed"], w["set_swell"], w["set_walls"], w["set_dispersion"] = 0.8, 0.8, 4.0, 1.5
        elif S.max_depth is None and not S.swell:                                  # nothing stands in DEEP's way
            w["set_dispersion"] = 4.0
        if S.max_depth is not None:
            w["set_bed"] = 2.0
        names = sorted(w)
        p = np.array([w[n] for n in names])
        table[names[int(rng.choice(len(names), p=p / p.sum()))]]()
    return ops


# The committed sequences: twelve seeds of forty operations.  The seeds were picked, out of 0 .. 149, for the coverage conditions of
# tests/test_ripple_seq_model.py; a seed whose sequence found a bug stays (DESIGN.md 8 names it)
LENGTH = 40
SEEDS = (0, 3, 6, 12, 14, 18, 23, 45, 101, 123, 124, 143)
