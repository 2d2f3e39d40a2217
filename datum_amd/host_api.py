"""ctypes view of the C++ host shim (datum_amd/host/ocean.h through host_capi.cpp).

Mirrors the reference's call sites: OceanParams + seed_ocean / lerp_ocean_* / update_ocean on the host,
OceanContext + initialise/prepare/render_ocean_surface over the HIP module.  No compute in Python.
"""

import ctypes
import os
from typing import NamedTuple

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(_HERE, "lib", "libdatum_ocean_host.so")

F, I, P, U32 = ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32


class OceanRippleBounds(NamedTuple):
    """ocean.h's OceanRippleBounds"""
    etamin: np.float32
    etamax: np.float32
    ratemin: np.float32
    ratemax: np.float32
    nonfinite: int
    active: int


class Scalars(ctypes.Structure):
    _fields_ = [
        ("plane", F * 4),
        ("swelllength", F), ("swellamplitude", F), ("swellsteepness", F), ("swellspeed", F),
        ("swelldirection", F * 2),
        ("wavescale", F), ("waveamplitude", F), ("windspeed", F),
        ("winddirection", F * 2),
        ("choppiness", F), ("smoothing", F),
        ("swellphase", F),
        ("flow", F * 2),
        ("resolution", I), ("rejectedseeds", I), ("pending", I),
    ]


class CameraDesc(ctypes.Structure):
    _fields_ = [("fov", F), ("aspect", F), ("znear", F), ("zfar", F), ("position", F * 3), ("target", F * 3), ("up", F * 3)]


def example_camera():
    """examples/ocean/ocean.cpp:33,63 with examples/ocean/ocean.h:17-18"""
    c = CameraDesc()
    c.fov = np.float32(60.0) * np.float32(np.pi) / np.float32(180.0)
    c.aspect = np.float32(1920.0) / np.float32(1080.0)
    c.znear, c.zfar = 0.1, 24000.0
    c.position[:] = (0, 0, 8)
    c.target[:] = (1, 0, 8)
    c.up[:] = (0, 0, 1)
    return c


_lib = None


def load():
    global _lib
    if _lib is None:
        capi.load()  # dependency, and fails loudly first
        if not os.path.exists(LIBPATH):
            raise OSError(f"{LIBPATH} not found: build the host shim first (`make` or __graft_entry__.build())")
        lib = ctypes.CDLL(LIBPATH)
        sig = {
            "datum_host_last_error": (ctypes.c_char_p, []),
            "datum_host_params_create": (P, [I]),
            "datum_host_params_destroy": (None, [P]),
            "datum_host_params_clone": (P, [P]),
            "datum_host_params_get": (None, [P, ctypes.POINTER(Scalars)]),
            "datum_host_params_set": (None, [P, ctypes.POINTER(Scalars)]),
            "datum_host_params_set_deviceheight": (None, [P, I]),
            "datum_host_params_set_hostphase": (I, [P, I]),
            "datum_host_params_poke_hostphase": (None, [P, I]),
            "datum_host_release_parked_states": (ctypes.c_size_t, [P, P]),
            "datum_host_parked_states": (I, [P]),
            "datum_host_params_to_pod": (I, [P, P]),
            "datum_host_params_from_pod": (P, [P]),
            "datum_host_pod_bytes": (I, []),
            "datum_host_params_seed": (ctypes.POINTER(F), [P]),
            "datum_host_params_height": (ctypes.POINTER(F), [P]),
            "datum_host_params_phase": (ctypes.POINTER(F), [P]),
            "datum_host_seed_ocean": (None, [P, U32, I]),
            "datum_host_lerp_ocean_swell": (None, [P, F, F, F, F, F, F]),
            "datum_host_lerp_ocean_waves": (None, [P, F, F, F, F, F, F]),
            "datum_host_update_ocean": (I, [P, F]),
            "datum_host_make_oceanset": (None, [ctypes.POINTER(CameraDesc), P, ctypes.POINTER(capi.OceanSet)]),
            "datum_host_twiddle_table": (I, [I, P]),
            "datum_host_context_create": (P, [I, I]),
            "datum_host_context_create_ex": (P, [I, I, I]),
            "datum_host_context_destroy": (None, [P]),
            "datum_host_context_handle": (P, [P]),
            "datum_host_ocean_create": (P, [P, I, I]),
            "datum_host_ocean_release": (None, [P, P]),
            "datum_host_ocean_vertices": (P, [P]),
            "datum_host_ocean_indices": (I, [P, P, P]),
            "datum_host_render_ocean_surface": (I, [P, P, ctypes.POINTER(CameraDesc), P]),
            "datum_host_displace_ocean_surface": (I, [P, P]),
            "datum_host_fetch_ocean_state": (I, [P, P]),
            "datum_host_read_ocean_displacement": (I, [P, P]),
            "datum_host_read_ocean_vertices": (I, [P, P, P]),
            "datum_host_set_ocean_foam": (I, [P, I]),
            "datum_host_set_ocean_foam_params": (I, [P, F, F, F]),
            "datum_host_read_ocean_foam": (I, [P, P]),
            "datum_host_query_ocean_surface": (I, [P, P, P, ctypes.c_size_t, P, I]),
            "datum_host_set_ocean_velocity": (I, [P, I]),
            "datum_host_read_ocean_velocity": (I, [P, P]),
            "datum_host_query_ocean_velocity": (I, [P, P, P, ctypes.c_size_t, P, I]),
            "datum_host_reduce_ocean_bodies": (I, [P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, P, I]),
            "datum_host_reduce_ocean_body_drag": (I, [P, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, P, I]),
            "datum_host_step_ocean_bodies": (I, [P, P, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, I, P, I]),
            "datum_host_set_ocean_ripples": (I, [P, I, F]),
            "datum_host_set_ocean_ripple_dispersion": (I, [P, I, F]),
            "datum_host_set_ocean_ripple_walls": (I, [P, P, ctypes.c_size_t]),
            "datum_host_read_ocean_ripple_walls": (I, [P, P]),
            "datum_host_set_ocean_ripple_bed": (I, [P, P, P]),
            "datum_host_read_ocean_ripple_bed": (I, [P, P, P]),
            "datum_host_set_ocean_ripple_swell": (I, [P, I]),
            "datum_host_refresh_ocean_ripple_swell": (I, [P, P, I]),
            "datum_host_read_ocean_ripple_swell": (I, [P, P]),
            "datum_host_center_ocean_ripples": (I, [P, F, F]),
            "datum_host_deposit_ocean_ripples": (I, [P, P, ctypes.c_size_t]),
            "datum_host_deposit_ocean_body_ripples": (I, [P, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, P, I]),
            "datum_host_step_ocean_ripples": (I, [P, F, I]),
            "datum_host_query_ocean_ripples": (I, [P, P, ctypes.c_size_t, P]),
            "datum_host_step_ocean_bodies_coupled": (I, [P, P, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, I, P, I]),
            "datum_host_step_ocean_bodies_contact": (I, [P, P, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, I, P, P, I]),
            "datum_host_cast_ocean_rays": (I, [P, P, P, ctypes.c_size_t, P, I, I, I]),
            "datum_host_query_ocean_surface_rippled": (I, [P, P, P, ctypes.c_size_t, P, I]),
            "datum_host_cast_ocean_rays_rippled": (I, [P, P, P, ctypes.c_size_t, P, I, I, I]),
            "datum_host_gen_ocean_surface_rippled": (I, [P, P, ctypes.POINTER(CameraDesc), P]),
            "datum_host_reduce_ocean_bounds": (I, [P]),
            "datum_host_ocean_surface_slab": (I, [P, P, P]),
            "datum_host_reduce_ocean_ripple_bounds": (I, [P, P, P]),
            "datum_host_ocean_surface_slab_rippled": (I, [P, P, P]),
            "datum_host_cast_ocean_rays_bounded": (I, [P, P, P, ctypes.c_size_t, P, I, I, I]),
            "datum_host_cast_ocean_rays_rippled_bounded": (I, [P, P, P, ctypes.c_size_t, P, I, I, I]),
            "datum_host_set_ocean_ripple_foam": (I, [P, I]),
            "datum_host_step_ocean_ripple_foam": (I, [P, F]),
            "datum_host_query_ocean_ripple_foam": (I, [P, P, ctypes.c_size_t, P]),
            "datum_host_read_ocean_ripple_foam": (I, [P, P]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class OceanParams:
    """OceanParams of datum_amd/host/ocean.h (src/renderer/ocean.h:48-73)."""

    def __init__(self, resolution=64, **tunables):
        self.lib = load()
        self.N = resolution
        self.p = self.lib.datum_host_params_create(resolution)
        if tunables:
            self.set(**tunables)

    def __del__(self):
        if getattr(self, "p", None):
            self.lib.datum_host_params_destroy(self.p)
            self.p = None

    def copy(self):
        """A C++ copy of the OceanParams (the reference's is a POD that game code copies freely)."""
        c = OceanParams.__new__(OceanParams)
        c.lib, c.N = self.lib, self.N
        c.p = self.lib.datum_host_params_clone(self.p)
        return c

    def to_pod(self):
        """The reference's OceanParams byte for byte (OceanParamsPod, 82000 bytes), or None while recorded steps are missing from the host phase."""
        buf = ctypes.create_string_buffer(self.lib.datum_host_pod_bytes())
        rc = self.lib.datum_host_params_to_pod(self.p, buf)
        if rc < 0:
            raise HostError(self.lib.datum_host_last_error().decode())
        return bytes(buf) if rc == 0 else None

    @classmethod
    def from_pod(cls, pod):
        lib = load()
        assert len(pod) == lib.datum_host_pod_bytes()
        c = cls.__new__(cls)
        c.lib, c.N = lib, 64
        c.p = lib.datum_host_params_from_pod(ctypes.create_string_buffer(pod, len(pod)))
        return c

    def scalars(self):
        s = Scalars()
        self.lib.datum_host_params_get(self.p, ctypes.byref(s))
        return s

    def set(self, **kw):
        s = self.scalars()
        for k, v in kw.items():
            cur = getattr(s, k)
            if hasattr(cur, "__len__"):
                cur[:] = v
            else:
                setattr(s, k, v)
        self.lib.datum_host_params_set(self.p, ctypes.byref(s))

    def _arr(self, fn, shape):
        ptr = fn(self.p)
        return np.ctypeslib.as_array(ptr, shape=shape)

    @property
    def seed(self):
        return self._arr(self.lib.datum_host_params_seed, (self.N, self.N, 2))

    @property
    def height(self):
        return self._arr(self.lib.datum_host_params_height, (self.N, self.N, 2))

    @property
    def phase(self):
        return self._arr(self.lib.datum_host_params_phase, (self.N, self.N))

    def set_deviceheight(self, on=True):
        """Extension: lerp_ocean_waves leaves the h0 rebuild to the device (datum_ocean_rebuild_height)."""
        self.lib.datum_host_params_set_deviceheight(self.p, 1 if on else 0)

    def set_hostphase(self, on=True):
        """Extension: update_ocean also advances the host copy of the phase, as the reference does (ocean.cpp:223-233)."""
        if self.lib.datum_host_params_set_hostphase(self.p, 1 if on else 0) != 0:
            raise HostError(self.lib.datum_host_last_error().decode())

    def poke_hostphase(self, on=True):
        """OceanParams::hostphase = on, as C++ code sets the public field (no validation; tests)."""
        self.lib.datum_host_params_poke_hostphase(self.p, 1 if on else 0)

    def seed_ocean(self, rngseed=None):
        self.lib.datum_host_seed_ocean(self.p, 0 if rngseed is None else rngseed, 1 if rngseed is None else 0)

    def lerp_ocean_swell(self, swelllength, swellamplitude, swellspeed, swelldirection, t):
        self.lib.datum_host_lerp_ocean_swell(self.p, swelllength, swellamplitude, swellspeed, swelldirection[0], swelldirection[1], t)

    def lerp_ocean_waves(self, wavescale, waveamplitude, windspeed, winddirection, t):
        self.lib.datum_host_lerp_ocean_waves(self.p, wavescale, waveamplitude, windspeed, winddirection[0], winddirection[1], t)

    def update_ocean(self, dt):
        if self.lib.datum_host_update_ocean(self.p, dt) != 0:
            raise HostError(self.lib.datum_host_last_error().decode())

    def oceanset(self, camera=None):
        out = capi.OceanSet()
        cam = camera or example_camera()
        self.lib.datum_host_make_oceanset(ctypes.byref(cam), self.p, ctypes.byref(out))
        return out


# example-ocean tunables (examples/ocean/ocean.cpp:46-50)
EXAMPLE_TUNABLES = dict(wavescale=22.0, waveamplitude=0.0025, swellamplitude=0.8, windspeed=7.9, smoothing=320.0)


def twiddle_table(N):
    stages = int(np.log2(N))
    w = np.empty((N, 2 * stages), np.float32)
    if load().datum_host_twiddle_table(N, w.ctypes.data_as(P)) != 0:
        raise RuntimeError(load().datum_host_last_error().decode())
    return w


class HostError(RuntimeError):
    pass


class OceanContext:
    """OceanContext after initialise_ocean_context + prepare_ocean_context, with a ResourceManager for Ocean meshes."""

    def __init__(self, resolution=64, device=0, spectrumfp16=False, literaltransform=False, heightfp16=False):
        """spectrumfp16 / literaltransform / heightfp16: the extension flags of the C++ OceanContext (datum_amd/host/ocean.h), set before prepare_ocean_context"""
        self.lib = load()
        self.N = resolution
        self.c = self.lib.datum_host_context_create_ex(device, resolution, (1 if spectrumfp16 else 0) | (2 if literaltransform else 0) | (4 if heightfp16 else 0))
        if not self.c:
            raise HostError(self.lib.datum_host_last_error().decode())
        self.meshes = []

    def close(self):
        if getattr(self, "c", None):
            for m in self.meshes:
                self.lib.datum_host_ocean_release(self.c, m)
            self.meshes = []
            self.lib.datum_host_context_destroy(self.c)
            self.c = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise HostError(self.lib.datum_host_last_error().decode())

    def create_ocean(self, sizex, sizey):
        m = self.lib.datum_host_ocean_create(self.c, sizex, sizey)
        if not m:
            raise HostError(self.lib.datum_host_last_error().decode())
        self.meshes.append(m)
        return (m, sizex, sizey)

    def render_ocean_surface(self, mesh, params, camera=None):
        cam = camera or example_camera()
        self._check(self.lib.datum_host_render_ocean_surface(self.c, mesh[0], ctypes.byref(cam), params.p))

    def displace_ocean_surface(self, params):
        self._check(self.lib.datum_host_displace_ocean_surface(self.c, params.p))

    def release_parked_states(self, keep=None):
        """Free the context's parked device copies (all but `keep`'s); returns the bytes given back."""
        return self.lib.datum_host_release_parked_states(self.c, keep.p if keep is not None else None)

    def parked_states(self):
        return self.lib.datum_host_parked_states(self.c)

    def fetch_ocean_state(self, params):
        self._check(self.lib.datum_host_fetch_ocean_state(self.c, params.p))

    def read_displacement(self):
        out = np.empty((2, self.N, self.N, 4), np.float32)
        self._check(self.lib.datum_host_read_ocean_displacement(self.c, out.ctypes.data_as(P)))
        return out

    def set_foam(self, mode):
        """set_ocean_foam: "off", "jacobian", "accumulate" or a capi.FOAM_* value"""
        self._check(self.lib.datum_host_set_ocean_foam(self.c, capi.FOAM_MODES[mode] if isinstance(mode, str) else int(mode)))

    def set_foam_params(self, threshold=0.5, gain=2.0, decay=1.0):
        self._check(self.lib.datum_host_set_ocean_foam_params(self.c, threshold, gain, decay))

    def read_foam(self):
        out = np.empty((self.N, self.N), np.float32)
        self._check(self.lib.datum_host_read_ocean_foam(self.c, out.ctypes.data_as(P)))
        return out

    def _query(self, fn, params, xy, iterations, floats):
        """a point query through the C function `fn`: `xy` as (M, 2) float32, (M, floats) float32 back"""
        pts = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.empty((pts.shape[0], floats), np.float32)
        self._check(fn(self.c, params.p, pts.ctypes.data_as(P), pts.shape[0], out.ctypes.data_as(P), iterations))
        return out

    def _cast(self, fn, params, rays, iterations, steps, refine):
        """a ray cast through the C function `fn`: `rays` as (n, RAY_FLOATS) float32, (n, RAY_RECORD_FLOATS) float32 back"""
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, capi.RAY_FLOATS)
        out = np.empty((r.shape[0], capi.RAY_RECORD_FLOATS), np.float32)
        self._check(fn(self.c, params.p, r.ctypes.data_as(P), r.shape[0], out.ctypes.data_as(P), iterations, steps, refine))
        return out

    def query_ocean_surface(self, params, xy, iterations=4):
        """query_ocean_surface: the surface above the (M, 2) world points on the maps the context last displaced, swell, plane and scale from
        `params`; returns (M, 8) float32 records (OceanSurfaceSample: position, residual, normal, foam)"""
        return self._query(self.lib.datum_host_query_ocean_surface, params, xy, iterations, capi.SURFACE_SAMPLE_FLOATS)

    def set_velocity(self, mode):
        """set_ocean_velocity: "off", "on" or a capi.VELOCITY_MODES value"""
        self._check(self.lib.datum_host_set_ocean_velocity(self.c, capi.VELOCITY_MODES[mode] if isinstance(mode, str) else int(mode)))

    def read_velocity(self):
        """read_ocean_velocity: [N][N][4] float32 (vx, vy, vz, 0)"""
        out = np.empty((self.N, self.N, 4), np.float32)
        self._check(self.lib.datum_host_read_ocean_velocity(self.c, out.ctypes.data_as(P)))
        return out

    def query_ocean_velocity(self, params, xy, iterations=4):
        """query_ocean_velocity: (M, 8) float32 records (OceanVelocitySample: position, residual, velocity, 0)"""
        return self._query(self.lib.datum_host_query_ocean_velocity, params, xy, iterations, capi.VELOCITY_SAMPLE_FLOATS)

    def reduce_ocean_bodies(self, params, bodies, probes, iterations=4):
        """reduce_ocean_bodies: `bodies` an array of capi.BODY_DTYPE, `probes` (n, 4) float32 (x, y, z, weight); returns (nbodies, 8) float32
        records (OceanBodyRecord: force, torque x, torque y, wet, weighted normal, largest residual)"""
        b = np.ascontiguousarray(bodies)
        assert b.dtype.itemsize == ctypes.sizeof(capi.Body)
        pr = np.ascontiguousarray(probes, np.float32).reshape(-1, capi.BODY_PROBE_FLOATS)
        out = np.empty((b.shape[0], capi.BODY_RECORD_FLOATS), np.float32)
        self._check(self.lib.datum_host_reduce_ocean_bodies(self.c, params.p, b.ctypes.data_as(P), b.shape[0], pr.ctypes.data_as(P), pr.shape[0], out.ctypes.data_as(P), iterations))
        return out

    def reduce_ocean_body_drag(self, params, bodies, motions, probes, iterations=4):
        """reduce_ocean_body_drag: `bodies` an array of capi.BODY_DTYPE, `motions` one of capi.BODY_MOTION_DTYPE of the same length, `probes`
        (n, 4) float32; returns (nbodies, 8) float32 records (OceanDragRecord: force, torque, submerged, largest residual)"""
        b = np.ascontiguousarray(bodies)
        mo = np.ascontiguousarray(motions)
        assert b.dtype.itemsize == ctypes.sizeof(capi.Body) and mo.dtype.itemsize == ctypes.sizeof(capi.BodyMotion) and mo.shape[0] == b.shape[0]
        pr = np.ascontiguousarray(probes, np.float32).reshape(-1, capi.BODY_PROBE_FLOATS)
        out = np.empty((b.shape[0], capi.DRAG_RECORD_FLOATS), np.float32)
        self._check(self.lib.datum_host_reduce_ocean_body_drag(self.c, params.p, b.ctypes.data_as(P), mo.ctypes.data_as(P), b.shape[0], pr.ctypes.data_as(P), pr.shape[0],
                                                               out.ctypes.data_as(P), iterations))
        return out

    def step_ocean_bodies(self, params, bodies, motions, props, probes, dt, substeps=1, iterations=4):
        """step_ocean_bodies: `bodies` (capi.BODY_DTYPE) and `motions` (capi.BODY_MOTION_DTYPE), contiguous, are advanced IN PLACE by dt in
        `substeps` sub-steps; `props` an array of capi.BODY_PROPS_DTYPE of the same length, `probes` (n, 4) float32; returns (nbodies, 8)
        float32 records (OceanStepRecord: force, torque, submerged of the last sub-step, largest residual)"""
        assert isinstance(bodies, np.ndarray) and isinstance(motions, np.ndarray) and bodies.flags.c_contiguous and motions.flags.c_contiguous
        assert bodies.flags.writeable and motions.flags.writeable
        pp = np.ascontiguousarray(props)
        assert bodies.dtype.itemsize == ctypes.sizeof(capi.Body) and motions.dtype.itemsize == ctypes.sizeof(capi.BodyMotion) and pp.dtype.itemsize == ctypes.sizeof(capi.BodyProps)
        assert motions.shape[0] == bodies.shape[0] == pp.shape[0]
        pr = np.ascontiguousarray(probes, np.float32).reshape(-1, capi.BODY_PROBE_FLOATS)
        out = np.empty((bodies.shape[0], capi.STEP_RECORD_FLOATS), np.float32)
        self._check(self.lib.datum_host_step_ocean_bodies(self.c, params.p, bodies.ctypes.data_as(P), motions.ctypes.data_as(P), pp.ctypes.data_as(P), bodies.shape[0],
                                                          pr.ctypes.data_as(P), pr.shape[0], dt, substeps, out.ctypes.data_as(P), iterations))
        return out

    def set_ocean_ripples(self, R, cellsize=1.0):
        """set_ocean_ripples: the ripple layer with R x R cells of `cellsize` metres (R one of capi.RIPPLE_SIZES), at rest; R = 0 frees it"""
        self._check(self.lib.datum_host_set_ocean_ripples(self.c, R, cellsize))

    def set_ocean_ripple_dispersion(self, mode, g=9.81):
        """set_ocean_ripple_dispersion: the ripple step's mode, 0 the wave equation (the default) or 1 deep water with gravity g"""
        self._check(self.lib.datum_host_set_ocean_ripple_dispersion(self.c, int(mode), g))

    def set_ocean_ripple_walls(self, walls=None):
        """set_ocean_ripple_walls: `walls` an array of capi.RIPPLE_WALL records (OceanRippleWall); None or empty turns walls off"""
        w = np.ascontiguousarray(walls if walls is not None else [], capi.RIPPLE_WALL).reshape(-1)
        self._check(self.lib.datum_host_set_ocean_ripple_walls(self.c, w.ctypes.data_as(P) if len(w) else None, len(w)))

    def read_ocean_ripple_walls(self, R):
        """read_ocean_ripple_walls: the (R, R) uint8 wall plane in window order"""
        out = np.empty((R, R), np.uint8)
        self._check(self.lib.datum_host_read_ocean_ripple_walls(self.c, out.ctypes.data_as(P)))
        return out

    def set_ocean_ripple_bed(self, bed=None, depths=None):
        """set_ocean_ripple_bed: `bed` a capi.RIPPLE_BED record (OceanRippleBed), `depths` its (height, width) float32 map; None turns the bed off"""
        if bed is None:
            self._check(self.lib.datum_host_set_ocean_ripple_bed(self.c, None, None))
            return
        b = np.array([bed], capi.RIPPLE_BED).reshape(-1)[:1]
        d = np.ascontiguousarray(depths, np.float32)
        if d.size != int(b["width"][0]) * int(b["height"][0]):
            raise ValueError("set_ocean_ripple_bed: depths must hold width * height values")
        self._check(self.lib.datum_host_set_ocean_ripple_bed(self.c, b.ctypes.data_as(P), d.ctypes.data_as(P)))

    def read_ocean_ripple_bed(self, R):
        """read_ocean_ripple_bed: the (R, R) float32 depth plane and the (R, R) uint8 surf plane in window order"""
        depth, surf = np.empty((R, R), np.float32), np.empty((R, R), np.uint8)
        self._check(self.lib.datum_host_read_ocean_ripple_bed(self.c, depth.ctypes.data_as(P), surf.ctypes.data_as(P)))
        return depth, surf

    def set_ocean_ripple_swell(self, on=True):
        """set_ocean_ripple_swell: the FFT swell reflects off the walls and the beach; WAVE mode only"""
        self._check(self.lib.datum_host_set_ocean_ripple_swell(self.c, int(bool(on))))

    def refresh_ocean_ripple_swell(self, params, iterations=4):
        """refresh_ocean_ripple_swell: the forcing plane from cascade 0's surface, the solid cells and the origin; marks it current"""
        self._check(self.lib.datum_host_refresh_ocean_ripple_swell(self.c, params.p, iterations))

    def read_ocean_ripple_swell(self, R):
        """read_ocean_ripple_swell: the (R, R) float32 forcing plane in MEMORY order"""
        out = np.empty((R, R), np.float32)
        self._check(self.lib.datum_host_read_ocean_ripple_swell(self.c, out.ctypes.data_as(P)))
        return out

    def center_ocean_ripples(self, x, y):
        """center_ocean_ripples: the window's middle becomes the cell of (x, y); entered cells are zeroed"""
        self._check(self.lib.datum_host_center_ocean_ripples(self.c, x, y))

    def deposit_ocean_ripples(self, impulses):
        """deposit_ocean_ripples: `impulses` (n, 4) float32 (OceanRippleImpulse: x, y, volume in m^3, 0)"""
        imp = np.ascontiguousarray(impulses, np.float32).reshape(-1, 4)
        self._check(self.lib.datum_host_deposit_ocean_ripples(self.c, imp.ctypes.data_as(P), imp.shape[0]))

    def deposit_ocean_body_ripples(self, params, bodies, motions, probes, dt, iterations=4):
        """deposit_ocean_body_ripples: the wake of the bodies over dt, reduce_ocean_body_drag's arrays; returns (nbodies, 8) float32 records
        (OceanWakeRecord: heave, surge x, surge y, dropped quanta, 0, 0, submerged, largest residual)"""
        b = np.ascontiguousarray(bodies)
        mo = np.ascontiguousarray(motions)
        assert b.dtype.itemsize == ctypes.sizeof(capi.Body) and mo.dtype.itemsize == ctypes.sizeof(capi.BodyMotion) and mo.shape[0] == b.shape[0]
        pr = np.ascontiguousarray(probes, np.float32).reshape(-1, capi.BODY_PROBE_FLOATS)
        out = np.empty((b.shape[0], capi.RIPPLE_RECORD_FLOATS), np.float32)
        self._check(self.lib.datum_host_deposit_ocean_body_ripples(self.c, params.p, b.ctypes.data_as(P), mo.ctypes.data_as(P), b.shape[0], pr.ctypes.data_as(P), pr.shape[0],
                                                                   dt, out.ctypes.data_as(P), iterations))
        return out

    def step_ocean_ripples(self, dt, substeps=1):
        """step_ocean_ripples: `substeps` sub-steps of dt / substeps; the first takes the pending deposits in"""
        self._check(self.lib.datum_host_step_ocean_ripples(self.c, dt, substeps))

    def query_ocean_ripples(self, xy):
        """query_ocean_ripples: (M, 4) float32 samples (OceanRippleSample: height, d/dx, d/dy, rate)"""
        pts = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.empty((pts.shape[0], 4), np.float32)
        self._check(self.lib.datum_host_query_ocean_ripples(self.c, pts.ctypes.data_as(P), pts.shape[0], out.ctypes.data_as(P)))
        return out

    def step_ocean_bodies_coupled(self, params, bodies, motions, props, probes, dt, substeps=1, iterations=4):
        """step_ocean_bodies_coupled: step_ocean_bodies' arguments; bodies and the ripple layer advance together, the bodies feeling the
        layer; returns (nbodies, 12) float32 records (OceanCoupledRecord: force, torque, submerged, largest residual, the wake's heave,
        surge x, surge y of the last sub-step, dropped quanta)"""
        assert isinstance(bodies, np.ndarray) and isinstance(motions, np.ndarray) and bodies.flags.c_contiguous and motions.flags.c_contiguous
        assert bodies.flags.writeable and motions.flags.writeable
        pp = np.ascontiguousarray(props)
        assert bodies.dtype.itemsize == ctypes.sizeof(capi.Body) and motions.dtype.itemsize == ctypes.sizeof(capi.BodyMotion) and pp.dtype.itemsize == ctypes.sizeof(capi.BodyProps)
        assert motions.shape[0] == bodies.shape[0] == pp.shape[0]
        pr = np.ascontiguousarray(probes, np.float32).reshape(-1, capi.BODY_PROBE_FLOATS)
        out = np.empty((bodies.shape[0], capi.COUPLED_RECORD_FLOATS), np.float32)
        self._check(self.lib.datum_host_step_ocean_bodies_coupled(self.c, params.p, bodies.ctypes.data_as(P), motions.ctypes.data_as(P), pp.ctypes.data_as(P), bodies.shape[0],
                                                                  pr.ctypes.data_as(P), pr.shape[0], dt, substeps, out.ctypes.data_as(P), iterations))
        return out

    def step_ocean_bodies_contact(self, params, bodies, motions, props, probes, dt, contact, substeps=1, iterations=4):
        """step_ocean_bodies_contact: step_ocean_bodies_coupled's arguments and a capi.BodyContact; hulls stop at the ripple walls and
        ground on the ripple bed; returns (nbodies, 16) float32 records (OceanContactRecord: the coupled record, the contact force of the
        last sub-step, the deepest penetration)"""
        assert isinstance(bodies, np.ndarray) and isinstance(motions, np.ndarray) and bodies.flags.c_contiguous and motions.flags.c_contiguous
        assert bodies.flags.writeable and motions.flags.writeable
        pp = np.ascontiguousarray(props)
        assert bodies.dtype.itemsize == ctypes.sizeof(capi.Body) and motions.dtype.itemsize == ctypes.sizeof(capi.BodyMotion) and pp.dtype.itemsize == ctypes.sizeof(capi.BodyProps)
        assert motions.shape[0] == bodies.shape[0] == pp.shape[0]
        pr = np.ascontiguousarray(probes, np.float32).reshape(-1, capi.BODY_PROBE_FLOATS)
        out = np.empty((bodies.shape[0], capi.CONTACT_RECORD_FLOATS), np.float32)
        self._check(self.lib.datum_host_step_ocean_bodies_contact(self.c, params.p, bodies.ctypes.data_as(P), motions.ctypes.data_as(P), pp.ctypes.data_as(P), bodies.shape[0],
                                                                  pr.ctypes.data_as(P), pr.shape[0], dt, substeps, out.ctypes.data_as(P), ctypes.cast(ctypes.byref(contact), P),
                                                                  iterations))
        return out

    def cast_ocean_rays(self, params, rays, iterations=4, steps=32, refine=8):
        """cast_ocean_rays: `rays` (n, 8) float32 (origin, tmin, direction, tmax); returns (n, 12) float32 records (OceanRayRecord: hi, lo,
        g(hi), status, the surface sample at hi)"""
        return self._cast(self.lib.datum_host_cast_ocean_rays, params, rays, iterations, steps, refine)

    def query_ocean_surface_rippled(self, params, xy, iterations=4):
        """query_ocean_surface_rippled: query_ocean_surface with the ripple layer's height and slopes on top; (M, 8) float32"""
        return self._query(self.lib.datum_host_query_ocean_surface_rippled, params, xy, iterations, capi.SURFACE_SAMPLE_FLOATS)

    def cast_ocean_rays_rippled(self, params, rays, iterations=4, steps=32, refine=8):
        """cast_ocean_rays_rippled: cast_ocean_rays' arguments and records, on the water with the ripple layer on top"""
        return self._cast(self.lib.datum_host_cast_ocean_rays_rippled, params, rays, iterations, steps, refine)

    def gen_ocean_surface_rippled(self, mesh, params, camera=None):
        """gen_ocean_surface_rippled: the rippled mesh of cascade 0 into the mesh's vertex buffer, from the maps last displaced"""
        cam = camera or example_camera()
        self._check(self.lib.datum_host_gen_ocean_surface_rippled(self.c, mesh[0], ctypes.byref(cam), params.p))

    def reduce_ocean_bounds(self):
        """reduce_ocean_bounds: enqueue the reduction of the displacement last computed; current until the next render / displace"""
        self._check(self.lib.datum_host_reduce_ocean_bounds(self.c))

    def ocean_surface_slab(self, params):
        """ocean_surface_slab: (zlo, zhi, reach.x, reach.y) as float32, blocking"""
        out = np.zeros(4, np.float32)
        self._check(self.lib.datum_host_ocean_surface_slab(self.c, params.p, out.ctypes.data_as(P)))
        return out[0], out[1], out[2], out[3]

    def cast_ocean_rays_bounded(self, params, rays, iterations=4, steps=32, refine=8):
        """cast_ocean_rays_bounded: cast_ocean_rays' arguments and records; raises unless the bounds are current"""
        return self._cast(self.lib.datum_host_cast_ocean_rays_bounded, params, rays, iterations, steps, refine)

    def reduce_ocean_ripple_bounds(self):
        """reduce_ocean_ripple_bounds: the OceanRippleBounds of the layer's current state, blocking: etamin, etamax, ratemin, ratemax as
        float32, nonfinite and active as integers (active == 0: the layer is at rest)"""
        extrema, counts = np.zeros(4, np.float32), np.zeros(2, np.uint32)
        self._check(self.lib.datum_host_reduce_ocean_ripple_bounds(self.c, extrema.ctypes.data_as(P), counts.ctypes.data_as(P)))
        return OceanRippleBounds(*extrema, int(counts[0]), int(counts[1]))

    def ocean_surface_slab_rippled(self, params):
        """ocean_surface_slab_rippled: (zlo, zhi, reach.x, reach.y) of the water with the ripple layer on top, as float32, blocking"""
        out = np.zeros(4, np.float32)
        self._check(self.lib.datum_host_ocean_surface_slab_rippled(self.c, params.p, out.ctypes.data_as(P)))
        return out[0], out[1], out[2], out[3]

    def cast_ocean_rays_rippled_bounded(self, params, rays, iterations=4, steps=32, refine=8):
        """cast_ocean_rays_rippled_bounded: cast_ocean_rays_rippled's arguments and records; raises unless both bounds are current"""
        return self._cast(self.lib.datum_host_cast_ocean_rays_rippled_bounded, params, rays, iterations, steps, refine)

    def set_ocean_ripple_foam(self, on=True):
        """set_ocean_ripple_foam: the wake foam plane beside the ripple layer, zeroed; False frees it"""
        self._check(self.lib.datum_host_set_ocean_ripple_foam(self.c, 1 if on else 0))

    def step_ocean_ripple_foam(self, dt):
        """step_ocean_ripple_foam: one update of the plane from the layer's current state"""
        self._check(self.lib.datum_host_step_ocean_ripple_foam(self.c, dt))

    def query_ocean_ripple_foam(self, xy):
        """query_ocean_ripple_foam: (M,) float32, the bilinear coverage at the positions"""
        pts = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.empty(pts.shape[0], np.float32)
        self._check(self.lib.datum_host_query_ocean_ripple_foam(self.c, pts.ctypes.data_as(P), pts.shape[0], out.ctypes.data_as(P)))
        return out

    def read_ocean_ripple_foam(self, R):
        """read_ocean_ripple_foam: the plane in window order, (R, R) float32 for the R given to set_ocean_ripples"""
        out = np.empty((R, R), np.float32)
        self._check(self.lib.datum_host_read_ocean_ripple_foam(self.c, out.ctypes.data_as(P)))
        return out

    def read_vertices(self, mesh):
        out = np.empty((mesh[2], mesh[1], 12), np.float32)
        self._check(self.lib.datum_host_read_ocean_vertices(self.c, mesh[0], out.ctypes.data_as(P)))
        return out

    def read_indices(self, mesh):
        out = np.empty(6 * (mesh[1] - 1) * (mesh[2] - 1), np.uint32)
        rc = self.lib.datum_host_ocean_indices(self.c, mesh[0], out.ctypes.data_as(P))
        if rc != 0:
            raise HostError(f"datum_ocean_device_read failed: {rc}")
        return out
