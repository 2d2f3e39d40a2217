"""ctypes binding of include/datum_ocean_hip.h (libdatum_ocean_hip.so).

No compute happens here and there is no fallback: if the library is missing, import-time loading raises.
"""

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DATUM_OCEAN_HIP_LIB selects another build of the same module (tuning variants); never a different implementation
LIBPATH = os.environ.get("DATUM_OCEAN_HIP_LIB") or os.path.join(_HERE, "lib", "libdatum_ocean_hip.so")

F = ctypes.c_float
I = ctypes.c_int
P = ctypes.c_void_p
D = ctypes.c_double

SUPPORTED = (64, 128, 256, 512, 1024, 2048, 4096)
MAX_CASCADES = 16

OK, EINVAL, ESTATE, ENOMEM, EUNSUPPORTED, ENOTREADY, ECOMM = 0, -1, -2, -3, -4, -5, -6
FARM_ID_BYTES = 128
PAYLOAD_MAPS, PAYLOAD_XYZ32, PAYLOAD_XYZ16 = 0, 1, 2


class OceanSet(ctypes.Structure):
    """datum_ocean_set == head of the reference's OceanSet (src/renderer/ocean.cpp:33-50), 216 bytes."""

    _fields_ = [
        ("proj", F * 16),
        ("invproj", F * 16),
        ("camera_real", F * 4),
        ("camera_dual", F * 4),
        ("plane", F * 4),
        ("swelllength", F),
        ("swellamplitude", F),
        ("swellsteepness", F),
        ("swellphase", F),
        ("swelldirection", F * 2),
        ("scale", F),
        ("choppiness", F),
        ("smoothing", F),
        ("size", ctypes.c_uint32),
    ]


assert ctypes.sizeof(OceanSet) == 216

# every symbol include/datum_ocean_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "datum_ocean_create": (I, [ctypes.POINTER(P), I, I, I]),
    "datum_ocean_destroy": (I, [P]),
    "datum_ocean_set_stream": (I, [P, P, I]),
    "datum_ocean_bind_maps": (I, [P, P, ctypes.c_size_t]),
    "datum_ocean_maps_device": (I, [P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)]),
    "datum_ocean_map_layout": (I, [I, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(I)]),
    "datum_ocean_set_cascade": (I, [P, I, F, F]),
    "datum_ocean_set_spectrum_format": (I, [P, I]),
    "datum_ocean_set_map_store_policy": (I, [P, I]),
    "datum_ocean_map_store_policy": (I, [P, ctypes.POINTER(I), ctypes.POINTER(I)]),
    "datum_ocean_upload_state": (I, [P, I, P, P]),
    "datum_ocean_read_state": (I, [P, I, P]),
    "datum_ocean_state_bytes": (ctypes.c_size_t, [I]),
    "datum_ocean_park_state": (I, [P, I, P, ctypes.c_size_t, ctypes.POINTER(I)]),
    "datum_ocean_resume_state": (I, [P, I, P, ctypes.c_size_t, I]),
    "datum_ocean_upload_seed": (I, [P, I, P]),
    "datum_ocean_rebuild_height": (I, [P, I, F, F, F, F, F]),
    "datum_ocean_read_height": (I, [P, I, P]),
    "datum_ocean_update": (I, [P, F]),
    "datum_ocean_displace": (I, [P]),
    "datum_ocean_gen": (I, [P, I, ctypes.POINTER(OceanSet), I, I, P]),
    "datum_ocean_payload_bytes": (I, [P, I, ctypes.POINTER(ctypes.c_size_t)]),
    "datum_ocean_pack_displacement": (I, [P, I, P, ctypes.c_size_t]),
    "datum_ocean_farm_unique_id": (I, [P, ctypes.c_size_t]),
    "datum_ocean_farm_init": (I, [P, P, ctypes.c_size_t, I, I, I, I]),
    "datum_ocean_farm_shutdown": (I, [P]),
    "datum_ocean_farm_info": (I, [P, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(I), ctypes.POINTER(I)]),
    "datum_ocean_farm_gather": (I, [P, ctypes.POINTER(I)]),
    "datum_ocean_farm_result": (I, [P, I, P, I, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)]),
    "datum_ocean_farm_release": (I, [P, I, P, I]),
    "datum_ocean_farm_query": (I, [P, I]),
    "datum_ocean_farm_wait": (I, [P, I, ctypes.POINTER(F)]),
    "datum_ocean_farm_partition": (I, [P, I]),
    "datum_ocean_own_stream": (I, [P, ctypes.POINTER(P)]),
    "datum_ocean_read_maps": (I, [P, I, P]),
    "datum_ocean_sync": (I, [P]),
    "datum_ocean_wait_event": (I, [P, P]),
    "datum_ocean_signal": (I, [P, ctypes.POINTER(P)]),
    "datum_ocean_on_complete": (I, [P, ctypes.CFUNCTYPE(None, ctypes.c_void_p), P]),
    "datum_ocean_query": (I, [P]),
    "datum_ocean_import_memory_fd": (I, [P, I, ctypes.c_size_t, ctypes.POINTER(P)]),
    "datum_ocean_release_memory": (I, [P, P]),
    "datum_ocean_import_semaphore_fd": (I, [P, I, ctypes.POINTER(P)]),
    "datum_ocean_release_semaphore": (I, [P, P]),
    "datum_ocean_signal_external": (I, [P, P]),
    "datum_ocean_wait_external": (I, [P, P]),
    "datum_ocean_device_alloc": (I, [P, ctypes.c_size_t, ctypes.POINTER(P)]),
    "datum_ocean_device_free": (I, [P, P]),
    "datum_ocean_device_write": (I, [P, P, P, ctypes.c_size_t]),
    "datum_ocean_device_read": (I, [P, P, P, ctypes.c_size_t]),
    "datum_ocean_last_error": (ctypes.c_char_p, [P]),
    "datum_ocean_reference_weights": (I, [I, P]),
    "datum_ocean_debug_sim": (I, [P, I, P, P, P]),
    "datum_ocean_debug_rowpass": (I, [P, I, P, P]),
    "datum_ocean_profile_begin": (I, [P, I, I]),
    "datum_ocean_profile_end": (I, [P, ctypes.POINTER(D), ctypes.POINTER(D), ctypes.POINTER(I)]),
    "datum_ocean_algorithmic_bytes": (I, [P, ctypes.POINTER(D), ctypes.POINTER(D)]),
    "datum_ocean_abi_version": (I, []),
    "datum_ocean_set_literal_transform": (I, [P, I]),
    "datum_ocean_export_maps": (I, [P, I, P, ctypes.c_size_t]),
    "datum_ocean_farm_stream_flags": (I, [P, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)]),
    "datum_ocean_set_phase_writeback": (I, [P, I]),
    "datum_ocean_phase_writeback": (I, [P, ctypes.POINTER(I)]),
    "datum_ocean_set_phase_store": (I, [P, I]),
    "datum_ocean_phase_store": (I, [P, ctypes.POINTER(I), ctypes.POINTER(ctypes.c_uint)]),
    "datum_ocean_set_cascade_group": (I, [P, I]),
    "datum_ocean_cascade_group": (I, [P, ctypes.POINTER(I), ctypes.POINTER(I)]),
    "datum_ocean_set_foam": (I, [P, I]),
    "datum_ocean_set_foam_params": (I, [P, I, F, F, F]),
    "datum_ocean_reset_foam": (I, [P, I]),
    "datum_ocean_bind_foam": (I, [P, P, ctypes.c_size_t]),
    "datum_ocean_foam_device": (I, [P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)]),
    "datum_ocean_read_foam": (I, [P, I, P]),
    "datum_ocean_upload_height": (I, [P, I, P]),
    "datum_ocean_sample_surface": (I, [P, I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P]),
    "datum_ocean_read_surface": (I, [P, I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P]),
    "datum_ocean_gen_blend": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, P]),
    "datum_ocean_sample_surface_blend": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P]),
    "datum_ocean_read_surface_blend": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P]),
    "datum_ocean_reduce_bodies": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P, ctypes.c_size_t, P]),
    "datum_ocean_read_bodies": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P, ctypes.c_size_t, P]),
    "datum_ocean_cast_rays": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, I, P, ctypes.c_size_t, P]),
    "datum_ocean_read_rays": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, I, P, ctypes.c_size_t, P]),
    "datum_ocean_reduce_bounds": (I, [P]),
    "datum_ocean_bounds_device": (I, [P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)]),
    "datum_ocean_read_bounds": (I, [P, P]),
    "datum_ocean_surface_slab": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), P, P, P, P]),
    "datum_ocean_cast_rays_bounded": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, I, P, ctypes.c_size_t, P]),
    "datum_ocean_read_rays_bounded": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, I, P, ctypes.c_size_t, P]),
    "datum_ocean_set_velocity": (I, [P, I]),
    "datum_ocean_bind_velocity": (I, [P, P, ctypes.c_size_t]),
    "datum_ocean_velocity_device": (I, [P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)]),
    "datum_ocean_read_velocity": (I, [P, I, P]),
    "datum_ocean_sample_velocity_blend": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P]),
    "datum_ocean_read_velocity_blend": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P]),
    "datum_ocean_reduce_body_drag": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, ctypes.c_size_t, P, ctypes.c_size_t, P]),
    "datum_ocean_read_body_drag": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, ctypes.c_size_t, P, ctypes.c_size_t, P]),
    "datum_ocean_step_bodies": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, I, P]),
    "datum_ocean_step_bodies_host": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, I, P]),
    "datum_ocean_set_ripples": (I, [P, I, F]),
    "datum_ocean_set_ripple_params": (I, [P, F, F, I, F]),
    "datum_ocean_set_ripple_dispersion": (I, [P, I, F]),
    "datum_ocean_ripple_deep_weights": (I, [P]),
    "datum_ocean_center_ripples": (I, [P, F, F]),
    "datum_ocean_reset_ripples": (I, [P]),
    "datum_ocean_ripples_device": (I, [P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(I), ctypes.POINTER(I)]),
    "datum_ocean_read_ripples": (I, [P, P]),
    "datum_ocean_step_ripples": (I, [P, F, I]),
    "datum_ocean_deposit_ripples": (I, [P, P, ctypes.c_size_t]),
    "datum_ocean_deposit_body_ripples": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, P]),
    "datum_ocean_deposit_ripples_host": (I, [P, P, ctypes.c_size_t]),
    "datum_ocean_deposit_body_ripples_host": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, P]),
    "datum_ocean_sample_ripples": (I, [P, P, ctypes.c_size_t, P]),
    "datum_ocean_query_ripples": (I, [P, P, ctypes.c_size_t, P]),
    "datum_ocean_step_bodies_coupled": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, I, P]),
    "datum_ocean_step_bodies_coupled_host": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, I, P]),
    "datum_ocean_step_bodies_contact": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, I, P, P]),
    "datum_ocean_step_bodies_contact_host": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, F, I, P, P]),
    "datum_ocean_gen_blend_rippled": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, P]),
    "datum_ocean_sample_surface_blend_rippled": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P]),
    "datum_ocean_read_surface_blend_rippled": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, P, ctypes.c_size_t, P]),
    "datum_ocean_cast_rays_rippled": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, I, P, ctypes.c_size_t, P]),
    "datum_ocean_read_rays_rippled": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, I, P, ctypes.c_size_t, P]),
    "datum_ocean_reduce_ripple_bounds": (I, [P]),
    "datum_ocean_ripple_bounds_device": (I, [P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)]),
    "datum_ocean_read_ripple_bounds": (I, [P, P]),
    "datum_ocean_surface_slab_rippled": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), P, P, P, P]),
    "datum_ocean_cast_rays_rippled_bounded": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, I, P, ctypes.c_size_t, P]),
    "datum_ocean_read_rays_rippled_bounded": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I, I, I, P, ctypes.c_size_t, P]),
    # wake foam (added at ABI 9): a coverage plane beside the ripple layer
    "datum_ocean_set_ripple_foam": (I, [P, I]),
    "datum_ocean_set_ripple_foam_params": (I, [P, F, F, F, F, F]),
    "datum_ocean_step_ripple_foam": (I, [P, F]),
    "datum_ocean_reset_ripple_foam": (I, [P]),
    "datum_ocean_ripple_foam_device": (I, [P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(I), ctypes.POINTER(I)]),
    "datum_ocean_read_ripple_foam": (I, [P, P]),
    "datum_ocean_sample_ripple_foam": (I, [P, P, ctypes.c_size_t, P]),
    "datum_ocean_query_ripple_foam": (I, [P, P, ctypes.c_size_t, P]),
    # ripple walls (added at ABI 9): a byte plane beside the ripple layer
    "datum_ocean_set_ripple_walls": (I, [P, P, I]),
    "datum_ocean_ripple_walls_device": (I, [P, ctypes.POINTER(P)]),
    "datum_ocean_read_ripple_walls": (I, [P, P]),
    # the ripple bed (added at ABI 9): a depth plane and a surf plane beside the ripple layer
    "datum_ocean_set_ripple_bed": (I, [P, P, P]),
    "datum_ocean_ripple_bed_device": (I, [P, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)]),
    "datum_ocean_read_ripple_bed": (I, [P, P, P]),
    # ripple swell: the FFT swell reflects off ripple walls and the beach
    "datum_ocean_set_ripple_swell": (I, [P, I]),
    "datum_ocean_refresh_ripple_swell": (I, [P, ctypes.POINTER(I), I, ctypes.POINTER(OceanSet), I]),
    "datum_ocean_ripple_swell_device": (I, [P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(I)]),
    "datum_ocean_read_ripple_swell": (I, [P, P]),
}


# DATUM_OCEAN_ABI_VERSION of include/datum_ocean_hip.h as SYMBOLS above was written against it.  A constant, not a read of the header: an
# installed or copied package has no include/ beside it (tests/test_golden_and_abi.py asserts that the two agree in the source tree).
ABI_VERSION = 9

# datum_ocean_set_spectrum_format's values (include/datum_ocean_hip.h)
SPECTRUM_FORMATS = {"fp32": 0, "fp16": 1, "fp16h0": 2}

# datum_ocean_set_map_store_policy's values
MAP_STORE_POLICIES = {"auto": 0, "written through": 1, "streamed": 2}
PHASE_STORES = {"auto": 0, "plane": 1}

# datum_ocean_set_velocity's modes, and the floats of a velocity query's record
VELOCITY_MODES = {"off": 0, "on": 1}
VELOCITY_SAMPLE_FLOATS = 8

# datum_ocean_set_foam's modes (ABI 9)
FOAM_OFF, FOAM_JACOBIAN, FOAM_ACCUMULATE = 0, 1, 2
FOAM_MODES = {"off": FOAM_OFF, "jacobian": FOAM_JACOBIAN, "accumulate": FOAM_ACCUMULATE}

# surface queries (datum_ocean_sample_surface, added at ABI 9): floats per record and the largest iteration count
SURFACE_SAMPLE_FLOATS = 8
SURFACE_MAX_ITERATIONS = 16

# the ripple layer (datum_ocean_set_ripples, added at ABI 9): the sizes a layer can have, floats per wake record, the limits of a step
RIPPLE_SIZES = (64, 128, 256, 512, 1024)
RIPPLE_WAVE, RIPPLE_DEEP = 0, 1          # DATUM_OCEAN_RIPPLE_WAVE, DATUM_OCEAN_RIPPLE_DEEP: datum_ocean_set_ripple_dispersion's modes
RIPPLE_RECORD_FLOATS = 8
# ripple walls (datum_ocean_set_ripple_walls): the kinds, the most records, and the 32-byte datum_ocean_ripple_wall
RIPPLE_WALL_BOX, RIPPLE_WALL_ELLIPSE = 0, 1
RIPPLE_MAX_WALLS = 256
RIPPLE_WALL = np.dtype([("center", np.float32, 2), ("axis", np.float32, 2), ("half", np.float32, 2), ("kind", np.int32), ("reserved", np.int32)])
# the ripple bed (datum_ocean_set_ripple_bed): the surf levels, the map's largest side, and the 40-byte datum_ocean_ripple_bed
RIPPLE_SURF_LEVELS = 16
RIPPLE_BED_MAX_SIDE = 4096
RIPPLE_BED = np.dtype([("width", np.int32), ("height", np.int32), ("origin", np.float32, 2), ("texel", np.float32), ("outside", np.float32),
                       ("max_depth", np.float32), ("dry_depth", np.float32), ("surf_depth", np.float32), ("surf_gamma", np.float32)])
RIPPLE_MAX_SUBSTEPS = 16
RIPPLE_MAX_SPONGE = 64

# coupled stepping (datum_ocean_step_bodies_coupled, added at ABI 9): floats per body record
COUPLED_RECORD_FLOATS = 12
# body contact (datum_ocean_step_bodies_contact, added at ABI 9): floats per body record, the flags, the 32-byte parameters
CONTACT_RECORD_FLOATS = 16
CONTACT_BED, CONTACT_WALLS = 1, 2


class BodyContact(ctypes.Structure):
    _fields_ = [("stiffness", F), ("damping", F), ("friction", F), ("flags", ctypes.c_uint), ("reserved", F * 4)]


assert ctypes.sizeof(BodyContact) == 32

# body buoyancy (datum_ocean_reduce_bodies, added at ABI 9): floats per body record and per probe
BODY_RECORD_FLOATS = 8
BODY_PROBE_FLOATS = 4


class Body(ctypes.Structure):
    """datum_ocean_body of include/datum_ocean_hip.h: 64 bytes"""

    _fields_ = [
        ("rotation", F * 9),
        ("position", F * 3),
        ("first", ctypes.c_int32),
        ("count", ctypes.c_int32),
        ("cap", F),
        ("pad", ctypes.c_int32),
    ]


# the same layout for numpy: an array of this dtype is an array of Body
BODY_DTYPE = np.dtype([("rotation", np.float32, 9), ("position", np.float32, 3), ("first", np.int32), ("count", np.int32), ("cap", np.float32), ("pad", np.int32)])

# body drag (datum_ocean_reduce_body_drag, added at ABI 9): floats per body record
DRAG_RECORD_FLOATS = 8


class BodyMotion(ctypes.Structure):
    """datum_ocean_body_motion of include/datum_ocean_hip.h: 32 bytes"""

    _fields_ = [
        ("linear", F * 3),
        ("angular", F * 3),
        ("cl", F),
        ("cq", F),
    ]


# the same layout for numpy: an array of this dtype is an array of BodyMotion
BODY_MOTION_DTYPE = np.dtype([("linear", np.float32, 3), ("angular", np.float32, 3), ("cl", np.float32), ("cq", np.float32)])

# body stepping (datum_ocean_step_bodies, added at ABI 9): floats per body record and the largest number of sub-steps of a call
STEP_RECORD_FLOATS = 8
STEP_MAX_SUBSTEPS = 16


class BodyProps(ctypes.Structure):
    """datum_ocean_body_props of include/datum_ocean_hip.h: 32 bytes"""

    _fields_ = [
        ("invmass", F),
        ("invinertia", F * 3),
        ("gravity", F),
        ("buoyancy", F),
        ("pad", F * 2),
    ]


# the same layout for numpy: an array of this dtype is an array of BodyProps
BODY_PROPS_DTYPE = np.dtype([("invmass", np.float32), ("invinertia", np.float32, 3), ("gravity", np.float32), ("buoyancy", np.float32), ("pad", np.float32, 2)])

# ray casts (datum_ocean_cast_rays, added at ABI 9): floats per ray (ox, oy, oz, tmin, dx, dy, dz, tmax) and per record (hi, lo, g(hi), status,
# the query's record at hi), the ranges of steps and refine, and the status values
RAY_FLOATS = 8
RAY_RECORD_FLOATS = 12
RAY_MAX_STEPS = 1024
RAY_MAX_REFINE = 24
RAY_MISS, RAY_ENTER, RAY_LEAVE = 0, 1, 2

# surface bounds (datum_ocean_reduce_bounds, added at ABI 9): floats per cascade record (zmin, zmax, xmin, xmax, ymin, ymax, nonfinite, 0)
BOUNDS_RECORD_FLOATS = 8
# ripple-layer bounds (datum_ocean_reduce_ripple_bounds, added at ABI 9): etamin, etamax, ratemin, ratemax, nonfinite, active, 0, 0
RIPPLE_BOUNDS_RECORD_FLOATS = 8


def header_abi_version():
    """DATUM_OCEAN_ABI_VERSION as include/datum_ocean_hip.h states it (source tree only: the tests compare it with ABI_VERSION)."""
    import re

    text = open(os.path.join(os.path.dirname(_HERE), "include", "datum_ocean_hip.h")).read()
    return int(re.search(r"#define\s+DATUM_OCEAN_ABI_VERSION\s+(\d+)", text).group(1))

_lib = None


def load():
    """Load the HIP module.  Raises OSError when it is not built (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBPATH):
            raise OSError(
                f"{LIBPATH} not found: build the HIP module first (`make` or __graft_entry__.build()); "
                "datum_amd has no CPU fallback"
            )
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 + libhsa-runtime64 and the
        # module links the same SONAME from /opt/rocm.  Whichever is mapped first serves both; torch cannot
        # initialise on top of the system pair, so when torch is importable it goes first (it is also what the
        # tests and bench.py use for device buffers and streams, which must come from the same runtime).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIBPATH)
        # no soname: a library built from another revision of the header (DATUM_OCEAN_HIP_LIB swaps builds freely) is refused
        # before any call goes through a signature it may not have
        try:
            lib.datum_ocean_abi_version.restype = I
            lib.datum_ocean_abi_version.argtypes = []
            have = lib.datum_ocean_abi_version()
        except AttributeError:
            have = None
        want = ABI_VERSION
        if have != want:
            raise OSError(f"{LIBPATH} reports ABI version {have}, this binding is written against version {want} of include/datum_ocean_hip.h: rebuild the HIP module (`make`)")
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                # entry points added within a version (include/datum_ocean_hip.h) are detected by symbol: a library without one is stale
                raise OSError(f"{LIBPATH} does not export {name}, which this binding of ABI version {want} declares: rebuild the HIP module (`make`)") from None
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class OceanError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"datum_ocean error {code}: {message}")
        self.code = code


def _ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(P)


def _dev(ptr):
    """an optional device pointer given as an integer: None and 0 are the C null"""
    return P(ptr) if ptr else None


def _body_batch(bodies, motions, props, probes, floats, in_place=False):
    """A body call's host arrays as its C arguments up to the records -- [bodies, (motions, (props,)) nbodies, probes, nprobes] -- and the
    records' (nbodies, floats) array to pass last.  `motions` and `props` are None where the call takes none; `in_place` (the step twins,
    which write bodies and motions back): both must be writable contiguous arrays already, and neither is copied."""
    if in_place:
        assert isinstance(bodies, np.ndarray) and isinstance(motions, np.ndarray) and bodies.flags.c_contiguous and motions.flags.c_contiguous
        assert bodies.flags.writeable and motions.flags.writeable
    arrays = [np.ascontiguousarray(np.frombuffer(bytes(bodies), BODY_DTYPE) if isinstance(bodies, ctypes.Array) else bodies)]
    arrays += [np.ascontiguousarray(a) for a in (motions, props) if a is not None]
    for a, struct in zip(arrays, (Body, BodyMotion, BodyProps)):
        assert a.dtype.itemsize == ctypes.sizeof(struct) and a.shape[0] == arrays[0].shape[0]
    pr = np.ascontiguousarray(probes, np.float32).reshape(-1, BODY_PROBE_FLOATS)
    out = np.empty((arrays[0].shape[0], floats), np.float32)
    return [_ptr(a) for a in arrays] + [arrays[0].shape[0], _ptr(pr), pr.shape[0]], out


class Ocean:
    """One handle of the C ABI (a device, a resolution, `cascades` independent grids)."""

    def __init__(self, resolution, cascades=1, device=0):
        self.lib = load()
        self.N = resolution
        self.cascades = cascades
        self.device = device
        h = P()
        rc = self.lib.datum_ocean_create(ctypes.byref(h), device, resolution, cascades)
        if rc != 0:
            raise OceanError(rc, self.lib.datum_ocean_last_error(None).decode())
        self.h = h

    def _check(self, rc):
        if rc != 0:
            raise OceanError(rc, self.lib.datum_ocean_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.datum_ocean_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, stream_ptr):
        """stream_ptr: a hipStream_t as an integer (0 = HIP's default stream); None = the handle's own stream."""
        if stream_ptr is None:
            self._check(self.lib.datum_ocean_set_stream(self.h, None, 1))
        else:
            self._check(self.lib.datum_ocean_set_stream(self.h, P(stream_ptr), 0))

    def bind_maps(self, device_ptr, nbytes):
        self._check(self.lib.datum_ocean_bind_maps(self.h, _dev(device_ptr), nbytes))

    def maps_device(self):
        p = P()
        n = ctypes.c_size_t()
        self._check(self.lib.datum_ocean_maps_device(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def set_cascade(self, cascade, wavescale, choppiness):
        self._check(self.lib.datum_ocean_set_cascade(self.h, cascade, wavescale, choppiness))

    def upload_state(self, cascade, h0, phase=None):
        h0 = np.ascontiguousarray(h0, np.float32)
        assert h0.size == 2 * self.N * self.N
        if phase is not None:
            phase = np.ascontiguousarray(phase, np.float32)
            assert phase.size == self.N * self.N
        self._check(self.lib.datum_ocean_upload_state(self.h, cascade, _ptr(h0), _ptr(phase) if phase is not None else None))

    def upload_height(self, cascade, h0):
        """replace the cascade's h0 and keep its phase and foam accumulator (datum_ocean_upload_height)"""
        h0 = np.ascontiguousarray(h0, np.float32)
        assert h0.size == 2 * self.N * self.N
        self._check(self.lib.datum_ocean_upload_height(self.h, cascade, _ptr(h0)))

    def upload_seed(self, cascade, seed):
        seed = np.ascontiguousarray(seed, np.float32)
        assert seed.size == 2 * self.N * self.N
        self._check(self.lib.datum_ocean_upload_seed(self.h, cascade, _ptr(seed)))

    def rebuild_height(self, cascade, wavescale, waveamplitude, windspeed, winddirection):
        self._check(self.lib.datum_ocean_rebuild_height(self.h, cascade, wavescale, waveamplitude, windspeed, winddirection[0], winddirection[1]))

    def read_height(self, cascade):
        out = np.empty((self.N, self.N, 2), np.float32)
        self._check(self.lib.datum_ocean_read_height(self.h, cascade, _ptr(out)))
        return out

    def read_state(self, cascade):
        out = np.empty((self.N, self.N), np.float32)
        self._check(self.lib.datum_ocean_read_state(self.h, cascade, _ptr(out)))
        return out

    def update(self, dt):
        self._check(self.lib.datum_ocean_update(self.h, dt))

    def displace(self):
        self._check(self.lib.datum_ocean_displace(self.h))

    def gen(self, cascade, oceanset, sizex, sizey, vertices_device_ptr):
        self._check(self.lib.datum_ocean_gen(self.h, cascade, ctypes.byref(oceanset), sizex, sizey, P(vertices_device_ptr)))

    def payload_bytes(self, fmt):
        n = ctypes.c_size_t()
        self._check(self.lib.datum_ocean_payload_bytes(self.h, fmt, ctypes.byref(n)))
        return n.value

    def pack_displacement(self, fmt, device_ptr, nbytes):
        """Enqueue the packing of every cascade's displacement into caller-owned device memory (all-gather payload)."""
        self._check(self.lib.datum_ocean_pack_displacement(self.h, fmt, P(device_ptr), nbytes))

    # -- the tile farm (include/datum_ocean_hip.h: datum_ocean_farm_*): the RCCL all-gather lives in the module --------

    def farm_init(self, unique_id, rank, world, fmt, slots=2):
        """Join the farm's communicator (collective over the ranks).  unique_id: the 128 bytes of farm_unique_id() on rank 0."""
        assert len(unique_id) == FARM_ID_BYTES
        buf = (ctypes.c_char * FARM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(self.lib.datum_ocean_farm_init(self.h, buf, FARM_ID_BYTES, rank, world, fmt, slots))

    def farm_shutdown(self):
        self._check(self.lib.datum_ocean_farm_shutdown(self.h))

    def farm_info(self):
        rank, world, fmt, slots, ver = I(), I(), I(), I(), I()
        nbytes = ctypes.c_size_t()
        self._check(self.lib.datum_ocean_farm_info(self.h, ctypes.byref(rank), ctypes.byref(world), ctypes.byref(fmt), ctypes.byref(nbytes), ctypes.byref(slots), ctypes.byref(ver)))
        return dict(rank=rank.value, world=world.value, format=fmt.value, payload_bytes=nbytes.value, slots=slots.value, rccl_version=ver.value)

    def farm_gather(self):
        """Enqueue pack + all-gather of the displacement field as of the last displace; returns the slot.  Does not block."""
        slot = I()
        self._check(self.lib.datum_ocean_farm_gather(self.h, ctypes.byref(slot)))
        return slot.value

    def farm_result(self, slot, stream_ptr=None):
        """(device pointer, bytes) of the slot's gathered block; `stream_ptr` (None: the handle's stream) waits for the collective."""
        p, n = P(), ctypes.c_size_t()
        self._check(self.lib.datum_ocean_farm_result(self.h, slot, _dev(stream_ptr), 1 if stream_ptr is None else 0, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def farm_release(self, slot, stream_ptr=None):
        self._check(self.lib.datum_ocean_farm_release(self.h, slot, _dev(stream_ptr), 1 if stream_ptr is None else 0))

    def farm_query(self, slot):
        rc = self.lib.datum_ocean_farm_query(self.h, slot)
        if rc == ENOTREADY:
            return False
        self._check(rc)
        return True

    def farm_partition(self, comm_cus):
        """The communication stream on `comm_cus` compute units of its own (comm_cus / 8 per XCD), the handle's own stream on the others; 0 undoes it."""
        self._check(self.lib.datum_ocean_farm_partition(self.h, comm_cus))

    def own_stream(self):
        """The handle's own hipStream_t as an integer (torch.cuda.ExternalStream takes it)."""
        p = P()
        self._check(self.lib.datum_ocean_own_stream(self.h, ctypes.byref(p)))
        return p.value

    def farm_wait(self, slot):
        """Host wait for the slot's collective; returns its duration on the communication stream in ms."""
        ms = F()
        self._check(self.lib.datum_ocean_farm_wait(self.h, slot, ctypes.byref(ms)))
        return ms.value

    def import_memory_fd(self, fd, nbytes):
        """Device pointer over memory another API exported as a POSIX fd (Vulkan external memory, opaque fd)."""
        p = P()
        self._check(self.lib.datum_ocean_import_memory_fd(self.h, fd, nbytes, ctypes.byref(p)))
        return p.value

    def release_memory(self, device_ptr):
        self._check(self.lib.datum_ocean_release_memory(self.h, P(device_ptr)))

    def signal(self):
        """Record the handle's completion event behind everything enqueued so far; returns the hipEvent_t."""
        p = P()
        self._check(self.lib.datum_ocean_signal(self.h, ctypes.byref(p)))
        return p.value

    def wait_event(self, hip_event):
        self._check(self.lib.datum_ocean_wait_event(self.h, P(hip_event)))

    def query(self):
        """True once everything enqueued before the last signal() has finished; never blocks."""
        rc = self.lib.datum_ocean_query(self.h)
        if rc == ENOTREADY:
            return False
        self._check(rc)
        return True

    def on_complete(self, fn):
        """`fn()` on a runtime thread once everything enqueued so far has finished.  The ctypes trampoline is kept alive on the handle."""
        cb = ctypes.CFUNCTYPE(None, ctypes.c_void_p)(lambda _user: fn())
        self._callbacks = getattr(self, "_callbacks", []) + [cb]
        self._check(self.lib.datum_ocean_on_complete(self.h, cb, None))

    def import_semaphore_fd(self, fd):
        p = P()
        self._check(self.lib.datum_ocean_import_semaphore_fd(self.h, fd, ctypes.byref(p)))
        return p.value

    def state_bytes(self):
        return self.lib.datum_ocean_state_bytes(self.N)

    def park_state(self, cascade, device_ptr, nbytes):
        """h0 and the phase as advanced so far into caller-owned device memory (device to device); returns the flags to hand back."""
        flags = I()
        self._check(self.lib.datum_ocean_park_state(self.h, cascade, P(device_ptr), nbytes, ctypes.byref(flags)))
        return flags.value

    def resume_state(self, cascade, device_ptr, nbytes, flags):
        self._check(self.lib.datum_ocean_resume_state(self.h, cascade, P(device_ptr), nbytes, flags))

    def read_maps(self, cascade):
        out = np.empty((2, self.N, self.N, 4), np.float32)
        self._check(self.lib.datum_ocean_read_maps(self.h, cascade, _ptr(out)))
        return out

    def sync(self):
        self._check(self.lib.datum_ocean_sync(self.h))

    def debug_sim(self, cascade):
        h, hx, hy = (np.empty((self.N, self.N, 2), np.float32) for _ in range(3))
        self._check(self.lib.datum_ocean_debug_sim(self.h, cascade, _ptr(h), _ptr(hx), _ptr(hy)))
        return h, hx, hy

    def set_spectrum_format(self, fp16):
        """Work spectrum between the passes as IEEE halves (True / "fp16") or fp32 (False / "fp32", default); "fp16h0": the halves and h0
        read as halves too (DATUM_OCEAN_SPECTRUM_FP16_H0)."""
        code = SPECTRUM_FORMATS[fp16] if isinstance(fp16, str) else (1 if fp16 else 0)
        self._check(self.lib.datum_ocean_set_spectrum_format(self.h, code))

    def debug_rowpass(self, cascade):
        c, d = (np.empty((self.N, self.N, 2), np.float32) for _ in range(2))
        self._check(self.lib.datum_ocean_debug_rowpass(self.h, cascade, _ptr(c), _ptr(d)))
        return c, d

    def profile_begin(self, max_samples, stride=1):
        self._check(self.lib.datum_ocean_profile_begin(self.h, max_samples, stride))

    def profile_end(self):
        row, col, n = D(), D(), I()
        self._check(self.lib.datum_ocean_profile_end(self.h, ctypes.byref(row), ctypes.byref(col), ctypes.byref(n)))
        return row.value, col.value, n.value

    def set_literal_transform(self, on):
        """validation mode: displace through the reference's radix-2 transforms and literal twiddle table (datum_ocean_set_literal_transform)"""
        self._check(self.lib.datum_ocean_set_literal_transform(self.h, 1 if on else 0))

    def farm_stream_flags(self):
        """hipStreamGetFlags of (communication stream, own stream): 0 = hipStreamDefault (synchronises with the null stream), 1 = hipStreamNonBlocking"""
        a, b = ctypes.c_uint(), ctypes.c_uint()
        self._check(self.lib.datum_ocean_farm_stream_flags(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_cascade_group(self, cascades_per_launch):
        """cascades per launch of the two passes; 0 = sized to the Infinity Cache (datum_ocean_set_cascade_group)"""
        self._check(self.lib.datum_ocean_set_cascade_group(self.h, cascades_per_launch))

    def cascade_group(self):
        """(cascades per launch, launches per pass and displace call)"""
        g, n = I(), I()
        self._check(self.lib.datum_ocean_cascade_group(self.h, ctypes.byref(g), ctypes.byref(n)))
        return g.value, n.value

    def set_phase_writeback(self, every):
        """the row pass stores the phase once per `every` steps' worth of dt's: 1 = every row pass, 0 = the module's choice; results do not
        depend on it (datum_ocean_set_phase_writeback)"""
        self._check(self.lib.datum_ocean_set_phase_writeback(self.h, int(every)))

    def phase_writeback(self):
        """the write-back interval in use"""
        e = I(0)
        self._check(self.lib.datum_ocean_phase_writeback(self.h, ctypes.byref(e)))
        return e.value

    def set_phase_store(self, mode):
        """where the phase is kept: "auto" (default: a symmetric cascade's as a quadrant table) or "plane"; results do not depend on it
        (datum_ocean_set_phase_store)"""
        self._check(self.lib.datum_ocean_set_phase_store(self.h, PHASE_STORES[mode] if isinstance(mode, str) else int(mode)))

    def phase_store(self):
        """(the mode set, the cascades whose phase is a quadrant table at this moment, one bit each)"""
        m, q = I(), ctypes.c_uint()
        self._check(self.lib.datum_ocean_phase_store(self.h, ctypes.byref(m), ctypes.byref(q)))
        return {v: k for k, v in PHASE_STORES.items()}[m.value], q.value

    def set_map_store_policy(self, policy):
        """how the column pass stores the maps: "auto" (default), "written through", "streamed" (datum_ocean_set_map_store_policy)"""
        self._check(self.lib.datum_ocean_set_map_store_policy(self.h, MAP_STORE_POLICIES[policy] if isinstance(policy, str) else int(policy)))

    def map_store_policy(self):
        """(the policy set, whether the next displace streams the maps)"""
        p, s = I(), I()
        self._check(self.lib.datum_ocean_map_store_policy(self.h, ctypes.byref(p), ctypes.byref(s)))
        return {v: k for k, v in MAP_STORE_POLICIES.items()}[p.value], bool(s.value)

    def export_maps(self, cascade, device_ptr, nbytes):
        """the cascade's maps as the reference's [layer][y][x][4] RGBA32F image, into DEVICE memory (datum_ocean_export_maps)"""
        self._check(self.lib.datum_ocean_export_maps(self.h, cascade, ctypes.c_void_p(device_ptr), nbytes))

    # -- foam (datum_ocean_set_foam ...): the Jacobian of the horizontal displacement, one fp32 plane per cascade --------------

    def set_foam(self, mode):
        """"off" (default), "jacobian" (the plane holds J) or "accumulate" (persistent coverage in [0, 1]); or a FOAM_* value"""
        self._check(self.lib.datum_ocean_set_foam(self.h, FOAM_MODES[mode] if isinstance(mode, str) else int(mode)))

    def set_foam_params(self, cascade, threshold=0.5, gain=2.0, decay=1.0):
        """the accumulation's parameters of one cascade (defaults: the module's)"""
        self._check(self.lib.datum_ocean_set_foam_params(self.h, cascade, threshold, gain, decay))

    def reset_foam(self, cascade):
        self._check(self.lib.datum_ocean_reset_foam(self.h, cascade))

    def bind_foam(self, device_ptr, nbytes):
        """caller-owned device memory (cascades * N * N * 4 bytes) becomes the foam plane; None / 0 restores the handle's own"""
        self._check(self.lib.datum_ocean_bind_foam(self.h, _dev(device_ptr), nbytes))

    def foam_device(self):
        """(device pointer, bytes) of the foam plane in use"""
        p = P()
        n = ctypes.c_size_t()
        self._check(self.lib.datum_ocean_foam_device(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def read_foam(self, cascade):
        out = np.empty((self.N, self.N), np.float32)
        self._check(self.lib.datum_ocean_read_foam(self.h, cascade, _ptr(out)))
        return out

    # -- surface queries (datum_ocean_sample_surface): the water surface above world points ---------------------------------------

    def sample_surface(self, cascade, oceanset, points_ptr, count, samples_ptr, iterations=4):
        """Enqueue the query of `count` float2 world points (device pointer, 8-byte aligned) into `count` records of 8 floats (device
        pointer, 16-byte aligned): surface point (x, y, height), residual, unit normal, foam.  `oceanset` as for gen()."""
        self._check(self.lib.datum_ocean_sample_surface(self.h, cascade, ctypes.byref(oceanset), iterations, _dev(points_ptr), count, _dev(samples_ptr)))

    def read_surface(self, cascade, oceanset, points, iterations=4):
        """the same from a host (M, 2) float32 array, blocking; returns (M, 8) float32"""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        out = np.empty((pts.shape[0], SURFACE_SAMPLE_FLOATS), np.float32)
        self._check(self.lib.datum_ocean_read_surface(self.h, cascade, ctypes.byref(oceanset), iterations, _ptr(pts), pts.shape[0], _ptr(out)))
        return out

    # -- several cascades at once (datum_ocean_gen_blend): the summed surface's mesh and queries -------------------------------------

    @staticmethod
    def _list(cascades):
        c = [int(x) for x in cascades]
        return (I * len(c))(*c), len(c)

    def _sample_points(self, fn, cascades, oceanset, iterations, points_ptr, count, samples_ptr):
        """a point query on device arrays through the C function `fn`: the list, the pointers, the return code"""
        arr, n = self._list(cascades)
        self._check(fn(self.h, arr, n, ctypes.byref(oceanset), iterations, _dev(points_ptr), count, _dev(samples_ptr)))

    def _read_points(self, fn, cascades, oceanset, iterations, points, floats):
        """its host twin: `points` as (M, 2) float32, (M, floats) float32 back"""
        arr, n = self._list(cascades)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        out = np.empty((pts.shape[0], floats), np.float32)
        self._check(fn(self.h, arr, n, ctypes.byref(oceanset), iterations, _ptr(pts), pts.shape[0], _ptr(out)))
        return out

    def _cast(self, fn, cascades, oceanset, iterations, steps, refine, rays_ptr, n, records_ptr):
        """a ray cast on device arrays through the C function `fn`"""
        arr, c = self._list(cascades)
        self._check(fn(self.h, arr, c, ctypes.byref(oceanset), iterations, steps, refine, _dev(rays_ptr), n, _dev(records_ptr)))

    def _read_cast(self, fn, cascades, oceanset, iterations, steps, refine, rays):
        """its host twin: `rays` as (n, RAY_FLOATS) float32, (n, RAY_RECORD_FLOATS) float32 back"""
        arr, c = self._list(cascades)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, RAY_FLOATS)
        out = np.empty((r.shape[0], RAY_RECORD_FLOATS), np.float32)
        self._check(fn(self.h, arr, c, ctypes.byref(oceanset), iterations, steps, refine, _ptr(r), r.shape[0], _ptr(out)))
        return out

    def gen_blend(self, cascades, oceanset, sizex, sizey, vertices_device_ptr):
        """gen() of the sum of the listed cascades, each sampled with the handle's own 1 / wavescale (oceanset.scale is ignored)"""
        arr, n = self._list(cascades)
        self._check(self.lib.datum_ocean_gen_blend(self.h, arr, n, ctypes.byref(oceanset), sizex, sizey, P(vertices_device_ptr)))

    def sample_surface_blend(self, cascades, oceanset, points_ptr, count, samples_ptr, iterations=4):
        """sample_surface() of the sum of the listed cascades: device pointers, enqueued on the handle's stream"""
        self._sample_points(self.lib.datum_ocean_sample_surface_blend, cascades, oceanset, iterations, points_ptr, count, samples_ptr)

    def read_surface_blend(self, cascades, oceanset, points, iterations=4):
        """the same from a host (M, 2) float32 array, blocking; returns (M, 8) float32"""
        return self._read_points(self.lib.datum_ocean_read_surface_blend, cascades, oceanset, iterations, points, SURFACE_SAMPLE_FLOATS)

    # -- surface velocity (datum_ocean_set_velocity): d/dt of map layer 0, one float4 plane per cascade -----------------------------------

    def set_velocity(self, mode):
        """"off" (default) or "on": datum_ocean_displace then writes (vx, vy, vz, 0) per texel"""
        if isinstance(mode, bool):
            mode = int(mode)
        self._check(self.lib.datum_ocean_set_velocity(self.h, VELOCITY_MODES[mode] if isinstance(mode, str) else int(mode)))

    def bind_velocity(self, device_ptr, nbytes):
        """caller-owned device memory (cascades * N * N * 16 bytes) becomes the velocity plane; None / 0 restores the handle's own"""
        self._check(self.lib.datum_ocean_bind_velocity(self.h, _dev(device_ptr), nbytes))

    def velocity_device(self):
        """(device pointer, bytes) of the velocity plane in use"""
        p = P()
        n = ctypes.c_size_t()
        self._check(self.lib.datum_ocean_velocity_device(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def read_velocity(self, cascade):
        """the cascade's plane [N][N][4] float32: (vx, vy, vz, 0)"""
        out = np.empty((self.N, self.N, 4), np.float32)
        self._check(self.lib.datum_ocean_read_velocity(self.h, cascade, _ptr(out)))
        return out

    def sample_velocity_blend(self, cascades, oceanset, points_ptr, count, out_ptr, iterations=4):
        """sample_surface_blend()'s solve, then the listed cascades' velocity planes at the same texels: device pointers, enqueued"""
        self._sample_points(self.lib.datum_ocean_sample_velocity_blend, cascades, oceanset, iterations, points_ptr, count, out_ptr)

    def read_velocity_blend(self, cascades, oceanset, points, iterations=4):
        """the same from a host (M, 2) float32 array, blocking; returns (M, 8) float32: V(b), residual, velocity, 0"""
        return self._read_points(self.lib.datum_ocean_read_velocity_blend, cascades, oceanset, iterations, points, VELOCITY_SAMPLE_FLOATS)

    # -- body buoyancy (datum_ocean_reduce_bodies): per-body force and torque from hull probes -----------------------------------------

    def reduce_bodies(self, cascades, oceanset, bodies_ptr, nbodies, probes_ptr, nprobes, records_ptr, iterations=4):
        """Enqueue the reduction of `nbodies` bodies (device pointer, 64 bytes each) over `nprobes` probes (device pointer, 16 bytes each:
        x, y, z, weight) into `nbodies` records of 8 floats (device pointer): Fz, tau x, tau y, wet, sum m n, max residual."""
        arr, n = self._list(cascades)
        self._check(self.lib.datum_ocean_reduce_bodies(self.h, arr, n, ctypes.byref(oceanset), iterations, _dev(bodies_ptr), nbodies, _dev(probes_ptr), nprobes, _dev(records_ptr)))

    def read_bodies(self, cascades, oceanset, bodies, probes, iterations=4):
        """the same from host arrays, blocking: `bodies` an array of BODY_DTYPE (or of Body), `probes` (n, 4) float32; returns (nbodies, 8)"""
        arr, n = self._list(cascades)
        args, out = _body_batch(bodies, None, None, probes, BODY_RECORD_FLOATS)
        self._check(self.lib.datum_ocean_read_bodies(self.h, arr, n, ctypes.byref(oceanset), iterations, *args, _ptr(out)))
        return out

    # -- body drag (datum_ocean_reduce_body_drag): per-body force and torque from the water's velocity relative to the hull ----------------

    def reduce_body_drag(self, cascades, oceanset, bodies_ptr, motions_ptr, nbodies, probes_ptr, nprobes, records_ptr, iterations=4):
        """Enqueue the reduction of `nbodies` bodies (device pointer, 64 bytes each) with their motions (device pointer, 32 bytes each) over
        `nprobes` probes (device pointer, 16 bytes each) into `nbodies` records of 8 floats (device pointer): Fx, Fy, Fz, tau x, tau y,
        tau z, sum m, max residual.  Needs velocity on and a displace since."""
        arr, n = self._list(cascades)
        self._check(self.lib.datum_ocean_reduce_body_drag(self.h, arr, n, ctypes.byref(oceanset), iterations, _dev(bodies_ptr), _dev(motions_ptr), nbodies,
                                                          _dev(probes_ptr), nprobes, _dev(records_ptr)))

    def read_body_drag(self, cascades, oceanset, bodies, motions, probes, iterations=4):
        """the same from host arrays, blocking: `bodies` an array of BODY_DTYPE, `motions` one of BODY_MOTION_DTYPE of the same length,
        `probes` (n, 4) float32; returns (nbodies, 8)"""
        arr, n = self._list(cascades)
        args, out = _body_batch(bodies, motions, None, probes, DRAG_RECORD_FLOATS)
        self._check(self.lib.datum_ocean_read_body_drag(self.h, arr, n, ctypes.byref(oceanset), iterations, *args, _ptr(out)))
        return out

    # -- body stepping (datum_ocean_step_bodies): buoyancy, drag and a semi-implicit Euler integrator per body, on the device -------------

    def step_bodies(self, cascades, oceanset, bodies_ptr, motions_ptr, props_ptr, nbodies, probes_ptr, nprobes, dt, substeps, records_ptr, iterations=4):
        """Enqueue `substeps` sub-steps of dt / substeps for `nbodies` bodies (device pointers: 64 bytes each, read and written), their motions
        (32 bytes each, read and written) and props (32 bytes each) over `nprobes` probes (16 bytes each) into `nbodies` records of 8 floats:
        Fx, Fy, Fz, tau x, tau y, tau z, sum m of the last sub-step, max residual.  Needs velocity on and a displace since."""
        arr, n = self._list(cascades)
        self._check(self.lib.datum_ocean_step_bodies(self.h, arr, n, ctypes.byref(oceanset), iterations, _dev(bodies_ptr), _dev(motions_ptr), _dev(props_ptr), nbodies,
                                                     _dev(probes_ptr), nprobes, dt, substeps, _dev(records_ptr)))

    def step_bodies_host(self, cascades, oceanset, bodies, motions, props, probes, dt, substeps=1, iterations=4):
        """the same from host arrays, blocking: `bodies` an array of BODY_DTYPE and `motions` one of BODY_MOTION_DTYPE, both contiguous and
        advanced IN PLACE, `props` one of BODY_PROPS_DTYPE of the same length, `probes` (n, 4) float32; returns the (nbodies, 8) records"""
        arr, n = self._list(cascades)
        args, out = _body_batch(bodies, motions, props, probes, STEP_RECORD_FLOATS, in_place=True)
        self._check(self.lib.datum_ocean_step_bodies_host(self.h, arr, n, ctypes.byref(oceanset), iterations, *args, dt, substeps, _ptr(out)))
        return out

    # -- the ripple layer (datum_ocean_set_ripples): a local, scrolling wave grid fed by impulses and by the bodies' wakes ---------------

    def set_ripples(self, R, s=1.0):
        """Switch the layer on with R x R cells of side `s` metres (R one of RIPPLE_SIZES), at rest, origin (-R/2, -R/2); R = 0 frees it."""
        self._check(self.lib.datum_ocean_set_ripples(self.h, R, s))

    def set_ripple_params(self, c=2.0, gamma=0.05, sponge_cells=8, sponge_gamma=4.0):
        """wave speed (m/s), damping (1/s), width of the absorbing border in cells (0: none) and its extra damping at the edge (1/s)"""
        self._check(self.lib.datum_ocean_set_ripple_params(self.h, c, gamma, sponge_cells, sponge_gamma))

    def set_ripple_dispersion(self, mode=RIPPLE_WAVE, g=9.81):
        """the step's mode: RIPPLE_WAVE (the default, the wave equation with speed c) or RIPPLE_DEEP (omega^2 = g |k|, a 13 x 13
        convolution); works while the layer is off, survives set_ripples and writes no state"""
        self._check(self.lib.datum_ocean_set_ripple_dispersion(self.h, mode, g))

    def set_ripple_walls(self, walls=None):
        """obstacles the layer's waves reflect off: `walls` an array of RIPPLE_WALL records (center, axis as (cosine, sine), half, kind
        RIPPLE_WALL_BOX or RIPPLE_WALL_ELLIPSE), at most RIPPLE_MAX_WALLS; None or an empty array turns walls off.  One launch writes
        the plane and zeroes the wall cells' state in both state buffers."""
        w = np.ascontiguousarray(walls if walls is not None else [], RIPPLE_WALL).reshape(-1)
        self._check(self.lib.datum_ocean_set_ripple_walls(self.h, _ptr(w) if len(w) else None, len(w)))

    def ripple_walls_device(self):
        """the device pointer of the wall plane (R x R bytes in memory order), None while walls are off"""
        ptr = P()
        self._check(self.lib.datum_ocean_ripple_walls_device(self.h, ctypes.byref(ptr)))
        return ptr.value

    def read_ripple_walls(self):
        """the wall plane in window order, (R, R) uint8: [j][i] is cell (ox + i, oy + j); blocking"""
        R = int(round((self.ripples_device()[1] // 8) ** 0.5))
        out = np.empty((R, R), np.uint8)
        self._check(self.lib.datum_ocean_read_ripple_walls(self.h, _ptr(out)))
        return out

    def set_ripple_bed(self, bed=None, depths=None):
        """still-water depth under the layer: `bed` a RIPPLE_BED record (width, height, origin, texel, outside, max_depth, dry_depth,
        surf_depth, surf_gamma), `depths` its (height, width) float32 map in metres, positive down; None turns the bed off.  One launch
        rasters the depth and surf planes and zeroes the solid cells' state in both state buffers.  WAVE mode only."""
        if bed is None:
            self._check(self.lib.datum_ocean_set_ripple_bed(self.h, None, None))
            return
        b = np.array([bed], RIPPLE_BED).reshape(-1)[:1]
        d = np.ascontiguousarray(depths, np.float32)
        if d.size != int(b["width"][0]) * int(b["height"][0]):
            raise ValueError("set_ripple_bed: depths must hold width * height values")
        self._check(self.lib.datum_ocean_set_ripple_bed(self.h, _ptr(b), _ptr(d)))

    def ripple_bed_device(self):
        """(depth pointer, surf pointer, cells): the device planes in memory order, R * R floats and R * R bytes; (None, None, 0) while
        the bed is off"""
        depth, surf, cells = P(), P(), ctypes.c_size_t()
        self._check(self.lib.datum_ocean_ripple_bed_device(self.h, ctypes.byref(depth), ctypes.byref(surf), ctypes.byref(cells)))
        return depth.value, surf.value, cells.value

    def read_ripple_bed(self):
        """(depth (R, R) float32, surf (R, R) uint8) in window order: [j][i] is cell (ox + i, oy + j); blocking"""
        R = int(round((self.ripples_device()[1] // 8) ** 0.5))
        depth, surf = np.empty((R, R), np.float32), np.empty((R, R), np.uint8)
        self._check(self.lib.datum_ocean_read_ripple_bed(self.h, _ptr(depth), _ptr(surf)))
        return depth, surf

    def set_ripple_swell(self, on=True):
        """the FFT swell as a source of the layer at every solid face (walls, dry land): True allocates the forcing plane, zeroed and
        not current; False frees it.  WAVE mode only.  The step reads the plane only while it is current (refresh_ripple_swell)."""
        self._check(self.lib.datum_ocean_set_ripple_swell(self.h, int(on)))

    def refresh_ripple_swell(self, cascades, oceanset, iterations=4):
        """one launch writes the forcing plane whole from the summed surface of the listed cascades (sample_surface_blend's list, set
        and iterations), the solid cells and the origin, and marks it current; call it after displace and center_ripples, before a step"""
        arr, n = self._list(cascades)
        self._check(self.lib.datum_ocean_refresh_ripple_swell(self.h, arr, n, ctypes.byref(oceanset), iterations))

    def ripple_swell_device(self):
        """(pointer, bytes, current): the device plane in memory order, R * R floats; (None, 0, False) while swell is off"""
        ptr, nbytes, current = P(), ctypes.c_size_t(), I()
        self._check(self.lib.datum_ocean_ripple_swell_device(self.h, ctypes.byref(ptr), ctypes.byref(nbytes), ctypes.byref(current)))
        return ptr.value, nbytes.value, bool(current.value)

    def read_ripple_swell(self):
        """the forcing plane in MEMORY order, (R, R) float32: [J mod R][I mod R] is world cell (I, J); blocking"""
        R = int(round((self.ripples_device()[1] // 8) ** 0.5))
        out = np.empty((R, R), np.float32)
        self._check(self.lib.datum_ocean_read_ripple_swell(self.h, _ptr(out)))
        return out

    def center_ripples(self, x, y):
        """Move the window so that the cell of (x, y) is its middle; the cells that entered are zeroed, none is copied."""
        self._check(self.lib.datum_ocean_center_ripples(self.h, x, y))

    def reset_ripples(self):
        self._check(self.lib.datum_ocean_reset_ripples(self.h))

    def ripples_device(self):
        """(device pointer of the CURRENT state buffer, bytes, ox, oy); the pointer alternates between two buffers with every sub-step"""
        ptr, nbytes, ox, oy = P(), ctypes.c_size_t(), I(), I()
        self._check(self.lib.datum_ocean_ripples_device(self.h, ctypes.byref(ptr), ctypes.byref(nbytes), ctypes.byref(ox), ctypes.byref(oy)))
        return ptr.value, nbytes.value, ox.value, oy.value

    def read_ripples(self):
        """the current state in window order, (R, R, 2) float32: [j][i] is cell (ox + i, oy + j), (height, rate); blocking"""
        _, nbytes, _, _ = self.ripples_device()
        R = int(round((nbytes // 8) ** 0.5))
        out = np.empty((R, R, 2), np.float32)
        self._check(self.lib.datum_ocean_read_ripples(self.h, _ptr(out)))
        return out

    def step_ripples(self, dt, substeps=1):
        """Enqueue `substeps` sub-steps of dt / substeps, one launch each; the first takes the pending deposits in."""
        self._check(self.lib.datum_ocean_step_ripples(self.h, dt, substeps))

    def deposit_ripples(self, impulses_ptr, n):
        """Enqueue `n` deposits (device pointer, 16 bytes each: x, y, volume in m^3, 0)."""
        self._check(self.lib.datum_ocean_deposit_ripples(self.h, _dev(impulses_ptr), n))

    def deposit_body_ripples(self, cascades, oceanset, bodies_ptr, motions_ptr, nbodies, probes_ptr, nprobes, dt, records_ptr, iterations=4):
        """Enqueue the wake of `nbodies` bodies over dt: reduce_body_drag's arguments; records of 8 floats: sum Vh, sum m sx, sum m sy,
        dropped quanta, 0, 0, sum m, max residual.  Needs velocity on and a displace since."""
        arr, n = self._list(cascades)
        self._check(self.lib.datum_ocean_deposit_body_ripples(self.h, arr, n, ctypes.byref(oceanset), iterations, _dev(bodies_ptr), _dev(motions_ptr), nbodies,
                                                              _dev(probes_ptr), nprobes, dt, _dev(records_ptr)))

    def deposit_ripples_host(self, impulses):
        """the same from a host array, blocking: `impulses` (n, 4) float32"""
        imp = np.ascontiguousarray(impulses, np.float32).reshape(-1, 4)
        self._check(self.lib.datum_ocean_deposit_ripples_host(self.h, _ptr(imp), imp.shape[0]))

    def deposit_body_ripples_host(self, cascades, oceanset, bodies, motions, probes, dt, iterations=4):
        """the wake from host arrays, blocking: `bodies` an array of BODY_DTYPE, `motions` one of BODY_MOTION_DTYPE of the same length,
        `probes` (n, 4) float32; returns (nbodies, 8)"""
        arr, n = self._list(cascades)
        args, out = _body_batch(bodies, motions, None, probes, RIPPLE_RECORD_FLOATS)
        self._check(self.lib.datum_ocean_deposit_body_ripples_host(self.h, arr, n, ctypes.byref(oceanset), iterations, *args, dt, _ptr(out)))
        return out

    def sample_ripples(self, points_ptr, n, out_ptr):
        """Enqueue the sample of `n` points (device pointer, 8 bytes each) into `n` float4 (device pointer): height, d/dx, d/dy, rate."""
        self._check(self.lib.datum_ocean_sample_ripples(self.h, _dev(points_ptr), n, _dev(out_ptr)))

    def query_ripples(self, points):
        """the same from a host array, blocking: `points` (n, 2) float32; returns (n, 4) float32"""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        out = np.empty((p.shape[0], 4), np.float32)
        self._check(self.lib.datum_ocean_query_ripples(self.h, _ptr(p), p.shape[0], _ptr(out)))
        return out

    # -- coupled stepping (datum_ocean_step_bodies_coupled): bodies and the ripple layer advance together, the wake pushes back ----------

    def step_bodies_coupled(self, cascades, oceanset, bodies_ptr, motions_ptr, props_ptr, nbodies, probes_ptr, nprobes, dt, substeps, records_ptr, iterations=4):
        """Enqueue `substeps` coupled sub-steps of dt / substeps: step_bodies' arguments (device pointers), with records of 12 floats per body:
        Fx, Fy, Fz, tau x, tau y, tau z, sum m of the last sub-step, max residual, the wake's sum Vh, sum m sx, sum m sy of the last sub-step,
        dropped quanta of all sub-steps.  Each sub-step the bodies feel the layer's height and rate and deposit their wake, then the layer
        steps.  Needs velocity on, a displace since, and the layer on."""
        arr, n = self._list(cascades)
        self._check(self.lib.datum_ocean_step_bodies_coupled(self.h, arr, n, ctypes.byref(oceanset), iterations, _dev(bodies_ptr), _dev(motions_ptr), _dev(props_ptr),
                                                             nbodies, _dev(probes_ptr), nprobes, dt, substeps, _dev(records_ptr)))

    def step_bodies_coupled_host(self, cascades, oceanset, bodies, motions, props, probes, dt, substeps=1, iterations=4):
        """the same from host arrays, blocking: `bodies` and `motions` as step_bodies_host takes them, advanced IN PLACE; returns the
        (nbodies, 12) records"""
        arr, n = self._list(cascades)
        args, out = _body_batch(bodies, motions, props, probes, COUPLED_RECORD_FLOATS, in_place=True)
        self._check(self.lib.datum_ocean_step_bodies_coupled_host(self.h, arr, n, ctypes.byref(oceanset), iterations, *args, dt, substeps, _ptr(out)))
        return out

    # -- body contact (datum_ocean_step_bodies_contact): the coupled step with hulls that stop at ripple walls and ground on the bed -----

    def step_bodies_contact(self, cascades, oceanset, bodies_ptr, motions_ptr, props_ptr, nbodies, probes_ptr, nprobes, dt, substeps, records_ptr, contact, iterations=4):
        """step_bodies_coupled with penalty contact: `contact` a BodyContact (stiffness, damping, friction per unit probe weight, flags
        CONTACT_BED | CONTACT_WALLS); records of 16 floats per body: the coupled record's twelve, the contact force of the last sub-step,
        the deepest penetration of all sub-steps.  A flag needs its object set (set_ripple_bed, set_ripple_walls)."""
        arr, n = self._list(cascades)
        self._check(self.lib.datum_ocean_step_bodies_contact(self.h, arr, n, ctypes.byref(oceanset), iterations, _dev(bodies_ptr), _dev(motions_ptr), _dev(props_ptr),
                                                             nbodies, _dev(probes_ptr), nprobes, dt, substeps, _dev(records_ptr), ctypes.cast(ctypes.byref(contact), P)))

    def step_bodies_contact_host(self, cascades, oceanset, bodies, motions, props, probes, dt, contact, substeps=1, iterations=4):
        """the same from host arrays, blocking: `bodies` and `motions` advanced IN PLACE; returns the (nbodies, 16) records"""
        arr, n = self._list(cascades)
        args, out = _body_batch(bodies, motions, props, probes, CONTACT_RECORD_FLOATS, in_place=True)
        self._check(self.lib.datum_ocean_step_bodies_contact_host(self.h, arr, n, ctypes.byref(oceanset), iterations, *args, dt, substeps, _ptr(out),
                                                                  ctypes.cast(ctypes.byref(contact), P)))
        return out

    # -- rippled reads (datum_ocean_gen_blend_rippled): the mesh, the query and the cast with the ripple layer's height and slopes on top -----

    def gen_blend_rippled(self, cascades, oceanset, sizex, sizey, vertices_device_ptr):
        """gen_blend() with the layer sampled at each vertex's stored (x, y): z lifted by its height, its slopes in the shaded normal"""
        arr, n = self._list(cascades)
        self._check(self.lib.datum_ocean_gen_blend_rippled(self.h, arr, n, ctypes.byref(oceanset), sizex, sizey, P(vertices_device_ptr)))

    def sample_surface_blend_rippled(self, cascades, oceanset, points_ptr, count, samples_ptr, iterations=4):
        """sample_surface_blend() with the layer sampled at the asked point: device pointers, enqueued on the handle's stream"""
        self._sample_points(self.lib.datum_ocean_sample_surface_blend_rippled, cascades, oceanset, iterations, points_ptr, count, samples_ptr)

    def read_surface_blend_rippled(self, cascades, oceanset, points, iterations=4):
        """the same from a host (M, 2) float32 array, blocking; returns (M, 8) float32"""
        return self._read_points(self.lib.datum_ocean_read_surface_blend_rippled, cascades, oceanset, iterations, points, SURFACE_SAMPLE_FLOATS)

    def cast_rays_rippled(self, cascades, oceanset, rays_ptr, n, records_ptr, iterations=4, steps=32, refine=8):
        """cast_rays() on the rippled water: every height of the search and the record at hi carry the layer"""
        self._cast(self.lib.datum_ocean_cast_rays_rippled, cascades, oceanset, iterations, steps, refine, rays_ptr, n, records_ptr)

    def read_rays_rippled(self, cascades, oceanset, rays, iterations=4, steps=32, refine=8):
        """the same from a host array, blocking: `rays` (n, 8) float32; returns (n, 12) float32"""
        return self._read_cast(self.lib.datum_ocean_read_rays_rippled, cascades, oceanset, iterations, steps, refine, rays)

    # -- ripple-layer bounds (datum_ocean_reduce_ripple_bounds), the rippled slab and the rippled casts that skip the samples it decides -----

    def reduce_ripple_bounds(self):
        """Enqueue the reduction of the layer's current state to its record; the record is current until the next call that writes a state
        buffer (step_ripples, step_bodies_coupled, a center_ripples that moves the window, reset_ripples, set_ripples)."""
        self._check(self.lib.datum_ocean_reduce_ripple_bounds(self.h))

    def ripple_bounds_device(self):
        """(device pointer, bytes) of the layer's record, 32 bytes"""
        p = P()
        n = ctypes.c_size_t()
        self._check(self.lib.datum_ocean_ripple_bounds_device(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def read_ripple_bounds(self):
        """reduce_ripple_bounds and a blocking read: (8,) float32 -- etamin, etamax, ratemin, ratemax, nonfinite, active, 0, 0"""
        out = np.empty(RIPPLE_BOUNDS_RECORD_FLOATS, np.float32)
        self._check(self.lib.datum_ocean_read_ripple_bounds(self.h, _ptr(out)))
        return out

    def surface_slab_rippled(self, cascades, oceanset):
        """blocking: (zlo, zhi, reachx, reachy) of the listed cascades' summed surface with the ripple layer on top, as float32"""
        arr, c = self._list(cascades)
        out = np.zeros(4, np.float32)
        base = out.ctypes.data
        self._check(self.lib.datum_ocean_surface_slab_rippled(self.h, arr, c, ctypes.byref(oceanset), P(base), P(base + 4), P(base + 8), P(base + 12)))
        return out[0], out[1], out[2], out[3]

    def cast_rays_rippled_bounded(self, cascades, oceanset, rays_ptr, n, records_ptr, iterations=4, steps=32, refine=8):
        """cast_rays_rippled with the samples outside the rippled slab decided without a height evaluation: the same records bit for bit.
        Needs current bounds of the maps (reduce_bounds) AND of the layer (reduce_ripple_bounds), else OceanError(ESTATE)."""
        self._cast(self.lib.datum_ocean_cast_rays_rippled_bounded, cascades, oceanset, iterations, steps, refine, rays_ptr, n, records_ptr)

    def read_rays_rippled_bounded(self, cascades, oceanset, rays, iterations=4, steps=32, refine=8):
        """the same from a host array, blocking: `rays` (n, 8) float32; returns (n, 12) float32"""
        return self._read_cast(self.lib.datum_ocean_read_rays_rippled_bounded, cascades, oceanset, iterations, steps, refine, rays)

    # -- wake foam (datum_ocean_set_ripple_foam): a coverage plane beside the ripple layer, fed by its slopes and rates --------------------

    def set_ripple_foam(self, on=True):
        """Allocate and zero the R x R coverage plane beside the ripple layer, or free it; OceanError(ESTATE) while the layer is off."""
        self._check(self.lib.datum_ocean_set_ripple_foam(self.h, 1 if on else 0))

    def set_ripple_foam_params(self, t1=0.04, k1=10.0, t2=0.5, k2=2.0, decay=0.5):
        """threshold and gain of the slope-squared source, threshold (m/s) and gain of the rate source, decay (1/s); a gain of 0 switches
        its source off.  The defaults are design choices, not measurements."""
        self._check(self.lib.datum_ocean_set_ripple_foam_params(self.h, t1, k1, t2, k2, decay))

    def step_ripple_foam(self, dt):
        """Enqueue one update of the plane from the layer's current state: one launch; the old coverage fades by exp(-decay dt)."""
        self._check(self.lib.datum_ocean_step_ripple_foam(self.h, dt))

    def reset_ripple_foam(self):
        self._check(self.lib.datum_ocean_reset_ripple_foam(self.h))

    def ripple_foam_device(self):
        """(device pointer of the plane, bytes, ox, oy); the pointer does not alternate"""
        ptr, nbytes, ox, oy = P(), ctypes.c_size_t(), I(), I()
        self._check(self.lib.datum_ocean_ripple_foam_device(self.h, ctypes.byref(ptr), ctypes.byref(nbytes), ctypes.byref(ox), ctypes.byref(oy)))
        return ptr.value, nbytes.value, ox.value, oy.value

    def read_ripple_foam(self):
        """the plane in window order, (R, R) float32: [j][i] is cell (ox + i, oy + j); blocking"""
        _, nbytes, _, _ = self.ripple_foam_device()
        R = int(round((nbytes // 4) ** 0.5))
        out = np.empty((R, R), np.float32)
        self._check(self.lib.datum_ocean_read_ripple_foam(self.h, _ptr(out)))
        return out

    def sample_ripple_foam(self, points_ptr, n, out_ptr):
        """Enqueue the sample of `n` points (device pointer, 8 bytes each) into `n` floats (device pointer): the bilinear coverage."""
        self._check(self.lib.datum_ocean_sample_ripple_foam(self.h, _dev(points_ptr), n, _dev(out_ptr)))

    def query_ripple_foam(self, points):
        """the same from a host array, blocking: `points` (n, 2) float32; returns (n,) float32"""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        out = np.empty(p.shape[0], np.float32)
        self._check(self.lib.datum_ocean_query_ripple_foam(self.h, _ptr(p), p.shape[0], _ptr(out)))
        return out

    # -- ray casts (datum_ocean_cast_rays): a fixed march and bisection per ray on the summed surface -----------------------------------

    def cast_rays(self, cascades, oceanset, rays_ptr, n, records_ptr, iterations=4, steps=32, refine=8):
        """Enqueue the cast of `n` rays (device pointer, 32 bytes each: ox, oy, oz, tmin, dx, dy, dz, tmax) into `n` records of 12 floats
        (device pointer): hi, lo, g(hi), status (0 miss, 1 enter, 2 leave) and the surface record at hi."""
        self._cast(self.lib.datum_ocean_cast_rays, cascades, oceanset, iterations, steps, refine, rays_ptr, n, records_ptr)

    def read_rays(self, cascades, oceanset, rays, iterations=4, steps=32, refine=8):
        """the same from a host array, blocking: `rays` (n, 8) float32; returns (n, 12) float32"""
        return self._read_cast(self.lib.datum_ocean_read_rays, cascades, oceanset, iterations, steps, refine, rays)

    # -- surface bounds (datum_ocean_reduce_bounds) and the ray casts that skip the samples they decide ------------------------------------

    def reduce_bounds(self):
        """Enqueue the reduction of every cascade's maps to its record; the records are current until the next displace or bind_maps."""
        self._check(self.lib.datum_ocean_reduce_bounds(self.h))

    def bounds_device(self):
        """(device pointer, bytes) of the handle's records, cascades x 32 bytes"""
        p = P()
        n = ctypes.c_size_t()
        self._check(self.lib.datum_ocean_bounds_device(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def read_bounds(self):
        """reduce_bounds and a blocking read: (cascades, 8) float32 -- zmin, zmax, xmin, xmax, ymin, ymax, nonfinite, 0"""
        out = np.empty((self.cascades, BOUNDS_RECORD_FLOATS), np.float32)
        self._check(self.lib.datum_ocean_read_bounds(self.h, _ptr(out)))
        return out

    def surface_slab(self, cascades, oceanset):
        """blocking: (zlo, zhi, reachx, reachy) of the listed cascades' summed surface under `oceanset`, as float32"""
        arr, c = self._list(cascades)
        out = np.zeros(4, np.float32)
        base = out.ctypes.data
        self._check(self.lib.datum_ocean_surface_slab(self.h, arr, c, ctypes.byref(oceanset), P(base), P(base + 4), P(base + 8), P(base + 12)))
        return out[0], out[1], out[2], out[3]

    def cast_rays_bounded(self, cascades, oceanset, rays_ptr, n, records_ptr, iterations=4, steps=32, refine=8):
        """cast_rays with the samples outside the slab decided without a height evaluation: the same records bit for bit.  Needs current
        bounds (reduce_bounds after the last displace or bind_maps), else OceanError(ESTATE)."""
        self._cast(self.lib.datum_ocean_cast_rays_bounded, cascades, oceanset, iterations, steps, refine, rays_ptr, n, records_ptr)

    def read_rays_bounded(self, cascades, oceanset, rays, iterations=4, steps=32, refine=8):
        """the same from a host array, blocking: `rays` (n, 8) float32; returns (n, 12) float32"""
        return self._read_cast(self.lib.datum_ocean_read_rays_bounded, cascades, oceanset, iterations, steps, refine, rays)

    def algorithmic_bytes(self):
        row, col = D(), D()
        self._check(self.lib.datum_ocean_algorithmic_bytes(self.h, ctypes.byref(row), ctypes.byref(col)))
        return row.value, col.value


def farm_unique_id():
    """The 128-byte id of a new farm communicator (rank 0 makes it, every rank passes it to Ocean.farm_init)."""
    buf = (ctypes.c_char * FARM_ID_BYTES)()
    rc = load().datum_ocean_farm_unique_id(buf, FARM_ID_BYTES)
    if rc != 0:
        raise OceanError(rc, load().datum_ocean_last_error(None).decode())
    return bytes(buf)


def map_layout(N):
    """(PW, PH, B, texel_bytes) of the device map layout at resolution N (include/datum_ocean_hip.h: datum_ocean_bind_maps):
    patches of PW x PH = 16 texels of 24 bytes, bands of B columns."""
    gx, gy, b, tb = I(), I(), I(), I()
    rc = load().datum_ocean_map_layout(N, ctypes.byref(gx), ctypes.byref(gy), ctypes.byref(b), ctypes.byref(tb))
    if rc != 0:
        raise OceanError(rc, load().datum_ocean_last_error(None).decode())
    return gx.value, gy.value, b.value, tb.value


def map_block_floats(N):
    """floats of one cascade's DEVICE map block"""
    return N * N * map_layout(N)[3] // 4


def map_layers(raw, N):
    """One cascade's DEVICE map block (map_block_floats(N) floats as the kernels lay them out, include/datum_ocean_hip.h) as
    the reference's logical image [layer][y][x][4] (.w = 0).  Works on numpy arrays and torch tensors alike.
    Bands of B columns, patches of PW x PH texels, 16 x (dx, dy, dz, nx) then 16 x (ny, nz) per patch."""
    GX, GY, B, TB = map_layout(N)
    assert TB == 24
    torchlike = hasattr(raw, "permute")
    v = raw.reshape(N // B, N // GY, B // GX, 96)                  # [band][y / PH][patch][96 floats]
    a = v[..., :64].reshape(N // B, N // GY, B // GX, GY, GX, 4)   # (dx, dy, dz, nx) per texel
    b = v[..., 64:].reshape(N // B, N // GY, B // GX, GY, GX, 2)   # (ny, nz) per texel
    order = (1, 3, 0, 2, 4, 5)                                     # -> [y / PH][y % PH][band][patch][x % PW][component]
    if torchlike:
        import torch

        a, b = a.permute(*order).reshape(N, N, 4), b.permute(*order).reshape(N, N, 2)
        z = torch.zeros_like(a[..., :1])
        return torch.stack([torch.cat([a[..., :3], z], -1), torch.cat([a[..., 3:], b, z], -1)])
    a, b = a.transpose(*order).reshape(N, N, 4), b.transpose(*order).reshape(N, N, 2)
    z = np.zeros_like(a[..., :1])
    return np.stack([np.concatenate([a[..., :3], z], -1), np.concatenate([a[..., 3:], b, z], -1)])


def reference_weights(N):
    stages = int(np.log2(N))
    w = np.empty((N, 2 * stages), np.float32)
    rc = load().datum_ocean_reference_weights(N, _ptr(w))
    if rc != 0:
        raise OceanError(rc, load().datum_ocean_last_error(None).decode())
    return w
