/* datum_ocean_hip.h -- C ABI of the MI355X (gfx950) ocean compute module.
 *
 * This is the drop-in boundary: the entry points below replace what
 * datum's src/renderer/ocean.cpp does through Vulkan compute between ":757" and ":803"
 * (five bind_pipeline + dispatch pairs: ocean.sim, ocean.fftx, ocean.ffty, ocean.map,
 * ocean.gen) plus the per-tick CPU phase advance of update_ocean (":217-236"), the
 * twiddle/spectrum/displacement-map allocations of prepare_ocean_context (":686-711") and the
 * per-frame OceanSet upload (":729-749").  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - every function returns 0 on success; a negative DATUM_OCEAN_E* code of this module (misuse, or ENOTREADY from the
 *     two polling calls); a positive value is a hipError_t (an ncclResult_t never leaves the module: the farm entry points
 *     map it to DATUM_OCEAN_ECOMM).  Nothing throws.  datum_ocean_last_error() gives the text.
 *     (reference: throw std::runtime_error on device failure, ocean.cpp:271 / vulkan.cpp:550;
 *     the C++ shim in datum_amd/host re-throws.)
 *   - one HIP stream per handle; calls enqueue and return; datum_ocean_sync() is the fence wait of
 *     ocean.cpp:725.  A handle is not re-entrant; distinct handles (GPUs) are independent.
 *   - h0 / phase stay device resident (the reference re-uploads 12*N*N bytes per frame).
 *   - "cascade" = one independent (OceanParams, N x N grid) problem; the reference has exactly one.
 *   - all arrays are fp32, row-major [m = y][n = x] like OceanParams (ocean.h:69-71).
 */

#ifndef DATUM_OCEAN_HIP_H
#define DATUM_OCEAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DATUM_OCEAN_MAX_CASCADES 16

/* Version of THIS header's contract: bumped whenever a signature, an error code's value or the device layout of a bound map
 * buffer changes (the shared object carries no soname).  A consumer compares it with what the library it loaded reports before its
 * first call -- datum_amd/capi.py, the C++ host shim (initialise_ocean_context) and both examples do -- so that a stale
 * libdatum_ocean_hip.so is refused instead of misread.
 *   3  round 3: ENOTREADY = +1, datum_ocean_map_layout with four arguments, 32-byte texels
 *   4  round 4: ENOTREADY = -5, datum_ocean_map_layout gained texel_bytes, 24-byte texels in bound map buffers, farm entry points
 *   5  round 5: datum_ocean_abi_version, datum_ocean_export_maps, datum_ocean_set_literal_transform
 *   6  round 5: datum_ocean_farm_partition, datum_ocean_own_stream
 *   7  round 6: datum_ocean_set_cascade_group / datum_ocean_cascade_group (DATUM_OCEAN_SPECTRUM_FP16_H0, a further value of an existing
 *      argument, came later in the round without a bump)
 *   8  round 6: datum_ocean_set_map_store_policy / datum_ocean_map_store_policy
 *   9  the Jacobian foam plane: datum_ocean_set_foam, datum_ocean_set_foam_params, datum_ocean_reset_foam, datum_ocean_bind_foam,
 *      datum_ocean_foam_device, datum_ocean_read_foam, datum_ocean_upload_height.
 *      Later added at 9 without a bump (nothing changed, entry points were only added): the surface queries datum_ocean_sample_surface and
 *      datum_ocean_read_surface; then the phase write-back interval, datum_ocean_set_phase_writeback and datum_ocean_phase_writeback; then
 *      the several-cascade calls datum_ocean_gen_blend, datum_ocean_sample_surface_blend and datum_ocean_read_surface_blend; then body
 *      buoyancy, datum_ocean_reduce_bodies and datum_ocean_read_bodies; then ray casts, datum_ocean_cast_rays and datum_ocean_read_rays; then
 *      surface bounds, datum_ocean_reduce_bounds, datum_ocean_bounds_device, datum_ocean_read_bounds and datum_ocean_surface_slab, with the
 *      bounded casts datum_ocean_cast_rays_bounded and datum_ocean_read_rays_bounded; then the surface velocity, datum_ocean_set_velocity,
 *      datum_ocean_bind_velocity, datum_ocean_velocity_device, datum_ocean_read_velocity, datum_ocean_sample_velocity_blend and
 *      datum_ocean_read_velocity_blend; then body drag, datum_ocean_reduce_body_drag and datum_ocean_read_body_drag; then body stepping,
 *      datum_ocean_step_bodies and datum_ocean_step_bodies_host; then the ripple layer, datum_ocean_set_ripples,
 *      datum_ocean_set_ripple_params, datum_ocean_center_ripples, datum_ocean_reset_ripples, datum_ocean_ripples_device,
 *      datum_ocean_read_ripples, datum_ocean_step_ripples, datum_ocean_deposit_ripples, datum_ocean_deposit_ripples_host,
 *      datum_ocean_deposit_body_ripples, datum_ocean_deposit_body_ripples_host, datum_ocean_sample_ripples and datum_ocean_query_ripples;
 *      then coupled stepping, datum_ocean_step_bodies_coupled and datum_ocean_step_bodies_coupled_host; then the rippled reads,
 *      datum_ocean_gen_blend_rippled, datum_ocean_sample_surface_blend_rippled, datum_ocean_read_surface_blend_rippled,
 *      datum_ocean_cast_rays_rippled and datum_ocean_read_rays_rippled; then the ripple layer's bounds, datum_ocean_reduce_ripple_bounds,
 *      datum_ocean_ripple_bounds_device, datum_ocean_read_ripple_bounds and datum_ocean_surface_slab_rippled, with the bounded rippled
 *      casts datum_ocean_cast_rays_rippled_bounded and datum_ocean_read_rays_rippled_bounded; then wake foam, datum_ocean_set_ripple_foam,
 *      datum_ocean_set_ripple_foam_params, datum_ocean_step_ripple_foam, datum_ocean_reset_ripple_foam, datum_ocean_ripple_foam_device,
 *      datum_ocean_read_ripple_foam, datum_ocean_sample_ripple_foam and datum_ocean_query_ripple_foam; then dispersive ripples,
 *      datum_ocean_set_ripple_dispersion and datum_ocean_ripple_deep_weights; then ripple walls, datum_ocean_set_ripple_walls,
 *      datum_ocean_ripple_walls_device and datum_ocean_read_ripple_walls; then the ripple bed, datum_ocean_set_ripple_bed,
 *      datum_ocean_ripple_bed_device and datum_ocean_read_ripple_bed; then the phase's store, datum_ocean_set_phase_store and
 *      datum_ocean_phase_store; then ripple swell, datum_ocean_set_ripple_swell, datum_ocean_refresh_ripple_swell,
 *      datum_ocean_ripple_swell_device and datum_ocean_read_ripple_swell.
 *      A consumer that needs them detects them by symbol (dlsym), not by the version */
#define DATUM_OCEAN_ABI_VERSION 9
int datum_ocean_abi_version(void);

enum
{
  DATUM_OCEAN_OK = 0,
  DATUM_OCEAN_EINVAL = -1,    /* bad argument (null pointer, unsupported resolution, cascade out of range) */
  DATUM_OCEAN_ESTATE = -2,    /* call order misuse (e.g. displace before upload_state)                     */
  DATUM_OCEAN_ENOMEM = -3,
  DATUM_OCEAN_EUNSUPPORTED = -4,  /* the HIP runtime on this machine lacks the feature (external semaphores on ROCm 7.0.x: use the
                                   host bridge, datum_ocean_on_complete / datum_ocean_query)                                  */
  DATUM_OCEAN_ECOMM = -6,         /* an RCCL call of the tile farm failed (datum_ocean_last_error has RCCL's own text)          */
  DATUM_OCEAN_ENOTREADY = -5      /* datum_ocean_query / datum_ocean_farm_query only: the work is still running (not a failure).
                                   A module code, because every positive return value is a hipError_t (hipErrorInvalidValue
                                   is 1) and a poller must be able to tell "not yet" from "the query itself failed"         */
};

typedef struct datum_ocean_ctx *datum_ocean_t;

/* The head of the reference's OceanSet SSBO (src/renderer/ocean.cpp:33-50; every shader mirrors it,
 * e.g. data/ocean.gen.comp:15-36): std430, row_major, same byte offsets, sizeof == 216.
 * Quaternions are (w, x, y, z) (data/transform.inc:13-28).  h0[] / phase[] that follow in the
 * reference struct live on the device here (datum_ocean_upload_state). */
typedef struct datum_ocean_set
{
  float proj[16];          /*   0  Camera::proj(), camera.cpp:77-89                        */
  float invproj[16];       /*  64  inverse(proj), ocean.cpp:732                            */
  float camera_real[4];    /* 128  camera.transform().real                                 */
  float camera_dual[4];    /* 144  camera.transform().dual                                 */
  float plane[4];          /* 160  (normal, distance), ocean.cpp:735                       */
  float swelllength;       /* 176 */
  float swellamplitude;    /* 180 */
  float swellsteepness;    /* 184 */
  float swellphase;        /* 188 */
  float swelldirection[2]; /* 192 */
  float scale;             /* 200  1 / wavescale, ocean.cpp:743                            */
  float choppiness;        /* 204 */
  float smoothing;         /* 208  1 / params.smoothing, ocean.cpp:745                     */
  uint32_t size;           /* 212  WaveResolution                                          */
} datum_ocean_set;

/* -- lifetime (replaces initialise_ocean_context / prepare_ocean_context, ocean.cpp:325-716) ------------ */

/* resolution: 64 (the reference's WaveResolution, ocean.h:16), 128, 256, 512, 1024, 2048 or 4096.
 * Allocates h0, phase, the work spectrum (ocean.cpp:61-68) and the 2-layer displacement map (ocean.cpp:706; stored as
 * 24-byte texels, datum_ocean_bind_maps) for `cascades` grids on HIP device `device`, and builds the twiddle table. */
int datum_ocean_create(datum_ocean_t *out, int device, int resolution, int cascades);
int datum_ocean_destroy(datum_ocean_t ctx);

/* use_own == 0: enqueue on the caller's hipStream_t (passed as void*; NULL is HIP's default stream).
 * use_own != 0: back to the handle's own stream.  Drains the stream in use before switching. */
int datum_ocean_set_stream(datum_ocean_t ctx, void *hip_stream, int use_own);

/* Let the displacement maps be written into caller-owned DEVICE memory of cascades * N * N * texel_bytes bytes (e.g. a buffer
 * that is later all-gathered); NULL restores the handle's own buffer.
 * DEVICE LAYOUT of a cascade's map block (the reference's displacementmap is a VK_IMAGE_TILING_OPTIMAL image,
 * ocean.cpp:706, whose physical layout is the driver's; its only reader is ocean.gen's sampler, ocean.cpp:759): 24 bytes per
 * texel -- the .w channels of the two RGBA32F layers are constant zero (map.comp:79-80) and are not stored.  Bands of B
 * columns (B = N except for the largest grids); inside a band PATCHES of PW x PH = 16 texels, patch rows one after the other;
 * a patch is 384 bytes = three 128-byte lines: 16 x float4 (dx, dy, dz, nx), then 16 x float2 (ny, nz), texel
 * j = (y % PH) * PW + x % PW of the patch at 16 j and 256 + 8 j.
 *   byte offset of texel (x, y)'s patch = (x / B) * 24 N B + ((y / PH) * (B / PW) + (x % B) / PW) * 384
 * with (PW, PH, B, texel_bytes) from datum_ocean_map_layout (texel_bytes = 24).
 * datum_ocean_read_maps returns the reference's logical image [layer][y][x][4] with .w = 0 on the host,
 * datum_ocean_export_maps writes the same image into device memory (a Vulkan-visible RGBA32F image). */
int datum_ocean_bind_maps(datum_ocean_t ctx, void *device_ptr, size_t bytes);
int datum_ocean_map_layout(int resolution, int *group_cols, int *group_rows, int *band, int *texel_bytes);
int datum_ocean_maps_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes);

/* -- state (OceanParams arrays, ocean.h:67-72) ------------------------------------------------------- */

/* per-cascade wave constants used by sim / map: OceanSet.scale = 1/wavescale, OceanSet.choppiness */
int datum_ocean_set_cascade(datum_ocean_t ctx, int cascade, float wavescale, float choppiness);

/* h0 = OceanParams::height, N*N*2 floats (ocean.cpp:748); phase = OceanParams::phase, N*N floats
 * (ocean.cpp:749) or NULL for all-zero (seed_ocean, ocean.cpp:144).  Host pointers. */
/* Extension (BASELINE.json configs[4]): how the work spectrum between the two passes is stored.  FP32 (default): 16 B
 * per point.  FP16: 8 B per point, arithmetic stays fp32; the values are scaled by a power of two sized from max |h0|
 * so that no row sum can overflow a half.  Displacement RMSE then 5e-5 .. 1.1e-4 of the largest displacement with the
 * example's parameters (tests state 4e-4; each stored half is the rounding of the fp32 row-pass value, and the column pass that
 * reads them is at fp32 precision: tests/test_gpu_pointwise.py).  Takes effect at the next datum_ocean_displace.
 * FP16_H0 (round 6; SURVEY.md 8d's own byte count for that config -- "spectrum + intermediates stored fp16": h0 4 B/pt): FP16, and the
 * row pass reads h0 as two halves per point as well, from a copy the module keeps beside the fp32 h0 (4 more bytes per point of
 * device memory; rebuilt on the device whenever h0 changes: upload, rebuild from the seed, resume): h0 times the power of two that
 * brings its largest component just under 2^15, rounded to nearest even.  What the caller uploads and fetches stays fp32; the phase
 * state never passes through a half and stays bit-exact.  Same stated tolerance (4e-4 of the largest displacement; measured with
 * the example's parameters: tests/test_gpu_parity.py, tests/test_gpu_pointwise.py). */
#define DATUM_OCEAN_SPECTRUM_FP32 0
#define DATUM_OCEAN_SPECTRUM_FP16 1
#define DATUM_OCEAN_SPECTRUM_FP16_H0 2
int datum_ocean_set_spectrum_format(datum_ocean_t ctx, int format);   /* DATUM_OCEAN_ESTATE while a profile is open (the format can change the cascade groups its samples are per) or the literal mode is on */

/* VALIDATION MODE (round 5): displace through the reference's own algorithm instead of the fused kernels -- ocean.sim, log2 N
 * radix-2 Stockham stages along rows and along columns with the LITERAL twiddle table of ocean.cpp:686-700 (cos / sin of unreduced
 * fp32 angles, datum_ocean_reference_weights), ocean.map -- the same operations in the same order as data/ocean.{sim,fftx,ffty,map}.comp,
 * one thread per point.  For comparing a HIP frame with a frame of the Vulkan build texel for texel: the fused path differs from the
 * literal arithmetic by that table's own error (RMSE 1.4e-5 at 1024^2, 7e-5 at 4096^2; it is the one closer to a float64 transform).
 * 4-17 x slower than the fused step (tools/literal_bench.py), 24 * N * N bytes of extra device memory once switched on; phase, maps, gen, read_maps,
 * export_maps and the farm work as before.  Takes effect at the next datum_ocean_displace. */
int datum_ocean_set_literal_transform(datum_ocean_t ctx, int on);   /* DATUM_OCEAN_ESTATE while a profile is open or the spectrum format is FP16 (and those two refuse while the mode is on) */

/* Cascades per launch of the two kernels (ABI 7).  The reference records one dispatch per shader for its one grid (ocean.cpp:769-789).
 * A handle whose working set (52 bytes per point and cascade, 44 with the fp16 spectrum) is at most 300 MB, resident in the Infinity Cache,
 * takes every cascade in one launch per kernel.  Beyond that the maps are streamed past the cache and row pass and column pass are launched
 * group by group -- row(g), column(g), row(g + 1), ... on the handle's stream -- so that what a group's row pass leaves for its column pass
 * (and h0 and the phase from step to step) stays in the cache: 0 (default) = the module's choice, the largest group whose 28 (20) bytes
 * per point fit 240 MB -- 8 cascades of 1024^2, 2 of 2048^2, 1 of 4096^2 -- in groups of equal size; n > 0: n cascades per launch (n >= cascades:
 * one launch per kernel).  Results do not depend on the group.  The getter reports the group in use and the launches per kernel and
 * displace call. */
int datum_ocean_set_cascade_group(datum_ocean_t ctx, int cascades_per_launch);
int datum_ocean_cascade_group(datum_ocean_t ctx, int *cascades_per_launch, int *launches_per_pass);

/* How the column pass stores the maps (ABI 8): written through (sc0 sc1: the lines stay in the Infinity Cache for ocean.gen and the next
 * step) or streamed (nt: past the cache).  AUTO (default): written through while the handle's working set is resident in the cache AND no
 * multi-rank farm is initialised; streamed otherwise -- a collective's gathered buffer (7 peers' payloads at 8 ranks: 352 MB per batch at
 * 1024^2 x 4) competes for the same cache, and with the maps kept out of it the step loses less under the collective (one-GPU stand-in,
 * profiles/r06_farm_standin.txt: 58.5-61.7 k -> 63.2-64.1 k grids/s at 1024^2 x 4, 13.9-14.1 k -> 14.7-15.4 k at 2048^2 x 1; without a
 * collective in flight streaming costs 2-4 % there).  The explicit values override that.  Grids below 1024^2 are always written through
 * and 4096^2 always streams (there is one form of their kernels).  Results do not depend on the policy.  The getter reports the policy
 * set and whether the next displace will stream. */
#define DATUM_OCEAN_MAPS_AUTO 0
#define DATUM_OCEAN_MAPS_WRITTEN_THROUGH 1
#define DATUM_OCEAN_MAPS_STREAMED 2
int datum_ocean_set_map_store_policy(datum_ocean_t ctx, int policy);
int datum_ocean_map_store_policy(datum_ocean_t ctx, int *policy, int *streamed);

/* How often the row pass writes the advanced phase back (added at ABI 9 without a bump: both entry points exist from the library build that
 * has the lazy write-back on; a consumer detects them by symbol).  datum_ocean_update only queues dt and the row pass of the next
 * datum_ocean_displace applies it to the phase it loads.  Nothing but the next row pass reads what it would store, so it stores only once
 * its list of applied dt's has reached `every` (1 ... 8; 1 = every row pass that advances, the behaviour of earlier builds; 0 = the
 * module's choice, the default) and is otherwise handed the same dt's again, in front of the newer ones: the same instructions on the same
 * stored value, so every map, every foam value and every phase a caller can obtain is bit for bit what `every` = 1 gives.
 * WHAT A CALLER MAY ASSUME: the device's phase array is private to the module, and every call that returns, copies, replaces or
 * re-interprets the phase brings it up to date first -- datum_ocean_read_state, datum_ocean_park_state / datum_ocean_resume_state,
 * datum_ocean_upload_state, datum_ocean_rebuild_height for a cascade without a state, datum_ocean_set_cascade with a new wavescale (under the old
 * dispersion), datum_ocean_debug_sim, and displace in the literal mode.  The value they see is the one the every-step path would hold.
 * DATUM_OCEAN_ESTATE while a profile is open (its samples are with the interval it began with; datum_ocean_profile_begin starts at the
 * beginning of an interval).  The getter reports the interval in use. */
int datum_ocean_set_phase_writeback(datum_ocean_t ctx, int every);
int datum_ocean_phase_writeback(datum_ocean_t ctx, int *every);

/* Where the module keeps the phase (added at ABI 9 without a bump; a consumer detects the two entry points by symbol).  update_ocean's
 * dispersion depends on (|y - N/2|, |x - N/2|) alone, so a phase that is a function of that index -- the zero phase of datum_ocean_create, of
 * datum_ocean_upload_state without a phase and of datum_ocean_rebuild_height, or an uploaded or resumed one that a device-side test finds
 * symmetric bit for bit -- stays one under every datum_ocean_update, whatever its dt.  AUTO (default): such a cascade's phase is kept as an
 * (N/2 + 1)^2 table and, where that holds for every cascade of the handle, none of them is outside [0, 2 pi), and neither the literal mode
 * nor the velocity plane is on, the row pass reads the table instead of the N^2 plane: the same values from a quarter of the bytes.
 * PLANE: always the plane, the behaviour of earlier builds.  Results do not depend on the mode, bit for bit, and WHAT A CALLER MAY ASSUME
 * above holds as it stands: every call that returns, copies, replaces or re-interprets the phase sees the plane it would have seen.
 * datum_ocean_resume_state now waits for the stream (it reads the test's result back).  DATUM_OCEAN_ESTATE while a profile is open.  The
 * getter reports the mode and, one bit per cascade, the cascades whose phase is a table at this moment: the next row pass reads the tables
 * if the bits of all cascades are set after the datum_ocean_displace that ran it. */
#define DATUM_OCEAN_PHASE_STORE_AUTO 0
#define DATUM_OCEAN_PHASE_STORE_PLANE 1
int datum_ocean_set_phase_store(datum_ocean_t ctx, int mode);
int datum_ocean_phase_store(datum_ocean_t ctx, int *mode, unsigned int *quadrants);

int datum_ocean_upload_state(datum_ocean_t ctx, int cascade, float const *h0, float const *phase);
int datum_ocean_read_state(datum_ocean_t ctx, int cascade, float *phase);

/* Replace the h0 of a cascade's state and keep everything else (ABI 9): the phase as advanced so far, the updates queued for it, and
 * the foam accumulator (datum_ocean_set_foam).  The same state with new wave parameters -- what lerp_ocean_waves does to
 * OceanParams::height on the host (ocean.cpp:194-211) -- where datum_ocean_upload_state would start a new one.  N*N*2 floats, host
 * pointer.  DATUM_OCEAN_ESTATE for a cascade that holds no state. */
int datum_ocean_upload_height(datum_ocean_t ctx, int cascade, float const *h0);

/* Park a cascade's state (h0 and the phase as advanced so far: 12 * N * N bytes, h0 first) in caller-owned DEVICE memory,
 * and bring a parked state back -- device to device on the handle's stream, no host round trip.  For a host object that
 * renders more states than the handle has cascades (the reference keeps every OceanParams' phase on the host and uploads
 * it per frame, ocean.cpp:748-749, so any context can render any params at any time; here the phase lives on the device).
 * Updates queued by datum_ocean_update are applied before either call.  `flags` carries what the module knows about
 * the parked phase (pass back what park returned).  bytes must be datum_ocean_state_bytes(). */
size_t datum_ocean_state_bytes(int resolution);
int datum_ocean_park_state(datum_ocean_t ctx, int cascade, void *device_dst, size_t bytes, int *flags);
int datum_ocean_resume_state(datum_ocean_t ctx, int cascade, void const *device_src, size_t bytes, int flags);

/* Device-side spectrum rebuild (what lerp_ocean_waves does on the host, ocean.cpp:194-211):
 * keep OceanParams::seed (N*N*2 floats, ocean.cpp:140-141) resident and recompute
 * h0 = seed * dk * sqrt(phillips(k, waveamplitude, windspeed, winddirection) / 2), dk = 2 pi / wavescale,
 * on the device when the wind changes, instead of an O(N^2) host loop plus an 8*N*N-byte upload.
 * rebuild_height also installs `wavescale` as the cascade's wave scale (choppiness is kept).
 * Arguments: a cascade out of range, a wavescale that is not positive, a waveamplitude that is negative or not finite, and a windspeed,
 * windx or windy that is not finite are DATUM_OCEAN_EINVAL (the error text names datum_ocean_rebuild_height); no seed on the device is
 * DATUM_OCEAN_ESTATE.  Every check comes before anything is installed: after a refused call the wave scale, h0, the phase and the launch
 * plan are as if it had not been made.  windspeed = 0 and waveamplitude = 0 are valid and give h0 = 0.  A seed never uploaded for this
 * cascade (while another's was) is zero.  What the kernel may compute at each point is stated by tests/h064.py (an interval walk of the
 * expression) and held to it by tests/test_gpu_h0.py. */
int datum_ocean_upload_seed(datum_ocean_t ctx, int cascade, float const *seed);
int datum_ocean_rebuild_height(datum_ocean_t ctx, int cascade, float wavescale, float waveamplitude, float windspeed, float windx, float windy);
int datum_ocean_read_height(datum_ocean_t ctx, int cascade, float *h0);

/* -- the per-frame path ---------------------------------------------------------------------------------- */

/* update_ocean's phase advance (ocean.cpp:223-233) for every cascade:
 * phase = fmod(phase + dispersion(k) * dt, 2 pi), in fp32, in call order.  It is applied on the device,
 * fused into the next datum_ocean_displace (bit-identical to applying each dt in turn; when the result is stored:
 * datum_ocean_set_phase_writeback). */
int datum_ocean_update(datum_ocean_t ctx, float dt);

/* ocean.sim -> ocean.fftx -> ocean.ffty -> ocean.map for every cascade (ocean.cpp:769-789), as two fused
 * kernels.  Result: per cascade [layer][y][x][4] floats, layer 0 = (dx, dy, dz, 0), layer 1 = (normal, 0)
 * (data/ocean.map.comp:79-80). */
int datum_ocean_displace(datum_ocean_t ctx);

/* ocean.gen (data/ocean.gen.comp, ocean.cpp:791-793): fills sizex*sizey Mesh::Vertex (48 bytes:
 * position3, texcoord2, normal3, tangent4 -- src/renderer/mesh.h:20-26) in DEVICE memory from the
 * cascade's displacement map.  sizex, sizey: multiples of 16 in the reference; any size >= 2 here. */
int datum_ocean_gen(datum_ocean_t ctx, int cascade, datum_ocean_set const *set, int sizex, int sizey, void *vertices_device);

/* What a rank contributes when the tiles of a multi-GPU farm are reassembled with one all-gather (SURVEY.md 8e;
 * nothing in the reference: it has one device).  Packs the displacement of every cascade of the handle into
 * caller-owned DEVICE memory, enqueued on the handle's stream behind the last displace, so that the collective can
 * read it on another stream while the next displace overwrites the maps:
 *   MAPS   the whole map block as it lies in memory, both layers (24 B per point, device layout of bind_maps)
 *   XYZ32  layer 0 only, [cascade][y][x] (dx, dy, dz) as three floats   (12 B per point, exact)
 *   XYZ16  layer 0 only, [cascade][y][x] (dx, dy, dz, 0) as four halves  (8 B per point, round to nearest) */
#define DATUM_OCEAN_PAYLOAD_MAPS 0
#define DATUM_OCEAN_PAYLOAD_XYZ32 1
#define DATUM_OCEAN_PAYLOAD_XYZ16 2
int datum_ocean_payload_bytes(datum_ocean_t ctx, int format, size_t *bytes);
int datum_ocean_pack_displacement(datum_ocean_t ctx, int format, void *payload_device, size_t bytes);

/* -- foam (ABI 9; nothing in the reference: SURVEY.md F3) ---------------------------------------------------------------------
 * Where the choppy surface pinches or folds over.  The mesh places each vertex at p - D(p), where D = (dx, dy) from map layer 0 with
 * choppiness already applied (ocean_gen.hip; reference gen.comp:122-124).  For that mapping, per texel:
 *
 *     J = (1 − a)(1 − d) − b·c
 *     a = ∂x dx,  b = ∂y dx,  c = ∂x dy,  d = ∂y dy
 *
 * each derivative a periodic central difference in world units, (f[i+1] − f[i−1]) / (2·h), h = wavescale / N the texel pitch (the map
 * covers wavescale metres: texcoord = position·scale, scale = 1/wavescale); x is the column index and y the row index, as in
 * datum_ocean_read_maps.  J < 0: the rendered mesh folds at that texel; J = 1: the surface is undisturbed.
 *
 * Modes, per handle (datum_ocean_set_foam):
 *   OFF (default)  nothing is computed or allocated; every other call behaves as without foam
 *   JACOBIAN       the plane holds J; no state
 *   ACCUMULATE     the plane holds a persistent coverage value in [0, 1]:
 *                    foam = max(clamp((threshold − J)·gain, 0, 1), foam_prev · fade),   fade = (float)exp(−(double)decay · (double)dt)
 *                  dt = the sum, in double, of the datum_ocean_update dt values queued since the previous displace (its own accumulator: it
 *                  does not depend on when queued steps are flushed); fade is computed on the host and held at 1 when that sum is negative.
 *                  Per cascade (datum_ocean_set_foam_params): threshold 0.5, gain 2, decay 1 s^-1 by default
 * STORAGE: one fp32 plane per cascade, row-major [cascade][y][x], 4 * N * N bytes -- a plain R32F image a renderer samples with the same
 * texture coordinate (and repeat addressing) as the displacement map, or imports (datum_ocean_bind_foam).  It lies beside the maps; their
 * 24-byte layout does not change, nor do the maps' values (bit for bit: the foam kernel reads them after the column pass).
 * Computed by datum_ocean_displace in every configuration (spectrum formats, literal mode, map-store policies, cascade groups, bound maps,
 * a running farm): one launch after each cascade group's column pass (after the literal dispatches in the literal mode).
 * NOT included in: the farm payloads, datum_ocean_gen, datum_ocean_export_maps, the profile's events, datum_ocean_algorithmic_bytes.
 *   set_foam         mode: allocates (own plane) and zero-fills the plane in use; OFF frees the own plane.  Drains the stream
 *   set_foam_params  EINVAL if a value is not finite or gain / decay is negative; takes effect at the next displace
 *   reset_foam       zeroes the cascade's plane (ESTATE while foam is OFF).  datum_ocean_upload_state and datum_ocean_resume_state do the
 *                    same to the cascade's accumulator in ACCUMULATE mode (a new state); datum_ocean_rebuild_height and
 *                    datum_ocean_upload_height do not (the same state with new wave parameters: lerp_ocean_waves, every frame)
 *   bind_foam        caller-owned DEVICE memory of at least cascades * N * N * 4 bytes, 16-byte aligned, becomes the plane (its contents are
 *                    the accumulator from then on: reset_foam to start from zero); NULL restores the handle's own.  Allowed in any mode
 *   foam_device      the plane in use and its bytes; ESTATE while foam is OFF
 *   read_foam        blocking read of the cascade's N * N floats (host pointer); ESTATE while foam is OFF */
#define DATUM_OCEAN_FOAM_OFF 0
#define DATUM_OCEAN_FOAM_JACOBIAN 1
#define DATUM_OCEAN_FOAM_ACCUMULATE 2
int datum_ocean_set_foam(datum_ocean_t ctx, int mode);
int datum_ocean_set_foam_params(datum_ocean_t ctx, int cascade, float threshold, float gain, float decay);
int datum_ocean_reset_foam(datum_ocean_t ctx, int cascade);
int datum_ocean_bind_foam(datum_ocean_t ctx, void *device_ptr, size_t bytes);
int datum_ocean_foam_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes);
int datum_ocean_read_foam(datum_ocean_t ctx, int cascade, float *foam);

/* -- surface queries (added at ABI 9; nothing in the reference: SURVEY.md F5) ---------------------------------------------------
 * Where is the water surface above the world point (x, y)?  For buoyancy, wakes, spray, "is the camera under water".  With choppy waves
 * the answer is not the map read at (x, y): the mesh places the vertex of base point b at P(b) − D(P(b)) horizontally (ocean_gen.hip;
 * reference gen.comp:122-124), so the water above (x, y) comes from another texel, and a plain lookup is wrong by about choppiness·|D|.
 *
 * The query uses the swell fields, `scale` (= 1/wavescale) and `plane[3]` of the set; everything else (camera, projection, smoothing) is
 * ignored.  For a base point b in the plane, with gen's own constants:
 *
 *     θ     = frequency · (swelldirection · b) + swellphase          frequency = 2π / swelllength
 *     P(b)  = b + qi · A · swelldirection · cos θ                    qi = swellsteepness / (frequency · A · 4 + 1e-6),  A = swellamplitude
 *     t     = P(b) · scale                                           texcoord; REPEAT bilinear, texel centres at (i + 0.5) / N, as gen
 *     D, m  = layer 0 (dx, dy, dz) and layer 1 (normal) of the cascade's map at t
 *     V(b)  = ( P.x − D.x,  P.y − D.y,  −plane.w + A · sin θ + D.z )   the vertex gen would place for base point b
 *
 * The query for a world point q = (qx, qy) is a fixed-point solve: start at b₀ = q, apply exactly `iterations` updates
 * b ← b + (q − V(b).xy) (no early exit: a point's result does not depend on which other points share its wave), then evaluate once more
 * at the final b.  Each point gets a record of DATUM_OCEAN_SURFACE_SAMPLE_FLOATS = 8 floats (32 bytes):
 *     0-2  V(b): the surface point found; .z is the water height above q
 *     3    residual = |V(b).xy − q|.  Large where the surface folds (J < 0 in the foam block's definition): there the surface is not a
 *          height field and no b solves the equation; also where `iterations` was too few for a steep, choppy state
 *     4-6  the unit normal: gen's tbn[2] at b with smoothing = 0, i.e. normalize(t0·m.x + t1·m.y + t2·m.z) with gen's Gerstner frame
 *          t0, t1, t2; it does not depend on the camera
 *     7    foam: the foam plane in use sampled at t with the same REPEAT bilinear fetch; 0 while foam is OFF
 * iterations = 0 is plain sampling at q (what a naive integration does; its residual shows how wrong that is).  A non-finite query
 * coordinate gives a record of quiet NaNs and fetches nothing.
 *
 *   sample_surface  enqueue and return: one kernel on the handle's stream behind the last displace; like datum_ocean_gen it applies no
 *                   pending update and reads the map as it lies (own buffer or datum_ocean_bind_maps).  points_device: `count` float2
 *                   (x, y), 8-byte aligned; samples_device: count * 32 bytes, 16-byte aligned.  DEVICE pointers
 *   read_surface    the same from HOST arrays, blocking: copies through device staging buffers the handle owns (grown on demand, freed by
 *                   datum_ocean_destroy), all on the handle's stream
 * DATUM_OCEAN_EINVAL for a null handle or set, null arrays with count > 0, a cascade out of range, iterations outside
 * [0, DATUM_OCEAN_SURFACE_MAX_ITERATIONS], misaligned arrays and count > INT32_MAX.  count == 0 enqueues nothing.  A query writes only
 * the samples: the maps and the foam plane are not touched. */
#define DATUM_OCEAN_SURFACE_SAMPLE_FLOATS 8
#define DATUM_OCEAN_SURFACE_MAX_ITERATIONS 16
int datum_ocean_sample_surface(datum_ocean_t ctx, int cascade, datum_ocean_set const *set, int iterations,
                               void const *points_device, size_t count, void *samples_device);
int datum_ocean_read_surface(datum_ocean_t ctx, int cascade, datum_ocean_set const *set, int iterations,
                             float const *points, size_t count, float *samples);

/* -- several cascades at once (added at ABI 9; nothing in the reference, whose example samples one cascade) ------------------------
 * A cascaded ocean is a few grids of different wavescale SUMMED at every vertex.  These calls are datum_ocean_gen and the surface queries
 * for that sum: one call gives the mesh of the summed surface, one call the height, normal and foam of the same surface above world points.
 * (Four gen launches added up by the caller repeat the ray stage and write 4 x 48 bytes per vertex; the queries cannot be added up at all:
 * the fixed-point solve V(b).xy = q is not additive over cascades.)
 *
 * All cascades of a handle share N.  A blend is a list cascades[count], 1 <= count <= DATUM_OCEAN_MAX_CASCADES, every entry in
 * [0, cascades of the handle); a cascade may be listed again and is then summed again.  Cascade c is sampled with the scale the HANDLE holds
 * for it, scale_c = 1 / wavescale as set by datum_ocean_set_cascade or datum_ocean_rebuild_height; set->scale is ignored.  Every other
 * field of the set means what it means to datum_ocean_gen and to the single-cascade query.
 *
 * For a position P (gen's position.xy after the swell; the query's P(b)) each listed cascade contributes, in list order:
 *
 *     t_c      = P.xy · scale_c
 *     D_c, m_c = layer 0 (dx, dy, dz) and layer 1 (normal) of cascade c at t_c: gen's REPEAT bilinear fetch -- the same weights, fract wrap
 *                and blend order, zero-weight corners pushed out of the buffer
 *     D        = D_c of the first listed cascade as it is; each further D_c added in list order, one fp32 addition per component.  A
 *                one-element list therefore gives the single-cascade call's bits (with set->scale = scale_c)
 *     p_c      = ( m_c.x / m_c.z,  m_c.y / m_c.z )          the map stores m = normalize(l.z − r.z, b.z − t.z, 4·wavescale/N), so
 *                m.x / m.z = −½ ∂z/∂x in world units for every cascade: SLOPES add, unit normals do not.  m_c.z > 0 in every texel
 *     p        = Σ p_c  in list order
 *     dn       = normalize(p.x, p.y, 1)
 *
 * dn takes the place of gen's displacementnormal in gen's shading (gen.comp:101-120); in the query it feeds
 * normalize(t0·dn.x + t1·dn.y + t2·dn.z).  The mesh vertex is gen's with D and dn as above; texcoord stays 0.1 · position.xy.  The query
 * record stays DATUM_OCEAN_SURFACE_SAMPLE_FLOATS = 8 floats with the same meaning:
 *
 *     V(b)  = ( P.x − D.x,  P.y − D.y,  −plane.w + A · sin θ + D.z )
 *
 * with exactly `iterations` updates b ← b + (q − V(b).xy) and no early exit.  The iteration converges where the SUMMED surface is a height
 * field (the Jacobian of P − D.xy over the list is positive); elsewhere the residual stays large, as in the single-cascade query.  A
 * non-finite q gives a record of quiet NaNs and fetches nothing.  Foam (field 7), from the listed cascades' planes sampled at t_c:
 *     DATUM_OCEAN_FOAM_ACCUMULATE   the largest sampled coverage of the list
 *     DATUM_OCEAN_FOAM_JACOBIAN     1 + Σ (J_c − 1): the Jacobian of the summed displacement to first order -- the cross terms between
 *                                   cascades (products of two cascades' gradients) are left out
 *     DATUM_OCEAN_FOAM_OFF          0
 *
 * Ordering and alignment are the single-cascade calls': every launch goes on the handle's stream behind the last displace, applies no
 * pending update and reads maps and foam planes as they lie (own buffers or bound ones).  read_surface_blend is sample_surface_blend from
 * HOST arrays, blocking, through the staging buffers datum_ocean_read_surface uses.  DATUM_OCEAN_EINVAL for a null list, count outside
 * [1, DATUM_OCEAN_MAX_CASCADES] or an entry out of range; otherwise the single-cascade calls' errors.  n == 0 enqueues nothing. */
int datum_ocean_gen_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int sizex, int sizey,
                          void *vertices_device);
int datum_ocean_sample_surface_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                     void const *points_device, size_t n, void *samples_device);
int datum_ocean_read_surface_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                   float const *points, size_t n, float *samples);

/* -- body buoyancy (added at ABI 9; nothing in the reference) ------------------------------------------------------------------------
 * Bodies floating on the summed surface: per body the net buoyant force, its torque about the body origin and a few aggregates, reduced on
 * the device from the body's hull probes.  (With the surface queries alone a caller transforms every probe, uploads 8 bytes and reads back
 * 32 bytes per probe and sums on the host; here 32 bytes per BODY come back.)
 *
 * A call takes a blend list cascades[count] -- the several-cascade calls' rules, the handle's scale_c, set->scale ignored; a one-element
 * list is the single-cascade case -- a set, an iteration count and two DEVICE arrays:
 *     probe, 16 bytes    (x, y, z, a): the body-local position in metres and the weight a, the cross-section the probe stands for in m².
 *                        The result is linear in a: fold ρ·g into it or multiply afterwards
 *     body, 64 bytes     datum_ocean_body below: rotation (row-major, local → world), position, the body's range [first, first + count)
 *                        of the probe array (ranges may share probes), and cap, the largest submersion one probe may report (the hull's
 *                        height above the probe; +inf: none)
 *
 * For probe i of body B, with R = rotation, T = position, every operation one fp32 operation as written (no contraction):
 *
 *     w.x = ((R[0]·x + R[1]·y) + R[2]·z) + T.x          w.y, w.z with rows 1, 2
 *     rec = the record of datum_ocean_sample_surface_blend for q = (w.x, w.y) with this list, set and iterations, bit for bit
 *     d   = min(max(rec.z − w.z, 0), cap)                submersion
 *     m   = a · d                                        force term, vertical (Archimedes)
 *     r   = (w.x − T.x, w.y − T.y)                       lever arm about the body origin
 *     terms: Fz = m,  τx = r.y · m,  τy = −(r.x · m),  wet = (d > 0 ? a : 0),  nx, ny, nz = m · rec.normal,  res = rec.residual
 *
 * Each body gets a record of DATUM_OCEAN_BODY_RECORD_FLOATS = 8 floats (32 bytes):
 *     Fz, τx, τy, wet, Σ m·n.x, Σ m·n.y, Σ m·n.z, max residual
 * The order of the sum is part of the definition, so that a result repeats from run to run and can be checked on a CPU: lane l (0 … 63)
 * holds one partial per field, started at +0.0f, and adds the terms of probes first + l, first + l + 64, … in increasing order; then for
 * s = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + s] for l < s; p[0] is the record.  Field 7 is the maximum (fmaxf) instead of the sum.
 * count == 0 gives eight zeros.  A body's record is eight quiet NaNs, and nothing is fetched for its bad probes, if its range is not
 * inside the probe array (first < 0, count < 0 or first + count > nprobes), if cap is a NaN, or if any probe of it has a non-finite w or a.
 * No index can fault: a body is read only for an index below nbodies, a probe only through a buffer resource laid over probes of its
 * body's range, after that range was found to lie inside the probe array.
 * A hull of more than a few thousand probes is better split into several bodies of the same pose: the records add, field 7 is their maximum.
 *
 *   reduce_bodies   enqueue and return: one kernel on the handle's stream behind the last displace; it applies no pending update and reads
 *                   maps and foam planes as they lie (own buffers or bound ones).  bodies_device: nbodies × 64 bytes; probes_device:
 *                   nprobes × 16 bytes; records_device: nbodies × 32 bytes; DEVICE pointers, 16-byte aligned
 *   read_bodies     the same from HOST arrays, blocking, through device staging buffers of its own (grown on demand, freed by
 *                   datum_ocean_destroy), all on the handle's stream
 * DATUM_OCEAN_EINVAL for what the several-cascade query refuses (list, handle, set, iterations), for a null bodies or records array with
 * nbodies > 0, a null probes array with nprobes > 0, misaligned arrays, and nbodies or nprobes above INT32_MAX.  nbodies == 0 enqueues
 * nothing.  A call writes only the records. */
#define DATUM_OCEAN_BODY_RECORD_FLOATS 8
typedef struct datum_ocean_body
{
  float rotation[9];       /*   0  row-major, body-local → world   */
  float position[3];       /*  36  the body origin in world space  */
  int32_t first;           /*  48  the body's first probe ...      */
  int32_t count;           /*  52  ... and how many                */
  float cap;               /*  56  largest submersion of one probe */
  int32_t pad;             /*  60                                  */
} datum_ocean_body;
int datum_ocean_reduce_bodies(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                              void const *bodies_device, size_t nbodies, void const *probes_device, size_t nprobes, void *records_device);
int datum_ocean_read_bodies(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                            datum_ocean_body const *bodies, size_t nbodies, float const *probes, size_t nprobes, float *records);

/* -- ray casts (added at ABI 9; nothing in the reference) -----------------------------------------------------------------------------
 * Where a segment meets the summed surface: picking, line of sight, projectiles, "is this sensor under water along its beam".  The result
 * is NOT "the intersection": it is the outcome of a fixed sequence of height evaluations, each of them the several-cascade query's, so
 * that a cast repeats from run to run and can be restated on a CPU on top of datum_ocean_read_surface_blend, bit for bit.  (With the
 * queries alone a caller spends one launch per evaluation, 8 bytes in and 32 bytes out per ray each time, with host logic in between.)
 *
 * A call takes a blend list cascades[count] -- the several-cascade calls' rules, the handle's scale_c, set->scale ignored; a one-element
 * list is the single-cascade case -- a set, the query's iteration count, steps S in [1, DATUM_OCEAN_RAY_MAX_STEPS], refine R in
 * [0, DATUM_OCEAN_RAY_MAX_REFINE] and n rays.  A ray is 32 bytes, (ox, oy, oz, tmin, dx, dy, dz, tmax); the direction need not be
 * normalised.  Every operation below is one fp32 operation as written (no contraction):
 *
 *     point(t) = ( ox + t·dx,  oy + t·dy,  oz + t·dz )
 *     rec(t)   = the record of datum_ocean_sample_surface_blend for q = point(t).xy with this list, set and iterations, bit for bit
 *                (eight NaNs where q is not finite, as there)
 *     g(t)     = point(t).z − rec(t).z
 *     below(t) = g(t) < 0                                 as written: a NaN is "not below"
 *     inv      = 1.0f / (float)S                          rounded once on the host and passed to the kernel
 *     Δ        = (tmax − tmin) · inv
 *     t_i      = tmin + (float)i · Δ   for i = 0 … S−1,   t_S = tmax
 *
 * March: side = below(t_0); take i = 1, 2, … S in order and stop at the first i with below(t_i) != side: lo = t_(i−1), hi = t_i.  If there
 * is none the ray is a MISS, lo = hi = tmax, and it is not refined.  A ray stops marching at its own bracket; its result depends on no
 * other ray.
 * Refinement, exactly R times on a bracket:
 *     mid = 0.5f · (lo + hi);   if below(mid) == side: lo = mid   else: hi = mid
 *
 * Each ray gets a record of DATUM_OCEAN_RAY_RECORD_FLOATS = 12 floats (48 bytes):
 *     0      hi, the first parameter known to lie on the other side (MISS: tmax)
 *     1      lo
 *     2      g(hi)
 *     3      the status as a float: 0 MISS, 1 ENTER (side was "not below"), 2 LEAVE (side was "below")
 *     4–11   rec(hi), the query's eight floats
 * A MISS with field 2 < 0 is a segment that lies under water throughout (as far as S samples can tell).
 * A ray is bad if any of its eight floats is not finite, if tmax < tmin, or if point(tmin) or point(tmax) is not finite: it gets twelve
 * quiet NaNs and fetches nothing.  No index can fault: a ray is read and a record written only through buffer resources laid over the rays
 * and records of the ray's own workgroup, the maps through the query's.
 *
 *   cast_rays   enqueue and return: one kernel on the handle's stream behind the last displace; it applies no pending update and reads
 *               maps and foam planes as they lie (own buffers or bound ones).  rays_device: n × 32 bytes; records_device: n × 48 bytes;
 *               DEVICE pointers, 16-byte aligned
 *   read_rays   the same from HOST arrays, blocking, through device staging buffers of its own (grown on demand, freed by
 *               datum_ocean_destroy), all on the handle's stream
 * DATUM_OCEAN_EINVAL for what the several-cascade query refuses (list, handle, set, iterations), for steps or refine out of range, a null
 * rays or records array with n > 0, misaligned arrays, and n above INT32_MAX.  n == 0 enqueues nothing.  A call writes only the records. */
#define DATUM_OCEAN_RAY_FLOATS 8
#define DATUM_OCEAN_RAY_RECORD_FLOATS 12
#define DATUM_OCEAN_RAY_MAX_STEPS 1024
#define DATUM_OCEAN_RAY_MAX_REFINE 24
#define DATUM_OCEAN_RAY_MISS 0
#define DATUM_OCEAN_RAY_ENTER 1
#define DATUM_OCEAN_RAY_LEAVE 2
int datum_ocean_cast_rays(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                          void const *rays_device, size_t n, void *records_device);
int datum_ocean_read_rays(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                          float const *rays, size_t n, float *records);

/* -- surface bounds per cascade, and ray casts that skip known air (added at ABI 9; nothing in the reference) ---------------------------
 * How high and how low can the water be right now, and how far can a vertex move sideways?  For frustum culling, the near plane, the
 * mesh's bounding box -- without datum_ocean_read_maps' 32 bytes per texel over the bus -- and for ray casts, whose march samples far
 * above the highest crest need no height evaluation to be known as "not below".
 *
 * Per cascade a record of DATUM_OCEAN_BOUNDS_RECORD_FLOATS = 8 floats (32 bytes):
 *     0, 1   zmin, zmax     2, 3   xmin, xmax     4, 5   ymin, ymax     6   nonfinite     7   0
 * the extrema over all N² texels of dz, dx, dy of map layer 0 AS STORED (the choppiness is in dx, dy), combined with fminf / fmaxf from
 * +inf / −inf: a NaN enters no extremum, an infinity does.  nonfinite is the number of texels with a non-finite dx, dy or dz.  The
 * extrema are exact and do not depend on the order of the reduction, but for the sign of a zero: compare them by value.
 *
 * The slab of a blend list cascades[count] under a set, each line one fp32 operation as written, sums taken in list order from the
 * parenthesised start (basez = −plane.w; A = swellamplitude; gx, gy = the Gerstner terms (qi·A)·swelldirection of the queries):
 *
 *     mag  = (|basez| + |A|) + Σ_c max(|zmin_c|, |zmax_c|)
 *     pad  = mag · 2^-16
 *     zhi  = ((basez + |A|) + Σ_c zmax_c) + pad
 *     zlo  = ((basez − |A|) + Σ_c zmin_c) − pad
 *     reach.x = |gx| + Σ_c max(|xmin_c|, |xmax_c|)         reach.y likewise
 *
 * Every height datum_ocean_sample_surface_blend can give for that list and set lies strictly between zlo and zhi, and its record's
 * position within reach of the point it was evaluated at.  pad is a stated margin, about 256 ulp of the magnitudes involved, for the
 * phase's sine (≤ 1 + 5e-7), the blend weights' sum and one rounding per cascade sum.  If a listed cascade has nonfinite > 0,
 * zlo = zhi = NaN: the slab then says nothing.
 *
 * The bounded cast is datum_ocean_cast_rays with
 *     below'(t) = point(t).z > zhi ? false : point(t).z < zlo ? true : below(t)
 * on every sample whose point(t).xy is finite: the first two cases evaluate no height.  A NaN point(t).z or a NaN bound makes both
 * comparisons false, and the sample is evaluated as in cast_rays.
 *
 *   reduce_bounds       enqueue and return: two launches on the handle's stream behind the last displace; reads the maps as they lie (own
 *                       buffer or a bound one) and applies no pending update.  The handle then holds the records and marks them CURRENT;
 *                       datum_ocean_displace and datum_ocean_bind_maps clear that mark, and so does a datum_ocean_release_memory that
 *                       unbinds the maps (a map buffer bound inside the released block: the handle's own maps are in use again, as
 *                       after bind_maps(NULL)); no other call does (datum_ocean_bind_foam leaves it: the records read no foam plane)
 *   bounds_device       the records on the device, cascades × 32 bytes, handle-owned (allocated by the first reduce, freed by
 *                       datum_ocean_destroy); DATUM_OCEAN_ESTATE before the first reduce.  Ordered on the handle's stream
 *   read_bounds         reduce_bounds, then a blocking read of cascades × 8 floats
 *   surface_slab        blocking: read_bounds, then the slab above on the host.  Any of the four outputs may be NULL
 *   cast_rays_bounded, read_rays_bounded
 *                       cast_rays' and read_rays' arguments, rules and DATUM_OCEAN_EINVAL cases.  DATUM_OCEAN_ESTATE unless the records
 *                       are current: a bounded cast that returns DATUM_OCEAN_OK has therefore written datum_ocean_cast_rays' records
 *                       BIT FOR BIT, all twelve floats of every ray.  A caller who writes into a bound map buffer behind the module's
 *                       back (datum_ocean_device_write, a kernel of its own) without a new reduce_bounds forfeits that guarantee.
 * When to use which: the bounded cast gains where march samples lie outside the slab -- a camera fan from above, long rays through air or
 * deep water.  Measured (tools/bounds_bench.py, 10^6 rays, 1024^2 maps, lists of 1 and 4): 0.57-0.60 of cast_rays' time
 * on the camera fan and 0.64 on the random set, whose rays start 0.5 to 4 m from the level and so mostly outside the slab as well; no
 * measured set was slower.  Rays that start and end inside the slab evaluate every sample either way and pay the comparisons and the
 * slab on top (not measured as a set of their own): for those datum_ocean_cast_rays is the call to prefer. */
#define DATUM_OCEAN_BOUNDS_RECORD_FLOATS 8
int datum_ocean_reduce_bounds(datum_ocean_t ctx);
int datum_ocean_bounds_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes);
int datum_ocean_read_bounds(datum_ocean_t ctx, float *records);
int datum_ocean_surface_slab(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, float *zlo, float *zhi, float *reachx, float *reachy);
int datum_ocean_cast_rays_bounded(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                  void const *rays_device, size_t n, void *records_device);
int datum_ocean_read_rays_bounded(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                  float const *rays, size_t n, float *records);

/* -- surface velocity (added at ABI 9; nothing in the reference) ------------------------------------------------------------------------
 * How is the water moving?  For drag and slamming forces on floating bodies, drift of debris and spray, foam advection, a renderer's
 * motion vectors.  The maps are overwritten every step and the difference of two steps cancels to noise in fp32 at a small dt; but the
 * maps are a linear function of h0 e^{i phase} with d phase / dt = omega(k), so the exact time derivative is one more spectrum and one
 * more pair of transforms.  In the notation of oracle/ocean_oracle.cpp: sim_rows / map_rows, with a = h0[k], m = h0[(N-1-y, N-1-x)],
 * phase = the phase the step's maps were formed from, omega = the value update_ocean advances that texel's phase by per second (the
 * handle's dispersion table) and k^ as in sim:
 *
 *     ht.re = omega · ( −(a.x + m.x) sin phase − (a.y + m.y) cos phase )
 *     ht.im = omega · (  (a.x − m.x) cos phase − (a.y − m.y) sin phase )        (= omega · d/d phase of sim's h)
 *     htx   = ( ht.im k^x, −ht.re k^x ),   hty = ( ht.im k^y, −ht.re k^y )
 *     vz = Re T(ht)·sigma,   vx = Re T(htx)·sigma·choppiness,   vy = Re T(hty)·sigma·choppiness
 *
 * T is the step's own 2-D transform, sigma = (−1)^(x+y).  (vx, vy, vz) is d/dt of map layer 0's (dx, dy, dz) at a fixed texel, in metres
 * per second where dt is in seconds.  THE SWELL IS NOT INCLUDED: the swell term of datum_ocean_gen is the caller's -- swellphase is a field
 * of the set the module does not advance -- and so is its time derivative.
 *
 * Modes, per handle (datum_ocean_set_velocity): OFF (default) -- nothing is computed or allocated, every other call behaves as without
 * velocity; ON -- datum_ocean_displace writes the plane.
 * STORAGE: one plane per cascade, row-major [cascade][y][x] of float4 (vx, vy, vz, 0), 16 * N * N bytes -- a plain RGBA32F image a renderer
 * samples with the displacement map's texture coordinate (and repeat addressing), or imports (datum_ocean_bind_velocity).  The plain
 * layout at every N, not the maps' patches.
 * Computed by datum_ocean_displace in every configuration (spectrum formats, literal mode, map-store policies, cascade groups, phase
 * write-back intervals, bound maps): two launches (columns, then rows) after each cascade group's column pass and foam launch (after the literal dispatches in
 * the literal mode).  They read the fp32 h0, the phase and the dispersion table whatever the spectrum format, and a work buffer of their own
 * (24 * N * N bytes per cascade of a group).  Maps, phase and foam are bit for bit those of a handle with velocity off, and the plane does
 * not depend on the write-back interval: where the step's row pass did not store the phase, the velocity column pass applies the same dt's
 * to the stored value by the same operations and stores nothing.
 * NOT included in: the farm payloads, datum_ocean_gen, datum_ocean_export_maps, the profile's events, datum_ocean_algorithmic_bytes.
 *   set_velocity            mode: ON allocates the own plane (zero-filled) and the work buffer; OFF frees both.  Drains the stream
 *   bind_velocity           caller-owned DEVICE memory of at least cascades * N * N * 16 bytes, 16-byte aligned, becomes the plane; NULL
 *                           restores the handle's own.  Allowed in any mode
 *   velocity_device         the plane in use and its bytes; ESTATE while velocity is OFF
 *   read_velocity           blocking read of the cascade's N * N * 4 floats (host pointer)
 *   sample_velocity_blend   datum_ocean_sample_surface_blend's arguments and rules (list, set, iterations, alignment, ordering; the
 *                           handle's scale_c).  Each point gets a record of DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS = 8 floats (32 bytes):
 *                             0-3  datum_ocean_sample_surface_blend's V(b) and residual, bit for bit
 *                             4-6  the sum over the list of the REPEAT bilinear sample of cascade c's velocity plane at t_c: the same weights,
 *                                  fract wrap and blend order; added in list order, the first cascade taken as it is
 *                             7    0
 *                           A non-finite q gives a record of quiet NaNs and fetches nothing
 *   read_velocity_blend     the same from HOST arrays, blocking, through the staging buffers datum_ocean_read_surface uses
 * Inside the module the plane has two consumers: body drag (datum_ocean_reduce_body_drag, below) turns these records into a force and a
 * torque per body on the device, and body stepping (datum_ocean_step_bodies, below it) moves the bodies with them.
 * DATUM_OCEAN_ESTATE from read_velocity and the two queries while velocity is OFF, and while no datum_ocean_displace has run since velocity
 * was switched on (the plane holds nothing yet); otherwise the foam calls' and the several-cascade query's errors. */
#define DATUM_OCEAN_VELOCITY_OFF 0
#define DATUM_OCEAN_VELOCITY_ON 1
#define DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS 8
int datum_ocean_set_velocity(datum_ocean_t ctx, int mode);
int datum_ocean_bind_velocity(datum_ocean_t ctx, void *device_ptr, size_t bytes);
int datum_ocean_velocity_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes);
int datum_ocean_read_velocity(datum_ocean_t ctx, int cascade, float *vel);
int datum_ocean_sample_velocity_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                      void const *points_device, size_t n, void *out_device);
int datum_ocean_read_velocity_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                    float const *points, size_t n, float *out);

/* -- body drag (added at ABI 9; nothing in the reference) ------------------------------------------------------------------------------
 * The other half of body buoyancy: per body the force and the torque about the body origin that the water's motion relative to the hull
 * exerts, reduced on the device from the same hull probes.  Buoyancy alone makes a body bob for ever; with this it settles, and the waves
 * push it along.  (With the velocity query alone a caller transforms every probe, uploads 8 bytes and reads back 32 bytes per probe, and
 * forms and sums k · (water − hull) on the host; here 32 bytes per BODY come back.)
 *
 * A call takes datum_ocean_reduce_bodies' arguments -- list, set, iterations, bodies, probes; their rules and layouts are those of "body
 * buoyancy" above -- and one more DEVICE array, motions, one datum_ocean_body_motion per body, 32 bytes, below: the velocity v = linear
 * of the body origin and the angular velocity ω = angular, both in world space, and two drag coefficients cl, cq.
 *
 * For probe i of body B, with R = rotation, T = position, every line one fp32 operation per operator as written (no contraction):
 *
 *     w   = body buoyancy's w (R, T and the probe's x, y, z), bit for bit
 *     rec = the record of datum_ocean_sample_velocity_blend for q = (w.x, w.y) with this list, set and iterations, bit for bit
 *     d   = min(max(rec[2] − w.z, 0), cap)         m = a · d                 body buoyancy's d and m
 *     r   = (w.x − T.x, w.y − T.y, w.z − T.z)                                lever arm about the body origin
 *     u.x = v.x + (ω.y·r.z − ω.z·r.y)   u.y = v.y + (ω.z·r.x − ω.x·r.z)   u.z = v.z + (ω.x·r.y − ω.y·r.x)      the hull's velocity at the probe
 *     e   = (rec[4] − u.x, rec[5] − u.y, rec[6] − u.z)                       the water relative to the hull
 *     s   = sqrt((e.x·e.x + e.y·e.y) + e.z·e.z)                              correctly rounded (IEEE)
 *     k   = m · (cl + cq · s)
 *     f   = (k·e.x, k·e.y, k·e.z)
 *     τx  = r.y·f.z − r.z·f.y     τy = r.z·f.x − r.x·f.z     τz = r.x·f.y − r.y·f.x
 *
 * Each body gets a record of DATUM_OCEAN_DRAG_RECORD_FLOATS = 8 floats (32 bytes):
 *     Fx, Fy, Fz, τx, τy, τz, Σ m, max residual
 * summed in body buoyancy's order by the same functions: lane l adds the terms of probes first + l, first + l + 64, … to partials started
 * at +0.0f, then the tree s = 32 … 1; field 7 is the maximum (fmaxf) of rec[3].  field 6 is datum_ocean_reduce_bodies' field 0 for the
 * same arguments, bit for bit: fold ρ (and the drag's own constants) into a or into cl, cq exactly as ρ·g for buoyancy -- the result is
 * linear in a, cl and cq together -- and check the wiring of a new caller with that field.  The weight of a probe is m, its submerged
 * volume, not a wet / dry switch: the force is continuous where a probe crosses the water line and grows with the draught, as the
 * buoyancy does.  count == 0 gives eight zeros.  A body's record is eight quiet NaNs, and nothing is fetched for its bad probes, where
 * datum_ocean_reduce_bodies says so (range, cap, a non-finite w or a) and where any of the motion's eight floats is not finite.  Huge
 * finite inputs follow the arithmetic as written: an s that overflows gives what fp32 gives.
 * THE SWELL IS NOT INCLUDED ("surface velocity" above: the velocity plane does not hold the swell's motion, so neither does e); a caller
 * who moves the swell adds its orbital velocity to `linear` with the opposite sign, or accepts the difference.
 *
 *   reduce_body_drag   enqueue and return: one kernel on the handle's stream behind the last displace; it applies no pending update and
 *                      reads maps and velocity planes as they lie (own or bound).  motions_device: nbodies × 32 bytes, a DEVICE pointer,
 *                      16-byte aligned; the other arrays as for reduce_bodies; records_device: nbodies × 32 bytes
 *   read_body_drag     the same from HOST arrays, blocking, through device staging buffers (those of read_bodies and one for the motions,
 *                      grown on demand, freed by datum_ocean_destroy), all on the handle's stream
 * DATUM_OCEAN_ESTATE exactly where datum_ocean_sample_velocity_blend returns it: while velocity is OFF, and while no datum_ocean_displace
 * has run since velocity was switched on or a plane was bound.  DATUM_OCEAN_EINVAL for everything datum_ocean_reduce_bodies refuses, and
 * for a null or misaligned motions array with nbodies > 0.  nbodies == 0 enqueues nothing.  A call writes only the records. */
#define DATUM_OCEAN_DRAG_RECORD_FLOATS 8
typedef struct datum_ocean_body_motion
{
  float linear[3];         /*   0  velocity of the body origin, world space, m/s */
  float angular[3];        /*  12  angular velocity, world space, rad/s          */
  float cl;                /*  24  linear drag coefficient                       */
  float cq;                /*  28  quadratic drag coefficient                    */
} datum_ocean_body_motion;
int datum_ocean_reduce_body_drag(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                 void const *bodies_device, void const *motions_device, size_t nbodies, void const *probes_device, size_t nprobes,
                                 void *records_device);
int datum_ocean_read_body_drag(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                               datum_ocean_body const *bodies, datum_ocean_body_motion const *motions, size_t nbodies, float const *probes, size_t nprobes,
                               float *records);

/* -- body stepping (added at ABI 9; nothing in the reference) --------------------------------------------------------------------------
 * What body buoyancy and body drag are for: one call advances every body's pose and motion by dt on the device, in `substeps` sub-steps
 * against the surface as it lies (a stiff buoyancy spring needs sub-steps; the water does not move between them).  Without it a caller
 * launches datum_ocean_reduce_bodies and datum_ocean_reduce_body_drag -- which solve the same query for every probe twice -- reads 2 × 32
 * bytes per body back, integrates on the host and uploads 64 + 32 bytes per body, per sub-step.  Here pose and motion stay in registers
 * from sub-step to sub-step, a sub-step makes one query per probe, and memory is written once at the end.
 *
 * A call takes datum_ocean_reduce_body_drag's arguments -- list, set, iterations, bodies, motions, probes; their rules and layouts are those
 * of "body buoyancy" and "body drag" above; bodies and motions are read AND written -- one more DEVICE array, props, one
 * datum_ocean_body_props per body, 32 bytes, below, and dt and substeps.  The body origin is the centre of mass: torques are about it, as in
 * both calls above.
 *
 *     inv = 1.0f / (float)substeps        h = dt · inv        both rounded once, on the host; every sub-step has the length h
 *
 * One sub-step, with R, T the body's pose, v, ω, cl, cq its motion; every operator one fp32 operation as written (no contraction), division
 * and sqrt the correctly rounded ones (IEEE):
 *
 *   1 the probe walk is body buoyancy's: the same lanes, probe order, partials started at +0.0f and tree s = 32 … 1.  Per probe ONE record
 *     rec of datum_ocean_sample_velocity_blend (its fields 0-3 are the surface record's, bit for bit); from it body buoyancy's terms 0-2 and
 *     body drag's terms 0-5 and 7: ten sums
 *         M = Σ m     bx = Σ r.y·m     by = Σ −(r.x·m)     D = (Fx, Fy, Fz, τx, τy, τz) of the drag     res = max rec[3]
 *     each of them, bit for bit, the field of datum_ocean_reduce_bodies (0-2) or datum_ocean_reduce_body_drag (0-5, 7) for the same pose,
 *     motion and arguments (the drag's field 6 is M)
 *   2 totals     F = (D.Fx, D.Fy, buoyancy·M + D.Fz)          τ = (buoyancy·bx + D.τx, buoyancy·by + D.τy, D.τz)
 *   3 linear     v'.x = v.x + h·(F.x·invmass)     v'.y likewise     v'.z = v.z + h·(F.z·invmass − gravity)
 *                T' = T + h·v'  per component                 semi-implicit Euler: the pose moves with the NEW velocity
 *   4 angular    τb_j = (R[j]·τ.x + R[3+j]·τ.y) + R[6+j]·τ.z          the torque in the body frame, j = 0, 1, 2
 *                αb_j = τb_j · invinertia[j]
 *                α.x = (R[0]·αb_0 + R[1]·αb_1) + R[2]·αb_2          α.y, α.z with rows 1, 2 (body buoyancy's w without T)
 *                ω' = ω + h·α  per component
 *                THE GYROSCOPIC TERM ω × Iω IS LEFT OUT: exact for a body whose three moments are equal, and for any body turning about
 *                one principal axis; a small error at the spin rates floating bodies reach
 *   5 rotation   c_j = (R[j], R[3+j], R[6+j]) the columns of R;  for j = 0, 1:
 *                c_j'.x = c_j.x + h·(ω'.y·c_j.z − ω'.z·c_j.y)   c_j'.y = c_j.y + h·(ω'.z·c_j.x − ω'.x·c_j.z)   c_j'.z = c_j.z + h·(ω'.x·c_j.y − ω'.y·c_j.x)
 *                |a| = sqrt((a.x·a.x + a.y·a.y) + a.z·a.z)
 *                x = c_0' / |c_0'|  per component
 *                y0 = c_1' − (x·c_1')·x  per component, x·c = (x.x·c.x + x.y·c.y) + x.z·c.z
 *                y = y0 / |y0|
 *                z = x × y:  z.x = x.y·y.z − x.z·y.y    z.y = x.z·y.x − x.x·y.z    z.z = x.x·y.y − x.y·y.x
 *                R' has the columns x, y, z
 *
 * Each body gets a record of DATUM_OCEAN_STEP_RECORD_FLOATS = 8 floats (32 bytes):
 *     F.x, F.y, F.z, τ.x, τ.y, τ.z, M -- of the LAST sub-step -- and the largest res over all sub-steps
 * A body is bad if datum_ocean_reduce_body_drag would call it bad for the pose and motion of any sub-step (range, cap, a non-finite w or a,
 * the motion), if one of the props' six fields is not finite, or if any float of the integrated pose or motion of any sub-step is not
 * finite (a column that the rotation step shrinks to length zero ends there).  A bad body's pose and motion in memory are left exactly as
 * they were, its record is eight quiet NaNs, and it walks no further sub-step.  Bodies and motions are written only after the last sub-step.
 * No index can fault, by body buoyancy's means; probe ranges may be shared between bodies, body and motion slots are a body's own.
 * Huge finite inputs and a negative dt follow the arithmetic as written.
 * THE SWELL IS NOT INCLUDED, as in body drag.  Added mass, wave radiation and collisions between bodies are not modelled.
 *
 *   step_bodies        enqueue and return: one kernel on the handle's stream behind the last displace; it applies no pending update and
 *                      reads maps and velocity planes as they lie (own or bound).  bodies_device: nbodies × 64 bytes, motions_device and
 *                      props_device: nbodies × 32 bytes, records_device: nbodies × 32 bytes; DEVICE pointers, 16-byte aligned.  It writes
 *                      only bodies (their rotation and position), motions and records
 *   step_bodies_host   the same from HOST arrays, blocking, through device staging buffers (those of read_body_drag and one for the
 *                      props, grown on demand, freed by datum_ocean_destroy), all on the handle's stream; bodies and motions are copied back
 * DATUM_OCEAN_ESTATE exactly where datum_ocean_reduce_body_drag returns it.  DATUM_OCEAN_EINVAL for everything that call refuses, for a
 * null or misaligned props array with nbodies > 0, for substeps outside [1, DATUM_OCEAN_STEP_MAX_SUBSTEPS] and for a non-finite dt.
 * nbodies == 0 enqueues nothing. */
#define DATUM_OCEAN_STEP_RECORD_FLOATS 8
#define DATUM_OCEAN_STEP_MAX_SUBSTEPS 16
typedef struct datum_ocean_body_props
{
  float invmass;           /*   0  1 / mass; 0: the body is not accelerated linearly                   */
  float invinertia[3];     /*   4  1 / principal moments, BODY frame (diagonal); 0: no spin-up         */
  float gravity;           /*  16  m/s², subtracted from the vertical acceleration as written          */
  float buoyancy;          /*  20  ρ·g: multiplies the Archimedes sums (the drag's ρ goes into cl, cq) */
  float pad[2];            /*  24                                                                      */
} datum_ocean_body_props;
int datum_ocean_step_bodies(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                            void *bodies_device, void *motions_device, void const *props_device, size_t nbodies, void const *probes_device, size_t nprobes,
                            float dt, int substeps, void *records_device);
int datum_ocean_step_bodies_host(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                 datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, size_t nbodies,
                                 float const *probes, size_t nprobes, float dt, int substeps, float *records);

/* -- ripple layer (added at ABI 9; nothing in the reference) ----------------------------------------------------------------------------
 * Everything above couples one way: the water moves the bodies.  The FFT surface is periodic and statistical and cannot carry a local
 * disturbance, so a wake, the rings round a bobbing crate or an impact live in a second, LOCAL layer: a small height field centred on the
 * camera or the action that obeys a damped wave equation, takes sources from bodies and impulses, scrolls with its centre, and is added to
 * the FFT surface by the renderer's shader, the way the foam plane is.  Off by default: while it is off nothing is
 * allocated or launched, and on or off no other call's result changes by a bit.
 *
 * The layer is R x R cells of side s metres, R one of 64, 128, 256, 512, 1024.  It holds
 *     state   two buffers of R·R float2 (η, η_t): the height in metres and its rate.  A sub-step reads one and writes the other
 *     src     one plane of R·R int32: pending deposits, in units of 2^-20 m of height
 * World cell (I, J) = (floor(x·invs), floor(y·invs)) lives at memory index (J mod R)·R + (I mod R), mod the floor one: a torus in memory.
 * invs = 1/s is rounded once from double.  The window is the cells ox <= I < ox + R, oy <= J < oy + R for an integer origin (ox, oy).  Moving
 * the window changes the origin and zeroes the cells that entered (both state buffers and src); no cell is copied.  Everything outside the
 * window is water at rest, η = 0.
 *
 * THE STEP.  step_ripples(dt, substeps) runs `substeps` sub-steps (1 .. DATUM_OCEAN_RIPPLE_MAX_SUBSTEPS) of
 *     inv = 1.0f / (float)substeps        h = dt · inv        both rounded once, on the host
 * Per window cell and sub-step, every operator one fp32 operation as written (no contraction):
 *     e   = η                       in the step's FIRST sub-step   e = η + (float)src · 2^-20   -- for the cell and for every neighbour it reads
 *     lap = ((eL + eR) + (eD + eU)) − 4·e         L, R the cells I − 1, I + 1; D, U the cells J − 1, J + 1; a neighbour outside the window is 0
 *     v1  = (η_t + h · (c2s2 · lap)) · f[k]       c2s2 = c²/s², rounded once on the host from double
 *     e1  = e + h · v1                            the new cell is (e1, v1)
 * the project's semi-implicit Euler: the rate first, the height with the new rate.  k = max(0, B − min(distance of the cell to the window's four
 * edges, in cells)) is the sponge index (the outermost ring has k = B) and f[k] = 1 / (1 + h (γ + γe (k/B)²)) for k = 0 .. B, built on the host
 * in double and rounded once; B = sponge_cells <= DATUM_OCEAN_RIPPLE_MAX_SPONGE, and with B = 0 there is no sponge and f[0] serves every cell.
 * dt = 0 is legal (the pending deposits become heights and nothing else moves); dt < 0 or not finite is DATUM_OCEAN_EINVAL: the damping would
 * grow.  After the first sub-step src is zero again.  The scheme is stable for c·h/s <= 1/√2; the call refuses c·h/s > 0.7 (that bound with a
 * margin) with DATUM_OCEAN_EINVAL, computed in double from c, s, dt and substeps.  Defaults: c = 2 m/s, γ = 0.05 1/s (as a float, like every value datum_ocean_set_ripple_params stores), B = 8, γe = 4 1/s.
 *
 * DEPOSITS are integers, so that a plane repeats bit for bit whatever the order of the atomics.  For a volume V m³ at (x, y):
 *     Q   = rint((V · (invs·invs)) · 2^20) clamped to ±2^30        rint to nearest, ties to even; Q = 0 deposits nothing
 *     u   = x·invs − 0.5     I0 = floor(u)     wx = u − I0         cell centres stand at (I + ½)·s; y, J0, wy likewise
 *     w00 = (1 − wx)·(1 − wy)     w10 = wx·(1 − wy)     w01 = (1 − wx)·wy
 *     q00 = rint((float)Q·w00)   q10 = rint((float)Q·w10)   q01 = rint((float)Q·w01)   q11 = Q − ((q00 + q10) + q01)
 * quantum q_ab goes to cell (I0 + a, J0 + b) with an atomic add on src: the plane's sum changes by Q exactly.  A quantum whose cell lies
 * outside the window is dropped.  A non-finite x, y or V, or |x·invs| or |y·invs| >= 2^30, deposits nothing.
 *   deposit_ripples        n records of 16 bytes (x, y, V, 0) in a DEVICE array, 16-byte aligned, one thread per record: impacts, rain,
 *                          explosions.
 *   deposit_body_ripples   THE WAKE.  datum_ocean_reduce_body_drag's arguments and rules, DATUM_OCEAN_ESTATE exactly where that call
 *                          returns it, and dt.  With body drag's w, rec, d, m, u, e for a probe, bit for bit:
 *                              heave   if 0 < d and d < cap:  splat Vh = (a · (−e.z)) · dt at (w.x, w.y)
 *                                      a column that sinks relative to the water pushes water out; a dry or a fully submerged one displaces
 *                                      nothing more
 *                              surge   if d > 0:  splat −m at (w.x, w.y) and +m at (w.x + sx, w.y + sy),  sx = −(e.x·dt), sy = −(e.y·dt)
 *                                      the column's displaced volume moves with the hull relative to the water; the two splats cancel
 *                                      exactly where their weights agree
 *                          Each body gets a record of DATUM_OCEAN_RIPPLE_RECORD_FLOATS = 8 floats, summed in body buoyancy's order by the
 *                          same tree:  Σ Vh,  Σ m·sx,  Σ m·sy,  the count of non-zero quanta dropped,  0,  0,  Σ m,  max residual.
 *                          Field 6 is datum_ocean_reduce_bodies' field 0 bit for bit.  A bad body or motion: eight quiet NaNs and no
 *                          deposit (a body that is bad only through one bad PROBE has deposited its other probes).  THE SWELL IS NOT INCLUDED, as in body drag.  This is a KINEMATIC SOURCE, NOT A RADIATION SOLUTION: no
 *                          boundary condition is solved on the hull, whose shape enters only through its probes.
 *
 *   set_ripples          R = 0 switches the layer off and frees everything.  Otherwise R must be one of the five sizes and s finite and
 *                        positive; the new layer is at rest, its origin (−R/2, −R/2), its parameters kept.  Waits for the stream.
 *   set_ripple_params    c finite and > 0; gamma and sponge_gamma finite and >= 0; sponge_cells 0 .. DATUM_OCEAN_RIPPLE_MAX_SPONGE.  Works
 *                        while the layer is off.
 *   center_ripples       the new origin is (floor(x·invs) − R/2, floor(y·invs) − R/2); one kernel zeroes the cells that entered; a jump of R
 *                        cells or more clears the layer.  x, y finite with |x·invs|, |y·invs| < 2^30, else DATUM_OCEAN_EINVAL.
 *   reset_ripples        water at rest, no pending deposit; the origin stays.
 *   ripples_device       the CURRENT state buffer (the one the next sub-step reads), its bytes and the origin, for a renderer that binds
 *                        it.  THE POINTER ALTERNATES between the layer's two buffers with every sub-step: ask again after each step.
 *   read_ripples         the current state to the HOST in window order, [j][i][2] for cell (ox + i, oy + j); blocking.
 *   sample_ripples       per DEVICE point (8 bytes, x y) a float4 (η, ∂xη, ∂yη, η_t), 16-byte aligned: the bilinear patch between the four
 *                        cell centres around the point, in the deposit's u, I0, wx:
 *                            a0 = η10 − η00   a1 = η11 − η01   e0 = η00 + wx·a0   e1 = η01 + wx·a1
 *                            η = e0 + wy·(e1 − e0)     ∂xη = (a0 + wy·(a1 − a0))·invs     ∂yη = (e1 − e0)·invs      η_t as η
 *                        Cells outside the window read 0.  A non-finite point gives four NaNs and fetches nothing; a finite one beyond
 *                        2^30 cells gives zeros.  Pending deposits are not seen before the next step.
 *   query_ripples        the same from HOST arrays, blocking, through the surface queries' staging.
 *   deposit_ripples_host, deposit_body_ripples_host   the two deposits from HOST arrays, through device staging buffers (the surface
 *                        queries' and read_body_drag's, grown on demand), all on the handle's stream; blocking: the arrays are free and, for
 *                        the wake, the records are written when the call returns.  The same checks, kernels and bits.
 * Every call but set_ripples and set_ripple_params returns DATUM_OCEAN_ESTATE while the layer is off.  All launches and memsets go on
 * the handle's stream.  The layer is not added into the surface queries, gen_blend, the ray casts or step_bodies themselves, which keep
 * their bits; the one call that feels it is datum_ocean_step_bodies_coupled ("coupled stepping", below), and the calls that SHOW it are
 * the mesh, the query and the cast of "rippled reads" (below, behind coupled stepping). */
#define DATUM_OCEAN_RIPPLE_RECORD_FLOATS 8
#define DATUM_OCEAN_RIPPLE_MAX_SUBSTEPS 16
#define DATUM_OCEAN_RIPPLE_MAX_SPONGE 64
int datum_ocean_set_ripples(datum_ocean_t ctx, int R, float s);
int datum_ocean_set_ripple_params(datum_ocean_t ctx, float c, float gamma, int sponge_cells, float sponge_gamma);
int datum_ocean_center_ripples(datum_ocean_t ctx, float x, float y);
int datum_ocean_reset_ripples(datum_ocean_t ctx);
int datum_ocean_ripples_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes, int *ox, int *oy);
int datum_ocean_read_ripples(datum_ocean_t ctx, float *state);
int datum_ocean_step_ripples(datum_ocean_t ctx, float dt, int substeps);
int datum_ocean_deposit_ripples(datum_ocean_t ctx, void const *impulses_device, size_t n);
int datum_ocean_deposit_body_ripples(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                     void const *bodies_device, void const *motions_device, size_t nbodies, void const *probes_device, size_t nprobes,
                                     float dt, void *records_device);
int datum_ocean_deposit_ripples_host(datum_ocean_t ctx, float const *impulses, size_t n);
int datum_ocean_deposit_body_ripples_host(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                          datum_ocean_body const *bodies, datum_ocean_body_motion const *motions, size_t nbodies, float const *probes, size_t nprobes,
                                          float dt, float *records);
int datum_ocean_sample_ripples(datum_ocean_t ctx, void const *points_device, size_t n, void *out_device);
int datum_ocean_query_ripples(datum_ocean_t ctx, float const *points, size_t n, float *out);

/* -- coupled stepping (added at ABI 9; nothing in the reference) ------------------------------------------------------------------------
 * The link the chain above lacks: a body that FEELS the ripple layer.  datum_ocean_step_bodies keeps pose and motion in registers over its
 * sub-steps and reads nothing back, so a caller has no place to add sample_ripples' height; here the bodies and the layer advance together
 * by dt in `substeps` coupled sub-steps (1 .. DATUM_OCEAN_STEP_MAX_SUBSTEPS), and a boat rocks in another boat's wake.
 *
 * A call takes datum_ocean_step_bodies' arguments, with their rules and layouts.
 *
 *     inv = 1.0f / (float)substeps        h = dt · inv        both rounded once, on the host, as in both parent calls
 *
 * Per coupled sub-step, in this order:
 *   1 BODIES.  One kernel walks every body's probes exactly as datum_ocean_step_bodies does: the same lanes, probe order and tree.  Per
 *     probe at w it makes ONE velocity record rec above (w.x, w.y) (datum_ocean_sample_velocity_blend's) and ONE sample
 *     s = (η, ∂xη, ∂yη, η_t) of the layer's CURRENT state buffer at (w.x, w.y) (datum_ocean_sample_ripples'; pending deposits are not
 *     seen, cells outside the window read 0).  THE RIPPLED RECORD is
 *         rec'[2] = rec[2] + s.η          rec'[6] = rec[6] + s.η_t          one fp32 addition each; every other field is rec's
 *     From rec' it forms datum_ocean_step_bodies' ten sums and datum_ocean_deposit_body_ripples' wake with dt = h -- the deposits go onto
 *     src, and the wake's Σ Vh, Σ m·sx, Σ m·sy and dropped count are summed beside the ten: fourteen fields in the body tree's order, the
 *     tenth the maximum.  Then datum_ocean_step_bodies' steps 2-5 with h, and pose, motion and record are stored.  The wake is that of the
 *     pose and motion at the START of the sub-step, as datum_ocean_deposit_body_ripples has it.
 *   2 WATER.  One sub-step of the layer of length h in the step's FIRST form (it takes src in), src zeroed behind it, the current buffer
 *     swapped: datum_ocean_step_ripples(h, 1), with f[k] and c2s2 built from h as that call builds them.
 * The result is therefore: K rounds of the two reductions and the wake from rippled records, through the integrator, then
 * datum_ocean_step_ripples(h, 1) -- bit for bit.  Every sub-step is a launch of its own: the layer's step between two of them needs
 * the whole device.
 *
 * Each body gets a record of DATUM_OCEAN_COUPLED_RECORD_FLOATS = 12 floats (48 bytes):
 *     0-6   F.x, F.y, F.z, τ.x, τ.y, τ.z, M of the LAST sub-step          7   the largest res over all sub-steps
 *     8-10  the wake's Σ Vh, Σ m·sx, Σ m·sy of the LAST sub-step          11  the dropped quanta summed over all sub-steps
 * Fields 7 and 11 fold from launch to launch through the record in memory: fmaxf and one fp32 addition with the old record's fields.
 *
 * Bad bodies follow datum_ocean_step_bodies' rules, with two differences that the launch per sub-step brings:
 *   - a bad body's pose and motion in memory are what its LAST GOOD SUB-STEP wrote, not those from before the call;
 *   - a body that turns bad through one bad probe has deposited its other probes of that sub-step (the wake's rule), and one that
 *     turns bad only behind the integrator -- a pose or motion that is not finite -- has deposited ALL its probes of that sub-step.
 * Its record is twelve quiet NaNs; a NaN in field 0 tells the next sub-step's launch that the body went bad, and it walks nothing and
 * deposits nothing from then on.
 *
 * STABILITY OF A BODY'S OWN WAKE: IT NEEDS DRAG.  The wake is a kinematic source, and a body that feels it closes a loop the source was
 * not made for: the heave splat lowers the cell under a sinking column by (a/s²)·(sink rate relative to the water)·h, the wave
 * equation fills the hollow, and the filling flow -- water rising relative to the hull, rec'[6] -- is read by the next sub-step as the
 * hull sinking further.  tests/test_couple64.py walks a box dropped from rest through 2000 sub-steps in float64 at the layer's default
 * parameters over the grid a/s² = 0.01, 0.05, 0.25, 1: with cl = cq = 0 the heave and the total of body and layer energy GROW at every
 * ratio of the grid (by a tenth of the drop at 0.01, without bound at 1), so no ratio is stable without damping and none is promised.
 * What bounds the loop is the body's linear drag: with cl·D >= buoyancy·(a/s²) (SI numbers; D the draught, buoyancy = ρ·g) the heave
 * never exceeds the drop, decays, and the total energy never exceeds its start -- measured at 0.01, 0.05 and 0.25; at a/s² = 1 that drag
 * keeps the heave below the drop but not the energy below its start.  Give floating bodies that drag AND probes that stand for a quarter
 * of a cell or less (a/s² <= 0.25): a small ratio alone does not bound it.  Another body's wake is no loop and needs none of this.
 *
 * THE FFT SURFACE IS FROZEN within a call; the layer is not.  THE SWELL IS NOT INCLUDED, as in body drag.  The ripple layer's other
 * calls, datum_ocean_step_bodies and every other call keep their bits.
 *
 *   step_bodies_coupled        enqueue and return: 2 kernels and a memset per sub-step on the handle's stream.  records_device: nbodies ×
 *                              48 bytes; every array a DEVICE pointer, 16-byte aligned.  It writes bodies, motions, records and the layer
 *   step_bodies_coupled_host   the same from HOST arrays, blocking, through datum_ocean_step_bodies_host's staging; bodies and motions
 *                              are copied back
 * DATUM_OCEAN_ESTATE exactly where datum_ocean_reduce_body_drag returns it, and while the layer is off.  DATUM_OCEAN_EINVAL for everything
 * datum_ocean_step_bodies refuses, for records that are not 16-byte aligned, for dt < 0 or not finite (the ripple step's rule) and for
 * c·h/s > 0.7, computed in double as in datum_ocean_step_ripples.  The layer is looked at first: while it is off the call returns
 * DATUM_OCEAN_ESTATE whatever its other arguments are (a null handle is DATUM_OCEAN_EINVAL).  A refused call enqueues nothing and
 * changes nothing.
 * nbodies == 0 still steps the water: it is datum_ocean_step_ripples(h, 1) × substeps.
 * LEFT OUT: a flag to feel the layer without depositing into it; temporal blocking of the ripple step; a several-sub-steps-per-launch
 * form.  (The layer in the surface query, gen_blend and the ray cast is no longer left out: "rippled reads", below.) */
#define DATUM_OCEAN_COUPLED_RECORD_FLOATS 12
int datum_ocean_step_bodies_coupled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                    void *bodies_device, void *motions_device, void const *props_device, size_t nbodies, void const *probes_device, size_t nprobes,
                                    float dt, int substeps, void *records_device);
int datum_ocean_step_bodies_coupled_host(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                         datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, size_t nbodies,
                                         float const *probes, size_t nprobes, float dt, int substeps, float *records);

/* -- rippled reads (added at ABI 9; nothing in the reference) ---------------------------------------------------------------------------
 * The read side of the ripple layer: the mesh, the surface query and the ray cast of the summed FFT surface WITH the layer on top -- the
 * water coupled stepping floats its bodies on, by coupled stepping's rule rec'[2] = rec[2] + s.η.  Opt-in: the parent calls
 * (datum_ocean_gen_blend, datum_ocean_sample_surface_blend, datum_ocean_cast_rays and their host twins), the ripple layer's calls and
 * datum_ocean_step_bodies_coupled keep their bits.
 *
 * Every call reads the layer's CURRENT state buffer (the one datum_ocean_ripples_device returns) and writes nothing into the layer.  As
 * in datum_ocean_sample_ripples and in coupled stepping: pending deposits are not seen; cells outside the window read 0; a coordinate
 * beyond 2^30 cells gives zeros; s = (η, ∂xη, ∂yη, η_t) is datum_ocean_sample_ripples' sample, unchanged.
 *
 * THE RIPPLED RECORD above a world point q.  rec is datum_ocean_sample_surface_blend's record (8 floats), s the layer's sample at
 * (q.x, q.y) -- the ASKED point, as coupled stepping samples at the probe's (w.x, w.y), not the solved base point b:
 *     rec'[2] = rec[2] + s.η                              one fp32 addition; fields 0, 1, 3 and 7 are rec's bits
 *     p' = (p.x + (−0.5f · s.∂xη), p.y + (−0.5f · s.∂yη))   one fp32 product and one addition per component, behind the loop over the list
 *     fields 4-6: dn = normalize(p'.x, p'.y, 1) through the same frame as the parent's
 * The layer is one more entry behind the cascade list in the map's own slope convention, m.x / m.z = −½ ∂z/∂x.  The solve
 * b ← b + (q − V(b).xy) is untouched: the layer displaces nothing horizontally.  A non-finite q gives eight quiet NaNs and fetches
 * nothing.
 *
 * THE RIPPLED HEIGHT is the parent's height + s.η, one fp32 addition: by construction the rippled record's field 2, bit for bit.
 *
 * THE RIPPLED MESH VERTEX is datum_ocean_gen_blend's vertex, with the layer sampled at the vertex's OWN horizontal position
 * (px, py) = position.xy − displacement.xy, the two floats the vertex stores:
 *     pz' = pz + s.η          in shaded waves slopex, slopey each + (−0.5f · ∂η) before dn is formed
 * A vertex whose stored x or y is not finite gets the sample's four NaNs: its z and, in a shaded wave, its normal are NaN (no ray of a
 * finite camera gives one: above the horizon gen puts the vertex 10^6 m away, which is finite).
 * Unshaded waves keep the plane normal (gen's rule).  Position x, y and the texcoord are gen_blend's bits; the tangent follows from the
 * new normal as in gen.
 *
 * THE RIPPLED CAST is datum_ocean_cast_rays with every height of the march and the bisection the rippled height, the record at hi the
 * rippled record and g taken from its field 2.
 *
 *   gen_blend_rippled                  datum_ocean_gen_blend's arguments, rules and ordering; one kernel
 *   sample_surface_blend_rippled       datum_ocean_sample_surface_blend's; one kernel
 *   read_surface_blend_rippled         datum_ocean_read_surface_blend's: HOST arrays, blocking, the queries' staging
 *   cast_rays_rippled                  datum_ocean_cast_rays'; one kernel
 *   read_rays_rippled                  datum_ocean_read_rays': HOST arrays, blocking
 * Each returns what its parent call returns for the same arguments, with its own name in the error text.  The layer is looked at first:
 * while it is off the call returns DATUM_OCEAN_ESTATE whatever its other arguments are (a null handle is DATUM_OCEAN_EINVAL).  n == 0
 * enqueues nothing.  A refused call enqueues nothing and changes nothing.
 * LEFT OUT: the layer's rate in datum_ocean_sample_velocity_blend; the layer in datum_ocean_reduce_bodies,
 * datum_ocean_reduce_body_drag and datum_ocean_step_bodies (datum_ocean_step_bodies_coupled is the call for that);
 * anything on the displace path.  (The foam from the layer is no longer left out: "wake foam", below, behind the ripple layer's bounds.) */
int datum_ocean_gen_blend_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int sizex, int sizey, void *vertices_device);
int datum_ocean_sample_surface_blend_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                             void const *points_device, size_t n, void *samples_device);
int datum_ocean_read_surface_blend_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                           float const *points, size_t n, float *samples);
int datum_ocean_cast_rays_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                  void const *rays_device, size_t n, void *records_device);
int datum_ocean_read_rays_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                  float const *rays, size_t n, float *records);

/* -- ripple-layer bounds, the rippled slab and the bounded rippled cast (added at ABI 9; nothing in the reference) -----------------------
 * How high and how low does the ripple layer stand right now, and is it at rest?  For the rippled water's bounding box, near plane and
 * culling slab, for the rippled cast's march samples far above the highest crest -- and for skipping datum_ocean_step_ripples and the
 * rippled reads altogether over a layer at rest, without datum_ocean_read_ripples' 8 bytes per cell over the bus.
 *
 * One record of DATUM_OCEAN_RIPPLE_BOUNDS_RECORD_FLOATS = 8 floats (32 bytes):
 *     0, 1   etamin, etamax     2, 3   ratemin, ratemax     4   nonfinite     5   active     6, 7   0
 * over all R² cells of the layer's CURRENT state buffer (the one datum_ocean_ripples_device returns; pending deposits are not seen, as in
 * datum_ocean_sample_ripples).  The extrema are combined with fminf / fmaxf from +inf / −inf: a NaN enters no extremum, an infinity
 * does; they are exact and do not depend on the order of the reduction, but for the sign of a zero: compare them by value.  nonfinite is
 * the number of cells with a non-finite η or rate, active the number of cells with η != 0 || rate != 0 (a NaN counts).  R² ≤ 2^20: both
 * counts are exact.  active == 0 is the test for a layer at rest: stepping it changes nothing unless deposits are pending, and the
 * rippled reads then give the parents' values.
 *
 * The rippled slab of a blend list under a set: the layer is one more entry behind the list.  It displaces nothing horizontally, and a
 * point outside the window reads 0, so 0 always lies inside the layer's interval.  With mag, hi, lo the running sums of
 * datum_ocean_surface_slab behind its loop over the list (before pad), each line one fp32 operation:
 *
 *     elo  = fminf(etamin, 0)                 ehi = fmaxf(etamax, 0)
 *     mag  = mag + fmaxf(|elo|, |ehi|)        hi  = hi + ehi             lo = lo + elo
 *     pad  = mag · 2^-16                      zhi = hi + pad             zlo = lo − pad          reach as in datum_ocean_surface_slab
 *
 * Every height datum_ocean_sample_surface_blend_rippled can give for that list, set and layer lies strictly between zlo and zhi: the
 * parent's height lies inside the parent's un-padded sums up to the parent's stated roundings, the bilinear η exceeds its four cells'
 * extrema by at most a few ulp of max |η|, the rippled height is one more rounded addition, and pad ≥ 128 ulp(mag) covers these.  If a
 * listed cascade or the layer has nonfinite > 0, zlo = zhi = NaN: the slab then says nothing.  datum_ocean_surface_slab keeps its results.
 *
 * The bounded rippled cast is datum_ocean_cast_rays_rippled with datum_ocean_cast_rays_bounded's rule over the rippled slab:
 *     below'(t) = point(t).z > zhi ? false : point(t).z < zlo ? true : below(t)
 *
 *   reduce_ripple_bounds       enqueue and return: two launches on the handle's stream.  The handle then holds the record and marks it
 *                              CURRENT.  Every call that writes a state buffer clears that mark: datum_ocean_step_ripples,
 *                              datum_ocean_step_bodies_coupled and its host twin, a datum_ocean_center_ripples that moves the window,
 *                              datum_ocean_reset_ripples and datum_ocean_set_ripples.  The deposit calls (they write only the pending
 *                              deposits), datum_ocean_set_ripple_params and every read leave it
 *   ripple_bounds_device       the record on the device, 32 bytes, handle-owned (allocated by the first reduce after a set_ripples, freed
 *                              with the layer); DATUM_OCEAN_ESTATE before that reduce.  Ordered on the handle's stream
 *   read_ripple_bounds         reduce_ripple_bounds, then a blocking read of 8 floats
 *   surface_slab_rippled       blocking: read_bounds and read_ripple_bounds (both marks are current afterwards), then the slab above on the
 *                              host.  datum_ocean_surface_slab's arguments; any of the four outputs may be NULL
 *   cast_rays_rippled_bounded, read_rays_rippled_bounded
 *                              cast_rays_rippled's and read_rays_rippled's arguments, rules and DATUM_OCEAN_EINVAL cases.
 *                              DATUM_OCEAN_ESTATE unless BOTH marks are current, the maps' (datum_ocean_reduce_bounds) and the layer's:
 *                              a call that returns DATUM_OCEAN_OK has therefore written datum_ocean_cast_rays_rippled's records BIT FOR
 *                              BIT, all twelve floats of every ray.  A caller who writes the layer's state through
 *                              datum_ocean_ripples_device's pointer behind the module's back without a new reduce_ripple_bounds forfeits
 *                              that guarantee, as one who writes into a bound map buffer does
 * The layer is looked at first: while it is off every call here returns DATUM_OCEAN_ESTATE whatever its other arguments are (a null
 * handle is DATUM_OCEAN_EINVAL).  A refused call enqueues nothing.
 * When to use which: as for the bounded cast (datum_ocean_cast_rays_bounded), the bounded rippled cast gains where march samples lie
 * outside the slab -- a camera fan from above, long rays through air or deep water.  Measured (DESIGN.md 5.23;
 * tools/ripple_bounds_bench.py, 10^6 rays, 1024^2 maps, R = 1024, lists of 1 and 4): 0.58 of datum_ocean_cast_rays_rippled's time on
 * the camera fan and 0.63-0.65 on the random set.  Rays that start and end inside the slab evaluate every sample either way and pay
 * the comparisons and the slab on top: 1.001-1.006 on such a set, for which datum_ocean_cast_rays_rippled is the call to prefer.
 * LEFT OUT: a single-launch reduction; bounds per tile of the window (a tighter slab over quiet water); a wave-uniform early-out in the
 * rippled mesh. */
#define DATUM_OCEAN_RIPPLE_BOUNDS_RECORD_FLOATS 8
int datum_ocean_reduce_ripple_bounds(datum_ocean_t ctx);
int datum_ocean_ripple_bounds_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes);
int datum_ocean_read_ripple_bounds(datum_ocean_t ctx, float *record);
int datum_ocean_surface_slab_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, float *zlo, float *zhi, float *reachx, float *reachy);
int datum_ocean_cast_rays_rippled_bounded(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                          void const *rays_device, size_t n, void *records_device);
int datum_ocean_read_rays_rippled_bounded(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                          float const *rays, size_t n, float *records);

/* -- wake foam (added at ABI 9; nothing in the reference) ---------------------------------------------------------------------------------
 * The white water of a wake.  The foam plane above ("foam") follows the periodic Jacobian of the FFT surface, which knows nothing of the
 * bodies: a boat's wake, the ring round a dropped crate and an impact leave no foam there.  This is an opt-in R x R plane of fp32
 * coverage in [0, 1] beside the ripple layer's state, on the layer's torus -- world cell (I, J) at (J mod R)·R + (I mod R) -- that scrolls
 * with the window and is updated from the layer's state by an explicit call; the renderer adds it to the FFT foam the way it adds η to
 * the height (sum, then clamp).  Off by default: while it is off nothing is allocated or launched and no call changes
 * by a bit; while it is on no other call's outputs change by a bit either -- the state buffers, src, the FFT foam plane, the maps and
 * every record keep their bits.
 *
 * THE UPDATE.  step_ripple_foam(dt), per window cell.  η_t is the cell's rate and eL, eR, eD, eU are the step's four neighbours' heights
 * in the layer's CURRENT state buffer (the one datum_ocean_ripples_device returns; pending deposits are not seen); a neighbour outside
 * the window is 0.  Every operator is one fp32 operation as written (no contraction):
 *     hx  = (eR − eL) · hinv          hinv = 0.5f · invs: the central difference over 2 s
 *     hy  = (eU − eD) · hinv
 *     q   = hx·hx + hy·hy             the slope squared (two products, one addition)
 *     g1  = (q − t1) · k1             breaking: slope² over a threshold
 *     g2  = (fabsf(η_t) − t2) · k2    churn: the rate over a threshold
 *     g   = fminf(fmaxf(fmaxf(g1, g2), 0.0f), 1.0f)
 *     new = fmaxf(g, old · fade)      fade = (float)exp(−(double)decay · (double)dt), on the host
 * FOAM_ACCUMULATE's rule with two sources.  A NaN loses every fmaxf; of two zeros of opposite sign fmaxf gives +0 here (C leaves that
 * case open, and a gain of 0 makes a −0 of every cell under its threshold: with the case decided the plane repeats bit for bit on the
 * device and on any host).  The plane stays in [0, 1].
 *
 *   set_ripple_foam          on != 0 allocates the plane (4 R² bytes) and zero-fills it, a second time as well; on == 0 frees it.  Waits for
 *                            the stream.  DATUM_OCEAN_ESTATE while the layer is off.  datum_ocean_set_ripples with any R, 0 included,
 *                            switches the foam off and frees the plane.
 *   set_ripple_foam_params   t1, k1, t2, k2, decay: all five finite, the gains k1, k2 and decay >= 0, else DATUM_OCEAN_EINVAL.  A gain of 0
 *                            switches its source off.  Works while the foam is off; kept over set_ripples and set_ripple_foam.  The
 *                            defaults are DESIGN CHOICES, NOT MEASUREMENTS: t1 = 0.04 (a slope of 0.2), k1 = 10, t2 = 0.5 m/s, k2 = 2,
 *                            decay = 0.5 1/s.
 *   step_ripple_foam         enqueues one launch on the handle's stream and returns.  dt < 0 or not finite is DATUM_OCEAN_EINVAL; dt = 0 is
 *                            legal and gives fade = 1.  It writes the plane only.
 *   reset_ripple_foam        no foam anywhere; one memset on the handle's stream.
 *   ripple_foam_device       the plane, its bytes and the layer's origin, for a renderer that binds it.  The pointer does not alternate:
 *                            it holds from one set_ripple_foam to the next (or to the next set_ripples).
 *   read_ripple_foam         the plane to the HOST in window order, [j][i] for cell (ox + i, oy + j); blocking.
 *   sample_ripple_foam       per DEVICE point (8 bytes, x y) one float, 4-byte aligned: the bilinear patch between the four cell centres
 *                            around the point, in the deposit's u, I0, wx:
 *                                f0 = f00 + wx·(f10 − f00)     f1 = f01 + wx·(f11 − f01)     f = f0 + wy·(f1 − f0)
 *                            Cells outside the window read 0.  A non-finite point gives NaN and fetches nothing; a finite one beyond
 *                            2^30 cells gives 0.
 *   query_ripple_foam        the same from HOST arrays, blocking, through the surface queries' staging, as datum_ocean_query_ripples.
 * While the foam is on, datum_ocean_center_ripples also zeroes the plane's cells that entered the window (one more launch; a jump of R
 * cells or more clears the plane) and datum_ocean_reset_ripples also clears the plane.
 * Every call but the two setters returns DATUM_OCEAN_ESTATE while the layer or the foam is off.  The layer is looked at first.  A null
 * handle is DATUM_OCEAN_EINVAL, with the call's name in the error text.  n == 0 enqueues nothing.  A refused call enqueues nothing.
 * LEFT OUT: fusing the update into the last ripple sub-step (it would read the state the step has in registers, and change the step's
 * device code); advection of the foam by the water's velocity; a direct source from src, that is, hull churn before it becomes a wave;
 * wake foam as field 7 of the rippled query's record; a bounds/`active` record for the plane. */
int datum_ocean_set_ripple_foam(datum_ocean_t ctx, int on);
int datum_ocean_set_ripple_foam_params(datum_ocean_t ctx, float t1, float k1, float t2, float k2, float decay);
int datum_ocean_step_ripple_foam(datum_ocean_t ctx, float dt);
int datum_ocean_reset_ripple_foam(datum_ocean_t ctx);
int datum_ocean_ripple_foam_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes, int *ox, int *oy);
int datum_ocean_read_ripple_foam(datum_ocean_t ctx, float *plane);
int datum_ocean_sample_ripple_foam(datum_ocean_t ctx, void const *points_device, size_t n, void *out_device);
int datum_ocean_query_ripple_foam(datum_ocean_t ctx, float const *points, size_t n, float *out);

/* -- dispersive ripples (added at ABI 9; nothing in the reference) ---------------------------------------------------------------------------
 * The ripple layer's step is the plain wave equation: c is one speed for every wavelength.  A boat at speed U then drags a Mach cone of
 * half-angle asin(c/U) and at U < c has no wake pattern at all.  Deep water has ω² = g·|k|: the Kelvin wedge of 19.47° whatever the speed
 * (here: while the wake's waves stay shorter than about 14 cells, see BELOW),
 * long waves outrunning short ones in the ring round a dropped crate, transverse waves behind the stern.  DEEP is a second, OPT-IN step mode
 * of the layer with that dispersion relation -- Tessendorf's iWave idea: the vertical-derivative operator √(−∇²) as a 13 × 13 convolution.
 * The default mode is DATUM_OCEAN_RIPPLE_WAVE, the step stated under "ripple layer", and in it every call keeps its bits.  Everything that
 * READS the state is unchanged in either mode: datum_ocean_sample_ripples, the rippled reads, the ripple bounds, wake foam,
 * datum_ocean_center_ripples and the deposits.
 *
 * WEIGHTS.  P = 6 (DATUM_OCEAN_RIPPLE_DEEP_RADIUS).  The quadrant table G[l][k], 0 <= k, l <= 6 (DATUM_OCEAN_RIPPLE_DEEP_WEIGHTS = 49
 * floats, [l][k]), is built once on the host in double:
 *   1  G0[l][k] = (1/M²) Σ_a Σ_b |θ_ab| cos(k θ_a) cos(l θ_b)     M = 1024, θ_a = 2π(a − M/2)/M, |θ_ab| = √(θ_a² + θ_b²)
 *      the truncated Fourier series of the cone, summed separably (over b for every a and l, then over a);
 *   2  unfold to the 169 weights F(di, dj) = G0[|dj|][|di|], subtract ΣF / 169 from every one, and round each to fp32;
 *   3  replace the centre by the fp32 value that makes the sum of the 169 fp32 weights, taken in double, the smallest value >= 0: round
 *      towards that, with one nextafterf upward if needed.
 * The subtraction is the least-squares correction for Ĝ(0) = 0, where the SYMBOL is Ĝ(θ) = Σ F(di, dj) cos(di·θx) cos(dj·θy): its effect on
 * the symbol is a Dirichlet kernel concentrated at θ = 0.  Of this table (tests/test_ripple_deep64.py): Ĝ >= 0, with its minimum at θ = 0;
 * |Ĝ − |θ|| / |θ| <= 0.08 for 0.5 <= |θ| <= 1 and <= 0.02 for 1 <= |θ| <= 3; max Ĝ = 4.30, Σ|F| = 5.37, F(0, 0) ≈ 2.40.
 * BELOW |θ| ≈ 0.45 (WAVELENGTHS ABOVE 14 CELLS) THE SYMBOL IS QUADRATIC AND SUCH WAVES RUN SLOW: the truncation's price.  The FFT surface
 * owns those wavelengths.
 *
 * THE SUB-STEP.  h, f[k], the sponge index, the first sub-step's e = η + (float)src · 2^-20, the window, the torus and the memset behind the
 * first launch are exactly datum_ocean_step_ripples'.  Per window cell, every operator one fp32 operation as written, no contraction:
 *     acc = 0.0f
 *     for dj = −6 .. 6 (outer), di = −6 .. 6 (inner):   acc = acc + G[|dj|][|di|] · e(I + di, J + dj)     a cell outside the window is 0.0f
 *     v1  = (η_t − h · (gs · acc)) · f[k]                gs = g / s, rounded once on the host from double
 *     e1  = e + h · v1                                   the new cell is (e1, v1)
 *
 * STABILITY.  Semi-implicit Euler needs h·Ω < 2, and Ω² <= gs · Σ|F|.  A step in DEEP computes h · √(g · Σ|F| / s) in double, Σ|F| from
 * the 169 fp32 weights, and refuses a value above 1.9 with DATUM_OCEAN_EINVAL.  This replaces the c·h/s > 0.7 check in this mode only; the
 * rules for dt < 0 and a dt that is not finite stay.
 *
 *   set_ripple_dispersion   mode DATUM_OCEAN_RIPPLE_WAVE (0, the default) or DATUM_OCEAN_RIPPLE_DEEP (1); g finite and > 0, default 9.81
 *                           (as a float); c is unused in DEEP and g in WAVE.  Works while the layer is off, survives
 *                           datum_ocean_set_ripples, writes no state, enqueues nothing and leaves the ripple bounds' CURRENT mark alone.  A
 *                           null handle, an unknown mode or a bad g is DATUM_OCEAN_EINVAL and changes nothing.
 *   ripple_deep_weights     takes NO HANDLE and needs no GPU: the table above, [l][k], 49 floats, the exact weights the kernel uses, for a
 *                           renderer or a test.  A null pointer is DATUM_OCEAN_EINVAL.
 * datum_ocean_step_ripples, datum_ocean_step_bodies_coupled and its host twin take the layer's mode.  Coupled stepping's contract holds in
 * DEEP bit for bit -- K rounds of the reductions and the wake from rippled records, then datum_ocean_step_ripples(h, 1) -- and its refusal
 * uses the DEEP bound.  A mode switch between two calls behaves as two layers would: the state is common, (η, η_t) in both modes.
 * LEFT OUT: temporal blocking; finite-depth dispersion (ω² = g·k·tanh(k·d)); radii other than 6; obstacles
 * (no longer left out: "ripple walls", below). */
#define DATUM_OCEAN_RIPPLE_WAVE 0
#define DATUM_OCEAN_RIPPLE_DEEP 1
#define DATUM_OCEAN_RIPPLE_DEEP_RADIUS 6
#define DATUM_OCEAN_RIPPLE_DEEP_WEIGHTS 49
int datum_ocean_set_ripple_dispersion(datum_ocean_t ctx, int mode, float g);
int datum_ocean_ripple_deep_weights(float *quadrant49);

/* -- ripple walls (added at ABI 9; nothing in the reference) -----------------------------------------------------------------------------------
 * Obstacles the ripple layer's waves reflect off: piers, quays, rocks, a harbour wall.  OPT-IN: while no list is set nothing is allocated,
 * nothing more is launched, and every call keeps its bits in both step modes.  Every reader of the layer (mesh, query, ray cast, bounds,
 * wake foam, coupled bodies) only reads the state, so walls in the step serve all of them.
 *
 * THE PLANE.  R × R bytes, 0 water, 1 wall; world cell (I, J) lives at the state's place on the torus, (J mod R)·R + (I mod R).
 *
 * THE SHAPES.  A wall is a 32-byte datum_ocean_ripple_wall; at most DATUM_OCEAN_RIPPLE_MAX_WALLS = 256 of them.  `axis` is the shape's
 * local x direction, GIVEN BY THE CALLER AS (cosine, sine): the library takes no sine or cosine of its own and DOES NOT NORMALISE the
 * axis -- a non-unit axis scales the shape.  `half` are the half extents (box) or semi-axes (ellipse) along the local x and y.
 *
 * THE RASTER RULE.  For world cell (I, J), s the fp32 cell side given to datum_ocean_set_ripples, every operator one fp32 operation as
 * written, no contraction, no division:
 *     x  = ((float)I + 0.5f) · s          y  = ((float)J + 0.5f) · s
 *     dx = x − center[0]                  dy = y − center[1]
 *     u  = dx·axis[0] + dy·axis[1]        v  = dy·axis[0] − dx·axis[1]
 *     BOX:      |u| <= half[0] && |v| <= half[1]
 *     ELLIPSE:  a = u·half[1], b = v·half[0], r = half[0]·half[1];   a·a + b·b <= r·r
 * A cell is wall if any record covers its centre.  The plane is a function of (list, world cell) only: after any
 * datum_ocean_center_ripples it equals that function at the new origin, cells that entered and a jump of R cells or more included (the
 * call rasterises the whole plane again behind the scroll).
 *
 * THE SUB-STEP WITH WALLS.  h, f[k], the sponge, the window test, the first sub-step's e = η + (float)src · 2^-20, the torus and the
 * memset behind the first launch are datum_ocean_step_ripples', unchanged.
 *   - a wall cell's new state is (+0.0f, +0.0f) in both modes; its src is ignored (a deposit that lands on a wall cell is lost, uncounted);
 *   - reading a neighbour: outside the WINDOW -> 0.0f, the wall flag of the torus-aliased cell is not consulted; else wall -> the rule of
 *     the mode; else its height;
 *   - WAVE: a wall neighbour reads as the cell's own e -- a hard vertical wall, the mirror plane the face between the two cells, the wave
 *     reflected without a change of sign; the update is the wave step's as it stands;
 *   - DEEP: a wall cell reads 0.0f in the convolution, the pending deposit of a first sub-step included (iWave's obstruction); the sum
 *     and the update are the DEEP step's as they stand, over an image in which wall cells are zero.
 * No new stability refusal: in WAVE the mirrored operator is the graph Laplacian of the open cells (symmetric, eigenvalues in [−8, 0]),
 * in DEEP a principal submatrix of the windowed operator (symmetric, the same bound gs·Σ|F|).
 *
 *   set_ripple_walls       `walls` is a HOST pointer to `count` records; the handle keeps its own copy.  count == 0 turns walls off and
 *                          frees the plane.  Otherwise ONE launch on the handle's stream writes the plane and makes the state of every wall
 *                          cell (+0, +0) in BOTH state buffers; the ripple bounds' CURRENT mark is cleared; src, the wake-foam plane and
 *                          everything else are left alone.  DATUM_OCEAN_EINVAL: a null handle, count < 0 or above the maximum, null walls
 *                          with count > 0, a field that is not finite, a half that is not > 0, an unknown kind.  DATUM_OCEAN_ESTATE while
 *                          the layer is off.  datum_ocean_set_ripples with any R drops the walls, as it drops the wake foam;
 *                          datum_ocean_reset_ripples keeps them.
 *   ripple_walls_device    *plane = the device plane in memory order, R·R bytes, null while walls are off; a renderer masks with it.
 *                          Stable until the next set_ripple_walls or set_ripples.
 *   read_ripple_walls      the plane to the HOST in window order, [j][i] for cell (ox + i, oy + j), as datum_ocean_read_ripple_foam;
 *                          blocking.  DATUM_OCEAN_ESTATE while walls are off.
 * LEFT OUT: moving walls and hull footprints as walls (a wall that moves must displace the water it covers; the wake deposit is the model
 * for hulls); fractional obstruction; walls in the bilinear sample (it blends the wall cell's zero as it is); walls in wake foam and the
 * ripple bounds (they see wall cells as water at rest); a count of deposits lost on wall cells; finite depth; a shoreline.
 * (Finite depth and a shoreline are no longer left out: "ripple bed", below.) */
#define DATUM_OCEAN_RIPPLE_WALL_BOX 0
#define DATUM_OCEAN_RIPPLE_WALL_ELLIPSE 1
#define DATUM_OCEAN_RIPPLE_MAX_WALLS 256
typedef struct datum_ocean_ripple_wall
{
  float center[2];      /* world metres */
  float axis[2];        /* the local x direction: (cosine, sine), not normalised by the library */
  float half[2];        /* half extents / semi-axes along the local x and y, each > 0 */
  int kind;             /* DATUM_OCEAN_RIPPLE_WALL_BOX or DATUM_OCEAN_RIPPLE_WALL_ELLIPSE */
  int reserved;         /* not read */
} datum_ocean_ripple_wall;
int datum_ocean_set_ripple_walls(datum_ocean_t ctx, datum_ocean_ripple_wall const *walls, int count);
int datum_ocean_ripple_walls_device(datum_ocean_t ctx, unsigned char const **plane);
int datum_ocean_read_ripple_walls(datum_ocean_t ctx, unsigned char *host);

/* -- ripple bed (added at ABI 9; nothing in the reference) --------------------------------------------------------------------------------------
 * Still-water depth under the ripple layer: waves slow, steepen and bend over a shoal and die on a beach.  OPT-IN: while no bed is set
 * nothing is allocated, the parents' kernels are launched, and every call keeps its bits in both step modes.  Every reader of the layer
 * (mesh, query, ray cast, bounds, wake foam, coupled bodies) only reads the state, so the bed in the step serves all of them.
 * The model is variable-depth shallow water, η_tt = ∇·(g·d·∇η): the wave step's five-point stencil with a coefficient per face.
 *
 * THE MAP.  `depths_host` is a HOST array of width × height floats, row-major, [j·width + i]: still-water depth in metres, POSITIVE DOWN
 * (a value <= 0 is land).  2 <= width, height <= DATUM_OCEAN_RIPPLE_BED_MAX_SIDE = 4096.  Texel (0, 0) stands at world `origin`, texel
 * (i, j) at origin + (i, j)·texel.  `outside` is the depth that a cell off the map reads.  The handle keeps a device copy of the map.
 *
 * THE PLANES.  Two on the layer's torus, world cell (I, J) at the state's place (J mod R)·R + (I mod R):
 *   d   R × R floats: the effective depth, +0.0f where the cell is SOLID (dry land, or a wall);
 *   q   R × R bytes: the surf level, 0 .. DATUM_OCEAN_RIPPLE_SURF_LEVELS = 16.
 * Both are a function of (map, parameters, wall plane, world cell) only: after any datum_ocean_center_ripples they equal that function at
 * the new origin, cells that entered and a jump of R cells or more included.
 *
 * THE RASTER RULE.  For world cell (I, J), s the fp32 cell side, every operator one fp32 operation as written, no contraction, no
 * division; invt = (float)(1.0 / texel) and invsurf = (float)(1.0 / surf_depth) are rounded once on the host from double:
 *     x = ((float)I + 0.5f) · s           y = ((float)J + 0.5f) · s                  (the centre, as the wall raster has it)
 *     u = (x − origin[0]) · invt          v = (y − origin[1]) · invt
 *     u < 0 or u > width − 1 or v < 0 or v > height − 1:   raw = outside
 *     else  i = min((int)floorf(u), width − 2), j = min((int)floorf(v), height − 2), wu = u − (float)i, wv = v − (float)j,
 *           c0 = map[j][i], c1 = map[j][i + 1], c2 = map[j + 1][i], c3 = map[j + 1][i + 1]
 *           a0 = c1 − c0, a1 = c3 − c2, e0 = c0 + wu·a0, e1 = c2 + wu·a1, raw = e0 + wv·(e1 − e0)     (the ripple sample's patch)
 *     d = fminf(fmaxf(raw, 0), max_depth);   d < dry_depth -> d = +0;   the cell's wall byte is 1 (walls on) -> d = +0
 *     q = 0 where d == 0 or surf_depth == 0 or d >= surf_depth, else min(16, (int)floorf((1 − d·invsurf)·16))
 *
 * THE SUB-STEP OVER A BED.  The WAVE mode with a bed.  h, fsponge[k], the sponge index, the window test, the first sub-step's
 * e = η + (float)src · 2^-20, the torus and the memset behind the first launch are datum_ocean_step_ripples', unchanged.  dc is the
 * cell's depth; for each of the four neighbours, depth dn and height en:
 *     outside the WINDOW (the depth and the flag of the torus-aliased cell are not consulted):   t = dc·(0 − e)
 *     the neighbour is solid (dn == 0):                                                         t = 0
 *     else                                                                                      t = (0.5f·(dc + dn))·(en − e)
 *     div = (tL + tR) + (tD + tU);   f = fsponge[k]·fsurf[q];   v1 = (η_t + h·(gs2·div))·f;   η' = e + h·v1;   η_t' = v1
 * gs2 = (float)(g / s²) with g the layer's g (datum_ocean_set_ripple_dispersion's, 9.81 by default);
 * fsurf[q] = (float)(1 / (1 + h·surf_gamma·(q/16)²)), built on the host in double beside fsponge: breaking as a damping that grows
 * towards the shore.  With surf_depth == 0 the factor is exactly 1.0f.  A solid cell's new state is (+0.0f, +0.0f); a deposit that lands
 * on it is lost, uncounted, as on a wall.  WHILE THE BED IS ON, datum_ocean_set_ripple_params' c IS NOT USED BY THE STEP: the speed is
 * sqrt(g·d) of the place.
 *
 * STABILITY.  The face coefficient is the mean of its two cells, so the operator is symmetric on the wet cells and its row sums are at most
 * 4·max_depth: the wave step's Gershgorin argument holds with c := sqrt(g·max_depth).  While the bed is on, datum_ocean_step_ripples and
 * datum_ocean_step_bodies_coupled refuse sqrt(g·max_depth)·dt / (substeps·s) above 0.7 where they refused c·dt / (substeps·s).
 *
 * DEEP.  The bed and the DEEP mode DO NOT COMBINE (a variable depth is not a convolution): datum_ocean_set_ripple_bed while the mode is
 * DATUM_OCEAN_RIPPLE_DEEP, and datum_ocean_set_ripple_dispersion(DATUM_OCEAN_RIPPLE_DEEP, ...) while a bed is set, return
 * DATUM_OCEAN_ESTATE.  Uniform finite depth for DEEP stays left out.
 *
 *   set_ripple_bed         a null `bed` turns the bed off and frees everything.  Otherwise the map is copied (blocking, as the wall list
 *                          is: the caller's array may go away behind the call), then ONE launch on the handle's stream rasters both
 *                          planes and makes the state of every solid cell (+0, +0) in BOTH state buffers; the ripple bounds' CURRENT mark
 *                          is cleared; src, the wake-foam plane and everything else are left alone.  DATUM_OCEAN_EINVAL: a null handle,
 *                          null depths_host, width or height outside [2, 4096], texel not finite or not > 0, origin or outside not
 *                          finite, max_depth not finite or not > 0, dry_depth not in (0, max_depth], surf_depth or surf_gamma not finite
 *                          or negative, a map value that is not finite (checked on the host).  DATUM_OCEAN_ESTATE while the layer is off
 *                          or its mode is DEEP.  datum_ocean_set_ripples with any R drops the bed, as it drops the walls;
 *                          datum_ocean_reset_ripples keeps it.  datum_ocean_center_ripples rebuilds both planes whole, in one launch
 *                          behind the wall raster; datum_ocean_set_ripple_walls rasters the bed again, since the wall byte enters d.
 *   ripple_bed_device      *depth and *surf = the device planes in memory order (R·R floats, R·R bytes), *cells = R·R; null and 0 while
 *                          the bed is off.  Any of the three may be null.  Stable until the next set_ripple_bed or set_ripples.
 *   read_ripple_bed        both planes to the HOST in window order, [j][i] for cell (ox + i, oy + j), as datum_ocean_read_ripple_walls;
 *                          either may be null; blocking.  DATUM_OCEAN_ESTATE while the bed is off.
 * LEFT OUT: the bed in DEEP, as tanh(k·d) weights; wetting and drying, run-up and non-linear steepening (the shoreline is fixed at
 * dry_depth); foam from the surf zone; bounds and wake foam treating solid cells as anything but water at rest; the FFT swell feeling the
 * bed; writing only the entered cells on a scroll; temporal blocking.
 * ("The FFT swell feeling the bed" is struck in part: the swell's source on a beach fades with the depth ("ripple swell", below); H
 * itself still does not shoal.) */
#define DATUM_OCEAN_RIPPLE_SURF_LEVELS 16
#define DATUM_OCEAN_RIPPLE_BED_MAX_SIDE 4096
typedef struct datum_ocean_ripple_bed
{
  int width, height;    /* texels of the map, each in [2, DATUM_OCEAN_RIPPLE_BED_MAX_SIDE] */
  float origin[2];      /* world metres of texel (0, 0) */
  float texel;          /* the side of a texel in metres, > 0 */
  float outside;        /* the depth a cell off the map reads */
  float max_depth;      /* > 0: depths are clamped to it, and it sets the stability bound */
  float dry_depth;      /* in (0, max_depth]: a cell shallower than this is solid */
  float surf_depth;     /* >= 0: the surf zone is where d < surf_depth; 0 for none */
  float surf_gamma;     /* >= 0: the damping rate 1/s at the shoreline end of the surf zone */
} datum_ocean_ripple_bed;
int datum_ocean_set_ripple_bed(datum_ocean_t ctx, datum_ocean_ripple_bed const *bed, float const *depths_host);
int datum_ocean_ripple_bed_device(datum_ocean_t ctx, void **depth, void **surf, size_t *cells);
int datum_ocean_read_ripple_bed(datum_ocean_t ctx, float *depth, unsigned char *surf);

/* -- ripple swell (added at ABI 9; nothing in the reference) ------------------------------------------------------------------------------------
 * The FFT swell reflects off ripple walls and the beach.  The renderer adds the summed surface H to the layer's η, and H passes through
 * every pier as if it were not there.  With swell on, the layer carries the SCATTERED FIELD: the difference between the open-sea swell
 * and the water that is really there.  No flux of the total H + η may pass through a solid face, so every solid face is a source for η
 * of strength minus the incident flux through it: in front of a wall that radiates the reflection, behind it −H, which is the shadow,
 * round its end the diffraction.  OPT-IN: while swell is off nothing is allocated, the parents' kernels are launched, and every call
 * keeps its bits.  Every reader of the layer (mesh, query, ray cast, bounds, wake foam, coupled bodies) only reads the state, so swell
 * in the step serves all of them; the renderer changes nothing.  SEEN IN FLOAT64 (tests/test_ripple_swell64.py), with a
 * refresh before every sub-step and no damping: the mirrored wave before a straight wall to 8 % of the amplitude at 16 cells a
 * wavelength, first order in the cell side; no flux of H + η through the wall's faces; rms(H + η) 0.59 of rms(H) close behind a
 * breakwater four wavelengths wide.  Not seen: either under a refresh every few sub-steps, or under the layer's damping γ, which acts on
 * η and not on H.
 *
 * THE FORCING PLANE.  F, R × R floats on the layer's torus, world cell (I, J) at the state's place (J mod R)·R + (I mod R).  A cell is
 * SOLID by its wall byte while the bed is off (no walls: nothing is solid), by d == +0 while the bed is on (that holds the walls).  A
 * neighbour n of world cell (I, J) COUNTS when it lies inside the window and is solid; a neighbour outside the window never counts, the
 * flag of the torus-aliased cell is not consulted.  Every operator one fp32 operation as written, no contraction:
 *     dX = (neighbour X counts) ? (Hc − Hn) : +0.0f                       X = L, R, D, U
 *     F  = (dL + dR) + (dD + dU)        for a cell that is itself not solid
 *     F  = +0.0f                        for a solid cell, and (the sum of four +0) for a cell none of whose neighbours count
 * Hc and Hn are the height of the summed surface above the centres of the cell and of that neighbour, centres at
 * x = ((float)I + 0.5f) · s, y = ((float)J + 0.5f) · s as the wall raster has them: FIELD 2 OF datum_ocean_sample_surface_blend's record at
 * that point, bit for bit, for the call's cascade list, set and iterations.
 *
 * THE SUB-STEP WITH SWELL.  The WAVE mode.  F is the cell's own value, read once, no halo.  Everything else is the parent's sub-step.
 *   - without a bed, the sub-step with walls as it stands (without walls nothing is solid, F is +0 and the plain sub-step runs), with
 *         lap = (((eL + eR) + (eD + eU)) − 4.0f·e) + F
 *     in place of the wave step's lap; a wall cell's new state is (+0.0f, +0.0f);
 *   - over a bed, the bed's sub-step as it stands, with
 *         div = ((tL + tR) + (tD + tU)) + dc·F
 *     THE FACE AT A SOLID NEIGHBOUR CARRIES THE CELL'S OWN DEPTH, the rule the bed has for the window's edge: on a beach the source
 *     fades with the depth.
 * F IS FROZEN OVER THE SUB-STEPS OF A CALL; the swell moves between calls, when the caller refreshes.  No new stability refusal: F is a
 * source term, the operator is the parent's.
 *
 * CURRENCY.  F is a function of the maps, the list and set, the solid cells and the origin.  datum_ocean_refresh_ripple_swell is its only
 * writer and sets a CURRENT mark on the handle.  The mark is cleared by datum_ocean_center_ripples when the origin moves, by
 * datum_ocean_set_ripple_walls, datum_ocean_set_ripple_bed, datum_ocean_set_ripples and datum_ocean_set_ripple_swell.  WHILE THE MARK IS
 * CLEAR THE PARENTS' KERNELS ARE LAUNCHED: a stale F is never read.  The handle cannot see the maps change: a caller that displaces or
 * scrolls every frame refreshes every frame, in the order displace -> center_ripples -> refresh_ripple_swell -> step_ripples or
 * step_bodies_coupled.  datum_ocean_reset_ripples keeps the plane and the mark; datum_ocean_set_ripples drops both with the layer.
 *
 * DEEP.  Swell and the DEEP mode DO NOT COMBINE (iWave's obstruction is a mask, not a face flux): datum_ocean_set_ripple_swell(1) while
 * the mode is DATUM_OCEAN_RIPPLE_DEEP, and datum_ocean_set_ripple_dispersion(DATUM_OCEAN_RIPPLE_DEEP, ...) while swell is on, return
 * DATUM_OCEAN_ESTATE, as the bed's pair does.
 *
 *   set_ripple_swell       on = 1 allocates the plane, +0.0f everywhere, between two 256-byte guards of 0xCD, the mark clear (an `on`
 *                          while swell is on starts again from that); on = 0 frees it.  Blocking.  DATUM_OCEAN_EINVAL: a null handle, `on`
 *                          outside {0, 1}.  DATUM_OCEAN_ESTATE while the layer is off or its mode is DEEP (with on = 1).
 *   refresh_ripple_swell   ONE launch on the handle's stream writes F WHOLE and sets the mark; nothing else is written.  The list, the set
 *                          and `iterations` are datum_ocean_sample_surface_blend's and are checked as that call checks them.
 *                          DATUM_OCEAN_ESTATE while the layer or swell is off.
 *   ripple_swell_device    *plane = the device plane in memory order, *bytes = R·R·4, *current = the mark; null, 0 and 0 while swell is
 *                          off.  Any of the three may be null.  Stable until the next set_ripple_swell or set_ripples.
 *   read_ripple_swell      the plane to the HOST IN MEMORY ORDER, R·R floats, [(J mod R)][(I mod R)]; blocking, as
 *                          datum_ocean_read_ripple_walls.  DATUM_OCEAN_ESTATE while the layer or swell is off.
 * LEFT OUT: swell in DEEP; H itself shoaling or breaking over the bed (only the source at a solid face knows the depth); a swell that
 * changes within a call's sub-steps; the layer's rate in datum_ocean_sample_velocity_blend; walls in the bilinear sample's patch (the
 * mesh blends a wall cell's zero with the water beside it, so H + η does not vanish inside a wall). */
int datum_ocean_set_ripple_swell(datum_ocean_t ctx, int on);
int datum_ocean_refresh_ripple_swell(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations);
int datum_ocean_ripple_swell_device(datum_ocean_t ctx, void **plane, size_t *bytes, int *current);
int datum_ocean_read_ripple_swell(datum_ocean_t ctx, float *plane);

/* -- body contact (added at ABI 9; nothing in the reference) ------------------------------------------------------------------------------------
 * Hulls stop at ripple walls and ground on the bed.  Every wave of the layer knows the walls and the bed; with this call the bodies of
 * coupled stepping know them too.  datum_ocean_step_bodies_contact is datum_ocean_step_bodies_coupled -- its arguments, its checks, its
 * host loop, its layer sub-step, its swell handling, its bad-body rules -- with PENALTY CONTACT added to every probe's terms.  OPT-IN per
 * call: the coupled call and every other call keep their bits, and a contact call in which no probe touches anything gives the coupled
 * call's poses, motions, record fields 0-11 and layer bit for bit.
 *
 * THE PARAMETERS.  datum_ocean_body_contact, 32 bytes, a HOST pointer given to each call (the handle keeps nothing): stiffness k >= 0
 * (N/m per m² of probe weight), damping c >= 0 (N·s/m per m²), friction ct >= 0 (a VISCOUS tangential rate, N·s/m per m²; not Coulomb) and
 * flags, DATUM_OCEAN_CONTACT_BED | DATUM_OCEAN_CONTACT_WALLS.  All three are per unit probe weight a, the a body buoyancy's terms take.
 *
 * Every operator below is one fp32 operation as written (no contraction), division and sqrt the correctly rounded ones.  w is the probe's
 * world point, a its weight, T, v, ω the body's position and motion at the START of the sub-step.
 *
 * GROUND (flag BED; a bed must be set).  The handle's device copy of the depth map, the bed's invt = (float)(1.0 / texel):
 *     u = (w.x − origin[0])·invt      v = (w.y − origin[1])·invt
 *     off the map (u < 0 or u > width − 1 or v < 0 or v > height − 1, a NaN is off):   raw = outside,  n = (0, 0, 1)
 *     else  i, j, wu, wv, c0..c3, a0, a1, e0, e1 and raw = e0 + wv·(e1 − e0) as the bed's raster rule has them (UNCLAMPED: negative on land)
 *           gx = (a0 + wv·(a1 − a0))·invt      gy = (e1 − e0)·invt      l = sqrt((gx·gx + gy·gy) + 1·1)      n = (gx / l, gy / l, 1 / l)
 *     zg = 0 − raw          the ground's elevation: the map is a depth, positive down
 *     p  = zg − w.z         the penetration; the probe TOUCHES when p > 0
 *
 * WALLS (flag WALLS; walls must be set).  Walls are vertical prisms of unbounded height: contact is horizontal, n.z = 0.  For every record
 * of the list IN LIST ORDER that covers (w.x, w.y) by the raster rule, with that rule's u, v:
 *     BOX       px = half[0] − |u|      py = half[1] − |v|
 *               px <= py:  q = px,  m = (u >= 0 ? 1 : −1, 0)          else  q = py,  m = (0, v >= 0 ? 1 : −1)
 *     ELLIPSE   eu = u / half[0]      ev = v / half[1]      ρ = sqrt(eu·eu + ev·ev)      q = (1 − ρ)·fminf(half[0], half[1])
 *               ρ == 0:  m = (1, 0)          else  lx = eu / half[0], ly = ev / half[1], l = sqrt(lx·lx + ly·ly), m = (lx / l, ly / l)
 *     n  = (m.x·axis[0] − m.y·axis[1],  m.x·axis[1] + m.y·axis[0],  0)          the local normal turned by the axis AS GIVEN
 *     p  = q·inv2          inv2 = (float)(1.0 / (axis[0]² + axis[1]²)), formed in double and rounded once by datum_ocean_set_ripple_walls
 * The shape touches when p > 0.  THE LIBRARY STILL DOES NOT NORMALISE THE AXIS: with a unit axis n is a unit vector and p a distance; an
 * axis of length L gives |n| = L and p = q / L², so that the spring term k·p·n is that of the scaled shape exactly while the damping and
 * friction terms carry a factor L².  A ZERO AXIS, which datum_ocean_set_ripple_walls accepts, covers every point with inv2 = ∞ and n = 0:
 * under flag WALLS its force is ∞·0, not a number, and EVERY body of the call ends as a bad body -- give walls an axis.  THE TEST IS THE ANALYTIC SHAPE, NOT THE BYTE PLANE: the plane stays what the waves see, and a shape
 * thinner than a cell can stop a hull without reflecting a wave.
 *
 * THE FORCE OF ONE CONTACT that touches, with its p and n:
 *     r  = w − T  per component                  u = v + ω × r  in body drag's form:  u.x = v.x + (ω.y·r.z − ω.z·r.y)  ...
 *     vn = (u.x·n.x + u.y·n.y) + u.z·n.z         fn = fmaxf(a·(k·p − c·vn), 0)          the ground never pulls
 *     g  = a·ct                                  F  = fn·n − g·(u − vn·n)  per component:  F.x = fn·n.x − g·(u.x − vn·n.x)  ...
 *     τ  = r × F:  τ.x = r.y·F.z − r.z·F.y       τ.y = r.z·F.x − r.x·F.z       τ.z = r.x·F.y − r.y·F.x
 * A probe's EIGHT contact terms start at +0 and take, one fp32 addition per field, first the ground's contact and then each touching
 * shape's in list order: F (3), τ (3), the count of touching contacts (+1 each), and the deepest p (fmaxf).  They are summed beside the
 * coupled call's fourteen in the body tree's order -- twenty-two fields, the tenth and the twenty-second maxima.
 *
 * THE INTEGRATOR is datum_ocean_step_bodies' steps 2-5, called and not restated.  A body whose count is 0 advances exactly as in the
 * coupled call.  Otherwise F, τ are that call's step 2 for the sub-step; F_total = F + F_contact and τ_total = τ + τ_contact, one fp32
 * addition per component; and steps 2-5 run once more with D = (F_total, τ_total), M = bx = by = 0 and buoyancy 0: step 2 then gives
 * 0·0 + F_total.z and the like, F_total and τ_total again (a −0 becomes +0), and steps 3-5 advance the body under them.
 *
 * Each body gets a record of DATUM_OCEAN_CONTACT_RECORD_FLOATS = 16 floats (64 bytes):
 *     0-11   the coupled record's fields, by its rules (0-5 are the totals the body advanced under: WITH the contact's share)
 *     12-14  the contact force F_contact of the LAST sub-step          15   the deepest p over all sub-steps (fmaxf through the record)
 * A bad body stores sixteen quiet NaNs; every rule of the coupled call's bad bodies holds.
 *
 * WHY A PENALTY.  The integrator is semi-implicit Euler, which is symplectic for a spring: a contact spring k·Σa under a mass m is stable
 * for h·sqrt(k·Σa·invmass) < 2 and conserves a shadow energy below that.  THE BOUND IS NOT CHECKED -- the host never sees the bodies --
 * and a body that blows up ends as a bad body.  Measured in float64 (tests/test_contact64.py): a box on flat land rests at
 * p* = gravity / (k·Σa·invmass); with c > 0 its energy never rises; with c = 0 inside the bound it stays bounded.
 *
 *   step_bodies_contact        enqueue and return, as step_bodies_coupled.  records_device: nbodies × 64 bytes.
 *   step_bodies_contact_host   the same from HOST arrays, blocking, through datum_ocean_step_bodies_host's staging.
 * DATUM_OCEAN_ESTATE and DATUM_OCEAN_EINVAL wherever the coupled call returns them, in its order; then DATUM_OCEAN_EINVAL for a null
 * contact struct, a rate that is not finite or is negative, and unknown flag bits; then DATUM_OCEAN_ESTATE for flag BED with no bed set
 * and for flag WALLS with no walls set.  A refused call enqueues nothing and changes nothing.  flags = 0 is legal: the coupled call with
 * a wider record.
 * LEFT OUT: Coulomb friction (the tangential force is viscous); contact between bodies; wall tops (a wall has no height: a hull cannot
 * ride over it); moving walls; contact outside the coupled step (datum_ocean_step_bodies has none); a check of the stability bound. */
#define DATUM_OCEAN_CONTACT_RECORD_FLOATS 16
#define DATUM_OCEAN_CONTACT_BED 1u
#define DATUM_OCEAN_CONTACT_WALLS 2u
typedef struct datum_ocean_body_contact
{
  float stiffness;         /*   0  k >= 0, per unit probe weight                                       */
  float damping;           /*   4  c >= 0, along the normal                                            */
  float friction;          /*   8  ct >= 0, viscous, along the tangent                                 */
  unsigned int flags;      /*  12  DATUM_OCEAN_CONTACT_BED | DATUM_OCEAN_CONTACT_WALLS                 */
  float reserved[4];       /*  16  not read                                                            */
} datum_ocean_body_contact;
int datum_ocean_step_bodies_contact(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                    void *bodies_device, void *motions_device, void const *props_device, size_t nbodies, void const *probes_device, size_t nprobes,
                                    float dt, int substeps, void *records_device, datum_ocean_body_contact const *contact);
int datum_ocean_step_bodies_contact_host(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                         datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, size_t nbodies,
                                         float const *probes, size_t nprobes, float dt, int substeps, float *records, datum_ocean_body_contact const *contact);

/* -- the tile farm: N processes, one GPU each, independent tiles / cascades, ONE all-gather per batch ------------------
 * (nothing in the reference, which has one device.)  The displacement step needs no exchange; what
 * north_star's "single RCCL all-gather over xGMI" reassembles is the displacement field of every rank's grids.  These
 * entry points own that step, so a C++ renderer farms tiles with this module alone: the RCCL communicator, a communication
 * stream, `slots` payload buffers (this rank's packed displacement, datum_ocean_pack_displacement's formats) and `slots`
 * gathered buffers (world x payload, ordered by rank), and the event choreography between them.
 *
 *   unique_id   rank 0 only: the 128-byte id of a new communicator; hand it to every rank (a pipe, a file, MPI, a socket)
 *   init        every rank, same id / world / format / slots: creates the communicator (blocks until all ranks have called)
 *   gather      enqueue and return: on the handle's stream, behind the last displace, the pack into the next slot's payload
 *               (first waiting, on the device, for the collective that last read that payload); on the communication stream,
 *               behind the pack and behind the slot's last release, ncclAllGather into the slot's gathered buffer.  The
 *               following displace calls overlap the collective.  *slot = which slot.
 *   result      `hip_stream` (or the handle's own stream when on_handle_stream != 0) waits for the slot's collective;
 *               *gathered_device = world x payload_bytes bytes, rank r's payload at r * payload_bytes.  A slot is gathered into
 *               again `slots` gathers later: take its result (and release it) before that
 *   release     `hip_stream` (or the handle's) has finished reading the gathered buffer up to this point: the slot's next
 *               collective waits for it.  Needed whenever a consumer reads on a stream of its own: a gather that comes round to
 *               a slot whose result went to another stream and was not released fails with DATUM_OCEAN_ESTATE.
 *   query       DATUM_OCEAN_OK once the slot's collective has finished, DATUM_OCEAN_ENOTREADY before; never blocks
 *   wait        blocks the host until it has; *collective_ms (may be NULL) = its duration on the communication stream
 *   shutdown    destroys communicator, stream and buffers (datum_ocean_destroy does it too)
 * RCCL is opened with dlopen at the first farm call (DATUM_OCEAN_RCCL_LIB, librccl.so.1): DATUM_OCEAN_EUNSUPPORTED when no
 * library is found; an ncclResult_t is reported as DATUM_OCEAN_ECOMM with RCCL's text in datum_ocean_last_error.
 * datum_ocean_farm_init is a COLLECTIVE over the ranks (ncclCommInitRank) and RCCL gives it no timeout: it returns when every rank of
 * the farm has called it, and not at all when one never does.  A launcher must therefore end the remaining ranks when one rank dies
 * before its farm_init (examples/ocean_farm.cpp reaps its ranks in the order they end and does so; bench.py's launcher likewise). */
#define DATUM_OCEAN_FARM_ID_BYTES 128
int datum_ocean_farm_unique_id(void *id, size_t bytes);
int datum_ocean_farm_init(datum_ocean_t ctx, void const *id, size_t bytes, int rank, int world, int format, int slots);
int datum_ocean_farm_shutdown(datum_ocean_t ctx);
int datum_ocean_farm_info(datum_ocean_t ctx, int *rank, int *world, int *format, size_t *payload_bytes, int *slots, int *rccl_version);
int datum_ocean_farm_gather(datum_ocean_t ctx, int *slot);
int datum_ocean_farm_result(datum_ocean_t ctx, int slot, void *hip_stream, int on_handle_stream, void **gathered_device, size_t *bytes);
int datum_ocean_farm_release(datum_ocean_t ctx, int slot, void *hip_stream, int on_handle_stream);
int datum_ocean_farm_query(datum_ocean_t ctx, int slot);
int datum_ocean_farm_wait(datum_ocean_t ctx, int slot, float *collective_ms);

/* The farm's two streams on DISJOINT compute units (hipExtStreamCreateWithCUMask; ABI 6).  RCCL's channels are workgroups that copy; while
 * they share compute units with the step's workgroups their bursts sit in the same in-order memory queues and the step kernels take 46-54 %
 * longer under a collective-sized copy (one-GPU stand-in, profiles/r05_gather_overhead.txt); with the copy on 32 compute units of its own and
 * the step on the other 224 it is 27-28 % (7 % of it the 32 CUs the step gives up).
 *   partition   after farm_init, nothing in flight: comm_cus (0 = undo, else a multiple of 8, at most half the device) compute units --
 *               comm_cus / 8 of each XCD -- for the communication stream, the others for the handle's OWN stream; both streams are
 *               recreated.  A handle that runs on a caller's stream (datum_ocean_set_stream) keeps it: hand it the own stream instead
 *   own_stream  the handle's own hipStream_t (e.g. to record events on it or to make it the current stream of a framework), valid until
 *               the next partition / shutdown / destroy
 * farm_shutdown undoes the partition.
 * NULL STREAM: hipExtStreamCreateWithCUMask takes no flags; the streams it makes report hipStreamDefault where this runtime says anything
 * (farm_stream_flags below: 0 = hipStreamDefault = BLOCKING, 1 = hipStreamNonBlocking), i.e. unlike the hipStreamNonBlocking streams they
 * replace they synchronise with the legacy null stream: an operation a caller puts on the null stream (a synchronous hipMemcpy, a
 * framework's default stream) while the farm runs serialises the communication and the compute stream and costs the overlap the
 * partition exists for -- results stay right.  The module itself never touches the null stream after datum_ocean_create (every copy,
 * memset and kernel of every entry point is on the handle's stream or the communication stream: tests/test_golden_and_abi.py holds
 * the sources to that); keep the caller's own work off it too while a partitioned farm is gathering. */
#define DATUM_OCEAN_FARM_PARTITION_AUTO (-1)   /* comm_cus: an eighth of the device in whole shares of 8 (32 of 256); 0 on a device with fewer than 64 compute units */
int datum_ocean_farm_partition(datum_ocean_t ctx, int comm_cus);
int datum_ocean_own_stream(datum_ocean_t ctx, void **hip_stream);
int datum_ocean_farm_stream_flags(datum_ocean_t ctx, unsigned int *communication_stream_flags, unsigned int *own_stream_flags);   /* hipStreamGetFlags of the two (ABI 7) */

/* blocking read-backs (host pointers).  maps: 2*N*N*4 floats. */
int datum_ocean_read_maps(datum_ocean_t ctx, int cascade, float *maps);

/* The same image on the DEVICE: a cascade's displacement map as the reference's shaders see it (ocean.cpp:706, map.comp:79-80:
 * N x N x 2 layers RGBA32F, [layer][y][x][4], .w = 0) written into caller-owned device memory of 2 * N * N * 16 bytes -- e.g. the
 * imported memory of a linear VkImage / VkBuffer the renderer samples itself (datum_ocean_import_memory_fd).  One kernel on
 * the handle's stream behind the last displace; the module's own 24-byte layout is untouched. */
int datum_ocean_export_maps(datum_ocean_t ctx, int cascade, void *device_dst, size_t bytes);

/* wait_fence (ocean.cpp:725) */
int datum_ocean_sync(datum_ocean_t ctx);

/* Cross-queue ordering (the reference's VkSemaphores: up to 8 wait dependencies, vulkan.cpp:1308-1328, and the
 * `rendercomplete` semaphore signalled by the submit, ocean.cpp:803, that render() waits on, renderer.cpp:6848).
 * wait_event: work enqueued afterwards waits for the caller's hipEvent_t.  signal: records the handle's own
 * completion hipEvent_t behind everything enqueued so far and returns it (owned by the handle). */
int datum_ocean_wait_event(datum_ocean_t ctx, void *hip_event);
int datum_ocean_signal(datum_ocean_t ctx, void **hip_event);

/* The host bridge for `rendercomplete` (ocean.cpp:341,803; waited on at renderer.cpp:6848) where the runtime cannot
 * import a VkSemaphore (hipImportExternalSemaphore returns "not supported" on ROCm 7.0.x: import_semaphore_fd then fails with
 * DATUM_OCEAN_EUNSUPPORTED):
 *   on_complete  `callback(user)` runs on a runtime thread once everything enqueued on the handle's stream so far has
 *                finished -- the integrator signals the renderer from it (vkSignalSemaphore on a timeline semaphore, or an
 *                empty vkQueueSubmit that signals the binary `rendercomplete`).  No HIP call may be made from the callback.
 *   query        DATUM_OCEAN_OK when everything enqueued before the last datum_ocean_signal has finished,
 *                DATUM_OCEAN_ENOTREADY while it has not; never blocks (a renderer that polls once per frame).
 * INTEGRATION.md 3a has the call sequence. */
int datum_ocean_on_complete(datum_ocean_t ctx, void (*callback)(void *user), void *user);
int datum_ocean_query(datum_ocean_t ctx);

/* -- Vulkan <-> HIP interop, the HIP half --------------------------------------------------
 * In datum the Ocean mesh's vertex buffer is a VkBuffer the graphics queue draws from (ocean.cpp:270, bound at
 * geometrylist.cpp:463,513) and the frame's submit waits on the ocean's `rendercomplete` VkSemaphore (ocean.cpp:803,
 * renderer.cpp:6848).  For the renderer to consume what this module writes without a copy, the renderer exports the
 * buffer's VkDeviceMemory and its semaphores as POSIX file descriptors (VK_KHR_external_memory_fd /
 * VK_KHR_external_semaphore_fd, handle type OPAQUE_FD) and this module imports them:
 *   import_memory_fd     hipImportExternalMemory + hipExternalMemoryGetMappedBuffer: a device pointer over the same
 *                        memory, valid for datum_ocean_gen (vertices) and datum_ocean_bind_maps.  On success the
 *                        descriptor belongs to the handle (do not close it); released by release_memory or destroy.
 *   import_semaphore_fd  hipImportExternalSemaphore; signal_external / wait_external enqueue a signal / a wait on the
 *                        handle's stream: the rendercomplete semaphore and the up to 8 wait dependencies of the
 *                        reference's submit (vulkan.cpp:1308-1328).  Returns DATUM_OCEAN_EUNSUPPORTED where the runtime
 *                        has no external semaphores (ROCm 7.0.x on the MI355X boxes: only the MEMORY import has ever
 *                        succeeded there, profiles/r02_external_memory_probe.txt); the host bridge above is what works.
 * INTEGRATION.md has the Vulkan side of the handshake. */
int datum_ocean_import_memory_fd(datum_ocean_t ctx, int fd, size_t bytes, void **device_ptr);
int datum_ocean_release_memory(datum_ocean_t ctx, void *device_ptr);
int datum_ocean_import_semaphore_fd(datum_ocean_t ctx, int fd, void **semaphore);
int datum_ocean_release_semaphore(datum_ocean_t ctx, void *semaphore);
int datum_ocean_signal_external(datum_ocean_t ctx, void *semaphore);
int datum_ocean_wait_external(datum_ocean_t ctx, void *semaphore);

/* Device memory for the Ocean mesh (vertex buffer with compute-writable usage + index buffer,
 * ResourceManager::create<Ocean>, ocean.cpp:262-288) for hosts that do not link HIP themselves.
 * write/read are ordered on the handle's stream; read blocks until the data is on the host. */
int datum_ocean_device_alloc(datum_ocean_t ctx, size_t bytes, void **device_ptr);
int datum_ocean_device_free(datum_ocean_t ctx, void *device_ptr);
int datum_ocean_device_write(datum_ocean_t ctx, void *device_dst, void const *host_src, size_t bytes);
int datum_ocean_device_read(datum_ocean_t ctx, void *host_dst, void const *device_src, size_t bytes);

char const *datum_ocean_last_error(datum_ocean_t ctx);

/* -- the reference's own host-side table, kept for API parity (ocean.cpp:686-700) ------------------------- */

/* weights[i * 2*log2(N) + 2*s + {0,1}] = cos / sin(-2 pi i / 2^(s+1)) evaluated exactly as the reference
 * does (fp32, unreduced angle).  The HIP kernels do not consume it. */
int datum_ocean_reference_weights(int resolution, float *weights);

/* -- diagnostics ------------------------------------------------------------------------------------------- */

/* ocean.sim alone from the current device state (no phase advance): N*N*2 floats each, host pointers */
int datum_ocean_debug_sim(datum_ocean_t ctx, int cascade, float *h, float *hx, float *hy);

/* the work spectrum after the row pass of the last datum_ocean_displace, converted back to row-major: N*N*2 floats
 * each, host pointers.  The module transforms two packed fields instead of the reference's three (what
 * ocean.map keeps is the real part of each transform): with F_S[y][x] = F[y][x] + conj(F[(N-y)%N][(N-x)%N])
 * (twice the Hermitian part; the halving is folded into the column pass),
 *   c = rows of ocean.fftx applied to  C = h_S + i hx_S
 *   d = rows of ocean.fftx applied to  D = hy_S + 2 sin(2 pi x / N) h_S
 * where h, hx, hy are ocean.sim's outputs (datum_ocean_debug_sim).  The call re-runs the row pass of this one cascade from its current
 * state (no pending update is applied) into work-spectrum slot 0; with the fp16 formats the values are the stored halves times 2^-e
 * (exact in fp32).  A cascade without a state (datum_ocean_upload_state) is refused with DATUM_OCEAN_ESTATE, as by datum_ocean_displace. */
int datum_ocean_debug_rowpass(datum_ocean_t ctx, int cascade, float *c, float *d);

/* hipEvent timing of the two kernels of datum_ocean_displace on the handle's stream.
 * begin: every `stride`-th displace call (at most max_samples of them) launches its two kernels with a start and a
 * stop event attached to the dispatch itself (hipExtLaunchKernel), i.e. each sampled kernel is timed from its first
 * to its last workgroup and nothing is inserted between the kernels; end: sync and return the mean kernel durations
 * in milliseconds and the number of displace calls sampled.
 * With several cascade groups per displace call (datum_ocean_set_cascade_group) a sample is the SUM over the call's launches of either kernel. */
int datum_ocean_profile_begin(datum_ocean_t ctx, int max_samples, int stride);
int datum_ocean_profile_end(datum_ocean_t ctx, double *rowpass_ms, double *colpass_ms, int *steps);

/* algorithmic bytes moved by one displace call of the handle (96 B per point per cascade;
 * split: row pass 16 in + 24 out, column pass 24 in + 32 out) */
int datum_ocean_algorithmic_bytes(datum_ocean_t ctx, double *rowpass_bytes, double *colpass_bytes);

#ifdef __cplusplus
}
#endif

#endif
