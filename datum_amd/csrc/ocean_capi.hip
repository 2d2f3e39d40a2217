// ocean_capi.hip -- the extern "C" module of include/datum_ocean_hip.h (host side of the HIP path).
//
// Owns the device buffers the reference keeps in OceanContext (src/renderer/ocean.h:12-46:
// oceanset, spectrum, displacementmap) and enqueues the kernels of ocean_kernels.hip where the
// reference records its five dispatches (src/renderer/ocean.cpp:769-793).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_ext.h>

#include "ocean_layout.h"
#include "ocean_quadrant.h"
#include "ocean_writeback.h"
#include "ocean_kernels.hip"
#include "ocean_gen.hip"
#include "ocean_literal.hip"
#include "ocean_farm.hip"
#include "ocean_foam.hip"
#include "ocean_surface.hip"
#include "ocean_query.hip"
#include "ocean_blend.hip"
#include "ocean_body.hip"
#include "ocean_ray.hip"
#include "ocean_bounds.hip"
#include "ocean_velocity.hip"
#include "ocean_drag.hip"
#include "ocean_step.hip"
#include "ocean_ripple.hip"
#include "ocean_ripple_deep.hip"
#include "ocean_couple.hip"
#include "ocean_contact.hip"
#include "ocean_rippled.hip"
#include "ocean_ripple_bounds.hip"
#include "ocean_ripple_foam.hip"
#include "ocean_ripple_wall.hip"
#include "ocean_ripple_bed.hip"
#include "ocean_ripple_swell.hip"

using namespace ocean;

// One kernel of the step as the module launches it: entry point, workgroup, dynamic LDS and work items per cascade (workgroups of row pairs
// for the row pass, tiles for the column pass)
struct PassKernel
{
  void const *kernel = nullptr;
  int threads = 0;
  size_t lds = 0;
  int items = 0;
  bool walks = false;                 // persistent workgroups, at most one per compute unit, walk their share of the items (col_walks)
};

// every kernel a step can launch at the handle's resolution (step_kernels), filled and configured once by datum_ocean_create
struct StepKernels
{
  PassKernel row[3][3];               // [DATUM_OCEAN_SPECTRUM_*][ROW_PLANE, ROW_WILD (a phase outside [0, 2 pi)), ROW_QUADRANT (the phase from the quadrant tables)]
  PassKernel col[2][2];               // [fp16 work spectrum][maps streamed]; the written-through kernel twice where there is no streamed form
};

enum { ROW_PLANE = 0, ROW_WILD = 1, ROW_QUADRANT = 2 };

// a device plane the caller can replace with memory of its own (datum_ocean_bind_maps, datum_ocean_bind_foam)
template<typename T>
struct BindablePlane
{
  T *own = nullptr;
  T *bound = nullptr;
  T *get() const { return bound ? bound : own; }   // the plane in use
};

// bytes of each guard round a plane of the ripple layer's: the plane keeps hipMalloc's alignment to that
constexpr size_t RIPPLE_GUARD_BYTES = 256;

// a device plane of the ripple layer's between two guards of 0xCD bytes, filled once and never written again: no kernel's resource covers
// the guards, and a test finds them whole.  Nothing is allocated, and get() is null, while the plane is off
// (in the module's own namespace: its functions are no symbols of the library)
namespace
{
  template<typename T>
  struct GuardedPlane
  {
    T *block = nullptr;                 // the allocation: a guard, the plane, a guard
    T *plane = nullptr;
    T *get() const { return plane; }

    static_assert(RIPPLE_GUARD_BYTES % sizeof(T) == 0, "a guard is a whole number of cells");

    // the fill goes on `stream`; after a failure the caller releases
    hipError_t allocate(size_t cells, hipStream_t stream)
    {
      size_t const bytes = cells * sizeof(T) + 2 * RIPPLE_GUARD_BYTES;

      hipError_t e = hipMalloc(&block, bytes);
      if (e == hipSuccess)
        e = hipMemsetAsync(block, 0xCD, bytes, stream);
      if (e == hipSuccess)
        plane = block + RIPPLE_GUARD_BYTES / sizeof(T);

      return e;
    }

    hipError_t release()
    {
      hipError_t const e = hipFree(block);
      if (e == hipSuccess)
        block = plane = nullptr;

      return e;
    }
  };

  // ripple swell's forcing plane: a guarded plane of floats that starts as +0 everywhere, and the mark that says it is the function of
  // the maps, the list and set, the solid cells and the origin that datum_ocean_refresh_ripple_swell last wrote.  A sub-step reads the
  // plane only while the mark stands
  struct RippleSwell : GuardedPlane<float>
  {
    bool current = false;

    // the guards' fill, then the plane's zeroes, go on `stream`; after a failure the caller turns it off
    hipError_t on(size_t cells, hipStream_t stream)
    {
      current = false;

      hipError_t e = allocate(cells, stream);
      if (e == hipSuccess)
        e = hipMemsetAsync(plane, 0, cells * sizeof(float), stream);

      return e;
    }

    hipError_t off()
    {
      current = false;

      return release();
    }

    float const *fresh() const { return current ? plane : nullptr; }   // what a sub-step may read
  };
}

// a device buffer of a host entry point's (read_*) staging, grown on demand
struct Staging
{
  void *ptr = nullptr;
  size_t capacity = 0;                // bytes

  int reserve(struct datum_ocean_ctx *ctx, size_t bytes);
};

// one per array a read_* query stages, kept apart per family: a family's growth frees nothing another family's launch may still read
enum { STAGE_POINTS, STAGE_SAMPLES, STAGE_BODIES, STAGE_BODY_RECORDS, STAGE_PROBES, STAGE_MOTIONS, STAGE_PROPS, STAGE_RAYS, STAGE_RAY_RECORDS, STAGE_COUNT };

// the host's record of one cascade (what the kernels read of it is CascadeConst)
struct CascadeState
{
  bool uploaded = false;              // holds a state (upload_state, resume_state, rebuild_height)
  bool wild = false;                  // its phase lies outside [0, 2 pi)
  bool quadrant = false;              // its phase is its quadrant table, not the plane (ocean_quadrant.h: where the truth lives)
  bool scaledirty = false;            // fp16 only: h0 changed since specscale was sized
  bool omegadirty = true;             // the wave scale changed since its dispersion table was built
  float omegamax = 0.0f;              // largest dispersion (table corner)
  float foamthreshold = 0.5f, foamgain = 2.0f, foamdecay = 1.0f;   // datum_ocean_set_foam_params

  // the transitions of include/datum_ocean_hip.h (foam): a new state (upload_state, resume_state; new_state_foam zeroes its accumulator),
  // and the same state with a new h0 (upload_height, rebuild_height), which keeps the phase, the updates queued for it and the accumulator
  void new_state(bool wildphase) { uploaded = true; wild = wildphase; scaledirty = true; }
  void new_height() { scaledirty = true; }
};

struct datum_ocean_ctx
{
  int device = 0;
  int N = 0;
  int cascades = 0;

  int cus = 0;                        // compute units of the device
  StepKernels kernels;

  hipStream_t stream = nullptr;       // the one in use
  hipStream_t ownstream = nullptr;

  float2 *h0 = nullptr;
  float2 *seed = nullptr;             // [cascade][N*N] OceanParams::seed, only when the caller uploads it
  float *phase = nullptr;
  float *qphase = nullptr;            // [cascade][(N/2+1)^2] the phase of the cascades whose CascadeState::quadrant is set
  int phasestore = DATUM_OCEAN_PHASE_STORE_AUTO;   // datum_ocean_set_phase_store
  void *spec = nullptr;               // cd[cascades][P], or ch[...] with the fp16 spectrum
  bool half = false;                  // DATUM_OCEAN_SPECTRUM_FP16 or _FP16_H0
  bool h0half = false;                // DATUM_OCEAN_SPECTRUM_FP16_H0: the row pass reads h0 as halves ...
  unsigned int *h0h = nullptr;        // ... from this copy, [cascades][P] x two halves, rebuilt with the scale when h0 changes (size_spectrum_scale)
  int cascadegroup = 0;               // cascades per launch of the two passes, 0 = sized to the Infinity Cache (plan_step)
  int mappolicy = DATUM_OCEAN_MAPS_AUTO;   // datum_ocean_set_map_store_policy

  // validation mode (datum_ocean_set_literal_transform): the reference's own radix-2 transforms with its literal twiddle table
  bool literal = false;
  float2 *litfields = nullptr;        // [3][N*N]: h, hx, hy of the cascade being displaced (the reference's Spectrum buffer, ocean.cpp:61-68)
  float *litweights = nullptr;        // [N][2 log2 N] (ocean.cpp:686-700)
  unsigned int *absmax = nullptr;     // device word for ocean_absmax_kernel
  BindablePlane<float4> maps;
  cf *tw = nullptr;
  float *omega = nullptr;             // [cascade][(N/2+1)^2] dispersion quadrant, rebuilt when a wavescale changes
  cf *scratch = nullptr;              // 3 row-major planes for the debug read-backs (lazy)

  CascadeConst casc[DATUM_OCEAN_MAX_CASCADES];
  CascadeState cstate[DATUM_OCEAN_MAX_CASCADES];

  std::vector<float> pending;         // queued update_ocean dt's no kernel has seen yet
  PhaseWriteback writeback;           // ... and those the last row pass applied without storing the phase (every cascade alike: each launch of a
                                      // displace call takes the same list)
  int writebackevery = 0;             // datum_ocean_set_phase_writeback; 0 = the module's choice (plan_step)

  // foam (datum_ocean_set_foam): one fp32 plane per cascade, computed by displace after the column pass
  int foammode = DATUM_OCEAN_FOAM_OFF;
  BindablePlane<float> foam;          // the own plane exists while foam is on; off, nothing reads the plane (a binding is kept)
  FoamKernels foamkernels = {};
  double foamdt = 0.0;                // sum of the update dt's since the last displace (pending can be flushed at any time)

  // surface velocity (datum_ocean_set_velocity): one float4 plane per cascade, computed by displace after the column pass and the foam
  int velocitymode = DATUM_OCEAN_VELOCITY_OFF;
  BindablePlane<float4> velocity;     // the own plane exists while velocity is on (a binding is kept)
  VelocityKernels velocitykernels;    // configured when velocity is first switched on
  cf *velocitywork = nullptr;         // [group][3][N*N] between the two velocity passes, while velocity is on
  int velocityworkgroup = 0;          // cascades it was sized for
  bool velocitycurrent = false;       // a displace has written the plane since velocity was switched on

  Staging staging[STAGE_COUNT];       // the read_* queries' device staging

  // datum_ocean_reduce_bounds: the records, [cascades] x 32 bytes, and the workgroups' partials, both allocated by the first reduce
  float4 *bounds = nullptr;
  float4 *boundspartials = nullptr;
  int boundsgroups = 0;               // workgroups per cascade the partials were sized for
  bool boundscurrent = false;         // the records are those of the maps as they lie: set by reduce_bounds, cleared by displace, bind_maps and a release_memory that unbinds the maps

  // the ripple layer (datum_ocean_set_ripples): nothing is allocated while rippleR == 0
  int rippleR = 0;                    // cells per side, 0 = off
  double ripples = 0.0;               // cell side, metres
  int rippleox = 0, rippleoy = 0;     // the window's origin, cells
  GuardedPlane<float2> ripplestate[2];   // the two state buffers: R x R cells of (height, rate) on the layer's torus
  int ripplecurrent = 0;              // the state buffer the next sub-step reads
  int *ripplesrc = nullptr;           // pending deposits
  // datum_ocean_set_ripple_params; the defaults are the fp32 values that call would store (0.05 is no float: as the double 0.05 the
  // default sponge table was one no call could set again, an ulp off set_ripple_params(2, 0.05f, 8, 4)'s in some entries)
  double ripplec = 2.0, ripplegamma = (double)0.05f, ripplespongegamma = 4.0;
  int ripplesponge = 8;
  int rippledispersion = DATUM_OCEAN_RIPPLE_WAVE;   // datum_ocean_set_ripple_dispersion: the step's mode, and g of the DEEP one (9.81 as a float)
  double rippleg = (double)9.81f;

  // datum_ocean_reduce_ripple_bounds: one block, allocated by the first reduce after a set_ripples and freed with the layer, of a guard, the
  // workgroups' partials, a guard, the layer's record and a guard, 32 bytes each but the partials: the guards are filled with 0xCD bytes
  // once and never written again (a test reads them round the record's pointer)
  float4 *rippleboundsblock = nullptr;
  bool rippleboundscurrent = false;   // the record is that of the current state buffer: set by reduce_ripple_bounds, cleared by every call that writes a state buffer

  // wake foam (datum_ocean_set_ripple_foam): nothing is allocated while ripplefoam is null; freed with the layer
  GuardedPlane<float> ripplefoam;     // the plane: R x R coverage on the layer's torus
  float ripplefoamt1 = 0.04f, ripplefoamk1 = 10.0f, ripplefoamt2 = 0.5f, ripplefoamk2 = 2.0f, ripplefoamdecay = 0.5f;   // datum_ocean_set_ripple_foam_params

  // ripple walls (datum_ocean_set_ripple_walls): nothing is allocated while ripplewall is null; freed with the layer
  GuardedPlane<unsigned char> ripplewall;               // the plane: R x R bytes on the layer's torus, 1 = wall
  datum_ocean_ripple_wall *ripplewalllist = nullptr;    // the handle's copy of the records, on the device
  int ripplewallcount = 0;

  // the ripple bed (datum_ocean_set_ripple_bed): nothing is allocated while ripplebed is null; freed with the layer
  GuardedPlane<float> ripplebed;                        // the depth plane: R x R floats on the layer's torus, +0 = solid
  GuardedPlane<unsigned char> ripplesurf;               // the surf plane: R x R bytes, 0 .. DATUM_OCEAN_RIPPLE_SURF_LEVELS
  float *ripplebedmap = nullptr;                        // the handle's copy of the map, on the device
  datum_ocean_ripple_bed ripplebedparams = {};

  // ripple swell (datum_ocean_set_ripple_swell): nothing is allocated while rippleswell is null; freed with the layer
  RippleSwell rippleswell;                              // the forcing plane: R x R floats on the layer's torus, and its CURRENT mark

  hipEvent_t complete = nullptr;      // "rendercomplete"

  // imported from the renderer (Vulkan external memory / semaphores)
  struct ImportedMemory { hipExternalMemory_t memory; void *ptr; size_t bytes; };
  std::vector<ImportedMemory> importedmemory;
  std::vector<hipExternalSemaphore_t> importedsemaphores;

  ocean::Farm *farm = nullptr;        // the tile farm's communicator, stream and double-buffered payload (datum_ocean_farm_init)

  // profiling
  bool profiling = false;
  int profmax = 0;
  int profsteps = 0;
  int profstride = 1;
  int profgroups = 0;                 // launches per pass when the profile began: the layout of events
  long profcalls = 0;
  std::vector<hipEvent_t> events;     // 4 per sampled step

  std::string error;
};

namespace
{
  std::string g_error;   // errors without a handle

  int fail(datum_ocean_ctx *ctx, int code, char const *what)
  {
    char buf[512];

    if (code > 0)
      snprintf(buf, sizeof(buf), "%s: %s (hipError %d)", what, hipGetErrorString((hipError_t)code), code);
    else
      snprintf(buf, sizeof(buf), "%s (code %d)", what, code);

    (ctx ? ctx->error : g_error) = buf;

    (void)hipGetLastError();   // the runtime's sticky last-error must not leak into a later, unrelated call

    return code;
  }

  // a refusal a shared check words for the call it serves: the text is exactly name + text
  int fail(datum_ocean_ctx *ctx, int code, char const *name, char const *text)
  {
    std::string const head = name;

    return fail(ctx, code, (head + text).c_str());
  }

  #define HIPCHECK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(ctx, (int)e_, #call); } while(0)

  bool supported(int n)
  {
    return n == 64 || n == 128 || n == 256 || n == 512 || n == 1024 || n == 2048 || n == 4096;
  }

  size_t plane(datum_ocean_ctx const *ctx) { return (size_t)ctx->N * ctx->N; }

  // one cascade's block of the maps (ocean_layout.h: map_compact_a / map_compact_b are offsets into it)
  char *map_block(datum_ocean_ctx const *ctx, int cascade)
  {
    return reinterpret_cast<char*>(ctx->maps.get()) + (size_t)cascade * map_cascade_bytes(ctx->N);
  }

  StepArgs make_args(datum_ocean_ctx *ctx, int ndt, float const *dt, bool storephase = true)
  {
    StepArgs a;
    a.h0 = ctx->h0;
    a.h0h = ctx->h0half ? ctx->h0h : nullptr;
    a.phase = ctx->phase;
    a.qphase = ctx->qphase;
    a.spec = ctx->spec;
    a.maps = ctx->maps.get();
    a.tw = ctx->tw;
    a.omega = ctx->omega;
    a.ndt = ndt;
    a.storephase = storephase ? 1 : 0;
    a.cascades = ctx->cascades;
    a.first = 0;

    for(int i = 0; i < MAX_PENDING; ++i)
      a.dt[i] = (i < ndt) ? dt[i] : 0.0f;
    memcpy(a.casc, ctx->casc, sizeof(a.casc));
    return a;
  }

  // The maps streamed past the Infinity Cache instead of written through (ocean_kernels.hip: MAP_STORE_AUX_STREAM; 1024^2 and 2048^2 have both
  // forms) where the handle's working set -- h0 8 + phase 4 + work spectrum 16 (8: fp16) + maps 24 bytes per point and cascade -- is beyond
  // this.  The working set up to which writing the maps through wins: 1024^2 x 4 (218 MB) 82.4 k grids/s written through against 78.9 k
  // streamed, x 5 (272 MB) 72.4-74.0 against 72.1-72.5 k, x 6 (327 MB) 68.8 against 76.1 k; 2048^2 x 1 and the fp16 spectrum's x 4 / x 6
  // (185 / 277 MB) written through by 0-3 % (profiles/r06_store_policies.txt).  4096^2 always streams (one cascade is 0.9 GB); grids below
  // 1024^2 never do (sixteen cascades of 512^2 still fit).
  constexpr double MAPS_RESIDENT_BYTES = 300.0e6;

  bool maps_stream(int N, int cascades, bool half)
  {
    return N >= 4096 || (N >= 1024 && (double)cascades * N * N * ((half ? 20.0 : 28.0) + MAP_TEXEL_BYTES) > MAPS_RESIDENT_BYTES);
  }

  // Cascades per launch of the two passes (replaces the one dispatch per shader of ocean.cpp:769-789).  A handle whose working set is resident
  // in the Infinity Cache takes every cascade in one launch per pass.  Beyond it the maps are streamed (ocean_kernels.hip: MAP_STORE_AUX) and
  // what can stay in the cache from the row pass to the column pass -- and for h0 and the phase from step to step -- is h0 8 + phase 4 + work
  // spectrum 16 (8: fp16) bytes per point: the passes are launched group by group -- row(g), column(g), row(g + 1), ... on the same stream,
  // the work spectrum's slots reused from group to group -- with the largest group whose share of that fits: 8 cascades of 1024^2, 2 of 2048^2,
  // 1 of 4096^2; groups of equal size where the cascades allow it (twelve as 6 + 6).  Measured (profiles/r06_cascade_groups.txt): 1024^2 x 16
  // as 2 x 8 77.8 k grids/s against 66.7 k in one launch and 71.1 k as 4 x 4; x 12 as 2 x 6 80.6 k against 74.2 k; x 8 in one launch 82.6 k
  // against 78.3 k as 2 x 4; 2048^2 x 4 as 2 x 2 18.2 k against 16.0 k in one launch and 17.2 k as 4 x 1.
  constexpr double CASCADE_GROUP_BYTES = 240.0e6;

  // The kernels of a displace call and how many launches of them: the one place where the spectrum format, a phase outside [0, 2 pi), the map
  // store policy, the farm and the requested group are combined.  displace, debug_rowpass, the profile and the two getters all read this.
  struct StepPlan
  {
    PassKernel const *row = nullptr;
    PassKernel const *col = nullptr;
    int group = 0;                    // cascades per launch of either pass
    int groups = 0;                   // launches per pass
    bool streamed = false;            // the maps streamed past the Infinity Cache
    int writeback = 1;                // the row pass stores the phase once its dt list holds this many (ocean_writeback.h)
    bool quadrant = false;            // the row pass reads and stores the phase in the quadrant tables (ocean_quadrant.h)
  };

  // whether every cascade's phase is its quadrant table: the one condition under which the row pass takes the tables
  bool every_quadrant(datum_ocean_ctx const *ctx)
  {
    for(int c = 0; c < ctx->cascades; ++c)
    {
      if (!ctx->cstate[c].quadrant)
        return false;
    }

    return true;
  }

  // The phase written back once per this many steps' worth of dt's unless the caller sets an interval (datum_ocean_set_phase_writeback).
  // Measured, parent build and intervals 1 / 2 / 4 / 8 alternated on one device (profiles/phase_writeback_ab.txt, phase_writeback_kernel_trace.txt):
  // 1024^2 x 4 fp32 82.8-83.0 k grids/s without (interval 1: 82.8-83.1 k) against 84.5-84.7 / 85.0-85.5 / 85.4-85.8 k, its row pass 22.64-22.66 us
  // against 21.75-21.78 / 21.33-21.45 / 21.17-21.25 us over 2100 launches; 1024^2 x 16 81.5 k against 83.1 / 83.8-83.9 / 83.8-84.1 k.  The
  // longest interval wins where the row pass runs at its memory path's rate: the re-applied dt's (4.5 on average at 8) hide under it.  At
  // 4096^2 with h0 as halves, where a workgroup's arithmetic is exposed, one trace each had 4 ahead of 8 (row pass 79.8 ->
  // 72.4 against 74.3 us) and the step equal within the device's drift (5.8-6.1 k both, 5.3-5.9 k without): not resolved, one value for all sizes.
  constexpr int PHASE_WRITEBACK_EVERY = MAX_PENDING;

  StepPlan plan_step(datum_ocean_ctx const *ctx)
  {
    int const N = ctx->N, C = ctx->cascades;
    bool const beyond = maps_stream(N, C, ctx->half);

    StepPlan p;

    // streamed where the handle's own working set is beyond the cache, and -- round 6, profiles/r06_farm_standin.txt -- while a farm of several
    // ranks is initialised: the collective's gathered buffer competes for the same cache, and the step loses less under it with the maps out
    // of the way.  4096^2 has the streamed form only, the grids below 1024^2 the written-through one only.
    if (N >= 4096 || N < 1024)
      p.streamed = N >= 4096;
    else if (ctx->mappolicy != DATUM_OCEAN_MAPS_AUTO)
      p.streamed = ctx->mappolicy == DATUM_OCEAN_MAPS_STREAMED;
    else
      p.streamed = beyond || (ctx->farm && ctx->farm->world > 1);

    // in groups only where the maps are streamed BECAUSE the working set is beyond the cache
    int g = ctx->cascadegroup;

    if (g > 0)
      g = std::min(g, C);
    else if (!p.streamed || !beyond)
      g = C;
    else
    {
      g = (int)(CASCADE_GROUP_BYTES / ((double)plane(ctx) * ((ctx->h0half ? 8.0 : 12.0) + (ctx->half ? 8.0 : 16.0))));
      g = std::max(1, std::min(g, C));

      int const groups = (C + g - 1) / g;

      g = (C + groups - 1) / groups;
    }

    p.group = g;
    p.groups = (C + g - 1) / g;

    // a phase outside [0, 2 pi) in some cascade (uploaded so, or left there by a negative dt): for the whole call the row pass whose sin / cos
    // take any argument
    bool wild = false;

    for(int c = 0; c < C; ++c)
      wild = wild || ctx->cstate[c].wild;

    int const format = ctx->h0half ? DATUM_OCEAN_SPECTRUM_FP16_H0 : (ctx->half ? DATUM_OCEAN_SPECTRUM_FP16 : DATUM_OCEAN_SPECTRUM_FP32);

    // the phase from the quadrant tables where EVERY cascade's phase is its table (displace settles that first: settle_phase_store)
    p.quadrant = every_quadrant(ctx);

    p.row = &ctx->kernels.row[format][p.quadrant ? ROW_QUADRANT : (wild ? ROW_WILD : ROW_PLANE)];
    p.col = &ctx->kernels.col[ctx->half][p.streamed];

    p.writeback = ctx->writebackevery > 0 ? ctx->writebackevery : PHASE_WRITEBACK_EVERY;

    return p;
  }

  // every kernel a step can launch at resolution N: the one place that names their instantiations (datum_ocean_create configures each)
  template<int N>
  StepKernels step_kernels()
  {
    typedef RowCfg<N, false> R;
    typedef RowCfg<N, true> RH;
    typedef ColCfg<N> C;

    auto k = [](auto *kernel) { return reinterpret_cast<void const*>(kernel); };

    StepKernels t;

    t.row[DATUM_OCEAN_SPECTRUM_FP32][ROW_PLANE] = { k(&ocean_rowpass_kernel<N, false>), R::THREADS, R::LDS, R::GROUPS };
    t.row[DATUM_OCEAN_SPECTRUM_FP32][ROW_WILD] = { k(&ocean_rowpass_kernel<N, false, true>), R::THREADS, R::LDS, R::GROUPS };
    t.row[DATUM_OCEAN_SPECTRUM_FP32][ROW_QUADRANT] = { k(&ocean_rowpass_kernel<N, false, false, false, true>), R::THREADS, R::LDS, R::GROUPS };
    t.row[DATUM_OCEAN_SPECTRUM_FP16][ROW_PLANE] = { k(&ocean_rowpass_kernel<N, true>), RH::THREADS, RH::LDS, RH::GROUPS };
    t.row[DATUM_OCEAN_SPECTRUM_FP16][ROW_WILD] = { k(&ocean_rowpass_kernel<N, true, true>), RH::THREADS, RH::LDS, RH::GROUPS };
    t.row[DATUM_OCEAN_SPECTRUM_FP16][ROW_QUADRANT] = { k(&ocean_rowpass_kernel<N, true, false, false, true>), RH::THREADS, RH::LDS, RH::GROUPS };
    t.row[DATUM_OCEAN_SPECTRUM_FP16_H0][ROW_PLANE] = { k(&ocean_rowpass_kernel<N, true, false, true>), RH::THREADS, RH::LDS, RH::GROUPS };
    t.row[DATUM_OCEAN_SPECTRUM_FP16_H0][ROW_WILD] = { k(&ocean_rowpass_kernel<N, true, true, true>), RH::THREADS, RH::LDS, RH::GROUPS };
    t.row[DATUM_OCEAN_SPECTRUM_FP16_H0][ROW_QUADRANT] = { k(&ocean_rowpass_kernel<N, true, false, true, true>), RH::THREADS, RH::LDS, RH::GROUPS };

    t.col[0][0] = t.col[0][1] = { colpass_entry<N, false>(), C::THREADS, C::LDS, C::TILES, col_walks<N, false>() };
    t.col[1][0] = t.col[1][1] = { colpass_entry<N, true>(), C::THREADS, C::LDS, C::TILES, col_walks<N, true>() };

    if constexpr (col_has_stream_variant<N>())
    {
      t.col[0][1].kernel = colpass_entry<N, false, true>();
      t.col[1][1].kernel = colpass_entry<N, true, true>();
    }

    return t;
  }

  // One launch of a pass over the cascades [a.first, a.first + a.cascades): the kernel's work items per cascade times the cascades, one
  // workgroup each -- or, where its workgroups walk (the LDS of a 1024-thread tile fills a CU), one persistent workgroup per compute unit.
  // ev != nullptr: the dispatch itself carries a start and a stop event (hipExtLaunchKernel), so a sampled kernel is
  // timed from its first to its last workgroup without event packets between the kernels -- an hipEventRecord between
  // the two passes held the second one back until the first had drained (+4 us per kernel at 1024^2 x 4).
  hipError_t launch(datum_ocean_ctx const *ctx, PassKernel const &k, StepArgs &a, hipEvent_t *ev)
  {
    void *args[] = { &a };
    int const items = k.items * a.cascades;
    dim3 const grid(k.walks ? std::min(items, ctx->cus) : items);

    if (ev)
      return hipExtLaunchKernel(k.kernel, grid, dim3(k.threads), args, k.lds, ctx->stream, ev[0], ev[1], 0);

    return hipLaunchKernel(k.kernel, grid, dim3(k.threads), args, k.lds, ctx->stream);
  }

  #define DISPATCH_N(n, expr) \
    switch(n) { \
      case 64: { constexpr int NN = 64; expr; } break; \
      case 128: { constexpr int NN = 128; expr; } break; \
      case 256: { constexpr int NN = 256; expr; } break; \
      case 512: { constexpr int NN = 512; expr; } break; \
      case 1024: { constexpr int NN = 1024; expr; } break; \
      case 2048: { constexpr int NN = 2048; expr; } break; \
      case 4096: { constexpr int NN = 4096; expr; } break; \
    }

  // (re)build the dispersion quadrant tables of the cascades whose wave scale changed
  int ensure_omega(datum_ocean_ctx *ctx)
  {
    unsigned int dirty = 0;
    for(int c = 0; c < ctx->cascades; ++c)
      dirty |= (unsigned int)ctx->cstate[c].omegadirty << c;

    if (!dirty)
      return DATUM_OCEAN_OK;

    WaveScales ws;

    for(int c = 0; c < DATUM_OCEAN_MAX_CASCADES; ++c)
    {
      ws.v[c] = ctx->casc[c].wavescale;

      // dispersion grows with |k|: its maximum is the table corner |m - N/2| = |n - N/2| = N/2 (same fp32 formula)
      float kc = (6.2831855f * (0.5f * (float)ctx->N)) / ws.v[c];
      float k2 = kc * kc + kc * kc;
      ctx->cstate[c].omegamax = sqrtf((9.81f * sqrtf(k2)) * (1.0f + k2 / 136900.0f));
    }

    hipLaunchKernelGGL(ocean_omega_kernel, dim3(512), dim3(256), 0, ctx->stream, ctx->omega, ctx->N, ctx->cascades, ws, dirty);
    HIPCHECK(ctx, hipGetLastError());

    for(CascadeState &s : ctx->cstate)
      s.omegadirty = false;

    return DATUM_OCEAN_OK;
  }

  // The fused row pass advances the phase with a single conditional subtraction, exact only while
  // 0 <= phase < 2 pi and 0 <= dispersion * dt < 2 pi.  Anything else goes through the phase-only kernel.
  bool fusable(datum_ocean_ctx *ctx)
  {
    for(int c = 0; c < ctx->cascades; ++c)
    {
      if (ctx->cstate[c].wild)
        return false;

      for(float dt : ctx->pending)
      {
        if (!dt_fusable(dt, ctx->cstate[c].omegamax))
          return false;
      }
    }

    return true;
  }

  //|---------------------- where a cascade's phase lives (ocean_quadrant.h) ---
  // The stored phase of a cascade is its quadrant table while CascadeState::quadrant is set, the plane otherwise; both are behind the
  // handle's true phase by the same retained dt's (ocean_writeback.h), whose flush acts on whichever it is.

  // the cascades whose phase is their table, bit by bit (ocean_advance_kernel)
  unsigned int quadrant_mask(datum_ocean_ctx const *ctx)
  {
    unsigned int mask = 0;

    for(int c = 0; c < ctx->cascades; ++c)
      mask |= (unsigned int)ctx->cstate[c].quadrant << c;

    return mask;
  }

  // The plane of a cascade made current for a call that reads or copies it: table -> plane; the table stays the truth.  The caller has
  // flushed whatever its reader must see (flush_retained, flush_phase).
  int materialise(datum_ocean_ctx *ctx, int cascade)
  {
    if (!ctx->cstate[cascade].quadrant)
      return DATUM_OCEAN_OK;

    hipLaunchKernelGGL(ocean_phaseexpand_kernel, dim3(1024), dim3(256), 0, ctx->stream, ctx->qphase + cascade * quadrant_count(ctx->N), ctx->phase + cascade * plane(ctx), ctx->N);
    HIPCHECK(ctx, hipGetLastError());

    return DATUM_OCEAN_OK;
  }

  // ... and a cascade moved back to the plane for good: from here on the plane is the truth
  int leave_quadrant(datum_ocean_ctx *ctx, int cascade)
  {
    int rc = materialise(ctx, cascade);

    ctx->cstate[cascade].quadrant = false;

    return rc;
  }

  // A zero phase, what every state without an uploaded one starts from: both homes filled, and the table the truth unless the handle is
  // held to the plane
  int zero_phase(datum_ocean_ctx *ctx, int cascade)
  {
    HIPCHECK(ctx, hipMemsetAsync(ctx->phase + cascade * plane(ctx), 0, plane(ctx) * sizeof(float), ctx->stream));
    HIPCHECK(ctx, hipMemsetAsync(ctx->qphase + cascade * quadrant_count(ctx->N), 0, quadrant_count(ctx->N) * sizeof(float), ctx->stream));

    ctx->cstate[cascade].quadrant = ctx->phasestore == DATUM_OCEAN_PHASE_STORE_AUTO;

    return DATUM_OCEAN_OK;
  }

  // A phase that has just been written into a cascade's plane (an upload, an adopted parked state, a switch back to the automatic mode):
  // whether it leaves [0, 2 pi) -- `knownwild` < 0: looked for on the device -- and whether it is symmetric, one word and one read-back for
  // both; a symmetric one in range moves into the table.  Synchronises the stream.
  int inspect_phase(datum_ocean_ctx *ctx, int cascade, int knownwild, bool *wild)
  {
    size_t const P = plane(ctx);
    float const *phase = ctx->phase + cascade * P;
    bool const symmetry = ctx->phasestore == DATUM_OCEAN_PHASE_STORE_AUTO && knownwild <= 0;

    unsigned int flags = 0;

    ctx->cstate[cascade].quadrant = false;

    if (knownwild < 0 || symmetry)
    {
      HIPCHECK(ctx, hipMemsetAsync(ctx->absmax, 0, sizeof(unsigned int), ctx->stream));

      // phases outside [0, 2 pi) take the general fmod kernel: looked for on the device, where the array now is
      if (knownwild < 0)
        hipLaunchKernelGGL(ocean_phaserange_kernel, dim3(1024), dim3(256), 0, ctx->stream, phase, P, ctx->absmax);

      if (symmetry)
        hipLaunchKernelGGL(ocean_phasesymmetry_kernel, dim3(1024), dim3(256), 0, ctx->stream, phase, ctx->N, ctx->absmax);

      HIPCHECK(ctx, hipGetLastError());
      HIPCHECK(ctx, hipMemcpyAsync(&flags, ctx->absmax, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    }

    *wild = (knownwild < 0) ? (flags & 1u) != 0 : knownwild > 0;

    if (symmetry && !*wild && !(flags & 2u))
    {
      hipLaunchKernelGGL(ocean_phasecompact_kernel, dim3(512), dim3(256), 0, ctx->stream, phase, ctx->qphase + cascade * quadrant_count(ctx->N), ctx->N);
      HIPCHECK(ctx, hipGetLastError());

      ctx->cstate[cascade].quadrant = true;
    }

    return DATUM_OCEAN_OK;
  }

  // Before a row pass (displace, debug_rowpass): its kernel takes every cascade's phase from one kind of home.  The tables, where every
  // cascade's phase is its table, none is wild and nothing else reads the stored plane in every step (the literal dispatches, the velocity
  // passes); otherwise the symmetric cascades are expanded and the plane kernel runs, as in builds before the table.
  int settle_phase_store(datum_ocean_ctx *ctx)
  {
    bool tables = every_quadrant(ctx) && !ctx->literal && ctx->velocitymode == DATUM_OCEAN_VELOCITY_OFF;

    for(int c = 0; c < ctx->cascades; ++c)
      tables = tables && !ctx->cstate[c].wild;

    if (tables)
      return DATUM_OCEAN_OK;

    for(int c = 0; c < ctx->cascades; ++c)
    {
      int rc = leave_quadrant(ctx, c);
      if (rc != DATUM_OCEAN_OK)
        return rc;
    }

    return DATUM_OCEAN_OK;
  }

  // Store the phase the handle stands at: the dt's the last row pass applied without storing, through the phase-only kernel (the same
  // roundings).  Before anything reads the stored phase, replaces it, or changes what the retained dt's mean (a cascade's dispersion table).
  int flush_retained(datum_ocean_ctx *ctx)
  {
    if (ctx->writeback.retained == 0)
      return DATUM_OCEAN_OK;

    int rc = ensure_omega(ctx);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    PhaseWriteback::Launch const l = ctx->writeback.repeat();

    StepArgs a = make_args(ctx, l.ndt, l.dt);

    hipLaunchKernelGGL(ocean_advance_kernel, dim3(1024, ctx->cascades), dim3(256), 0, ctx->stream, a, ctx->N, quadrant_mask(ctx));
    HIPCHECK(ctx, hipGetLastError());

    ctx->writeback.clear();

    return DATUM_OCEAN_OK;
  }

  // flush queued updates that do not fit into one displace call (behind the retained ones, which come first in time)
  int flush_pending(datum_ocean_ctx *ctx, size_t keep)
  {
    if (ctx->pending.size() > keep)
    {
      int rc = flush_retained(ctx);
      if (rc == DATUM_OCEAN_OK)
        rc = ensure_omega(ctx);
      if (rc != DATUM_OCEAN_OK)
        return rc;
    }

    while (ctx->pending.size() > keep)
    {
      int n = (int)std::min<size_t>(MAX_PENDING, ctx->pending.size() - keep);

      StepArgs a = make_args(ctx, n, ctx->pending.data());

      // fmod keeps the sign of its first operand: a negative dt can leave phases below zero, which the
      // fused fast path must never see
      for(int i = 0; i < n; ++i)
      {
        if (!dt_keeps_range(ctx->pending[i]))
        {
          for(int c = 0; c < ctx->cascades; ++c)
            ctx->cstate[c].wild = true;
        }
      }

      dim3 grid(1024, ctx->cascades);
      hipLaunchKernelGGL(ocean_advance_kernel, grid, dim3(256), 0, ctx->stream, a, ctx->N, quadrant_mask(ctx));
      HIPCHECK(ctx, hipGetLastError());

      ctx->pending.erase(ctx->pending.begin(), ctx->pending.begin() + n);
    }

    return DATUM_OCEAN_OK;
  }

  // the stored phase brought up to every update the handle has been given: retained and queued
  int flush_phase(datum_ocean_ctx *ctx)
  {
    int rc = flush_retained(ctx);

    return (rc == DATUM_OCEAN_OK) ? flush_pending(ctx, 0) : rc;
  }

  // fp16 work spectrum: the power of two that brings the largest possible row sum under the largest half.
  // With mu = max |h0| (complex modulus): |h~| <= 2 mu, |h~[k] + conj(h~[-k])| <= 4 mu, |C| <= 8 mu, |D| <= 12 mu,
  // so no component after the row transform exceeds 12 N mu.  Typical values are ~ sqrt(N) times smaller and
  // still far above half's denormal range.
  int size_spectrum_scale(datum_ocean_ctx *ctx)
  {
    if (!ctx->half)
      return DATUM_OCEAN_OK;

    size_t const P = plane(ctx);

    for(int c = 0; c < ctx->cascades; ++c)
    {
      if (!ctx->cstate[c].scaledirty)
        continue;

      unsigned int bits = 0;

      HIPCHECK(ctx, hipMemsetAsync(ctx->absmax, 0, sizeof(unsigned int), ctx->stream));
      hipLaunchKernelGGL(ocean_absmax_kernel, dim3(1024), dim3(256), 0, ctx->stream, ctx->h0 + c * P, P, ctx->absmax);
      HIPCHECK(ctx, hipGetLastError());
      HIPCHECK(ctx, hipMemcpyAsync(&bits, ctx->absmax, sizeof(bits), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

      float m;
      memcpy(&m, &bits, sizeof(m));

      if (!(m < 3.0e38f))
        return fail(ctx, DATUM_OCEAN_EINVAL, "fp16 spectrum: h0 holds a NaN or an infinity");

      double const bound = 12.0 * ctx->N * (1.41421356 * (double)m);
      int e = (bound > 0) ? (int)std::floor(std::log2(60000.0 / bound)) : 0;

      // (the exponent follows max |h0| over the whole range in which 2^e and 2^-e are normal floats with room to spare: a
      // sea 2^-40 times smaller than the example's must not land in half's denormals.  Round 3 clamped at +-24.)
      e = e > 100 ? 100 : (e < -100 ? -100 : e);

      ctx->casc[c].specscale = std::ldexp(1.0f, e);
      ctx->casc[c].specinv = std::ldexp(1.0f, -e);
      ctx->casc[c].rowscale = ctx->casc[c].specscale;

      if (ctx->h0half)
      {
        // h0 as halves: the power of two that brings the largest component just under 2^15 (the whole of half's range below it is
        // h0's: 2^-29 of the largest value is still a normal half, 2^-39 a denormal one); the row pass takes it out again with the
        // work spectrum's scale in one exact factor
        int eh = (m > 0) ? (int)std::floor(std::log2(32768.0 / (double)m)) : 0;

        if (m > 0 && std::ldexp((double)m, eh) >= 32768.0)
          eh -= 1;

        eh = eh > 120 ? 120 : (eh < -120 ? -120 : eh);

        hipLaunchKernelGGL(ocean_h0half_kernel, dim3(2048), dim3(256), 0, ctx->stream, ctx->h0 + c * P, ctx->h0h + c * P, P, std::ldexp(1.0f, eh));
        HIPCHECK(ctx, hipGetLastError());

        ctx->casc[c].rowscale = std::ldexp(1.0f, e - eh);
      }

      ctx->cstate[c].scaledirty = false;
    }

    return DATUM_OCEAN_OK;
  }

  int ensure_scratch(datum_ocean_ctx *ctx)
  {
    if (!ctx->scratch)
      HIPCHECK(ctx, hipMalloc(&ctx->scratch, 3 * plane(ctx) * sizeof(cf)));

    return DATUM_OCEAN_OK;
  }

  // the pack of datum_ocean_pack_displacement / datum_ocean_farm_gather, on the handle's stream (arguments checked by the callers)
  int pack_into(datum_ocean_ctx *ctx, int format, void *payload_device, size_t need)
  {
    if (format == DATUM_OCEAN_PAYLOAD_MAPS)
    {
      // the map block as it lies in memory (device layout), so that the producer may go on writing its own buffer
      HIPCHECK(ctx, hipMemcpyAsync(payload_device, ctx->maps.get(), need, hipMemcpyDeviceToDevice, ctx->stream));
    }
    else
    {
      int const blocks = std::min<size_t>((size_t)ctx->cus * 8, ((size_t)ctx->cascades * plane(ctx) / 4 + 255) / 256);

      PackShape const sh = pack_shape(ctx->N);

      if (format == DATUM_OCEAN_PAYLOAD_XYZ16)
        hipLaunchKernelGGL(ocean_pack_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, ctx->maps.get(), ctx->N, ctx->cascades, payload_device, sh);
      else
        hipLaunchKernelGGL(ocean_pack_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, ctx->maps.get(), ctx->N, ctx->cascades, payload_device, sh);

      HIPCHECK(ctx, hipGetLastError());
    }

    return DATUM_OCEAN_OK;
  }

  size_t foam_bytes(datum_ocean_ctx const *ctx) { return (size_t)ctx->cascades * plane(ctx) * sizeof(float); }

  // zero one cascade's foam plane (-1: all of them), on the handle's stream
  int zero_foam(datum_ocean_ctx *ctx, int cascade)
  {
    size_t const P = plane(ctx);

    if (cascade < 0)
      HIPCHECK(ctx, hipMemsetAsync(ctx->foam.get(), 0, foam_bytes(ctx), ctx->stream));
    else
      HIPCHECK(ctx, hipMemsetAsync(ctx->foam.get() + cascade * P, 0, P * sizeof(float), ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // a new state in the cascade (CascadeState::new_state) starts without foam: its accumulator is zeroed, on the handle's stream
  int new_state_foam(datum_ocean_ctx *ctx, int cascade)
  {
    return (ctx->foammode == DATUM_OCEAN_FOAM_ACCUMULATE) ? zero_foam(ctx, cascade) : DATUM_OCEAN_OK;
  }

  // datum_ocean_bind_maps, datum_ocean_bind_foam: the size and alignment checks, then the drain (nullptr: the handle's own plane again)
  template<typename T>
  int bind_plane(datum_ocean_ctx *ctx, BindablePlane<T> &target, void *device_ptr, size_t bytes, size_t need, char const *too_small, char const *unaligned)
  {
    if (device_ptr && bytes < need)
      return fail(ctx, DATUM_OCEAN_EINVAL, too_small);

    if (device_ptr && ((uintptr_t)device_ptr & 15))
      return fail(ctx, DATUM_OCEAN_EINVAL, unaligned);

    HIPCHECK(ctx, hipSetDevice(ctx->device));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

    target.bound = static_cast<T*>(device_ptr);

    return DATUM_OCEAN_OK;
  }

  // the literal mode's step for the cascades [first, first + count): the reference's five dispatches, cascade by cascade (ocean.cpp:769-789),
  // after the general kernel advanced the phase
  int launch_literals(datum_ocean_ctx *ctx, int first, int count)
  {
    size_t const P = plane(ctx);

    for(int c = first; c < first + count; ++c)
    {
      LiteralArgs a;
      a.h0 = ctx->h0 + c * P;
      a.phase = ctx->phase + c * P;
      a.h = ctx->litfields;
      a.hx = ctx->litfields + P;
      a.hy = ctx->litfields + 2 * P;
      a.weights = ctx->litweights;
      a.maps = map_block(ctx, c);
      a.N = ctx->N;
      a.scale = ctx->casc[c].scale;
      a.choppiness = ctx->casc[c].choppiness;

      HIPCHECK(ctx, launch_literal(a, ctx->stream));
    }

    return DATUM_OCEAN_OK;
  }

  // the foam plane for the cascades [first, first + count), read from the maps the column pass (or the literal dispatches) just wrote;
  // written through or streamed as the plan stores the maps
  int launch_foam(datum_ocean_ctx *ctx, FoamArgs &fa, int first, int count, bool streamed)
  {
    fa.first = first;

    void *args[] = { &fa };
    int tiles = 0;

    DISPATCH_N(ctx->N, tiles = foam_tiles<NN>());

    bool const accum = ctx->foammode == DATUM_OCEAN_FOAM_ACCUMULATE;

    HIPCHECK(ctx, hipLaunchKernel(ctx->foamkernels.k[accum][streamed], dim3(tiles, count), dim3(FOAM_THREADS), args, 0, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // the arguments of a displace call's foam launches; consumes the dt accumulated since the last displace
  FoamArgs foam_args(datum_ocean_ctx *ctx)
  {
    FoamArgs fa = {};
    fa.maps = ctx->maps.get();
    fa.foam = ctx->foam.get();

    double const dt = ctx->foamdt;

    for(int c = 0; c < ctx->cascades; ++c)
    {
      FoamCascade &f = fa.casc[c];
      f.inv2h = (float)((double)ctx->N / (2.0 * (double)ctx->casc[c].wavescale));
      f.threshold = ctx->cstate[c].foamthreshold;
      f.gain = ctx->cstate[c].foamgain;
      f.fade = (float)std::min(1.0, std::exp(-(double)ctx->cstate[c].foamdecay * dt));
    }

    return fa;
  }

  size_t velocity_bytes(datum_ocean_ctx const *ctx) { return (size_t)ctx->cascades * plane(ctx) * sizeof(float4); }

  // the velocity passes' work buffer, sized for `group` cascades (grown where the cascade group has grown since velocity was switched on)
  int ensure_velocity_work(datum_ocean_ctx *ctx, int group)
  {
    if (ctx->velocitywork && ctx->velocityworkgroup >= group)
      return DATUM_OCEAN_OK;

    if (ctx->velocitywork)
    {
      HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
      HIPCHECK(ctx, hipFree(ctx->velocitywork));
      ctx->velocitywork = nullptr;
      ctx->velocityworkgroup = 0;
    }

    HIPCHECK(ctx, hipMalloc(&ctx->velocitywork, (size_t)group * 3 * plane(ctx) * sizeof(cf)));
    ctx->velocityworkgroup = group;

    return DATUM_OCEAN_OK;
  }

  // the arguments of a displace call's velocity launches: the stored phase is behind the step's by the dt's its row pass did not store
  VelocityArgs velocity_args(datum_ocean_ctx *ctx, PhaseWriteback::Launch const &step)
  {
    VelocityArgs va = {};
    va.h0 = ctx->h0;
    va.phase = ctx->phase;
    va.omega = ctx->omega;
    va.tw = ctx->tw;
    va.work = ctx->velocitywork;
    va.vel = ctx->velocity.get();
    va.ndt = step.store ? 0 : step.ndt;

    for(int c = 0; c < ctx->cascades; ++c)
      va.wild = va.wild || ctx->cstate[c].wild;

    for(int i = 0; i < MAX_PENDING; ++i)
      va.dt[i] = (i < va.ndt) ? step.dt[i] : 0.0f;

    memcpy(va.casc, ctx->casc, sizeof(va.casc));

    return va;
  }

  // the velocity plane of the cascades [first, first + count): column pass, then row pass, on the handle's stream behind the group's step
  int launch_velocity(datum_ocean_ctx *ctx, VelocityArgs &va, int first, int count, bool streamed)
  {
    va.first = first;

    void *args[] = { &va };
    VelocityKernels const &k = ctx->velocitykernels;

    HIPCHECK(ctx, hipLaunchKernel(k.col, dim3(k.coltiles, count), dim3(k.colthreads), args, k.collds, ctx->stream));
    HIPCHECK(ctx, hipLaunchKernel(k.row[streamed], dim3(k.rowgroups, count), dim3(k.rowthreads), args, k.rowlds, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // an ncclResult_t never leaves the module
  int fail_comm(datum_ocean_ctx *ctx, ocean::RcclApi *api, ncclComm_t comm, ncclResult_t r, char const *what)
  {
    char buf[768];

    char const *last = (api && api->GetLastError) ? api->GetLastError(comm) : "";

    snprintf(buf, sizeof(buf), "%s: %s (ncclResult %d)%s%s", what, (api && api->GetErrorString) ? api->GetErrorString(r) : "?", (int)r, (last && *last) ? ": " : "", (last && *last) ? last : "");

    (ctx ? ctx->error : g_error) = buf;

    // a communicator that failed is not destroyed (ncclCommDestroy waits for its outstanding operations) but aborted: farm_teardown
    if (ctx && ctx->farm && comm && comm == ctx->farm->comm)
      ctx->farm->failed = true;

    return DATUM_OCEAN_ECOMM;
  }

  #define RCCLCHECK(ctx, api, comm, call) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) return fail_comm(ctx, api, comm, r_, #call); } while(0)

  void farm_teardown(datum_ocean_ctx *ctx)
  {
    ocean::Farm *f = ctx->farm;

    if (!f)
      return;

    if (f->stream && !f->failed)
      (void)hipStreamSynchronize(f->stream);

    if (f->comm && f->api)
    {
      if (f->failed && f->api->CommAbort)
        (void)f->api->CommAbort(f->comm);
      else
        (void)f->api->CommDestroy(f->comm);
    }

    if (f->stream && f->failed)
      (void)hipStreamSynchronize(f->stream);

    for(auto &sl : f->slots)
    {
      (void)hipFree(sl.payload);
      (void)hipFree(sl.gathered);

      for(hipEvent_t e : { sl.packed, sl.start, sl.done, sl.consumed })
        if (e)
          (void)hipEventDestroy(e);
    }

    if (f->stream)
      (void)hipStreamDestroy(f->stream);

    // datum_ocean_farm_partition had confined the handle's own stream to the compute units the collective left it: all of them again
    if (f->commcus && ctx->ownstream)
    {
      hipStream_t whole = nullptr;

      (void)hipStreamSynchronize(ctx->ownstream);

      if (hipStreamCreateWithFlags(&whole, hipStreamNonBlocking) == hipSuccess)
      {
        bool const onown = ctx->stream == ctx->ownstream;

        (void)hipStreamDestroy(ctx->ownstream);
        ctx->ownstream = whole;

        if (onown)
          ctx->stream = whole;
      }
    }

    delete f;

    ctx->farm = nullptr;
  }
}

extern "C"
{

int datum_ocean_create(datum_ocean_t *out, int device, int resolution, int cascades)
{
  if (!out)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_create: null out pointer");

  *out = nullptr;

  if (!supported(resolution))
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_create: resolution must be a power of two in [64, 4096]");

  if (cascades < 1 || cascades > DATUM_OCEAN_MAX_CASCADES)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_create: cascades out of range");

  HIPCHECK(nullptr, hipSetDevice(device));

  datum_ocean_ctx *ctx = new (std::nothrow) datum_ocean_ctx;
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_ENOMEM, "datum_ocean_create: out of host memory");

  ctx->device = device;
  ctx->N = resolution;
  ctx->cascades = cascades;

  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1)
      cus = 256;
    ctx->cus = cus;
  }

  size_t const P = plane(ctx);

  #define CREATECHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { int rc_ = fail(nullptr, (int)e_, #call); datum_ocean_destroy(ctx); return rc_; } } while(0)

  CREATECHECK(hipStreamCreateWithFlags(&ctx->ownstream, hipStreamNonBlocking));
  ctx->stream = ctx->ownstream;

  CREATECHECK(hipMalloc(&ctx->h0, cascades * P * sizeof(float2)));
  CREATECHECK(hipMalloc(&ctx->phase, cascades * P * sizeof(float)));
  CREATECHECK(hipMalloc(&ctx->qphase, cascades * quadrant_count(resolution) * sizeof(float)));
  CREATECHECK(hipMalloc(&ctx->spec, cascades * P * sizeof(cd)));
  CREATECHECK(hipMalloc(&ctx->absmax, sizeof(unsigned int)));
  CREATECHECK(hipMalloc(&ctx->maps.own, cascades * map_cascade_bytes(resolution)));
  CREATECHECK(hipMalloc(&ctx->tw, resolution * sizeof(cf)));
  CREATECHECK(hipMalloc(&ctx->omega, (size_t)cascades * (resolution / 2 + 1) * (resolution / 2 + 1) * sizeof(float)));

  CREATECHECK(hipMemsetAsync(ctx->h0, 0, cascades * P * sizeof(float2), ctx->stream));
  CREATECHECK(hipMemsetAsync(ctx->phase, 0, cascades * P * sizeof(float), ctx->stream));
  CREATECHECK(hipMemsetAsync(ctx->qphase, 0, cascades * quadrant_count(resolution) * sizeof(float), ctx->stream));

  // (a zero phase is symmetric: every cascade starts in its table)
  for(int c = 0; c < cascades; ++c)
    ctx->cstate[c].quadrant = true;
  CREATECHECK(hipMemsetAsync(ctx->maps.own, 0, cascades * map_cascade_bytes(resolution), ctx->stream));

  // exp(+2 pi i k / N), rounded once from double (the reference's table -- ocean.cpp:686-700 -- is per
  // lane and stage and evaluated at unreduced fp32 angles; see datum_ocean_reference_weights)
  std::vector<cf> tw(resolution);
  for(int k = 0; k < resolution; ++k)
  {
    double ang = 2.0 * 3.14159265358979323846 * k / resolution;
    tw[k] = cf{ (float)std::cos(ang), (float)std::sin(ang) };
  }
  // exact values on the axes and diagonals
  tw[0] = cf{ 1.0f, 0.0f };
  tw[resolution/4] = cf{ 0.0f, 1.0f };
  tw[resolution/2] = cf{ -1.0f, 0.0f };
  tw[3*resolution/4] = cf{ 0.0f, -1.0f };

  CREATECHECK(hipMemcpy(ctx->tw, tw.data(), resolution * sizeof(cf), hipMemcpyHostToDevice));

  for(int c = 0; c < DATUM_OCEAN_MAX_CASCADES; ++c)
  {
    // OceanParams defaults (ocean.h:60,64)
    ctx->casc[c].wavescale = 64.0f;
    ctx->casc[c].scale = 1 / 64.0f;
    ctx->casc[c].choppiness = 1.35f;
    ctx->casc[c].nz = 4 / (ctx->casc[c].scale * resolution);
    ctx->casc[c].specscale = 1.0f;
    ctx->casc[c].specinv = 1.0f;
    ctx->casc[c].rowscale = 1.0f;
  }

  DISPATCH_N(resolution, ctx->foamkernels = foam_kernels<NN>());

  // the LDS limit of every kernel in the table: a kernel the module launches is one it configured
  DISPATCH_N(resolution, ctx->kernels = step_kernels<NN>());

  for(auto const &format : ctx->kernels.row)
    for(PassKernel const &k : format)
      CREATECHECK(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));

  for(auto const &half : ctx->kernels.col)
    for(PassKernel const &k : half)
      CREATECHECK(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));

  CREATECHECK(hipStreamSynchronize(ctx->stream));

  #undef CREATECHECK

  *out = ctx;

  return DATUM_OCEAN_OK;
}

int datum_ocean_destroy(datum_ocean_t ctx)
{
  if (!ctx)
    return DATUM_OCEAN_OK;

  (void)hipSetDevice(ctx->device);

  if (ctx->stream)
    (void)hipStreamSynchronize(ctx->stream);

  farm_teardown(ctx);

  for(hipEvent_t e : ctx->events)
    (void)hipEventDestroy(e);

  if (ctx->complete)
    (void)hipEventDestroy(ctx->complete);

  for(auto &im : ctx->importedmemory)
    (void)hipDestroyExternalMemory(im.memory);

  for(hipExternalSemaphore_t sem : ctx->importedsemaphores)
    (void)hipDestroyExternalSemaphore(sem);

  (void)hipFree(ctx->h0);
  (void)hipFree(ctx->seed);
  (void)hipFree(ctx->phase);
  (void)hipFree(ctx->qphase);
  (void)hipFree(ctx->spec);
  (void)hipFree(ctx->absmax);
  (void)hipFree(ctx->h0h);
  (void)hipFree(ctx->maps.own);
  (void)hipFree(ctx->tw);
  (void)hipFree(ctx->omega);
  (void)hipFree(ctx->litfields);
  (void)hipFree(ctx->litweights);
  (void)hipFree(ctx->scratch);
  (void)hipFree(ctx->foam.own);
  (void)hipFree(ctx->velocity.own);
  (void)hipFree(ctx->velocitywork);
  (void)ctx->ripplestate[0].release();
  (void)ctx->ripplestate[1].release();
  (void)hipFree(ctx->ripplesrc);
  (void)hipFree(ctx->rippleboundsblock);
  (void)ctx->ripplefoam.release();
  (void)ctx->ripplewall.release();
  (void)hipFree(ctx->ripplewalllist);
  (void)ctx->ripplebed.release();
  (void)ctx->ripplesurf.release();
  (void)hipFree(ctx->ripplebedmap);
  (void)ctx->rippleswell.off();

  for(Staging &st : ctx->staging)
    (void)hipFree(st.ptr);

  (void)hipFree(ctx->bounds);
  (void)hipFree(ctx->boundspartials);

  if (ctx->ownstream)
    (void)hipStreamDestroy(ctx->ownstream);

  delete ctx;

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_stream(datum_ocean_t ctx, void *hip_stream, int use_own)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_stream: null handle");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  ctx->stream = use_own ? ctx->ownstream : (hipStream_t)hip_stream;

  return DATUM_OCEAN_OK;
}

int datum_ocean_bind_maps(datum_ocean_t ctx, void *device_ptr, size_t bytes)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_bind_maps: null handle");

  int const rc = bind_plane(ctx, ctx->maps, device_ptr, bytes, ctx->cascades * map_cascade_bytes(ctx->N),
                            "datum_ocean_bind_maps: buffer smaller than cascades * N * N * texel_bytes (datum_ocean_map_layout)", "datum_ocean_bind_maps: buffer must be 16-byte aligned");

  // other maps: the bounds records (datum_ocean_reduce_bounds) are no longer theirs
  if (rc == DATUM_OCEAN_OK)
    ctx->boundscurrent = false;

  return rc;
}

int datum_ocean_maps_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes)
{
  if (!ctx || !device_ptr)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_maps_device: null argument");

  *device_ptr = ctx->maps.get();

  if (bytes)
    *bytes = ctx->cascades * map_cascade_bytes(ctx->N);

  return DATUM_OCEAN_OK;
}

int datum_ocean_map_layout(int resolution, int *group_cols, int *group_rows, int *band, int *texel_bytes)
{
  if (!supported(resolution) || !group_cols || !group_rows || !band || !texel_bytes)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_map_layout: bad argument");

  *group_cols = map_patch_cols(resolution);
  *group_rows = map_patch_rows(resolution);
  *band = band_cols(resolution);
  *texel_bytes = MAP_TEXEL_BYTES;

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_cascade(datum_ocean_t ctx, int cascade, float wavescale, float choppiness)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_cascade: null handle");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_cascade: cascade out of range");

  if (!(wavescale > 0))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_cascade: wavescale must be positive");

  // queued updates, and those a row pass applied without storing the phase, were issued under the old wavescale: apply them first, while
  // the dispersion table is still the old one
  if (wavescale != ctx->casc[cascade].wavescale && (!ctx->pending.empty() || ctx->writeback.retained > 0))
  {
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    int rc = flush_phase(ctx);
    if (rc != DATUM_OCEAN_OK)
      return rc;
  }

  CascadeConst &cc = ctx->casc[cascade];

  if (cc.wavescale != wavescale)
    ctx->cstate[cascade].omegadirty = true;

  cc.wavescale = wavescale;
  cc.scale = 1 / wavescale;                      // ocean.cpp:743
  cc.choppiness = choppiness;                    // ocean.cpp:744
  cc.nz = 4 / (cc.scale * ctx->N);               // ocean.map.comp:77

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_spectrum_format(datum_ocean_t ctx, int format)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_spectrum_format: null handle");

  if (format != DATUM_OCEAN_SPECTRUM_FP32 && format != DATUM_OCEAN_SPECTRUM_FP16 && format != DATUM_OCEAN_SPECTRUM_FP16_H0)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_spectrum_format: unknown format");

  if (ctx->profiling)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_spectrum_format: a profile is open (the format can change the cascade groups its samples are per)");

  if (format != DATUM_OCEAN_SPECTRUM_FP32 && ctx->literal)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_spectrum_format: the handle is in the literal mode (the reference's fp32 arithmetic); switch it off first");

  if (format == DATUM_OCEAN_SPECTRUM_FP16_H0 && !ctx->h0h)
  {
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    HIPCHECK(ctx, hipMalloc(&ctx->h0h, (size_t)ctx->cascades * plane(ctx) * sizeof(unsigned int)));
  }

  ctx->half = (format != DATUM_OCEAN_SPECTRUM_FP32);
  ctx->h0half = (format == DATUM_OCEAN_SPECTRUM_FP16_H0);

  for(int c = 0; c < ctx->cascades; ++c)
  {
    ctx->cstate[c].scaledirty = ctx->half;

    if (!ctx->half)
      ctx->casc[c].specscale = ctx->casc[c].specinv = ctx->casc[c].rowscale = 1.0f;
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_upload_state(datum_ocean_t ctx, int cascade, float const *h0, float const *phase)
{
  if (!ctx || !h0)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_upload_state: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_upload_state: cascade out of range");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  // the new state replaces the old one: updates queued against the old state (or applied to it and not stored) are applied first so that
  // the other cascades keep them
  int rc = flush_phase(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  size_t const P = plane(ctx);

  HIPCHECK(ctx, hipMemcpyAsync(ctx->h0 + cascade * P, h0, P * sizeof(float2), hipMemcpyHostToDevice, ctx->stream));

  bool wild = false;

  if (phase)
  {
    HIPCHECK(ctx, hipMemcpyAsync(ctx->phase + cascade * P, phase, P * sizeof(float), hipMemcpyHostToDevice, ctx->stream));

    rc = inspect_phase(ctx, cascade, -1, &wild);
  }
  else
    rc = zero_phase(ctx, cascade);

  if (rc == DATUM_OCEAN_OK)
    rc = new_state_foam(ctx, cascade);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));   // the host buffers are the caller's again

  ctx->cstate[cascade].new_state(wild);

  return DATUM_OCEAN_OK;
}

int datum_ocean_upload_height(datum_ocean_t ctx, int cascade, float const *h0)
{
  if (!ctx || !h0)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_upload_height: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_upload_height: cascade out of range");

  if (!ctx->cstate[cascade].uploaded)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_upload_height: the cascade holds no state (datum_ocean_upload_state)");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  size_t const P = plane(ctx);

  HIPCHECK(ctx, hipMemcpyAsync(ctx->h0 + cascade * P, h0, P * sizeof(float2), hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));   // the host buffer is the caller's again

  ctx->cstate[cascade].new_height();

  return DATUM_OCEAN_OK;
}

int datum_ocean_upload_seed(datum_ocean_t ctx, int cascade, float const *seed)
{
  if (!ctx || !seed)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_upload_seed: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_upload_seed: cascade out of range");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  size_t const P = plane(ctx);

  if (!ctx->seed)
  {
    HIPCHECK(ctx, hipMalloc(&ctx->seed, ctx->cascades * P * sizeof(float2)));
    HIPCHECK(ctx, hipMemsetAsync(ctx->seed, 0, ctx->cascades * P * sizeof(float2), ctx->stream));
  }

  HIPCHECK(ctx, hipMemcpyAsync(ctx->seed + cascade * P, seed, P * sizeof(float2), hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_rebuild_height(datum_ocean_t ctx, int cascade, float wavescale, float waveamplitude, float windspeed, float windx, float windy)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_rebuild_height: null handle");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_rebuild_height: cascade out of range");

  if (!ctx->seed)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_rebuild_height: no seed on the device (datum_ocean_upload_seed)");

  if (!(wavescale > 0))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_rebuild_height: wavescale must be positive");

  // refused before anything is installed: such arguments make every h0 a NaN (include/datum_ocean_hip.h)
  if (!(waveamplitude >= 0) || !std::isfinite(waveamplitude))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_rebuild_height: waveamplitude must be finite and not negative");

  if (!std::isfinite(windspeed) || !std::isfinite(windx) || !std::isfinite(windy))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_rebuild_height: windspeed and the wind direction must be finite");

  // queued updates belong to the old wave scale
  int rc = datum_ocean_set_cascade(ctx, cascade, wavescale, ctx->casc[cascade].choppiness);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  size_t const P = plane(ctx);

  hipLaunchKernelGGL(ocean_height_kernel, dim3(1024), dim3(256), 0, ctx->stream, ctx->seed + cascade * P, ctx->h0 + cascade * P, ctx->N, wavescale, waveamplitude, windspeed, windx, windy);
  ctx->cstate[cascade].new_height();
  HIPCHECK(ctx, hipGetLastError());

  // a cascade without a state gets one with phase zero -- its foam accumulator is not reset (include/datum_ocean_hip.h).  The phase is
  // replaced: like upload_state and resume_state the call brings it up to date first, so that the new state takes none of the updates
  // queued before it (set_cascade above has done so only where the wave scale changed) and the other cascades keep them
  if (!ctx->cstate[cascade].uploaded)
  {
    rc = flush_phase(ctx);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    rc = zero_phase(ctx, cascade);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    ctx->cstate[cascade].new_state(false);
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_height(datum_ocean_t ctx, int cascade, float *h0)
{
  if (!ctx || !h0)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_height: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_height: cascade out of range");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  size_t const P = plane(ctx);

  HIPCHECK(ctx, hipMemcpyAsync(h0, ctx->h0 + cascade * P, P * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_state(datum_ocean_t ctx, int cascade, float *phase)
{
  if (!ctx || !phase)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_state: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_state: cascade out of range");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  int rc = flush_phase(ctx);
  if (rc == DATUM_OCEAN_OK)
    rc = materialise(ctx, cascade);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  size_t const P = plane(ctx);

  HIPCHECK(ctx, hipMemcpyAsync(phase, ctx->phase + cascade * P, P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

size_t datum_ocean_state_bytes(int resolution)
{
  return (size_t)resolution * resolution * (sizeof(float2) + sizeof(float));
}

int datum_ocean_park_state(datum_ocean_t ctx, int cascade, void *device_dst, size_t bytes, int *flags)
{
  if (!ctx || !device_dst || !flags)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_park_state: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_park_state: cascade out of range");

  if (bytes != datum_ocean_state_bytes(ctx->N))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_park_state: buffer must be datum_ocean_state_bytes()");

  if (!ctx->cstate[cascade].uploaded)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_park_state: the cascade holds no state");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  int rc = flush_phase(ctx);
  if (rc == DATUM_OCEAN_OK)
    rc = materialise(ctx, cascade);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  size_t const P = plane(ctx);

  HIPCHECK(ctx, hipMemcpyAsync(device_dst, ctx->h0 + cascade * P, P * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHECK(ctx, hipMemcpyAsync(static_cast<char*>(device_dst) + P * sizeof(float2), ctx->phase + cascade * P, P * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));

  *flags = ctx->cstate[cascade].wild ? 1 : 0;

  return DATUM_OCEAN_OK;
}

int datum_ocean_resume_state(datum_ocean_t ctx, int cascade, void const *device_src, size_t bytes, int flags)
{
  if (!ctx || !device_src)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_resume_state: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_resume_state: cascade out of range");

  if (bytes != datum_ocean_state_bytes(ctx->N))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_resume_state: buffer must be datum_ocean_state_bytes()");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  // updates queued against the state that is being replaced, or applied to it and not stored, are applied first (the other cascades keep them)
  int rc = flush_phase(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  size_t const P = plane(ctx);

  HIPCHECK(ctx, hipMemcpyAsync(ctx->h0 + cascade * P, device_src, P * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->phase + cascade * P, static_cast<char const*>(device_src) + P * sizeof(float2), P * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));

  // (the range is the flag's word; whether the adopted phase is symmetric is looked for on the device: one read-back)
  bool wild = false;

  rc = inspect_phase(ctx, cascade, (flags & 1) ? 1 : 0, &wild);

  if (rc == DATUM_OCEAN_OK)
    rc = new_state_foam(ctx, cascade);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  ctx->cstate[cascade].new_state(wild);

  return DATUM_OCEAN_OK;
}

int datum_ocean_update(datum_ocean_t ctx, float dt)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_update: null handle");

  ctx->pending.push_back(dt);
  ctx->foamdt += (double)dt;

  if (ctx->pending.size() > 4 * MAX_PENDING)
  {
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    return flush_pending(ctx, MAX_PENDING);
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_displace(datum_ocean_t ctx)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_displace: null handle");

  for(int c = 0; c < ctx->cascades; ++c)
    if (!ctx->cstate[c].uploaded)
      return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_displace: a cascade has no state (datum_ocean_upload_state)");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  int rc = DATUM_OCEAN_OK;

  // What the row pass cannot take goes through the phase-only kernel first, which stores: everything in the literal mode (its dispatches
  // read the stored phase) and where a queued dt or a phase is outside the fused advance's range; otherwise the oldest of more than
  // MAX_PENDING -- the retained dt's, which the row pass would have to apply in front of the queued ones, first
  if (ctx->literal)
    rc = flush_phase(ctx);
  else if (!ctx->pending.empty())
  {
    rc = ensure_omega(ctx);

    if (rc == DATUM_OCEAN_OK)
      rc = fusable(ctx) ? flush_pending(ctx, MAX_PENDING) : flush_phase(ctx);

    if (rc == DATUM_OCEAN_OK && !ctx->writeback.fits((int)ctx->pending.size()))
      rc = flush_retained(ctx);
  }

  if (rc != DATUM_OCEAN_OK)
    return rc;

  rc = size_spectrum_scale(ctx);
  if (rc == DATUM_OCEAN_OK)
    rc = settle_phase_store(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  StepPlan plan = plan_step(ctx);

  // the literal mode -- an fp32 spectrum, no update queued, no profile open -- as one group of every cascade
  if (ctx->literal)
  {
    plan.group = ctx->cascades;
    plan.groups = 1;
  }

  bool const velocity = ctx->velocitymode != DATUM_OCEAN_VELOCITY_OFF;

  // (the velocity column pass multiplies by the dispersion even where no update is queued)
  if (velocity)
  {
    rc = ensure_omega(ctx);
    if (rc == DATUM_OCEAN_OK)
      rc = ensure_velocity_work(ctx, plan.group);
    if (rc != DATUM_OCEAN_OK)
      return rc;
  }

  bool const sampling = ctx->profiling && ctx->profsteps < ctx->profmax;
  bool const prof = sampling && ctx->profcalls % ctx->profstride == 0;

  // (refused before anything is consumed: the queued updates stay for the next call)
  if (prof && plan.groups != ctx->profgroups)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_displace: the cascade groups changed while profiling (its samples are per group)");

  // the retained dt's once more, then the queued ones; stored, or retained for the next row pass (ocean_writeback.h)
  PhaseWriteback::Launch const step = ctx->writeback.step(ctx->pending.data(), (int)ctx->pending.size(), plan.writeback);

  StepArgs a = make_args(ctx, step.ndt, step.dt, step.store);
  ctx->pending.clear();

  bool const foam = ctx->foammode != DATUM_OCEAN_FOAM_OFF;
  FoamArgs fa;

  if (foam)
    fa = foam_args(ctx);

  ctx->foamdt = 0.0;

  VelocityArgs va;

  if (velocity)
    va = velocity_args(ctx, step);

  // new maps from here on: the bounds records (datum_ocean_reduce_bounds) are no longer theirs
  ctx->boundscurrent = false;

  if (sampling)
    ctx->profcalls += 1;

  // group by group: row(g), column(g) -- or the literal dispatches -- and foam(g), then row(g + 1), ...
  for(int g = 0; g < plan.groups; ++g)
  {
    a.first = g * plan.group;
    a.cascades = std::min(plan.group, ctx->cascades - a.first);

    if (ctx->literal)
    {
      rc = launch_literals(ctx, a.first, a.cascades);
      if (rc != DATUM_OCEAN_OK)
        return rc;
    }
    else
    {
      hipEvent_t *ev = prof ? &ctx->events[4 * ((size_t)ctx->profsteps * plan.groups + g)] : nullptr;   // row start, row stop, column start, column stop

      HIPCHECK(ctx, launch(ctx, *plan.row, a, ev));
      HIPCHECK(ctx, launch(ctx, *plan.col, a, ev ? ev + 2 : nullptr));
    }

    // the group's foam while its maps are still in the cache (not sampled: the profile times the two passes)
    if (foam)
    {
      rc = launch_foam(ctx, fa, a.first, a.cascades, plan.streamed);
      if (rc != DATUM_OCEAN_OK)
        return rc;
    }

    // ... and its velocity plane (not sampled either)
    if (velocity)
    {
      rc = launch_velocity(ctx, va, a.first, a.cascades, plan.streamed);
      if (rc != DATUM_OCEAN_OK)
        return rc;
    }
  }

  if (velocity)
    ctx->velocitycurrent = true;

  if (prof)
    ctx->profsteps += 1;

  return DATUM_OCEAN_OK;
}

int datum_ocean_gen(datum_ocean_t ctx, int cascade, datum_ocean_set const *set, int sizex, int sizey, void *vertices_device)
{
  if (!ctx || !set || !vertices_device)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_gen: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_gen: cascade out of range");

  if (sizex < 2 || sizey < 2)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_gen: mesh must be at least 2 x 2");

  if ((uintptr_t)vertices_device & 15)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_gen: vertex buffer must be 16-byte aligned");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  GenArgs g;
  g.set = *set;
  g.map = reinterpret_cast<float4 const*>(map_block(ctx, cascade));
  g.vertices = (float*)vertices_device;
  gen_shape(g, ctx->N, sizex, sizey);

  // (one launch: the mesh as two half launches on two streams at once, joined by events, was measured and removed -- the fork and
  // join cost about 20 us per call on this runtime, 36 against 16 us: profiles/r04_gen_levers.txt)
  HIPCHECK(ctx, launch_gen(g, ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_payload_bytes(datum_ocean_t ctx, int format, size_t *bytes)
{
  if (!ctx || !bytes)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_payload_bytes: null argument");

  size_t const points = (size_t)ctx->cascades * plane(ctx);

  switch(format)
  {
    case DATUM_OCEAN_PAYLOAD_MAPS: *bytes = (size_t)ctx->cascades * map_cascade_bytes(ctx->N); break;
    case DATUM_OCEAN_PAYLOAD_XYZ32: *bytes = points * 12; break;
    case DATUM_OCEAN_PAYLOAD_XYZ16: *bytes = points * 8; break;
    default: return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_payload_bytes: unknown format");
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_pack_displacement(datum_ocean_t ctx, int format, void *payload_device, size_t bytes)
{
  if (!ctx || !payload_device)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_pack_displacement: null argument");

  size_t need = 0;

  int rc = datum_ocean_payload_bytes(ctx, format, &need);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (bytes < need)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_pack_displacement: payload buffer too small (datum_ocean_payload_bytes)");

  if ((uintptr_t)payload_device & 15)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_pack_displacement: payload buffer must be 16-byte aligned");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return pack_into(ctx, format, payload_device, need);
}

/* -- the tile farm ------------------------------------------------------------------------------------------------------ */

int datum_ocean_farm_unique_id(void *id, size_t bytes)
{
  if (!id || bytes != DATUM_OCEAN_FARM_ID_BYTES)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_farm_unique_id: the id is DATUM_OCEAN_FARM_ID_BYTES bytes");

  static_assert(sizeof(ncclUniqueId) == DATUM_OCEAN_FARM_ID_BYTES, "ncclUniqueId");

  std::string why;
  RcclApi *api = rccl_api(&why);

  if (!api)
    return fail(nullptr, DATUM_OCEAN_EUNSUPPORTED, ("datum_ocean_farm_unique_id: no RCCL library could be opened: " + why).c_str());

  ncclUniqueId uid;

  RCCLCHECK(nullptr, api, nullptr, api->GetUniqueId(&uid));

  memcpy(id, &uid, sizeof(uid));

  return DATUM_OCEAN_OK;
}

int datum_ocean_farm_init(datum_ocean_t ctx, void const *id, size_t idbytes, int rank, int world, int format, int slots)
{
  if (!ctx || !id || idbytes != DATUM_OCEAN_FARM_ID_BYTES)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_farm_init: null argument, or an id that is not DATUM_OCEAN_FARM_ID_BYTES bytes");

  if (world < 1 || rank < 0 || rank >= world)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_farm_init: rank outside [0, world)");

  if (slots < 1 || slots > 8)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_farm_init: 1 to 8 slots (2 = double-buffered)");

  if (ctx->farm)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_farm_init: the handle already farms (datum_ocean_farm_shutdown first)");

  size_t bytes = 0;

  int rc = datum_ocean_payload_bytes(ctx, format, &bytes);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  std::string why;
  RcclApi *api = rccl_api(&why);

  if (!api)
    return fail(ctx, DATUM_OCEAN_EUNSUPPORTED, ("datum_ocean_farm_init: no RCCL library could be opened: " + why).c_str());

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  Farm *f = new (std::nothrow) Farm;
  if (!f)
    return fail(ctx, DATUM_OCEAN_ENOMEM, "datum_ocean_farm_init: out of host memory");

  ctx->farm = f;

  f->api = api;
  f->rank = rank;
  f->world = world;
  f->format = format;
  f->bytes = bytes;

  #define FARMCHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { int rc_ = fail(ctx, (int)e_, #call); farm_teardown(ctx); return rc_; } } while(0)

  FARMCHECK(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));

  try { f->slots.resize(slots); } catch (...) { farm_teardown(ctx); return fail(ctx, DATUM_OCEAN_ENOMEM, "datum_ocean_farm_init: out of host memory"); }

  for(auto &sl : f->slots)
  {
    FARMCHECK(hipMalloc(&sl.payload, bytes));
    FARMCHECK(hipMalloc(&sl.gathered, bytes * world));
    FARMCHECK(hipEventCreateWithFlags(&sl.packed, hipEventDisableTiming));
    FARMCHECK(hipEventCreate(&sl.start));
    FARMCHECK(hipEventCreate(&sl.done));
    FARMCHECK(hipEventCreateWithFlags(&sl.consumed, hipEventDisableTiming));
  }

  #undef FARMCHECK

  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));

  // (collective over the ranks: returns when every rank of the farm has called it)
  ncclResult_t r = api->CommInitRank(&f->comm, world, uid, rank);

  if (r != ncclSuccess)
  {
    int rc_ = fail_comm(ctx, api, nullptr, r, "ncclCommInitRank");
    f->comm = nullptr;
    farm_teardown(ctx);
    return rc_;
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_farm_shutdown(datum_ocean_t ctx)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_farm_shutdown: null handle");

  (void)hipSetDevice(ctx->device);

  farm_teardown(ctx);

  return DATUM_OCEAN_OK;
}

int datum_ocean_farm_info(datum_ocean_t ctx, int *rank, int *world, int *format, size_t *payload_bytes, int *slots, int *rccl_version)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_farm_info: null handle");

  if (!ctx->farm)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_farm_info: datum_ocean_farm_init first");

  Farm const *f = ctx->farm;

  if (rank) *rank = f->rank;
  if (world) *world = f->world;
  if (format) *format = f->format;
  if (payload_bytes) *payload_bytes = f->bytes;
  if (slots) *slots = (int)f->slots.size();

  if (rccl_version)
  {
    *rccl_version = 0;
    (void)f->api->GetVersion(rccl_version);
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_farm_gather(datum_ocean_t ctx, int *slot)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_farm_gather: null handle");

  if (!ctx->farm)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_farm_gather: datum_ocean_farm_init first");

  Farm *f = ctx->farm;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  int const s = f->head;
  FarmSlot &sl = f->slots[s];

  // a consumer on a stream of its own took this slot's result and never said when it was done reading: the collective below
  // would overwrite what it may still be reading, and nothing orders the two
  if (sl.held)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_farm_gather: the next slot's result was handed to another stream and not released (datum_ocean_farm_release)");

  // WAR on the payload: the collective that last READ this slot's payload must have finished before the pack overwrites it
  if (sl.launched)
    HIPCHECK(ctx, hipStreamWaitEvent(ctx->stream, sl.done, 0));

  // the pack, on the handle's stream behind the last displace
  int rc = pack_into(ctx, f->format, sl.payload, f->bytes);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipEventRecord(sl.packed, ctx->stream));

  // the collective, on the communication stream: behind the pack, and behind the consumer that may still read gathered[s]
  HIPCHECK(ctx, hipStreamWaitEvent(f->stream, sl.packed, 0));

  if (sl.busy)
  {
    HIPCHECK(ctx, hipStreamWaitEvent(f->stream, sl.consumed, 0));
    sl.busy = false;
  }

  HIPCHECK(ctx, hipEventRecord(sl.start, f->stream));

  RCCLCHECK(ctx, f->api, f->comm, f->api->AllGather(sl.payload, sl.gathered, f->bytes, ncclInt8, f->comm, f->stream));

  HIPCHECK(ctx, hipEventRecord(sl.done, f->stream));

  sl.launched = true;

  f->head = (s + 1) % (int)f->slots.size();
  f->gathers += 1;

  if (slot)
    *slot = s;

  return DATUM_OCEAN_OK;
}

namespace
{
  static int farm_slot(datum_ocean_ctx *ctx, int slot, char const *who, FarmSlot **out)
  {
    if (!ctx)
      return fail(nullptr, DATUM_OCEAN_EINVAL, who);

    if (!ctx->farm)
      return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_farm_*: datum_ocean_farm_init first");

    if (slot < 0 || slot >= (int)ctx->farm->slots.size())
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_farm_*: no such slot");

    if (!ctx->farm->slots[slot].launched)
      return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_farm_*: nothing was gathered into this slot yet");

    *out = &ctx->farm->slots[slot];

    return DATUM_OCEAN_OK;
  }
}

int datum_ocean_farm_result(datum_ocean_t ctx, int slot, void *hip_stream, int on_handle_stream, void **gathered_device, size_t *bytes)
{
  FarmSlot *sl = nullptr;

  int rc = farm_slot(ctx, slot, "datum_ocean_farm_result: null handle", &sl);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!gathered_device)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_farm_result: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamWaitEvent(on_handle_stream ? ctx->stream : (hipStream_t)hip_stream, sl->done, 0));

  // (a reader on the handle's stream is ordered before the slot's next pack, and with it before its next collective; any
  // other stream has to release)
  if (!on_handle_stream && (hipStream_t)hip_stream != ctx->stream)
    sl->held = true;

  *gathered_device = sl->gathered;

  if (bytes)
    *bytes = ctx->farm->bytes * ctx->farm->world;

  return DATUM_OCEAN_OK;
}

int datum_ocean_farm_release(datum_ocean_t ctx, int slot, void *hip_stream, int on_handle_stream)
{
  FarmSlot *sl = nullptr;

  int rc = farm_slot(ctx, slot, "datum_ocean_farm_release: null handle", &sl);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipEventRecord(sl->consumed, on_handle_stream ? ctx->stream : (hipStream_t)hip_stream));

  sl->busy = true;
  sl->held = false;

  return DATUM_OCEAN_OK;
}

int datum_ocean_farm_query(datum_ocean_t ctx, int slot)
{
  FarmSlot *sl = nullptr;

  int rc = farm_slot(ctx, slot, "datum_ocean_farm_query: null handle", &sl);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  hipError_t const e = hipEventQuery(sl->done);

  if (e == hipErrorNotReady)
  {
    (void)hipGetLastError();
    return DATUM_OCEAN_ENOTREADY;
  }

  HIPCHECK(ctx, e);

  return DATUM_OCEAN_OK;
}

int datum_ocean_farm_wait(datum_ocean_t ctx, int slot, float *collective_ms)
{
  FarmSlot *sl = nullptr;

  int rc = farm_slot(ctx, slot, "datum_ocean_farm_wait: null handle", &sl);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipEventSynchronize(sl->done));

  if (collective_ms)
    HIPCHECK(ctx, hipEventElapsedTime(collective_ms, sl->start, sl->done));

  return DATUM_OCEAN_OK;
}

namespace
{
  // a stream on the compute units [first, first + count) of the device's CU-mask order (bit i: CU i / 8 of XCD i % 8 on an MI355X,
  // tools/cumask_probe.py); count == 0: an ordinary stream
  hipError_t make_stream(hipStream_t *stream, int cus, int first, int count)
  {
    if (count == 0)
      return hipStreamCreateWithFlags(stream, hipStreamNonBlocking);

    std::vector<uint32_t> words((cus + 31) / 32, 0u);

    for(int i = first; i < first + count; ++i)
      words[i / 32] |= 1u << (i % 32);

    return hipExtStreamCreateWithCUMask(stream, (uint32_t)words.size(), words.data());
  }
}

int datum_ocean_farm_partition(datum_ocean_t ctx, int comm_cus)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_farm_partition: null handle");

  Farm *f = ctx->farm;

  if (!f)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_farm_partition: the handle does not farm (datum_ocean_farm_init first)");

  // DATUM_OCEAN_FARM_PARTITION_AUTO: an eighth of the device in whole shares of 8 (one compute unit per XCD and share: 32 of an MI355X's
  // 256; none on a device with fewer than 64 compute units, where the call then leaves both streams on the whole device)
  if (comm_cus == DATUM_OCEAN_FARM_PARTITION_AUTO)
    comm_cus = (ctx->cus / 64) * 8;

  if (comm_cus < 0 || comm_cus % 8 != 0 || comm_cus > ctx->cus / 2)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_farm_partition: comm_cus must be 0, DATUM_OCEAN_FARM_PARTITION_AUTO or a multiple of 8 (one share per XCD), at most half the device");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  // nothing in flight on either stream while they are replaced (the slots' events stay valid: they have completed)
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->ownstream));
  HIPCHECK(ctx, hipStreamSynchronize(f->stream));

  hipStream_t comm = nullptr, own = nullptr;

  HIPCHECK(ctx, make_stream(&comm, ctx->cus, 0, comm_cus));

  hipError_t const e = make_stream(&own, ctx->cus, comm_cus, comm_cus ? ctx->cus - comm_cus : 0);

  if (e != hipSuccess)
  {
    (void)hipStreamDestroy(comm);
    return fail(ctx, (int)e, "datum_ocean_farm_partition: hipExtStreamCreateWithCUMask");
  }

  bool const onown = ctx->stream == ctx->ownstream;

  (void)hipStreamDestroy(f->stream);
  (void)hipStreamDestroy(ctx->ownstream);

  f->stream = comm;
  f->commcus = comm_cus;
  ctx->ownstream = own;

  if (onown)
    ctx->stream = own;

  return DATUM_OCEAN_OK;
}

int datum_ocean_farm_stream_flags(datum_ocean_t ctx, unsigned int *communication_stream_flags, unsigned int *own_stream_flags)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_farm_stream_flags: null handle");

  if (!ctx->farm)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_farm_stream_flags: the handle does not farm (datum_ocean_farm_init first)");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  // (CU-masked streams come without a flags argument: what the runtime made of them is what decides whether a null-stream operation of the
  // caller's serialises the two streams -- include/datum_ocean_hip.h, datum_ocean_farm_partition)
  if (communication_stream_flags)
    HIPCHECK(ctx, hipStreamGetFlags(ctx->farm->stream, communication_stream_flags));

  if (own_stream_flags)
    HIPCHECK(ctx, hipStreamGetFlags(ctx->ownstream, own_stream_flags));

  return DATUM_OCEAN_OK;
}

int datum_ocean_own_stream(datum_ocean_t ctx, void **hip_stream)
{
  if (!ctx || !hip_stream)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_own_stream: null argument");

  *hip_stream = ctx->ownstream;

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_maps(datum_ocean_t ctx, int cascade, float *maps)
{
  if (!ctx || !maps)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_maps: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_maps: cascade out of range");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  size_t const P = plane(ctx);

  // the device layout is the module's own (ocean_layout.h: map_compact_a / map_compact_b); hand out the reference's logical
  // image, [layer][y][x] RGBA32F with the .w channels zero (map.comp:79-80)
  size_t const bytes = map_cascade_bytes(ctx->N);

  std::vector<float> raw;
  try { raw.resize(bytes / sizeof(float)); } catch (...) { return fail(ctx, DATUM_OCEAN_ENOMEM, "datum_ocean_read_maps: out of host memory"); }

  HIPCHECK(ctx, hipMemcpyAsync(raw.data(), map_block(ctx, cascade), bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  int const N = ctx->N;
  float4 *out = reinterpret_cast<float4*>(maps);

  for(int y = 0; y < N; ++y)
  {
    for(int x = 0; x < N; ++x)
    {
      float const *a = raw.data() + map_compact_a(N, y, x) / sizeof(float);
      float const *b = raw.data() + map_compact_b(N, y, x) / sizeof(float);

      out[(size_t)y * N + x] = make_float4(a[0], a[1], a[2], 0.0f);
      out[P + (size_t)y * N + x] = make_float4(a[3], b[0], b[1], 0.0f);
    }
  }

  return DATUM_OCEAN_OK;
}

/* -- foam ------------------------------------------------------------------------------------------------------------------ */

int datum_ocean_set_foam(datum_ocean_t ctx, int mode)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_foam: null handle");

  if (mode != DATUM_OCEAN_FOAM_OFF && mode != DATUM_OCEAN_FOAM_JACOBIAN && mode != DATUM_OCEAN_FOAM_ACCUMULATE)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_foam: unknown mode");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  if (mode == DATUM_OCEAN_FOAM_OFF)
  {
    if (ctx->foam.own)
    {
      HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
      HIPCHECK(ctx, hipFree(ctx->foam.own));
      ctx->foam.own = nullptr;
    }

    ctx->foammode = mode;

    return DATUM_OCEAN_OK;
  }

  if (!ctx->foam.own)
    HIPCHECK(ctx, hipMalloc(&ctx->foam.own, foam_bytes(ctx)));

  ctx->foammode = mode;

  int rc = zero_foam(ctx, -1);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_foam_params(datum_ocean_t ctx, int cascade, float threshold, float gain, float decay)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_foam_params: null handle");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_foam_params: cascade out of range");

  if (!std::isfinite(threshold) || !std::isfinite(gain) || !std::isfinite(decay))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_foam_params: threshold, gain and decay must be finite");

  if (gain < 0 || decay < 0)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_foam_params: gain and decay must not be negative");

  ctx->cstate[cascade].foamthreshold = threshold;
  ctx->cstate[cascade].foamgain = gain;
  ctx->cstate[cascade].foamdecay = decay;

  return DATUM_OCEAN_OK;
}

int datum_ocean_reset_foam(datum_ocean_t ctx, int cascade)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_reset_foam: null handle");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_reset_foam: cascade out of range");

  if (ctx->foammode == DATUM_OCEAN_FOAM_OFF)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_reset_foam: foam is off (datum_ocean_set_foam)");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return zero_foam(ctx, cascade);
}

int datum_ocean_bind_foam(datum_ocean_t ctx, void *device_ptr, size_t bytes)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_bind_foam: null handle");

  return bind_plane(ctx, ctx->foam, device_ptr, bytes, foam_bytes(ctx),
                    "datum_ocean_bind_foam: buffer smaller than cascades * N * N * 4 bytes", "datum_ocean_bind_foam: buffer must be 16-byte aligned");
}

int datum_ocean_foam_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes)
{
  if (!ctx || !device_ptr)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_foam_device: null argument");

  if (ctx->foammode == DATUM_OCEAN_FOAM_OFF)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_foam_device: foam is off (datum_ocean_set_foam)");

  *device_ptr = ctx->foam.get();

  if (bytes)
    *bytes = foam_bytes(ctx);

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_foam(datum_ocean_t ctx, int cascade, float *foam)
{
  if (!ctx || !foam)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_foam: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_foam: cascade out of range");

  if (ctx->foammode == DATUM_OCEAN_FOAM_OFF)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_read_foam: foam is off (datum_ocean_set_foam)");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  size_t const P = plane(ctx);

  HIPCHECK(ctx, hipMemcpyAsync(foam, ctx->foam.get() + cascade * P, P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

}   // extern "C"

/* -- surface queries ------------------------------------------------------------------------------------------------------- */

int Staging::reserve(datum_ocean_ctx *ctx, size_t bytes)
{
  if (bytes <= capacity)
    return DATUM_OCEAN_OK;

  // the old staging may still be read by an earlier launch of this stream (a call that grows several buffers waits once for
  // each: after the first the stream holds at most that call's own copy in)
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHECK(ctx, hipFree(ptr));
  ptr = nullptr;
  capacity = 0;

  HIPCHECK(ctx, hipMalloc(&ptr, bytes));
  capacity = bytes;

  return DATUM_OCEAN_OK;
}

namespace
{
  // a read_* twin behind its checks: `in` and `out` grown to hold the call's arrays, `src` copied in on the handle's stream, `run` -- the
  // device-array twin's own launch path -- on the staging, the result copied out to `dst` and waited for
  template<class Run>
  int read_staged(datum_ocean_ctx *ctx, Staging &in, void const *src, size_t inbytes, Staging &out, void *dst, size_t outbytes, Run &&run)
  {
    int rc = in.reserve(ctx, inbytes);
    if (rc == DATUM_OCEAN_OK)
      rc = out.reserve(ctx, outbytes);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    HIPCHECK(ctx, hipMemcpyAsync(in.ptr, src, inbytes, hipMemcpyHostToDevice, ctx->stream));

    rc = run(in.ptr, out.ptr);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    HIPCHECK(ctx, hipMemcpyAsync(dst, out.ptr, outbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // ... of a one-point-per-thread query: `count` points in, two float4 per point out
  template<class Run>
  int read_points(datum_ocean_ctx *ctx, float const *points, size_t count, float *samples, Run &&run)
  {
    return read_staged(ctx, ctx->staging[STAGE_POINTS], points, count * sizeof(float2), ctx->staging[STAGE_SAMPLES], samples, count * 2 * sizeof(float4), run);
  }

  // the arrays of a one-point-per-thread query; `name` goes into the error text
  int check_points(datum_ocean_ctx *ctx, void const *points, size_t count, void const *samples, char const *name)
  {
    if (count > 0 && (!points || !samples))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null points or samples");

    if (((uintptr_t)points & 7) || ((uintptr_t)samples & 15))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": points must be 8-byte and samples 16-byte aligned");

    if (count > (size_t)INT32_MAX)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": count above INT32_MAX");

    return DATUM_OCEAN_OK;
  }

  // the argument checks both single-cascade entry points share
  int check_surface_args(datum_ocean_ctx *ctx, int cascade, datum_ocean_set const *set, int iterations, void const *points, size_t count, void const *samples, char const *name)
  {
    if (!ctx || !set)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null handle or set");

    if (cascade < 0 || cascade >= ctx->cascades)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": cascade out of range");

    if (iterations < 0 || iterations > DATUM_OCEAN_SURFACE_MAX_ITERATIONS)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": iterations outside [0, DATUM_OCEAN_SURFACE_MAX_ITERATIONS]");

    return check_points(ctx, points, count, samples, name);
  }

  // the launch both single-cascade entry points share: device arrays, count > 0
  int run_surface(datum_ocean_ctx *ctx, int cascade, datum_ocean_set const *set, int iterations, void const *points, size_t count, void *samples)
  {
    SurfaceArgs s;
    s.set = *set;
    s.map = reinterpret_cast<float4 const*>(map_block(ctx, cascade));
    s.foam = (ctx->foammode != DATUM_OCEAN_FOAM_OFF) ? ctx->foam.get() + (size_t)cascade * plane(ctx) : nullptr;
    s.points = static_cast<float2 const*>(points);
    s.samples = static_cast<float4*>(samples);
    s.N = ctx->N;
    s.count = (int)count;
    s.iterations = iterations;

    HIPCHECK(ctx, launch_surface(s, ctx->stream));

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_sample_surface(datum_ocean_t ctx, int cascade, datum_ocean_set const *set, int iterations, void const *points_device, size_t count, void *samples_device)
{
  int rc = check_surface_args(ctx, cascade, set, iterations, points_device, count, samples_device, "datum_ocean_sample_surface");
  if (rc != DATUM_OCEAN_OK || count == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_surface(ctx, cascade, set, iterations, points_device, count, samples_device);
}

int datum_ocean_read_surface(datum_ocean_t ctx, int cascade, datum_ocean_set const *set, int iterations, float const *points, size_t count, float *samples)
{
  int rc = check_surface_args(ctx, cascade, set, iterations, points, count, samples, "datum_ocean_read_surface");
  if (rc != DATUM_OCEAN_OK || count == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return read_points(ctx, points, count, samples, [&](void const *in, void *out) { return run_surface(ctx, cascade, set, iterations, in, count, out); });
}

}   // extern "C"

/* -- several cascades at once (ocean_blend.hip) ------------------------------------------------------------------------------- */

namespace
{
  // a query as the caller gave it: the listed cascades, the set and the solve's iterations (0 where a call has none: the mesh calls and
  // surface_slab, which check the list alone)
  struct Query { int const *cascades; int count; datum_ocean_set const *set; int iterations; };

  // a body call's arrays as the caller gave them, device or host alike; motions and props are null where the call takes none
  struct BodyBatch { void const *bodies, *motions, *props; size_t nbodies; void const *probes; size_t nprobes; void *records; };

  // a ray cast's own arguments and arrays as the caller gave them, device or host alike
  struct RayCall { int steps, refine; void const *rays; size_t n; void *records; };

  // what a read of the summed surface takes besides: the ripple layer on top, and (a cast) the samples the slab decides skipped
  struct ReadVariant { bool rippled, bounded; };

  // the ripple layer as the reads see it, defined with the layer and with its bounds below
  int check_ripples(datum_ocean_ctx *ctx, char const *name);
  RippledLayer rippled_layer(datum_ocean_ctx const *ctx);
  float4 *ripple_bounds_record(datum_ocean_ctx const *ctx);

  // the list's checks, shared by every entry point that takes one; `name` goes into the error text
  int check_blend_list(datum_ocean_ctx *ctx, Query const &q, char const *name)
  {
    if (!ctx)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null handle");

    if (!q.cascades)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null cascade list");

    if (q.count < 1 || q.count > DATUM_OCEAN_MAX_CASCADES)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": count outside [1, DATUM_OCEAN_MAX_CASCADES]");

    for(int i = 0; i < q.count; ++i)
      if (q.cascades[i] < 0 || q.cascades[i] >= ctx->cascades)
        return fail(ctx, DATUM_OCEAN_EINVAL, name, ": cascade out of range");

    return DATUM_OCEAN_OK;
  }

  // what every query on the summed surface checks first: the handle and the list, the set, the iterations
  int check_query(datum_ocean_ctx *ctx, Query const &q, char const *name)
  {
    int rc = check_blend_list(ctx, q, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (!q.set)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null set");

    if (q.iterations < 0 || q.iterations > DATUM_OCEAN_SURFACE_MAX_ITERATIONS)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": iterations outside [0, DATUM_OCEAN_SURFACE_MAX_ITERATIONS]");

    return DATUM_OCEAN_OK;
  }

  BlendList blend_list(datum_ocean_ctx *ctx, Query const &q)
  {
    BlendList l = {};
    l.count = q.count;
    l.foammode = ctx->foammode;

    for(int i = 0; i < q.count; ++i)
    {
      int const c = q.cascades[i];

      l.casc[i].map = reinterpret_cast<float4 const*>(map_block(ctx, c));
      l.casc[i].foam = (ctx->foammode != DATUM_OCEAN_FOAM_OFF) ? ctx->foam.get() + (size_t)c * plane(ctx) : nullptr;
      l.casc[i].scale = ctx->casc[c].scale;
    }

    return l;
  }

  // (the frame is the launch's: query_frame)
  QueryArgs query_args(datum_ocean_ctx *ctx, Query const &q)
  {
    QueryArgs a = {};
    a.set = *q.set;
    a.list = blend_list(ctx, q);
    a.N = ctx->N;
    a.iterations = q.iterations;
    return a;
  }

  int check_surface_blend_args(datum_ocean_ctx *ctx, Query const &q, void const *points, size_t n, void const *samples, char const *name)
  {
    int rc = check_query(ctx, q, name);

    return rc != DATUM_OCEAN_OK ? rc : check_points(ctx, points, n, samples, name);
  }

  // what the several-cascade mesh calls check; `name` goes into the error text
  int check_gen_blend_args(datum_ocean_ctx *ctx, Query const &q, int sizex, int sizey, void const *vertices, char const *name)
  {
    if (!ctx || !q.set || !vertices)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null argument");

    int rc = check_blend_list(ctx, q, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (sizex < 2 || sizey < 2)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": mesh must be at least 2 x 2");

    if ((uintptr_t)vertices & 15)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": vertex buffer must be 16-byte aligned");

    return DATUM_OCEAN_OK;
  }

  // (the shape is the launch's: gen_shape)
  GenBlendArgs gen_blend_args(datum_ocean_ctx *ctx, Query const &q, void *vertices)
  {
    GenBlendArgs b;
    b.g.set = *q.set;
    b.g.map = nullptr;
    b.g.vertices = (float*)vertices;
    b.list = blend_list(ctx, q);
    return b;
  }

  SurfaceBlendArgs surface_blend_args(datum_ocean_ctx *ctx, Query const &q, void const *points, size_t n, void *samples)
  {
    SurfaceBlendArgs b;
    b.q = query_args(ctx, q);
    b.points = static_cast<float2 const*>(points);
    b.samples = static_cast<float4*>(samples);
    b.count = (int)n;
    return b;
  }

  // the mesh of the summed surface, with the ripple layer on top where `rippled`: the layer's check first (a null handle EINVAL, the
  // layer off ESTATE), then the mesh's own, then the launch
  int gen_blend(datum_ocean_ctx *ctx, Query const &q, int sizex, int sizey, void *vertices, bool rippled, char const *name)
  {
    int rc = rippled ? check_ripples(ctx, name) : DATUM_OCEAN_OK;
    if (rc == DATUM_OCEAN_OK)
      rc = check_gen_blend_args(ctx, q, sizex, sizey, vertices, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    HIPCHECK(ctx, hipSetDevice(ctx->device));

    GenBlendArgs b = gen_blend_args(ctx, q, vertices);

    if (rippled)
    {
      GenBlendRippledArgs r = { b, rippled_layer(ctx) };

      HIPCHECK(ctx, launch_gen_blend_rippled(r, ctx->N, sizex, sizey, ctx->stream));
    }
    else
      HIPCHECK(ctx, launch_gen_blend(b, ctx->N, sizex, sizey, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // the point read's checks in their order: the layer where it is on top, then the query and the arrays
  int check_surface_read(datum_ocean_ctx *ctx, Query const &q, void const *points, size_t n, void const *samples, bool rippled, char const *name)
  {
    int rc = rippled ? check_ripples(ctx, name) : DATUM_OCEAN_OK;

    return rc != DATUM_OCEAN_OK ? rc : check_surface_blend_args(ctx, q, points, n, samples, name);
  }

  // device arrays, n > 0
  int run_surface_blend(datum_ocean_ctx *ctx, Query const &q, void const *points, size_t n, void *samples, bool rippled)
  {
    SurfaceBlendArgs b = surface_blend_args(ctx, q, points, n, samples);

    if (rippled)
    {
      SurfaceBlendRippledArgs r = { b, rippled_layer(ctx) };

      HIPCHECK(ctx, launch_surface_blend_rippled(r, ctx->stream));
    }
    else
      HIPCHECK(ctx, launch_surface_blend(b, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // the point read on device arrays
  int sample_surface_blend(datum_ocean_ctx *ctx, Query const &q, void const *points, size_t n, void *samples, bool rippled, char const *name)
  {
    int rc = check_surface_read(ctx, q, points, n, samples, rippled, name);
    if (rc != DATUM_OCEAN_OK || n == 0)
      return rc;

    HIPCHECK(ctx, hipSetDevice(ctx->device));

    return run_surface_blend(ctx, q, points, n, samples, rippled);
  }

  // ... and its host twin
  int read_surface_blend(datum_ocean_ctx *ctx, Query const &q, float const *points, size_t n, float *samples, bool rippled, char const *name)
  {
    int rc = check_surface_read(ctx, q, points, n, samples, rippled, name);
    if (rc != DATUM_OCEAN_OK || n == 0)
      return rc;

    HIPCHECK(ctx, hipSetDevice(ctx->device));

    return read_points(ctx, points, n, samples, [&](void const *in, void *out) { return run_surface_blend(ctx, q, in, n, out, rippled); });
  }
}

extern "C"
{

int datum_ocean_gen_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int sizex, int sizey, void *vertices_device)
{
  Query const q = { cascades, count, set, 0 };

  return gen_blend(ctx, q, sizex, sizey, vertices_device, false, "datum_ocean_gen_blend");
}

int datum_ocean_sample_surface_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, void const *points_device, size_t n, void *samples_device)
{
  Query const q = { cascades, count, set, iterations };

  return sample_surface_blend(ctx, q, points_device, n, samples_device, false, "datum_ocean_sample_surface_blend");
}

int datum_ocean_read_surface_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, float const *points, size_t n, float *samples)
{
  Query const q = { cascades, count, set, iterations };

  return read_surface_blend(ctx, q, points, n, samples, false, "datum_ocean_read_surface_blend");
}

}   // extern "C"

/* -- surface velocity (ocean_velocity.hip) -------------------------------------------------------------------------------------- */

namespace
{
  // what read_velocity and the two queries refuse; `name` goes into the error text
  int check_velocity_state(datum_ocean_ctx *ctx, char const *name)
  {
    if (ctx->velocitymode == DATUM_OCEAN_VELOCITY_OFF)
      return fail(ctx, DATUM_OCEAN_ESTATE, name, ": velocity is off (datum_ocean_set_velocity)");

    if (!ctx->velocitycurrent)
      return fail(ctx, DATUM_OCEAN_ESTATE, name, ": no datum_ocean_displace since velocity was switched on");

    return DATUM_OCEAN_OK;
  }

  // the several-cascade query's checks, then the state both velocity queries need
  int check_velocity_blend_args(datum_ocean_ctx *ctx, Query const &q, void const *points, size_t n, void const *out, char const *name)
  {
    int rc = check_surface_blend_args(ctx, q, points, n, out, name);

    return rc != DATUM_OCEAN_OK ? rc : check_velocity_state(ctx, name);
  }

  // the velocity planes of a query's list, in list order (the entries past the list stay as the caller zeroed them)
  void velocity_planes(datum_ocean_ctx *ctx, Query const &q, float4 const **vel)
  {
    for(int i = 0; i < q.count; ++i)
      vel[i] = ctx->velocity.get() + (size_t)q.cascades[i] * plane(ctx);
  }

  // device arrays, n > 0
  int run_velocity_blend(datum_ocean_ctx *ctx, Query const &q, void const *points, size_t n, void *out)
  {
    VelocityBlendArgs vb = {};
    vb.q = query_args(ctx, q);
    vb.points = static_cast<float2 const*>(points);
    vb.samples = static_cast<float4*>(out);
    vb.count = (int)n;

    velocity_planes(ctx, q, vb.vel);

    HIPCHECK(ctx, launch_velocity_blend(vb, ctx->stream));

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_set_velocity(datum_ocean_t ctx, int mode)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_velocity: null handle");

  if (mode != DATUM_OCEAN_VELOCITY_OFF && mode != DATUM_OCEAN_VELOCITY_ON)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_velocity: unknown mode");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  if (mode == DATUM_OCEAN_VELOCITY_OFF)
  {
    HIPCHECK(ctx, hipFree(ctx->velocity.own));
    ctx->velocity.own = nullptr;
    HIPCHECK(ctx, hipFree(ctx->velocitywork));
    ctx->velocitywork = nullptr;
    ctx->velocityworkgroup = 0;
    ctx->velocitymode = mode;
    ctx->velocitycurrent = false;

    return DATUM_OCEAN_OK;
  }

  if (ctx->velocitymode == mode)
    return DATUM_OCEAN_OK;

  // the LDS limit of the kernels the mode launches: a kernel the module launches is one it configured
  if (!ctx->velocitykernels.col)
  {
    VelocityKernels k;

    DISPATCH_N(ctx->N, k = velocity_kernels<NN>());

    HIPCHECK(ctx, hipFuncSetAttribute(k.col, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.collds));
    HIPCHECK(ctx, hipFuncSetAttribute(k.row[0], hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.rowlds));
    HIPCHECK(ctx, hipFuncSetAttribute(k.row[1], hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.rowlds));

    ctx->velocitykernels = k;
  }

  if (!ctx->velocity.own)
    HIPCHECK(ctx, hipMalloc(&ctx->velocity.own, velocity_bytes(ctx)));

  HIPCHECK(ctx, hipMemsetAsync(ctx->velocity.own, 0, velocity_bytes(ctx), ctx->stream));

  int rc = ensure_velocity_work(ctx, plan_step(ctx).group);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  ctx->velocitymode = mode;
  ctx->velocitycurrent = false;

  return DATUM_OCEAN_OK;
}

int datum_ocean_bind_velocity(datum_ocean_t ctx, void *device_ptr, size_t bytes)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_bind_velocity: null handle");

  int rc = bind_plane(ctx, ctx->velocity, device_ptr, bytes, velocity_bytes(ctx),
                      "datum_ocean_bind_velocity: buffer smaller than cascades * N * N * 16 bytes", "datum_ocean_bind_velocity: buffer must be 16-byte aligned");

  // the plane in use changed: it holds a velocity again after the next displace
  if (rc == DATUM_OCEAN_OK)
    ctx->velocitycurrent = false;

  return rc;
}

int datum_ocean_velocity_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes)
{
  if (!ctx || !device_ptr)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_velocity_device: null argument");

  if (ctx->velocitymode == DATUM_OCEAN_VELOCITY_OFF)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_velocity_device: velocity is off (datum_ocean_set_velocity)");

  *device_ptr = ctx->velocity.get();

  if (bytes)
    *bytes = velocity_bytes(ctx);

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_velocity(datum_ocean_t ctx, int cascade, float *vel)
{
  if (!ctx || !vel)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_velocity: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_velocity: cascade out of range");

  int rc = check_velocity_state(ctx, "datum_ocean_read_velocity");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  size_t const P = plane(ctx);

  HIPCHECK(ctx, hipMemcpyAsync(vel, ctx->velocity.get() + cascade * P, P * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_sample_velocity_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, void const *points_device, size_t n, void *out_device)
{
  Query const q = { cascades, count, set, iterations };
  int rc = check_velocity_blend_args(ctx, q, points_device, n, out_device, "datum_ocean_sample_velocity_blend");
  if (rc != DATUM_OCEAN_OK || n == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_velocity_blend(ctx, q, points_device, n, out_device);
}

int datum_ocean_read_velocity_blend(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, float const *points, size_t n, float *out)
{
  Query const q = { cascades, count, set, iterations };
  int rc = check_velocity_blend_args(ctx, q, points, n, out, "datum_ocean_read_velocity_blend");
  if (rc != DATUM_OCEAN_OK || n == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return read_points(ctx, points, n, out, [&](void const *in, void *dev) { return run_velocity_blend(ctx, q, in, n, dev); });
}

}   // extern "C"

/* -- body buoyancy (ocean_body.hip) -------------------------------------------------------------------------------------------- */

namespace
{
  // the checks both entry points share; `name` goes into the error text
  int check_body_args(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, char const *name)
  {
    int rc = check_query(ctx, q, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if ((b.nbodies > 0 && (!b.bodies || !b.records)) || (b.nprobes > 0 && !b.probes))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null bodies, probes or records");

    if (((uintptr_t)b.bodies & 15) || ((uintptr_t)b.probes & 15) || ((uintptr_t)b.records & 15))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": bodies, probes and records must be 16-byte aligned");

    if (b.nbodies > (size_t)INT32_MAX || b.nprobes > (size_t)INT32_MAX)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": nbodies or nprobes above INT32_MAX");

    return DATUM_OCEAN_OK;
  }

  // a body kernel's share of its arguments from a query and a device batch, filled in place (the struct is large); the drag, wake, step
  // and couple fillers add their own fields beside it
  void fill_body_args(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, BodyArgs &a)
  {
    a.q = query_args(ctx, q);
    a.bodies = static_cast<datum_ocean_body const*>(b.bodies);
    a.probes = static_cast<BodyProbe const*>(b.probes);
    a.records = static_cast<float4*>(b.records);
    a.nbodies = (int)b.nbodies;
    a.nprobes = (int)b.nprobes;
  }

  // device arrays, nbodies > 0
  int run_bodies(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b)
  {
    BodyArgs a;
    fill_body_args(ctx, q, b, a);

    HIPCHECK(ctx, launch_bodies(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // a host twin of a body call behind its checks, first half: the device made current, the staging of each array the batch has (one per
  // array: STAGE_*) and of its records, `recordfloats` floats per body, each grown on its own, then the arrays copied in on the handle's
  // stream (an empty one is not); `dev` is the batch as the family's run_* takes it
  int stage_batch(datum_ocean_ctx *ctx, BodyBatch const &host, size_t recordfloats, BodyBatch &dev)
  {
    int const stage[4] = { STAGE_BODIES, STAGE_MOTIONS, STAGE_PROPS, STAGE_PROBES };
    void const *const src[4] = { host.bodies, host.motions, host.props, host.probes };
    size_t const bytes[4] = { host.nbodies * sizeof(datum_ocean_body), host.nbodies * sizeof(datum_ocean_body_motion),
                              host.nbodies * sizeof(datum_ocean_body_props), host.nprobes * sizeof(BodyProbe) };
    void *ptr[4] = {};

    HIPCHECK(ctx, hipSetDevice(ctx->device));

    int rc = ctx->staging[STAGE_BODY_RECORDS].reserve(ctx, host.nbodies * recordfloats * sizeof(float));

    for(int i = 0; i < 4 && rc == DATUM_OCEAN_OK; ++i)
      if (src[i])
        rc = ctx->staging[stage[i]].reserve(ctx, bytes[i]);

    if (rc != DATUM_OCEAN_OK)
      return rc;

    for(int i = 0; i < 4; ++i)
    {
      if (src[i])
        ptr[i] = ctx->staging[stage[i]].ptr;

      if (src[i] && bytes[i] > 0)
        HIPCHECK(ctx, hipMemcpyAsync(ptr[i], src[i], bytes[i], hipMemcpyHostToDevice, ctx->stream));
    }

    dev = BodyBatch{ ptr[0], ptr[1], ptr[2], host.nbodies, ptr[3], host.nprobes, ctx->staging[STAGE_BODY_RECORDS].ptr };

    return DATUM_OCEAN_OK;
  }

  // ... second half, after the launches: the records -- and of a step (`stepped`) the bodies and motions it advanced -- copied back to the
  // caller's arrays and waited for; no body, no copy
  int fetch_batch(datum_ocean_ctx *ctx, BodyBatch const &host, BodyBatch const &dev, size_t recordfloats, bool stepped)
  {
    if (host.nbodies > 0 && stepped)
    {
      // (a step's entry points take both arrays writable)
      HIPCHECK(ctx, hipMemcpyAsync(const_cast<void*>(host.bodies), dev.bodies, host.nbodies * sizeof(datum_ocean_body), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHECK(ctx, hipMemcpyAsync(const_cast<void*>(host.motions), dev.motions, host.nbodies * sizeof(datum_ocean_body_motion), hipMemcpyDeviceToHost, ctx->stream));
    }

    if (host.nbodies > 0)
      HIPCHECK(ctx, hipMemcpyAsync(host.records, dev.records, host.nbodies * recordfloats * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));

    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_reduce_bodies(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                              void const *bodies_device, size_t nbodies, void const *probes_device, size_t nprobes, void *records_device)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const b = { bodies_device, nullptr, nullptr, nbodies, probes_device, nprobes, records_device };

  int rc = check_body_args(ctx, q, b, "datum_ocean_reduce_bodies");
  if (rc != DATUM_OCEAN_OK || nbodies == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_bodies(ctx, q, b);
}

int datum_ocean_read_bodies(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                            datum_ocean_body const *bodies, size_t nbodies, float const *probes, size_t nprobes, float *records)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const host = { bodies, nullptr, nullptr, nbodies, probes, nprobes, records };
  BodyBatch dev;

  int rc = check_body_args(ctx, q, host, "datum_ocean_read_bodies");
  if (rc != DATUM_OCEAN_OK || nbodies == 0)
    return rc;

  rc = stage_batch(ctx, host, DATUM_OCEAN_BODY_RECORD_FLOATS, dev);
  if (rc == DATUM_OCEAN_OK)
    rc = run_bodies(ctx, q, dev);

  return rc != DATUM_OCEAN_OK ? rc : fetch_batch(ctx, host, dev, DATUM_OCEAN_BODY_RECORD_FLOATS, false);
}

}   // extern "C"

/* -- body drag (ocean_drag.hip) --------------------------------------------------------------------------------------------------- */

namespace
{
  // the body calls' checks with the motions beside the bodies, then the state the velocity queries need; `name` goes into the error text
  int check_body_drag_args(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, char const *name)
  {
    int rc = check_body_args(ctx, q, b, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (b.nbodies > 0 && !b.motions)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null motions");

    if ((uintptr_t)b.motions & 15)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": motions must be 16-byte aligned");

    return check_velocity_state(ctx, name);
  }

  // body buoyancy's share, the motions and the list's velocity planes: what the drag, wake, step and couple kernels all read
  void fill_drag_args(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, DragArgs &d)
  {
    fill_body_args(ctx, q, b, d.b);
    d.motions = static_cast<datum_ocean_body_motion const*>(b.motions);
    velocity_planes(ctx, q, d.vel);
  }

  // device arrays, nbodies > 0
  int run_body_drag(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b)
  {
    DragArgs a = {};
    fill_drag_args(ctx, q, b, a);

    HIPCHECK(ctx, launch_body_drag(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_reduce_body_drag(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                 void const *bodies_device, void const *motions_device, size_t nbodies, void const *probes_device, size_t nprobes,
                                 void *records_device)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const b = { bodies_device, motions_device, nullptr, nbodies, probes_device, nprobes, records_device };

  int rc = check_body_drag_args(ctx, q, b, "datum_ocean_reduce_body_drag");
  if (rc != DATUM_OCEAN_OK || nbodies == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_body_drag(ctx, q, b);
}

int datum_ocean_read_body_drag(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                               datum_ocean_body const *bodies, datum_ocean_body_motion const *motions, size_t nbodies, float const *probes, size_t nprobes,
                               float *records)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const host = { bodies, motions, nullptr, nbodies, probes, nprobes, records };
  BodyBatch dev;

  int rc = check_body_drag_args(ctx, q, host, "datum_ocean_read_body_drag");
  if (rc != DATUM_OCEAN_OK || nbodies == 0)
    return rc;

  rc = stage_batch(ctx, host, DATUM_OCEAN_DRAG_RECORD_FLOATS, dev);
  if (rc == DATUM_OCEAN_OK)
    rc = run_body_drag(ctx, q, dev);

  return rc != DATUM_OCEAN_OK ? rc : fetch_batch(ctx, host, dev, DATUM_OCEAN_DRAG_RECORD_FLOATS, false);
}

}   // extern "C"

/* -- body stepping (ocean_step.hip) ----------------------------------------------------------------------------------------------- */

namespace
{
  // body drag's checks with the props beside the motions, then the step's own two numbers; `name` goes into the error text
  int check_step_args(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, float dt, int substeps, char const *name)
  {
    // (the state last: ESTATE exactly where body drag returns it, EINVAL first as there)
    int rc = check_body_args(ctx, q, b, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (b.nbodies > 0 && (!b.motions || !b.props))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null motions or props");

    if (((uintptr_t)b.motions & 15) || ((uintptr_t)b.props & 15))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": motions and props must be 16-byte aligned");

    if (substeps < 1 || substeps > DATUM_OCEAN_STEP_MAX_SUBSTEPS)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": substeps outside [1, DATUM_OCEAN_STEP_MAX_SUBSTEPS]");

    if (!std::isfinite(dt))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": dt is not finite");

    return check_velocity_state(ctx, name);
  }

  // a sub-step's length as every stepping call rounds it, once, on the host: two fp32 operations, the reciprocal and then the product (as
  // the ray cast's inv), never dt / substeps
  float substep_length(float dt, int substeps)
  {
    float const inv = 1.0f / (float)substeps;
    return dt * inv;
  }

  // device arrays, nbodies > 0
  int run_step_bodies(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, float dt, int substeps)
  {
    BodyStepArgs a = {};
    fill_drag_args(ctx, q, b, a.d);
    a.bodies = const_cast<datum_ocean_body*>(a.d.b.bodies);             // (the step's entry points take both writable)
    a.motions = const_cast<datum_ocean_body_motion*>(a.d.motions);
    a.props = static_cast<datum_ocean_body_props const*>(b.props);
    a.h = substep_length(dt, substeps);
    a.substeps = substeps;

    HIPCHECK(ctx, launch_step_bodies(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_step_bodies(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                            void *bodies_device, void *motions_device, void const *props_device, size_t nbodies, void const *probes_device, size_t nprobes,
                            float dt, int substeps, void *records_device)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const b = { bodies_device, motions_device, props_device, nbodies, probes_device, nprobes, records_device };

  int rc = check_step_args(ctx, q, b, dt, substeps, "datum_ocean_step_bodies");
  if (rc != DATUM_OCEAN_OK || nbodies == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_step_bodies(ctx, q, b, dt, substeps);
}

int datum_ocean_step_bodies_host(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                 datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, size_t nbodies,
                                 float const *probes, size_t nprobes, float dt, int substeps, float *records)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const host = { bodies, motions, props, nbodies, probes, nprobes, records };
  BodyBatch dev;

  int rc = check_step_args(ctx, q, host, dt, substeps, "datum_ocean_step_bodies_host");
  if (rc != DATUM_OCEAN_OK || nbodies == 0)
    return rc;

  // bodies and motions come back beside the records
  rc = stage_batch(ctx, host, DATUM_OCEAN_STEP_RECORD_FLOATS, dev);
  if (rc == DATUM_OCEAN_OK)
    rc = run_step_bodies(ctx, q, dev, dt, substeps);

  return rc != DATUM_OCEAN_OK ? rc : fetch_batch(ctx, host, dev, DATUM_OCEAN_STEP_RECORD_FLOATS, true);
}

}   // extern "C"

/* -- the ripple layer's planes: the window read, and the wake foam's, the walls' and the bed's share of the layer's own calls --------------- */

namespace
{
  size_t ripple_cells(datum_ocean_ctx const *ctx) { return (size_t)ctx->rippleR * ctx->rippleR; }

  // a plane of the layer's in window order, from the torus in memory: the copies of ripple_window's rectangles, on the handle's stream
  // (the caller waits)
  template<typename T>
  int read_ripple_window(datum_ocean_ctx *ctx, T const *plane, T *host)
  {
    size_t const pitch = (size_t)ctx->rippleR * sizeof(T);

    RippleRect rect[4];

    int const n = ripple_window(ctx->rippleox, ctx->rippleoy, ctx->rippleR, rect);

    for(int k = 0; k < n; ++k)
      HIPCHECK(ctx, hipMemcpy2DAsync(host + rect[k].to, pitch, plane + rect[k].from, pitch, (size_t)rect[k].w * sizeof(T), (size_t)rect[k].h, hipMemcpyDeviceToHost, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // wake foam's share of set_ripples, reset_ripples and center_ripples: each does nothing while the foam is off

  int free_ripple_foam(datum_ocean_ctx *ctx)
  {
    HIPCHECK(ctx, ctx->ripplefoam.release());

    return DATUM_OCEAN_OK;
  }

  // no foam anywhere, on the handle's stream
  int clear_ripple_foam(datum_ocean_ctx *ctx)
  {
    if (ctx->ripplefoam.get())
      HIPCHECK(ctx, hipMemsetAsync(ctx->ripplefoam.get(), 0, ripple_cells(ctx) * sizeof(float), ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // the window moved from (oldx, oldy) to g's origin: the cells that entered hold no foam
  int scroll_ripple_foam(datum_ocean_ctx *ctx, RippleGrid const &g, int oldx, int oldy)
  {
    if (!ctx->ripplefoam.get())
      return DATUM_OCEAN_OK;

    RippleFoamScrollArgs a;
    a.foam = ctx->ripplefoam.get();
    a.g = g;
    a.oldx = oldx;
    a.oldy = oldy;

    HIPCHECK(ctx, launch_ripple_foam_scroll(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // what the walls' raster and the bed's take alike: the grid, the cell side and the two state buffers, which the launch writes with
  // `zero` (the ripple bounds' record is then no longer that of the current one)
  template<typename Args>
  void fill_ripple_raster(datum_ocean_ctx *ctx, RippleGrid const &g, bool zero, Args &a)
  {
    a.state[0] = ctx->ripplestate[0].get();
    a.state[1] = ctx->ripplestate[1].get();
    a.zero = zero ? 1 : 0;
    a.g = g;
    a.s = (float)ctx->ripples;

    ctx->rippleboundscurrent = ctx->rippleboundscurrent && !zero;
  }

  // the walls' share of set_ripples and center_ripples: each does nothing while walls are off

  int free_ripple_walls(datum_ocean_ctx *ctx)
  {
    HIPCHECK(ctx, ctx->ripplewall.release());
    HIPCHECK(ctx, hipFree(ctx->ripplewalllist));
    ctx->ripplewalllist = nullptr;
    ctx->ripplewallcount = 0;

    return DATUM_OCEAN_OK;
  }

  // the whole plane from the handle's list at g's origin, on the handle's stream; with `zero` the wall cells' state in both buffers too
  int raster_ripple_walls(datum_ocean_ctx *ctx, RippleGrid const &g, bool zero)
  {
    if (!ctx->ripplewall.get())
      return DATUM_OCEAN_OK;

    RippleWallRasterArgs a;
    a.wall = ctx->ripplewall.get();
    a.walls = ctx->ripplewalllist;
    a.count = ctx->ripplewallcount;
    fill_ripple_raster(ctx, g, zero, a);

    HIPCHECK(ctx, launch_ripple_wall_raster(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // the bed's share of set_ripples, center_ripples and set_ripple_walls: each does nothing while the bed is off

  int free_ripple_bed(datum_ocean_ctx *ctx)
  {
    HIPCHECK(ctx, ctx->ripplebed.release());
    HIPCHECK(ctx, ctx->ripplesurf.release());
    HIPCHECK(ctx, hipFree(ctx->ripplebedmap));
    ctx->ripplebedmap = nullptr;
    ctx->ripplebedparams = {};

    return DATUM_OCEAN_OK;
  }

  // the bed's share of a sub-step's arguments, the surf table for a sub-step of length h, rounded once from double:
  // fsurf[q] = 1 / (1 + h surf_gamma (q / 16)^2), beside the sponge table's entries: exactly 1 at q = 0
  void fill_ripple_surf(datum_ocean_ctx const *ctx, float h, float *fsurf)
  {
    for(int q = 0; q <= RIPPLE_SURF_LEVELS; ++q)
    {
      double const u = (double)q / RIPPLE_SURF_LEVELS;

      fsurf[q] = (float)(1.0 / (1.0 + (double)h * ((double)ctx->ripplebedparams.surf_gamma * (u * u))));
    }
  }

  // the bed as the arithmetic sees it (ocean_ripple_bed.h: RippleBed), for the raster and for body contact
  RippleBed ripple_bed_terms(datum_ocean_ripple_bed const &p)
  {
    RippleBed b;
    b.width = p.width;
    b.height = p.height;
    b.ox = p.origin[0];
    b.oy = p.origin[1];
    b.invt = (float)(1.0 / (double)p.texel);
    b.outside = p.outside;
    b.max_depth = p.max_depth;
    b.dry_depth = p.dry_depth;
    b.surf_depth = p.surf_depth;
    b.invsurf = p.surf_depth > 0.0f ? (float)(1.0 / (double)p.surf_depth) : 0.0f;
    return b;
  }

  // both planes whole from the handle's map, its parameters and the wall plane at g's origin, on the handle's stream (behind the wall
  // raster, where there is one); with `zero` the solid cells' state in both buffers too
  int raster_ripple_bed(datum_ocean_ctx *ctx, RippleGrid const &g, bool zero)
  {
    if (!ctx->ripplebed.get())
      return DATUM_OCEAN_OK;

    datum_ocean_ripple_bed const &p = ctx->ripplebedparams;

    RippleBedRasterArgs a;
    a.depth = ctx->ripplebed.get();
    a.surf = ctx->ripplesurf.get();
    a.map = ctx->ripplebedmap;
    a.wall = ctx->ripplewall.get();
    fill_ripple_raster(ctx, g, zero, a);

    a.b = ripple_bed_terms(p);

    HIPCHECK(ctx, launch_ripple_bed_raster(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }
}

/* -- the ripple layer (ocean_ripple.hip) ------------------------------------------------------------------------------------------ */

namespace
{
  // what every call that needs the layer refuses; `name` goes into the error text
  int check_ripples(datum_ocean_ctx *ctx, char const *name)
  {
    if (!ctx)
      return fail(nullptr, DATUM_OCEAN_EINVAL, name, ": null handle");

    if (ctx->rippleR == 0)
      return fail(ctx, DATUM_OCEAN_ESTATE, name, ": the ripple layer is off (datum_ocean_set_ripples)");

    return DATUM_OCEAN_OK;
  }

  RippleGrid ripple_grid(datum_ocean_ctx const *ctx)
  {
    RippleGrid g;
    g.R = ctx->rippleR;
    g.ox = ctx->rippleox;
    g.oy = ctx->rippleoy;
    g.invs = (float)(1.0 / ctx->ripples);
    return g;
  }

  int free_ripples(datum_ocean_ctx *ctx)
  {
    int const rc = free_ripple_foam(ctx);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    int const rcw = free_ripple_walls(ctx);
    if (rcw != DATUM_OCEAN_OK)
      return rcw;

    int const rcb = free_ripple_bed(ctx);
    if (rcb != DATUM_OCEAN_OK)
      return rcb;

    HIPCHECK(ctx, ctx->rippleswell.off());

    HIPCHECK(ctx, ctx->ripplestate[0].release());
    HIPCHECK(ctx, ctx->ripplestate[1].release());
    HIPCHECK(ctx, hipFree(ctx->ripplesrc));
    ctx->ripplesrc = nullptr;
    HIPCHECK(ctx, hipFree(ctx->rippleboundsblock));
    ctx->rippleboundsblock = nullptr;
    ctx->rippleboundscurrent = false;
    ctx->rippleR = 0;

    return DATUM_OCEAN_OK;
  }

  // water at rest: both state buffers and the pending deposits, on the handle's stream
  int clear_ripples(datum_ocean_ctx *ctx)
  {
    size_t const cells = ripple_cells(ctx);

    ctx->rippleboundscurrent = false;

    HIPCHECK(ctx, hipMemsetAsync(ctx->ripplestate[0].get(), 0, cells * sizeof(float2), ctx->stream));
    HIPCHECK(ctx, hipMemsetAsync(ctx->ripplestate[1].get(), 0, cells * sizeof(float2), ctx->stream));
    HIPCHECK(ctx, hipMemsetAsync(ctx->ripplesrc, 0, cells * sizeof(int), ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // device arrays, n > 0
  int run_ripple_samples(datum_ocean_ctx *ctx, void const *points, size_t n, void *out)
  {
    RippleSampleArgs a;
    a.state = ctx->ripplestate[ctx->ripplecurrent].get();
    a.points = static_cast<float2 const*>(points);
    a.samples = static_cast<float4*>(out);
    a.g = ripple_grid(ctx);
    a.count = (int)n;

    HIPCHECK(ctx, launch_ripple_samples(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // what both impulse deposits refuse; `name` goes into the error text
  int check_ripple_impulses(datum_ocean_ctx *ctx, void const *impulses, size_t n, char const *name)
  {
    int rc = check_ripples(ctx, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (n > 0 && !impulses)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null impulses");

    if ((uintptr_t)impulses & 15)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": impulses must be 16-byte aligned");

    if (n > (size_t)INT32_MAX / 16)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": n above INT32_MAX / 16");

    return DATUM_OCEAN_OK;
  }

  // a device array, n > 0
  int run_ripple_impulses(datum_ocean_ctx *ctx, void const *impulses, size_t n)
  {
    RippleImpulseArgs a;
    a.impulses = static_cast<float4 const*>(impulses);
    a.src = ctx->ripplesrc;
    a.g = ripple_grid(ctx);
    a.count = (int)n;

    HIPCHECK(ctx, launch_ripple_impulses(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // the layer, dt, then body drag's checks: ESTATE exactly where that call returns it once the layer is on
  int check_ripple_wake_args(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, float dt, char const *name)
  {
    int rc = check_ripples(ctx, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (!std::isfinite(dt))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": dt is not finite");

    return check_body_drag_args(ctx, q, b, name);
  }

  // device arrays, nbodies > 0
  int run_ripple_wake(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, float dt)
  {
    RippleWakeArgs a = {};
    fill_drag_args(ctx, q, b, a.d);
    a.src = ctx->ripplesrc;
    a.g = ripple_grid(ctx);
    a.dt = dt;

    HIPCHECK(ctx, launch_ripple_wake(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }

  // c h / s in double, which a step holds against the scheme's stability bound; over a bed c is the fastest speed it allows,
  // sqrt(g max_depth)
  double ripple_courant(datum_ocean_ctx const *ctx, float h)
  {
    double const c = ctx->ripplebed.get() ? std::sqrt(ctx->rippleg * (double)ctx->ripplebedparams.max_depth) : ctx->ripplec;

    return c * (double)h / ctx->ripples;
  }

  // the DEEP step's weights (ocean_ripple_deep.h), built by the first call that asks for them: the table and Sum |F| of its 169 weights
  struct RippleDeepTable
  {
    float G[RIPPLE_DEEP_WEIGHTS];
    double mass;

    RippleDeepTable() { mass = ripple_deep_weights(G); }
  };

  RippleDeepTable const &ripple_deep_table()
  {
    static RippleDeepTable const table;

    return table;
  }

  // h sqrt(g Sum |F| / s) in double, which a DEEP step holds against semi-implicit Euler's bound h Omega < 2
  double ripple_deep_bound(datum_ocean_ctx const *ctx, float h)
  {
    return (double)h * std::sqrt(ctx->rippleg * ripple_deep_table().mass / ctx->ripples);
  }

  // the stability rule of the layer's mode for a sub-step of length h; `wave` is what a refusal in the WAVE mode says behind the call's name
  int check_ripple_stability(datum_ocean_ctx *ctx, float h, char const *name, char const *wave)
  {
    if (ctx->rippledispersion == DATUM_OCEAN_RIPPLE_DEEP)
    {
      if (ripple_deep_bound(ctx, h) > 1.9)
        return fail(ctx, DATUM_OCEAN_EINVAL, name, ": dt / substeps * sqrt(g * sum|F| / s) above 1.9, the DEEP step's stability bound of 2 with a margin");
    }
    else if (ripple_courant(ctx, h) > 0.7)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, wave);

    return DATUM_OCEAN_OK;
  }

  // a sub-step in the layer's mode: the wave step's arguments (a.s, its two state buffers among them), which the DEEP step takes too,
  // and the DEEP step's own
  struct RippleStep
  {
    bool deep;
    RippleDeepStepArgs a;
    unsigned char const *wall;      // the wall plane, null while walls are off
    float const *bed;               // the bed's depth plane, null while the bed is off; then its surf plane, g / s^2 and the surf table
    unsigned char const *surf;
    float gs2;
    float fsurf[RIPPLE_SURF_LEVELS + 1];
    float const *swell;             // ripple swell's forcing plane, null while swell is off or its plane is not current
  };

  // what a sub-step of length h takes but its two state buffers: src, the grid, c2s2 and the sponge table, rounded once from double,
  // and in the DEEP mode g / s and the weights
  // (datum_ocean_step_ripples, and datum_ocean_step_bodies_coupled for the layer's share of a coupled sub-step)
  RippleStep ripple_step_args(datum_ocean_ctx const *ctx, float h)
  {
    RippleStep r = {};
    r.deep = ctx->rippledispersion == DATUM_OCEAN_RIPPLE_DEEP;
    r.wall = ctx->ripplewall.get();
    r.bed = ctx->ripplebed.get();
    r.surf = ctx->ripplesurf.get();
    r.swell = ctx->rippleswell.fresh();

    if (r.bed)
    {
      r.gs2 = (float)(ctx->rippleg / (ctx->ripples * ctx->ripples));
      fill_ripple_surf(ctx, h, r.fsurf);
    }

    if (r.deep)
    {
      r.a.gs = (float)(ctx->rippleg / ctx->ripples);
      std::memcpy(r.a.G, ripple_deep_table().G, sizeof r.a.G);
    }

    RippleStepArgs &a = r.a.s;
    a.src = ctx->ripplesrc;
    a.g = ripple_grid(ctx);
    a.B = ctx->ripplesponge;
    a.h = h;
    a.c2s2 = (float)(ctx->ripplec * ctx->ripplec / (ctx->ripples * ctx->ripples));

    for(int k = 0; k <= a.B; ++k)
    {
      double const u = a.B > 0 ? (double)k / a.B : 0.0;

      a.f[k] = (float)(1.0 / (1.0 + (double)h * (ctx->ripplegamma + ctx->ripplespongegamma * (u * u))));
    }

    return r;
  }

  // the one place where the mode, the walls, the bed and the swell choose the kernel (the name is ocean::launch_ripple_step's: a call
  // site reads the same in either mode, with walls or without, over a bed or not).  The bed's kernel runs whether walls are on or off:
  // they are in its depths; the bed and the DEEP mode do not meet (both setters refuse), nor do swell and the DEEP mode.  The swell's
  // kernels run only while its plane is current (r.swell): a stale plane is never read, the parents' kernels run instead.  Swell
  // without walls and without a bed has nothing solid and a plane of +0: the plain parent runs
  hipError_t launch_ripple_step(RippleStep &r, bool first, hipStream_t stream)
  {
    if (r.bed)
    {
      RippleBedStepArgs b;
      b.s = r.a.s;
      b.depth = r.bed;
      b.surf = r.surf;
      b.gs2 = r.gs2;
      std::memcpy(b.fsurf, r.fsurf, sizeof b.fsurf);

      if (r.swell)
      {
        RippleBedSwellStepArgs w = { b, r.swell };

        return launch_ripple_bed_swell_step(w, first, stream);
      }

      return launch_ripple_bed_step(b, first, stream);
    }

    if (r.swell && r.wall && !r.deep)
    {
      RippleWallSwellStepArgs w = { { r.a.s, r.wall }, r.swell };

      return launch_ripple_step_walls_swell(w, first, stream);
    }

    if (r.wall && r.deep)
    {
      RippleWallDeepStepArgs w = { r.a, r.wall };

      return launch_ripple_deep_step_walls(w, first, stream);
    }

    if (r.wall)
    {
      RippleWallStepArgs w = { r.a.s, r.wall };

      return launch_ripple_step_walls(w, first, stream);
    }

    return r.deep ? ocean::launch_ripple_deep_step(r.a, first, stream) : ocean::launch_ripple_step(r.a.s, first, stream);
  }

  int check_ripple_points(datum_ocean_ctx *ctx, void const *points, size_t n, void const *out, char const *name)
  {
    int rc = check_ripples(ctx, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (n > 0 && (!points || !out))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null points or out");

    if (((uintptr_t)points & 7) || ((uintptr_t)out & 15))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": points must be 8-byte and out 16-byte aligned");

    if (n > (size_t)INT32_MAX / 16)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": n above INT32_MAX / 16");

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_set_ripples(datum_ocean_t ctx, int R, float s)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripples: null handle");

  if (R != 0 && R != 64 && R != 128 && R != 256 && R != 512 && R != 1024)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripples: R must be 0, 64, 128, 256, 512 or 1024");

  if (R != 0 && !(std::isfinite(s) && s > 0.0f))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripples: s must be finite and positive");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  int rc = free_ripples(ctx);
  if (rc != DATUM_OCEAN_OK || R == 0)
    return rc;

  size_t const cells = (size_t)R * R;

  hipError_t e = ctx->ripplestate[0].allocate(cells, ctx->stream);
  if (e == hipSuccess)
    e = ctx->ripplestate[1].allocate(cells, ctx->stream);
  if (e == hipSuccess)
    e = hipMalloc(&ctx->ripplesrc, cells * sizeof(int));

  if (e != hipSuccess)
  {
    (void)free_ripples(ctx);
    return fail(ctx, (int)e, "datum_ocean_set_ripples: hipMalloc");
  }

  ctx->rippleR = R;
  ctx->ripples = (double)s;
  ctx->rippleox = ctx->rippleoy = -R / 2;
  ctx->ripplecurrent = 0;

  rc = clear_ripples(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_ripple_params(datum_ocean_t ctx, float c, float gamma, int sponge_cells, float sponge_gamma)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_params: null handle");

  if (!(std::isfinite(c) && c > 0.0f))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_params: c must be finite and positive");

  if (!std::isfinite(gamma) || gamma < 0.0f)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_params: gamma must be finite and not negative");

  if (sponge_cells < 0 || sponge_cells > DATUM_OCEAN_RIPPLE_MAX_SPONGE)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_params: sponge_cells outside [0, DATUM_OCEAN_RIPPLE_MAX_SPONGE]");

  if (!std::isfinite(sponge_gamma) || sponge_gamma < 0.0f)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_params: sponge_gamma must be finite and not negative");

  ctx->ripplec = (double)c;
  ctx->ripplegamma = (double)gamma;
  ctx->ripplesponge = sponge_cells;
  ctx->ripplespongegamma = (double)sponge_gamma;

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_ripple_dispersion(datum_ocean_t ctx, int mode, float g)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_dispersion: null handle");

  if (mode != DATUM_OCEAN_RIPPLE_WAVE && mode != DATUM_OCEAN_RIPPLE_DEEP)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_dispersion: mode must be DATUM_OCEAN_RIPPLE_WAVE or DATUM_OCEAN_RIPPLE_DEEP");

  if (!std::isfinite(g) || !(g > 0.0f))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_dispersion: g must be finite and positive");

  if (mode == DATUM_OCEAN_RIPPLE_DEEP && ctx->ripplebed.get())
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_ripple_dispersion: a ripple bed is set, and the bed and the DEEP mode do not combine (datum_ocean_set_ripple_bed)");

  if (mode == DATUM_OCEAN_RIPPLE_DEEP && ctx->rippleswell.get())
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_ripple_dispersion: ripple swell is on, and swell and the DEEP mode do not combine (datum_ocean_set_ripple_swell)");

  ctx->rippledispersion = mode;
  ctx->rippleg = (double)g;

  return DATUM_OCEAN_OK;
}

int datum_ocean_ripple_deep_weights(float *quadrant49)
{
  if (!quadrant49)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_ripple_deep_weights: null argument");

  std::memcpy(quadrant49, ripple_deep_table().G, sizeof ripple_deep_table().G);

  return DATUM_OCEAN_OK;
}

int datum_ocean_center_ripples(datum_ocean_t ctx, float x, float y)
{
  int rc = check_ripples(ctx, "datum_ocean_center_ripples");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  RippleGrid g = ripple_grid(ctx);

  if (!(ripple_coord_ok(x, g.invs) && ripple_coord_ok(y, g.invs)))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_center_ripples: x and y must be finite and within 2^30 cells");

  // the cell of (x, y) as a deposit at it would take it: one fp32 product, floor
  int const ox = (int)floorf(x * g.invs) - g.R / 2, oy = (int)floorf(y * g.invs) - g.R / 2;

  if (ox == g.ox && oy == g.oy)
    return DATUM_OCEAN_OK;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  RippleScrollArgs a;
  a.state[0] = ctx->ripplestate[0].get();
  a.state[1] = ctx->ripplestate[1].get();
  a.src = ctx->ripplesrc;
  a.oldx = g.ox;
  a.oldy = g.oy;
  g.ox = ox;
  g.oy = oy;
  a.g = g;

  ctx->rippleboundscurrent = false;
  ctx->rippleswell.current = false;

  HIPCHECK(ctx, launch_ripple_scroll(a, ctx->stream));

  rc = scroll_ripple_foam(ctx, a.g, a.oldx, a.oldy);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  rc = raster_ripple_walls(ctx, a.g, false);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  rc = raster_ripple_bed(ctx, a.g, false);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  ctx->rippleox = ox;
  ctx->rippleoy = oy;

  return DATUM_OCEAN_OK;
}

int datum_ocean_reset_ripples(datum_ocean_t ctx)
{
  int rc = check_ripples(ctx, "datum_ocean_reset_ripples");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  rc = clear_ripples(ctx);

  return rc != DATUM_OCEAN_OK ? rc : clear_ripple_foam(ctx);
}

int datum_ocean_ripples_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes, int *ox, int *oy)
{
  int rc = check_ripples(ctx, "datum_ocean_ripples_device");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!device_ptr)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_ripples_device: null argument");

  *device_ptr = ctx->ripplestate[ctx->ripplecurrent].get();

  if (bytes)
    *bytes = ripple_cells(ctx) * sizeof(float2);
  if (ox)
    *ox = ctx->rippleox;
  if (oy)
    *oy = ctx->rippleoy;

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_ripples(datum_ocean_t ctx, float *state)
{
  int rc = check_ripples(ctx, "datum_ocean_read_ripples");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!state)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_ripples: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  rc = read_ripple_window(ctx, ctx->ripplestate[ctx->ripplecurrent].get(), reinterpret_cast<float2*>(state));
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_step_ripples(datum_ocean_t ctx, float dt, int substeps)
{
  int rc = check_ripples(ctx, "datum_ocean_step_ripples");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (substeps < 1 || substeps > DATUM_OCEAN_RIPPLE_MAX_SUBSTEPS)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_step_ripples: substeps outside [1, DATUM_OCEAN_RIPPLE_MAX_SUBSTEPS]");

  // (a negative dt would turn the damping into growth: f[k] above 1, unbounded where h (gamma + gamma_e) = -1)
  if (!std::isfinite(dt) || dt < 0.0f)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_step_ripples: dt is not finite or is negative");

  float const h = substep_length(dt, substeps);

  // the wave scheme's stability bound is c h / s <= 1 / sqrt 2
  rc = check_ripple_stability(ctx, h, "datum_ocean_step_ripples", ": c * dt / (substeps * s) above 0.7, the scheme's stability bound with a margin");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  RippleStep r = ripple_step_args(ctx, h);

  ctx->rippleboundscurrent = false;

  for(int i = 0; i < substeps; ++i)
  {
    r.a.s.in = ctx->ripplestate[ctx->ripplecurrent].get();
    r.a.s.out = ctx->ripplestate[ctx->ripplecurrent ^ 1].get();

    HIPCHECK(ctx, launch_ripple_step(r, i == 0, ctx->stream));

    ctx->ripplecurrent ^= 1;

    // the first sub-step's neighbours read src too: no kernel clears it
    if (i == 0)
      HIPCHECK(ctx, hipMemsetAsync(ctx->ripplesrc, 0, ripple_cells(ctx) * sizeof(int), ctx->stream));
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_deposit_ripples(datum_ocean_t ctx, void const *impulses_device, size_t n)
{
  int rc = check_ripple_impulses(ctx, impulses_device, n, "datum_ocean_deposit_ripples");
  if (rc != DATUM_OCEAN_OK || n == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_ripple_impulses(ctx, impulses_device, n);
}

int datum_ocean_deposit_ripples_host(datum_ocean_t ctx, float const *impulses, size_t n)
{
  int rc = check_ripple_impulses(ctx, impulses, n, "datum_ocean_deposit_ripples_host");
  if (rc != DATUM_OCEAN_OK || n == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  // the surface queries' point staging; the call waits, so the caller's array is free when it returns
  Staging &in = ctx->staging[STAGE_POINTS];

  rc = in.reserve(ctx, n * sizeof(float4));
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipMemcpyAsync(in.ptr, impulses, n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));

  rc = run_ripple_impulses(ctx, in.ptr, n);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_deposit_body_ripples(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                     void const *bodies_device, void const *motions_device, size_t nbodies, void const *probes_device, size_t nprobes,
                                     float dt, void *records_device)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const b = { bodies_device, motions_device, nullptr, nbodies, probes_device, nprobes, records_device };

  int rc = check_ripple_wake_args(ctx, q, b, dt, "datum_ocean_deposit_body_ripples");
  if (rc != DATUM_OCEAN_OK || nbodies == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_ripple_wake(ctx, q, b, dt);
}

int datum_ocean_deposit_body_ripples_host(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                          datum_ocean_body const *bodies, datum_ocean_body_motion const *motions, size_t nbodies, float const *probes, size_t nprobes,
                                          float dt, float *records)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const host = { bodies, motions, nullptr, nbodies, probes, nprobes, records };
  BodyBatch dev;

  int rc = check_ripple_wake_args(ctx, q, host, dt, "datum_ocean_deposit_body_ripples_host");
  if (rc != DATUM_OCEAN_OK || nbodies == 0)
    return rc;

  rc = stage_batch(ctx, host, DATUM_OCEAN_RIPPLE_RECORD_FLOATS, dev);
  if (rc == DATUM_OCEAN_OK)
    rc = run_ripple_wake(ctx, q, dev, dt);

  return rc != DATUM_OCEAN_OK ? rc : fetch_batch(ctx, host, dev, DATUM_OCEAN_RIPPLE_RECORD_FLOATS, false);
}

int datum_ocean_sample_ripples(datum_ocean_t ctx, void const *points_device, size_t n, void *out_device)
{
  int rc = check_ripple_points(ctx, points_device, n, out_device, "datum_ocean_sample_ripples");
  if (rc != DATUM_OCEAN_OK || n == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_ripple_samples(ctx, points_device, n, out_device);
}

int datum_ocean_query_ripples(datum_ocean_t ctx, float const *points, size_t n, float *out)
{
  int rc = check_ripple_points(ctx, points, n, out, "datum_ocean_query_ripples");
  if (rc != DATUM_OCEAN_OK || n == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return read_staged(ctx, ctx->staging[STAGE_POINTS], points, n * sizeof(float2), ctx->staging[STAGE_SAMPLES], out, n * sizeof(float4),
                     [&](void const *in, void *dev) { return run_ripple_samples(ctx, in, n, dev); });
}

}   // extern "C"

/* -- ray casts (ocean_ray.hip) ---------------------------------------------------------------------------------------------------- */

namespace
{
  // the checks of the eight casts in their order: the layer where it is on top (a null handle EINVAL, the layer off ESTATE), the query, the
  // cast's own arguments and arrays, then the marks a bounded cast needs: the maps' records, and with the layer on top the layer's record
  int check_rays(datum_ocean_ctx *ctx, Query const &q, RayCall const &call, ReadVariant v, char const *name)
  {
    int rc = v.rippled ? check_ripples(ctx, name) : DATUM_OCEAN_OK;
    if (rc == DATUM_OCEAN_OK)
      rc = check_query(ctx, q, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (call.steps < 1 || call.steps > DATUM_OCEAN_RAY_MAX_STEPS)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": steps outside [1, DATUM_OCEAN_RAY_MAX_STEPS]");

    if (call.refine < 0 || call.refine > DATUM_OCEAN_RAY_MAX_REFINE)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": refine outside [0, DATUM_OCEAN_RAY_MAX_REFINE]");

    if (call.n > 0 && (!call.rays || !call.records))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null rays or records");

    if (((uintptr_t)call.rays & 15) || ((uintptr_t)call.records & 15))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": rays and records must be 16-byte aligned");

    if (call.n > (size_t)INT32_MAX)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": n above INT32_MAX");

    if (v.bounded && !ctx->boundscurrent)
      return fail(ctx, DATUM_OCEAN_ESTATE, name, ": the bounds are not current (datum_ocean_reduce_bounds after the last displace or bind_maps)");

    if (v.bounded && v.rippled && !ctx->rippleboundscurrent)
      return fail(ctx, DATUM_OCEAN_ESTATE, name, ": the ripple bounds are not current (datum_ocean_reduce_ripple_bounds after the last call that stepped, moved, reset or set the layer)");

    return DATUM_OCEAN_OK;
  }

  RayBatch ray_batch(RayCall const &call)
  {
    RayBatch r;
    r.rays = static_cast<float4 const*>(call.rays);
    r.records = static_cast<float4*>(call.records);
    r.n = (int)call.n;
    r.steps = call.steps;
    r.refine = call.refine;
    r.inv = 0.0f;           // ray_launch
    return r;
  }

  // the list as cascade numbers, as the bounded kernels index the handle's records
  void list_cascades(Query const &q, int *cascades)
  {
    for(int c = 0; c < DATUM_OCEAN_MAX_CASCADES; ++c)
      cascades[c] = (c < q.count) ? q.cascades[c] : 0;
  }

  // device arrays, n > 0: the variant's kernel argument filled from the one query and the one batch, and its launch
  int run_rays(datum_ocean_ctx *ctx, Query const &q, RayCall const &call, ReadVariant v)
  {
    RayArgs a;
    a.q = query_args(ctx, q);
    a.r = ray_batch(call);

    if (!v.rippled && !v.bounded)
      HIPCHECK(ctx, launch_rays(a, ctx->stream));
    else if (!v.rippled)
    {
      RayBoundedArgs b;
      b.q = a.q;
      b.r = a.r;
      b.bounds = reinterpret_cast<float const*>(ctx->bounds);
      list_cascades(q, b.cascades);

      HIPCHECK(ctx, launch_rays_bounded(b, ctx->stream));
    }
    else if (!v.bounded)
    {
      RayRippledArgs r = { a, rippled_layer(ctx) };

      HIPCHECK(ctx, launch_rays_rippled(r, ctx->stream));
    }
    else
    {
      RayRippledBoundedArgs b;
      b.r.a = a;
      b.r.layer = rippled_layer(ctx);
      b.bounds = reinterpret_cast<float const*>(ctx->bounds);
      b.layerbounds = reinterpret_cast<float const*>(ripple_bounds_record(ctx));
      list_cascades(q, b.cascades);

      HIPCHECK(ctx, launch_rays_rippled_bounded(b, ctx->stream));
    }

    return DATUM_OCEAN_OK;
  }

  // a cast on device arrays
  int cast_rays(datum_ocean_ctx *ctx, Query const &q, RayCall const &call, ReadVariant v, char const *name)
  {
    int rc = check_rays(ctx, q, call, v, name);
    if (rc != DATUM_OCEAN_OK || call.n == 0)
      return rc;

    HIPCHECK(ctx, hipSetDevice(ctx->device));

    return run_rays(ctx, q, call, v);
  }

  // ... and its host twin: `n` rays in, a record per ray out
  int read_rays(datum_ocean_ctx *ctx, Query const &q, RayCall const &call, ReadVariant v, char const *name)
  {
    int rc = check_rays(ctx, q, call, v, name);
    if (rc != DATUM_OCEAN_OK || call.n == 0)
      return rc;

    HIPCHECK(ctx, hipSetDevice(ctx->device));

    return read_staged(ctx, ctx->staging[STAGE_RAYS], call.rays, call.n * RAY_BYTES, ctx->staging[STAGE_RAY_RECORDS], call.records, call.n * RAY_RECORD_BYTES,
                       [&](void const *in, void *out) { return run_rays(ctx, q, RayCall{ call.steps, call.refine, in, call.n, out }, v); });
  }
}

extern "C"
{

int datum_ocean_cast_rays(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                          void const *rays_device, size_t n, void *records_device)
{
  Query const q = { cascades, count, set, iterations };
  RayCall const call = { steps, refine, rays_device, n, records_device };

  return cast_rays(ctx, q, call, ReadVariant{ false, false }, "datum_ocean_cast_rays");
}

int datum_ocean_read_rays(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                          float const *rays, size_t n, float *records)
{
  Query const q = { cascades, count, set, iterations };
  RayCall const call = { steps, refine, rays, n, records };

  return read_rays(ctx, q, call, ReadVariant{ false, false }, "datum_ocean_read_rays");
}

}   // extern "C"

/* -- surface bounds and the bounded ray casts (ocean_bounds.hip) ------------------------------------------------------------------------ */

namespace
{
  // the records and the partials, allocated by the first reduce, and the two launches
  int reduce_bounds(datum_ocean_ctx *ctx)
  {
    HIPCHECK(ctx, hipSetDevice(ctx->device));

    if (!ctx->bounds)
    {
      int const groups = bounds_groups(ctx->N, ctx->cascades);

      float4 *records = nullptr, *partials = nullptr;

      HIPCHECK(ctx, hipMalloc(&records, (size_t)ctx->cascades * BOUNDS_BYTES));

      hipError_t const e = hipMalloc(&partials, (size_t)ctx->cascades * groups * BOUNDS_BYTES);

      if (e != hipSuccess)
      {
        (void)hipFree(records);
        return fail(ctx, (int)e, "datum_ocean_reduce_bounds: hipMalloc");
      }

      ctx->bounds = records;
      ctx->boundspartials = partials;
      ctx->boundsgroups = groups;
    }

    BoundsArgs a;
    a.maps = ctx->maps.get();
    a.partials = ctx->boundspartials;
    a.records = ctx->bounds;
    a.N = ctx->N;
    a.groups = ctx->boundsgroups;

    HIPCHECK(ctx, launch_bounds(a, ctx->cascades, ctx->stream));

    ctx->boundscurrent = true;

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_reduce_bounds(datum_ocean_t ctx)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_reduce_bounds: null handle");

  return reduce_bounds(ctx);
}

int datum_ocean_bounds_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes)
{
  if (!ctx || !device_ptr)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_bounds_device: null argument");

  if (!ctx->bounds)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_bounds_device: no records yet (datum_ocean_reduce_bounds)");

  *device_ptr = ctx->bounds;

  if (bytes)
    *bytes = (size_t)ctx->cascades * BOUNDS_BYTES;

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_bounds(datum_ocean_t ctx, float *records)
{
  if (!ctx || !records)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_bounds: null argument");

  int rc = reduce_bounds(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipMemcpyAsync(records, ctx->bounds, (size_t)ctx->cascades * BOUNDS_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_surface_slab(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, float *zlo, float *zhi, float *reachx, float *reachy)
{
  Query const q = { cascades, count, set, 0 };
  int rc = check_blend_list(ctx, q, "datum_ocean_surface_slab");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!set)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_surface_slab: null set");

  float records[DATUM_OCEAN_MAX_CASCADES * BOUNDS_FIELDS];

  rc = datum_ocean_read_bounds(ctx, records);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  GenFrame const f = make_gen_frame(*set, ctx->N, 2, 2);      // the camera's terms are not read

  BoundsSlab const s = bounds_slab(records, cascades, count, f.basez, set->swellamplitude, f.gx, f.gy);

  if (zlo) *zlo = s.zlo;
  if (zhi) *zhi = s.zhi;
  if (reachx) *reachx = s.reachx;
  if (reachy) *reachy = s.reachy;

  return DATUM_OCEAN_OK;
}

int datum_ocean_cast_rays_bounded(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                  void const *rays_device, size_t n, void *records_device)
{
  Query const q = { cascades, count, set, iterations };
  RayCall const call = { steps, refine, rays_device, n, records_device };

  return cast_rays(ctx, q, call, ReadVariant{ false, true }, "datum_ocean_cast_rays_bounded");
}

int datum_ocean_read_rays_bounded(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                  float const *rays, size_t n, float *records)
{
  Query const q = { cascades, count, set, iterations };
  RayCall const call = { steps, refine, rays, n, records };

  return read_rays(ctx, q, call, ReadVariant{ false, true }, "datum_ocean_read_rays_bounded");
}

}   // extern "C"

/* -- coupled stepping (ocean_couple.hip) -------------------------------------------------------------------------------------------- */

namespace
{
  // the layer and the ripple step's rule for dt, then body stepping's checks (ESTATE exactly where body drag returns it once the layer is
  // on), then the ripple step's stability bound for the sub-step; `name` goes into the error text
  int check_coupled_args(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, float dt, int substeps, char const *name)
  {
    int rc = check_ripples(ctx, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (!std::isfinite(dt) || dt < 0.0f)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": dt is not finite or is negative");

    rc = check_step_args(ctx, q, b, dt, substeps, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    return check_ripple_stability(ctx, substep_length(dt, substeps), name, ": c * dt / (substeps * s) above 0.7, the ripple step's stability bound with a margin");
  }

  // device arrays; `substeps` rounds of: the bodies' coupled sub-step (nbodies > 0), then the layer's sub-step in its first form.  With
  // `scene` (body contact's share of the arguments, filled in by its caller) the bodies' sub-step is body contact's kernel, everything
  // else the same
  int run_step_bodies_coupled(datum_ocean_ctx *ctx, Query const &q, BodyBatch const &b, float dt, int substeps, ContactArgs *scene = nullptr)
  {
    float const h = substep_length(dt, substeps);

    ContactArgs plain = {};
    ContactArgs &ca = scene ? *scene : plain;

    CoupleArgs &a = ca.c;
    fill_drag_args(ctx, q, b, a.d);
    a.bodies = const_cast<datum_ocean_body*>(a.d.b.bodies);             // (writable, as the step's)
    a.motions = const_cast<datum_ocean_body_motion*>(a.d.motions);
    a.props = static_cast<datum_ocean_body_props const*>(b.props);
    a.src = ctx->ripplesrc;
    a.g = ripple_grid(ctx);
    a.h = h;

    RippleStep r = ripple_step_args(ctx, h);

    ctx->rippleboundscurrent = false;

    for(int i = 0; i < substeps; ++i)
    {
      if (b.nbodies > 0)
      {
        a.state = ctx->ripplestate[ctx->ripplecurrent].get();
        a.first = i == 0;

        HIPCHECK(ctx, scene ? launch_contact(ca, ctx->stream) : launch_couple(a, ctx->stream));
      }

      // datum_ocean_step_ripples(h, 1): the first form takes the deposits in, and no kernel clears src
      r.a.s.in = ctx->ripplestate[ctx->ripplecurrent].get();
      r.a.s.out = ctx->ripplestate[ctx->ripplecurrent ^ 1].get();

      HIPCHECK(ctx, launch_ripple_step(r, true, ctx->stream));

      ctx->ripplecurrent ^= 1;

      HIPCHECK(ctx, hipMemsetAsync(ctx->ripplesrc, 0, ripple_cells(ctx) * sizeof(int), ctx->stream));
    }

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_step_bodies_coupled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                    void *bodies_device, void *motions_device, void const *props_device, size_t nbodies, void const *probes_device, size_t nprobes,
                                    float dt, int substeps, void *records_device)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const b = { bodies_device, motions_device, props_device, nbodies, probes_device, nprobes, records_device };

  int rc = check_coupled_args(ctx, q, b, dt, substeps, "datum_ocean_step_bodies_coupled");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_step_bodies_coupled(ctx, q, b, dt, substeps);
}

int datum_ocean_step_bodies_coupled_host(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                         datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, size_t nbodies,
                                         float const *probes, size_t nprobes, float dt, int substeps, float *records)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const host = { bodies, motions, props, nbodies, probes, nprobes, records };
  BodyBatch dev;

  int rc = check_coupled_args(ctx, q, host, dt, substeps, "datum_ocean_step_bodies_coupled_host");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  // (no body: nothing is staged or copied, and the layer still steps)
  rc = stage_batch(ctx, host, DATUM_OCEAN_COUPLED_RECORD_FLOATS, dev);
  if (rc == DATUM_OCEAN_OK)
    rc = run_step_bodies_coupled(ctx, q, dev, dt, substeps);

  return rc != DATUM_OCEAN_OK ? rc : fetch_batch(ctx, host, dev, DATUM_OCEAN_COUPLED_RECORD_FLOATS, true);
}

}   // extern "C"

/* -- body contact (ocean_contact.hip): the coupled call's checks and loop, and the contact's own ---------------------------------------- */

namespace
{
  // behind check_coupled_args: the parameters, then the objects the flags ask for
  int check_contact_args(datum_ocean_ctx *ctx, datum_ocean_body_contact const *c, char const *name)
  {
    if (!c)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null contact");

    for(float v : { c->stiffness, c->damping, c->friction })
      if (!std::isfinite(v) || v < 0.0f)
        return fail(ctx, DATUM_OCEAN_EINVAL, name, ": stiffness, damping and friction must be finite and not negative");

    if (c->flags & ~CONTACT_FLAGS)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": unknown flag bits");

    if ((c->flags & DATUM_OCEAN_CONTACT_BED) && !ctx->ripplebedmap)
      return fail(ctx, DATUM_OCEAN_ESTATE, name, ": DATUM_OCEAN_CONTACT_BED and no bed is set (datum_ocean_set_ripple_bed)");

    if ((c->flags & DATUM_OCEAN_CONTACT_WALLS) && !ctx->ripplewalllist)
      return fail(ctx, DATUM_OCEAN_ESTATE, name, ": DATUM_OCEAN_CONTACT_WALLS and no walls are set (datum_ocean_set_ripple_walls)");

    return DATUM_OCEAN_OK;
  }

  // body contact's share of the kernel's arguments: the parameters, and the map and the list only where their flag is set
  ContactArgs contact_scene(datum_ocean_ctx const *ctx, datum_ocean_body_contact const &c)
  {
    ContactArgs ca = {};
    ca.s.k = c;

    if (c.flags & DATUM_OCEAN_CONTACT_BED)
    {
      ca.s.bed = ripple_bed_terms(ctx->ripplebedparams);
      ca.map = ctx->ripplebedmap;
    }

    if (c.flags & DATUM_OCEAN_CONTACT_WALLS)
    {
      ca.s.walls = ctx->ripplewalllist;
      ca.s.nwalls = ctx->ripplewallcount;
    }

    return ca;
  }
}

extern "C"
{

int datum_ocean_step_bodies_contact(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                    void *bodies_device, void *motions_device, void const *props_device, size_t nbodies, void const *probes_device, size_t nprobes,
                                    float dt, int substeps, void *records_device, datum_ocean_body_contact const *contact)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const b = { bodies_device, motions_device, props_device, nbodies, probes_device, nprobes, records_device };

  int rc = check_coupled_args(ctx, q, b, dt, substeps, "datum_ocean_step_bodies_contact");
  if (rc == DATUM_OCEAN_OK)
    rc = check_contact_args(ctx, contact, "datum_ocean_step_bodies_contact");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  ContactArgs scene = contact_scene(ctx, *contact);

  return run_step_bodies_coupled(ctx, q, b, dt, substeps, &scene);
}

int datum_ocean_step_bodies_contact_host(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations,
                                         datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, size_t nbodies,
                                         float const *probes, size_t nprobes, float dt, int substeps, float *records, datum_ocean_body_contact const *contact)
{
  Query const q = { cascades, count, set, iterations };
  BodyBatch const host = { bodies, motions, props, nbodies, probes, nprobes, records };
  BodyBatch dev;

  int rc = check_coupled_args(ctx, q, host, dt, substeps, "datum_ocean_step_bodies_contact_host");
  if (rc == DATUM_OCEAN_OK)
    rc = check_contact_args(ctx, contact, "datum_ocean_step_bodies_contact_host");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  ContactArgs scene = contact_scene(ctx, *contact);

  rc = stage_batch(ctx, host, DATUM_OCEAN_CONTACT_RECORD_FLOATS, dev);
  if (rc == DATUM_OCEAN_OK)
    rc = run_step_bodies_coupled(ctx, q, dev, dt, substeps, &scene);

  return rc != DATUM_OCEAN_OK ? rc : fetch_batch(ctx, host, dev, DATUM_OCEAN_CONTACT_RECORD_FLOATS, true);
}

}   // extern "C"

/* -- rippled reads: the layer in the mesh, the surface query and the ray cast (ocean_rippled.hip) ---------------------------------------- */

namespace
{
  // the layer's current state as a read sees it (the buffer datum_ocean_ripples_device returns)
  RippledLayer rippled_layer(datum_ocean_ctx const *ctx)
  {
    RippledLayer l;
    l.state = ctx->ripplestate[ctx->ripplecurrent].get();
    l.g = ripple_grid(ctx);
    return l;
  }
}

extern "C"
{

// (each is its parent call with the layer on top: the layer's check first, then the parent's own under this call's name)

int datum_ocean_gen_blend_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int sizex, int sizey, void *vertices_device)
{
  Query const q = { cascades, count, set, 0 };

  return gen_blend(ctx, q, sizex, sizey, vertices_device, true, "datum_ocean_gen_blend_rippled");
}

int datum_ocean_sample_surface_blend_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, void const *points_device, size_t n, void *samples_device)
{
  Query const q = { cascades, count, set, iterations };

  return sample_surface_blend(ctx, q, points_device, n, samples_device, true, "datum_ocean_sample_surface_blend_rippled");
}

int datum_ocean_read_surface_blend_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, float const *points, size_t n, float *samples)
{
  Query const q = { cascades, count, set, iterations };

  return read_surface_blend(ctx, q, points, n, samples, true, "datum_ocean_read_surface_blend_rippled");
}

int datum_ocean_cast_rays_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                  void const *rays_device, size_t n, void *records_device)
{
  Query const q = { cascades, count, set, iterations };
  RayCall const call = { steps, refine, rays_device, n, records_device };

  return cast_rays(ctx, q, call, ReadVariant{ true, false }, "datum_ocean_cast_rays_rippled");
}

int datum_ocean_read_rays_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                  float const *rays, size_t n, float *records)
{
  Query const q = { cascades, count, set, iterations };
  RayCall const call = { steps, refine, rays, n, records };

  return read_rays(ctx, q, call, ReadVariant{ true, false }, "datum_ocean_read_rays_rippled");
}

}   // extern "C"

// a cascade's maps as the reference's 2-layer RGBA32F image (datum_ocean_export_maps); one thread per texel.  LAYOUT (up to 1024^2): in the
// order of the map layout like the pack kernel -- consecutive lanes read consecutive parts A and B of a patch, 16-byte stores in runs of
// a patch row (1024^2: 13.0 -> 9.3 us); otherwise in the order of the image -- from 2048^2 up, beyond the Infinity Cache, whole lines
// written count for more than whole lines read (2048^2: 35.4 against 38.0 us, 4096^2: 228 against 240 us; profiles/r05_pack.txt)
template<bool LAYOUT>
__global__ void __launch_bounds__(256) ocean_export_kernel(char const *maps, int N, float4 *dst, ocean::PackShape sh)
{
  size_t const P = (size_t)N * N;

  for(size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < P; r += (size_t)gridDim.x * blockDim.x)
  {
    size_t i, oa, ob;

    if constexpr (LAYOUT)
    {
      ocean::MapPart const m = ocean::map_part(sh, r);

      oa = m.a;
      ob = m.b;
      i = ((size_t)m.y << sh.n2) + m.x;
    }
    else
    {
      int const y = (int)(r >> sh.n2), x = (int)(r & (N - 1));

      oa = ocean::map_compact_a(N, y, x);
      ob = ocean::map_compact_b(N, y, x);
      i = r;
    }

    float4 const a = *reinterpret_cast<float4 const*>(maps + oa);
    float2 const b = *reinterpret_cast<float2 const*>(maps + ob);

    dst[i] = make_float4(a.x, a.y, a.z, 0.0f);
    dst[P + i] = make_float4(a.w, b.x, b.y, 0.0f);
  }
}

extern "C"
{

int datum_ocean_export_maps(datum_ocean_t ctx, int cascade, void *device_dst, size_t bytes)
{
  if (!ctx || !device_dst)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_export_maps: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_export_maps: cascade out of range");

  if (bytes < 2 * plane(ctx) * sizeof(float4))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_export_maps: destination smaller than 2 * N * N * 16 bytes");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  size_t const P = plane(ctx);
  int const blocks = (int)((P + 255) / 256 < 4096 ? (P + 255) / 256 : 4096);

  char const *block = map_block(ctx, cascade);

  if (ctx->N <= 1024)
    hipLaunchKernelGGL(ocean_export_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, block, ctx->N, static_cast<float4*>(device_dst), pack_shape(ctx->N));
  else
    hipLaunchKernelGGL(ocean_export_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, block, ctx->N, static_cast<float4*>(device_dst), pack_shape(ctx->N));

  HIPCHECK(ctx, hipGetLastError());

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_literal_transform(datum_ocean_t ctx, int on)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_literal_transform: null handle");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  // (profiling samples and the fp16 spectrum format belong to the fused kernels: refused together with the literal mode rather than ignored)
  if (on && ctx->profiling)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_literal_transform: a profile is open (datum_ocean_profile_end first): the literal mode's dispatches are not sampled");

  if (on && ctx->half)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_literal_transform: the handle stores an fp16 spectrum (datum_ocean_set_spectrum_format): the literal mode is the reference's fp32 arithmetic");

  if (on && !ctx->litfields)
  {
    size_t const P = plane(ctx);

    int stages = 0;
    while ((1 << stages) < ctx->N)
      ++stages;

    std::vector<float> weights;
    try { weights.resize((size_t)ctx->N * 2 * stages); } catch (...) { return fail(ctx, DATUM_OCEAN_ENOMEM, "datum_ocean_set_literal_transform: out of host memory"); }

    int rc = datum_ocean_reference_weights(ctx->N, weights.data());
    if (rc != DATUM_OCEAN_OK)
      return rc;

    // both buffers or neither: a failure between the two must not leave one behind for the next call to allocate over
    float *lw = nullptr;
    float2 *lf = nullptr;

    hipError_t e = hipMalloc(&lw, weights.size() * sizeof(float));

    if (e == hipSuccess)
      e = hipMalloc(&lf, 3 * P * sizeof(float2));

    if (e == hipSuccess)
      e = hipMemcpyAsync(lw, weights.data(), weights.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream);

    if (e == hipSuccess)
      e = hipStreamSynchronize(ctx->stream);       // (the host vector goes out of scope)

    if (e != hipSuccess)
    {
      (void)hipFree(lw);
      (void)hipFree(lf);

      return fail(ctx, (int)e, "datum_ocean_set_literal_transform: buffers of the literal mode");
    }

    ctx->litweights = lw;
    ctx->litfields = lf;
  }

  ctx->literal = on != 0;

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_cascade_group(datum_ocean_t ctx, int cascades_per_launch)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_cascade_group: null handle");

  if (cascades_per_launch < 0)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_cascade_group: negative group");

  if (ctx->profiling)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_cascade_group: a profile is open (its samples are per group)");

  ctx->cascadegroup = cascades_per_launch;

  return DATUM_OCEAN_OK;
}

int datum_ocean_cascade_group(datum_ocean_t ctx, int *cascades_per_launch, int *launches_per_pass)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_cascade_group: null handle");

  StepPlan const plan = plan_step(ctx);

  if (cascades_per_launch) *cascades_per_launch = plan.group;
  if (launches_per_pass) *launches_per_pass = plan.groups;

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_map_store_policy(datum_ocean_t ctx, int policy)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_map_store_policy: null handle");

  if (policy != DATUM_OCEAN_MAPS_AUTO && policy != DATUM_OCEAN_MAPS_WRITTEN_THROUGH && policy != DATUM_OCEAN_MAPS_STREAMED)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_map_store_policy: unknown policy");

  if (ctx->profiling)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_map_store_policy: a profile is open (the policy can change the cascade groups its samples are per)");

  ctx->mappolicy = policy;

  return DATUM_OCEAN_OK;
}

int datum_ocean_map_store_policy(datum_ocean_t ctx, int *policy, int *streamed)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_map_store_policy: null handle");

  if (policy) *policy = ctx->mappolicy;
  if (streamed) *streamed = plan_step(ctx).streamed ? 1 : 0;

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_phase_writeback(datum_ocean_t ctx, int every)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_phase_writeback: null handle");

  if (every < 0 || every > MAX_PENDING)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_phase_writeback: the interval is 1 ... 8 row passes, or 0 for the module's choice");

  if (ctx->profiling)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_phase_writeback: a profile is open (its row-pass samples are with the interval it began with)");

  // (dt's retained under the old interval need no flush: the next row pass takes them and stores if the new interval says so)
  ctx->writebackevery = every;

  return DATUM_OCEAN_OK;
}

int datum_ocean_phase_writeback(datum_ocean_t ctx, int *every)
{
  if (!ctx || !every)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_phase_writeback: null argument");

  *every = plan_step(ctx).writeback;

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_phase_store(datum_ocean_t ctx, int mode)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_phase_store: null handle");

  if (mode != DATUM_OCEAN_PHASE_STORE_AUTO && mode != DATUM_OCEAN_PHASE_STORE_PLANE)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_phase_store: unknown mode");

  if (ctx->profiling)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_phase_store: a profile is open (its row-pass samples are with the phase store it began with)");

  if (mode == ctx->phasestore)
    return DATUM_OCEAN_OK;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  ctx->phasestore = mode;

  // (table and plane are behind the handle's phase by the same retained dt's: neither move needs them flushed)
  for(int c = 0; c < ctx->cascades; ++c)
  {
    int rc = DATUM_OCEAN_OK;

    if (mode == DATUM_OCEAN_PHASE_STORE_PLANE)
      rc = leave_quadrant(ctx, c);
    else if (!ctx->cstate[c].wild)
    {
      bool wild = false;

      rc = inspect_phase(ctx, c, 0, &wild);
    }

    if (rc != DATUM_OCEAN_OK)
      return rc;
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_phase_store(datum_ocean_t ctx, int *mode, unsigned int *quadrants)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_phase_store: null handle");

  if (mode) *mode = ctx->phasestore;
  if (quadrants) *quadrants = quadrant_mask(ctx);

  return DATUM_OCEAN_OK;
}

int datum_ocean_abi_version(void)
{
  return DATUM_OCEAN_ABI_VERSION;
}

int datum_ocean_sync(datum_ocean_t ctx)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_sync: null handle");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_wait_event(datum_ocean_t ctx, void *hip_event)
{
  if (!ctx || !hip_event)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_wait_event: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamWaitEvent(ctx->stream, (hipEvent_t)hip_event, 0));

  return DATUM_OCEAN_OK;
}

int datum_ocean_signal(datum_ocean_t ctx, void **hip_event)
{
  if (!ctx || !hip_event)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_signal: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  if (!ctx->complete)
    HIPCHECK(ctx, hipEventCreateWithFlags(&ctx->complete, hipEventDisableTiming));

  HIPCHECK(ctx, hipEventRecord(ctx->complete, ctx->stream));

  *hip_event = ctx->complete;

  return DATUM_OCEAN_OK;
}

int datum_ocean_on_complete(datum_ocean_t ctx, void (*callback)(void *user), void *user)
{
  if (!ctx || !callback)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_on_complete: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipLaunchHostFunc(ctx->stream, callback, user));

  return DATUM_OCEAN_OK;
}

int datum_ocean_query(datum_ocean_t ctx)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_query: null handle");

  if (!ctx->complete)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_query: datum_ocean_signal first");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  hipError_t const e = hipEventQuery(ctx->complete);

  if (e == hipErrorNotReady)
  {
    (void)hipGetLastError();
    return DATUM_OCEAN_ENOTREADY;
  }

  HIPCHECK(ctx, e);

  return DATUM_OCEAN_OK;
}

int datum_ocean_import_memory_fd(datum_ocean_t ctx, int fd, size_t bytes, void **device_ptr)
{
  if (!ctx || !device_ptr)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_import_memory_fd: null argument");

  *device_ptr = nullptr;

  if (fd < 0 || bytes == 0)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_import_memory_fd: bad descriptor or size");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  hipExternalMemoryHandleDesc desc = {};
  desc.type = hipExternalMemoryHandleTypeOpaqueFd;       // VK_EXTERNAL_MEMORY_HANDLE_TYPE_OPAQUE_FD_BIT
  desc.handle.fd = fd;
  desc.size = bytes;

  hipExternalMemory_t memory = nullptr;

  HIPCHECK(ctx, hipImportExternalMemory(&memory, &desc));

  hipExternalMemoryBufferDesc buffer = {};
  buffer.offset = 0;
  buffer.size = bytes;

  void *ptr = nullptr;

  hipError_t e = hipExternalMemoryGetMappedBuffer(&ptr, memory, &buffer);

  if (e != hipSuccess || !ptr)
  {
    (void)hipDestroyExternalMemory(memory);
    return fail(ctx, e != hipSuccess ? (int)e : DATUM_OCEAN_ENOMEM, "hipExternalMemoryGetMappedBuffer");
  }

  ctx->importedmemory.push_back({ memory, ptr, bytes });

  *device_ptr = ptr;

  return DATUM_OCEAN_OK;
}

int datum_ocean_release_memory(datum_ocean_t ctx, void *device_ptr)
{
  if (!ctx || !device_ptr)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_release_memory: null argument");

  for(size_t i = 0; i < ctx->importedmemory.size(); ++i)
  {
    if (ctx->importedmemory[i].ptr == device_ptr)
    {
      HIPCHECK(ctx, hipSetDevice(ctx->device));
      HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));    // nothing enqueued may still write it

      // a plane bound inside the block is the handle's own again (a VkBuffer commonly sits at an offset inside its VkDeviceMemory: the
      // maps or the foam plane may be bound anywhere inside it)
      char const *lo = static_cast<char const*>(device_ptr), *hi = lo + ctx->importedmemory[i].bytes;
      auto inside = [lo, hi](void const *p) { return static_cast<char const*>(p) >= lo && static_cast<char const*>(p) < hi; };

      // (other maps from here on, as after datum_ocean_bind_maps: the bounds records are no longer theirs)
      if (inside(ctx->maps.bound))
      {
        ctx->maps.bound = nullptr;
        ctx->boundscurrent = false;
      }

      if (inside(ctx->foam.bound))
        ctx->foam.bound = nullptr;

      if (inside(ctx->velocity.bound))
      {
        ctx->velocity.bound = nullptr;
        ctx->velocitycurrent = false;
      }

      hipError_t e = hipDestroyExternalMemory(ctx->importedmemory[i].memory);

      ctx->importedmemory.erase(ctx->importedmemory.begin() + i);

      if (e != hipSuccess)
        return fail(ctx, (int)e, "hipDestroyExternalMemory");

      return DATUM_OCEAN_OK;
    }
  }

  return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_release_memory: not a pointer this handle imported");
}

int datum_ocean_import_semaphore_fd(datum_ocean_t ctx, int fd, void **semaphore)
{
  if (!ctx || !semaphore)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_import_semaphore_fd: null argument");

  *semaphore = nullptr;

  if (fd < 0)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_import_semaphore_fd: bad descriptor");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  hipExternalSemaphoreHandleDesc desc = {};
  desc.type = hipExternalSemaphoreHandleTypeOpaqueFd;    // VK_EXTERNAL_SEMAPHORE_HANDLE_TYPE_OPAQUE_FD_BIT
  desc.handle.fd = fd;

  hipExternalSemaphore_t sem = nullptr;

  hipError_t const e = hipImportExternalSemaphore(&sem, &desc);

  if (e == hipErrorNotSupported)
  {
    (void)hipGetLastError();
    return fail(ctx, DATUM_OCEAN_EUNSUPPORTED, "datum_ocean_import_semaphore_fd: this HIP runtime has no external semaphores (hipImportExternalSemaphore: not supported); "
                                               "bridge rendercomplete on the host: datum_ocean_on_complete or datum_ocean_signal + datum_ocean_query");
  }

  HIPCHECK(ctx, e);

  ctx->importedsemaphores.push_back(sem);

  *semaphore = sem;

  return DATUM_OCEAN_OK;
}

namespace
{
  static bool owns_semaphore(datum_ocean_ctx *ctx, void *semaphore)
  {
    for(hipExternalSemaphore_t s : ctx->importedsemaphores)
      if (s == semaphore)
        return true;

    return false;
  }
}

int datum_ocean_release_semaphore(datum_ocean_t ctx, void *semaphore)
{
  if (!ctx || !semaphore || !owns_semaphore(ctx, semaphore))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_release_semaphore: not a semaphore this handle imported");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  for(size_t i = 0; i < ctx->importedsemaphores.size(); ++i)
    if (ctx->importedsemaphores[i] == semaphore)
      ctx->importedsemaphores.erase(ctx->importedsemaphores.begin() + i--);

  HIPCHECK(ctx, hipDestroyExternalSemaphore((hipExternalSemaphore_t)semaphore));

  return DATUM_OCEAN_OK;
}

int datum_ocean_signal_external(datum_ocean_t ctx, void *semaphore)
{
  if (!ctx || !semaphore || !owns_semaphore(ctx, semaphore))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_signal_external: not a semaphore this handle imported");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  hipExternalSemaphore_t sem = (hipExternalSemaphore_t)semaphore;
  hipExternalSemaphoreSignalParams params = {};

  HIPCHECK(ctx, hipSignalExternalSemaphoresAsync(&sem, &params, 1, ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_wait_external(datum_ocean_t ctx, void *semaphore)
{
  if (!ctx || !semaphore || !owns_semaphore(ctx, semaphore))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_wait_external: not a semaphore this handle imported");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  hipExternalSemaphore_t sem = (hipExternalSemaphore_t)semaphore;
  hipExternalSemaphoreWaitParams params = {};

  HIPCHECK(ctx, hipWaitExternalSemaphoresAsync(&sem, &params, 1, ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_device_alloc(datum_ocean_t ctx, size_t bytes, void **device_ptr)
{
  if (!ctx || !device_ptr || bytes == 0)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_device_alloc: bad argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipMalloc(device_ptr, bytes));

  return DATUM_OCEAN_OK;
}

int datum_ocean_device_free(datum_ocean_t ctx, void *device_ptr)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_device_free: null handle");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHECK(ctx, hipFree(device_ptr));

  return DATUM_OCEAN_OK;
}

int datum_ocean_device_write(datum_ocean_t ctx, void *device_dst, void const *host_src, size_t bytes)
{
  if (!ctx || !device_dst || !host_src)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_device_write: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipMemcpyAsync(device_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_device_read(datum_ocean_t ctx, void *host_dst, void const *device_src, size_t bytes)
{
  if (!ctx || !host_dst || !device_src)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_device_read: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

char const *datum_ocean_last_error(datum_ocean_t ctx)
{
  return ctx ? ctx->error.c_str() : g_error.c_str();
}

int datum_ocean_reference_weights(int resolution, float *weights)
{
  if (!supported(resolution) || !weights)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_reference_weights: bad argument");

  int stages = 0;
  while ((1 << stages) < resolution)
    ++stages;

  float const pi = 3.14159265358979323846f;

  // lane i, stage n: angle = -2 pi i / 2^(n+1), all in fp32 as the reference evaluates it
  for(int i = 0; i < resolution; ++i)
  {
    float *row = weights + (size_t)i * 2 * stages;

    for(int n = 0; n < stages; ++n)
    {
      float angle = -2 * pi * i / (2 * powf(2.0f, (float)n));

      row[2*n+0] = cosf(angle);
      row[2*n+1] = sinf(angle);
    }
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_debug_sim(datum_ocean_t ctx, int cascade, float *h, float *hx, float *hy)
{
  if (!ctx || !h || !hx || !hy)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_debug_sim: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_debug_sim: cascade out of range");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  int rc = flush_phase(ctx);
  if (rc == DATUM_OCEAN_OK)
    rc = materialise(ctx, cascade);
  if (rc == DATUM_OCEAN_OK)
    rc = ensure_scratch(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  size_t const P = plane(ctx);

  StepArgs a = make_args(ctx, 0, nullptr);

  if (ctx->cstate[cascade].wild)
    hipLaunchKernelGGL(ocean_sim_kernel<true>, dim3(1024), dim3(256), 0, ctx->stream, a, ctx->N, cascade, ctx->scratch, ctx->scratch + P, ctx->scratch + 2 * P);
  else
    hipLaunchKernelGGL(ocean_sim_kernel<false>, dim3(1024), dim3(256), 0, ctx->stream, a, ctx->N, cascade, ctx->scratch, ctx->scratch + P, ctx->scratch + 2 * P);
  HIPCHECK(ctx, hipGetLastError());

  HIPCHECK(ctx, hipMemcpyAsync(h, ctx->scratch, P * sizeof(cf), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipMemcpyAsync(hx, ctx->scratch + P, P * sizeof(cf), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipMemcpyAsync(hy, ctx->scratch + 2 * P, P * sizeof(cf), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_debug_rowpass(datum_ocean_t ctx, int cascade, float *c, float *d)
{
  if (!ctx || !c || !d)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_debug_rowpass: null argument");

  if (cascade < 0 || cascade >= ctx->cascades)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_debug_rowpass: cascade out of range");

  // (as datum_ocean_displace: without a state the row pass would read h0 and phase the caller never wrote -- in FP16_H0 a spurious
  // "NaN or an infinity" from size_spectrum_scale)
  if (!ctx->cstate[cascade].uploaded)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_debug_rowpass: the cascade has no state (datum_ocean_upload_state)");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  int rc = ensure_scratch(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  size_t const P = plane(ctx);

  // The work spectrum belongs to a launch, not to a cascade (slot cascade - first of the group: ocean_kernels.hip), and the last displace may
  // have left another cascade's values in the slot: the row pass of this one cascade once more -- with the dt's the last displace applied and
  // did not store, if any, and no queued one, so the phase is not stored and the values are those of the last displace -- into slot 0
  rc = size_spectrum_scale(ctx);
  if (rc == DATUM_OCEAN_OK)
    rc = settle_phase_store(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  {
    PhaseWriteback::Launch const again = ctx->writeback.repeat();

    StepArgs a = make_args(ctx, again.ndt, again.dt, false);
    a.first = cascade;
    a.cascades = 1;

    HIPCHECK(ctx, launch(ctx, *plan_step(ctx).row, a, nullptr));
  }

  if (ctx->half)
    hipLaunchKernelGGL(ocean_unpack_kernel<true>, dim3(1024), dim3(256), 0, ctx->stream, static_cast<ch const*>(ctx->spec), ctx->N, ctx->casc[cascade].specinv, ctx->scratch, ctx->scratch + P);
  else
    hipLaunchKernelGGL(ocean_unpack_kernel<false>, dim3(1024), dim3(256), 0, ctx->stream, static_cast<cd const*>(ctx->spec), ctx->N, 1.0f, ctx->scratch, ctx->scratch + P);
  HIPCHECK(ctx, hipGetLastError());
  HIPCHECK(ctx, hipMemcpyAsync(c, ctx->scratch, P * sizeof(cf), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipMemcpyAsync(d, ctx->scratch + P, P * sizeof(cf), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_profile_begin(datum_ocean_t ctx, int max_steps, int stride)
{
  if (!ctx || max_steps < 1 || stride < 1)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_profile_begin: bad argument");

  if (ctx->literal)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_profile_begin: the handle is in the literal mode, whose dispatches are not sampled");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  // (the sampled row passes start at the beginning of a write-back interval, whatever came before)
  int rc = flush_retained(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  int const groups = plan_step(ctx).groups;

  while (ctx->events.size() < (size_t)4 * max_steps * groups)
  {
    hipEvent_t e;
    HIPCHECK(ctx, hipEventCreate(&e));
    ctx->events.push_back(e);
  }

  ctx->profiling = true;
  ctx->profmax = max_steps;
  ctx->profsteps = 0;
  ctx->profstride = stride;
  ctx->profgroups = groups;
  ctx->profcalls = 0;

  return DATUM_OCEAN_OK;
}

int datum_ocean_profile_end(datum_ocean_t ctx, double *rowpass_ms, double *colpass_ms, int *steps)
{
  if (!ctx || !ctx->profiling)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_profile_end: profiling was not started");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  double row = 0, col = 0;

  // a sampled step = one launch of either pass per cascade group: the sums over a step's launches
  for(int i = 0; i < ctx->profsteps * ctx->profgroups; ++i)
  {
    float ms;
    HIPCHECK(ctx, hipEventElapsedTime(&ms, ctx->events[4*i+0], ctx->events[4*i+1]));
    row += ms;
    HIPCHECK(ctx, hipEventElapsedTime(&ms, ctx->events[4*i+2], ctx->events[4*i+3]));
    col += ms;
  }

  int n = ctx->profsteps;

  if (rowpass_ms) *rowpass_ms = n ? row / n : 0.0;
  if (colpass_ms) *colpass_ms = n ? col / n : 0.0;
  if (steps) *steps = n;

  ctx->profiling = false;

  return DATUM_OCEAN_OK;
}

int datum_ocean_algorithmic_bytes(datum_ocean_t ctx, double *rowpass_bytes, double *colpass_bytes)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_algorithmic_bytes: null handle");

  double pts = (double)plane(ctx) * ctx->cascades;

  // the ALGORITHM's bytes as the reference states it, three transforms (bench.py's roofline):
  // h0 8 + phase in 4 + phase out 4 + spectrum out 24 | spectrum in 24 + two RGBA32F layers 32.
  // The packed step moves 16 instead of 24 spectrum bytes each way and 24-byte texels: 32 + 40 = 72 B/pt of HBM traffic.
  // fp16-stored spectrum: 4 + 4 + 4 + 12 | 12 + 32 = 68 B/pt; this build keeps h0 in fp32 and
  // moves 8 + 4 + 4 + 8 | 8 + 24 = 56 B/pt in the format FP16, and with h0 as halves too (FP16_H0) 4 + 4 + 4 + 8 | 8 + 24 = 52 B/pt.
  if (rowpass_bytes) *rowpass_bytes = (ctx->half ? 24.0 : 40.0) * pts;
  if (colpass_bytes) *colpass_bytes = (ctx->half ? 44.0 : 56.0) * pts;

  return DATUM_OCEAN_OK;
}

}

/* -- ripple walls: a byte plane beside the ripple layer (ocean_ripple_wall.hip) ------------------------------------------------------------ */

extern "C"
{

int datum_ocean_set_ripple_walls(datum_ocean_t ctx, datum_ocean_ripple_wall const *walls, int count)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_walls: null handle");

  if (count < 0 || count > DATUM_OCEAN_RIPPLE_MAX_WALLS)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_walls: count outside [0, DATUM_OCEAN_RIPPLE_MAX_WALLS]");

  if (count > 0 && !walls)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_walls: null walls");

  for(int k = 0; k < count; ++k)
  {
    datum_ocean_ripple_wall const &w = walls[k];

    for(float v : { w.center[0], w.center[1], w.axis[0], w.axis[1], w.half[0], w.half[1] })
      if (!std::isfinite(v))
        return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_walls: a field is not finite");

    if (!(w.half[0] > 0.0f && w.half[1] > 0.0f))
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_walls: half must be positive");

    if (w.kind != DATUM_OCEAN_RIPPLE_WALL_BOX && w.kind != DATUM_OCEAN_RIPPLE_WALL_ELLIPSE)
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_walls: kind must be DATUM_OCEAN_RIPPLE_WALL_BOX or DATUM_OCEAN_RIPPLE_WALL_ELLIPSE");
  }

  int rc = check_ripples(ctx, "datum_ocean_set_ripple_walls");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  rc = free_ripple_walls(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  ctx->rippleswell.current = false;

  // (the wall byte enters the bed's depth: with or without walls now, a bed is rastered again)
  if (count == 0)
    return raster_ripple_bed(ctx, ripple_grid(ctx), false);

  hipError_t e = ctx->ripplewall.allocate(ripple_cells(ctx), ctx->stream);
  if (e == hipSuccess)
    e = hipMalloc(&ctx->ripplewalllist, (size_t)count * sizeof(datum_ocean_ripple_wall));
  // (the caller's array may go away behind the call: the copy is waited for)
  // (the copy's `reserved` holds inv2 for body contact, ocean_contact.h; the raster does not read the field.  8 KiB at the most, on
  // the stack: nothing here can throw)
  datum_ocean_ripple_wall list[DATUM_OCEAN_RIPPLE_MAX_WALLS];

  for(int k = 0; k < count; ++k)
  {
    list[k] = walls[k];
    contact_wall_prepare(list[k]);
  }

  if (e == hipSuccess)
    e = hipMemcpyAsync(ctx->ripplewalllist, list, (size_t)count * sizeof(datum_ocean_ripple_wall), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize(ctx->stream);

  if (e != hipSuccess)
  {
    (void)free_ripple_walls(ctx);
    return fail(ctx, (int)e, "datum_ocean_set_ripple_walls: hipMalloc");
  }

  ctx->ripplewallcount = count;

  rc = raster_ripple_walls(ctx, ripple_grid(ctx), true);

  return rc != DATUM_OCEAN_OK ? rc : raster_ripple_bed(ctx, ripple_grid(ctx), false);
}

int datum_ocean_ripple_walls_device(datum_ocean_t ctx, unsigned char const **plane)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_ripple_walls_device: null handle");

  if (!plane)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_ripple_walls_device: null argument");

  *plane = ctx->ripplewall.get();

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_ripple_walls(datum_ocean_t ctx, unsigned char *host)
{
  int rc = check_ripples(ctx, "datum_ocean_read_ripple_walls");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!ctx->ripplewall.get())
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_read_ripple_walls: walls are off (datum_ocean_set_ripple_walls)");

  if (!host)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_ripple_walls: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  rc = read_ripple_window(ctx, ctx->ripplewall.get(), host);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

}

/* -- the ripple bed: depth and surf planes beside the ripple layer (ocean_ripple_bed.hip) ------------------------------------------------- */

extern "C"
{

int datum_ocean_set_ripple_bed(datum_ocean_t ctx, datum_ocean_ripple_bed const *bed, float const *depths_host)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_bed: null handle");

  if (bed)
  {
    if (bed->width < 2 || bed->width > DATUM_OCEAN_RIPPLE_BED_MAX_SIDE || bed->height < 2 || bed->height > DATUM_OCEAN_RIPPLE_BED_MAX_SIDE)
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_bed: width and height must lie in [2, DATUM_OCEAN_RIPPLE_BED_MAX_SIDE]");

    if (!depths_host)
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_bed: null depths_host");

    if (!(std::isfinite(bed->texel) && bed->texel > 0.0f))
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_bed: texel must be finite and positive");

    if (!(std::isfinite(bed->origin[0]) && std::isfinite(bed->origin[1]) && std::isfinite(bed->outside)))
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_bed: origin and outside must be finite");

    if (!(std::isfinite(bed->max_depth) && bed->max_depth > 0.0f))
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_bed: max_depth must be finite and positive");

    if (!(bed->dry_depth > 0.0f && bed->dry_depth <= bed->max_depth))
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_bed: dry_depth must lie in (0, max_depth]");

    if (!std::isfinite(bed->surf_depth) || bed->surf_depth < 0.0f || !std::isfinite(bed->surf_gamma) || bed->surf_gamma < 0.0f)
      return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_bed: surf_depth and surf_gamma must be finite and not negative");

    size_t const texels = (size_t)bed->width * bed->height;

    for(size_t k = 0; k < texels; ++k)
      if (!std::isfinite(depths_host[k]))
        return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_bed: a map value is not finite");
  }

  int rc = check_ripples(ctx, "datum_ocean_set_ripple_bed");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (bed && ctx->rippledispersion == DATUM_OCEAN_RIPPLE_DEEP)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_ripple_bed: the layer's mode is DATUM_OCEAN_RIPPLE_DEEP, and the bed and the DEEP mode do not combine");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  ctx->rippleswell.current = false;

  rc = free_ripple_bed(ctx);
  if (rc != DATUM_OCEAN_OK || !bed)
    return rc;

  size_t const cells = ripple_cells(ctx), texels = (size_t)bed->width * bed->height;

  hipError_t e = ctx->ripplebed.allocate(cells, ctx->stream);
  if (e == hipSuccess)
    e = ctx->ripplesurf.allocate(cells, ctx->stream);
  if (e == hipSuccess)
    e = hipMalloc(&ctx->ripplebedmap, texels * sizeof(float));
  // (the caller's array may go away behind the call: the copy is waited for)
  if (e == hipSuccess)
    e = hipMemcpyAsync(ctx->ripplebedmap, depths_host, texels * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize(ctx->stream);

  if (e != hipSuccess)
  {
    (void)free_ripple_bed(ctx);
    return fail(ctx, (int)e, "datum_ocean_set_ripple_bed: hipMalloc");
  }

  ctx->ripplebedparams = *bed;

  return raster_ripple_bed(ctx, ripple_grid(ctx), true);
}

int datum_ocean_ripple_bed_device(datum_ocean_t ctx, void **depth, void **surf, size_t *cells)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_ripple_bed_device: null handle");

  if (depth)
    *depth = ctx->ripplebed.get();
  if (surf)
    *surf = ctx->ripplesurf.get();
  if (cells)
    *cells = ctx->ripplebed.get() ? ripple_cells(ctx) : 0;

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_ripple_bed(datum_ocean_t ctx, float *depth, unsigned char *surf)
{
  int rc = check_ripples(ctx, "datum_ocean_read_ripple_bed");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!ctx->ripplebed.get())
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_read_ripple_bed: the bed is off (datum_ocean_set_ripple_bed)");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  if (depth)
    rc = read_ripple_window(ctx, ctx->ripplebed.get(), depth);
  if (rc == DATUM_OCEAN_OK && surf)
    rc = read_ripple_window(ctx, ctx->ripplesurf.get(), surf);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

}

/* -- ripple swell: a forcing plane beside the ripple layer (ocean_ripple_swell.hip) ------------------------------------------------------- */

namespace
{
  // what every call that needs the plane refuses, the layer first; `name` goes into the error text
  int check_ripple_swell(datum_ocean_ctx *ctx, char const *name)
  {
    int rc = check_ripples(ctx, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (!ctx->rippleswell.get())
      return fail(ctx, DATUM_OCEAN_ESTATE, name, ": ripple swell is off (datum_ocean_set_ripple_swell)");

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_set_ripple_swell(datum_ocean_t ctx, int on)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_swell: null handle");

  if (on != 0 && on != 1)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_swell: on must be 0 or 1");

  int rc = check_ripples(ctx, "datum_ocean_set_ripple_swell");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (on && ctx->rippledispersion == DATUM_OCEAN_RIPPLE_DEEP)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_set_ripple_swell: the layer's mode is DATUM_OCEAN_RIPPLE_DEEP, and swell and the DEEP mode do not combine");

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  HIPCHECK(ctx, ctx->rippleswell.off());

  if (!on)
    return DATUM_OCEAN_OK;

  hipError_t e = ctx->rippleswell.on(ripple_cells(ctx), ctx->stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize(ctx->stream);

  if (e != hipSuccess)
  {
    (void)ctx->rippleswell.off();
    return fail(ctx, (int)e, "datum_ocean_set_ripple_swell: hipMalloc");
  }

  return DATUM_OCEAN_OK;
}

int datum_ocean_refresh_ripple_swell(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations)
{
  Query const q = { cascades, count, set, iterations };

  // the layer and the plane first (a null handle EINVAL, either off ESTATE), then the blended sample's checks of the list, set and iterations
  int rc = check_ripple_swell(ctx, "datum_ocean_refresh_ripple_swell");
  if (rc == DATUM_OCEAN_OK)
    rc = check_query(ctx, q, "datum_ocean_refresh_ripple_swell");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  RippleSwellRefreshArgs a;
  a.swell = ctx->rippleswell.get();
  a.wall = ctx->ripplewall.get();
  a.depth = ctx->ripplebed.get();
  a.g = ripple_grid(ctx);
  a.s = (float)ctx->ripples;
  a.q = query_args(ctx, q);

  HIPCHECK(ctx, launch_ripple_swell_refresh(a, ctx->stream));

  ctx->rippleswell.current = true;

  return DATUM_OCEAN_OK;
}

int datum_ocean_ripple_swell_device(datum_ocean_t ctx, void **plane, size_t *bytes, int *current)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_ripple_swell_device: null handle");

  if (plane)
    *plane = ctx->rippleswell.get();
  if (bytes)
    *bytes = ctx->rippleswell.get() ? ripple_cells(ctx) * sizeof(float) : 0;
  if (current)
    *current = ctx->rippleswell.current ? 1 : 0;

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_ripple_swell(datum_ocean_t ctx, float *plane)
{
  int rc = check_ripple_swell(ctx, "datum_ocean_read_ripple_swell");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!plane)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_ripple_swell: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  // (memory order: the plane as it lies on the torus, one copy)
  HIPCHECK(ctx, hipMemcpyAsync(plane, ctx->rippleswell.get(), ripple_cells(ctx) * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

}

/* -- wake foam: a coverage plane beside the ripple layer (ocean_ripple_foam.hip) ---------------------------------------------------------- */

namespace
{
  // what every call that needs the plane refuses, the layer first; `name` goes into the error text
  int check_ripple_foam(datum_ocean_ctx *ctx, char const *name)
  {
    int rc = check_ripples(ctx, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (!ctx->ripplefoam.get())
      return fail(ctx, DATUM_OCEAN_ESTATE, name, ": the wake foam is off (datum_ocean_set_ripple_foam)");

    return DATUM_OCEAN_OK;
  }

  int check_ripple_foam_points(datum_ocean_ctx *ctx, void const *points, size_t n, void const *out, char const *name)
  {
    int rc = check_ripple_foam(ctx, name);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    if (n > 0 && (!points || !out))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": null points or out");

    if (((uintptr_t)points & 7) || ((uintptr_t)out & 3))
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": points must be 8-byte and out 4-byte aligned");

    if (n > (size_t)INT32_MAX / 16)
      return fail(ctx, DATUM_OCEAN_EINVAL, name, ": n above INT32_MAX / 16");

    return DATUM_OCEAN_OK;
  }

  // device arrays, n > 0
  int run_ripple_foam_samples(datum_ocean_ctx *ctx, void const *points, size_t n, void *out)
  {
    RippleFoamSampleArgs a;
    a.foam = ctx->ripplefoam.get();
    a.points = static_cast<float2 const*>(points);
    a.samples = static_cast<float*>(out);
    a.g = ripple_grid(ctx);
    a.count = (int)n;

    HIPCHECK(ctx, launch_ripple_foam_samples(a, ctx->stream));

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_set_ripple_foam(datum_ocean_t ctx, int on)
{
  int rc = check_ripples(ctx, "datum_ocean_set_ripple_foam");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  rc = free_ripple_foam(ctx);
  if (rc != DATUM_OCEAN_OK || !on)
    return rc;

  hipError_t const e = ctx->ripplefoam.allocate(ripple_cells(ctx), ctx->stream);

  if (e != hipSuccess)
  {
    (void)free_ripple_foam(ctx);
    return fail(ctx, (int)e, "datum_ocean_set_ripple_foam: hipMalloc");
  }

  rc = clear_ripple_foam(ctx);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_set_ripple_foam_params(datum_ocean_t ctx, float t1, float k1, float t2, float k2, float decay)
{
  if (!ctx)
    return fail(nullptr, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_foam_params: null handle");

  if (!(std::isfinite(t1) && std::isfinite(t2)))
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_foam_params: t1 and t2 must be finite");

  if (!std::isfinite(k1) || k1 < 0.0f || !std::isfinite(k2) || k2 < 0.0f)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_foam_params: k1 and k2 must be finite and not negative");

  if (!std::isfinite(decay) || decay < 0.0f)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_set_ripple_foam_params: decay must be finite and not negative");

  ctx->ripplefoamt1 = t1;
  ctx->ripplefoamk1 = k1;
  ctx->ripplefoamt2 = t2;
  ctx->ripplefoamk2 = k2;
  ctx->ripplefoamdecay = decay;

  return DATUM_OCEAN_OK;
}

int datum_ocean_step_ripple_foam(datum_ocean_t ctx, float dt)
{
  int rc = check_ripple_foam(ctx, "datum_ocean_step_ripple_foam");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  // (a negative dt would make the fade a growth)
  if (!std::isfinite(dt) || dt < 0.0f)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_step_ripple_foam: dt is not finite or is negative");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  RippleFoamArgs a;
  a.state = ctx->ripplestate[ctx->ripplecurrent].get();
  a.foam = ctx->ripplefoam.get();
  a.g = ripple_grid(ctx);
  a.p.hinv = 0.5f * a.g.invs;
  a.p.t1 = ctx->ripplefoamt1;
  a.p.k1 = ctx->ripplefoamk1;
  a.p.t2 = ctx->ripplefoamt2;
  a.p.k2 = ctx->ripplefoamk2;
  a.p.fade = (float)std::exp(-(double)ctx->ripplefoamdecay * (double)dt);

  HIPCHECK(ctx, launch_ripple_foam(a, ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_reset_ripple_foam(datum_ocean_t ctx)
{
  int rc = check_ripple_foam(ctx, "datum_ocean_reset_ripple_foam");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return clear_ripple_foam(ctx);
}

int datum_ocean_ripple_foam_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes, int *ox, int *oy)
{
  int rc = check_ripple_foam(ctx, "datum_ocean_ripple_foam_device");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!device_ptr)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_ripple_foam_device: null argument");

  *device_ptr = ctx->ripplefoam.get();

  if (bytes)
    *bytes = ripple_cells(ctx) * sizeof(float);
  if (ox)
    *ox = ctx->rippleox;
  if (oy)
    *oy = ctx->rippleoy;

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_ripple_foam(datum_ocean_t ctx, float *plane)
{
  int rc = check_ripple_foam(ctx, "datum_ocean_read_ripple_foam");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!plane)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_ripple_foam: null argument");

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  rc = read_ripple_window(ctx, ctx->ripplefoam.get(), plane);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

  return DATUM_OCEAN_OK;
}

int datum_ocean_sample_ripple_foam(datum_ocean_t ctx, void const *points_device, size_t n, void *out_device)
{
  int rc = check_ripple_foam_points(ctx, points_device, n, out_device, "datum_ocean_sample_ripple_foam");
  if (rc != DATUM_OCEAN_OK || n == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  return run_ripple_foam_samples(ctx, points_device, n, out_device);
}

int datum_ocean_query_ripple_foam(datum_ocean_t ctx, float const *points, size_t n, float *out)
{
  int rc = check_ripple_foam_points(ctx, points, n, out, "datum_ocean_query_ripple_foam");
  if (rc != DATUM_OCEAN_OK || n == 0)
    return rc;

  HIPCHECK(ctx, hipSetDevice(ctx->device));

  // datum_ocean_query_ripples' staging: the surface queries' two buffers, grown on demand
  return read_staged(ctx, ctx->staging[STAGE_POINTS], points, n * sizeof(float2), ctx->staging[STAGE_SAMPLES], out, n * sizeof(float),
                     [&](void const *in, void *dev) { return run_ripple_foam_samples(ctx, in, n, dev); });
}

}   // extern "C"

/* -- bounds of the ripple layer, the rippled slab and the bounded rippled cast (ocean_ripple_bounds.hip) --------------------------------- */

namespace
{
  // the block of datum_ocean_reduce_ripple_bounds in float4s: guard, partials, guard, record, guard (2 float4 = 32 bytes each but the partials).
  // No GuardedPlane: that is one region between 256-byte guards, this is two regions in one allocation with a guard between them too
  constexpr size_t RIPPLE_BOUNDS_GUARD = 2;

  float4 *ripple_bounds_partials(datum_ocean_ctx const *ctx) { return ctx->rippleboundsblock + RIPPLE_BOUNDS_GUARD; }

  float4 *ripple_bounds_record(datum_ocean_ctx const *ctx)
  {
    return ripple_bounds_partials(ctx) + 2 * (size_t)ripple_bounds_groups(ctx->rippleR) + RIPPLE_BOUNDS_GUARD;
  }

  // the block, allocated by the first reduce after a set_ripples, and the two launches
  int reduce_ripple_bounds(datum_ocean_ctx *ctx)
  {
    HIPCHECK(ctx, hipSetDevice(ctx->device));

    int const groups = ripple_bounds_groups(ctx->rippleR);

    if (!ctx->rippleboundsblock)
    {
      size_t const bytes = (3 * RIPPLE_BOUNDS_GUARD + 2 * (size_t)groups + 2) * sizeof(float4);

      float4 *block = nullptr;

      HIPCHECK(ctx, hipMalloc(&block, bytes));

      hipError_t const e = hipMemsetAsync(block, 0xCD, bytes, ctx->stream);

      if (e != hipSuccess)
      {
        (void)hipFree(block);
        return fail(ctx, (int)e, "datum_ocean_reduce_ripple_bounds: hipMemsetAsync");
      }

      ctx->rippleboundsblock = block;
    }

    RippleBoundsArgs a;
    a.state = reinterpret_cast<float4 const*>(ctx->ripplestate[ctx->ripplecurrent].get());
    a.partials = ripple_bounds_partials(ctx);
    a.record = ripple_bounds_record(ctx);
    a.pairs = (int)(ripple_cells(ctx) / 2);
    a.groups = groups;

    HIPCHECK(ctx, launch_ripple_bounds(a, ctx->stream));

    ctx->rippleboundscurrent = true;

    return DATUM_OCEAN_OK;
  }

  // reduce, then a blocking read of the record
  int read_ripple_bounds(datum_ocean_ctx *ctx, float *record)
  {
    int rc = reduce_ripple_bounds(ctx);
    if (rc != DATUM_OCEAN_OK)
      return rc;

    HIPCHECK(ctx, hipMemcpyAsync(record, ripple_bounds_record(ctx), RIPPLE_BOUNDS_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));

    return DATUM_OCEAN_OK;
  }
}

extern "C"
{

int datum_ocean_reduce_ripple_bounds(datum_ocean_t ctx)
{
  int rc = check_ripples(ctx, "datum_ocean_reduce_ripple_bounds");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  return reduce_ripple_bounds(ctx);
}

int datum_ocean_ripple_bounds_device(datum_ocean_t ctx, void **device_ptr, size_t *bytes)
{
  int rc = check_ripples(ctx, "datum_ocean_ripple_bounds_device");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!device_ptr)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_ripple_bounds_device: null argument");

  if (!ctx->rippleboundsblock)
    return fail(ctx, DATUM_OCEAN_ESTATE, "datum_ocean_ripple_bounds_device: no record yet (datum_ocean_reduce_ripple_bounds)");

  *device_ptr = ripple_bounds_record(ctx);

  if (bytes)
    *bytes = RIPPLE_BOUNDS_BYTES;

  return DATUM_OCEAN_OK;
}

int datum_ocean_read_ripple_bounds(datum_ocean_t ctx, float *record)
{
  int rc = check_ripples(ctx, "datum_ocean_read_ripple_bounds");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!record)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_read_ripple_bounds: null argument");

  return read_ripple_bounds(ctx, record);
}

int datum_ocean_surface_slab_rippled(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, float *zlo, float *zhi, float *reachx, float *reachy)
{
  Query const q = { cascades, count, set, 0 };
  int rc = check_ripples(ctx, "datum_ocean_surface_slab_rippled");
  if (rc == DATUM_OCEAN_OK)
    rc = check_blend_list(ctx, q, "datum_ocean_surface_slab_rippled");
  if (rc != DATUM_OCEAN_OK)
    return rc;

  if (!set)
    return fail(ctx, DATUM_OCEAN_EINVAL, "datum_ocean_surface_slab_rippled: null set");

  float records[DATUM_OCEAN_MAX_CASCADES * BOUNDS_FIELDS];
  float layer[RIPPLE_BOUNDS_FIELDS];

  rc = datum_ocean_read_bounds(ctx, records);
  if (rc == DATUM_OCEAN_OK)
    rc = read_ripple_bounds(ctx, layer);
  if (rc != DATUM_OCEAN_OK)
    return rc;

  GenFrame const f = make_gen_frame(*set, ctx->N, 2, 2);      // the camera's terms are not read

  BoundsSlab const s = ripple_bounds_slab(records, cascades, count, f.basez, set->swellamplitude, f.gx, f.gy, layer);

  if (zlo) *zlo = s.zlo;
  if (zhi) *zhi = s.zhi;
  if (reachx) *reachx = s.reachx;
  if (reachy) *reachy = s.reachy;

  return DATUM_OCEAN_OK;
}

int datum_ocean_cast_rays_rippled_bounded(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                          void const *rays_device, size_t n, void *records_device)
{
  Query const q = { cascades, count, set, iterations };
  RayCall const call = { steps, refine, rays_device, n, records_device };

  return cast_rays(ctx, q, call, ReadVariant{ true, true }, "datum_ocean_cast_rays_rippled_bounded");
}

int datum_ocean_read_rays_rippled_bounded(datum_ocean_t ctx, int const *cascades, int count, datum_ocean_set const *set, int iterations, int steps, int refine,
                                          float const *rays, size_t n, float *records)
{
  Query const q = { cascades, count, set, iterations };
  RayCall const call = { steps, refine, rays, n, records };

  return read_rays(ctx, q, call, ReadVariant{ true, true }, "datum_ocean_read_rays_rippled_bounded");
}

}   // extern "C"
