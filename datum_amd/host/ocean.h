//
// ocean.h -- host-side mirror of datum's ocean API (src/renderer/ocean.h:12-99) over the HIP module
//
// Same type names, field names, defaults and free-function signatures as the reference, so code written
// against datum's ocean API (examples/ocean/ocean.cpp:31,46-52,59,135,165,179) compiles against this header
// with three documented differences:
//   1. WaveResolution is a run-time value (OceanContext::resolution / OceanParams::resolution, default 64 =
//      ocean.h:16); the [64][64] state arrays of OceanParams (ocean.h:69-71) are sized by it.  The reference's POD itself
//      (memcpy / serialise by value) is OceanParamsPod below, with to_pod / from_pod.
//   2. The Vulkan objects of OceanContext are replaced by one opaque HIP-module handle
//      (include/datum_ocean_hip.h); VkSemaphore dependencies become hipEvent_t handles (void*).
//   3. update_ocean's phase loop (ocean.cpp:223-233) runs on the device: update_ocean() queues dt,
//      render_ocean_surface() applies the queue in order, bit-identically.  At the reference's own resolution
//      (N <= 64) update_ocean ALSO runs the loop on the host, as the reference does (OceanParams::hostphase, on by
//      default there: OceanParams::phase is current after every call); above it OceanParams::phase on the host
//      is the state as of the last fetch_ocean_state().
// Device failures throw std::runtime_error as the reference does (ocean.cpp:271, vulkan.cpp:550);
// misuse trips assert (ocean.cpp:351,722-723); prepare_ocean_context returns bool (ocean.cpp:493-501).
//

#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "lml.h"
#include "../../include/datum_ocean_hip.h"

//|---------------------- stand-ins for the surrounding engine ---------------
// only what the ocean call sites name

namespace DatumPlatform
{
  // src/platform.h: render_device() -> VkDevice + queues.  Here: which HIP device the ocean runs on.
  struct PlatformInterface
  {
    int hipdevice = 0;
  };
}

class AssetManager   // src/asset.h: the HIP module embeds its kernels, no asset pack is consulted
{
};

class Camera   // src/renderer/camera.h:16-107, the subset the ocean path reads
{
  public:
    Camera();

    lml::Vec3 position() const { return m_position; }
    lml::Quaternion3 rotation() const { return m_rotation; }

    float fov() const { return m_fov; }
    float aspect() const { return m_aspect; }
    float znear() const { return m_znear; }
    float zfar() const { return m_zfar; }

    lml::Matrix4f proj() const;                                                                       // camera.cpp:77-91
    lml::Transform transform() const { return lml::Transform::lookat(m_position, m_rotation); }       // camera.h:48

    void set_projection(float fov, float aspect, float znear = 0.1f, float zfar = 24000.0f);          // camera.h:52
    void set_position(lml::Vec3 const &position) { m_position = position; }
    void set_rotation(lml::Quaternion3 const &rotation) { m_rotation = rotation; }
    void lookat(lml::Vec3 const &position, lml::Vec3 const &target, lml::Vec3 const &up);             // camera.cpp:151-155

  private:

    float m_fov, m_aspect, m_znear, m_zfar;
    lml::Vec3 m_position;
    lml::Quaternion3 m_rotation;
};

class Mesh   // src/renderer/mesh.h:16-80, the parts Ocean uses
{
  public:

    struct Vertex
    {
      lml::Vec3 position;
      lml::Vec2 texcoord;
      lml::Vec3 normal;
      lml::Vec4 tangent;
    };

    enum class State { Empty, Loading, Waiting, Testing, Ready };

    bool ready() const { return state == State::Ready; }

    // vertex buffer in DEVICE memory (compute-writable, ocean.cpp:270) + static index buffer
    struct VertexBuffer
    {
      uint32_t vertexcount = 0;
      uint32_t vertexsize = 0;
      uint32_t indexcount = 0;
      uint32_t indexsize = 0;
      void *vertices = nullptr;
      void *indices = nullptr;
    } vertexbuffer;

    State state = State::Empty;
};

static_assert(sizeof(Mesh::Vertex) == 48, "Mesh::Vertex must be 48 bytes (mesh.h:20-26)");

class Ocean;
struct OceanContext;

class ResourceManager   // src/renderer/resource.h: create / release / destroy for the Ocean mesh only
{
  public:
    explicit ResourceManager(OceanContext &context) : m_context(&context) { }

    template<typename Resource, typename ...Args>
    Resource const *create(Args... args);

    template<typename Resource>
    void release(Resource const *resource);

    template<typename Resource>
    void destroy(Resource const *resource);

  private:
    OceanContext *m_context;
};

//|---------------------- Ocean ---------------------------------------------
//|--------------------------------------------------------------------------

struct OceanContext
{
  bool ready = false;

  static const int WaveResolution = 64;   // ocean.h:16: the default; `resolution` is what is used

  int resolution = WaveResolution;

  int device = 0;

  bool spectrumfp16 = false;              // extension: store the module's work spectrum as halves (set before prepare_ocean_context)
  bool heightfp16 = false;                // with spectrumfp16: the module reads OceanParams::height as halves too, from a device copy of its own
                                          // (DATUM_OCEAN_SPECTRUM_FP16_H0; what the caller holds and fetches stays fp32)
  bool literaltransform = false;          // validation: displace through the reference's own radix-2 transforms and literal twiddle table
                                          // (datum_ocean_set_literal_transform; set before prepare_ocean_context) -- for texel-for-texel A/B with the Vulkan build;
                                          // not together with spectrumfp16 (the mode is the reference's fp32 arithmetic: prepare_ocean_context throws)

  datum_ocean_t hip = nullptr;            // replaces vulkan / pipelines / oceanset / spectrum / displacementmap

  void *rendercomplete = nullptr;         // hipEvent_t recorded behind the last render (ocean.h:45)

  std::uint64_t boundstate = 0;           // which OceanParams state is resident on the device (0: none; state ids start at 1)
  std::uint64_t boundheight = 0;
  std::uint64_t boundseed = 0;            // which OceanParams seed is resident on the device (deviceheight only)
  std::uint64_t appliedupdates = 0;       // how many of that state's update_ocean calls the device has applied (OceanParams::updates)
  std::uint64_t appliedlineage = 0;       // OceanParams::lineage_at(appliedupdates) of the history those updates came from

  // States this context has rendered before and had to make room for: h0 and the phase as advanced so far, parked in
  // device memory (datum_ocean_park_state), so that alternating between several OceanParams on one context costs two
  // device-to-device copies per switch and replays only the updates issued since -- the reference keeps every params'
  // phase on the host and any context renders any params at any time (ocean.cpp:217-236,748-749).
  struct Parked
  {
    std::uint64_t stateid = 0, heightid = 0, appliedupdates = 0, appliedlineage = 0, lastuse = 0;
    void *device = nullptr;
    int flags = 0;
  };

  // Capacity and footprint: up to MaxParkedStates parked copies + one spare buffer of datum_ocean_state_bytes(resolution) =
  // 12 N^2 bytes each (64^2: 48 KB; 1024^2: 12.6 MB; 4096^2: 201 MB, i.e. up to 1 GB of HBM per context), allocated on first
  // use and held until release_parked_states() or the context's destruction -- a slot whose OceanParams was re-seeded or
  // destroyed is not noticed by the context.  The bound state and the slot being resumed trade places through the spare, so
  // MaxParkedStates + 1 states alternate without an eviction; with MORE, the least recently used slot is given up and its state
  // falls back to the host copy + recorded history (OceanParams::hostphase, or a fetch_ocean_state at least every
  // MaxRecordedUpdates / 2 steps, keeps that possible).
  static const std::size_t MaxParkedStates = 4;

  std::vector<Parked> parked;
  std::uint64_t useclock = 0;

  void *spare = nullptr;                  // one more buffer of the same size: the bound state and the slot being resumed trade places through it
  int spareflags = 0;

  OceanContext() = default;
  OceanContext(OceanContext const &) = delete;
  OceanContext &operator=(OceanContext const &) = delete;
  ~OceanContext();
};

struct OceanParams
{
  lml::Plane plane = { { 0.0f, 0.0f, 1.0f }, 0.0f };

  // Swell
  float swelllength = 40.0f;
  float swellamplitude = 0.8f;
  float swellsteepness = 0.0f;
  float swellspeed = 1.25f;
  lml::Vec2 swelldirection = { 0.780869f, 0.624695f };

  // Waves
  float wavescale = 64.0f;
  float waveamplitude = 0.00002f;
  float windspeed = 30.0f;
  lml::Vec2 winddirection = { 0.780869f, 0.624695f };
  float choppiness = 1.35f;
  float smoothing = 280.0f;

  // State
  float swellphase = 0.0f;
  int resolution;                 // N (the reference: OceanContext::WaveResolution)
  std::vector<float> seed;        // [N][N][2]
  std::vector<float> height;      // [N][N][2]   h0
  std::vector<float> phase;       // [N][N]      as of seed_ocean / the last fetch_ocean_state
  lml::Vec2 flow = { 0.0f, 0.0f };

  // extension: let lerp_ocean_waves leave the h0 rebuild (ocean.cpp:194-211) to the device: the seed is uploaded once
  // and render_ocean_surface runs the rebuild kernel when the wave parameters have changed.  `height` on the host is
  // then stale until fetch_ocean_state().  Off by default (the reference recomputes on the host).
  bool deviceheight = false;

  // Also advance `phase` on the host in every update_ocean call, as the reference does (ocean.cpp:223-233; N * N fmod per call).
  // ON by default at the reference's own resolution (N <= WaveResolution = 64: 33 us per call) -- there an OceanParams behaves
  // exactly like the reference's: `phase` is current after every update_ocean, any context renders any params at any time,
  // to_pod() always succeeds -- and OFF above it (the constructor decides), where the N * N host loop is what had to leave the
  // CPU: the phase lives on the device (and in the contexts' parked copies), the host copy is the state as of seed_ocean /
  // the last fetch_ocean_state and is only needed by a context that holds no copy.  Either way the device advances its own
  // copy (the row-pass kernel, bit for bit the same values).
  bool hostphase = false;

  // device residency bookkeeping (not in the reference)
  //
  // update_ocean's phase loop runs on the device, so update_ocean() only RECORDS the step: entry number
  // `firstupdate + i` of this state's history is updates[i] = (dt, the wavescale in force at that call).  The history
  // belongs to the state (stateid), not to one OceanParams object: OceanParams stays freely copyable like the reference's
  // POD -- a per-frame copy handed to the render thread carries the same stateid and a prefix-consistent history -- and
  // rendering is const: render_ocean_surface applies the entries the CONTEXT has not applied yet
  // (OceanContext::appliedupdates) and never touches the params.  The history keeps the last MaxRecordedUpdates entries.  A
  // context that alternates between several params parks the one it is not rendering (OceanContext::Parked) and continues
  // from there; without hostphase (N > 64, or switched off) a context that holds NO copy of a state whose host phase is older
  // than the recorded history throws (render or fetch a state every MaxRecordedUpdates / 2 steps, or set hostphase).
  // (lineage: a running hash over the history up to and including this entry.  A copy of an OceanParams that is then
  // advanced on its own -- update_ocean(P, a), update_ocean(Q, b) -- shares P's stateid and history NUMBERS but not their
  // contents; a context tells the two apart by the lineage of the last entry it applied.)
  struct Update { float dt, wavescale; std::uint64_t lineage; };

  static const std::size_t MaxRecordedUpdates = 4096;

  std::uint64_t stateid;                // a fresh id per constructed / seeded state (never 0)
  std::uint64_t heightid = 0;           // changes when `height` is recomputed (lerp_ocean_waves)
  std::uint64_t firstupdate = 0;        // history number of updates[0]
  std::vector<Update> updates;          // update_ocean calls since firstupdate
  std::uint64_t phaseupdates = 0;       // how many entries of the history `phase` (on the host) already contains
  std::uint64_t baselineage = 0;        // lineage of history entry firstupdate - 1 (0 at the start of a history)

  // lineage of the history's first `count` entries (count in [firstupdate, firstupdate + updates.size()])
  std::uint64_t lineage_at(std::uint64_t count) const { return count == firstupdate ? baselineage : updates[count - firstupdate - 1].lineage; }
  int rejectedseeds = 0;                // seed pairs whose 8 polar draws were all rejected (see seed_ocean)

  explicit OceanParams(int resolution = OceanContext::WaveResolution);
};

// The reference's OceanParams byte for byte (src/renderer/ocean.h:48-73 with WaveResolution = 64, ocean.h:16): for callers that
// memcpy, serialise or load an OceanParams by value -- OceanParams above carries run-time sized arrays and device bookkeeping and
// is not that POD.  to_pod() needs the host phase to be current (fetch_ocean_state, or hostphase):
// it returns false, and leaves `pod` alone, when update_ocean calls are recorded that `params.phase` does not contain yet.
struct OceanParamsPod
{
  lml::Plane plane;

  float swelllength, swellamplitude, swellsteepness, swellspeed;
  lml::Vec2 swelldirection;

  float wavescale, waveamplitude, windspeed;
  lml::Vec2 winddirection;
  float choppiness, smoothing;

  float swellphase;
  float seed[OceanContext::WaveResolution][OceanContext::WaveResolution][2];
  float height[OceanContext::WaveResolution][OceanContext::WaveResolution][2];
  float phase[OceanContext::WaveResolution][OceanContext::WaveResolution];
  lml::Vec2 flow;
};

static_assert(sizeof(OceanParamsPod) == 82000, "OceanParamsPod must be the reference's OceanParams (ocean.h:48-73): 80 bytes of tunables + swellphase, 3 arrays, flow");

bool to_pod(OceanParams const &params, OceanParamsPod &pod);         // resolution must be 64
OceanParams from_pod(OceanParamsPod const &pod);                      // a fresh state (new state id, empty history) holding the pod's arrays

class Ocean : public Mesh
{
  public:
    friend class ResourceManager;

    int sizex;
    int sizey;

  protected:
    Ocean() = default;

    OceanContext *context = nullptr;
};

template<> Ocean const *ResourceManager::create<Ocean>(int sizex, int sizey);
template<> void ResourceManager::release<Ocean>(Ocean const *ocean);
template<> void ResourceManager::destroy<Ocean>(Ocean const *ocean);

void seed_ocean(OceanParams &params);
void seed_ocean(OceanParams &params, std::uint32_t rngseed);   // extension: reproducible entropy (the reference uses random_device, ocean.cpp:132)
void lerp_ocean_swell(OceanParams &params, float swelllength, float swellamplitude, float swellspeed, lml::Vec2 swelldirection, float t);
void lerp_ocean_waves(OceanParams &params, float wavescale, float waveamplitude, float windspeed, lml::Vec2 winddirection, float t);
void update_ocean(OceanParams &params, float dt);

// Initialise
void initialise_ocean_context(DatumPlatform::PlatformInterface &platform, OceanContext &context, uint32_t queueindex);

// Prepare
bool prepare_ocean_context(DatumPlatform::PlatformInterface &platform, OceanContext &context, AssetManager &assets);

// Render
void render_ocean_surface(OceanContext &context, Ocean const *target, Camera const &camera, OceanParams const &params, void *const (&dependancies)[8] = {});

// Extensions (not in the reference)

// displacement maps only (ocean.sim .. ocean.map), no mesh: what the bench times
void displace_ocean_surface(OceanContext &context, OceanParams const &params);

// free the context's parked device copies (all of them, or all but `keep`'s): returns the bytes of HBM given back.  The states
// themselves are not lost while their OceanParams can still be uploaded (host phase + recorded history)
std::size_t release_parked_states(OceanContext &context, OceanParams const *keep = nullptr);

// copy the device-resident phase (and, with deviceheight, h0) back into params (applies any queued update first)
void fetch_ocean_state(OceanContext &context, OceanParams &params);

// foam (include/datum_ocean_hip.h, ABI 9): DATUM_OCEAN_FOAM_OFF / _JACOBIAN / _ACCUMULATE on the context's handle (after
// prepare_ocean_context).  The plane is computed by every displace; a context that binds another state (upload or resume of a parked
// one) starts that state's accumulation from zero, as the C ABI does.  The same state with new wave parameters (lerp_ocean_waves, with
// or without OceanParams::deviceheight) keeps it
void set_ocean_foam(OceanContext &context, int mode);
void set_ocean_foam_params(OceanContext &context, float threshold, float gain, float decay);
void read_ocean_foam(OceanContext &context, float *foam /* [N][N] */);
void ocean_foam_device(OceanContext &context, void **device_ptr, std::size_t *bytes);

// surface queries (include/datum_ocean_hip.h: datum_ocean_read_surface, the definition there): the water surface above world points, for
// buoyancy and the like.  The maps are the ones the context last displaced (as read_ocean_displacement's); swell, plane and scale come from
// `params` (through make_oceanset -- the camera's fields are not read).  Blocking; after render_ocean_surface or displace_ocean_surface.
// Throws before prepare_ocean_context
struct OceanSurfaceSample
{
  lml::Vec3 position;                     // the surface point found; .z is the water height above the query point
  float residual;                         // |position.xy - query|: large where the surface folds over (no height field there)
  lml::Vec3 normal;                       // unit normal (the mesh's, without distance smoothing)
  float foam;                             // the foam plane there, 0 while foam is off
};

static_assert(sizeof(OceanSurfaceSample) == 32, "OceanSurfaceSample must be the C ABI's record of DATUM_OCEAN_SURFACE_SAMPLE_FLOATS floats");

void query_ocean_surface(OceanContext &context, OceanParams const &params, lml::Vec2 const *positions, std::size_t count, OceanSurfaceSample *samples, int iterations = 4);

// surface velocity (include/datum_ocean_hip.h: datum_ocean_set_velocity, the definition there): d/dt of the displacement at every texel,
// computed by every displace while on (DATUM_OCEAN_VELOCITY_OFF / _ON), and the same surface point as query_ocean_surface with the
// velocity there instead of normal and foam.  One cascade, as query_ocean_surface; the swell's own motion is not included.  Blocking.
// read_ocean_velocity and query_ocean_velocity throw while velocity is off and until a displace has written the plane
struct OceanVelocitySample
{
  lml::Vec3 position;                     // the surface point found: query_ocean_surface's, bit for bit
  float residual;                         // ... and its residual
  lml::Vec3 velocity;                     // (vx, vy, vz) in metres per second
  float pad;                              // 0
};

static_assert(sizeof(OceanVelocitySample) == 32, "OceanVelocitySample must be the C ABI's record of DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS floats");

void set_ocean_velocity(OceanContext &context, int mode);
void read_ocean_velocity(OceanContext &context, float *velocity /* [N][N][4] */);
void query_ocean_velocity(OceanContext &context, OceanParams const &params, lml::Vec2 const *positions, std::size_t count, OceanVelocitySample *samples, int iterations = 4);

// body buoyancy (include/datum_ocean_hip.h: datum_ocean_read_bodies, the definition there): per body the net buoyant force, its torque
// and a few aggregates over the body's hull probes, reduced on the device.  One cascade, as query_ocean_surface; the maps the context last
// displaced, swell and plane from `params`.  Host arrays, blocking.  Throws before prepare_ocean_context
struct OceanBodyProbe
{
  lml::Vec3 position;                     // body-local, metres
  float weight;                           // the cross-section the probe stands for, m^2 (the result is linear in it: fold rho g in, or multiply after)
};

struct OceanBodyRecord
{
  float force;                            // Fz = sum weight * submersion
  float torquex, torquey;                 // about the body origin
  float wet;                              // sum of the weights of the submerged probes
  lml::Vec3 normal;                       // sum of (weight * submersion) * the surface normal above the probe
  float residual;                         // the largest residual of the probes' surface records
};

static_assert(sizeof(OceanBodyProbe) == 16, "OceanBodyProbe must be the C ABI's probe");
static_assert(sizeof(OceanBodyRecord) == 32, "OceanBodyRecord must be the C ABI's record of DATUM_OCEAN_BODY_RECORD_FLOATS floats");

void reduce_ocean_bodies(OceanContext &context, OceanParams const &params, datum_ocean_body const *bodies, std::size_t nbodies, OceanBodyProbe const *probes, std::size_t nprobes, OceanBodyRecord *records, int iterations = 4);

// body drag (include/datum_ocean_hip.h: datum_ocean_read_body_drag, the definition there): per body the force and the torque of the water's
// motion relative to the hull, from the same bodies and probes as reduce_ocean_bodies and one datum_ocean_body_motion per body.  The same
// one-cascade list and set.  Needs set_ocean_velocity(ON) and a displace since: throws otherwise, as query_ocean_velocity does
struct OceanDragRecord
{
  lml::Vec3 force;                        // sum of k (water - hull), k = weight * submersion * (cl + cq |water - hull|)
  lml::Vec3 torque;                       // about the body origin
  float submerged;                        // sum weight * submersion: reduce_ocean_bodies' force, bit for bit
  float residual;                         // the largest residual of the probes' velocity records
};

static_assert(sizeof(OceanDragRecord) == 32, "OceanDragRecord must be the C ABI's record of DATUM_OCEAN_DRAG_RECORD_FLOATS floats");

void reduce_ocean_body_drag(OceanContext &context, OceanParams const &params, datum_ocean_body const *bodies, datum_ocean_body_motion const *motions, std::size_t nbodies, OceanBodyProbe const *probes, std::size_t nprobes, OceanDragRecord *records, int iterations = 4);

// body stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies_host, the definition there): advances every body's pose and motion IN
// PLACE by dt, in `substeps` sub-steps against the surface as it lies -- buoyancy, drag and a semi-implicit Euler integrator on the device --
// with one datum_ocean_body_props per body.  The same one-cascade list, set and state as reduce_ocean_body_drag; throws where it does
struct OceanStepRecord
{
  lml::Vec3 force;                        // of the last sub-step: buoyancy * submerged (vertical) and the drag
  lml::Vec3 torque;                       // about the body origin
  float submerged;                        // sum weight * submersion of the last sub-step
  float residual;                         // the largest residual of the probes' records over all sub-steps
};

static_assert(sizeof(OceanStepRecord) == 32, "OceanStepRecord must be the C ABI's record of DATUM_OCEAN_STEP_RECORD_FLOATS floats");

void step_ocean_bodies(OceanContext &context, OceanParams const &params, datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, std::size_t nbodies, OceanBodyProbe const *probes, std::size_t nprobes, float dt, int substeps, OceanStepRecord *records, int iterations = 4);

// the ripple layer (include/datum_ocean_hip.h: "ripple layer", the definition there): a local R x R wave grid of `cellsize`-metre cells that
// carries what bodies and impacts do to the water; off until set_ocean_ripples, R = 0 frees it.  Host arrays, blocking, as every call
// here; the same one-cascade list, set and state as reduce_ocean_body_drag for the wake, which throws where that call does.  Every call
// but set_ocean_ripples throws while the layer is off
struct OceanRippleImpulse
{
  lml::Vec2 position;                     // world x, y, metres
  float volume;                           // m^3 of water added (negative: taken away)
  float pad;                              // 0
};

struct OceanRippleSample
{
  float height;                           // eta, metres
  float dx, dy;                           // its slopes
  float rate;                             // d eta / dt, m/s
};

struct OceanWakeRecord
{
  float heave;                            // sum of the heave volumes deposited, m^3
  lml::Vec2 surge;                        // sum of displaced volume times the hull's shift through the water
  float dropped;                          // non-zero quanta that fell outside the window
  float pad[2];                           // 0
  float submerged;                        // sum weight * submersion: reduce_ocean_bodies' force, bit for bit
  float residual;                         // the largest residual of the probes' velocity records
};

static_assert(sizeof(OceanRippleImpulse) == 16 && sizeof(OceanRippleSample) == 16, "the C ABI's 16-byte impulse and sample");
static_assert(sizeof(OceanWakeRecord) == 32, "OceanWakeRecord must be the C ABI's record of DATUM_OCEAN_RIPPLE_RECORD_FLOATS floats");

void set_ocean_ripples(OceanContext &context, int R, float cellsize);
void center_ocean_ripples(OceanContext &context, lml::Vec2 const &centre);
void deposit_ocean_ripples(OceanContext &context, OceanRippleImpulse const *impulses, std::size_t count);
void deposit_ocean_body_ripples(OceanContext &context, OceanParams const &params, datum_ocean_body const *bodies, datum_ocean_body_motion const *motions, std::size_t nbodies, OceanBodyProbe const *probes, std::size_t nprobes, float dt, OceanWakeRecord *records, int iterations = 4);
void step_ocean_ripples(OceanContext &context, float dt, int substeps = 1);
void query_ocean_ripples(OceanContext &context, lml::Vec2 const *positions, std::size_t count, OceanRippleSample *samples);

// coupled stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies_coupled_host, the definition there): step_ocean_bodies' arguments;
// bodies and the ripple layer advance together by dt in `substeps` coupled sub-steps -- each sub-step the bodies feel the layer's height
// and rate and deposit their wake, then the layer steps.  Throws where step_ocean_bodies does, and while the layer is off
struct OceanCoupledRecord
{
  lml::Vec3 force;                        // of the last sub-step
  lml::Vec3 torque;                       // about the body origin
  float submerged;                        // sum weight * submersion of the last sub-step
  float residual;                         // the largest residual of the probes' records over all sub-steps
  float heave;                            // the wake of the last sub-step: sum of the heave volumes deposited, m^3
  lml::Vec2 surge;                        // ... and of displaced volume times the hull's shift through the water
  float dropped;                          // non-zero quanta that fell outside the window, all sub-steps
};

static_assert(sizeof(OceanCoupledRecord) == 48, "OceanCoupledRecord must be the C ABI's record of DATUM_OCEAN_COUPLED_RECORD_FLOATS floats");

void step_ocean_bodies_coupled(OceanContext &context, OceanParams const &params, datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, std::size_t nbodies, OceanBodyProbe const *probes, std::size_t nprobes, float dt, int substeps, OceanCoupledRecord *records, int iterations = 4);

// body contact (include/datum_ocean_hip.h: datum_ocean_step_bodies_contact_host, the definition there): step_ocean_bodies_coupled's
// arguments and the contact parameters; hulls stop at the ripple walls and ground on the ripple bed by a penalty force per probe.  Throws
// where step_ocean_bodies_coupled does, for parameters that are negative or not finite, and for a flag whose bed or walls are not set
struct OceanContactRecord
{
  OceanCoupledRecord coupled;             // force and torque are the totals, the contact's share included
  lml::Vec3 contact;                      // the contact force of the last sub-step
  float deepest;                          // the deepest penetration over all sub-steps, metres
};

static_assert(sizeof(OceanContactRecord) == 64, "OceanContactRecord must be the C ABI's record of DATUM_OCEAN_CONTACT_RECORD_FLOATS floats");

void step_ocean_bodies_contact(OceanContext &context, OceanParams const &params, datum_ocean_body *bodies, datum_ocean_body_motion *motions, datum_ocean_body_props const *props, std::size_t nbodies, OceanBodyProbe const *probes, std::size_t nprobes, float dt, int substeps, OceanContactRecord *records, datum_ocean_body_contact const &contact, int iterations = 4);

// ray casts (include/datum_ocean_hip.h: datum_ocean_read_rays, the definition there): per ray a fixed march of `steps` samples to the first
// change of side, `refine` bisections of that bracket, and the surface sample at the bracket's far end.  One cascade, as
// query_ocean_surface; the maps the context last displaced, swell and plane from `params`.  Host arrays, blocking.  Throws before
// prepare_ocean_context
struct OceanRay
{
  lml::Vec3 origin;
  float tmin;
  lml::Vec3 direction;                    // need not be normalised
  float tmax;
};

struct OceanRayRecord
{
  float hi;                               // the first parameter known to lie on the other side of the surface (a miss: tmax)
  float lo;                               // the last one known to lie on the starting side
  float g;                                // point(hi).z - the water height there
  float status;                           // 0 miss, 1 enter (started above), 2 leave (started below)
  OceanSurfaceSample sample;              // the surface at point(hi)
};

static_assert(sizeof(OceanRay) == 32, "OceanRay must be the C ABI's ray of DATUM_OCEAN_RAY_FLOATS floats");
static_assert(sizeof(OceanRayRecord) == 48, "OceanRayRecord must be the C ABI's record of DATUM_OCEAN_RAY_RECORD_FLOATS floats");

void cast_ocean_rays(OceanContext &context, OceanParams const &params, OceanRay const *rays, std::size_t n, OceanRayRecord *records, int iterations = 4, int steps = 32, int refine = 8);

// rippled reads (include/datum_ocean_hip.h: "rippled reads", the definition there): query_ocean_surface, cast_ocean_rays and the mesh WITH
// the ripple layer's current state on top -- the water step_ocean_bodies_coupled floats its bodies on.  Cascade 0 and host arrays, as their
// parents; gen_ocean_surface_rippled writes the rippled mesh of cascade 0 into `target`'s vertex buffer from the maps the context last
// displaced (after a render_ocean_surface / displace_ocean_surface) and displaces nothing itself.  All three throw before
// prepare_ocean_context, and while the layer is off (set_ocean_ripples)
void query_ocean_surface_rippled(OceanContext &context, OceanParams const &params, lml::Vec2 const *positions, std::size_t count, OceanSurfaceSample *samples, int iterations = 4);
void cast_ocean_rays_rippled(OceanContext &context, OceanParams const &params, OceanRay const *rays, std::size_t n, OceanRayRecord *records, int iterations = 4, int steps = 32, int refine = 8);
void gen_ocean_surface_rippled(OceanContext &context, Ocean const *target, Camera const &camera, OceanParams const &params);

// surface bounds (include/datum_ocean_hip.h: datum_ocean_reduce_bounds, the definition there): the extrema of the displacement the context
// last displaced, reduced on the device, and what they say about the surface under `params`: every height lies strictly between zlo and
// zhi, every vertex within `reach` of its undisplaced position along x and y.  One cascade, as query_ocean_surface.  reduce_ocean_bounds
// enqueues and returns; ocean_surface_slab reduces and blocks; cast_ocean_rays_bounded is cast_ocean_rays with the samples outside the slab
// decided without a height evaluation -- the same records bit for bit -- and throws unless reduce_ocean_bounds (or ocean_surface_slab) was
// called after the last render_ocean_surface / displace_ocean_surface.  All three throw before prepare_ocean_context
struct OceanSurfaceSlab
{
  float zlo, zhi;
  lml::Vec2 reach;
};

void reduce_ocean_bounds(OceanContext &context);
OceanSurfaceSlab ocean_surface_slab(OceanContext &context, OceanParams const &params);
void cast_ocean_rays_bounded(OceanContext &context, OceanParams const &params, OceanRay const *rays, std::size_t n, OceanRayRecord *records, int iterations = 4, int steps = 32, int refine = 8);

// ripple-layer bounds (include/datum_ocean_hip.h: datum_ocean_reduce_ripple_bounds, the definition there): the extrema of the ripple layer's
// height and rate, the cells that are not finite and the cells that are not at rest (active == 0: the layer is at rest, and stepping it or
// reading through it can be skipped); the slab of the rippled water, ocean_surface_slab with the layer on top; and cast_ocean_rays_rippled
// with the samples outside that slab decided without a height evaluation -- the same records bit for bit.  reduce_ocean_ripple_bounds
// reduces and blocks; ocean_surface_slab_rippled reduces both the displacement and the layer and blocks; cast_ocean_rays_rippled_bounded
// throws unless both were reduced after the last call that displaced and the last that stepped, moved, reset or set the layer.  All three
// throw before prepare_ocean_context, and while the layer is off (set_ocean_ripples)
struct OceanRippleBounds
{
  float etamin, etamax;
  float ratemin, ratemax;
  std::uint32_t nonfinite;
  std::uint32_t active;
};

OceanRippleBounds reduce_ocean_ripple_bounds(OceanContext &context);
OceanSurfaceSlab ocean_surface_slab_rippled(OceanContext &context, OceanParams const &params);
void cast_ocean_rays_rippled_bounded(OceanContext &context, OceanParams const &params, OceanRay const *rays, std::size_t n, OceanRayRecord *records, int iterations = 4, int steps = 32, int refine = 8);

// wake foam (include/datum_ocean_hip.h: "wake foam", the definition there): an R x R plane of coverage in [0, 1] beside the ripple layer, off
// until set_ocean_ripple_foam(context, true); set_ocean_ripples switches it off again.  step_ocean_ripple_foam updates it from the layer's
// current state (one launch, enqueued); query_ocean_ripple_foam gives the bilinear coverage at `count` positions and read_ocean_ripple_foam
// the whole plane in window order, R x R floats for the R given to set_ocean_ripples -- host arrays, blocking.  All four throw before
// prepare_ocean_context and while the layer is off; all but set_ocean_ripple_foam while the foam is off
void set_ocean_ripple_foam(OceanContext &context, bool on);
void step_ocean_ripple_foam(OceanContext &context, float dt);
void query_ocean_ripple_foam(OceanContext &context, lml::Vec2 const *positions, std::size_t count, float *coverage);
void read_ocean_ripple_foam(OceanContext &context, float *plane);

// dispersive ripples (include/datum_ocean_hip.h: "dispersive ripples", the definition there): the mode of step_ocean_ripples and of the
// layer's share of step_ocean_bodies_coupled -- the wave equation (the default) or deep water, omega^2 = g |k|, with gravity `g`.  Works
// while the layer is off and survives set_ocean_ripples; writes no state.  Throws before prepare_ocean_context
enum class OceanRippleDispersion
{
  Wave = 0,                               // DATUM_OCEAN_RIPPLE_WAVE
  Deep = 1,                               // DATUM_OCEAN_RIPPLE_DEEP
};

void set_ocean_ripple_dispersion(OceanContext &context, OceanRippleDispersion mode, float g = 9.81f);

// ripple walls (include/datum_ocean_hip.h: "ripple walls", the definition there): obstacles the layer's waves reflect off, boxes and
// ellipses whose axis the caller gives as (cosine, sine); a harbour is a list of boxes.  count == 0 turns walls off.  The read returns the
// R x R byte plane in window order.  Both throw before prepare_ocean_context and while the layer is off
typedef datum_ocean_ripple_wall OceanRippleWall;

void set_ocean_ripple_walls(OceanContext &context, OceanRippleWall const *walls, size_t count);
void read_ocean_ripple_walls(OceanContext &context, unsigned char *plane /* [R][R] */);

// the ripple bed (include/datum_ocean_hip.h: "ripple bed", the definition there): still-water depth under the layer from a host map of
// bed->width x bed->height floats, positive down; waves shoal, refract and break on it.  A null bed turns it off.  WAVE mode only.  The
// read returns the effective-depth plane and the surf-level plane in window order; either may be null.  Both throw before
// prepare_ocean_context and while the layer is off
typedef datum_ocean_ripple_bed OceanRippleBed;

void set_ocean_ripple_bed(OceanContext &context, OceanRippleBed const *bed, float const *depths);
void read_ocean_ripple_bed(OceanContext &context, float *depth /* [R][R] */, unsigned char *surf /* [R][R] */);

// ripple swell (include/datum_ocean_hip.h: "ripple swell", the definition there): the FFT swell reflects off the walls and the beach --
// the layer carries the reflection, the shadow and the diffraction.  WAVE mode only.  Per frame, after the displacement and
// center_ocean_ripples and before step_ocean_ripples or step_ocean_bodies_coupled, refresh_ocean_ripple_swell writes the forcing plane
// from cascade 0's surface (one launch, enqueued); a step reads it only while it is current.  The read returns the plane in MEMORY
// order.  All three throw before prepare_ocean_context and while the layer is off; the last two while swell is off
void set_ocean_ripple_swell(OceanContext &context, bool on);
void refresh_ocean_ripple_swell(OceanContext &context, OceanParams const &params, int iterations = 4);
void read_ocean_ripple_swell(OceanContext &context, float *plane /* [R][R] */);

// blocking read-backs for tools and tests
void read_ocean_displacement(OceanContext &context, float *maps /* [2][N][N][4] */);
void read_ocean_vertices(OceanContext &context, Ocean const *ocean, Mesh::Vertex *vertices);

// the OceanSet header render_ocean_surface uploads (ocean.cpp:731-747)
datum_ocean_set make_oceanset(Camera const &camera, OceanParams const &params);

// the reference's twiddle table (ocean.cpp:686-700), N x 2 log2(N) floats; kept for API parity
std::vector<float> ocean_twiddle_table(int resolution);
