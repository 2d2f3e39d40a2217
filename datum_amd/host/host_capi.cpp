//
// host_capi.cpp -- a flat C view of the C++ ocean API (ocean.h) so that the Python tests and bench.py
// can drive the host shim exactly as game code would (examples/ocean/ocean.cpp:31,46-52,59,135,165,179).
// Exceptions become a return code plus a message.
//

#include "ocean.h"

#include <cstdio>
#include <cstring>
#include <exception>

using namespace lml;

extern "C"
{
  struct datum_host_scalars
  {
    float plane[4];
    float swelllength, swellamplitude, swellsteepness, swellspeed;
    float swelldirection[2];
    float wavescale, waveamplitude, windspeed;
    float winddirection[2];
    float choppiness, smoothing;
    float swellphase;
    float flow[2];
    int resolution;
    int rejectedseeds;
    int pending;
  };

  struct datum_host_camera
  {
    float fov, aspect, znear, zfar;
    float position[3], target[3], up[3];
  };
}

namespace
{
  struct HostContext
  {
    DatumPlatform::PlatformInterface platform;
    AssetManager assets;
    OceanContext context;
    ResourceManager resources{context};
  };

  thread_local char g_error[512];

  int caught(std::exception const &e)
  {
    snprintf(g_error, sizeof(g_error), "%s", e.what());
    return -1;
  }

  // the flat view of a shim ray cast, and of a surface query: the arrays as the shim types them, an exception as the return code
  using CastRays = void (*)(OceanContext&, OceanParams const&, OceanRay const*, std::size_t, OceanRayRecord*, int, int, int);
  using QuerySurface = void (*)(OceanContext&, OceanParams const&, Vec2 const*, std::size_t, OceanSurfaceSample*, int);

  int cast_rays(CastRays cast, void *c, void *p, float const *rays, size_t n, float *records, int iterations, int steps, int refine)
  {
    try
    {
      cast(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), reinterpret_cast<OceanRay const*>(rays), n, reinterpret_cast<OceanRayRecord*>(records), iterations, steps, refine);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int query_surface(QuerySurface query, void *c, void *p, float const *xy, size_t count, float *samples, int iterations)
  {
    try
    {
      query(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), reinterpret_cast<Vec2 const*>(xy), count, reinterpret_cast<OceanSurfaceSample*>(samples), iterations);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  Camera make_camera(datum_host_camera const &c)
  {
    Camera camera;
    camera.set_projection(c.fov, c.aspect, c.znear, c.zfar);
    camera.lookat(Vec3(c.position[0], c.position[1], c.position[2]), Vec3(c.target[0], c.target[1], c.target[2]), Vec3(c.up[0], c.up[1], c.up[2]));
    return camera;
  }
}

extern "C"
{
  char const *datum_host_last_error() { return g_error; }

  void *datum_host_params_create(int resolution) { return new OceanParams(resolution); }
  void datum_host_params_destroy(void *p) { delete static_cast<OceanParams*>(p); }
  void *datum_host_params_clone(void *p) { return new OceanParams(*static_cast<OceanParams*>(p)); }       // OceanParams is copyable, like the reference's POD

  void datum_host_params_get(void *p, datum_host_scalars *s)
  {
    OceanParams const &o = *static_cast<OceanParams*>(p);

    s->plane[0] = o.plane.normal.x; s->plane[1] = o.plane.normal.y; s->plane[2] = o.plane.normal.z; s->plane[3] = o.plane.distance;
    s->swelllength = o.swelllength; s->swellamplitude = o.swellamplitude; s->swellsteepness = o.swellsteepness; s->swellspeed = o.swellspeed;
    s->swelldirection[0] = o.swelldirection.x; s->swelldirection[1] = o.swelldirection.y;
    s->wavescale = o.wavescale; s->waveamplitude = o.waveamplitude; s->windspeed = o.windspeed;
    s->winddirection[0] = o.winddirection.x; s->winddirection[1] = o.winddirection.y;
    s->choppiness = o.choppiness; s->smoothing = o.smoothing;
    s->swellphase = o.swellphase;
    s->flow[0] = o.flow.x; s->flow[1] = o.flow.y;
    s->resolution = o.resolution;
    s->rejectedseeds = o.rejectedseeds;
    s->pending = (int)o.updates.size();      // recorded update_ocean calls (OceanParams::updates)
  }

  // tunables only; state (swellphase, flow, arrays) is left alone
  void datum_host_params_set(void *p, datum_host_scalars const *s)
  {
    OceanParams &o = *static_cast<OceanParams*>(p);

    o.plane = { { s->plane[0], s->plane[1], s->plane[2] }, s->plane[3] };
    o.swelllength = s->swelllength; o.swellamplitude = s->swellamplitude; o.swellsteepness = s->swellsteepness; o.swellspeed = s->swellspeed;
    o.swelldirection = Vec2(s->swelldirection[0], s->swelldirection[1]);
    o.wavescale = s->wavescale; o.waveamplitude = s->waveamplitude; o.windspeed = s->windspeed;
    o.winddirection = Vec2(s->winddirection[0], s->winddirection[1]);
    o.choppiness = s->choppiness; o.smoothing = s->smoothing;
  }

  void datum_host_params_set_deviceheight(void *p, int on) { static_cast<OceanParams*>(p)->deviceheight = (on != 0); }
  // 0, or -1 when the history behind the host phase is gone (hostphase stays off: fetch_ocean_state first)
  int datum_host_params_set_hostphase(void *p, int on)
  {
    OceanParams &o = *static_cast<OceanParams*>(p);

    if (on && o.phaseupdates < o.firstupdate)
    {
      snprintf(g_error, sizeof(g_error), "hostphase: the update history behind OceanParams::phase is no longer recorded; fetch_ocean_state first");
      return -1;
    }

    o.hostphase = (on != 0);

    return 0;
  }

  // the field itself, as C++ code would set it (no validation: update_ocean then throws)
  void datum_host_params_poke_hostphase(void *p, int on) { static_cast<OceanParams*>(p)->hostphase = (on != 0); }

  // the reference's POD (OceanParamsPod, 82000 bytes): 0 / 1 = not current (fetch_ocean_state first) / -1 = not a 64 x 64 params
  int datum_host_params_to_pod(void *p, void *pod)
  {
    try
    {
      return to_pod(*static_cast<OceanParams*>(p), *static_cast<OceanParamsPod*>(pod)) ? 0 : 1;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  void *datum_host_params_from_pod(void const *pod) { return new OceanParams(from_pod(*static_cast<OceanParamsPod const*>(pod))); }

  int datum_host_pod_bytes() { return (int)sizeof(OceanParamsPod); }

  float *datum_host_params_seed(void *p) { return static_cast<OceanParams*>(p)->seed.data(); }
  float *datum_host_params_height(void *p) { return static_cast<OceanParams*>(p)->height.data(); }
  float *datum_host_params_phase(void *p) { return static_cast<OceanParams*>(p)->phase.data(); }

  void datum_host_seed_ocean(void *p, uint32_t rngseed, int use_random_device)
  {
    if (use_random_device)
      seed_ocean(*static_cast<OceanParams*>(p));
    else
      seed_ocean(*static_cast<OceanParams*>(p), rngseed);
  }

  void datum_host_lerp_ocean_swell(void *p, float swelllength, float swellamplitude, float swellspeed, float dx, float dy, float t)
  {
    lerp_ocean_swell(*static_cast<OceanParams*>(p), swelllength, swellamplitude, swellspeed, Vec2(dx, dy), t);
  }

  void datum_host_lerp_ocean_waves(void *p, float wavescale, float waveamplitude, float windspeed, float dx, float dy, float t)
  {
    lerp_ocean_waves(*static_cast<OceanParams*>(p), wavescale, waveamplitude, windspeed, Vec2(dx, dy), t);
  }

  int datum_host_update_ocean(void *p, float dt)
  {
    try
    {
      update_ocean(*static_cast<OceanParams*>(p), dt);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  void datum_host_make_oceanset(datum_host_camera const *camera, void *p, datum_ocean_set *out)
  {
    *out = make_oceanset(make_camera(*camera), *static_cast<OceanParams*>(p));
  }

  int datum_host_twiddle_table(int resolution, float *weights)
  {
    try
    {
      auto w = ocean_twiddle_table(resolution);
      memcpy(weights, w.data(), w.size() * sizeof(float));
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  // initialise_ocean_context + prepare_ocean_context (examples/ocean/ocean.cpp:31,165); flags: 1 = OceanContext::spectrumfp16, 2 = ::literaltransform, 4 = ::heightfp16
  void *datum_host_context_create_ex(int device, int resolution, int flags)
  {
    HostContext *hc = nullptr;

    try
    {
      hc = new HostContext;
      hc->platform.hipdevice = device;
      hc->context.resolution = resolution;
      hc->context.spectrumfp16 = (flags & 1) != 0;
      hc->context.literaltransform = (flags & 2) != 0;
      hc->context.heightfp16 = (flags & 4) != 0;

      initialise_ocean_context(hc->platform, hc->context, 0);

      while (!prepare_ocean_context(hc->platform, hc->context, hc->assets))
        ;

      return hc;
    }
    catch(std::exception const &e)
    {
      caught(e);
      delete hc;
      return nullptr;
    }
  }

  void *datum_host_context_create(int device, int resolution) { return datum_host_context_create_ex(device, resolution, 0); }

  void datum_host_context_destroy(void *c) { delete static_cast<HostContext*>(c); }

  void *datum_host_context_handle(void *c) { return static_cast<HostContext*>(c)->context.hip; }

  void *datum_host_ocean_create(void *c, int sizex, int sizey)
  {
    try
    {
      return const_cast<Ocean*>(static_cast<HostContext*>(c)->resources.create<Ocean>(sizex, sizey));
    }
    catch(std::exception const &e)
    {
      caught(e);
      return nullptr;
    }
  }

  void datum_host_ocean_release(void *c, void *ocean) { static_cast<HostContext*>(c)->resources.release<Ocean>(static_cast<Ocean const*>(ocean)); }

  void *datum_host_ocean_vertices(void *ocean) { return static_cast<Ocean const*>(ocean)->vertexbuffer.vertices; }

  int datum_host_ocean_indices(void *c, void *ocean, uint32_t *indices)
  {
    Ocean const *o = static_cast<Ocean const*>(ocean);

    return datum_ocean_device_read(static_cast<HostContext*>(c)->context.hip, indices, o->vertexbuffer.indices, (size_t)o->vertexbuffer.indexcount * sizeof(uint32_t));
  }

  int datum_host_render_ocean_surface(void *c, void *ocean, datum_host_camera const *camera, void *p)
  {
    try
    {
      render_ocean_surface(static_cast<HostContext*>(c)->context, static_cast<Ocean const*>(ocean), make_camera(*camera), *static_cast<OceanParams*>(p));
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_displace_ocean_surface(void *c, void *p)
  {
    try
    {
      displace_ocean_surface(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p));
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  size_t datum_host_release_parked_states(void *c, void *keep)
  {
    return release_parked_states(static_cast<HostContext*>(c)->context, static_cast<OceanParams const*>(keep));
  }

  int datum_host_parked_states(void *c) { return (int)static_cast<HostContext*>(c)->context.parked.size(); }

  int datum_host_fetch_ocean_state(void *c, void *p)
  {
    try
    {
      fetch_ocean_state(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p));
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_read_ocean_displacement(void *c, float *maps)
  {
    try
    {
      read_ocean_displacement(static_cast<HostContext*>(c)->context, maps);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_set_ocean_foam(void *c, int mode)
  {
    try
    {
      set_ocean_foam(static_cast<HostContext*>(c)->context, mode);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_set_ocean_foam_params(void *c, float threshold, float gain, float decay)
  {
    try
    {
      set_ocean_foam_params(static_cast<HostContext*>(c)->context, threshold, gain, decay);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_read_ocean_foam(void *c, float *foam)
  {
    try
    {
      read_ocean_foam(static_cast<HostContext*>(c)->context, foam);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_query_ocean_surface(void *c, void *p, float const *xy, size_t count, float *samples, int iterations)
  {
    return query_surface(query_ocean_surface, c, p, xy, count, samples, iterations);
  }

  int datum_host_set_ocean_velocity(void *c, int mode)
  {
    try
    {
      set_ocean_velocity(static_cast<HostContext*>(c)->context, mode);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_read_ocean_velocity(void *c, float *velocity)
  {
    try
    {
      read_ocean_velocity(static_cast<HostContext*>(c)->context, velocity);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_query_ocean_velocity(void *c, void *p, float const *xy, size_t count, float *samples, int iterations)
  {
    try
    {
      query_ocean_velocity(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), reinterpret_cast<Vec2 const*>(xy), count, reinterpret_cast<OceanVelocitySample*>(samples), iterations);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_reduce_ocean_bodies(void *c, void *p, void const *bodies, size_t nbodies, float const *probes, size_t nprobes, float *records, int iterations)
  {
    try
    {
      reduce_ocean_bodies(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), static_cast<datum_ocean_body const*>(bodies), nbodies, reinterpret_cast<OceanBodyProbe const*>(probes), nprobes, reinterpret_cast<OceanBodyRecord*>(records), iterations);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_reduce_ocean_body_drag(void *c, void *p, void const *bodies, void const *motions, size_t nbodies, float const *probes, size_t nprobes, float *records, int iterations)
  {
    try
    {
      reduce_ocean_body_drag(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), static_cast<datum_ocean_body const*>(bodies), static_cast<datum_ocean_body_motion const*>(motions), nbodies, reinterpret_cast<OceanBodyProbe const*>(probes), nprobes, reinterpret_cast<OceanDragRecord*>(records), iterations);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_step_ocean_bodies(void *c, void *p, void *bodies, void *motions, void const *props, size_t nbodies, float const *probes, size_t nprobes, float dt, int substeps, float *records, int iterations)
  {
    try
    {
      step_ocean_bodies(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), static_cast<datum_ocean_body*>(bodies), static_cast<datum_ocean_body_motion*>(motions), static_cast<datum_ocean_body_props const*>(props), nbodies, reinterpret_cast<OceanBodyProbe const*>(probes), nprobes, dt, substeps, reinterpret_cast<OceanStepRecord*>(records), iterations);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_set_ocean_ripples(void *c, int R, float cellsize)
  {
    try
    {
      set_ocean_ripples(static_cast<HostContext*>(c)->context, R, cellsize);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_set_ocean_ripple_dispersion(void *c, int mode, float g)
  {
    try
    {
      set_ocean_ripple_dispersion(static_cast<HostContext*>(c)->context, static_cast<OceanRippleDispersion>(mode), g);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_set_ocean_ripple_walls(void *c, void const *walls, size_t count)
  {
    try
    {
      set_ocean_ripple_walls(static_cast<HostContext*>(c)->context, static_cast<OceanRippleWall const*>(walls), count);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_read_ocean_ripple_walls(void *c, unsigned char *plane)
  {
    try
    {
      read_ocean_ripple_walls(static_cast<HostContext*>(c)->context, plane);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_set_ocean_ripple_bed(void *c, void const *bed, float const *depths)
  {
    try
    {
      set_ocean_ripple_bed(static_cast<HostContext*>(c)->context, static_cast<OceanRippleBed const*>(bed), depths);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_read_ocean_ripple_bed(void *c, float *depth, unsigned char *surf)
  {
    try
    {
      read_ocean_ripple_bed(static_cast<HostContext*>(c)->context, depth, surf);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_set_ocean_ripple_swell(void *c, int on)
  {
    try
    {
      set_ocean_ripple_swell(static_cast<HostContext*>(c)->context, on != 0);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_refresh_ocean_ripple_swell(void *c, void *p, int iterations)
  {
    try
    {
      refresh_ocean_ripple_swell(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), iterations);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_read_ocean_ripple_swell(void *c, float *plane)
  {
    try
    {
      read_ocean_ripple_swell(static_cast<HostContext*>(c)->context, plane);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_center_ocean_ripples(void *c, float x, float y)
  {
    try
    {
      center_ocean_ripples(static_cast<HostContext*>(c)->context, Vec2(x, y));
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_deposit_ocean_ripples(void *c, float const *impulses, size_t count)
  {
    try
    {
      deposit_ocean_ripples(static_cast<HostContext*>(c)->context, reinterpret_cast<OceanRippleImpulse const*>(impulses), count);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_deposit_ocean_body_ripples(void *c, void *p, void const *bodies, void const *motions, size_t nbodies, float const *probes, size_t nprobes, float dt, float *records, int iterations)
  {
    try
    {
      deposit_ocean_body_ripples(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), static_cast<datum_ocean_body const*>(bodies), static_cast<datum_ocean_body_motion const*>(motions), nbodies, reinterpret_cast<OceanBodyProbe const*>(probes), nprobes, dt, reinterpret_cast<OceanWakeRecord*>(records), iterations);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_step_ocean_ripples(void *c, float dt, int substeps)
  {
    try
    {
      step_ocean_ripples(static_cast<HostContext*>(c)->context, dt, substeps);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_query_ocean_ripples(void *c, float const *xy, size_t count, float *samples)
  {
    try
    {
      query_ocean_ripples(static_cast<HostContext*>(c)->context, reinterpret_cast<Vec2 const*>(xy), count, reinterpret_cast<OceanRippleSample*>(samples));
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_step_ocean_bodies_coupled(void *c, void *p, void *bodies, void *motions, void const *props, size_t nbodies, float const *probes, size_t nprobes, float dt, int substeps, float *records, int iterations)
  {
    try
    {
      step_ocean_bodies_coupled(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), static_cast<datum_ocean_body*>(bodies), static_cast<datum_ocean_body_motion*>(motions), static_cast<datum_ocean_body_props const*>(props), nbodies, reinterpret_cast<OceanBodyProbe const*>(probes), nprobes, dt, substeps, reinterpret_cast<OceanCoupledRecord*>(records), iterations);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_step_ocean_bodies_contact(void *c, void *p, void *bodies, void *motions, void const *props, size_t nbodies, float const *probes, size_t nprobes, float dt, int substeps, float *records, void const *contact, int iterations)
  {
    try
    {
      step_ocean_bodies_contact(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p), static_cast<datum_ocean_body*>(bodies), static_cast<datum_ocean_body_motion*>(motions), static_cast<datum_ocean_body_props const*>(props), nbodies, reinterpret_cast<OceanBodyProbe const*>(probes), nprobes, dt, substeps, reinterpret_cast<OceanContactRecord*>(records), *static_cast<datum_ocean_body_contact const*>(contact), iterations);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_cast_ocean_rays(void *c, void *p, float const *rays, size_t n, float *records, int iterations, int steps, int refine)
  {
    return cast_rays(cast_ocean_rays, c, p, rays, n, records, iterations, steps, refine);
  }

  int datum_host_query_ocean_surface_rippled(void *c, void *p, float const *xy, size_t count, float *samples, int iterations)
  {
    return query_surface(query_ocean_surface_rippled, c, p, xy, count, samples, iterations);
  }

  int datum_host_cast_ocean_rays_rippled(void *c, void *p, float const *rays, size_t n, float *records, int iterations, int steps, int refine)
  {
    return cast_rays(cast_ocean_rays_rippled, c, p, rays, n, records, iterations, steps, refine);
  }

  int datum_host_gen_ocean_surface_rippled(void *c, void *ocean, datum_host_camera const *camera, void *p)
  {
    try
    {
      gen_ocean_surface_rippled(static_cast<HostContext*>(c)->context, static_cast<Ocean const*>(ocean), make_camera(*camera), *static_cast<OceanParams*>(p));
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_reduce_ocean_bounds(void *c)
  {
    try
    {
      reduce_ocean_bounds(static_cast<HostContext*>(c)->context);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  // slab[4]: zlo, zhi, reach.x, reach.y
  int datum_host_ocean_surface_slab(void *c, void *p, float *slab)
  {
    try
    {
      OceanSurfaceSlab const s = ocean_surface_slab(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p));
      slab[0] = s.zlo; slab[1] = s.zhi; slab[2] = s.reach.x; slab[3] = s.reach.y;
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_cast_ocean_rays_bounded(void *c, void *p, float const *rays, size_t n, float *records, int iterations, int steps, int refine)
  {
    return cast_rays(cast_ocean_rays_bounded, c, p, rays, n, records, iterations, steps, refine);
  }

  // extrema[4]: etamin, etamax, ratemin, ratemax; counts[2]: nonfinite, active
  int datum_host_reduce_ocean_ripple_bounds(void *c, float *extrema, std::uint32_t *counts)
  {
    try
    {
      OceanRippleBounds const b = reduce_ocean_ripple_bounds(static_cast<HostContext*>(c)->context);
      extrema[0] = b.etamin; extrema[1] = b.etamax; extrema[2] = b.ratemin; extrema[3] = b.ratemax;
      counts[0] = b.nonfinite; counts[1] = b.active;
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  // slab[4]: zlo, zhi, reach.x, reach.y
  int datum_host_ocean_surface_slab_rippled(void *c, void *p, float *slab)
  {
    try
    {
      OceanSurfaceSlab const s = ocean_surface_slab_rippled(static_cast<HostContext*>(c)->context, *static_cast<OceanParams*>(p));
      slab[0] = s.zlo; slab[1] = s.zhi; slab[2] = s.reach.x; slab[3] = s.reach.y;
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_cast_ocean_rays_rippled_bounded(void *c, void *p, float const *rays, size_t n, float *records, int iterations, int steps, int refine)
  {
    return cast_rays(cast_ocean_rays_rippled_bounded, c, p, rays, n, records, iterations, steps, refine);
  }

  int datum_host_set_ocean_ripple_foam(void *c, int on)
  {
    try
    {
      set_ocean_ripple_foam(static_cast<HostContext*>(c)->context, on != 0);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_step_ocean_ripple_foam(void *c, float dt)
  {
    try
    {
      step_ocean_ripple_foam(static_cast<HostContext*>(c)->context, dt);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_query_ocean_ripple_foam(void *c, float const *xy, size_t count, float *coverage)
  {
    try
    {
      query_ocean_ripple_foam(static_cast<HostContext*>(c)->context, reinterpret_cast<Vec2 const*>(xy), count, coverage);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_read_ocean_ripple_foam(void *c, float *plane)
  {
    try
    {
      read_ocean_ripple_foam(static_cast<HostContext*>(c)->context, plane);
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }

  int datum_host_read_ocean_vertices(void *c, void *ocean, float *vertices)
  {
    try
    {
      read_ocean_vertices(static_cast<HostContext*>(c)->context, static_cast<Ocean const*>(ocean), reinterpret_cast<Mesh::Vertex*>(vertices));
      return 0;
    }
    catch(std::exception const &e) { return caught(e); }
  }
}
