// ocean_drag.hip -- body drag (include/datum_ocean_hip.h: datum_ocean_reduce_body_drag): per body, the force and the torque of the water's
// motion relative to the hull, summed over the body's hull probes.  The arithmetic of a probe is ocean_drag.h's (a CPU walks the same
// functions); the walk over the probes, the bad-body rules, the register tree and the store are body buoyancy's, the same function
// (ocean_body.hip: body_each_probe); the velocity record of a probe is the several-cascade velocity query's, the same functions
// (ocean_query.hip), so its bits are datum_ocean_sample_velocity_blend's.
//
//   * one wave per body, four bodies per 256-thread workgroup, as ocean_body_kernel;
//   * the body's 64 bytes and the motion's 32 are read with the wave-uniform index: scalar loads;
//   * a body with a bad motion walks no probe and fetches nothing; its record is eight quiet NaNs.
// This file makes no texel and loads from no map or plane itself.  No LDS, no barrier, no atomics, no scratch (make resource-usage).

#pragma once

#include "ocean_drag.h"
#include "ocean_body.hip"

namespace ocean
{
  struct DragArgs
  {
    BodyArgs b;                                           // b.q.list's foam planes are not read
    datum_ocean_body_motion const *motions;               // one per body
    float4 const *vel[DATUM_OCEAN_MAX_CASCADES];          // the listed cascades' velocity planes, in list order (as VelocityBlendArgs)
  };

  template<int LAYOUT>
  __global__ void __launch_bounds__(BODY_THREADS) ocean_drag_kernel(DragArgs a)
  {
    body_each_probe(a.b.bodies, a.b.probes, a.b.records, a.b.nbodies, a.b.nprobes, [&](int body, datum_ocean_body const &B, bool &bad)
    {
      datum_ocean_body_motion const M = a.motions[body];

      bad = bad || drag_motion_bad(M);

      return [&a, &B, M](BodyWorld const &w, float weight)
      {
        float2 const q = make_float2(w.x, w.y);

        QueryRecord const r = query_velocity<LAYOUT>(a.b.q, query_solve<LAYOUT>(a.b.q, q), q, a.vel);

        float const rec[DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS] = { r.v.x, r.v.y, r.v.z, r.v.w, r.m.x, r.m.y, r.m.z, r.m.w };

        return drag_terms(B, M, w, weight, rec);
      };
    });
  }

  // a.b (but its frame), motions and vel filled in; a.b.nbodies > 0
  inline hipError_t launch_body_drag(DragArgs &a, hipStream_t stream)
  {
    query_frame(a.b.q);

    void *args[] = { &a };

    return hipLaunchKernel(layout_kernel(a.b.q.N, &ocean_drag_kernel<GEN_PLAIN>, &ocean_drag_kernel<GEN_BANDED>), dim3((unsigned)(((size_t)a.b.nbodies + BODY_WAVES - 1) / BODY_WAVES)), dim3(BODY_THREADS), args, 0, stream);
  }
}
