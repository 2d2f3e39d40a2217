// ocean_step.hip -- body stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies): per body, `substeps` sub-steps of buoyancy, drag and
// a semi-implicit Euler integrator against the surface as it lies, the pose and the motion written back once.  The arithmetic of a probe,
// the ten sums and the integrator are ocean_step.h's (a CPU walks the same functions); the passes over the probes are body buoyancy's, the
// same function (ocean_body.hip: body_walk), the tree is body_tree; the velocity record of a probe is the several-cascade velocity
// query's, the same functions (ocean_query.hip), solved ONCE per probe and sub-step for both the buoyancy's and the drag's terms.
//
//   * one wave per body, four bodies per 256-thread workgroup, as ocean_body_kernel;
//   * the body's 64 bytes, the motion's 32 and the props' 32 are read with the wave-uniform index: scalar loads;
//   * pose and motion stay in registers from sub-step to sub-step: after each tree lane 0's ten sums are made wave-uniform
//     (readfirstlane), every lane integrates the same numbers and so holds the next pose;
//   * lane 0 stores pose (48 bytes: first, count, cap do not change), motion and record once, after the last sub-step, as 16-byte stores
//     through resources laid over this body's slots; a bad body stores only its record of eight quiet NaNs;
//   * a body that turns bad walks no further sub-step and fetches nothing from then on.
// This file makes no texel and loads from no map or plane itself.  No LDS, no barrier, no atomics, no scratch (make resource-usage).

#pragma once

#include "ocean_step.h"
#include "ocean_drag.hip"

namespace ocean
{
  struct BodyStepArgs
  {
    DragArgs d;                                           // d.b.records: the step's records
    datum_ocean_body *bodies;                             // d.b.bodies and d.motions once more, to be written
    datum_ocean_body_motion *motions;
    datum_ocean_body_props const *props;                  // one per body
    float h;                                              // dt * (1.0f / substeps), rounded on the host
    int substeps;
  };

  // the wave's 64 ten-field partials, one per lane (ocean_body.h: body_tree)
  struct StepWave
  {
    StepPartial p;

    template<int S>
    __device__ __forceinline__ void step()
    {
      StepPartial o;

      #pragma unroll
      for(int k = 0; k < STEP_FIELDS; ++k)
        o.f[k] = body_lane_up<S>(p.f[k]);

      body_add(p, o);
    }
  };

  template<int LAYOUT>
  __global__ void __launch_bounds__(BODY_THREADS) ocean_step_kernel(BodyStepArgs a)
  {
    BodyArgs const &ba = a.d.b;

    int const lane = (int)threadIdx.x & (BODY_LANES - 1);
    int const body = __builtin_amdgcn_readfirstlane((int)blockIdx.x * BODY_WAVES + ((int)threadIdx.x >> 6));

    // (the whole wave: the last workgroup's waves without a body)
    if (body >= ba.nbodies)
      return;

    datum_ocean_body B = ba.bodies[body];
    datum_ocean_body_motion M = a.d.motions[body];
    datum_ocean_body_props const P = a.props[body];

    // every `bad` below is wave-uniform: scalar loads, a ballot, sums that went through readfirstlane
    bool bad = body_range_bad(B, ba.nprobes) || step_props_bad(P) || drag_motion_bad(M);

    StepTotals total = {};
    float submerged = 0.0f, residual = 0.0f;

    for(int s = 0; s < a.substeps && !bad; ++s)
    {
      StepWave wave;
      wave.p = step_zero();

      bool const badprobe = body_walk(B, ba.probes, B.count, lane, wave.p, [&a, &ba, &B, &M](BodyWorld const &w, float weight)
      {
        float2 const q = make_float2(w.x, w.y);

        QueryRecord const r = query_velocity<LAYOUT>(ba.q, query_solve<LAYOUT>(ba.q, q), q, a.d.vel);

        float const rec[DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS] = { r.v.x, r.v.y, r.v.z, r.v.w, r.m.x, r.m.y, r.m.z, r.m.w };

        return step_terms(B, M, w, weight, rec);
      });

      bad = __builtin_amdgcn_ballot_w64(badprobe) != 0;

      if (bad)
        break;

      body_tree(wave);

      StepPartial sums;

      #pragma unroll
      for(int k = 0; k < STEP_FIELDS; ++k)
        sums.f[k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wave.p.f[k])));

      total = step_integrate(B, M, P, sums, a.h);
      submerged = sums.f[0];
      residual = fmaxf(residual, sums.f[STEP_FIELDS - 1]);

      bad = !step_state_finite(B, M);
    }

    if (lane == 0)
    {
      float const nan = __builtin_nanf("");

      __amdgpu_buffer_rsrc_t const rrecord = make_rsrc(ba.records + 2 * (size_t)body, 2 * sizeof(float4));

      if (bad)
      {
        buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecord, 0, 0);
        buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecord, 16, 0);
      }
      else
      {
        float const *R = B.rotation, *T = B.position, *F = total.force, *Q = total.torque;

        __amdgpu_buffer_rsrc_t const rbody = make_rsrc(a.bodies + (size_t)body, 3 * sizeof(float4));
        __amdgpu_buffer_rsrc_t const rmotion = make_rsrc(a.motions + (size_t)body, 2 * sizeof(float4));

        buf_store_f32x4_aux<0>(make_float4(R[0], R[1], R[2], R[3]), rbody, 0, 0);
        buf_store_f32x4_aux<0>(make_float4(R[4], R[5], R[6], R[7]), rbody, 16, 0);
        buf_store_f32x4_aux<0>(make_float4(R[8], T[0], T[1], T[2]), rbody, 32, 0);

        buf_store_f32x4_aux<0>(make_float4(M.linear[0], M.linear[1], M.linear[2], M.angular[0]), rmotion, 0, 0);
        buf_store_f32x4_aux<0>(make_float4(M.angular[1], M.angular[2], M.cl, M.cq), rmotion, 16, 0);

        buf_store_f32x4_aux<0>(make_float4(F[0], F[1], F[2], Q[0]), rrecord, 0, 0);
        buf_store_f32x4_aux<0>(make_float4(Q[1], Q[2], submerged, residual), rrecord, 16, 0);
      }
    }
  }

  inline void const *step_kernel_for(int N)
  {
    switch(gen_layout(N))
    {
      case GEN_PLAIN: return reinterpret_cast<void const*>(&ocean_step_kernel<GEN_PLAIN>);
      default: return reinterpret_cast<void const*>(&ocean_step_kernel<GEN_BANDED>);
    }
  }

  // a.d (but its frame), bodies, motions, props, h and substeps filled in; a.d.b.nbodies > 0
  inline hipError_t launch_step_bodies(BodyStepArgs &a, hipStream_t stream)
  {
    query_frame(a.d.b.q);

    void *args[] = { &a };

    return hipLaunchKernel(step_kernel_for(a.d.b.q.N), dim3((unsigned)(((size_t)a.d.b.nbodies + BODY_WAVES - 1) / BODY_WAVES)), dim3(BODY_THREADS), args, 0, stream);
  }
}
