// ocean_couple.hip -- coupled stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies_coupled): ONE coupled sub-step of every body --
// buoyancy, drag and the wake from records that carry the ripple layer's height and rate, then the integrator -- per launch; the host
// puts a sub-step of the layer between two launches (ocean_capi.hip), which needs the whole device.  The arithmetic is ocean_couple.h's,
// and through it ocean_step.h's and ocean_ripple.h's (a CPU walks the same functions); the passes over the probes are body buoyancy's
// (ocean_body.hip: body_walk), the tree is body_tree; the velocity record of a probe is the several-cascade velocity query's
// (ocean_query.hip), solved ONCE per probe for the step's and the wake's terms.
//
//   * one wave per body, four bodies per 256-thread workgroup, as ocean_step_kernel;
//   * the body's 64 bytes, the motion's 32, the props' 32 and, after the call's first sub-step, three floats of the old record are read
//     with the wave-uniform index: scalar loads;
//   * a probe's four cells of the layer are fetched through a buffer resource over exactly the current state plane; ripple_sample asks
//     only for cells inside the window, whose indices lie inside the plane;
//   * the deposits are vector atomics on the int plane in plain C++, at indices ripple_splat hands over: inside the plane;
//   * after the tree lane 0's fourteen sums are made wave-uniform (readfirstlane) and every lane integrates the same numbers;
//   * lane 0 stores pose (48 bytes), motion and record (48 bytes) as 16-byte stores through resources laid over this body's slots; a bad
//     body stores only its record of twelve quiet NaNs, and one that was bad before this sub-step fetches and deposits nothing.
// No LDS, no barrier, no scratch (make resource-usage).

#pragma once

#include "ocean_couple.h"
#include "ocean_step.hip"
#include "ocean_ripple.hip"

namespace ocean
{
  struct CoupleArgs
  {
    DragArgs d;                                           // d.b.records: the coupled records, 3 float4 per body
    datum_ocean_body *bodies;                             // d.b.bodies and d.motions once more, to be written
    datum_ocean_body_motion *motions;
    datum_ocean_body_props const *props;                  // one per body
    float2 const *state;                                  // [R][R] (eta, rate): the layer's current state, read only
    int *src;                                             // [R][R] pending deposits
    RippleGrid g;
    float h;                                              // dt * (1.0f / substeps), rounded on the host
    int first;                                            // the call's first sub-step: the old record is not read
  };

  // the wave's 64 fourteen-field partials, one per lane (ocean_body.h: body_tree)
  struct CoupleWave
  {
    CouplePartial p;

    template<int S>
    __device__ __forceinline__ void step()
    {
      CouplePartial o;

      #pragma unroll
      for(int k = 0; k < STEP_FIELDS; ++k)
        o.s.f[k] = body_lane_up<S>(p.s.f[k]);

      #pragma unroll
      for(int k = 0; k < COUPLE_WAKE_FIELDS; ++k)
        o.w[k] = body_lane_up<S>(p.w[k]);

      body_add(p, o);
    }
  };

  __device__ __forceinline__ float couple_uniform(float v)
  {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
  }

  template<int LAYOUT>
  __global__ void __launch_bounds__(BODY_THREADS) ocean_couple_kernel(CoupleArgs a)
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

    float old7 = 0.0f, old11 = 0.0f;

    if (!a.first)
    {
      float4 const *old = ba.records + 3 * (size_t)body;

      bad = bad || couple_was_bad(old[0].x);
      old7 = old[1].w;
      old11 = old[2].w;
    }

    CoupleWave wave;
    wave.p = couple_zero();

    StepTotals total = {};

    if (!bad)
    {
      __amdgpu_buffer_rsrc_t const rstate = make_rsrc(a.state, (size_t)a.g.R * a.g.R * sizeof(float2));

      bool const badprobe = body_walk(B, ba.probes, B.count, lane, wave.p, [&a, &ba, &B, &M, &rstate](BodyWorld const &w, float weight)
      {
        float2 const q = make_float2(w.x, w.y);

        QueryRecord const r = query_velocity<LAYOUT>(ba.q, query_solve<LAYOUT>(ba.q, q), q, a.d.vel);

        float const rec[DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS] = { r.v.x, r.v.y, r.v.z, r.v.w, r.m.x, r.m.y, r.m.z, r.m.w };

        RippleSample const s = ripple_sample(a.g, w.x, w.y, [&rstate](int index)
        {
          float2 const c = buf_load_f32x2(rstate, index * (int)sizeof(float2), 0);

          return RippleCell{ c.x, c.y };
        });

        float rippled[DATUM_OCEAN_VELOCITY_SAMPLE_FLOATS];

        couple_record(rippled, rec, s);

        return couple_terms(B, M, w, weight, rippled, a.h, [&a](float x, float y, float V)
        {
          return ripple_splat(a.g, x, y, V, [&a](int index, int quantum) { atomicAdd(a.src + index, quantum); });
        });
      });

      bad = __builtin_amdgcn_ballot_w64(badprobe) != 0;
    }

    CouplePartial sums = couple_zero();

    if (!bad)
    {
      body_tree(wave);

      #pragma unroll
      for(int k = 0; k < STEP_FIELDS; ++k)
        sums.s.f[k] = couple_uniform(wave.p.s.f[k]);

      #pragma unroll
      for(int k = 0; k < COUPLE_WAKE_FIELDS; ++k)
        sums.w[k] = couple_uniform(wave.p.w[k]);

      total = step_integrate(B, M, P, sums.s, a.h);

      bad = !step_state_finite(B, M);
    }

    if (lane == 0)
    {
      float const nan = __builtin_nanf("");

      __amdgpu_buffer_rsrc_t const rrecord = make_rsrc(ba.records + 3 * (size_t)body, 3 * sizeof(float4));

      if (bad)
      {
        buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecord, 0, 0);
        buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecord, 16, 0);
        buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecord, 32, 0);
      }
      else
      {
        float const *R = B.rotation, *T = B.position;

        CoupleRecord const c = couple_fold(total, sums, a.first != 0, old7, old11);

        __amdgpu_buffer_rsrc_t const rbody = make_rsrc(a.bodies + (size_t)body, 3 * sizeof(float4));
        __amdgpu_buffer_rsrc_t const rmotion = make_rsrc(a.motions + (size_t)body, 2 * sizeof(float4));

        buf_store_f32x4_aux<0>(make_float4(R[0], R[1], R[2], R[3]), rbody, 0, 0);
        buf_store_f32x4_aux<0>(make_float4(R[4], R[5], R[6], R[7]), rbody, 16, 0);
        buf_store_f32x4_aux<0>(make_float4(R[8], T[0], T[1], T[2]), rbody, 32, 0);

        buf_store_f32x4_aux<0>(make_float4(M.linear[0], M.linear[1], M.linear[2], M.angular[0]), rmotion, 0, 0);
        buf_store_f32x4_aux<0>(make_float4(M.angular[1], M.angular[2], M.cl, M.cq), rmotion, 16, 0);

        buf_store_f32x4_aux<0>(make_float4(c.f[0], c.f[1], c.f[2], c.f[3]), rrecord, 0, 0);
        buf_store_f32x4_aux<0>(make_float4(c.f[4], c.f[5], c.f[6], c.f[7]), rrecord, 16, 0);
        buf_store_f32x4_aux<0>(make_float4(c.f[8], c.f[9], c.f[10], c.f[11]), rrecord, 32, 0);
      }
    }
  }

  // a.d (but its frame), bodies, motions, props, the layer, h and first filled in; a.d.b.nbodies > 0
  inline hipError_t launch_couple(CoupleArgs &a, hipStream_t stream)
  {
    query_frame(a.d.b.q);

    void *args[] = { &a };

    return hipLaunchKernel(layout_kernel(a.d.b.q.N, &ocean_couple_kernel<GEN_PLAIN>, &ocean_couple_kernel<GEN_BANDED>), dim3((unsigned)(((size_t)a.d.b.nbodies + BODY_WAVES - 1) / BODY_WAVES)), dim3(BODY_THREADS), args, 0, stream);
  }
}
