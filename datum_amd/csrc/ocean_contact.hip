// ocean_contact.hip -- body contact (include/datum_ocean_hip.h: datum_ocean_step_bodies_contact): ONE coupled sub-step of every body with
// penalty contact against the ripple bed and the ripple walls, per launch; the host puts a sub-step of the layer between two launches
// exactly as it does for coupled stepping (ocean_capi.hip: one loop for both).  The kernel is ocean_couple_kernel's shape (ocean_couple.hip)
// and its first walk over the probes is that kernel's, callable and all; the contact terms are summed in a second walk over the same
// probes in the same order -- each field's chain of additions is what one walk would give -- so that the scene's scalars and the
// several-cascade query's are never held at once.  The arithmetic is ocean_contact.h's, and through it ocean_couple.h's,
// ocean_step.h's, ocean_ripple_bed.h's and ocean_ripple_wall.h's (a CPU walks the same functions).
//
//   * one wave per body, four bodies per 256-thread workgroup;
//   * the body, the motion, the props and, after the call's first sub-step, four floats of the old record are read with the wave-uniform
//     index: scalar loads; the contact parameters and the bed's terms come with the kernel's arguments;
//   * a wall record is 32 bytes at a wave-uniform address: one load of the line that every lane shares, its eight dwords then made
//     scalars (readfirstlane), so the shape's arithmetic that does not depend on the probe is scalar; the cover test comes first, and a
//     shape that covers no lane's probe is passed over by the whole wave;
//   * a probe's four texels of the depth map are fetched through a buffer resource over exactly the handle's copy of the map;
//     ripple_bed_patch asks only for texels of the map;
//   * the probes of the second walk are the first walk's loads again (16 bytes a lane and pass, from cache);
//   * the layer's cells, the deposits, the tree, the uniform sums and the stores are coupled stepping's; lane 0 stores the record as four
//     16-byte stores, a bad body sixteen quiet NaNs.
// No LDS, no barrier, no scratch (make resource-usage).

#pragma once

#include "ocean_contact.h"
#include "ocean_couple.hip"

namespace ocean
{
  struct ContactArgs
  {
    CoupleArgs c;                                         // c.d.b.records: the contact records, 4 float4 per body
    ContactScene s;
    float const *map;                                     // [height][width] the depth map, read under flag BED only
  };

  // the wave's 64 twenty-two-field partials, one per lane (ocean_body.h: body_tree)
  struct ContactWave
  {
    ContactPartial p;

    template<int S>
    __device__ __forceinline__ void step()
    {
      ContactPartial o;

      #pragma unroll
      for(int k = 0; k < STEP_FIELDS; ++k)
        o.c.s.f[k] = body_lane_up<S>(p.c.s.f[k]);

      #pragma unroll
      for(int k = 0; k < COUPLE_WAKE_FIELDS; ++k)
        o.c.w[k] = body_lane_up<S>(p.c.w[k]);

      #pragma unroll
      for(int k = 0; k < CONTACT_FIELDS; ++k)
        o.k[k] = body_lane_up<S>(p.k[k]);

      body_add(p, o);
    }
  };

  template<int LAYOUT>
  __global__ void __launch_bounds__(BODY_THREADS) ocean_contact_kernel(ContactArgs ca)
  {
    CoupleArgs const &a = ca.c;
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

    float old7 = 0.0f, old11 = 0.0f, old15 = 0.0f;

    if (!a.first)
    {
      float4 const *old = ba.records + 4 * (size_t)body;

      bad = bad || couple_was_bad(old[0].x);
      old7 = old[1].w;
      old11 = old[2].w;
      old15 = old[3].w;
    }

    ContactWave wave;
    wave.p = contact_zero();

    StepTotals total = {};

    if (!bad)
    {
      __amdgpu_buffer_rsrc_t const rstate = make_rsrc(a.state, (size_t)a.g.R * a.g.R * sizeof(float2));
      // the coupled kernel's walk, as it stands there, into the fourteen fields
      bool const badprobe = body_walk(B, ba.probes, B.count, lane, wave.p.c, [&a, &ba, &B, &M, &rstate](BodyWorld const &w, float weight)
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

      // the contact's eight fields in a walk of their own over the same probes, in the same order: the same chains of additions, and
      // the scene's scalars are not held beside the query's
      ContactSums contact;

      #pragma unroll
      for(int k = 0; k < CONTACT_FIELDS; ++k)
        contact.k[k] = 0.0f;

      __amdgpu_buffer_rsrc_t const rmap = make_rsrc(ca.map, (size_t)ca.s.bed.width * ca.s.bed.height * sizeof(float));

      body_walk(B, ba.probes, B.count, lane, contact, [&ca, &B, &M, &rmap](BodyWorld const &w, float weight)
      {
        ContactSums t;

        contact_terms(t.k, B, M, ca.s, w, weight, [&rmap](int index) { return buf_load_f32(rmap, index * (int)sizeof(float), 0); }, [&ca](int i)
        {
          // the record's eight dwords, the same in every lane, made scalars
          datum_ocean_ripple_wall const v = ca.s.walls[i];

          datum_ocean_ripple_wall u;
          u.center[0] = couple_uniform(v.center[0]);
          u.center[1] = couple_uniform(v.center[1]);
          u.axis[0] = couple_uniform(v.axis[0]);
          u.axis[1] = couple_uniform(v.axis[1]);
          u.half[0] = couple_uniform(v.half[0]);
          u.half[1] = couple_uniform(v.half[1]);
          u.kind = __builtin_amdgcn_readfirstlane(v.kind);
          u.reserved = __builtin_amdgcn_readfirstlane(v.reserved);
          return u;
        });

        return t;
      });

      #pragma unroll
      for(int k = 0; k < CONTACT_FIELDS; ++k)
        wave.p.k[k] = contact.k[k];

      bad = __builtin_amdgcn_ballot_w64(badprobe) != 0;
    }

    ContactPartial sums = contact_zero();

    if (!bad)
    {
      body_tree(wave);

      #pragma unroll
      for(int k = 0; k < STEP_FIELDS; ++k)
        sums.c.s.f[k] = couple_uniform(wave.p.c.s.f[k]);

      #pragma unroll
      for(int k = 0; k < COUPLE_WAKE_FIELDS; ++k)
        sums.c.w[k] = couple_uniform(wave.p.c.w[k]);

      #pragma unroll
      for(int k = 0; k < CONTACT_FIELDS; ++k)
        sums.k[k] = couple_uniform(wave.p.k[k]);

      total = contact_integrate(B, M, P, sums, a.h);

      bad = !step_state_finite(B, M);
    }

    if (lane == 0)
    {
      float const nan = __builtin_nanf("");

      __amdgpu_buffer_rsrc_t const rrecord = make_rsrc(ba.records + 4 * (size_t)body, 4 * sizeof(float4));

      if (bad)
      {
        buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecord, 0, 0);
        buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecord, 16, 0);
        buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecord, 32, 0);
        buf_store_f32x4_aux<0>(make_float4(nan, nan, nan, nan), rrecord, 48, 0);
      }
      else
      {
        float const *R = B.rotation, *T = B.position;

        ContactRecord const c = contact_fold(total, sums, a.first != 0, old7, old11, old15);

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
        buf_store_f32x4_aux<0>(make_float4(c.f[12], c.f[13], c.f[14], c.f[15]), rrecord, 48, 0);
      }
    }
  }

  // a.c as launch_couple takes it, the scene and the map filled in; a.c.d.b.nbodies > 0
  inline hipError_t launch_contact(ContactArgs &a, hipStream_t stream)
  {
    query_frame(a.c.d.b.q);

    void *args[] = { &a };

    return hipLaunchKernel(layout_kernel(a.c.d.b.q.N, &ocean_contact_kernel<GEN_PLAIN>, &ocean_contact_kernel<GEN_BANDED>), dim3((unsigned)(((size_t)a.c.d.b.nbodies + BODY_WAVES - 1) / BODY_WAVES)), dim3(BODY_THREADS), args, 0, stream);
  }
}
