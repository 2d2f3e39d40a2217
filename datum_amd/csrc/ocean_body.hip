// ocean_body.hip -- body buoyancy (include/datum_ocean_hip.h: datum_ocean_reduce_bodies): per body, the net buoyant force, its torque and a
// few aggregates over the body's hull probes, each probe moved to world space with the body's pose and held against the summed surface
// above it.  The arithmetic of a probe and the order of the sum are ocean_body.h's (a CPU walks the same functions); the surface record of
// a probe is the several-cascade query's, the same functions (ocean_query.hip: query_solve, query_record), so its bits are
// datum_ocean_sample_surface_blend's.
//
//   * one wave per body, four bodies per 256-thread workgroup; lane l takes probes first + l, first + l + 64, ...;
//   * a probe is one 16-byte load per lane, 64 consecutive probes per wave and pass, through a buffer resource laid over exactly the
//     probes of that pass: no first / count can reach outside the probe array (a bad range is refused before, body_range_bad);
//   * the body's 64 bytes are read with a wave-uniform index: scalar loads;
//   * the 64 partials are added across lanes in registers -- the half exchange of v_permlane32_swap and v_permlane16_swap for the strides
//     32 and 16, DPP row shifts below -- every lane alive to the end; lane 0 stores the record, two 16-byte stores;
//   * a bad probe fetches nothing; its body's record is eight quiet NaNs.
// No LDS, no barrier, no atomics, no scratch (make resource-usage).
// The walk (body_each_probe) takes the per-probe terms as a callable, as query_each_point does for points: body drag (ocean_drag.hip) is
// the same walk with other terms.

#pragma once

#include "ocean_body.h"
#include "ocean_blend.hip"

namespace ocean
{
  struct BodyArgs
  {
    QueryArgs q;
    datum_ocean_body const *bodies;
    BodyProbe const *probes;
    float4 *records;        // 2 float4 per body
    int nbodies;
    int nprobes;
  };

  constexpr int BODY_THREADS = 256;
  constexpr int BODY_WAVES = BODY_THREADS / BODY_LANES;

  // lane l + S's value in lane l, for l < S (what the other lanes get is not used)
  template<int S>
  __device__ __forceinline__ float body_lane_up(float v)
  {
    unsigned int const u = __builtin_bit_cast(unsigned int, v);

    // v_permlane32_swap a, b exchanges lanes 32-63 of a with lanes 0-31 of b, v_permlane16_swap the odd rows (of 16 lanes) of a with the
    // even rows of b: given the same value twice, b then holds lane l + S's value in lane l; the builtin returns (a, b).  (The element
    // goes through a scalar: __builtin_bit_cast applied to the element itself read element 0 with this compiler)
    if constexpr (S == 32)
    {
      unsigned int const b = __builtin_amdgcn_permlane32_swap(u, u, false, false)[1];
      return __builtin_bit_cast(float, b);
    }
    else if constexpr (S == 16)
    {
      unsigned int const b = __builtin_amdgcn_permlane16_swap(u, u, false, false)[1];
      return __builtin_bit_cast(float, b);
    }
    else
      return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, (int)u, 0x100 + S, 0xF, 0xF, true));   // row_shl:S
  }

  // the wave's 64 partials, one per lane (ocean_body.h: body_tree)
  struct BodyWave
  {
    BodyPartial p;

    template<int S>
    __device__ __forceinline__ void step()
    {
      BodyPartial o;

      #pragma unroll
      for(int k = 0; k < BODY_FIELDS; ++k)
        o.f[k] = body_lane_up<S>(p.f[k]);

      body_add(p, o);
    }
  };

  // The passes over the first n probes of body B's range (n = 0: none), stated once for every kernel that sums per body: every lane walks
  // the passes, loads its probe through a resource over that pass's probes, transforms it, and adds to its partial p the terms -- a
  // callable (w, a) -> Partial, added with body_add -- of a probe that is its own and not bad.  True in a lane that met a bad probe.
  // (ocean_step.hip loops over this, one walk per sub-step, with a pose that moves)
  template<class Partial, class Terms>
  __device__ __forceinline__ bool body_walk(datum_ocean_body const &B, BodyProbe const *probes, int n, int lane, Partial &p, Terms &&terms)
  {
    bool badprobe = false;

    // lane 0 has the most probes: every lane walks its passes (wave-uniform), `have` says whether a pass holds a probe for this lane
    for(int k = 0; k < body_lane_probes(n, 0); ++k)
    {
      // this pass's probes and nothing else: lanes beyond the body's last probe load zeros
      int const left = n - k * BODY_LANES;

      __amdgpu_buffer_rsrc_t const rprobes = make_rsrc(probes + (size_t)body_lane_probe(B.first, 0, k), (size_t)(left < BODY_LANES ? left : BODY_LANES) * sizeof(BodyProbe));

      float4 const raw = buf_load_f32x4_aux<0>(rprobes, lane * (int)sizeof(BodyProbe), 0);

      BodyProbe const probe = { raw.x, raw.y, raw.z, raw.w };

      BodyWorld const w = body_transform(B, probe);

      bool const have = k < body_lane_probes(n, lane);
      bool const probebad = body_probe_bad(w, probe.a);

      badprobe = badprobe || (have && probebad);

      if (have && !probebad)
        body_add(p, terms(w, probe.a));
    }

    return badprobe;
  }

  // The walk over a body's probes, stated once for the kernels that reduce per body (this file's, ocean_drag.hip's): wave `body` reads its
  // body (wave-uniform index: scalar loads) and asks `begin(body, B, bad)` for the per-probe terms -- a callable (w, a) -> BodyPartial;
  // begin may set `bad` for a reason of its own, and a bad body walks no probe.  Then the passes (body_walk), the ballot, the tree and
  // lane 0's store of the record or of eight NaNs
  template<class Begin>
  __device__ __forceinline__ void body_each_probe(datum_ocean_body const *bodies, BodyProbe const *probes, float4 *records, int nbodies, int nprobes, Begin &&begin)
  {
    int const lane = (int)threadIdx.x & (BODY_LANES - 1);
    int const body = __builtin_amdgcn_readfirstlane((int)blockIdx.x * BODY_WAVES + ((int)threadIdx.x >> 6));

    // (the whole wave: the last workgroup's waves without a body)
    if (body >= nbodies)
      return;

    datum_ocean_body const B = bodies[body];

    bool bad = body_range_bad(B, nprobes);

    auto const terms = begin(body, B, bad);

    int const n = bad ? 0 : B.count;

    BodyWave wave;
    wave.p = body_zero();

    bool const badprobe = body_walk(B, probes, n, lane, wave.p, terms);

    bad = bad || __builtin_amdgcn_ballot_w64(badprobe) != 0;

    body_tree(wave);

    if (lane == 0)
    {
      float const nan = __builtin_nanf("");

      float const *r = wave.p.f;

      __amdgpu_buffer_rsrc_t const rrecord = make_rsrc(records + 2 * (size_t)body, 2 * sizeof(float4));

      buf_store_f32x4_aux<0>(bad ? make_float4(nan, nan, nan, nan) : make_float4(r[0], r[1], r[2], r[3]), rrecord, 0, 0);
      buf_store_f32x4_aux<0>(bad ? make_float4(nan, nan, nan, nan) : make_float4(r[4], r[5], r[6], r[7]), rrecord, 16, 0);
    }
  }

  template<int LAYOUT>
  __global__ void __launch_bounds__(BODY_THREADS) ocean_body_kernel(BodyArgs a)
  {
    body_each_probe(a.bodies, a.probes, a.records, a.nbodies, a.nprobes, [&](int, datum_ocean_body const &B, bool &)
    {
      return [&a, &B](BodyWorld const &w, float weight)
      {
        float2 const q = make_float2(w.x, w.y);

        QueryRecord const r = query_record<LAYOUT>(a.q, query_solve<LAYOUT>(a.q, q), q);

        float const rec[DATUM_OCEAN_SURFACE_SAMPLE_FLOATS] = { r.v.x, r.v.y, r.v.z, r.v.w, r.m.x, r.m.y, r.m.z, r.m.w };

        return body_terms(B, w, weight, rec);
      };
    });
  }

  // a.q (but its frame), bodies, probes, records, nbodies (> 0) and nprobes filled in
  inline hipError_t launch_bodies(BodyArgs &a, hipStream_t stream)
  {
    query_frame(a.q);

    void *args[] = { &a };

    return hipLaunchKernel(layout_kernel(a.q.N, &ocean_body_kernel<GEN_PLAIN>, &ocean_body_kernel<GEN_BANDED>), dim3((unsigned)(((size_t)a.nbodies + BODY_WAVES - 1) / BODY_WAVES)), dim3(BODY_THREADS), args, 0, stream);
  }
}
