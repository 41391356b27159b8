// Thin names for the gfx950 wave64 primitives the kernels use.  The only alternative
// definition of these names is the CPU sanitizer harness in tests/emu/hip_emu.h (-DGE_EMU),
// which exists because GPU sanitizers are not available; the shipped library is always built
// from the HIP definitions below.
#pragma once
#ifdef GE_EMU
#include "hip_emu.h"
#else
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GE_DEV static __device__ __forceinline__
#define GE_DEVFN __device__
#define GE_KERNEL __global__ void
#define GE_KERNEL_LB(threads, waves_per_simd) __global__ void __launch_bounds__(threads, waves_per_simd)
#define GE_HOSTDEV __host__ __device__ inline
#define GE_CONSTANT static __constant__ const

GE_DEV int ge_tid() { return (int)threadIdx.x; }
// The same value behind an opaque move.  Read at the top of the per-slot body of a persistent (slot-loop) kernel, it keeps the
// compiler from hoisting everything it derives from the thread id -- lane masks, shuffle sources, LDS addresses -- out of the slot
// loop, where those values stay live across the whole body and are spilled to scratch (ge_k_reset: 78 spilled VGPRs without it).
GE_DEV int ge_tid_fresh() { int t = (int)threadIdx.x; asm volatile("" : "+v"(t)); return t; }
GE_DEV int ge_bid() { return (int)blockIdx.x; }
GE_DEV int ge_bdim() { return (int)blockDim.x; }
GE_DEV int ge_gdim() { return (int)gridDim.x; }
GE_DEV unsigned char *ge_dyn_smem() {
  extern __shared__ __align__(16) unsigned char ge_smem_raw[];
  return ge_smem_raw;
}
GE_DEV void ge_sync() { __syncthreads(); }
// issue priority of this wave among the waves of its SIMD (s_setprio, 0 = default .. 3; the instruction takes an immediate).  The
// arbitration is between ALL waves resident on the SIMD, whichever kernel and stream they belong to: see GE_PRIO_* below
GE_DEV void ge_wave_priority(int p) {
  switch (p) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}
// LDS hand-off between lanes of ONE wave (the other waves of the workgroup do not take part)
GE_DEV void ge_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); }
// Ordering point between the four lanes of a quad that execute identical control flow: LDS operations of one wave
// are performed in issue order, so only the compiler has to be kept from moving accesses across this point.
GE_DEV void ge_quad_sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
// value of the lane (lane ^ 1) / (lane ^ 2) inside the quad: one DPP move (quad_perm), no LDS
GE_DEV uint32_t ge_quad_xor1(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true); }
GE_DEV uint32_t ge_quad_xor2(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true); }
// the 16-bit values of the four lanes of a quad as one 64-bit word (lane k of the quad in bits [16k, 16k+16)): four quad_perm broadcasts
GE_DEV uint64_t ge_quad_gather16(uint32_t v) {
  const uint32_t b0 = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x00, 0xf, 0xf, true), b1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x55, 0xf, 0xf, true);
  const uint32_t b2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xAA, 0xf, 0xf, true), b3 = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xFF, 0xf, 0xf, true);
  return (uint64_t)((b0 & 0xffffu) | (b1 << 16)) | ((uint64_t)((b2 & 0xffffu) | (b3 << 16)) << 32);
}
// OR over the eight lanes of an octet (lanes 8k .. 8k+7 of the wave), the result in every one of them: two quad_perm exchanges and a
// row_half_mirror (lane i of the eight <-> lane 7 - i), three DPP moves, no LDS.  Every lane of the octet must execute it.
GE_DEV uint32_t ge_oct_or32(uint32_t v) {
  v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);
  v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true);
  v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, true);
  return v;
}
// fire-and-forget LDS adds (ds_add_u32 / ds_add_f64, no return value, nothing to wait for)
GE_DEV void ge_lds_add_u32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
GE_DEV void ge_lds_add_f64(double *p, double v) { unsafeAtomicAdd(p, v); }
// every outstanding load has returned (s_waitcnt vmcnt(0)): placed where that is already true, in front of a block of
// stores, it keeps the compiler's conservative per-register waits at control-flow joins from landing between the
// stores, where they would wait for store acknowledgements
GE_DEV void ge_wait_loads() { __builtin_amdgcn_s_waitcnt(0x0F70); }
GE_DEV uint64_t ge_ballot(bool p) { return (uint64_t)__ballot(p ? 1 : 0); }
GE_DEV int ge_shfl_i32(int v, int src) { return __shfl(v, src, 64); }
GE_DEV uint32_t ge_shfl_u32(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src, 64); }
GE_DEV uint64_t ge_shfl_u64(uint64_t v, int src) {
  int lo = __shfl((int)(uint32_t)v, src, 64), hi = __shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
GE_DEV double ge_shfl_f64(double v, int src) { return __longlong_as_double((long long)ge_shfl_u64((uint64_t)__double_as_longlong(v), src)); }
// value of lane `idx` where idx is wave-uniform: v_readlane_b32, no LDS
GE_DEV uint32_t ge_readlane_u32(uint32_t v, int idx) { return (uint32_t)__builtin_amdgcn_readlane((int)v, idx); }
// v with lane `idx` replaced by `val` (idx and val wave-uniform): a compare against the lane id and a select (v_writelane_b32
// would need the lane index in M0 beside the scalar value: one constant-bus operand only)
GE_DEV uint32_t ge_writelane_u32(uint32_t v, uint32_t val, int idx) { return ((int)(threadIdx.x & 63u) == idx) ? val : v; }
// value known to be the same in every lane: keep it (and what is computed from it) on the scalar unit
GE_DEV uint32_t ge_uniform_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
GE_DEV double ge_u64_as_f64(uint64_t v) { return __longlong_as_double((long long)v); }
GE_DEV uint64_t ge_f64_as_u64(double v) { return (uint64_t)__double_as_longlong(v); }
GE_DEV int ge_popc64(uint64_t v) { return __popcll(v); }
// set bits of the (wave-uniform) mask below this lane: v_mbcnt_lo / v_mbcnt_hi, no lane mask to build
GE_DEV int ge_mbcnt(uint64_t m) { return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
GE_DEV int ge_ctz64(uint64_t v) { return v ? (int)__builtin_ctzll(v) : 64; }
GE_DEV int ge_clz32(uint32_t v) { return v ? (int)__builtin_clz(v) : 32; }

#define GE_LAUNCH(kernel, grid, block, smem, stream, ...) \
  hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3((unsigned)(block)), (size_t)(smem), (hipStream_t)(stream), __VA_ARGS__)
#define GE_SET_MAX_DYN_LDS(kernel, bytes) \
  hipFuncSetAttribute((const void *)(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))
#endif

// 16-bit floating-point storage (both builds): the words of a bfloat16 / float16 tensor, converted at the load and at the store.
// Up: exact.  Down: round to nearest even for every finite value; NaN stays NaN (which one is not defined).  The HIP build uses the
// hardware conversions (v_cvt_f32_f16 / v_cvt_f16_f32, v_cvt_pk_bf16_f32; bfloat16 up is a shift); the CPU harness's compiler has
// neither _Float16 nor __bf16 and converts on the bits -- the same values (tests/test_policy_dtype.py walks all 65 536 patterns of
// both types and a million float32 values against torch).
struct ge_bf16 { uint16_t u; };
struct ge_f16 { uint16_t u; };
GE_DEV float ge_bits_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
GE_DEV uint32_t ge_f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
GE_DEV float ge_to_f32(ge_bf16 h) { return ge_bits_f32((uint32_t)h.u << 16); }
#ifdef GE_EMU
GE_DEV ge_bf16 ge_from_f32(float f, ge_bf16) {
  uint32_t u = ge_f32_bits(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return ge_bf16{(uint16_t)((u >> 16) | 0x40u)};
  u += 0x7fffu + ((u >> 16) & 1u);  // (half of the dropped 16 bits, a tie towards the even word; a carry runs on into the exponent)
  return ge_bf16{(uint16_t)(u >> 16)};
}
GE_DEV float ge_to_f32(ge_f16 h) {
  const uint32_t s = (uint32_t)(h.u & 0x8000u) << 16, e = (h.u >> 10) & 31u, m = h.u & 0x3ffu;
  if (e == 31u) return ge_bits_f32(s | 0x7f800000u | (m << 13));
  if (e != 0u) return ge_bits_f32(s | ((e + 112u) << 23) | (m << 13));
  return ge_bits_f32(s | ge_f32_bits((float)m * 0x1p-24f));  // subnormal (and zero): m quanta of 2^-24
}
GE_DEV ge_f16 ge_from_f32(float f, ge_f16) {
  const uint32_t u = ge_f32_bits(f), a = u & 0x7fffffffu;
  const uint16_t s = (uint16_t)((u >> 16) & 0x8000u);
  if (a > 0x7f800000u) return ge_f16{(uint16_t)(s | 0x7e00u)};
  if (a >= 0x38800000u) {  // 2^-14 and above: a float16 normal, or past its range
    uint32_t r = a - 0x38000000u;  // exponent rebias 127 -> 15
    r += 0xfffu + ((r >> 13) & 1u);  // (half of the dropped 13 bits, a tie towards the even word; a carry runs on into the exponent)
    r >>= 13;
    return ge_f16{(uint16_t)(s | (r >= 0x7c00u ? 0x7c00u : r))};
  }
  // below 2^-14: a count of 2^-24 quanta.  0.5f + |f| has exactly that quantum, so the float32 add does the rounding to nearest even
  return ge_f16{(uint16_t)(s | (ge_f32_bits(ge_bits_f32(a) + 0.5f) - 0x3f000000u))};
}
#else
GE_DEV ge_bf16 ge_from_f32(float f, ge_bf16) { const __bf16 b = (__bf16)f; ge_bf16 h; __builtin_memcpy(&h.u, &b, 2); return h; }
// (the float32 value passes through an opaque move on either side of the float16 conversion: without it the compiler folds a float32
// multiply next to the conversion into one v_fma_mix* instruction -- fma(a, b, 0) converted -- whose words differed from multiply-
// then-convert on the MI355X in 3 gradient elements of 1 500; with it the multiply and v_cvt_f16_f32 / v_cvt_f32_f16 stay apart)
GE_DEV float ge_to_f32(ge_f16 h) { _Float16 v; __builtin_memcpy(&v, &h.u, 2); float f = (float)v; asm("" : "+v"(f)); return f; }
GE_DEV ge_f16 ge_from_f32(float f, ge_f16) { asm("" : "+v"(f)); const _Float16 v = (_Float16)f; ge_f16 h; __builtin_memcpy(&h.u, &v, 2); return h; }
#endif
GE_DEV float ge_to_f32(float f) { return f; }
GE_DEV float ge_from_f32(float f, float) { return f; }
// v * s, s the same in every lane, as ONE v_mul_f32 whose result replaces v in its register (round to nearest even like the `*` it
// stands for, and never contracted with a neighbour).  For a multiply applied to many loaded values at once -- a row held in
// registers: the compiler otherwise keeps loaded values and products apart and the kernel's register count rises with the row
#ifdef GE_EMU
GE_DEV float ge_mul_f32_inplace(float v, float s) { return v * s; }
#else
GE_DEV float ge_mul_f32_inplace(float v, float s) { asm("v_mul_f32 %0, %1, %0" : "+v"(v) : "s"(s)); return v; }
#endif

// Issue priority by role (ge_wave_priority; both builds see these, the CPU harness ignores them).  A shard's step runs at the
// latency of its own launch chain, beside the other shards' kernels on the same SIMDs: a kernel that is a handful of waves doing
// dependent round trips outranks the feature kernels, which are the throughput tenants and fill the issue slots the others leave.
// Only the assignments that were measured beside other engines carry a level: the n <= 64 step kernel and the probe of the generic
// feature kernel's LIST launch.  ge_k_step, ge_k_step_edge, ge_k_swap and ge_k_feat_combine stay at 0 until the configs that launch
// them are measured.  The graph kernel's regenerating waves stay at 0 (retrying ones at 1): raised as a whole it gains nothing, and
// raised above its own seeding workgroups it starves them and the launch ends later (profiles/README.md round 5);
// the seeding workgroups ALONE are raised (round 8).
#ifndef GE_PRIO_SEED
#define GE_PRIO_SEED 1   // the seeding workgroups of the queue-mode graph launch (ge_k_reset): two waves per 64 queued slots running a chain of
                         // 1 869 dependent steps, the LAST waves of the launch to finish (without them the launch is 57 us instead of 74 beside
                         // two other shards, profiles/README.md round 8) -- a handful of waves on the whole chip, so raising them costs nobody
#endif
#ifndef GE_PRIO_SEED2
#define GE_PRIO_SEED2 GE_PRIO_SEED  // the pass-2 workgroups at the head of ge_k_features64's queue launch (split seeding, GE_SEED_SPLIT)
#endif
#define GE_PRIO_STEP 3   // ge_k_step_path64: every wave, from entry to exit
#define GE_PRIO_PROBE 3  // a LIST-mode launch of ge_k_features until it has read work_count; with work to do it drops to 0
