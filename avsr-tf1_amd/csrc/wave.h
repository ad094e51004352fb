// Wave-level device helpers of the step-loop kernels, one copy of each: DPP reductions, LDS-only barrier, log-add, fast gates.  Needs common.h alone.
#pragma once
#include <math.h>
#include "common.h"

namespace avsr {

// DPP reductions: __shfl_xor lowers to ds_bpermute (an LDS round trip per step); inside a row of 16 lanes the data-parallel primitives
// rotate for one VALU issue.  row16_*: every lane of the row gets the row's result.
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) { return __builtin_bit_cast(float, dpp_i<CTRL>(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ float rdlane_f(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0x128>(v);      // row_ror:8
  v += dpp_f<0x124>(v);      // row_ror:4
  v += dpp_f<0x122>(v);      // row_ror:2
  v += dpp_f<0x121>(v);      // row_ror:1
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_f<0x128>(v));
  v = fmaxf(v, dpp_f<0x124>(v));
  v = fmaxf(v, dpp_f<0x122>(v));
  v = fmaxf(v, dpp_f<0x121>(v));
  return v;
}
// Whole-wave results (uniform, deterministic): the four row results combined in a fixed order, (0 + 16) + (32 + 48).  NOT the order of
// common.h's wave_sum (an xor butterfly): swapping the two changes bits, so every user keeps the one it has.
__device__ __forceinline__ float wave64_sum(float v) {
  v = row16_sum(v);
  return (rdlane_f(v, 0) + rdlane_f(v, 16)) + (rdlane_f(v, 32) + rdlane_f(v, 48));
}
__device__ __forceinline__ float wave64_max(float v) {
  v = row16_max(v);
  return fmaxf(fmaxf(rdlane_f(v, 0), rdlane_f(v, 16)), fmaxf(rdlane_f(v, 32), rdlane_f(v, 48)));
}
__device__ __forceinline__ int wave64_min_i(int v) {
  v = min(v, dpp_i<0x128>(v));
  v = min(v, dpp_i<0x124>(v));
  v = min(v, dpp_i<0x122>(v));
  v = min(v, dpp_i<0x121>(v));
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// Workgroup barrier that does NOT drain the vector-memory queue: LDS ordering and arrival only.  __syncthreads() carries a
// workgroup-scope fence, which the compiler lowers to s_waitcnt vmcnt(0) before s_barrier: every operand prefetched for the NEXT step of
// a step loop, and the stores of this one, would be waited for on the critical path of THIS step (measured in ctc.hip: 1.37 ms for the
// launch at B = 64, T = 500 with __syncthreads() at the per-step barrier).  For barriers whose cross-thread traffic is LDS only; a global
// hand-over across one is safe only where a thread has consumed (so received) its loads before it arrives (ctc.hip: row t of dz is read
// as log-probabilities before the step's barrier, overwritten with the gradient after it).  Stores are drained explicitly where published.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// a (+) b in the log domain; (-inf) (+) (-inf) = -inf, never NaN
__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(1.f + expf(-fabsf(a - b)));
}

// fast gates, v_exp_f32 / v_rcp_f32 based: |err| ~1e-7 absolute, far inside the 1e-4 parity budget
__device__ __forceinline__ float p_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float p_tanh(float x) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)) - 1.0f; }

}  // namespace avsr
