// The wave-level (64-lane) device primitives, each defined once: LDS ordering
// inside a wave, lane reads, DPP and permlane moves, and the reductions of
// one scalar per lane. A merge of two spellings into one stays only while the
// gfx950 device code of every source is unchanged (scripts/device_asm_digest.py);
// where it is not, both forms are kept here and say so.
#pragma once

#include <math.h>

#include "common.h"

namespace hrec {

// The lanes below this one that are set in a __ballot mask: a lane's rank
// among the lanes that voted yes (two v_mbcnt).
__device__ __forceinline__ int lanes_below(uint64_t mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// A condition that is the same in every lane, as a scalar (one
// v_readfirstlane): the branch on it is a scalar branch.
__device__ __forceinline__ bool uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

// Orders this wave's LDS accesses around a point, for LDS that one wave owns
// (a wave's LDS operations complete in issue order): compiler fences only,
// no instruction and no s_barrier.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lane `src`'s (wave-uniform) 32- or 64-bit value in every lane: one
// v_readlane_b32 per 32 bits, the result is scalar.
template <typename T>
__device__ __forceinline__ T lane_read(T x, int src) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- or 64-bit values");
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src));
  } else {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
    return __builtin_bit_cast(T, ((uint64_t)hi << 32) | lo);
  }
}

// A 32- / 64-bit value moved across lanes by one DPP pattern (CTRL: gfx9
// dpp_ctrl, every source lane valid): one v_mov_b32_dpp per 32 bits, which
// the compiler may fold into the instruction that uses it.
template <int CTRL, typename T>
__device__ __forceinline__ T dpp32(T x) {
  static_assert(sizeof(T) == 4, "32-bit values");
  return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
template <int CTRL, typename T>
__device__ __forceinline__ T dpp64(T x) {
  static_assert(sizeof(T) == 8, "64-bit values");
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(T, ((uint64_t)hi << 32) | lo);
}

// x of lane (l & 48) | ((l + 16 - N) & 15): a rotation inside each 16-lane
// row (DPP row_ror:N on both halves of the double, two v_mov_b32_dpp). Kept
// apart from dpp64<0x120 + N>: the mov_dpp builtin has no `old` operand, and
// writing it as update_dpp(0, ...) changes the ALS half-sweep's generated
// code (csrc/als_nonneg.hip).
template <int N>
__device__ __forceinline__ double row_ror(double x) {
  const long long v = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_mov_dpp((int)v, 0x120 + N, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(v >> 32), 0x120 + N, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// The 32-bit value of lane ^ 16 / lane ^ 32 by the gfx950 row / half swaps
// (v_permlane16_swap / v_permlane32_swap: one VALU instruction and a select,
// no LDS round trip): with the same register as both operands, the swap
// leaves the partner's value in the first result for lanes with that bit set
// and in the second for the others.
template <typename T>
__device__ __forceinline__ T xor16(T x) {
  static_assert(sizeof(T) == 4, "32-bit values");
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __builtin_bit_cast(T, (uint32_t)((threadIdx.x & 16) ? r[0] : r[1]));
}
template <typename T>
__device__ __forceinline__ T xor32(T x) {
  static_assert(sizeof(T) == 4, "32-bit values");
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(T, (uint32_t)((threadIdx.x & 32) ? r[0] : r[1]));
}
// v_permlane32_swap of two registers (one VALU instruction): a's upper lane
// half trades places with b's lower half, so lanes < 32 get (a[l], a[l + 32])
// and lanes >= 32 get (b[l - 32], b[l]), as two raw 32-bit words.
typedef uint32_t lane_u2 __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ lane_u2 half_swap(T a, T b) {
  static_assert(sizeof(T) == 4, "32-bit values");
  return __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), false,
                                          false);
}

// min / max of two scalars as the reductions below take them: fmin / fmax
// for floating point (a NaN loses to a number), a compare for integers.
__device__ __forceinline__ double lane_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float lane_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double lane_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float lane_max(float a, float b) { return fmaxf(a, b); }
template <typename T>
__device__ __forceinline__ T lane_min(T a, T b) {
  return b < a ? b : a;
}
template <typename T>
__device__ __forceinline__ T lane_max(T a, T b) {
  return b > a ? b : a;
}

// The xor-tree reductions of one scalar per lane, the result in every lane:
// six rounds (lane ^ 32, 16, ... 1) of one cross-lane move per 32 bits and
// one operation. The sum's order is this tree's: lane l first adds lane
// l ^ 32.
template <typename T>
__device__ __forceinline__ T wave_xor_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_xor_min(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = lane_min(v, __shfl_xor(v, off, kWave));
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_xor_max(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = lane_max(v, __shfl_xor(v, off, kWave));
  return v;
}

// Sum / min of a double over the wave by another tree, so another summation
// order than wave_xor_sum's: four row_ror rounds inside each 16-lane row (8
// v_mov_b32_dpp), then the four row results by lane_read, added as
// (r0 + r1) + (r2 + r3). The NNLS solver's order (csrc/als_nonneg.hip).
__device__ __forceinline__ double wave_row_sum(double v) {
  v += row_ror<8>(v);
  v += row_ror<4>(v);
  v += row_ror<2>(v);
  v += row_ror<1>(v);
  return (lane_read(v, 0) + lane_read(v, 16)) + (lane_read(v, 32) + lane_read(v, 48));
}
__device__ __forceinline__ double wave_row_min(double v) {
  v = fmin(v, row_ror<8>(v));
  v = fmin(v, row_ror<4>(v));
  v = fmin(v, row_ror<2>(v));
  v = fmin(v, row_ror<1>(v));
  return fmin(fmin(lane_read(v, 0), lane_read(v, 16)), fmin(lane_read(v, 32), lane_read(v, 48)));
}

}  // namespace hrec
