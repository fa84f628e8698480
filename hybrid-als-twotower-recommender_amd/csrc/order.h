// The number-format and ordering rules that every ranking kernel shares, each
// with its one definition: the bf16 rounding (hrec_f32_to_bf16), the directed
// f64 -> f32 roundings of the pruning bounds, the top-k order (sorted(...,
// reverse=True) over the reference's candidate order, src/hybrid_system.py:108)
// and that order as unsigned integer keys.
#pragma once

#include <math.h>

#include "common.h"

namespace hrec {

// f32 -> bf16 bits, round to nearest even (NaN stays NaN): hrec_f32_to_bf16.
__device__ __forceinline__ uint32_t bf16_rne(float v) {
  const uint32_t x = __float_as_uint(v);
  if ((x & 0x7fffffffu) > 0x7f800000u) return (x >> 16) | 0x40u;
  return (x + 0x7fffu + ((x >> 16) & 1u)) >> 16;
}

// The smallest float >= x and the largest float <= x.
__device__ __forceinline__ float f32_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = nextafterf(f, INFINITY);
  return f;
}
__device__ __forceinline__ float f32_down(double x) {
  float f = (float)x;
  if ((double)f > x) f = nextafterf(f, -INFINITY);
  return f;
}

// Order of every top-k: larger value first; equal values -> smaller index
// first (a stable descending sort of the input order). NaN sorts last.
template <typename T>
__device__ __forceinline__ bool better(T va, int64_t ia, T vb, int64_t ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return !na && nb ? true : (na && nb ? ia < ib : false);
  return va > vb || (va == vb && ia < ib);
}

template <typename T>
struct KV {
  T v;
  int64_t i;
};

// The wave's best (value, index) by better(), in every lane: the xor tree
// over both fields (three cross-lane moves or more and a compare per round).
template <typename T>
__device__ __forceinline__ KV<T> wave_best(KV<T> x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    KV<T> y;
    y.v = __shfl_xor(x.v, off, kWave);
    y.i = __shfl_xor(x.i, off, kWave);
    // lanes without a candidate carry i = INT64_MAX and lose every comparison
    const bool take = (x.i == INT64_MAX) ? (y.i != INT64_MAX)
                                         : (y.i != INT64_MAX && better(y.v, y.i, x.v, x.i));
    if (take) x = y;
  }
  return x;
}

// better()'s value order as one unsigned key (larger = better, equal values
// share a key): 0 = NaN, numbers above by their ordered bits.
__device__ __forceinline__ uint64_t order_key(double v) {
  if (v != v) return 0;  // NaN ranks below every number
  const uint64_t b = (uint64_t)__double_as_longlong(v + 0.0);  // -0 -> +0 (they compare equal)
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(uint64_t k) {
  if (k == 0) return __builtin_nan("");
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
// order_key for an f32 value, in 32 bits.
__device__ __forceinline__ uint32_t order_key32(float v) {
  if (v != v) return 0;
  const uint32_t b = __float_as_uint(v + 0.0f);  // -0 -> +0
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
// order_key with a key below NaN's for an empty slot (idx INT64_MAX): 0 =
// empty, 1 = NaN, numbers by order_key (ties -> the smaller item).
__device__ __forceinline__ uint64_t slot_order_key(double v, int64_t idx) {
  const uint64_t ord = order_key(v);
  return idx == INT64_MAX ? 0ull : (v != v ? 1ull : ord);
}

}  // namespace hrec
