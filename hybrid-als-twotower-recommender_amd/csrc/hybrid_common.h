// Device helpers shared by the scoring, top-k and fusion kernels: the bf16
// rounding (hrec_f32_to_bf16), the top-k order (sorted(..., reverse=True) over
// the reference's candidate order, src/hybrid_system.py:108), the fusion
// arithmetic (src/hybrid_system.py:57-75) and 64-bit lane moves. Each rule
// has its one definition here.
#pragma once

#include <float.h>
#include <math.h>

#include "common.h"

namespace hrec {

typedef hrec_f4 hp_f4;

// f32 -> bf16 bits, round to nearest even (NaN stays NaN): hrec_f32_to_bf16.
__device__ __forceinline__ uint32_t bf16_rne(float v) {
  const uint32_t x = __float_as_uint(v);
  if ((x & 0x7fffffffu) > 0x7f800000u) return (x >> 16) | 0x40u;
  return (x + 0x7fffu + ((x >> 16) & 1u)) >> 16;
}

// sklearn MinMaxScaler's range (container sklearn _data.py:518-522, 261-262):
// a range below 10 eps of its dtype scales by 1.
__device__ __forceinline__ double mm_range(double r) { return r < 10.0 * DBL_EPSILON ? 1.0 : r; }
__device__ __forceinline__ float mm_range(float r) { return r < 10.0f * FLT_EPSILON ? 1.0f : r; }

// The scaler coefficients of the batched fusion (MinMaxScaler.fit_transform:
// scale = 1 / range, min_ = 0 - min * scale; ALS in f64 as the reference's
// als scores are Python floats, two-tower in f32 as np.float32 scores).
struct HpScale {
  double ascale, amin_;
  float tscale, tmin_;
};
__device__ __forceinline__ HpScale hp_scale(float amin, float amax, float tmin, float tmax) {
#pragma clang fp contract(off)
  HpScale s;
  s.ascale = 1.0 / mm_range((double)amax - (double)amin);
  s.amin_ = 0.0 - (double)amin * s.ascale;
  s.tscale = 1.0f / mm_range(tmax - tmin);
  s.tmin_ = 0.0f - tmin * s.tscale;
  return s;
}
// fused = w0 * als_norm + w1 * (double)tt_norm (y = x * scale + min_, two
// roundings each in the input dtype; numpy 1.21 scalar promotion widens the
// f32 tt_norm before the multiply). Non-decreasing in a and in t (positive
// scales and weights, rounding is monotone): the fused score of an upper
// bound of (a, t) bounds the item's.
__device__ __forceinline__ double hp_fuse(const HpScale& s, float a, float t, double w0, double w1) {
#pragma clang fp contract(off)
  const double an = (double)a * s.ascale + s.amin_;
  const float tn = t * s.tscale + s.tmin_;
  return w0 * an + w1 * (double)tn;
}

// The same with genuine f64 ALS extremes and scores (hrec_hybrid_lists: the
// cold-start fallback vector is f64): hrec_fuse_topk's coefficients, and
// hp_scale's bit for bit when amin / amax are widened f32 values.
__device__ __forceinline__ HpScale hp_scale64(double amin, double amax, float tmin, float tmax) {
#pragma clang fp contract(off)
  HpScale s;
  s.ascale = 1.0 / mm_range(amax - amin);
  s.amin_ = 0.0 - amin * s.ascale;
  s.tscale = 1.0f / mm_range(tmax - tmin);
  s.tmin_ = 0.0f - tmin * s.tscale;
  return s;
}
__device__ __forceinline__ double hp_fuse64(const HpScale& s, double a, float t, double w0, double w1) {
#pragma clang fp contract(off)
  const double an = a * s.ascale + s.amin_;
  const float tn = t * s.tscale + s.tmin_;
  return w0 * an + w1 * (double)tn;
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
// The same with a key below NaN's for an empty slot (idx INT64_MAX): 0 =
// empty, 1 = NaN, numbers by order_key (ties -> the smaller item).
__device__ __forceinline__ uint64_t hp_order_key(double v, int64_t idx) {
  const uint64_t ord = order_key(v);
  return idx == INT64_MAX ? 0ull : (v != v ? 1ull : ord);
}

// What hrec_hybrid_lists (csrc/hybrid_lists.hip) and hrec_hybrid_model_f1
// (csrc/hybrid_f1.hip) share: the sample / list sizes, the segment a wave
// covers, the substituted ALS score and the key of a live column.
constexpr int kHlSample = HREC_HYBRID_LISTS_SAMPLE;  // HYBRID_LISTS_SAMPLE of src/_hrec.py
constexpr int kHlCap = HREC_HYBRID_LISTS_CAP;        // >= kHlSample: n <= kHlSample never overflows
constexpr int kHlPer = 16;       // columns per lane per segment
constexpr int kHlSeg = 64 * kHlPer;
constexpr int kHlBoundBlock = 256;
constexpr int kHlBoundPer = kHlSample / kHlBoundBlock;
static_assert(kHlCap >= kHlSample && kHlCap >= kTopkSelectMax, "a list holds the sample and any top_k");

__device__ __forceinline__ void hl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a_rj: the f32 score widened, or the column's fallback value where it is NaN
__device__ __forceinline__ double hl_als(float a, const double* __restrict__ fb, int64_t j) {
  return (a != a && fb) ? fb[j] : (double)a;
}

// hp_order_key of a live (non-excluded) column
__device__ __forceinline__ uint64_t hl_key(double v) { return hp_order_key(v, 0); }

// 64-bit moves across lanes: DPP (CTRL: gfx9 dpp_ctrl, all sources valid)
// and readlane, as two 32-bit halves.
template <int CTRL, typename T>
__device__ __forceinline__ T hp_dpp64(T x) {
  static_assert(sizeof(T) == 8, "64-bit values");
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  u = ((uint64_t)hi << 32) | lo;
  T r;
  __builtin_memcpy(&r, &u, 8);
  return r;
}
template <int CTRL>
__device__ __forceinline__ float hp_dpp32(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
// lane ^ 16 / lane ^ 32 by v_permlane16_swap / v_permlane32_swap (see
// csrc/hybrid_scores.hip hs_xor16)
__device__ __forceinline__ float hp_xor16(float x) {
  const uint32_t u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __uint_as_float((threadIdx.x & 16) ? r[0] : r[1]);
}
__device__ __forceinline__ float hp_xor32(float x) {
  const uint32_t u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float((threadIdx.x & 32) ? r[0] : r[1]);
}
template <typename T>
__device__ __forceinline__ T hp_readlane64(T x, int src) {
  static_assert(sizeof(T) == 8, "64-bit values");
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
  u = ((uint64_t)hi << 32) | lo;
  T r;
  __builtin_memcpy(&r, &u, 8);
  return r;
}

__device__ __forceinline__ float hp_pick(const hp_f4& a, int r) {
  return r == 0 ? a[0] : (r == 1 ? a[1] : (r == 2 ? a[2] : a[3]));
}

// The wave's best (bv, bi) into every lane (empty slots: bi == INT64_MAX,
// worse than everything): the order as one integer key per entry, reduced
// by DPP within each 16-lane row (quad swaps, half-row and row mirrors:
// register moves, no LDS round trip) and across the 4 rows by readlanes.
__device__ __forceinline__ void hp_wave_best(double& bv, int64_t& bi) {
  uint64_t k = hp_order_key(bv, bi);
  int64_t i = bi;
  double v = bv;
  auto fold = [&](uint64_t ok, int64_t oi, double ov) {
    const bool tk = (ok > k) | ((ok == k) & (oi < i));
    k = tk ? ok : k;
    i = tk ? oi : i;
    v = tk ? ov : v;
  };
  fold(hp_dpp64<0xB1>(k), hp_dpp64<0xB1>(i), hp_dpp64<0xB1>(v));     // quad_perm [1,0,3,2]
  fold(hp_dpp64<0x4E>(k), hp_dpp64<0x4E>(i), hp_dpp64<0x4E>(v));     // quad_perm [2,3,0,1]
  fold(hp_dpp64<0x141>(k), hp_dpp64<0x141>(i), hp_dpp64<0x141>(v));  // row_half_mirror
  fold(hp_dpp64<0x140>(k), hp_dpp64<0x140>(i), hp_dpp64<0x140>(v));  // row_mirror
  uint64_t bk = hp_readlane64(k, 0);
  int64_t bi2 = hp_readlane64(i, 0);
  double bv2 = hp_readlane64(v, 0);
#pragma unroll
  for (int r = 1; r < 4; ++r) {
    const uint64_t ok = hp_readlane64(k, 16 * r);
    const int64_t oi = hp_readlane64(i, 16 * r);
    const double ov = hp_readlane64(v, 16 * r);
    const bool tk = (ok > bk) | ((ok == bk) & (oi < bi2));
    bk = tk ? ok : bk;
    bi2 = tk ? oi : bi2;
    bv2 = tk ? ov : bv2;
  }
  bv = bv2;
  bi = bi2;
}

// A lane's sorted best KK (value, item) entries (empty: INT64_MAX).
template <int KK>
struct HpList {
  double v[KK];
  int64_t i[KK];
  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int j = 0; j < KK; ++j) {
      v[j] = 0.0;
      i[j] = INT64_MAX;
    }
  }
  __device__ __forceinline__ void insert(double xv, int64_t xi) {
#pragma unroll
    for (int j = 0; j < KK; ++j) {  // compare-exchange chain (sorted list)
      const bool sw = i[j] == INT64_MAX || better(xv, xi, v[j], i[j]);
      const double tv = v[j];
      const int64_t ti = i[j];
      v[j] = sw ? xv : tv;
      i[j] = sw ? xi : ti;
      xv = sw ? tv : xv;
      xi = sw ? ti : xi;
    }
  }
  // the wave's kk best entries, rank r into (rv[r], ri[r]) of lane 0; the
  // lanes' lists lose them (called wave-uniformly)
  __device__ __forceinline__ void wave_top(int kk, int lane, double* rv, int64_t* ri) {
    for (int r = 0; r < kk; ++r) {
      double bv = v[0];
      int64_t bi = i[0];
      hp_wave_best(bv, bi);
      if (lane == 0) {
        rv[r] = bv;
        ri[r] = bi;
      }
      if (bi != INT64_MAX && i[0] == bi) {  // the (unique) owner pops its head
#pragma unroll
        for (int j = 0; j + 1 < KK; ++j) {
          v[j] = v[j + 1];
          i[j] = i[j + 1];
        }
        i[KK - 1] = INT64_MAX;
      }
    }
  }
};

}  // namespace hrec
