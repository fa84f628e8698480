// What only the hybrid kernels share: the fusion arithmetic
// (src/hybrid_system.py:57-75: sklearn's MinMaxScaler per model, then the
// weighted sum), the sizes and keys of the hybrid lists (csrc/hybrid_lists.hip,
// csrc/hybrid_f1.hip) and the per-lane sorted lists of the pruned paths with
// their DPP best-of reduction. The ranking order and number formats are
// csrc/order.h's, the lane moves csrc/wave.h's.
#pragma once

#include <float.h>
#include <math.h>

#include "order.h"
#include "wave.h"

namespace hrec {

typedef hrec_f4 hp_f4;

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

// a_rj: the f32 score widened, or the column's fallback value where it is NaN
__device__ __forceinline__ double hl_als(float a, const double* __restrict__ fb, int64_t j) {
  return (a != a && fb) ? fb[j] : (double)a;
}

// slot_order_key of a live (non-excluded) column
__device__ __forceinline__ uint64_t hl_key(double v) { return slot_order_key(v, 0); }

__device__ __forceinline__ float hp_pick(const hp_f4& a, int r) {
  return r == 0 ? a[0] : (r == 1 ? a[1] : (r == 2 ? a[2] : a[3]));
}

// The wave's best (bv, bi) into every lane (empty slots: bi == INT64_MAX,
// worse than everything): the order as one integer key per entry, reduced
// by DPP within each 16-lane row (quad swaps, half-row and row mirrors:
// register moves, no LDS round trip) and across the 4 rows by readlanes.
__device__ __forceinline__ void hp_wave_best(double& bv, int64_t& bi) {
  uint64_t k = slot_order_key(bv, bi);
  int64_t i = bi;
  double v = bv;
  auto fold = [&](uint64_t ok, int64_t oi, double ov) {
    const bool tk = (ok > k) | ((ok == k) & (oi < i));
    k = tk ? ok : k;
    i = tk ? oi : i;
    v = tk ? ov : v;
  };
  fold(dpp64<0xB1>(k), dpp64<0xB1>(i), dpp64<0xB1>(v));     // quad_perm [1,0,3,2]
  fold(dpp64<0x4E>(k), dpp64<0x4E>(i), dpp64<0x4E>(v));     // quad_perm [2,3,0,1]
  fold(dpp64<0x141>(k), dpp64<0x141>(i), dpp64<0x141>(v));  // row_half_mirror
  fold(dpp64<0x140>(k), dpp64<0x140>(i), dpp64<0x140>(v));  // row_mirror
  uint64_t bk = lane_read(k, 0);
  int64_t bi2 = lane_read(i, 0);
  double bv2 = lane_read(v, 0);
#pragma unroll
  for (int r = 1; r < 4; ++r) {
    const uint64_t ok = lane_read(k, 16 * r);
    const int64_t oi = lane_read(i, 16 * r);
    const double ov = lane_read(v, 16 * r);
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
