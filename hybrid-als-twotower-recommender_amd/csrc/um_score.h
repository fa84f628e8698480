// The four score sources of hrec_user_metrics (csrc/user_metrics.hip) and
// hrec_rank_positions (csrc/rank_positions.hip): one definition of the value a
// source gives for (row, column), so both entries rank and grade the same bits.
// include/hrec.h (HREC_UM_SRC_*) has the contract.
#pragma once

#include "hybrid_common.h"

namespace hrec {

// What a source reads: scores [n_rows][ld] (f64 or f32 by source), the
// two-tower matrix of the fused source, the per-column ALS fallback.
struct UmSource {
  const void* sa;
  const float* sb;
  int64_t ld;
  const double* fb;
};

// The score dtype of a source: the dense f32 matrix keeps np.float32 (the
// two-tower rule), every other source is f64.
template <int SRC>
struct UmScore {
  typedef double type;
};
template <>
struct UmScore<HREC_UM_SRC_F32> {
  typedef float type;
};

// The fused source's row state: hrec_hybrid_lists' coefficients from its out_minmax row, and the row's weights.
struct UmFuse {
  HpScale sc;
  double w0, w1;
};
__device__ __forceinline__ UmFuse um_fuse_row(const double* __restrict__ minmax, const int32_t* __restrict__ wins,
                                              int64_t row) {
  UmFuse f;
  const double* mm = minmax + 4 * row;
  f.sc = hp_scale64(mm[0], mm[1], (float)mm[2], (float)mm[3]);
  const bool w = wins[row] != 0;
  f.w0 = w ? 0.8 : 0.2;
  f.w1 = w ? 0.2 : 0.8;
  return f;
}

// The value of column c from the entries already loaded (a: scores, t: the
// two-tower entry of the fused source).
template <int SRC, typename A>
__device__ __forceinline__ typename UmScore<SRC>::type um_value(const UmSource& P, A a, float t, int64_t c,
                                                                const UmFuse& f) {
  if constexpr (SRC == HREC_UM_SRC_F64 || SRC == HREC_UM_SRC_F32) {
    return a;
  } else if constexpr (SRC == HREC_UM_SRC_ALS) {
    return hl_als(a, P.fb, c);
  } else {
    return hp_fuse64(f.sc, hl_als(a, P.fb, c), t, f.w0, f.w1);
  }
}

template <int SRC>
__device__ __forceinline__ typename UmScore<SRC>::type um_score(const UmSource& P, int64_t row, int64_t c,
                                                                const UmFuse& f) {
  const int64_t at = row * P.ld + c;
  if constexpr (SRC == HREC_UM_SRC_F64) {
    return static_cast<const double*>(P.sa)[at];
  } else if constexpr (SRC == HREC_UM_SRC_F32) {
    return static_cast<const float*>(P.sa)[at];
  } else if constexpr (SRC == HREC_UM_SRC_ALS) {
    return um_value<SRC>(P, static_cast<const float*>(P.sa)[at], 0.0f, c, f);
  } else {
    return um_value<SRC>(P, static_cast<const float*>(P.sa)[at], P.sb[at], c, f);
  }
}

}  // namespace hrec
