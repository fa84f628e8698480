// What the fused ALS top-k (csrc/score.hip) and the pruned one (csrc/als_prune.hip) share. A variant build
// that overrides HREC_SCORE_SAMPLE rebuilds both sources (scripts/build_variant_obj.sh).
#pragma once

#include "common.h"

namespace hrec {

constexpr int kScoreKMax = 256;  // widest factor row (rank 256)
#ifndef HREC_SCORE_SAMPLE
#define HREC_SCORE_SAMPLE 2048
#endif
constexpr int kSample = HREC_SCORE_SAMPLE;  // items scored for the survivor bound
constexpr int kCap = 4096;                  // candidates per user

// kk of a call: min(top_k, n_items), within the selection kernels' [1, 1024]
inline int score_kk(int64_t n_items, int top_k) {
  const int64_t kk = top_k < n_items ? top_k : n_items;
  return (int)(kk < 1 ? 1 : (kk > 1024 ? 1024 : kk));
}

// csrc/score.hip: hrec_als_score_topk[_excluding] (x.on), also the pruned
// path's small-catalogue arm.
int score_topk_run(const char* fn, const float* user_factors, const int64_t* user_rows, int n_users,
                   const float* item_factors_t, int64_t ld_items, int64_t n_items, int k, int kp, int top_k,
                   int64_t* out_idx, float* out_val, int* overflow, void* workspace, size_t workspace_bytes,
                   const Excl& x, void* stream);

}  // namespace hrec
