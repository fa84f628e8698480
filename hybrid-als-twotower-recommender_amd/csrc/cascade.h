// The sample-bound top-k cascade of hrec_als_score_topk[_pruned][_excluding]
// and hrec_dot_topk[_excluding]: score a sample -> a lower bound of the kk-th
// best -> score-and-filter every item against it -> drop the excluded
// survivors -> exact stable top-k of the rest. The scoring and filter launches
// are each driver's own; the steps between them are csrc/cascade.hip's.
#pragma once

#include "common.h"

namespace hrec {

// The buffers every cascade carves from its workspace.
struct CascadeWs {
  float* samp;  // [B][S] sample scores
  char* tws;    // sample top-k workspace
  float* sv;    // [B][kk] sample top-k values / indices
  int64_t* si;
  float* cv;    // [B][cap] candidates
  int64_t* ci;
  int* cn;      // [B] counters (+ cn_pad bytes)
  char* fws;    // final top-k workspace
};
CascadeWs cascade_carve(Carver& c, int B, int64_t S, int64_t cap, int kk, size_t cn_pad);

// The small-catalogue arm: the stable top-kk of the full rows w.samp[B][n_items]; under an exclusion the
// excluded scores become NaN first (ranked after every score that stays) and x.out_len is written.
int cascade_rank_all(const CascadeWs& w, int n_users, int64_t n_items, int kk, const Excl& x, int64_t* out_idx,
                     float* out_val, hipStream_t s);
// The filter's bound *thr / *thr_stride from the sample w.samp[B][S].
int cascade_bound(const CascadeWs& w, int n_users, int64_t S, int64_t step, int64_t n_excl, int kk, const Excl& x,
                  int32_t* out_len, bool lane_maxima, int* zero_cnt, const float** thr, int* thr_stride,
                  hipStream_t s);
// The tail: the excluded survivors leave (out_len optional); the exact stable top-kk of the lists (ties: item).
int cascade_tail(const CascadeWs& w, int n_users, int64_t cap, int kk, const Excl& x, int32_t* out_len,
                 int64_t* out_idx, float* out_val, hipStream_t s);

// One wave, m = this lane's maximum over its share of a row: the kk-th largest
// (kk <= 64) of the 64 lane maxima, the lowest lane holding the maximum
// retired each round (-inf when fewer than kk lanes hold a number).
__device__ __forceinline__ float kth_of_lane_maxima(float m, int kk, int lane) {
  float t = -__builtin_inff();
  for (int r = 0; r < kk; ++r) {
    float w = m;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) w = fmaxf(w, __shfl_xor(w, off, kWave));
    t = w;
    const uint64_t hold = __ballot(m == w);
    if (hold && lane == __builtin_ctzll(hold)) m = -__builtin_inff();
  }
  return t;
}

}  // namespace hrec
