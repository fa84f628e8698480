// The exclusion (seen items) CSR of the *_excluding entry points, as device
// inlines: the one place under csrc/ that spells the convention out
// (include/hrec.h states it for callers under hrec_mask_rows_f32).
//   - The set of row i is cols[indptr[r] .. indptr[r + 1]) with r = row_ids[i];
//     a negative r (or no CSR at all) is the empty set.
//   - Columns are ascending; duplicates are allowed; a column outside [0, n)
//     belongs to no set and is never used as an index.
//   - A column counts towards the set's size where it is in [0, n) and differs
//     from its left neighbour in the segment.
#pragma once

#include "common.h"

namespace hrec {

struct ExclSeg {
  int64_t lo, hi;  // positions [lo, hi) of cols
};

// The segment of factor / query row r.
__device__ __forceinline__ ExclSeg excl_segment(const int64_t* __restrict__ indptr, int64_t r) {
  if (!indptr || r < 0) return {0, 0};
  return {indptr[r], indptr[r + 1]};
}
// The segment of row i of a call (row_ids null: no CSR).
__device__ __forceinline__ ExclSeg excl_segment(const int64_t* __restrict__ row_ids,
                                                const int64_t* __restrict__ indptr, int64_t i) {
  if (!row_ids) return {0, 0};
  return excl_segment(indptr, row_ids[i]);
}

// The first position of [lo, hi) whose column is >= j (hi: none); negative
// columns fall before any j >= 0.
__device__ __forceinline__ int64_t excl_lower_bound(const int32_t* __restrict__ cols, int64_t lo, int64_t hi,
                                                    int64_t j) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)cols[mid] < j) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ bool excl_contains(const int32_t* __restrict__ cols, int64_t lo, int64_t hi, int64_t j) {
  const int64_t a = excl_lower_bound(cols, lo, hi, j);
  return a < hi && (int64_t)cols[a] == j;
}

// Whether position p of the segment starting at lo counts: in [0, n) and not
// its left neighbour's column again.
__device__ __forceinline__ bool excl_counts(const int32_t* __restrict__ cols, int64_t lo, int64_t p, int64_t n) {
  const int64_t c = cols[p];
  return c >= 0 && c < n && (p == lo || (int64_t)cols[p - 1] != c);
}

// One wave walks positions [from, hi) of a segment starting at lo (from = lo,
// or a lower bound inside it), lanes striding: f(c) for every column c in
// [0, n), duplicates included, and the number of positions that count. The
// walk ends after the first stride that meets a column >= n (ascending:
// nothing in range follows); the trip count is wave-uniform.
template <typename F>
__device__ __forceinline__ int64_t excl_wave_walk(const int32_t* __restrict__ cols, int64_t lo, int64_t from,
                                                  int64_t hi, int64_t n, int lane, F&& f) {
  int64_t distinct = 0;
  for (int64_t p0 = from; p0 < hi; p0 += kWave) {
    const int64_t p = p0 + lane;
    bool counted = false, past = false;
    if (p < hi) {
      const int64_t c = cols[p];
      past = c >= n;
      if (c >= 0 && !past) {
        f(c);
        counted = excl_counts(cols, lo, p, n);
      }
    }
    distinct += __popcll(__ballot(counted));
    if (__ballot(past)) break;
  }
  return distinct;
}

}  // namespace hrec
