// The two kernels every *_excluding top-k path shares (convention:
// csrc/exclusion.h): masking a score matrix's excluded columns and dropping a
// candidate list's excluded items; and hrec_mask_rows_f32.
#include "exclusion.h"

namespace hrec {

// Masking, strided: vals is [n_rows][row_stride], column s < S holding item
// s * step (a sample of hrec_dot_topk; step 1 and S = n: a full score row).
// One wave per row (excl_wave_walk): an excluded item c in [0, n) with
// c % step == 0 and c / step < S gets vals[i][c / step] = fill; any other
// column touches nothing. vals may be null (lengths only). kept_out[i]
// (optional) = min(len_cap, n - distinct columns in [0, n)).
__global__ __launch_bounds__(256) void excl_mask_kernel(float* __restrict__ vals, int64_t n_rows, int64_t row_stride,
                                                        int64_t S, int64_t step, int64_t n,
                                                        const int64_t* __restrict__ row_ids,
                                                        const int64_t* __restrict__ excl_indptr,
                                                        const int32_t* __restrict__ excl_cols, float fill,
                                                        int64_t len_cap, int32_t* __restrict__ kept_out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;  // wave-uniform
  const ExclSeg x = excl_segment(row_ids, excl_indptr, row);
  float* __restrict__ rv = vals + row * row_stride;
  const int64_t distinct = excl_wave_walk(excl_cols, x.lo, x.lo, x.hi, n, lane, [&](int64_t c) {
    const int64_t sc = step == 1 ? c : c / step;  // wave-uniform choice
    if (vals && sc * step == c && sc < S) rv[sc] = fill;  // duplicates store the same value
  });
  if (lane == 0 && kept_out) {
    const int64_t kept = n - distinct;
    kept_out[row] = (int32_t)(kept < len_cap ? kept : len_cap);
  }
}

// The filter's candidates without the excluded items: one block per query, a
// thread per candidate, a binary search of the query's ascending segment; an
// excluded candidate's score becomes NaN (better() ranks NaN last, so the
// top-k over the list passes it only after every candidate that stays). The
// lists hold the columns' own indices (hrec_dot_topk: local item indices, the
// offset is added to the ranked result afterwards); the (-inf, INT64_MAX - 1)
// fillers of an overflowed list match no column. A list past the cap (the
// filter raised *overflow) is read up to the cap. out_len[b] (optional) =
// min(kk, candidates that stay), counted by ballots into an LDS integer.
__global__ __launch_bounds__(256) void excl_drop_kernel(const int64_t* __restrict__ row_ids,
                                                        const int64_t* __restrict__ excl_indptr,
                                                        const int32_t* __restrict__ excl_cols,
                                                        float* __restrict__ cand_v,
                                                        const int64_t* __restrict__ cand_i,
                                                        const int* __restrict__ cand_n, int cap, int kk,
                                                        int32_t* __restrict__ out_len) {
  __shared__ int s_kept;
  const int b = blockIdx.x;
  const ExclSeg x = excl_segment(row_ids, excl_indptr, b);
  if (!out_len && x.lo >= x.hi) return;  // block-uniform: nothing to drop or count
  if (out_len) {  // block-uniform, as are the tests of it below
    if (threadIdx.x == 0) s_kept = 0;
    __syncthreads();
  }
  const int n = cand_n[b] < cap ? cand_n[b] : cap;
  const float qnan = __builtin_nanf("");
  for (int e0 = 0; e0 < n; e0 += blockDim.x) {  // block-uniform trip count: the ballots see whole waves
    const int e = e0 + threadIdx.x;
    bool keep = false;
    if (e < n) {
      keep = !excl_contains(excl_cols, x.lo, x.hi, cand_i[(int64_t)b * cap + e]);
      if (!keep) cand_v[(int64_t)b * cap + e] = qnan;
    }
    if (out_len) {
      const uint64_t m = __ballot(keep);
      if (m && (threadIdx.x & 63) == 0) atomicAdd(&s_kept, __popcll(m));  // LDS, integer
    }
  }
  if (!out_len) return;  // block-uniform
  __syncthreads();
  if (threadIdx.x == 0) out_len[b] = s_kept < kk ? s_kept : kk;
}

int excl_mask_run(float* vals, int64_t n_rows, int64_t row_stride, int64_t S, int64_t step, int64_t n,
                  const Excl& x, float fill, int64_t len_cap, int32_t* kept_out, hipStream_t s) {
  hipLaunchKernelGGL(excl_mask_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, vals, n_rows, row_stride,
                     S, step, n, x.rows, x.indptr, x.cols, fill, len_cap, kept_out);
  return check_launch("excl_mask_kernel");
}

int excl_drop_run(const Excl& x, int n_users, float* cand_v, const int64_t* cand_i, const int* cand_n, int cap,
                  int kk, int32_t* out_len, hipStream_t s) {
  hipLaunchKernelGGL(excl_drop_kernel, dim3((unsigned)n_users), dim3(256), 0, s, x.rows, x.indptr, x.cols, cand_v,
                     cand_i, cand_n, cap, kk, out_len);
  return check_launch("excl_drop_kernel");
}

}  // namespace hrec

using namespace hrec;

extern "C" int hrec_mask_rows_f32(float* vals, int64_t n_rows, int64_t n, int64_t row_stride, const int64_t* row_ids,
                                  const int64_t* excl_indptr, const int32_t* excl_cols, float fill,
                                  int32_t* kept_out, void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 0 && row_stride >= n, "mask_rows_f32: bad shape");
  HREC_REQUIRE(n < ((int64_t)1 << 31) && n_rows < ((int64_t)1 << 31), "mask_rows_f32: n and n_rows must be < 2^31");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE((vals || n == 0) && row_ids && excl_indptr && excl_cols && kept_out, "mask_rows_f32: null pointer");
  return excl_mask_run(vals, n_rows, row_stride, n, 1, n, Excl{true, row_ids, excl_indptr, excl_cols, nullptr}, fill,
                       INT64_MAX, kept_out, as_stream(stream));
}
