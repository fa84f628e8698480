// K2r: Spark's RankingMetrics (binary relevance) over ranked id lists that
// are already on the device: per row precision@k, recall@k, average precision,
// average precision@k and NDCG@k in f64, and their sums over the rows (what
// RankingEvaluator divides by the row count).
//
// Shape: a set membership test per (row, position), no arithmetic to speak of:
// the bytes are the label rows, the lists and the row pointer, each read
// once. One wave owns a row; a workgroup of 4 waves strides over the rows.
//  1. the lanes stride over the label row (sorted ascending, duplicates
//     allowed): a neighbour compare per entry counts the distinct labels m and
//     finds a descending pair (the *unsorted flag); rows of up to
//     kRankLdsLabels labels are copied into the wave's LDS slice on the way, so
//     the searches below stay on the CU;
//  2. the lanes stride over the list positions i in steps of 64, each with a
//     binary search of pred[i] in the label row; the ballot of the hits is the
//     wave's view of 64 positions;
//  3. the two sequential sums (sum cnt / (i + 1), sum gain[i]) walk the set
//     bits of that mask in ascending i: at most len additions per row, the
//     same in every lane (wave-uniform, no cross-lane step).
// A row's loads would otherwise wait on each other (row pointer -> labels ->
// list -> search), so the next row's pointer pair and list length are read a
// row ahead, the list's first 64 entries are requested before the label pass,
// and the label pass has 8 loads per lane in flight.
// Every per-row value is one IEEE division of integers or of sums added in
// ascending i from the caller's tables, so it has one value, whatever the
// machine. The sums over rows: each wave adds its rows in ascending order,
// the block adds its four waves in wave order into one partial, a second
// launch adds the partials in a fixed order (no floating-point atomics).
#include "wave.h"  // wave_lds_fence, wave_xor_sum

namespace hrec {

constexpr int kRankBlock = 256;       // 4 waves, one row each per step
constexpr int kRankMaxBlocks = 2048;  // grid cap: the rows beyond are taken in grid strides
constexpr int kRankLdsLabels = 512;   // label rows up to this many entries are searched in LDS
constexpr int kRankMax = 1024;        // largest k and list length
constexpr int kRankBatch = 8;         // label loads per lane in flight (64 * 8 = one LDS slice)

// Blocks of a launch over n rows: a function of n alone (one partial layout,
// one summation order per n).
__host__ __device__ inline int64_t rank_blocks(int64_t n) {
  const int64_t b = n / 4 + (n % 4 != 0);
  return b < 1 ? 1 : (b > kRankMaxBlocks ? kRankMaxBlocks : b);
}

// Whether x is among the n ascending entries of a.
__device__ __forceinline__ bool rank_contains(const int64_t* a, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;  // the first entry >= x lies in [lo, hi]
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && a[lo] == x;
}

__global__ __launch_bounds__(kRankBlock) void ranking_metrics_kernel(
    const int64_t* __restrict__ pred, int64_t pred_ld, int pred_len_max, const int32_t* __restrict__ pred_len,
    const int64_t* __restrict__ label_indptr, const int64_t* __restrict__ labels, int64_t n_rows, int k,
    const double* __restrict__ gain, const double* __restrict__ idcg, double* __restrict__ per_row,
    double* __restrict__ partials, int32_t* __restrict__ unsorted) {
#pragma clang fp contract(off)
  __shared__ int64_t slab[4][kRankLdsLabels];
  __shared__ double red[4][HREC_RANK_SUMS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double s[HREC_RANK_SUMS];
#pragma unroll
  for (int i = 0; i < HREC_RANK_SUMS; ++i) s[i] = 0.0;

  // a row's pointer pair and list length, read one row ahead of their use
  const int64_t r_step = (int64_t)gridDim.x * 4;
  int64_t r = (int64_t)blockIdx.x * 4 + w;
  int64_t lo_n = 0, hi_n = 0;
  int len_n = 0;
  auto fetch_row = [&](int64_t rr) {
    if (rr < n_rows) {
      lo_n = label_indptr[rr];
      hi_n = label_indptr[rr + 1];
      len_n = pred_len ? pred_len[rr] : pred_len_max;
    }
  };
  fetch_row(r);
  for (; r < n_rows; r += r_step) {  // wave-uniform
    const int64_t lo = lo_n, hi = hi_n;
    int len = len_n;
    fetch_row(r + r_step);
    len = len < 0 ? 0 : (len > pred_len_max ? pred_len_max : len);
    const int64_t n_lab = hi > lo ? hi - lo : 0;
    const int64_t* __restrict__ row = labels + lo;
    const int64_t* __restrict__ list = pred + r * pred_ld;
    const bool staged = n_lab <= kRankLdsLabels;
    // the first 64 list entries do not wait for the labels
    const int64_t first = lane < len ? list[lane] : 0;
    // 1. distinct labels, order check, LDS copy: kRankBatch entries (and their
    //    left neighbours, cache hits) per lane in flight before the first use
    int distinct = 0;
    bool desc = false;
    for (int64_t j0 = 0; j0 < n_lab; j0 += 64 * kRankBatch) {
      int64_t x[kRankBatch], p[kRankBatch];
#pragma unroll
      for (int t = 0; t < kRankBatch; ++t) {
        const int64_t j = j0 + t * 64 + lane;
        x[t] = j < n_lab ? row[j] : 0;
        p[t] = (j < n_lab && j > 0) ? row[j - 1] : 0;
      }
#pragma unroll
      for (int t = 0; t < kRankBatch; ++t) {
        const int64_t j = j0 + t * 64 + lane;
        if (j < n_lab) {
          if (staged) slab[w][j] = x[t];
          distinct += (j == 0) || (p[t] != x[t]);
          desc |= j > 0 && p[t] > x[t];
        }
      }
    }
#pragma unroll  // written out: wave_xor_sum here changes the generated code
    for (int off = 32; off > 0; off >>= 1) distinct += __shfl_xor(distinct, off, kWave);
    if (desc) *unsorted = 1;  // every writer stores the same value
    wave_lds_fence();
    const int64_t* a = staged ? slab[w] : row;
    const int64_t m = distinct;

    const int nk = len < k ? len : k;  // positions that count for precision, recall and AP@k
    const int64_t big = len > m ? len : m;
    const int n_ndcg = (int)(big < k ? big : k);
    const int nd = n_ndcg < len ? n_ndcg : len;  // positions that count for the DCG
    // 2. + 3. hits per 64 positions, then the sequential sums over the set bits
    int cnt = 0, hits_k = 0;
    double ap = 0.0, apk = 0.0, dcg = 0.0;
    if (m > 0) {
      for (int i0 = 0; i0 < len; i0 += 64) {
        const int i = i0 + lane;
        const bool hit = i < len && rank_contains(a, n_lab, i0 == 0 ? first : list[i]);
        unsigned long long mask = __ballot(hit);
        while (mask) {
          const int p = i0 + __builtin_ctzll(mask);
          mask &= mask - 1;
          ++cnt;
          const double t = (double)cnt / (double)(p + 1);
          ap = ap + t;
          if (p < nk) {
            ++hits_k;
            apk = apk + t;
          }
          if (p < nd) dcg = dcg + gain[p];
        }
      }
    }
    wave_lds_fence();  // the next row overwrites the LDS copy
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (m > 0) {
      const int64_t mk = m < k ? m : (int64_t)k;
      const int64_t mi = m < n_ndcg ? m : (int64_t)n_ndcg;
      v[0] = (double)hits_k / (double)k;
      v[1] = (double)hits_k / (double)m;
      v[2] = ap / (double)m;  // min(m, max(len, m)) = m
      v[3] = apk / (double)mk;
      v[4] = dcg / idcg[mi];
    }
    if (per_row && lane == 0) {
#pragma unroll
      for (int i = 0; i < 5; ++i) per_row[r * 5 + i] = v[i];
    }
    s[HREC_RANK_N_ROWS] += 1.0;
    s[HREC_RANK_N_EMPTY] += m > 0 ? 0.0 : 1.0;
    s[HREC_RANK_HITS] += (double)hits_k;
    s[HREC_RANK_SUM_PRECISION] += v[0];
    s[HREC_RANK_SUM_RECALL] += v[1];
    s[HREC_RANK_SUM_AP] += v[2];
    s[HREC_RANK_SUM_AP_K] += v[3];
    s[HREC_RANK_SUM_NDCG] += v[4];
  }
  // a wave's sums are the same in all its lanes; the four waves in wave order
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < HREC_RANK_SUMS; ++i) red[w][i] = s[i];
  }
  __syncthreads();
  if (threadIdx.x < HREC_RANK_SUMS) {
    const int i = threadIdx.x;
    partials[(int64_t)blockIdx.x * HREC_RANK_SUMS + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

// sums[i] = the blocks' partials of slot i: wave i, lane l adds blocks l,
// l + 64, ... in ascending order, then the lanes' xor tree.
__global__ __launch_bounds__(64 * HREC_RANK_SUMS) void ranking_reduce_kernel(const double* __restrict__ partials,
                                                                            int64_t n_blocks,
                                                                            double* __restrict__ sums) {
  const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;
  double v = 0.0;
  for (int64_t b = lane; b < n_blocks; b += 64) v += partials[b * HREC_RANK_SUMS + i];
  v = wave_xor_sum(v);
  if (lane == 0) sums[i] = v;
}

}  // namespace hrec

using namespace hrec;

extern "C" size_t hrec_ranking_metrics_workspace_bytes(int64_t n_rows) {
  return al256((size_t)rank_blocks(n_rows > 0 ? n_rows : 0) * HREC_RANK_SUMS * sizeof(double));
}

extern "C" int hrec_ranking_metrics(const int64_t* pred, int64_t pred_ld, int pred_len_max, const int32_t* pred_len,
                                    const int64_t* label_indptr, const int64_t* labels, int64_t n_rows, int k,
                                    const double* gain, const double* idcg, double* per_row, double* sums_out,
                                    int32_t* unsorted, void* workspace, size_t workspace_bytes, void* stream) {
  HREC_REQUIRE(n_rows >= 0, "ranking_metrics: negative n_rows");
  HREC_REQUIRE(k >= 1 && k <= kRankMax, "ranking_metrics: k must be in [1, %d] (got %d)", kRankMax, k);
  HREC_REQUIRE(pred_len_max >= 0 && pred_len_max <= kRankMax,
               "ranking_metrics: pred_len_max must be in [0, %d] (got %d)", kRankMax, pred_len_max);
  HREC_REQUIRE(pred_ld >= pred_len_max, "ranking_metrics: pred_ld must be >= pred_len_max");
  hipStream_t s = as_stream(stream);
  if (n_rows == 0) {  // nothing to read: zeros
    if ((unsorted && hipMemsetAsync(unsorted, 0, sizeof(int32_t), s) != hipSuccess) ||
        (sums_out && hipMemsetAsync(sums_out, 0, HREC_RANK_SUMS * sizeof(double), s) != hipSuccess))
      return check_launch("ranking_metrics: memset");
    return HREC_OK;
  }
  HREC_REQUIRE(pred && label_indptr && labels && gain && idcg, "ranking_metrics: null pointer");
  HREC_REQUIRE(sums_out && unsorted && workspace, "ranking_metrics: null sums, unsorted flag or workspace");
  const size_t need = hrec_ranking_metrics_workspace_bytes(n_rows);
  HREC_REQUIRE(workspace_bytes >= need, "ranking_metrics: workspace of %zu bytes, need %zu", workspace_bytes, need);
  if (hipMemsetAsync(unsorted, 0, sizeof(int32_t), s) != hipSuccess) return check_launch("ranking_metrics: memset");
  const int64_t nb = rank_blocks(n_rows);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(ranking_metrics_kernel, dim3((unsigned)nb), dim3(kRankBlock), 0, s, pred, pred_ld, pred_len_max,
                     pred_len, label_indptr, labels, n_rows, k, gain, idcg, per_row, part, unsorted);
  hipLaunchKernelGGL(ranking_reduce_kernel, dim3(1), dim3(64 * HREC_RANK_SUMS), 0, s, part, nb, sums_out);
  return check_launch("ranking_metrics_kernel");
}
