// Per-user evaluation by the reference's own protocol (hrec_user_metrics):
// RecommenderEvaluator's Precision@k / Recall@k against the +-0.1 band around
// the user's mean rating, NDCG on three grades and MAE / RMSE after the 1-5
// rescale (src/evaluation.py:19-149), for every row of a batch whose ranked
// lists and scores are already on the device. include/hrec.h has the contract.
//
// Shape: a handful of rated items per user against lists of up to 1024
// columns: a membership test per list position and a gather of the rated
// items' scores; no arithmetic to speak of. One wave owns a row, four rows per
// block (hf_finish_kernel's shape):
//   1. lane 0 adds the row's ratings in frame order the way np.mean does
//      (numpy's pairwise summation; um_sum) -> the band;
//   2. the lanes stride over the row's actual segment: the band's size, the
//      common items (column in [0, n)), the extremes of their ratings and
//      scores;
//   3. the lanes stride over the list positions below max(k): a binary search
//      of the column in the segment (csrc/exclusion.h), the found item's
//      rating against the band, one hit counter per k;
//   4. a second walk over the common items: grades of both sides on the true
//      ratings' min-max fit (counting, three grades), |t - p| and (t - p)^2 of
//      the 1-5 rescales; the scores are gathered again (cache hits);
//   5. lane 0 finishes: the tie-averaged DCG over the three predicted-grade
//      groups from the host's discount prefix sums, IDCG, the divisions.
// Every sum over a row's items is a lane-strided partial followed by the xor
// tree: one order per (row length), so equal inputs give equal bits. The sums
// over rows: the block adds its four waves in wave order into one partial per
// slot, a second launch adds the partials in a fixed order (no
// floating-point atomics).
#include "exclusion.h"
#include "hybrid_common.h"
#include "um_score.h"

#pragma clang fp contract(off)

namespace hrec {

constexpr int kUmMaxK = HREC_UM_MAX_K;
constexpr int kUmMaxCols = 2 * kUmMaxK + 3;
constexpr int kUmMaxSlots = 2 * kUmMaxCols + HREC_UM_STATUS_BITS;
constexpr int kUmListMax = 1024;  // largest k and list length
constexpr int kUmWork = 96;       // um_sum's work stack: 2 entries per halving level + 1 (counts < 2^31: 26 levels)
constexpr int kUmVals = 48;

struct UmParams : UmSource {  // sa, sb, ld, fb: csrc/um_score.h
  const int64_t* ranked;
  int64_t ranked_ld;
  int list_n;
  const int32_t* list_len;
  int64_t n_rows, n;
  int k[kUmMaxK];
  int n_k, kmax, ndcg_k;
  const double* cs;
  const int64_t* rows;
  const int64_t* indptr;
  const int32_t* cols;
  const double* ratings;
  const double* frame;
  const double* minmax;
  const int32_t* wins;
  double* per_row;
  int32_t* status;
  double* partials;
};

// numpy's pairwise sum of n <= 128 contiguous values: serial below 8, else
// eight interleaved accumulators and the tail.
__device__ __forceinline__ double um_leaf(const double* __restrict__ a, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// The same for any n: the recursive halving (split rounded down to a multiple
// of 8) as a post-order walk over explicit stacks in the wave's LDS slice
// (one lane runs this). wn < 0 marks "add the two values on top".
__device__ double um_sum(const double* __restrict__ a, int64_t n, double* vs, int64_t* wo, int64_t* wn) {
  if (n <= 128) return um_leaf(a, (int)n);
  int wt = 1, vt = 0;
  wo[0] = 0;
  wn[0] = n;
  while (wt > 0) {
    --wt;
    const int64_t off = wo[wt], cnt = wn[wt];
    if (cnt < 0) {
      const double b = vs[--vt];
      const double x = vs[--vt];
      vs[vt++] = x + b;
    } else if (cnt <= 128) {
      if (vt >= kUmVals) break;  // unreachable for counts < 2^31
      vs[vt++] = um_leaf(a + off, (int)cnt);
    } else {
      if (wt + 3 > kUmWork) break;  // unreachable for counts < 2^31
      int64_t n2 = cnt / 2;
      n2 -= n2 % 8;
      wo[wt] = 0, wn[wt] = -1, ++wt;
      wo[wt] = off + n2, wn[wt] = cnt - n2, ++wt;
      wo[wt] = off, wn[wt] = n2, ++wt;
    }
  }
  return vs[0];
}

// np.digitize(x, [0.33, 0.66]): NaN sorts past both edges.
__device__ __forceinline__ int um_grade(double x) { return x != x ? 2 : (x >= 0.33 ? 1 : 0) + (x >= 0.66 ? 1 : 0); }

// One row, one wave; out: the wave's slots of the block's partial (zeroed).
template <int SRC>
__device__ __forceinline__ void um_row(const UmParams& P, int64_t row, int lane, double* out, double* vs, int64_t* wo,
                                       int64_t* wn) {
  typedef typename UmScore<SRC>::type S;
  const int nk = P.n_k, ncol = 2 * nk + 3;
  const int64_t q = P.rows ? P.rows[row] : -1;
  const ExclSeg x = excl_segment(P.indptr, q);
  const int64_t cnt = x.hi - x.lo;
  double* pr = P.per_row + row * ncol;
  if (cnt <= 0) {  // no ratings: zeros, counted in no column
    for (int i = lane; i < ncol; i += kWave) pr[i] = 0.0;
    if (lane == 0) {
      P.status[row] = HREC_UM_NO_RATINGS | HREC_UM_NO_COMMON | HREC_UM_NO_RELEVANT;
      out[2 * ncol + 2] = out[2 * ncol + 3] = out[2 * ncol + 4] = 1.0;
    }
    return;
  }
  // 1. the band
  double thr = 0.0;
  if (lane == 0) thr = um_sum(P.frame + x.lo, cnt, vs, wo, wn) / (double)cnt;
  thr = __shfl(thr, 0, kWave);
  const double blo = thr - 0.1, bhi = thr + 0.1;
  UmFuse f{};
  if constexpr (SRC == HREC_UM_SRC_FUSED) f = um_fuse_row(P.minmax, P.wins, row);
  // 2. band size, common items, extremes
  int n_rel = 0, m = 0, inf = 0;
  double tmin = __builtin_inf(), tmax = -__builtin_inf();
  S pmin = (S)__builtin_inf(), pmax = (S)-__builtin_inf();
  for (int64_t p = x.lo + lane; p < x.hi; p += kWave) {
    const double r = P.ratings[p];
    const int64_t c = P.cols[p];
    n_rel += (blo <= r && r <= bhi) ? 1 : 0;
    if (c >= 0 && c < P.n) {
      ++m;
      const S s = um_score<SRC>(P, row, c, f);
      tmin = fmin(tmin, r), tmax = fmax(tmax, r);
      pmin = lane_min(pmin, s), pmax = lane_max(pmax, s);
      inf |= (s - s != (S)0 && s == s) ? 1 : 0;
    }
  }
  n_rel = wave_xor_sum(n_rel), m = wave_xor_sum(m), inf = wave_xor_sum(inf);
  tmin = wave_xor_min(tmin), tmax = wave_xor_max(tmax);
  pmin = wave_xor_min(pmin), pmax = wave_xor_max(pmax);
  // 3. hits below each k
  int len = P.list_len ? P.list_len[row] : P.list_n;
  len = len < 0 ? 0 : (len > P.list_n ? P.list_n : len);
  const int lim = len < P.kmax ? len : P.kmax;
  int hk[kUmMaxK];
#pragma unroll
  for (int i = 0; i < kUmMaxK; ++i) hk[i] = 0;
  for (int pos = lane; pos < lim; pos += kWave) {
    const int64_t c = P.ranked[row * P.ranked_ld + pos];
    if (c < 0 || c >= P.n) continue;
    const int64_t a = excl_lower_bound(P.cols, x.lo, x.hi, c);
    if (a >= x.hi || (int64_t)P.cols[a] != c) continue;
    const double r = P.ratings[a];
    if (!(blo <= r && r <= bhi)) continue;
#pragma unroll
    for (int i = 0; i < kUmMaxK; ++i) hk[i] += (i < nk && pos < P.k[i]) ? 1 : 0;
  }
#pragma unroll
  for (int i = 0; i < kUmMaxK; ++i) hk[i] = wave_xor_sum(hk[i]);
  // 4. grades and errors over the common items
  int c2 = 0, c1 = 0, c0 = 0, s2 = 0, s1 = 0, s0 = 0, t2 = 0, t1 = 0, bad = 0;
  double sabs = 0.0, ssq = 0.0;
  if (m > 0) {
    const double scale = 1.0 / mm_range(tmax - tmin);
    const double min_ = 0.0 - tmin * scale;
    const double trange = tmax - tmin;
    const S prange = pmax - pmin;
    for (int64_t p = x.lo + lane; p < x.hi; p += kWave) {
      const int64_t c = P.cols[p];
      if (c < 0 || c >= P.n) continue;
      const double t = P.ratings[p];
      const S s = um_score<SRC>(P, row, c, f);
      const int gt = um_grade(t * scale + min_);
      double pn;
      double p5;
      if constexpr (SRC == HREC_UM_SRC_F32) {  // the scaler's in-place f32 column; the rescale all in f32
        const float y = (float)((double)s * scale);
        pn = (double)(float)((double)y + min_);
        p5 = (double)((4.0f * (s - pmin)) / prange + 1.0f);
      } else {
        pn = s * scale + min_;
        p5 = (4.0 * (s - pmin)) / prange + 1.0;
      }
      const int gp = um_grade(pn);
      c2 += gp == 2, c1 += gp == 1, c0 += gp == 0;
      s2 += gp == 2 ? gt : 0, s1 += gp == 1 ? gt : 0, s0 += gp == 0 ? gt : 0;
      t2 += gt == 2, t1 += gt == 1;
      const double t5 = (4.0 * (t - tmin)) / trange + 1.0;
      const double d = t5 - p5;
      bad |= (d - d != 0.0) ? 1 : 0;  // NaN or infinite on either side
      sabs += fabs(d);
      ssq += d * d;
    }
    c2 = wave_xor_sum(c2), c1 = wave_xor_sum(c1), c0 = wave_xor_sum(c0);
    s2 = wave_xor_sum(s2), s1 = wave_xor_sum(s1), s0 = wave_xor_sum(s0);
    t2 = wave_xor_sum(t2), t1 = wave_xor_sum(t1), bad = wave_xor_sum(bad);
    sabs = wave_xor_sum(sabs), ssq = wave_xor_sum(ssq);
  }
  if (lane != 0) return;
  // 5. the row's values
  int st = (n_rel ? 0 : HREC_UM_NO_RELEVANT) | (m ? 0 : HREC_UM_NO_COMMON);
#pragma unroll
  for (int i = 0; i < kUmMaxK; ++i) {
    if (i < nk) {
      const double pk = (double)hk[i] / (double)P.k[i];
      const double rk = n_rel ? (double)hk[i] / (double)n_rel : 0.0;
      pr[i] = pk, pr[nk + i] = rk;
      out[i] = pk, out[nk + i] = rk;
      out[ncol + i] = out[ncol + nk + i] = 1.0;
    }
  }
  double ndcg = 0.0, mae = 0.0, rmse = 0.0;
  if (m > 0) {
    if (m == 1 || inf) {
      st |= HREC_UM_NDCG_UNDEFINED;
      ndcg = __builtin_nan("");
    } else {
      auto at = [&](int j) { return P.cs[j < P.ndcg_k ? j : P.ndcg_k]; };
      double dcg = 0.0;
      int end = 0;
      auto group = [&](int c, int s) {  // a predicted-grade group: its mean true grade times its positions' discounts
        if (c == 0) return;
        const double w = end == 0 ? at(c) : at(end + c) - at(end);
        dcg = dcg + ((double)s / (double)c) * w;
        end += c;
      };
      group(c2, s2), group(c1, s1), group(c0, s0);
      const double idcg = 2.0 * at(t2) + (at(t2 + t1) - at(t2));
      ndcg = idcg != 0.0 ? dcg / idcg : 0.0;
    }
    if (bad) {
      st |= HREC_UM_ERR_UNDEFINED;
      mae = rmse = __builtin_nan("");
    } else {
      mae = sabs / (double)m;
      rmse = sqrt(ssq / (double)m);
    }
  }
  pr[2 * nk] = ndcg, pr[2 * nk + 1] = mae, pr[2 * nk + 2] = rmse;
  P.status[row] = st;
  if (!(st & HREC_UM_NDCG_UNDEFINED)) out[2 * nk] = ndcg, out[ncol + 2 * nk] = 1.0;
  if (!(st & HREC_UM_ERR_UNDEFINED)) {
    out[2 * nk + 1] = mae, out[2 * nk + 2] = rmse;
    out[ncol + 2 * nk + 1] = out[ncol + 2 * nk + 2] = 1.0;
  }
#pragma unroll
  for (int b = 0; b < HREC_UM_STATUS_BITS; ++b) out[2 * ncol + b] = (st >> b) & 1 ? 1.0 : 0.0;
}

template <int SRC>
__global__ __launch_bounds__(256) void um_kernel(const UmParams P) {
  __shared__ double red[4][kUmMaxSlots];
  __shared__ double vs[4][kUmVals];
  __shared__ int64_t wo[4][kUmWork], wn[4][kUmWork];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  const int nslots = 2 * (2 * P.n_k + 3) + HREC_UM_STATUS_BITS;
  for (int i = lane; i < kUmMaxSlots; i += kWave) red[w][i] = 0.0;
  wave_lds_fence();
  if (row < P.n_rows) um_row<SRC>(P, row, lane, red[w], vs[w], wo[w], wn[w]);  // wave-uniform
  __syncthreads();
  if ((int)threadIdx.x < nslots) {
    const int i = threadIdx.x;
    P.partials[(int64_t)blockIdx.x * nslots + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

// sums[i] = the blocks' partials of slot i (block i of the launch): lane l adds
// blocks l, l + 64, ... in ascending order, then the lanes' xor tree.
__global__ __launch_bounds__(64) void um_reduce_kernel(const double* __restrict__ partials, int64_t n_blocks, int nslots,
                                                       double* __restrict__ sums) {
  const int lane = threadIdx.x, i = blockIdx.x;
  double v = 0.0;
  for (int64_t b = lane; b < n_blocks; b += 64) v += partials[b * nslots + i];
  v = wave_xor_sum(v);
  if (lane == 0) sums[i] = v;
}

}  // namespace hrec

using namespace hrec;

static int64_t um_blocks(int64_t n_rows) { return n_rows > 0 ? (n_rows + 3) / 4 : 1; }

extern "C" size_t hrec_user_metrics_workspace_bytes(int64_t n_rows) {
  return al256((size_t)um_blocks(n_rows) * kUmMaxSlots * sizeof(double));
}

extern "C" int hrec_user_metrics(const int64_t* ranked, int64_t ranked_ld, int list_n, const int32_t* list_len,
                                 int64_t n_rows, int64_t n, const int32_t* k_values, int n_k, int ndcg_k,
                                 const double* disc_cs, const int64_t* act_rows, const int64_t* act_indptr,
                                 const int32_t* act_cols, const double* act_ratings, const double* act_frame,
                                 int source, const void* scores, const float* tt_scores, int64_t ld,
                                 const double* als_fallback, const double* minmax, const int32_t* row_wins,
                                 double* per_row, int32_t* status, double* sums_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 1, "user_metrics: bad shape");
  HREC_REQUIRE(n_k >= 1 && n_k <= kUmMaxK, "user_metrics: n_k must be in [1, %d] (got %d)", kUmMaxK, n_k);
  HREC_REQUIRE(k_values, "user_metrics: null pointer (k_values)");
  for (int i = 0; i < n_k; ++i)
    HREC_REQUIRE(k_values[i] >= 1 && k_values[i] <= kUmListMax, "user_metrics: k must be in [1, %d] (got %d)",
                 kUmListMax, k_values[i]);
  HREC_REQUIRE(ndcg_k >= 1 && ndcg_k <= kUmListMax, "user_metrics: ndcg_k must be in [1, %d] (got %d)", kUmListMax,
               ndcg_k);
  HREC_REQUIRE(list_n >= 0 && list_n <= kUmListMax, "user_metrics: list_n must be in [0, %d] (got %d)", kUmListMax,
               list_n);
  HREC_REQUIRE(ranked_ld >= list_n, "user_metrics: ranked_ld must be >= list_n");
  HREC_REQUIRE(ld >= n, "user_metrics: ld must be >= n");
  HREC_REQUIRE(n_rows < 65536, "user_metrics: at most 65535 rows per call");
  HREC_REQUIRE(source >= HREC_UM_SRC_F64 && source <= HREC_UM_SRC_FUSED, "user_metrics: source must be in [0, 3]");
  const bool any_act = act_rows || act_indptr || act_cols || act_ratings || act_frame;
  HREC_REQUIRE(!any_act || (act_rows && act_indptr && act_cols && act_ratings && act_frame),
               "user_metrics: the actual CSR needs act_rows, act_indptr, act_cols, act_ratings and act_frame (or "
               "none of them)");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(ranked && disc_cs && scores && per_row && status && sums_out && workspace,
               "user_metrics: null pointer");
  HREC_REQUIRE(source != HREC_UM_SRC_FUSED || (tt_scores && minmax && row_wins),
               "user_metrics: the fused source needs tt_scores, minmax and row_wins");
  const size_t need = hrec_user_metrics_workspace_bytes(n_rows);
  HREC_REQUIRE(workspace_bytes >= need, "user_metrics: workspace %zu < %zu", workspace_bytes, need);
  UmParams P{};
  P.ranked = ranked, P.ranked_ld = ranked_ld, P.list_n = list_n, P.list_len = list_len;
  P.n_rows = n_rows, P.n = n;
  P.n_k = n_k, P.kmax = 0, P.ndcg_k = ndcg_k;
  for (int i = 0; i < kUmMaxK; ++i) {
    P.k[i] = i < n_k ? k_values[i] : 0;
    P.kmax = P.k[i] > P.kmax ? P.k[i] : P.kmax;
  }
  P.cs = disc_cs;
  P.rows = act_rows, P.indptr = act_indptr, P.cols = act_cols, P.ratings = act_ratings, P.frame = act_frame;
  P.sa = scores, P.sb = tt_scores, P.ld = ld;
  P.fb = (source == HREC_UM_SRC_ALS || source == HREC_UM_SRC_FUSED) ? als_fallback : nullptr;
  P.minmax = minmax, P.wins = row_wins;
  P.per_row = per_row, P.status = status, P.partials = static_cast<double*>(workspace);
  hipStream_t s = as_stream(stream);
  const int64_t nb = um_blocks(n_rows);
  const int nslots = 2 * (2 * n_k + 3) + HREC_UM_STATUS_BITS;
  const dim3 grid((unsigned)nb), block(256);
  switch (source) {
    case HREC_UM_SRC_F64: hipLaunchKernelGGL(um_kernel<HREC_UM_SRC_F64>, grid, block, 0, s, P); break;
    case HREC_UM_SRC_F32: hipLaunchKernelGGL(um_kernel<HREC_UM_SRC_F32>, grid, block, 0, s, P); break;
    case HREC_UM_SRC_ALS: hipLaunchKernelGGL(um_kernel<HREC_UM_SRC_ALS>, grid, block, 0, s, P); break;
    default: hipLaunchKernelGGL(um_kernel<HREC_UM_SRC_FUSED>, grid, block, 0, s, P); break;
  }
  const int rc = check_launch("um_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(um_reduce_kernel, dim3((unsigned)nslots), dim3(64), 0, s, P.partials, nb, nslots, sums_out);
  return check_launch("um_reduce_kernel");
}
