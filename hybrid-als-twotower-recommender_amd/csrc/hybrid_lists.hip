// Hybrid ranked lists (hrec_hybrid_lists): for every row of two f32 score
// matrices, hrec_fuse_topk's fusion (ALS side in f64 after the cold-start
// substitution, two-tower side in f32, scalers over ALL columns) and the
// stable descending top-kk of the columns outside the row's exclusion set.
//   1. hl_extremes_kernel: per-row extremes -> scaler coefficients, out_minmax,
//      out_len; clears the row counters and the overflow flag;
//   2. mode 0: hl_bound_kernel takes the kk-th best fused key of the row's
//      first kHlSample columns (excluded ones emptied) — kk distinct
//      non-excluded columns have key >= bound, so the answer's kk-th key has
//      too and every entry of the answer passes `key >= bound`;
//      hl_pass_kernel<0> appends the columns that pass to the row's list,
//      topk_rows ranks the lists by (value, column);
//   3. mode 1: hl_pass_kernel<1> writes every fused value and its column (-1
//      where excluded) and topk_rows ranks the whole rows.
// Keys are slot_order_key's: 0 = excluded / empty, 1 = NaN, numbers above.
// hrec_hybrid_lists_rowwise is the same body with the fusion weights chosen
// per row (row_wins, hrec_hybrid_model_f1's output) instead of per call.
#include "exclusion.h"
#include "hybrid_common.h"

namespace hrec {

// The fusion weights of row r: (0.8, 0.2) when ALS wins, else (0.2, 0.8); row_wins (optional) decides per row.
struct HlWeights {
  double w0, w1;
};
__device__ __forceinline__ HlWeights hl_weights(const int32_t* __restrict__ row_wins, int als_wins, int64_t r) {
  const bool wins = row_wins ? row_wins[r] != 0 : als_wins != 0;
  return {wins ? 0.8 : 0.2, wins ? 0.2 : 0.8};
}

// One 1024-thread block per row: ALS min / max in f64 after the substitution,
// two-tower min / max in f32 (NaN ignored; hrec_fuse_topk's fmin / fmax from
// +-DBL_MAX), the scaler coefficients, the row's list length, and the resets.
__global__ __launch_bounds__(1024) void hl_extremes_kernel(
    const float* __restrict__ als, const float* __restrict__ tt, int64_t n, int64_t ld, int vec4,
    const double* __restrict__ fb, const int64_t* __restrict__ excl_rows, const int64_t* __restrict__ excl_indptr,
    const int32_t* __restrict__ excl_cols, int kk, HpScale* __restrict__ coef, double* __restrict__ out_minmax,
    int32_t* __restrict__ out_len, int* __restrict__ cnt, int* __restrict__ overflow) {
  __shared__ double s_amin[16], s_amax[16];
  __shared__ float s_tmin[16], s_tmax[16];
  __shared__ int s_dist[16];
  const int64_t r = blockIdx.x;
  const float* ar = als + r * ld;
  const float* tr = tt + r * ld;
  double amin = DBL_MAX, amax = -DBL_MAX;
  float tmin = __builtin_inff(), tmax = -__builtin_inff();
  auto take = [&](float a, float t, int64_t j) {
    const double ad = hl_als(a, fb, j);
    amin = fmin(amin, ad);
    amax = fmax(amax, ad);
    tmin = fminf(tmin, t);
    tmax = fmaxf(tmax, t);
  };
  int64_t j0 = 0;
  if (vec4) {
    const int64_t n4 = n >> 2;
    const float4* a4 = reinterpret_cast<const float4*>(ar);
    const float4* t4 = reinterpret_cast<const float4*>(tr);
    for (int64_t j = threadIdx.x; j < n4; j += 1024) {
      const float4 a = a4[j], t = t4[j];
      take(a.x, t.x, 4 * j);
      take(a.y, t.y, 4 * j + 1);
      take(a.z, t.z, 4 * j + 2);
      take(a.w, t.w, 4 * j + 3);
    }
    j0 = n4 << 2;
  }
  for (int64_t j = j0 + threadIdx.x; j < n; j += 1024) take(ar[j], tr[j], j);
  // distinct in-range excluded columns
  const ExclSeg x = excl_segment(excl_rows, excl_indptr, r);
  int dist = 0;
  for (int64_t p = x.lo + threadIdx.x; p < x.hi; p += 1024) dist += excl_counts(excl_cols, x.lo, p, n) ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    amin = fmin(amin, __shfl_xor(amin, off, kWave));
    amax = fmax(amax, __shfl_xor(amax, off, kWave));
    tmin = fminf(tmin, __shfl_xor(tmin, off, kWave));
    tmax = fmaxf(tmax, __shfl_xor(tmax, off, kWave));
    dist += __shfl_xor(dist, off, kWave);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_amin[w] = amin;
    s_amax[w] = amax;
    s_tmin[w] = tmin;
    s_tmax[w] = tmax;
    s_dist[w] = dist;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int q = 1; q < 16; ++q) {
    amin = fmin(amin, s_amin[q]);
    amax = fmax(amax, s_amax[q]);
    tmin = fminf(tmin, s_tmin[q]);
    tmax = fmaxf(tmax, s_tmax[q]);
    dist += s_dist[q];
  }
  coef[r] = hp_scale64(amin, amax, tmin, tmax);
  if (out_minmax) {  // hrec_fuse_topk's out_minmax: the two-tower pair starts from +-DBL_MAX too
    out_minmax[4 * r + 0] = amin;
    out_minmax[4 * r + 1] = amax;
    out_minmax[4 * r + 2] = fmin(DBL_MAX, (double)tmin);
    out_minmax[4 * r + 3] = fmax(-DBL_MAX, (double)tmax);
  }
  const int64_t kept = n - dist;
  out_len[r] = (int32_t)(kept < kk ? kept : kk);
  cnt[r] = 0;
  if (r == 0) *overflow = 0;
}

// One block per row (n > kHlSample): the kk-th best key of the first
// kHlSample columns with the excluded ones emptied, by a search over the key
// bits (the largest T with at least kk keys >= T). Fewer than kk live sample
// columns leave T = 0: everything passes.
__global__ __launch_bounds__(kHlBoundBlock) void hl_bound_kernel(
    const float* __restrict__ als, const float* __restrict__ tt, int64_t ld, const double* __restrict__ fb,
    const int64_t* __restrict__ excl_rows, const int64_t* __restrict__ excl_indptr,
    const int32_t* __restrict__ excl_cols, const HpScale* __restrict__ coef, const int32_t* __restrict__ row_wins,
    int als_wins, int kk, uint64_t* __restrict__ bound) {
  __shared__ uint32_t bm[kHlSample / 32];
  __shared__ int cn[64];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  for (int q = tid; q < kHlSample / 32; q += kHlBoundBlock) bm[q] = 0;
  if (tid < 64) cn[tid] = 0;
  __syncthreads();
  const ExclSeg x = excl_segment(excl_rows, excl_indptr, r);
  for (int64_t p = x.lo + tid; p < x.hi; p += kHlBoundBlock) {
    const int64_t c = excl_cols[p];
    if (c >= kHlSample) break;  // ascending: nothing of the sample follows
    if (c >= 0) atomicOr(&bm[c >> 5], 1u << (c & 31));
  }
  __syncthreads();
  const HpScale sc = coef[r];
  const auto [w0, w1] = hl_weights(row_wins, als_wins, r);
  uint64_t key[kHlBoundPer];
#pragma unroll
  for (int e = 0; e < kHlBoundPer; ++e) {
    const int j = e * kHlBoundBlock + tid;
    const float a = als[r * ld + j], t = tt[r * ld + j];
    const uint64_t k = hl_key(hp_fuse64(sc, hl_als(a, fb, j), t, w0, w1));
    key[e] = ((bm[j >> 5] >> (j & 31)) & 1u) ? 0ull : k;
  }
  uint64_t T = 0;
  for (int b = 63; b >= 0; --b) {
    const uint64_t cand = T | (1ull << b);
    int c = 0;
#pragma unroll
    for (int e = 0; e < kHlBoundPer; ++e) c += key[e] >= cand ? 1 : 0;
#pragma unroll  // written out: wave_xor_sum here changes the generated code
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
    if ((tid & 63) == 0) atomicAdd(&cn[b], c);
    __syncthreads();
    if (cn[b] >= kk) T = cand;  // block-uniform
  }
  if (tid == 0) bound[r] = T;
}

// One wave per segment of kHlSeg contiguous columns of one row: substitute,
// fuse, drop the row's excluded columns (a per-wave LDS bitmap marked from the
// row's ascending list, lower-bounded at the segment start) and
//   MODE 0: ballot-compact the columns whose key reaches the row's bound into
//           the row's list of L entries (value, column); cnt[r] counts them
//           all, so cnt[r] > L tells an overflow;
//   MODE 1: write every value and its column (-1: excluded) to [n_rows][n].
template <int MODE>
__global__ __launch_bounds__(256) void hl_pass_kernel(
    const float* __restrict__ als, const float* __restrict__ tt, int64_t n, int64_t ld, int64_t segs,
    const double* __restrict__ fb, const int64_t* __restrict__ excl_rows, const int64_t* __restrict__ excl_indptr,
    const int32_t* __restrict__ excl_cols, const HpScale* __restrict__ coef, const int32_t* __restrict__ row_wins,
    int als_wins, const uint64_t* __restrict__ bound, int64_t L, double* __restrict__ out_v,
    int64_t* __restrict__ out_i, int* __restrict__ cnt) {
  __shared__ uint32_t bm_sh[4][kHlSeg / 32];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t seg = (int64_t)blockIdx.x * 4 + wv;
  if (seg >= segs) return;  // wave-uniform; no block barrier below
  const int64_t r = blockIdx.y;
  const int64_t seg0 = seg * kHlSeg;
  const int nvalid = (int)((n - seg0) < kHlSeg ? (n - seg0) : kHlSeg);
  uint32_t* bm = bm_sh[wv];
  if (lane < kHlSeg / 32) bm[lane] = 0;
  wave_lds_fence();
  const ExclSeg x = excl_segment(excl_rows, excl_indptr, r);
  if (x.lo < x.hi) {
    // from the first column >= seg0; columns past the segment (or past n) end the walk unused
    excl_wave_walk(excl_cols, x.lo, excl_lower_bound(excl_cols, x.lo, x.hi, seg0), x.hi, seg0 + nvalid, lane,
                   [&](int64_t c) {  // c >= seg0 always, when the columns ascend
                     if (c >= seg0) atomicOr(&bm[(c - seg0) >> 5], 1u << ((c - seg0) & 31));
                   });
  }
  wave_lds_fence();
  const HpScale sc = coef[r];
  const auto [w0, w1] = hl_weights(row_wins, als_wins, r);
  const uint64_t tk = (MODE == 0 && bound) ? bound[r] : 0ull;
  const float* ar = als + r * ld + seg0 + lane;
  const float* tr = tt + r * ld + seg0 + lane;
  float av[kHlPer], tv[kHlPer];
  if (nvalid == kHlSeg) {  // full segment: unconditional loads
#pragma unroll
    for (int e = 0; e < kHlPer; ++e) {
      av[e] = ar[e * 64];
      tv[e] = tr[e * 64];
    }
  } else {
#pragma unroll
    for (int e = 0; e < kHlPer; ++e) {
      const bool v = e * 64 + lane < nvalid;
      av[e] = v ? ar[e * 64] : 0.0f;
      tv[e] = v ? tr[e * 64] : 0.0f;
    }
  }
#pragma unroll
  for (int e = 0; e < kHlPer; ++e) {
    const int pos = e * 64 + lane;
    const bool valid = pos < nvalid;
    const int64_t j = seg0 + pos;
    const double fused = hp_fuse64(sc, hl_als(av[e], valid ? fb : nullptr, j), tv[e], w0, w1);
    const bool excluded = (bm[pos >> 5] >> (pos & 31)) & 1u;
    if (MODE == 1) {
      if (valid) {
        out_v[r * n + j] = fused;
        out_i[r * n + j] = excluded ? -1 : j;
      }
    } else {
      const bool c = valid && !excluded && hl_key(fused) >= tk;
      const uint64_t m = __ballot(c);
      if (m == 0) continue;  // wave-uniform
      int base = 0;
      if (lane == 0) base = atomicAdd(&cnt[r], __popcll(m));
      base = __builtin_amdgcn_readfirstlane(base);
      const int64_t slot = (int64_t)base + lanes_below(m);
      if (c && slot < L) {
        out_v[r * L + slot] = fused;
        out_i[r * L + slot] = j;
      }
    }
  }
}

}  // namespace hrec

using namespace hrec;

// Workspace of hrec_hybrid_lists, in carve order.
struct HlWs {
  HpScale* coef;    // [n_rows]
  uint64_t* bound;  // [n_rows] mode 0
  int* cnt;         // [n_rows] mode 0: columns that passed the bound
  double* v;        // mode 0: [n_rows][L] lists; mode 1: [n_rows][n]
  int64_t* i;
  char* tws;
  int64_t L;
  size_t total;
};

static HlWs hl_layout(void* base, int64_t n_rows, int64_t n, int kk, int mode) {
  HlWs w{};
  Carver c(base);
  w.L = mode == 0 ? (n < kHlCap ? n : kHlCap) : n;
  w.coef = (HpScale*)c.take((size_t)n_rows * sizeof(HpScale));
  w.bound = (uint64_t*)c.take((size_t)n_rows * 8);
  w.cnt = (int*)c.take((size_t)n_rows * 4);
  w.v = (double*)c.take((size_t)n_rows * w.L * 8);
  w.i = (int64_t*)c.take((size_t)n_rows * w.L * 8);
  w.tws = c.take(topk_ws_bytes(n_rows, w.L, kk, 8));
  w.total = c.total();
  return w;
}

extern "C" size_t hrec_hybrid_lists_workspace_bytes(int64_t n_rows, int64_t n, int top_k, int mode) {
  n_rows = n_rows > 0 ? n_rows : 0;
  n = n > 0 ? n : 0;
  return hl_layout(nullptr, n_rows, n, (int)(top_k < n ? top_k : n), mode == 1 ? 1 : 0).total;
}

// The body of hrec_hybrid_lists (row_wins null: als_wins for every row) and
// hrec_hybrid_lists_rowwise (rowwise: row_wins[r] != 0 chooses row r's weights).
static int hl_run(const char* who, bool rowwise, const float* als, const float* tt, int64_t n_rows, int64_t n,
                  int64_t ld, const double* als_fallback, const int32_t* row_wins, int als_wins, int top_k, int mode,
                  const int64_t* excl_rows, const int64_t* excl_indptr, const int32_t* excl_cols, int64_t* out_idx,
                  double* out_val, int32_t* out_len, double* out_minmax, int* overflow, void* workspace,
                  size_t workspace_bytes, void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 1, "%s: bad shape", who);
  HREC_REQUIRE(ld >= n, "%s: ld must be >= n", who);
  HREC_REQUIRE(n_rows < 65536, "%s: at most 65535 rows per call", who);
  HREC_REQUIRE(top_k >= 1 && top_k <= 1024, "%s: top_k must be in [1, 1024]", who);
  HREC_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 or 1", who);
  const bool any_excl = excl_rows || excl_indptr || excl_cols;
  HREC_REQUIRE(!any_excl || (excl_rows && excl_indptr && excl_cols),
               "%s: the exclusion CSR needs excl_rows, excl_indptr and excl_cols (or none of them)", who);
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(als && tt && out_idx && out_val && out_len && overflow && workspace && (row_wins || !rowwise),
               "%s: null pointer", who);
  const size_t need = hrec_hybrid_lists_workspace_bytes(n_rows, n, top_k, mode);
  HREC_REQUIRE(workspace_bytes >= need, "%s: workspace %zu < %zu", who, workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const int kk = (int)(top_k < n ? top_k : n);
  const HlWs w = hl_layout(workspace, n_rows, n, kk, mode);
  const int vec4 = (ld % 4 == 0) && (((reinterpret_cast<uintptr_t>(als) | reinterpret_cast<uintptr_t>(tt)) & 15) == 0);
  hipLaunchKernelGGL(hl_extremes_kernel, dim3((unsigned)n_rows), dim3(1024), 0, s, als, tt, n, ld, vec4, als_fallback,
                     excl_rows, excl_indptr, excl_cols, kk, w.coef, out_minmax, out_len, w.cnt, overflow);
  int rc = check_launch("hl_extremes_kernel");
  if (rc) return rc;
  const int64_t segs = (n + kHlSeg - 1) / kHlSeg;
  const dim3 gp((unsigned)((segs + 3) / 4), (unsigned)n_rows);
  if (mode == 1) {
    hipLaunchKernelGGL(hl_pass_kernel<1>, gp, dim3(256), 0, s, als, tt, n, ld, segs, als_fallback, excl_rows,
                       excl_indptr, excl_cols, w.coef, row_wins, als_wins, (const uint64_t*)nullptr, n, w.v, w.i,
                       w.cnt);
    rc = check_launch("hl_pass_kernel (full)");
    if (rc) return rc;
    return topk_rows<double>(w.v, n_rows, n, n, kk, out_idx, out_val, w.tws, (size_t)1 << 62, s, w.i);
  }
  const bool sampled = n > kHlSample;  // else the whole row is the sample: every live column goes to the list
  if (sampled) {
    hipLaunchKernelGGL(hl_bound_kernel, dim3((unsigned)n_rows), dim3(kHlBoundBlock), 0, s, als, tt, ld, als_fallback,
                       excl_rows, excl_indptr, excl_cols, w.coef, row_wins, als_wins, kk, w.bound);
    rc = check_launch("hl_bound_kernel");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(hl_pass_kernel<0>, gp, dim3(256), 0, s, als, tt, n, ld, segs, als_fallback, excl_rows,
                     excl_indptr, excl_cols, w.coef, row_wins, als_wins,
                     sampled ? (const uint64_t*)w.bound : nullptr, w.L, w.v, w.i, w.cnt);
  rc = check_launch("hl_pass_kernel (bounded)");
  if (rc) return rc;
  rc = count_overflow(w.cnt, (int)n_rows, (int)w.L, overflow, s);
  if (rc) return rc;
  return topk_rows<double>(w.v, n_rows, w.L, w.L, kk, out_idx, out_val, w.tws, (size_t)1 << 62, s, w.i, w.cnt);
}

extern "C" int hrec_hybrid_lists(const float* als, const float* tt, int64_t n_rows, int64_t n, int64_t ld,
                                 const double* als_fallback, int als_wins, int top_k, int mode,
                                 const int64_t* excl_rows, const int64_t* excl_indptr, const int32_t* excl_cols,
                                 int64_t* out_idx, double* out_val, int32_t* out_len, double* out_minmax,
                                 int* overflow, void* workspace, size_t workspace_bytes, void* stream) {
  return hl_run("hybrid_lists", false, als, tt, n_rows, n, ld, als_fallback, nullptr, als_wins, top_k, mode, excl_rows,
                excl_indptr, excl_cols, out_idx, out_val, out_len, out_minmax, overflow, workspace, workspace_bytes,
                stream);
}

extern "C" int hrec_hybrid_lists_rowwise(const float* als, const float* tt, int64_t n_rows, int64_t n, int64_t ld,
                                         const double* als_fallback, const int32_t* row_wins, int top_k, int mode,
                                         const int64_t* excl_rows, const int64_t* excl_indptr,
                                         const int32_t* excl_cols, int64_t* out_idx, double* out_val,
                                         int32_t* out_len, double* out_minmax, int* overflow, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  return hl_run("hybrid_lists_rowwise", true, als, tt, n_rows, n, ld, als_fallback, row_wins, 0, top_k, mode,
                excl_rows, excl_indptr, excl_cols, out_idx, out_val, out_len, out_minmax, overflow, workspace,
                workspace_bytes, stream);
}
