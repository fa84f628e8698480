// Per-row, per-model F1@k (hrec_hybrid_model_f1): for every row of the two f32
// score matrices hrec_hybrid_lists fuses, each model's own stable descending
// top-min(k, n) (ALS keys: hl_als' f64 values, two-tower keys: the f32 scores
// widened, which keeps their order, ties and NaNs) and compute_f1_score's
// arithmetic of that selection against the row's label set -> the two F1s and
// the row's fusion choice f1_als > f1_tt (hrec_hybrid_lists_rowwise's row_wins).
//   1. mode 0, n > kHlSample: hf_bound_kernel takes, per model, the kk-th best
//      key of the row's first kHlSample columns — kk columns reach it, so the
//      selection's kk-th key does and every selected column passes `key >=
//      bound`; hf_pass_kernel<0> reads both matrices once (16-byte loads where
//      the rows are aligned) and appends each model's passing columns to that
//      model's list of the row, one slot reservation per wave and model;
//      topk_rows ranks the lists by (value, column). n <= kHlSample: the whole
//      row is the list.
//   2. mode 1: hf_pass_kernel<1> writes both key rows whole and topk_rows
//      ranks them.
//   3. hf_finish_kernel: the labels found in each selection (a binary search
//      in the row's ascending label columns), the F1s, out_wins, out_top.
// Buffers of the two models are model-major: [2][n_rows][...], ALS first.
#include "exclusion.h"
#include "hybrid_common.h"

namespace hrec {

// One block per row (n > kHlSample): per model the largest T with at least kk
// sample keys >= T, by a search over the key bits (hl_bound_kernel's, with one
// counter per model and bit). Keys are >= 1 (NaN), so T >= 1.
__global__ __launch_bounds__(kHlBoundBlock) void hf_bound_kernel(const float* __restrict__ als,
                                                                 const float* __restrict__ tt, int64_t ld,
                                                                 const double* __restrict__ fb, int kk,
                                                                 int64_t n_rows, uint64_t* __restrict__ bound) {
  __shared__ int cn[2][64];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < 128) cn[tid >> 6][tid & 63] = 0;
  __syncthreads();
  uint64_t ka[kHlBoundPer], kt[kHlBoundPer];
#pragma unroll
  for (int e = 0; e < kHlBoundPer; ++e) {
    const int j = e * kHlBoundBlock + tid;
    ka[e] = hl_key(hl_als(als[r * ld + j], fb, j));
    kt[e] = hl_key((double)tt[r * ld + j]);
  }
  uint64_t Ta = 0, Tt = 0;
  for (int b = 63; b >= 0; --b) {
    const uint64_t ca = Ta | (1ull << b), ct = Tt | (1ull << b);
    int na = 0, nt = 0;
#pragma unroll
    for (int e = 0; e < kHlBoundPer; ++e) {
      na += ka[e] >= ca ? 1 : 0;
      nt += kt[e] >= ct ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      na += __shfl_xor(na, off, kWave);
      nt += __shfl_xor(nt, off, kWave);
    }
    if ((tid & 63) == 0) {
      atomicAdd(&cn[0][b], na);
      atomicAdd(&cn[1][b], nt);
    }
    __syncthreads();
    if (cn[0][b] >= kk) Ta = ca;  // block-uniform
    if (cn[1][b] >= kk) Tt = ct;
  }
  if (tid == 0) {
    bound[r] = Ta;
    bound[n_rows + r] = Tt;
  }
}

// A lane's register slot q (0 .. kHlPer - 1) holds segment position hf_pos<VEC>(q, lane):
// VEC 1: q * 64 + lane (4-byte loads, any alignment); VEC 4: four consecutive
// columns per 16-byte load (rows 16-byte aligned: ld % 4 == 0, aligned bases).
template <int VEC>
__device__ __forceinline__ int hf_pos(int q, int lane) {
  return VEC == 4 ? ((q >> 2) * 64 + lane) * 4 + (q & 3) : q * 64 + lane;
}

// The lanes' slots set in `mask` go to list `list` of L entries as (val(q),
// column): one reservation per wave on the list's counter (an inclusive scan
// of the lanes' counts), which counts them all, so cnt[list] > L tells an
// overflow. Wave-uniform call.
template <int VEC, typename F>
__device__ __forceinline__ void hf_flush(uint32_t mask, int lane, int64_t seg0, int64_t list, int64_t L,
                                         double* __restrict__ out_v, int64_t* __restrict__ out_i,
                                         int* __restrict__ cnt, F&& val) {
  if (__ballot(mask != 0) == 0) return;  // wave-uniform
  const int mine = __popc(mask);
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, kWave);
    if (lane >= off) incl += up;
  }
  const int total = __shfl(incl, 63, kWave);
  int base = 0;
  if (lane == 0) base = atomicAdd(&cnt[list], total);
  base = __builtin_amdgcn_readfirstlane(base);
  int64_t slot = (int64_t)base + incl - mine;
#pragma unroll
  for (int q = 0; q < kHlPer; ++q) {
    if ((mask >> q) & 1u) {
      if (slot < L) {
        out_v[list * L + slot] = val(q);
        out_i[list * L + slot] = seg0 + hf_pos<VEC>(q, lane);
      }
      ++slot;
    }
  }
}

// One wave per segment of kHlSeg contiguous columns of one row, both models
// from one read of the two matrices:
//   MODE 0: each model's columns whose key reaches that model's bound of the
//           row (null: every column) go to its list (hf_flush);
//   MODE 1: write both key rows to out_v[2][n_rows][n].
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void hf_pass_kernel(const float* __restrict__ als, const float* __restrict__ tt,
                                                      int64_t n, int64_t ld, int64_t segs,
                                                      const double* __restrict__ fb, int64_t n_rows,
                                                      const uint64_t* __restrict__ bound, int64_t L,
                                                      double* __restrict__ out_v, int64_t* __restrict__ out_i,
                                                      int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t seg = (int64_t)blockIdx.x * 4 + wv;
  if (seg >= segs) return;  // wave-uniform; no block barrier below
  const int64_t r = blockIdx.y;
  const int64_t seg0 = seg * kHlSeg;
  const int nvalid = (int)((n - seg0) < kHlSeg ? (n - seg0) : kHlSeg);
  const uint64_t ba = (MODE == 0 && bound) ? bound[r] : 0ull;
  const uint64_t bt = (MODE == 0 && bound) ? bound[n_rows + r] : 0ull;
  const float* ar = als + r * ld + seg0;
  const float* tr = tt + r * ld + seg0;
  float av[kHlPer], tv[kHlPer];
  if (VEC == 4) {
#pragma unroll
    for (int g = 0; g < kHlPer / 4; ++g) {
      const int p = (g * 64 + lane) * 4;
      if (p + 3 < nvalid) {
        const float4 a = reinterpret_cast<const float4*>(ar)[g * 64 + lane];
        const float4 t = reinterpret_cast<const float4*>(tr)[g * 64 + lane];
        av[4 * g] = a.x, av[4 * g + 1] = a.y, av[4 * g + 2] = a.z, av[4 * g + 3] = a.w;
        tv[4 * g] = t.x, tv[4 * g + 1] = t.y, tv[4 * g + 2] = t.z, tv[4 * g + 3] = t.w;
      } else {  // the row's last columns
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool v = p + c < nvalid;
          av[4 * g + c] = v ? ar[p + c] : 0.0f;
          tv[4 * g + c] = v ? tr[p + c] : 0.0f;
        }
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < kHlPer; ++e) {
      const bool v = e * 64 + lane < nvalid;
      av[e] = v ? ar[e * 64 + lane] : 0.0f;
      tv[e] = v ? tr[e * 64 + lane] : 0.0f;
    }
  }
  auto a_of = [&](int q) {  // the substituted ALS key value of a valid slot
    return hl_als(av[q], fb, seg0 + hf_pos<VEC>(q, lane));
  };
  uint32_t ma = 0, mt = 0;
#pragma unroll
  for (int q = 0; q < kHlPer; ++q) {
    const int pos = hf_pos<VEC>(q, lane);
    if (pos >= nvalid) continue;
    const double a = a_of(q);
    const double t = (double)tv[q];
    if (MODE == 1) {
      out_v[r * n + seg0 + pos] = a;
      out_v[(n_rows + r) * n + seg0 + pos] = t;
    } else {
      ma |= (hl_key(a) >= ba ? 1u : 0u) << q;
      mt |= (hl_key(t) >= bt ? 1u : 0u) << q;
    }
  }
  if (MODE == 0) {
    hf_flush<VEC>(ma, lane, seg0, r, L, out_v, out_i, cnt, a_of);
    hf_flush<VEC>(mt, lane, seg0, n_rows + r, L, out_v, out_i, cnt, [&](int q) { return (double)tv[q]; });
  }
}

// compute_f1_score's arithmetic on tp hits of a selection of k against a set
// of `total` items (src/als_model.py: precision = tp / k, recall = tp /
// len(actual), 2 * (p * r) / (p + r) or 0), in f64, unfused.
__device__ __forceinline__ double hf_f1(int tp, int k, int total) {
#pragma clang fp contract(off)
  const double p = (double)tp / (double)k;
  const double r = (double)tp / (double)total;
  const double s = p + r;
  return s > 0.0 ? 2.0 * (p * r) / s : 0.0;
}

// One wave per row: the row's labels found in each model's selection top_i[2][n_rows][kk],
// the two F1s and the choice; out_top (optional) gets the selections.
__global__ __launch_bounds__(256) void hf_finish_kernel(const int64_t* __restrict__ top_i, int64_t n_rows, int kk,
                                                        int k, const int64_t* __restrict__ label_rows,
                                                        const int64_t* __restrict__ label_indptr,
                                                        const int32_t* __restrict__ label_cols,
                                                        const int32_t* __restrict__ label_total, int default_wins,
                                                        double* __restrict__ out_f1, int32_t* __restrict__ out_wins,
                                                        int64_t* __restrict__ out_top) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;  // wave-uniform
  const int64_t q = label_rows ? label_rows[row] : -1;
  const ExclSeg x = excl_segment(label_indptr, q);
  const int total = q >= 0 ? label_total[q] : 0;
  int tp[2] = {0, 0};
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int64_t* sel = top_i + ((int64_t)m * n_rows + row) * kk;
    for (int p = lane; p < kk; p += 64) {
      const int64_t c = sel[p];
      if (out_top) out_top[(row * 2 + m) * kk + p] = c;
      tp[m] += (c >= 0 && excl_contains(label_cols, x.lo, x.hi, c)) ? 1 : 0;
    }
#pragma unroll  // written out: wave_xor_sum here changes the generated code
    for (int off = 32; off > 0; off >>= 1) tp[m] += __shfl_xor(tp[m], off, kWave);
  }
  if (lane != 0) return;
  if (total <= 0) {  // no ground truth: the instance's choice, no F1
    out_f1[2 * row] = out_f1[2 * row + 1] = __builtin_nan("");
    out_wins[row] = default_wins ? 1 : 0;
    return;
  }
  const double fa = hf_f1(tp[0], k, total), ft = hf_f1(tp[1], k, total);
  out_f1[2 * row] = fa;
  out_f1[2 * row + 1] = ft;
  out_wins[row] = fa > ft ? 1 : 0;
}

}  // namespace hrec

using namespace hrec;

// Workspace of hrec_hybrid_model_f1, in carve order.
struct HfWs {
  uint64_t* bound;  // [2][n_rows] mode 0
  int* cnt;         // [2][n_rows] mode 0: columns that passed the bound
  double* v;        // mode 0: [2][n_rows][L] lists; mode 1: [2][n_rows][n]
  int64_t* i;       // mode 0: the lists' columns
  int64_t* top_i;   // [2][n_rows][kk]
  double* top_v;
  char* tws;
  int64_t L;
  size_t total;
};

static HfWs hf_layout(void* base, int64_t n_rows, int64_t n, int kk, int mode) {
  HfWs w{};
  Carver c(base);
  w.L = mode == 0 ? (n < kHlCap ? n : kHlCap) : n;
  w.bound = (uint64_t*)c.take((size_t)2 * n_rows * 8);
  w.cnt = (int*)c.take((size_t)2 * n_rows * 4);
  w.v = (double*)c.take((size_t)2 * n_rows * w.L * 8);
  w.i = (int64_t*)c.take(mode == 0 ? (size_t)2 * n_rows * w.L * 8 : 0);
  w.top_i = (int64_t*)c.take((size_t)2 * n_rows * kk * 8);
  w.top_v = (double*)c.take((size_t)2 * n_rows * kk * 8);
  w.tws = c.take(topk_ws_bytes(n_rows, w.L, kk, 8));
  w.total = c.total();
  return w;
}

static int hf_kk(int64_t n, int k) {
  const int kc = k < 1 ? 1 : (k > kTopkSelectMax ? kTopkSelectMax : k);
  return (int)(kc < n ? kc : n);
}

extern "C" size_t hrec_hybrid_model_f1_workspace_bytes(int64_t n_rows, int64_t n, int k, int mode) {
  n_rows = n_rows > 0 ? n_rows : 0;
  n = n > 0 ? n : 0;
  return hf_layout(nullptr, n_rows, n, hf_kk(n, k), mode == 1 ? 1 : 0).total;
}

extern "C" int hrec_hybrid_model_f1(const float* als, const float* tt, int64_t n_rows, int64_t n, int64_t ld,
                                    const double* als_fallback, int k, int mode, const int64_t* label_rows,
                                    const int64_t* label_indptr, const int32_t* label_cols,
                                    const int32_t* label_total, int default_wins, double* out_f1, int32_t* out_wins,
                                    int64_t* out_top, int* overflow, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 1, "hybrid_model_f1: bad shape");
  HREC_REQUIRE(ld >= n, "hybrid_model_f1: ld must be >= n");
  HREC_REQUIRE(n_rows < 65536, "hybrid_model_f1: at most 65535 rows per call");
  HREC_REQUIRE(k >= 1 && k <= 1024, "hybrid_model_f1: k must be in [1, 1024]");
  HREC_REQUIRE(mode == 0 || mode == 1, "hybrid_model_f1: mode must be 0 or 1");
  const bool any_label = label_rows || label_indptr || label_cols || label_total;
  HREC_REQUIRE(!any_label || (label_rows && label_indptr && label_cols && label_total),
               "hybrid_model_f1: the label CSR needs label_rows, label_indptr, label_cols and label_total (or none "
               "of them)");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(als && tt && out_f1 && out_wins && overflow && workspace, "hybrid_model_f1: null pointer");
  const size_t need = hrec_hybrid_model_f1_workspace_bytes(n_rows, n, k, mode);
  HREC_REQUIRE(workspace_bytes >= need, "hybrid_model_f1: workspace %zu < %zu", workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const int kk = hf_kk(n, k);
  const HfWs w = hf_layout(workspace, n_rows, n, kk, mode);
  if (hipMemsetAsync(overflow, 0, sizeof(int), s) != hipSuccess ||
      hipMemsetAsync(w.cnt, 0, (size_t)2 * n_rows * 4, s) != hipSuccess)
    return check_launch("hybrid_model_f1: memset");
  int rc;
  const int64_t segs = (n + kHlSeg - 1) / kHlSeg;
  const dim3 gp((unsigned)((segs + 3) / 4), (unsigned)n_rows);
  const size_t tws_bytes = (size_t)1 << 62;
  // 16-byte loads where every row starts on a 16-byte boundary (segments start at multiples of kHlSeg columns)
  const bool vec4 = (ld % 4 == 0) && (((reinterpret_cast<uintptr_t>(als) | reinterpret_cast<uintptr_t>(tt)) & 15) == 0);
  if (mode == 1) {
    hipLaunchKernelGGL((vec4 ? hf_pass_kernel<1, 4> : hf_pass_kernel<1, 1>), gp, dim3(256), 0, s, als, tt, n, ld,
                       segs, als_fallback, n_rows, (const uint64_t*)nullptr, n, w.v, (int64_t*)nullptr, w.cnt);
    rc = check_launch("hf_pass_kernel (full)");
    if (rc) return rc;
    for (int m = 0; m < 2; ++m) {
      rc = topk_rows<double>(w.v + (size_t)m * n_rows * n, n_rows, n, n, kk, w.top_i + (size_t)m * n_rows * kk,
                             w.top_v + (size_t)m * n_rows * kk, w.tws, tws_bytes, s);
      if (rc) return rc;
    }
  } else {
    const bool sampled = n > kHlSample;  // else the whole row is the sample: every column goes to both lists
    if (sampled) {
      hipLaunchKernelGGL(hf_bound_kernel, dim3((unsigned)n_rows), dim3(kHlBoundBlock), 0, s, als, tt, ld,
                         als_fallback, kk, n_rows, w.bound);
      rc = check_launch("hf_bound_kernel");
      if (rc) return rc;
    }
    hipLaunchKernelGGL((vec4 ? hf_pass_kernel<0, 4> : hf_pass_kernel<0, 1>), gp, dim3(256), 0, s, als, tt, n, ld,
                       segs, als_fallback, n_rows, sampled ? (const uint64_t*)w.bound : nullptr, w.L, w.v, w.i,
                       w.cnt);
    rc = check_launch("hf_pass_kernel (bounded)");
    if (rc) return rc;
    rc = count_overflow(w.cnt, (int)(2 * n_rows), (int)w.L, overflow, s);
    if (rc) return rc;
    for (int m = 0; m < 2; ++m) {
      const size_t o = (size_t)m * n_rows * w.L;
      rc = topk_rows<double>(w.v + o, n_rows, w.L, w.L, kk, w.top_i + (size_t)m * n_rows * kk,
                             w.top_v + (size_t)m * n_rows * kk, w.tws, tws_bytes, s, w.i + o, w.cnt + m * n_rows);
      if (rc) return rc;
    }
  }
  hipLaunchKernelGGL(hf_finish_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, w.top_i, n_rows, kk, k,
                     label_rows, label_indptr, label_cols, label_total, default_wins, out_f1, out_wins, out_top);
  return check_launch("hf_finish_kernel");
}
