// Generic stable top-k (the reference's sorted(..., reverse=True)[:k]): kk
// rounds of arg-best over segments held in registers, or one wave per row
// with per-lane sorted lists; the order is better() of order.h.
// Larger top_k than kTopkSelectMax: the sort path (csrc/sort_topk.hip).
#include "order.h"  // better, KV, wave_best

namespace hrec {

constexpr int kTopkBlock = 256;
constexpr int kTopkPer = 16;  // elements per thread per segment
constexpr int kTopkSeg = kTopkBlock * kTopkPer;

// Stage 1: rows x segments; each block selects the top `kk` of its segment
// of one row by kk rounds of block arg-best over elements held in registers.
// `src_idx` (optional) maps positions to original indices (stage 2 input).
template <typename T>
__global__ __launch_bounds__(kTopkBlock) void topk_segment_kernel(const T* __restrict__ vals,
                                                                  const int64_t* __restrict__ src_idx,
                                                                  const int* __restrict__ row_n,
                                                                  int64_t n, int64_t row_stride, int kk,
                                                                  T* __restrict__ out_v,
                                                                  int64_t* __restrict__ out_i,
                                                                  int64_t out_row_stride,
                                                                  const int* __restrict__ gate) {
  __shared__ KV<T> red[kTopkBlock / 64];
  __shared__ int64_t win;
  if (gate && *gate == 0) return;
  const int64_t row = blockIdx.y;
  const int64_t seg0 = (int64_t)blockIdx.x * kTopkSeg;
  const T* __restrict__ rv = vals + row * row_stride;
  const int64_t* __restrict__ ri = src_idx ? src_idx + row * row_stride : nullptr;
  if (row_n) {
    const int64_t rn = row_n[row];
    n = rn < n ? rn : n;
  }
  T v[kTopkPer];
  int64_t id[kTopkPer];
#pragma unroll
  for (int e = 0; e < kTopkPer; ++e) {
    const int64_t p = seg0 + (int64_t)e * kTopkBlock + threadIdx.x;
    if (p < n) {
      v[e] = rv[p];
      id[e] = ri ? ri[p] : p;
    } else {
      v[e] = 0;
      id[e] = -1;
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r = 0; r < kk; ++r) {
    KV<T> best{(T)0, -1};
#pragma unroll
    for (int e = 0; e < kTopkPer; ++e) {
      if (id[e] >= 0 && (best.i < 0 || better(v[e], id[e], best.v, best.i))) best = KV<T>{v[e], id[e]};
    }
    if (best.i < 0) best.i = INT64_MAX;
    KV<T> wb = wave_best(best);
    if (lane == 0) red[w] = wb;
    __syncthreads();
    if (threadIdx.x == 0) {
      KV<T> b = red[0];
      for (int q = 1; q < kTopkBlock / 64; ++q) {
        if (red[q].i == INT64_MAX) continue;
        if (b.i == INT64_MAX || better(red[q].v, red[q].i, b.v, b.i)) b = red[q];
      }
      const int64_t o = row * out_row_stride + (int64_t)blockIdx.x * kk + r;
      out_v[o] = b.v;
      out_i[o] = b.i == INT64_MAX ? -1 : b.i;
      win = b.i;
    }
    __syncthreads();
    const int64_t wi = win;
#pragma unroll
    for (int e = 0; e < kTopkPer; ++e)
      if (id[e] == wi) id[e] = -1;
    __syncthreads();
  }
}

// Small top-k (kk <= 16) of rows of at most kTopkWaveMax elements: one wave
// per row. Each lane streams its elements (p = lane, lane + 64, ...) through a
// sorted register list of its KK best (a compare-exchange chain, no
// branches), then kk rounds of wave arg-best over the list heads, the winner
// popping its head. Same order, same output as topk_segment_kernel, without
// its block barriers.
constexpr int kTopkWaveMax = 8192;

template <typename T, int KK>
__global__ __launch_bounds__(256) void topk_wave_kernel(const T* __restrict__ vals,
                                                        const int64_t* __restrict__ src_idx,
                                                        const int* __restrict__ row_n, int64_t n_rows, int64_t n,
                                                        int64_t row_stride, int kk, T* __restrict__ out_v,
                                                        int64_t* __restrict__ out_i, int64_t out_row_stride,
                                                        const int* __restrict__ gate) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows || (gate && *gate == 0)) return;  // wave-uniform
  if (row_n) {
    const int64_t rn = row_n[row];
    n = rn < n ? rn : n;
  }
  const T* __restrict__ rv = vals + row * row_stride;
  const int64_t* __restrict__ ri = src_idx ? src_idx + row * row_stride : nullptr;
  T lv[KK];
  int64_t li[KK];
#pragma unroll
  for (int j = 0; j < KK; ++j) {
    lv[j] = (T)0;
    li[j] = INT64_MAX;  // empty slot: loses to every element
  }
  constexpr int B = 8;  // loads in flight per lane before the first insertion
  for (int64_t p0 = lane; p0 < n; p0 += 64 * B) {
    T bv[B];
    int64_t bi[B];
#pragma unroll
    for (int e = 0; e < B; ++e) {
      const int64_t p = p0 + 64 * e;
      const bool in = p < n;
      bv[e] = in ? rv[p] : (T)0;
      bi[e] = in ? (ri ? ri[p] : p) : -1;
    }
#pragma unroll
    for (int e = 0; e < B; ++e) {
      T xv = bv[e];
      int64_t xi = bi[e] < 0 ? INT64_MAX : bi[e];  // absent: an empty slot, inserts as a no-op
#pragma unroll
      for (int j = 0; j < KK; ++j) {
        const bool sw = xi != INT64_MAX && (li[j] == INT64_MAX || better(xv, xi, lv[j], li[j]));
        const T tv = lv[j];
        const int64_t ti = li[j];
        lv[j] = sw ? xv : tv;
        li[j] = sw ? xi : ti;
        xv = sw ? tv : xv;
        xi = sw ? ti : xi;
      }
    }
  }
  for (int r = 0; r < kk; ++r) {
    const KV<T> w = wave_best(KV<T>{lv[0], li[0]});
    if (lane == 0) {
      const int64_t o = row * out_row_stride + r;
      out_v[o] = w.i == INT64_MAX ? (T)0 : w.v;
      out_i[o] = w.i == INT64_MAX ? -1 : w.i;
    }
    if (w.i != INT64_MAX && li[0] == w.i) {  // the (unique) owner pops its head
#pragma unroll
      for (int j = 0; j + 1 < KK; ++j) {
        lv[j] = lv[j + 1];
        li[j] = li[j + 1];
      }
      li[KK - 1] = INT64_MAX;
    }
  }
}

// Workspace for a stable top-k of n_rows rows of n elements (bytes) by the
// segment selections (kk <= kTopkSelectMax). Each pass keeps kk of every
// kTopkSeg elements, so it shrinks the row only while kk < kTopkSeg / 2; the
// loop stops as soon as a pass would not shrink it (larger kk go through the
// sort path, csrc/sort_topk.hip).
size_t topk_ws_bytes(int64_t n_rows, int64_t n, int kk, size_t elem) {
  size_t total = 0;
  int64_t m = n;
  if (kk < 1 || kk > kTopkSelectMax) return 256;
  while (true) {
    const int64_t segs = (m + kTopkSeg - 1) / kTopkSeg;
    if (segs <= 1) break;
    const int64_t cand = segs * kk;
    if (cand >= m) break;
    total += (size_t)n_rows * (size_t)cand * (elem + 8);
    m = cand;
  }
  return total + 256;
}

template <typename T>
int topk_rows(const T* vals, int64_t n_rows, int64_t n, int64_t row_stride, int kk, int64_t* out_idx,
              T* out_val, void* ws, size_t ws_bytes, hipStream_t s, const int64_t* src_idx, const int* row_n,
              const int* gate) {
  // Multi-pass: segments -> candidates (kk per segment) -> ... -> one segment.
  const T* cur_v = vals;
  const int64_t* cur_i = src_idx;
  int64_t m = n, stride = row_stride;
  char* w = (char*)ws;
  size_t used = 0;
  while (true) {
    const int64_t segs = (m + kTopkSeg - 1) / kTopkSeg;
    if (segs <= 1 || (m <= kTopkWaveMax && kk <= 16)) {
      if (kk <= 16 && m <= kTopkWaveMax) {
        const dim3 g((unsigned)((n_rows + 3) / 4));
#define HREC_TOPK_WAVE(KK)                                                                                    \
  hipLaunchKernelGGL((topk_wave_kernel<T, KK>), g, dim3(256), 0, s, cur_v, cur_i, row_n, n_rows, m, stride, kk, \
                     out_val, out_idx, (int64_t)kk, gate)
        if (kk <= 2)
          HREC_TOPK_WAVE(2);
        else if (kk <= 4)
          HREC_TOPK_WAVE(4);
        else if (kk == 5)  // the reference's default top_k: 5-deep lane lists
          HREC_TOPK_WAVE(5);
        else if (kk <= 8)
          HREC_TOPK_WAVE(8);
        else
          HREC_TOPK_WAVE(16);
#undef HREC_TOPK_WAVE
        return check_launch("topk_wave_kernel");
      }
      hipLaunchKernelGGL((topk_segment_kernel<T>), dim3(1, (unsigned)n_rows), dim3(kTopkBlock), 0, s, cur_v,
                         cur_i, row_n, m, stride, kk, out_val, out_idx, (int64_t)kk, gate);
      return check_launch("topk_segment_kernel");
    }
    const int64_t cand = segs * kk;
    const size_t vb = (size_t)n_rows * cand * sizeof(T), ib = (size_t)n_rows * cand * 8;
    if (used + vb + ib > ws_bytes) {
      set_error("topk: workspace too small");
      return HREC_E_INVALID;
    }
    int64_t* ni = (int64_t*)(w + used);
    T* nv = (T*)(w + used + ib);
    used += vb + ib;
    hipLaunchKernelGGL((topk_segment_kernel<T>), dim3((unsigned)segs, (unsigned)n_rows), dim3(kTopkBlock), 0, s,
                       cur_v, cur_i, row_n, m, stride, kk, nv, ni, cand, gate);
    int rc = check_launch("topk_segment_kernel");
    if (rc) return rc;
    cur_v = nv;
    cur_i = ni;
    row_n = nullptr;  // later passes: every row holds segs * kk entries
    m = cand;
    stride = cand;
  }
}
template int topk_rows<float>(const float*, int64_t, int64_t, int64_t, int, int64_t*, float*, void*, size_t,
                              hipStream_t, const int64_t*, const int*, const int*);
template int topk_rows<double>(const double*, int64_t, int64_t, int64_t, int, int64_t*, double*, void*, size_t,
                               hipStream_t, const int64_t*, const int*, const int*);
}  // namespace hrec

using namespace hrec;

extern "C" size_t hrec_topk_workspace_bytes(int64_t n_rows, int64_t n, int top_k, int is_f64) {
  const int64_t kk = top_k < n ? top_k : n;
  if (kk > kTopkSelectMax) return sort_topk_ws_bytes(n_rows, n);
  return topk_ws_bytes(n_rows, n, (int)kk, is_f64 ? 8 : 4);
}

extern "C" int hrec_topk_f32(const float* vals, int64_t n_rows, int64_t n, int64_t row_stride, int top_k,
                             int64_t* out_idx, float* out_val, void* workspace, size_t workspace_bytes,
                             void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 0 && row_stride >= n, "topk_f32: bad shape");
  HREC_REQUIRE(top_k >= 1, "topk_f32: top_k must be >= 1");
  if (n_rows == 0 || n == 0) return HREC_OK;
  HREC_REQUIRE(n_rows < 65536, "topk_f32: at most 65535 rows per call");
  HREC_REQUIRE(vals && out_idx && out_val, "topk_f32: null pointer");
  const int kk = (int)(top_k < n ? top_k : n);
  if (kk > kTopkSelectMax)
    return sort_topk_rows<float>(vals, n_rows, n, row_stride, kk, out_idx, out_val, workspace, workspace_bytes,
                                as_stream(stream));
  return topk_rows<float>(vals, n_rows, n, row_stride, kk, out_idx, out_val, workspace, workspace_bytes,
                          as_stream(stream));
}

extern "C" int hrec_topk_f64(const double* vals, int64_t n_rows, int64_t n, int64_t row_stride, int top_k,
                             int64_t* out_idx, double* out_val, void* workspace, size_t workspace_bytes,
                             void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 0 && row_stride >= n, "topk_f64: bad shape");
  HREC_REQUIRE(top_k >= 1, "topk_f64: top_k must be >= 1");
  if (n_rows == 0 || n == 0) return HREC_OK;
  HREC_REQUIRE(n_rows < 65536, "topk_f64: at most 65535 rows per call");
  HREC_REQUIRE(vals && out_idx && out_val, "topk_f64: null pointer");
  const int kk = (int)(top_k < n ? top_k : n);
  if (kk > kTopkSelectMax)
    return sort_topk_rows<double>(vals, n_rows, n, row_stride, kk, out_idx, out_val, workspace, workspace_bytes,
                                as_stream(stream));
  return topk_rows<double>(vals, n_rows, n, row_stride, kk, out_idx, out_val, workspace, workspace_bytes,
                           as_stream(stream));
}

extern "C" int hrec_topk_f64_keyed(const double* vals, const int64_t* keys, int64_t n_rows, int64_t n, int top_k,
                                   int64_t* out_idx, double* out_val, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 0, "topk_f64_keyed: bad shape");
  HREC_REQUIRE(top_k >= 1 && top_k <= 1024, "topk_f64_keyed: top_k must be in [1, 1024]");
  if (n_rows == 0 || n == 0) return HREC_OK;
  HREC_REQUIRE(n_rows < 65536, "topk_f64_keyed: at most 65535 rows per call");
  HREC_REQUIRE(vals && keys && out_idx && out_val, "topk_f64_keyed: null pointer");
  const int kk = (int)(top_k < n ? top_k : n);
  HREC_REQUIRE(workspace_bytes >= topk_ws_bytes(n_rows, n, kk, 8), "topk_f64_keyed: workspace too small");
  return topk_rows<double>(vals, n_rows, n, n, kk, out_idx, out_val, workspace, workspace_bytes, as_stream(stream),
                           keys);
}
