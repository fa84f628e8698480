// The host steps of the sample-bound top-k cascades (csrc/cascade.h) and the lane-maxima bound kernel.
#include "cascade.h"

namespace hrec {

// Survivor threshold from a sample row (one wave per row, kk <= 64): the
// kk-th largest of the 64 lane maxima (lane l: elements l, l + 64, ...), kk
// distinct sample elements, so a lower bound of the row's kk-th best. NaN
// elements are ignored (fmaxf); a row without a number yields -inf.
__global__ __launch_bounds__(256) void sample_threshold_kernel(const float* __restrict__ vals, int64_t n_rows,
                                                               int64_t n, int kk, float* __restrict__ thr,
                                                               int* __restrict__ zero_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;  // wave-uniform
  const float* __restrict__ rv = vals + row * n;
  float m = -__builtin_inff();
  int64_t p = lane;
  for (; p + 64 * 3 < n; p += 64 * 4) {  // four loads in flight per lane
    const float a = rv[p], b = rv[p + 64], c = rv[p + 128], d = rv[p + 192];
    m = fmaxf(m, fmaxf(fmaxf(a, b), fmaxf(c, d)));
  }
  for (; p < n; p += 64) m = fmaxf(m, rv[p]);
  const float t = kth_of_lane_maxima(m, kk, lane);
  if (lane == 0) {
    thr[row] = t;
    if (zero_cnt) zero_cnt[row] = 0;
  }
}

CascadeWs cascade_carve(Carver& c, int B, int64_t S, int64_t cap, int kk, size_t cn_pad) {
  CascadeWs w{};
  w.samp = (float*)c.take((size_t)B * S * 4);
  w.tws = c.take(topk_ws_bytes(B, S, kk, 4));
  w.sv = (float*)c.take((size_t)B * kk * 4);
  w.si = (int64_t*)c.take((size_t)B * kk * 8);
  w.cv = (float*)c.take((size_t)B * cap * 4);
  w.ci = (int64_t*)c.take((size_t)B * cap * 8);
  w.cn = (int*)c.take((size_t)B * 4 + cn_pad);
  w.fws = c.take(topk_ws_bytes(B, cap, kk, 4));
  return w;
}

int cascade_rank_all(const CascadeWs& w, int n_users, int64_t n_items, int kk, const Excl& x, int64_t* out_idx,
                     float* out_val, hipStream_t s) {
  const float nan = __builtin_nanf("");
  const int rc = x.on ? excl_mask_run(w.samp, n_users, n_items, n_items, 1, n_items, x, nan, kk, x.out_len, s) : 0;
  if (rc) return rc;
  return topk_rows<float>(w.samp, n_users, n_items, n_items, kk, out_idx, out_val, w.tws, (size_t)1 << 62, s);
}

// Why a sample bound is sound. The sample is S of the call's items (column c
// holds item c * step) under the filter's own scoring. Its kk-th best t_b is
// reached by kk distinct items, so the kk-th best of all items is >= t_b:
// every entry of the answer passes a filter at t_b (or at any lower bound of
// it: the lane-maxima form), and the exact top-k of the survivors is the
// answer. Under an exclusion the sample's excluded columns are set to -inf
// first (columns read over [0, n_excl); out_len, when given, = min(kk, n_excl
// - the row's excluded items)): kk distinct NON-EXCLUDED items reach t_b, so
// the kk-th best non-excluded score is >= t_b and the argument holds for the
// answer, which has no excluded entry. The filter also keeps excluded items
// that reach the bound: they leave in cascade_tail. A row with fewer than kk
// sample items that stay gets -inf and keeps every item; a list past its
// capacity raises the caller's overflow flag (the pruned ALS path turns a
// -inf bound into the flag itself) and the caller's exact fallback answers.
//   lane_maxima: kk <= 64 may take sample_threshold_kernel, which also zeroes
//   zero_cnt (the filter's counters); otherwise the exact kk-th, then a memset.
int cascade_bound(const CascadeWs& w, int n_users, int64_t S, int64_t step, int64_t n_excl, int kk, const Excl& x,
                  int32_t* out_len, bool lane_maxima, int* zero_cnt, const float** thr, int* thr_stride,
                  hipStream_t s) {
  const float ninf = -__builtin_inff();
  int rc = x.on ? excl_mask_run(w.samp, n_users, S, S, step, n_excl, x, ninf, out_len ? kk : 0, out_len, s) : 0;
  if (rc) return rc;
  const bool lm = lane_maxima && kk <= 64;
  *thr = lm ? w.sv : w.sv + (kk - 1);
  *thr_stride = lm ? 1 : kk;
  if (lm) {
    hipLaunchKernelGGL(sample_threshold_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, s, w.samp,
                       (int64_t)n_users, S, kk, w.sv, zero_cnt);
    return check_launch("sample_threshold_kernel");
  }
  rc = topk_rows<float>(w.samp, n_users, S, S, kk, w.si, w.sv, w.tws, (size_t)1 << 62, s);
  if (rc == HREC_OK && hipMemsetAsync(zero_cnt, 0, (size_t)n_users * 4, s) != hipSuccess)
    rc = check_launch("cascade_bound: memset");
  return rc;
}

int cascade_tail(const CascadeWs& w, int n_users, int64_t cap, int kk, const Excl& x, int32_t* out_len,
                 int64_t* out_idx, float* out_val, hipStream_t s) {
  const int rc = x.on ? excl_drop_run(x, n_users, w.cv, w.ci, w.cn, (int)cap, kk, out_len, s) : 0;
  if (rc) return rc;
  return topk_rows<float>(w.cv, n_users, cap, cap, kk, out_idx, out_val, w.fws, (size_t)1 << 62, s, w.ci, w.cn);
}

}  // namespace hrec
