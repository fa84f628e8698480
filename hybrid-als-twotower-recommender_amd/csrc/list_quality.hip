// What the served lists look like as a whole (hrec_list_quality): per list the
// intra-list diversity, the unexpectedness against the user's history and the
// means of up to four per-item tables (novelty, popularity), and the exposure
// count of every item over all lists, for lists that are already on the device
// as candidate columns. hrec_row_inv_norms makes the 1 / |v_j| the cosines
// need, once per item table. include/hrec.h has the contract.
//
// Shape: a list of up to 1024 columns and a history segment of any length,
// each entry one gathered row of d <= 256 floats: no arithmetic to speak of,
// bound by the latency of the row gathers. One wave owns a row, four rows per
// block (um_kernel's shape):
//   1. the lanes stride over the list positions, 64 at a time: the column is
//      read and checked (position below the row's length, column in [0, n)),
//      a valid one adds 1 to its exposure counter (integer atomic, one per
//      lane) and its table values to the lane's partial means;
//   2. the 64 columns are handed round by lane shuffles, kLqFly at a time:
//      the gathers of kLqFly item rows (lane l holds components l, l + 64,
//      l + 128, l + 192) and their inverse norms are issued together, then
//      x = v * inv_norm is added into the lane's slice of S and x * x into the
//      lane's Q, entries in list order;
//   3. the history segment the same way into H (no Q, no exposure);
//   4. three wave reductions (S.S, Q, S.H) and the integer counts; lane 0
//      writes the row: 1 - (S.S - Q) / (m (m - 1)) is one minus the mean
//      cosine over the m (m - 1) ordered pairs, O(m d) instead of O(m^2 d).
// The sums over rows: the block adds its four waves in wave order into one
// partial per slot, a second launch adds the partials in a fixed order onto
// sums_out (no floating-point atomics): equal inputs give equal bits.
#include "exclusion.h"
#include "wave.h"  // wave_lds_fence, wave_xor_sum

#pragma clang fp contract(off)

namespace hrec {

constexpr int kLqMaxTab = HREC_LQ_MAX_TABLES;
constexpr int kLqMaxCols = 2 + kLqMaxTab;
constexpr int kLqMaxSlots = 2 * kLqMaxCols;
constexpr int kLqListMax = 1024;
constexpr int kLqMaxD = 256;
constexpr int kLqFly = 8;  // item rows gathered together per wave (divides the wave)
static_assert(kWave % kLqFly == 0, "a stride of 64 columns is whole groups");

struct LqParams {
  const int64_t* lists;
  int64_t lists_ld;
  int list_n;
  const int32_t* list_len;
  int64_t n_rows, n;
  const float* vectors;
  int d;
  int64_t ld;
  const double* inv_norm;
  const int64_t* hrows;
  const int64_t* hindptr;
  const int32_t* hcols;
  const double* tables;
  int n_tab;
  unsigned long long* exposure;
  double* per_row;
  int32_t* row_n;
  double* partials;
};

// The wave's 64 columns c (one per lane, -1: not an entry), in lane order:
// acc[j] += x_(l + 64 j) of each, q += the lane's x * x [LIST]. An item with
// inv_norm 0 is a zero vector whatever its components are.
template <int NJ, bool LIST>
__device__ __forceinline__ void lq_gather(const LqParams& P, int64_t c, int cnt, int lane, double (&acc)[NJ],
                                          double& q) {
  for (int e = 0; e < cnt; e += kLqFly) {
    float v[kLqFly][NJ];
    double in[kLqFly];
#pragma unroll
    for (int u = 0; u < kLqFly; ++u) {  // every load of the group before any use
      const int64_t cu = __shfl(c, e + u, kWave);
      const int64_t cc = cu < 0 ? 0 : cu;  // row 0 stands in: n >= 1, the value is dropped
      const float* __restrict__ r = P.vectors + cc * P.ld;
#pragma unroll
      for (int j = 0; j < NJ; ++j) v[u][j] = (lane + 64 * j < P.d) ? r[lane + 64 * j] : 0.0f;
      in[u] = cu < 0 ? 0.0 : P.inv_norm[cc];
    }
#pragma unroll
    for (int u = 0; u < kLqFly; ++u) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const double x = in[u] != 0.0 ? (double)v[u][j] * in[u] : 0.0;
        acc[j] += x;
        if constexpr (LIST) q += x * x;
      }
    }
  }
}

// One row, one wave; out: the wave's slots of the block's partial (zeroed).
template <int NJ>
__device__ __forceinline__ void lq_row(const LqParams& P, int64_t row, int lane, double* out) {
  const int ncol = 2 + P.n_tab;
  int len = P.list_len ? P.list_len[row] : P.list_n;
  len = len < 0 ? 0 : (len > P.list_n ? P.list_n : len);
  double S[NJ], H[NJ], q = 0.0, unused = 0.0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) S[j] = H[j] = 0.0;
  double ts[kLqMaxTab];
  int tc[kLqMaxTab], m = 0, g = 0;
#pragma unroll
  for (int t = 0; t < kLqMaxTab; ++t) ts[t] = 0.0, tc[t] = 0;
  // 1, 2. the list
  const int64_t* __restrict__ lrow = P.lists + row * P.lists_ld;
  for (int base = 0; base < len; base += kWave) {
    const int pos = base + lane;
    int64_t c = -1;
    if (pos < len) {
      c = lrow[pos];
      c = (c < 0 || c >= P.n) ? -1 : c;
    }
    if (c >= 0) {
      ++m;
      atomicAdd(P.exposure + c, 1ull);
#pragma unroll
      for (int t = 0; t < kLqMaxTab; ++t) {
        if (t < P.n_tab) {
          const double x = P.tables[(int64_t)t * P.n + c];
          if (x == x) ts[t] += x, ++tc[t];
        }
      }
    }
    lq_gather<NJ, true>(P, c, len - base < kWave ? len - base : kWave, lane, S, q);
  }
  // 3. the history
  const ExclSeg hs = excl_segment(P.hrows, P.hindptr, row);
  for (int64_t b = hs.lo; b < hs.hi; b += kWave) {
    const int64_t p = b + lane;
    int64_t c = -1;
    if (p < hs.hi) {
      c = P.hcols[p];
      c = (c < 0 || c >= P.n) ? -1 : c;
    }
    g += c >= 0 ? 1 : 0;
    lq_gather<NJ, false>(P, c, hs.hi - b < kWave ? (int)(hs.hi - b) : kWave, lane, H, unused);
  }
  // 4. the row's values
  double ss = 0.0, sh = 0.0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) ss += S[j] * S[j], sh += S[j] * H[j];
  ss = wave_xor_sum(ss), q = wave_xor_sum(q), sh = wave_xor_sum(sh);
  m = wave_xor_sum(m), g = wave_xor_sum(g);
#pragma unroll
  for (int t = 0; t < kLqMaxTab; ++t) ts[t] = wave_xor_sum(ts[t]), tc[t] = wave_xor_sum(tc[t]);
  if (lane != 0) return;
  const double nan = __builtin_nan("");
  double* pr = P.per_row + row * ncol;
  int32_t* rn = P.row_n + row * ncol;
  const double ild = m >= 2 ? 1.0 - (ss - q) / ((double)m * (double)(m - 1)) : nan;
  const double unx = (m >= 1 && g >= 1) ? 1.0 - sh / ((double)m * (double)g) : nan;
  pr[0] = ild, pr[1] = unx;
  rn[0] = m, rn[1] = g;
  if (m >= 2) out[0] = ild, out[ncol] = 1.0;
  if (m >= 1 && g >= 1) out[1] = unx, out[ncol + 1] = 1.0;
#pragma unroll
  for (int t = 0; t < kLqMaxTab; ++t) {
    if (t < P.n_tab) {
      const double mean = tc[t] > 0 ? ts[t] / (double)tc[t] : nan;
      pr[2 + t] = mean;
      rn[2 + t] = tc[t];
      if (tc[t] > 0) out[2 + t] = mean, out[ncol + 2 + t] = 1.0;
    }
  }
}

template <int NJ>
__global__ __launch_bounds__(256) void lq_kernel(const LqParams P) {
  __shared__ double red[4][kLqMaxSlots];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  const int nslots = 2 * (2 + P.n_tab);
  for (int i = lane; i < kLqMaxSlots; i += kWave) red[w][i] = 0.0;
  wave_lds_fence();
  if (row < P.n_rows) lq_row<NJ>(P, row, lane, red[w]);  // wave-uniform
  __syncthreads();
  if ((int)threadIdx.x < nslots) {
    const int i = threadIdx.x;
    P.partials[(int64_t)blockIdx.x * nslots + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

// sums[i] += the blocks' partials of slot i (block i of the launch): lane l
// adds blocks l, l + 64, ... in ascending order, then the lanes' xor tree.
__global__ __launch_bounds__(64) void lq_reduce_kernel(const double* __restrict__ partials, int64_t n_blocks, int nslots,
                                                       double* __restrict__ sums) {
  const int lane = threadIdx.x, i = blockIdx.x;
  double v = 0.0;
  for (int64_t b = lane; b < n_blocks; b += 64) v += partials[b * nslots + i];
  v = wave_xor_sum(v);
  if (lane == 0) sums[i] = sums[i] + v;
}

// out[j] = 1 / sqrt(sum of squares of row j), one wave per row: the lanes'
// strided partials in f64, then the xor tree.
__global__ __launch_bounds__(256) void lq_inv_norm_kernel(const float* __restrict__ vectors, int64_t n, int d, int64_t ld,
                                                          double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;  // wave-uniform
  double s = 0.0;
  for (int c = lane; c < d; c += kWave) {
    const double x = (double)vectors[j * ld + c];
    s += x * x;
  }
  s = wave_xor_sum(s);
  if (lane == 0) out[j] = (s > 0.0 && s - s == 0.0) ? 1.0 / sqrt(s) : 0.0;
}

}  // namespace hrec

using namespace hrec;

static int64_t lq_blocks(int64_t n_rows) { return n_rows > 0 ? (n_rows + 3) / 4 : 1; }

extern "C" size_t hrec_list_quality_workspace_bytes(int64_t n_rows) {
  return al256((size_t)lq_blocks(n_rows) * kLqMaxSlots * sizeof(double));
}

extern "C" int hrec_row_inv_norms(const float* vectors, int64_t n, int d, int64_t ld, double* out, void* stream) {
  HREC_REQUIRE(d >= 1 && d <= kLqMaxD, "row_inv_norms: d must be in [1, %d] (got %d)", kLqMaxD, d);
  HREC_REQUIRE(ld >= d, "row_inv_norms: ld must be >= d");
  HREC_REQUIRE(n >= 0 && n <= INT32_MAX, "row_inv_norms: n must be in [0, 2^31)");
  if (n == 0) return HREC_OK;
  HREC_REQUIRE(vectors && out, "row_inv_norms: null pointer");
  hipLaunchKernelGGL(lq_inv_norm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), vectors, n, d,
                     ld, out);
  return check_launch("lq_inv_norm_kernel");
}

extern "C" int hrec_list_quality(const int64_t* lists, int64_t lists_ld, int list_n, const int32_t* list_len,
                                 int64_t n_rows, int64_t n, const float* vectors, int d, int64_t ld,
                                 const double* inv_norm, const int64_t* hist_rows, const int64_t* hist_indptr,
                                 const int32_t* hist_cols, const double* item_tables, int n_tab, int64_t* exposure,
                                 double* per_row, int32_t* row_n, double* sums_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  HREC_REQUIRE(d >= 1 && d <= kLqMaxD, "list_quality: d must be in [1, %d] (got %d)", kLqMaxD, d);
  HREC_REQUIRE(ld >= d, "list_quality: ld must be >= d");
  HREC_REQUIRE(list_n >= 0 && list_n <= kLqListMax, "list_quality: list_n must be in [0, %d] (got %d)", kLqListMax,
               list_n);
  HREC_REQUIRE(lists_ld >= list_n, "list_quality: lists_ld must be >= list_n");
  HREC_REQUIRE(n_tab >= 0 && n_tab <= kLqMaxTab, "list_quality: n_tab must be in [0, %d] (got %d)", kLqMaxTab, n_tab);
  HREC_REQUIRE(n >= 1 && n <= INT32_MAX, "list_quality: n must be in [1, 2^31)");
  HREC_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX, "list_quality: bad shape");
  const bool any_hist = hist_rows || hist_indptr || hist_cols;
  HREC_REQUIRE(!any_hist || (hist_rows && hist_indptr && hist_cols),
               "list_quality: the history CSR needs hist_rows, hist_indptr and hist_cols (or none of them)");
  if (n_rows == 0) return HREC_OK;
  const size_t need = hrec_list_quality_workspace_bytes(n_rows);
  HREC_REQUIRE(workspace_bytes >= need, "list_quality: workspace %zu < %zu", workspace_bytes, need);
  HREC_REQUIRE(vectors && inv_norm && exposure && per_row && row_n && sums_out && workspace && (lists || list_n == 0) &&
                   (item_tables || n_tab == 0),
               "list_quality: null pointer");
  LqParams P{};
  P.lists = lists, P.lists_ld = lists_ld, P.list_n = list_n, P.list_len = list_len;
  P.n_rows = n_rows, P.n = n;
  P.vectors = vectors, P.d = d, P.ld = ld, P.inv_norm = inv_norm;
  P.hrows = hist_rows, P.hindptr = hist_indptr, P.hcols = hist_cols;
  P.tables = item_tables, P.n_tab = n_tab;
  P.exposure = reinterpret_cast<unsigned long long*>(exposure);
  P.per_row = per_row, P.row_n = row_n, P.partials = static_cast<double*>(workspace);
  hipStream_t s = as_stream(stream);
  const int64_t nb = lq_blocks(n_rows);
  const int nslots = 2 * (2 + n_tab);
  const dim3 grid((unsigned)nb), block(256);
  switch ((d + kWave - 1) / kWave) {  // components per lane
    case 1: hipLaunchKernelGGL(lq_kernel<1>, grid, block, 0, s, P); break;
    case 2: hipLaunchKernelGGL(lq_kernel<2>, grid, block, 0, s, P); break;
    case 3: hipLaunchKernelGGL(lq_kernel<3>, grid, block, 0, s, P); break;
    default: hipLaunchKernelGGL(lq_kernel<4>, grid, block, 0, s, P); break;
  }
  const int rc = check_launch("lq_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(lq_reduce_kernel, dim3((unsigned)nslots), dim3(64), 0, s, P.partials, nb, nslots, sums_out);
  return check_launch("lq_reduce_kernel");
}
