// Diversity-aware re-ranking of a candidate pool (hrec_mmr_rerank): greedy
// Maximal Marginal Relevance (Carbonell and Goldstein 1998). Per list, top_n
// steps; each step takes the unselected entry with the largest
//   lambda * rel_p - (1 - lambda) * max_{q selected} cos(p, q)
// and then folds the cosines against the new pick into every entry's running
// maximum. include/hrec.h has the contract.
//
// Shape: the steps of one list are sequential, the work inside a step is one
// dot product of d <= 256 components per pool entry. One block owns a list,
// one THREAD owns a pool position (KP of them when the pool is longer than the
// block: p = tid, tid + T, ...), so a dot product is a private f64 chain with
// no reduction, and rel_p, maxsim_p, inv_norm_p and the selected flag stay in
// the thread's registers for the whole selection. Per step:
//   1. every thread offers its best unselected (value, position); a wave xor
//      tree, then the waves' winners through LDS, read in wave order by every
//      thread: a fixed reduction, larger value first, then smaller position;
//   2. the winner's x_q = v_q * inv_norm_q (d doubles) is written to LDS by
//      the whole block and read back as a broadcast;
//   3. every unselected thread reads its own vector once and updates maxsim.
// STAGED: the pool's f32 rows are copied to LDS once (coalesced, row stride
// d | 1 dwords so that the lanes of a wave hit distinct banks) when they fit
// kMmrStageBytes; otherwise every step re-reads them from global memory (a
// pool is at most 1 MiB: it stays in L2).
#include "common.h"

#pragma clang fp contract(off)

namespace hrec {

constexpr int kMmrPoolMax = 1024;
constexpr int kMmrMaxD = 256;
constexpr int kMmrThreads = 256;
// Dynamic LDS for the staged rows: with the 6.1 KiB of static LDS below a
// block stays under 64 KiB, so at least two blocks share a CU's 160 KiB.
constexpr size_t kMmrStageBytes = 56 * 1024;

struct MmrParams {
  const int64_t* pool;
  int64_t pool_ld;
  int pool_n;
  const int32_t* pool_len;
  const void* scores;
  int64_t scores_ld;
  int64_t n;
  const float* vectors;
  int d;
  int64_t ld;
  const double* inv_norm;
  double lambda;
  int top_n;
  int32_t* out_pos;
  int32_t* out_len;
  double* out_value;
};

struct MmrBest {
  double v;
  int p;  // INT32_MAX: no candidate
};

// a before b: the larger value, then the smaller position.
__device__ __forceinline__ bool mmr_before(const MmrBest& a, const MmrBest& b) {
  return a.v > b.v || (a.v == b.v && a.p < b.p);
}

__device__ __forceinline__ MmrBest mmr_wave_best(MmrBest x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    MmrBest y;
    y.v = __shfl_xor(x.v, off, kWave);
    y.p = __shfl_xor(x.p, off, kWave);
    if (mmr_before(y, x)) x = y;
  }
  return x;
}

// x_p . x_q over d components: x_p = (double)row[c] * inv (inv != 0), xq from
// LDS. Four partial sums (c mod 4), added pairwise at the end.
__device__ __forceinline__ double mmr_dot(const float* __restrict__ row, double inv, const double* xq, int d) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int c = 0;
  for (; c + 4 <= d; c += 4) {
    a0 += ((double)row[c] * inv) * xq[c];
    a1 += ((double)row[c + 1] * inv) * xq[c + 1];
    a2 += ((double)row[c + 2] * inv) * xq[c + 2];
    a3 += ((double)row[c + 3] * inv) * xq[c + 3];
  }
  if (c < d) a0 += ((double)row[c] * inv) * xq[c];
  if (c + 1 < d) a1 += ((double)row[c + 1] * inv) * xq[c + 1];
  if (c + 2 < d) a2 += ((double)row[c + 2] * inv) * xq[c + 2];
  return (a0 + a1) + (a2 + a3);
}

template <int KP, bool STAGED, typename ST>
__global__ __launch_bounds__(kMmrThreads) void mmr_kernel(const MmrParams P) {
  extern __shared__ float stage[];  // STAGED: [len][sld] f32 rows
  __shared__ double xq[kMmrMaxD];
  __shared__ int cols[kMmrPoolMax];  // the validated column of a position, -1: not an entry
  __shared__ double red_v[4], red_lo[4], red_hi[4];
  __shared__ int red_p[4], red_n[4];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, w = tid >> 6, nw = T >> 6;
  const int64_t row = blockIdx.x;
  const int d = P.d, sld = d | 1;
  int len = P.pool_len ? P.pool_len[row] : P.pool_n;
  len = len < 0 ? 0 : (len > P.pool_n ? P.pool_n : len);
  const double inf = __builtin_inf();

  // The thread's positions: column, score, inverse norm.
  double s[KP], inv[KP], rel[KP], maxsim[KP];
  int col[KP];
  bool open[KP];  // valid and not selected yet
  double lo = inf, hi = -inf;
  int valid = 0;
  const ST* __restrict__ srow = static_cast<const ST*>(P.scores) + row * P.scores_ld;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int p = tid + k * T;
    col[k] = -1, s[k] = 0.0, inv[k] = 0.0, maxsim[k] = 0.0;
    if (p < len) {
      const int64_t c = P.pool[row * P.pool_ld + p];
      if (c >= 0 && c < P.n) {
        col[k] = (int)c;
        s[k] = (double)srow[p];
        inv[k] = P.inv_norm[c];
        ++valid;
        if (s[k] - s[k] == 0.0) lo = s[k] < lo ? s[k] : lo, hi = s[k] > hi ? s[k] : hi;
      }
    }
    open[k] = col[k] >= 0;
    if (p < P.pool_n) cols[p] = col[k];
  }
  // lo, hi and the number of valid entries over the block (order-free).
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double l2 = __shfl_xor(lo, off, kWave), h2 = __shfl_xor(hi, off, kWave);
    lo = l2 < lo ? l2 : lo, hi = h2 > hi ? h2 : hi;
    valid += __shfl_xor(valid, off, kWave);
  }
  if (lane == 0) red_lo[w] = lo, red_hi[w] = hi, red_n[w] = valid;
  __syncthreads();  // also: cols[] is complete
  lo = red_lo[0], hi = red_hi[0], valid = red_n[0];
  for (int i = 1; i < nw; ++i) {
    lo = red_lo[i] < lo ? red_lo[i] : lo, hi = red_hi[i] > hi ? red_hi[i] : hi;
    valid += red_n[i];
  }
  const int m = valid < P.top_n ? valid : P.top_n;  // block-uniform
  int32_t* __restrict__ opos = P.out_pos + row * P.top_n;
  double* __restrict__ oval = P.out_value ? P.out_value + row * P.top_n : nullptr;
  for (int t = m + tid; t < P.top_n; t += T) {
    opos[t] = -1;
    if (oval) oval[t] = __builtin_nan("");
  }
  if (tid == 0) P.out_len[row] = m;
  if (m == 0) return;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const bool finite = s[k] - s[k] == 0.0;
    rel[k] = !finite ? -inf : (hi == lo ? 1.0 : (s[k] - lo) / (hi - lo));
  }
  if constexpr (STAGED) {  // one wave per row, the lanes over its components
    for (int p = w; p < len; p += nw) {
      const int c = cols[p];
      if (c < 0) continue;  // wave-uniform; the row is never read
      const float* __restrict__ r = P.vectors + (int64_t)c * P.ld;
      for (int j = lane; j < d; j += kWave) stage[p * sld + j] = r[j];
    }
    // visible after the first step's barrier, before any read
  }

  const double lam = P.lambda, oml = 1.0 - P.lambda;
  for (int t = 0; t < m; ++t) {
    // 1. the best unselected entry
    MmrBest b{-inf, INT32_MAX};
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (!open[k]) continue;
      double v = rel[k] == -inf ? -inf : (t == 0 ? lam * rel[k] : lam * rel[k] - oml * maxsim[k]);
      v = v == v ? v : -inf;
      const MmrBest c{v, tid + k * T};
      if (mmr_before(c, b)) b = c;
    }
    b = mmr_wave_best(b);
    if (lane == 0) red_v[w] = b.v, red_p[w] = b.p;
    __syncthreads();
    b = MmrBest{red_v[0], red_p[0]};
    for (int i = 1; i < nw; ++i) {
      const MmrBest c{red_v[i], red_p[i]};
      if (mmr_before(c, b)) b = c;
    }
    // m <= the valid entries: an open entry exists, b.p < pool_n
    if (tid == 0) {
      opos[t] = b.p;
      if (oval) oval[t] = b.v;
    }
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (tid + k * T == b.p) open[k] = false;
    if (t + 1 == m) break;  // block-uniform
    // 2. x_q to LDS
    const int cq = cols[b.p];
    const double iq = P.inv_norm[cq];
    const float* __restrict__ rq = STAGED ? stage + b.p * sld : P.vectors + (int64_t)cq * P.ld;
    for (int j = tid; j < d; j += T) xq[j] = iq != 0.0 ? (double)rq[j] * iq : 0.0;
    __syncthreads();
    // 3. the cosines against it
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (!open[k]) continue;
      const float* __restrict__ r = STAGED ? stage + (tid + k * T) * sld : P.vectors + (int64_t)col[k] * P.ld;
      const double sim = inv[k] != 0.0 ? mmr_dot(r, inv[k], xq, d) : 0.0;
      maxsim[k] = (t == 0 || sim > maxsim[k]) ? sim : maxsim[k];
    }
    // the next step's barrier orders these reads of xq before its rewrite, and
    // this step's second barrier ordered the reads of red_* before theirs
  }
}

template <int KP, bool STAGED>
static void mmr_launch(const MmrParams& P, int f64, int64_t n_rows, int threads, size_t lds, hipStream_t s) {
  const dim3 grid((unsigned)n_rows), block((unsigned)threads);
  if (f64)
    hipLaunchKernelGGL((mmr_kernel<KP, STAGED, double>), grid, block, lds, s, P);
  else
    hipLaunchKernelGGL((mmr_kernel<KP, STAGED, float>), grid, block, lds, s, P);
}

}  // namespace hrec

using namespace hrec;

extern "C" int hrec_mmr_rerank(const int64_t* pool, int64_t pool_ld, int pool_n, const int32_t* pool_len,
                               const void* scores, int scores_f64, int64_t scores_ld, int64_t n_rows, int64_t n,
                               const float* vectors, int d, int64_t ld, const double* inv_norm, double lambda,
                               int top_n, int32_t* out_pos, int32_t* out_len, double* out_value, void* stream) {
  HREC_REQUIRE(d >= 1 && d <= kMmrMaxD, "mmr_rerank: d must be in [1, %d] (got %d)", kMmrMaxD, d);
  HREC_REQUIRE(ld >= d, "mmr_rerank: ld must be >= d");
  HREC_REQUIRE(pool_n >= 1 && pool_n <= kMmrPoolMax, "mmr_rerank: pool_n must be in [1, %d] (got %d)", kMmrPoolMax,
               pool_n);
  HREC_REQUIRE(top_n >= 1 && top_n <= pool_n, "mmr_rerank: top_n must be in [1, pool_n] (got %d)", top_n);
  HREC_REQUIRE(pool_ld >= pool_n, "mmr_rerank: pool_ld must be >= pool_n");
  HREC_REQUIRE(scores_ld >= pool_n, "mmr_rerank: scores_ld must be >= pool_n");
  HREC_REQUIRE(scores_f64 == 0 || scores_f64 == 1, "mmr_rerank: scores_f64 must be 0 or 1");
  HREC_REQUIRE(lambda >= 0.0 && lambda <= 1.0, "mmr_rerank: lambda must be in [0, 1]");
  HREC_REQUIRE(n >= 1 && n <= INT32_MAX, "mmr_rerank: n must be in [1, 2^31)");
  HREC_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX, "mmr_rerank: bad shape");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(pool && scores && vectors && inv_norm && out_pos && out_len, "mmr_rerank: null pointer");
  MmrParams P{};
  P.pool = pool, P.pool_ld = pool_ld, P.pool_n = pool_n, P.pool_len = pool_len;
  P.scores = scores, P.scores_ld = scores_ld, P.n = n;
  P.vectors = vectors, P.d = d, P.ld = ld, P.inv_norm = inv_norm;
  P.lambda = lambda, P.top_n = top_n;
  P.out_pos = out_pos, P.out_len = out_len, P.out_value = out_value;
  hipStream_t s = as_stream(stream);
  const int threads = pool_n >= kMmrThreads ? kMmrThreads : (pool_n + kWave - 1) / kWave * kWave;
  const int kp = (pool_n + threads - 1) / threads;  // positions per thread: 1 .. 4
  const size_t bytes = (size_t)pool_n * (size_t)(d | 1) * sizeof(float);
  const bool staged = bytes <= kMmrStageBytes;
  const size_t lds = staged ? bytes : 0;
  if (kp == 1) {
    staged ? mmr_launch<1, true>(P, scores_f64, n_rows, threads, lds, s)
           : mmr_launch<1, false>(P, scores_f64, n_rows, threads, lds, s);
  } else if (kp == 2) {
    staged ? mmr_launch<2, true>(P, scores_f64, n_rows, threads, lds, s)
           : mmr_launch<2, false>(P, scores_f64, n_rows, threads, lds, s);
  } else {
    staged ? mmr_launch<4, true>(P, scores_f64, n_rows, threads, lds, s)
           : mmr_launch<4, false>(P, scores_f64, n_rows, threads, lds, s);
  }
  return check_launch("mmr_kernel");
}
