// The non-negative ALS half-sweep (Spark ALS nonnegative = true): the row
// pipeline of csrc/als.hip up to the normal equations (gram_row, explicit or
// implicit), then Spark's NNLS.solve on the wave in place of factor_row.
#undef HREC_ALS_STAMPS  // the per-phase cycle stamps are a diagnostic of als.hip's kernels
#include "als_row.h"

namespace hrec {

// ---- non-negative least squares (Spark's nonnegative = true) ---------------
// The wave's sums and minimum are wave_row_sum / wave_row_min (csrc/wave.h:
// wave-uniform, the DPP-row order); the branches on them go through uniform().
// y_lane = sum_j arow[j] v[j]: the lane's row of A from registers, v from LDS
// as wave-uniform 16-B reads (a broadcast: no bank conflicts); four chains.
template <int KP>
__device__ __forceinline__ double symv(const double (&arow)[KP], const double* v) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
  for (int j = 0; j < KP; j += 4) {
    const double2 u = *reinterpret_cast<const double2*>(v + j);
    const double2 w = *reinterpret_cast<const double2*>(v + j + 2);
    s0 = fma(arow[j], u.x, s0);
    s1 = fma(arow[j + 1], u.y, s1);
    s2 = fma(arow[j + 2], w.x, s2);
    s3 = fma(arow[j + 3], w.y, s3);
  }
  return (s0 + s1) + (s2 + s3);
}

// Spark 3.5 mllib NNLS.solve (ALS.NNLSSolver) of one row's normal equations
// on one wave, in place of factor_row: min x^T A x / 2 - b^T x over x >= 0 by
// projected gradients with conjugate-gradient directions, x from 0, f64.
// acc (tile layout) and b (bsh) are those of gram_row, in its permuted basis
// q = 16 T + m <-> column NT m + T; lane q owns entry q of x, grad, dir,
// lastDir and res and keeps ROW q of A in registers (A is copied once through
// the column-packed triangle in Up). A v is then KP fmas per lane with v read
// from LDS as wave-uniform broadcasts. Lanes of padding columns stay at 0.
// Every branch is taken on a wave-uniform value (reduce, then read one lane),
// and the loop is bounded by iterMax = max(400, 20 k): it ends on any input
// (a NaN step stops it). Returns the number of iterations that moved x.
template <int NT>
__device__ __forceinline__ int nnls_row(int lane, d4 (&acc)[NT * (NT + 1) / 2], double* __restrict__ Up,
                                        double* __restrict__ scratch, const double* __restrict__ bsh, int k,
                                        float* __restrict__ out) {
  constexpr int KP = 16 * NT;
  double* xb = scratch;        // x
  double* gb = scratch + 64;   // grad
  double* db = scratch + 128;  // the conjugate direction (2 KP doubles there)
  const int sub = lane >> 4, col = lane & 15;
  auto pidx = [](int I, int K) { return I * NT - (I * (I - 1)) / 2 + (K - I); };
  // the upper triangle of the permuted A, column-packed: Up[tri(c) + q], q <= c
#pragma unroll
  for (int J = 0; J < NT; ++J) {
#pragma unroll
    for (int K = J; K < NT; ++K) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int q = 16 * J + sub + 4 * rr, c = 16 * K + col;
        if (q <= c) Up[tri(c) + q] = acc[pidx(J, K)][rr];
      }
    }
  }
  wave_lds_fence();
  const bool live = lane < KP && NT * col + sub < k;  // sub = the tile T of lane q = 16 T + m when lane < KP
  const int me = lane < KP ? lane : 0;
  double arow[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) arow[j] = Up[j <= me ? tri(me) + j : tri(j) + me];
  const double b = bsh[me];
  double x = 0.0, last_dir = 0.0, last_norm = 0.0;
  int last_wall = 0, iterno = 0;
  const int iter_max = 20 * k > 400 ? 20 * k : 400;
  auto stop = [](double step, double ndir, double nx) {
    return step != step || step < 1e-7 || step > 1e40 || ndir < 1e-12 * nx || ndir < 1e-32;
  };
  for (; iterno < iter_max; ++iterno) {
    if (lane < KP) xb[lane] = x;
    wave_lds_fence();
    const double res = live ? symv<KP>(arow, xb) - b : 0.0;
    const double grad = (res > 0.0 && x == 0.0) ? 0.0 : res;
    const double ngrad = wave_row_sum(grad * grad);
    const double nx = wave_row_sum(x * x);
    const bool cg = iterno > last_wall + 1;  // wave-uniform
    const double dirc = cg ? fma(ngrad / last_norm, last_dir, grad) : grad;
    if (lane < KP) {
      gb[lane] = grad;
      db[lane] = dirc;
    }
    wave_lds_fence();
    const double ag = live ? symv<KP>(arow, gb) : 0.0;
    double step = wave_row_sum(grad * res) / (wave_row_sum(ag * grad) + 1e-20);
    double dir = grad, ndir = ngrad;
    if (cg) {
      const double ad = live ? symv<KP>(arow, db) : 0.0;
      const double dstep = wave_row_sum(dirc * res) / (wave_row_sum(ad * dirc) + 1e-20);
      const double ndirc = wave_row_sum(dirc * dirc);
      if (!uniform(stop(dstep, ndirc, nx))) {  // else: reject the CG step, dir = grad
        dir = dirc;
        ndir = ndirc;
        step = dstep;
      }
    }
    if (uniform(stop(step, ndir, nx))) break;
    // Don't cross a wall. Spark walks i upwards with a shrinking step; an
    // entry that fails its test against the shrunken step has a ratio
    // x_i / dir_i no smaller than that step, so the result is the minimum of
    // the ratios over the entries that pass the test against the INITIAL step.
    step = fmin(step, wave_row_min(step * dir > x ? x / dir : __builtin_inf()));
    const bool hit = step * dir > x * (1.0 - 1e-14);
    x = hit ? 0.0 : x - step * dir;
    if (__ballot(hit) != 0ull) last_wall = iterno;
    last_dir = dir;
    last_norm = ngrad;
  }
  if (lane < KP) out[NT * col + sub] = (float)x;
  wave_lds_fence();  // the next row on this wave reuses the LDS slice
  return iterno;
}

// The non-negative half-sweep: gram_row as the explicit (IMP = false) or the
// implicit kernel instantiates it, then nnls_row in place of factor_row.
// iters_out (nullable) receives the row's NNLS iteration count.
template <int NT, int CH, bool IMP>
__global__ __launch_bounds__(64, HREC_ALS_WAVES) void als_half_sweep_nonneg_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ values, int64_t n_rows, const float* __restrict__ src, int64_t n_src,
    int k, double reg, double alpha, const double* __restrict__ yty, float* __restrict__ dst,
    int32_t* __restrict__ iters_out) {
  constexpr int KP = 16 * NT;
  __shared__ __attribute__((aligned(16))) double lds[RowLds<KP>::kSize];
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t beg = indptr[row];
  const int64_t end = indptr[row + 1];
  float* __restrict__ out = dst + row * KP;
  int iters = 0;
  bool solve = end != beg;
  d4 acc[NT * (NT + 1) / 2];
  double* scratch = lds + RowLds<KP>::kUpPad;
  double* bsh = scratch + 128 + 2 * KP;
  if (solve) {
    if constexpr (IMP) {
      int n_pos = 0;
      gram_row<NT, CH, 0, false, true>(beg, end, lane, indices, values, src, n_src, k, reg, acc, bsh, lds, alpha, yty,
                                       &n_pos);
      solve = n_pos != 0;  // no rating > 0: b = 0, the factor is exactly zero (wave-uniform)
    } else {
      gram_row<NT, CH, 0>(beg, end, lane, indices, values, src, n_src, k, reg, acc, bsh, lds);
    }
  }
  if (solve) iters = nnls_row<NT>(lane, acc, lds, scratch, bsh, k, out);
  else if (lane < KP) out[lane] = 0.f;
  if (iters_out != nullptr && lane == 0) iters_out[row] = iters;
}

}  // namespace hrec

using namespace hrec;

extern "C" int hrec_als_half_sweep_nonneg(const int64_t* indptr, const int32_t* indices, const float* values,
                                          int64_t n_rows, const float* src_factors, int64_t n_src, int k, int kp,
                                          double reg_param, int implicit, double alpha, const double* yty,
                                          float* dst_factors, int32_t* iters_out, void* stream) {
  HREC_REQUIRE(kp == 16 || kp == 32 || kp == 64,
               "als_half_sweep_nonneg: kp must be 16, 32 or 64 (nonnegative supports rank <= 64; got kp %d)", kp);
  HREC_REQUIRE(k >= 1 && k <= kp, "als_half_sweep_nonneg: need 1 <= k <= kp (k=%d kp=%d)", k, kp);
  HREC_REQUIRE(n_rows >= 0 && n_src >= 0, "als_half_sweep_nonneg: negative size");
  HREC_REQUIRE(n_rows < 0x7fffffffll && n_src < 0x7fffffffll, "als_half_sweep_nonneg: too many rows for one launch");
  HREC_REQUIRE(implicit == 0 || implicit == 1, "als_half_sweep_nonneg: implicit must be 0 or 1 (got %d)", implicit);
  HREC_REQUIRE(alpha >= 0.0, "als_half_sweep_nonneg: alpha must be >= 0 (got %g)", alpha);
  HREC_REQUIRE(reg_param >= 0.0, "als_half_sweep_nonneg: reg_param must be >= 0");
  HREC_REQUIRE(kp != 64 || n_src * (int64_t)kp * 4 <= (int64_t)0xffffffffll,
               "als_half_sweep_nonneg: %lld source rows of %d floats exceed the 4 GiB a gather resource spans; "
               "shard the source side", (long long)n_src, kp);
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(indptr && dst_factors && (!implicit || yty), "als_half_sweep_nonneg: null pointer");
  HREC_REQUIRE(n_src > 0 && src_factors && indices && values,
               "als_half_sweep_nonneg: null source factors / CSR arrays");
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)n_rows), block(64);
#define HREC_SWEEP(NT, CH, IMP)                                                                                  \
  hipLaunchKernelGGL((als_half_sweep_nonneg_kernel<NT, CH, IMP>), grid, block, 0, s, indptr, indices, values,    \
                     n_rows, src_factors, n_src, k, reg_param, alpha, yty, dst_factors, iters_out)
  if (implicit) {
    if (kp == 64) HREC_SWEEP(4, HREC_ALS_CH0, true);
    else if (kp == 32) HREC_SWEEP(2, 8, true);
    else HREC_SWEEP(1, 8, true);
  } else {
    if (kp == 64) HREC_SWEEP(4, HREC_ALS_CH0, false);
    else if (kp == 32) HREC_SWEEP(2, 8, false);
    else HREC_SWEEP(1, 8, false);
  }
#undef HREC_SWEEP
  return check_launch("als_half_sweep_nonneg_kernel");
}
