// K1: ALS half-sweep — CSR row gather -> f64 MFMA Gramian -> Cholesky solve.
//
// Replaces Spark 3.5.1 ALS.computeFactors / NormalEquation.add /
// CholeskySolver.solve [ext], reached from src/als_model.py:62 (als.fit).
// Per destination row r (one wave per row):
//   A = sum_j v_j v_j^T  (f64),  b = sum_j r_j v_j (f64),  n = #ratings
//   A[d][d] += reg * n, solve A x = b (Cholesky, f64), store f32.
// Implicit feedback (IMP, Spark's implicitPrefs branch), c1_j = alpha |r_j|:
//   A = YtY + sum_j c1_j v_j v_j^T,  b = sum_{r_j > 0} (1 + c1_j) v_j,
//   A[d][d] += reg * #{r_j > 0}  (YtY: csrc/als_gramian.hip).
//
// Gramian on the matrix cores: v_mfma_f64_16x16x4_f64 with the 4 nnz of a
// step as the K dimension. Each lane loads ONE 16-B vector (NT floats) of a
// gathered factor row: lane l holds row (l>>4) of the step, columns
// NT*(l&15) .. +NT-1. Column c = NT*m + T belongs to tile T at index m, so
// component T of the lane's vector is exactly the MFMA operand of tile T
// (A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]) — no shuffles, fully coalesced
// 256-B row reads. Tile pair (I,J), I<=J, accumulates G[NT*m+I][NT*m'+J].
#include "als_row.h"

namespace hrec {

template <int NT, int CH, int MODE, bool S64 = false, bool IMP = false>
__device__ __forceinline__ void als_row(int64_t row, int lane, const int64_t* __restrict__ indptr,
                                        const int32_t* __restrict__ indices, const float* __restrict__ values,
                                        const float* __restrict__ src, int64_t n_src, int k, double reg,
                                        float* __restrict__ dst, double* __restrict__ lds, double alpha = 0.0,
                                        const double* __restrict__ yty = nullptr) {
  constexpr int KP = 16 * NT;
  const int64_t beg = indptr[row];
  const int64_t end = indptr[row + 1];
  float* __restrict__ out = dst + row * KP;
  if (end == beg) {
    if (lane < KP) out[lane] = 0.f;
    return;
  }
  d4 acc[NT * (NT + 1) / 2];
  double* scratch = lds + RowLds<KP>::kUpPad;
  double* bsh = scratch + 128 + 2 * KP;
  if constexpr (IMP) {
    int n_pos = 0;
    gram_row<NT, CH, MODE, NoHook, S64, true>(beg, end, lane, indices, values, src, n_src, k, reg, acc, bsh, lds,
                                              NoHook(), alpha, yty, &n_pos);
    if (n_pos == 0) {  // no rating > 0: b = 0, the factor is exactly zero (wave-uniform)
      if (lane < KP) out[lane] = 0.f;
      return;
    }
  } else {
    gram_row<NT, CH, MODE, NoHook, S64>(beg, end, lane, indices, values, src, n_src, k, reg, acc, bsh, lds);
  }
  factor_row<NT>(lane, acc, lds, scratch, bsh, out);
}

// One wave per destination row. S64: src points at f64 source factors.
template <int NT, int CH, int MODE, bool S64 = false>
__global__ __launch_bounds__(64, HREC_ALS_WAVES) void als_half_sweep_f64_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ values, int64_t n_rows, const float* __restrict__ src, int64_t n_src,
    int k, double reg, float* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) double lds[RowLds<16 * NT>::kSize];
  als_row<NT, CH, MODE, S64>(blockIdx.x, threadIdx.x, indptr, indices, values, src, n_src, k, reg, dst, lds);
}

// The implicit-feedback half-sweep: the same row pipeline with the confidence
// weights and the source Gramian yty[KP][KP] (row-major f64).
template <int NT, int CH>
__global__ __launch_bounds__(64, HREC_ALS_WAVES) void als_half_sweep_implicit_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ values, int64_t n_rows, const float* __restrict__ src, int64_t n_src,
    int k, double reg, double alpha, const double* __restrict__ yty, float* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) double lds[RowLds<16 * NT>::kSize];
  als_row<NT, CH, 0, false, true>(blockIdx.x, threadIdx.x, indptr, indices, values, src, n_src, k, reg, dst, lds,
                                  alpha, yty);
}

__global__ __launch_bounds__(256) void f32_to_f64_kernel(const float* __restrict__ in, int64_t n,
                                                         double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = (double)in[i];
}

__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, int64_t rows,
                                                        int64_t cols, float* __restrict__ out, int64_t ld_out) {
  __shared__ float tile[64][65];
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int64_t c0 = (int64_t)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int64_t r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < rows && c < cols) ? in[r * cols + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int64_t c = c0 + i, r = r0 + tx;
    if (r < rows && c < cols) out[c * ld_out + r] = tile[tx][i];
  }
}

}  // namespace hrec

using namespace hrec;

extern "C" int hrec_als_half_sweep(const int64_t* indptr, const int32_t* indices, const float* values,
                                   int64_t n_rows, const float* src_factors, int64_t n_src, int k,
                                   int kp, double reg_param, int accum_mode, float* dst_factors,
                                   void* stream) {
  HREC_REQUIRE(hrec_factor_ld_ok(kp), "als_half_sweep: kp must be 16, 32, 64, 96, 128, 192 or 256 (got %d)", kp);
  HREC_REQUIRE(k >= 1 && k <= kp, "als_half_sweep: need 1 <= k <= kp (k=%d kp=%d)", k, kp);
  HREC_REQUIRE(n_rows >= 0 && n_src >= 0, "als_half_sweep: negative size");
  HREC_REQUIRE(n_rows < 0x7fffffffll, "als_half_sweep: too many rows for one launch");
  HREC_REQUIRE(accum_mode == 0 || accum_mode == 1, "als_half_sweep: accum_mode %d unsupported", accum_mode);
  HREC_REQUIRE(reg_param >= 0.0, "als_half_sweep: reg_param must be >= 0");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(indptr && dst_factors, "als_half_sweep: null pointer");
  HREC_REQUIRE(n_src > 0 && src_factors && indices && values,
               "als_half_sweep: null source factors / CSR arrays");
  HREC_REQUIRE(n_src < 0x7fffffffll, "als_half_sweep: too many source rows for one launch");
  // the kp-64 gather addresses source rows through one buffer resource, whose
  // 32-bit byte offsets span 4 GiB (16.7M f32 rows of 64)
  HREC_REQUIRE(kp != 64 || n_src * (int64_t)kp * 4 <= (int64_t)0xffffffffll,
               "als_half_sweep: %lld source rows of %d floats exceed the 4 GiB a gather resource spans; shard the "
               "source side", (long long)n_src, kp);
  if (kp > 64) {
    HREC_REQUIRE(accum_mode == 0, "als_half_sweep: kp > 64 supports accum_mode 0 (f64) only");
    return hrec_als_half_sweep_wide(indptr, indices, values, n_rows, src_factors, n_src, k, kp, reg_param,
                                    dst_factors, stream);
  }
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)n_rows), block(64);
#define HREC_SWEEP(NT, CH, M)                                                                      \
  hipLaunchKernelGGL((als_half_sweep_f64_kernel<NT, CH, M>), grid, block, 0, s, indptr, indices, values, \
                     n_rows, src_factors, n_src, k, reg_param, dst_factors)
  if (accum_mode == 0) {
    if (kp == 64) HREC_SWEEP(4, HREC_ALS_CH0, 0);
    else if (kp == 32) HREC_SWEEP(2, 8, 0);
    else HREC_SWEEP(1, 8, 0);
  } else {
    if (kp == 64) HREC_SWEEP(4, HREC_ALS_CH1, 1);
    else if (kp == 32) HREC_SWEEP(2, 4, 1);
    else HREC_SWEEP(1, 4, 1);
  }
#undef HREC_SWEEP
  return check_launch("als_half_sweep_f64_kernel");
}

extern "C" int hrec_als_half_sweep_implicit(const int64_t* indptr, const int32_t* indices, const float* values,
                                            int64_t n_rows, const float* src_factors, int64_t n_src, int k, int kp,
                                            double reg_param, double alpha, const double* yty, float* dst_factors,
                                            void* stream) {
  HREC_REQUIRE(kp == 16 || kp == 32 || kp == 64,
               "als_half_sweep_implicit: kp must be 16, 32 or 64 (implicit feedback supports rank <= 64; got kp %d)",
               kp);
  HREC_REQUIRE(k >= 1 && k <= kp, "als_half_sweep_implicit: need 1 <= k <= kp (k=%d kp=%d)", k, kp);
  HREC_REQUIRE(n_rows >= 0 && n_src >= 0, "als_half_sweep_implicit: negative size");
  HREC_REQUIRE(n_rows < 0x7fffffffll && n_src < 0x7fffffffll, "als_half_sweep_implicit: too many rows for one launch");
  HREC_REQUIRE(alpha >= 0.0, "als_half_sweep_implicit: alpha must be >= 0 (got %g)", alpha);
  HREC_REQUIRE(reg_param >= 0.0, "als_half_sweep_implicit: reg_param must be >= 0");
  HREC_REQUIRE(kp != 64 || n_src * (int64_t)kp * 4 <= (int64_t)0xffffffffll,
               "als_half_sweep_implicit: %lld source rows of %d floats exceed the 4 GiB a gather resource spans; "
               "shard the source side", (long long)n_src, kp);
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(indptr && dst_factors && yty, "als_half_sweep_implicit: null pointer");
  HREC_REQUIRE(n_src > 0 && src_factors && indices && values,
               "als_half_sweep_implicit: null source factors / CSR arrays");
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)n_rows), block(64);
#define HREC_SWEEP(NT, CH)                                                                                  \
  hipLaunchKernelGGL((als_half_sweep_implicit_kernel<NT, CH>), grid, block, 0, s, indptr, indices, values, \
                     n_rows, src_factors, n_src, k, reg_param, alpha, yty, dst_factors)
  if (kp == 64) HREC_SWEEP(4, HREC_ALS_CH0);
  else if (kp == 32) HREC_SWEEP(2, 8);
  else HREC_SWEEP(1, 8);
#undef HREC_SWEEP
  return check_launch("als_half_sweep_implicit_kernel");
}

extern "C" int hrec_f32_to_f64(const float* in, int64_t n, double* out, void* stream) {
  HREC_REQUIRE(n >= 0, "f32_to_f64: negative size");
  if (n == 0) return HREC_OK;
  HREC_REQUIRE(in && out, "f32_to_f64: null pointer");
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(f32_to_f64_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), in, n, out);
  return check_launch("f32_to_f64_kernel");
}

extern "C" int hrec_als_half_sweep_src64(const int64_t* indptr, const int32_t* indices, const float* values,
                                         int64_t n_rows, const double* src64, int64_t n_src, int k, int kp,
                                         double reg_param, float* dst_factors, void* stream) {
  HREC_REQUIRE(kp == 64, "als_half_sweep_src64: kp must be 64 (got %d)", kp);
  HREC_REQUIRE(k >= 1 && k <= kp, "als_half_sweep_src64: need 1 <= k <= kp (k=%d kp=%d)", k, kp);
  HREC_REQUIRE(n_rows >= 0 && n_src >= 0, "als_half_sweep_src64: negative size");
  HREC_REQUIRE(n_rows < 0x7fffffffll && n_src < 0x7fffffffll, "als_half_sweep_src64: too many rows for one launch");
  HREC_REQUIRE(n_src * (int64_t)kp * 8 <= (int64_t)0xffffffffll,
               "als_half_sweep_src64: %lld f64 source rows exceed the 4 GiB a gather resource spans", (long long)n_src);
  HREC_REQUIRE(reg_param >= 0.0, "als_half_sweep_src64: reg_param must be >= 0");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(indptr && dst_factors, "als_half_sweep_src64: null pointer");
  HREC_REQUIRE(n_src > 0 && src64 && indices && values, "als_half_sweep_src64: null source factors / CSR arrays");
  HREC_REQUIRE(((uintptr_t)src64 & 15) == 0, "als_half_sweep_src64: src64 must be 16-B aligned");
  hipLaunchKernelGGL((als_half_sweep_f64_kernel<4, HREC_ALS_CH0, 0, true>), dim3((unsigned)n_rows), dim3(64), 0,
                     as_stream(stream), indptr, indices, values, n_rows, reinterpret_cast<const float*>(src64), n_src,
                     k, reg_param, dst_factors);
  return check_launch("als_half_sweep_f64_kernel (f64 sources)");
}

extern "C" int hrec_transpose_f32(const float* in, int64_t rows, int64_t cols, float* out, int64_t ld_out,
                                  void* stream) {
  HREC_REQUIRE(rows >= 0 && cols >= 0, "transpose: negative size");
  HREC_REQUIRE(ld_out >= rows, "transpose: ld_out < rows");
  if (rows == 0 || cols == 0) return HREC_OK;
  HREC_REQUIRE(in && out, "transpose: null pointer");
  const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((cols + 63) / 64)), block(256);
  hipLaunchKernelGGL(transpose_kernel, grid, block, 0, as_stream(stream), in, rows, cols, out, ld_out);
  return check_launch("transpose_kernel");
}

#ifdef HREC_ALS_STAMPS
extern "C" int hrec_debug_als_stamps(unsigned long long* host_out, int reset) {
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_als_stamps), sizeof(g_als_stamps)) != hipSuccess) return -2;
  if (reset) {
    unsigned long long z[8] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_als_stamps), z, sizeof(z)) != hipSuccess) return -2;
  }
  return 0;
}
#endif
