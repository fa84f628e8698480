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
#include <mutex>

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
    gram_row<NT, CH, MODE, S64, true>(beg, end, lane, indices, values, src, n_src, k, reg, acc, bsh, lds, alpha, yty,
                                      &n_pos);
    if (n_pos == 0) {  // no rating > 0: b = 0, the factor is exactly zero (wave-uniform)
      if (lane < KP) out[lane] = 0.f;
      return;
    }
  } else {
    gram_row<NT, CH, MODE, S64>(beg, end, lane, indices, values, src, n_src, k, reg, acc, bsh, lds);
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

// ---- pooled kernel: three waves per SIMD, 12 waves sharing 8 LDS slices ----
// A wave needs its LDS slice only from the end of its Gramian (the staging of
// the diagonal tiles) to the last read of the back substitution, so the 12
// waves of a CU (3 per SIMD, <= 168 VGPRs: factor_row_lds keeps the Gramian in
// the slice) share 8 slices of RowLds<64>::kSize doubles = 153,600 B. Each SIMD class
// (wave index & 3: waves are placed round-robin over the 4 SIMDs,
// scripts/micro/hwid_probe.hip; another placement would only cost speed) owns
// 2 slices, so at most 2 of a SIMD's 3 waves are in their epilogue / solve and
// one Gramian stream always feeds the SIMD's f64 pipe (f64 sources: a wave
// whose class has none free may borrow another class's, HREC_ALS_POOL_ANY64).
// A wave without a slice sleeps; it holds none, so the holders always finish:
// no deadlock.
// 1 = a wave may take any free slice (its class's two first), so all 3 waves
// of a SIMD may be in their solves; per source type (measured)
#ifndef HREC_ALS_POOL_ANY32
#define HREC_ALS_POOL_ANY32 0
#endif
#ifndef HREC_ALS_POOL_ANY64
#define HREC_ALS_POOL_ANY64 1
#endif
#ifndef HREC_ALS_POOL_SLEEP
#define HREC_ALS_POOL_SLEEP 8  // s_sleep argument (x 64 cycles) between two tries for a slice
#endif
constexpr int kPoolWaves = 12, kPoolSlices = 8;
constexpr size_t kPoolLdsBytes = (size_t)kPoolSlices * RowLds<64>::kSize * sizeof(double);

// One of the class's two slices (wave-uniform); busy[] lives in LDS.
template <bool ANY>
__device__ __forceinline__ int slice_acquire(int* busy, int cls, int lane) {
  int slot, zero = 0;
  asm volatile("" : "+v"(zero));  // not the accumulators' zero tuple kept live for this
  for (;;) {
    int got = -1;
    if (lane == 0) {
      for (int i = 0; i < (ANY ? kPoolSlices : 2) && got < 0; ++i) {
        const int sl = (2 * cls + i) % kPoolSlices;
        if (atomicCAS(&busy[sl], zero, 1) == 0) got = sl;
      }
    }
    slot = __builtin_amdgcn_readfirstlane(got);
    if (slot >= 0) break;
    __builtin_amdgcn_s_sleep(HREC_ALS_POOL_SLEEP);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return slot;
}

// After the wave's last access to the slice (a wave's LDS operations complete
// in issue order, so the flag clears behind them).
__device__ __forceinline__ void slice_release(int* busy, int slot, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (lane == 0) atomicExch(&busy[slot], 0);
}

// Persistent: one 12-wave workgroup per CU; every wave claims whole rows, one
// ticket per row from *ticket (zeroed before the launch, private to it), and
// carries nothing from row to row. Same arithmetic as the one-wave kernel
// (gram_row, then factor_row_lds = factor_row's operations): the same bits.
template <bool S64>
__global__ __launch_bounds__(64 * kPoolWaves, 3) void als_half_sweep_f64_kernel_pooled(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const float* __restrict__ values,
    int64_t n_rows, const float* __restrict__ src, int64_t n_src, int k, double reg, float* __restrict__ dst,
    unsigned* __restrict__ ticket) {
  constexpr int NT = 4, KP = 64;
  extern __shared__ __attribute__((aligned(16))) double pool[];
  __shared__ int busy[kPoolSlices];
  if (threadIdx.x < kPoolSlices) busy[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int cls = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & 3;
  for (;;) {
    unsigned t = 0;
    if (lane == 0) t = atomicAdd(ticket, 1u);
    const int64_t row = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)t);
    if (row >= n_rows) return;
    const int64_t beg = indptr[row];
    const int64_t end = indptr[row + 1];
    float* __restrict__ out = dst + row * KP;
    if (end == beg) {
      if (lane < KP) out[lane] = 0.f;
      continue;
    }
    // The row loop makes everything that depends on the lane alone loop
    // invariant (the solve's address offsets and lane masks): hoisted out, it
    // would stay live through the Gramian and spill. An opaque copy of the
    // lane per phase keeps each phase's values inside it.
    int gl = lane, fl = lane;
    asm volatile("" : "+v"(gl));
    d4 acc[NT * (NT + 1) / 2];
    int slot = -1;
    auto acquire = [&]() -> double* {
      slot = slice_acquire<S64 ? HREC_ALS_POOL_ANY64 != 0 : HREC_ALS_POOL_ANY32 != 0>(busy, cls, lane);
      return pool + slot * RowLds<KP>::kSize;
    };
    // the slice is taken inside gram_row, when the Gramian loop is done
    gram_row<NT, HREC_ALS_CH0, 0, S64, false, true>(beg, end, gl, indices, values, src, n_src, k, reg, acc, nullptr,
                                                    nullptr, 0.0, nullptr, nullptr, acquire);
    double* lds = pool + slot * RowLds<KP>::kSize;
    double* scratch = lds + RowLds<KP>::kUpPad;
    asm volatile("" : "+v"(fl));
    factor_row_lds<NT>(fl, acc, lds, scratch, scratch + 128 + 2 * KP, out);
    slice_release(busy, slot, lane);
  }
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

namespace {

// The pooled kernel's row tickets: one word per launch out of a ring of device
// words the library owns (per device, allocated at the first pooled launch),
// zeroed on the launch's own stream right before the kernel. Launches on
// different streams never share a word unless kTicketRing later launches are
// enqueued while one is still running.
constexpr int kTicketRing = 4096;
constexpr int kMaxDevices = 64;

struct PoolDevice {
  unsigned* ring = nullptr;
  unsigned next = 0;
  int cus = 0;
};

int pooled_ticket(unsigned** word, int* cus) {
  static std::mutex mu;
  static PoolDevice devs[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
    set_error("als_half_sweep (pooled): no current device");
    return HREC_E_LAUNCH;
  }
  std::lock_guard<std::mutex> lock(mu);
  PoolDevice& d = devs[dev];
  if (!d.ring) {
    if (hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || d.cus < 1 ||
        hipMalloc(&d.ring, kTicketRing * sizeof(unsigned)) != hipSuccess) {
      d.ring = nullptr;
      return check_launch("als_half_sweep (pooled): ticket words");
    }
  }
  *word = d.ring + (d.next++ % kTicketRing);
  *cus = d.cus;
  return HREC_OK;
}

template <bool S64>
int launch_pooled(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                  const float* src, int64_t n_src, int k, double reg, float* dst, hipStream_t s) {
  auto kfn = als_half_sweep_f64_kernel_pooled<S64>;
  if (!allow_max_lds(kfn)) return check_launch("als_half_sweep_f64_kernel_pooled: LDS attribute");
  unsigned* ticket = nullptr;
  int cus = 0;
  const int rc = pooled_ticket(&ticket, &cus);
  if (rc != HREC_OK) return rc;
  if (hipMemsetAsync(ticket, 0, sizeof(unsigned), s) != hipSuccess)
    return check_launch("als_half_sweep_f64_kernel_pooled: memset");
  const int64_t need = (n_rows + kPoolWaves - 1) / kPoolWaves;
  const dim3 grid((unsigned)(need < cus ? need : cus)), block(64 * kPoolWaves);
  hipLaunchKernelGGL(kfn, grid, block, kPoolLdsBytes, s, indptr, indices, values, n_rows, src, n_src, k, reg, dst,
                     ticket);
  return check_launch("als_half_sweep_f64_kernel_pooled");
}

// Which kernel a kp-64, accum_mode-0 half-sweep takes (0 = one wave per row,
// 1 = pooled), from the launch's shape alone. Measured on one MI355X (DESIGN
// §3, "three waves per SIMD"): at c2 the pooled kernel wins on both sides
// (item side, 100k rows of ~5000 ratings, f32 sources: 35.65 -> 35.1 ms; user
// side, 1M rows of ~500, f64 sources: 41.55 -> 41.05 ms); at c2s (20k rows of
// ~500 and 100k rows of ~100) the two tie within the run-to-run noise, and
// below a few rows per resident wave (12 x CUs) a persistent grid cannot
// balance. So: pooled from 65536 rows on, for either source type.
constexpr int64_t kPooledMinRows = 65536;
constexpr bool kPooledF32 = true;  // f32 sources
constexpr bool kPooledF64 = true;  // f64 sources
inline int pick_kernel(bool s64, int64_t n_rows) {
  return (s64 ? kPooledF64 : kPooledF32) && n_rows >= kPooledMinRows ? 1 : 0;
}

}  // namespace

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
  if (kp == 64 && accum_mode == 0 && pick_kernel(false, n_rows) == 1)
    return launch_pooled<false>(indptr, indices, values, n_rows, src_factors, n_src, k, reg_param, dst_factors, s);
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

// kernel: -1 = by pick_kernel, 0 = one wave per row, 1 = pooled.
static int half_sweep_src64(const char* name, const int64_t* indptr, const int32_t* indices, const float* values,
                            int64_t n_rows, const double* src64, int64_t n_src, int k, int kp, double reg_param,
                            int kernel, float* dst_factors, void* stream) {
  HREC_REQUIRE(kp == 64, "%s: kp must be 64 (got %d)", name, kp);
  HREC_REQUIRE(k >= 1 && k <= kp, "%s: need 1 <= k <= kp (k=%d kp=%d)", name, k, kp);
  HREC_REQUIRE(n_rows >= 0 && n_src >= 0, "%s: negative size", name);
  HREC_REQUIRE(n_rows < 0x7fffffffll && n_src < 0x7fffffffll, "%s: too many rows for one launch", name);
  HREC_REQUIRE(n_src * (int64_t)kp * 8 <= (int64_t)0xffffffffll,
               "%s: %lld f64 source rows exceed the 4 GiB a gather resource spans", name, (long long)n_src);
  HREC_REQUIRE(reg_param >= 0.0, "%s: reg_param must be >= 0", name);
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(indptr && dst_factors, "%s: null pointer", name);
  HREC_REQUIRE(n_src > 0 && src64 && indices && values, "%s: null source factors / CSR arrays", name);
  HREC_REQUIRE(((uintptr_t)src64 & 15) == 0, "%s: src64 must be 16-B aligned", name);
  if (kernel < 0) kernel = pick_kernel(true, n_rows);
  if (kernel == 1)
    return launch_pooled<true>(indptr, indices, values, n_rows, reinterpret_cast<const float*>(src64), n_src, k,
                               reg_param, dst_factors, as_stream(stream));
  hipLaunchKernelGGL((als_half_sweep_f64_kernel<4, HREC_ALS_CH0, 0, true>), dim3((unsigned)n_rows), dim3(64), 0,
                     as_stream(stream), indptr, indices, values, n_rows, reinterpret_cast<const float*>(src64), n_src,
                     k, reg_param, dst_factors);
  return check_launch("als_half_sweep_f64_kernel (f64 sources)");
}

extern "C" int hrec_als_half_sweep_src64(const int64_t* indptr, const int32_t* indices, const float* values,
                                         int64_t n_rows, const double* src64, int64_t n_src, int k, int kp,
                                         double reg_param, float* dst_factors, void* stream) {
  return half_sweep_src64("als_half_sweep_src64", indptr, indices, values, n_rows, src64, n_src, k, kp, reg_param, -1,
                          dst_factors, stream);
}

extern "C" int hrec_als_half_sweep_kernel(const int64_t* indptr, const int32_t* indices, const float* values,
                                          int64_t n_rows, const void* src, int src_f64, int64_t n_src, int k, int kp,
                                          double reg_param, int kernel, float* dst_factors, void* stream) {
  HREC_REQUIRE(kernel == 0 || kernel == 1, "als_half_sweep_kernel: kernel must be 0 (one wave per row) or 1 (pooled), got %d",
               kernel);
  HREC_REQUIRE(kp == 64, "als_half_sweep_kernel: kp must be 64 (got %d)", kp);
  if (src_f64)
    return half_sweep_src64("als_half_sweep_kernel", indptr, indices, values, n_rows, static_cast<const double*>(src),
                            n_src, k, kp, reg_param, kernel, dst_factors, stream);
  HREC_REQUIRE(k >= 1 && k <= kp, "als_half_sweep_kernel: need 1 <= k <= kp (k=%d kp=%d)", k, kp);
  HREC_REQUIRE(n_rows >= 0 && n_src >= 0, "als_half_sweep_kernel: negative size");
  HREC_REQUIRE(n_rows < 0x7fffffffll && n_src < 0x7fffffffll, "als_half_sweep_kernel: too many rows for one launch");
  HREC_REQUIRE(n_src * (int64_t)kp * 4 <= (int64_t)0xffffffffll,
               "als_half_sweep_kernel: %lld source rows exceed the 4 GiB a gather resource spans", (long long)n_src);
  HREC_REQUIRE(reg_param >= 0.0, "als_half_sweep_kernel: reg_param must be >= 0");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(indptr && dst_factors, "als_half_sweep_kernel: null pointer");
  HREC_REQUIRE(n_src > 0 && src && indices && values, "als_half_sweep_kernel: null source factors / CSR arrays");
  const float* src32 = static_cast<const float*>(src);
  if (kernel == 1)
    return launch_pooled<false>(indptr, indices, values, n_rows, src32, n_src, k, reg_param, dst_factors,
                                as_stream(stream));
  hipLaunchKernelGGL((als_half_sweep_f64_kernel<4, HREC_ALS_CH0, 0>), dim3((unsigned)n_rows), dim3(64), 0,
                     as_stream(stream), indptr, indices, values, n_rows, src32, n_src, k, reg_param, dst_factors);
  return check_launch("als_half_sweep_f64_kernel");
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
