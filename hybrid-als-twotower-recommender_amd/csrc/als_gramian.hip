// Source Gramian of the implicit-feedback half-sweep (Spark 3.5 ALS
// computeYtY: NormalEquation.add(y, 0.0) over every source factor):
//   YtY = sum_s y_s y_s^T  (f64),  y_s = src[s][0..kp) converted to f64.
//
// A tall-skinny SYRK on v_mfma_f64_16x16x4_f64, with 4 source rows as the K
// dimension of a step (the operand layout of csrc/als.hip: lane l holds row
// l >> 4 of the step, columns NT * (l & 15) .. + NT - 1, so component T of the
// lane's vector is the A and the B operand of tile T). Pass 1: one workgroup
// per slab of kGramSlab rows, its 4 waves take the slab's steps round-robin,
// their accumulators are summed in wave order through LDS and stored as the
// slab's partial (tile layout) in the workspace. Pass 2: every output element
// sums its partials in slab order. No atomics and no hand-off inside a
// launch; the slabs depend on n_src and kp alone, so equal buffers give equal
// bits on every call, device and rank.
#include "common.h"

namespace hrec {

typedef double gd4 __attribute__((ext_vector_type(4)));

constexpr int kGramSlab = 2048;  // source rows per workgroup (512 steps, 128 per wave)
constexpr int kGramUnroll = 4;   // steps whose loads are in flight per wave

inline int64_t gram_slabs(int64_t n_src) { return (n_src + kGramSlab - 1) / kGramSlab; }
inline size_t gram_partial_doubles(int kp) {
  const int nt = kp / 16;
  return (size_t)(nt * (nt + 1) / 2) * 256;
}

template <int NT>
__device__ __forceinline__ void gram_load(const float* __restrict__ src, int64_t row, int64_t n_src, int col,
                                          double (&a)[NT]) {
  constexpr int KP = 16 * NT;
  if (row >= n_src) {
#pragma unroll
    for (int t = 0; t < NT; ++t) a[t] = 0.0;
    return;
  }
  const float* p = src + row * KP + NT * col;
  if constexpr (NT == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    a[0] = (double)v.x, a[1] = (double)v.y, a[2] = (double)v.z, a[3] = (double)v.w;
  } else if constexpr (NT == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    a[0] = (double)v.x, a[1] = (double)v.y;
  } else {
    a[0] = (double)*p;
  }
}

template <int NT>
__global__ __launch_bounds__(256) void gramian_slab_kernel(const float* __restrict__ src, int64_t n_src,
                                                           double* __restrict__ partials) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  __shared__ double red[NPAIR * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane >> 4, col = lane & 15;
  const int64_t row0 = (int64_t)blockIdx.x * kGramSlab;
  gd4 acc[NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) acc[p] = gd4{0.0, 0.0, 0.0, 0.0};
  // wave w: steps w, w + 4, ... of the slab's kGramSlab / 4 (the steps past
  // n_src load zeros, so every wave runs the same trip count)
  for (int s0 = wave; s0 < kGramSlab / 4; s0 += 4 * kGramUnroll) {
    double a[kGramUnroll][NT];
#pragma unroll
    for (int u = 0; u < kGramUnroll; ++u) gram_load<NT>(src, row0 + 4 * (int64_t)(s0 + 4 * u) + sub, n_src, col, a[u]);
#pragma unroll
    for (int u = 0; u < kGramUnroll; ++u) {
      int p = 0;
#pragma unroll
      for (int I = 0; I < NT; ++I) {
#pragma unroll
        for (int J = I; J < NT; ++J) {
          acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][I], a[u][J], acc[p], 0, 0, 0);
          ++p;
        }
      }
    }
    if (row0 + 4 * (int64_t)(s0 + 4 * kGramUnroll) >= n_src) break;  // the rest of the slab is past the end
  }
  // waves 1, 2, 3 -> wave 0, in that order
  for (int w = 1; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int p = 0; p < NPAIR; ++p) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) red[p * 256 + rr * 64 + lane] = acc[p][rr];
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int p = 0; p < NPAIR; ++p) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[p][rr] += red[p * 256 + rr * 64 + lane];
      }
    }
    __syncthreads();
  }
  if (wave == 0) {
    double* out = partials + (size_t)blockIdx.x * (NPAIR * 256);
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) out[p * 256 + rr * 64 + lane] = acc[p][rr];
    }
  }
}

// One workgroup per 64 elements of the tile layout: wave w sums the slabs
// s = w (mod 4) in ascending order, the four sums are added in wave order.
// Element (tile p = (I, J), register rr, lane) is G[NT i + I][NT j + J] with
// i = (lane >> 4) + 4 rr, j = lane & 15; it is stored with its mirror. Rows
// and columns >= k are written as zero.
template <int NT>
__global__ __launch_bounds__(256) void gramian_reduce_kernel(const double* __restrict__ partials, int64_t n_slabs,
                                                             int k, double* __restrict__ yty) {
  constexpr int KP = 16 * NT;
  constexpr int NPAIR = NT * (NT + 1) / 2;
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;  // < NPAIR * 256
  double sum = 0.0;
  for (int64_t s = wave; s < n_slabs; s += 4) sum += partials[(size_t)s * (NPAIR * 256) + e];
  red[wave][lane] = sum;
  __syncthreads();
  if (wave != 0) return;
  sum = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
  const int p = e >> 8, rr = (e >> 6) & 3;
  int I = 0, J = 0;
  for (int q = 0, i2 = 0; i2 < NT; ++i2) {
    for (int j2 = i2; j2 < NT; ++j2, ++q) {
      if (q == p) I = i2, J = j2;
    }
  }
  const int i = (lane >> 4) + 4 * rr, j = lane & 15;
  const int r = NT * i + I, c = NT * j + J;
  if (I == J && i > j) return;  // a diagonal tile holds both triangles: keep the upper one
  const double v = (r < k && c < k) ? sum : 0.0;
  yty[r * KP + c] = v;
  yty[c * KP + r] = v;
}

}  // namespace hrec

using namespace hrec;

static bool gram_kp_ok(int kp) { return kp == 16 || kp == 32 || kp == 64; }

extern "C" size_t hrec_als_gramian_workspace_bytes(int64_t n_src, int kp) {
  if (n_src < 0 || !gram_kp_ok(kp)) return 0;
  const int64_t slabs = gram_slabs(n_src);
  return al256((size_t)(slabs > 0 ? slabs : 1) * gram_partial_doubles(kp) * sizeof(double));
}

extern "C" int hrec_als_gramian(const float* src_factors, int64_t n_src, int k, int kp, double* yty, void* workspace,
                                size_t workspace_bytes, void* stream) {
  HREC_REQUIRE(gram_kp_ok(kp), "als_gramian: kp must be 16, 32 or 64 (implicit feedback supports rank <= 64; got kp %d)",
               kp);
  HREC_REQUIRE(k >= 1 && k <= kp, "als_gramian: need 1 <= k <= kp (k=%d kp=%d)", k, kp);
  HREC_REQUIRE(n_src >= 0, "als_gramian: negative size");
  HREC_REQUIRE(n_src < 0x7fffffffll, "als_gramian: too many source rows");
  HREC_REQUIRE(yty && workspace, "als_gramian: null output or workspace");
  HREC_REQUIRE(n_src == 0 || src_factors, "als_gramian: null source factors");
  HREC_REQUIRE(workspace_bytes >= hrec_als_gramian_workspace_bytes(n_src, kp),
               "als_gramian: workspace of %zu bytes, need %zu", workspace_bytes,
               hrec_als_gramian_workspace_bytes(n_src, kp));
  HREC_REQUIRE(((uintptr_t)src_factors & 15) == 0, "als_gramian: src_factors must be 16-B aligned");
  hipStream_t s = as_stream(stream);
  const int64_t slabs = gram_slabs(n_src);
  double* part = static_cast<double*>(workspace);
  const int nt = kp / 16;
  const unsigned red_blocks = (unsigned)(nt * (nt + 1) / 2 * 4);
#define HREC_GRAM(NT)                                                                                            \
  do {                                                                                                           \
    if (slabs > 0)                                                                                               \
      hipLaunchKernelGGL((gramian_slab_kernel<NT>), dim3((unsigned)slabs), dim3(256), 0, s, src_factors, n_src, \
                         part);                                                                                  \
    hipLaunchKernelGGL((gramian_reduce_kernel<NT>), dim3(red_blocks), dim3(256), 0, s, part, slabs, k, yty);    \
  } while (0)
  if (kp == 64) HREC_GRAM(4);
  else if (kp == 32) HREC_GRAM(2);
  else HREC_GRAM(1);
#undef HREC_GRAM
  return check_launch("gramian kernels");
}
