// Cosine neighbours of rows of one matrix (hrec_cosine_topk): per query row
// the stable top-k of sim(q, j) over every row j, the query itself left out
// on request, cut at a minimum similarity. include/hrec.h has the contract.
//   dot(q, j) = the f64 chain acc = acc + (double)v_q[c] * (double)v_j[c], c
//               ascending from 0.0 (a product of two f32 values is exact in
//               f64, so the chain has one rounding per step, fused or not);
//   sim(q, j) = (dot * inv_norm[q]) * inv_norm[j], +0.0 where either is 0.
//
// Exhaustive arm (mode 1; small catalogues; the fallback): cos_sims_kernel
// writes the f64 sims of a sub-batch of queries to the workspace, the query's
// own column as NaN (better() ranks NaN last, and kk <= n - 1 then), and the
// f64 stable top-k (csrc/topk.hip) ranks the rows. A block owns 256 items,
// one per thread, and kCosQ queries whose components cos_stage_kernel wrote
// as f64, component-major: the item rows are staged in LDS by coalesced loads,
// a thread reads its own row from there and runs kCosQ independent chains,
// the query components arriving as scalar operands (cos_sims_kernel has the
// reasons).
//
// Pruned arm (mode 2), the cascade of csrc/cascade.h as in csrc/als_prune.hip:
// the unit rows are prepared once per matrix as bf16 (hrec_cosine_items), a
// query's operand is its own prepared row, and s~(q, j) is their dot on the
// bf16 matrix cores with f32 accumulation.
//   The bound E. Write x_c = v_c * inv_norm (real arithmetic) for the scaled
//   components of a row with inv_norm != 0; sum_c |x_qc x_jc| <= |x_q| |x_j|
//   <= (1 + 2^-40)^2, since inv_norm is 1 / sqrt of an f64 sum of d <= 256
//   squares (relative error below 2^-44). The four sources of error:
//   1. the prepared component is bf16(f32(v_c * inv_norm)): the f64 product
//      and its f32 rounding are within 2^-24 + 2^-52 of x_c relatively, the
//      bf16 rounding (8 significant bits, to nearest even) within 2^-8 of
//      that, so xh_c = x_c (1 + e), |e| <= delta = 2^-8 + 2^-23;
//   2. a product of two such operands is within 2 delta + delta^2 <= 2^-7 +
//      2^-15 of x_qc x_jc relatively, and is exact in f32 (16 bits);
//   3. the f32 accumulation of dk <= 256 such products in any order is within
//      2 * 256 * 2^-24 = 2^-15 of their sum relative to sum |xh_qc xh_jc| <=
//      (1 + 2^-6) sum |x_qc x_jc| (twice the textbook bound: it also covers an
//      accumulator that truncates);
//   4. the exact value: the f64 chain is within d 2^-53 sum |v_qc v_jc| of
//      v_q . v_j and the two multiplications add 2^-52 relatively: below
//      2^-44 sum |x_qc x_jc| together.
//   Sum: |s~ - sim| <= (2^-7 + 2^-15 + 2^-15 (1 + 2^-6) + 2^-44) (1 + 2^-40)^2
//   < 2^-7 + 2^-13 =: E, an absolute constant; + 1e-30 for components that
//   are subnormal in f32 or products the matrix cores flush (each below
//   2^-126, 256 of them). A row with inv_norm == 0 is a zero operand: s~ = 0
//   and sim = +0.0 exactly.
//   1. t_b = (a lower bound of) the kk-th best s~ over the first S rows, the
//      query's own column excluded (a one-column exclusion CSR built per
//      call; cascade_bound has the argument): kk rows other than the query
//      have sim >= s~ - E >= t_b - E =: tau_b;
//   2. the matrix-core filter (dot_filter_run) at down(tau_b - E) keeps every
//      row whose sim can reach tau_b;
//   3. cos_rescore_kernel runs the exact chain over the kept rows; those with
//      sim >= tau_b (the query's own row dropped) are the candidates, a
//      superset of the top kk;
//   4. the f64 stable top-k of the candidates, ties -> the smaller column.
//   A zero query (inv_norm 0) ties with every row at +0.0, which no margin can
//   prune: it keeps nothing and cos_finish_kernel writes its list, the columns
//   in order without its own, directly.
//   A kept list past kCosCap, or fewer than kk candidates, raises *overflow:
//   the caller reruns the batch in mode 1 (hrec_als_score_topk_pruned's
//   convention).
// Both arms end in cos_finish_kernel: the ranked prefix with sim > min_sim,
// -1 / NaN behind it. No floating-point atomics anywhere; the filter's lists
// are in arrival order, but a stable top-k over (value, column) does not
// depend on it: equal inputs give equal bits on every call and in every mode.
#include "cascade.h"
#include "order.h"  // bf16_rne, f32_down
#include "wave.h"   // lanes_below

#pragma clang fp contract(off)

namespace hrec {

constexpr int kCosMaxD = 256;
constexpr int kCosTopMax = 1024;
constexpr double kCosE = 0x1p-7 + 0x1p-13 + 1e-30;
constexpr int kCosCap = 4096;      // kept rows per query
constexpr int kCosSample = 8192;   // rows of the sample bound, kk <= 64 (lane maxima)
constexpr int kCosSampleK = 32768; // kk > 64 (the exact kk-th: about kk n / S rows beat it)
constexpr int kCosSampleUB = 64;   // resident queries per block of the sample's dot
constexpr int kCosQ = 16;          // chains per thread of the exhaustive kernel
// queries of one exhaustive sub-batch: their f64 sims fit this many bytes
constexpr size_t kCosSimBytes = (size_t)512 << 20;
// auto (mode 0): catalogues below this take the exhaustive arm. Measured on
// MI355X, 4096 queries, top 10, d = 64, pruned / exhaustive ms per call: n 1024
// 0.565 / 0.094, 2048 0.182 / 0.159, 3072 0.203 / 0.338, 4096 0.214 / 0.480,
// 8192 0.223 / 0.900, 16384 0.227 / 1.232, 100000 0.629 / 7.783
// (profiles/similar_quick_c2.txt).
constexpr int64_t kCosAutoCut = 3072;

__host__ __device__ constexpr int cos_dk(int d) { return d <= 32 ? 32 : (d <= 64 ? 64 : (d <= 128 ? 128 : 256)); }

// The prepared operand: bf16 unit rows [n][dk], zero beyond d and where
// inv_norm is 0. One wave per row, a lane per pair of columns: the row is
// read and written by consecutive lanes.
__global__ __launch_bounds__(256) void cos_items_kernel(const float* __restrict__ vectors, int64_t n, int d,
                                                        int64_t ld, const double* __restrict__ inv_norm, int dk,
                                                        uint16_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  const double inv = inv_norm[row];
  const float* __restrict__ v = vectors + row * ld;
  uint32_t* __restrict__ o = reinterpret_cast<uint32_t*>(out + row * dk);
  for (int c = 2 * lane; c < dk; c += 128) {
    const float x0 = (inv != 0.0 && c < d) ? (float)((double)v[c] * inv) : 0.f;
    const float x1 = (inv != 0.0 && c + 1 < d) ? (float)((double)v[c + 1] * inv) : 0.f;
    o[c >> 1] = bf16_rne(x0) | (bf16_rne(x1) << 16);
  }
}

// Per query (one wave): the checked row (-1: unknown). Pruned arm (items
// given): the query's bf16 operand, its one-column exclusion (local row b ->
// segment [b, b + 1) -> the query's own column, -1 when nothing is skipped)
// and *overflow = 0.
__global__ __launch_bounds__(256) void cos_prep_kernel(const int64_t* __restrict__ query_rows, int n_q, int64_t n,
                                                       int skip_self, const uint16_t* __restrict__ items, int dk,
                                                       int64_t* __restrict__ qrow, uint16_t* __restrict__ uop,
                                                       int64_t* __restrict__ xrows, int64_t* __restrict__ xptr,
                                                       int32_t* __restrict__ xcols, int* __restrict__ overflow) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;
  if (b >= n_q) return;  // wave-uniform
  int64_t r = query_rows[b];
  if (r < 0 || r >= n) r = -1;
  if (lane == 0) qrow[b] = r;
  if (!items) return;
  if (lane == 0) {
    xrows[b] = b;
    xptr[b] = b;
    if (b == n_q - 1) xptr[n_q] = n_q;
    xcols[b] = (skip_self && r >= 0) ? (int32_t)r : -1;
  }
  if (lane < dk / 8) {
    int4 x{0, 0, 0, 0};
    if (r >= 0) x = *reinterpret_cast<const int4*>(items + r * dk + 8 * lane);
    *reinterpret_cast<int4*>(uop + (int64_t)b * dk + 8 * lane) = x;
  }
}

// The exhaustive arm's query operand: qf[g][c][q] = (double)v[row of query g * kCosQ + q][c] (0.0 for an unknown
// or absent query), one block per group g of kCosQ queries.
__global__ __launch_bounds__(256) void cos_stage_kernel(const float* __restrict__ vectors, int d, int64_t ld,
                                                        const int64_t* __restrict__ qrow, int n_q,
                                                        double* __restrict__ qf) {
  const int q0 = blockIdx.x * kCosQ;
  for (int o = threadIdx.x; o < d * kCosQ; o += 256) {
    const int c = o / kCosQ, q = o % kCosQ;
    const int64_t r = q0 + q < n_q ? qrow[q0 + q] : -1;
    qf[(int64_t)blockIdx.x * d * kCosQ + o] = r >= 0 ? (double)vectors[r * ld + c] : 0.0;
  }
}

// The exhaustive arm's sims: block (x: 256 items, y: kCosQ queries), one item
// per thread, kCosQ chains per thread. The block's item rows pass through LDS
// in tiles of kCosTC components: whole 128-B lines loaded by consecutive lanes,
// then read back one row per lane (row stride kCosTC + 1 dwords: the lanes hit
// distinct banks). A lane reading its own row straight from global memory
// touches 64 cache lines per load and the 256 rows of a block do not fit the
// vector cache, so every line came from L2 eight times: 11.2 ms per 4096 x
// 100k x 64 call, against the numbers in profiles/similar_quick_c2.txt.
// The queries' f64 components are the same for every lane, read through
// wave-uniform addresses of a buffer no launch of this kernel writes, so the
// compiler can keep them in scalar registers: in the build that was measured
// the loop is s_load_dwordx16 feeding v_fma_f64 with a scalar operand (read
// from the device assembly; nothing in the build enforces it, and the result
// does not depend on it). The product of two f32 values is exact in f64: a
// fused step has the chain's bits.
constexpr int kCosTC = 32;

__global__ __launch_bounds__(256) void cos_sims_kernel(const float* __restrict__ vectors, int64_t n, int d,
                                                       int64_t ld, const double* __restrict__ inv_norm,
                                                       const int64_t* __restrict__ qrow,
                                                       const double* __restrict__ qf, int n_q, int skip_self,
                                                       double* __restrict__ sims) {
  __shared__ float tile[256 * (kCosTC + 1)];
  __shared__ double s_inq[kCosQ];
  __shared__ int64_t s_r[kCosQ];
  const int q0 = blockIdx.y * kCosQ;
  const int64_t j0 = (int64_t)blockIdx.x * 256;
  const int64_t j = j0 + threadIdx.x;
  const double* __restrict__ cos_sq = qf + (int64_t)blockIdx.y * d * kCosQ;  // [d][kCosQ], wave-uniform
  if (threadIdx.x < kCosQ) {
    const int64_t r = q0 + (int)threadIdx.x < n_q ? qrow[q0 + threadIdx.x] : -1;
    s_r[threadIdx.x] = r;
    s_inq[threadIdx.x] = r >= 0 ? inv_norm[r] : 0.0;
  }
  double acc[kCosQ];
#pragma unroll
  for (int q = 0; q < kCosQ; ++q) acc[q] = 0.0;
  const float* __restrict__ mine = tile + threadIdx.x * (kCosTC + 1);
  for (int c0 = 0; c0 < d; c0 += kCosTC) {  // block-uniform
    const int cw = d - c0 < kCosTC ? d - c0 : kCosTC;
    __syncthreads();  // the previous tile's readers are done
    if (cw == kCosTC) {  // a whole tile: row and column by shifts
      for (int e = threadIdx.x; e < 256 * kCosTC; e += 256) {
        const int row = e / kCosTC, cc = e % kCosTC;
        tile[row * (kCosTC + 1) + cc] = j0 + row < n ? vectors[(j0 + row) * ld + c0 + cc] : 0.f;
      }
    } else {  // the last tile of a d that is no multiple of kCosTC
      for (int e = threadIdx.x; e < 256 * cw; e += 256) {
        const int row = e / cw, cc = e - row * cw;
        tile[row * (kCosTC + 1) + cc] = j0 + row < n ? vectors[(j0 + row) * ld + c0 + cc] : 0.f;
      }
    }
    __syncthreads();
    const double* __restrict__ s = cos_sq + (int64_t)c0 * kCosQ;
    for (int cc = 0; cc < cw; ++cc) {
      const double x = (double)mine[cc];
#pragma unroll
      for (int q = 0; q < kCosQ; ++q) acc[q] = __builtin_fma(s[cc * kCosQ + q], x, acc[q]);
    }
  }
  __syncthreads();  // s_r / s_inq (d >= 1: also ordered by the tile barriers)
  if (j >= n) return;
  const double inj = inv_norm[j];
  const double qnan = __builtin_nan("");
#pragma unroll
  for (int q = 0; q < kCosQ; ++q) {
    if (q0 + q >= n_q) break;  // block-uniform
    const int64_t r = s_r[q];
    const double inq = s_inq[q];
    double sim = (inq == 0.0 || inj == 0.0) ? 0.0 : (acc[q] * inq) * inj;
    if (r < 0 || (skip_self && j == r)) sim = qnan;
    sims[(int64_t)(q0 + q) * n + j] = sim;
  }
}

// Per query: tau_b (f64, the exact test) and down(tau_b - E) (the filter's
// f32 bound). Unknown query: +inf, nothing passes; so for a zero query
// (inv_norm 0: sim +0.0 to every row, a tie no margin separates), whose list
// cos_finish_kernel writes directly. A sample without kk rows that stay
// (-inf): every row is kept.
__global__ __launch_bounds__(256) void cos_thr_kernel(int n_q, const int64_t* __restrict__ qrow,
                                                      const double* __restrict__ inv_norm,
                                                      const float* __restrict__ thr, int thr_stride,
                                                      double* __restrict__ tau, float* __restrict__ thr2) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_q) return;
  const float t = thr[(int64_t)b * thr_stride];
  double ta = __builtin_inf();
  float t2 = INFINITY;
  if (qrow[b] >= 0 && inv_norm[qrow[b]] != 0.0) {
    if (t == t && t > -INFINITY) {
      ta = (double)t - kCosE;
      t2 = f32_down(ta - kCosE);
    } else {
      ta = -__builtin_inf();
      t2 = -INFINITY;
    }
  }
  tau[b] = ta;
  thr2[b] = t2;
}

// The exact chain for every row the filter kept (one block per query, a
// thread per kept row): ev / ei hold (sim, column) where sim >= tau_b and the
// column is not the skipped query, (NaN, -1) otherwise (the top-k skips -1).
__global__ __launch_bounds__(256) void cos_rescore_kernel(const float* __restrict__ vectors, int64_t n, int d,
                                                          int64_t ld, const double* __restrict__ inv_norm,
                                                          const int64_t* __restrict__ qrow, int skip_self,
                                                          const int64_t* __restrict__ ci, const int* __restrict__ cn,
                                                          int cap, const double* __restrict__ tau, int kk,
                                                          double* __restrict__ ev, int64_t* __restrict__ ei,
                                                          int* __restrict__ overflow) {
  __shared__ double sq[kCosMaxD];
  __shared__ int s_kept;
  const int b = blockIdx.x;
  const int64_t r = qrow[b];
  if (r < 0 || inv_norm[r] == 0.0) return;  // block-uniform: unknown or zero query, the filter kept nothing
  const int cnt = cn[b];
  if (threadIdx.x == 0) {
    s_kept = 0;
    if (cnt > cap) atomicOr(overflow, 1);
  }
  for (int c = threadIdx.x; c < d; c += blockDim.x) sq[c] = (double)vectors[r * ld + c];
  __syncthreads();
  const int m = cnt < cap ? cnt : cap;
  const double inq = inv_norm[r], t = tau[b];
  const bool vec = (ld & 3) == 0 && ((uintptr_t)vectors & 15) == 0;
  const double qnan = __builtin_nan("");
  for (int e0 = 0; e0 < m; e0 += blockDim.x) {  // block-uniform trip count: the ballots see whole waves
    const int e = e0 + threadIdx.x;
    bool keep = false;
    double sim = qnan;
    int64_t j = -1;
    if (e < m) {
      j = ci[(int64_t)b * cap + e];
      if (j >= 0 && j < n && !(skip_self && j == r)) {  // an overflowed list's fillers match no row
        const float* __restrict__ v = vectors + j * ld;
        double acc = 0.0;
        int c = 0;
        if (vec) {
          for (; c + 4 <= d; c += 4) {
            const float4 x = *reinterpret_cast<const float4*>(v + c);
            acc = acc + sq[c] * (double)x.x;
            acc = acc + sq[c + 1] * (double)x.y;
            acc = acc + sq[c + 2] * (double)x.z;
            acc = acc + sq[c + 3] * (double)x.w;
          }
        }
        for (; c < d; ++c) acc = acc + sq[c] * (double)v[c];
        const double inj = inv_norm[j];
        sim = (inq == 0.0 || inj == 0.0) ? 0.0 : (acc * inq) * inj;
        keep = sim >= t;
      }
      ev[(int64_t)b * cap + e] = keep ? sim : qnan;
      ei[(int64_t)b * cap + e] = keep ? j : -1;
    }
    const uint64_t km = __ballot(keep);
    if (km && (threadIdx.x & 63) == 0) atomicAdd(&s_kept, __popcll(km));  // LDS, integer
  }
  __syncthreads();
  // fewer than kk candidates: tau_b was above the kk-th best sim (a bound slip) -> the caller's exhaustive rerun
  if (threadIdx.x == 0 && s_kept < kk) atomicOr(overflow, 1);
}

// The ranked rows ti / tv [n_q][kk] (best first; -1 or NaN where a row ran
// short) -> the outputs: the prefix with sim > min_sim, then -1 / NaN. One
// wave per query. zero_inv (the pruned arm: inv_norm; null otherwise): a query
// with inverse norm 0 has sim +0.0 to every row, so its ranking is the columns
// in order without its own, written here without a ranked row.
__global__ __launch_bounds__(256) void cos_finish_kernel(int n_q, const int64_t* __restrict__ qrow, int kk, int top_k,
                                                         double min_sim, const double* __restrict__ zero_inv,
                                                         int skip_self, const int64_t* __restrict__ ti,
                                                         const double* __restrict__ tv, int64_t* __restrict__ out_idx,
                                                         double* __restrict__ out_val, int32_t* __restrict__ out_len) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= n_q) return;  // wave-uniform
  const int64_t r = qrow[b];
  const bool known = r >= 0;
  int len = 0;
  if (known && zero_inv && zero_inv[r] == 0.0) {  // wave-uniform
    len = 0.0 > min_sim ? kk : 0;
    for (int p = lane; p < top_k; p += 64) {
      const bool in = p < len;
      out_idx[(int64_t)b * top_k + p] = in ? ((skip_self && p >= r) ? p + 1 : p) : -1;
      out_val[(int64_t)b * top_k + p] = in ? 0.0 : __builtin_nan("");
    }
    if (lane == 0) out_len[b] = len;
    return;
  }
  if (known) {
    for (int p0 = 0; p0 < kk; p0 += 64) {
      const int p = p0 + lane;
      const bool ok = p < kk && ti[(int64_t)b * kk + p] >= 0 && tv[(int64_t)b * kk + p] > min_sim;
      const uint64_t m = __ballot(ok);
      // descending values: the entries that pass are a prefix
      const int run = m == ~0ull ? 64 : __builtin_ctzll(~m);
      len += run;
      if (run < 64) break;
    }
  }
  for (int p = lane; p < top_k; p += 64) {
    const bool in = p < len;
    out_idx[(int64_t)b * top_k + p] = in ? ti[(int64_t)b * kk + p] : -1;
    out_val[(int64_t)b * top_k + p] = in ? tv[(int64_t)b * kk + p] : __builtin_nan("");
  }
  if (lane == 0) out_len[b] = len;
}

struct CosExhWs {
  int64_t* qrow;  // [n_q]
  double* qf;     // [ceil(QB / kCosQ)][d][kCosQ] f64 query components
  double* sims;   // [QB][n]
  char* tws;
  int64_t* ti;    // [QB][kk]
  double* tv;
  int qb;
  size_t total;
};

static CosExhWs cos_exh_layout(char* base, int n_q, int64_t n, int kk, int d) {
  CosExhWs w{};
  Carver c(base);
  int64_t qb = (int64_t)(kCosSimBytes / ((size_t)n * 8));
  qb = qb < 1 ? 1 : (qb > n_q ? n_q : qb);
  w.qb = (int)qb;
  w.qrow = (int64_t*)c.take((size_t)n_q * 8);
  w.qf = (double*)c.take((size_t)((qb + kCosQ - 1) / kCosQ) * kCosQ * d * 8);
  w.sims = (double*)c.take((size_t)qb * n * 8);
  w.tws = c.take(topk_ws_bytes(qb, n, kk, 8));
  w.ti = (int64_t*)c.take((size_t)qb * kk * 8);
  w.tv = (double*)c.take((size_t)qb * kk * 8);
  w.total = c.total() + 256;
  return w;
}

struct CosPruneWs {
  CascadeWs c;  // samp, the sample top-k, cv / ci / cn: the filter's kept rows
  int64_t* qrow;
  int64_t* xrows;  // the one-column exclusion
  int64_t* xptr;
  int32_t* xcols;
  uint16_t* uop;  // [B][dk]
  float* thr2;
  double* tau;
  double* ev;  // [B][cap] exact candidates
  int64_t* ei;
  char* fws;
  int64_t* ti;  // [B][kk]
  double* tv;
  int64_t S;
  size_t total;
};

static CosPruneWs cos_prune_layout(char* base, int B, int64_t n, int kk, int dk) {
  CosPruneWs w{};
  Carver c(base);
  const int64_t smax = kk <= 64 ? kCosSample : kCosSampleK;
  w.S = n < smax ? n : smax;
  w.c = cascade_carve(c, B, w.S, kCosCap, kk, 0);
  w.qrow = (int64_t*)c.take((size_t)B * 8);
  w.xrows = (int64_t*)c.take((size_t)B * 8);
  w.xptr = (int64_t*)c.take((size_t)(B + 1) * 8);
  w.xcols = (int32_t*)c.take((size_t)B * 4);
  w.uop = (uint16_t*)c.take((size_t)B * dk * 2);
  w.thr2 = (float*)c.take((size_t)B * 4);
  w.tau = (double*)c.take((size_t)B * 8);
  w.ev = (double*)c.take((size_t)B * kCosCap * 8);
  w.ei = (int64_t*)c.take((size_t)B * kCosCap * 8);
  w.fws = c.take(topk_ws_bytes(B, kCosCap, kk, 8));
  w.ti = (int64_t*)c.take((size_t)B * kk * 8);
  w.tv = (double*)c.take((size_t)B * kk * 8);
  w.total = c.total() + 256;
  return w;
}

static int cos_kk(int64_t n, int top_k, int skip_self) {
  const int64_t m = n - (skip_self ? 1 : 0);
  return (int)(top_k < m ? top_k : m);
}

// Whether the call takes the pruned arm. Auto: from kCosAutoCut rows on, with
// an operand, and only while the sample bound can be expected to leave a list
// below half its capacity: about kk n / S rows beat the kk-th best of S sample
// rows (top_k 1024 at 100k rows: 3125 and the margin's band, past the
// capacity every time: both arms would run).
static bool cos_pruned(int mode, int64_t n, int kk, const void* items) {
  if (mode != 0) return mode == 2;
  if (items == nullptr || n < kCosAutoCut) return false;
  const int64_t smax = kk <= 64 ? kCosSample : kCosSampleK;
  const int64_t S = n < smax ? n : smax;
  return (int64_t)kk * n <= S * (kCosCap / 2);
}

}  // namespace hrec

using namespace hrec;

extern "C" size_t hrec_cosine_items_bytes(int64_t n, int d) {
  const int64_t m = n > 0 ? n : 0;
  const int dd = d < 1 ? 1 : (d > kCosMaxD ? kCosMaxD : d);
  return al256((size_t)m * cos_dk(dd) * 2) + 256;
}

extern "C" int hrec_cosine_items(const float* vectors, int64_t n, int d, int64_t ld, const double* inv_norm,
                                 void* out, void* stream) {
  HREC_REQUIRE(d >= 1 && d <= kCosMaxD, "cosine_items: d must be in [1, %d] (got %d)", kCosMaxD, d);
  HREC_REQUIRE(ld >= d, "cosine_items: ld must be >= d");
  HREC_REQUIRE(n >= 0 && n <= INT32_MAX, "cosine_items: n must be in [0, 2^31)");
  if (n == 0) return HREC_OK;
  HREC_REQUIRE(vectors && inv_norm && out, "cosine_items: null pointer");
  HREC_REQUIRE(((uintptr_t)out & 255) == 0, "cosine_items: output must be 256-B aligned");
  hipLaunchKernelGGL(cos_items_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), vectors, n,
                     d, ld, inv_norm, cos_dk(d), static_cast<uint16_t*>(out));
  return check_launch("cos_items_kernel");
}

extern "C" size_t hrec_cosine_topk_workspace_bytes(int n_q, int64_t n, int top_k, int d, int mode) {
  const int B = n_q > 0 ? n_q : 0;
  const int64_t N = n > 0 ? n : 1;
  const int tk = top_k < 1 ? 1 : (top_k > kCosTopMax ? kCosTopMax : top_k);
  const int kk = cos_kk(N, tk, 0);  // skip_self only shortens the lists
  const int dd = d < 1 ? 1 : (d > kCosMaxD ? kCosMaxD : d);
  const size_t exh = cos_exh_layout(nullptr, B, N, kk, dd).total;
  if (mode == 1 || (mode == 0 && N < kCosAutoCut)) return exh;
  const size_t pr = cos_prune_layout(nullptr, B, N, kk, cos_dk(dd)).total;
  return mode == 2 ? pr : (pr > exh ? pr : exh);
}

// Diagnostics of the last mode-2 call on this workspace (same n_q, n, top_k, d): out int32 [n_q] = the rows the
// matrix-core filter kept per query (above kCosCap: that list overflowed).
extern "C" int hrec_cosine_topk_counts(const void* workspace, int n_q, int64_t n, int top_k, int d, int32_t* out,
                                       void* stream) {
  HREC_REQUIRE(d >= 1 && d <= kCosMaxD && n >= 1 && n <= INT32_MAX && n_q >= 0 && n_q < 65536 && top_k >= 1 &&
                   top_k <= kCosTopMax,
               "cosine_topk_counts: bad shape");
  if (n_q == 0) return HREC_OK;
  HREC_REQUIRE(workspace && out, "cosine_topk_counts: null pointer");
  const CosPruneWs w = cos_prune_layout((char*)workspace, n_q, n, cos_kk(n, top_k, 0), cos_dk(d));
  if (hipMemcpyAsync(out, w.c.cn, (size_t)n_q * 4, hipMemcpyDeviceToDevice, as_stream(stream)) != hipSuccess)
    return check_launch("cosine_topk_counts: copy");
  return HREC_OK;
}

extern "C" int hrec_cosine_topk(const float* vectors, int64_t n, int d, int64_t ld, const double* inv_norm,
                                const int64_t* query_rows, int n_q, int top_k, int skip_self, double min_sim,
                                int mode, const void* items, int64_t* out_idx, double* out_val, int32_t* out_len,
                                int* overflow, void* workspace, size_t workspace_bytes, void* stream) {
  HREC_REQUIRE(d >= 1 && d <= kCosMaxD, "cosine_topk: d must be in [1, %d] (got %d)", kCosMaxD, d);
  HREC_REQUIRE(ld >= d, "cosine_topk: ld must be >= d");
  HREC_REQUIRE(n >= 1 && n <= INT32_MAX, "cosine_topk: n must be in [1, 2^31)");
  HREC_REQUIRE(n_q >= 0 && n_q < 65536, "cosine_topk: n_q must be in [0, 65536)");
  HREC_REQUIRE(top_k >= 1 && top_k <= kCosTopMax, "cosine_topk: top_k must be in [1, %d] (got %d)", kCosTopMax, top_k);
  HREC_REQUIRE(skip_self == 0 || skip_self == 1, "cosine_topk: skip_self must be 0 or 1");
  HREC_REQUIRE(min_sim == min_sim, "cosine_topk: min_sim must not be NaN");
  HREC_REQUIRE(mode >= 0 && mode <= 2, "cosine_topk: mode must be 0, 1 or 2");
  if (n_q == 0) return HREC_OK;
  HREC_REQUIRE(vectors && inv_norm && query_rows && out_idx && out_val && out_len && overflow && workspace &&
                   (items || mode != 2),
               "cosine_topk: null pointer");
  HREC_REQUIRE(((uintptr_t)items & 255) == 0, "cosine_topk: items must be 256-B aligned");
  const size_t need = hrec_cosine_topk_workspace_bytes(n_q, n, top_k, d, mode);
  HREC_REQUIRE(workspace_bytes >= need, "cosine_topk: workspace %zu < %zu", workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const int kk = cos_kk(n, top_k, skip_self);
  const dim3 wave_grid((unsigned)((n_q + 3) / 4)), block(256);
  int rc;
  if (!cos_pruned(mode, n, kk, items) || kk == 0) {
    const CosExhWs w = cos_exh_layout((char*)workspace, n_q, n, cos_kk(n, top_k, 0), d);
    hipLaunchKernelGGL(cos_prep_kernel, wave_grid, block, 0, s, query_rows, n_q, n, skip_self, nullptr, 0, w.qrow,
                       nullptr, nullptr, nullptr, nullptr, overflow);
    rc = check_launch("cos_prep_kernel");
    if (rc) return rc;
    for (int b0 = 0; b0 < n_q; b0 += w.qb) {
      const int nb = n_q - b0 < w.qb ? n_q - b0 : w.qb;
      if (kk > 0) {
        const unsigned groups = (unsigned)((nb + kCosQ - 1) / kCosQ);
        hipLaunchKernelGGL(cos_stage_kernel, dim3(groups), block, 0, s, vectors, d, ld, w.qrow + b0, nb, w.qf);
        rc = check_launch("cos_stage_kernel");
        if (rc) return rc;
        const dim3 grid((unsigned)((n + 255) / 256), groups);
        hipLaunchKernelGGL(cos_sims_kernel, grid, block, 0, s, vectors, n, d, ld, inv_norm, w.qrow + b0, w.qf, nb,
                           skip_self, w.sims);
        rc = check_launch("cos_sims_kernel");
        if (rc) return rc;
        rc = topk_rows<double>(w.sims, nb, n, n, kk, w.ti, w.tv, w.tws, (size_t)1 << 62, s);
        if (rc) return rc;
      }
      hipLaunchKernelGGL(cos_finish_kernel, dim3((unsigned)((nb + 3) / 4)), block, 0, s, nb, w.qrow + b0, kk, top_k,
                         min_sim, (const double*)nullptr, skip_self, w.ti, w.tv, out_idx + (int64_t)b0 * top_k,
                         out_val + (int64_t)b0 * top_k, out_len + b0);
      rc = check_launch("cos_finish_kernel");
      if (rc) return rc;
    }
    return HREC_OK;
  }
  const int dk = cos_dk(d);
  const CosPruneWs w = cos_prune_layout((char*)workspace, n_q, n, cos_kk(n, top_k, 0), dk);
  const uint16_t* it = static_cast<const uint16_t*>(items);
  // 0) the checked rows, the bf16 query operands, the one-column exclusion, *overflow = 0
  hipLaunchKernelGGL(cos_prep_kernel, wave_grid, block, 0, s, query_rows, n_q, n, skip_self, it, dk, w.qrow, w.uop,
                     w.xrows, w.xptr, w.xcols, overflow);
  rc = check_launch("cos_prep_kernel");
  if (rc) return rc;
  // 1) s~ over the first S rows; the kk-th best of those that stay; zeroes the filter's counters
  rc = dot_scores_run(w.uop, n_q, it, w.S, dk, 1, w.c.samp, w.S, s, kCosSampleUB);
  if (rc) return rc;
  const Excl x = skip_self ? Excl{true, w.xrows, w.xptr, w.xcols, nullptr} : Excl{};
  const float* thr;
  int thr_stride;
  rc = cascade_bound(w.c, n_q, w.S, 1, w.S, kk, x, nullptr, true, w.c.cn, &thr, &thr_stride, s);
  if (rc) return rc;
  hipLaunchKernelGGL(cos_thr_kernel, dim3((unsigned)((n_q + 255) / 256)), block, 0, s, n_q, w.qrow, inv_norm, thr,
                     thr_stride,
                     w.tau, w.thr2);
  rc = check_launch("cos_thr_kernel");
  if (rc) return rc;
  // 2) the matrix-core filter over every row at down(tau_b - E)
  rc = dot_filter_run(w.uop, n_q, it, n, dk, 1, w.thr2, 1, 0, kCosCap, w.c.cv, w.c.ci, w.c.cn, s);
  if (rc) return rc;
  // 3) the exact chain over the kept rows
  hipLaunchKernelGGL(cos_rescore_kernel, dim3((unsigned)n_q), block, 0, s, vectors, n, d, ld, inv_norm, w.qrow,
                     skip_self, w.c.ci, w.c.cn, kCosCap, w.tau, kk, w.ev, w.ei, overflow);
  rc = check_launch("cos_rescore_kernel");
  if (rc) return rc;
  // 4) the f64 stable top-k of the candidates (ties: column), then the min_sim cut
  rc = topk_rows<double>(w.ev, n_q, kCosCap, kCosCap, kk, w.ti, w.tv, w.fws, (size_t)1 << 62, s, w.ei, w.c.cn);
  if (rc) return rc;
  hipLaunchKernelGGL(cos_finish_kernel, wave_grid, block, 0, s, n_q, w.qrow, kk, top_k, min_sim, inv_norm, skip_self, w.ti,
                     w.tv, out_idx,
                     out_val, out_len);
  return check_launch("cos_finish_kernel");
}
