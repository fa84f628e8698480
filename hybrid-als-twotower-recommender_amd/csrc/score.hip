// K2: ALS scoring (Spark ALSModel.transform, JVM-exact f32 chain) and its
// fused top-k. K2p, the pruned ALS top-k, is csrc/als_prune.hip, the cascade
// steps both share csrc/cascade.hip, the generic stable top-k csrc/topk.hip,
// the hybrid fusion (K9) csrc/fuse.hip.
#include "cascade.h"
#include "score.h"
#include "wave.h"  // lanes_below

namespace hrec {

#ifndef HREC_SCORE_PAIR_STORE
#define HREC_SCORE_PAIR_STORE 1  // full-row JVM-exact scores: 8-B stores of item pairs
#endif

// --------------------------------------------------------------- ALS score
// One thread per item; UB users per block row held in LDS (broadcast reads).
// The item matrix is stored transposed [kp][ld] so every c-step is one
// coalesced 1-KiB read per wave. Sequential c order, product rounded, sum
// rounded: Spark's `dotProduct += featuresA(i) * featuresB(i)` on floats.
template <int UB>
__global__ __launch_bounds__(256) void als_score_kernel(const float* __restrict__ U,
                                                        const int64_t* __restrict__ user_rows, int n_users,
                                                        const float* __restrict__ Vt, int64_t ld,
                                                        const int64_t* __restrict__ item_rows,
                                                        int64_t n_items, int k, int kp,
                                                        float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float ush[UB][kScoreKMax];
  __shared__ int uok[UB];
  const int b0 = blockIdx.y * UB;
  for (int t = threadIdx.x; t < UB * kp; t += blockDim.x) {
    const int b = t / kp, c = t % kp;
    const int64_t ur = (b0 + b < n_users) ? user_rows[b0 + b] : -1;
    ush[b][c] = ur >= 0 ? U[ur * kp + c] : 0.f;
    if (c == 0) uok[b] = ur >= 0;
  }
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_items) return;
  const int64_t ir = item_rows ? item_rows[j] : j;
  float acc[UB];
#pragma unroll
  for (int b = 0; b < UB; ++b) acc[b] = 0.f;
  if (ir >= 0) {
    const float* __restrict__ v = Vt + ir;
    for (int c = 0; c < k; ++c) {
      const float vc = v[(int64_t)c * ld];
#pragma unroll
      for (int b = 0; b < UB; ++b) {
        const float prod = ush[b][c] * vc;
        acc[b] = acc[b] + prod;
      }
    }
  }
  const float qnan = __builtin_nanf("");
#pragma unroll
  for (int b = 0; b < UB; ++b) {
    if (b0 + b < n_users) out[(int64_t)(b0 + b) * n_items + j] = (ir >= 0 && uok[b]) ? acc[b] : qnan;
  }
}

// Fast path of K2 for whole item ranges (no item_rows gather): 4 items per
// thread (two float2 loads of the transposed item matrix per rank step),
// UB users per block kept TRANSPOSED in LDS (one ds_read_b128 feeds 4 users),
// packed f32 multiply + add (v_pk_mul_f32 / v_pk_add_f32; contraction off so
// every product and sum is rounded exactly like the JVM loop).
// FILTER: instead of writing the scores, append (score, item) pairs with
// score >= thr[b] to a per-user candidate list (wave-aggregated atomics).
typedef hrec_f2 f2v;
typedef hrec_rsrc_t i4v;

template <int UB, bool FILTER>
__global__ __launch_bounds__(256) void als_score_fast_kernel(
    const float* __restrict__ U, const int64_t* __restrict__ user_rows, int n_users,
    const float* __restrict__ Vt, int64_t ld, int64_t n_items, int k, int kp, float* __restrict__ out,
    const float* __restrict__ thr, int thr_stride, int cap, float* __restrict__ cand_v,
    int64_t* __restrict__ cand_i, int* __restrict__ cand_n, int* __restrict__ overflow) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float us[kScoreKMax + 1][UB];  // + the row read ahead past the end
  __shared__ int uok[UB];
  // grid: x = user group (fastest-varying), y = 1024-item slice, so the
  // blocks of one item slice are dispatched back to back and share it in L2
  const int b0 = blockIdx.x * UB;
  const int64_t j0 = (int64_t)blockIdx.y * 1024 + 2 * threadIdx.x;
  const int64_t j1 = j0 + 512;
  // Rank-step c reads row c of Vt through a raw buffer resource spanning
  // [0, ld) of that row (rows c >= k span nothing): columns past the row end
  // read as zero without a branch, and rank steps c + 1 ... c + P - 1 are
  // already in flight while step c computes. ld is even, so both items of a
  // pair are in range together; items in [n_items, ld) are dropped below.
  constexpr int P = 4;
  const uint64_t vbase = (uint64_t)Vt;
  const int rec = (int)(ld * 4);
  auto rsrc_of = [&](int c) {
    const uint64_t a = vbase + (uint64_t)c * (uint64_t)ld * 4u;
    i4v r;
    r.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    r.y = __builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    r.z = __builtin_amdgcn_readfirstlane(c < k ? rec : 0);
    r.w = 0x00020000;
    return r;
  };
  const int o0 = (int)(j0 * 4), o1 = (int)(j1 * 4);
  f2v r0[P], r1[P];
#pragma unroll
  for (int q = 0; q < P; ++q) {  // issued before the user staging: independent of it
    const i4v rs = rsrc_of(q);
    r0[q] = rbuf_load_f2(rs, o0, 0, 0);
    r1[q] = rbuf_load_f2(rs, o1, 0, 0);
  }
  for (int t = threadIdx.x; t < UB * kp; t += blockDim.x) {
    const int b = t / kp, c = t % kp;
    const int64_t ur = (b0 + b < n_users) ? user_rows[b0 + b] : -1;
    us[c][b] = (ur >= 0 && c < k) ? U[ur * kp + c] : 0.f;
    if (c == 0) uok[b] = ur >= 0;
  }
  float tb[UB];  // survivor thresholds, read ahead of the loop
#pragma unroll
  for (int b = 0; b < UB; ++b) tb[b] = (FILTER && b0 + b < n_users) ? thr[(int64_t)(b0 + b) * thr_stride] : 0.f;
  __syncthreads();
  f2v acc0[UB], acc1[UB];
#pragma unroll
  for (int b = 0; b < UB; ++b) {
    acc0[b] = f2v{0.f, 0.f};
    acc1[b] = f2v{0.f, 0.f};
  }
  // user values for rank step c + 1 are read from LDS while step c computes
  // (two register sets, alternating with the parity of the unrolled step)
  float4 ub[2][UB / 4];
#pragma unroll
  for (int b = 0; b < UB; b += 4) ub[0][b / 4] = *reinterpret_cast<const float4*>(&us[0][b]);
  for (int c0 = 0; c0 < k; c0 += P) {
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int c = c0 + q;  // may pass k by < P: zero factors there (us staged 0)
#pragma unroll
      for (int b = 0; b < UB; b += 4) ub[(q + 1) & 1][b / 4] = *reinterpret_cast<const float4*>(&us[c + 1][b]);
      {
        const f2v v0 = r0[q], v1 = r1[q];
#pragma unroll
        for (int b = 0; b < UB; b += 4) {
          const float4 u4 = ub[q & 1][b / 4];
          const float uu[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f2v us2 = f2v{uu[e], uu[e]};
            const f2v p0 = us2 * v0;
            const f2v p1 = us2 * v1;
            acc0[b + e] = acc0[b + e] + p0;
            acc1[b + e] = acc1[b + e] + p1;
          }
        }
        // refill the slot only once its values are dead, so the load lands in
        // the slot's own registers (no copy waiting on it at the back edge)
        const i4v rs = rsrc_of(c + P);
        r0[q] = rbuf_load_f2(rs, o0, 0, 0);
        r1[q] = rbuf_load_f2(rs, o1, 0, 0);
      }
    }
  }
  if (!FILTER) {
    const float qnan = __builtin_nanf("");
    // pairs (j, j + 1) as one 8-B store when rows are 8-B aligned: a wave
    // then writes 512 contiguous bytes per instruction
    const bool pair = HREC_SCORE_PAIR_STORE && (n_items % 2 == 0) && ((reinterpret_cast<uintptr_t>(out) & 7) == 0);
#pragma unroll
    for (int b = 0; b < UB; ++b) {
      if (b0 + b >= n_users) break;
      float* o = out + (int64_t)(b0 + b) * n_items;
      const bool ok = uok[b];
      if (pair) {
        if (j0 + 1 < n_items) *reinterpret_cast<float2*>(o + j0) = ok ? make_float2(acc0[b].x, acc0[b].y)
                                                                        : make_float2(qnan, qnan);
        if (j1 + 1 < n_items) *reinterpret_cast<float2*>(o + j1) = ok ? make_float2(acc1[b].x, acc1[b].y)
                                                                        : make_float2(qnan, qnan);
        continue;
      }
      if (j0 < n_items) o[j0] = ok ? acc0[b].x : qnan;
      if (j0 + 1 < n_items) o[j0 + 1] = ok ? acc0[b].y : qnan;
      if (j1 < n_items) o[j1] = ok ? acc1[b].x : qnan;
      if (j1 + 1 < n_items) o[j1 + 1] = ok ? acc1[b].y : qnan;
    }
  } else {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int b = 0; b < UB; ++b) {
      if (b0 + b >= n_users || !uok[b]) continue;  // block-uniform
      const float t = tb[b];
      const float sv[4] = {acc0[b].x, acc0[b].y, acc1[b].x, acc1[b].y};
      const int64_t sj[4] = {j0, j0 + 1, j1, j1 + 1};
      // one compare per user in the common case: nothing of this wave passes
      // (NaN scores fail >= like the per-item test; columns >= n_items may
      // pass here and are dropped by the exact test below)
      const float mx = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
      if (__ballot(mx >= t) == 0) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool pass = sj[e] < n_items && sv[e] >= t;
        const uint64_t m = __ballot(pass);
        if (m == 0) continue;
        int base = 0;
        const int leader = __builtin_ctzll(m);
        if (lane == leader) {
          base = atomicAdd(&cand_n[b0 + b], __popcll(m));
          if (base + __popcll(m) > cap) *overflow = 1;  // this user's survivors exceed the list
        }
        base = __shfl(base, leader, kWave);
        if (pass) {
          const int pos = base + lanes_below(m);
          if (pos < cap) {
            cand_v[(int64_t)(b0 + b) * cap + pos] = sv[e];
            cand_i[(int64_t)(b0 + b) * cap + pos] = sj[e];
          }
        }
      }
    }
  }
}

}  // namespace hrec

using namespace hrec;

extern "C" int hrec_als_score(const float* user_factors, const int64_t* user_rows, int n_users,
                              const float* item_factors_t, int64_t ld_items, const int64_t* item_rows,
                              int64_t n_items, int k, int kp, float* out, void* stream) {
  HREC_REQUIRE(hrec_factor_ld_ok(kp), "als_score: kp must be 16, 32, 64, 96, 128, 192 or 256");
  HREC_REQUIRE(k >= 1 && k <= kp, "als_score: need 1 <= k <= kp");
  HREC_REQUIRE(n_users >= 0 && n_items >= 0 && ld_items >= 0, "als_score: negative size");
  if (n_users == 0 || n_items == 0) return HREC_OK;
  HREC_REQUIRE(user_factors && user_rows && item_factors_t && out, "als_score: null pointer");
  HREC_REQUIRE(item_rows != nullptr || n_items <= ld_items, "als_score: n_items > ld_items");
  constexpr int UB = 16;
  if (item_rows == nullptr && ld_items % 2 == 0 && ld_items < ((int64_t)1 << 29) &&
      (reinterpret_cast<uintptr_t>(item_factors_t) & 7) == 0) {
    // every item in order: the packed-f32 kernel (same JVM-exact chain)
    const dim3 grid((unsigned)((n_users + UB - 1) / UB), (unsigned)((n_items + 1023) / 1024));
    hipLaunchKernelGGL((als_score_fast_kernel<UB, false>), grid, dim3(256), 0, as_stream(stream), user_factors,
                       user_rows, n_users, item_factors_t, ld_items, n_items, k, kp, out, nullptr, 0, 0, nullptr,
                       nullptr, nullptr, nullptr);
    return check_launch("als_score_fast_kernel");
  }
  const dim3 grid((unsigned)((n_items + 255) / 256), (unsigned)((n_users + UB - 1) / UB));
  hipLaunchKernelGGL((als_score_kernel<UB>), grid, dim3(256), 0, as_stream(stream), user_factors, user_rows,
                     n_users, item_factors_t, ld_items, item_rows, n_items, k, kp, out);
  return check_launch("als_score_kernel");
}

#ifndef HREC_SCORE_UB
#define HREC_SCORE_UB 16
#endif
static constexpr int kScoreUB = HREC_SCORE_UB;
static constexpr int kSampleUB = 4;

// Workspace of the fused path: the cascade's buffers over min(N, kSample) sample items and
// kCap candidates, the counters padded by 16 B, and a 256-B tail.
extern "C" size_t hrec_als_score_topk_workspace_bytes(int n_users, int64_t n_items, int top_k) {
  const int64_t N = n_items > 0 ? n_items : 0;
  Carver c(nullptr);
  cascade_carve(c, n_users > 0 ? n_users : 0, N < kSample ? N : kSample, kCap, score_kk(n_items, top_k), 16);
  return c.total() + 256;
}

// hrec_als_score_topk and hrec_als_score_topk_excluding (x.on; x.rows are the
// call's user_rows): the same launches, the exclusion's two kernels inside the
// cascade's steps (csrc/cascade.hip: why the bound stays sound under one).
int hrec::score_topk_run(const char* fn, const float* user_factors, const int64_t* user_rows, int n_users,
                         const float* item_factors_t, int64_t ld_items, int64_t n_items, int k, int kp, int top_k,
                         int64_t* out_idx, float* out_val, int* overflow, void* workspace, size_t workspace_bytes,
                         const Excl& x, void* stream) {
  HREC_REQUIRE(hrec_factor_ld_ok(kp), "%s: kp must be 16, 32, 64, 96, 128, 192 or 256", fn);
  HREC_REQUIRE(k >= 1 && k <= kp, "%s: need 1 <= k <= kp", fn);
  HREC_REQUIRE(n_users >= 0 && n_users < 65536 && n_items >= 0, "%s: bad shape", fn);
  HREC_REQUIRE(ld_items >= n_items && ld_items % 4 == 0 && ld_items < ((int64_t)1 << 29),
               "%s: ld_items must be >= n_items, %% 4 and < 2^29", fn);
  HREC_REQUIRE(top_k >= 1 && top_k <= 1024, "%s: top_k must be in [1, 1024]", fn);
  if (n_users == 0 || n_items == 0) return HREC_OK;
  HREC_REQUIRE(user_factors && user_rows && item_factors_t && out_idx && out_val && overflow && workspace,
               "%s: null pointer", fn);
  HREC_REQUIRE(!x.on || (x.indptr && x.cols && x.out_len), "%s: null exclusion or out_len", fn);
  const size_t need = hrec_als_score_topk_workspace_bytes(n_users, n_items, top_k);
  HREC_REQUIRE(workspace_bytes >= need, "%s: workspace %zu < %zu", fn, workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const int kk = (int)(top_k < n_items ? top_k : n_items);
  const int64_t S = n_items < kSample ? n_items : kSample;
  Carver carver(workspace);
  const CascadeWs w = cascade_carve(carver, n_users, S, kCap, kk, 16);  // as the size query carves it
  const dim3 blk(256);
  const unsigned gy = (unsigned)((n_users + kScoreUB - 1) / kScoreUB);
  if (hipMemsetAsync(overflow, 0, sizeof(int), s) != hipSuccess) return check_launch("score_topk memset");
  if (n_items <= kSample) {  // small: score everything, exact top-k
    hipLaunchKernelGGL((als_score_fast_kernel<kScoreUB, false>), dim3(gy, (unsigned)((n_items + 1023) / 1024)), blk,
                       0, s, user_factors, user_rows, n_users, item_factors_t, ld_items, n_items, k, kp, w.samp,
                       nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr);
    const int rc = check_launch("als_score_fast_kernel");
    return rc ? rc : cascade_rank_all(w, n_users, n_items, kk, x, out_idx, out_val, s);
  }
  // 1) thresholds: the kk-th best of the first S items bounds the final kk-th from below
  //    (4 users per block: the sample is too small to fill the chip with 16)
  hipLaunchKernelGGL((als_score_fast_kernel<kSampleUB, false>),
                     dim3((unsigned)((n_users + kSampleUB - 1) / kSampleUB), (unsigned)((S + 1023) / 1024)), blk, 0,
                     s, user_factors, user_rows, n_users, item_factors_t, ld_items, S, k, kp, w.samp, nullptr, 0, 0,
                     nullptr, nullptr, nullptr, nullptr);
  int rc = check_launch("als_score_fast_kernel(sample)");
  if (rc) return rc;
  //    no lengths here; kk <= 64: the lane maxima, which also zero the survivor counters
  const float* thr;
  int thr_stride;
  rc = cascade_bound(w, n_users, S, 1, S, kk, x, nullptr, true, w.cn, &thr, &thr_stride, s);
  if (rc) return rc;
  // 2) fused score + filter over all items; a user whose survivors exceed
  //    kCap raises *overflow from inside the filter (the caller falls back)
  hipLaunchKernelGGL((als_score_fast_kernel<kScoreUB, true>), dim3(gy, (unsigned)((n_items + 1023) / 1024)), blk, 0,
                     s, user_factors, user_rows, n_users, item_factors_t, ld_items, n_items, k, kp, nullptr,
                     thr, thr_stride, kCap, w.cv, w.ci, w.cn, overflow);
  rc = check_launch("als_score_fast_kernel(filter)");
  if (rc) return rc;
  // 3) the excluded survivors leave (writing out_len); exact stable top-k over the rest
  return cascade_tail(w, n_users, kCap, kk, x, x.out_len, out_idx, out_val, s);
}

extern "C" int hrec_als_score_topk(const float* user_factors, const int64_t* user_rows, int n_users,
                                   const float* item_factors_t, int64_t ld_items, int64_t n_items, int k, int kp,
                                   int top_k, int64_t* out_idx, float* out_val, int* overflow, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return score_topk_run("als_score_topk", user_factors, user_rows, n_users, item_factors_t, ld_items, n_items, k, kp,
                        top_k, out_idx, out_val, overflow, workspace, workspace_bytes, Excl{}, stream);
}

// The exclusion lives in the caller's buffers: the workspace is the fused path's.
extern "C" size_t hrec_als_score_topk_excluding_workspace_bytes(int n_users, int64_t n_items, int top_k) {
  return hrec_als_score_topk_workspace_bytes(n_users, n_items, top_k);
}

extern "C" int hrec_als_score_topk_excluding(const float* user_factors, const int64_t* user_rows, int n_users,
                                             const float* item_factors_t, int64_t ld_items, int64_t n_items, int k,
                                             int kp, int top_k, const int64_t* excl_indptr, const int32_t* excl_cols,
                                             int64_t* out_idx, float* out_val, int32_t* out_len, int* overflow,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  return score_topk_run("als_score_topk_excluding", user_factors, user_rows, n_users, item_factors_t, ld_items,
                        n_items, k, kp, top_k, out_idx, out_val, overflow, workspace, workspace_bytes,
                        Excl{true, user_rows, excl_indptr, excl_cols, out_len}, stream);
}

