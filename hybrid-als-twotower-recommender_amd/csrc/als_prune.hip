#include <float.h>

#include "cascade.h"
#include "exclusion.h"
#include "order.h"  // bf16_rne, f32_up / f32_down
#include "score.h"
#include "wave.h"  // lanes_below, wave_xor_max

using namespace hrec;

// ---------------------------------------------------- K2p: pruned ALS top-k
// (the fused path, K2, is csrc/score.hip; the steps both share csrc/cascade.hip)
// hrec_als_score_topk's result (the stable top-k of the JVM-exact scores)
// without the exact chain over every pair: the scores are first bounded on
// the bf16 matrix cores, and the exact chain runs only for the pairs the
// bound cannot rule out.
//   bf16 operands (8 significant bits, round to nearest even: |x - bf16(x)|
//   <= 2^-8 |x|; e.g. 1 + 2^-8 + 2^-20 -> 1 + 2^-7) give products within
//   (2^-7 + 2^-16) |u_c v_c| of the exact ones, so s~ = sum uh_c vh_c has
//   |s~ - u.v| <= (2^-7 + 2^-16 + k 2^-24 (1 + 2^-6)) sum |u_c v_c| (the f32
//   accumulation of k exact bf16 products, any order), and the JVM chain is
//   within 2k 2^-24 sum |u_c v_c| of u.v; for k <= 256 both fit in
//   E_b = (2^-7 + 2^-13) ||u_b|| max_j ||v_j|| (2^-16 + 3 * 256 * 2^-24 <
//   2^-13; + 1e-30 for products the matrix cores may flush).
//   1. tau_b: the kk-th best s~ over the first 8192 items (bf16 dot on the
//      matrix cores, the fused path's lane-maxima bound) minus E_b, rounded
//      down: kk items have chain >= s~ - E_b >= tau_b, so the kk-th best
//      chain over all items is >= tau_b;
//   2. the bf16 filter (als_bound_filter_kernel) at tau_b - E_b keeps
//      every item whose chain can reach tau_b;
//   3. the JVM chain over the kept items; those >= tau_b are the candidates,
//      a superset of the top kk, ranked by the same stable top-k as the
//      fused path (ties -> smaller item).
// Under an exclusion (hrec_als_score_topk_pruned_excluding) step 1 takes the
// bound over the sample's non-excluded items, steps 2 and 3 are unchanged, and
// the excluded candidates leave before the ranking (score_topk_pruned_run).
// Users whose bound is not finite (a non-finite factor anywhere) or whose
// kept list overflows raise *overflow: the caller's fallback (the
// materialised scores + hrec_topk_f32) answers the call, as for the fused
// path's list overflow. Unknown users (row < 0) keep no candidates, as there.
constexpr double kPruneRel = 0x1p-7 + 0x1p-13;
constexpr double kPruneAbs = 1e-30;
// items of the bf16 sample bound: kk <= 64 takes the first 32768 items'
// wave-tile maxima (no score matrix; 8192 / 16384 / 32768 items -> 105 /
// 96 / 94 us per 1024 x 100k call: a larger sample leaves fewer pairs to the
// filter), kk > 64 the exact kk-th of the first 8192 items' scores (a
// materialised [B][8192] sample: 4096 / 8192 / 16384 / 32768 items measured
// 160 / 144 / 145 / 153 us before the maxima form)
constexpr int kPruneSampleMax = 32768;
constexpr int kPruneSample = 8192;
// resident users per block of the sample's dot (the full 128 KiB of users
// leaves 16 blocks for 8192 items: 64 -> 144 us, 128 -> 148, 256 -> 154;
// the filter over all items keeps the kernel's own tile, capping it measured
// no faster)
constexpr int kPruneSampleUB = 64;

// Item operand: bf16 rows [N][dk] (zero beyond k) and the largest row norm
// rounded up (+inf for a non-finite value), one thread per row.
__global__ __launch_bounds__(256) void als_items_bf16_kernel(const float* __restrict__ V, int64_t ldv, int64_t N,
                                                             int k, int dk, uint16_t* __restrict__ out,
                                                             unsigned* __restrict__ max_norm) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double ss = 0.0;
  bool bad = false;
  if (row < N) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + row * dk);
    for (int c = 0; c < dk; c += 2) {
      const float v0 = c < k ? V[row * ldv + c] : 0.f;
      const float v1 = c + 1 < k ? V[row * ldv + c + 1] : 0.f;
      ss += (double)v0 * v0 + (double)v1 * v1;
      bad = bad || !isfinite(v0) || !isfinite(v1);
      o[c >> 1] = bf16_rne(v0) | (bf16_rne(v1) << 16);
    }
  }
  const double nrm = sqrt(ss) * (1.0 + 1e-6);
  unsigned f = __float_as_uint((bad || !(nrm < 0x1p60)) ? INFINITY : f32_up(nrm));
  f = wave_xor_max(f);  // non-negative floats order as their bits
  if ((threadIdx.x & 63) == 0) atomicMax(max_norm, f);
}

// Per user (one wave): the bf16 user operand and E_b (+inf: no usable bound,
// NaN: unknown user).
__global__ __launch_bounds__(256) void als_prune_user_kernel(const float* __restrict__ U, int kp,
                                                             const int64_t* __restrict__ user_rows, int n_users,
                                                             int k, int dk, const float* __restrict__ max_norm,
                                                             uint16_t* __restrict__ uop, double* __restrict__ err,
                                                             int* __restrict__ overflow) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;  // the call's first kernel (no memset launch)
  if (b >= n_users) return;  // wave-uniform
  const int64_t r = user_rows[b];
  double ss = 0.0;
  bool bad = false;
  for (int c = lane; c < dk; c += 64) {
    const float v = (r >= 0 && c < k) ? U[r * kp + c] : 0.f;
    ss += (double)v * v;
    bad = bad || !isfinite(v);
    uop[(int64_t)b * dk + c] = (uint16_t)bf16_rne(v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ss += __shfl_xor(ss, off, kWave);
    bad = bad || __shfl_xor((int)bad, off, kWave);
  }
  if (lane == 0) {
    const double e = kPruneRel * (sqrt(ss) * (1.0 + 1e-6)) * (double)max_norm[0] + kPruneAbs;
    err[b] = r < 0 ? __builtin_nan("") : ((bad || !(e < 0x1p100)) ? INFINITY : e);
  }
}

// Per user: tau_b = down(t_b - E_b) for the exact test, down(tau_b - E_b)
// for the bf16 filter; the candidate counter zeroed.
__device__ __forceinline__ void pr_bounds(int b, double t, const double* __restrict__ err, float* __restrict__ tau,
                                          float* __restrict__ thr2, int* __restrict__ cn,
                                          int* __restrict__ overflow) {
  cn[b] = 0;
  const double e = err[b];
  float t1 = INFINITY, t2 = INFINITY;  // unknown user / no bound: nothing passes
  if (e == e) {
    const double lo1 = t - e;
    const double lo2 = (double)f32_down(lo1) - e;
    if (isfinite(t) && isfinite(e) && isfinite(lo2)) {
      t1 = f32_down(lo1);
      t2 = f32_down(lo2);
      if (!isfinite(t2)) t2 = -FLT_MAX;  // below every finite f32 score
      if (!isfinite(t1)) t1 = -FLT_MAX;
    } else {
      atomicOr(overflow, 1);  // no usable bound: the caller's exact fallback
    }
  }
  tau[b] = t1;
  thr2[b] = t2;
}

__global__ __launch_bounds__(256) void als_prune_thr_kernel(int n_users, const float* __restrict__ thr,
                                                            int thr_stride, const double* __restrict__ err,
                                                            float* __restrict__ tau, float* __restrict__ thr2,
                                                            int* __restrict__ cn, int* __restrict__ overflow) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_users) return;
  pr_bounds(b, thr[(int64_t)b * thr_stride], err, tau, thr2, cn, overflow);
}

// kk <= 64: sample_threshold_kernel's lane-maxima bound over the wave-tile
// maxima and the bounds above in one launch (one wave per user; zeroes the
// filter's counter too).
__global__ __launch_bounds__(256) void als_prune_sample_thr_kernel(const float* __restrict__ vals, int n_users,
                                                                   int64_t n, int kk, const double* __restrict__ err,
                                                                   float* __restrict__ tau, float* __restrict__ thr2,
                                                                   int* __restrict__ cn, int* __restrict__ pn,
                                                                   int* __restrict__ overflow) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= n_users) return;  // wave-uniform
  const float* __restrict__ rv = vals + (int64_t)b * n;
  float m = -INFINITY;
  for (int64_t p = lane; p < n; p += 64) m = fmaxf(m, rv[p]);
  const float t = kth_of_lane_maxima(m, kk, lane);
  if (lane == 0) {
    pn[b] = 0;
    pr_bounds(b, t, err, tau, thr2, cn, overflow);
  }
}

// The exact JVM chain for every pair the bf16 filter kept (one block per
// user; a thread per candidate; the item's row-major factors as 16-B loads),
// appended to the candidate lists when it reaches tau_b. Steps c in
// [k, 4 ceil(k / 4)) add the fused kernel's zero products (its rank loop
// runs in steps of 4). A kept list past the cap raises *overflow here.
__global__ __launch_bounds__(256) void als_rescore_kernel(const float* __restrict__ U, int kp,
                                                          const int64_t* __restrict__ user_rows, int n_users, int k,
                                                          const float* __restrict__ V, int64_t ldv,
                                                          const int64_t* __restrict__ pre_i,
                                                          const int* __restrict__ pre_n, int cap,
                                                          const float* __restrict__ tau, int kk,
                                                          float* __restrict__ cand_v, int64_t* __restrict__ cand_i,
                                                          int* __restrict__ cand_n, int* __restrict__ overflow) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float su[kScoreKMax];
  const int b = blockIdx.x;
  const int64_t r = user_rows[b];
  if (r < 0) return;  // block-uniform: no candidates were kept
  if (threadIdx.x == 0 && pre_n[b] > cap) atomicOr(overflow, 1);
  for (int c = threadIdx.x; c < kp; c += blockDim.x) su[c] = c < k ? U[r * kp + c] : 0.f;
  __syncthreads();
  const int n = pre_n[b] < cap ? pre_n[b] : cap;
  const float t = tau[b];
  const int kr = (k + 3) & ~3;
  const int lane = threadIdx.x & 63;
  const bool vec = (ldv & 3) == 0 && ((uintptr_t)V & 15) == 0;
  for (int e0 = 0; e0 < n; e0 += blockDim.x) {  // block-uniform trip count: the ballots see whole waves
    const int e = e0 + threadIdx.x;
    float acc = 0.f;
    int64_t j = -1;
    if (e < n) {
      j = pre_i[(int64_t)b * cap + e];
      const float* v = V + j * ldv;
      int c = 0;
      if (vec) {
        for (; c + 4 <= k; c += 4) {
          const float4 x = *reinterpret_cast<const float4*>(v + c);
          acc = acc + su[c] * x.x;
          acc = acc + su[c + 1] * x.y;
          acc = acc + su[c + 2] * x.z;
          acc = acc + su[c + 3] * x.w;
        }
      }
      for (; c < k; ++c) acc = acc + su[c] * v[c];
      for (; c < kr; ++c) acc = acc + 0.f * 0.f;
    }
    const bool pass = e < n && acc >= t;
    const uint64_t m = __ballot(pass);
    if (m == 0) continue;
    int base = 0;
    const int leader = __builtin_ctzll(m);
    if (lane == leader) {
      base = atomicAdd(&cand_n[b], __popcll(m));
      if (base + __popcll(m) > cap) atomicOr(overflow, 1);
    }
    base = __shfl(base, leader, kWave);
    if (pass) {
      const int pos = base + lanes_below(m);
      if (pos < cap) {
        cand_v[(int64_t)b * cap + pos] = acc;
        cand_i[(int64_t)b * cap + pos] = j;
      }
    }
  }
  // fewer than kk candidates: tau_b was above the kk-th best chain (a bound
  // slip) -> the caller's exact fallback instead of (0, -1) padding
  __syncthreads();
  if (threadIdx.x == 0 && atomicAdd(&cand_n[b], 0) < kk) atomicOr(overflow, 1);
}

// 2. The bf16 bound filter: block = (UBK users staged in LDS, 64 NI items),
// wave = 16 NI items held in registers for the whole block, swept over the
// users in chunks of 64 (v_mfma_f32_16x16x32_bf16: A = items, B = users, so
// lane (g, c) holds user c and items 4 g + r). A pair passes when its s~
// reaches the user's bound; survivors are rare (~0.1 %): they are staged in
// LDS (LDS atomics) and leave at the block's end with one list reservation
// per user (a returning global atomic per survivor in the loop serialised the
// waves on its round trip: 84 us against 24 us of GEMM); a lane's passing
// pairs take one LDS reservation (a mask, then the entries), their per-user
// ranks are counted at the flush (LDS atomics per survivor in the loop: 56 us
// per launch against 46; the same launch without the survivor test: 16). Measured per
// 1024 x 100k call (whole call): 2 blocks per CU and 2048 staged survivors
// 130 us; 3 per CU / 1024 staged 138; 4 per CU 132; 1 per CU 161; the next
// tile's fragments prefetched (186 VGPRs) 175.
typedef __bf16 pr_bf8 __attribute__((ext_vector_type(8)));
__host__ __device__ constexpr int prune_filter_users(int dk) { return dk <= 64 ? 256 : (dk == 128 ? 128 : 64); }
typedef float pr_f4 __attribute__((ext_vector_type(4)));

// MAXONLY (the sample bound, step 1): no test; per (user, wave tile of 16 NI
// items) the largest s~ goes to wmax[b * n_wt + tile] — disjoint item sets,
// so the kk-th largest of those maxima is reached by kk distinct items.
template <int DK, bool MAXONLY>
__global__ __launch_bounds__(256) void als_bound_filter_kernel(const uint16_t* __restrict__ uop, int n_users,
                                                               const uint16_t* __restrict__ items, int64_t N,
                                                               const float* __restrict__ thr2, int cap,
                                                               int64_t* __restrict__ pre_i, int* __restrict__ pre_n,
                                                               float* __restrict__ wmax) {
  constexpr int KS = DK / 32;
  constexpr int NI = DK <= 64 ? 4 : (DK == 128 ? 2 : 1);
  constexpr int UBK = prune_filter_users(DK);  // <= 36 KiB of users per block
  constexpr int RB = DK * 2 + 16;  // padded LDS rows: the 16 lanes of a row group hit different banks
  constexpr int CPR = DK / 8;      // 16-B chunks per user row
  constexpr int kPer = UBK * CPR / 256;
  static_assert(kPer * 256 == UBK * CPR, "whole chunks per thread");
  constexpr int kSB = 2048;  // survivors a block stages (then one list reservation per user)
  __shared__ __attribute__((aligned(16))) char us[UBK * RB];
  __shared__ float sth[UBK];
  __shared__ int s_cnt[UBK];
  __shared__ int s_n;
  __shared__ uint32_t s_item[kSB];
  __shared__ int s_rank[kSB];
  __shared__ uint16_t s_user[kSB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int n_ut = (n_users + UBK - 1) / UBK;
  const int ut = (int)(blockIdx.x % (unsigned)n_ut);
  const int64_t it0 = blockIdx.x / (unsigned)n_ut, it_step = gridDim.x / (unsigned)n_ut;
  const int64_t n_it = (N + 64 * NI - 1) / (64 * NI);
  const int b0 = ut * UBK;
  const int ub = n_users - b0 < UBK ? n_users - b0 : UBK;
  int4 fa[KS][NI];  // this item tile's fragments
  auto load_items = [&](int64_t it, int4 (&fi)[KS][NI]) {
    const int64_t j0 = it * (64 * NI) + 16 * NI * w;
#pragma unroll
    for (int t = 0; t < NI; ++t) {
      const int64_t j = j0 + 16 * t + c;
      const int64_t jr = j < N ? j : N - 1;  // rows past the end: a valid row, masked at the test
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        fi[ks][t] = *reinterpret_cast<const int4*>(items + jr * DK + 32 * ks + 8 * g);
    }
  };
  if (it0 < n_it) load_items(it0, fa);  // in flight while the users are staged
  {  // users -> LDS: every load of a thread in flight before its stores
    int4 v[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int o = threadIdx.x + 256 * e, r = o / CPR, q = o % CPR;
      v[e] = r < ub ? *reinterpret_cast<const int4*>(uop + (int64_t)(b0 + r) * DK + 8 * q) : int4{0, 0, 0, 0};
    }
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int o = threadIdx.x + 256 * e, r = o / CPR, q = o % CPR;
      *reinterpret_cast<int4*>(us + r * RB + 16 * q) = v[e];
    }
  }
  for (int o = threadIdx.x; o < UBK; o += 256) {
    sth[o] = (!MAXONLY && o < ub) ? thr2[b0 + o] : __builtin_nanf("");  // MAXONLY: no bounds (thr2 null)
    s_cnt[o] = 0;
  }
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int nch = (ub + 63) / 64;
  auto tile = [&](int64_t it, int4 (&fi)[KS][NI]) {
    if (it != it0) load_items(it, fi);
    const int64_t j0 = it * (64 * NI) + 16 * NI * w;
    for (int ch = 0; ch < nch; ++ch) {
      pr_f4 acc[4][NI];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int t = 0; t < NI; ++t) acc[u][t] = pr_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        int4 uf[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          uf[u] = *reinterpret_cast<const int4*>(us + (64 * ch + 16 * u + c) * RB + 64 * ks + 16 * g);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int t = 0; t < NI; ++t)
            acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pr_bf8, fi[ks][t]),
                                                                __builtin_bit_cast(pr_bf8, uf[u]), acc[u][t], 0, 0,
                                                                0);
      }
      const bool full = j0 + 16 * NI <= N;  // wave-uniform: every item of the wave in range
      if constexpr (MAXONLY) {
        const int64_t n_wt = (N + 16 * NI - 1) / (16 * NI);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float mx = -INFINITY;
#pragma unroll
          for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (full || j0 + 16 * t + 4 * g + r < N) mx = fmaxf(mx, acc[u][t][r]);
          mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
          mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
          const int ul = 64 * ch + 16 * u + c;
          if (g == 0 && ul < ub && j0 < N) wmax[(int64_t)(b0 + ul) * n_wt + j0 / (16 * NI)] = mx;
        }
        continue;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ul = 64 * ch + 16 * u + c;
        const float th = sth[ul];  // NaN (absent user): nothing passes
        float mx = -INFINITY;
        if (full) {
#pragma unroll
          for (int t = 0; t < NI; ++t)
            mx = fmaxf(mx, fmaxf(fmaxf(acc[u][t][0], acc[u][t][1]), fmaxf(acc[u][t][2], acc[u][t][3])));
        } else {
#pragma unroll
          for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (j0 + 16 * t + 4 * g + r < N) mx = fmaxf(mx, acc[u][t][r]);
        }
        if (__ballot(mx >= th) == 0) continue;
        {
          // the lane's passing (t, r) as a mask; one LDS reservation per lane
          uint32_t m = 0;
#pragma unroll
          for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (j0 + 16 * t + 4 * g + r < N && acc[u][t][r] >= th) m |= 1u << (4 * t + r);
          if (m) {
            int e = atomicAdd(&s_n, __popc(m));  // LDS
            while (m) {
              const int q = __builtin_ctz(m);
              m &= m - 1;
              const int64_t j = j0 + 16 * (q >> 2) + 4 * g + (q & 3);
              if (e < kSB) {
                s_item[e] = (uint32_t)j;
                s_user[e] = (uint16_t)ul;
              } else {  // staging full: straight to the user's list
                const int64_t b = b0 + ul;
                const int p = atomicAdd(&pre_n[b], 1);
                if (p < cap) pre_i[b * cap + p] = j;
              }
              ++e;
            }
          }
        }
      }
    }
  };
  for (int64_t it = it0; it < n_it; it += it_step) tile(it, fa);
  if constexpr (MAXONLY) return;
  // flush: one list reservation per user with staged survivors, then the entries
  __syncthreads();
  {  // ranks per user (LDS atomics, off the MFMA loop)
    const int ne0 = s_n < kSB ? s_n : kSB;
    for (int e = threadIdx.x; e < ne0; e += 256) s_rank[e] = atomicAdd(&s_cnt[s_user[e]], 1);
    __syncthreads();
  }
  for (int o = threadIdx.x; o < ub; o += 256) {
    const int k = s_cnt[o];
    s_cnt[o] = k ? atomicAdd(&pre_n[b0 + o], k) : 0;
  }
  __syncthreads();
  const int ne = s_n < kSB ? s_n : kSB;
  for (int e = threadIdx.x; e < ne; e += 256) {
    const int ul = s_user[e];
    const int p = s_cnt[ul] + s_rank[e];
    if (p < cap) pre_i[(int64_t)(b0 + ul) * cap + p] = (int64_t)s_item[e];
  }
}

// 3+4 fused for kk <= 8: the candidates stay in LDS and wave 0 ranks them
// exactly as topk_wave_kernel does (per-lane sorted lists of KK, then kk
// rounds of wave arg-best; absent entries -> (0, -1)), so the call skips the
// list round trip and the top-k launch. cand_n[b] still counts the
// candidates (the bench's diagnostics; > cap raises *overflow).
// EXCL (hrec_als_score_topk_pruned_excluding): a candidate whose chain reaches
// tau_b is looked up in the query's ascending exclusion segment (the binary
// search of excl_drop_kernel) and, when found, never enters the LDS list;
// the ones that stay are counted by ballots (the loop's trip count is rounded
// up to whole blocks so the ballots see whole waves) into s_n, an LDS integer,
// which also reserves their slots: cand_n[b] and the overflow tests are then
// over the candidates that stay, and out_len[b] = min(kk, s_n). Without EXCL
// the three extra arguments are not read.
template <int KK, bool EXCL>
__global__ __launch_bounds__(256) void als_rescore_topk_kernel(const float* __restrict__ U, int kp,
                                                               const int64_t* __restrict__ user_rows, int n_users,
                                                               int k, const float* __restrict__ V, int64_t ldv,
                                                               const int64_t* __restrict__ pre_i,
                                                               const int* __restrict__ pre_n, int cap,
                                                               const float* __restrict__ tau, int kk,
                                                               int64_t* __restrict__ out_idx,
                                                               float* __restrict__ out_val, int* __restrict__ cand_n,
                                                               int* __restrict__ overflow,
                                                               const int64_t* __restrict__ excl_indptr,
                                                               const int32_t* __restrict__ excl_cols,
                                                               int32_t* __restrict__ out_len) {
#pragma clang fp contract(off)
  constexpr int kL = 2048;  // candidates kept in LDS (more: *overflow, the caller's fallback)
  __shared__ __attribute__((aligned(16))) float su[kScoreKMax];
  __shared__ float s_v[kL];
  __shared__ int s_j[kL];
  __shared__ int s_n;
  const int b = blockIdx.x;
  const int64_t r = user_rows[b];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) s_n = 0;
  if (r >= 0) {
    if (threadIdx.x == 0 && pre_n[b] > cap) atomicOr(overflow, 1);
    for (int c = threadIdx.x; c < kp; c += blockDim.x) su[c] = c < k ? U[r * kp + c] : 0.f;
  }
  __syncthreads();
  if (r >= 0) {
    const int n = pre_n[b] < cap ? pre_n[b] : cap;
    const float t = tau[b];
    const int kr = (k + 3) & ~3;
    const bool vec = (ldv & 3) == 0 && ((uintptr_t)V & 15) == 0;
    const ExclSeg xs = excl_segment(EXCL ? excl_indptr : nullptr, r);
    // EXCL: a block-uniform trip count, so the ballots below see whole waves
    const int e_end = EXCL ? (int)((n + blockDim.x - 1) / blockDim.x * blockDim.x) : n;
    for (int e = threadIdx.x; e < e_end; e += blockDim.x) {
      float acc = 0.f;
      int64_t j = 0;
      bool pass = false;
      if (!EXCL || e < n) {
        j = pre_i[(int64_t)b * cap + e];
        const float* v = V + j * ldv;
        int c = 0;
        if (vec) {
          for (; c + 4 <= k; c += 4) {
            const float4 x = *reinterpret_cast<const float4*>(v + c);
            acc = acc + su[c] * x.x;
            acc = acc + su[c + 1] * x.y;
            acc = acc + su[c + 2] * x.z;
            acc = acc + su[c + 3] * x.w;
          }
        }
        for (; c < k; ++c) acc = acc + su[c] * v[c];
        for (; c < kr; ++c) acc = acc + 0.f * 0.f;
        pass = acc >= t;
      }
      if constexpr (EXCL) {
        pass = pass && !excl_contains(excl_cols, xs.lo, xs.hi, j);
        const uint64_t keep = __ballot(pass);
        if (keep) {
          int base = 0;
          const int leader = __builtin_ctzll(keep);
          if (lane == leader) base = atomicAdd(&s_n, __popcll(keep));  // LDS, integer
          base = __shfl(base, leader, kWave);
          const int p = base + lanes_below(keep);
          if (pass && p < kL) {
            s_v[p] = acc;
            s_j[p] = (int)j;
          }
        }
      } else if (pass) {
        const int p = atomicAdd(&s_n, 1);  // LDS
        if (p < kL) {
          s_v[p] = acc;
          s_j[p] = (int)j;
        }
      }
    }
  }
  __syncthreads();
  const int m = s_n;
  if (threadIdx.x == 0) {
    if constexpr (EXCL) out_len[b] = m < kk ? m : kk;
    cand_n[b] = m;
    // fewer than kk candidates for a known user: tau_b was above the kk-th
    // best chain (a bound slip) -> the caller's exact fallback, never short ids
    if (m > kL || m > cap || (r >= 0 && m < kk)) atomicOr(overflow, 1);
  }
  if (threadIdx.x >= 64) return;  // wave 0 ranks
  const int mm = m < kL ? m : kL;
  float lv[KK];
  int64_t li[KK];
#pragma unroll
  for (int q = 0; q < KK; ++q) {
    lv[q] = 0.f;
    li[q] = INT64_MAX;
  }
  for (int p = lane; p < mm; p += 64) {
    float xv = s_v[p];
    int64_t xi = s_j[p];
#pragma unroll
    for (int q = 0; q < KK; ++q) {
      const bool sw = li[q] == INT64_MAX || better(xv, xi, lv[q], li[q]);
      const float tv = lv[q];
      const int64_t ti = li[q];
      lv[q] = sw ? xv : tv;
      li[q] = sw ? xi : ti;
      xv = sw ? tv : xv;
      xi = sw ? ti : xi;
      if (xi == INT64_MAX) break;
    }
  }
  for (int q = 0; q < kk; ++q) {
    const KV<float> w = wave_best(KV<float>{lv[0], li[0]});
    if (lane == 0) {
      out_val[(int64_t)b * kk + q] = w.i == INT64_MAX ? 0.f : w.v;
      out_idx[(int64_t)b * kk + q] = w.i == INT64_MAX ? -1 : w.i;
    }
    if (w.i != INT64_MAX && li[0] == w.i) {
#pragma unroll
      for (int x = 0; x + 1 < KK; ++x) {
        lv[x] = lv[x + 1];
        li[x] = li[x + 1];
      }
      li[KK - 1] = INT64_MAX;
    }
  }
}

// The exact fallback of the pruned top-k for kk <= 8, on the device: when
// *gate != 0 (a user overflowed a list or had no finite bound), every user's
// stable top-kk of the JVM chain over ALL items — the chain of
// als_rescore_topk_kernel (and of the fused path), one block per user, a
// sorted list of KK per thread, then wave and block merges by arg-best rounds
// (ties -> smaller item, NaN last). An unknown user (row < 0) gets the
// pruned path's answer for it, no candidates: (0, -1) entries. Gate 0:
// every block returns after one load (no host round trip decides the
// fallback).
template <int KK>
__global__ __launch_bounds__(256) void als_exact_topk_kernel(const float* __restrict__ U, int kp,
                                                             const int64_t* __restrict__ user_rows, int n_users,
                                                             int k, const float* __restrict__ V, int64_t ldv,
                                                             int64_t N, int kk, const int* __restrict__ gate,
                                                             int64_t* __restrict__ out_idx,
                                                             float* __restrict__ out_val) {
#pragma clang fp contract(off)
  if (*gate == 0) return;  // block-uniform
  __shared__ __attribute__((aligned(16))) float su[kScoreKMax];
  __shared__ float s_v[4 * KK];
  __shared__ int64_t s_i[4 * KK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int kr = (k + 3) & ~3;
  const bool vec = (ldv & 3) == 0 && ((uintptr_t)V & 15) == 0;
  for (int b = blockIdx.x; b < n_users; b += gridDim.x) {  // block-uniform trip count
    const int64_t r = user_rows[b];
    if (r < 0) {
      for (int q = threadIdx.x; q < kk; q += blockDim.x) {
        out_val[(int64_t)b * kk + q] = 0.f;
        out_idx[(int64_t)b * kk + q] = -1;
      }
      continue;
    }
    __syncthreads();  // the previous user's readers of su / s_v are done
    for (int c = threadIdx.x; c < kp; c += blockDim.x) su[c] = c < k ? U[r * kp + c] : 0.f;
    __syncthreads();
    float lv[KK];
    int64_t li[KK];
#pragma unroll
    for (int q = 0; q < KK; ++q) {
      lv[q] = 0.f;
      li[q] = INT64_MAX;
    }
    for (int64_t j = threadIdx.x; j < N; j += blockDim.x) {
      float acc = 0.f;
      const float* v = V + j * ldv;
      int c = 0;
      if (vec) {
        for (; c + 4 <= k; c += 4) {
          const float4 x = *reinterpret_cast<const float4*>(v + c);
          acc = acc + su[c] * x.x;
          acc = acc + su[c + 1] * x.y;
          acc = acc + su[c + 2] * x.z;
          acc = acc + su[c + 3] * x.w;
        }
      }
      for (; c < k; ++c) acc = acc + su[c] * v[c];
      for (; c < kr; ++c) acc = acc + 0.f * 0.f;
      float xv = acc;
      int64_t xi = j;
#pragma unroll
      for (int q = 0; q < KK; ++q) {
        const bool sw = li[q] == INT64_MAX || better(xv, xi, lv[q], li[q]);
        const float tv = lv[q];
        const int64_t ti = li[q];
        lv[q] = sw ? xv : tv;
        li[q] = sw ? xi : ti;
        xv = sw ? tv : xv;
        xi = sw ? ti : xi;
      }
    }
    // each wave's best kk -> LDS, then wave 0 merges the four lists
    for (int q = 0; q < kk; ++q) {
      const KV<float> x = wave_best(KV<float>{lv[0], li[0]});
      if (lane == 0) {
        s_v[w * KK + q] = x.v;
        s_i[w * KK + q] = x.i;
      }
      if (x.i != INT64_MAX && li[0] == x.i) {
#pragma unroll
        for (int e = 0; e + 1 < KK; ++e) {
          lv[e] = lv[e + 1];
          li[e] = li[e + 1];
        }
        li[KK - 1] = INT64_MAX;
      }
    }
    __syncthreads();
    if (w == 0) {
      KV<float> m{0.f, INT64_MAX};
      if (lane < 4 * KK && lane % KK < kk) m = KV<float>{s_v[lane], s_i[lane]};
      for (int q = 0; q < kk; ++q) {
        const KV<float> x = wave_best(m);
        if (lane == 0) {
          out_val[(int64_t)b * kk + q] = x.i == INT64_MAX ? 0.f : x.v;
          out_idx[(int64_t)b * kk + q] = x.i == INT64_MAX ? -1 : x.i;
        }
        if (x.i != INT64_MAX && m.i == x.i) m.i = INT64_MAX;
      }
    }
  }
}

template <bool MAXONLY>
static int bound_filter_launch(int dk, dim3 grid, hipStream_t s, const uint16_t* uop, int n_users,
                               const uint16_t* items, int64_t N, const float* thr2, int cap, int64_t* pre_i,
                               int* pre_n, float* wmax) {
  switch (dk) {
    case 32: hipLaunchKernelGGL((als_bound_filter_kernel<32, MAXONLY>), grid, dim3(256), 0, s, uop, n_users, items, N,
                                thr2, cap, pre_i, pre_n, wmax); break;
    case 64: hipLaunchKernelGGL((als_bound_filter_kernel<64, MAXONLY>), grid, dim3(256), 0, s, uop, n_users, items, N,
                                thr2, cap, pre_i, pre_n, wmax); break;
    case 128: hipLaunchKernelGGL((als_bound_filter_kernel<128, MAXONLY>), grid, dim3(256), 0, s, uop, n_users, items,
                                 N, thr2, cap, pre_i, pre_n, wmax); break;
    default: hipLaunchKernelGGL((als_bound_filter_kernel<256, MAXONLY>), grid, dim3(256), 0, s, uop, n_users, items,
                                N, thr2, cap, pre_i, pre_n, wmax); break;
  }
  return check_launch("als_bound_filter_kernel");
}

// blocks of the bound filter over n items: two per CU, each walking its user
// tile over every (grid / n_ut)-th item tile (the staged users serve several)
static dim3 bound_filter_grid(int dk, int n_users, int64_t n) {
  const int64_t n_ut = (n_users + prune_filter_users(dk) - 1) / prune_filter_users(dk);
  const int per = dk <= 64 ? 256 : (dk == 128 ? 128 : 64);  // items per block round
  const int64_t n_it = (n + per - 1) / per;
  int64_t per_ut = (512 + n_ut - 1) / n_ut;
  if (per_ut > n_it) per_ut = n_it;
  return dim3((unsigned)(n_ut * per_ut));
}

static int prune_dk(int k) { return k <= 32 ? 32 : (k <= 64 ? 64 : (k <= 128 ? 128 : 256)); }

extern "C" size_t hrec_als_items_bf16_bytes(int64_t n_items, int k) {
  const int64_t n = n_items > 0 ? n_items : 0;
  return al256((size_t)n * prune_dk(k) * 2) + 256;
}

extern "C" int hrec_als_items_bf16(const float* item_factors, int64_t ld_v, int64_t n_items, int k, void* out,
                                   size_t out_bytes, void* stream) {
  HREC_REQUIRE(k >= 1 && k <= kScoreKMax && n_items >= 0 && ld_v >= k, "als_items_bf16: bad shape");
  HREC_REQUIRE(out && out_bytes >= hrec_als_items_bf16_bytes(n_items, k) && ((uintptr_t)out & 255) == 0,
               "als_items_bf16: output must be 256-B aligned, %zu bytes", hrec_als_items_bf16_bytes(n_items, k));
  HREC_REQUIRE(n_items == 0 || item_factors, "als_items_bf16: null factors");
  hipStream_t s = as_stream(stream);
  const int dk = prune_dk(k);
  unsigned* nrm = reinterpret_cast<unsigned*>(static_cast<char*>(out) + hrec_als_items_bf16_bytes(n_items, k) - 256);
  if (hipMemsetAsync(nrm, 0, 4, s) != hipSuccess) return check_launch("als_items_bf16: memset");
  if (n_items == 0) return HREC_OK;
  hipLaunchKernelGGL(als_items_bf16_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, s, item_factors,
                     ld_v, n_items, k, dk, static_cast<uint16_t*>(out), nrm);
  return check_launch("als_items_bf16_kernel");
}

// Workspace of the pruned path: the cascade's buffers (samp: bf16 sample scores or wave-tile maxima; cv / ci /
// cn: the candidates with chain >= tau) and its own (hrec_als_score_topk_pruned_counts reads the two counters).
struct PruneWs {
  CascadeWs c;
  double* err;   // [B] E_b
  float* tau;    // [B]
  float* thr2;   // [B]
  uint16_t* uop; // [B][dk]
  int64_t* pi;   // [B][cap] the bf16 filter's kept items
  int* pn;       // [B]
  size_t total;
};

static PruneWs prune_layout(char* base, int B, int64_t N, int kk, int dk) {
  PruneWs w{};
  Carver c(base);
  // counters of exactly B ints here (the fused layout pads its own by 16 B); a 256-B tail as there
  w.c = cascade_carve(c, B, N < kPruneSample ? N : kPruneSample, kCap, kk, 0);
  w.err = (double*)c.take((size_t)B * 8);
  w.tau = (float*)c.take((size_t)B * 4);
  w.thr2 = (float*)c.take((size_t)B * 4);
  w.uop = (uint16_t*)c.take((size_t)B * dk * 2);
  w.pi = (int64_t*)c.take((size_t)B * kCap * 8);
  w.pn = (int*)c.take((size_t)B * 4);
  w.total = c.total() + 256;
  return w;
}

extern "C" size_t hrec_als_score_topk_pruned_workspace_bytes(int n_users, int64_t n_items, int top_k, int k) {
  const int B = n_users > 0 ? n_users : 0;
  const int64_t N = n_items > 0 ? n_items : 0;
  const int kk = score_kk(N, top_k);
  const size_t fused = hrec_als_score_topk_workspace_bytes(n_users, n_items, top_k);  // the small-catalogue path
  const size_t own = prune_layout(nullptr, B, N, kk, prune_dk(k)).total;
  return own > fused ? own : fused;
}

extern "C" int hrec_als_score_topk_pruned_counts(const void* workspace, int n_users, int64_t n_items, int top_k,
                                                 int k, int32_t* out, void* stream) {
  HREC_REQUIRE(workspace && out && n_users >= 0 && n_items >= 0 && k >= 1 && k <= kScoreKMax && top_k >= 1,
               "als_score_topk_pruned_counts: bad argument");
  if (n_users == 0) return HREC_OK;
  hipStream_t s = as_stream(stream);
  if (n_items <= kSample) {  // the fused path ran: no bf16 filter
    if (hipMemsetAsync(out, 0, (size_t)2 * n_users * 4, s) != hipSuccess)
      return check_launch("als_score_topk_pruned_counts: memset");
    return HREC_OK;
  }
  const PruneWs w = prune_layout((char*)workspace, n_users, n_items, score_kk(n_items, top_k), prune_dk(k));
  if (hipMemcpyAsync(out, w.pn, (size_t)n_users * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(out + n_users, w.c.cn, (size_t)n_users * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return check_launch("als_score_topk_pruned_counts: copy");
  return HREC_OK;
}

// The small-catalogue path is hrec_als_score_topk_excluding's: the larger of the two needs.
extern "C" size_t hrec_als_score_topk_pruned_excluding_workspace_bytes(int n_users, int64_t n_items, int top_k,
                                                                       int k) {
  const size_t own = hrec_als_score_topk_pruned_workspace_bytes(n_users, n_items, top_k, k);
  const size_t fused = hrec_als_score_topk_excluding_workspace_bytes(n_users, n_items, top_k);
  return own > fused ? own : fused;
}

// hrec_als_score_topk_pruned and hrec_als_score_topk_pruned_excluding (x.on):
// the same launches, the exclusion behind x.on.
//   Under an exclusion the bf16 scores s~ of the first S = min(n_items, 8192)
//   items are materialised for every kk (the wave-tile maxima of the kk <= 64
//   form have no per-item score to mask) and cascade_bound (csrc/cascade.hip
//   has the argument) gives t_b over the sample's items that stay: kk such
//   items have chain >= s~ - E_b >= t_b - E_b >= tau_b, so every entry of the
//   answer passes the filter at tau_b - E_b and the exact test. A t_b of -inf
//   becomes the overflow flag in pr_bounds. The excluded items the filter kept
//   leave after the exact chain (kk > 8: cascade_tail; kk <= 8: inside the
//   fused rescore-and-rank kernel). als_rescore_kernel's "fewer than kk
//   candidates" test counts before the drop and stays right: with a finite
//   bound at least kk non-excluded items reach tau_b. Nothing is resolved on
//   the device here: a set *overflow means the answer is incomplete at every kk.
static int score_topk_pruned_run(const char* fn, const float* user_factors, const int64_t* user_rows, int n_users,
                                 const float* item_factors_t, int64_t ld_items, const float* item_factors,
                                 int64_t ld_v, const void* items_bf16, int64_t n_items, int k, int kp, int top_k,
                                 int64_t* out_idx, float* out_val, int* overflow, void* workspace,
                                 size_t workspace_bytes, const Excl& x, void* stream) {
  const bool excl = x.on;
  HREC_REQUIRE(hrec_factor_ld_ok(kp), "%s: kp must be 16, 32, 64, 96, 128, 192 or 256", fn);
  HREC_REQUIRE(k >= 1 && k <= kp, "%s: need 1 <= k <= kp", fn);
  HREC_REQUIRE(n_users >= 0 && n_users < 65536 && n_items >= 0, "%s: bad shape", fn);
  HREC_REQUIRE(ld_items >= n_items && ld_items % 4 == 0 && ld_items < ((int64_t)1 << 29),
               "%s: ld_items must be >= n_items, %% 4 and < 2^29", fn);
  HREC_REQUIRE(ld_v >= k, "%s: ld_v must be >= k", fn);
  HREC_REQUIRE(top_k >= 1 && top_k <= 1024, "%s: top_k must be in [1, 1024]", fn);
  if (n_users == 0 || n_items == 0) return HREC_OK;
  HREC_REQUIRE(user_factors && user_rows && item_factors_t && item_factors && items_bf16 && out_idx && out_val &&
                   overflow && workspace,
               "%s: null pointer", fn);
  HREC_REQUIRE(!excl || (x.indptr && x.cols && x.out_len), "%s: null exclusion or out_len", fn);
  HREC_REQUIRE(((uintptr_t)items_bf16 & 255) == 0, "%s: items_bf16 must be 256-B aligned", fn);
  const size_t need = excl ? hrec_als_score_topk_pruned_excluding_workspace_bytes(n_users, n_items, top_k, k)
                           : hrec_als_score_topk_pruned_workspace_bytes(n_users, n_items, top_k, k);
  HREC_REQUIRE(workspace_bytes >= need, "%s: workspace %zu < %zu", fn, workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const int kk = (int)(top_k < n_items ? top_k : n_items);
  // kk <= 8: a set *overflow is resolved here, on the device (the gated
  // exact top-k over every item), so the result is always exact
  auto exact_fallback = [&]() {
    if (kk > 8) return (int)HREC_OK;
#define HREC_EXT(KK)                                                                                             \
  hipLaunchKernelGGL(als_exact_topk_kernel<KK>, dim3((unsigned)(n_users < 512 ? n_users : 512)), dim3(256), 0, s,  \
                     user_factors, kp, user_rows, n_users, k, item_factors, ld_v, n_items, kk, overflow, out_idx,     \
                     out_val)
    if (kk <= 2) HREC_EXT(2);
    else if (kk <= 4) HREC_EXT(4);
    else HREC_EXT(8);
#undef HREC_EXT
    return check_launch("als_exact_topk_kernel");
  };
  if (n_items <= kSample) {  // small: the fused path scores everything anyway
    const int rc = score_topk_run(fn, user_factors, user_rows, n_users, item_factors_t, ld_items, n_items, k, kp,
                                  top_k, out_idx, out_val, overflow, workspace, workspace_bytes, x, stream);
    return (rc || excl) ? rc : exact_fallback();
  }
  const int dk = prune_dk(k);
  const PruneWs w = prune_layout((char*)workspace, n_users, n_items, kk, dk);
  const int64_t S = n_items < kPruneSample ? n_items : kPruneSample;
  const float* max_norm = reinterpret_cast<const float*>(static_cast<const char*>(items_bf16) +
                                                         hrec_als_items_bf16_bytes(n_items, k) - 256);
  // 1) bf16 user operands and E_b (and *overflow = 0); the sample's bf16 scores; its bound
  hipLaunchKernelGGL(als_prune_user_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, s, user_factors, kp,
                     user_rows, n_users, k, dk, max_norm, w.uop, w.err, overflow);
  int rc = check_launch("als_prune_user_kernel");
  if (rc) return rc;
  if (kk <= 64 && !excl) {
    // per (user, 16 NI-item wave tile) maxima of the sample (no score
    // matrix), then the kk-th of their 64 lane maxima: kk distinct items of
    // the sample reach it; zeroes pn
    const int ni = dk <= 64 ? 4 : (dk == 128 ? 2 : 1);
    const int64_t SM = n_items < kPruneSampleMax ? n_items : kPruneSampleMax;
    const int64_t n_wt = (SM + 16 * ni - 1) / (16 * ni);  // <= min(n_items, 8192) = the samp row length
    rc = bound_filter_launch<true>(dk, bound_filter_grid(dk, n_users, SM), s, w.uop, n_users,
                                   static_cast<const uint16_t*>(items_bf16), SM, nullptr, 0, nullptr, nullptr,
                                   w.c.samp);
    if (rc) return rc;
    hipLaunchKernelGGL(als_prune_sample_thr_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, s,
                       w.c.samp, n_users, n_wt, kk, w.err, w.tau, w.thr2, w.c.cn, w.pn, overflow);
    rc = check_launch("als_prune_sample_thr_kernel");
    if (rc) return rc;
  } else {
    rc = dot_scores_run(w.uop, n_users, items_bf16, S, dk, 1, w.c.samp, S, s, kPruneSampleUB);
    if (rc) return rc;
    // the first S items, no lengths; kk <= 64 (under an exclusion only) takes the lane maxima; zeroes pn
    const float* thr;
    int thr_stride;
    rc = cascade_bound(w.c, n_users, S, 1, S, kk, x, nullptr, true, w.pn, &thr, &thr_stride, s);
    if (rc) return rc;
    hipLaunchKernelGGL(als_prune_thr_kernel, dim3((unsigned)((n_users + 255) / 256)), dim3(256), 0, s, n_users,
                       thr, thr_stride, w.err, w.tau, w.thr2, w.c.cn, overflow);
    rc = check_launch("als_prune_thr_kernel");
    if (rc) return rc;
  }
  // 2) the matrix-core filter over every item at tau_b - E_b
  rc = bound_filter_launch<false>(dk, bound_filter_grid(dk, n_users, n_items), s, w.uop, n_users,
                                  static_cast<const uint16_t*>(items_bf16), n_items, w.thr2, kCap, w.pi, w.pn, nullptr);
  if (rc) return rc;
  // 3) the exact chain over the kept pairs -> candidates (chain >= tau_b);
  //    kk <= 8: ranked in the same block
  if (kk <= 8) {
#define HREC_RTK(KK, EXCL)                                                                                     \
  hipLaunchKernelGGL((als_rescore_topk_kernel<KK, EXCL>), dim3((unsigned)n_users), dim3(256), 0, s, user_factors,  \
                     kp, user_rows, n_users, k, item_factors, ld_v, w.pi, w.pn, kCap, w.tau, kk, out_idx, out_val, \
                     w.c.cn, overflow, x.indptr, x.cols, x.out_len)
    if (excl) {  // the excluded candidates never enter the ranked list; writes out_len
      if (kk <= 2) HREC_RTK(2, true);
      else if (kk <= 4) HREC_RTK(4, true);
      else HREC_RTK(8, true);
      return check_launch("als_rescore_topk_kernel(excluding)");
    }
    if (kk <= 2) HREC_RTK(2, false);
    else if (kk <= 4) HREC_RTK(4, false);
    else HREC_RTK(8, false);
#undef HREC_RTK
    rc = check_launch("als_rescore_topk_kernel");
    return rc ? rc : exact_fallback();
  }
  hipLaunchKernelGGL(als_rescore_kernel, dim3((unsigned)n_users), dim3(256), 0, s, user_factors, kp, user_rows,
                     n_users, k, item_factors, ld_v, w.pi, w.pn, kCap, w.tau, kk, w.c.cv, w.c.ci, w.c.cn, overflow);
  rc = check_launch("als_rescore_kernel");
  if (rc) return rc;
  // 4) the excluded candidates leave (writing out_len); the same exact stable top-k over the rest
  return cascade_tail(w.c, n_users, kCap, kk, x, x.out_len, out_idx, out_val, s);
}

extern "C" int hrec_als_score_topk_pruned(const float* user_factors, const int64_t* user_rows, int n_users,
                                          const float* item_factors_t, int64_t ld_items, const float* item_factors,
                                          int64_t ld_v, const void* items_bf16, int64_t n_items, int k, int kp,
                                          int top_k, int64_t* out_idx, float* out_val, int* overflow,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return score_topk_pruned_run("als_score_topk_pruned", user_factors, user_rows, n_users, item_factors_t, ld_items,
                               item_factors, ld_v, items_bf16, n_items, k, kp, top_k, out_idx, out_val, overflow,
                               workspace, workspace_bytes, Excl{}, stream);
}

extern "C" int hrec_als_score_topk_pruned_excluding(const float* user_factors, const int64_t* user_rows, int n_users,
                                                    const float* item_factors_t, int64_t ld_items,
                                                    const float* item_factors, int64_t ld_v, const void* items_bf16,
                                                    int64_t n_items, int k, int kp, int top_k,
                                                    const int64_t* excl_indptr, const int32_t* excl_cols,
                                                    int64_t* out_idx, float* out_val, int32_t* out_len, int* overflow,
                                                    void* workspace, size_t workspace_bytes, void* stream) {
  return score_topk_pruned_run("als_score_topk_pruned_excluding", user_factors, user_rows, n_users, item_factors_t,
                               ld_items, item_factors, ld_v, items_bf16, n_items, k, kp, top_k, out_idx, out_val,
                               overflow, workspace, workspace_bytes,
                               Excl{true, user_rows, excl_indptr, excl_cols, out_len}, stream);
}
