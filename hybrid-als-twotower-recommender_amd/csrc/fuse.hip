// K9: hybrid min-max fusion (src/hybrid_system.py:57-75) + top-k (:108):
// the single-row form (hrec_fuse_topk, f64 ALS scores) and the batched rows
// form (hrec_fuse_rows_topk, f32 scores with given per-row min / max). The
// scaler and fusion arithmetic is hp_scale / hp_fuse of hybrid_common.h, the
// top-k of the fused scores csrc/topk.hip.
#include "hybrid_common.h"

namespace hrec {

// ---------------------------------------------------------------- fusion
// sklearn MinMaxScaler.fit_transform (container sklearn _data.py:518-522,
// 261-262): scale = 1/range (range < 10*eps -> 1), min_ = 0 - min*scale,
// y = x*scale + min_ ; two roundings each, in the input dtype.
__global__ __launch_bounds__(256) void minmax_partial_kernel(const double* __restrict__ als,
                                                             const void* __restrict__ tt, int tt_f32,
                                                             int64_t n, double* __restrict__ part) {
  __shared__ double sh[4][256];
  double amin = DBL_MAX, amax = -DBL_MAX, tmin = DBL_MAX, tmax = -DBL_MAX;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const double a = als[p];
    const double t = tt_f32 ? (double)((const float*)tt)[p] : ((const double*)tt)[p];
    amin = fmin(amin, a);
    amax = fmax(amax, a);
    tmin = fmin(tmin, t);
    tmax = fmax(tmax, t);
  }
  sh[0][threadIdx.x] = amin;
  sh[1][threadIdx.x] = amax;
  sh[2][threadIdx.x] = tmin;
  sh[3][threadIdx.x] = tmax;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sh[0][threadIdx.x] = fmin(sh[0][threadIdx.x], sh[0][threadIdx.x + s]);
      sh[1][threadIdx.x] = fmax(sh[1][threadIdx.x], sh[1][threadIdx.x + s]);
      sh[2][threadIdx.x] = fmin(sh[2][threadIdx.x], sh[2][threadIdx.x + s]);
      sh[3][threadIdx.x] = fmax(sh[3][threadIdx.x], sh[3][threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) part[blockIdx.x * 4 + threadIdx.x] = sh[threadIdx.x][0];
}

// coef = {als_scale, als_min_, tt_scale, tt_min_} as doubles (the tt pair is
// the exact f32 values widened when tt_f32).
__global__ void minmax_final_kernel(const double* __restrict__ part, int nparts, int tt_f32,
                                    double* __restrict__ coef, double* __restrict__ out_minmax) {
  if (threadIdx.x != 0) return;
  double amin = DBL_MAX, amax = -DBL_MAX, tmin = DBL_MAX, tmax = -DBL_MAX;
  for (int q = 0; q < nparts; ++q) {
    amin = fmin(amin, part[4 * q + 0]);
    amax = fmax(amax, part[4 * q + 1]);
    tmin = fmin(tmin, part[4 * q + 2]);
    tmax = fmax(tmax, part[4 * q + 3]);
  }
  if (out_minmax) {  // the fitted MinMaxScalers' data_min_ / data_max_ (src/hybrid_system.py:66-67)
    out_minmax[0] = amin;
    out_minmax[1] = amax;
    out_minmax[2] = tmin;
    out_minmax[3] = tmax;
  }
  const double ascale = 1.0 / mm_range(amax - amin);
  coef[0] = ascale;
  coef[1] = 0.0 - amin * ascale;
  if (tt_f32) {
    const float fmin_ = (float)tmin, fmax_ = (float)tmax;
    const float fscale = 1.0f / mm_range(fmax_ - fmin_);
    const float fmin2 = 0.0f - fmin_ * fscale;
    coef[2] = (double)fscale;
    coef[3] = (double)fmin2;
  } else {
    const double tscale = 1.0 / mm_range(tmax - tmin);
    coef[2] = tscale;
    coef[3] = 0.0 - tmin * tscale;
  }
}

// fused = w0*als_norm + w1*tt_norm, f64 (numpy 1.21 scalar promotion: the
// f32 tt_norm element is widened before the multiply — SURVEY App. A.3).
__global__ __launch_bounds__(256) void fuse_kernel(const double* __restrict__ als, const void* __restrict__ tt,
                                                   int tt_f32, int64_t n, const double* __restrict__ coef,
                                                   double w0, double w1, double* __restrict__ fused) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const double an = als[p] * coef[0] + coef[1];
  double tn;
  if (tt_f32) {
    const float x = ((const float*)tt)[p];
    const float y = x * (float)coef[2] + (float)coef[3];
    tn = (double)y;
  } else {
    tn = ((const double*)tt)[p] * coef[2] + coef[3];
  }
  fused[p] = w0 * an + w1 * tn;
}

// --------------------------------------------- batched fusion (K9, rows)
// Per-row min / max of an f32 score matrix (NaN ignored, like np.nanmin):
// out[r] = min, out[n_rows + r] = max (two contiguous halves, so the
// cross-shard reduction is one MIN and one MAX all-reduce). One block per row.
// Per-row min / max (NaN ignored, like fminf). One 1024-thread block per
// row streams it with 16-B loads (rows 16-B aligned) — HBM-bound.
__global__ __launch_bounds__(1024) void rows_minmax_kernel(const float* __restrict__ x, int64_t n, int64_t ld,
                                                           int vec4, float* __restrict__ out) {
  __shared__ float smin[16], smax[16];
  const float* r = x + (int64_t)blockIdx.x * ld;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  int64_t j0 = 0;
  if (vec4) {
    const int64_t n4 = n >> 2;
    const float4* r4 = reinterpret_cast<const float4*>(r);
    for (int64_t j = threadIdx.x; j < n4; j += 1024) {
      const float4 v = r4[j];
      lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
      hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    j0 = n4 << 2;
  }
  for (int64_t j = j0 + threadIdx.x; j < n; j += 1024) {
    lo = fminf(lo, r[j]);
    hi = fmaxf(hi, r[j]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, kWave));
    hi = fmaxf(hi, __shfl_xor(hi, off, kWave));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    smin[w] = lo;
    smax[w] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 16; ++q) {
      lo = fminf(lo, smin[q]);
      hi = fmaxf(hi, smax[q]);
    }
    out[blockIdx.x] = lo;              // mins  [n_rows]
    out[gridDim.x + blockIdx.x] = hi;  // maxes [n_rows]
  }
}

// fused[r][j] = w0 * minmax64(als[r][j]) + w1 * (double)minmax32(tt[r][j]),
// with each row's min/max given (global over every shard of the row): the
// ALS side is min-max scaled in f64 (the reference's als scores are Python
// floats), the two-tower side in f32 (np.float32 scores), then f64 fusion
// with numpy 1.21's scalar promotion — hrec_fuse_topk per row.
__global__ __launch_bounds__(256) void fuse_rows_kernel(const float* __restrict__ als, const float* __restrict__ tt,
                                                        int64_t n, int64_t ld, const float* __restrict__ als_mm,
                                                        const float* __restrict__ tt_mm, double w0, double w1,
                                                        double* __restrict__ fused) {
#pragma clang fp contract(off)
  const int64_t r = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int64_t R = gridDim.y;  // min/max layout: [2][n_rows]
  const HpScale sc = hp_scale(als_mm[r], als_mm[R + r], tt_mm[r], tt_mm[R + r]);
  fused[r * n + j] = hp_fuse(sc, als[r * ld + j], tt[r * ld + j], w0, w1);
}

// fuse_rows_kernel's arithmetic + a stable top-kk (kk <= kFuseK) of each
// segment of kFuseSeg items, without materialising the fused row. One WAVE
// per segment (no block barriers). Each fused f64 becomes an order-preserving
// u64 key (NaN lowest, as `better` ranks it), so every comparison is one
// integer compare; lane l holds items seg0 + 64 e + l (ascending e =
// ascending index, so a strict '>' keeps the earlier item on ties).
//   1. t = the kk-th best of the 64 lane maxima (by each lane's rank among
//      them: broadcast LDS reads, no dependent cross-lane rounds) — a lower
//      bound of the segment's kk-th best, since those kk maxima are kk
//      distinct items;
//   2. items not worse than t are the candidates (ballot-compacted into LDS;
//      typically ~kk of them; more than 64 — heavy ties — falls back to
//      exact rescans);
//   3. each candidate's rank among them (key desc, index asc) is its slot
//      -> [row][seg*kk] (value, index).
constexpr int kFuseK = 8;
#ifndef HREC_FUSE_PER
#define HREC_FUSE_PER 16
#endif
constexpr int kFusePer = HREC_FUSE_PER;  // items per lane per segment
constexpr int kFuseSeg = 64 * kFusePer;

// Lane l's items seg0 + 64 e + l of a segment's two score rows (ar / tr: the
// lane's first item). In a partial segment (nvalid < kFuseSeg) an item past
// the end re-reads the lane's first one; the callers mask it by position.
__device__ __forceinline__ void fuse_segment_load(const float* __restrict__ ar, const float* __restrict__ tr, int lane,
                                                  int nvalid, float (&av)[kFusePer], float (&tv)[kFusePer]) {
  if (nvalid == kFuseSeg) {  // full segment: unconditional loads
#pragma unroll
    for (int e = 0; e < kFusePer; ++e) {
      av[e] = ar[e * 64];
      tv[e] = tr[e * 64];
    }
  } else {
#pragma unroll
    for (int e = 0; e < kFusePer; ++e) {
      const int off = e * 64 + lane < nvalid ? e * 64 : 0;
      av[e] = ar[off];
      tv[e] = tr[off];
    }
  }
}

struct KI {
  uint64_t k;
  int64_t i;  // INT64_MAX: no item
};
__device__ __forceinline__ bool ki_better(const KI& a, const KI& b) {  // a ranks before b
  return a.i != INT64_MAX && (b.i == INT64_MAX || a.k > b.k || (a.k == b.k && a.i < b.i));
}
__device__ __forceinline__ KI wave_best_ki(KI x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    KI y;
    y.k = ((uint64_t)(uint32_t)__shfl_xor((int)(x.k >> 32), off, kWave) << 32) |
          (uint32_t)__shfl_xor((int)x.k, off, kWave);
    y.i = __shfl_xor(x.i, off, kWave);
    if (ki_better(y, x)) x = y;
  }
  return x;
}

// One segment (seg of row r, R rows) on one wave; ck / ce: the wave's 128
// LDS slots ([64, 128): scratch of non-candidates).
template <int KK>
__device__ __forceinline__ void fuse_segment_one(
    int64_t seg, int64_t r, int64_t R, const float* __restrict__ als, const float* __restrict__ tt, int64_t n,
    int64_t ld, int64_t segs, const float* __restrict__ als_mm, const float* __restrict__ tt_mm, double w0, double w1,
    double* __restrict__ cand_v, int64_t* __restrict__ cand_i, uint64_t* __restrict__ ck, int* __restrict__ ce) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const HpScale sc = hp_scale(als_mm[r], als_mm[R + r], tt_mm[r], tt_mm[R + r]);
  const int64_t seg0 = seg * kFuseSeg;
  const int nvalid = (int)((n - seg0) < kFuseSeg ? (n - seg0) : kFuseSeg);  // items of this segment
  uint64_t key[kFusePer];
  float av[kFusePer], tv[kFusePer];
  fuse_segment_load(als + r * ld + seg0 + lane, tt + r * ld + seg0 + lane, lane, nvalid, av, tv);
#pragma unroll
  for (int e = 0; e < kFusePer; ++e) {
    const uint64_t kv = order_key(hp_fuse(sc, av[e], tv[e], w0, w1));
    key[e] = e * 64 + lane < nvalid ? kv : 0;
  }
  const int nmine = nvalid > lane ? (nvalid - lane + 63) >> 6 : 0;  // live items of this lane
  // 1. lane arg-best (strict '>' in ascending e keeps the earliest of equals)
  uint64_t bk = key[0];
  int be = 0;
#pragma unroll
  for (int e = 1; e < kFusePer; ++e) {
    const bool gt = key[e] > bk;
    bk = gt ? key[e] : bk;
    be = gt ? e : be;
  }
  KI t{0, INT64_MAX};
  {
    // t = the min(kk, live lanes)-th best lane maximum, by each lane's RANK
    // among the 64 maxima (one pass of broadcast LDS reads, no dependent
    // cross-lane rounds); in-segment positions order equal keys
    const int mpos = nmine > 0 ? be * 64 + lane : -1;
    ck[64 + lane] = bk;
    ce[64 + lane] = mpos;
    wave_lds_fence();
    int rank = 0;
#pragma unroll 8
    for (int q = 0; q < 64; ++q) {
      const uint64_t ok = ck[64 + q];
      const int op = ce[64 + q];
      rank += (op >= 0 && (mpos < 0 || ok > bk || (ok == bk && op < mpos))) ? 1 : 0;
    }
    const int nvl = __popcll(__ballot(mpos >= 0));
    const int target = (nvl < KK ? nvl : KK) - 1;
    const uint64_t hit = __ballot(mpos >= 0 && rank == target);
    if (hit) {
      const int src = __builtin_ctzll(hit);
      t.k = lane_read(bk, src);
      t.i = seg0 + lane_read(mpos, src);
    }
    wave_lds_fence();
  }
  // 2. candidates: items not worse than t (no t: fewer than kk items, take all)
  int nc = 0;
  bool overflow = false;
#pragma unroll
  for (int e = 0; e < kFusePer; ++e) {
    const int64_t j = seg0 + (int64_t)e * 64 + lane;
    const bool live = e < nmine;
    const bool c = live && (t.i == INT64_MAX || key[e] > t.k || (key[e] == t.k && j <= t.i));
    const uint64_t m = __ballot(c);
    const int cnt = __popcll(m);
    if (nc + cnt > 64) {
      overflow = true;
      break;
    }
    const int below = lanes_below(m);
    const int slot = c ? nc + below : 64 + lane;  // branch-free append
    ck[slot] = key[e];
    ce[slot] = e * 64 + lane;
    nc += cnt;
  }
  const int64_t obase = r * segs * KK + seg * KK;
  if (!overflow) {
    wave_lds_fence();
    // each candidate's rank among the nc candidates = its output slot
    const uint64_t mk = lane < nc ? ck[lane] : 0;
    const int mp = lane < nc ? ce[lane] : 0;
    int rank = 0;
    for (int q = 0; q < nc; ++q) {
      const uint64_t ok = ck[q];
      const int op = ce[q];
      rank += (ok > mk || (ok == mk && op < mp)) ? 1 : 0;
    }
    if (lane < nc && rank < KK) {
      cand_v[obase + rank] = key_value(mk);
      cand_i[obase + rank] = seg0 + mp;
    }
    if (lane >= nc && lane < KK) {  // fewer candidates than kk: empty slots
      cand_v[obase + lane] = key_value(0);
      cand_i[obase + lane] = -1;
    }
    return;
  }
  // heavy ties: exact selection by rescans (the winning lane drops its item)
  uint32_t live_mask = nmine >= 32 ? 0xffffffffu : ((1u << nmine) - 1u);  // kFusePer <= 32
  auto rescan = [&](KI& m2) {
    m2 = KI{0, INT64_MAX};
#pragma unroll
    for (int e = 0; e < kFusePer; ++e) {
      const KI x{key[e], seg0 + (int64_t)e * 64 + lane};
      if (((live_mask >> e) & 1u) && ki_better(x, m2)) m2 = x;
    }
  };
  KI m2;
  rescan(m2);
  for (int q = 0; q < KK; ++q) {
    const KI w = wave_best_ki(m2);
    if (lane == 0) {
      cand_v[obase + q] = key_value(w.k);
      cand_i[obase + q] = w.i == INT64_MAX ? -1 : w.i;
    }
    if (w.i != INT64_MAX && w.i == m2.i) {
      live_mask &= ~(1u << (int)((w.i - seg0) >> 6));
      rescan(m2);
    }
  }
}

template <int KK>
__global__ __launch_bounds__(256) void fuse_segment_topk_kernel(
    const float* __restrict__ als, const float* __restrict__ tt, int64_t n, int64_t ld, int64_t segs,
    const float* __restrict__ als_mm, const float* __restrict__ tt_mm, double w0, double w1,
    double* __restrict__ cand_v, int64_t* __restrict__ cand_i, const int* __restrict__ gate, int* __restrict__ clear) {
  // clear (the sample launch): reset the filter's overflow flag for this call
  if (clear && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *clear = 0;
  if (gate && *gate == 0) return;
  __shared__ uint64_t ck_sh[4][128];
  __shared__ int ce_sh[4][128];
  const int wv = threadIdx.x >> 6;
  // block-stride over the row's segment groups (a gated launch uses one block
  // per row, so skipping it costs a small grid)
  for (int64_t sb = blockIdx.x; sb * 4 < segs; sb += gridDim.x) {
    const int64_t seg = sb * 4 + wv;
    if (seg < segs)
      fuse_segment_one<KK>(seg, blockIdx.y, gridDim.y, als, tt, n, ld, segs, als_mm, tt_mm, w0, w1, cand_v, cand_i,
                           ck_sh[wv], ce_sh[wv]);
  }
}

// Threshold filter for the batched fusion top-k (kk <= kFuseK): the same
// fused f64 keys as fuse_segment_topk_kernel, one wave per segment, but each
// row first takes a threshold key tk = the best of its sample segments'
// kk-th best keys (fuse_segment_topk_kernel over the row's first G segments
// -> samp). Those are kk distinct items of the row, so at least kk items have
// key >= tk and the row's top kk all do. Per item: the fusion, one compare
// and a ballot; the (few) items with key >= tk are compacted into LDS and
// the segment's stable top-kk among them is taken by rank (each candidate
// counts the better ones, a handful of broadcast LDS reads) -> [row][seg*kk]
// like fuse_segment_topk_kernel, and the same merge follows. A segment with
// more than kFuseSlots candidates (heavy ties, or a row whose best items
// cluster) raises *overflow, which gates the exact segment path on the
// device (the sample launch of fuse_segment_topk_kernel resets it first).
constexpr int kFuseSlots = 64;
__global__ __launch_bounds__(256) void fuse_filter_kernel(
    const float* __restrict__ als, const float* __restrict__ tt, int64_t n, int64_t ld, int64_t segs,
    const float* __restrict__ als_mm, const float* __restrict__ tt_mm, double w0, double w1,
    const double* __restrict__ samp, int G, int kk, double* __restrict__ cand_v, int64_t* __restrict__ cand_i,
    int* __restrict__ overflow) {
#pragma clang fp contract(off)
  __shared__ uint64_t ck_sh[4][kFuseSlots];
  __shared__ int ce_sh[4][kFuseSlots];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t seg = (int64_t)blockIdx.x * 4 + wv;
  if (seg >= segs) return;
  const int64_t r = blockIdx.y;
  const int64_t R = gridDim.y;
  uint64_t tk = 0;
  for (int g = 0; g < G; ++g) {
    const uint64_t k = order_key(samp[(r * G + g) * kk + kk - 1]);
    tk = k > tk ? k : tk;
  }
  const HpScale sc = hp_scale(als_mm[r], als_mm[R + r], tt_mm[r], tt_mm[R + r]);
  const int64_t seg0 = seg * kFuseSeg;
  const int nvalid = (int)((n - seg0) < kFuseSeg ? (n - seg0) : kFuseSeg);
  float av[kFusePer], tv[kFusePer];
  fuse_segment_load(als + r * ld + seg0 + lane, tt + r * ld + seg0 + lane, lane, nvalid, av, tv);
  int nc = 0;
#pragma unroll
  for (int e = 0; e < kFusePer; ++e) {
    const uint64_t key = order_key(hp_fuse(sc, av[e], tv[e], w0, w1));
    const bool c = e * 64 + lane < nvalid && key >= tk;
    const uint64_t m = __ballot(c);
    if (m == 0) continue;  // wave-uniform
    const int below = lanes_below(m);
    const int slot = nc + below;
    if (c && slot < kFuseSlots) {
      ck_sh[wv][slot] = key;
      ce_sh[wv][slot] = e * 64 + lane;
    }
    nc += __popcll(m);
  }
  if (nc > kFuseSlots) {
    if (lane == 0) *overflow = 1;
    return;
  }
  wave_lds_fence();
  // each candidate's rank among the nc (key desc, position asc) = its slot
  const uint64_t mk = lane < nc ? ck_sh[wv][lane] : 0;
  const int mp = lane < nc ? ce_sh[wv][lane] : 0;
  int rank = 0;
  for (int q = 0; q < nc; ++q) {
    const uint64_t ok = ck_sh[wv][q];
    const int op = ce_sh[wv][q];
    rank += (ok > mk || (ok == mk && op < mp)) ? 1 : 0;
  }
  const int64_t obase = (r * segs + seg) * kk;
  if (lane < nc && rank < kk) {
    cand_v[obase + rank] = key_value(mk);
    cand_i[obase + rank] = seg0 + mp;
  }
  if (lane >= nc && lane < kk) {  // fewer candidates than kk: empty slots
    cand_v[obase + lane] = key_value(0);
    cand_i[obase + lane] = -1;
  }
}

}  // namespace hrec

using namespace hrec;

static constexpr int kMinmaxParts = 256;

// Workspace of hrec_fuse_topk, in carve order.
struct FuseWs {
  double* part;   // [kMinmaxParts][4] partial min / max
  double* coef;   // [4] scaler coefficients
  double* fused;  // [n] (unused when the caller takes the fused scores)
  char* tws;      // top-k workspace
  size_t total;
};

static FuseWs fuse_layout(void* base, int64_t n, int top_k) {
  FuseWs w{};
  Carver c(base);
  const int64_t kk = top_k < n ? top_k : n;
  w.part = (double*)c.take((size_t)kMinmaxParts * 4 * 8);
  w.coef = (double*)c.take(4 * 8);
  w.fused = (double*)c.take((size_t)n * 8);
  w.tws = c.take(kk > kTopkSelectMax ? sort_topk_ws_bytes(1, n) : topk_ws_bytes(1, n, (int)kk, 8));
  w.total = c.total();
  return w;
}

extern "C" size_t hrec_fuse_workspace_bytes(int64_t n, int top_k) {
  return fuse_layout(nullptr, n > 0 ? n : 0, top_k).total;
}

extern "C" int hrec_fuse_topk(const double* als, const void* tt, int tt_is_f32, int64_t n, int als_wins,
                              int top_k, int64_t* out_idx, double* out_score, double* out_fused,
                              double* out_minmax, void* workspace, size_t workspace_bytes, void* stream) {
  HREC_REQUIRE(n >= 0, "fuse_topk: negative n");
  HREC_REQUIRE(top_k >= 0, "fuse_topk: top_k must be >= 0");
  if (n == 0) return HREC_OK;
  HREC_REQUIRE(als && tt, "fuse_topk: null input");
  HREC_REQUIRE(top_k == 0 || (out_idx && out_score), "fuse_topk: null output");
  const size_t need = hrec_fuse_workspace_bytes(n, top_k);
  HREC_REQUIRE(workspace && workspace_bytes >= need, "fuse_topk: workspace %zu < %zu", workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const FuseWs w = fuse_layout(workspace, n, top_k);
  double* part = w.part;
  double* coef = w.coef;
  double* fused = out_fused ? out_fused : w.fused;
  char* tws = w.tws;
  const size_t tws_bytes = workspace_bytes - (size_t)(w.tws - (char*)workspace);
  const int parts = (int)((n + 255) / 256 < kMinmaxParts ? (n + 255) / 256 : kMinmaxParts);
  hipLaunchKernelGGL(minmax_partial_kernel, dim3(parts), dim3(256), 0, s, als, tt, tt_is_f32, n, part);
  int rc = check_launch("minmax_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(64), 0, s, part, parts, tt_is_f32, coef,
                     out_minmax);
  rc = check_launch("minmax_final_kernel");
  if (rc) return rc;
  // src/hybrid_system.py:69 — strict '>' picks (0.8, 0.2), else (0.2, 0.8).
  const double w0 = als_wins ? 0.8 : 0.2, w1 = als_wins ? 0.2 : 0.8;
  hipLaunchKernelGGL(fuse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, als, tt, tt_is_f32, n,
                     coef, w0, w1, fused);
  rc = check_launch("fuse_kernel");
  if (rc || top_k == 0) return rc;
  const int kk = (int)(top_k < n ? top_k : n);
  if (kk > kTopkSelectMax) return sort_topk_rows<double>(fused, 1, n, n, kk, out_idx, out_score, tws, tws_bytes, s);
  rc = topk_rows<double>(fused, 1, n, n, kk, out_idx, out_score, tws, tws_bytes, s);
  return rc;
}

extern "C" int hrec_rows_minmax_f32(const float* x, int64_t n_rows, int64_t n, int64_t ld, float* out, void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 0 && ld >= n, "rows_minmax: bad shape");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(n_rows < (1ll << 31), "rows_minmax: too many rows");
  HREC_REQUIRE(x && out, "rows_minmax: null pointer");
  const int vec4 = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  hipLaunchKernelGGL(rows_minmax_kernel, dim3((unsigned)n_rows), dim3(1024), 0, as_stream(stream), x, n, ld, vec4,
                     out);
  return check_launch("rows_minmax_kernel");
}

// Threshold-filter path (kk <= kFuseK): sample segments per row
static int64_t fuse_sample_segs(int64_t n, int /*kk*/) {
  // ~kk / G expected candidates per segment (the bound is the best of G
  // segments' kk-th best) against kFuseSlots
  const int64_t segs = (n + kFuseSeg - 1) / kFuseSeg;
  return segs < 4 ? segs : 4;
}
// One segment pass's candidates ([n_rows][segs * kk] values / indices) and
// the workspace of their top-k, in carve order.
struct SegWs {
  double* v;
  int64_t* i;
  char* tws;
};
static SegWs seg_take(Carver& c, int64_t n_rows, int64_t segs, int kk) {
  SegWs w;
  w.v = (double*)c.take((size_t)n_rows * segs * kk * 8);
  w.i = (int64_t*)c.take((size_t)n_rows * segs * kk * 8);
  w.tws = c.take(topk_ws_bytes(n_rows, segs * kk, kk, 8));
  return w;
}

// Workspace of hrec_fuse_rows_topk, in carve order: the threshold-filter
// path (kk <= kFuseK) or the materialised fused rows.
struct FuseRowsWs {
  double* sv;   // [n_rows][G * kk] the sample segments' top-kk
  int64_t* si;
  int* over;    // the filter's overflow flag
  SegWs filt;   // the filter's candidates
  SegWs exact;  // the gated exact path (fuse_rows_exact)
  double* fused;  // kk > kFuseK: [n_rows][n]
  char* tws;
  size_t total;
};
static FuseRowsWs fuse_rows_layout(void* base, int64_t n_rows, int64_t n, int kk) {
  FuseRowsWs w{};
  Carver c(base);
  if (kk >= 1 && kk <= kFuseK) {
    const int64_t segs = (n + kFuseSeg - 1) / kFuseSeg, G = fuse_sample_segs(n, kk);
    w.sv = (double*)c.take((size_t)n_rows * G * kk * 8);
    w.si = (int64_t*)c.take((size_t)n_rows * G * kk * 8);
    w.over = (int*)c.take(4);
    w.filt = seg_take(c, n_rows, segs, kk);
    w.exact = seg_take(c, n_rows, segs, kk);
  } else {
    w.fused = (double*)c.take((size_t)n_rows * n * 8);
    w.tws = c.take(topk_ws_bytes(n_rows, n, kk, 8));
  }
  w.total = c.total();
  return w;
}

extern "C" size_t hrec_fuse_rows_workspace_bytes(int64_t n_rows, int64_t n, int top_k) {
  return fuse_rows_layout(nullptr, n_rows > 0 ? n_rows : 0, n > 0 ? n : 0, (int)(top_k < n ? top_k : n)).total;
}

extern "C" int hrec_fuse_rows_topk(const float* als, const float* tt, int64_t n_rows, int64_t n, int64_t ld,
                                   const float* als_minmax, const float* tt_minmax, int als_wins, int top_k,
                                   int64_t idx_offset, int64_t* out_idx, double* out_val, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 1 && ld >= n, "fuse_rows_topk: bad shape");
  HREC_REQUIRE(n_rows < 65536, "fuse_rows_topk: at most 65535 rows per call");
  HREC_REQUIRE(top_k >= 1 && top_k <= 1024, "fuse_rows_topk: top_k must be in [1, 1024]");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(als && tt && als_minmax && tt_minmax && out_idx && out_val && workspace, "fuse_rows_topk: null pointer");
  const size_t need = hrec_fuse_rows_workspace_bytes(n_rows, n, top_k);
  HREC_REQUIRE(workspace_bytes >= need, "fuse_rows_topk: workspace %zu < %zu", workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const double w0 = als_wins ? 0.8 : 0.2, w1 = als_wins ? 0.2 : 0.8;
  const int kk = (int)(top_k < n ? top_k : n);
  const FuseRowsWs w = fuse_rows_layout(workspace, n_rows, n, kk);
  int rc;
  if (kk <= kFuseK) {
    // 1. sample: the exact top-kk of each row's first G segments
    // 2. filter: every item whose fused key reaches the sample bound -> row list
    // 3. exact keyed top-kk of the lists
    // 4. (gated on overflow) the exact segment path over every segment
    const int64_t segs = (n + kFuseSeg - 1) / kFuseSeg, G = fuse_sample_segs(n, kk);
    const dim3 gs((unsigned)((G + 3) / 4), (unsigned)n_rows);
    switch (kk) {  // also clears the overflow flag
#define HREC_FUSE_K(K)                                                                                              \
  case K:                                                                                                           \
    hipLaunchKernelGGL(fuse_segment_topk_kernel<K>, gs, dim3(256), 0, s, als, tt, n, ld, G, als_minmax, tt_minmax, \
                       w0, w1, w.sv, w.si, nullptr, w.over);                                                        \
    break;
      HREC_FUSE_K(1) HREC_FUSE_K(2) HREC_FUSE_K(3) HREC_FUSE_K(4) HREC_FUSE_K(5) HREC_FUSE_K(6) HREC_FUSE_K(7)
      default : HREC_FUSE_K(8)
#undef HREC_FUSE_K
    }
    rc = check_launch("fuse_segment_topk_kernel (sample)");
    if (rc) return rc;
    const dim3 gf((unsigned)((segs + 3) / 4), (unsigned)n_rows);
    hipLaunchKernelGGL(fuse_filter_kernel, gf, dim3(256), 0, s, als, tt, n, ld, segs, als_minmax, tt_minmax, w0, w1,
                       w.sv, (int)G, kk, w.filt.v, w.filt.i, w.over);
    rc = check_launch("fuse_filter_kernel");
    if (rc) return rc;
    rc = topk_rows<double>(w.filt.v, n_rows, segs * kk, segs * kk, kk, out_idx, out_val, w.filt.tws, (size_t)1 << 62,
                           s, w.filt.i);
    if (rc) return rc;
    // exact path, run only if some row overflowed its list (one block per
    // row: a skipped launch costs a small grid)
    rc = fuse_rows_exact(als, tt, n_rows, n, ld, als_minmax, tt_minmax, w0, w1, kk, out_idx, out_val, w.exact.v, s,
                         w.over);
  } else {
    hipLaunchKernelGGL(fuse_rows_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n_rows), dim3(256), 0, s, als,
                       tt, n, ld, als_minmax, tt_minmax, w0, w1, w.fused);
    rc = check_launch("fuse_rows_kernel");
    if (rc) return rc;
    rc = topk_rows<double>(w.fused, n_rows, n, n, kk, out_idx, out_val, w.tws, (size_t)1 << 62, s);
  }
  if (rc || idx_offset == 0) return rc;
  return offset_ids(out_idx, n_rows * kk, idx_offset, s);
}

namespace hrec {
// The exact segment path of hrec_fuse_rows_topk (kk <= kFuseK), gated on a
// device flag (launches do nothing while *gate == 0): the pruned hybrid
// top-k's fallback (csrc/hybrid_prune.hip). One block per row walks every
// segment; then the keyed top-kk of the segments' candidates.
size_t fuse_rows_exact_ws_bytes(int64_t n_rows, int64_t n, int kk) {
  Carver c(nullptr);
  seg_take(c, n_rows, (n + kFuseSeg - 1) / kFuseSeg, kk);
  return c.total();
}

int fuse_rows_exact(const float* als, const float* tt, int64_t n_rows, int64_t n, int64_t ld, const float* als_mm,
                    const float* tt_mm, double w0, double w1, int kk, int64_t* out_idx, double* out_val, void* ws,
                    hipStream_t s, const int* gate) {
  if (kk < 1 || kk > kFuseK) {
    set_error("fuse_rows_exact: kk must be in [1, %d]", kFuseK);
    return HREC_E_INVALID;
  }
  const int64_t segs = (n + kFuseSeg - 1) / kFuseSeg;
  Carver c(ws);
  const SegWs g = seg_take(c, n_rows, segs, kk);
  const dim3 grid(1, (unsigned)n_rows);
  switch (kk) {
#define HREC_FX(K)                                                                                                  \
  case K:                                                                                                           \
    hipLaunchKernelGGL(fuse_segment_topk_kernel<K>, grid, dim3(256), 0, s, als, tt, n, ld, segs, als_mm, tt_mm, w0, \
                       w1, g.v, g.i, gate, nullptr);                                                                \
    break;
    HREC_FX(1) HREC_FX(2) HREC_FX(3) HREC_FX(4) HREC_FX(5) HREC_FX(6) HREC_FX(7) default : HREC_FX(8)
#undef HREC_FX
  }
  const int rc = check_launch("fuse_segment_topk_kernel (exact, gated)");
  if (rc) return rc;
  return topk_rows<double>(g.v, n_rows, segs * kk, segs * kk, kk, out_idx, out_val, g.tws, (size_t)1 << 62, s, g.i,
                           nullptr, gate);
}
}  // namespace hrec
