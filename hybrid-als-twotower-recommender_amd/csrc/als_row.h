// The row pipeline of the ALS half-sweeps, shared by csrc/als.hip (Cholesky)
// and csrc/als_nonneg.hip (NNLS): gram_row (CSR gather -> f64 MFMA Gramian and
// rhs of one destination row on one wave) and factor_row (factor + solve).
#pragma once
#include <type_traits>

#include "wave.h"  // row_ror, lane_read, wave_lds_fence

// Occupancy target of the half-sweep (waves per SIMD; caps VGPRs at 168 for
// 3) and the pipeline chunk (steps of 4 ratings) per accumulation mode.
#ifndef HREC_ALS_WAVES
#define HREC_ALS_WAVES 2
#endif
#ifndef HREC_ALS_CH0
#define HREC_ALS_CH0 8
#endif
#ifndef HREC_ALS_ABLATE
#define HREC_ALS_ABLATE 0  // timing-only builds: 1 = skip factor+solve, 3 = skip the back substitution, 4 = skip the Gramian
#endif
#ifndef HREC_ALS_SOLVE_UNROLL
#define HREC_ALS_SOLVE_UNROLL 8  // unroll of the two 64-step triangular-solve loops
#endif
#ifndef HREC_ALS_CH1
#define HREC_ALS_CH1 4
#endif
// The kp-64 ring pipeline of gram_row (explicit feedback):
#ifndef HREC_ALS_PF
#define HREC_ALS_PF 8  // gather prefetch distance in steps of 4 ratings
#endif
#ifndef HREC_ALS_PF64
#define HREC_ALS_PF64 4  // prefetch distance of f64-source gathers (steps)
#endif
#ifndef HREC_ALS_ROT1DPP
#define HREC_ALS_ROT1DPP 1  // f32 sources: rotation by 4 by DPP moves of the converted operands (0: rotated load + conversion)
#endif
#ifndef HREC_ALS_ROT1DPP64
#define HREC_ALS_ROT1DPP64 0  // f64 sources: rotation by 4 by DPP moves of the gathered operands (0: rotated loads; 1 measured 41.6 -> 41.9 ms user side, bit-identical)
#endif
#ifndef HREC_ALS_PR
#define HREC_ALS_PR 2  // f64 accumulation: prefetch distance of the rotated loads (steps)
#endif
// The pooled kernel (3 waves per SIMD, <= 168 VGPRs) takes its own gather knobs.
#ifndef HREC_ALS_POOL_PF
#define HREC_ALS_POOL_PF 8  // as HREC_ALS_PF
#endif
#ifndef HREC_ALS_POOL_PF64
#define HREC_ALS_POOL_PF64 4  // as HREC_ALS_PF64
#endif
#ifndef HREC_ALS_POOL_ROT1DPP64
#define HREC_ALS_POOL_ROT1DPP64 1  // as HREC_ALS_ROT1DPP64; 0 keeps 16 more VGPRs of rotated loads in flight and spills in the step loop
#endif

// The step's ds_bpermute addresses (same bits either way):
#ifndef HREC_ALS_BPERM_IMM
#define HREC_ALS_BPERM_IMM 3  // f32 sources: N opaque per-window copies of the lane's base + immediate offsets (0: the 16 sums hoisted into registers)
#endif
#ifndef HREC_ALS_BPERM_IMM64
#define HREC_ALS_BPERM_IMM64 0  // as HREC_ALS_BPERM_IMM, f64 sources (1 and 2 spill inside the pooled kernel's step loop)
#endif
#ifndef HREC_ALS_RATING_CVT
#define HREC_ALS_RATING_CVT 1  // f32 sources: a window's ratings converted to f64 once per lane, both halves permuted (0: permute the f32, convert per step)
#endif
#ifndef HREC_ALS_RATING_CVT64
#define HREC_ALS_RATING_CVT64 1  // as HREC_ALS_RATING_CVT, f64 sources
#endif

namespace hrec {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef hrec_f4 f4;

template <int NT>
struct Vec;
template <>
struct Vec<4> {
  float x[4];
  __device__ static Vec load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    return Vec{{t.x, t.y, t.z, t.w}};
  }
};
template <>
struct Vec<2> {
  float x[2];
  __device__ static Vec load(const float* p) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    return Vec{{t.x, t.y}};
  }
};
template <>
struct Vec<1> {
  float x[1];
  __device__ static Vec load(const float* p) { return Vec{{*p}}; }
};

__device__ __forceinline__ int tri(int i) { return (i * (i + 1)) >> 1; }

// Structured buffer loads (sbuf_load_f4 / _f2 / _f1 of common.h): address =
// base + vindex * stride + voffset, with the hardware range check
// (vindex >= num_records reads as zero).
typedef hrec_rsrc_t i4v;
typedef hrec_f2 f2;

// Four f64 source-factor columns (32 B) of one gathered row: two 16-B
// structured loads (S64 gathers: source factors kept in f64, no conversion).
struct VecD {
  double x[4];
};
__device__ __forceinline__ VecD struct_load_d(i4v rsrc, int vindex, int voffset) {
  const f4 lo = sbuf_load_f4(rsrc, vindex, voffset, 0, 0);
  // soffset adds to the address like voffset (no swizzle; the range check is
  // on vindex alone), as a constant of the instruction: both loads take the
  // same (vindex, voffset) register pair
  const f4 hi = sbuf_load_f4(rsrc, vindex, voffset, 16, 0);
  VecD v;
  v.x[0] = __hiloint2double(__float_as_int(lo.y), __float_as_int(lo.x));
  v.x[1] = __hiloint2double(__float_as_int(lo.w), __float_as_int(lo.z));
  v.x[2] = __hiloint2double(__float_as_int(hi.y), __float_as_int(hi.x));
  v.x[3] = __hiloint2double(__float_as_int(hi.w), __float_as_int(hi.z));
  return v;
}

// Two f64 source-factor columns (16 B).
struct VecD2 {
  double x[2];
};
__device__ __forceinline__ VecD2 struct_load_d2(i4v rsrc, int vindex, int voffset) {
  const f4 t = sbuf_load_f4(rsrc, vindex, voffset, 0, 0);
  VecD2 v;
  v.x[0] = __hiloint2double(__float_as_int(t.y), __float_as_int(t.x));
  v.x[1] = __hiloint2double(__float_as_int(t.w), __float_as_int(t.z));
  return v;
}

template <int NT>
__device__ __forceinline__ Vec<NT> struct_load(i4v rsrc, int vindex, int voffset) {
  Vec<NT> v;
  if constexpr (NT == 4) {
    const f4 t = sbuf_load_f4(rsrc, vindex, voffset, 0, 0);
    v.x[0] = t.x, v.x[1] = t.y, v.x[2] = t.z, v.x[3] = t.w;
  } else if constexpr (NT == 2) {
    const f2 t = sbuf_load_f2(rsrc, vindex, voffset, 0, 0);
    v.x[0] = t.x, v.x[1] = t.y;
  } else {
    v.x[0] = sbuf_load_f1(rsrc, vindex, voffset, 0, 0);
  }
  return v;
}

#ifdef HREC_ALS_STAMPS
// Diagnostic builds only: per-phase cycle sums (s_memtime) over all waves.
__device__ unsigned long long g_als_stamps[8];
#define STAMP(i)                                                                      \
  do {                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                \
    const unsigned long long _t = __builtin_amdgcn_s_memtime();                       \
    __builtin_amdgcn_sched_barrier(0);                                                \
    if (threadIdx.x == 0 && (i) > 0) atomicAdd(&g_als_stamps[(i) > 0 ? (i) - 1 : 0], _t - _stamp_prev); \
    _stamp_prev = _t;                                                                 \
  } while (0)
#define STAMP_DECL unsigned long long _stamp_prev = 0
#else
#define STAMP(i) \
  do {           \
  } while (0)
#define STAMP_DECL
#endif

// v_writelane_b32: `old` with lane `lane` replaced by the wave-uniform `src`
// (this compiler has no builtin for it; declared like the buffer loads of common.h).
__device__ int writelane_i32(int src, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// Per-wave LDS slice of the half-sweep (doubles).
template <int KP>
struct RowLds {
  static constexpr int kUp = KP * (KP + 1) / 2;  // Ut, column-packed
  // Up doubles as the MODE 1 re-layout stage (256); keep colbuf 16-B aligned
  static constexpr int kUpPad = ((kUp > 256 ? kUp : 256) + 1) & ~1;
  static constexpr int kSize = kUpPad + 128 + 3 * KP;
};

// gram_row's `acquire` of a caller that passes its LDS slice itself.
struct NoAcquire {};

// Gramian + rhs of one destination row on one wave (lane = 0..63):
// acc = sum_j v_j v_j^T (tile layout, + n*reg on the diagonal), b -> bsh.
// NT floats per lane (kp = 16*NT), CH steps of 4 nnz per pipeline chunk.
// MODE 0: v_mfma_f64_16x16x4_f64 accumulates the Gramian in f64 (Spark's
//         f64 NormalEquation, any row length).
// MODE 1: v_mfma_f32_16x16x4_f32 (2x the f64 matrix rate) accumulates each
//         chunk of 16 ratings in f32 (an exact f32 fma chain), and the chunk
//         partials are flushed into f64 accumulators — f64 summation across
//         chunks, f32 rounding only inside a chunk.
// IMP: the A-side MFMA operand of a step carries the rating's confidence
// weight c1 = alpha |r| (the K index of both operands is the step's nnz, so
// the products are c1 v v^T), the rhs weight is 1 + c1 for r > 0 and 0
// otherwise, n_pos = #{r > 0} replaces n on the diagonal and YtY is added to
// the tiles before the factorisation. *npos receives n_pos (wave-uniform).
// Implicit rows take the chunked gather loop at every kp (the ring pipeline
// of kp = 64 is left to the explicit kernels, whose code must not change).
// `acquire` (pooled kernel only): called once the ring loop is done, before
// the first LDS write of the row (the staging of the diagonal tiles); returns
// the wave's LDS slice, which replaces stage / bsh. The default, NoAcquire,
// takes both as passed.
template <int NT, int CH, int MODE, bool S64 = false, bool IMP = false, bool POOLED = false,
          typename Acq = NoAcquire>
__device__ __forceinline__ void gram_row(int64_t beg, int64_t end, int lane, const int32_t* __restrict__ indices,
                                         const float* __restrict__ values, const float* __restrict__ src,
                                         int64_t n_src, int k, double reg, d4 (&acc)[NT * (NT + 1) / 2],
                                         double* __restrict__ bsh, double* __restrict__ stage, double alpha = 0.0,
                                         const double* __restrict__ yty = nullptr, int* npos = nullptr,
                                         Acq acquire = Acq()) {
  constexpr bool kAcq = !std::is_same_v<Acq, NoAcquire>;
  static_assert(!kAcq || (NT == 4 && !IMP), "late slice acquisition: the kp-64 ring pipeline only");
  static_assert(!IMP || (MODE == 0 && !S64), "implicit feedback: f64 accumulation of f32 sources only");
  constexpr int KP = 16 * NT;
  constexpr int NPAIR = NT * (NT + 1) / 2;
  constexpr int CHN = 4 * CH;  // nnz per chunk (<= 64)
  const int sub = lane >> 4;  // which nnz of the step this lane loads
  const int col = lane & 15;  // which NT-column group
  const int64_t n = end - beg;
  int n_pos = 0;  // IMP: ratings > 0 (one ballot per window / chunk of ratings)

  STAMP_DECL;
  STAMP(0);
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) acc[p] = d4{0.0, 0.0, 0.0, 0.0};
  if constexpr (HREC_ALS_ABLATE == 4) {  // timing-only: factor/solve without the Gramian (SPD stand-in)
#pragma unroll
    for (int I = 0, p = 0; I < NT; p += NT - I, ++I)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) acc[p][rr] = (sub + 4 * rr == col) ? 1.0 + reg * (double)n : 0.0;
    if constexpr (kAcq) bsh = acquire() + RowLds<KP>::kUpPad + 128 + 2 * KP;
    if (lane < KP) bsh[lane] = 1.0;
    wave_lds_fence();
    return;
  }
  f4 fa[NPAIR];
  double bp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bp[t] = 0.0;

  // Chunk c's (index, rating) pairs live in lanes 0..CHN-1; padding entries
  // point at row 0 (always valid) with a zero mask so no load is predicated.
  auto load_iv = [&](int64_t base, int& ii, float& vv) {
    const int64_t p = base + (lane % CHN);
    const bool ok = (lane < CHN) && (p < end);
    ii = ok ? indices[p] : -1;
    vv = ok ? values[p] : 0.f;
  };
  auto gather = [&](Vec<NT> (&buf)[CH], int ii) {
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      const int idx = __shfl(ii, 4 * s + sub, kWave);
      const int safe = idx < 0 ? 0 : idx;
      Vec<NT> v = Vec<NT>::load(src + (int64_t)safe * KP + NT * col);
#pragma unroll
      for (int t = 0; t < NT; ++t) v.x[t] = idx < 0 ? 0.f : v.x[t];
      buf[s] = v;
    }
  };

  // The ring pipeline for kp = 64 (at kp <= 32 the scheduler hoists the
  // unrolled window into a spill; those sizes keep the chunked loop)
  if constexpr (NT == 4 && !IMP) {
  // Ring pipeline over WINDOWS of 16 steps (64 nnz: one index and one rating
  // per lane). Step s's gather is issued PF steps ahead into ring slot
  // s % PF; the index reaches the lane group by ds_bpermute and feeds a
  // structured buffer load (vindex = source row, stride = one factor row,
  // voffset = this lane's 16-B column slice). Padding entries carry index -1:
  // the buffer range check returns zeros for them, so the loop has no
  // branches, masks or address arithmetic on the VALU.
  // f64 sources sit in the MALL: shorter distance
  constexpr int PF = POOLED ? (S64 ? HREC_ALS_POOL_PF64 : HREC_ALS_POOL_PF) : (S64 ? HREC_ALS_PF64 : HREC_ALS_PF);
  static_assert(16 % PF == 0, "prefetch distance must divide the window");
  static_assert(!S64 || MODE == 0, "f64 sources: kp 64, f64 accumulation only");
  const int voff = (S64 ? 8 : 4) * NT * col;
  const int bp_addr = 4 * sub;  // ds_bpermute byte address of nnz (4s + sub) is 16 s + 4 sub
  const uint64_t sbase = (uint64_t)src;
  i4v rsrc;
  rsrc.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)sbase);
  rsrc.y = __builtin_amdgcn_readfirstlane((int)(uint32_t)(sbase >> 32) | ((KP * (S64 ? 8 : 4)) << 16));
  rsrc.z = __builtin_amdgcn_readfirstlane((int)n_src);
  rsrc.w = 0x00020000;
  auto load_win = [&](int64_t w, int& ii, float& vv) {
    const int64_t p = beg + 64 * w + lane;
    const int64_t pc = p < end ? p : end - 1;
    const int iraw = indices[pc];
    const float vraw = values[pc];
    ii = p < end ? iraw : -1;
    vv = p < end ? vraw : 0.f;
  };
  // bpw[u]: bp_addr, made opaque once per window below, so that the constant
  // part of every step's address stays in the loop and folds into the
  // instruction's offset field (hoisted, the 16 sums are 16 registers or an
  // add per permute). One copy per use in the step — u = 0 the ring index,
  // 1 the rotated loads' index, 2 the rating: a sum shared between two steps
  // would be formed once, in the earlier one, and reach the later in a register.
  constexpr int kBpImm = S64 ? HREC_ALS_BPERM_IMM64 : HREC_ALS_BPERM_IMM;  // copies (0: none, hoisted sums)
  static_assert(kBpImm >= 0 && kBpImm <= 3, "one base per use at the most");
  int bpw[3] = {bp_addr, bp_addr, bp_addr};
  auto bperm = [&](int win, int s, int u = 0) -> int {
    return __builtin_amdgcn_ds_bpermute(bpw[u < kBpImm ? u : (kBpImm > 0 ? kBpImm - 1 : 0)] + 16 * s, win);
  };
  const int64_t nsteps = (n + 3) >> 2;
  int iw0, iw1;
  float rw0, rw1;
  load_win(0, iw0, rw0);
  load_win(1, iw1, rw1);
  using RingT = std::conditional_t<S64, VecD, Vec<NT>>;
  auto ring_load = [&](int vi) -> RingT {
    if constexpr (S64) return struct_load_d(rsrc, vi, voff);
    else return struct_load<NT>(rsrc, vi, voff);
  };
  RingT ring[PF];
#pragma unroll
  for (int s = 0; s < PF; ++s) ring[s] = ring_load(bperm(iw0, s));
  int nidx = bperm(iw0, PF);  // source row of the next gather (one step ahead)
  // f64 accumulation (MODE 0) splits the diagonal tiles off the 16x16x4
  // MFMAs: a diagonal tile's 16 x 16 block is 16 sub-blocks of 4 x 4, of
  // which 10 are distinct (symmetry). v_mfma_f64_4x4x4_4b runs 4 independent
  // 4 x 4 x 4 blocks at the 16x16x4 rate (16 vs 64 cycles, measured:
  // scripts/micro/mfma_f64_rate.hip); with A = B = the lane's operand it
  // yields the 4 diagonal sub-blocks (b, b), with B rotated by 4 / 8 lanes
  // inside each 16-lane row the sub-blocks (b, b + 1) and (b, b + 2) mod 4:
  // all 10, in 3/4 of the 16x16x4 time.
  // The rotated operands are gathered from memory, PR steps ahead: more
  // structured loads of the same source rows at the column slices of lane
  // col + 4 and col + 8 — no cross-lane moves. (kRot1Dpp: the rotation by 4
  // is two 32-bit DPP moves of the own operand instead of a load.)
  constexpr bool kDiag4 = MODE == 0;
  constexpr int PR = HREC_ALS_PR;  // rotated-load prefetch distance (steps)
  constexpr bool kRot1Dpp = S64 ? (POOLED ? HREC_ALS_POOL_ROT1DPP64 : HREC_ALS_ROT1DPP64) : HREC_ALS_ROT1DPP;
  static_assert(PR < PF, "rotated loads are issued from the current windows");
  const int voff1 = (S64 ? 8 : 4) * NT * ((col + 4) & 15), voff2 = (S64 ? 8 : 4) * NT * ((col + 8) & 15);
  auto rot_load = [&](int vi, int vo) -> RingT {
    if constexpr (S64) return struct_load_d(rsrc, vi, vo);
    else return struct_load<NT>(rsrc, vi, vo);
  };
  // The rotation-by-8 product of a diagonal tile has 2 distinct sub-blocks in
  // its 4 blocks, so two tiles share one v_mfma_f64_4x4x4_4b: blocks 0, 1
  // (lanes with col < 8) take the operands of tile P, blocks 2, 3 those of
  // tile P + 2 (P = 0, 1). The pairs (0, 2) and (1, 3) make the operands
  // adjacent components: lanes col < 8 need components {0, 1}, lanes col >= 8
  // {2, 3} — of the own slice (A) and of the col + 8 slice (B). Two half-width
  // loads at a per-lane offset deliver exactly those, so no lane selects are
  // needed.
  using PairT = std::conditional_t<S64, VecD2, Vec<2>>;
  const int hoff = (lane & 8) ? (S64 ? 16 : 8) : 0;
  auto pair_load = [&](int vi, int vo) -> PairT {
    if constexpr (S64) return struct_load_d2(rsrc, vi, vo);
    else return struct_load<2>(rsrc, vi, vo);
  };
  RingT rot1[PR];
  PairT rotA[PR], rotB[PR];
  if constexpr (kDiag4) {
#pragma unroll
    for (int q = 0; q < PR; ++q) {
      const int vi = bperm(iw0, q);
      if constexpr (!kRot1Dpp) rot1[q] = rot_load(vi, voff1);
      rotA[q] = pair_load(vi, voff + hoff);
      rotB[q] = pair_load(vi, voff2 + hoff);
    }
  }
  // diagonal tile t: dg[t][0] the (b, b) sub-blocks, dg[t][1] the (b, b + 1);
  // dc[P] the shared (b, b + 2) product of tiles P and P + 2. (dg[t][2] is
  // not used. The array keeps the slot, as ar2 below keeps 2 of its 4: with
  // either array smaller the compiler allocates the kernels' registers
  // differently, which would have to be measured.)
  double dg[NT][3], dc[2];
#pragma unroll
  for (int t = 0; t < NT; ++t) dg[t][0] = dg[t][1] = 0.0;
#pragma unroll
  for (int t = 0; t < 2; ++t) dc[t] = 0.0;
  for (int64_t w = 0;; ++w) {
    int iw2;
    float rw2;
    load_win(w + 2, iw2, rw2);
    if constexpr (kBpImm == 3) asm volatile("" : "+v"(bpw[0]), "+v"(bpw[1]), "+v"(bpw[2]));
    else if constexpr (kBpImm == 2) asm volatile("" : "+v"(bpw[0]), "+v"(bpw[1]));
    else if constexpr (kBpImm == 1) asm volatile("" : "+v"(bpw[0]));
    // kRatCvt: the current window's ratings as f64, converted here once per
    // lane (exact for every float); a step then permutes the two halves
    constexpr bool kRatCvt = (S64 ? HREC_ALS_RATING_CVT64 : HREC_ALS_RATING_CVT) != 0;
    const long long rd0 = __double_as_longlong((double)rw0);
    bool stop = false;
    const int rem = __builtin_amdgcn_readfirstlane((int)(nsteps - 16 * w < 16 ? nsteps - 16 * w : 16));
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s >= rem) {  // wave-uniform (scalar) tail exit
        stop = true;
        break;
      }
      const RingT cur = ring[s % PF];
      // a: the own operands; ar1: rotated by 4 lanes; apair[P] / ar2[P]: the
      // A / B operands of the shared rotation-by-8 product P (P = 0, 1)
      double a[NT], ar1[NT], ar2[NT], apair[2];
#pragma unroll
      for (int t = 0; t < NT; ++t) a[t] = (double)cur.x[t];
      ring[s % PF] = ring_load(nidx);
      if constexpr (kDiag4) {
#pragma unroll
        for (int t = 0; t < NT; ++t) ar1[t] = kRot1Dpp ? row_ror<12>(a[t]) : (double)rot1[s % PR].x[t];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          apair[t] = (double)rotA[s % PR].x[t];
          ar2[t] = (double)rotB[s % PR].x[t];
        }
        const int vr = (s + PR < 16) ? bperm(iw0, s + PR, 1) : bperm(iw1, s + PR - 16, 1);
        if constexpr (!kRot1Dpp) rot1[s % PR] = rot_load(vr, voff1);
        rotA[s % PR] = pair_load(vr, voff + hoff);
        rotB[s % PR] = pair_load(vr, voff2 + hoff);
      }
      nidx = (s + 1 + PF < 16) ? bperm(iw0, s + 1 + PF) : bperm(iw1, s + 1 + PF - 16);
      double rv;
      if constexpr (kRatCvt) {
        rv = __hiloint2double(bperm((int)(rd0 >> 32), s, 2), bperm((int)rd0, s, 2));
      } else {
        rv = (double)__int_as_float(bperm(__float_as_int(rw0), s, 2));
      }
      if (MODE == 1 && (s % HREC_ALS_CH1) == 0) {
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) fa[p] = f4{0.f, 0.f, 0.f, 0.f};
      }
      int p = 0;
#pragma unroll
      for (int I = 0; I < NT; ++I) {
#pragma unroll
        for (int J = I; J < NT; ++J) {
          if (MODE == 0) {
            if (I == J) {
              dg[I][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[I], a[I], dg[I][0], 0, 0, 0);
              dg[I][1] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[I], ar1[I], dg[I][1], 0, 0, 0);
              // tiles I and I + 2
              if (I < 2) dc[I] = __builtin_amdgcn_mfma_f64_4x4x4f64(apair[I], ar2[I], dc[I], 0, 0, 0);
            } else {
              acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[I], a[J], acc[p], 0, 0, 0);
            }
          } else {
            fa[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.x[I], cur.x[J], fa[p], 0, 0, 0);
          }
          ++p;
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) bp[t] = fma(rv, a[t], bp[t]);
      if (MODE == 1 && ((s % HREC_ALS_CH1) == HREC_ALS_CH1 - 1 || s + 1 == rem)) {
#pragma unroll
        for (int p2 = 0; p2 < NPAIR; ++p2) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) acc[p2][rr] += (double)fa[p2][rr];
        }
      }
    }
    if (stop || 16 * (w + 1) >= nsteps) break;
    iw0 = iw1;
    rw0 = rw1;
    iw1 = iw2;
    rw1 = rw2;
  }
  if constexpr (kAcq) {
    double* base = acquire();
    stage = base;
    bsh = base + RowLds<KP>::kUpPad + 128 + 2 * KP;
  }
  if constexpr (kDiag4) {
    // 4x4x4 block C[i][j] of block q sits at lane 16 i + 4 q + j and holds
    // G[4q + i][4((q + s) & 3) + j] for rotation s; write it and its mirror
    // into a 16 x 16 LDS image, read back the 16x16x4 C layout (one pass per
    // diagonal tile and row)
    const int i4 = lane >> 4, q4 = (lane >> 2) & 3, j4 = lane & 3;
#pragma unroll
    for (int I = 0, p = 0; I < NT; p += NT - I, ++I) {
#pragma unroll
      for (int sh = 0; sh < 3; ++sh) {
        const int r = 4 * q4 + i4, c = 4 * ((q4 + sh) & 3) + j4;
        if (sh == 2) {  // this tile's blocks of the shared product (with their mirrors: all 4)
          // the other tile's lanes write the same values to the junk slots 256, 257
          const bool mine = (q4 >= 2) == (I >= 2);
          const double v = dc[I & 1];
          stage[mine ? r * 16 + c : 256] = v;
          stage[mine ? c * 16 + r : 257] = v;
          continue;
        }
        stage[r * 16 + c] = dg[I][sh];
        stage[c * 16 + r] = dg[I][sh];
      }
      wave_lds_fence();
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) acc[p][rr] = stage[(sub + 4 * rr) * 16 + col];
      wave_lds_fence();
    }
  }
  } else {
  int i0, i1;
  float r0, r1;
  load_iv(beg, i0, r0);
  load_iv(beg + CHN, i1, r1);
  Vec<NT> buf[CH];
  gather(buf, i0);

  for (int64_t base = beg; base < end; base += CHN) {
    Vec<NT> nbuf[CH];
    const bool more = base + CHN < end;
    if (more) gather(nbuf, i1);
    int i2;
    float r2;
    load_iv(base + 2 * CHN, i2, r2);
    if constexpr (IMP) n_pos += __builtin_popcountll(__ballot(r0 > 0.f));
    if (MODE == 1) {
#pragma unroll
      for (int p = 0; p < NPAIR; ++p) fa[p] = f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      const double rv = (double)__shfl(r0, 4 * s + sub, kWave);
      double a[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) a[t] = (double)buf[s].x[t];
      double aw[NT], bw = rv;
      if constexpr (IMP) {
        const double c1 = alpha * fabs(rv);
        bw = rv > 0.0 ? 1.0 + c1 : 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) aw[t] = c1 * a[t];
      }
      auto lhs = [&](int t) -> double {
        if constexpr (IMP) return aw[t];
        else return a[t];
      };
      int p = 0;
#pragma unroll
      for (int I = 0; I < NT; ++I) {
#pragma unroll
        for (int J = I; J < NT; ++J) {
          if (MODE == 0)
            acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(lhs(I), a[J], acc[p], 0, 0, 0);
          else
            fa[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(buf[s].x[I], buf[s].x[J], fa[p], 0, 0, 0);
          ++p;
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) bp[t] = fma(bw, a[t], bp[t]);
    }
    if (MODE == 1) {
#pragma unroll
      for (int p = 0; p < NPAIR; ++p) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[p][rr] += (double)fa[p][rr];
      }
    }
    if (more) {
#pragma unroll
      for (int s = 0; s < CH; ++s) buf[s] = nbuf[s];
    }
    i0 = i1;
    r0 = r1;
    i1 = i2;
    r1 = r2;
  }
  }

  STAMP(1);  // phase 1: Gramian (gather + MFMA)
  // b: sum the four row-groups of lanes.
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    bp[t] += __shfl_xor(bp[t], 16, kWave);
    bp[t] += __shfl_xor(bp[t], 32, kWave);
  }
  // ---- blocked Cholesky in the matrix-core tile layout -------------------
  // Work in the permuted basis q = 16*T + m  <->  physical column NT*m + T:
  // tile (I,J) of the accumulators is then block (I,J) of the permuted
  // Gramian (rows of block I, columns of block J, I <= J: the upper block
  // triangle). A symmetric permutation does not change the solution; b and
  // x are permuted on the way in and out. Factor A = U^T U block row by
  // block row: a 16-pivot panel step with one LANE PER COLUMN (compact,
  // fully in registers), then the trailing update of every later block
  // U_KM -= U_JK^T U_JM on the f64 matrix cores, straight from the
  // accumulator registers (the C/D layout of tile (J,K) is exactly the A/B
  // operand layout of the 4 k-steps).
  if (sub == 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) bsh[16 * t + col] = bp[t];  // permuted b
  }
  if (MODE == 1) {
    // f32 C/D map (row = 4*(lane>>4) + reg) -> f64 map (row = (lane>>4) + 4*reg)
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) stage[(4 * sub + rr) * 16 + col] = acc[p][rr];
      wave_lds_fence();
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) acc[p][rr] = stage[(sub + 4 * rr) * 16 + col];
      wave_lds_fence();
    }
  }
  STAMP(2);  // phase 2: b + layout
  if constexpr (IMP) {
    // + YtY: tile (I, J) register rr holds G[NT * (sub + 4 rr) + I][NT * col + J]
    int p = 0;
#pragma unroll
    for (int I = 0; I < NT; ++I) {
#pragma unroll
      for (int J = I; J < NT; ++J) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[p][rr] += yty[(NT * (sub + 4 * rr) + I) * KP + NT * col + J];
        ++p;
      }
    }
    *npos = n_pos;
  }
  // lambda = numExplicits * regParam on the diagonal (1.0 on padding columns)
  const double lambda = (double)(IMP ? (int64_t)n_pos : n) * reg;
  {
    int p = 0;
#pragma unroll
    for (int I = 0; I < NT; ++I) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        if (sub + 4 * rr == col) acc[p][rr] += (NT * col + I < k) ? lambda : 1.0;
      }
      p += NT - I;
    }
  }
}

// Factor + solve of one row's normal equations on one wave: acc (tile layout,
// consumed), b in bsh; Ut in Up (KP(KP+1)/2), row buffers and pivots in
// scratch (128 + 2 KP); x -> out[0..KP).
// LDSG (factor_row_lds): the Gramian leaves the accumulator registers at once
// — all tiles go to Up, in the layout step (a) writes — and every trailing
// tile is loaded from Up, updated by the same 4 MFMAs in the same order and
// stored back (q <= c; the lower halves of diagonal tiles are never read, so
// what gets loaded for them does not matter). Same operations on the same
// values as the register form: the same bits, in 80 fewer live VGPRs.
template <int NT, bool LDSG>
__device__ __forceinline__ void factor_row_impl(int lane, d4 (&acc)[NT * (NT + 1) / 2], double* __restrict__ Up,
                                           double* __restrict__ scratch, const double* __restrict__ bsh,
                                           float* __restrict__ out) {
  constexpr int KP = 16 * NT;
  constexpr int NPAIR = NT * (NT + 1) / 2;
  double* __restrict__ colbuf = scratch;    // two 64-entry row buffers (16-B aligned)
  double* __restrict__ dsh = colbuf + 128;  // pivots d_r (the KP doubles behind them are not used)
  const int sub = lane >> 4, col = lane & 15;
  // kp 64: every lane of the wave owns a column, so the tests against KP are
  // true at compile time (a caller may pass a lane the compiler cannot bound)
  constexpr bool kFull = KP == 64;
  const bool incol = kFull || lane < KP;
  STAMP_DECL;
  STAMP(0);
  if constexpr (HREC_ALS_ABLATE == 1) {  // timing-only: Gramian without factor/solve
    double sum = 0.0;
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) sum += acc[p][0] + acc[p][1] + acc[p][2] + acc[p][3];
    wave_lds_fence();
    if (lane < KP) out[lane] = (float)(sum + bsh[lane]);
    return;
  }
  // A = Ut^T D Ut with Ut unit upper triangular, stored column-packed in LDS
  // (Ut[tri(c) + r], r <= c), pivots d_r in dsh (and on lane r). A x = b is
  //   Ut^T w = b,  v = D^-1 w,  Ut x = v
  // and each of the 2 x KP substitution steps is one broadcast + one masked fma.
  // (Spark's dppsv factors A = U^T U with U = D^1/2 Ut: the same solution.)
  auto pidx = [](int I, int K) { return I * NT - (I * (I - 1)) / 2 + (K - I); };
  // The forward substitution Ut^T w = b rides along the panels: at pivot pv
  // lane c > pv holds Ut[pv][c] (= ut) and w_pv is lane pv's b, final since
  // pivot pv - 1, so b_c -= Ut[pv][c] w_pv is one broadcast + one fma off the
  // panel's critical chain — the same operands in the same (pv ascending)
  // order as a separate substitution loop, so the same bits.
  double bs = 0.0;
  // dcap: lane pv's copy of its pivot d_pv (every pivot is wave-uniform, so a
  // v_writelane puts it there without a lane test or a branch); a panel's 16
  // go to dsh in one store after the panel — dq[] below is their first reader
  double dcap = 0.0;
#pragma unroll
  for (int J = 0; J < NT; ++J) {
    // (a) block row J -> LDS (only q <= c: the upper triangle); LDSG: every
    //     block row, once
    if (!LDSG || J == 0) {
#pragma unroll
      for (int I = J; I < (LDSG ? NT : J + 1); ++I) {
#pragma unroll
        for (int K = I; K < NT; ++K) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int q = 16 * I + sub + 4 * rr, c = 16 * K + col;
            if (q <= c) Up[tri(c) + q] = acc[pidx(I, K)][rr];
          }
        }
      }
      wave_lds_fence();
    }
    if (J == 0) bs = incol ? bsh[lane] : 0.0;
    // (b) lane c >= 16J owns column c of block row J
    const int c = lane;
    const bool own = c >= 16 * J && incol;
    double a[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int q = 16 * J + m;
      a[m] = (own && q <= c) ? Up[tri(c) + q] : 0.0;
    }
    // (c) 16 pivots of A = Ut^T D Ut (LDL^T: no square roots), right-looking,
    //     columns on lanes. The unscaled pivot row goes to LDS (alternating
    //     buffers) and comes back as wave-uniform ds_read_b128 pairs; the next
    //     pivot is formed on its own lane ahead of that round trip (its update
    //     needs only the lane's own entries), so the per-pivot critical path is
    //     rcp -> Newton -> scale -> fma -> readlane.
    double piv = lane_read(a[0], 16 * J);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int pv = 16 * J + i;
      double* cb = colbuf + 64 * (i & 1);
      if (incol) cb[c] = a[i];  // A[pv][c] (lane pv: the pivot)
      // 1 / piv: v_rcp_f64 (~2^-24 relative) + one Newton step
      const double r0 = __builtin_amdgcn_rcp(piv);
      const double r = fma(r0, fma(-piv, r0, 1.0), r0);
      const double ut = a[i] * r;  // Ut[pv][c]
      if (own && c > pv) Up[tri(c) + pv] = ut;
      {
        const long long pb = __double_as_longlong(piv), db = __double_as_longlong(dcap);
        const int lo = writelane_i32((int)pb, pv, (int)db);
        const int hi = writelane_i32((int)(pb >> 32), pv, (int)(db >> 32));
        dcap = __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
      }
      {
        const double wq = lane_read(bs, pv);
        if (own && c > pv) bs = fma(-ut, wq, bs);
      }
      if (i < 15) {
        piv = lane_read(fma(-a[i], ut, a[i + 1]), pv + 1);
        wave_lds_fence();
#pragma unroll
        for (int m0 = (i + 1) & ~1; m0 < 16; m0 += 2) {
          const double2 u = *reinterpret_cast<const double2*>(cb + 16 * J + m0);
          if (m0 > i) a[m0] = fma(-u.x, ut, a[m0]);
          a[m0 + 1] = fma(-u.y, ut, a[m0 + 1]);
        }
      }
    }
    if (own) dsh[c] = dcap;  // lanes of later panels: 0.0, replaced after their own panel
    wave_lds_fence();
    // (e) Ut_JK (K > J) back into tile registers, with a D_J-scaled copy;
    // (f) trailing update A_KM -= Ut_JK^T D_J Ut_JM on the f64 matrix cores
    if (J + 1 < NT) {
      double dq[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) dq[rr] = dsh[16 * J + sub + 4 * rr];
      d4 yv[NT];
#pragma unroll
      for (int K = J + 1; K < NT; ++K) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const double x = Up[tri(16 * K + col) + 16 * J + sub + 4 * rr];
          acc[pidx(J, K)][rr] = x;
          yv[K][rr] = x * dq[rr];
        }
      }
#pragma unroll
      for (int K = J + 1; K < NT; ++K) {
#pragma unroll
        for (int M = K; M < NT; ++M) {
          if constexpr (LDSG) {
            // q > c of a diagonal tile reads past its column, still inside Up
            // (tri(c) + q <= tri(KP - 2) + KP - 1 < kUp), and is not stored
            d4 t;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) t[rr] = Up[tri(16 * M + col) + 16 * K + sub + 4 * rr];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
              t = __builtin_amdgcn_mfma_f64_16x16x4f64(-acc[pidx(J, K)][rr], yv[M][rr], t, 0, 0, 0);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const int q = 16 * K + sub + 4 * rr, c = 16 * M + col;
              if (q <= c) Up[tri(c) + q] = t[rr];
            }
          } else {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
              acc[pidx(K, M)] = __builtin_amdgcn_mfma_f64_16x16x4f64(-acc[pidx(J, K)][rr], yv[M][rr],
                                                                      acc[pidx(K, M)], 0, 0, 0);
          }
        }
      }
      if constexpr (LDSG) wave_lds_fence();  // the next panel reads what other lanes stored
    }
  }
  STAMP(3);  // phase 3: factorisation
  // 1 / d_lane: the pivot loop's r, formed again by the same two steps on the
  // same value (lanes >= KP: not used)
  const double rd0 = __builtin_amdgcn_rcp(dcap);
  const double myrd = fma(rd0, fma(-dcap, rd0, 1.0), rd0);
  if constexpr (HREC_ALS_ABLATE == 3) {  // timing-only: factor without the substitutions
    if (lane < KP) out[lane] = (float)(myrd + Up[tri(lane)]);
    return;
  }
  double bi = bs * myrd;  // v = D^-1 w (w from the panels)
  // back     Ut x = v     (step q: lanes c < q subtract Ut[c][q] * x_q)
#pragma unroll HREC_ALS_SOLVE_UNROLL
  for (int q = KP - 1; q >= 0; --q) {
    const double u = Up[tri(q) + (incol ? lane : 0)];  // Ut[lane][q] for lane < q
    const double xq = lane_read(bi, q);
    if (lane < q) bi = fma(-u, xq, bi);
  }
  STAMP(4);  // phase 4: triangular solves
  if (incol) out[NT * (lane & 15) + (lane >> 4)] = (float)bi;
  wave_lds_fence();  // the next row on this wave reuses the LDS slice
}

template <int NT>
__device__ __forceinline__ void factor_row(int lane, d4 (&acc)[NT * (NT + 1) / 2], double* __restrict__ Up,
                                           double* __restrict__ scratch, const double* __restrict__ bsh,
                                           float* __restrict__ out) {
  factor_row_impl<NT, false>(lane, acc, Up, scratch, bsh, out);
}

template <int NT>
__device__ __forceinline__ void factor_row_lds(int lane, d4 (&acc)[NT * (NT + 1) / 2], double* __restrict__ Up,
                                               double* __restrict__ scratch, const double* __restrict__ bsh,
                                               float* __restrict__ out) {
  factor_row_impl<NT, true>(lane, acc, Up, scratch, bsh, out);
}

}  // namespace hrec
