// The position of every held-out item among all candidates
// (hrec_rank_positions): for each label entry of a row, how many live columns
// stand before it in the list order better() (csrc/order.h) — the
// 0-based position the item would have in a top-n list of length n — and from
// those positions the row's AUC, reciprocal rank and percentile-rank sums.
// include/hrec.h has the contract.
//
// Shape: a few (up to thousands of) labels against a row of up to 10^5 scores
// that is read once: memory-bound on the score row. One workgroup of 256 owns
// a row:
//   1. the row's exclusion segment is counted (excl_counts) -> live;
//   2. per chunk of kRpChunk label entries: each entry is keyed by (order_key
//      of its value, column), entries that cannot be ranked (column outside
//      [0, n), or excluded: excl_contains) become sentinels that sort last;
//      a bitonic sort puts the chunk into list order in LDS;
//   3. the row is streamed with 16-byte non-temporal loads (a scalar head and
//      tail around the aligned body, the next vector in flight); a column
//      that stands after the chunk's last entry is done after one compare,
//      every other does one branch-free binary search over the chunk's keys
//      (the number of entries it does not precede) and one LDS counter
//      increment. The f32 source packs the value's 32-bit key and the column
//      into one 64-bit key, so a probe is one LDS read and one compare;
//   4. the excluded columns, which the stream counted like any other, are
//      taken out again by the same search (one decrement each);
//   5. an inclusive prefix sum over the counters is the rank of each sorted
//      entry; ranks go out by entry, and into the row's integer sums once per
//      distinct column (a duplicate is adjacent in the sorted chunk, or found
//      by searching the columns of earlier chunks);
//   6. the weighted percentile ranks are added per thread over the entries it
//      owns in CSR order, then over the threads in a fixed tree.
// A row with more labels than a chunk repeats 2-6 (and the stream) per chunk.
// The sums over rows: rp_partial_kernel adds blocks of 256 rows in a fixed
// order into the workspace, rp_reduce_kernel adds the partials (no
// floating-point atomics): equal inputs give equal bits.
#include <type_traits>

#include "exclusion.h"
#include "hybrid_common.h"
#include "um_score.h"

#pragma clang fp contract(off)

namespace hrec {

constexpr int kRpChunk = HREC_RP_CHUNK;
constexpr int kRpBlock = 256;
constexpr int kRpSums = HREC_RP_SUMS;
constexpr int32_t kRpNoCol = INT32_MAX;  // a sentinel's column: after every real column of its key
static_assert(kRpChunk % kRpBlock == 0 && (kRpChunk & (kRpChunk - 1)) == 0, "a power of two, whole strides");

typedef double rp_d2 __attribute__((ext_vector_type(2)));

struct RpParams : UmSource {
  int64_t n_rows, n;
  const double* minmax;
  const int32_t* wins;
  const int64_t* lrows;
  const int64_t* lindptr;
  const int32_t* lcols;
  const double* lweight;
  const int64_t* xrows;
  const int64_t* xindptr;
  const int32_t* xcols;
  int32_t* out_rank;
  double* out_row;
  int32_t* out_row_n;
};

struct RpLds {
  uint64_t key[kRpChunk];  // sorted: list order, sentinels last
  int32_t col[kRpChunk];
  int32_t idx[kRpChunk];   // the entry's offset in the chunk (-1: sentinel)
  int32_t cnt[kRpChunk + 1];
  int32_t rank[kRpChunk];  // by entry offset (-1: unranked)
  uint8_t dup[kRpChunk];   // by sorted position: the column was counted already
  int64_t red_i[kRpBlock / kWave][4];
  double red_d[kRpBlock / kWave][2];
  int32_t scan[kRpBlock / kWave];
};

// (ka, ca) stands before (kb, cb) in the list order
__device__ __forceinline__ bool rp_before(uint64_t ka, int32_t ca, uint64_t kb, int32_t cb) {
  return ka > kb || (ka == kb && ca < cb);
}

// The packed key of the f32 source: the value's 32-bit key above the
// complemented column, so one unsigned compare is the list order (a larger
// key stands first) and equal keys are equal columns; above 0, the sentinel's.
__device__ __forceinline__ uint64_t rp_packed_key(float v, int64_t c) {
  return ((uint64_t)order_key32(v) << 32) | (uint32_t)(0xffffffffu - (uint32_t)c);
}

// The number of sorted entries e (of P, a power of two >= 2) with
// e before (k, c) [STRICT] or e before-or-equal (k, c) [!STRICT]: a prefix.
// PACKED: the keys are rp_packed_key's and decide alone.
template <bool STRICT, bool PACKED>
__device__ __forceinline__ int rp_search(const RpLds& L, int P, uint64_t k, int32_t c) {
  auto pred = [&](int i) {
    const uint64_t ek = L.key[i];
    if constexpr (PACKED) {
      return STRICT ? ek > k : ek >= k;
    } else {
      const int32_t ec = L.col[i];
      return ek > k || (ek == k && (STRICT ? ec < c : ec <= c));
    }
  };
  int pos = 0;
  for (int step = P >> 1; step > 0; step >>= 1) pos += pred(pos + step - 1) ? step : 0;
  return pos + (pred(pos) ? 1 : 0);
}

// The block's sum of v in every thread (waves added in wave order).
__device__ __forceinline__ int64_t rp_block_sum(RpLds& L, int64_t v) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = wave_xor_sum(v);
  __syncthreads();
  if (lane == 0) L.red_i[w][0] = v;
  __syncthreads();
  return ((L.red_i[0][0] + L.red_i[1][0]) + L.red_i[2][0]) + L.red_i[3][0];
}

// Bitonic sort of the first P (a power of two) entries into list order; equal
// (key, column) pairs by entry offset, so the result is one fixed permutation.
__device__ __forceinline__ void rp_sort(RpLds& L, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < P; i += kRpBlock) {
        const int l = i ^ j;
        if (l <= i) continue;
        const uint64_t ki = L.key[i], kl = L.key[l];
        const int32_t ci = L.col[i], cl = L.col[l];
        const int32_t ii = L.idx[i], il = L.idx[l];
        const bool l_first = rp_before(kl, cl, ki, ci) || (kl == ki && cl == ci && (uint32_t)il < (uint32_t)ii);
        const bool i_first = rp_before(ki, ci, kl, cl) || (kl == ki && cl == ci && (uint32_t)ii < (uint32_t)il);
        if ((i & k) == 0 ? l_first : i_first) {
          L.key[i] = kl, L.key[l] = ki;
          L.col[i] = cl, L.col[l] = ci;
          L.idx[i] = il, L.idx[l] = ii;
        }
      }
    }
  }
  __syncthreads();
}

// cnt[i] <- cnt[0] + ... + cnt[i] for i < P (P <= kRpChunk): four consecutive
// counters per thread, the wave's scan by lane shifts, the waves in order.
__device__ __forceinline__ void rp_scan(RpLds& L, int P) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int kPer = kRpChunk / kRpBlock;
  int v[kPer], s = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int i = threadIdx.x * kPer + e;
    v[e] = i < P ? L.cnt[i] : 0;
    s += v[e];
    v[e] = s;
  }
  int inc = s;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int o = __shfl_up(inc, off, kWave);
    inc += lane >= off ? o : 0;
  }
  if (lane == kWave - 1) L.scan[w] = inc;
  __syncthreads();
  int base = inc - s;
  for (int x = 0; x < w; ++x) base += L.scan[x];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int i = threadIdx.x * kPer + e;
    if (i < P) L.cnt[i] = base + v[e];
  }
  __syncthreads();
}

template <int SRC>
__global__ __launch_bounds__(kRpBlock) void rp_kernel(const RpParams P) {
  typedef typename std::conditional<SRC == HREC_UM_SRC_F64, double, float>::type A;  // the stored element
  typedef typename std::conditional<SRC == HREC_UM_SRC_F64, rp_d2, hp_f4>::type V;   // 16 bytes of them
  constexpr int kVec = 16 / (int)sizeof(A);
  constexpr bool kPacked = SRC == HREC_UM_SRC_F32;  // 64 bits hold the value's key and the column
  __shared__ RpLds L;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t row = blockIdx.x;
  const int64_t n = P.n;
  const ExclSeg lab = excl_segment(P.lrows, P.lindptr, row);
  const ExclSeg xs = excl_segment(P.xrows, P.xindptr, row);
  const int64_t m = lab.hi > lab.lo ? lab.hi - lab.lo : 0;

  // 1. live columns
  int64_t gone = 0;
  for (int64_t p = xs.lo + tid; p < xs.hi; p += kRpBlock) gone += excl_counts(P.xcols, xs.lo, p, n) ? 1 : 0;
  gone = rp_block_sum(L, gone);
  const int64_t live = n - gone;

  UmFuse f{};
  if constexpr (SRC == HREC_UM_SRC_FUSED) f = um_fuse_row(P.minmax, P.wins, row);
  const A* __restrict__ ra = static_cast<const A*>(P.sa) + row * P.ld;
  const float* __restrict__ rb = nullptr;
  if constexpr (SRC == HREC_UM_SRC_FUSED) rb = P.sb + row * P.ld;
  auto key_of = [&](A a, float t, int64_t c) {
    if constexpr (kPacked) return rp_packed_key(um_value<SRC>(P, a, t, c, f), c);
    else return order_key((double)um_value<SRC>(P, a, t, c, f));
  };
  auto key_at = [&](int64_t c) {
    if constexpr (SRC == HREC_UM_SRC_FUSED) return key_of(ra[c], rb[c], c);
    else return key_of(ra[c], 0.0f, c);
  };
  // the aligned body of the row: [head, head + body), whole 16-byte vectors
  int64_t head = (int64_t)((kVec - (int)(((uintptr_t)ra / sizeof(A)) % kVec)) % kVec);
  if constexpr (SRC == HREC_UM_SRC_FUSED) {
    if (((uintptr_t)ra & 15) != ((uintptr_t)rb & 15)) head = n;  // no common alignment: scalar
  }
  head = head < n ? head : n;
  const int64_t body = (n - head) / kVec * kVec;

  int64_t sum_rank = 0, h = 0, ranked = 0, min_rank = INT64_MAX;
  double sw = 0.0, swpr = 0.0;
  const double denom = (double)(live - 1);

  for (int64_t c0 = 0; c0 < m; c0 += kRpChunk) {
    const int mc = (int)(m - c0 < kRpChunk ? m - c0 : kRpChunk);
    int Pn = 2;
    while (Pn < mc) Pn <<= 1;
    // 2. key the chunk
    __syncthreads();
    int valid = 0;
    for (int i = tid; i < Pn; i += kRpBlock) {
      uint64_t k = 0;
      int32_t c = kRpNoCol, id = -1;
      if (i < mc) {
        const int64_t lc = P.lcols[lab.lo + c0 + i];
        if (lc >= 0 && lc < n && !excl_contains(P.xcols, xs.lo, xs.hi, lc)) {
          k = key_at(lc), c = (int32_t)lc, id = i;
          ++valid;
        }
        L.rank[i] = -1;
      }
      L.key[i] = k, L.col[i] = c, L.idx[i] = id;
      L.cnt[i] = 0;
      L.dup[i] = 0;
    }
    if (tid == 0) L.cnt[Pn] = 0;
    valid = (int)rp_block_sum(L, valid);
    if (valid > 0) {  // block-uniform
      rp_sort(L, Pn);
      // 3. the stream
      // a column after the chunk's last ranked entry stands before none of them: no search, no counter (on
      // a model that ranks the held-out items high that is most of the row, and it would be one hot counter)
      const uint64_t last_k = L.key[valid - 1];
      const int32_t last_c = L.col[valid - 1];
      auto visit = [&](uint64_t k, int64_t c) {
        if (kPacked ? last_k > k : rp_before(last_k, last_c, k, (int32_t)c)) return;
        const int t = rp_search<false, kPacked>(L, Pn, k, (int32_t)c);
        if (t < valid) atomicAdd(&L.cnt[t], 1);
      };
      for (int64_t j = tid; j < head; j += kRpBlock) visit(key_at(j), j);
      // the next vector is in flight while this one is searched
      const int64_t end = head + body, stride = (int64_t)kRpBlock * kVec;
      int64_t j = head + (int64_t)tid * kVec;
      V a_next{};
      hp_f4 t_next{};
      if (j < end) {
        a_next = __builtin_nontemporal_load(reinterpret_cast<const V*>(ra + j));
        if constexpr (SRC == HREC_UM_SRC_FUSED) {
          t_next = __builtin_nontemporal_load(reinterpret_cast<const hp_f4*>(rb + j));
        }
      }
      for (; j < end; j += stride) {
        const V a = a_next;
        const hp_f4 t = t_next;
        if (j + stride < end) {
          a_next = __builtin_nontemporal_load(reinterpret_cast<const V*>(ra + j + stride));
          if constexpr (SRC == HREC_UM_SRC_FUSED) {
            t_next = __builtin_nontemporal_load(reinterpret_cast<const hp_f4*>(rb + j + stride));
          }
        }
#pragma unroll
        for (int e = 0; e < kVec; ++e) visit(key_of(a[e], SRC == HREC_UM_SRC_FUSED ? t[e] : 0.0f, j + e), j + e);
      }
      for (int64_t j = head + body + tid; j < n; j += kRpBlock) visit(key_at(j), j);
      // 4. the excluded columns leave
      for (int64_t p = xs.lo + tid; p < xs.hi; p += kRpBlock) {
        if (!excl_counts(P.xcols, xs.lo, p, n)) continue;
        const int64_t c = P.xcols[p];
        const int t = rp_search<false, kPacked>(L, Pn, key_at(c), (int32_t)c);
        if (t < valid) atomicSub(&L.cnt[t], 1);
      }
      __syncthreads();
      // 5. ranks
      rp_scan(L, Pn);
      for (int i = tid; i < Pn; i += kRpBlock) {
        if (L.idx[i] >= 0 && i > 0 && L.col[i - 1] == L.col[i] && L.key[i - 1] == L.key[i]) L.dup[i] = 1;
      }
      __syncthreads();
      for (int64_t e = tid; e < c0; e += kRpBlock) {  // columns the earlier chunks counted
        const int64_t lc = P.lcols[lab.lo + e];
        if (lc < 0 || lc >= n) continue;
        const uint64_t k = key_at(lc);
        const int i = rp_search<true, kPacked>(L, Pn, k, (int32_t)lc);
        if (i < Pn && L.col[i] == (int32_t)lc && L.key[i] == k) L.dup[i] = 1;
      }
      __syncthreads();
      for (int i = tid; i < Pn; i += kRpBlock) {
        const int id = L.idx[i];
        if (id < 0) continue;
        const int64_t r = L.cnt[i];
        L.rank[id] = (int32_t)r;
        ++ranked;
        if (!L.dup[i]) {
          sum_rank += r, ++h;
          min_rank = r < min_rank ? r : min_rank;
        }
      }
      __syncthreads();
    }
    // 6. by entry, in CSR order
    for (int i = tid; i < mc; i += kRpBlock) {
      const int32_t r = L.rank[i];
      if (P.out_rank) P.out_rank[lab.lo + c0 + i] = r;
      if (r < 0) continue;
      const double wt = P.lweight ? P.lweight[lab.lo + c0 + i] : 1.0;
      const double pr = live == 1 ? 0.0 : (double)r / denom;
      swpr += wt * pr;
      sw += wt;
    }
  }

  // the row's values: integers exactly, the doubles in a fixed tree
  sum_rank = wave_xor_sum(sum_rank), h = wave_xor_sum(h), ranked = wave_xor_sum(ranked);
  min_rank = wave_xor_min(min_rank);
  sw = wave_xor_sum(sw), swpr = wave_xor_sum(swpr);
  __syncthreads();
  if (lane == 0) {
    L.red_i[w][0] = sum_rank, L.red_i[w][1] = h, L.red_i[w][2] = ranked, L.red_i[w][3] = min_rank;
    L.red_d[w][0] = swpr, L.red_d[w][1] = sw;
  }
  __syncthreads();
  if (tid != 0) return;
  sum_rank = h = ranked = 0;
  min_rank = INT64_MAX;
  for (int x = 0; x < kRpBlock / kWave; ++x) {
    sum_rank += L.red_i[x][0], h += L.red_i[x][1], ranked += L.red_i[x][2];
    min_rank = L.red_i[x][3] < min_rank ? L.red_i[x][3] : min_rank;
  }
  swpr = ((L.red_d[0][0] + L.red_d[1][0]) + L.red_d[2][0]) + L.red_d[3][0];
  sw = ((L.red_d[0][1] + L.red_d[1][1]) + L.red_d[2][1]) + L.red_d[3][1];
  const double nan = __builtin_nan("");
  double auc = nan, rr = nan;
  if (h > 0) {
    rr = 1.0 / (double)(1 + min_rank);
    if (live != h) auc = 1.0 - (double)(sum_rank - h * (h - 1) / 2) / ((double)h * (double)(live - h));
  }
  double* o = P.out_row + 4 * row;
  o[0] = auc, o[1] = rr, o[2] = swpr, o[3] = sw;
  int32_t* on = P.out_row_n + 3 * row;
  on[0] = (int32_t)live, on[1] = (int32_t)ranked, on[2] = (int32_t)(m - ranked);
}

// Slot s of row r's contribution to the sums (include/hrec.h: HREC_RP_SUMS).
__device__ __forceinline__ double rp_slot(const double* __restrict__ o, const int32_t* __restrict__ on, int s) {
  const bool has = on[1] > 0;
  switch (s) {
    case 0: return o[0] == o[0] ? o[0] : 0.0;
    case 1: return o[1] == o[1] ? o[1] : 0.0;
    case 2: return has ? o[2] : 0.0;
    case 3: return has ? o[3] : 0.0;
    case 4: return o[0] == o[0] ? 1.0 : 0.0;
    case 5: return o[1] == o[1] ? 1.0 : 0.0;
    case 6:
    case 7: return has ? 1.0 : 0.0;
    case 8: return (double)on[1];
    default: return (double)on[2];
  }
}

// partials[b][s] = slot s over rows [256 b, 256 b + 256): the lanes' xor tree, the waves in order.
__global__ __launch_bounds__(kRpBlock) void rp_partial_kernel(const double* __restrict__ out_row,
                                                             const int32_t* __restrict__ out_row_n, int64_t n_rows,
                                                             double* __restrict__ partials) {
  __shared__ double red[kRpBlock / kWave][kRpSums];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * kRpBlock + threadIdx.x;
#pragma unroll
  for (int s = 0; s < kRpSums; ++s) {
    double v = row < n_rows ? rp_slot(out_row + 4 * row, out_row_n + 3 * row, s) : 0.0;
    v = wave_xor_sum(v);
    if (lane == 0) red[w][s] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < kRpSums) {
    const int s = threadIdx.x;
    partials[(int64_t)blockIdx.x * kRpSums + s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
  }
}

// sums[s] = the partials of slot s (block s of the launch): lane l adds
// blocks l, l + 64, ... in ascending order, then the lanes' xor tree.
__global__ __launch_bounds__(64) void rp_reduce_kernel(const double* __restrict__ partials, int64_t n_blocks,
                                                       double* __restrict__ sums) {
  const int lane = threadIdx.x, s = blockIdx.x;
  double v = 0.0;
  for (int64_t b = lane; b < n_blocks; b += 64) v += partials[b * kRpSums + s];
  v = wave_xor_sum(v);
  if (lane == 0) sums[s] = v;
}

}  // namespace hrec

using namespace hrec;

static int64_t rp_blocks(int64_t n_rows) { return n_rows > 0 ? (n_rows + kRpBlock - 1) / kRpBlock : 1; }

extern "C" size_t hrec_rank_positions_workspace_bytes(int64_t n_rows) {
  return al256((size_t)rp_blocks(n_rows) * kRpSums * sizeof(double));
}

extern "C" int hrec_rank_positions(int64_t n_rows, int64_t n, int source, const void* scores, const float* tt_scores,
                                   int64_t ld, const double* als_fallback, const double* minmax,
                                   const int32_t* row_wins, const int64_t* label_rows, const int64_t* label_indptr,
                                   const int32_t* label_cols, const double* label_weight, const int64_t* excl_rows,
                                   const int64_t* excl_indptr, const int32_t* excl_cols, int32_t* out_rank,
                                   double* out_row, int32_t* out_row_n, double* sums_out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  HREC_REQUIRE(n_rows >= 0 && n >= 1 && n <= INT32_MAX && n_rows <= INT32_MAX, "rank_positions: bad shape");
  HREC_REQUIRE(ld >= n, "rank_positions: ld must be >= n");
  HREC_REQUIRE(source >= HREC_UM_SRC_F64 && source <= HREC_UM_SRC_FUSED, "rank_positions: source must be in [0, 3]");
  const bool any_lab = label_rows || label_indptr || label_cols;
  HREC_REQUIRE(!any_lab || (label_rows && label_indptr && label_cols),
               "rank_positions: the label CSR needs label_rows, label_indptr and label_cols (or none of them)");
  HREC_REQUIRE(!label_weight || any_lab, "rank_positions: label_weight without a label CSR");
  const bool any_excl = excl_rows || excl_indptr || excl_cols;
  HREC_REQUIRE(!any_excl || (excl_rows && excl_indptr && excl_cols),
               "rank_positions: the exclusion CSR needs excl_rows, excl_indptr and excl_cols (or none of them)");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(scores && out_row && out_row_n && sums_out && workspace, "rank_positions: null pointer");
  HREC_REQUIRE(source != HREC_UM_SRC_FUSED || (tt_scores && minmax && row_wins),
               "rank_positions: the fused source needs tt_scores, minmax and row_wins");
  const size_t need = hrec_rank_positions_workspace_bytes(n_rows);
  HREC_REQUIRE(workspace_bytes >= need, "rank_positions: workspace %zu < %zu", workspace_bytes, need);
  RpParams P{};
  P.sa = scores, P.sb = tt_scores, P.ld = ld;
  P.fb = (source == HREC_UM_SRC_ALS || source == HREC_UM_SRC_FUSED) ? als_fallback : nullptr;
  P.n_rows = n_rows, P.n = n;
  P.minmax = minmax, P.wins = row_wins;
  P.lrows = label_rows, P.lindptr = label_indptr, P.lcols = label_cols, P.lweight = label_weight;
  P.xrows = excl_rows, P.xindptr = excl_indptr, P.xcols = excl_cols;
  P.out_rank = out_rank, P.out_row = out_row, P.out_row_n = out_row_n;
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)n_rows), block(kRpBlock);
  switch (source) {
    case HREC_UM_SRC_F64: hipLaunchKernelGGL(rp_kernel<HREC_UM_SRC_F64>, grid, block, 0, s, P); break;
    case HREC_UM_SRC_F32: hipLaunchKernelGGL(rp_kernel<HREC_UM_SRC_F32>, grid, block, 0, s, P); break;
    case HREC_UM_SRC_ALS: hipLaunchKernelGGL(rp_kernel<HREC_UM_SRC_ALS>, grid, block, 0, s, P); break;
    default: hipLaunchKernelGGL(rp_kernel<HREC_UM_SRC_FUSED>, grid, block, 0, s, P); break;
  }
  int rc = check_launch("rp_kernel");
  if (rc) return rc;
  const int64_t nb = rp_blocks(n_rows);
  double* partials = static_cast<double*>(workspace);
  hipLaunchKernelGGL(rp_partial_kernel, dim3((unsigned)nb), block, 0, s, out_row, out_row_n, n_rows, partials);
  rc = check_launch("rp_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(rp_reduce_kernel, dim3(kRpSums), dim3(64), 0, s, partials, nb, sums_out);
  return check_launch("rp_reduce_kernel");
}
