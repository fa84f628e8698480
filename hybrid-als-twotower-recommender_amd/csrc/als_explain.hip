// hrec_als_explain: why an ALS prediction is what it is, by the user's history
// (Hu, Koren and Volinsky 2008, section 5). A user row is the solution of its
// normal equations, x_u = A_u^-1 b_u with b_u = sum_j beta_j y_j, so
//   y_i . x_u = sum_j beta_j (y_i^T A_u^-1 y_j) = sum_j c_ij
// over the history entries j. Per kernel row (a user and one list of candidate
// columns): A and b as the half-sweeps form them, A = Ut^T D Ut once, then per
// list entry i the solve A w_i = y_i and, per history entry j,
// c_ij = beta_j (w_i . y_j); their sum, and the top_m largest with their
// positions in the history segment. include/hrec.h has the contract.
//
// Shape: one wave per row (one block of 64 threads).
//   1. gram_row + factor_row of csrc/als_row.h, unchanged, with the row's real
//      b: x = A^-1 b goes to out_row, and Ut (Up, column-packed, permuted
//      basis q = 16 T + m <-> column NT m + T) and the pivots (dsh) stay in the
//      wave's LDS slice.
//   2. The list in groups of kExGroup = 16 entries. Four right-hand sides at a
//      time, one lane per column: forward Ut^T z = y_i, z / d, back Ut w = z —
//      2 KP steps of one LDS read of Ut, then per right-hand side one
//      v_readlane broadcast and one masked fma. w_i goes to LDS in physical
//      column order.
//   3. The history in windows of 64 entries: lane l holds y_j of entry
//      64 w + l in registers (KP floats), and per list entry of the group runs
//      the fma chain over components 0..KP-1 ascending against w_i read as LDS
//      broadcasts (components >= k are exact zeros on both sides). c_ij adds
//      into the lane's partial of entry i (LDS, the lane's own slot); the
//      window's eligible c_ij merge into the entry's sorted top_m list (LDS,
//      one lane per slot while merging): best remaining candidate by a wave xor
//      tree over (value, lane), inserted behind every list value >= it, until
//      none beats the list's last value.
//   4. Per entry: the 64 partials through a fixed xor tree -> out_total.
// Fixed orders throughout, no atomics: equal inputs give equal bits.
//
// LDS per block at kp 64 / 32 / 16 (bytes): the half-sweep's slice
// RowLds<KP>::kSize * 8 = 19,200 / 6,016 / 3,456; w of a group 16 * KP * 8 =
// 8,192 / 4,096 / 2,048; partials 16 * 64 * 8 = 8,192; top lists 16 * 32 * 12 =
// 6,144; the row's x 4 * KP. Total 41,984 / 24,576 / 19,904 (what the compiler
// reports): three blocks per CU at kp 64 (160 KiB). No scratch at any kp.
#include "als_row.h"

namespace hrec {

constexpr int kExGroup = 16;    // list entries per group
constexpr int kExTopMax = 32;   // top_m limit (one lane per slot)
constexpr int kExListMax = 1024;

struct ExplainParams {
  const int64_t* lists;
  int64_t lists_ld;
  int list_n;
  const int32_t* list_len;
  const int64_t* hist_rows;
  const int64_t* hist_indptr;
  const int32_t* hist_cols;
  const float* hist_vals;
  const float* items;
  int64_t n_items;
  int k;
  double reg;
  double alpha;
  const double* yty;
  int top_m;
  double* out_total;
  int32_t* out_pos;
  double* out_val;
  int32_t* out_len;
  float* out_row;
};

// Entries [e0, e1) of row `row` get "nothing to say": length 0, total NaN,
// positions -1, values NaN.
__device__ __forceinline__ void explain_blank(const ExplainParams& P, int64_t row, int e0, int e1, int lane) {
  const double nan = __builtin_nan("");
  for (int e = e0 + lane; e < e1; e += kWave) {
    const int64_t o = row * P.list_n + e;
    P.out_len[o] = 0;
    P.out_total[o] = nan;
  }
  const int cnt = (e1 - e0) * P.top_m;
  const int64_t base = (row * P.list_n + e0) * (int64_t)P.top_m;
  for (int i = lane; i < cnt; i += kWave) {
    P.out_pos[base + i] = -1;
    P.out_val[base + i] = nan;
  }
}

// The window's candidates (v on live lanes, history position pos0 + lane) into
// the sorted list of one entry: lane s < L holds slot s (lv, lp). Larger value
// first, equal values: the earlier position (every candidate is later than
// every list member, and a lower lane is earlier).
__device__ __forceinline__ void explain_merge(double v, bool live, int pos0, int lane, int top_m, int& L, double& lv,
                                              int& lp) {
  const double ninf = -__builtin_inf();
  for (;;) {
    if (L == top_m) live = live && v > lane_read(lv, top_m - 1);
    if (__ballot(live) == 0) break;
    double bv = live ? v : ninf;
    int bl = live ? lane : kWave;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv, off, kWave);
      const int ol = __shfl_xor(bl, off, kWave);
      if (ov > bv || (ov == bv && ol < bl)) bv = ov, bl = ol;
    }
    const int p = __builtin_popcountll(__ballot(lane < L && lv >= bv));
    const double upv = __shfl_up(lv, 1, kWave);
    const int upp = __shfl_up(lp, 1, kWave);
    if (lane == p) {
      lv = bv, lp = pos0 + bl;
    } else if (lane > p && lane <= L && lane < top_m) {
      lv = upv, lp = upp;
    }
    L = L < top_m ? L + 1 : L;
    if (lane == bl) live = false;
  }
}

template <int NT, bool IMP>
__global__ __launch_bounds__(64) void als_explain_kernel(const ExplainParams P) {
  constexpr int KP = 16 * NT;
  constexpr int CH = 8;  // gram_row's chunk, as the half-sweeps instantiate it
  __shared__ __attribute__((aligned(16))) double lds[RowLds<KP>::kSize];
  __shared__ __attribute__((aligned(16))) double wsh[kExGroup * KP];
  __shared__ double psh[kExGroup * kWave];
  __shared__ double topv[kExGroup * kExTopMax];
  __shared__ int topp[kExGroup * kExTopMax];
  __shared__ __attribute__((aligned(16))) float xrow[KP];
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const bool incol = lane < KP;
  const int phys = NT * (lane & 15) + ((lane >> 4) & (NT - 1));  // the column lane `lane` owns in the permuted basis
  const double nan = __builtin_nan(""), ninf = -__builtin_inf();

  int len = P.list_len ? P.list_len[row] : P.list_n;
  len = len < 0 ? 0 : (len > P.list_n ? P.list_n : len);
  const int64_t q = P.hist_rows[row];
  const int64_t beg = q < 0 ? 0 : P.hist_indptr[q];
  const int64_t end = q < 0 ? 0 : P.hist_indptr[q + 1];
  const int64_t n = end - beg;

  double* scratch = lds + RowLds<KP>::kUpPad;
  double* bsh = scratch + 128 + 2 * KP;
  const double* dsh = scratch + 128;
  bool ok = n > 0;  // wave-uniform
  if (ok) {
    d4 acc[NT * (NT + 1) / 2];
    if constexpr (IMP) {
      int n_pos = 0;
      gram_row<NT, CH, 0, false, true>(beg, end, lane, P.hist_cols, P.hist_vals, P.items, P.n_items, P.k, P.reg, acc,
                                       bsh, lds, P.alpha, P.yty, &n_pos);
      ok = n_pos > 0;
      if (ok) factor_row<NT>(lane, acc, lds, scratch, bsh, xrow);
    } else {
      gram_row<NT, CH, 0>(beg, end, lane, P.hist_cols, P.hist_vals, P.items, P.n_items, P.k, P.reg, acc, bsh, lds);
      factor_row<NT>(lane, acc, lds, scratch, bsh, xrow);
    }
  }
  // rows the half-sweep leaves at zero (no history, no rating > 0): zero here
  const float xr = (ok && incol) ? xrow[lane] : 0.f;
  if (P.out_row && incol) P.out_row[row * KP + lane] = xr;
  const double dl = (ok && incol) ? dsh[lane] : 1.0;
  if (ok) {
    // a usable factorisation: every pivot positive and finite, x finite
    const bool bad = !(dl > 0.0 && dl < __builtin_inf()) || !(xr - xr == 0.f);
    ok = __ballot(bad) == 0;
  }
  if (!ok) {
    explain_blank(P, row, 0, P.list_n, lane);
    return;
  }

  const int top_m = P.top_m;
  const int64_t* __restrict__ lrow = P.lists + row * P.lists_ld;
  for (int g0 = 0; g0 < P.list_n; g0 += kExGroup) {
    const int gn = P.list_n - g0 < kExGroup ? P.list_n - g0 : kExGroup;
    // the group's validated columns on lanes 0..15 (-1: not an entry)
    int gv = -1;
    if (lane < gn && g0 + lane < len) {
      const int64_t c = lrow[g0 + lane];
      gv = (c >= 0 && c < P.n_items) ? (int)c : -1;
    }
    const uint64_t gmask = __ballot(gv >= 0);
    if (gmask == 0) {
      explain_blank(P, row, g0, g0 + gn, lane);
      continue;
    }
    // ---- w_i = A^-1 y_i, four right-hand sides per pass
    for (int p0 = 0; p0 < gn; p0 += 4) {
      if (((gmask >> p0) & 0xf) == 0) continue;
      double z[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int c = lane_read(gv, (p0 + s) & (kExGroup - 1));
        z[s] = (c >= 0 && incol) ? (double)P.items[(int64_t)c * KP + phys] : 0.0;
      }
      // forward  Ut^T z = y   (step pv: lanes c > pv subtract Ut[pv][c] * z_pv)
#pragma unroll 4
      for (int pv = 0; pv < KP - 1; ++pv) {
        const bool act = incol && lane > pv;
        const double u = act ? lds[tri(lane) + pv] : 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double zq = lane_read(z[s], pv);
          if (act) z[s] = fma(-u, zq, z[s]);
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) z[s] = z[s] / dl;
      // back     Ut w = z     (step c: lanes r < c subtract Ut[r][c] * w_c)
#pragma unroll 4
      for (int c = KP - 1; c > 0; --c) {
        const bool act = lane < c;
        const double u = lds[tri(c) + (act ? lane : 0)];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double wq = lane_read(z[s], c);
          if (act) z[s] = fma(-u, wq, z[s]);
        }
      }
      if (incol) {
#pragma unroll
        for (int s = 0; s < 4; ++s) wsh[(p0 + s) * KP + phys] = z[s];
      }
    }
    for (int t = 0; t < gn; ++t) psh[t * kWave + lane] = 0.0;
    wave_lds_fence();

    // ---- the history, 64 entries per window
    int64_t elig_before = 0;
    for (int64_t w0 = 0; w0 < n; w0 += kWave) {
      const int64_t j = w0 + lane;
      const bool has = j < n;
      int hc = has ? P.hist_cols[beg + j] : 0;
      hc = (hc < 0 || hc >= P.n_items) ? 0 : hc;  // never an index out of the matrix
      const double r = has ? (double)P.hist_vals[beg + j] : 0.0;
      double beta = r;
      bool elig = has;
      if constexpr (IMP) {
        const double c1 = P.alpha * fabs(r);
        elig = has && r > 0.0;
        beta = r > 0.0 ? 1.0 + c1 : 0.0;
      }
      float yj[KP];
      const float4* __restrict__ yp = reinterpret_cast<const float4*>(P.items + (int64_t)hc * KP);
#pragma unroll
      for (int c = 0; c < KP / 4; ++c) {
        const float4 t4 = yp[c];
        yj[4 * c] = t4.x, yj[4 * c + 1] = t4.y, yj[4 * c + 2] = t4.z, yj[4 * c + 3] = t4.w;
      }
      const int ne = __builtin_popcountll(__ballot(elig));
      const int L0 = (int)(elig_before < top_m ? elig_before : top_m);
      for (int t = 0; t < gn; ++t) {
        if (((gmask >> t) & 1) == 0) continue;
        const double* __restrict__ w = wsh + t * KP;
        double dot = 0.0;
#pragma unroll
        for (int c = 0; c < KP; c += 2) {
          const double2 w2 = *reinterpret_cast<const double2*>(w + c);
          dot = fma(w2.x, (double)yj[c], dot);
          dot = fma(w2.y, (double)yj[c + 1], dot);
        }
        const double cv = beta * dot;
        if (elig) psh[t * kWave + lane] += cv;
        if (ne == 0) continue;
        int L = L0;
        double lv = lane < L ? topv[t * kExTopMax + (lane & (kExTopMax - 1))] : ninf;
        int lp = lane < L ? topp[t * kExTopMax + (lane & (kExTopMax - 1))] : -1;
        explain_merge(cv == cv ? cv : ninf, elig, (int)w0, lane, top_m, L, lv, lp);
        if (lane < L) topv[t * kExTopMax + lane] = lv, topp[t * kExTopMax + lane] = lp;
      }
      elig_before += ne;
      wave_lds_fence();
    }

    // ---- the group's outputs
    const int Lf = (int)(elig_before < top_m ? elig_before : top_m);
    for (int t = 0; t < gn; ++t) {
      const int64_t o = row * P.list_n + g0 + t;
      if (((gmask >> t) & 1) == 0) {
        explain_blank(P, row, g0 + t, g0 + t + 1, lane);
        continue;
      }
      double tot = psh[t * kWave + lane];
#pragma unroll  // written out: wave_xor_sum here changes the generated code
      for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, kWave);
      if (lane == 0) {
        P.out_total[o] = Lf > 0 ? tot : nan;
        P.out_len[o] = Lf;
      }
      if (lane < top_m) {
        P.out_pos[o * top_m + lane] = lane < Lf ? topp[t * kExTopMax + lane] : -1;
        P.out_val[o * top_m + lane] = lane < Lf ? topv[t * kExTopMax + lane] : nan;
      }
    }
    wave_lds_fence();  // the next group rewrites w, the partials and the lists
  }
}

}  // namespace hrec

using namespace hrec;

extern "C" int hrec_als_explain(const int64_t* lists, int64_t lists_ld, int list_n, const int32_t* list_len,
                                int64_t n_rows, const int64_t* hist_rows, const int64_t* hist_indptr,
                                const int32_t* hist_cols, const float* hist_vals, const float* item_factors,
                                int64_t n_items, int k, int kp, double reg_param, int implicit, double alpha,
                                const double* yty, int top_m, double* out_total, int32_t* out_pos, double* out_val,
                                int32_t* out_len, float* out_row, void* stream) {
  HREC_REQUIRE(kp == 16 || kp == 32 || kp == 64,
               "als_explain: kp must be 16, 32 or 64 (explanations support rank <= 64; got kp %d)", kp);
  HREC_REQUIRE(k >= 1 && k <= kp, "als_explain: need 1 <= k <= kp (k=%d kp=%d)", k, kp);
  HREC_REQUIRE(top_m >= 1 && top_m <= kExTopMax, "als_explain: top_m must be in [1, %d] (got %d)", kExTopMax, top_m);
  HREC_REQUIRE(list_n >= 0 && list_n <= kExListMax, "als_explain: list_n must be in [0, %d] (got %d)", kExListMax,
               list_n);
  HREC_REQUIRE(lists_ld >= list_n, "als_explain: lists_ld must be >= list_n");
  HREC_REQUIRE(implicit == 0 || implicit == 1, "als_explain: implicit must be 0 or 1");
  HREC_REQUIRE(alpha >= 0.0, "als_explain: alpha must be >= 0 (got %g)", alpha);
  HREC_REQUIRE(reg_param >= 0.0, "als_explain: reg_param must be >= 0");
  HREC_REQUIRE(n_rows >= 0 && n_items >= 0, "als_explain: negative size");
  HREC_REQUIRE(n_rows < 0x7fffffffll && n_items < 0x7fffffffll, "als_explain: too many rows for one launch");
  HREC_REQUIRE(kp != 64 || n_items * (int64_t)kp * 4 <= (int64_t)0xffffffffll,
               "als_explain: %lld item rows of %d floats exceed the 4 GiB a gather resource spans", (long long)n_items,
               kp);
  HREC_REQUIRE(!implicit || yty, "als_explain: implicit needs yty (hrec_als_gramian of item_factors)");
  if (n_rows == 0 || list_n == 0) return HREC_OK;
  HREC_REQUIRE(lists && hist_rows && hist_indptr && hist_cols && hist_vals && out_total && out_pos && out_val &&
                   out_len,
               "als_explain: null pointer");
  HREC_REQUIRE(n_items > 0 && item_factors, "als_explain: null item factors");
  ExplainParams P{};
  P.lists = lists, P.lists_ld = lists_ld, P.list_n = list_n, P.list_len = list_len;
  P.hist_rows = hist_rows, P.hist_indptr = hist_indptr, P.hist_cols = hist_cols, P.hist_vals = hist_vals;
  P.items = item_factors, P.n_items = n_items, P.k = k, P.reg = reg_param, P.alpha = alpha, P.yty = yty;
  P.top_m = top_m;
  P.out_total = out_total, P.out_pos = out_pos, P.out_val = out_val, P.out_len = out_len, P.out_row = out_row;
  const dim3 grid((unsigned)n_rows), block(64);
  hipStream_t s = as_stream(stream);
#define HREC_EXPLAIN(NT)                                                                    \
  do {                                                                                      \
    if (implicit) hipLaunchKernelGGL((als_explain_kernel<NT, true>), grid, block, 0, s, P); \
    else hipLaunchKernelGGL((als_explain_kernel<NT, false>), grid, block, 0, s, P);         \
  } while (0)
  if (kp == 64) HREC_EXPLAIN(4);
  else if (kp == 32) HREC_EXPLAIN(2);
  else HREC_EXPLAIN(1);
#undef HREC_EXPLAIN
  return check_launch("als_explain_kernel");
}
