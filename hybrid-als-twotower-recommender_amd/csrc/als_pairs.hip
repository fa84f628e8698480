// K2x: ALS predictions for a list of (user, item) pairs (Spark
// ALSModel.transform on a pair frame) and, fused, the sums behind Spark's
// RegressionEvaluator (rmse / mse / mae / r2 / var).
//
//   out[p] = sum_{c<k} U[user_rows[p]][c] * V[item_rows[p]][c]
//
// as hrec_als_score's chain: f32, sequential in c from 0.0f, the product
// rounded, then the sum rounded (contraction off). A row index outside
// [0, n_rows) on either side gives a quiet NaN and is never turned into an
// address (one unsigned compare per side).
//
// Shape: a row gather without reuse, two kp-float rows per pair. One wave owns
// a tile of 64 pairs. The chain of a pair cannot be split across lanes, the
// loads can: CW / 4 lanes x float4 fetch CW columns of one row (16 lanes per
// 256-B row at CW = 64), so one wave-instruction fetches 64 / (CW / 4) rows in
// full lines, and kPairBatch such instructions per side are in flight before
// the first LDS write. The fetching lane holds the same columns of the
// pair's user and item row, so it forms the rounded products there and the
// tile in LDS holds products only: [64 pairs][CW + 1] floats per wave, the odd
// row stride putting lane l's walk over its own pair's row on bank (l + c)
// mod 32. Each lane then adds its pair's products in order; the sum is carried
// in a register across the chunks of CW columns of a wider row. At CW = 64 a
// workgroup of 4 waves holds 66,560 B of tiles + 4 KiB of row indices: two
// workgroups = 8 waves per CU.
#include "pairs.h"

namespace hrec {

// CW: columns per chunk (16, 32 or 64; kp is a multiple of it). METRICS: also
// the f64 sums of the pairs with a prediction (label - prediction), one
// partial of HREC_PAIR_SUMS doubles per block in `partials`; out may be null.
template <int CW, bool METRICS>
__global__ __launch_bounds__(kPairBlock) void als_pairs_kernel(
    const float* __restrict__ U, int64_t n_u, const float* __restrict__ V, int64_t n_v, int k, int kp,
    const int64_t* __restrict__ user_rows, const int64_t* __restrict__ item_rows, int64_t n,
    float* __restrict__ out, const double* __restrict__ labels, double* __restrict__ partials) {
#pragma clang fp contract(off)
  constexpr int LPR = CW / 4;    // lanes per row piece
  constexpr int RPI = 64 / LPR;  // rows per wave-instruction
  constexpr int NIT = LPR;       // instructions per side that cover the tile's 64 rows
  constexpr int NB = NIT < kPairBatch ? NIT : kPairBatch;
  constexpr int STR = CW + 1;    // odd row stride (dwords)
  __shared__ float prod[4][64 * STR];
  __shared__ int64_t srow[4][2][64];
  __shared__ double red[METRICS ? 4 : 1][HREC_PAIR_SUMS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane / LPR, q = lane % LPR;
  float* __restrict__ tile = prod[w];
  const int64_t n_tiles = (n + 63) / 64;
  const int64_t t_step = (int64_t)gridDim.x * 4;
  double s[HREC_PAIR_SUMS];
#pragma unroll
  for (int i = 0; i < HREC_PAIR_SUMS; ++i) s[i] = 0.0;

  // this tile's row indices (and label), read one tile ahead of their use
  int64_t t = (int64_t)blockIdx.x * 4 + w;
  int64_t ur = -1, ir = -1;
  double y = 0.0;
  auto fetch_ids = [&](int64_t tt, int64_t& u, int64_t& i, double& lab) {
    const int64_t p = tt * 64 + lane;
    u = i = -1;
    lab = 0.0;
    if (tt < n_tiles && p < n) {
      u = user_rows[p];
      i = item_rows[p];
      if (METRICS) lab = labels[p];
    }
  };
  fetch_ids(t, ur, ir, y);
  for (; t < n_tiles; t += t_step) {  // wave-uniform
    const int64_t p = t * 64 + lane;
    const int64_t mu = pair_row(ur, n_u), mv = pair_row(ir, n_v);
    const bool known = mu >= 0 && mv >= 0;
    const double yy = y;
    srow[w][0][lane] = mu;
    srow[w][1][lane] = mv;
    fetch_ids(t + t_step, ur, ir, y);
    wave_lds_fence();
    float acc = 0.f;
    for (int c0 = 0; c0 < k; c0 += CW) {
#pragma unroll
      for (int b0 = 0; b0 < NIT; b0 += NB) {
        float4 a[NB], b[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {  // every fetch of the batch issued before the first product
          const int j = (b0 + i) * RPI + r;
          const int64_t ju = srow[w][0][j], jv = srow[w][1][j];
          a[i] = b[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (ju >= 0 && jv >= 0) {
            a[i] = *reinterpret_cast<const float4*>(U + ju * kp + c0 + 4 * q);
            b[i] = *reinterpret_cast<const float4*>(V + jv * kp + c0 + 4 * q);
          }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          float* o = tile + ((b0 + i) * RPI + r) * STR + 4 * q;
          o[0] = a[i].x * b[i].x;
          o[1] = a[i].y * b[i].y;
          o[2] = a[i].z * b[i].z;
          o[3] = a[i].w * b[i].w;
        }
      }
      wave_lds_fence();
      const int kc = k - c0 < CW ? k - c0 : CW;
      const float* __restrict__ mine = tile + lane * STR;
      int c = 0;
      for (; c + 8 <= kc; c += 8) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = mine[c + e];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = acc + x[e];
      }
      for (; c < kc; ++c) acc = acc + mine[c];
      wave_lds_fence();  // the next chunk / tile overwrites the products
    }
    const float pred = known ? acc : __builtin_nanf("");
    if (p < n) {
      if (out) out[p] = pred;
      if (METRICS) {
        if (pred != pred) {
          s[HREC_PAIR_N_NAN] += 1.0;
        } else {
          const double yh = (double)pred, e = yy - yh;
          s[HREC_PAIR_N_OK] += 1.0;
          s[HREC_PAIR_SUM_E] += e;
          s[HREC_PAIR_SUM_ABS_E] += fabs(e);
          s[HREC_PAIR_SUM_E2] += e * e;
          s[HREC_PAIR_SUM_Y] += yy;
          s[HREC_PAIR_SUM_Y2] += yy * yy;
          s[HREC_PAIR_SUM_P] += yh;
          s[HREC_PAIR_SUM_P2] += yh * yh;
          s[HREC_PAIR_SUM_YP] += yy * yh;
        }
      }
    }
  }
  if (!METRICS) return;
  // lanes (xor tree), then the four waves in wave order: a fixed order
#pragma unroll
  for (int i = 0; i < HREC_PAIR_SUMS; ++i) {
#pragma unroll  // written out: wave_xor_sum here changes the generated code
    for (int off = 32; off > 0; off >>= 1) s[i] += __shfl_xor(s[i], off, kWave);
    if (lane == 0) red[w][i] = s[i];
  }
  __syncthreads();
  if (threadIdx.x < HREC_PAIR_SUMS) {
    const int i = threadIdx.x;
    partials[(int64_t)blockIdx.x * HREC_PAIR_SUMS + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

static int pair_chunk(int kp) { return kp == 16 ? 16 : ((kp == 32 || kp == 96) ? 32 : 64); }

// The checks both entries share, then the launch (metrics: labels != null).
static int pairs_run(const char* who, bool metrics, const float* U, int64_t n_u, const float* V, int64_t n_v, int k,
                     int kp, const int64_t* user_rows, const int64_t* item_rows, int64_t n, float* out,
                     const double* labels, double* sums, void* ws, size_t ws_bytes, void* stream) {
  HREC_REQUIRE(hrec_factor_ld_ok(kp), "%s: kp must be 16, 32, 64, 96, 128, 192 or 256 (got kp %d)", who, kp);
  HREC_REQUIRE(k >= 1 && k <= kp, "%s: need 1 <= k <= kp (k=%d kp=%d)", who, k, kp);
  HREC_REQUIRE(n >= 0 && n_u >= 0 && n_v >= 0, "%s: negative size", who);
  if (metrics) {
    HREC_REQUIRE(sums && ws, "%s: null sums or workspace", who);
    const size_t need = hrec_als_pair_metrics_workspace_bytes(n);
    HREC_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", who, ws_bytes, need);
  } else if (n == 0) {
    return HREC_OK;
  }
  if (n > 0) {
    HREC_REQUIRE(user_rows && item_rows && (metrics ? labels != nullptr : out != nullptr), "%s: null pointer", who);
    HREC_REQUIRE((U || n_u == 0) && (V || n_v == 0), "%s: null factors", who);
    HREC_REQUIRE((((uintptr_t)U | (uintptr_t)V) & 15) == 0, "%s: factors must be 16-B aligned", who);
  }
  hipStream_t s = as_stream(stream);
  const int64_t nb = n > 0 ? pair_blocks(n) : 0;
  double* part = static_cast<double*>(ws);
#define HREC_PAIRS(CW, M)                                                                                        \
  hipLaunchKernelGGL((als_pairs_kernel<CW, M>), dim3((unsigned)nb), dim3(kPairBlock), 0, s, U, n_u, V, n_v, k, kp, \
                     user_rows, item_rows, n, out, labels, part)
  if (nb > 0) {
    const int cw = pair_chunk(kp);
    if (metrics) {
      if (cw == 16) HREC_PAIRS(16, true);
      else if (cw == 32) HREC_PAIRS(32, true);
      else HREC_PAIRS(64, true);
    } else {
      if (cw == 16) HREC_PAIRS(16, false);
      else if (cw == 32) HREC_PAIRS(32, false);
      else HREC_PAIRS(64, false);
    }
  }
#undef HREC_PAIRS
  if (metrics)
    hipLaunchKernelGGL(pairs_reduce_kernel, dim3(1), dim3(64 * HREC_PAIR_SUMS), 0, s, part, nb, sums);
  return check_launch("als_pairs_kernel");
}

}  // namespace hrec

using namespace hrec;

extern "C" int hrec_als_predict_pairs(const float* user_factors, int64_t n_user_rows, const float* item_factors,
                                      int64_t n_item_rows, int k, int kp, const int64_t* user_rows,
                                      const int64_t* item_rows, int64_t n, float* out, void* stream) {
  return pairs_run("als_predict_pairs", false, user_factors, n_user_rows, item_factors, n_item_rows, k, kp,
                   user_rows, item_rows, n, out, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" size_t hrec_als_pair_metrics_workspace_bytes(int64_t n) {
  return al256((size_t)pair_blocks(n > 0 ? n : 0) * HREC_PAIR_SUMS * sizeof(double));
}

extern "C" int hrec_als_pair_metrics(const float* user_factors, int64_t n_user_rows, const float* item_factors,
                                     int64_t n_item_rows, int k, int kp, const int64_t* user_rows,
                                     const int64_t* item_rows, int64_t n, const double* labels, float* pred_out,
                                     double* sums_out, void* workspace, size_t workspace_bytes, void* stream) {
  return pairs_run("als_pair_metrics", true, user_factors, n_user_rows, item_factors, n_item_rows, k, kp, user_rows,
                   item_rows, n, pred_out, labels, sums_out, workspace, workspace_bytes, stream);
}
