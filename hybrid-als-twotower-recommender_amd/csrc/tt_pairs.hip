// K8p: two-tower scores for a list of (user row, item row) pairs and, fused,
// the sums behind the regression metrics (rmse / mse / mae / r2 / var).
//
//   out[p] = <user_vec[user_rows[p]], item_vec[item_rows[p]]>
//
// in the one order of every two-tower score (tt_chain_dot, csrc/tt.hip): an
// fmaf chain from 0.f over k = k0 + 4 g + e (steps of 16, g fastest) for d in
// {32, 64, 128, 256} and over k = 0 .. d-1 for any other d, so a pair has the
// bits hrec_tt_pair_score / hrec_tt_score give it. A row index outside
// [0, n_rows) on either side gives a quiet NaN and is never turned into an
// address (one unsigned compare per side).
//
// Shape (csrc/als_pairs.hip's): a row gather without reuse, two d-float rows
// per pair. One wave owns a tile of 64 pairs. The chain of a pair cannot be
// split across lanes, the loads can: kTTPairChunk / VW lanes x VW floats fetch
// one 128-B piece of a row, so one wave-instruction fetches 64 / (32 / VW) row
// pieces in full lines, and kPairBatch such instructions per side are in
// flight before the first LDS write. The chain is fmaf(u, v, acc) - the
// product is never rounded - so the tile holds BOTH rows' pieces (a tile of
// products, as the ALS kernel keeps, would have other bits): [2 sides][64
// pairs][32 + 1] floats per wave, the odd row stride putting lane l's walk
// over its own pair's rows on bank (l + c) mod 32. Each lane then runs its
// pair's chain over the chunk in chain order; the sum is carried in a register
// across the chunks of a wider row (in the permuted order a chunk is two whole
// steps of 16). A workgroup of 4 waves holds 67,584 B of tiles + 4 KiB of row
// indices: two workgroups = 8 waves per CU, 16 KiB of fetches in flight each.
//
// Rows are d floats without padding, so they are 16-B aligned only when
// d % 4 == 0. VW, the load width in floats, is the largest of 4, 2, 1 that
// divides d: every row then starts on a VW * 4-byte boundary, every vector
// lies inside its row (never past column d of a matrix's last row), and no
// load is misaligned.
#include "pairs.h"

namespace hrec {

constexpr int kTTPairChunk = 32;  // columns per chunk: one 128-B line of each row

// tt_dot_order of csrc/tt.hip: the widths whose chain runs in the permuted order.
__host__ __device__ inline bool tt_pairs_permuted(int d) { return d == 32 || d == 64 || d == 128 || d == 256; }

template <int VW>
struct PairVec {
  float x[VW];
};
template <int VW>
__device__ __forceinline__ PairVec<VW> pair_vec_load(const float* __restrict__ p);
template <>
__device__ __forceinline__ PairVec<4> pair_vec_load<4>(const float* __restrict__ p) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  return {{v.x, v.y, v.z, v.w}};
}
template <>
__device__ __forceinline__ PairVec<2> pair_vec_load<2>(const float* __restrict__ p) {
  const float2 v = *reinterpret_cast<const float2*>(p);
  return {{v.x, v.y}};
}
template <>
__device__ __forceinline__ PairVec<1> pair_vec_load<1>(const float* __restrict__ p) {
  return {{*p}};
}

// VW: floats per load (4, 2 or 1; d is a multiple of it). METRICS: also the
// f64 sums of the pairs with a prediction (label - prediction), one partial
// of HREC_PAIR_SUMS doubles per block in `partials`; out may be null.
template <int VW, bool METRICS>
__global__ __launch_bounds__(kPairBlock) void tt_pairs_kernel(
    const float* __restrict__ U, int64_t n_u, const float* __restrict__ V, int64_t n_v, int d,
    const int64_t* __restrict__ user_rows, const int64_t* __restrict__ item_rows, int64_t n,
    float* __restrict__ out, const double* __restrict__ labels, double* __restrict__ partials) {
  constexpr int CW = kTTPairChunk;
  constexpr int LPR = CW / VW;   // lanes per row piece
  constexpr int RPI = 64 / LPR;  // row pieces per wave-instruction
  constexpr int NIT = LPR;       // instructions per side that cover the tile's 64 rows
  constexpr int NB = NIT < kPairBatch ? NIT : kPairBatch;
  constexpr int STR = CW + 1;    // odd row stride (dwords)
  __shared__ float piece[4][2][64 * STR];
  __shared__ int64_t srow[4][2][64];
  __shared__ double red[METRICS ? 4 : 1][HREC_PAIR_SUMS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane / LPR, q = lane % LPR;
  float* __restrict__ tu = piece[w][0];
  float* __restrict__ tv = piece[w][1];
  const bool permuted = tt_pairs_permuted(d);
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
    for (int c0 = 0; c0 < d; c0 += CW) {
      const int col = c0 + VW * q;  // this lane's first column; VW divides d, so col < d covers the vector
#pragma unroll
      for (int b0 = 0; b0 < NIT; b0 += NB) {
        PairVec<VW> a[NB], b[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {  // every fetch of the batch issued before the first LDS write
          const int j = (b0 + i) * RPI + r;
          const int64_t ju = srow[w][0][j], jv = srow[w][1][j];
#pragma unroll
          for (int e = 0; e < VW; ++e) a[i].x[e] = b[i].x[e] = 0.f;
          if (col < d && ju >= 0 && jv >= 0) {
            a[i] = pair_vec_load<VW>(U + ju * d + col);
            b[i] = pair_vec_load<VW>(V + jv * d + col);
          }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const int o = ((b0 + i) * RPI + r) * STR + VW * q;
#pragma unroll
          for (int e = 0; e < VW; ++e) {
            tu[o + e] = a[i].x[e];
            tv[o + e] = b[i].x[e];
          }
        }
      }
      wave_lds_fence();
      const float* __restrict__ xu = tu + lane * STR;
      const float* __restrict__ xv = tv + lane * STR;
      if (permuted) {  // d is a multiple of CW: two whole steps of 16 per chunk
#pragma unroll
        for (int k0 = 0; k0 < CW; k0 += 16) {
          float x[16], z[16];
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            x[c] = xu[k0 + c];
            z[c] = xv[k0 + c];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc = fmaf(x[4 * g + e], z[4 * g + e], acc);
        }
      } else {
        const int kc = d - c0 < CW ? d - c0 : CW;
        int c = 0;
        for (; c + 8 <= kc; c += 8) {
          float x[8], z[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            x[e] = xu[c + e];
            z[e] = xv[c + e];
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) acc = fmaf(x[e], z[e], acc);
        }
        for (; c < kc; ++c) acc = fmaf(xu[c], xv[c], acc);
      }
      wave_lds_fence();  // the next chunk / tile overwrites the pieces
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

static int tt_pair_width(int d) { return d % 4 == 0 ? 4 : (d % 2 == 0 ? 2 : 1); }

// The checks both entries share, then the launch (metrics: labels != null).
static int tt_pairs_run(const char* who, bool metrics, const float* U, int64_t n_u, const float* V, int64_t n_v, int d,
                        const int64_t* user_rows, const int64_t* item_rows, int64_t n, float* out,
                        const double* labels, double* sums, void* ws, size_t ws_bytes, void* stream) {
  HREC_REQUIRE(d >= 1 && d <= 256, "%s: need 1 <= d <= 256 (got d %d)", who, d);
  HREC_REQUIRE(n >= 0 && n_u >= 0 && n_v >= 0, "%s: negative size", who);
  if (metrics) {
    HREC_REQUIRE(sums && ws, "%s: null sums or workspace", who);
    const size_t need = hrec_tt_pair_metrics_workspace_bytes(n);
    HREC_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", who, ws_bytes, need);
  } else if (n == 0) {
    return HREC_OK;
  }
  const int vw = tt_pair_width(d);
  if (n > 0) {
    HREC_REQUIRE(user_rows && item_rows && (metrics ? labels != nullptr : out != nullptr), "%s: null pointer", who);
    HREC_REQUIRE((U || n_u == 0) && (V || n_v == 0), "%s: null vectors", who);
    HREC_REQUIRE((((uintptr_t)U | (uintptr_t)V) & (uintptr_t)(4 * vw - 1)) == 0,
                 "%s: vectors of width %d must be %d-B aligned", who, d, 4 * vw);
  }
  hipStream_t s = as_stream(stream);
  const int64_t nb = n > 0 ? pair_blocks(n) : 0;
  double* part = static_cast<double*>(ws);
#define HREC_TT_PAIRS(VW, M)                                                                                      \
  hipLaunchKernelGGL((tt_pairs_kernel<VW, M>), dim3((unsigned)nb), dim3(kPairBlock), 0, s, U, n_u, V, n_v, d, \
                     user_rows, item_rows, n, out, labels, part)
  if (nb > 0) {
    if (metrics) {
      if (vw == 4) HREC_TT_PAIRS(4, true);
      else if (vw == 2) HREC_TT_PAIRS(2, true);
      else HREC_TT_PAIRS(1, true);
    } else {
      if (vw == 4) HREC_TT_PAIRS(4, false);
      else if (vw == 2) HREC_TT_PAIRS(2, false);
      else HREC_TT_PAIRS(1, false);
    }
  }
#undef HREC_TT_PAIRS
  if (metrics) hipLaunchKernelGGL(pairs_reduce_kernel, dim3(1), dim3(64 * HREC_PAIR_SUMS), 0, s, part, nb, sums);
  return check_launch("tt_pairs_kernel");
}

}  // namespace hrec

using namespace hrec;

extern "C" int hrec_tt_predict_pairs(const float* user_vec, int64_t n_user_rows, const float* item_vec,
                                     int64_t n_item_rows, int d, const int64_t* user_rows, const int64_t* item_rows,
                                     int64_t n, float* out, void* stream) {
  return tt_pairs_run("tt_predict_pairs", false, user_vec, n_user_rows, item_vec, n_item_rows, d, user_rows,
                      item_rows, n, out, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" size_t hrec_tt_pair_metrics_workspace_bytes(int64_t n) {
  return al256((size_t)pair_blocks(n > 0 ? n : 0) * HREC_PAIR_SUMS * sizeof(double));
}

extern "C" int hrec_tt_pair_metrics(const float* user_vec, int64_t n_user_rows, const float* item_vec,
                                    int64_t n_item_rows, int d, const int64_t* user_rows, const int64_t* item_rows,
                                    int64_t n, const double* labels, float* pred_out, double* sums_out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  return tt_pairs_run("tt_pair_metrics", true, user_vec, n_user_rows, item_vec, n_item_rows, d, user_rows, item_rows,
                      n, pred_out, labels, sums_out, workspace, workspace_bytes, stream);
}
