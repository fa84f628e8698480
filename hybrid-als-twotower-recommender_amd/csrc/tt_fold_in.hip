// K6f: fold users into the two-tower model. Each row of emb is fitted to its
// own rating history with every other variable frozen: what model.fit does
// to that embedding row when the user's whole history is one batch per step.
//
//   per step   u     = LN_u(e)                          (ln_regs: ln_row's arithmetic)
//              err_j = <u, item_vec[row_j]> - r_j       over the usable entries, CSR order
//              du    = (2 / n) sum_j err_j item_vec[row_j]
//              g     = rstd (dxh - mean(dxh) - xh mean(dxh xh)),  dxh = du gamma   (tt_backward_kernel's)
//              e     = Keras' sparse Adam step of a row touched at every step, from m = v = 0 (adam_elem)
//
// One user's row depends on no other user's, so a batch of users is one
// launch: one wave per user, four waves per 256-thread block, no LDS, no
// atomics. A lane holds columns lane, lane + 64, .. of e, m, v, gamma, beta
// (NE = ceil(d / 64) <= 4 registers each), so a row of item_vec is one
// coalesced lane-strided load per 64 columns. The history is walked 64
// entries at a time: each lane reads one (item row, rating), a ballot marks
// the entries with 0 <= item row < n_items - the others are skipped and never
// turned into an address - and the marked ones are taken four at a time in
// CSR order, their four rows loaded before the first dot so the loads overlap.
// Every sum has a fixed order (columns ascending inside a lane, then the xor
// butterfly of wave_xor_sum; entries in CSR order), so equal inputs give equal
// bits. The item vectors of a user are re-read from the caches at every step
// (a short history is a few KiB); staging them in LDS was not tried. Not tuned.
#include "tt_ln.h"

namespace hrec {

constexpr int kFoldWaves = 4;  // users per block
constexpr int kFoldGroup = 4;  // history entries whose rows are in flight together

template <int NE>
__global__ __launch_bounds__(kFoldWaves* kWave) void tt_fold_in_kernel(
    float* __restrict__ emb, int64_t n_rows, int d, const float* __restrict__ ln_gamma,
    const float* __restrict__ ln_beta, const float* __restrict__ item_vec, int64_t n_items,
    const int64_t* __restrict__ indptr, const int64_t* __restrict__ item_rows, const float* __restrict__ ratings,
    int steps, const float* __restrict__ step_lr, float b1, float omb1, float b2, float omb2, float eps,
    float* __restrict__ out_loss) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * kFoldWaves + (threadIdx.x >> 6);
  if (u >= n_rows) return;  // wave-uniform
  const int64_t p0 = indptr[u], p1 = indptr[u + 1];
  int64_t n = 0;  // usable entries
  for (int64_t p = p0; p < p1; p += kWave) {
    const int64_t q = p + lane;
    const bool ok = q < p1 && (uint64_t)item_rows[q] < (uint64_t)n_items;
    n += __popcll(__ballot(ok));
  }
  if (n == 0) {  // the row stays as it is
    if (out_loss && lane == 0) out_loss[2 * u] = out_loss[2 * u + 1] = __builtin_nanf("");
    return;
  }
  float e[NE], gam[NE], bet[NE], m[NE], v[NE];
  bool on[NE];
  float* __restrict__ row = emb + u * d;
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int c = lane + kWave * i;
    on[i] = c < d;
    e[i] = on[i] ? row[c] : 0.f;
    gam[i] = on[i] ? ln_gamma[c] : 0.f;
    bet[i] = on[i] ? ln_beta[c] : 0.f;
    m[i] = v[i] = 0.f;
  }
  const float fn = (float)n, scale = 2.0f / fn;
  float loss0 = 0.f, loss = 0.f;
  for (int t = 0;; ++t) {
    float uv[NE], xh[NE], du[NE];
    const float rstd = ln_regs<NE>(e, on, d, gam, bet, uv, xh);
#pragma unroll
    for (int i = 0; i < NE; ++i) du[i] = 0.f;
    float sq = 0.f;
    const bool last = t >= steps;  // wave-uniform: the pass after the last step needs the loss alone
    for (int64_t p = p0; p < p1; p += kWave) {
      const int64_t q = p + lane;
      int64_t ir = -1;
      float rt = 0.f;
      if (q < p1) {
        ir = item_rows[q];
        rt = ratings[q];
      }
      uint64_t todo = __ballot((uint64_t)ir < (uint64_t)n_items);
      while (todo) {  // wave-uniform
        int src[kFoldGroup], cnt = 0;
#pragma unroll
        for (int g = 0; g < kFoldGroup; ++g) {
          if (todo) {
            src[g] = __builtin_ctzll(todo);
            todo &= todo - 1;
            ++cnt;
          } else {
            src[g] = src[0];  // a usable entry again: loaded, not used
          }
        }
        float vr[kFoldGroup][NE], dot[kFoldGroup], rr[kFoldGroup];
#pragma unroll
        for (int g = 0; g < kFoldGroup; ++g) {
          const int64_t r = lane_read(ir, src[g]);
          const float* __restrict__ vp = item_vec + r * d;
          rr[g] = lane_read(rt, src[g]);
#pragma unroll
          for (int i = 0; i < NE; ++i) vr[g][i] = on[i] ? vp[lane + kWave * i] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < kFoldGroup; ++g) {
          float s = 0.f;
#pragma unroll
          for (int i = 0; i < NE; ++i) s = fmaf(uv[i], vr[g][i], s);
          dot[g] = s;
        }
#pragma unroll
        for (int g = 0; g < kFoldGroup; ++g) dot[g] = wave_xor_sum(dot[g]);
#pragma unroll
        for (int g = 0; g < kFoldGroup; ++g) {
          if (g < cnt) {
            const float err = dot[g] - rr[g];
            sq += err * err;
            if (!last) {
#pragma unroll
              for (int i = 0; i < NE; ++i) du[i] += err * vr[g][i];
            }
          }
        }
      }
    }
    loss = sq / fn;
    if (t == 0) loss0 = loss;
    if (last) break;
    // LayerNorm backward, then the row's Adam step
    float m1 = 0.f, m2 = 0.f;
    float dxh[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      dxh[i] = (scale * du[i]) * gam[i];
      if (on[i]) {
        m1 += dxh[i];
        m2 += dxh[i] * xh[i];
      }
    }
    m1 = wave_xor_sum(m1) / (float)d;
    m2 = wave_xor_sum(m2) / (float)d;
    const float lr = step_lr[t];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const float g = rstd * (dxh[i] - m1 - xh[i] * m2);
      if (on[i]) adam_elem(m[i], v[i], e[i], g, true, lr, b1, omb1, b2, omb2, eps);
    }
  }
  if (steps > 0) {
#pragma unroll
    for (int i = 0; i < NE; ++i)
      if (on[i]) row[lane + kWave * i] = e[i];
  }
  if (out_loss && lane == 0) {
    out_loss[2 * u] = loss0;
    out_loss[2 * u + 1] = loss;
  }
}

}  // namespace hrec

using namespace hrec;

extern "C" int hrec_tt_fold_in_users(float* emb, int64_t n_rows, int d, const float* ln_gamma, const float* ln_beta,
                                     const float* item_vec, int64_t n_items, const int64_t* indptr,
                                     const int64_t* item_rows, const float* ratings, int steps, const float* step_lr,
                                     float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                                     float epsilon, float* out_loss, void* stream) {
  HREC_REQUIRE(d >= 1 && d <= 256, "tt_fold_in_users: need 1 <= d <= 256 (got d %d)", d);
  HREC_REQUIRE(n_rows >= 0 && n_items >= 0 && steps >= 0, "tt_fold_in_users: negative size");
  if (n_rows == 0) return HREC_OK;
  HREC_REQUIRE(emb && ln_gamma && ln_beta && indptr && item_rows && ratings && (step_lr || steps == 0),
               "tt_fold_in_users: null pointer");
  HREC_REQUIRE(item_vec || n_items == 0, "tt_fold_in_users: null vectors");
  const int vw = d % 4 == 0 ? 4 : (d % 2 == 0 ? 2 : 1);  // hrec_tt_predict_pairs' rule
  HREC_REQUIRE((((uintptr_t)emb | (uintptr_t)item_vec) & (uintptr_t)(4 * vw - 1)) == 0,
               "tt_fold_in_users: rows of width %d must be %d-B aligned", d, 4 * vw);
  const int64_t nb = (n_rows + kFoldWaves - 1) / kFoldWaves;
  HREC_REQUIRE(nb < (1ll << 31), "tt_fold_in_users: grid too large");
  hipStream_t s = as_stream(stream);
#define HREC_TT_FOLD_IN(NE)                                                                                       \
  hipLaunchKernelGGL(tt_fold_in_kernel<NE>, dim3((unsigned)nb), dim3(kFoldWaves* kWave), 0, s, emb, n_rows, d,   \
                     ln_gamma, ln_beta, item_vec, n_items, indptr, item_rows, ratings, steps, step_lr, beta1,     \
                     one_minus_beta1, beta2, one_minus_beta2, epsilon, out_loss)
  switch ((d + kWave - 1) / kWave) {
    case 1: HREC_TT_FOLD_IN(1); break;
    case 2: HREC_TT_FOLD_IN(2); break;
    case 3: HREC_TT_FOLD_IN(3); break;
    default: HREC_TT_FOLD_IN(4); break;
  }
#undef HREC_TT_FOLD_IN
  return check_launch("tt_fold_in_kernel");
}
