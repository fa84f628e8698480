// The two-tower row arithmetic that more than one source must round alike:
// the Keras LayerNormalization of one row by one wave (csrc/tt.hip's towers
// and backward saves, csrc/tt_fold_in.hip's per-user fit) and one element of
// Keras' sparse Adam step.
#pragma once

#include "wave.h"  // wave_xor_sum

namespace hrec {

constexpr float kLnEps = 1e-3f;

// LayerNorm of one row held in LDS (length d), one wave. Writes y (and the
// normalised row + 1/std when save != nullptr).
__device__ __forceinline__ void ln_row(const float* __restrict__ x, int d, const float* __restrict__ gamma,
                                       const float* __restrict__ beta, float* __restrict__ y,
                                       float* __restrict__ xhat_out, float* __restrict__ rstd_out, int lane) {
  float s = 0.f;
  for (int c = lane; c < d; c += kWave) s += x[c];
  const float mean = wave_xor_sum(s) / (float)d;
  float q = 0.f;
  for (int c = lane; c < d; c += kWave) {
    const float t = x[c] - mean;
    q += t * t;
  }
  const float var = wave_xor_sum(q) / (float)d;
  const float rstd = 1.0f / sqrtf(var + kLnEps);
  for (int c = lane; c < d; c += kWave) {
    const float xh = (x[c] - mean) * rstd;
    y[c] = xh * gamma[c] + beta[c];
    if (xhat_out) xhat_out[c] = xh;
  }
  if (rstd_out && lane == 0) *rstd_out = rstd;
}

// ln_row for a row held in registers: element i of a lane is column
// lane + 64 i (on[i]: that column is < d; gamma / beta hold the same columns).
// The same expressions in the same order: a lane's partial sums add its
// columns ascending, as ln_row's lane-strided loops do. Returns 1/std.
template <int NE>
__device__ __forceinline__ float ln_regs(const float (&x)[NE], const bool (&on)[NE], int d, const float (&gamma)[NE],
                                         const float (&beta)[NE], float (&y)[NE], float (&xhat)[NE]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NE; ++i)
    if (on[i]) s += x[i];
  const float mean = wave_xor_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NE; ++i)
    if (on[i]) {
      const float t = x[i] - mean;
      q += t * t;
    }
  const float var = wave_xor_sum(q) / (float)d;
  const float rstd = 1.0f / sqrtf(var + kLnEps);
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const float xh = (x[i] - mean) * rstd;
    xhat[i] = on[i] ? xh : 0.f;
    y[i] = on[i] ? xh * gamma[i] + beta[i] : 0.f;
  }
  return rstd;
}

// One element of the whole-table Adam step (has_g: the row is in the batch;
// g its summed gradient). The two fma are spelled out so every kernel that
// updates a row (the sweep, the touched-rows kernel of the phased form, the
// fold-in fit) rounds it identically.
__device__ __forceinline__ void adam_elem(float& m, float& v, float& x, float g, bool has_g, float lr, float b1,
                                          float omb1, float b2, float omb2, float eps) {
  float me = m * b1;
  float ve = v * b2;
  if (has_g) {
    me = __builtin_fmaf(g, omb1, me);
    ve = __builtin_fmaf(g * g, omb2, ve);
  }
  m = me;
  v = ve;
  x = x - (lr * me) / (sqrtf(ve) + eps);
}

}  // namespace hrec
