// What the pair kernels (csrc/als_pairs.hip, csrc/tt_pairs.hip) share: the
// launch shape, the row-index check and the fixed-order reduction of the
// metrics partials (the wave-level LDS ordering is wave_lds_fence of wave.h).
#pragma once

#include "wave.h"

namespace hrec {

constexpr int kPairBlock = 256;        // 4 waves, one tile of 64 pairs each per step
constexpr int kPairMaxBlocks = 2048;   // grid cap: the tiles beyond are taken in grid strides
constexpr int kPairBatch = 8;          // row fetches per side in flight per lane (at most)

// Blocks of a launch over n pairs: a function of n alone, so the partial sums
// of the metrics mode have one layout (and one summation order) per n.
__host__ __device__ inline int64_t pair_blocks(int64_t n) {
  const int64_t b = (n + kPairBlock - 1) / kPairBlock;
  return b < 1 ? 1 : (b > kPairMaxBlocks ? kPairMaxBlocks : b);
}

// A row index as the kernel uses it: itself when inside [0, n_rows), else -1.
__device__ __forceinline__ int64_t pair_row(int64_t r, int64_t n_rows) {
  return (uint64_t)r < (uint64_t)n_rows ? r : -1;
}

// sums[i] = the blocks' partials of slot i: wave i, lane l adds blocks l,
// l + 64, ... in ascending order, then the lanes' xor tree. (static: one copy
// per including source, each registered with its own code object.)
static __global__ __launch_bounds__(64 * HREC_PAIR_SUMS) void pairs_reduce_kernel(const double* __restrict__ partials,
                                                                                 int64_t n_blocks,
                                                                                 double* __restrict__ sums) {
  const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;
  double v = 0.0;
  for (int64_t b = lane; b < n_blocks; b += 64) v += partials[b * HREC_PAIR_SUMS + i];
  v = wave_xor_sum(v);
  if (lane == 0) sums[i] = v;
}

}  // namespace hrec
