// selfreduce.h — the fixed-order block sums and per-shard reduce shared by the kernels whose
// blocks leave one partial each in d_work (selfpairs.hip, triplets.hip, mmd.hip): a wave
// butterfly, the four wave sums added in a fixed order, then one block per shard adding that
// shard's partials lane-strided in a fixed order.  No atomics and nothing to zero: results do
// not depend on scheduling.  Also the triangle index of the kernels that walk each unordered
// pair of tiles once (selfpairs.hip, mmd.hip).
#pragma once
#include "tw_common.h"
#include <cmath>
#include <type_traits>

namespace tw {

__device__ __forceinline__ double self_block_sum_f64(double v, double* part) {
  v = wave_sum_f64(v);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  __syncthreads();  // part's previous readers
  if (lane == 0) part[wid] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

__device__ __forceinline__ unsigned long long self_block_sum_u64(unsigned long long v,
                                                                 unsigned long long* part) {
  v = wave_sum_u64(v);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  __syncthreads();
  if (lane == 0) part[wid] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// out[s][k] = ordered sum of work[s * per + i][k], i < per: one block per shard, lane-strided
// partial sums in a fixed order, then the fixed butterfly and wave order of the block sums.
template <typename A, int W>
__global__ __launch_bounds__(kBlock) void k_self_reduce(const A* __restrict__ work, int per,
                                                        A* __restrict__ out) {
  __shared__ unsigned long long part[kBlock / kWave];
  const A* __restrict__ w = work + (int64_t)blockIdx.x * per * W;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    A v = A(0);
#pragma unroll 4
    for (int i = threadIdx.x; i < per; i += kBlock) v += w[(int64_t)i * W + k];
    A b;
    if constexpr (std::is_floating_point<A>::value) b = self_block_sum_f64(v, (double*)part);
    else b = self_block_sum_u64(v, part);
    if (threadIdx.x == 0) out[(int64_t)blockIdx.x * W + k] = b;
  }
}

// Triangle index p = J (J + 1) / 2 + I, I <= J, back to (I, J): the double root is exact
// enough to land within one of J for every p < 2^52, the two loops settle it.
__device__ __forceinline__ void self_tile_of(int64_t p, int& I, int& J) {
  int64_t j = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while (j * (j + 1) / 2 > p) --j;
  while ((j + 1) * (j + 2) / 2 <= p) ++j;
  J = (int)j;
  I = (int)(p - j * (j + 1) / 2);
}

}  // namespace tw
