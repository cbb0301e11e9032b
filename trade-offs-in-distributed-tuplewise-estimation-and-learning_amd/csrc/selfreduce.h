// selfreduce.h — the fixed-order block sums and per-shard reduce shared by the kernels whose
// blocks leave one partial each in d_work (selfpairs.hip, triplets.hip): a wave butterfly, the
// four wave sums added in a fixed order, then one block per shard adding that shard's partials
// lane-strided in a fixed order.  No atomics and nothing to zero: results do not depend on
// scheduling.
#pragma once
#include "tw_common.h"
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

}  // namespace tw
