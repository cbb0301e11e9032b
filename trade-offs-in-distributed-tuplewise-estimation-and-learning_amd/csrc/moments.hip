// moments.hip — exact integer moments of the per-point pair counts.
//
// For one shard with n scores x and m scores z, g_ij = 1{x_i > z_j} (TW_PRED_GT) or
// 2*1{x_i > z_j} + 1{x_i == z_j} (TW_PRED_HALF, half-units), a_i = sum_j g_ij, b_j = sum_i g_ij:
//   S = sum a_i,  A2 = sum a_i^2,  B2 = sum b_j^2,  Q = sum g_ij^2      (u64, all exact)
// from which the host forms DeLong's components and the variance of Un, UnN and UnNT
// (estimation.VarianceComponents).  NumPy's comparison semantics as in count.hip /
// rankcount.hip: a NaN on either side compares false, -0 == +0, int64 compared as integers.
//
// One block owns one (shard, side, tile): a tile of x-values whose a_i it forms against the
// shard's z, or a tile of z-values whose b_j it forms against the shard's x.  Two ways to the
// same integers:
//   all pairs  (k_moments_pairs): a lane keeps 4 values of its side in registers and loops over
//     the other side from LDS with the native compare of the scores' own type;
//   sorted     (k_moments_sort + k_moments_search): both sides of every shard are sorted in
//     chunks of C <= 4096 order keys (sortkeys.h: the bitonic network of rankcount.hip), and a
//     lane binary-searches its 4 keys in every sorted chunk of the other side staged in LDS:
//       lo = #{keys < k}, hi = #{keys <= k} among the chunk's non-NaN scores,
//       x side: #{z < x} = sum lo, #{z <= x} = sum hi;
//       z side: #{x > z} = V - sum hi, #{x >= z} = V - sum lo,  V = the shard's non-NaN x.
//     A chunk's NaN scores and its padding both carry the top key; V's share of a chunk is one
//     more search (doubles: #{keys < top}) or the chunk's length (int64 has no NaN, and the
//     clamp hi <= V keeps the padding out when a score is INT64_MAX, whose key is the top key).
// Either way the lane squares its counts in u64, a wave butterfly and one LDS pass give the
// block's partial sums, and one integer atomic per sum adds them to the shard's row: integer
// addition commutes, so the result does not depend on the order the blocks arrive in.
#include "sortkeys.h"
#include <algorithm>
#include <type_traits>

namespace tw {

constexpr int kMomPer = 4;                                // values of its own side per lane
constexpr int kMomPairThreads = 256;
constexpr int kMomPairTile = kMomPairThreads * kMomPer;   // own values per all-pairs block
constexpr int kMomPairStage = 2048;                       // other side's values per LDS stage
constexpr int kMomSearchTile = kSortThreads * kMomPer;    // own values per search block
constexpr int64_t kMomMaxC = 4096;                        // sorted chunk (keys), a power of two
constexpr int kMomMaxGroup = (int)(kMaxChunk / 1024);     // chunks staged at once, at most

static int g_moments_algo = 0;  // tw_pair_moments_set_algo

// (shard, side, tile) of a block; side 0 = the block owns x-values, 1 = z-values
struct MomBlock {
  int s, side, t;
};
__device__ __forceinline__ MomBlock mom_block(int tiles) {
  const int lb = xcd_block(blockIdx.x, gridDim.x);  // a shard's blocks share one L2
  MomBlock b;
  b.s = lb / (2 * tiles);
  const int r = lb - b.s * 2 * tiles;
  b.side = r / tiles;
  b.t = r - b.side * tiles;
  return b;
}

// Block sums of (cnt, cnt^2, q) added to the shard's row {S, A2, B2, Q}: the x side feeds S, A2
// and Q, the z side B2.
__device__ __forceinline__ void mom_commit(unsigned long long c, unsigned long long c2,
                                           unsigned long long q, int side,
                                           unsigned long long* __restrict__ row) {
  __shared__ unsigned long long part[3][kSortThreads / kWave];
  c = wave_sum_u64(c);
  c2 = wave_sum_u64(c2);
  q = wave_sum_u64(q);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) {
    part[0][wid] = c;
    part[1][wid] = c2;
    part[2][wid] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0, b = 0, d = 0;
    const int nw = blockDim.x / kWave;
    for (int w = 0; w < nw; ++w) {
      a += part[0][w];
      b += part[1][w];
      d += part[2][w];
    }
    if (side == 0) {
      if (a) atomicAdd(row + 0, a);
      if (b) atomicAdd(row + 1, b);
      if (d) atomicAdd(row + 3, d);
    } else if (b) {
      atomicAdd(row + 2, b);
    }
  }
}

// ------------------------------------------------------------------------------ all pairs
template <typename T, int PRED>
__global__ __launch_bounds__(kMomPairThreads) void k_moments_pairs(
    const T* __restrict__ x, const int64_t* __restrict__ x_off, const T* __restrict__ z,
    const int64_t* __restrict__ z_off, int tiles, unsigned long long* __restrict__ out) {
  __shared__ T stage[kMomPairStage];
  const MomBlock b = mom_block(tiles);
  const bool zs = b.side != 0;
  const T* own = zs ? z : x;
  const T* oth = zs ? x : z;
  const int64_t sb = zs ? z_off[b.s] : x_off[b.s], se = zs ? z_off[b.s + 1] : x_off[b.s + 1];
  const int64_t ob = zs ? x_off[b.s] : z_off[b.s], oe = zs ? x_off[b.s + 1] : z_off[b.s + 1];
  const int64_t i0 = sb + (int64_t)b.t * kMomPairTile;
  if (i0 >= se || ob >= oe) return;  // block-uniform
  T v[kMomPer];
  bool in[kMomPer];
  uint32_t gt[kMomPer], eq[kMomPer];
#pragma unroll
  for (int e = 0; e < kMomPer; ++e) {
    const int64_t i = i0 + e * kMomPairThreads + threadIdx.x;
    in[e] = i < se;
    v[e] = in[e] ? own[i] : (T)0;
    gt[e] = eq[e] = 0;
  }
  for (int64_t o0 = ob; o0 < oe; o0 += kMomPairStage) {
    const int cnt = (int)std::min<int64_t>(kMomPairStage, oe - o0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += kMomPairThreads) stage[j] = oth[o0 + j];
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const T o = stage[j];  // one address for the whole wave: an LDS broadcast
#pragma unroll
      for (int e = 0; e < kMomPer; ++e) {
        gt[e] += zs ? (o > v[e]) : (v[e] > o);
        if (PRED == TW_PRED_HALF) eq[e] += (o == v[e]);
      }
    }
  }
  unsigned long long c = 0, c2 = 0, q = 0;
#pragma unroll
  for (int e = 0; e < kMomPer; ++e) {
    if (!in[e]) continue;
    const unsigned long long a =
        PRED == TW_PRED_HALF ? 2ull * gt[e] + eq[e] : (unsigned long long)gt[e];
    c += a;
    c2 += a * a;
    q += PRED == TW_PRED_HALF ? 4ull * gt[e] + eq[e] : a;
  }
  mom_commit(c, c2, q, b.side, out + 4 * (int64_t)b.s);
}

// ------------------------------------------------------------------------------ sorted
// First sorted chunk of (shard s, side): chunk slots are dealt by position,
//   p(s) = floor((x_off[s] - x_off[0]) / C) + floor((z_off[s] - z_off[0]) / C) + 2 s,
// x's chunks first, then z's.  Whatever the mix of sizes, p(s + 1) - p(s) >= floor(nx / C) +
// floor(nz / C) + 2 >= the ceil(nx / C) + ceil(nz / C) slots shard s needs, and all shards take
// at most total_nx / C + total_nz / C + 2 n_shards slots (tw_pair_moments_work_bytes).
__device__ __forceinline__ int64_t mom_first_chunk(const int64_t* __restrict__ x_off,
                                                   const int64_t* __restrict__ z_off, int s,
                                                   int side, int C) {
  int64_t p = (x_off[s] - x_off[0]) / C + (z_off[s] - z_off[0]) / C + 2 * (int64_t)s;
  if (side) p += (x_off[s + 1] - x_off[s] + C - 1) / C;
  return p;
}

// One block per (shard, side, chunk): the chunk's order keys sorted into the workspace.
template <typename T>
__global__ __launch_bounds__(kSortThreads) void k_moments_sort(
    const T* __restrict__ x, const int64_t* __restrict__ x_off, const T* __restrict__ z,
    const int64_t* __restrict__ z_off, int chunks, int C, uint64_t* __restrict__ sorted) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  const int s = blockIdx.x / (2 * chunks);
  const int r = blockIdx.x - s * 2 * chunks;
  const int side = r / chunks;
  const int c = r - side * chunks;
  const T* own = side ? z : x;
  const int64_t* off = side ? z_off : x_off;
  const int64_t sb = off[s], se = off[s + 1];
  const int64_t c0 = sb + (int64_t)c * C;
  if (c0 >= se) return;  // block-uniform: the searches never read a chunk past the shard's end
  const int nthr = blockDim.x;  // == C / 4
  for (int i = threadIdx.x; i < C; i += nthr) {
    const int64_t g = c0 + i;
    keys[i] = (g < se) ? order_key<T>(own[g]) : ~0ull;
  }
  __syncthreads();
  uint64_t* dst = sorted + (mom_first_chunk(x_off, z_off, s, side, C) + c) * C;
  sort_keys_block<4>(keys, C, dst);
}

template <typename T, int PRED>
__global__ __launch_bounds__(kSortThreads) void k_moments_search(
    const T* __restrict__ x, const int64_t* __restrict__ x_off, const T* __restrict__ z,
    const int64_t* __restrict__ z_off, const uint64_t* __restrict__ sorted, int C, int group,
    int tiles, unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  __shared__ uint32_t nonnan[kMomMaxGroup];
  const MomBlock b = mom_block(tiles);
  const bool zs = b.side != 0;
  const T* own = zs ? z : x;
  const int64_t* soff = zs ? z_off : x_off;
  const int64_t* ooff = zs ? x_off : z_off;
  const int64_t sb = soff[b.s], se = soff[b.s + 1];
  const int64_t n_o = ooff[b.s + 1] - ooff[b.s];
  const int64_t i0 = sb + (int64_t)b.t * kMomSearchTile;
  if (i0 >= se || n_o <= 0) return;  // block-uniform
  uint64_t k[kMomPer];
  bool valid[kMomPer];
  unsigned long long lo[kMomPer], hi[kMomPer];
#pragma unroll
  for (int e = 0; e < kMomPer; ++e) {
    const int64_t i = i0 + e * kSortThreads + threadIdx.x;
    valid[e] = i < se;
    const T v = valid[e] ? own[i] : (T)0;
    valid[e] = valid[e] && !is_nan_score<T>(v);
    k[e] = order_key<T>(v);
    lo[e] = hi[e] = 0;
  }
  const int chunks = (int)((n_o + C - 1) / C);
  const uint64_t* src0 = sorted + mom_first_chunk(x_off, z_off, b.s, zs ? 0 : 1, C) * C;
  unsigned long long V = 0;  // the other side's non-NaN scores
  for (int c0 = 0; c0 < chunks; c0 += group) {
    const int ng = std::min(group, chunks - c0);
    const uint64_t* src = src0 + (int64_t)c0 * C;
    __syncthreads();
    for (int i = threadIdx.x; i < ng * C; i += kSortThreads) keys[i] = src[i];
    __syncthreads();
    if ((int)threadIdx.x < ng) {
      const int g = threadIdx.x;
      uint32_t nn = (uint32_t)std::min<int64_t>(C, n_o - (int64_t)(c0 + g) * C);
      if (std::is_floating_point<T>::value)
        nn = std::min(nn, lower_bound_lds(keys + g * C, C, ~0ull));
      nonnan[g] = nn;
    }
    __syncthreads();
    for (int g = 0; g < ng; ++g) {
      const uint64_t* kc = keys + g * C;
      const uint32_t nn = nonnan[g];
      V += nn;
#pragma unroll
      for (int e = 0; e < kMomPer; ++e) {
        if (valid[e]) {
          // strict on the x side needs lo alone, on the z side hi alone; half needs both
          if (PRED == TW_PRED_HALF || !zs) lo[e] += lower_bound_lds(kc, C, k[e]);
          if (PRED == TW_PRED_HALF || zs) hi[e] += std::min(upper_bound_lds(kc, C, k[e]), nn);
        }
      }
    }
  }
  unsigned long long c = 0, c2 = 0, q = 0;
#pragma unroll
  for (int e = 0; e < kMomPer; ++e) {
    if (!valid[e]) continue;
    // x side: (#{z < x}, #{z <= x});  z side: (#{x > z}, #{x >= z})
    const unsigned long long first = zs ? V - hi[e] : lo[e];
    const unsigned long long second = zs ? V - lo[e] : hi[e];
    const unsigned long long a = PRED == TW_PRED_HALF ? first + second : first;
    c += a;
    c2 += a * a;
    q += PRED == TW_PRED_HALF ? 3ull * first + second : a;  // 4 #{>} + #{==}
  }
  mom_commit(c, c2, q, b.side, out + 4 * (int64_t)b.s);
}

template <typename T, int PRED>
int launch_moments_pairs(const void* x, const int64_t* x_off, const void* z, const int64_t* z_off,
                         int32_t n_shards, int64_t max_n, uint64_t* out, hipStream_t st) {
  const int64_t tiles = ceil_div(max_n, kMomPairTile);
  TW_ARG_CHECK((int64_t)n_shards * 2 * tiles < (1ll << 31), "tw_pair_moments: grid too large");
  hipLaunchKernelGGL((k_moments_pairs<T, PRED>), dim3((unsigned)(n_shards * 2 * tiles)),
                     dim3(kMomPairThreads), 0, st, (const T*)x, x_off, (const T*)z, z_off,
                     (int)tiles, (unsigned long long*)out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

inline int64_t moments_chunk(int64_t max_n) {
  int64_t C = 1024;  // sort_keys_block<4>: C / 4 threads, at least four waves
  while (C < max_n && C < kMomMaxC) C <<= 1;
  return C;
}

template <typename T, int PRED>
int launch_moments_sorted(const void* x, const int64_t* x_off, const void* z,
                          const int64_t* z_off, int32_t n_shards, int64_t max_n, void* work,
                          uint64_t* out, hipStream_t st) {
  TW_ARG_CHECK(work != nullptr, "tw_pair_moments: the sorted algorithm needs d_work");
  const int64_t C = moments_chunk(max_n);
  const int64_t chunks = ceil_div(max_n, C);
  const int64_t tiles = ceil_div(max_n, kMomSearchTile);
  TW_ARG_CHECK((int64_t)n_shards * 2 * chunks < (1ll << 31) &&
                   (int64_t)n_shards * 2 * tiles < (1ll << 31),
               "tw_pair_moments: grid too large");
  static bool attrs_set = false;  // > 64 KiB of dynamic LDS must be opted into once
  if (!attrs_set) {
    TW_HIP_CHECK(hipFuncSetAttribute((const void*)k_moments_search<T, PRED>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(sizeof(uint64_t) * kMaxChunk)));
    attrs_set = true;
  }
  hipLaunchKernelGGL((k_moments_sort<T>), dim3((unsigned)(n_shards * 2 * chunks)),
                     dim3((unsigned)(C / 4)), sizeof(uint64_t) * C, st, (const T*)x, x_off,
                     (const T*)z, z_off, (int)chunks, (int)C, (uint64_t*)work);
  TW_LAUNCH_CHECK();
  // as many sorted chunks as fit in 128 KiB of LDS are staged at once
  const int group = (int)std::min<int64_t>(chunks, kMaxChunk / C);
  hipLaunchKernelGGL((k_moments_search<T, PRED>), dim3((unsigned)(n_shards * 2 * tiles)),
                     dim3(kSortThreads), sizeof(uint64_t) * group * C, st, (const T*)x, x_off,
                     (const T*)z, z_off, (const uint64_t*)work, (int)C, group, (int)tiles,
                     (unsigned long long*)out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

template <typename T>
int launch_moments(bool sorted, const void* x, const int64_t* x_off, const void* z,
                   const int64_t* z_off, int32_t n_shards, int64_t max_n, int32_t pred,
                   void* work, uint64_t* out, hipStream_t st) {
  if (sorted) {
    if (pred == TW_PRED_HALF)
      return launch_moments_sorted<T, TW_PRED_HALF>(x, x_off, z, z_off, n_shards, max_n, work,
                                                    out, st);
    return launch_moments_sorted<T, TW_PRED_GT>(x, x_off, z, z_off, n_shards, max_n, work, out,
                                                st);
  }
  if (pred == TW_PRED_HALF)
    return launch_moments_pairs<T, TW_PRED_HALF>(x, x_off, z, z_off, n_shards, max_n, out, st);
  return launch_moments_pairs<T, TW_PRED_GT>(x, x_off, z, z_off, n_shards, max_n, out, st);
}

}  // namespace tw

using namespace tw;

extern "C" int tw_pair_moments_set_algo(int32_t algo) {
  TW_ARG_CHECK(algo >= 0 && algo <= 2,
               "tw_pair_moments_set_algo: 0 (auto), 1 (all pairs), 2 (sorted)");
  g_moments_algo = algo;
  return TW_OK;
}

extern "C" int64_t tw_pair_moments_work_bytes(int32_t n_shards, int64_t total_nx,
                                              int64_t total_nz) {
  if (n_shards < 0 || total_nx < 0 || total_nz < 0) return 0;
  // (total_nx / C + total_nz / C + 2 n_shards) chunk slots of C <= kMomMaxC keys
  return (int64_t)sizeof(uint64_t) * (total_nx + total_nz + 2 * (int64_t)n_shards * kMomMaxC);
}

extern "C" int tw_pair_moments(const void* d_x, const int64_t* d_x_off, const void* d_z,
                               const int64_t* d_z_off, int32_t n_shards, int64_t max_nx,
                               int64_t max_nz, int32_t dtype, int32_t pred, void* d_work,
                               uint64_t* d_out, void* stream) {
  TW_ARG_CHECK(n_shards >= 0 && max_nx >= 0 && max_nz >= 0,
               "tw_pair_moments: bad sizes (n_shards, max_nx and max_nz must be >= 0)");
  TW_ARG_CHECK(pred == TW_PRED_GT || pred == TW_PRED_HALF,
               "tw_pair_moments: predicate must be TW_PRED_GT or TW_PRED_HALF");
  TW_ARG_CHECK(dtype == TW_F64 || dtype == TW_I64, "tw_pair_moments: unknown dtype %d", dtype);
  // a per-point count u * n stays below 2^32 (its square is summed in u64; the caller refuses
  // blocks whose sums of squares could reach 2^64)
  const int64_t unit = pred == TW_PRED_HALF ? 2 : 1;
  TW_ARG_CHECK(max_nx < (1ll << 32) / unit && max_nz < (1ll << 32) / unit,
               "tw_pair_moments: a per-point count would not fit 32 bits");
  hipStream_t st = (hipStream_t)stream;
  if (n_shards == 0) return TW_OK;
  TW_HIP_CHECK(tw_zero_async(d_out, 0, sizeof(uint64_t) * 4 * n_shards, st));
  if (max_nx == 0 || max_nz == 0) return TW_OK;
  const uint64_t pairs = (uint64_t)max_nx * (uint64_t)max_nz;  // < 2^64 by the check above
  const bool sorted = g_moments_algo == 2 ||
                      (g_moments_algo == 0 && pairs >= (uint64_t)TW_MOMENTS_SORTED_MIN_PAIRS);
  const int64_t max_n = std::max(max_nx, max_nz);
  if (dtype == TW_F64)
    return launch_moments<double>(sorted, d_x, d_x_off, d_z, d_z_off, n_shards, max_n, pred,
                                  d_work, d_out, st);
  return launch_moments<long long>(sorted, d_x, d_x_off, d_z, d_z_off, n_shards, max_n, pred,
                                   d_work, d_out, st);
}
