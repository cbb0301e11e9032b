// selfpairs.hip — one-sample, degree-2 U-statistics (tuplewise.onesample; an extension, not in
// the reference): pairs i < j drawn from ONE sample S,
//   TW_SELF_GINI     |s_i - s_j|                     (Gini mean difference)
//   TW_SELF_VAR      (s_i - s_j)^2 / 2               (unbiased sample variance)
//   TW_SELF_KENDALL  concordant / discordant / tied  (Kendall's tau on points (a, b))
// tw_self_pairs walks the TRIANGLE of tile pairs (I <= J) of every shard: tile J is staged in
// LDS, every lane holds kSelfR points of tile I in registers, an off-diagonal tile pair does
// all T^2 pairs and a diagonal one only i < j, so each unordered pair is visited once (the
// two-sample kernels called with X = Z visit it twice, and the diagonal besides).
// tw_self_pairs_idx32 evaluates given index pairs (UB_indices).  Sums are deterministic as in
// pairsum.hip: every block writes its partials in a fixed lane/wave order into d_work and a
// second kernel adds a shard's partials in a fixed order — the Kendall integers the same way
// (no atomics, nothing to zero).
#include "tw_common.h"
#include "selfreduce.h"
#include <algorithm>
#include <cmath>
#include <type_traits>

namespace tw {

constexpr int kSelfR = 2;                  // points of tile I per lane
constexpr int kSelfT = kBlock * kSelfR;    // points per tile edge
constexpr int kSelfG = 4;                  // tile pairs per block
constexpr int kSelfPPT = 8;                // index pairs per lane (tw_self_pairs_idx32)

inline int64_t self_tile_pairs(int64_t max_n) {
  const int64_t nt = std::max<int64_t>(1, ceil_div(max_n, kSelfT));
  return nt * (nt + 1) / 2;
}
inline int64_t self_blocks_per_shard(int64_t max_n) {
  return ceil_div(self_tile_pairs(max_n), kSelfG);
}
inline int64_t self_idx_blocks_per_shard(int64_t max_pairs) {
  return std::max<int64_t>(1, ceil_div(max_pairs, (int64_t)kBlock * kSelfPPT));
}

// One Kendall point: the LDS tile holds them as 16-byte items (one ds_read_b128 per j,
// broadcast to the wave).
template <typename V>
struct alignas(16) SelfPt {
  V a, b;
};

struct KendallAcc {
  unsigned c, d, tx, ty, txy;
};

// The Kendall predicates by comparisons only (NaN: all false; -0.0 == 0.0), as NumPy's >, <, ==
template <typename V, bool MASK>
__device__ __forceinline__ void kendall_pair(V ai, V bi, V aj, V bj, bool ok, KendallAcc& k) {
  const bool ga = ai > aj, la = ai < aj, gb = bi > bj, lb = bi < bj;
  const bool ea = ai == aj, eb = bi == bj;
  // logical operators: the predicates stay lane masks (scalar and / or) and every counter
  // takes one add-with-carry-in
  bool c = (ga && gb) || (la && lb), d = (ga && lb) || (la && gb), x = ea, y = eb, xy = ea && eb;
  if (MASK) {
    c = c && ok;
    d = d && ok;
    x = x && ok;
    y = y && ok;
    xy = xy && ok;
  }
  k.c += c;
  k.d += d;
  k.tx += x;
  k.ty += y;
  k.txy += xy;
}

template <int K>
__device__ __forceinline__ double self_fkern(double si, double sj) {
  const double d = si - sj;
  if constexpr (K == TW_SELF_GINI) return fabs(d);
  else return d * d;  // halved once per block partial (an exact scaling)
}

// Block `blockIdx.x` = (shard, group of kSelfG consecutive tile pairs of the triangle).
// V: double or int64_t (Kendall compares int64 as int64); the float kernels take double only.
template <typename V, int K>
__global__ __launch_bounds__(kBlock) void k_self_pairs(const V* __restrict__ s,
                                                       const int64_t* __restrict__ off,
                                                       int blocks_per_shard, int64_t tile_pairs,
                                                       void* __restrict__ work) {
  constexpr bool KEN = K == TW_SELF_KENDALL;
  constexpr int W = KEN ? 2 : 1;  // 8-byte values per item
  __shared__ SelfPt<V> tile2[KEN ? kSelfT : 1];
  __shared__ V tile1[KEN ? 1 : kSelfT];
  __shared__ unsigned long long part[kBlock / kWave];
  const int sh = (int)blockIdx.x / blocks_per_shard;
  const int g = (int)blockIdx.x - sh * blocks_per_shard;
  const int64_t sb = off[sh], n = off[sh + 1] - sb;
  const V* __restrict__ base = s + sb * W;
  const int64_t p_end = std::min<int64_t>(tile_pairs, (int64_t)(g + 1) * kSelfG);
  KendallAcc tot = {0u, 0u, 0u, 0u, 0u};
  double ftot = 0.0;
  for (int64_t p = (int64_t)g * kSelfG; p < p_end; ++p) {
    int I, J;
    self_tile_of(p, I, J);
    const int64_t i0 = (int64_t)I * kSelfT, j0 = (int64_t)J * kSelfT;
    if (j0 >= n) break;  // block-uniform: later p have J at least this large
    const int nj = (int)std::min<int64_t>(kSelfT, n - j0);
    __syncthreads();  // the previous tile's readers
    for (int q = threadIdx.x; q < nj; q += kBlock) {
      if constexpr (KEN) tile2[q] = SelfPt<V>{base[(j0 + q) * 2], base[(j0 + q) * 2 + 1]};
      else tile1[q] = base[j0 + q];
    }
    V ai[kSelfR], bi[kSelfR];
    bool valid[kSelfR];
#pragma unroll
    for (int r = 0; r < kSelfR; ++r) {
      const int64_t i = i0 + r * kBlock + threadIdx.x;
      valid[r] = i < n;
      ai[r] = valid[r] ? base[i * W] : V(0);
      bi[r] = (KEN && valid[r]) ? base[i * W + 1] : V(0);
    }
    __syncthreads();
    KendallAcc ka[kSelfR];
    double fa[kSelfR];
#pragma unroll
    for (int r = 0; r < kSelfR; ++r) {
      ka[r] = KendallAcc{0u, 0u, 0u, 0u, 0u};
      fa[r] = 0.0;
    }
    // (the Kendall loops are unrolled by 2 only: six lane masks a pair live in scalar
    // registers, and a deeper unroll spills them)
    if (I != J) {  // all nj points of tile J against this lane's points
      if constexpr (KEN) {
#pragma unroll 2
        for (int j = 0; j < nj; ++j) {
          const SelfPt<V> pj = tile2[j];
#pragma unroll
          for (int r = 0; r < kSelfR; ++r)
            kendall_pair<V, false>(ai[r], bi[r], pj.a, pj.b, true, ka[r]);
        }
      } else {
#pragma unroll 4
        for (int j = 0; j < nj; ++j) {
          const double sj = tile1[j];
#pragma unroll
          for (int r = 0; r < kSelfR; ++r) fa[r] += self_fkern<K>(ai[r], sj);
        }
      }
    } else {  // the diagonal tile: only j above this lane's own position
      if constexpr (KEN) {
#pragma unroll 2
        for (int j = 0; j < nj; ++j) {
          const SelfPt<V> pj = tile2[j];
#pragma unroll
          for (int r = 0; r < kSelfR; ++r)
            kendall_pair<V, true>(ai[r], bi[r], pj.a, pj.b, j > r * kBlock + (int)threadIdx.x,
                                  ka[r]);
        }
      } else {
#pragma unroll 4
        for (int j = 0; j < nj; ++j) {
          const double sj = tile1[j];
#pragma unroll
          for (int r = 0; r < kSelfR; ++r) {
            const double v = self_fkern<K>(ai[r], sj);
            fa[r] += j > r * kBlock + (int)threadIdx.x ? v : 0.0;
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kSelfR; ++r) {
      if (!valid[r]) continue;
      if constexpr (KEN) {
        tot.c += ka[r].c;
        tot.d += ka[r].d;
        tot.tx += ka[r].tx;
        tot.ty += ka[r].ty;
        tot.txy += ka[r].txy;
      } else {
        ftot += fa[r];
      }
    }
  }
  // every slot is written, also by blocks whose tile pairs lie outside a short shard
  if constexpr (KEN) {
    unsigned long long* w = (unsigned long long*)work + (int64_t)blockIdx.x * 5;
    const unsigned v[5] = {tot.c, tot.d, tot.tx, tot.ty, tot.txy};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const unsigned long long b = self_block_sum_u64(v[k], part);
      if (threadIdx.x == 0) w[k] = b;
    }
  } else {
    const double b = self_block_sum_f64(ftot, (double*)part);
    if (threadIdx.x == 0) ((double*)work)[blockIdx.x] = K == TW_SELF_VAR ? 0.5 * b : b;
  }
}

// The given index pairs (absolute item positions in s) of every shard's pair range.
template <typename V, int K>
__global__ __launch_bounds__(kBlock) void k_self_pairs_idx(const V* __restrict__ s,
                                                           const int32_t* __restrict__ ii,
                                                           const int32_t* __restrict__ jj,
                                                           const int64_t* __restrict__ pair_off,
                                                           int blocks_per_shard,
                                                           void* __restrict__ work) {
  constexpr bool KEN = K == TW_SELF_KENDALL;
  __shared__ unsigned long long part[kBlock / kWave];
  const int sh = (int)blockIdx.x / blocks_per_shard;
  const int bi = (int)blockIdx.x - sh * blocks_per_shard;
  const int64_t pb = pair_off[sh], pe = pair_off[sh + 1];
  const int64_t p0 = pb + (int64_t)bi * (kBlock * kSelfPPT);
  KendallAcc ka = {0u, 0u, 0u, 0u, 0u};
  double fa = 0.0;
#pragma unroll
  for (int k = 0; k < kSelfPPT; ++k) {
    const int64_t p = p0 + k * kBlock + threadIdx.x;
    if (p < pe) {
      const int64_t i = ii[p], j = jj[p];
      if constexpr (KEN) kendall_pair<V, false>(s[2 * i], s[2 * i + 1], s[2 * j], s[2 * j + 1], true, ka);
      else fa += self_fkern<K>(s[i], s[j]);
    }
  }
  if constexpr (KEN) {
    unsigned long long* w = (unsigned long long*)work + (int64_t)blockIdx.x * 5;
    const unsigned v[5] = {ka.c, ka.d, ka.tx, ka.ty, ka.txy};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const unsigned long long b = self_block_sum_u64(v[k], part);
      if (threadIdx.x == 0) w[k] = b;
    }
  } else {
    const double b = self_block_sum_f64(fa, (double*)part);
    if (threadIdx.x == 0) ((double*)work)[blockIdx.x] = K == TW_SELF_VAR ? 0.5 * b : b;
  }
}

template <typename V, int K>
int self_pairs_launch(const void* d_s, const int64_t* d_off, int32_t n_shards, int64_t max_n,
                      void* d_work, void* d_out, hipStream_t st) {
  const int64_t per = self_blocks_per_shard(max_n);
  TW_ARG_CHECK(per * n_shards < (1ll << 31), "tw_self_pairs: grid too large");
  hipLaunchKernelGGL((k_self_pairs<V, K>), dim3((unsigned)(per * n_shards)), dim3(kBlock), 0, st,
                     (const V*)d_s, d_off, (int)per, self_tile_pairs(max_n), d_work);
  TW_LAUNCH_CHECK();
  if constexpr (K == TW_SELF_KENDALL)
    hipLaunchKernelGGL((k_self_reduce<unsigned long long, 5>), dim3(n_shards), dim3(kBlock), 0,
                       st, (const unsigned long long*)d_work, (int)per,
                       (unsigned long long*)d_out);
  else
    hipLaunchKernelGGL((k_self_reduce<double, 1>), dim3(n_shards), dim3(kBlock), 0, st,
                       (const double*)d_work, (int)per, (double*)d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

template <typename V, int K>
int self_pairs_idx_launch(const void* d_s, const int32_t* d_i, const int32_t* d_j,
                          const int64_t* d_pair_off, int32_t n_shards, int64_t max_pairs,
                          void* d_work, void* d_out, hipStream_t st) {
  const int64_t per = self_idx_blocks_per_shard(max_pairs);
  TW_ARG_CHECK(per * n_shards < (1ll << 31), "tw_self_pairs_idx32: grid too large");
  hipLaunchKernelGGL((k_self_pairs_idx<V, K>), dim3((unsigned)(per * n_shards)), dim3(kBlock), 0,
                     st, (const V*)d_s, d_i, d_j, d_pair_off, (int)per, d_work);
  TW_LAUNCH_CHECK();
  if constexpr (K == TW_SELF_KENDALL)
    hipLaunchKernelGGL((k_self_reduce<unsigned long long, 5>), dim3(n_shards), dim3(kBlock), 0,
                       st, (const unsigned long long*)d_work, (int)per,
                       (unsigned long long*)d_out);
  else
    hipLaunchKernelGGL((k_self_reduce<double, 1>), dim3(n_shards), dim3(kBlock), 0, st,
                       (const double*)d_work, (int)per, (double*)d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

}  // namespace tw

using namespace tw;

#define TW_SELF_ARG_CHECKS(fn, size, size_name)                                               \
  TW_ARG_CHECK(n_shards >= 0, fn ": n_shards %d < 0", n_shards);                              \
  TW_ARG_CHECK(size >= 0, fn ": " size_name " %lld < 0", (long long)size);                    \
  TW_ARG_CHECK(kern >= TW_SELF_GINI && kern <= TW_SELF_KENDALL, fn ": unknown kern %d", kern); \
  TW_ARG_CHECK(dtype == TW_F64 || dtype == TW_I64, fn ": unknown dtype %d", dtype);           \
  TW_ARG_CHECK(kern == TW_SELF_KENDALL || dtype == TW_F64,                                    \
               fn ": dtype TW_I64 with a float kern %d (float kernels take TW_F64)", kern)

extern "C" int32_t tw_self_pairs_tile(void) { return kSelfT; }

extern "C" int64_t tw_self_pairs_work_bytes(int32_t n_shards, int64_t max_n) {
  if (n_shards < 0 || max_n < 0) return 0;
  return std::max<int64_t>(8, self_blocks_per_shard(max_n) * n_shards * 5 * 8);
}

extern "C" int64_t tw_self_pairs_idx_work_bytes(int32_t n_shards, int64_t max_pairs) {
  if (n_shards < 0 || max_pairs < 0) return 0;
  return std::max<int64_t>(8, self_idx_blocks_per_shard(max_pairs) * n_shards * 5 * 8);
}

extern "C" int tw_self_pairs(const void* d_s, const int64_t* d_off, int32_t n_shards,
                             int64_t max_n, int32_t dtype, int32_t kern, void* d_work,
                             void* d_out, void* stream) {
  TW_SELF_ARG_CHECKS("tw_self_pairs", max_n, "max_n");
  hipStream_t st = (hipStream_t)stream;
  if (n_shards == 0) return TW_OK;
  if (kern == TW_SELF_GINI)
    return self_pairs_launch<double, TW_SELF_GINI>(d_s, d_off, n_shards, max_n, d_work, d_out, st);
  if (kern == TW_SELF_VAR)
    return self_pairs_launch<double, TW_SELF_VAR>(d_s, d_off, n_shards, max_n, d_work, d_out, st);
  if (dtype == TW_F64)
    return self_pairs_launch<double, TW_SELF_KENDALL>(d_s, d_off, n_shards, max_n, d_work, d_out, st);
  return self_pairs_launch<int64_t, TW_SELF_KENDALL>(d_s, d_off, n_shards, max_n, d_work, d_out, st);
}

extern "C" int tw_self_pairs_idx32(const void* d_s, const int32_t* d_i, const int32_t* d_j,
                                   const int64_t* d_pair_off, int32_t n_shards,
                                   int64_t max_pairs, int32_t dtype, int32_t kern, void* d_work,
                                   void* d_out, void* stream) {
  TW_SELF_ARG_CHECKS("tw_self_pairs_idx32", max_pairs, "max_pairs");
  hipStream_t st = (hipStream_t)stream;
  if (n_shards == 0) return TW_OK;
  if (kern == TW_SELF_GINI)
    return self_pairs_idx_launch<double, TW_SELF_GINI>(d_s, d_i, d_j, d_pair_off, n_shards, max_pairs, d_work, d_out, st);
  if (kern == TW_SELF_VAR)
    return self_pairs_idx_launch<double, TW_SELF_VAR>(d_s, d_i, d_j, d_pair_off, n_shards, max_pairs, d_work, d_out, st);
  if (dtype == TW_F64)
    return self_pairs_idx_launch<double, TW_SELF_KENDALL>(d_s, d_i, d_j, d_pair_off, n_shards, max_pairs, d_work, d_out, st);
  return self_pairs_idx_launch<int64_t, TW_SELF_KENDALL>(d_s, d_i, d_j, d_pair_off, n_shards, max_pairs, d_work, d_out, st);
}
