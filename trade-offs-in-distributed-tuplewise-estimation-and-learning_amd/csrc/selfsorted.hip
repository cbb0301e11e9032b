// selfsorted.hip — the one-sample Kendall counters and the Gini pair sum of ONE large sample
// without walking its n (n - 1) / 2 pairs (selfpairs.hip is the all-pairs way
// to the same numbers).  Built from sortkeys.h like moments.hip's sorted branch: every shard is
// cut into chunks of C order keys, each chunk is sorted in LDS, and a point learns how many keys
// of the shard lie below it (lo) and how many equal it (eq) by two binary searches in every
// sorted chunk staged in LDS.  Cost class: O(n * (n / C) * log C) per pass — not O(n log n), but
// n / C * log C instead of n per point.
//
// Kendall (TW_F64, TW_I64), the five integers of tw_self_pairs on every input:
//   1 k_ss_sort_vals   sorted chunks of the a keys and of the b keys (doubles: also of the keys
//                      of CLEAN points only — both coordinates non-NaN — the rest as padding);
//   2 k_ss_count       from the sorted keys themselves (lanes on neighbouring keys search
//                      along nearly one path): the dense min-rank lo of every a key and every b
//                      key, and the tie counts 2 Tx = sum over non-NaN a of (eq_a - 1), 2 Ty
//                      likewise.  A shard that holds a point with exactly one NaN coordinate
//                      runs the searches on the clean-only chunks too: Tx', Ty' among clean
//                      points.  k_ss_compose: a point finds its keys in its own chunk's sorted
//                      arrays (one search each) and takes their ranks: the composite key
//                      (ra << 32) | rb of every clean point, ~0 for the others; v = #clean;
//   3 k_ss_sort_keys   sorted chunks of the composite keys; k_ss_order: the position of every
//                      clean point in the (a, b) lexicographic order = #{keys below} + #{equal
//                      keys in earlier chunks} + its offset in its own chunk's run of equals;
//                      rb is scattered there.  The tie-breaks sum to Txy;
//   4 k_ss_sort_keys   per chunk of that rb sequence: the strict inversions inside the chunk
//                      (all pairs in LDS, u32 compares), then the chunk sorted; k_ss_cross:
//                      every element of chunk q against the sorted chunks p < q, C_p -
//                      upper_bound.  Both add to D;
//   5 k_ss_final       C = v (v - 1) / 2 - Tx' - Ty' + Txy - D.
// A NaN key and chunk padding share the top key ~0; so does INT64_MAX, which is a value: every
// upper bound is clamped to the chunk's item count, as moments.hip does.  Partial counts are
// added with integer atomics (addition commutes); everything that can pass 2^32 is uint64.
//
// Gini (TW_F64): sum_{i<j} |s_i - s_j| = sum_i (lo_i + hi_i - n) s_i with hi = lo + eq (the
// sorted formula sum_i (2 i - n + 1) s_(i), a run of equal values sharing its coefficients),
// summed over the sorted chunks' keys, which decode to the values.  The product is an exact
// two-product, all sums are double-double in a fixed order (lane's keys, wave butterfly, waves,
// tiles of the shard's own chunks), rounded once per shard; non-finite values by counts.
#include "ddmath.h"
#include "sortkeys.h"
#include <algorithm>
#include <type_traits>

namespace tw {

constexpr int kSsChunk = 4096;   // the default chunk
constexpr int kSsAcc = 8;        // u64 accumulators per shard
// Kendall: 2Tx, 2Ty, 2Tx', 2Ty', Txy, v, D, flag "a point with exactly one NaN coordinate";
// Gini: #NaN, #+inf, #-inf
enum { kAccTx = 0, kAccTy = 1, kAccTxC = 2, kAccTyC = 3, kAccTxy = 4, kAccV = 5, kAccD = 6,
       kAccHalf = 7 };
constexpr int kSsGiniPer = 4;    // keys per lane of the Gini pass (fixes the summation order)
constexpr int kSsGroup = 16;     // sorted chunks per block of the cross-chunk inversion count

// First chunk slot of shard s: floor(items before it / C) + s.  Shard s needs ceil(n_s / C) <=
// floor(n_s / C) + 1 <= slot0(s + 1) - slot0(s) slots whatever the mix of sizes, and all shards
// take fewer than total_n / C + n_shards.
__device__ __forceinline__ int64_t ss_slot0(const int64_t* __restrict__ off, int s, int C) {
  return (off[s] - off[0]) / C + s;
}

// Block sum of v added to *target (one integer atomic, none for a zero).
__device__ __forceinline__ void ss_block_add(unsigned long long v, unsigned long long* target,
                                             unsigned long long* part) {
  v = wave_sum_u64(v);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  __syncthreads();  // part's previous readers
  if (lane == 0) part[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    const int nw = (blockDim.x + kWave - 1) / kWave;
    for (int w = 0; w < nw; ++w) t += part[w];
    if (t) atomicAdd(target, t);
  }
}

// lo[e] += #{keys < k[e]}, eq[e] += #{keys == k[e]} over the shard's sorted chunks at src (chunk
// c holds min(C, n - c C) items, then padding).  Every thread of the block calls it.
template <int PER>
__device__ __forceinline__ void ss_search_chunks(const uint64_t* __restrict__ src, int chunks,
                                                 int64_t n, int C, uint64_t* keys,
                                                 const uint64_t (&k)[PER], const bool (&ok)[PER],
                                                 uint32_t (&lo)[PER], uint32_t (&eq)[PER]) {
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();  // the previous chunk's readers
    for (int i = threadIdx.x; i < C; i += blockDim.x) keys[i] = src[(int64_t)c * C + i];
    __syncthreads();
    const uint32_t len = (uint32_t)std::min<int64_t>(C, n - (int64_t)c * C);
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      if (ok[e]) {
        const uint32_t l = lower_bound_lds(keys, C, k[e]);
        const uint32_t h = std::min(upper_bound_lds(keys, C, k[e]), len);
        lo[e] += l;
        eq[e] += h - l;
      }
    }
  }
}

// ------------------------------------------------------------------------------ chunk sorts
// One block per (shard, array, chunk) of the raw values: array 0 = the keys of column 0, 1 =
// column 1, 2 and 3 = the same with every point that is not clean turned into padding.  W
// 8-byte values per item.  C / kE threads.
template <typename T, int kE>
__global__ __launch_bounds__(kSortThreads) void k_ss_sort_vals(
    const T* __restrict__ v, const int64_t* __restrict__ off, int chunks, int C, int W, int NW,
    uint64_t* __restrict__ arrays, int64_t arr_stride, unsigned long long* __restrict__ acc) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  const int s = (int)blockIdx.x / (NW * chunks);
  const int r = (int)blockIdx.x - s * NW * chunks;
  const int which = r / chunks, c = r - which * chunks;
  const int col = which & 1;
  const bool clean = which >= 2;
  const int64_t sb = off[s], n = off[s + 1] - sb, c0 = (int64_t)c * C;
  if (c0 >= n) return;  // block-uniform: the searches never read a chunk past the shard's end
  bool half = false;
  for (int i = threadIdx.x; i < C; i += blockDim.x) {
    uint64_t k = ~0ull;
    if (c0 + i < n) {
      const T* __restrict__ p = v + (sb + c0 + i) * W;
      const T x = p[col];
      k = order_key<T>(x);
      if (clean) {
        const bool other_nan = is_nan_score<T>(p[1 - col]);
        half |= other_nan != is_nan_score<T>(x);
        if (other_nan) k = ~0ull;
      }
    }
    keys[i] = k;
  }
  if (half && which == 2) acc[(int64_t)s * kSsAcc + kAccHalf] = 1ull;
  __syncthreads();
  sort_keys_block<kE>(keys, C, arrays + which * arr_stride + (ss_slot0(off, s, C) + c) * C);
}

// One block per (shard, chunk) of a u64 sequence laid out by item position (src[off[s] - off[0]
// + i]): the composite keys (INV false, n items), or the rb sequence of the clean points (INV
// true, v items), whose in-chunk strict inversions #{i < j : src[i] > src[j]} are counted before
// the chunk is sorted.  C / kE threads.
template <int kE, bool INV>
__global__ __launch_bounds__(kSortThreads) void k_ss_sort_keys(
    const uint64_t* __restrict__ src, const int64_t* __restrict__ off, int chunks, int C,
    uint64_t* __restrict__ dst, unsigned long long* __restrict__ acc) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  __shared__ unsigned long long part[kSortThreads / kWave];
  const int s = (int)blockIdx.x / chunks, c = (int)blockIdx.x - s * chunks;
  const int64_t cnt = INV ? (int64_t)acc[(int64_t)s * kSsAcc + kAccV] : off[s + 1] - off[s];
  const int64_t c0 = (int64_t)c * C;
  if (c0 >= cnt) return;  // block-uniform
  const int len = (int)std::min<int64_t>(C, cnt - c0);
  const uint64_t* __restrict__ from = src + (off[s] - off[0]) + c0;
  for (int i = threadIdx.x; i < C; i += blockDim.x) keys[i] = i < len ? from[i] : ~0ull;
  __syncthreads();
  if constexpr (INV) {
    // the values are ranks below 2^31: their low words, one broadcast read per j
    const uint32_t* __restrict__ k32 = (const uint32_t*)keys;
    uint32_t mine[kE], inv[kE];
    int idx[kE];
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      idx[e] = e * (int)blockDim.x + (int)threadIdx.x;
      mine[e] = idx[e] < len ? k32[2 * idx[e]] : 0xFFFFFFFFu;  // nothing exceeds a pad
      inv[e] = 0;
    }
#pragma unroll 4
    for (int j = 0; j < len; ++j) {
      const uint32_t x = k32[2 * j];
#pragma unroll
      for (int e = 0; e < kE; ++e) inv[e] += (x > mine[e]) && (j < idx[e]);
    }
    unsigned long long t = 0;
#pragma unroll
    for (int e = 0; e < kE; ++e) t += inv[e];
    ss_block_add(t, acc + (int64_t)s * kSsAcc + kAccD, part);
  }
  sort_keys_block<kE>(keys, C, dst + (ss_slot0(off, s, C) + c) * C);
}

// ------------------------------------------------------------------------------ Kendall
// The tile of 1024 PER chunk-slot positions of a shard's sorted chunks that a block searches
// FROM: neighbouring lanes hold neighbouring keys of one sorted chunk, so their binary searches
// walk nearly the same path and most LDS reads of a wave are broadcasts (a search from the
// points in sample order has every lane on a path of its own; DESIGN.md §4.9b has the times).
// real[e]: position e holds one of the chunk's items (its padding does not).
template <int PER>
struct SsTile {
  uint64_t k[PER];
  bool real[PER];
  int own[PER];      // the position's chunk
  uint32_t at[PER];  // and its place in it
};
template <int PER>
__device__ __forceinline__ SsTile<PER> ss_load_tile(const uint64_t* __restrict__ src, int64_t p0,
                                                    int chunks, int64_t n, int C) {
  SsTile<PER> t;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int64_t p = p0 + e * kSortThreads + threadIdx.x;
    const bool in = p < (int64_t)chunks * C;
    t.k[e] = in ? src[p] : ~0ull;
    t.own[e] = (int)(p / C);
    t.at[e] = (uint32_t)(p - (int64_t)t.own[e] * C);
    t.real[e] = in && (int64_t)t.at[e] < n - (int64_t)t.own[e] * C;
  }
  return t;
}

// One block per (shard, array, tile of chunk-slot positions) of the sorted value chunks: lo and
// eq of every key among the shard's keys of that array.  Arrays 0 and 1 (all points): the ranks
// into `rank` at the key's position, 2 Tx and 2 Ty; arrays 2 and 3 (clean points, only where
// the shard's kAccHalf flag is set): 2 Tx' and 2 Ty'.
template <typename T, int PER>
__global__ __launch_bounds__(kSortThreads) void k_ss_count(
    const int64_t* __restrict__ off, int tiles, int NW, int C, const uint64_t* __restrict__ arrays,
    int64_t arr_stride, uint32_t* __restrict__ rank, unsigned long long* __restrict__ acc) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  __shared__ unsigned long long part[kSortThreads / kWave];
  const int lb = xcd_block(blockIdx.x, gridDim.x);  // a shard's tiles share one L2
  const int s = lb / (NW * tiles);
  const int r = lb - s * NW * tiles;
  const int w = r / tiles, t = r - w * tiles;
  const int64_t n = off[s + 1] - off[s];
  const int chunks = (int)((n + C - 1) / C);
  const int64_t p0 = (int64_t)t * (kSortThreads * PER);
  if (p0 >= (int64_t)chunks * C) return;  // block-uniform
  unsigned long long* a = acc + (int64_t)s * kSsAcc;
  if (w >= 2 && a[kAccHalf] == 0) return;  // block-uniform: Tx' = Tx, Ty' = Ty
  const int64_t base = w * arr_stride + ss_slot0(off, s, C) * C;
  const SsTile<PER> tl = ss_load_tile<PER>(arrays + base, p0, chunks, n, C);
  bool ok[PER];
  uint32_t lo[PER], eq[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    // a double with the top key is a NaN (or, in arrays 2 and 3, a point that is not clean);
    // an int64 with the top key is INT64_MAX
    ok[e] = tl.real[e] && (!std::is_floating_point<T>::value || tl.k[e] != ~0ull);
    lo[e] = eq[e] = 0;
  }
  ss_search_chunks<PER>(arrays + base, chunks, n, C, keys, tl.k, ok, lo, eq);
  unsigned long long ties = 0;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    if (!ok[e]) continue;
    ties += eq[e] - 1;  // the key itself is among its equals
    if (w < 2) rank[base + p0 + e * kSortThreads + threadIdx.x] = lo[e];
  }
  ss_block_add(ties, a + w, part);  // kAccTx, kAccTy, kAccTxC, kAccTyC
}

// One thread per point: its ranks are those of its keys' first places in its own chunk's sorted
// arrays (one binary search each, in global memory); the composite key of a clean point.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ss_compose(
    const T* __restrict__ v, const int64_t* __restrict__ off, int tiles, int C,
    const uint64_t* __restrict__ arrays, int64_t arr_stride, const uint32_t* __restrict__ rank,
    uint64_t* __restrict__ comp, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long part[kBlock / kWave];
  const int s = (int)blockIdx.x / tiles, t = (int)blockIdx.x - s * tiles;
  const int64_t sb = off[s], n = off[s + 1] - sb;
  if ((int64_t)t * kBlock >= n) return;  // block-uniform
  const int64_t i = (int64_t)t * kBlock + threadIdx.x;
  bool clean = false;
  if (i < n) {
    const T pa = v[(sb + i) * 2], pb = v[(sb + i) * 2 + 1];
    clean = !is_nan_score<T>(pa) && !is_nan_score<T>(pb);
    uint64_t key = ~0ull;
    if (clean) {
      const int64_t base = (ss_slot0(off, s, C) + i / C) * C;
      const uint32_t ra = rank[base + lower_bound_lds(arrays + base, C, order_key<T>(pa))];
      const uint32_t rb = rank[arr_stride + base +
                               lower_bound_lds(arrays + arr_stride + base, C, order_key<T>(pb))];
      key = ((uint64_t)ra << 32) | rb;
    }
    comp[(sb - off[0]) + i] = key;
  }
  ss_block_add(clean, acc + (int64_t)s * kSsAcc + kAccV, part);
}

// One block per (shard, tile of 1024 PER chunk-slot positions) of the sorted composite chunks:
// the lexicographic position of every clean point, rb scattered there.
template <int PER>
__global__ __launch_bounds__(kSortThreads) void k_ss_order(
    const int64_t* __restrict__ off, int tiles, int C, const uint64_t* __restrict__ sorted,
    uint64_t* __restrict__ seq, unsigned long long* __restrict__ acc) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  __shared__ unsigned long long part[kSortThreads / kWave];
  const int lb = xcd_block(blockIdx.x, gridDim.x);
  const int s = lb / tiles, t = lb - s * tiles;
  const int64_t n = off[s + 1] - off[s];
  const int chunks = (int)((n + C - 1) / C);
  const int64_t p0 = (int64_t)t * (kSortThreads * PER);
  if (p0 >= (int64_t)chunks * C) return;  // block-uniform
  const uint64_t* __restrict__ src = sorted + ss_slot0(off, s, C) * C;
  const SsTile<PER> tl = ss_load_tile<PER>(src, p0, chunks, n, C);
  bool ok[PER];
  uint32_t below[PER], before[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    ok[e] = tl.k[e] != ~0ull;  // padding and the points that are not clean
    below[e] = before[e] = 0;
  }
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += kSortThreads) keys[i] = src[(int64_t)c * C + i];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      if (ok[e]) {
        const uint32_t l = lower_bound_lds(keys, C, tl.k[e]);
        below[e] += l;
        // equal keys ordered before this one: all of an earlier chunk's, and the run of its own
        // chunk up to its place (a clean key is below the padding: no clamp)
        if (c < tl.own[e]) before[e] += upper_bound_lds(keys, C, tl.k[e]) - l;
        else if (c == tl.own[e]) before[e] += tl.at[e] - l;
      }
    }
  }
  unsigned long long txy = 0;
  uint64_t* __restrict__ out = seq + (off[s] - off[0]);
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    if (ok[e]) {
      const int64_t pos = (int64_t)below[e] + before[e];
      if (pos < n) out[pos] = tl.k[e] & 0xFFFFFFFFull;
      txy += before[e];
    }
  }
  ss_block_add(txy, acc + (int64_t)s * kSsAcc + kAccTxy, part);
}

// One block per (shard, tile of chunk-slot positions of the sorted rb chunks, group of G
// earlier chunks): D += #{(x, y) : x in chunk p < q, y in chunk q, x > y}.
template <int PER>
__global__ __launch_bounds__(kSortThreads) void k_ss_cross(
    const int64_t* __restrict__ off, int tiles, int groups, int G, int C,
    const uint64_t* __restrict__ sorted, unsigned long long* __restrict__ acc) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  __shared__ unsigned long long part[kSortThreads / kWave];
  const int s = (int)blockIdx.x / (tiles * groups);
  const int r = (int)blockIdx.x - s * tiles * groups;
  const int t = r / groups, g = r - t * groups;
  const int64_t v = (int64_t)acc[(int64_t)s * kSsAcc + kAccV];
  const int chunks = (int)((v + C - 1) / C);
  const int64_t p0 = (int64_t)t * (kSortThreads * PER);
  if (p0 >= (int64_t)chunks * C) return;  // block-uniform, as is the next
  const int q_max = (int)std::min<int64_t>((p0 + kSortThreads * PER - 1) / C, chunks - 1);
  const int c_beg = g * G, c_end = std::min(c_beg + G, q_max);  // chunks c < q <= q_max
  if (c_beg >= c_end) return;
  const uint64_t* __restrict__ src = sorted + ss_slot0(off, s, C) * C;
  const SsTile<PER> tl = ss_load_tile<PER>(src, p0, chunks, v, C);
  unsigned long long d = 0;
  for (int c = c_beg; c < c_end; ++c) {
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += kSortThreads) keys[i] = src[(int64_t)c * C + i];
    __syncthreads();
    const uint32_t len = (uint32_t)std::min<int64_t>(C, v - (int64_t)c * C);
#pragma unroll
    for (int e = 0; e < PER; ++e)
      if (tl.real[e] && c < tl.own[e])
        d += len - std::min(upper_bound_lds(keys, C, tl.k[e]), len);
  }
  ss_block_add(d, acc + (int64_t)s * kSsAcc + kAccD, part);
}

__global__ __launch_bounds__(kBlock) void k_ss_final_kendall(
    const unsigned long long* __restrict__ acc, int n_shards, unsigned long long* __restrict__ out) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_shards) return;
  const unsigned long long* a = acc + (int64_t)s * kSsAcc;
  const unsigned long long tx = a[kAccTx] / 2, ty = a[kAccTy] / 2, txy = a[kAccTxy];
  const unsigned long long txc = a[kAccHalf] ? a[kAccTxC] / 2 : tx;
  const unsigned long long tyc = a[kAccHalf] ? a[kAccTyC] / 2 : ty;
  const unsigned long long v = a[kAccV], d = a[kAccD];
  const unsigned long long pv = v ? (v & 1 ? v * ((v - 1) / 2) : (v / 2) * (v - 1)) : 0;
  unsigned long long* o = out + (int64_t)s * 5;
  o[0] = pv - txc - tyc + txy - d;
  o[1] = d;
  o[2] = tx;
  o[3] = ty;
  o[4] = txy;
}

// ------------------------------------------------------------------------------ Gini
// One block per (shard, tile of 1024 kSsGiniPer chunk-slot positions) of the sorted chunks: the
// double-double partial sum of (lo + hi - n) s over the tile's finite values (the key decodes
// to the value; -0.0 comes back as 0.0), and the shard's non-finite counts.
__global__ __launch_bounds__(kSortThreads) void k_ss_gini(
    const int64_t* __restrict__ off, int tiles, int C, const uint64_t* __restrict__ sorted,
    double* __restrict__ part_out, unsigned long long* __restrict__ acc) {
  constexpr int PER = kSsGiniPer;
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  __shared__ unsigned long long part[kSortThreads / kWave];
  __shared__ ddv wpart[kSortThreads / kWave];
  const int lb = xcd_block(blockIdx.x, gridDim.x);
  const int s = lb / tiles, t = lb - s * tiles;
  const int64_t n = off[s + 1] - off[s];
  const int chunks = (int)((n + C - 1) / C);
  const int64_t p0 = (int64_t)t * (kSortThreads * PER);
  // block-uniform; k_ss_final_gini reads the tiles below the shard's last chunk only
  if (p0 >= (int64_t)chunks * C) return;
  const uint64_t* __restrict__ src = sorted + ss_slot0(off, s, C) * C;
  const SsTile<PER> tl = ss_load_tile<PER>(src, p0, chunks, n, C);
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  double x[PER];
  bool ok[PER];
  uint32_t lo[PER], eq[PER];
  unsigned long long nan = 0, pinf = 0, minf = 0;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    x[e] = key_to_double(tl.k[e]);  // the top key (a NaN item, padding) decodes to a NaN
    nan += tl.real[e] && x[e] != x[e];
    pinf += tl.real[e] && x[e] == inf;
    minf += tl.real[e] && x[e] == -inf;
    ok[e] = tl.real[e] && finite_d(x[e]);
    lo[e] = eq[e] = 0;
  }
  ss_search_chunks<PER>(src, chunks, n, C, keys, tl.k, ok, lo, eq);
  ddv sum = {0.0, 0.0};
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    if (ok[e]) {
      const double coef = (double)(2 * (int64_t)lo[e] + (int64_t)eq[e] - n);  // |coef| < 2^32
      sum = dd_add(sum, two_prod(coef, x[e]));
    }
  }
  // fixed order: butterfly in the wave, then the waves in order
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) sum = dd_add(sum, dd_shfl_xor(sum, o));
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) wpart[wid] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    ddv b = {0.0, 0.0};
    for (int w = 0; w < kSortThreads / kWave; ++w) b = dd_add(b, wpart[w]);
    part_out[((int64_t)s * tiles + t) * 2] = b.hi;
    part_out[((int64_t)s * tiles + t) * 2 + 1] = b.lo;
  }
  unsigned long long* a = acc + (int64_t)s * kSsAcc;
  ss_block_add(nan, a + 0, part);
  ss_block_add(pinf, a + 1, part);
  ss_block_add(minf, a + 2, part);
}

__global__ __launch_bounds__(kBlock) void k_ss_final_gini(
    const double* __restrict__ part, const unsigned long long* __restrict__ acc,
    const int64_t* __restrict__ off, int n_shards, int tiles, int C, double* __restrict__ out) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_shards) return;
  const int64_t n = off[s + 1] - off[s];
  const int64_t slots = (n + C - 1) / C * C;  // chunk-slot positions of the shard
  const int used = (int)((slots + kSortThreads * kSsGiniPer - 1) / (kSortThreads * kSsGiniPer));
  ddv b = {0.0, 0.0};
  for (int t = 0; t < used; ++t)
    b = dd_add(b, ddv{part[((int64_t)s * tiles + t) * 2], part[((int64_t)s * tiles + t) * 2 + 1]});
  const unsigned long long* a = acc + (int64_t)s * kSsAcc;
  double r = b.hi + b.lo;
  if (n < 2)
    r = 0.0;
  else if (a[0] || a[1] >= 2 || a[2] >= 2)
    r = __longlong_as_double(0x7FF8000000000000ll);  // a NaN term: NaN - s, inf - inf
  else if (a[1] || a[2])
    r = __longlong_as_double(0x7FF0000000000000ll);  // |+-inf - finite|, |inf - -inf|
  out[s] = r;
}

// ------------------------------------------------------------------------------ host
struct SsPlan {
  int C, E, per, chunks, tiles_point, tiles_slot, groups, G;
  int64_t arr_stride;                          // keys per sorted-chunk array
  int64_t arrays, rank, comp, seq, part, acc;  // workspace byte offsets
  int64_t bytes;
};

static bool ss_chunk_ok(int32_t chunk) {
  return chunk == 0 || (chunk >= 1024 && chunk <= kMaxChunk && (chunk & (chunk - 1)) == 0);
}

static SsPlan plan_ss(int32_t n_shards, int64_t total_n, int64_t max_n, int32_t kern,
                      int32_t chunk) {
  SsPlan p{};
  p.C = chunk ? chunk : kSsChunk;
  p.E = std::max(4, p.C / kSortThreads);
  const bool ken = kern == TW_SELF_KENDALL;
  // Kendall's integers do not depend on the tile: 4 points a lane once that still leaves most
  // CUs a block, else 1.  Gini's tile fixes its summation order and never changes.
  p.per = ken ? (ceil_div(total_n, kSortThreads * 4) >= 192 ? 4 : 1) : kSsGiniPer;
  const int64_t tile = (int64_t)kSortThreads * p.per;
  p.chunks = (int)std::max<int64_t>(1, ceil_div(max_n, p.C));
  p.tiles_point = (int)std::max<int64_t>(1, ceil_div(max_n, kBlock));  // k_ss_compose
  p.tiles_slot = (int)std::max<int64_t>(1, ceil_div((int64_t)p.chunks * p.C, tile));
  p.G = (int)std::max<int64_t>(kSsGroup, ceil_div(p.chunks, 64));
  p.groups = (int)ceil_div(p.chunks, p.G);
  p.arr_stride = (total_n / p.C + n_shards + 1) * p.C;
  auto al = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  p.arrays = 0;
  p.rank = al((ken ? 4 : 1) * p.arr_stride * 8);
  p.comp = p.rank + (ken ? al(2 * p.arr_stride * 4) : 0);
  p.seq = p.comp + (ken ? al(total_n * 8) : 0);
  p.part = p.seq + (ken ? al(total_n * 8) : 0);
  p.acc = p.part + (ken ? 0 : al((int64_t)n_shards * p.tiles_slot * 16));
  p.bytes = p.acc + al((int64_t)n_shards * kSsAcc * 8);
  return p;
}

template <typename F>
static int ss_by_E(int E, F f) {
  if (E == 4) return f(std::integral_constant<int, 4>{});
  if (E == 8) return f(std::integral_constant<int, 8>{});
  return f(std::integral_constant<int, 16>{});
}

// dynamic LDS above 64 KiB (chunks of 16384 keys) must be opted into
template <typename K, typename... A>
static int ss_launch(K kern, int64_t grid, int block, size_t lds, hipStream_t st, A... args) {
  if (lds > 64 * 1024)
    TW_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)block), lds, st, args...);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

#define SS_TRY(call)            \
  do {                          \
    const int rc_ = (call);     \
    if (rc_ != TW_OK) return rc_; \
  } while (0)

template <typename T, int PER>
static int ss_kendall(const SsPlan& p, const void* d_s, const int64_t* off, int32_t ns, void* work,
                      void* d_out, hipStream_t st) {
  char* w = (char*)work;
  uint64_t* arrays = (uint64_t*)(w + p.arrays);
  uint32_t* rank = (uint32_t*)(w + p.rank);
  uint64_t* comp = (uint64_t*)(w + p.comp);
  uint64_t* seq = (uint64_t*)(w + p.seq);
  unsigned long long* acc = (unsigned long long*)(w + p.acc);
  // the ranks are done with arrays 0 and 1 before the composite chunks (0) and the rb chunks (1)
  // are sorted into them
  uint64_t* comp_sorted = arrays;
  uint64_t* seq_sorted = arrays + p.arr_stride;
  const int NW = std::is_floating_point<T>::value ? 4 : 2;  // int64 has no NaN: no clean arrays
  const size_t lds = sizeof(uint64_t) * p.C;
  const int sort_threads = p.C / p.E;
  SS_TRY(ss_by_E(p.E, [&](auto e) {
    return ss_launch(k_ss_sort_vals<T, decltype(e)::value>, (int64_t)ns * NW * p.chunks,
                     sort_threads, lds, st, (const T*)d_s, off, p.chunks, p.C, 2, NW, arrays,
                     p.arr_stride, acc);
  }));
  SS_TRY(ss_launch(k_ss_count<T, PER>, (int64_t)ns * NW * p.tiles_slot, kSortThreads, lds, st, off,
                   p.tiles_slot, NW, p.C, (const uint64_t*)arrays, p.arr_stride, rank, acc));
  SS_TRY(ss_launch(k_ss_compose<T>, (int64_t)ns * p.tiles_point, kBlock, 0, st, (const T*)d_s, off,
                   p.tiles_point, p.C, (const uint64_t*)arrays, p.arr_stride,
                   (const uint32_t*)rank, comp, acc));
  SS_TRY(ss_by_E(p.E, [&](auto e) {
    return ss_launch(k_ss_sort_keys<decltype(e)::value, false>, (int64_t)ns * p.chunks,
                     sort_threads, lds, st, (const uint64_t*)comp, off, p.chunks, p.C, comp_sorted,
                     acc);
  }));
  SS_TRY(ss_launch(k_ss_order<PER>, (int64_t)ns * p.tiles_slot, kSortThreads, lds, st, off,
                   p.tiles_slot, p.C, (const uint64_t*)comp_sorted, seq, acc));
  SS_TRY(ss_by_E(p.E, [&](auto e) {
    return ss_launch(k_ss_sort_keys<decltype(e)::value, true>, (int64_t)ns * p.chunks,
                     sort_threads, lds, st, (const uint64_t*)seq, off, p.chunks, p.C, seq_sorted,
                     acc);
  }));
  if (p.chunks > 1)
    SS_TRY(ss_launch(k_ss_cross<PER>, (int64_t)ns * p.tiles_slot * p.groups, kSortThreads, lds, st,
                     off, p.tiles_slot, p.groups, p.G, p.C, (const uint64_t*)seq_sorted, acc));
  return ss_launch(k_ss_final_kendall, ceil_div(ns, kBlock), kBlock, 0, st,
                   (const unsigned long long*)acc, (int)ns, (unsigned long long*)d_out);
}

static int ss_gini(const SsPlan& p, const void* d_s, const int64_t* off, int32_t ns, void* work,
                   void* d_out, hipStream_t st) {
  char* w = (char*)work;
  uint64_t* sorted = (uint64_t*)(w + p.arrays);
  double* part = (double*)(w + p.part);
  unsigned long long* acc = (unsigned long long*)(w + p.acc);
  const size_t lds = sizeof(uint64_t) * p.C;
  SS_TRY(ss_by_E(p.E, [&](auto e) {
    return ss_launch(k_ss_sort_vals<double, decltype(e)::value>, (int64_t)ns * p.chunks,
                     p.C / p.E, lds, st, (const double*)d_s, off, p.chunks, p.C, 1, 1, sorted,
                     p.arr_stride, acc);
  }));
  SS_TRY(ss_launch(k_ss_gini, (int64_t)ns * p.tiles_slot, kSortThreads, lds, st, off, p.tiles_slot,
                   p.C, (const uint64_t*)sorted, part, acc));
  return ss_launch(k_ss_final_gini, ceil_div(ns, kBlock), kBlock, 0, st, (const double*)part,
                   (const unsigned long long*)acc, off, (int)ns, p.tiles_slot, p.C,
                   (double*)d_out);
}

}  // namespace tw

using namespace tw;

extern "C" int32_t tw_self_sorted_chunk(void) { return kSsChunk; }

extern "C" int64_t tw_self_sorted_work_bytes(int32_t n_shards, int64_t total_n, int64_t max_n,
                                             int32_t kern, int32_t chunk) {
  if (n_shards < 0 || total_n < 0 || max_n < 0 || max_n > total_n || !ss_chunk_ok(chunk) ||
      (kern != TW_SELF_GINI && kern != TW_SELF_KENDALL))
    return 0;
  return plan_ss(n_shards, total_n, max_n, kern, chunk).bytes;
}

extern "C" int tw_self_sorted(const void* d_s, const int64_t* d_off, int32_t n_shards,
                              int64_t total_n, int64_t max_n, int32_t dtype, int32_t kern,
                              int32_t chunk, void* d_work, void* d_out, void* stream) {
  TW_ARG_CHECK(n_shards >= 0, "tw_self_sorted: n_shards %d < 0", n_shards);
  TW_ARG_CHECK(total_n >= 0 && max_n >= 0 && max_n <= total_n,
               "tw_self_sorted: bad sizes (0 <= max_n %lld <= total_n %lld)", (long long)max_n,
               (long long)total_n);
  TW_ARG_CHECK(kern != TW_SELF_VAR,
               "tw_self_sorted: kern TW_SELF_VAR has no sorted path (the variance is O(n) from "
               "the moments)");
  TW_ARG_CHECK(kern == TW_SELF_GINI || kern == TW_SELF_KENDALL, "tw_self_sorted: unknown kern %d",
               kern);
  TW_ARG_CHECK(dtype == TW_F64 || dtype == TW_I64, "tw_self_sorted: unknown dtype %d", dtype);
  TW_ARG_CHECK(kern == TW_SELF_KENDALL || dtype == TW_F64,
               "tw_self_sorted: dtype TW_I64 with a float kern %d (float kernels take TW_F64)",
               kern);
  TW_ARG_CHECK(ss_chunk_ok(chunk),
               "tw_self_sorted: chunk %d is neither 0 nor a power of two in [1024, 16384]", chunk);
  TW_ARG_CHECK(max_n < (1ll << 31), "tw_self_sorted: a shard of %lld items (at most 2^31 - 1)",
               (long long)max_n);
  if (n_shards == 0) return TW_OK;
  TW_ARG_CHECK(d_work != nullptr, "tw_self_sorted: d_work is null");
  const SsPlan p = plan_ss(n_shards, total_n, max_n, kern, chunk);
  const int64_t widest =  // blocks per shard of the widest launch
      std::max<int64_t>({(int64_t)p.tiles_slot * std::max(p.groups, 4), 4ll * p.chunks,
                         (int64_t)p.tiles_point});
  TW_ARG_CHECK((int64_t)n_shards * widest < (1ll << 31), "tw_self_sorted: grid too large");
  hipStream_t st = (hipStream_t)stream;
  TW_HIP_CHECK(tw_zero_async((char*)d_work + p.acc, 0, (size_t)n_shards * kSsAcc * 8, st));
  if (kern == TW_SELF_GINI) return ss_gini(p, d_s, d_off, n_shards, d_work, d_out, st);
  if (dtype == TW_F64)
    return p.per == 4 ? ss_kendall<double, 4>(p, d_s, d_off, n_shards, d_work, d_out, st)
                      : ss_kendall<double, 1>(p, d_s, d_off, n_shards, d_work, d_out, st);
  return p.per == 4 ? ss_kendall<long long, 4>(p, d_s, d_off, n_shards, d_work, d_out, st)
                    : ss_kendall<long long, 1>(p, d_s, d_off, n_shards, d_work, d_out, st);
}
