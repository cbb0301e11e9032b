// kendall.hip — Kendall tau over MANY columns (tuplewise.kendall; an extension,
// not in the reference).  With s_a(i, j) = sign(S[i, a] - S[j, a]) the matrix
//     M[a, b] = sum_{i<j} s_a(i, j) s_b(i, j)          (C - D of columns a and b; M[a, a] = U_a)
// is Sgn^T Sgn of a (pairs x p) sign matrix that is generated on the fly and multiplied on the
// int8 matrix unit (v_mfma_i32_16x16x64_i8, int32 accumulators, exact).
//
// tw_col_ranks     every column of every shard -> its strict-less ranks r_i = #{j : x_j < x_i}
//                  (sortkeys.h order keys, chunk sorts in LDS, lower_bound summed over the
//                  shard's sorted chunks: the scheme of selfsorted.hip).  sign(r_i - r_j) =
//                  sign(x_i - x_j), the same for float64 and int64, in 16 or 32 bits.
// tw_kendall_matrix  walks the triangle of tile pairs (I <= J) of every shard.  A wave keeps 16
//                  points of tile J per column in registers (lane l: column 16 cb + (l & 15))
//                  and streams the anchors of tile I, 4 per matrix instruction (k-slab l >> 4):
//                  one instruction covers 64 pairs.  Byte j of a lane's 16-byte fragment is
//                  sign(anchor - point j); the SAME fragment is the A operand (rows) and the B
//                  operand (columns), so the product does not depend on how the hardware orders
//                  k inside a slab.  C/D: col = lane & 15, row = 4 (lane >> 4) + reg.
//                  A diagonal tile pair walks its full square (a self pair has sign 0, every
//                  other pair is met twice) and is added with weight 1, an off-diagonal one with
//                  weight 2: the work buffer holds 2 M, which k_km_final halves exactly.  Rows
//                  past a shard's end are masked in the packed sign registers, on the tile
//                  pairs that have such rows only.
#include "kendalltile.h"
#include "selfreduce.h"
#include "sortkeys.h"
#include <algorithm>
#include <type_traits>

namespace tw {

constexpr int kKrChunk = 4096;   // the largest chunk of the rank sorts (keys)
constexpr int kKrE = 4;          // keys per thread of a chunk sort
constexpr int kKrPer = 4;        // points per lane of the rank search
constexpr int kKrTile = kBlock * kKrPer;

constexpr int kKmG = 64;         // columns per group (4 blocks of 16)
constexpr int kKmMaxP = 1024;
constexpr int64_t kKmMax16 = 65536;  // the largest shard whose ranks fit 16 bits
constexpr int kKmGrid = 2048;    // default plan: about this many workgroups per launch

static int g_km_width = 0, g_km_flush = 0, g_km_plan = 0;

__device__ __forceinline__ int64_t kr_slot0(const int64_t* __restrict__ off, int s, int C) {
  return (off[s] - off[0]) / C + s;  // selfsorted.hip ss_slot0
}

// ------------------------------------------------------------------------------ ranks
// One block per (shard, column, chunk): the chunk's order keys sorted into `sorted`.  Shard s
// owns p (slot0(s + 1) - slot0(s)) chunk slots from slot0(s) p on; column col takes the
// ceil(n_s / C) of them that start at col ceil(n_s / C).
template <typename T>
__global__ __launch_bounds__(kSortThreads) void k_kr_sort(const T* __restrict__ v,
                                                          const int64_t* __restrict__ off, int p,
                                                          int chunks, int C,
                                                          uint64_t* __restrict__ sorted) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  const int c = (int)(blockIdx.x % (unsigned)chunks);
  const int64_t r = blockIdx.x / (unsigned)chunks;
  const int col = (int)(r % p), s = (int)(r / p);
  const int64_t sb = off[s], n = off[s + 1] - sb, c0 = (int64_t)c * C;
  if (c0 >= n) return;  // block-uniform
  const int64_t nch = (n + C - 1) / C;
  for (int i = threadIdx.x; i < C; i += blockDim.x)
    keys[i] = c0 + i < n ? order_key<T>(v[(sb + c0 + i) * p + col]) : ~0ull;
  __syncthreads();
  sort_keys_block<kKrE>(keys, C, sorted + (kr_slot0(off, s, C) * p + col * nch + c) * C);
}

// One block per (shard, column, tile of kKrTile points): r_i summed over the shard's sorted
// chunks of that column (padding and INT64_MAX share the top key; nothing is below it twice:
// lower_bound never counts a key that is not strictly less).  R: uint16_t (rank - 32768 read as
// int16) or int32_t.
template <typename T, typename R>
__global__ __launch_bounds__(kBlock) void k_kr_rank(const T* __restrict__ v,
                                                    const int64_t* __restrict__ off, int p,
                                                    int tiles, int C,
                                                    const uint64_t* __restrict__ sorted,
                                                    R* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  const int t = (int)(blockIdx.x % (unsigned)tiles);
  const int64_t r = blockIdx.x / (unsigned)tiles;
  const int col = (int)(r % p), s = (int)(r / p);
  const int64_t sb = off[s], n = off[s + 1] - sb, p0 = (int64_t)t * kKrTile;
  if (p0 >= n) return;  // block-uniform
  const int64_t nch = (n + C - 1) / C;
  const uint64_t* __restrict__ src = sorted + (kr_slot0(off, s, C) * p + col * nch) * C;
  uint64_t k[kKrPer];
  uint32_t lo[kKrPer];
  bool ok[kKrPer];
#pragma unroll
  for (int e = 0; e < kKrPer; ++e) {
    const int64_t i = p0 + e * kBlock + threadIdx.x;
    ok[e] = i < n;
    k[e] = ok[e] ? order_key<T>(v[(sb + i) * p + col]) : 0ull;
    lo[e] = 0;
  }
  for (int64_t c = 0; c < nch; ++c) {
    __syncthreads();  // the previous chunk's readers
    for (int i = threadIdx.x; i < C; i += kBlock) keys[i] = src[c * C + i];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kKrPer; ++e)
      if (ok[e]) lo[e] += lower_bound_lds(keys, C, k[e]);
  }
  R* __restrict__ o = out + (sb - off[0]) * p + (int64_t)col * n;
#pragma unroll
  for (int e = 0; e < kKrPer; ++e) {
    const int64_t i = p0 + e * kBlock + threadIdx.x;
    if (!ok[e]) continue;
    if constexpr (sizeof(R) == 2) o[i] = (R)(lo[e] ^ 0x8000u);
    else o[i] = (R)lo[e];
  }
}

static int kr_chunk_of(int64_t max_n) {
  return max_n <= 1024 ? 1024 : max_n <= 2048 ? 2048 : kKrChunk;
}

// ------------------------------------------------------------------------------ pair kernel
constexpr int kKmAcc = kKmG * kKmG;  // int64 sums of a group pair in LDS, then 2 x 64 for U
template <int W>
constexpr size_t km_lds_bytes(bool two) {
  return (size_t)(kKmAcc + 2 * kKmG) * 8 +
         (size_t)(two ? 2 : 1) * kKmG * KmTy<W>::kStride * sizeof(typename KmTy<W>::R);
}

// Rows [row0, row0 + T) of columns [col0, col0 + 16 nblk) of a shard's rank image (column-major,
// n rows, pcols columns) into st[col][kStride]; 0 for rows past n and columns past pcols.
template <int W>
__device__ __forceinline__ void km_stage(typename KmTy<W>::R* st,
                                         const typename KmTy<W>::R* __restrict__ img, int64_t n,
                                         int pcols, int col0, int nblk, int64_t row0) {
  using R = typename KmTy<W>::R;
  for (int idx = threadIdx.x; idx < nblk * 16 * kKmT; idx += kBlock) {
    const int col = idx / kKmT, row = idx - col * kKmT;
    R x = R(0);
    if (col0 + col < pcols && row0 + row < n) x = img[(int64_t)(col0 + col) * n + row0 + row];
    st[col * KmTy<W>::kStride + row] = x;
  }
}

// What one workgroup carries through its tile pairs.  DIAG: a diagonal group pair of the
// symmetric call (fragments 0..3 = the group's column blocks, products x <= y); else fragments
// 0..3 are the A columns, 4..7 the B columns, products (x, 4 + y), and the squares (x, x),
// (4 + y, 4 + y) where this group pair owes Ua / Ub.
template <int W, bool DIAG>
struct KmState {
  static constexpr int NF = DIAG ? 4 : 8;
  uint32_t pts[NF][KmTy<W>::kPR];
  v4i c[4][4];
  v4i cu[DIAG ? 1 : 8];
  int nca, ncb;
  bool ua, ub;
  // MODE 0: by the run-time block counts (uniform branches; any shape, and the flush hook).
  // MODE > 0: compile-time shapes without branches, so that the matrix instructions of a step
  // issue back to back — DIAG: MODE column blocks; else all 4 x 4 blocks, MODE 2 with all 8
  // squares (the flush keeps the owed ones).
  template <int MODE = 0>
  __device__ __forceinline__ bool frag_on(int f) const {
    if constexpr (MODE == 0) return f < 4 ? f < nca : f - 4 < ncb;
    else if constexpr (DIAG) return f < MODE;
    else return true;
  }
  template <int MODE = 0>
  __device__ __forceinline__ bool prod_on(int x, int y) const {
    if constexpr (MODE == 0) return DIAG ? (x <= y && y < nca) : (x < nca && y < ncb);
    else if constexpr (DIAG) return x <= y && y < MODE;
    else return true;
  }
  template <int MODE = 0>
  __device__ __forceinline__ bool sq_on(int f) const {
    if constexpr (DIAG) return false;
    else if constexpr (MODE == 0) return f < 4 ? ua && f < nca : ub && f - 4 < ncb;
    else return MODE == 2;
  }
};

// The int32 accumulators times `weight` into the workgroup's int64 sums in LDS, then zeroed.
template <int W, bool DIAG>
__device__ __forceinline__ void km_flush(KmState<W, DIAG>& st, long long* acc, int weight) {
  const int lane = threadIdx.x & (kWave - 1), c16 = lane & 15, h = lane >> 4;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      if (DIAG && x > y) continue;
      if (!st.prod_on(x, y)) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int v = st.c[x][y][g];
        if (v)
          atomicAdd((unsigned long long*)&acc[(16 * x + 4 * h + g) * kKmG + 16 * y + c16],
                    (unsigned long long)((long long)v * weight));
      }
      st.c[x][y] = v4i{0, 0, 0, 0};
    }
  }
  if constexpr (!DIAG) {
#pragma unroll
    for (int f = 0; f < 8; ++f) {
      if (!st.sq_on(f)) continue;
      // the diagonal of a 16 x 16 block: row 4 h + g == col c16
      const int g = c16 & 3;
      const int v = g == 0 ? st.cu[f][0] : g == 1 ? st.cu[f][1] : g == 2 ? st.cu[f][2] : st.cu[f][3];
      if ((c16 >> 2) == h && v)
        atomicAdd((unsigned long long*)&acc[kKmAcc + 16 * f + c16],
                  (unsigned long long)((long long)v * weight));
      st.cu[f] = v4i{0, 0, 0, 0};
    }
  }
}

// The 16 anchor steps of one tile pair: every anchor of the staged tile I against the wave's 16
// points.  EDGE: rows past the shard's end exist on this tile pair (pm: the wave's valid point
// bytes; an anchor past the end clears the whole fragment).
template <int W, bool DIAG, bool EDGE, int MODE>
__device__ __forceinline__ void km_steps(KmState<W, DIAG>& st, const typename KmTy<W>::R* stA,
                                         const typename KmTy<W>::R* stB, int64_t anchors_left,
                                         const uint32_t (&pm)[4], int flush, int& since,
                                         long long* acc, int weight) {
  using Ty = KmTy<W>;
  constexpr int NF = KmState<W, DIAG>::NF;
  const int lane = threadIdx.x & (kWave - 1), c16 = lane & 15, h = lane >> 4;
  const uint32_t m1 = 0xFFFFFFFFu, p1 = 0x00010001u;
  for (int ch = 0; ch < 16 / Ty::kAP; ++ch) {
    uint32_t an[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      if (!st.template frag_on<MODE>(f)) continue;
      const typename Ty::R* q = (f < 4 ? stA : stB) + (16 * (f & 3) + c16) * Ty::kStride + 16 * h +
                                ch * Ty::kAP;
      const uint4 u = *(const uint4*)q;
      an[f][0] = u.x;
      an[f][1] = u.y;
      an[f][2] = u.z;
      an[f][3] = u.w;
    }
    auto step = [&](auto tt_) {
      constexpr int TT = decltype(tt_)::value;
      v4i F[NF];
      uint32_t lm[4] = {0, 0, 0, 0};
      if constexpr (EDGE) {
        const bool av = 16 * h + ch * Ty::kAP + TT < anchors_left;
#pragma unroll
        for (int w = 0; w < 4; ++w) lm[w] = av ? pm[w] : 0u;
      }
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if (!st.template frag_on<MODE>(f)) continue;
        F[f] = km_frag<W, TT>(an[f], st.pts[f], m1, p1);
        if constexpr (EDGE) {
#pragma unroll
          for (int w = 0; w < 4; ++w) F[f][w] &= (int)lm[w];
        }
      }
#pragma unroll
      for (int x = 0; x < 4; ++x) {
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          if (DIAG && x > y) continue;
          if (!st.template prod_on<MODE>(x, y)) continue;
          st.c[x][y] = __builtin_amdgcn_mfma_i32_16x16x64_i8(F[x], F[DIAG ? y : 4 + y], st.c[x][y],
                                                             0, 0, 0);
        }
      }
      if constexpr (!DIAG) {
#pragma unroll
        for (int f = 0; f < 8; ++f) {
          if (!st.template sq_on<MODE>(f)) continue;
          st.cu[f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(F[f], F[f], st.cu[f], 0, 0, 0);
        }
      }
      if constexpr (MODE == 0) {
        if (flush > 0 && ++since >= flush) {
          km_flush<W, DIAG>(st, acc, weight);
          since = 0;
        }
      }
    };
    step(std::integral_constant<int, 0>{});
    step(std::integral_constant<int, 1>{});
    step(std::integral_constant<int, 2>{});
    step(std::integral_constant<int, 3>{});
    if constexpr (Ty::kAP == 8) {
      step(std::integral_constant<int, 4>{});
      step(std::integral_constant<int, 5>{});
      step(std::integral_constant<int, 6>{});
      step(std::integral_constant<int, 7>{});
    }
  }
}

template <int W, bool DIAG, bool EDGE>
__device__ __forceinline__ void km_modes(int mode, KmState<W, DIAG>& st,
                                         const typename KmTy<W>::R* stA,
                                         const typename KmTy<W>::R* stB, int64_t anchors_left,
                                         const uint32_t (&pm)[4], int flush, int& since,
                                         long long* acc, int weight) {
#define KM_GO(M) km_steps<W, DIAG, EDGE, M>(st, stA, stB, anchors_left, pm, flush, since, acc, weight)
  if (mode == 1) KM_GO(1);
  else if (mode == 2) KM_GO(2);
  else if (DIAG && mode == 3) KM_GO((DIAG ? 3 : 0));
  else if (DIAG && mode == 4) KM_GO((DIAG ? 4 : 0));
  else KM_GO(0);
#undef KM_GO
}

// A workgroup's tile pairs [p_beg, p_end) of the triangle of one shard and one group pair.
// Consecutive pairs share tile J (p = J (J + 1) / 2 + I): the point registers are reloaded only
// when J changes, tile I is staged for every pair.
template <int W, bool DIAG>
__device__ __forceinline__ void km_run(const typename KmTy<W>::R* __restrict__ imgA,
                                       const typename KmTy<W>::R* __restrict__ imgB, int64_t n,
                                       int pa, int pb, int colA0, int colB0, int nca, int ncb,
                                       bool ua, bool ub, int64_t p_beg, int64_t p_end, int flush,
                                       long long* acc, typename KmTy<W>::R* stA,
                                       typename KmTy<W>::R* stB) {
  using Ty = KmTy<W>;
  constexpr int NF = KmState<W, DIAG>::NF;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, c16 = lane & 15;
  KmState<W, DIAG> st;
  st.nca = nca;
  st.ncb = ncb;
  st.ua = ua;
  st.ub = ub;
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) st.c[x][y] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int f = 0; f < (DIAG ? 1 : 8); ++f) st.cu[f] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int k = 0; k < Ty::kPR; ++k) st.pts[f][k] = 0;
  int prevJ = -1, since = 0;
  const int mode = flush > 0 ? 0 : DIAG ? nca : (nca == 4 && ncb == 4) ? (ua || ub ? 2 : 1) : 0;
  for (int64_t p = p_beg; p < p_end; ++p) {
    int I, J;
    self_tile_of(p, I, J);
    if (J != prevJ) {
      __syncthreads();  // the previous pair's anchor reads
      km_stage<W>(stA, imgA, n, pa, colA0, nca, (int64_t)J * kKmT);
      if constexpr (!DIAG) km_stage<W>(stB, imgB, n, pb, colB0, ncb, (int64_t)J * kKmT);
      __syncthreads();
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if (!st.frag_on(f)) continue;
        const uint4* q = (const uint4*)((f < 4 ? stA : stB) + (16 * (f & 3) + c16) * Ty::kStride +
                                        16 * wv);
#pragma unroll
        for (int k = 0; k < Ty::kPR / 4; ++k) {
          const uint4 u = q[k];
          st.pts[f][4 * k] = u.x;
          st.pts[f][4 * k + 1] = u.y;
          st.pts[f][4 * k + 2] = u.z;
          st.pts[f][4 * k + 3] = u.w;
        }
      }
      prevJ = J;
    }
    __syncthreads();  // the point loads, or the previous pair's anchor reads
    km_stage<W>(stA, imgA, n, pa, colA0, nca, (int64_t)I * kKmT);
    if constexpr (!DIAG) km_stage<W>(stB, imgB, n, pb, colB0, ncb, (int64_t)I * kKmT);
    __syncthreads();
    const int weight = I == J ? 1 : 2;
    uint32_t pm[4] = {0, 0, 0, 0};
    if ((int64_t)(J + 1) * kKmT > n) {  // block-uniform: the shard ends inside tile J
      const int64_t left = n - ((int64_t)J * kKmT + 16 * wv);  // the wave's valid points
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int64_t b = std::min<int64_t>(4, std::max<int64_t>(0, left - 4 * w));
        pm[w] = b == 0 ? 0u : 0xFFFFFFFFu >> (32 - 8 * (int)b);
      }
      km_modes<W, DIAG, true>(mode, st, stA, stB, n - (int64_t)I * kKmT, pm, flush, since, acc,
                              weight);
    } else {
      km_modes<W, DIAG, false>(mode, st, stA, stB, kKmT, pm, flush, since, acc, weight);
    }
    km_flush<W, DIAG>(st, acc, weight);
    since = 0;
  }
}

// Block = (shard, group pair, workgroup of the plan).  sym: one image against itself — group
// pairs ga <= gb by the triangle index, the diagonal ones by their upper 16 x 16 blocks.  ONE:
// the symmetric call of at most 64 columns, whose only group pair is diagonal (the kernel
// without the cross path's registers).
template <int W, bool ONE>
__global__ __launch_bounds__(kBlock) void k_km(const void* __restrict__ ra_,
                                               const void* __restrict__ rb_,
                                               const int64_t* __restrict__ off, int pa, int pb,
                                               int sym, int ngp, int groups_b, int wgs, int flush,
                                               unsigned long long* __restrict__ m2,
                                               unsigned long long* __restrict__ u2a,
                                               unsigned long long* __restrict__ u2b) {
  using R = typename KmTy<W>::R;
  extern __shared__ __attribute__((aligned(16))) unsigned char km_smem[];
  long long* acc = (long long*)km_smem;
  R* stA = (R*)(acc + kKmAcc + 2 * kKmG);
  R* stB = stA + kKmG * KmTy<W>::kStride;
  const int w = (int)(blockIdx.x % (unsigned)wgs);
  const int64_t r = blockIdx.x / (unsigned)wgs;
  const int gp = (int)(r % ngp), s = (int)(r / ngp);
  int ga, gb;
  if (sym) self_tile_of(gp, ga, gb);
  else {
    ga = gp / groups_b;
    gb = gp - ga * groups_b;
  }
  const int64_t sb = off[s] - off[0], n = off[s + 1] - off[s];
  if (n < 2) return;  // block-uniform
  const int64_t nt = (n + kKmT - 1) / kKmT, tp = nt * (nt + 1) / 2;
  const int64_t q = tp / wgs, rem = tp - q * wgs;
  const int64_t p_beg = w * q + std::min<int64_t>(w, rem), p_end = p_beg + q + (w < rem ? 1 : 0);
  if (p_beg >= p_end) return;  // block-uniform
  for (int i = threadIdx.x; i < kKmAcc + 2 * kKmG; i += kBlock) acc[i] = 0;
  // (km_run's first barrier orders these stores before any flush)
  const int colA0 = ga * kKmG, colB0 = gb * kKmG;
  const int colsA = std::min(kKmG, pa - colA0), colsB = std::min(kKmG, pb - colB0);
  const int nca = (colsA + 15) / 16, ncb = (colsB + 15) / 16;
  const R* imgA = (const R*)ra_ + sb * pa;
  const R* imgB = (const R*)rb_ + sb * pb;
  const bool diag = ONE || (sym && ga == gb);
  if (diag)
    km_run<W, true>(imgA, imgA, n, pa, pa, colA0, colA0, nca, nca, false, false, p_beg, p_end,
                    flush, acc, stA, stA);
  else if constexpr (!ONE)
    km_run<W, false>(imgA, imgB, n, pa, pb, colA0, colB0, nca, ncb, !sym && gb == 0,
                     !sym && ga == 0, p_beg, p_end, flush, acc, stA, stB);
  __syncthreads();
  unsigned long long* m = m2 + (int64_t)s * pa * pb;
  for (int i = threadIdx.x; i < kKmAcc; i += kBlock) {
    const int row = i / kKmG, col = i - row * kKmG;
    const long long v = acc[i];
    if (v && row < colsA && col < colsB)
      atomicAdd(&m[(int64_t)(colA0 + row) * pb + colB0 + col], (unsigned long long)v);
  }
  if (!sym && threadIdx.x < 2 * kKmG) {
    const int i = threadIdx.x, c = i & (kKmG - 1);
    const long long v = acc[kKmAcc + i];
    if (i < kKmG) {
      if (gb == 0 && c < colsA && v) atomicAdd(&u2a[(int64_t)s * pa + colA0 + c], (unsigned long long)v);
    } else {
      if (ga == 0 && c < colsB && v) atomicAdd(&u2b[(int64_t)s * pb + colB0 + c], (unsigned long long)v);
    }
  }
}

// 2 M -> M (exact: every entry is even), the lower 16 x 16 blocks of the symmetric call from
// their mirrors, and U.
__global__ __launch_bounds__(kBlock) void k_km_final(const long long* __restrict__ m2,
                                                     const long long* __restrict__ u2a,
                                                     const long long* __restrict__ u2b,
                                                     int n_shards, int pa, int pb, int sym,
                                                     long long* __restrict__ m,
                                                     long long* __restrict__ ua,
                                                     long long* __restrict__ ub) {
  const int64_t per = (int64_t)pa * pb, total = per * n_shards;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
    const int64_t s = i / per, e = i - s * per;
    const int a = (int)(e / pb), b = (int)(e - (int64_t)a * pb);
    const bool mirror = sym && (a >> 4) > (b >> 4);
    m[i] = m2[s * per + (mirror ? (int64_t)b * pb + a : e)] / 2;
  }
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (int64_t)n_shards * pa;
       i += stride) {
    const int64_t s = i / pa, a = i - s * pa;
    ua[i] = (sym ? m2[s * per + a * pb + a] : u2a[i]) / 2;
  }
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (int64_t)n_shards * pb;
       i += stride) {
    const int64_t s = i / pb, b = i - s * pb;
    ub[i] = (sym ? m2[s * per + b * pb + b] : u2b[i]) / 2;
  }
}

static int64_t km_al(int64_t b) { return (b + 255) & ~(int64_t)255; }

}  // namespace tw

using namespace tw;

extern "C" int32_t tw_kendall_matrix_tile(void) { return kKmT; }

extern "C" int32_t tw_kendall_matrix_width(int64_t max_n) {
  if (max_n > kKmMax16) return 32;
  return g_km_width ? g_km_width : 16;
}

extern "C" int32_t tw_col_ranks_chunk(int64_t max_n) { return kr_chunk_of(max_n); }

extern "C" int32_t tw_kendall_matrix_set_width(int32_t width) {
  TW_ARG_CHECK(width == 0 || width == 16 || width == 32,
               "tw_kendall_matrix_set_width: width %d is not 0, 16 or 32", width);
  g_km_width = width;
  return TW_OK;
}

extern "C" int32_t tw_kendall_matrix_set_flush(int32_t k) {
  TW_ARG_CHECK(k >= 0 && k < (1 << 24),
               "tw_kendall_matrix_set_flush: %d instructions (0 = default, below 2^24)", k);
  g_km_flush = k;
  return TW_OK;
}

extern "C" int32_t tw_kendall_matrix_set_plan(int32_t max_wgs) {
  TW_ARG_CHECK(max_wgs >= 0, "tw_kendall_matrix_set_plan: max_wgs %d < 0", max_wgs);
  g_km_plan = max_wgs;
  return TW_OK;
}

extern "C" int64_t tw_col_ranks_work_bytes(int32_t n_shards, int64_t total_n, int64_t max_n,
                                           int32_t p) {
  if (n_shards < 0 || total_n < 0 || max_n < 0 || max_n > total_n || p < 1 || p > kKmMaxP)
    return 0;
  const int C = kr_chunk_of(max_n);
  return std::max<int64_t>(8, (total_n / C + n_shards + 1) * C * (int64_t)p * 8);
}

extern "C" int tw_col_ranks(const void* d_s, const int64_t* d_off, int32_t n_shards,
                            int64_t total_n, int64_t max_n, int32_t p, int32_t dtype,
                            int32_t width, void* d_work, void* d_ranks, void* stream) {
  TW_ARG_CHECK(n_shards >= 0, "tw_col_ranks: n_shards %d < 0", n_shards);
  TW_ARG_CHECK(total_n >= 0 && max_n >= 0 && max_n <= total_n,
               "tw_col_ranks: bad sizes (0 <= max_n %lld <= total_n %lld)", (long long)max_n,
               (long long)total_n);
  TW_ARG_CHECK(p >= 1 && p <= kKmMaxP, "tw_col_ranks: %d columns (1 to %d)", p, kKmMaxP);
  TW_ARG_CHECK(dtype == TW_F64 || dtype == TW_I64, "tw_col_ranks: unknown dtype %d", dtype);
  TW_ARG_CHECK(width == 16 || width == 32, "tw_col_ranks: width %d is not 16 or 32", width);
  TW_ARG_CHECK(width == 32 || max_n <= kKmMax16,
               "tw_col_ranks: a shard of %lld rows does not fit 16-bit ranks (at most 65536)",
               (long long)max_n);
  TW_ARG_CHECK(max_n < (1ll << 31), "tw_col_ranks: a shard of %lld rows (at most 2^31 - 1)",
               (long long)max_n);
  if (n_shards == 0 || max_n == 0) return TW_OK;
  TW_ARG_CHECK(d_s && d_off && d_work && d_ranks, "tw_col_ranks: a null buffer");
  const int C = kr_chunk_of(max_n);
  const int64_t chunks = ceil_div(max_n, C), tiles = ceil_div(max_n, kKrTile);
  TW_ARG_CHECK((int64_t)n_shards * p * std::max(chunks, tiles) < (1ll << 31),
               "tw_col_ranks: grid too large");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = sizeof(uint64_t) * C;
  const unsigned g1 = (unsigned)((int64_t)n_shards * p * chunks);
  const unsigned g2 = (unsigned)((int64_t)n_shards * p * tiles);
  uint64_t* sorted = (uint64_t*)d_work;
  auto run = [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((k_kr_sort<T>), dim3(g1), dim3(C / kKrE), lds, st, (const T*)d_s, d_off,
                       (int)p, (int)chunks, C, sorted);
    TW_LAUNCH_CHECK();
    if (width == 16)
      hipLaunchKernelGGL((k_kr_rank<T, uint16_t>), dim3(g2), dim3(kBlock), lds, st, (const T*)d_s,
                         d_off, (int)p, (int)tiles, C, (const uint64_t*)sorted,
                         (uint16_t*)d_ranks);
    else
      hipLaunchKernelGGL((k_kr_rank<T, int32_t>), dim3(g2), dim3(kBlock), lds, st, (const T*)d_s,
                         d_off, (int)p, (int)tiles, C, (const uint64_t*)sorted,
                         (int32_t*)d_ranks);
    TW_LAUNCH_CHECK();
    return TW_OK;
  };
  return dtype == TW_F64 ? run(double{}) : run((long long)0);
}

extern "C" int64_t tw_kendall_matrix_work_bytes(int32_t n_shards, int32_t pa, int32_t pb) {
  if (n_shards < 0 || pa < 1 || pa > kKmMaxP || pb < 1 || pb > kKmMaxP) return 0;
  return std::max<int64_t>(8, km_al((int64_t)n_shards * pa * pb * 8) +
                                  km_al((int64_t)n_shards * pa * 8) +
                                  km_al((int64_t)n_shards * pb * 8));
}

extern "C" int tw_kendall_matrix(const void* d_ra, int32_t pa, const void* d_rb, int32_t pb,
                                 const int64_t* d_off, int32_t n_shards, int64_t max_n,
                                 int32_t width, void* d_work, int64_t* d_m, int64_t* d_ua,
                                 int64_t* d_ub, void* stream) {
  TW_ARG_CHECK(n_shards >= 0, "tw_kendall_matrix: n_shards %d < 0", n_shards);
  TW_ARG_CHECK(max_n >= 0 && max_n < (1ll << 31),
               "tw_kendall_matrix: max_n %lld (0 to 2^31 - 1)", (long long)max_n);
  TW_ARG_CHECK(pa >= 1 && pa <= kKmMaxP && pb >= 1 && pb <= kKmMaxP,
               "tw_kendall_matrix: %d x %d columns (1 to %d each)", pa, pb, kKmMaxP);
  TW_ARG_CHECK(width == 16 || width == 32, "tw_kendall_matrix: width %d is not 16 or 32", width);
  TW_ARG_CHECK(width == 32 || max_n <= kKmMax16,
               "tw_kendall_matrix: a shard of %lld rows does not fit 16-bit ranks (at most 65536)",
               (long long)max_n);
  if (n_shards == 0) return TW_OK;
  TW_ARG_CHECK(d_ra && d_rb && d_off && d_work && d_m && d_ua && d_ub,
               "tw_kendall_matrix: a null buffer");
  const bool sym = d_ra == d_rb && pa == pb;
  const int groups_a = (int)ceil_div(pa, kKmG), groups_b = (int)ceil_div(pb, kKmG);
  const int ngp = sym ? groups_a * (groups_a + 1) / 2 : groups_a * groups_b;
  const int64_t nt = std::max<int64_t>(1, ceil_div(max_n, kKmT)), tp = nt * (nt + 1) / 2;
  const int64_t cap = g_km_plan ? g_km_plan
                                : std::max<int64_t>(1, ceil_div(kKmGrid, (int64_t)n_shards * ngp));
  const int64_t wgs = std::min(tp, cap);
  TW_ARG_CHECK((int64_t)n_shards * ngp * wgs < (1ll << 31), "tw_kendall_matrix: grid too large");
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)d_work;
  const int64_t b_m = km_al((int64_t)n_shards * pa * pb * 8), b_a = km_al((int64_t)n_shards * pa * 8);
  unsigned long long* m2 = (unsigned long long*)w;
  unsigned long long* u2a = (unsigned long long*)(w + b_m);
  unsigned long long* u2b = (unsigned long long*)(w + b_m + b_a);
  TW_HIP_CHECK(tw_zero_async(w, 0, (size_t)tw_kendall_matrix_work_bytes(n_shards, pa, pb), st));
  const bool two = !(sym && groups_a == 1);  // a second staged column set
  const unsigned grid = (unsigned)((int64_t)n_shards * ngp * wgs);
  auto launch = [&](auto kern, size_t lds) -> int {
    if (lds > 64 * 1024)
      TW_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, d_ra, d_rb, d_off, (int)pa,
                       (int)pb, (int)sym, ngp, groups_b, (int)wgs, g_km_flush, m2, u2a, u2b);
    return TW_OK;
  };
  int rc;
  if (width == 16)
    rc = two ? launch(k_km<16, false>, km_lds_bytes<16>(true))
             : launch(k_km<16, true>, km_lds_bytes<16>(false));
  else
    rc = two ? launch(k_km<32, false>, km_lds_bytes<32>(true))
             : launch(k_km<32, true>, km_lds_bytes<32>(false));
  if (rc != TW_OK) return rc;
  TW_LAUNCH_CHECK();
  const int64_t cells = (int64_t)n_shards * pa * pb;
  hipLaunchKernelGGL(k_km_final, dim3((unsigned)std::min<int64_t>(1024, ceil_div(cells, kBlock))),
                     dim3(kBlock), 0, st, (const long long*)m2, (const long long*)u2a,
                     (const long long*)u2b, (int)n_shards, (int)pa, (int)pb, (int)sym,
                     (long long*)d_m, (long long*)d_ua, (long long*)d_ub);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
