// kendall_rows.hip — the per-point row sums behind the variance of a Kendall tau matrix
// (tuplewise.kendall_var; an extension, not in the reference).  With
// s_a(i, j) = sign(S[i, a] - S[j, a]) over the rows of one shard and
//     c_i(a, b) = sum_{j != i} s_a(i, j) s_b(i, j)        (c_i(a, a) = u_i(a), the points not
//                                                          tied with i in column a)
// tw_kendall_rows returns R = sum_i c_i, Q = sum_i c_i^2, F[a, b] = sum_i c_i(a, b) u_i(a) and
// E[a, b] = sum_i u_i(a) u_i(b): exact int64, from one rank image of tw_col_ranks.
//
// A wave carries KA anchors (points i) at once.  Lane l holds column 16 cb + (l & 15) and, per
// 64-point chunk of the shard, the 16 points 16 (l >> 4) .. + 15: all four k-slabs of one
// v_mfma_i32_16x16x64_i8 belong to ONE anchor, the same km_frag fragment is the A and the B
// operand, and summed over all chunks of the shard the accumulators are c_i(a, b) itself
// (|c_i| < 2^20: no flush inside an anchor).  The point chunks are staged in LDS once per
// workgroup and 4 KA anchors and shared by its four waves (two buffers: the next step's loads
// are in flight while this step is computed).  After the last chunk a lane takes
// the diagonal u_i of its rows and columns from the lanes that hold it (ds_bpermute) and adds
// c, c^2, c u_i(row), c u_i(col) and u_i(row) u_i(col) to int64 sums in LDS (ds_add_u64); those
// go once per workgroup to the zeroed work buffer by int64 atomics, and k_kw_final mirrors.
//
// Work items: the diagonal group pairs (64 columns; NB = 1..4 column blocks, compile-time
// shapes, products x <= y) and, for p > 64, the pairs ga < gb in two halves of gb: 4 x 2 blocks
// and the 6 squares F_x F_x for both groups' diagonals on the matrix unit (the five int64 sum
// matrices of 4 x 4 blocks would not fit the LDS) — NB = 5 between two full groups, compile-time;
// NB = 0 against the partly filled last group, by run-time block counts.
#include "kendalltile.h"
#include "selfreduce.h"
#include <algorithm>

namespace tw {

constexpr int kKwG = 64;              // columns per group (4 blocks of 16)
constexpr int kKwMaxP = 1024;
constexpr int64_t kKwMax16 = 65536;   // the largest shard whose ranks fit 16 bits
constexpr int64_t kKwMaxN = 1 << 20;  // sum_i c^2 and sum_i c u stay below 2^63
constexpr int kKwGrid = 256;          // default plan: about this many workgroups per kernel launch
constexpr int kKwAnchors = 4;         // default anchors per wave (2 where 4 do not fit)
constexpr int kKwSums = 5;            // R, Q, F by rows, F by columns, E
constexpr int kKwBlk = 256;           // entries of a 16 x 16 block

static int g_kw_plan = 0, g_kw_anchors = 0;

template <int W>
struct KwTy {
  using R = typename KmTy<W>::R;
  static constexpr int kRows = W == 16 ? 128 : 64;             // rows per staging step
  static constexpr int kStride = kRows + 16 / (int)sizeof(R);  // 272 bytes a column
};

// NB 1..4: a diagonal group pair of NB column blocks, fragments 0..NB-1, products x <= y (the
// product (x, x) holds the diagonal).  NB 0 and 5: groups ga < gb — fragments 0..3 the blocks of
// ga, 4..5 two blocks of gb, products (x, 4 + y) and the squares of all six; 5: all in use.
template <int NB>
struct KwShape {
  static constexpr bool DIAG = NB >= 1 && NB <= 4;
  static constexpr bool FULL = NB == 5;
  static constexpr int NF = DIAG ? NB : 6;
  static constexpr int NX = DIAG ? NB : 4;
  static constexpr int NY = DIAG ? NB : 2;
  static constexpr int NP = DIAG ? NB * (NB + 1) / 2 : 8;
  static constexpr int NSQ = DIAG ? 1 : 6;
  static constexpr int pidx(int x, int y) {
    return DIAG ? x * NB - x * (x - 1) / 2 + (y - x) : 2 * x + y;
  }
};

template <int W, int NB>
constexpr size_t kw_lds_bytes() {
  return (size_t)kKwSums * KwShape<NB>::NP * kKwBlk * 8 +
         (size_t)2 * KwShape<NB>::NF * 16 * KwTy<W>::kStride * sizeof(typename KwTy<W>::R);
}

template <int W, int NB, int KA>
struct KwState {
  using Sh = KwShape<NB>;
  v4i c[KA][Sh::NP];
  v4i cu[KA][Sh::NSQ];
  int nca, ncb;  // NB 0: the blocks in use
  __device__ __forceinline__ bool frag_on(int f) const {
    if constexpr (Sh::DIAG || Sh::FULL) return true;
    else return f < 4 ? f < nca : f - 4 < ncb;
  }
  __device__ __forceinline__ bool prod_on(int x, int y) const {
    if constexpr (Sh::DIAG) return x <= y;
    else if constexpr (Sh::FULL) return true;
    else return x < nca && y < ncb;
  }
};

// A staging step in flight: rows [row0, row0 + kRows) of the item's 16 NF columns of a shard's
// rank image (column-major, n rows, p columns), NE elements a thread, element e of thread t at
// index e kBlock + t = col kRows + row (kRows is a multiple of the wave).  kw_fetch issues the loads (clamped into the image, so
// that none is predicated and all are in flight together) while the previous step is computed;
// kw_put writes them to st[col][kStride], 0 for rows past n and columns past p.
template <int W, int NB>
struct KwPre {
  static constexpr int NE = KwShape<NB>::NF * 16 * KwTy<W>::kRows / kBlock;
  typename KwTy<W>::R v[NE];
};

template <int W, int NB>
__device__ __forceinline__ void kw_fetch(KwPre<W, NB>& pre,
                                         const typename KwTy<W>::R* __restrict__ img, int64_t n,
                                         int p, int colA0, int colB0, int64_t row0) {
  using Ty = KwTy<W>;
#pragma unroll
  for (int e = 0; e < KwPre<W, NB>::NE; ++e) {
    // a wave's 64 threads share the column: its offsets stay in scalar registers
    const int col = e * (kBlock / Ty::kRows) + __builtin_amdgcn_readfirstlane(threadIdx.x / Ty::kRows);
    const int row = threadIdx.x % Ty::kRows;
    const int gc = col < 64 ? colA0 + col : colB0 + col - 64;
    pre.v[e] = img[(int64_t)std::min(gc, p - 1) * n + std::min<int64_t>(row0 + row, n - 1)];
  }
}

template <int W, int NB>
__device__ __forceinline__ void kw_put(const KwPre<W, NB>& pre, typename KwTy<W>::R* st, int64_t n,
                                       int p, int colA0, int colB0, int64_t row0) {
  using Ty = KwTy<W>;
  using R = typename Ty::R;
#pragma unroll
  for (int e = 0; e < KwPre<W, NB>::NE; ++e) {
    // a wave's 64 threads share the column: its offsets stay in scalar registers
    const int col = e * (kBlock / Ty::kRows) + __builtin_amdgcn_readfirstlane(threadIdx.x / Ty::kRows);
    const int row = threadIdx.x % Ty::kRows;
    const int gc = col < 64 ? colA0 + col : colB0 + col - 64;
    st[col * Ty::kStride + row] = gc < p && row0 + row < n ? pre.v[e] : R(0);
  }
}

// One 64-point chunk (staged at `stc`: the chunk's first row of column 0) against the wave's KA
// anchors.  EDGE: the shard ends inside this chunk (pm: the lane's valid point bytes).
template <int W, int NB, int KA, bool EDGE>
__device__ __forceinline__ void kw_chunk(KwState<W, NB, KA>& st, const typename KwTy<W>::R* stc,
                                         const uint32_t (&an)[KA][KwShape<NB>::NF],
                                         const uint32_t (&pm)[4]) {
  using Ty = KwTy<W>;
  using Sh = KwShape<NB>;
  constexpr int PR = KmTy<W>::kPR;
  const int lane = threadIdx.x & (kWave - 1), c16 = lane & 15, h = lane >> 4;
  const uint32_t m1 = 0xFFFFFFFFu, p1 = 0x00010001u;
  uint32_t pts[Sh::NF][PR];
#pragma unroll
  for (int f = 0; f < Sh::NF; ++f) {
    if (!st.frag_on(f)) continue;
    const uint4* q = (const uint4*)(stc + (16 * f + c16) * Ty::kStride + 16 * h);
#pragma unroll
    for (int k = 0; k < PR / 4; ++k) {
      const uint4 u = q[k];
      pts[f][4 * k] = u.x;
      pts[f][4 * k + 1] = u.y;
      pts[f][4 * k + 2] = u.z;
      pts[f][4 * k + 3] = u.w;
    }
  }
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    v4i F[Sh::NF];
#pragma unroll
    for (int f = 0; f < Sh::NF; ++f) {
      if (!st.frag_on(f)) continue;
      const uint32_t a4[4] = {an[k][f], 0u, 0u, 0u};
      F[f] = km_frag<W, 0>(a4, pts[f], m1, p1);
      if constexpr (EDGE) {
#pragma unroll
        for (int w = 0; w < 4; ++w) F[f][w] &= (int)pm[w];
      }
    }
#pragma unroll
    for (int x = 0; x < Sh::NX; ++x) {
#pragma unroll
      for (int y = 0; y < Sh::NY; ++y) {
        if (Sh::DIAG && x > y) continue;
        if (!st.prod_on(x, y)) continue;
        st.c[k][Sh::pidx(x, y)] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
            F[x], F[Sh::DIAG ? y : 4 + y], st.c[k][Sh::pidx(x, y)], 0, 0, 0);
      }
    }
    if constexpr (!Sh::DIAG) {
#pragma unroll
      for (int f = 0; f < Sh::NF; ++f) {
        if (!st.frag_on(f)) continue;
        st.cu[k][f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(F[f], F[f], st.cu[k][f], 0, 0, 0);
      }
    }
  }
}

__device__ __forceinline__ void kw_add(long long* p, long long v) {
  if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

// Anchor k is complete: its accumulators and diagonal into the workgroup's int64 sums.  C/D of a
// 16 x 16 block: col = lane & 15, row = 4 (lane >> 4) + reg, so the diagonal entry of column
// c16 sits in register c16 & 3 of lane 16 (c16 >> 2) + c16.
template <int W, int NB, int KA>
__device__ __forceinline__ void kw_epilogue(const KwState<W, NB, KA>& st, int k, long long* acc) {
  using Sh = KwShape<NB>;
  const int lane = threadIdx.x & (kWave - 1), c16 = lane & 15, h = lane >> 4;
  int ucol[Sh::NF], urow[Sh::NF][4];
#pragma unroll
  for (int f = 0; f < Sh::NF; ++f) {
    if (!st.frag_on(f)) continue;
    v4i dv;
    if constexpr (Sh::DIAG) dv = st.c[k][Sh::pidx(f, f)];
    else dv = st.cu[k][f];
    const int g = c16 & 3;
    const int d = g == 0 ? dv[0] : g == 1 ? dv[1] : g == 2 ? dv[2] : dv[3];
    ucol[f] = __shfl(d, 16 * (c16 >> 2) + c16, kWave);
#pragma unroll
    for (int r = 0; r < 4; ++r) urow[f][r] = __shfl(d, 16 * h + 4 * h + r, kWave);
  }
  constexpr int M = Sh::NP * kKwBlk;
#pragma unroll
  for (int x = 0; x < Sh::NX; ++x) {
#pragma unroll
    for (int y = 0; y < Sh::NY; ++y) {
      if (Sh::DIAG && x > y) continue;
      if (!st.prod_on(x, y)) continue;
      const int fy = Sh::DIAG ? y : 4 + y;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long v = st.c[k][Sh::pidx(x, y)][r];
        const long long ur = urow[x][r], uc = ucol[fy];
        long long* a = acc + Sh::pidx(x, y) * kKwBlk + (4 * h + r) * 16 + c16;
        if (v) {
          kw_add(a, v);
          kw_add(a + M, v * v);
          kw_add(a + 2 * M, v * ur);
          kw_add(a + 3 * M, v * uc);
        }
        kw_add(a + 4 * M, ur * uc);
      }
    }
  }
}

// The anchors [a_beg, a_end) of one shard for one work item, 4 KA at a time: anchor
// a0 + KA wave + k, each against every chunk of the shard.
template <int W, int NB, int KA>
__device__ __forceinline__ void kw_run(const typename KwTy<W>::R* __restrict__ img, int64_t n,
                                       int p, int colA0, int colB0, int nca, int ncb,
                                       int64_t a_beg, int64_t a_end, long long* acc,
                                       typename KwTy<W>::R* stg) {
  using Ty = KwTy<W>;
  using Sh = KwShape<NB>;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, c16 = lane & 15,
            h = lane >> 4;
  constexpr int kStg = Sh::NF * 16 * Ty::kStride;  // elements of a staging buffer
  KwState<W, NB, KA> st;
  st.nca = nca;
  st.ncb = ncb;
  for (int64_t a0 = a_beg; a0 < a_end; a0 += 4 * KA) {
    uint32_t an[KA][Sh::NF];
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      // an anchor past the run is computed on row n - 1 and dropped
      const int64_t i = std::min<int64_t>(a0 + KA * wv + k, n - 1);
#pragma unroll
      for (int f = 0; f < Sh::NF; ++f) {
        const int col = (f < 4 ? colA0 + 16 * f : colB0 + 16 * (f - 4)) + c16;
        an[k][f] = st.frag_on(f) && col < p ? (uint32_t)img[(int64_t)col * n + i] : 0u;
      }
#pragma unroll
      for (int q = 0; q < Sh::NP; ++q) st.c[k][q] = v4i{0, 0, 0, 0};
#pragma unroll
      for (int q = 0; q < Sh::NSQ; ++q) st.cu[k][q] = v4i{0, 0, 0, 0};
    }
    // two staging buffers: step it + 1 is fetched before and written after step it is computed,
    // one barrier a step
    KwPre<W, NB> pre;
    kw_fetch<W, NB>(pre, img, n, p, colA0, colB0, 0);
    __syncthreads();  // the previous anchors' last point reads (and the zeroed sums)
    kw_put<W, NB>(pre, stg, n, p, colA0, colB0, 0);
    int buf = 0;
    for (int64_t row0 = 0; row0 < n; row0 += Ty::kRows, buf ^= 1) {
      __syncthreads();  // this step's points are written, the other buffer's readers are done
      const bool more = row0 + Ty::kRows < n;  // block-uniform
      if (more) kw_fetch<W, NB>(pre, img, n, p, colA0, colB0, row0 + Ty::kRows);
      const typename Ty::R* cur = stg + buf * kStg;
      const int nch = (int)std::min<int64_t>(Ty::kRows / 64, (n - row0 + 63) / 64);
      for (int ch = 0; ch < nch; ++ch) {
        const int64_t left = n - (row0 + 64 * ch);  // block-uniform
        uint32_t pm[4] = {0, 0, 0, 0};
        if (left < 64) {
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const int64_t b = std::min<int64_t>(4, std::max<int64_t>(0, left - 16 * h - 4 * w));
            pm[w] = b == 0 ? 0u : 0xFFFFFFFFu >> (32 - 8 * (int)b);
          }
          kw_chunk<W, NB, KA, true>(st, cur + 64 * ch, an, pm);
        } else {
          kw_chunk<W, NB, KA, false>(st, cur + 64 * ch, an, pm);
        }
      }
      if (more) kw_put<W, NB>(pre, stg + (buf ^ 1) * kStg, n, p, colA0, colB0, row0 + Ty::kRows);
    }
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (a0 + KA * wv + k < a_end) kw_epilogue<W, NB, KA>(st, k, acc);  // wave-uniform
  }
}

// Block = (shard, work item, workgroup of the plan).  NB 1..4: the item is diagonal group
// g0 + item (all of NB blocks).  NB 5: item = 2 pair + half, the pairs ga < gb < g0 of the strict
// triangle of full groups.  NB 0: item = 2 ga + half against gb = g0, the partly filled last
// group.  work: kKwSums x (n_shards, p, p) int64, zeroed.
template <int W, int NB, int KA>
__global__ __launch_bounds__(kBlock) void k_kw(const void* __restrict__ ranks,
                                               const int64_t* __restrict__ off, int p, int g0,
                                               int items, int wgs, int64_t sum_stride,
                                               unsigned long long* __restrict__ work) {
  using R = typename KwTy<W>::R;
  using Sh = KwShape<NB>;
  extern __shared__ __attribute__((aligned(16))) unsigned char kw_smem[];
  long long* acc = (long long*)kw_smem;
  constexpr int M = Sh::NP * kKwBlk;
  R* stg = (R*)(acc + kKwSums * M);
  const int w = (int)(blockIdx.x % (unsigned)wgs);
  const int64_t r = blockIdx.x / (unsigned)wgs;
  const int item = (int)(r % items), s = (int)(r / items);
  int colA0, colB0, nca, ncb;
  if constexpr (Sh::DIAG) {
    colA0 = colB0 = (g0 + item) * kKwG;
    nca = ncb = NB;
  } else {
    int I = item >> 1, J = g0 - 1;
    if constexpr (Sh::FULL) self_tile_of(item >> 1, I, J);  // ga = I <= J = gb - 1
    colA0 = I * kKwG;
    colB0 = (J + 1) * kKwG + 32 * (item & 1);
    if (colB0 >= p) return;  // block-uniform: the last group has no second half
    nca = 4;                 // ga is never the last group
    ncb = std::min(2, (p - colB0 + 15) / 16);
  }
  const int64_t sb = off[s] - off[0], n = off[s + 1] - off[s];
  if (n < 2) return;  // block-uniform
  int64_t per = (n + wgs - 1) / wgs;
  per = (per + 4 * KA - 1) / (4 * KA) * (4 * KA);
  const int64_t a_beg = w * per, a_end = std::min(n, a_beg + per);
  if (a_beg >= a_end) return;  // block-uniform
  for (int i = threadIdx.x; i < kKwSums * M; i += kBlock) acc[i] = 0;
  // (kw_run's first barrier orders these stores before any epilogue)
  kw_run<W, NB, KA>((const R*)ranks + sb * p, n, p, colA0, colB0, nca, ncb, a_beg, a_end, acc,
                    stg);
  __syncthreads();
  for (int i = threadIdx.x; i < kKwSums * M; i += kBlock) {
    const long long v = acc[i];
    if (!v) continue;
    const int m = i / M, e = i - m * M, q = e / kKwBlk, row = (e >> 4) & 15, col = e & 15;
    int x = 0, y = 0;  // the product q
#pragma unroll
    for (int xx = 0; xx < Sh::NX; ++xx)
#pragma unroll
      for (int yy = 0; yy < Sh::NY; ++yy)
        if ((!Sh::DIAG || xx <= yy) && Sh::pidx(xx, yy) == q) {
          x = xx;
          y = yy;
        }
    const int a = colA0 + 16 * x + row, b = colB0 + 16 * y + col;
    if (a < p && b < p)
      atomicAdd(&work[m * sum_stride + ((int64_t)s * p + a) * p + b], (unsigned long long)v);
  }
}

// The work buffer holds the entries whose 16-column block of a is not past that of b.  R, Q and
// E are symmetric; F[a, b] pairs c(a, b) with u(a): by rows where (a, b) is held, else (b, a)'s
// sum by columns.
__global__ __launch_bounds__(kBlock) void k_kw_final(const long long* __restrict__ work,
                                                     int64_t sum_stride, int n_shards, int p,
                                                     long long* __restrict__ R,
                                                     long long* __restrict__ Q,
                                                     long long* __restrict__ F,
                                                     long long* __restrict__ E) {
  const int64_t per = (int64_t)p * p, total = per * n_shards;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
    const int64_t s = i / per, e = i - s * per;
    const int a = (int)(e / p), b = (int)(e - (int64_t)a * p);
    const bool mirror = (a >> 4) > (b >> 4);
    const int64_t src = s * per + (mirror ? (int64_t)b * p + a : e);
    R[i] = work[src];
    Q[i] = work[sum_stride + src];
    F[i] = work[(mirror ? 3 : 2) * sum_stride + src];
    E[i] = work[4 * sum_stride + src];
  }
}

static int64_t kw_al(int64_t b) { return (b + 255) & ~(int64_t)255; }

// KA anchors a wave where they fit the 512 registers: 4 anchors spill between two groups (56
// accumulators an anchor) and, by 3 registers, at 4 column blocks of int32 ranks; those run 2,
// and the run-time shape of int32 ranks, which spills 2 registers at 2 anchors, runs 1.
template <int W, int NB, int KA>
static int kw_launch(const void* ranks, const int64_t* off, int p, int g0, int items,
                     int64_t max_n, int n_shards, int64_t sum_stride, unsigned long long* work,
                     hipStream_t st) {
  constexpr size_t lds = kw_lds_bytes<W, NB>();
  static_assert(lds <= 160 * 1024, "the sums and the staged points fit the LDS");
  constexpr int K = NB == 0 && W == 32 ? 1
                    : KA > 2 && (NB == 0 || NB == 5 || (NB == 4 && W == 32)) ? 2 : KA;
  // the plan of this launch: each launch fills the device by itself (they run one after the
  // other), with the anchors that really run
  const int64_t cap = g_kw_plan ? g_kw_plan
                                : std::max<int64_t>(1, ceil_div(kKwGrid, (int64_t)n_shards * items));
  const int wgs = (int)std::min(std::max<int64_t>(1, ceil_div(max_n, 4 * K)), cap);
  auto kern = k_kw<W, NB, K>;
  if (lds > 64 * 1024)
    TW_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)n_shards * items * wgs)), dim3(kBlock), lds, st,
                     ranks, off, p, g0, items, wgs, sum_stride, work);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

template <int W, int KA>
static int kw_launch_nb(int nb, const void* ranks, const int64_t* off, int p, int g0, int items,
                        int64_t max_n, int n_shards, int64_t sum_stride, unsigned long long* work,
                        hipStream_t st) {
#define KW_GO(NB) kw_launch<W, NB, KA>(ranks, off, p, g0, items, max_n, n_shards, sum_stride, work, st)
  switch (nb) {
    case 0: return KW_GO(0);
    case 1: return KW_GO(1);
    case 2: return KW_GO(2);
    case 3: return KW_GO(3);
    case 4: return KW_GO(4);
    default: return KW_GO(5);
  }
#undef KW_GO
}

}  // namespace tw

using namespace tw;

extern "C" int32_t tw_kendall_rows_set_plan(int32_t max_wgs) {
  const int32_t old = g_kw_plan;
  if (max_wgs < 0) {
    set_error("tw_kendall_rows_set_plan: max_wgs %d < 0", max_wgs);
    return -1;
  }
  g_kw_plan = max_wgs;
  return old;
}

extern "C" int32_t tw_kendall_rows_set_anchors(int32_t k) {
  const int32_t old = g_kw_anchors;
  if (k != 0 && k != 1 && k != 2 && k != 4) {
    set_error("tw_kendall_rows_set_anchors: %d anchors per wave is not 0 (default), 1, 2 or 4", k);
    return -1;
  }
  g_kw_anchors = k;
  return old;
}

extern "C" int64_t tw_kendall_rows_work_bytes(int32_t n_shards, int32_t p) {
  if (n_shards < 0 || p < 1 || p > kKwMaxP) return 0;
  return std::max<int64_t>(8, kKwSums * kw_al((int64_t)n_shards * p * p * 8));
}

extern "C" int tw_kendall_rows(const void* d_ranks, int32_t p, const int64_t* d_off,
                               int32_t n_shards, int64_t max_n, int32_t width, void* d_work,
                               int64_t* d_r, int64_t* d_q, int64_t* d_f, int64_t* d_e,
                               void* stream) {
  TW_ARG_CHECK(n_shards >= 0, "tw_kendall_rows: n_shards %d < 0", n_shards);
  TW_ARG_CHECK(max_n >= 0 && max_n <= kKwMaxN, "tw_kendall_rows: max_n %lld (0 to 2^20)",
               (long long)max_n);
  TW_ARG_CHECK(p >= 1 && p <= kKwMaxP, "tw_kendall_rows: %d columns (1 to %d)", p, kKwMaxP);
  TW_ARG_CHECK(width == 16 || width == 32, "tw_kendall_rows: width %d is not 16 or 32", width);
  TW_ARG_CHECK(width == 32 || max_n <= kKwMax16,
               "tw_kendall_rows: a shard of %lld rows does not fit 16-bit ranks (at most 65536)",
               (long long)max_n);
  if (n_shards == 0) return TW_OK;
  TW_ARG_CHECK(d_ranks && d_off && d_work && d_r && d_q && d_f && d_e,
               "tw_kendall_rows: a null buffer");
  const int ka = g_kw_anchors ? g_kw_anchors : kKwAnchors;
  const int groups = (int)ceil_div(p, kKwG), full = p / kKwG;
  const int last_nb = (int)ceil_div(p - full * kKwG, 16);  // blocks of a partly filled last group
  const int off_full = full * (full - 1);                  // pairs ga < gb of full groups, two
  const int off_last = last_nb > 0 ? 2 * full : 0;         // halves each; pairs with the last
  const int off_items = std::max(off_full, off_last);
  // (an upper bound of every launch's workgroups per shard and item)
  const int64_t wmax = std::min<int64_t>(std::max<int64_t>(1, ceil_div(max_n, 4)),
                                         g_kw_plan ? g_kw_plan : kKwGrid);
  TW_ARG_CHECK((int64_t)n_shards * std::max<int64_t>(groups, off_items) * wmax < (1ll << 31),
               "tw_kendall_rows: grid too large");
  hipStream_t st = (hipStream_t)stream;
  const int64_t b_sum = kw_al((int64_t)n_shards * p * p * 8), sum_stride = b_sum / 8;
  unsigned long long* work = (unsigned long long*)d_work;
  TW_HIP_CHECK(tw_zero_async(d_work, 0, (size_t)(kKwSums * b_sum), st));
  auto go = [&](auto w_, auto ka_) -> int {
    constexpr int W = decltype(w_)::value, KA = decltype(ka_)::value;
    int rc = TW_OK;
    if (full > 0)
      rc = kw_launch_nb<W, KA>(4, d_ranks, d_off, p, 0, full, max_n, n_shards, sum_stride, work, st);
    if (rc == TW_OK && last_nb > 0)
      rc = kw_launch_nb<W, KA>(last_nb, d_ranks, d_off, p, full, 1, max_n, n_shards, sum_stride,
                               work, st);
    if (rc == TW_OK && off_full > 0)
      rc = kw_launch_nb<W, KA>(5, d_ranks, d_off, p, full, off_full, max_n, n_shards, sum_stride,
                               work, st);
    if (rc == TW_OK && off_last > 0)
      rc = kw_launch_nb<W, KA>(0, d_ranks, d_off, p, full, off_last, max_n, n_shards, sum_stride,
                               work, st);
    return rc;
  };
  using I16 = std::integral_constant<int, 16>;
  using I32 = std::integral_constant<int, 32>;
  using K1 = std::integral_constant<int, 1>;
  using K2 = std::integral_constant<int, 2>;
  using K4 = std::integral_constant<int, 4>;
  int rc;
  if (width == 16) rc = ka == 1 ? go(I16{}, K1{}) : ka == 2 ? go(I16{}, K2{}) : go(I16{}, K4{});
  else rc = ka == 1 ? go(I32{}, K1{}) : ka == 2 ? go(I32{}, K2{}) : go(I32{}, K4{});
  if (rc != TW_OK) return rc;
  const int64_t cells = (int64_t)n_shards * p * p;
  hipLaunchKernelGGL(k_kw_final, dim3((unsigned)std::min<int64_t>(1024, ceil_div(cells, kBlock))),
                     dim3(kBlock), 0, st, (const long long*)work, sum_stride, (int)n_shards, (int)p,
                     (long long*)d_r, (long long*)d_q, (long long*)d_f, (long long*)d_e);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
