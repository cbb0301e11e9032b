// mmd_perm.hip — the permutation test of the kernel two-sample statistics (tuplewise.mmd
// permutation_sums / permutation_test; an extension, not in the reference): the
// three sums of tw_mmd_sums for EVERY relabelling of the pooled sample in one launch.
// Under a permutation only the labels of the pooled rows w_0 .. w_{N-1} change, the values
// g_ij = g(w_i, w_j) do not.  With s[i] = 1 iff row i is in the first sample under a column,
//   Sxx = sum_{i<j} s[i] s[j] g_ij     A = sum_{i<j} (s[i] + s[j]) g_ij     T = sum_{i<j} g_ij
//   Sxz = A - 2 Sxx                    Szz = T - A + Sxx
// so a g is evaluated once per pass of kPermC columns and the label products are a float64
// matrix product G S, on v_mfma_f64_16x16x4_f64.  Work items are the triangle of kMmdT-row tile
// pairs of the pooled sample (a diagonal tile counts anchor > point only); a wave computes the
// squared distances of 16 anchors by 128 points exactly as k_mmd_sums does (trip_chunk), applies
// mmd_g, and lays the 16 x 64 doubles of each half of the points over ITS OWN anchors in LDS
// (they are read no more), rotated by 4 doubles a row so that the A fragments (lane l: anchor
// l & 15, point 4 ks + (l >> 4)) are read two lanes a bank.  B fragments (lane l: point
// 4 ks + (l >> 4), column l & 15) are the label bits of the tile's points, staged once per item in
// LDS, as 0.0 / 1.0.  C/D is the f64 layout: column = lane & 15, anchor = (lane >> 4) + 4 * reg.
// The column blocks of a pass are accumulated kPermGB at a time over the 16 k-steps of a half
// (so that two workgroups fit a CU's registers), and after each group the epilogue adds, per lane
// and column block,
//   sxx += s[anchor] * C    A += C + s[anchor] * R
// where R = G 1 (one more accumulator with B = 1.0, formed beside the half's first group) are the
// anchors' row sums over the half, T their sum.
// Products with an exact 0.0 / 1.0 are exact, so every sum is a plain sum of g in the kernel's
// order; a NaN coordinate makes every column NaN (0 * NaN).  A column's sums depend only on the
// rows and on that column's labels: the partition of the items over workgroups depends on n_rows
// alone, every column of a block meets the same instructions in the same order, and
// k_mmd_perm_reduce adds a column's partials in k_self_reduce's fixed order.  No atomics and
// nothing to zero.
#include "tw_common.h"
#include "selfreduce.h"
#include "tripdist.h"
#include "mmdtile.h"
#include <algorithm>
#include <cmath>

namespace tw {

#ifndef TW_MMD_PERM_COLS
#define TW_MMD_PERM_COLS 128  // (tools/time_mmd_perm.py --lib times other builds: make ab-mmdperm)
#endif
constexpr int kPermC = TW_MMD_PERM_COLS;       // columns (permutations) per pass
constexpr int kPermCB = kPermC / 16;           // column blocks of one MFMA tile
constexpr int kPermGB = 4;                     // column blocks accumulated together
static_assert(kPermCB % kPermGB == 0, "whole groups of column blocks");
constexpr int kPermWords = kPermC / 32;        // label words of a row per pass: whole uint4s
constexpr int kPermSlots = 2 * kPermC + 16;    // doubles a workgroup leaves: sxx, A, T
constexpr int64_t kPermMaxWG = 512;            // workgroups per pass, at most (2 a CU)
constexpr int kPermHalf = kWave;               // points of one half of a tile (one r of a lane)
static_assert(kPermC % 128 == 0, "a row's label words of a pass are read as whole uint4s");
static_assert(kTripTA == 16 && kTripMaxD == kPermHalf, "a wave's anchors hold its 16 x 64 g");
static_assert(kPermSlots * (kBlock / kWave) <= kMmdSA * kTripMaxD, "the block sums fit in sa");

// Two workgroups a CU (two waves a SIMD: one's loads and LDS reads behind the other's arithmetic)
// fit the register file at 128 columns a pass; the 256-column A/B build runs one.
#if TW_MMD_PERM_COLS <= 128
#define TW_MMD_PERM_WAVES __attribute__((amdgpu_waves_per_eu(2, 2)))
#else
#define TW_MMD_PERM_WAVES
#endif

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct PermPlan {
  int64_t items, ipw;  // tile pairs, and tile pairs per workgroup
  int64_t wgs;         // workgroups per pass
};
// Depends on n_rows alone: a column's partials are the same whatever n_perm is.
inline PermPlan perm_plan(int64_t n_rows) {
  const int64_t t = ceil_div(n_rows, kMmdT);
  PermPlan p;
  p.items = t * (t + 1) / 2;
  p.ipw = std::max<int64_t>(1, ceil_div(p.items, kPermMaxWG));
  p.wgs = ceil_div(p.items, p.ipw);
  return p;
}

// Bit `bit` of a label word as 0.0 / 1.0.
__device__ __forceinline__ double perm_label(uint32_t word, int bit) {
  return __hiloint2double(((word >> bit) & 1u) ? 0x3FF00000 : 0, 0);
}
struct PermWords {
  uint4 v[kPermWords / 4];
  __device__ __forceinline__ uint32_t operator[](int k) const {  // k is a compile-time constant
    const uint4& q = v[k >> 2];
    return (k & 3) == 0 ? q.x : (k & 3) == 1 ? q.y : (k & 3) == 2 ? q.z : q.w;
  }
};
__device__ __forceinline__ PermWords perm_words(const uint4* rows, int row) {
  PermWords w;
#pragma unroll
  for (int k = 0; k < kPermWords / 4; ++k) w.v[k] = rows[row * (kPermWords / 4) + k];
  return w;
}

// Workgroup blockIdx.x = (pass, group of ipw consecutive tile pairs).
template <int K>
__global__ __launch_bounds__(kBlock) TW_MMD_PERM_WAVES void k_mmd_perm(
    const double* __restrict__ w, int64_t n, int d, const uint32_t* __restrict__ labels,
    int64_t n_words, int n_perm, int64_t items, int64_t ipw, int wgs, double c,
    double* __restrict__ work) {
  __shared__ double sa[kMmdSA * kTripMaxD];
  // the label words of the item's points and anchors, kPermWords a row
  __shared__ uint4 lp[kMmdT * (kPermWords / 4)], la[kMmdT * (kPermWords / 4)];
  const int pass = (int)blockIdx.x / wgs;
  const int g = (int)blockIdx.x - pass * wgs;
  const int ncb = std::min(kPermCB, (n_perm - pass * kPermC + 15) / 16);  // >= 1
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int lo = lane & 15, q = lane >> 4;  // A: anchor lo, point q; B: point q, column lo
  double* gw = sa + wid * kTripTA * kTripMaxD;  // this wave's anchors, then its 16 x 64 g
  double sxx[kPermCB], asum[kPermCB], tsum = 0.0;
#pragma unroll
  for (int cb = 0; cb < kPermCB; ++cb) sxx[cb] = asum[cb] = 0.0;
  const int64_t it_end = std::min<int64_t>(items, (int64_t)(g + 1) * ipw);
  for (int64_t it = (int64_t)g * ipw; it < it_end; ++it) {
    int I, J;  // point tile I <= anchor tile J: workgroup-uniform
    self_tile_of(it, I, J);
    const int64_t p0 = (int64_t)I * kMmdT, a0 = (int64_t)J * kMmdT;
    const int na = (int)std::min<int64_t>(kMmdT, n - a0);  // >= 1
    const bool diag = I == J;
    bool valid[kTripR];
    const double* __restrict__ row[kTripR];
    bool all_valid = true;
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      const int64_t p = p0 + r * kWave + lane;
      valid[r] = p < n;
      row[r] = w + (valid[r] ? p : p0) * d;  // a lane past the end reads the tile's first point
      all_valid = all_valid && p0 + r * kWave + kWave <= n;
    }
    __syncthreads();  // the previous item's readers of lp and la
    // this pass's label words of the tile's rows (zeros past the sample and past the last word);
    // the step's second barrier orders them before their readers
    for (int e = threadIdx.x; e < 2 * kMmdT * kPermWords; e += kBlock) {
      const int anchors = e / (kMmdT * kPermWords), rem = e - anchors * (kMmdT * kPermWords);
      const int64_t rw = (anchors ? a0 : p0) + rem / kPermWords;
      const int64_t wi = (int64_t)pass * kPermWords + rem % kPermWords;
      const uint32_t v = (rw < n && wi < n_words) ? labels[rw * n_words + wi] : 0u;
      ((uint32_t*)(anchors ? la : lp))[rem] = v;
    }
    const int n_full = d / kTripDC;
    const bool tail = n_full * kTripDC < d;
    for (int s0 = 0; s0 < na; s0 += kMmdSA) {
      double pc[kTripR][kTripDC];
      if (n_full > 0) mmd_load<false>(row, 0, d, pc);
      else mmd_load<true>(row, 0, d, pc);
      __syncthreads();  // the previous step's readers
      for (int e = threadIdx.x; e < kMmdSA * d; e += kBlock) {
        const int a = e / d, cc = e - a * d;
        sa[a * kTripMaxD + cc] = s0 + a < na ? w[(a0 + s0) * d + e] : 0.0;
      }
      __syncthreads();
      double acc[kTripTA][kTripR];
#pragma unroll
      for (int a = 0; a < kTripTA; ++a)
#pragma unroll
        for (int r = 0; r < kTripR; ++r) acc[a][r] = 0.0;
      for (int ch = 0; ch < n_full; ++ch) {
        double pn[kTripR][kTripDC];
        const int c1 = (ch + 1) * kTripDC;
        if (ch + 1 < n_full) mmd_load<false>(row, c1, d, pn);
        else if (tail) mmd_load<true>(row, c1, d, pn);
        trip_chunk<false>(gw, ch * kTripDC, d, pc, acc);
#pragma unroll
        for (int r = 0; r < kTripR; ++r)
#pragma unroll
          for (int cc = 0; cc < kTripDC; ++cc) pc[r][cc] = pn[r][cc];
      }
      if (tail) trip_chunk<true>(gw, n_full * kTripDC, d, pc, acc);
      const int a_first = s0 + wid * kTripTA;  // this wave's anchors of the step, tile-relative
      const bool full = !diag && all_valid && s0 + kMmdSA <= na;  // workgroup-uniform
      const int diag_shift = diag ? 0 : kMmdT;
#pragma unroll
      for (int h = 0; h < kTripR; ++h) {
        __syncthreads();  // the anchors, and the first half's g, have been read
        // g of this half of the points over the wave's anchors: row a rotated by 4 a doubles.
        // Masked pairs (past either end, anchor <= point on a diagonal tile) are an exact 0.0.
#pragma unroll
        for (int a = 0; a < kTripTA; ++a) {
          double v = mmd_g<K>(acc[a][h], c);
          if (!full) {
            const bool ok = valid[h] && a_first + a < na &&
                            a_first + a + diag_shift > h * kWave + lane;
            v = ok ? v : 0.0;
          }
          gw[a * kPermHalf + ((lane + 4 * a) & (kPermHalf - 1))] = v;
        }
        __syncthreads();
        f64x4 R = {0.0, 0.0, 0.0, 0.0};  // the anchors' row sums over this half (group 0 forms them)
#pragma unroll
        for (int grp = 0; grp < kPermCB / kPermGB; ++grp) {
          if (grp * kPermGB >= ncb) continue;  // wave-uniform
          f64x4 C[kPermGB];
#pragma unroll
          for (int j = 0; j < kPermGB; ++j) C[j] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
          for (int ks = 0; ks < kPermHalf / 4; ++ks) {
            const double av = gw[lo * kPermHalf + ((4 * ks + q + 4 * lo) & (kPermHalf - 1))];
            const PermWords wv = perm_words(lp, h * kPermHalf + 4 * ks + q);
#pragma unroll
            for (int j = 0; j < kPermGB; ++j) {
              const int cb = grp * kPermGB + j;
              if (cb < ncb)  // wave-uniform
                C[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                    av, perm_label(wv[cb >> 1], (cb & 1) * 16 + lo), C[j], 0, 0, 0);
            }
            if (grp == 0) R = __builtin_amdgcn_mfma_f64_16x16x4f64(av, 1.0, R, 0, 0, 0);
          }
          // C[j][reg]: anchor q + 4 reg of the wave by column (grp * kPermGB + j) * 16 + lo
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const PermWords wv = perm_words(la, a_first + q + 4 * reg);
            if (grp == 0) tsum += R[reg];
#pragma unroll
            for (int j = 0; j < kPermGB; ++j) {
              const int cb = grp * kPermGB + j;
              if (cb < ncb) {
                const double s = perm_label(wv[cb >> 1], (cb & 1) * 16 + lo);
                sxx[cb] = __builtin_fma(C[j][reg], s, sxx[cb]);  // s is 0.0 or 1.0: exact
                asum[cb] += __builtin_fma(R[reg], s, C[j][reg]);
              }
            }
          }
        }
      }
    }
  }
  // a wave's four anchor groups in a fixed order, then the four waves in a fixed order: every
  // slot is written, also by a pass's unused column blocks (zeros)
  __syncthreads();  // the last readers of sa
  double* red = sa;
  auto fold = [](double v) {
    v += __shfl_xor(v, 16, kWave);
    v += __shfl_xor(v, 32, kWave);
    return v;
  };
#pragma unroll
  for (int cb = 0; cb < kPermCB; ++cb) {
    const double a = fold(sxx[cb]), b = fold(asum[cb]);
    if (q == 0) {
      red[wid * kPermSlots + cb * 16 + lo] = a;
      red[wid * kPermSlots + kPermC + cb * 16 + lo] = b;
    }
  }
  tsum = fold(tsum);
  if (q == 0) red[wid * kPermSlots + 2 * kPermC + lo] = tsum;
  __syncthreads();
  double* __restrict__ out = work + (int64_t)blockIdx.x * kPermSlots;
  for (int e = threadIdx.x; e < kPermSlots; e += kBlock)
    out[e] = (red[e] + red[kPermSlots + e]) + (red[2 * kPermSlots + e] + red[3 * kPermSlots + e]);
}

// One block per column p: its pass's partials added lane-strided in a fixed order, then the
// fixed butterfly and wave order of the block sums (k_self_reduce's way), then the identities.
__global__ __launch_bounds__(kBlock) void k_mmd_perm_reduce(const double* __restrict__ work,
                                                            int wgs, double* __restrict__ out) {
  __shared__ double part[kBlock / kWave];
  const int p = (int)blockIdx.x, pass = p / kPermC, cc = p - pass * kPermC;
  const double* __restrict__ wk = work + (int64_t)pass * wgs * kPermSlots;
  const int slot[3] = {cc, kPermC + cc, 2 * kPermC + (cc & 15)};
  double tot[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double v = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < wgs; i += kBlock) v += wk[(int64_t)i * kPermSlots + slot[k]];
    tot[k] = self_block_sum_f64(v, part);
  }
  if (threadIdx.x == 0) {
    const double sxx = tot[0], A = tot[1], T = tot[2];
    out[(int64_t)p * 3 + 0] = sxx;
    out[(int64_t)p * 3 + 1] = (T - A) + sxx;
    out[(int64_t)p * 3 + 2] = A - 2.0 * sxx;
  }
}

}  // namespace tw

using namespace tw;

extern "C" int32_t tw_mmd_perm_cols(void) { return kPermC; }

extern "C" int64_t tw_mmd_perm_work_bytes(int64_t n_rows, int32_t n_perm) {
  if (n_rows < 4 || n_rows >= (1ll << 31) || n_perm < 1) return 0;
  return perm_plan(n_rows).wgs * ceil_div(n_perm, kPermC) * kPermSlots * 8;
}

extern "C" int tw_mmd_perm_sums(const double* d_w, int64_t n_rows, int32_t d,
                                const uint32_t* d_labels, int32_t n_perm, int32_t kern, double c,
                                void* d_work, double* d_out, void* stream) {
  TW_ARG_CHECK(d_w && d_labels && d_work && d_out, "tw_mmd_perm_sums: null pointer");
  TW_ARG_CHECK(n_rows >= 4 && n_rows < (1ll << 31),
               "tw_mmd_perm_sums: n_rows %lld outside [4, 2^31) (two rows of each sample)",
               (long long)n_rows);
  TW_ARG_CHECK(n_perm >= 1, "tw_mmd_perm_sums: n_perm %d < 1 (a test has the observed split)",
               n_perm);
  TW_MMD_KERN_CHECKS("tw_mmd_perm_sums");
  hipStream_t st = (hipStream_t)stream;
  const PermPlan pl = perm_plan(n_rows);
  const int64_t passes = ceil_div(n_perm, kPermC);
  TW_ARG_CHECK(pl.wgs * passes < (1ll << 31), "tw_mmd_perm_sums: grid too large");
  const dim3 g((unsigned)(pl.wgs * passes)), b(kBlock);
  const int64_t n_words = ceil_div(n_perm, 32);
  if (kern == TW_MMD_GAUSSIAN)
    hipLaunchKernelGGL(k_mmd_perm<TW_MMD_GAUSSIAN>, g, b, 0, st, d_w, n_rows, (int)d, d_labels,
                       n_words, (int)n_perm, pl.items, pl.ipw, (int)pl.wgs, c, (double*)d_work);
  else
    hipLaunchKernelGGL(k_mmd_perm<TW_MMD_ENERGY>, g, b, 0, st, d_w, n_rows, (int)d, d_labels,
                       n_words, (int)n_perm, pl.items, pl.ipw, (int)pl.wgs, c, (double*)d_work);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mmd_perm_reduce, dim3((unsigned)n_perm), dim3(kBlock), 0, st,
                     (const double*)d_work, (int)pl.wgs, d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
