// hsic_perm.hip — the permutation test of the kernel independence statistics (tuplewise.hsic_perm
// permutation_sums / permutation_test; an extension, not in the reference): the
// two sums of tw_hsic_sums that a permutation of the pairing moves, for EVERY permutation in one
// launch.  Under a permutation pi of one side's rows the other side's pair function H_ij, both
// sides' row sums and six of §4.14's eight sums stay; with M the moved side's pair function and
// h, m the row sums of the unpermuted sample, column p has
//   S_p   = sum_{i<j} H_ij M_{idx[p][i] idx[p][j]}        Rab_p = sum_i h_i m_{idx[p][i]}
// The kernel does not know which side is X: a caller that moves X passes the inverse permutation,
// Y as the held side and the row sums swapped.
// Work items are the triangle of kMmdT-row tile pairs of the HELD side (a diagonal tile counts
// anchor > point only).  A step is k_hsic_sums' (hsictile.h: kHsicTA anchors a wave, two points a
// lane): the wave evaluates the held side's 16 values a lane once, keeps them in registers, and
// for each of the kHPermC columns of the workgroup's chunk runs the moved side on the GATHERED
// anchors moved[idx[p][a]] (staged in LDS) and the lane's two gathered points, folds
// s += H * g(M) (masked pairs selected to 0.0) and adds the lane's sum into that column's
// per-thread running slot in LDS (kBlock * kHPermC doubles: no reduction inside the loop).
// The staging is double-buffered: while a column's arithmetic runs from one buffer, the next
// column's anchors are in flight in registers and the index entries of the column after that are
// loaded, so neither the index load nor the row load it addresses is waited for; the first chunk
// of the lane's next points is loaded under this column's g.  One barrier a column.  The held
// anchors of a step borrow the second buffer before column 1 needs it.
// Every gathered index is clamped into [0, n) by an unsigned min, so the device reads inside the
// two arrays whatever d_idx holds; the sums are unspecified for rows that are not permutations.
// Lanes and anchors past the end read a valid row and are selected away.
// No atomics and nothing to zero: the four waves are folded in a fixed order, one double per
// workgroup and column goes to d_work, k_hsic_perm_reduce (one block a column) adds the column's
// partials in k_self_reduce's order and forms Rab_p by a fixed-order gather-dot.  The partition
// of the items over workgroups depends on n and wgs alone and every column of a chunk meets the
// same instructions in the same order: a column's two doubles depend only on the data, on that
// column's index row and on wgs.
#include "tw_common.h"
#include "selfreduce.h"
#include "tripdist.h"
#include "mmdtile.h"
#include "hsictile.h"
#include <algorithm>
#include <cmath>

namespace tw {

constexpr int kHPermC = 16;                    // columns that share one evaluation of the held side
constexpr int64_t kHPermMaxWG = 512;           // workgroups per chunk of columns when wgs = 0
constexpr int kHPermGT = kBlock / kHsicSA;     // threads that gather one anchor's coordinates
constexpr int kHPermGK = kTripMaxD / kHPermGT; // coordinates a thread gathers, at most
static_assert(kHPermGT * kHsicSA == kBlock && kHPermGK * kHPermGT == kTripMaxD,
              "one anchor per kHPermGT threads, kHPermGK coordinates each");
static_assert(kBlock / kWave <= kHsicSA * kTripMaxD, "the block sums' scratch aliases a buffer");

struct HPermPlan {
  int64_t items, ipw;  // tile pairs, and tile pairs per workgroup
  int64_t wgs;         // workgroups per chunk of columns
  int64_t chunks;      // chunks of kHPermC columns
};
// The partition depends on n and wgs alone: a column's partials are the same whatever n_cols is.
// false: the shape is refused.
inline bool hperm_plan(int64_t n, int32_t n_cols, int32_t wgs, HPermPlan& p) {
  if (n < 4 || n >= (1ll << 31) || n_cols < 1 || wgs < 0) return false;
  const int64_t t = ceil_div(n, kMmdT);
  p.items = t * (t + 1) / 2;
  p.ipw = std::max<int64_t>(1, ceil_div(p.items, wgs > 0 ? (int64_t)wgs : kHPermMaxWG));
  p.wgs = ceil_div(p.items, p.ipw);
  p.chunks = ceil_div(n_cols, kHPermC);
  return p.wgs * p.chunks < (1ll << 31);
}

// A gathered row: the index entry clamped into [0, n) (a negative entry is a large unsigned).
__device__ __forceinline__ int64_t hperm_clamp(int32_t i, uint32_t n_minus_1) {
  return (int64_t)std::min((uint32_t)i, n_minus_1);
}

template <int K, bool MASK>
__device__ __forceinline__ double hperm_fold(const double (&h)[kHsicTA][kTripR],
                                             const double (&am)[kHsicTA][kTripR], double cm,
                                             int a_first, int na, int diag_shift, int lane,
                                             const bool (&valid)[kTripR]) {
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < kHsicTA; ++a) {
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      double t = h[a][r] * mmd_g<K>(am[a][r], cm);
      if (MASK) t = hsic_ok<MASK>(a, r, a_first, na, diag_shift, lane, valid) ? t : 0.0;
      s += t;
    }
  }
  return s;
}

// Workgroup blockIdx.x = (chunk of kHPermC columns, group of ipw consecutive tile pairs).
template <int K>
__global__ __launch_bounds__(kBlock, 2) void k_hsic_perm(
    const double* __restrict__ held, int dh, const double* __restrict__ moved, int dm, int64_t n,
    const int32_t* __restrict__ idx, int n_cols, int64_t items, int64_t ipw, int wgs, double c_held,
    double c_moved, double* __restrict__ work) {
  __shared__ double buf[2][kHsicSA * kTripMaxD];  // a column's gathered anchors, double-buffered
  __shared__ double slot[kHPermC * kBlock];       // the columns' running sums, one per thread
  const int chunk = (int)blockIdx.x / wgs;
  const int g = (int)blockIdx.x - chunk * wgs;
  const int ncols = std::min(kHPermC, n_cols - chunk * kHPermC);  // >= 1
  const int32_t* __restrict__ idx0 = idx + (int64_t)chunk * kHPermC * n;  // the chunk's first row
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int ga = threadIdx.x / kHPermGT, gc = threadIdx.x % kHPermGT;  // gather: anchor, coordinate
  const uint32_t nm1 = (uint32_t)(n - 1);
  const int woff = wid * kHsicTA * kTripMaxD;  // this wave's anchors of a buffer
#pragma unroll
  for (int c = 0; c < kHPermC; ++c) slot[c * kBlock + threadIdx.x] = 0.0;  // the thread's own
  const int64_t it_end = std::min<int64_t>(items, (int64_t)(g + 1) * ipw);
  for (int64_t it = (int64_t)g * ipw; it < it_end; ++it) {
    int I, J;  // point tile I <= anchor tile J: workgroup-uniform
    self_tile_of(it, I, J);
    const int64_t p0 = (int64_t)I * kMmdT, a0 = (int64_t)J * kMmdT;
    const int na = (int)std::min<int64_t>(kMmdT, n - a0);  // >= 1
    const bool diag = I == J;
    bool valid[kTripR];
    int64_t ppos[kTripR];  // the lane's points: positions in an index row, rows of the held side
    const double* __restrict__ rowh[kTripR];
    bool all_valid = true;
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      const int64_t p = p0 + r * kWave + lane;
      valid[r] = p < n;
      ppos[r] = valid[r] ? p : p0;  // a lane past the end reads the tile's first row
      rowh[r] = held + ppos[r] * dh;
      all_valid = all_valid && p0 + r * kWave + kWave <= n;
    }
    for (int s0 = 0; s0 < na; s0 += kHsicSA) {
      const int a_first = s0 + wid * kHsicTA;  // this wave's anchors of the step, tile-relative
      const bool plain = !diag && all_valid && s0 + kHsicSA <= na;  // workgroup-uniform
      const int shift = diag ? 0 : kMmdT;
      // the position of this thread's gathered anchor (past the end: the last row, masked)
      const int64_t apos = std::min<int64_t>(a0 + s0 + ga, n - 1);
      double pc[kTripR][kTripDC];
      if (dh >= kTripDC) mmd_load<false>(rowh, 0, dh, pc);
      else mmd_load<true>(rowh, 0, dh, pc);
      // (the previous step's last column ended with a barrier: both buffers are free)
      hsic_stage(buf[1], held + (a0 + s0) * dh, dh, na - s0);
      const double* __restrict__ rowm[kTripR];
      {  // column 0: its anchors straight into buf[0], its points' rows
        const double* __restrict__ src = moved + hperm_clamp(idx0[apos], nm1) * dm;
#pragma unroll
        for (int k = 0; k < kHPermGK; ++k) {
          const int cc = gc + k * kHPermGT;
          if (cc < dm) buf[0][ga * kTripMaxD + cc] = src[cc];
        }
#pragma unroll
        for (int r = 0; r < kTripR; ++r) rowm[r] = moved + hperm_clamp(idx0[ppos[r]], nm1) * dm;
      }
      int32_t ian = 0, ipn[kTripR] = {0, 0};  // column c + 1's index entries, loaded a column early
      if (ncols > 1) {
        ian = idx0[n + apos];
#pragma unroll
        for (int r = 0; r < kTripR; ++r) ipn[r] = idx0[n + ppos[r]];
      }
      __syncthreads();
      double h[kHsicTA][kTripR];
      {
        double ah[kHsicTA][kTripR];
#pragma unroll
        for (int a = 0; a < kHsicTA; ++a)
#pragma unroll
          for (int r = 0; r < kTripR; ++r) ah[a][r] = 0.0;
        hsic_side(rowh, dh, buf[1] + woff, pc, ah);
        // column 0's first chunk in flight under the held side's g
        if (dm >= kTripDC) mmd_load<false>(rowm, 0, dm, pc);
        else mmd_load<true>(rowm, 0, dm, pc);
#pragma unroll
        for (int a = 0; a < kHsicTA; ++a) {
#pragma unroll
          for (int r = 0; r < kTripR; ++r) {
            const double v = mmd_g<K>(ah[a][r], c_held);
            h[a][r] = (plain || hsic_ok<true>(a, r, a_first, na, shift, lane, valid)) ? v : 0.0;
          }
        }
      }
      __syncthreads();  // the held anchors have been read: buf[1] is column 1's
      for (int c = 0; c < ncols; ++c) {
        const bool more = c + 1 < ncols;  // workgroup-uniform
        double st[kHPermGK];
        const double* __restrict__ rown[kTripR];
        if (more) {  // column c + 1's rows, addressed by the entries loaded a column ago
          const double* __restrict__ src = moved + hperm_clamp(ian, nm1) * dm;
#pragma unroll
          for (int k = 0; k < kHPermGK; ++k) {
            const int cc = gc + k * kHPermGT;
            st[k] = cc < dm ? src[cc] : 0.0;
          }
#pragma unroll
          for (int r = 0; r < kTripR; ++r) rown[r] = moved + hperm_clamp(ipn[r], nm1) * dm;
          if (c + 2 < ncols) {  // and column c + 2's entries
            const int32_t* __restrict__ row2 = idx0 + (int64_t)(c + 2) * n;
            ian = row2[apos];
#pragma unroll
            for (int r = 0; r < kTripR; ++r) ipn[r] = row2[ppos[r]];
          }
        }
        double am[kHsicTA][kTripR];
#pragma unroll
        for (int a = 0; a < kHsicTA; ++a)
#pragma unroll
          for (int r = 0; r < kTripR; ++r) am[a][r] = 0.0;
        hsic_side(rowm, dm, buf[c & 1] + woff, pc, am);
        if (more) {  // the next points' first chunk in flight under this column's g (pc is free)
#pragma unroll
          for (int r = 0; r < kTripR; ++r) rowm[r] = rown[r];
          if (dm >= kTripDC) mmd_load<false>(rowm, 0, dm, pc);
          else mmd_load<true>(rowm, 0, dm, pc);
        }
        const double s =
            plain ? hperm_fold<K, false>(h, am, c_moved, a_first, na, 0, lane, valid)
                  : hperm_fold<K, true>(h, am, c_moved, a_first, na, shift, lane, valid);
        slot[c * kBlock + threadIdx.x] += s;
        if (more) {  // buf[(c + 1) & 1] was read last in column c - 1, before its barrier
          double* __restrict__ dst = buf[(c + 1) & 1] + ga * kTripMaxD;
#pragma unroll
          for (int k = 0; k < kHPermGK; ++k) {
            const int cc = gc + k * kHPermGT;
            if (cc < dm) dst[cc] = st[k];
          }
        }
        __syncthreads();
      }
    }
  }
  // a column's 256 running sums: the wave butterfly, then the four waves in a fixed order.  Every
  // slot of d_work is written, also a short chunk's unused columns (zeros).
  double* __restrict__ out = work + (int64_t)blockIdx.x * kHPermC;
  for (int c = 0; c < kHPermC; ++c) {
    const double s = self_block_sum_f64(slot[c * kBlock + threadIdx.x], buf[0]);
    if (threadIdx.x == 0) out[c] = s;
  }
}

// One block per column p: its chunk's partials added lane-strided in a fixed order, then the
// fixed butterfly and wave order of the block sums (k_self_reduce's way); Rab_p the same way over
// the rows.
__global__ __launch_bounds__(kBlock) void k_hsic_perm_reduce(
    const double* __restrict__ work, int wgs, const int32_t* __restrict__ idx, int64_t n,
    const double* __restrict__ rows_held, const double* __restrict__ rows_moved,
    double* __restrict__ out) {
  __shared__ double part[kBlock / kWave];
  const int p = (int)blockIdx.x, chunk = p / kHPermC, cc = p - chunk * kHPermC;
  const double* __restrict__ wk = work + (int64_t)chunk * wgs * kHPermC;
  double v = 0.0;
#pragma unroll 4
  for (int i = threadIdx.x; i < wgs; i += kBlock) v += wk[(int64_t)i * kHPermC + cc];
  const double s = self_block_sum_f64(v, part);
  const int32_t* __restrict__ row = idx + (int64_t)p * n;
  const uint32_t nm1 = (uint32_t)(n - 1);
  v = 0.0;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < n; i += kBlock)
    v += rows_held[i] * rows_moved[hperm_clamp(row[i], nm1)];
  const double rab = self_block_sum_f64(v, part);
  if (threadIdx.x == 0) {
    out[(int64_t)p * 2 + 0] = s;
    out[(int64_t)p * 2 + 1] = rab;
  }
}

}  // namespace tw

using namespace tw;

static_assert(TW_HSIC_GAUSSIAN == TW_MMD_GAUSSIAN && TW_HSIC_DISTANCE == TW_MMD_ENERGY,
              "mmd_g is instantiated by the TW_MMD ids");

extern "C" int32_t tw_hsic_perm_cols(void) { return kHPermC; }

extern "C" int64_t tw_hsic_perm_work_bytes(int64_t n, int32_t n_cols, int32_t wgs) {
  HPermPlan p;
  return hperm_plan(n, n_cols, wgs, p) ? p.wgs * p.chunks * kHPermC * 8 : 0;
}

extern "C" int tw_hsic_perm_sums(const double* d_held, int32_t d_h, const double* d_moved,
                                 int32_t d_m, int64_t n, const int32_t* d_idx, int32_t n_cols,
                                 const double* d_rows_held, const double* d_rows_moved,
                                 int32_t kern, double c_held, double c_moved, int32_t wgs,
                                 void* d_work, double* d_out, void* stream) {
  TW_ARG_CHECK(d_held && d_moved && d_idx && d_rows_held && d_rows_moved && d_work && d_out,
               "tw_hsic_perm_sums: null pointer");
  TW_ARG_CHECK(d_h >= 1 && d_h <= kTripMaxD, "tw_hsic_perm_sums: d_h %d outside [1, %d]", d_h,
               kTripMaxD);
  TW_ARG_CHECK(d_m >= 1 && d_m <= kTripMaxD, "tw_hsic_perm_sums: d_m %d outside [1, %d]", d_m,
               kTripMaxD);
  TW_ARG_CHECK(n >= 4 && n < (1ll << 31),
               "tw_hsic_perm_sums: n %lld outside [4, 2^31) (a 4-tuple needs four items)",
               (long long)n);
  TW_ARG_CHECK(n_cols >= 1, "tw_hsic_perm_sums: n_cols %d < 1", n_cols);
  TW_ARG_CHECK(kern == TW_HSIC_GAUSSIAN || kern == TW_HSIC_DISTANCE,
               "tw_hsic_perm_sums: unknown kernel %d", kern);
  TW_ARG_CHECK(kern != TW_HSIC_GAUSSIAN || (std::isfinite(c_held) && c_held <= 0.0 &&
                                            std::isfinite(c_moved) && c_moved <= 0.0),
               "tw_hsic_perm_sums: c_held = %g, c_moved = %g for the Gaussian kernel (finite and "
               "<= 0: -1 / (2 sigma^2))", c_held, c_moved);
  TW_ARG_CHECK(wgs >= 0, "tw_hsic_perm_sums: wgs %d < 0", wgs);
  HPermPlan pl;
  TW_ARG_CHECK(hperm_plan(n, n_cols, wgs, pl), "tw_hsic_perm_sums: grid too large (n %lld, "
               "n_cols %d, wgs %d)", (long long)n, n_cols, wgs);
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)(pl.wgs * pl.chunks)), b(kBlock);
  if (kern == TW_HSIC_GAUSSIAN)
    hipLaunchKernelGGL(k_hsic_perm<TW_MMD_GAUSSIAN>, g, b, 0, st, d_held, (int)d_h, d_moved,
                       (int)d_m, n, d_idx, (int)n_cols, pl.items, pl.ipw, (int)pl.wgs, c_held,
                       c_moved, (double*)d_work);
  else
    hipLaunchKernelGGL(k_hsic_perm<TW_MMD_ENERGY>, g, b, 0, st, d_held, (int)d_h, d_moved,
                       (int)d_m, n, d_idx, (int)n_cols, pl.items, pl.ipw, (int)pl.wgs, c_held,
                       c_moved, (double*)d_work);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hsic_perm_reduce, dim3((unsigned)n_cols), b, 0, st, (const double*)d_work,
                     (int)pl.wgs, d_idx, n, d_rows_held, d_rows_moved, d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
