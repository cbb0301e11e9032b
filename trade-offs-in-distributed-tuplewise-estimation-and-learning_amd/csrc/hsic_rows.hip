// hsic_rows.hip — three row sums per point of the kernel independence statistics, for a grid of
// bandwidth pairs (tuplewise.hsic_var; an extension, not in the reference).  For
// every row i of a block of tw_hsic_sums' partition and every coefficient pair (c_x[s], c_y[s])
//   p_i = sum_{j != i} K_ij L_ij    a_i = sum_j K_ij wk_j    b_i = sum_j L_ij wl_j
// with wk = wl = 1 (a_i = k_i, b_i = l_i: the row sums of K and L) or, given a previous launch's
// rows as weights, wk_j = l_j and wl_j = k_j (a = K l, b = L k): what the Hajek projection of
// HSIC_u is made of.  D is tripdist.h's, g is mmdtile.h's mmd_g and the step is hsictile.h's
// (kHsicTA anchors a wave, both sides staged), so a K_ij or L_ij has the bits k_hsic_sums gives it.
// Work items are the tile pairs of a block's triangle of tiles, one per workgroup.  Every
// unordered pair is visited ONCE: both sides' squared distances of a step are held in registers
// while a runtime loop over s applies g per side, so D costs 3 (dx + dy) lane-ops a pair whatever
// the grid's length.  A pair feeds its point's three sums (register adds, summed over steps in the
// lane's own LDS slots and over the four waves at the item's end) and its anchor's: 8 values a
// lane and sum that hsictile.h's reduce-scatter butterfly adds over the wave's 128 points; a
// wave's anchors of a step belong to no other wave or step, so the butterfly's result is the
// anchor's whole partial of the item and goes straight to d_work.
// One partial per row, tile COLUMN, sum and sigma goes to d_work.  Row i of tile T of a block of t
// tiles has T + 1 anchor-side partials (items (I, T), I <= T, column I) and t - T point-side ones
// (items (T, J), J >= T, column J + 1): t + 1 columns, a diagonal tile filling two.  No atomics
// and nothing to zero: k_hsic_rows3_add adds a row's columns in a fixed order.  Everything is
// indexed relative to the block and by the block's own size, so a block's rows are the same bits
// alone, beside other blocks and wherever the partition starts; the loop over s runs the same
// instructions on the same D for every s, so a pair's rows do not depend on the grid; the weights
// enter only the second and third sum, so p is the same bits with and without them.
// (k_hsic_rows is hsic.hip's column adder; the kernels here are k_hsic_rows3 and
// k_hsic_rows3_add.)
#include "tw_common.h"
#include "selfreduce.h"
#include "tripdist.h"
#include "mmdtile.h"   // kMmdT, mmd_g, mmd_load
#include "hsictile.h"  // kHsicTA, kHsicSA, hsic_stage, hsic_side, hsic_ok, hsic_anchor_sums
#include <algorithm>
#include <cmath>

namespace tw {

// Bandwidth pairs per launch: 12 KiB of point sums each beside the 32 KiB of staged anchors, so 4
// fill the 80 KiB that two workgroups a CU leave each (DESIGN.md §4.20 has the figures).
constexpr int kHsicRows3MaxS = 4;
constexpr int kHsicRows3Q = 3;                           // sums per row
constexpr int64_t kHsicRows3WorkBudget = 1ll << 30;      // bytes of d_work a launch may ask for
constexpr int kHsicRows3AddRows = kWave;                 // rows per workgroup of k_hsic_rows3_add
static_assert(2 * kHsicSA * kTripMaxD * 8 +
                      kHsicRows3MaxS * kHsicRows3Q * (kBlock / kWave) * kMmdT * 8 <= 80 * 1024,
              "two workgroups a CU");

// The launch plan: everything tw_hsic_rows_work_bytes and the launch agree on.
struct HsicRows3Plan {
  int64_t tm;      // tiles of the largest block
  int64_t per;     // workgroups per block: the tile pairs of the largest block
  int64_t words;   // doubles of d_work per block and sigma: (tm + 1) columns of max_n rows of 3
  int64_t chunks;  // workgroups of k_hsic_rows3_add per block and sigma
};

inline bool hsic_rows3_plan(int64_t n_blocks, int64_t max_n, int n_sigma, HsicRows3Plan& p) {
  if (n_blocks < 1 || max_n < 4 || max_n >= (1ll << 31) || n_sigma < 1 ||
      n_sigma > kHsicRows3MaxS)
    return false;
  p.tm = ceil_div(max_n, kMmdT);
  p.per = p.tm * (p.tm + 1) / 2;
  p.chunks = ceil_div(max_n, kHsicRows3AddRows);
  p.words = (p.tm + 1) * max_n * kHsicRows3Q;  // < 2^57
  if ((double)p.per * (double)n_blocks >= 2147483648.0 ||
      (double)p.chunks * (double)n_blocks * n_sigma >= 2147483648.0)
    return false;
  return (double)p.words * (double)n_blocks * n_sigma * 8.0 <= (double)kHsicRows3WorkBudget;
}

// g per side of the wave's kHsicTA x kTripR held distances: pr[q][r] the lane's points' terms over
// the anchors in ascending order, v[q][a] the anchors' terms of this lane's two points.  W: the
// second sum's terms are K_ij times the OTHER end's weight wk, the third's L_ij times wl (wa the
// anchors' weights, wp the points'); a masked pair's product is selected away, so the weight of a
// masked pair never enters.  MASK as in hsic_ok.
template <int K, bool MASK, bool W>
__device__ __forceinline__ void hsic_rows3_fold(
    const double (&ak)[kHsicTA][kTripR], const double (&al)[kHsicTA][kTripR], double cx, double cy,
    int a_first, int na, int diag_shift, int lane, const bool (&valid)[kTripR],
    const double (&wa)[kHsicTA][2], const double (&wp)[kTripR][2],
    double (&pr)[kHsicRows3Q][kTripR], double (&v)[kHsicRows3Q][kHsicTA]) {
#pragma unroll
  for (int q = 0; q < kHsicRows3Q; ++q)
#pragma unroll
    for (int r = 0; r < kTripR; ++r) pr[q][r] = 0.0;
#pragma unroll
  for (int a = 0; a < kHsicTA; ++a) {
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      double k = mmd_g<K>(ak[a][r], cx);
      double l = mmd_g<K>(al[a][r], cy);
      const bool ok = hsic_ok<MASK>(a, r, a_first, na, diag_shift, lane, valid);
      if (MASK) {
        k = ok ? k : 0.0;
        l = ok ? l : 0.0;
      }
      const double kl = k * l;
      double kp = k, ka = k, lp = l, la = l;  // the point's and the anchor's terms
      if (W) {
        kp = k * wa[a][0];
        ka = k * wp[r][0];
        lp = l * wa[a][1];
        la = l * wp[r][1];
        if (MASK) {
          kp = ok ? kp : 0.0;
          ka = ok ? ka : 0.0;
          lp = ok ? lp : 0.0;
          la = ok ? la : 0.0;
        }
      }
      pr[0][r] += kl;
      pr[1][r] += kp;
      pr[2][r] += lp;
      v[0][a] = r == 0 ? kl : v[0][a] + kl;
      v[1][a] = r == 0 ? ka : v[1][a] + ka;
      v[2][a] = r == 0 ? la : v[2][a] + la;
    }
  }
}

// The distance kernel's g takes no coefficient, so K and L themselves are held (masked pairs as
// 0.0) and the three sums are formed one after the other, a butterfly each: the same terms in the
// same order as hsic_rows3_fold.  One form for every step, the weighted products of masked pairs
// always selected away: with a plain and a masked form the compiler evaluates both and selects,
// and the kernel spills.
template <bool W>
__device__ __forceinline__ void hsic_rows3_fold_held(
    const double (&ak)[kHsicTA][kTripR], const double (&al)[kHsicTA][kTripR], int a_first, int na,
    int diag_shift, int lane, const bool (&valid)[kTripR], const double (&wa)[kHsicTA][2],
    const double (&wp)[kTripR][2], double (&pr)[kHsicRows3Q][kTripR],
    double (&av)[kHsicRows3Q]) {
#pragma unroll
  for (int q = 0; q < kHsicRows3Q; ++q) {
    double v[kHsicTA];
#pragma unroll
    for (int r = 0; r < kTripR; ++r) pr[q][r] = 0.0;
#pragma unroll
    for (int a = 0; a < kHsicTA; ++a) {
#pragma unroll
      for (int r = 0; r < kTripR; ++r) {
        const double g = q == 2 ? al[a][r] : ak[a][r];
        double tp = q == 0 ? g * al[a][r] : g, ta = tp;  // the point's and the anchor's term
        if (W && q > 0) {
          const bool ok = hsic_ok<true>(a, r, a_first, na, diag_shift, lane, valid);
          tp = ok ? g * wa[a][q - 1] : 0.0;
          ta = ok ? g * wp[r][q - 1] : 0.0;
        }
        pr[q][r] += tp;
        v[a] = r == 0 ? ta : v[a] + ta;
      }
    }
    av[q] = hsic_anchor_sums(v, lane);
  }
}

// Workgroup blockIdx.x = (block of the partition, tile pair of that block's OWN triangle).
// w: a previous launch's rows (n_sigma, rows, 3), rows = blk_off[n_blocks]; [.., 2] weighs K's sum
// and [.., 1] weighs L's; [.., 0] is not read.
template <int K, bool W>
__global__ __launch_bounds__(kBlock, 2) void k_hsic_rows3(
    const double* __restrict__ x, int dx, const double* __restrict__ y, int dy,
    const int64_t* __restrict__ blk_off, int n_blocks, int per, const double* __restrict__ cs,
    int n_sigma, const double* __restrict__ w, int64_t max_n,
    int64_t tm, double* __restrict__ work) {
  __shared__ double sax[kHsicSA * kTripMaxD];  // a step's anchors, X side
  __shared__ double say[kHsicSA * kTripMaxD];  // and Y side
  // the points' sums per sigma, sum and wave (80 KiB of LDS in all: two workgroups a CU)
  __shared__ double psum[kHsicRows3MaxS][kHsicRows3Q][kBlock / kWave][kMmdT];
  const int b = (int)blockIdx.x / per;
  const int it = (int)blockIdx.x - b * per;
  const int64_t r0 = blk_off[b], n = blk_off[b + 1] - r0;
  const int64_t rows = blk_off[n_blocks];
  const int64_t tiles = (n + kMmdT - 1) / kMmdT;
  // (a workgroup past a short block's tile pairs has nothing to do: every slot k_hsic_rows3_add
  // reads is written by an item of the block's own triangle)
  if (it >= tiles * (tiles + 1) / 2) return;  // workgroup-uniform, before any barrier
  // (the wave's index as a scalar, so that its anchors' weights are scalar loads)
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const double* __restrict__ swx = sax + wid * kHsicTA * kTripMaxD;
  const double* __restrict__ swy = say + wid * kHsicTA * kTripMaxD;
  const double* __restrict__ xb = x + r0 * dx;
  const double* __restrict__ yb = y + r0 * dy;
  const int64_t words = (tm + 1) * max_n * kHsicRows3Q;
  double* __restrict__ wb = work + (int64_t)b * n_sigma * words;
  int I, J;
  self_tile_of(it, I, J);  // points' tile I <= anchors' tile J
  const int64_t p0 = (int64_t)I * kMmdT, a0 = (int64_t)J * kMmdT;
  const int na = (int)std::min<int64_t>(kMmdT, n - a0);  // >= 1: J is a tile of the block
  const bool diag = I == J;
  const int64_t pcol = (int64_t)(J + 1) * max_n, acol = (int64_t)I * max_n;
  bool valid[kTripR];
  const double* __restrict__ rowx[kTripR];
  const double* __restrict__ rowy[kTripR];
  bool all_valid = true;
#pragma unroll
  for (int r = 0; r < kTripR; ++r) {
    const int64_t p = p0 + r * kWave + lane;
    valid[r] = p < n;
    rowx[r] = xb + (valid[r] ? p : p0) * dx;  // a lane past the end reads the tile's first row
    rowy[r] = yb + (valid[r] ? p : p0) * dy;
    all_valid = all_valid && p0 + r * kWave + kWave <= n;
  }
  for (int s0 = 0; s0 < na; s0 += kHsicSA) {
    double pc[kTripR][kTripDC];
    double ak[kHsicTA][kTripR], al[kHsicTA][kTripR];
    const int a_first = s0 + wid * kHsicTA;  // this wave's anchors of the step, tile-relative
    const bool plain = !diag && all_valid && s0 + kHsicSA <= na;  // workgroup-uniform
    const int shift = diag ? 0 : kMmdT;
    // k_hsic_sums' step: the lane's first chunk in flight while both sides' anchors are staged
    if (dx >= kTripDC) mmd_load<false>(rowx, 0, dx, pc);
    else mmd_load<true>(rowx, 0, dx, pc);
    __syncthreads();  // the previous step's readers of sax, say
    hsic_stage(sax, xb + (a0 + s0) * dx, dx, na - s0);
    hsic_stage(say, yb + (a0 + s0) * dy, dy, na - s0);
    __syncthreads();
#pragma unroll
    for (int a = 0; a < kHsicTA; ++a)
#pragma unroll
      for (int r = 0; r < kTripR; ++r) ak[a][r] = al[a][r] = 0.0;
    hsic_side(rowx, dx, swx, pc, ak);
    if (dy >= kTripDC) mmd_load<false>(rowy, 0, dy, pc);
    else mmd_load<true>(rowy, 0, dy, pc);
    hsic_side(rowy, dy, swy, pc, al);
    if constexpr (K != TW_MMD_GAUSSIAN) {  // K and L in place (hsic_rows3_fold_held)
#pragma unroll
      for (int a = 0; a < kHsicTA; ++a) {
#pragma unroll
        for (int r = 0; r < kTripR; ++r) {
          const bool ok = plain || hsic_ok<true>(a, r, a_first, na, shift, lane, valid);
          const double k = mmd_g<K>(ak[a][r], 0.0), l = mmd_g<K>(al[a][r], 0.0);
          ak[a][r] = ok ? k : 0.0;
          al[a][r] = ok ? l : 0.0;
        }
      }
    }
    // the held distances under every pair of the launch
#pragma unroll 1
    for (int s = 0; s < n_sigma; ++s) {
      const double cx = K == TW_MMD_GAUSSIAN ? cs[2 * s] : 0.0;  // (wave-uniform loads)
      const double cy = K == TW_MMD_GAUSSIAN ? cs[2 * s + 1] : 0.0;
      double wa[kHsicTA][2], wp[kTripR][2];
      if (W) {  // the weights of rows inside the block only: 0.0 for the masked ones
        const double* __restrict__ ws = w + ((int64_t)s * rows + r0) * kHsicRows3Q;
#pragma unroll
        for (int a = 0; a < kHsicTA; ++a) {
          const bool in = a_first + a < na;
          const int64_t j = a0 + (in ? a_first + a : 0);
          const double t0 = ws[j * kHsicRows3Q + 2], t1 = ws[j * kHsicRows3Q + 1];
          wa[a][0] = in ? t0 : 0.0;
          wa[a][1] = in ? t1 : 0.0;
        }
#pragma unroll
        for (int r = 0; r < kTripR; ++r) {
          const int64_t i = valid[r] ? p0 + r * kWave + lane : p0;
          const double t0 = ws[i * kHsicRows3Q + 2], t1 = ws[i * kHsicRows3Q + 1];
          wp[r][0] = valid[r] ? t0 : 0.0;
          wp[r][1] = valid[r] ? t1 : 0.0;
        }
      }
      double pr[kHsicRows3Q][kTripR], av[kHsicRows3Q];
      if constexpr (K == TW_MMD_GAUSSIAN) {
        double v[kHsicRows3Q][kHsicTA];
        if (plain)
          hsic_rows3_fold<K, false, W>(ak, al, cx, cy, a_first, na, 0, lane, valid, wa, wp, pr, v);
        else
          hsic_rows3_fold<K, true, W>(ak, al, cx, cy, a_first, na, shift, lane, valid, wa, wp, pr,
                                      v);
#pragma unroll
        for (int q = 0; q < kHsicRows3Q; ++q) av[q] = hsic_anchor_sums(v[q], lane);
      } else {
        hsic_rows3_fold_held<W>(ak, al, a_first, na, shift, lane, valid, wa, wp, pr, av);
      }
      // one lane per anchor; no other wave or step holds it: the item's whole partial
      const int a = a_first + hsic_anchor_of(lane);
      if (hsic_anchor_lane(lane) && a < na) {
        double* __restrict__ o = wb + (int64_t)s * words + (acol + a0 + a) * kHsicRows3Q;
#pragma unroll
        for (int q = 0; q < kHsicRows3Q; ++q) o[q] = av[q];
      }
      // the lane's own slots: no other lane touches them before the barrier below
#pragma unroll
      for (int q = 0; q < kHsicRows3Q; ++q)
#pragma unroll
        for (int r = 0; r < kTripR; ++r) {
          double* __restrict__ ps = &psum[s][q][wid][r * kWave + lane];
          *ps = s0 == 0 ? pr[q][r] : *ps + pr[q][r];
        }
    }
  }
  // the tile's points: the four waves' sums in a fixed order, out to the item's column
  __syncthreads();
  for (int t = threadIdx.x; t < n_sigma * kHsicRows3Q * kMmdT; t += kBlock) {
    const int sq = t / kMmdT, p = t - sq * kMmdT;
    const int s = sq / kHsicRows3Q, q = sq - s * kHsicRows3Q;
    const double (&ps)[kBlock / kWave][kMmdT] = psum[s][q];
    const double sum = (ps[0][p] + ps[1][p]) + (ps[2][p] + ps[3][p]);
    if (p0 + p < n) wb[(int64_t)s * words + (pcol + p0 + p) * kHsicRows3Q + q] = sum;
  }
}

// Row i of (block, sigma), kHsicRows3AddRows rows a workgroup.  Wave p adds the row's columns p,
// p + 4, ... in ascending order (one row a lane, so that a row's loads are four waves deep) and
// the four waves' sums are paired: a fixed order.
__global__ __launch_bounds__(kBlock) void k_hsic_rows3_add(
    const int64_t* __restrict__ blk_off, int n_blocks, int n_sigma, int chunks, int64_t max_n,
    int64_t tm, const double* __restrict__ work, double* __restrict__ out) {
  __shared__ double col[kBlock / kWave][kHsicRows3AddRows][kHsicRows3Q];
  const int ch = (int)blockIdx.x % chunks;
  const int bs = (int)blockIdx.x / chunks;
  const int b = bs / n_sigma, s = bs - b * n_sigma;
  const int64_t r0 = blk_off[b], n = blk_off[b + 1] - r0;
  const int64_t rows = blk_off[n_blocks];
  const int64_t cols = (n + kMmdT - 1) / kMmdT + 1;
  const int64_t words = (tm + 1) * max_n * kHsicRows3Q;
  const double* __restrict__ wk = work + ((int64_t)b * n_sigma + s) * words;
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int64_t i = (int64_t)ch * kHsicRows3AddRows + lane;
  const bool live = i < n;
  double t[kHsicRows3Q] = {0.0, 0.0, 0.0};
  if (live) {
#pragma unroll 4
    for (int64_t c = wid; c < cols; c += kBlock / kWave) {
#pragma unroll
      for (int q = 0; q < kHsicRows3Q; ++q) t[q] += wk[(c * max_n + i) * kHsicRows3Q + q];
    }
  }
#pragma unroll
  for (int q = 0; q < kHsicRows3Q; ++q) col[wid][lane][q] = t[q];
  __syncthreads();
  if (wid != 0 || !live) return;
  double* __restrict__ o = out + ((int64_t)s * rows + r0 + i) * kHsicRows3Q;
#pragma unroll
  for (int q = 0; q < kHsicRows3Q; ++q)
    o[q] = (col[0][lane][q] + col[1][lane][q]) + (col[2][lane][q] + col[3][lane][q]);
}

}  // namespace tw

using namespace tw;

static_assert(TW_HSIC_GAUSSIAN == TW_MMD_GAUSSIAN && TW_HSIC_DISTANCE == TW_MMD_ENERGY,
              "mmd_g is instantiated by the TW_MMD ids");

extern "C" int32_t tw_hsic_rows_max_sigma(void) { return kHsicRows3MaxS; }

extern "C" int64_t tw_hsic_rows_work_bytes(int32_t n_blocks, int64_t max_n, int32_t n_sigma) {
  HsicRows3Plan p;
  if (!hsic_rows3_plan(n_blocks, max_n, n_sigma, p)) return 0;
  return p.words * n_blocks * n_sigma * 8;
}

template <int K, bool W>
static void hsic_rows3_launch(const HsicRows3Plan& p, const double* d_x, int dx, const double* d_y,
                              int dy, const int64_t* d_blk_off, int n_blocks, int64_t max_n,
                              const double* d_c, int n_sigma,
                              const double* d_w, double* work, hipStream_t st) {
  hipLaunchKernelGGL((k_hsic_rows3<K, W>), dim3((unsigned)(p.per * n_blocks)), dim3(kBlock), 0, st,
                     d_x, dx, d_y, dy, d_blk_off, n_blocks, (int)p.per, d_c, n_sigma, d_w,
                     max_n, p.tm, work);
}

extern "C" int tw_hsic_rows(const double* d_x, int32_t dx, const double* d_y, int32_t dy,
                            const int64_t* d_blk_off, int32_t n_blocks, int64_t max_n,
                            int32_t kern, const double* d_c, int32_t n_sigma,
                            const double* d_w, void* d_work, double* d_rows, void* stream) {
  TW_ARG_CHECK(d_x && d_y && d_blk_off && d_work && d_rows &&
                   (d_c || kern == TW_HSIC_DISTANCE),
               "tw_hsic_rows: null pointer");
  TW_ARG_CHECK(n_blocks >= 0 && max_n >= 0, "tw_hsic_rows: negative size (n_blocks %d, max_n %lld)",
               n_blocks, (long long)max_n);
  TW_ARG_CHECK(dx >= 1 && dx <= kTripMaxD, "tw_hsic_rows: dx %d outside [1, %d]", dx, kTripMaxD);
  TW_ARG_CHECK(dy >= 1 && dy <= kTripMaxD, "tw_hsic_rows: dy %d outside [1, %d]", dy, kTripMaxD);
  TW_ARG_CHECK(kern == TW_HSIC_GAUSSIAN || kern == TW_HSIC_DISTANCE,
               "tw_hsic_rows: unknown kernel %d", kern);
  TW_ARG_CHECK(n_sigma >= 1 && n_sigma <= kHsicRows3MaxS,
               "tw_hsic_rows: n_sigma %d outside [1, %d]", n_sigma, kHsicRows3MaxS);
  TW_ARG_CHECK(kern != TW_HSIC_DISTANCE || n_sigma == 1,
               "tw_hsic_rows: n_sigma %d for the distance kernel (it takes no sigma: 1)", n_sigma);
  if (n_blocks == 0) return TW_OK;
  TW_ARG_CHECK(max_n >= 4, "tw_hsic_rows: max_n %lld: a block needs at least 4 rows",
               (long long)max_n);
  TW_ARG_CHECK(max_n < (1ll << 31), "tw_hsic_rows: max_n %lld is 2^31 or more", (long long)max_n);
  HsicRows3Plan p;
  TW_ARG_CHECK(hsic_rows3_plan(n_blocks, max_n, n_sigma, p),
               "tw_hsic_rows: grid too large or d_work past %lld bytes (n_blocks %d, max_n %lld, "
               "n_sigma %d)", (long long)kHsicRows3WorkBudget, n_blocks, (long long)max_n, n_sigma);
  hipStream_t st = (hipStream_t)stream;
  double* work = (double*)d_work;
  const bool g = kern == TW_HSIC_GAUSSIAN;
  if (g && d_w)
    hsic_rows3_launch<TW_MMD_GAUSSIAN, true>(p, d_x, dx, d_y, dy, d_blk_off, n_blocks, max_n, d_c,
                                             n_sigma, d_w, work, st);
  else if (g)
    hsic_rows3_launch<TW_MMD_GAUSSIAN, false>(p, d_x, dx, d_y, dy, d_blk_off, n_blocks, max_n, d_c,
                                              n_sigma, d_w, work, st);
  else if (d_w)
    hsic_rows3_launch<TW_MMD_ENERGY, true>(p, d_x, dx, d_y, dy, d_blk_off, n_blocks, max_n, d_c,
                                           n_sigma, d_w, work, st);
  else
    hsic_rows3_launch<TW_MMD_ENERGY, false>(p, d_x, dx, d_y, dy, d_blk_off, n_blocks, max_n, d_c,
                                            n_sigma, d_w, work, st);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hsic_rows3_add, dim3((unsigned)(p.chunks * n_blocks * n_sigma)),
                     dim3(kBlock), 0, st, d_blk_off, (int)n_blocks, (int)n_sigma, (int)p.chunks,
                     max_n, p.tm, (const double*)work, d_rows);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
