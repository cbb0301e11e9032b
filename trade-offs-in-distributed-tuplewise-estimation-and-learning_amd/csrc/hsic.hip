// hsic.hip — kernel independence U-statistics of degree 4 on ONE paired sample (tuplewise.hsic;
// DESIGN.md §4.14; an extension, not in the reference): the unbiased Hilbert-Schmidt independence
// criterion (Song et al. 2012) and the unbiased squared distance covariance (Szekely-Rizzo 2014).
// With K_ij = g_x(D(x_i, x_j)), L_ij = g_y(D(y_i, y_j)) (zero diagonals; D of tripdist.h, g of
// mmdtile.h, so a K_ij has the bits k_mmd_sums gives it) and the row sums k_i = sum_j K_ij,
// l_i = sum_j L_ij, tw_hsic_sums leaves eight doubles per block of the partition,
//   S_KL S_KK S_LL (sums over i < j of K L, K K, L L)   R_K R_L R_KL R_KK R_LL (sums over i of
//   k, l, k l, k k, l l)
// and, if asked, the row sums themselves.  Every unordered pair is evaluated ONCE: the micro-tile
// is k_mmd_sums' own (trip_chunk: a step's anchors in LDS read as broadcasts, two points a lane in
// registers) with kHsicTA = 8 anchors a wave, so that one side's g values and the other side's
// accumulators fit in registers beside each other at two waves per SIMD (16 anchors need 318
// registers).  A step stages both sides' anchors; a wave runs the X side, folds K in place (S_KK,
// the row sums' K terms), runs the Y side of the same anchors and points and folds L against the
// held K (S_KL, S_LL).  A pair feeds the row sum of the lane's own point (a register add) and of
// the anchor: 8 values a side that a reduce-scatter butterfly sums over the wave's 128 points
// (about 70 VALU a side and step against the step's 1650).
// A workgroup owns a super-tile of group x group tiles (kMmdT rows a tile edge) of the triangle
// of super-tiles; a diagonal super-tile and a diagonal tile visit anchor > point only.  The
// anchors' row sums live in LDS across the super-tile's tile pairs, the points' in registers
// across a tile row; one partial per row and super-tile COLUMN goes to d_work (row i of
// super-tile R, column C: the point side of workgroup (R, C) if C > R, the anchor side of (C, R)
// if C < R, both sides of (R, R)), so the partials are n * ceil(n / (128 group)) pairs of doubles.
// No atomics and nothing to zero: k_hsic_rows adds a row's partials in a fixed order, writes the
// row sums and sums the five R's per 64 rows, k_hsic_final adds a block's partials in a fixed
// order.  Everything is indexed relative to the block and by the block's own size, so a
// block's outputs are the same bits alone, beside other blocks and wherever the partition starts.
// tw_hsic_idx32 evaluates given 4-tuples (the incomplete statistic).
#include "tw_common.h"
#include "selfreduce.h"
#include "tripdist.h"
#include "mmdtile.h"  // kMmdT, kMmdSA, mmd_g, mmd_load (shared with mmd.hip, mmd_perm.hip)
#include "hsictile.h"  // kHsicTA, kHsicSA, hsic_stage, hsic_side, hsic_ok, hsic_anchor_sums (shared)
#include <algorithm>
#include <cmath>

namespace tw {

constexpr int kHsicMaxGroup = 8;                        // tiles per super-tile edge, at most
constexpr int kHsicRowsPerWg = kWave;                   // rows per workgroup of k_hsic_rows
constexpr int kHsicQPT = 4;                             // 4-tuples per lane (tw_hsic_idx32)
constexpr int64_t kHsicWorkBudget = 1ll << 30;          // bytes of d_work a launch may ask for
constexpr int64_t kHsicMinWgs = 2 * 2 * 256;            // two rounds on 256 CUs x 2 workgroups
static_assert(kBlock / kWave * kMmdT * 2 <= kHsicSA * kTripMaxD, "the point scratch aliases sax");
static_assert(2 * kMmdT == kBlock, "one thread per point and side in the point-side combine");

// The launch plan of tw_hsic_sums: everything tw_hsic_work_bytes and the launch agree on.
struct HsicPlan {
  int group;        // tiles per super-tile edge
  int64_t smax;     // super-tiles per edge of the largest block
  int64_t per;      // workgroups per block: the triangle of super-tiles
  int64_t rpad;     // rows of the largest block, rounded up to whole super-tiles
  int64_t chunks;   // workgroups of k_hsic_rows per block
  int64_t off_rows, off_r5, words;  // layout of d_work in doubles: [pair sums | R partials | rows]
};

inline bool hsic_plan_at(int64_t n_blocks, int64_t max_n, int group, HsicPlan& p) {
  const int64_t tiles = ceil_div(max_n, kMmdT);
  p.group = group;
  p.smax = ceil_div(tiles, group);
  p.per = p.smax * (p.smax + 1) / 2;
  p.rpad = p.smax * group * kMmdT;
  p.chunks = ceil_div(max_n, kHsicRowsPerWg);
  if (p.per * n_blocks >= (1ll << 31) || p.chunks * n_blocks >= (1ll << 31)) return false;
  p.off_r5 = n_blocks * p.per * 3;
  p.off_rows = p.off_r5 + n_blocks * p.chunks * 5;
  if ((double)n_blocks * (double)p.smax * (double)p.rpad * 16.0 > (double)kHsicWorkBudget)
    return false;  // (and no overflow below)
  p.words = p.off_rows + n_blocks * p.smax * p.rpad * 2;
  return p.words * 8 <= kHsicWorkBudget;
}

// group = 0: the largest group that still leaves kHsicMinWgs workgroups (1 if none does), raised
// while d_work is over the budget.  false: the shape is refused.
inline bool hsic_plan(int64_t n_blocks, int64_t max_n, int group, HsicPlan& p) {
  if (n_blocks < 1 || max_n < 4 || max_n >= (1ll << 31) || group < 0 || group > kHsicMaxGroup)
    return false;
  if (group > 0) return hsic_plan_at(n_blocks, max_n, group, p);
  int g = 1;
  for (int t = kHsicMaxGroup; t > 1; --t) {
    const int64_t s = ceil_div(ceil_div(max_n, kMmdT), t);
    if (s * (s + 1) / 2 * n_blocks >= kHsicMinWgs) {
      g = t;
      break;
    }
  }
  for (; g <= kHsicMaxGroup; ++g)
    if (hsic_plan_at(n_blocks, max_n, g, p)) return true;
  return false;
}

inline int64_t hsic_idx_blocks_per_shard(int64_t max_quads) {
  return std::max<int64_t>(1, ceil_div(max_quads, (int64_t)kBlock * kHsicQPT));
}

// (hsic_stage, hsic_side, hsic_ok and the butterfly hsic_anchor_sums are hsictile.h's.)  The fold
// runs one side at a time so that only one side's distances are live beside the other's g values.
// The X side: ak becomes K (masked), S_KK, the lane's points' k terms, the anchors' terms vk.
template <int K, bool MASK>
__device__ __forceinline__ void hsic_fold_k(double (&ak)[kHsicTA][kTripR], double cx, int a_first,
                                            int na, int diag_shift, int lane,
                                            const bool (&valid)[kTripR], double& skk,
                                            double (&rk)[kTripR], double (&vk)[kHsicTA]) {
#pragma unroll
  for (int a = 0; a < kHsicTA; ++a) {
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      double k = mmd_g<K>(ak[a][r], cx);
      if (MASK) k = hsic_ok<MASK>(a, r, a_first, na, diag_shift, lane, valid) ? k : 0.0;
      ak[a][r] = k;
      skk += k * k;
      rk[r] += k;
      vk[a] = r == 0 ? k : vk[a] + k;
    }
  }
}

// The Y side against the K of hsic_fold_k: S_KL, S_LL, the points' l terms, the anchors' vl.
template <int K, bool MASK>
__device__ __forceinline__ void hsic_fold_l(const double (&ak)[kHsicTA][kTripR],
                                            const double (&al)[kHsicTA][kTripR], double cy,
                                            int a_first, int na, int diag_shift, int lane,
                                            const bool (&valid)[kTripR], double& skl, double& sll,
                                            double (&rl)[kTripR], double (&vl)[kHsicTA]) {
#pragma unroll
  for (int a = 0; a < kHsicTA; ++a) {
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      double l = mmd_g<K>(al[a][r], cy);
      if (MASK) l = hsic_ok<MASK>(a, r, a_first, na, diag_shift, lane, valid) ? l : 0.0;
      skl += ak[a][r] * l;
      sll += l * l;
      rl[r] += l;
      vl[a] = r == 0 ? l : vl[a] + l;
    }
  }
}

// Workgroup blockIdx.x = (block of the partition, super-tile pair of that block's OWN triangle).
template <int K>
__global__ __launch_bounds__(kBlock, 2) void k_hsic_sums(
    const double* __restrict__ x, int dx, const double* __restrict__ y, int dy,
    const int64_t* __restrict__ blk_off, int per, int group, int64_t smax, int64_t rpad, double cx,
    double cy, double* __restrict__ work_s, double* __restrict__ work_rows) {
  __shared__ double sax[kHsicSA * kTripMaxD];         // a step's anchors, X side; the point scratch
  __shared__ double say[kHsicSA * kTripMaxD];         // and Y side
  __shared__ double asum[2][kHsicMaxGroup * kMmdT];   // the anchors' row sums (K, L)
  __shared__ double part[kBlock / kWave];
  const int b = (int)blockIdx.x / per;
  const int w = (int)blockIdx.x - b * per;
  const int64_t r0 = blk_off[b], n = blk_off[b + 1] - r0;
  const int64_t tiles = (n + kMmdT - 1) / kMmdT, st = (tiles + group - 1) / group;
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const double* __restrict__ swx = sax + wid * kHsicTA * kTripMaxD;
  const double* __restrict__ swy = say + wid * kHsicTA * kTripMaxD;
  const double* __restrict__ xb = x + r0 * dx;
  const double* __restrict__ yb = y + r0 * dy;
  double* __restrict__ wr = work_rows + (int64_t)b * smax * rpad * 2;
  double tot[3] = {0.0, 0.0, 0.0};
  if (w < st * (st + 1) / 2) {  // workgroup-uniform: a super-tile pair of this block
    int SI, SJ;
    self_tile_of(w, SI, SJ);  // points' super-tile SI <= anchors' super-tile SJ
    const bool sdiag = SI == SJ;
    for (int q = threadIdx.x; q < group * kMmdT; q += kBlock) asum[0][q] = asum[1][q] = 0.0;
    for (int ti = 0; ti < group; ++ti) {
      const int64_t I = (int64_t)SI * group + ti;
      if (I >= tiles) break;
      const int64_t p0 = I * kMmdT;
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
      double rk[kTripR] = {0.0, 0.0}, rl[kTripR] = {0.0, 0.0};
      for (int tj = sdiag ? ti : 0; tj < group; ++tj) {
        const int64_t J = (int64_t)SJ * group + tj;
        if (J >= tiles) break;
        const int64_t a0 = J * kMmdT;
        const int na = (int)std::min<int64_t>(kMmdT, n - a0);  // >= 1: J is a tile of the block
        const bool diag = I == J;
        for (int s0 = 0; s0 < na; s0 += kHsicSA) {
          double pc[kTripR][kTripDC];
          double ak[kHsicTA][kTripR], al[kHsicTA][kTripR], v[kHsicTA];
          const int a_first = s0 + wid * kHsicTA;  // this wave's anchors of the step, tile-relative
          const bool plain = !diag && all_valid && s0 + kHsicSA <= na;  // workgroup-uniform
          const int shift = diag ? 0 : kMmdT;
          // the X side: the lane's first chunk is in flight while both sides' anchors are staged
          if (dx >= kTripDC) mmd_load<false>(rowx, 0, dx, pc);
          else mmd_load<true>(rowx, 0, dx, pc);
          __syncthreads();  // the previous readers of sax, say
          hsic_stage(sax, xb + (a0 + s0) * dx, dx, na - s0);
          hsic_stage(say, yb + (a0 + s0) * dy, dy, na - s0);
          __syncthreads();
#pragma unroll
          for (int a = 0; a < kHsicTA; ++a)
#pragma unroll
            for (int r = 0; r < kTripR; ++r) ak[a][r] = 0.0;
          hsic_side(rowx, dx, swx, pc, ak);
          // the Y side of the same anchors and points: its first chunk in flight under K's fold
          if (dy >= kTripDC) mmd_load<false>(rowy, 0, dy, pc);
          else mmd_load<true>(rowy, 0, dy, pc);
          if (plain) hsic_fold_k<K, false>(ak, cx, a_first, na, 0, lane, valid, tot[1], rk, v);
          else hsic_fold_k<K, true>(ak, cx, a_first, na, shift, lane, valid, tot[1], rk, v);
          const double sk = hsic_anchor_sums(v, lane);
#pragma unroll
          for (int a = 0; a < kHsicTA; ++a)
#pragma unroll
            for (int r = 0; r < kTripR; ++r) al[a][r] = 0.0;
          hsic_side(rowy, dy, swy, pc, al);
          if (plain) hsic_fold_l<K, false>(ak, al, cy, a_first, na, 0, lane, valid, tot[0], tot[2],
                                           rl, v);
          else hsic_fold_l<K, true>(ak, al, cy, a_first, na, shift, lane, valid, tot[0], tot[2], rl,
                                    v);
          const double sl = hsic_anchor_sums(v, lane);
          if (hsic_anchor_lane(lane)) {  // one lane per anchor; no other wave or step holds it
            const int q = tj * kMmdT + a_first + hsic_anchor_of(lane);
            asum[0][q] += sk;
            asum[1][q] += sl;
          }
        }
      }
      // the tile row's points: the four waves' sums in a fixed order, one thread per point and side
      __syncthreads();  // sax's readers; asum's writers
      sax[(wid * kMmdT + lane) * 2 + 0] = rk[0];
      sax[(wid * kMmdT + lane) * 2 + 1] = rl[0];
      sax[(wid * kMmdT + kWave + lane) * 2 + 0] = rk[1];
      sax[(wid * kMmdT + kWave + lane) * 2 + 1] = rl[1];
      __syncthreads();
      {
        const int p = threadIdx.x >> 1, side = threadIdx.x & 1;
        double v = (sax[p * 2 + side] + sax[(kMmdT + p) * 2 + side]) +
                   (sax[(2 * kMmdT + p) * 2 + side] + sax[(3 * kMmdT + p) * 2 + side]);
        // a diagonal super-tile: the row's anchor side is complete (tiles I' <= I are done)
        if (sdiag) v += asum[side][ti * kMmdT + p];
        if (p0 + p < n) wr[((int64_t)SJ * rpad + p0 + p) * 2 + side] = v;
      }
    }
    if (!sdiag) {  // the anchors' rows, column SI
      __syncthreads();
      for (int q = threadIdx.x; q < group * kMmdT * 2; q += kBlock) {
        const int64_t row = (int64_t)SJ * group * kMmdT + (q >> 1);
        if (row < n) wr[((int64_t)SI * rpad + row) * 2 + (q & 1)] = asum[q & 1][q >> 1];
      }
    }
  }
  // every slot is written, also by workgroups past a short block's super-tile pairs
  double* __restrict__ ws = work_s + (int64_t)blockIdx.x * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double s = self_block_sum_f64(tot[k], part);
    if (threadIdx.x == 0) ws[k] = s;
  }
}

// Row i of block b: its partials added in a fixed order (wave p of the workgroup adds the columns
// c = p, p + 4, ... in ascending order, then the four waves' sums are paired), the row sums out,
// the five R terms summed over the workgroup's kHsicRowsPerWg rows.
__global__ __launch_bounds__(kBlock) void k_hsic_rows(
    const int64_t* __restrict__ blk_off, int chunks, int group, int64_t smax, int64_t rpad,
    const double* __restrict__ work_rows, double* __restrict__ work_r5,
    double* __restrict__ rows) {
  __shared__ double col[kBlock / kWave][kHsicRowsPerWg][2];
  const int b = (int)blockIdx.x / chunks;
  const int ch = (int)blockIdx.x - b * chunks;
  const int64_t r0 = blk_off[b], n = blk_off[b + 1] - r0;
  const int64_t tiles = (n + kMmdT - 1) / kMmdT, st = (tiles + group - 1) / group;
  const double* __restrict__ wr = work_rows + (int64_t)b * smax * rpad * 2;
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int64_t i = (int64_t)ch * kHsicRowsPerWg + lane;
  double k = 0.0, l = 0.0;
  if (i < n) {
#pragma unroll 8
    for (int64_t c = wid; c < st; c += kBlock / kWave) {
      k += wr[(c * rpad + i) * 2 + 0];
      l += wr[(c * rpad + i) * 2 + 1];
    }
  }
  col[wid][lane][0] = k;
  col[wid][lane][1] = l;
  __syncthreads();
  if (wid != 0) return;
  k = (col[0][lane][0] + col[1][lane][0]) + (col[2][lane][0] + col[3][lane][0]);
  l = (col[0][lane][1] + col[1][lane][1]) + (col[2][lane][1] + col[3][lane][1]);
  if (i < n && rows) {
    rows[(r0 + i) * 2 + 0] = k;
    rows[(r0 + i) * 2 + 1] = l;
  }
  const double t[5] = {k, l, k * l, k * k, l * l};  // (zeros from the lanes past the block)
  double* __restrict__ w5 = work_r5 + (int64_t)blockIdx.x * 5;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const double s = wave_sum_f64(t[q]);
    if (lane == 0) w5[q] = s;
  }
}

// out[b][0..2] = the block's pair sums over its `per` workgroups, out[b][3..7] = the R terms over
// its `chunks` workgroups: k_self_reduce's order (lane-strided, butterfly, waves).
__global__ __launch_bounds__(kBlock) void k_hsic_final(const double* __restrict__ work_s, int per,
                                                       const double* __restrict__ work_r5,
                                                       int chunks, double* __restrict__ out) {
  __shared__ double part[kBlock / kWave];
  const double* __restrict__ ws = work_s + (int64_t)blockIdx.x * per * 3;
  const double* __restrict__ w5 = work_r5 + (int64_t)blockIdx.x * chunks * 5;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double v = 0.0;
    if (k < 3) {
#pragma unroll 4
      for (int i = threadIdx.x; i < per; i += kBlock) v += ws[(int64_t)i * 3 + k];
    } else {
#pragma unroll 4
      for (int i = threadIdx.x; i < chunks; i += kBlock) v += w5[(int64_t)i * 5 + (k - 3)];
    }
    const double s = self_block_sum_f64(v, part);
    if (threadIdx.x == 0) out[(int64_t)blockIdx.x * 8 + k] = s;
  }
}

// The given 4-tuples of every shard's range (absolute rows of both arrays): A = sum K_ij L_ij,
// B = sum K_ij L_qr, C = sum K_ij L_iq.
template <int K>
__global__ __launch_bounds__(kBlock) void k_hsic_idx(
    const double* __restrict__ x, int dx, const double* __restrict__ y, int dy,
    const int32_t* __restrict__ ii, const int32_t* __restrict__ jj,
    const int32_t* __restrict__ qq, const int32_t* __restrict__ rr,
    const int64_t* __restrict__ quad_off, int blocks_per_shard, double cx, double cy,
    double* __restrict__ work) {
  __shared__ double part[kBlock / kWave];
  const int sh = (int)blockIdx.x / blocks_per_shard;
  const int bi = (int)blockIdx.x - sh * blocks_per_shard;
  const int64_t pe = quad_off[sh + 1];
  const int64_t p0 = quad_off[sh] + (int64_t)bi * (kBlock * kHsicQPT);
  double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < kHsicQPT; ++t) {
    const int64_t p = p0 + t * kBlock + threadIdx.x;
    if (p < pe) {
      const int64_t i = ii[p], j = jj[p], q = qq[p], r = rr[p];
      const double kij = mmd_g<K>(trip_dist(x + i * dx, x + j * dx, dx), cx);
      s[0] += kij * mmd_g<K>(trip_dist(y + i * dy, y + j * dy, dy), cy);
      s[1] += kij * mmd_g<K>(trip_dist(y + q * dy, y + r * dy, dy), cy);
      s[2] += kij * mmd_g<K>(trip_dist(y + i * dy, y + q * dy, dy), cy);
    }
  }
  double* __restrict__ w = work + (int64_t)blockIdx.x * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double b = self_block_sum_f64(s[k], part);
    if (threadIdx.x == 0) w[k] = b;  // every slot is written
  }
}

}  // namespace tw

using namespace tw;

#define TW_HSIC_KERN_CHECKS(fn)                                                                 \
  TW_ARG_CHECK(dx >= 1 && dx <= kTripMaxD, fn ": dx %d outside [1, %d]", dx, kTripMaxD);        \
  TW_ARG_CHECK(dy >= 1 && dy <= kTripMaxD, fn ": dy %d outside [1, %d]", dy, kTripMaxD);        \
  TW_ARG_CHECK(kern == TW_HSIC_GAUSSIAN || kern == TW_HSIC_DISTANCE, fn ": unknown kernel %d",  \
               kern);                                                                           \
  TW_ARG_CHECK(kern != TW_HSIC_GAUSSIAN ||                                                      \
                   (std::isfinite(c_x) && c_x <= 0.0 && std::isfinite(c_y) && c_y <= 0.0),      \
               fn ": c_x = %g, c_y = %g for the Gaussian kernel (finite and <= 0: -1 / (2 "     \
                  "sigma^2))", c_x, c_y)
static_assert(TW_HSIC_GAUSSIAN == TW_MMD_GAUSSIAN && TW_HSIC_DISTANCE == TW_MMD_ENERGY,
              "mmd_g is instantiated by the TW_MMD ids");

extern "C" int32_t tw_hsic_tile(void) { return kMmdT; }

extern "C" int64_t tw_hsic_work_bytes(int32_t n_blocks, int64_t max_n, int32_t group) {
  HsicPlan p;
  return hsic_plan(n_blocks, max_n, group, p) ? p.words * 8 : 0;
}

extern "C" int64_t tw_hsic_idx_work_bytes(int32_t n_shards, int64_t max_quads) {
  if (n_shards < 0 || max_quads < 0) return 0;
  const int64_t per = hsic_idx_blocks_per_shard(max_quads);
  if (per * n_shards >= (1ll << 31)) return 0;
  return std::max<int64_t>(8, per * n_shards * 3 * 8);
}

extern "C" int tw_hsic_sums(const double* d_x, int32_t dx, const double* d_y, int32_t dy,
                            const int64_t* d_blk_off, int32_t n_blocks, int64_t max_n,
                            int32_t kern, double c_x, double c_y, int32_t group, void* d_work,
                            double* d_rows, double* d_out, void* stream) {
  TW_ARG_CHECK(d_x && d_y && d_blk_off && d_work && d_out, "tw_hsic_sums: null pointer");
  TW_ARG_CHECK(n_blocks >= 0 && max_n >= 0, "tw_hsic_sums: negative size (n_blocks %d, max_n %lld)",
               n_blocks, (long long)max_n);
  TW_HSIC_KERN_CHECKS("tw_hsic_sums");
  TW_ARG_CHECK(group >= 0 && group <= kHsicMaxGroup, "tw_hsic_sums: group %d outside [0, %d]",
               group, kHsicMaxGroup);
  if (n_blocks == 0) return TW_OK;
  TW_ARG_CHECK(max_n >= 4, "tw_hsic_sums: max_n %lld: a block needs at least 4 rows",
               (long long)max_n);
  HsicPlan p;
  TW_ARG_CHECK(hsic_plan(n_blocks, max_n, group, p),
               "tw_hsic_sums: grid too large or d_work past %lld bytes (n_blocks %d, max_n %lld, "
               "group %d)", (long long)kHsicWorkBudget, n_blocks, (long long)max_n, group);
  hipStream_t st = (hipStream_t)stream;
  double* work = (double*)d_work;
  const dim3 g((unsigned)(p.per * n_blocks)), b(kBlock);
  if (kern == TW_HSIC_GAUSSIAN)
    hipLaunchKernelGGL(k_hsic_sums<TW_MMD_GAUSSIAN>, g, b, 0, st, d_x, (int)dx, d_y, (int)dy,
                       d_blk_off, (int)p.per, p.group, p.smax, p.rpad, c_x, c_y, work,
                       work + p.off_rows);
  else
    hipLaunchKernelGGL(k_hsic_sums<TW_MMD_ENERGY>, g, b, 0, st, d_x, (int)dx, d_y, (int)dy,
                       d_blk_off, (int)p.per, p.group, p.smax, p.rpad, c_x, c_y, work,
                       work + p.off_rows);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hsic_rows, dim3((unsigned)(p.chunks * n_blocks)), b, 0, st, d_blk_off,
                     (int)p.chunks, p.group, p.smax, p.rpad, (const double*)(work + p.off_rows),
                     work + p.off_r5, d_rows);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hsic_final, dim3(n_blocks), b, 0, st, (const double*)work, (int)p.per,
                     (const double*)(work + p.off_r5), (int)p.chunks, d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int tw_hsic_idx32(const double* d_x, int32_t dx, const double* d_y, int32_t dy,
                             const int32_t* d_i, const int32_t* d_j, const int32_t* d_q,
                             const int32_t* d_r, const int64_t* d_quad_off, int32_t n_shards,
                             int64_t max_quads, int32_t kern, double c_x, double c_y, void* d_work,
                             double* d_out, void* stream) {
  TW_ARG_CHECK(d_x && d_y && d_i && d_j && d_q && d_r && d_quad_off && d_work && d_out,
               "tw_hsic_idx32: null pointer");
  TW_ARG_CHECK(n_shards >= 0 && max_quads >= 0,
               "tw_hsic_idx32: negative size (n_shards %d, max_quads %lld)", n_shards,
               (long long)max_quads);
  TW_HSIC_KERN_CHECKS("tw_hsic_idx32");
  if (n_shards == 0) return TW_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = hsic_idx_blocks_per_shard(max_quads);
  TW_ARG_CHECK(per * n_shards < (1ll << 31), "tw_hsic_idx32: grid too large");
  const dim3 g((unsigned)(per * n_shards)), b(kBlock);
  if (kern == TW_HSIC_GAUSSIAN)
    hipLaunchKernelGGL(k_hsic_idx<TW_MMD_GAUSSIAN>, g, b, 0, st, d_x, (int)dx, d_y, (int)dy, d_i,
                       d_j, d_q, d_r, d_quad_off, (int)per, c_x, c_y, (double*)d_work);
  else
    hipLaunchKernelGGL(k_hsic_idx<TW_MMD_ENERGY>, g, b, 0, st, d_x, (int)dx, d_y, (int)dy, d_i,
                       d_j, d_q, d_r, d_quad_off, (int)per, c_x, c_y, (double*)d_work);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_self_reduce<double, 3>), dim3(n_shards), dim3(kBlock), 0, st,
                     (const double*)d_work, (int)per, d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
