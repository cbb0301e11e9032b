// mmd_rows.hip — the row sums of the kernel two-sample statistics for a grid of bandwidths
// (tuplewise.mmd_var; an extension, not in the reference).  For every row x_i
// and z_k of a block of tw_mmd_sums' partition and every coefficient c_s of the launch
//   a_i = sum_{j != i} g_s(x_i, x_j)   r_i = sum_k g_s(x_i, z_k)
//   q_k = sum_i g_s(x_i, z_k)          b_k = sum_{l != k} g_s(z_k, z_l)
// the Hajek projections the variance of MMD^2_u is estimated from.  D is tripdist.h's and g is
// mmdtile.h's mmd_g, so a term has the bits k_mmd_sums gives it.  Work items are k_mmd_sums' tile
// pairs (the triangle of X tiles, the triangle of Z tiles, the rectangle), one per workgroup, and
// the micro-tile is its own: a step's anchors in LDS read as broadcasts, two points a lane in
// registers, the four waves split the anchors of a step.  Every unordered pair is visited ONCE and
// its D is held in registers while the loop over s applies g: D costs 3 d lane-ops a pair whatever
// the grid's length.  A pair feeds its point's sum (a register add, summed over steps and waves in
// LDS) and its anchor's: 16 values a lane that hsictile.h's reduce-scatter butterfly sums over the
// wave's 128 points, 8 at a time; a wave's anchors of a step belong to no other wave or step, so
// the butterfly's result is the anchor's whole partial of the item (held in LDS to the item's end).
// One partial per row, tile COLUMN and sigma goes to d_work.  Row i of tile T of the X triangle
// has T + 1 anchor-side partials (items (I, T), I <= T, column I) and tx - T point-side ones
// (items (T, J), J >= T, column J + 1): tx + 1 columns, a diagonal tile filling two.  The Z
// triangle likewise; the rectangle gives r its tz columns (point side) and q its tx (anchor side).
// No atomics and nothing to zero: k_mmd_rows_add adds a row's columns in a fixed order.
// Everything is indexed relative to the block and by the block's own size, so a block's rows are
// the same bits alone, beside other blocks and wherever the partition starts; the loop over s runs
// the same instructions on the same D for every s, so a sigma's rows do not depend on the grid.
#include "tw_common.h"
#include "selfreduce.h"
#include "tripdist.h"
#include "mmdtile.h"   // kMmdT, kMmdSA, mmd_g, mmd_load
#include "hsictile.h"  // hsic_anchor_sums, hsic_anchor_of, hsic_anchor_lane
#include <algorithm>
#include <cmath>

namespace tw {

constexpr int kMmdRowsG = 1;                            // tile pairs per workgroup (2 measured slower)
constexpr int kMmdRowsMaxS = 8;                         // sigmas per launch (32 KiB of point sums)
constexpr int64_t kMmdRowsWorkBudget = 1ll << 30;       // bytes of d_work a launch may ask for
constexpr int kMmdAddRows = kWave;                      // rows per workgroup of k_mmd_rows_add
static_assert(kTripTA == 2 * kHsicTA, "a wave's anchors are two butterflies");

// The launch plan: everything tw_mmd_rows_work_bytes and the launch agree on.
struct MmdRowsPlan {
  int64_t per;     // workgroups per block: the tile pairs of the largest block, kMmdRowsG each
  int64_t txm, tzm;  // tiles of the largest block
  int64_t words;   // doubles of d_work per block and sigma: (txm + tzm + 1) (max_n + max_m)
  int64_t chunks;  // workgroups of k_mmd_rows_add per block and sigma
};

inline bool mmd_rows_plan(int64_t n_blocks, int64_t max_n, int64_t max_m, int n_sigma,
                          MmdRowsPlan& p) {
  if (n_blocks < 0 || max_n < 0 || max_m < 0 || max_n >= (1ll << 31) || max_m >= (1ll << 31) ||
      n_sigma < 1 || n_sigma > kMmdRowsMaxS)
    return false;
  p.txm = ceil_div(max_n, kMmdT);
  p.tzm = ceil_div(max_m, kMmdT);
  p.per = std::max<int64_t>(
      1, ceil_div(p.txm * (p.txm + 1) / 2 + p.tzm * (p.tzm + 1) / 2 + p.txm * p.tzm, kMmdRowsG));
  p.chunks = std::max<int64_t>(1, ceil_div(max_n + max_m, kMmdAddRows));
  p.words = (p.txm + p.tzm + 1) * (max_n + max_m);  // < 2^57
  if ((double)p.per * (double)n_blocks >= 2147483648.0 ||
      (double)p.chunks * (double)n_blocks * n_sigma >= 2147483648.0)
    return false;
  return (double)p.words * (double)n_blocks * n_sigma * 8.0 <= (double)kMmdRowsWorkBudget;
}

// g_s of the wave's kTripTA x kTripR distances: pr[r] the lane's points' sums over the anchors in
// ascending order, v[a] the anchors' terms of this lane's two points.  MASK as in mmd_fold.
template <int K, bool MASK>
__device__ __forceinline__ void mmd_rows_fold(const double (&acc)[kTripTA][kTripR], double c,
                                              int a_first, int na, int diag_shift, int lane,
                                              const bool (&valid)[kTripR], double (&pr)[kTripR],
                                              double (&v)[2][kHsicTA]) {
#pragma unroll
  for (int r = 0; r < kTripR; ++r) pr[r] = 0.0;
#pragma unroll
  for (int a = 0; a < kTripTA; ++a) {
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      double g = mmd_g<K>(acc[a][r], c);
      if (MASK) g = hsic_ok<MASK>(a, r, a_first, na, diag_shift, lane, valid) ? g : 0.0;
      pr[r] += g;
      v[a / kHsicTA][a % kHsicTA] = r == 0 ? g : v[a / kHsicTA][a % kHsicTA] + g;
    }
  }
}

// Workgroup blockIdx.x = (block of the partition, group of kMmdRowsG consecutive items of that
// block's OWN item list).
template <int K>
__global__ __launch_bounds__(kBlock, 2) void k_mmd_rows(
    const double* __restrict__ x, const double* __restrict__ z, int d,
    const int64_t* __restrict__ blk_x_off, const int64_t* __restrict__ blk_z_off, int per,
    const double* __restrict__ cs, int n_sigma, int64_t max_n, int64_t max_m, int64_t txm,
    int64_t tzm, double* __restrict__ work) {
  __shared__ double sa[kMmdSA * kTripMaxD];
  __shared__ double psum[kMmdRowsMaxS][kBlock / kWave][kMmdT];  // the points' sums per sigma, wave
  // the anchors' sums per sigma, held to the item's end and written beside the points' (72 KiB of
  // LDS in all: two workgroups a CU, which is what the registers allow)
  __shared__ double asum[kMmdRowsMaxS][kMmdT];
  const int b = (int)blockIdx.x / per;
  const int g = (int)blockIdx.x - b * per;
  const int64_t xb = blk_x_off[b], n = blk_x_off[b + 1] - xb;
  const int64_t zb = blk_z_off[b], m = blk_z_off[b + 1] - zb;
  const int64_t tx = (n + kMmdT - 1) / kMmdT, tz = (m + kMmdT - 1) / kMmdT;
  const int64_t ixx = tx * (tx + 1) / 2, izz = tz * (tz + 1) / 2, items = ixx + izz + tx * tz;
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const double* __restrict__ swave = sa + wid * kTripTA * kTripMaxD;
  // d_work of (block, sigma): [a: txm + 1 columns of max_n | r: tzm of max_n | q: txm of max_m |
  // b: tzm + 1 of max_m]; an item's point side and anchor side each fill one column
  const int64_t words = (txm + tzm + 1) * (max_n + max_m);
  const int64_t off_r = (txm + 1) * max_n, off_q = off_r + tzm * max_n, off_b = off_q + txm * max_m;
  double* __restrict__ wb = work + (int64_t)b * n_sigma * words;
  const int n_full = d / kTripDC;  // whole chunks of coordinates; the rest is the tail chunk
  const bool tail = n_full * kTripDC < d;
  // (a workgroup past a short block's items has nothing to do: every slot k_mmd_rows_add reads
  // is written by an item of the block's own list)
  const int64_t it_end = std::min<int64_t>(items, (int64_t)(g + 1) * kMmdRowsG);
  for (int64_t it = (int64_t)g * kMmdRowsG; it < it_end; ++it) {
    // the item's kind (0 xx, 1 zz, 2 xz), point tile I and anchor tile J: workgroup-uniform
    int kind, I, J;
    if (it < ixx) {
      kind = 0;
      self_tile_of(it, I, J);
    } else if (it < ixx + izz) {
      kind = 1;
      self_tile_of(it - ixx, I, J);
    } else {
      kind = 2;
      const int64_t q = it - ixx - izz;
      I = (int)(q / tz);
      J = (int)(q - (int64_t)I * tz);
    }
    const double* __restrict__ pts = kind == 1 ? z + zb * d : x + xb * d;
    const double* __restrict__ anc = kind == 0 ? x + xb * d : z + zb * d;
    const int64_t np = kind == 1 ? m : n, nanc = kind == 0 ? n : m;
    const int64_t p0 = (int64_t)I * kMmdT, a0 = (int64_t)J * kMmdT;
    const int na = (int)std::min<int64_t>(kMmdT, nanc - a0);  // >= 1: J is a tile of the block
    const bool diag = kind != 2 && I == J;
    const int64_t pcol = kind == 0 ? (int64_t)(J + 1) * max_n
                                   : kind == 1 ? off_b + (int64_t)(J + 1) * max_m
                                               : off_r + (int64_t)J * max_n;
    const int64_t acol = kind == 0 ? (int64_t)I * max_n
                                   : kind == 1 ? off_b + (int64_t)I * max_m
                                               : off_q + (int64_t)I * max_m;
    bool valid[kTripR];
    const double* __restrict__ row[kTripR];
    bool all_valid = true;
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      const int64_t p = p0 + r * kWave + lane;
      valid[r] = p < np;
      row[r] = pts + (valid[r] ? p : p0) * d;  // a lane past the end reads the tile's first point
      all_valid = all_valid && p0 + r * kWave + kWave <= np;
    }
    for (int s0 = 0; s0 < na; s0 += kMmdSA) {
      // k_mmd_sums' step: the lane's first chunk in flight while the anchors are staged
      double pc[kTripR][kTripDC];
      if (n_full > 0) mmd_load<false>(row, 0, d, pc);
      else mmd_load<true>(row, 0, d, pc);
      __syncthreads();  // the previous step's readers
      for (int q = threadIdx.x; q < kMmdSA * d; q += kBlock) {
        const int a = q / d, cc = q - a * d;
        sa[a * kTripMaxD + cc] = s0 + a < na ? anc[(a0 + s0) * d + q] : 0.0;
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
        trip_chunk<false>(swave, ch * kTripDC, d, pc, acc);
#pragma unroll
        for (int r = 0; r < kTripR; ++r)
#pragma unroll
          for (int cc = 0; cc < kTripDC; ++cc) pc[r][cc] = pn[r][cc];
      }
      if (tail) trip_chunk<true>(swave, n_full * kTripDC, d, pc, acc);
      const int a_first = s0 + wid * kTripTA;  // this wave's anchors of the step, tile-relative
      const bool plain = !diag && all_valid && s0 + kMmdSA <= na;  // workgroup-uniform
      // the held distances under every sigma of the launch
#pragma unroll 1
      for (int s = 0; s < n_sigma; ++s) {
        const double c = K == TW_MMD_GAUSSIAN ? cs[s] : 0.0;  // (a wave-uniform load)
        double pr[kTripR], v[2][kHsicTA];
        if (plain) mmd_rows_fold<K, false>(acc, c, a_first, na, 0, lane, valid, pr, v);
        else mmd_rows_fold<K, true>(acc, c, a_first, na, diag ? 0 : kMmdT, lane, valid, pr, v);
        const double lo = hsic_anchor_sums(v[0], lane), hi = hsic_anchor_sums(v[1], lane);
        if (hsic_anchor_lane(lane)) {  // one lane per anchor; no other wave or step holds it
          const int a = a_first + hsic_anchor_of(lane);
          asum[s][a] = lo;
          asum[s][a + kHsicTA] = hi;
        }
        // the lane's own slots: no other lane touches them before the barrier below
#pragma unroll
        for (int r = 0; r < kTripR; ++r) {
          double* __restrict__ ps = &psum[s][wid][r * kWave + lane];
          *ps = s0 == 0 ? pr[r] : *ps + pr[r];
        }
      }
    }
    // the tile's points: the four waves' sums in a fixed order, out to the item's column; the tile's
    // anchors to theirs
    __syncthreads();
    for (int q = threadIdx.x; q < n_sigma * kMmdT; q += kBlock) {
      const int s = q / kMmdT, p = q - s * kMmdT;
      const double t = (psum[s][0][p] + psum[s][1][p]) + (psum[s][2][p] + psum[s][3][p]);
      if (p0 + p < np) wb[(int64_t)s * words + pcol + p0 + p] = t;
      if (p < na) wb[(int64_t)s * words + acol + a0 + p] = asum[s][p];
    }
    // (the next item writes psum and asum behind its first step's barriers)
  }
}

// Row t of (block, sigma), kMmdAddRows rows a workgroup: an X row (t < max_n) or a Z row.  Wave p
// adds the row's columns p, p + 4, ... in ascending order (one row a lane, so that a row's loads
// are four waves deep) and the four waves' sums are paired: a fixed order.
__global__ __launch_bounds__(kBlock) void k_mmd_rows_add(
    const int64_t* __restrict__ blk_x_off, const int64_t* __restrict__ blk_z_off, int n_blocks,
    int n_sigma, int chunks, int64_t max_n, int64_t max_m, int64_t txm, int64_t tzm,
    const double* __restrict__ work, double* __restrict__ rows_x, double* __restrict__ rows_z) {
  __shared__ double col[kBlock / kWave][kMmdAddRows][2];
  const int ch = (int)blockIdx.x % chunks;
  const int bs = (int)blockIdx.x / chunks;
  const int b = bs / n_sigma, s = bs - b * n_sigma;
  const int64_t xb = blk_x_off[b], n = blk_x_off[b + 1] - xb;
  const int64_t zb = blk_z_off[b], m = blk_z_off[b + 1] - zb;
  const int64_t nx = blk_x_off[n_blocks], nz = blk_z_off[n_blocks];
  const int64_t tx = (n + kMmdT - 1) / kMmdT, tz = (m + kMmdT - 1) / kMmdT;
  const int64_t words = (txm + tzm + 1) * (max_n + max_m);
  const int64_t off_r = (txm + 1) * max_n, off_q = off_r + tzm * max_n, off_b = off_q + txm * max_m;
  const double* __restrict__ w = work + ((int64_t)b * n_sigma + s) * words;
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int64_t t = (int64_t)ch * kMmdAddRows + lane;
  const bool is_x = t < max_n;
  const int64_t i = is_x ? t : t - max_n;
  const bool live = i < (is_x ? n : m);
  // the sample's own triangle (tiles + 1 columns) and the rectangle (the other sample's tiles)
  const int64_t stride = is_x ? max_n : max_m;
  const double* __restrict__ ws = w + (is_x ? 0 : off_b) + i;
  const double* __restrict__ wc = w + (is_x ? off_r : off_q) + i;
  const int64_t self_cols = (is_x ? tx : tz) + 1, cross_cols = is_x ? tz : tx;
  double self = 0.0, cross = 0.0;
  if (live) {
#pragma unroll 8
    for (int64_t c = wid; c < self_cols; c += kBlock / kWave) self += ws[c * stride];
#pragma unroll 8
    for (int64_t c = wid; c < cross_cols; c += kBlock / kWave) cross += wc[c * stride];
  }
  col[wid][lane][0] = self;
  col[wid][lane][1] = cross;
  __syncthreads();
  if (wid != 0 || !live) return;
  self = (col[0][lane][0] + col[1][lane][0]) + (col[2][lane][0] + col[3][lane][0]);
  cross = (col[0][lane][1] + col[1][lane][1]) + (col[2][lane][1] + col[3][lane][1]);
  if (is_x) {
    double* __restrict__ o = rows_x + ((int64_t)s * nx + xb + i) * 2;
    o[0] = self;
    o[1] = cross;
  } else {
    double* __restrict__ o = rows_z + ((int64_t)s * nz + zb + i) * 2;
    o[0] = cross;
    o[1] = self;
  }
}

}  // namespace tw

using namespace tw;

extern "C" int32_t tw_mmd_rows_max_sigma(void) { return kMmdRowsMaxS; }

extern "C" int64_t tw_mmd_rows_work_bytes(int32_t n_blocks, int64_t max_n, int64_t max_m,
                                          int32_t n_sigma) {
  MmdRowsPlan p;
  if (!mmd_rows_plan(n_blocks, max_n, max_m, n_sigma, p)) return 0;
  return std::max<int64_t>(8, p.words * n_blocks * n_sigma * 8);
}

extern "C" int tw_mmd_rows(const double* d_x, const double* d_z, int32_t d,
                           const int64_t* d_blk_x_off, const int64_t* d_blk_z_off,
                           int32_t n_blocks, int64_t max_n, int64_t max_m, int32_t kern,
                           const double* d_c, int32_t n_sigma, void* d_work, double* d_rows_x,
                           double* d_rows_z, void* stream) {
  TW_ARG_CHECK(d_x && d_z && d_blk_x_off && d_blk_z_off && d_work && d_rows_x && d_rows_z &&
                   (d_c || kern == TW_MMD_ENERGY),
               "tw_mmd_rows: null pointer");
  TW_ARG_CHECK(n_blocks >= 0 && max_n >= 0 && max_m >= 0,
               "tw_mmd_rows: negative size (n_blocks %d, max_n %lld, max_m %lld)", n_blocks,
               (long long)max_n, (long long)max_m);
  TW_ARG_CHECK(d >= 1 && d <= kTripMaxD, "tw_mmd_rows: d %d outside [1, %d]", d, kTripMaxD);
  TW_ARG_CHECK(kern == TW_MMD_GAUSSIAN || kern == TW_MMD_ENERGY, "tw_mmd_rows: unknown kernel %d",
               kern);
  TW_ARG_CHECK(n_sigma >= 1 && n_sigma <= kMmdRowsMaxS, "tw_mmd_rows: n_sigma %d outside [1, %d]",
               n_sigma, kMmdRowsMaxS);
  TW_ARG_CHECK(kern != TW_MMD_ENERGY || n_sigma == 1,
               "tw_mmd_rows: n_sigma %d for the energy kernel (it takes no sigma: 1)", n_sigma);
  MmdRowsPlan p;
  TW_ARG_CHECK(mmd_rows_plan(n_blocks, max_n, max_m, n_sigma, p),
               "tw_mmd_rows: a size past 2^31, grid too large or d_work past %lld bytes (n_blocks "
               "%d, max_n %lld, max_m %lld, n_sigma %d)", (long long)kMmdRowsWorkBudget, n_blocks,
               (long long)max_n, (long long)max_m, n_sigma);
  if (n_blocks == 0) return TW_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)(p.per * n_blocks)), b(kBlock);
  if (kern == TW_MMD_GAUSSIAN)
    hipLaunchKernelGGL(k_mmd_rows<TW_MMD_GAUSSIAN>, g, b, 0, st, d_x, d_z, (int)d, d_blk_x_off,
                       d_blk_z_off, (int)p.per, d_c, (int)n_sigma, max_n, max_m, p.txm, p.tzm,
                       (double*)d_work);
  else
    hipLaunchKernelGGL(k_mmd_rows<TW_MMD_ENERGY>, g, b, 0, st, d_x, d_z, (int)d, d_blk_x_off,
                       d_blk_z_off, (int)p.per, d_c, (int)n_sigma, max_n, max_m, p.txm, p.tzm,
                       (double*)d_work);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mmd_rows_add, dim3((unsigned)(p.chunks * n_blocks * n_sigma)), b, 0, st,
                     d_blk_x_off, d_blk_z_off, (int)n_blocks, (int)n_sigma, (int)p.chunks, max_n,
                     max_m, p.txm, p.tzm, (const double*)d_work, d_rows_x, d_rows_z);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
