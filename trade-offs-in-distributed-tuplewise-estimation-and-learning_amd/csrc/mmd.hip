// mmd.hip — kernel two-sample U-statistics of degree (2,2) (tuplewise.mmd; an
// extension, not in the reference): the unbiased MMD^2 and the energy distance,
//   h((x, x'), (z, z')) = g(x, x') + g(z, z') - g(x, z') - g(x', z)
// with g = exp(c * D) (TW_MMD_GAUSSIAN, c = -1 / (2 sigma^2)) or g = sqrt(D) (TW_MMD_ENERGY) of
// the squared Euclidean distance D of tripdist.h (one arithmetic order, never fused).
// tw_mmd_sums REDUCES: per block of the partition nothing but the three sums
//   Sxx = sum_{i<j} g(x_i, x_j)   Szz = sum_{k<l} g(z_k, z_l)   Sxz = sum_{i,k} g(x_i, z_k)
// leaves the chip.  Work items are tile pairs (kMmdT rows a side): the triangle of X tiles, the
// triangle of Z tiles (a diagonal tile counts anchor > point only) and the rectangle of X tiles
// by Z tiles, kMmdG consecutive items per workgroup.  The micro-tile is k_triplet_rows' own
// (trip_chunk): anchors staged in LDS and read as wave-uniform broadcasts, two points per lane in
// registers by chunks of coordinates, accumulators in registers; after the last chunk g is
// applied and added to a per-lane double.  The four waves of a workgroup hold the SAME kMmdT
// points and split the anchors of a step, so the rows a lane re-reads for every chunk are one
// 8 d kMmdT-byte set per workgroup (at most 64 KiB) that four waves pull through the CU's L1
// together: d / 8 bytes per pair, a quarter of k_triplet_rows' d / 2, and each chunk's loads are
// issued one chunk ahead of its arithmetic.
// tw_mmd_idx32 evaluates given quadruples.  Sums are deterministic as in selfpairs.hip: every
// workgroup writes its partials in a fixed lane / wave order into d_work and a second kernel adds
// a block's partials in a fixed order (no atomics, nothing to zero).
#include "tw_common.h"
#include "selfreduce.h"
#include "tripdist.h"
#include "mmdtile.h"  // kMmdT, kMmdSA, mmd_g, mmd_load, TW_MMD_KERN_CHECKS (shared with mmd_perm.hip)
#include <algorithm>
#include <cmath>

namespace tw {

constexpr int kMmdG = 2;                                // tile pairs per workgroup
constexpr int kMmdQPT = 4;                              // quadruples per lane (tw_mmd_idx32)

inline int64_t mmd_tiles(int64_t n) { return ceil_div(n, kMmdT); }
inline int64_t mmd_items(int64_t n, int64_t m) {
  const int64_t tx = mmd_tiles(n), tz = mmd_tiles(m);
  return tx * (tx + 1) / 2 + tz * (tz + 1) / 2 + tx * tz;
}
inline int64_t mmd_blocks_per_block(int64_t max_n, int64_t max_m) {
  return std::max<int64_t>(1, ceil_div(mmd_items(max_n, max_m), kMmdG));
}
inline int64_t mmd_idx_blocks_per_shard(int64_t max_quads) {
  return std::max<int64_t>(1, ceil_div(max_quads, (int64_t)kBlock * kMmdQPT));
}

// g of the wave's kTripTA x kTripR distances, added in a fixed order.  MASK: anchors past the
// tile's end (staged as zeros), points past the end and, on a diagonal tile, anchor <= point add
// nothing (a select, so a NaN of a masked pair does not enter).
template <int K, bool MASK>
__device__ __forceinline__ double mmd_fold(const double (&acc)[kTripTA][kTripR], double c,
                                           int a_first, int na, int diag_shift,
                                           const bool (&valid)[kTripR]) {
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < kTripTA; ++a) {
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      const double v = mmd_g<K>(acc[a][r], c);
      if (MASK) {
        // diag_shift: 0 on a diagonal tile (anchor index above the point's), else past every point
        const bool ok = valid[r] && a_first + a < na &&
                        a_first + a + diag_shift > r * kWave + (int)(threadIdx.x & (kWave - 1));
        s += ok ? v : 0.0;
      } else {
        s += v;
      }
    }
  }
  return s;
}

// Workgroup blockIdx.x = (block of the partition, group of kMmdG consecutive items of that
// block's OWN item list): a block's partials do not depend on the other blocks of the launch.
template <int K>
__global__ __launch_bounds__(kBlock) void k_mmd_sums(
    const double* __restrict__ x, const double* __restrict__ z, int d,
    const int64_t* __restrict__ blk_x_off, const int64_t* __restrict__ blk_z_off,
    int blocks_per_block, double c, double* __restrict__ work) {
  __shared__ double sa[kMmdSA * kTripMaxD];
  __shared__ double part[kBlock / kWave];
  const int b = (int)blockIdx.x / blocks_per_block;
  const int g = (int)blockIdx.x - b * blocks_per_block;
  const int64_t xb = blk_x_off[b], n = blk_x_off[b + 1] - xb;
  const int64_t zb = blk_z_off[b], m = blk_z_off[b + 1] - zb;
  const int64_t tx = (n + kMmdT - 1) / kMmdT, tz = (m + kMmdT - 1) / kMmdT;
  const int64_t ixx = tx * (tx + 1) / 2, izz = tz * (tz + 1) / 2, items = ixx + izz + tx * tz;
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const double* __restrict__ swave = sa + wid * kTripTA * kTripMaxD;
  double tot[3] = {0.0, 0.0, 0.0};
  const int64_t it_end = std::min<int64_t>(items, (int64_t)(g + 1) * kMmdG);
  for (int64_t it = (int64_t)g * kMmdG; it < it_end; ++it) {
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
    const int n_full = d / kTripDC;  // whole chunks of coordinates; the rest is the tail chunk
    const bool tail = n_full * kTripDC < d;
    double sum = 0.0;
    for (int s0 = 0; s0 < na; s0 += kMmdSA) {
      // this lane's points, first chunk: in flight while the anchors are staged
      double pc[kTripR][kTripDC];
      if (n_full > 0) mmd_load<false>(row, 0, d, pc);
      else mmd_load<true>(row, 0, d, pc);
      __syncthreads();  // the previous step's readers
      // the step's anchors: up to kMmdSA * d consecutive doubles, row stride kTripMaxD in LDS
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
        // the next chunk's loads are issued before this chunk's arithmetic (workgroup-uniform
        // branches): two waves a SIMD do not hide a load issued where it is needed
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
      if (!diag && all_valid && s0 + kMmdSA <= na)  // workgroup-uniform
        sum += mmd_fold<K, false>(acc, c, a_first, na, 0, valid);
      else
        sum += mmd_fold<K, true>(acc, c, a_first, na, diag ? 0 : kMmdT, valid);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) tot[k] += kind == k ? sum : 0.0;  // (no indexed register array)
  }
  // every slot is written, also by groups past a short block's items
  double* __restrict__ w = work + (int64_t)blockIdx.x * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double s = self_block_sum_f64(tot[k], part);
    if (threadIdx.x == 0) w[k] = s;
  }
}

// The given quadruples of every shard's range: absolute rows i, j of x and k, l of z.
template <int K>
__global__ __launch_bounds__(kBlock) void k_mmd_idx(
    const double* __restrict__ x, const double* __restrict__ z, int d,
    const int32_t* __restrict__ ii, const int32_t* __restrict__ jj,
    const int32_t* __restrict__ kk, const int32_t* __restrict__ ll,
    const int64_t* __restrict__ quad_off, int blocks_per_shard, double c,
    double* __restrict__ work) {
  __shared__ double part[kBlock / kWave];
  const int sh = (int)blockIdx.x / blocks_per_shard;
  const int bi = (int)blockIdx.x - sh * blocks_per_shard;
  const int64_t pe = quad_off[sh + 1];
  const int64_t p0 = quad_off[sh] + (int64_t)bi * (kBlock * kMmdQPT);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < kMmdQPT; ++q) {
    const int64_t p = p0 + q * kBlock + threadIdx.x;
    if (p < pe) {
      const double* __restrict__ xi = x + (int64_t)ii[p] * d;
      const double* __restrict__ xj = x + (int64_t)jj[p] * d;
      const double* __restrict__ zk = z + (int64_t)kk[p] * d;
      const double* __restrict__ zl = z + (int64_t)ll[p] * d;
      s[0] += mmd_g<K>(trip_dist(xi, xj, d), c);
      s[1] += mmd_g<K>(trip_dist(zk, zl, d), c);
      s[2] += mmd_g<K>(trip_dist(xi, zl, d), c);
      s[3] += mmd_g<K>(trip_dist(xj, zk, d), c);
    }
  }
  double* __restrict__ w = work + (int64_t)blockIdx.x * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double b = self_block_sum_f64(s[k], part);
    if (threadIdx.x == 0) w[k] = b;  // every slot is written
  }
}

}  // namespace tw

using namespace tw;

extern "C" int32_t tw_mmd_tile(void) { return kMmdT; }

extern "C" int64_t tw_mmd_work_bytes(int32_t n_blocks, int64_t max_n, int64_t max_m) {
  if (n_blocks < 0 || max_n < 0 || max_m < 0) return 0;
  return std::max<int64_t>(8, mmd_blocks_per_block(max_n, max_m) * n_blocks * 3 * 8);
}

extern "C" int64_t tw_mmd_idx_work_bytes(int32_t n_shards, int64_t max_quads) {
  if (n_shards < 0 || max_quads < 0) return 0;
  return std::max<int64_t>(8, mmd_idx_blocks_per_shard(max_quads) * n_shards * 4 * 8);
}

extern "C" int tw_mmd_sums(const double* d_x, const double* d_z, int32_t d,
                           const int64_t* d_blk_x_off, const int64_t* d_blk_z_off,
                           int32_t n_blocks, int64_t max_n, int64_t max_m, int32_t kern, double c,
                           void* d_work, double* d_out, void* stream) {
  TW_ARG_CHECK(d_x && d_z && d_blk_x_off && d_blk_z_off && d_work && d_out,
               "tw_mmd_sums: null pointer");
  TW_ARG_CHECK(n_blocks >= 0 && max_n >= 0 && max_m >= 0,
               "tw_mmd_sums: negative size (n_blocks %d, max_n %lld, max_m %lld)", n_blocks,
               (long long)max_n, (long long)max_m);
  TW_MMD_KERN_CHECKS("tw_mmd_sums");
  if (n_blocks == 0) return TW_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = mmd_blocks_per_block(max_n, max_m);
  TW_ARG_CHECK(per * n_blocks < (1ll << 31), "tw_mmd_sums: grid too large");
  const dim3 g((unsigned)(per * n_blocks)), b(kBlock);
  if (kern == TW_MMD_GAUSSIAN)
    hipLaunchKernelGGL(k_mmd_sums<TW_MMD_GAUSSIAN>, g, b, 0, st, d_x, d_z, (int)d, d_blk_x_off,
                       d_blk_z_off, (int)per, c, (double*)d_work);
  else
    hipLaunchKernelGGL(k_mmd_sums<TW_MMD_ENERGY>, g, b, 0, st, d_x, d_z, (int)d, d_blk_x_off,
                       d_blk_z_off, (int)per, c, (double*)d_work);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_self_reduce<double, 3>), dim3(n_blocks), dim3(kBlock), 0, st,
                     (const double*)d_work, (int)per, d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int tw_mmd_idx32(const double* d_x, const double* d_z, int32_t d, const int32_t* d_i,
                            const int32_t* d_j, const int32_t* d_k, const int32_t* d_l,
                            const int64_t* d_quad_off, int32_t n_shards, int64_t max_quads,
                            int32_t kern, double c, void* d_work, double* d_out, void* stream) {
  TW_ARG_CHECK(d_x && d_z && d_i && d_j && d_k && d_l && d_quad_off && d_work && d_out,
               "tw_mmd_idx32: null pointer");
  TW_ARG_CHECK(n_shards >= 0 && max_quads >= 0,
               "tw_mmd_idx32: negative size (n_shards %d, max_quads %lld)", n_shards,
               (long long)max_quads);
  TW_MMD_KERN_CHECKS("tw_mmd_idx32");
  if (n_shards == 0) return TW_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = mmd_idx_blocks_per_shard(max_quads);
  TW_ARG_CHECK(per * n_shards < (1ll << 31), "tw_mmd_idx32: grid too large");
  const dim3 g((unsigned)(per * n_shards)), b(kBlock);
  if (kern == TW_MMD_GAUSSIAN)
    hipLaunchKernelGGL(k_mmd_idx<TW_MMD_GAUSSIAN>, g, b, 0, st, d_x, d_z, (int)d, d_i, d_j, d_k,
                       d_l, d_quad_off, (int)per, c, (double*)d_work);
  else
    hipLaunchKernelGGL(k_mmd_idx<TW_MMD_ENERGY>, g, b, 0, st, d_x, d_z, (int)d, d_i, d_j, d_k,
                       d_l, d_quad_off, (int)per, c, (double*)d_work);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_self_reduce<double, 4>), dim3(n_shards), dim3(kBlock), 0, st,
                     (const double*)d_work, (int)per, d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
