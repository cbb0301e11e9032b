// triplets.hip — two-sample triplet U-statistics of degree (2,1) (tuplewise.triplets; DESIGN.md
// §4.10; an extension, not in the reference): h = 1{D(x_i, z_k) > D(x_i, x_j)}, j != i, with D
// the squared Euclidean distance accumulated in ascending coordinate order, multiply and add
// separate (the build has -ffp-contract=off):
//   acc = 0.0; for c in 0..d-1: t = a_c - b_c; acc = acc + t * t
// For a fixed anchor x_i the count over all (j, k) is a two-sample count between two rows of
// distances, so tw_triplet_rows only WRITES those rows (the "other" row D(x_i, z_k) and the
// "own" row D(x_i, x_j), j != i) and tw_count_pairs / tw_count_pairs_sorted count them, one
// anchor one shard.  tw_triplet_idx32 evaluates given triplets (i, j, k) directly.
#include "tw_common.h"
#include "selfreduce.h"
#include "tripdist.h"
#include <algorithm>

namespace tw {

constexpr int kTripP = kBlock * kTripR;       // points per tile edge
constexpr int kTripPPT = 4;                   // triplets per lane (tw_triplet_idx32)

// A NaN distance is stored as THE quiet NaN 0x7ff8000000000000: which NaN an operation returns
// (sign, payload) is the hardware's choice — a subtraction here negates its NaN operand, an x86
// one does not — and the rows are specified bit for bit.  Counts never see the difference.
__device__ __forceinline__ double trip_canon(double v) {
  return v != v ? __longlong_as_double(0x7ff8000000000000ll) : v;
}

// Grid: blockIdx.y = block of the partition (blk_first + y), blockIdx.x = (anchor tile of that
// block, point tile), point tiles [0, pt_other) over the block's Z rows (the "other" row) and
// [pt_other, pt_all) over its X rows (the "own" row, the anchor itself left out).  A workgroup
// whose tile lies outside its block's anchors or points leaves at once, so blocks of any mix of
// sizes share one launch.
__global__ __launch_bounds__(kBlock) void k_triplet_rows(
    const double* __restrict__ x, const double* __restrict__ z, int d,
    const int64_t* __restrict__ blk_x_off, const int64_t* __restrict__ blk_z_off, int blk_first,
    int64_t a_begin, int64_t a_end, int pt_other, int pt_all,
    const int64_t* __restrict__ other_off, const int64_t* __restrict__ own_off,
    double* __restrict__ other, double* __restrict__ own) {
  __shared__ double sa[kTripTA * kTripMaxD];
  const int b = blk_first + (int)blockIdx.y;
  const int64_t xb = blk_x_off[b], xe = blk_x_off[b + 1];
  const int64_t lo = std::max(xb, a_begin), hi = std::min(xe, a_end);
  const int at = (int)(blockIdx.x / (unsigned)pt_all);
  int pt = (int)(blockIdx.x - (unsigned)at * (unsigned)pt_all);
  const int64_t a0 = lo + (int64_t)at * kTripTA;
  if (a0 >= hi) return;
  const int na = (int)std::min<int64_t>(kTripTA, hi - a0);
  const bool is_own = pt >= pt_other;
  if (is_own) pt -= pt_other;
  const int64_t zb = blk_z_off[b];
  const int64_t np = is_own ? xe - xb : blk_z_off[b + 1] - zb;
  const int64_t p0 = (int64_t)pt * kTripP;
  if (p0 >= np) return;
  const double* __restrict__ pts = is_own ? x + xb * d : z + zb * d;

  // the tile's anchors: na * d consecutive doubles of x, row stride kTripMaxD in LDS
  for (int q = threadIdx.x; q < kTripTA * d; q += kBlock) {
    const int a = q / d, c = q - a * d;
    sa[a * kTripMaxD + c] = a < na ? x[a0 * d + q] : 0.0;
  }
  __syncthreads();

  double acc[kTripTA][kTripR];
#pragma unroll
  for (int a = 0; a < kTripTA; ++a)
#pragma unroll
    for (int r = 0; r < kTripR; ++r) acc[a][r] = 0.0;
  bool valid[kTripR];
  const double* __restrict__ row[kTripR];
#pragma unroll
  for (int r = 0; r < kTripR; ++r) {
    const int64_t p = p0 + r * kBlock + threadIdx.x;
    valid[r] = p < np;
    row[r] = pts + (valid[r] ? p : p0) * d;  // a lane past the end reads the tile's first point
  }
  int c0 = 0;
  for (; c0 + kTripDC <= d; c0 += kTripDC) {
    double pc[kTripR][kTripDC];
#pragma unroll
    for (int r = 0; r < kTripR; ++r)
#pragma unroll
      for (int c = 0; c < kTripDC; ++c) pc[r][c] = row[r][c0 + c];
    trip_chunk<false>(sa, c0, d, pc, acc);
  }
  if (c0 < d) {
    double pc[kTripR][kTripDC];
#pragma unroll
    for (int r = 0; r < kTripR; ++r)
#pragma unroll
      for (int c = 0; c < kTripDC; ++c) pc[r][c] = c0 + c < d ? row[r][c0 + c] : 0.0;
    trip_chunk<true>(sa, c0, d, pc, acc);
  }

  // rows: consecutive lanes write consecutive entries (the own row one to the left past i)
#pragma unroll
  for (int a = 0; a < kTripTA; ++a) {
    const int64_t ai = a0 + a;
    const bool live = a < na;  // (no break: the unrolled loop keeps acc in registers)
    if (live && !is_own) {
      double* __restrict__ dst = other + other_off[ai - a_begin];
#pragma unroll
      for (int r = 0; r < kTripR; ++r) {
        const int64_t p = p0 + r * kBlock + threadIdx.x;
        if (valid[r]) dst[p] = trip_canon(acc[a][r]);
      }
    }
    if (live && is_own) {
      double* __restrict__ dst = own + own_off[ai - a_begin];
      const int64_t self = ai - xb;
#pragma unroll
      for (int r = 0; r < kTripR; ++r) {
        const int64_t p = p0 + r * kBlock + threadIdx.x;
        if (valid[r] && p != self) dst[p - (p > self ? 1 : 0)] = trip_canon(acc[a][r]);
      }
    }
  }
}

// The given triplets of every shard's range: absolute rows i, j of x and k of z.
template <int PRED>
__global__ __launch_bounds__(kBlock) void k_triplet_idx(
    const double* __restrict__ x, const double* __restrict__ z, int d,
    const int32_t* __restrict__ ii, const int32_t* __restrict__ jj,
    const int32_t* __restrict__ kk, const int64_t* __restrict__ trip_off, int blocks_per_shard,
    unsigned long long* __restrict__ work) {
  __shared__ unsigned long long part[kBlock / kWave];
  const int sh = (int)blockIdx.x / blocks_per_shard;
  const int bi = (int)blockIdx.x - sh * blocks_per_shard;
  const int64_t pe = trip_off[sh + 1];
  const int64_t p0 = trip_off[sh] + (int64_t)bi * (kBlock * kTripPPT);
  unsigned cnt = 0;
#pragma unroll
  for (int q = 0; q < kTripPPT; ++q) {
    const int64_t p = p0 + q * kBlock + threadIdx.x;
    if (p < pe) {
      const double* __restrict__ xi = x + (int64_t)ii[p] * d;
      const double other = trip_dist(xi, z + (int64_t)kk[p] * d, d);
      const double own = trip_dist(xi, x + (int64_t)jj[p] * d, d);
      if constexpr (PRED == TW_PRED_HALF) cnt += 2u * (other > own) + (other == own);
      else cnt += other > own;
    }
  }
  const unsigned long long s = self_block_sum_u64(cnt, part);
  if (threadIdx.x == 0) work[blockIdx.x] = s;  // every slot is written
}

inline int64_t trip_idx_blocks_per_shard(int64_t max_triplets) {
  return std::max<int64_t>(1, ceil_div(max_triplets, (int64_t)kBlock * kTripPPT));
}

}  // namespace tw

using namespace tw;

extern "C" int32_t tw_triplet_rows_tile(void) { return kTripP; }

extern "C" int tw_triplet_rows(const double* d_x, const double* d_z, int32_t d,
                               const int64_t* d_blk_x_off, const int64_t* d_blk_z_off,
                               int32_t blk_first, int32_t blk_count, int64_t a_begin,
                               int64_t a_end, int64_t max_n, int64_t max_m,
                               const int64_t* d_other_off, const int64_t* d_own_off,
                               double* d_other, double* d_own, void* stream) {
  TW_ARG_CHECK(d_x && d_z && d_blk_x_off && d_blk_z_off && d_other_off && d_own_off && d_other &&
                   d_own,
               "tw_triplet_rows: null pointer");
  TW_ARG_CHECK(d >= 1 && d <= kTripMaxD, "tw_triplet_rows: d %d outside [1, %d]", d, kTripMaxD);
  TW_ARG_CHECK(blk_first >= 0 && blk_count >= 1 && max_n >= 0 && max_m >= 0 && a_begin >= 0,
               "tw_triplet_rows: negative size (blk_first %d, blk_count %d, max_n %lld, max_m "
               "%lld, a_begin %lld)",
               blk_first, blk_count, (long long)max_n, (long long)max_m, (long long)a_begin);
  TW_ARG_CHECK(a_end > a_begin, "tw_triplet_rows: empty anchor range [%lld, %lld)",
               (long long)a_begin, (long long)a_end);
  if (max_n == 0) return TW_OK;  // no anchors in any block
  const int64_t pt_other = ceil_div(max_m, kTripP), pt_all = pt_other + ceil_div(max_n, kTripP);
  const int64_t gx = ceil_div(std::min(max_n, a_end - a_begin), kTripTA) * pt_all;
  TW_ARG_CHECK(gx < (1ll << 31) && blk_count <= 65535,
               "tw_triplet_rows: grid too large (%lld x %d workgroups)", (long long)gx, blk_count);
  hipLaunchKernelGGL(k_triplet_rows, dim3((unsigned)gx, (unsigned)blk_count), dim3(kBlock), 0,
                     (hipStream_t)stream, d_x, d_z, (int)d, d_blk_x_off, d_blk_z_off,
                     (int)blk_first, a_begin, a_end, (int)pt_other, (int)pt_all, d_other_off,
                     d_own_off, d_other, d_own);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int64_t tw_triplet_idx_work_bytes(int32_t n_shards, int64_t max_triplets) {
  if (n_shards < 0 || max_triplets < 0) return 0;
  return std::max<int64_t>(8, trip_idx_blocks_per_shard(max_triplets) * n_shards * 8);
}

extern "C" int tw_triplet_idx32(const double* d_x, const double* d_z, int32_t d,
                                const int32_t* d_i, const int32_t* d_j, const int32_t* d_k,
                                const int64_t* d_trip_off, int32_t n_shards,
                                int64_t max_triplets, int32_t pred, void* d_work, uint64_t* d_out,
                                void* stream) {
  TW_ARG_CHECK(d_x && d_z && d_i && d_j && d_k && d_trip_off && d_work && d_out,
               "tw_triplet_idx32: null pointer");
  TW_ARG_CHECK(d >= 1 && d <= kTripMaxD, "tw_triplet_idx32: d %d outside [1, %d]", d, kTripMaxD);
  TW_ARG_CHECK(n_shards >= 0, "tw_triplet_idx32: n_shards %d < 0", n_shards);
  TW_ARG_CHECK(max_triplets >= 0, "tw_triplet_idx32: max_triplets %lld < 0",
               (long long)max_triplets);
  TW_ARG_CHECK(pred == TW_PRED_GT || pred == TW_PRED_HALF,
               "tw_triplet_idx32: predicate %d (TW_PRED_GT or TW_PRED_HALF)", pred);
  if (n_shards == 0) return TW_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = trip_idx_blocks_per_shard(max_triplets);
  TW_ARG_CHECK(per * n_shards < (1ll << 31), "tw_triplet_idx32: grid too large");
  auto* w = (unsigned long long*)d_work;
  const dim3 g((unsigned)(per * n_shards)), b(kBlock);
  if (pred == TW_PRED_HALF)
    hipLaunchKernelGGL(k_triplet_idx<TW_PRED_HALF>, g, b, 0, st, d_x, d_z, (int)d, d_i, d_j, d_k,
                       d_trip_off, (int)per, w);
  else
    hipLaunchKernelGGL(k_triplet_idx<TW_PRED_GT>, g, b, 0, st, d_x, d_z, (int)d, d_i, d_j, d_k,
                       d_trip_off, (int)per, w);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_self_reduce<unsigned long long, 1>), dim3(n_shards), dim3(kBlock), 0, st,
                     (const unsigned long long*)w, (int)per, (unsigned long long*)d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
