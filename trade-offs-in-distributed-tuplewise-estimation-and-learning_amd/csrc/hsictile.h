// hsictile.h — the step of hsic.hip that hsic_perm.hip shares: kHsicTA
// anchors a wave staged in LDS, one side's squared distances of a lane's two points to them, and
// the mask of a pair, so that a K_ij has the same bits in both files.
#pragma once
#include "tw_common.h"
#include "tripdist.h"
#include "mmdtile.h"

namespace tw {

constexpr int kHsicTA = 8;                              // anchors per wave and step: two sides'
                                                        // accumulators beside each other in VGPRs
constexpr int kHsicSA = (kBlock / kWave) * kHsicTA;     // anchors staged per step, both sides
static_assert(kMmdT % kHsicSA == 0, "a tile is a whole number of anchor steps");

// The step's anchors: up to kHsicSA rows of d doubles from `src`, row stride kTripMaxD in LDS,
// zeros past the tile's end (`left` anchors remain).
__device__ __forceinline__ void hsic_stage(double* __restrict__ sa, const double* __restrict__ src,
                                           int d, int left) {
  for (int q = threadIdx.x; q < kHsicSA * d; q += kBlock) {
    const int a = q / d, cc = q - a * d;
    sa[a * kTripMaxD + cc] = a < left ? src[q] : 0.0;
  }
}

// acc += the squared distances of this lane's points (coordinates [0, 8) already in pc) to the
// wave's anchors: k_mmd_sums' chunk loop, the next chunk's loads issued before this chunk's
// arithmetic.
__device__ __forceinline__ void hsic_side(const double* __restrict__ const (&row)[kTripR], int d,
                                          const double* __restrict__ swave,
                                          double (&pc)[kTripR][kTripDC],
                                          double (&acc)[kHsicTA][kTripR]) {
  const int n_full = d / kTripDC;
  const bool tail = n_full * kTripDC < d;
  for (int ch = 0; ch < n_full; ++ch) {
    double pn[kTripR][kTripDC];
    const int c1 = (ch + 1) * kTripDC;
    if (ch + 1 < n_full) mmd_load<false>(row, c1, d, pn);
    else if (tail) mmd_load<true>(row, c1, d, pn);
    trip_chunk<false, kHsicTA>(swave, ch * kTripDC, d, pc, acc);
#pragma unroll
    for (int r = 0; r < kTripR; ++r)
#pragma unroll
      for (int cc = 0; cc < kTripDC; ++cc) pc[r][cc] = pn[r][cc];
  }
  if (tail) trip_chunk<true, kHsicTA>(swave, n_full * kTripDC, d, pc, acc);
}

// The fold, one side at a time so that only one side's distances are live beside the other's g
// values.  MASK: anchors past the tile's end, points past the end and, on a diagonal tile,
// anchor <= point add nothing anywhere (selects, so a NaN of a masked pair does not enter).
// diag_shift: 0 on a diagonal tile (anchor index above the point's), else past every point.
template <bool MASK>
__device__ __forceinline__ bool hsic_ok(int a, int r, int a_first, int na, int diag_shift, int lane,
                                        const bool (&valid)[kTripR]) {
  return !MASK || (valid[r] && a_first + a < na && a_first + a + diag_shift > r * kWave + lane);
}

}  // namespace tw
