// tripdist.h — the squared Euclidean distance of the triplet and MMD kernels (triplets.hip,
// mmd.hip; include/tuplewise.h states the contract) in its ONE arithmetic order, multiply and add
// separate (the build has -ffp-contract=off):
//   acc = 0.0; for c in 0..d-1: t = a_c - b_c; acc = acc + t * t
// trip_chunk is the register micro-tile (anchors broadcast from LDS, a lane's points in
// registers), trip_dist one pair of rows in global memory.  Both kernels share these functions,
// so a distance has the same bits wherever it is computed.
#pragma once
#include "tw_common.h"

namespace tw {

constexpr int kTripMaxD = 64;                 // coordinates per row, at most
constexpr int kTripTA = 16;                   // anchors per tile (feature rows staged in LDS)
constexpr int kTripR = 2;                     // points per lane
constexpr int kTripDC = 8;                    // coordinates of a lane's points held in registers

// One chunk of coordinates [c0, c0 + kTripDC) of this lane's points against every anchor of the
// tile: the anchor's coordinate is one wave-uniform LDS read (a broadcast), used for kTripR
// points.  TAIL: the chunk runs past d (block-uniform tests, no lane diverges).  TA: the anchors
// of the micro-tile (kTripTA everywhere but hsic.hip, which holds two sides' accumulators).
template <bool TAIL, int TA = kTripTA>
__device__ __forceinline__ void trip_chunk(const double* __restrict__ sa, int c0, int d,
                                           const double (&pc)[kTripR][kTripDC],
                                           double (&acc)[TA][kTripR]) {
#pragma unroll
  for (int a = 0; a < TA; ++a) {
#pragma unroll
    for (int c = 0; c < kTripDC; ++c) {
      if (!TAIL || c0 + c < d) {
        const double s = sa[a * kTripMaxD + c0 + c];
#pragma unroll
        for (int r = 0; r < kTripR; ++r) {
          const double t = s - pc[r][c];
          acc[a][r] = acc[a][r] + t * t;
        }
      }
    }
  }
}

// D(a, b) over d coordinates in the contract's order.
__device__ __forceinline__ double trip_dist(const double* __restrict__ a,
                                            const double* __restrict__ b, int d) {
  double acc = 0.0;
#pragma unroll 4
  for (int c = 0; c < d; ++c) {
    const double t = a[c] - b[c];
    acc = acc + t * t;
  }
  return acc;
}

}  // namespace tw
