// mmdtile.h — the tile constants, the pair function and the row loads that mmd.hip, mmd_perm.hip
// and hsic.hip share, so that a g has the same bits in all of them.
#pragma once
#include "tw_common.h"
#include "tripdist.h"
#include <cmath>

namespace tw {

constexpr int kMmdT = kWave * kTripR;                   // rows per tile edge (points of a lane: r * 64 + lane)
constexpr int kMmdSA = (kBlock / kWave) * kTripTA;      // anchors staged per step, kTripTA a wave
static_assert(kMmdT % kMmdSA == 0, "a tile is a whole number of anchor steps");

template <int K>
__device__ __forceinline__ double mmd_g(double dist, double c) {
  if constexpr (K == TW_MMD_GAUSSIAN) return exp(c * dist);
  else return sqrt(dist);
}

// Coordinates [c0, c0 + kTripDC) of this lane's points.  TAIL: the chunk runs past d (zeros there).
template <bool TAIL>
__device__ __forceinline__ void mmd_load(const double* __restrict__ const (&row)[kTripR], int c0,
                                         int d, double (&pc)[kTripR][kTripDC]) {
#pragma unroll
  for (int r = 0; r < kTripR; ++r)
#pragma unroll
    for (int cc = 0; cc < kTripDC; ++cc)
      pc[r][cc] = (!TAIL || c0 + cc < d) ? row[r][c0 + cc] : 0.0;
}

}  // namespace tw

#define TW_MMD_KERN_CHECKS(fn)                                                                  \
  TW_ARG_CHECK(d >= 1 && d <= kTripMaxD, fn ": d %d outside [1, %d]", d, kTripMaxD);            \
  TW_ARG_CHECK(kern == TW_MMD_GAUSSIAN || kern == TW_MMD_ENERGY, fn ": unknown kernel %d", kern); \
  TW_ARG_CHECK(kern != TW_MMD_GAUSSIAN || (std::isfinite(c) && c <= 0.0),                       \
               fn ": c = %g for the Gaussian kernel (finite and <= 0: -1 / (2 sigma^2))", c)
