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

// The anchor side's cross-lane sums (hsic.hip, mmd_rows.hip).
static_assert(kHsicTA == 8 && kTripR == 2 && kWave == 64, "hsic_anchor_sums' butterfly");

// v of lane (l ^ O) by a DPP lane move.
template <int O>
__device__ __forceinline__ double hsic_lane_xor(double v) {
  static_assert(O == 1 || O == 2 || O == 8, "a DPP pattern");
  if constexpr (O == 1) return dpp_f64<0xB1>(v);        // quad_perm [1,0,3,2]
  else if constexpr (O == 2) return dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  else return dpp_f64<0x128>(v);                        // row_ror:8
}

// One level of the reduce-scatter: lanes whose bit O is clear keep the lower half of the 2 N
// values, the others the upper half, and each adds what its partner (lane ^ O) holds of them.
template <int O, int N>
__device__ __forceinline__ void hsic_halve(double (&v)[kHsicTA], bool up) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double keep = up ? v[i + N] : v[i], send = up ? v[i] : v[i + N];
    v[i] = keep + hsic_lane_xor<O>(send);
  }
}

// v[a] = this lane's two points' terms of anchor a.  Returns, in every lane, the sum over the
// wave's 128 points for anchor hsic_anchor_of(lane): 8 -> 4 -> 2 -> 1 values a lane over lane
// bits 0, 1, 3 (DPP moves), then the lanes that hold the same anchor are added over bits 2, 4, 5.
// A fixed order.
__device__ __forceinline__ double hsic_anchor_sums(double (&v)[kHsicTA], int lane) {
  hsic_halve<1, 4>(v, lane & 1);
  hsic_halve<2, 2>(v, lane & 2);
  hsic_halve<8, 1>(v, lane & 8);
  double s = v[0];
  s += __shfl_xor(s, 4, kWave);
  s += __shfl_xor(s, 16, kWave);
  s += __shfl_xor(s, 32, kWave);
  return s;
}
__device__ __forceinline__ int hsic_anchor_of(int lane) {
  return ((lane & 1) << 2) | (lane & 2) | ((lane & 8) >> 3);
}
__device__ __forceinline__ bool hsic_anchor_lane(int lane) { return (lane & ~0xB) == 0; }

}  // namespace tw
