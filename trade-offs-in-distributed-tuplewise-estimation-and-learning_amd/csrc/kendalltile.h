// kendalltile.h — the sign fragments that kendall.hip and kendall_rows.hip share (DESIGN.md
// §4.18, §4.19): the element types of the two rank widths, and the 16 sign bytes of one anchor
// against a lane's 16 points as an operand of v_mfma_i32_16x16x64_i8, so that a sign is built by
// the same instructions in both files.
#pragma once
#include "tw_common.h"

namespace tw {

constexpr int kKmT = 64;         // rows per tile edge (4 waves x 16 points)

typedef int v4i __attribute__((ext_vector_type(4)));

template <int W>
struct KmTy;
template <>
struct KmTy<16> {
  using R = uint16_t;
  static constexpr int kStride = kKmT + 8;  // ranks per staged column: 144 bytes
  static constexpr int kPR = 8;             // registers of a lane's 16 point ranks
  static constexpr int kAP = 8;             // anchors per 16-byte LDS read
};
template <>
struct KmTy<32> {
  using R = int32_t;
  static constexpr int kStride = kKmT + 4;  // 272 bytes
  static constexpr int kPR = 16;
  static constexpr int kAP = 4;
};

// Two int16 signs: clamp(anchor - point) limited to [-1, 1]; the anchor is the low (HI false)
// or the high half of `anc` for both halves of the result.
template <bool HI>
__device__ __forceinline__ uint32_t km_sign16(uint32_t anc, uint32_t pt, uint32_t m1, uint32_t p1) {
  uint32_t d;
  if constexpr (HI)
    asm("v_pk_sub_i16 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] clamp" : "=v"(d) : "v"(anc), "v"(pt));
  else
    asm("v_pk_sub_i16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] clamp" : "=v"(d) : "v"(anc), "v"(pt));
  asm("v_pk_max_i16 %0, %1, %2" : "=v"(d) : "v"(d), "v"(m1));
  asm("v_pk_min_i16 %0, %1, %2" : "=v"(d) : "v"(d), "v"(p1));
  return d;
}

// The 16 sign bytes of one anchor (number tt of the 16 bytes `an` read from LDS) against a
// lane's 16 points: byte q of word w is point 4 w + q.
template <int W, int TT>
__device__ __forceinline__ v4i km_frag(const uint32_t (&an)[4], const uint32_t (&pts)[KmTy<W>::kPR],
                                       uint32_t m1, uint32_t p1) {
  v4i f;
  if constexpr (W == 16) {
    uint32_t d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = km_sign16<(TT & 1) != 0>(an[TT >> 1], pts[k], m1, p1);
#pragma unroll
    for (int w = 0; w < 4; ++w) f[w] = (int)__builtin_amdgcn_perm(d[2 * w + 1], d[2 * w], 0x06040200u);
  } else {
    const int a = (int)an[TT];
    int m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      // ranks are below 2^31: the difference cannot wrap.  (The plain min / max form is
      // compiled into two compares and two selects a sign.)
      const uint32_t d = (uint32_t)a - pts[k];
      asm("v_med3_i32 %0, %1, -1, 1" : "=v"(m[k]) : "v"(d));
    }
#pragma unroll
    for (int w = 0; w < 4; ++w)
      f[w] = (int)(__builtin_amdgcn_perm((uint32_t)m[4 * w + 1], (uint32_t)m[4 * w], 0x0c0c0400u) |
                   __builtin_amdgcn_perm((uint32_t)m[4 * w + 3], (uint32_t)m[4 * w + 2], 0x04000c0cu));
  }
  return f;
}

}  // namespace tw
