// bitcount.h — the bit-sliced compare-and-count of rank images (csrc/chain.hip's
// k_count_chain_planes and its class-run forms), beside pkcount.h's packed-f32
// form.
//
// Images are integers in [0, bound], bound < 2^NB <= 2^24.  A lane keeps 32 x images as NB bit
// PLANES (plane b: bit k = bit b of image k), and the unsigned compare x > z is the carry out of
// x + ~z over NB bits.  With z wave-uniform, ~z's bit b is a 0 / ~0 mask in an SGPR (one
// s_bfe_i32) and the carry of 32 pairs advances by one three-input bit operation per bit:
//     c = plane[0] & mask[0]                               v_and_b32
//     c = majority(plane[b], mask[b], c)   b = 1 .. NB-1   v_bitop3_b32 (table 0xE8)
//     acc += popcount(c)                                   v_bcnt_u32_b32
// = NB + 1 VALU wave-instructions per 64 * 32 pairs, against 1 per 64 for the packed form.
//
// The helpers are plain C++ (host and device), so tests/native/bitcount_driver.cpp checks the
// logic without a GPU; the wave item itself (device only) is at the end.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TW_BITS_HD __host__ __device__ __forceinline__
#else
#define TW_BITS_HD inline
#endif

namespace tw {

// The instantiated plane counts: the least of them that holds image_bound; 0 if none does.
TW_BITS_HD int bits_pick_nb(int64_t image_bound) {
  if (image_bound < 0) return 0;
  for (int nb = 16; nb <= 24; nb += 2)
    if (image_bound < ((int64_t)1 << nb)) return nb;
  return 0;
}

// An x image as an integer: the float image is integer-valued in [0, 2^24); NaN and the
// "never" image (-2^25, pkcount.h's kImgNever) become 0, which is greater than no z image.
TW_BITS_HD uint32_t bits_x_image(float gx) {
  return gx > 0.0f ? (uint32_t)gx : 0u;
}
// A z image (stored negated, -g(z)) complemented, so that its bits are the carry chain's masks.
TW_BITS_HD uint32_t bits_z_image(float ngz) {
  return ~(ngz < 0.0f ? (uint32_t)(-ngz) : 0u);
}
// The complemented z image greater than or equal to every x image: padded z slots count nothing.
constexpr uint32_t kBitsZNever = 0u;

// (a) 32 x 32 bit transpose in place, the log-step swap network (5 stages of 16 swaps):
// afterwards bit k of a[b] is bit b of the former a[k].  With images in a[], a[b] is plane b.
TW_BITS_HD void bits_transpose32(uint32_t (&a)[32]) {
  uint32_t m = 0x0000FFFFu;
#pragma unroll
  for (int s = 16; s > 0; s >>= 1) {
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      if (k & s) continue;
      const uint32_t t = ((a[k] >> s) ^ a[k + s]) & m;
      a[k + s] ^= t;
      a[k] ^= t << s;
    }
    m ^= m << (s >> 1);
  }
}

// ~z's bit b as a 0 / ~0 mask (zc: the complemented z image, wave-uniform: s_bfe_i32)
TW_BITS_HD uint32_t bits_mask(uint32_t zc, int b) {
  return (uint32_t)((int32_t)(zc << (31 - b)) >> 31);
}

// (b) the carry step: majority(plane, mask, c)
TW_BITS_HD uint32_t bits_carry(uint32_t plane, uint32_t mask, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(plane, mask, c, 0xE8);
#else
  return (plane & mask) | (plane & c) | (mask & c);
#endif
}

// (c) the popcount accumulate (u32: at most 32 per z, chunks of < 2^24 z)
TW_BITS_HD uint32_t bits_popc_add(uint32_t c, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (asm: left to itself the compiler counts into a fresh register and adds two z at a time
  // with v_add3_u32, 3 instructions per 2 counts)
  asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(c));
  return acc;
#else
  uint32_t n = 0;
  for (uint32_t v = c; v; v &= v - 1) ++n;
  return acc + n;
#endif
}

// [x_k > z] for the 32 images of NB planes against one complemented z image
template <int NB>
TW_BITS_HD uint32_t bits_gt32(const uint32_t (&plane)[NB], uint32_t zc) {
  uint32_t c = plane[0] & bits_mask(zc, 0);
#pragma unroll
  for (int b = 1; b < NB; ++b) c = bits_carry(plane[b], bits_mask(zc, b), c);
  return c;
}

#if defined(__HIPCC__)
// a wave-uniform offset held in VGPRs (the item's division) moved to SGPRs: loads then take
// the scalar base + 32-bit lane offset form, one address VGPR each instead of two
__device__ __forceinline__ int64_t bits_uniform(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The scalar-side loop of a wave item: n wave-uniform images against the lane's R groups of NB
// planes.  load(j) gives lane l the image j + l, complemented z or plain x (0 past the end); the
// images go 64 at a time through one VGPR, the next 64 in flight, and reach the scalar side by
// v_readlane_b32: one extra VALU instruction per image and wave.
template <int NB, int R, class Load>
__device__ __forceinline__ void bits_scalar_loop(const uint32_t (&pl)[R][NB], uint32_t (&acc)[R],
                                                 int n, Load load) {
  uint32_t next = load(0);
  for (int j = 0; j < n; j += 64) {
    const uint32_t sv = next;
    next = load(j + 64);
    const int cnt = min(64, n - j);
    for (int l = 0; l < cnt; l += 2) {  // an odd last image pairs with a padded slot: 0
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t sc = (uint32_t)__builtin_amdgcn_readlane((int)sv, l + u);
        uint32_t m[NB], c[R];
#pragma unroll
        for (int b = 0; b < NB; ++b) m[b] = bits_mask(sc, b);
#pragma unroll
        for (int r = 0; r < R; ++r) c[r] = pl[r][0] & m[0];
#pragma unroll
        for (int b = 1; b < NB; ++b)
#pragma unroll
          for (int r = 0; r < R; ++r) c[r] = bits_carry(pl[r][b], m[b], c[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = bits_popc_add(c[r], acc[r]);
      }
    }
  }
}

// One wave item on planes built beforehand (chainplan.h; chain.hip's k_chain_planes): R groups
// of NB plane words per lane at pw (group r, plane b: pw[(r * NB + b) * 64 + lane]) against
// the ns scalar-side images at sf — a z chunk (stored negated; complemented here), or, with
// the roles SWAPPED, x images against complemented z planes: the carry out of x + ~z does not
// care which operand is the lane's.  The scalar loop is bits_scalar_loop; padded scalar
// slots hold 0 in either role (a complemented z that is never less, an x that is never more).
template <int NB, int R>
__device__ __forceinline__ unsigned long long bits_count_planes(const uint32_t* __restrict__ pw,
                                                                const float* __restrict__ sf,
                                                                int ns, bool swapped, int lane) {
  uint32_t pl[R][NB], acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int b = 0; b < NB; ++b) pl[r][b] = pw[(r * NB + b) * 64 + lane];
    acc[r] = 0;
  }
  auto s_load = [&](int j) -> uint32_t {
    const float f = sf[min(j + lane, ns - 1)];  // (no branch around the load)
    const uint32_t v = swapped ? bits_x_image(f) : bits_z_image(f);
    return j + lane < ns ? v : 0u;
  };
  bits_scalar_loop<NB, R>(pl, acc, ns, s_load);
  unsigned long long tot = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) tot += acc[r];
  return tot;
}
#endif  // __HIPCC__

}  // namespace tw
