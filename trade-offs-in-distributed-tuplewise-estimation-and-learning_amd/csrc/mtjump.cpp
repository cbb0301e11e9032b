// mtjump.cpp — MT19937 jump-ahead on the host, host code.
//
// The raw (untempered) MT19937 word sequence x[k] (Matsumoto & Nishimura 1998:
// x[k+624] = x[k+397] ^ twist(upper(x[k]), lower(x[k+1]))) is linear over GF(2), and every bit
// of it obeys one linear recurrence whose characteristic polynomial phi(t) has degree 19937
// (primitive, so any non-zero bit sequence has phi as its minimal polynomial).  With
// g(t) = t^J mod phi(t) the sequence J words ahead is the GF(2) convolution
//     x[J + j] = XOR_{i : g_i = 1} x[i + j]                       (Haramoto et al. 2008),
// which advances a state by any J in O(19937 * 624) word operations.  Here: phi by
// Berlekamp-Massey on 2 * 19937 bits of one output bit, t^J by square-and-multiply on
// bit-packed polynomials (312 64-bit words), and the jump of a NumPy (key[624], pos) state
// (np.random.get_state()) — the starting states of csrc/mtdraw.hip's device sub-streams.
//
// The word-0 trap: the MT19937 state is the top bit of word 0 and words 1..623; the low 31
// bits of word 0 obey no recurrence (after seed() they are not sequence values, and the twist
// never reads them), but NumPy's key[0] after any regeneration is the true sequence word.  So
// a window is never taken at the target offset M itself: the convolution runs at M - 1, which
// holds x[M .. M+622] whole and the top bit of x[M-1], and one recurrence step makes x[M+623].
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/tuplewise.h"

namespace {

constexpr int kN = 624, kM = 397;
constexpr int kDeg = 19937;          // degree of phi
constexpr int kPW = 312;             // 64-bit words of a polynomial (19968 bits: phi fits whole)
constexpr int kSeq = kDeg + kN - 1;  // raw words x[0 .. 19936 + 623] a window's convolution reads
constexpr uint32_t kMatrixA = 0x9908b0dfu, kUpper = 0x80000000u, kLower = 0x7fffffffu;

inline uint32_t twist(uint32_t a, uint32_t b, uint32_t src) {
  const uint32_t y = (a & kUpper) | (b & kLower);
  return src ^ (y >> 1) ^ ((0u - (y & 1u)) & kMatrixA);
}

// x[0, n): x[0..623] = key, then the recurrence (x[0]'s low 31 bits are never read)
void raw_sequence(const uint32_t* key, uint32_t* x, int n) {
  memcpy(x, key, sizeof(uint32_t) * kN);
  for (int k = kN; k < n; ++k) x[k] = twist(x[k - kN], x[k - kN + 1], x[k - kN + kM]);
}

// Berlekamp-Massey over GF(2), bit-packed, on s[0, n) (bit k of s = s_k).  Returns the linear
// complexity L and the connection polynomial C (c_0 = 1; s_k = XOR_{i=1..L} c_i s_{k-i}).
int berlekamp_massey(const std::vector<uint64_t>& s, int n, std::vector<uint64_t>& C) {
  const int W = n / 64 + 3;
  // R holds s reversed (bit n-1-k = s_k): the discrepancy XOR_i c_i s_{k-i} is then the parity
  // of C AND (R >> (n-1-k)), 64 coefficients a step
  std::vector<uint64_t> R(W + 2, 0), B(W, 0), T(W, 0);
  for (int k = 0; k < n; ++k)
    if (s[k >> 6] >> (k & 63) & 1) R[(n - 1 - k) >> 6] |= 1ull << ((n - 1 - k) & 63);
  C.assign(W, 0);
  C[0] = B[0] = 1;
  int L = 0, m = 1;
  for (int k = 0; k < n; ++k) {
    const int off = n - 1 - k, q = off >> 6, sh = off & 63;
    uint64_t acc = 0;
    for (int w = 0; w <= L >> 6; ++w) {
      const uint64_t r = sh ? (R[q + w] >> sh) | (R[q + w + 1] << (64 - sh)) : R[q + w];
      acc ^= C[w] & r;
    }
    if (!(__builtin_popcountll(acc) & 1)) {
      ++m;
      continue;
    }
    const bool grow = 2 * L <= k;
    if (grow) T = C;
    const int ws = m >> 6, bs = m & 63;  // C ^= B << m
    for (int w = 0; w + ws < W; ++w) {
      C[w + ws] ^= B[w] << bs;
      if (bs && w + ws + 1 < W) C[w + ws + 1] ^= B[w] >> (64 - bs);
    }
    if (grow) {
      L = k + 1 - L;
      B.swap(T);
      m = 1;
    } else {
      ++m;
    }
  }
  return L;
}

struct Phi {
  uint64_t w[kPW];
  bool ok;
};

// phi(t), computed once per process: bit 0 of x[1 .. 2*19937] of a fixed non-zero state
const Phi& phi() {
  static const Phi p = [] {
    Phi r;
    memset(&r, 0, sizeof r);
    const int n = 2 * kDeg;
    std::vector<uint32_t> x(n + 1);
    uint32_t key[kN];
    key[0] = 19650218u;  // init_genrand's recurrence: any non-zero state serves
    for (int i = 1; i < kN; ++i) key[i] = 1812433253u * (key[i - 1] ^ (key[i - 1] >> 30)) + (uint32_t)i;
    raw_sequence(key, x.data(), n + 1);
    std::vector<uint64_t> s((n + 63) / 64, 0), C;
    for (int k = 0; k < n; ++k)
      if (x[k + 1] & 1u) s[k >> 6] |= 1ull << (k & 63);
    const int L = berlekamp_massey(s, n, C);
    r.ok = L == kDeg;
    if (r.ok)  // characteristic polynomial: phi_k = c_{L-k}
      for (int k = 0; k <= kDeg; ++k)
        if (C[(kDeg - k) >> 6] >> ((kDeg - k) & 63) & 1) r.w[k >> 6] |= 1ull << (k & 63);
    return r;
  }();
  return p;
}

inline bool reduced(const uint64_t* a) { return (a[kPW - 1] >> (kDeg & 63)) == 0; }

// out = a * b mod phi (a, b of degree < 19937; out may alias either)
void mulmod(const uint64_t* a, const uint64_t* b, uint64_t* out) {
  const uint64_t* ph = phi().w;
  uint64_t prod[2 * kPW + 1];
  memset(prod, 0, sizeof prod);
  for (int wa = 0; wa < kPW; ++wa) {
    uint64_t bits = a[wa];
    while (bits) {
      const int sh = __builtin_ctzll(bits);
      bits &= bits - 1;
      uint64_t* p = prod + wa;
      if (sh == 0) {
        for (int w = 0; w < kPW; ++w) p[w] ^= b[w];
      } else {
        uint64_t carry = 0;
        for (int w = 0; w < kPW; ++w) {
          p[w] ^= (b[w] << sh) | carry;
          carry = b[w] >> (64 - sh);
        }
        p[kPW] ^= carry;
      }
    }
  }
  for (int bit = 2 * (kDeg - 1); bit >= kDeg; --bit) {
    if (!(prod[bit >> 6] >> (bit & 63) & 1)) continue;
    const int d = bit - kDeg, ws = d >> 6, sh = d & 63;  // prod ^= phi << d
    uint64_t* p = prod + ws;
    if (sh == 0) {
      for (int w = 0; w < kPW; ++w) p[w] ^= ph[w];
    } else {
      uint64_t carry = 0;
      for (int w = 0; w < kPW; ++w) {
        p[w] ^= (ph[w] << sh) | carry;
        carry = ph[w] >> (64 - sh);
      }
      p[kPW] ^= carry;
    }
  }
  memcpy(out, prod, sizeof(uint64_t) * kPW);
}

// out = t^J mod phi, left-to-right square-and-multiply (the multiply by t is a shift)
void power(int64_t J, uint64_t* out) {
  const uint64_t* ph = phi().w;
  memset(out, 0, sizeof(uint64_t) * kPW);
  out[0] = 1;
  if (J == 0) return;
  for (int b = 63 - __builtin_clzll((uint64_t)J); b >= 0; --b) {
    mulmod(out, out, out);
    if (J >> b & 1) {
      uint64_t carry = 0;
      for (int w = 0; w < kPW; ++w) {
        const uint64_t nc = out[w] >> 63;
        out[w] = (out[w] << 1) | carry;
        carry = nc;
      }
      if (out[kPW - 1] >> (kDeg & 63) & 1)
        for (int w = 0; w < kPW; ++w) out[w] ^= ph[w];
    }
  }
}

// y[j] = XOR_{i : g_i = 1} x[i + j], j in [0, 624), over x[0, kSeq)
void convolve(const uint32_t* x, const uint64_t* g, uint32_t* y) {
  memset(y, 0, sizeof(uint32_t) * kN);
  for (int w = 0; w < kPW; ++w) {
    uint64_t bits = g[w];
    while (bits) {
      const uint32_t* s = x + w * 64 + __builtin_ctzll(bits);
      bits &= bits - 1;
      for (int j = 0; j < kN; ++j) y[j] ^= s[j];
    }
  }
}

}  // namespace

extern "C" {

// phi(t) into out[312] (bit k of the packed words = the coefficient of t^k; bit 19937 is set).
// Returns 0, or 2 if Berlekamp-Massey did not find degree 19937 (never, for MT19937).
int tw_mt_minpoly(uint64_t* out) {
  if (!out) return 1;
  const Phi& p = phi();
  if (!p.ok) return 2;
  memcpy(out, p.w, sizeof p.w);
  return 0;
}

// t^J mod phi into out[312], J >= 0.
int tw_mt_jump_poly(int64_t J, uint64_t* out) {
  if (!out || J < 0) return 1;
  if (!phi().ok) return 2;
  power(J, out);
  return 0;
}

// out = a * b mod phi for reduced a, b (degree < 19937); out may alias a or b.
int tw_mt_poly_mulmod(const uint64_t* a, const uint64_t* b, uint64_t* out) {
  if (!a || !b || !out || !reduced(a) || !reduced(b)) return 1;
  if (!phi().ok) return 2;
  mulmod(a, b, out);
  return 0;
}

// Advance a NumPy MT19937 state (key[624], pos in [0, 624]) by exactly J >= 0 words: the state
// J genrand_int32 calls would leave, in NumPy's representation (regeneration is lazy: after
// J >= 1 words pos ends in [1, 624], so a jump by a multiple of 624 keeps pos).  A target in the
// current key block only moves pos; any other is the window at M - 1 (M = the target block's
// first word) plus one recurrence step — see the word-0 trap above.
int tw_mt_jump_host(uint32_t* key, int32_t* pos, int64_t J) {
  if (!key || !pos || J < 0 || *pos < 0 || *pos > kN || J > (1ll << 62)) return 1;
  if (J == 0) return 0;
  const int64_t P = (int64_t)*pos + J, b = (P - 1) / kN;
  if (b > 0) {
    if (!phi().ok) return 2;
    std::vector<uint64_t> g(kPW);
    power(b * kN - 1, g.data());
    std::vector<uint32_t> x(kSeq);
    raw_sequence(key, x.data(), kSeq);
    uint32_t y[kN];
    convolve(x.data(), g.data(), y);  // y[j] = x[M - 1 + j]; y[0]: top bit only
    memcpy(key, y + 1, sizeof(uint32_t) * (kN - 1));
    key[kN - 1] = twist(y[0], y[1], y[kM]);
  }
  *pos = (int32_t)(P - b * kN);
  return 0;
}

}  // extern "C"
