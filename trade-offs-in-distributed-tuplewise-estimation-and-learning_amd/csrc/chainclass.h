// chainclass.h — the class-run form of the plane-reading chain count (csrc/chain.hip's
// k_chain_zclasses + k_count_chain_classes), beside chainplan.h's items.
//
// With zc the complemented z image, x > z is the carry out of x + zc over NB bits (bitcount.h).
// Split the bits into the low bits [0, NB - k) and a TOP FIELD [NB - k, NB), and let D be the
// top field of zc — the z image's CLASS.  For a carry c into the top field the carry out is
//     G | (P & c),   G = the top field's own chain with carry-in 0    (x_top >  z_top)
//                    P = the same chain with carry-in all-ones         (x_top >= z_top)
// and G is a subset of P, so that is majority(G, P, c): one bits_carry with three VGPR sources.
// G and P depend on the x planes and D alone.  The scalar-side z of a bag are therefore grouped
// by class once per launch (a counting sort into a class-ordered region of the workspace) and
// an item compares its x groups against a RUN of z of one class: G and P once per item and
// group (2 k instructions), then (NB - k) + 1 + 1 per z and group instead of NB + 1.  Every
// pair still gets its own low-bit chain and its own popcount bit; only the subexpression
// common to a class is hoisted.
//
// Two properties the count depends on (tests/native/chainclass_driver.cpp checks both):
//  * a padded x slot (plane words 0) counts nothing: its low carry is 0 and its G is 0;
//  * a padded SCALAR slot is NOT harmless here — complemented 0 leaves c = 0 but counts G — so
//    the class loop takes exactly the run's images and never evaluates a slot past its end.
//
// The class-constant term.  G is a subset of P, so with E = P & ~G — the x whose
// top field EQUALS the class —
//     popc(G | (P & c)) = popc(G) + popc(E & c):
// popc(G) is the same for every z of a run and is counted once per item as len * popc(G), with
// len the run's exact length.  E & c needs no instruction of its own: a slot whose low planes
// are all 0 never carries from carry-in 0, so the low chain on the planes ANDed with E once per
// item yields exactly E & c.  Per z and group the lane side is then NL + 1 (the chain and one
// popcount).  Every pair still runs through its own low-bit chain.
//
// Everything here is plain C++ (host and device).
#pragma once
#include <stdint.h>

#include "bitcount.h"
#include "chainplan.h"

namespace tw {

constexpr int kClassMaxBits = 8;        // class bits k: 1 .. min(8, NB - 8)
constexpr int64_t kClassMinChunk = 8;   // shortest run length a plan may ask for

// The class of a complemented z image: the top k of its low nb bits
TW_BITS_HD uint32_t class_of(uint32_t zc, int nb, int k) {
  return (zc >> (nb - k)) & ((1u << k) - 1u);
}

// G and P of one x group against class D: top[b] is plane NB - K + b
template <int K>
TW_BITS_HD void class_gp(const uint32_t (&top)[K], uint32_t D, uint32_t& G, uint32_t& P) {
  const uint32_t m0 = bits_mask(D, 0);
  G = top[0] & m0;  // carry-in 0
  P = top[0] | m0;  // carry-in all-ones
#pragma unroll
  for (int b = 1; b < K; ++b) {
    const uint32_t m = bits_mask(D, b);
    G = bits_carry(top[b], m, G);
    P = bits_carry(top[b], m, P);
  }
}

// [x_k > z] for the 32 images of a group from its NL low planes, G and P of z's class
template <int NL>
TW_BITS_HD uint32_t class_gt32(const uint32_t (&low)[NL], uint32_t G, uint32_t P, uint32_t zc) {
  return bits_carry(G, P, bits_gt32<NL>(low, zc));
}

// E: the x of a group whose top field equals the class (G subset of P)
TW_BITS_HD uint32_t class_equal_mask(uint32_t G, uint32_t P) { return P & ~G; }

// The low planes of a group ANDed with E, once per item and group
template <int NL>
TW_BITS_HD void class_mask_planes(const uint32_t (&low)[NL], uint32_t E, uint32_t (&masked)[NL]) {
#pragma unroll
  for (int b = 0; b < NL; ++b) masked[b] = low[b] & E;
}

// The masked form of class_gt32: popc(class_gt32(low, G, P, zc)) == popc(constant) + popc(word)
// with constant = G for every z of the class and word = E & c_low from the MASKED planes
struct ClassMasked {
  uint32_t constant, word;  // disjoint: G and a subset of E
};
template <int NL>
TW_BITS_HD ClassMasked class_gt32_masked(const uint32_t (&masked)[NL], uint32_t G, uint32_t zc) {
  return ClassMasked{G, bits_gt32<NL>(masked, zc)};
}

// ------------------------------------------------------------------------- the digit tables
// The low chain by table lookup.  The NL low planes are cut into kClassDigits
// DIGITS of at most kClassDigitBits planes, digit 0 the lowest.  For each of the 2^w values d a
// z image's digit can take, the carry through the digit is majority(G_d, P_d, c) with
//     G_d = the digit's own chain with carry-in 0,   P_d = the same chain with carry-in ones
// — class_gp's arithmetic on w planes — and G_d, P_d depend on the x planes and d alone: they
// are built once per item and group and the per-z chain is one step per DIGIT, its operands
// chosen by d.  G_d is the carry out of x_digit + d, so a carry-in of one is one more in d:
//     P_d = G_(d+1),   G_0 = 0,   G_(2^w) = ones,
// and one table of 2^w + 1 entries serves both: the step reads entries d and d + 1.  Digit 0 has
// carry-in 0: its step is c = G_d and it needs no entry 2^w.  The top digit's planes are ANDed
// with E and its entry 2^w is E, which makes its entries G_d & E: the chain yields E & c,
// class_gt32_masked's word.
constexpr int kClassDigits = 4;     // digits of the low field, whatever its width
constexpr int kClassDigitBits = 3;  // widest digit: tables of 2^3 (+ 1) entries
constexpr int kClassDigitMaxNL = kClassDigits * kClassDigitBits;
constexpr int kClassDigitEntries = (1 << kClassDigitBits) + 1;

// The split: NL / 4 planes each, the NL mod 4 lowest digits one more (12: 3,3,3,3; 11:
// 3,3,3,2; 10: 3,3,2,2; 9: 3,2,2,2; 8: 2,2,2,2)
constexpr int class_digit_width(int nl, int j) {
  return nl / kClassDigits + (j < nl % kClassDigits ? 1 : 0);
}
constexpr int class_digit_shift(int nl, int j) {
  int s = 0;
  for (int i = 0; i < j; ++i) s += class_digit_width(nl, i);
  return s;
}
// a low field the tables take: every digit has 1 .. kClassDigitBits planes
constexpr bool class_digits_fit(int nl) { return nl >= kClassDigits && nl <= kClassDigitMaxNL; }
// table entries (VGPRs per lane and group) the split uses: 2^w of digit 0, 2^w + 1 of the others
constexpr int class_digit_table_regs(int nl) {
  int n = 1 << class_digit_width(nl, 0);
  for (int j = 1; j < kClassDigits; ++j) n += (1 << class_digit_width(nl, j)) + 1;
  return n;
}

// The digit-ready form of a complemented z image (pre-pass 2 writes it under the digit loop):
// digit j in byte j, so that the loop's index instructions, which read bits [7:0] of a scalar,
// take digit 0 from the word itself and the others after one shift.  Every digit is masked to
// its width here and to kClassDigitBits bits in class_digit_of: no index leaves its table.
TW_BITS_HD uint32_t class_digit_encode(uint32_t zc, int nl) {
  uint32_t w = 0;
  for (int j = 0; j < kClassDigits; ++j)
    w |= ((zc >> class_digit_shift(nl, j)) & ((1u << class_digit_width(nl, j)) - 1u)) << (8 * j);
  return w;
}
TW_BITS_HD uint32_t class_digit_of(uint32_t word, int j) {
  return (word >> (8 * j)) & ((1u << kClassDigitBits) - 1u);
}

// G_d of one digit of W planes for d = 0 .. 2^W, with the planes ANDed with E and entry 2^W = E
// (lower digits: E = ~0; the top digit: the equal-top mask).  Built level by level: bit b of d
// is z's mask of plane b, so an entry of b + 1 planes is the entry of its low b bits ANDed
// (mask 0) or ORed (mask ones) with plane b — majority with a constant.  With old[0] = 0 and
// old[2^b] = E both rules give plane b at d = 2^b.
template <int W>
TW_BITS_HD void class_digit_table(const uint32_t (&plane)[W], uint32_t E,
                                  uint32_t (&G)[(1 << W) + 1]) {
  G[0] = 0u, G[1] = plane[0] & E, G[2] = E;
#pragma unroll
  for (int b = 1; b < W; ++b) {
    const uint32_t pb = plane[b] & E;
    G[2 << b] = E;
#pragma unroll
    for (int d = (1 << b) - 1; d >= 1; --d) {
      G[d + (1 << b)] = pb | G[d];
      G[d] = pb & G[d];
    }
    G[1 << b] = pb;
  }
}

// The tables of one x group: entry d of digit j at g[j][d], d = 0 .. 2^w; entries past that are
// 0 and never read
struct ClassDigitTables {
  uint32_t g[kClassDigits][kClassDigitEntries];
};
template <int NL, int J>
TW_BITS_HD void class_digit_tables_one(const uint32_t (&low)[NL], uint32_t E,
                                       ClassDigitTables& t) {
  constexpr int W = class_digit_width(NL, J), S = class_digit_shift(NL, J);
  uint32_t pl[W], G[(1 << W) + 1];
#pragma unroll
  for (int b = 0; b < W; ++b) pl[b] = low[S + b];
  class_digit_table<W>(pl, J == kClassDigits - 1 ? E : ~0u, G);
#pragma unroll
  for (int d = 0; d < kClassDigitEntries; ++d)
    t.g[J][d] = d <= (1 << W) ? G[d <= (1 << W) ? d : 0] : 0u;
}
// low: the group's UNMASKED low planes; E: class_equal_mask of its G and P
template <int NL>
TW_BITS_HD void class_digit_tables(const uint32_t (&low)[NL], uint32_t E, ClassDigitTables& t) {
  static_assert(class_digits_fit(NL), "low field too wide for the digit tables");
  class_digit_tables_one<NL, 0>(low, E, t);
  class_digit_tables_one<NL, 1>(low, E, t);
  class_digit_tables_one<NL, 2>(low, E, t);
  class_digit_tables_one<NL, 3>(low, E, t);
}

// class_gt32_masked by table lookup: word is a z image's digit-ready form (class_digit_encode)
TW_BITS_HD ClassMasked class_gt32_digits(const ClassDigitTables& t, uint32_t G, uint32_t word) {
  uint32_t c = t.g[0][class_digit_of(word, 0)];
  for (int j = 1; j < kClassDigits; ++j) {
    const uint32_t d = class_digit_of(word, j);
    c = bits_carry(t.g[j][d], t.g[j][d + 1], c);
  }
  return ClassMasked{G, c};
}

// -------------------------------------------------------------------- the wide digit tables
// A second split for the widest low field: NL = 12 as kClassWideDigits digits of
// kClassWideBits planes instead of four of three — one table step and one shift + index less per
// z image, for tables of 2^4 (+ 1) entries: 16 + 17 + 17 = 50 registers per group instead of 35.
// Same arithmetic (class_digit_table<4>), same contract: the top digit is built under E with
// entry 16 = E, digit 0 needs no entry 16.  Narrower low fields stay on the split above.
constexpr int kClassWideDigits = 3;
constexpr int kClassWideBits = 4;
constexpr int kClassWideNL = kClassWideDigits * kClassWideBits;
constexpr int kClassWideEntries = (1 << kClassWideBits) + 1;
// a low field the wide tables take
constexpr bool class_wide_fit(int nl) { return nl == kClassWideNL; }
// table entries per group: 16 of digit 0, 17 of digits 1 and 2
constexpr int class_wide_table_regs() {
  return (1 << kClassWideBits) + (kClassWideDigits - 1) * kClassWideEntries;
}
// The device loop's register map (R <= kClassWideMaxR groups): group g's tables from
// v(kClassWideBase + 50 g), entry d of digit j at flat register class_wide_reg(j, d) inside it
// — digit 0 at + 0, digits 1 and 2 at + 16 and + 33 — so two groups end at v123.
constexpr int kClassWideBase = 24, kClassWideMaxR = 2;
constexpr int kClassWideGroupRegs = class_wide_table_regs();
constexpr int class_wide_reg(int j, int d) {
  return j == 0 ? d : (1 << kClassWideBits) + kClassWideEntries * (j - 1) + d;
}
constexpr int class_wide_group_base(int g) { return kClassWideBase + kClassWideGroupRegs * g; }
constexpr int class_wide_last_reg(int groups) { return class_wide_group_base(groups) - 1; }

// The digit-ready word of the wide split: digit j in byte j, bytes 0 .. 2 used, byte 3 zero.
// Every digit is masked to kClassWideBits bits here and again in class_wide_of: no index leaves
// a 17-entry table (the loop reads entries d and d + 1 <= 16).
TW_BITS_HD uint32_t class_wide_encode(uint32_t zc) {
  uint32_t w = 0;
  for (int j = 0; j < kClassWideDigits; ++j)
    w |= ((zc >> (kClassWideBits * j)) & ((1u << kClassWideBits) - 1u)) << (8 * j);
  return w;
}
TW_BITS_HD uint32_t class_wide_of(uint32_t word, int j) {
  return (word >> (8 * j)) & ((1u << kClassWideBits) - 1u);
}

// The tables of one x group: entry d of digit j at g[j][d], d = 0 .. 16 (g[0][16] is never read)
struct ClassWideTables {
  uint32_t g[kClassWideDigits][kClassWideEntries];
};
// digit J of the group's UNMASKED low planes; E as in class_digit_tables_one
template <int J>
TW_BITS_HD void class_wide_tables_one(const uint32_t (&low)[kClassWideNL], uint32_t E,
                                      ClassWideTables& t) {
  uint32_t pl[kClassWideBits];
#pragma unroll
  for (int b = 0; b < kClassWideBits; ++b) pl[b] = low[kClassWideBits * J + b];
  class_digit_table<kClassWideBits>(pl, J == kClassWideDigits - 1 ? E : ~0u, t.g[J]);
}
TW_BITS_HD void class_wide_tables(const uint32_t (&low)[kClassWideNL], uint32_t E,
                                  ClassWideTables& t) {
  class_wide_tables_one<0>(low, E, t);
  class_wide_tables_one<1>(low, E, t);
  class_wide_tables_one<2>(low, E, t);
}
// class_gt32_masked by the wide tables: word is a z image's class_wide_encode
TW_BITS_HD ClassMasked class_gt32_wide(const ClassWideTables& t, uint32_t G, uint32_t word) {
  uint32_t c = t.g[0][class_wide_of(word, 0)];
  for (int j = 1; j < kClassWideDigits; ++j) {
    const uint32_t d = class_wide_of(word, j);
    c = bits_carry(t.g[j][d], t.g[j][d + 1], c);
  }
  return ClassMasked{G, c};
}
// The digit width a launch of (nb, k) runs under the hook's setting (0 automatic, 3, 4) where
// it runs a digit loop at all: kClassWideBits only at the widest low field, kClassDigitBits at
// every other.  Automatic: the wide digits wherever they fit (sweep: DESIGN §4.1k).
constexpr int kClassDigitsAuto = kClassWideBits;
TW_BITS_HD int class_digit_bits(int nb, int k, int setting) {
  const int want = setting == 0 ? kClassDigitsAuto : setting;
  return want == kClassWideBits && class_wide_fit(nb - k) ? kClassWideBits : kClassDigitBits;
}

// ------------------------------------------------------------- the low-field table in LDS
// A third form of the 12-plane low field.  The wide loop's carry after its first
// two steps — digits 0 and 1, the low 8 planes — does not depend on the class: it is one of 256
// words per lane, fixed for an x tile.  A block tabulates them once in LDS and its waves read
// the word of a z image's low byte d8 from there; per z and group only the top digit's step
// under E and the popcount are left.
//  Layout: entry d8, lane l is the 8 bytes {group 0 word, group 1 word} at byte
// d8 * kClassLdsEntryBytes + l * 8; 256 entries of two groups end at kClassLdsTableBytes.
constexpr int kClassLdsBits = 8;      // ClassPlan::dbits of this form: planes the table covers
constexpr int kClassLdsGroups = 2;    // x groups of a tile (one 8-byte read serves both)
constexpr int kClassLdsEntries = 1 << kClassLdsBits;
constexpr int kClassLdsEntryBytes = 64 * 4 * kClassLdsGroups;
constexpr int kClassLdsTableBytes = kClassLdsEntries * kClassLdsEntryBytes;
constexpr uint32_t kClassLdsOffsetMask = (uint32_t)(kClassLdsEntries - 1) * kClassLdsEntryBytes;
static_assert(kClassLdsEntryBytes == 512 && kClassLdsTableBytes == 131072 &&
                  kClassLdsOffsetMask == 0x1FE00u,
              "the constants named in the loop's statements");
// The digit-ready word of this form: the top digit (planes 8 .. 11) in bits [3:0] — the byte the
// VGPR index mode reads, below 16 — and the low byte d8 in bits [16:9], so that
// word & kClassLdsOffsetMask is the byte offset of entry d8.  Every other bit is zero.
TW_BITS_HD uint32_t class_lds_encode(uint32_t zc) {
  return ((zc >> kClassLdsBits) & ((1u << kClassWideBits) - 1u)) |
         ((zc & (uint32_t)(kClassLdsEntries - 1)) << 9);
}
TW_BITS_HD uint32_t class_lds_top(uint32_t word) { return word & ((1u << kClassWideBits) - 1u); }
TW_BITS_HD uint32_t class_lds_offset(uint32_t word) { return word & kClassLdsOffsetMask; }
// the complemented image's low 12 bits again
TW_BITS_HD uint32_t class_lds_decode(uint32_t word) {
  return (class_lds_top(word) << kClassLdsBits) | (class_lds_offset(word) / kClassLdsEntryBytes);
}
// Entry d8 of a group: t's digit tables 0 and 1 (class_wide_tables_one<0>, <1> under ~0u)
TW_BITS_HD uint32_t class_lds_entry(const ClassWideTables& t, uint32_t d8) {
  const uint32_t d0 = d8 & 15u, d1 = (d8 >> 4) & 15u;
  return bits_carry(t.g[1][d1], t.g[1][d1 + 1], t.g[0][d0]);
}
// class_gt32_masked through the table: c_low = class_lds_entry of the word's low byte, top the
// top digit's table under E (t.g[2] of class_wide_tables)
TW_BITS_HD ClassMasked class_gt32_lds(uint32_t c_low, const uint32_t (&top)[kClassWideEntries],
                                      uint32_t G, uint32_t word) {
  const uint32_t d = class_lds_top(word);
  return ClassMasked{G, bits_carry(top[d], top[d + 1], c_low)};
}
// Words the loop's scalar loads may read past a run's end (never used): they stay inside the
// count region behind the class-ordered images, as the other loops' batches do
constexpr int kClassLdsOverReadWords = 8;
static_assert(kClassLdsOverReadWords < 64, "the over-read must stay inside the count region");
// The form takes the launches the wide loop takes
constexpr bool class_lds_fit(int nl) { return class_wide_fit(nl); }
// Whether a launch runs the form.  mode: tw_count_chain_class_lds' setting (0 automatic, 1 off,
// 2 on wherever it fits); dbits: the planes per digit the launch's digit loop would run; p: its
// plan.  It fits where that loop is the wide one, a tile is kClassLdsGroups groups and the plan
// has no swapped items.
//  The automatic rule.  The launch is one block per (bag, x tile) and a block fills a CU, so the
// chip takes the blocks in rounds of kClassLdsCus while the wide loop's wave items fill it
// evenly: the form gains 0.72 - 0.76 of the wide launch's time at whole rounds and loses where
// a short last round leaves most CUs idle.  Sweep over 128 .. 1024 blocks (DESIGN §4.1m,
// profiles/r17_classlds_blocks_ab.json; ratio to the wide loop): 128 blocks 1.09 - 1.10, 192
// 0.87, 256 0.72, 320 1.03 - 1.04, 384 0.90, 448 0.82, 512 0.74, 576 0.93, 640 0.86, 768 0.75, 832
// 0.89, 1024 0.75.  So: from kClassLdsMinBlocks on; in the second round only from half a round;
// in the third from a quarter (576 is measured, 513 .. 575 are not); any later round.
constexpr int64_t kClassLdsCus = 256, kClassLdsMinBlocks = 192;
TW_BITS_HD bool class_lds_auto(int64_t blocks) {
  if (blocks < kClassLdsMinBlocks) return false;
  const int64_t rounds = planes_ceil_div(blocks, kClassLdsCus);
  const int64_t last = blocks - (rounds - 1) * kClassLdsCus;  // blocks of the last round
  if (rounds == 2) return 2 * last >= kClassLdsCus;
  if (rounds == 3) return 4 * last >= kClassLdsCus;
  return true;
}
TW_BITS_HD bool class_lds_runs(int mode, int dbits, const PlanesPlan& p, int64_t n_bags) {
  if (mode == 1 || dbits != kClassWideBits || p.R != kClassLdsGroups ||
      p.tiles_s * p.schunks != 0)
    return false;
  return mode == 2 || class_lds_auto(n_bags * p.tiles_x);
}

// ---------------------------------------------------------------------------- the run table
// Per bag: for each non-empty class, ceil(n_c / chunk) runs of near-equal length over the
// class's range of the class-ordered region, classes in ascending order.  An entry is two u32
// words {z0 | class << 24, len} (z0 < 2^24: bags of < 2^24 z images; class < 2^8).
struct ClassRun {
  int64_t z0, len;
  uint32_t cls;
};

// Runs never ask for fewer than kClassMinChunk images, whatever the plan's z chunk: the
// workspace is sized without knowing the plan (the tuning hooks may change between the sizing
// call and the count).
TW_BITS_HD int64_t class_chunk(int64_t z_chunk) {
  return z_chunk < kClassMinChunk ? kClassMinChunk : z_chunk;
}
TW_BITS_HD int64_t class_runs(int64_t n, int64_t chunk) { return planes_ceil_div(n, chunk); }
// run j of the nr = class_runs(n, chunk) runs of a class whose range is [c0, c0 + n)
TW_BITS_HD ClassRun class_run(int64_t c0, int64_t n, int64_t nr, int64_t j, uint32_t cls) {
  const int64_t a = j * n / nr, b = (j + 1) * n / nr;
  return ClassRun{c0 + a, b - a, cls};
}
// class_run for a class of at most 2^16 images: (j + 1) * n < 2^32 (j < nr <= n), so the same
// quotients come from 32-bit arithmetic
TW_BITS_HD ClassRun class_run32(uint32_t c0, uint32_t n, uint32_t nr, uint32_t j, uint32_t cls) {
  const uint32_t a = j * n / nr, b = (j + 1) * n / nr;
  return ClassRun{(int64_t)(c0 + a), (int64_t)(b - a), cls};
}
TW_BITS_HD uint32_t class_entry_lo(const ClassRun& r) { return (uint32_t)r.z0 | (r.cls << 24); }
TW_BITS_HD uint32_t class_entry_hi(const ClassRun& r) { return (uint32_t)r.len; }
TW_BITS_HD ClassRun class_entry(uint32_t lo, uint32_t hi) {
  return ClassRun{(int64_t)(lo & 0xFFFFFFu), (int64_t)hi, lo >> 24};
}

// Entries a bag's table can hold: every non-empty class has at most one run shorter than
// chunk, so sum ceil(n_c / chunk) <= 2^k + nz / chunk.
TW_BITS_HD int64_t class_capacity(int64_t max_nz, int k, int64_t z_chunk) {
  return ((int64_t)1 << k) + planes_ceil_div(max_nz, class_chunk(z_chunk));
}

// The whole table of one bag from its class histogram (the device builds the same entries with
// one thread per class: class_runs + class_run at the scanned offsets).  tab: 2 words per
// entry; returns the number of entries.
TW_BITS_HD int64_t class_table(const uint32_t* hist, int k, int64_t z_chunk, uint32_t* tab) {
  const int64_t chunk = class_chunk(z_chunk);
  int64_t c0 = 0, e = 0;
  for (uint32_t c = 0; c < (1u << k); ++c) {
    const int64_t n = hist[c], nr = class_runs(n, chunk);
    for (int64_t j = 0; j < nr; ++j, ++e) {
      const ClassRun r = class_run(c0, n, nr, j, c);
      tab[2 * e] = class_entry_lo(r);
      tab[2 * e + 1] = class_entry_hi(r);
    }
    c0 += n;
  }
  return e;
}

// ------------------------------------------------------------------------------ the regions
// u32 words after chainplan.h's planes: the class-ordered complemented z images
// [bag][zs_stride], the bags' entry counts [bag], the run tables [bag][cap][2].  Sized for the
// largest table any plan can ask for (k = kClassMaxBits, runs of kClassMinChunk); a launch
// lays its own, smaller table out at the stride of its own capacity.
TW_BITS_HD int64_t class_round64(int64_t n) { return planes_ceil_div(n, 64) * 64; }
TW_BITS_HD int64_t class_work_words(int64_t max_nz, int64_t n_bags) {
  return n_bags * (class_round64(max_nz) +
                   2 * class_capacity(max_nz, kClassMaxBits, kClassMinChunk)) +
         class_round64(n_bags);
}

// ------------------------------------------------------------------------------- the spans
// An item of the class count walks a SPAN of M consecutive table entries of its bag on one x
// tile: what it builds from the tile alone — the low digit tables — serves all
// of them.  Span q of a bag holds entries [q M, min((q + 1) M, cnt)), cnt the bag's entry count;
// the launch reserves class_spans(cap, M) spans per bag and tile, tile-major, and a span past
// the bag's count exits.  M = 1 is the launch of one item per entry.
TW_BITS_HD int class_span_clamp(int64_t runs, int cap) {
  return (int)(runs < 1 ? 1 : runs > cap ? (cap < 1 ? 1 : cap) : runs);
}
TW_BITS_HD int class_spans(int cap, int m) { return (cap + m - 1) / m; }
struct ClassSpan {
  int e0, e1;  // the entries [e0, e1) of span q; empty: e0 >= e1
};
TW_BITS_HD ClassSpan class_span_entries(int q, int m, int cnt) {
  const int64_t a = (int64_t)q * m, b = a + m;
  return ClassSpan{(int)(a < cnt ? a : cnt), (int)(b < cnt ? b : cnt)};
}
struct ClassSpanItem {
  int tx, q;  // x tile and span of slot rem in [0, tiles_x * spans)
};
TW_BITS_HD ClassSpanItem class_span_item(int rem, int spans) {
  const int tx = rem / spans;
  return ClassSpanItem{tx, rem - tx * spans};
}

// The automatic span: the largest power of two M <= kClassSpanMax that still leaves the launch
// kClassSpanFill items for every wave the chip holds at the digit loop's four waves per SIMD
// (256 CUs x 4 SIMDs x 4 waves); with few bags long spans leave CUs idle (32 bags: M = 32 took
// 1.49x the time of M = 1, M = 8 0.89x).  Past 8 the setup left to spread is about 1 % of an
// item's instructions and the sweep no longer orders the spans: 16 was the faster at 20-step
// launches of 64 bags per step (0.76 against 0.78 of M = 1) and the slower at 32-step ones (0.79
// against 0.75).  Sweep: profiles/r13_classspan_ab.json.
constexpr int kClassSpanMax = 8;
constexpr int64_t kClassSpanFill = 1, kClassSpanChipWaves = 256 * 4 * 4;
TW_BITS_HD int class_span_auto(int64_t n_bags, int tiles_x, int cap) {
  int m = 1;
  while (2 * m <= kClassSpanMax && 2 * m <= cap &&
         n_bags * tiles_x * class_spans(cap, 2 * m) >= kClassSpanFill * kClassSpanChipWaves)
    m *= 2;
  return m;
}

struct ClassPlan {
  int k;              // class bits; 0: classes off (k_count_chain_planes)
  int cap;            // table entries per bag of this launch
  int per_bag;        // items per bag: tiles_x * class_spans(cap, span) + tiles_s * schunks
  int64_t chunk;      // longest run
  int64_t zs_stride;  // words per bag of the class-ordered region
  int64_t off_zs, off_cnt, off_tab;  // word offsets into the workspace
  int digits;  // > 0: pre-pass 2 writes the images digit-ready for this many low planes (the
               // launcher sets it for the digit loop; same words, same regions)
  int span;    // table entries an item walks (1 .. cap; the masked-plane loop: always 1)
  int dbits;   // planes per digit of the launch's digit loop: kClassWideBits under the wide
               // loop (pre-pass 2 then writes class_wide_encode), anything else the four-digit
               // split (the launcher sets it; class_plan leaves 0)
};

// A lane's u32 sums over a span — its popcounts, at most 32 per image and group, and
// len * popc(G) — stay below 2^32 for every span inside one bag: bags hold fewer than 2^24 z
// (checked where the workspace is taken) and an item has at most four groups.
constexpr int64_t kClassMaxBagZ = (int64_t)1 << 24;
static_assert(kClassMaxBagZ * 32 * 4 * 2 <= ((int64_t)1 << 32), "a span's u32 lane sums");

TW_BITS_HD ClassPlan class_plan(const PlanesPlan& p, int64_t max_nx, int64_t max_nz,
                                int64_t n_bags, int nb, int k, int64_t runs = 1) {
  ClassPlan c{};
  c.k = k;
  c.chunk = class_chunk(p.z_chunk);
  c.cap = (int)class_capacity(max_nz, k, p.z_chunk);
  c.span = class_span_clamp(runs, c.cap);
  c.per_bag = p.tiles_x * class_spans(c.cap, c.span) + p.tiles_s * p.schunks;
  c.zs_stride = class_round64(max_nz);
  c.off_zs = planes_work_words(max_nx, max_nz, n_bags, nb);
  c.off_cnt = c.off_zs + n_bags * c.zs_stride;
  c.off_tab = c.off_cnt + class_round64(n_bags);
  return c;
}
// words this launch's regions reach (<= planes_work_words + class_work_words)
TW_BITS_HD int64_t class_plan_end(const ClassPlan& c, int64_t n_bags) {
  return c.off_tab + n_bags * 2 * (int64_t)c.cap;
}

// The automatic class bits: the largest k <= min(8, NB - 8) whose mean run max_nz / 2^k stays
// >= kClassMinRun — the shortest measured (k = 8 at the bench's 15625-image bags, runs of 61)
// was the fastest at every multi-bag shape, so the bound only keeps tiny bags from runs of a
// few images that no longer amortise an item's plane loads and its G / P — and none in
// launches of fewer than kClassMinBags bags: pre-pass 2 sorts a bag per block, so with few
// bags it runs on a few CUs for as long as one bag takes (C2's single 1e5-image bag: 1.17x
// the time of k = 0 at best; 32 bags of 15625: 0.82x).  Sweeps: DESIGN §4.1g,
// profiles/r10_count_classes_sweep.json, profiles/r10_count_classes_ab.json.
constexpr int64_t kClassMinRun = 48;
constexpr int64_t kClassMinBags = 32;
TW_BITS_HD int class_bits_auto(int64_t max_nz, int64_t n_bags, int nb) {
  if (n_bags < kClassMinBags) return 0;
  int k = 0;
  while (k < kClassMaxBits && k < nb - 8 && max_nz / ((int64_t)2 << k) >= kClassMinRun) ++k;
  return k;
}

// The swap mode a launch plans with (0 never, 1 chainplan.h's rule, 2 always) from the hook's
// setting.  chainplan.h's automatic rule swaps the x remainder where it takes fewer SLOTS; under
// class runs a padded slot costs NL + 1 VALU per z and group and a swapped one NB + 1.25, so the
// automatic setting keeps the swap only where the swapped remainder of the largest bag is also
// the cheaper in instructions: rx * ceil(nz / 2048) * (NB + 1.25) < nz * (NL + 1).  At the bench
// shape (rx = 1289, nz = 15625, NB = 20, k = 8: 219 k against 203 k) that is no swap, measured
// 0.93-0.95 of the swapped launch's time; a remainder of a few images stays
// swapped.  Forced settings and launches without classes are left alone.
// slot_valu: what a padded slot costs per z and group in the loop the launch runs — 0 stands
// for the masked-plane loop's NL + 1; the digit loop passes kClassDigits + 1,
// the wide-digit loop kClassWideDigits + 1 (§4.1k: neither decision of the sweep moved).
TW_BITS_HD int class_swap_mode(int swap, int64_t max_nx, int64_t max_nz, int nb, int k,
                               int slot_valu = 0) {
  if (k == 0 || swap != 1) return swap;
  const int64_t rx = max_nx % kPlaneGroup, zg = planes_ceil_div(max_nz, kPlaneGroup);
  const int64_t slot = slot_valu > 0 ? slot_valu : nb - k + 1;
  return rx * zg * (4 * nb + 5) < max_nz * 4 * slot ? 1 : 0;
}

// ------------------------------------------------------------------- the fused pre-pass grid
// With class bits both pre-passes run as ONE launch (chain.hip's k_chain_prepass):
// blocks [0, n_bags) sort the z images of one bag each into class runs — first in the grid, so
// the longest blocks start first — and the blocks after them build the planes, wave w of them
// the wave w of k_chain_planes' own grid.  The roles write disjoint regions of the workspace and
// never wait for one another.  Everything below is what the kernel itself evaluates
// (tests/native/chainprepass_driver.cpp enumerates it on the host).
constexpr int kPrepassWaves = 4;  // waves of a pre-pass block (chain.hip: kBlock / kWave)
constexpr int kPrepassThreads = 64 * kPrepassWaves;

// Wave w of the plane pre-pass: the x groups of every bag [bag][gx], then the z groups
// [bag][gz]; `group` is the wave's group of the workspace (planes_word's)
struct PlanesWave {
  bool active, zside;
  int bag, g;
  int64_t group;
};
TW_BITS_HD PlanesWave planes_wave(int64_t w, int64_t n_bags, int gx, int gz) {
  PlanesWave r{};
  const int64_t x_waves = n_bags * gx;
  r.zside = w >= x_waves;
  const int G = r.zside ? gz : gx;
  const int64_t ws = r.zside ? w - x_waves : w;
  if (w < 0 || G == 0 || ws >= n_bags * G) return r;
  r.active = true;
  r.bag = (int)(ws / G);
  r.g = (int)(ws - (int64_t)r.bag * G);
  r.group = w;  // (x side: w; z side: x_waves + ws, the same number)
  return r;
}

struct PrepassGrid {
  int64_t zblocks;  // the z-class blocks, one per bag: block indices [0, zblocks)
  int64_t pblocks;  // the plane blocks after them, kPrepassWaves waves each
  int64_t blocks;
};
TW_BITS_HD PrepassGrid prepass_grid(int64_t n_bags, int gx, int gz) {
  PrepassGrid g{};
  g.zblocks = n_bags;
  g.pblocks = planes_ceil_div(n_bags * ((int64_t)gx + gz), kPrepassWaves);
  g.blocks = g.zblocks + g.pblocks;
  return g;
}
// a grid the launch takes: its block count and the plane waves stay below 2^31
TW_BITS_HD bool prepass_grid_fits(int64_t n_bags, int gx, int gz) {
  return prepass_grid(n_bags, gx, gz).blocks < ((int64_t)1 << 31) &&
         n_bags * ((int64_t)gx + gz) < ((int64_t)1 << 31);
}

enum { kPrepassZClass = 0, kPrepassPlanes = 1, kPrepassIdle = 2 };
struct PrepassRole {
  int role;   // kPrepassZClass: the whole block sorts `bag`; kPrepassPlanes: this wave builds
              // group g of side `zside` of `bag`; kPrepassIdle: a wave past the last group
  int bag, g;
  bool zside;
  int64_t group;
};
TW_BITS_HD PrepassRole prepass_role(int64_t block, int wave, int64_t n_bags, int gx, int gz) {
  if (block < n_bags) return PrepassRole{kPrepassZClass, (int)block, 0, false, 0};
  const PlanesWave w = planes_wave((block - n_bags) * kPrepassWaves + wave, n_bags, gx, gz);
  if (!w.active) return PrepassRole{kPrepassIdle, 0, 0, false, 0};
  return PrepassRole{kPrepassPlanes, w.bag, w.g, w.zside, w.group};
}

// The z-class role keeps a bag of up to kPrepassCap images in registers, kPrepassPer per thread
// (kPrepassPerSmall where the bag fits that), and reads it from global memory once; a larger
// (or empty) bag runs the two-pass streaming loop.  An image's index inside its class is below
// kPrepassCap: two of them share a register.
constexpr int kPrepassPer = 64, kPrepassPerSmall = 16;
constexpr int64_t kPrepassCap = (int64_t)kPrepassThreads * kPrepassPer;
constexpr int64_t kPrepassCapSmall = (int64_t)kPrepassThreads * kPrepassPerSmall;
static_assert(kPrepassCap <= (1 << 16), "two 16-bit class indices per register");
// images per thread a bag of nz images is sorted with; 0: the streaming loop
TW_BITS_HD int prepass_per_thread(int64_t nz) {
  return nz < 1 || nz > kPrepassCap ? 0 : nz <= kPrepassCapSmall ? kPrepassPerSmall : kPrepassPer;
}
// The form a launch runs (tw_count_chain_prepass_of): 1 the separate launches, 2 fused with
// every bag register-resident, 3 fused with bags that may take the streaming loop.
// mode: tw_count_chain_prepass' setting (0 automatic: fused wherever the class form runs)
TW_BITS_HD int prepass_form(int mode, int k, int64_t max_nz) {
  if (k <= 0 || mode == 1) return 1;
  return max_nz <= kPrepassCap ? 2 : 3;
}

#if defined(__HIPCC__)
// Images per scalar load of the masked-plane loop (widths 2, 8 and 16 lost: DESIGN §4.1h)
constexpr int kClassBatch = 4;
// A scalar batch starts inside its run and may read up to kClassBatch - 1 words past the run's
// end: into the same bag's later runs, the next bag's region or — from the last run of the last
// bag — the entry counts, class_round64(n_bags) >= 64 words that follow the class-ordered
// region (class_plan: off_cnt = off_zs + n_bags * zs_stride).  Always inside the workspace; the
// words read past the end are never compared.
static_assert(kClassBatch - 1 < 64, "the over-read must stay inside the count region");

// The masked-plane loop, the class loop of every (NB, K) whose low field the
// digit tables do not take.  One wave item: R groups of NB plane words per lane at pw
// (bits_count_planes' layout) against the run's len >= 1 images at zs, complemented u32 of
// class cls (wave-uniform).  Once per item and group: G and P of the class from the K top
// planes, the NL low planes ANDed with E = P & ~G, and popc(G) into ng.  Per z and group: the
// low chain on the masked planes and one popcount of its carry; the class-constant term is
// added once, as len * ng.  Exactly len images are evaluated: a padded scalar slot would be
// missed by the len * ng term.
//  zs is wave-uniform, so the run is read through the constant address space (s_load_dwordx4
// straight into SGPRs): whole batches of kClassBatch images in an unrolled trip with the next
// batch in flight, the last len mod kClassBatch images one at a time from the batch already
// loaded.
template <int NB, int K, int R>
__device__ __forceinline__ unsigned long long bits_count_class(const uint32_t* __restrict__ pw,
                                                               const uint32_t* __restrict__ zs,
                                                               int len, uint32_t cls, int lane) {
  constexpr int NL = NB - K;
  uint32_t lo[R][NL], acc[R];
  uint32_t ng = 0;  // popc(G) over the groups: the class-constant term of one z
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint32_t top[K];
#pragma unroll
    for (int b = 0; b < NL; ++b) lo[r][b] = pw[(r * NB + b) * 64 + lane];
#pragma unroll
    for (int b = 0; b < K; ++b) top[b] = pw[(r * NB + NL + b) * 64 + lane];
    uint32_t g, p;
    class_gp<K>(top, cls, g, p);
    class_mask_planes<NL>(lo[r], class_equal_mask(g, p), lo[r]);
    ng = bits_popc_add(g, ng);
    acc[r] = 0;
  }
  auto step = [&](uint32_t sc) {
    uint32_t m[NL], c[R];
#pragma unroll
    for (int b = 0; b < NL; ++b) m[b] = bits_mask(sc, b);
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = lo[r][0] & m[0];
#pragma unroll
    for (int b = 1; b < NL; ++b)
#pragma unroll
      for (int r = 0; r < R; ++r) c[r] = bits_carry(lo[r][b], m[b], c[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = bits_popc_add(c[r], acc[r]);
  };
  constexpr int B = kClassBatch;
  typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
  const ConstWords zc = (ConstWords)(uintptr_t)zs;
  uint32_t cur[B], next[B];
  auto load = [&](int j, uint32_t (&w)[B]) {
#pragma unroll
    for (int u = 0; u < B; ++u) w[u] = zc[j + u];
  };
  load(0, next);
  int j = 0;
  for (; j + B <= len; j += B) {
#pragma unroll
    for (int u = 0; u < B; ++u) cur[u] = next[u];
    load(min(j + B, len - 1), next);  // (starts inside the run; past a last whole batch: unused)
#pragma unroll
    for (int u = 0; u < B; ++u) step(cur[u]);
  }
  for (; j < len; ++j) {  // next holds the images from j on: never a word past the run's end
    step(next[0]);
#pragma unroll
    for (int u = 0; u + 1 < B; ++u) next[u] = next[u + 1];
  }
  unsigned long long tot = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) tot += acc[r];
  tot += (unsigned long long)(uint32_t)len * ng;  // the run's exact length
  return tot;
}
// The loop a launch of (nb, k) runs: 3 the digit tables (§4.1i) where the low field fits
// them, 2 the masked-plane loop everywhere else
constexpr int class_loop_form(int nb, int k) { return class_digits_fit(nb - k) ? 3 : 2; }
// Groups per item under the digit loops: their register maps hold two, which keeps 4 waves per
// SIMD (3 and 4 groups — 3 and 2 waves — lost: DESIGN §4.1i)
constexpr int kClassDigitsMaxR = 2;

// The digit loop.  A group's tables sit in FIXED VGPRs and the hardware's VGPR
// index mode picks the entry: between s_set_gpr_idx_on and _off, M0[7:0] — a z digit — is added
// to the register numbers of a VALU instruction's first two sources (mode 0x3), so
//     v_mov_b32    c, v24                     c = G0[d0]
//     v_bitop3_b32 c, v32, v33, c  0xE8       c = majority(G1[d1], G1[d1 + 1], c)
// read v(24 + d0) and v(32 + d1), v(33 + d1); the third source and the destination are not
// indexed.  Register map, two groups (g = 0, 1): v8 .. v23 the carries of a batch, four
// registers per image of which the groups use the first two (image u, group g: v(8 + 4u + g));
// group g's 36 table registers from v(24 + 36g) — digit 0 at + 0 (8 entries), digits 1, 2, 3 at
// + 8, + 17, + 26 (9 entries each), one spare — so group 0 is v24 .. v59 and group 1 v60 .. v95.
// Per z the scalar side shifts the digit-ready word (class_digit_encode) three times and sets
// the index four times; per z and group the lane side issues 4 chain instructions and, after
// _off — v_bcnt's operands would be indexed too — 1 popcount into the group's counter.  M0 and
// MODE are written and consumed inside one asm statement (the compiler keeps nothing in M0
// across a statement).  Only words pre-pass 2 encoded reach M0: every digit is below
// 2^kClassDigitBits, so an indexed read stays inside its table.
typedef uint32_t ClassVec4 __attribute__((ext_vector_type(4)));
typedef uint32_t ClassVec32 __attribute__((ext_vector_type(32)));
constexpr int kClassDigitGroupRegs = 36;
static_assert(class_digit_table_regs(kClassDigitMaxNL) <= kClassDigitGroupRegs, "register map");
// flat register of entry d of digit j inside a group's 36
constexpr int class_digit_reg(int j, int d) { return j == 0 ? d : 8 + 9 * (j - 1) + d; }
static_assert(kClassDigitsMaxR == 2, "the registers named below: two groups, v24 .. v95");

#define TW_DG_OP(C, A, B) "v_bitop3_b32 " C ", " A ", " B ", " C " bitop3:0xe8\n\t"
#define TW_DG_MOV(C, A) "v_mov_b32 " C ", " A "\n\t"
#define TW_DG_IDX(Z, T, SH) "s_lshr_b32 " T ", " Z ", " SH "\n\ts_set_gpr_idx_idx " T "\n\t"
// digit steps of the groups: C0 .. C3 the carry registers of one image (groups: C0, C1)
#define TW_DG_D0_1(C0, C1, C2, C3) TW_DG_MOV(C0, "v24")
#define TW_DG_D0_2(C0, C1, C2, C3) TW_DG_D0_1(C0, C1, C2, C3) TW_DG_MOV(C1, "v60")
#define TW_DG_D1_1(C0, C1, C2, C3) TW_DG_OP(C0, "v32", "v33")
#define TW_DG_D1_2(C0, C1, C2, C3) TW_DG_D1_1(C0, C1, C2, C3) TW_DG_OP(C1, "v68", "v69")
#define TW_DG_D2_1(C0, C1, C2, C3) TW_DG_OP(C0, "v41", "v42")
#define TW_DG_D2_2(C0, C1, C2, C3) TW_DG_D2_1(C0, C1, C2, C3) TW_DG_OP(C1, "v77", "v78")
#define TW_DG_D3_1(C0, C1, C2, C3) TW_DG_OP(C0, "v50", "v51")
#define TW_DG_D3_2(C0, C1, C2, C3) TW_DG_D3_1(C0, C1, C2, C3) TW_DG_OP(C1, "v86", "v87")
// one image against R groups; the index already holds its digit 0
#define TW_DG_Z(R, Z, T, C0, C1, C2, C3)                        \
  TW_DG_D0_##R(C0, C1, C2, C3)                                  \
  TW_DG_IDX(Z, T, "8") TW_DG_D1_##R(C0, C1, C2, C3)             \
  TW_DG_IDX(Z, T, "16") TW_DG_D2_##R(C0, C1, C2, C3)            \
  TW_DG_IDX(Z, T, "24") TW_DG_D3_##R(C0, C1, C2, C3)
// the popcounts of one image's carries, after _off (their operands would be indexed too)
#define TW_DG_CNT(C, A) "v_bcnt_u32_b32 " A ", " C ", " A "\n\t"
#define TW_DG_C_1(C0, C1, C2, C3) TW_DG_CNT(C0, "%[a0]")
#define TW_DG_C_2(C0, C1, C2, C3) TW_DG_C_1(C0, C1, C2, C3) TW_DG_CNT(C1, "%[a1]")
#define TW_DG_ONE(R)                                            \
  "s_set_gpr_idx_on %[z0], 0x3\n\t"                             \
  TW_DG_Z(R, "%[z0]", "%[t]", "v8", "v9", "v10", "v11") "s_set_gpr_idx_off\n\t" \
  TW_DG_C_##R("v8", "v9", "v10", "v11")
// (the statement loads the next batch itself and waits for it after the chains: a load issued
// outside would be waited for before the statement)
#define TW_DG_BATCH(R)                                                                   \
  "s_load_dwordx4 %[nx], %[p], 0x0\n\ts_set_gpr_idx_on %[z0], 0x3\n\t"                   \
  TW_DG_Z(R, "%[z0]", "%[t]", "v8", "v9", "v10", "v11") "s_set_gpr_idx_idx %[z1]\n\t"   \
  TW_DG_Z(R, "%[z1]", "%[t]", "v12", "v13", "v14", "v15") "s_set_gpr_idx_idx %[z2]\n\t" \
  TW_DG_Z(R, "%[z2]", "%[t]", "v16", "v17", "v18", "v19") "s_set_gpr_idx_idx %[z3]\n\t" \
  TW_DG_Z(R, "%[z3]", "%[t]", "v20", "v21", "v22", "v23") "s_set_gpr_idx_off\n\t"       \
  TW_DG_C_##R("v8", "v9", "v10", "v11") TW_DG_C_##R("v12", "v13", "v14", "v15")         \
  TW_DG_C_##R("v16", "v17", "v18", "v19") TW_DG_C_##R("v20", "v21", "v22", "v23")       \
  "s_waitcnt lgkmcnt(0)"
#define TW_DG_ACC_1(a) [a0] "+v"(a[0])
#define TW_DG_ACC_2(a) TW_DG_ACC_1(a), [a1] "+v"(a[1])
// (s_lshr_b32 writes SCC: without the clobber a compare is scheduled across the statement)
#define TW_DG_CARRIES1 "scc", "v8", "v9", "v10", "v11"
#define TW_DG_CARRIES4                                                                   \
  TW_DG_CARRIES1, "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", \
      "v22", "v23"
#define TW_DG_TAB_1(a, b) "{v[24:55]}"(a[0]), "{v[56:59]}"(b[0])
#define TW_DG_TAB_2(a, b) TW_DG_TAB_1(a, b), "{v[60:91]}"(a[1]), "{v[92:95]}"(b[1])
#define TW_DG_CASE_BATCH(R)                                                                \
  if constexpr (kR == R)                                                                   \
    asm volatile(TW_DG_BATCH(R)                                                            \
                 : TW_DG_ACC_##R(acc), [t] "=&s"(t), [nx] "=&s"(next)                      \
                 : [z0] "s"(z[0]), [z1] "s"(z[1]), [z2] "s"(z[2]), [z3] "s"(z[3]),         \
                   [p] "s"(nz), TW_DG_TAB_##R(ta, tb)                                      \
                 : TW_DG_CARRIES4);
#define TW_DG_CASE_ONE(R)                                                                  \
  if constexpr (kR == R)                                                                   \
    asm volatile(TW_DG_ONE(R)                                                              \
                 : TW_DG_ACC_##R(acc), [t] "=&s"(t)                                        \
                 : [z0] "s"(z), TW_DG_TAB_##R(ta, tb)                                      \
                 : TW_DG_CARRIES1);

// The class count of one item under the digit loop: R <= kClassDigitsMaxR groups
// against the n >= 1 runs of a SPAN, whose table entries start at tab; the bag's class-ordered
// images, digit-ready, at zbag.  Once per item: the groups' planes are loaded, digit tables 0-2
// — which depend on the x tile alone — go to their pinned registers, and the K top planes and
// the top digit's planes stay in registers or are reloaded per class (kKeep below: whichever
// keeps the instantiation's waves per SIMD).  Per run of a new class: G, P and E, popc(G), and
// the top digit's entries (flat registers 26 .. 34 of the group: they span the ClassVec32 /
// ClassVec4 pair); consecutive runs of one class — a class longer than the chunk — keep them.
//  Per run: whole batches of four images per asm statement, each loading the batch after it
// (two statements per trip, the batches' registers swapping roles); the last len mod 4 images
// one statement each from the batch already loaded, so exactly len images are evaluated and no
// word past the run's end reaches M0.  A whole batch's load reads up to four words past the
// run's end (never used): inside the workspace, as in bits_count_class.
//  The lane sums are u32 over the whole span: see kClassMaxBagZ.
constexpr int kClassDigitBatch = 4;  // images per statement and scalar load
static_assert(kClassDigitBatch < 64, "the over-read must stay inside the count region");
template <int NB, int K, int R>
__device__ __forceinline__ unsigned long long bits_count_span_digits(
    const uint32_t* __restrict__ pw, const uint32_t* __restrict__ zbag,
    const uint32_t* __restrict__ tab, int n, int lane) {
  constexpr int NL = NB - K;
  constexpr int kTop = kClassDigits - 1;  // the digit whose planes are ANDed with E
  constexpr int W3 = class_digit_width(NL, kTop), S3 = class_digit_shift(NL, kTop);
  [[maybe_unused]] constexpr int kR = R;
  static_assert(R >= 1 && R <= kClassDigitsMaxR, "the register map holds kClassDigitsMaxR groups");
  // The class-dependent planes (K top, W3 of the top digit) stay in registers where the tables
  // fill the register map anyway (NL = 12: 4 waves per SIMD with or without them); at narrower
  // low fields the map ends at v95 — 5 waves — and a new class reloads them (cache hits).
  constexpr bool kKeep = NL == kClassDigitMaxNL;
  constexpr int RK = kKeep ? R : 1;
  ClassVec32 ta[R];
  ClassVec4 tb[R];
  [[maybe_unused]] uint32_t top[RK][K], hi[RK][W3];
  uint32_t acc[R];
  auto place = [&](int r, int j, int d, uint32_t v) {
    const int f = class_digit_reg(j, d);
    if (f < 32)
      ta[r][f] = v;
    else
      tb[r][f - 32] = v;
  };
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint32_t low[NL];
#pragma unroll
    for (int b = 0; b < NL; ++b) low[b] = pw[(r * NB + b) * 64 + lane];
    if constexpr (kKeep) {
#pragma unroll
      for (int b = 0; b < K; ++b) top[r][b] = pw[(r * NB + NL + b) * 64 + lane];
#pragma unroll
      for (int b = 0; b < W3; ++b) hi[r][b] = low[S3 + b];
    }
    ClassDigitTables t;
    class_digit_tables_one<NL, 0>(low, ~0u, t);
    class_digit_tables_one<NL, 1>(low, ~0u, t);
    class_digit_tables_one<NL, 2>(low, ~0u, t);
    ta[r] = 0u, tb[r] = 0u;
#pragma unroll
    for (int j = 0; j < kTop; ++j)
#pragma unroll
      for (int d = 0; d < (j == 0 ? 8 : kClassDigitEntries); ++d) place(r, j, d, t.g[j][d]);
    acc[r] = 0;
  }
  typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
  const ConstWords ct = (ConstWords)(uintptr_t)tab;
  const ConstWords zc = (ConstWords)(uintptr_t)zbag;
  // z: the four images to evaluate; the statement loads the four words at nz into next
  auto batch = [&](const ClassVec4 z, ConstWords nz, ClassVec4& next) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t t;
    TW_DG_CASE_BATCH(1) TW_DG_CASE_BATCH(2)
#else
    next = z;
#endif
  };
  auto one = [&](uint32_t z) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t t;
    TW_DG_CASE_ONE(1) TW_DG_CASE_ONE(2)
#endif
  };
  uint32_t ng = 0, cg = 0;  // popc(G) over the groups of the class at hand; sum of len * ng
  uint32_t cls = ~0u;       // (no class)
  for (int e = 0; e < n; ++e) {
    const ClassRun run = class_entry(ct[2 * e], ct[2 * e + 1]);
    if (run.cls != cls) {  // wave-uniform
      cls = run.cls;
      ng = 0;
      int ql = lane;  // (opaque per class: the reloads are not hoisted out of the span)
#if defined(__HIP_DEVICE_COMPILE__)
      if constexpr (!kKeep) asm volatile("" : "+v"(ql));
#endif
#pragma unroll
      for (int r = 0; r < R; ++r) {
        uint32_t G, P, g[(1 << W3) + 1], tp[K], hp[W3];
#pragma unroll
        for (int b = 0; b < K; ++b)
          tp[b] = kKeep ? top[kKeep ? r : 0][b] : pw[(r * NB + NL + b) * 64 + ql];
#pragma unroll
        for (int b = 0; b < W3; ++b)
          hp[b] = kKeep ? hi[kKeep ? r : 0][b] : pw[(r * NB + S3 + b) * 64 + ql];
        class_gp<K>(tp, cls, G, P);
        ng = bits_popc_add(G, ng);
        class_digit_table<W3>(hp, class_equal_mask(G, P), g);
#pragma unroll
        for (int d = 1; d <= (1 << W3); ++d) place(r, kTop, d, g[d]);  // (entry 0 stays 0)
      }
    }
    const int len = (int)run.len;  // >= 1: only non-empty classes have runs
    cg += (uint32_t)len * ng;      // the run's exact length
    ConstWords p = zc + run.z0;
    ClassVec4 a, b;
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = p[u];
    int j = 0;
    for (; j + 8 <= len; j += 8, p += 8) {
      batch(a, p + 4, b);
      batch(b, p + 8, a);
    }
    if (j + 4 <= len) {
      batch(a, p + 4, b);
      a = b, j += 4;
    }
    for (; j < len; ++j) {  // a holds the images from j on: never a word past the run's end
      one(a[0]);
      a = a.yzww;
    }
  }
  unsigned long long tot = cg;
#pragma unroll
  for (int r = 0; r < R; ++r) tot += acc[r];
  return tot;
}
// The instantiation for an item's ng <= R groups (wave-uniform): no group tests in the loop
template <int NB, int K, int R>
__device__ __forceinline__ unsigned long long bits_count_span_digits_of(
    const uint32_t* __restrict__ pw, const uint32_t* __restrict__ zbag,
    const uint32_t* __restrict__ tab, int n, int lane, int ng) {
  if constexpr (R > 1)
    if (ng < R) return bits_count_span_digits_of<NB, K, R - 1>(pw, zbag, tab, n, lane, ng);
  return bits_count_span_digits<NB, K, R>(pw, zbag, tab, n, lane);
}

// The wide-digit loop: bits_count_span_digits on the three 4-plane digits of a
// 12-plane low field (class_wide_*); its register map holds the kClassDigitsMaxR groups of an
// item.  Per z the scalar side shifts the word twice and sets the index three times (5 SALU,
// not 7); per z and group the lane side issues one v_mov, two v_bitop3 and one v_bcnt (4 VALU,
// not 5).  Register map: v8 .. v15 the carries of a batch
// (image u, group g: v(8 + 2u + g)); group g's 50 table registers from v(24 + 50g): digit 0 at
// + 0 (16 entries), digits 1 and 2 at + 16 and + 33 (17 entries each); two groups end at v123.
// Only words pre-pass 2 wrote with class_wide_encode reach M0: every digit is below 16, so an
// indexed read of entries d and d + 1 stays inside its table.
typedef uint32_t ClassVec2 __attribute__((ext_vector_type(2)));
typedef uint32_t ClassVec16 __attribute__((ext_vector_type(16)));
static_assert(kClassDigitsMaxR <= kClassWideMaxR, "the wide register map holds two groups");
static_assert(class_wide_group_base(0) == 24 && class_wide_group_base(1) == 74 &&
                  class_wide_last_reg(2) == 123,
              "the registers named below");
static_assert(class_wide_reg(1, 0) == 40 - 24 && class_wide_reg(2, 0) == 57 - 24 &&
                  class_wide_reg(2, 16) == 73 - 24,
              "the registers named below");
#define TW_WD_D0_1(C0, C1) TW_DG_MOV(C0, "v24")
#define TW_WD_D0_2(C0, C1) TW_WD_D0_1(C0, C1) TW_DG_MOV(C1, "v74")
#define TW_WD_D1_1(C0, C1) TW_DG_OP(C0, "v40", "v41")
#define TW_WD_D1_2(C0, C1) TW_WD_D1_1(C0, C1) TW_DG_OP(C1, "v90", "v91")
#define TW_WD_D2_1(C0, C1) TW_DG_OP(C0, "v57", "v58")
#define TW_WD_D2_2(C0, C1) TW_WD_D2_1(C0, C1) TW_DG_OP(C1, "v107", "v108")
// one image against R groups; the index already holds its digit 0
#define TW_WD_Z(R, Z, T, C0, C1)                                \
  TW_WD_D0_##R(C0, C1)                                          \
  TW_DG_IDX(Z, T, "8") TW_WD_D1_##R(C0, C1)                     \
  TW_DG_IDX(Z, T, "16") TW_WD_D2_##R(C0, C1)
#define TW_WD_C_1(C0, C1) TW_DG_CNT(C0, "%[a0]")
#define TW_WD_C_2(C0, C1) TW_WD_C_1(C0, C1) TW_DG_CNT(C1, "%[a1]")
#define TW_WD_ONE(R)                                            \
  "s_set_gpr_idx_on %[z0], 0x3\n\t"                             \
  TW_WD_Z(R, "%[z0]", "%[t]", "v8", "v9") "s_set_gpr_idx_off\n\t" TW_WD_C_##R("v8", "v9")
#define TW_WD_BATCH(R)                                                        \
  "s_load_dwordx4 %[nx], %[p], 0x0\n\ts_set_gpr_idx_on %[z0], 0x3\n\t"        \
  TW_WD_Z(R, "%[z0]", "%[t]", "v8", "v9") "s_set_gpr_idx_idx %[z1]\n\t"      \
  TW_WD_Z(R, "%[z1]", "%[t]", "v10", "v11") "s_set_gpr_idx_idx %[z2]\n\t"    \
  TW_WD_Z(R, "%[z2]", "%[t]", "v12", "v13") "s_set_gpr_idx_idx %[z3]\n\t"    \
  TW_WD_Z(R, "%[z3]", "%[t]", "v14", "v15") "s_set_gpr_idx_off\n\t"          \
  TW_WD_C_##R("v8", "v9") TW_WD_C_##R("v10", "v11")                          \
  TW_WD_C_##R("v12", "v13") TW_WD_C_##R("v14", "v15")                        \
  "s_waitcnt lgkmcnt(0)"
#define TW_WD_CARRIES1 "scc", "v8", "v9"
#define TW_WD_CARRIES4 TW_WD_CARRIES1, "v10", "v11", "v12", "v13", "v14", "v15"
#define TW_WD_TAB_1(a, b, c) "{v[24:55]}"(a[0]), "{v[56:71]}"(b[0]), "{v[72:73]}"(c[0])
#define TW_WD_TAB_2(a, b, c) \
  TW_WD_TAB_1(a, b, c), "{v[74:105]}"(a[1]), "{v[106:121]}"(b[1]), "{v[122:123]}"(c[1])
#define TW_WD_CASE_BATCH(R)                                                                \
  if constexpr (kR == R)                                                                   \
    asm volatile(TW_WD_BATCH(R)                                                            \
                 : TW_DG_ACC_##R(acc), [t] "=&s"(t), [nx] "=&s"(next)                      \
                 : [z0] "s"(z[0]), [z1] "s"(z[1]), [z2] "s"(z[2]), [z3] "s"(z[3]),         \
                   [p] "s"(nz), TW_WD_TAB_##R(ta, tb, tc)                                  \
                 : TW_WD_CARRIES4);
#define TW_WD_CASE_ONE(R)                                                                  \
  if constexpr (kR == R)                                                                   \
    asm volatile(TW_WD_ONE(R)                                                              \
                 : TW_DG_ACC_##R(acc), [t] "=&s"(t)                                        \
                 : [z0] "s"(z), TW_WD_TAB_##R(ta, tb, tc)                                  \
                 : TW_WD_CARRIES1);

// The class count of one item under the wide-digit loop: bits_count_span_digits' contract and
// statement structure — whole batches of four images per asm statement, each loading the batch
// after it; the last len mod 4 images one statement each from the batch already loaded, so
// exactly len images are evaluated and no word past a run's end reaches M0.  Once per item:
// digit tables 0 and 1.  The K top planes and the top digit's four planes are reloaded per new
// class (cache hits; the opaque lane index keeps the reloads inside the span): keeping them
// would cost the fourth wave per SIMD.  The per-class rebuild writes the top digit's entries
// 1 .. 16 in place; entry 0 stays 0.
template <int NB, int K, int R>
__device__ __forceinline__ unsigned long long bits_count_span_wide(
    const uint32_t* __restrict__ pw, const uint32_t* __restrict__ zbag,
    const uint32_t* __restrict__ tab, int n, int lane) {
  constexpr int NL = NB - K;
  static_assert(class_wide_fit(NL), "the wide split is that of the 12-plane low field");
  constexpr int kTop = kClassWideDigits - 1;  // the digit whose planes are ANDed with E
  constexpr int W = kClassWideBits, S = W * kTop;
  [[maybe_unused]] constexpr int kR = R;
  static_assert(R >= 1 && R <= kClassWideMaxR, "the register map holds kClassWideMaxR groups");
  ClassVec32 ta[R];
  ClassVec16 tb[R];
  ClassVec2 tc[R];
  uint32_t acc[R];
  auto place = [&](int r, int j, int d, uint32_t v) {
    const int f = class_wide_reg(j, d);
    if (f < 32)
      ta[r][f] = v;
    else if (f < 48)
      tb[r][f - 32] = v;
    else
      tc[r][f - 48] = v;
  };
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint32_t low[NL];
#pragma unroll
    for (int b = 0; b < S; ++b) low[b] = pw[(r * NB + b) * 64 + lane];
#pragma unroll
    for (int b = S; b < NL; ++b) low[b] = 0u;  // (the top digit's planes: per class)
    ClassWideTables t;
    class_wide_tables_one<0>(low, ~0u, t);
    class_wide_tables_one<1>(low, ~0u, t);
    ta[r] = 0u, tb[r] = 0u, tc[r] = 0u;
#pragma unroll
    for (int j = 0; j < kTop; ++j)
#pragma unroll
      for (int d = 0; d < (j == 0 ? 1 << W : kClassWideEntries); ++d) place(r, j, d, t.g[j][d]);
    acc[r] = 0;
  }
  typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
  const ConstWords ct = (ConstWords)(uintptr_t)tab;
  const ConstWords zc = (ConstWords)(uintptr_t)zbag;
  // z: the four images to evaluate; the statement loads the four words at nz into next
  auto batch = [&](const ClassVec4 z, ConstWords nz, ClassVec4& next) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t t;
    TW_WD_CASE_BATCH(1) TW_WD_CASE_BATCH(2)
#else
    next = z;
#endif
  };
  auto one = [&](uint32_t z) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t t;
    TW_WD_CASE_ONE(1) TW_WD_CASE_ONE(2)
#endif
  };
  uint32_t ng = 0, cg = 0;  // popc(G) over the groups of the class at hand; sum of len * ng
  uint32_t cls = ~0u;       // (no class)
  for (int e = 0; e < n; ++e) {
    const ClassRun run = class_entry(ct[2 * e], ct[2 * e + 1]);
    if (run.cls != cls) {  // wave-uniform
      cls = run.cls;
      ng = 0;
      int ql = lane;  // (opaque per class: the reloads are not hoisted out of the span)
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" : "+v"(ql));
#endif
#pragma unroll
      for (int r = 0; r < R; ++r) {
        uint32_t G, P, g[kClassWideEntries], tp[K], hp[W];
#pragma unroll
        for (int b = 0; b < K; ++b) tp[b] = pw[(r * NB + NL + b) * 64 + ql];
#pragma unroll
        for (int b = 0; b < W; ++b) hp[b] = pw[(r * NB + S + b) * 64 + ql];
        class_gp<K>(tp, cls, G, P);
        ng = bits_popc_add(G, ng);
        class_digit_table<W>(hp, class_equal_mask(G, P), g);
#pragma unroll
        for (int d = 1; d <= (1 << W); ++d) place(r, kTop, d, g[d]);  // (entry 0 stays 0)
      }
    }
    const int len = (int)run.len;  // >= 1: only non-empty classes have runs
    cg += (uint32_t)len * ng;      // the run's exact length
    ConstWords p = zc + run.z0;
    ClassVec4 a, b;
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = p[u];
    int j = 0;
    for (; j + 8 <= len; j += 8, p += 8) {
      batch(a, p + 4, b);
      batch(b, p + 8, a);
    }
    if (j + 4 <= len) {
      batch(a, p + 4, b);
      a = b, j += 4;
    }
    for (; j < len; ++j) {  // a holds the images from j on: never a word past the run's end
      one(a[0]);
      a = a.yzww;
    }
  }
  unsigned long long tot = cg;
#pragma unroll
  for (int r = 0; r < R; ++r) tot += acc[r];
  return tot;
}
template <int NB, int K, int R>
__device__ __forceinline__ unsigned long long bits_count_span_wide_of(
    const uint32_t* __restrict__ pw, const uint32_t* __restrict__ zbag,
    const uint32_t* __restrict__ tab, int n, int lane, int ng) {
  if constexpr (R > 1)
    if (ng < R) return bits_count_span_wide_of<NB, K, R - 1>(pw, zbag, tab, n, lane, ng);
  return bits_count_span_wide<NB, K, R>(pw, zbag, tab, n, lane);
}

// The LDS-table loop: the wide loop with its first two steps read from the
// block's table (class_lds_*).  Per z: s_and (the entry's offset), one v_add_u32 (offset + the
// lane's table address), one ds_read_b64 (both groups' words), one s_set_gpr_idx_idx; per z and
// group one v_bitop3 on the top digit's table — its third source the word read — and one v_bcnt:
// 5 VALU + 2 SALU + 1 LDS per z at two groups (the trip's own 9 scalar instructions per 8 z on
// top).  A whole run is ONE asm statement, so nothing the compiler allocates lives in the
// registers named here while LDS reads are in flight.  Register map, all of it clobbers or
// pinned inputs: two sets of carries, A = v8 .. v15 and B = v16 .. v23 (image u, group g:
// v(base + 2u + g), the pair one ds_read_b64 fills); v4, v5 the LDS addresses; the top digit's
// 17 entries of group 0 in v24 .. v40, of group 1 in v42 .. v58 (tuples start even); the eight
// words at hand in s40 .. s47 (W), the eight after them in s48 .. s55 (N), s56 a temporary.
//  A trip of the main loop takes two batches of four images: it loads N, reads batch 1's words
// from LDS into B while the chains of batch 0 run on A, then reads the next trip's batch 0 into
// A (from N) while the chains of batch 1 run on B.  Every wait is s_waitcnt lgkmcnt(0): scalar
// loads return out of order and share the counter with LDS.  The LDS instructions and the
// address adds sit outside s_set_gpr_idx_on / _off.  Only words of the run reach M0 or an LDS
// address: a set is read ahead for a WHOLE batch only (the main loop runs while 12 images are
// left), the last 1 .. 3 images go one at a time.  The scalar loads read up to 8 words past the
// run's end — inside the workspace, as in bits_count_class — and never use them.
constexpr int kClassLdsTopBase0 = 24, kClassLdsTopBase1 = 42;
static_assert(kClassLdsTopBase0 + kClassWideEntries - 1 == 40 && kClassLdsTopBase1 % 2 == 0 &&
                  kClassLdsTopBase1 > 40 && kClassLdsTopBase1 + kClassWideEntries - 1 == 58,
              "the registers named below");
static_assert(kClassLdsOverReadWords == 8, "the loop's eight-word loads");
#define TW_LD_RD(Z, A, C) \
  "s_and_b32 s56, " Z ", 0x1fe00\n\tv_add_u32 " A ", s56, %[l8]\n\tds_read_b64 " C ", " A "\n\t"
#define TW_LD_OPS(C0, C1) TW_DG_OP(C0, "v24", "v25") TW_DG_OP(C1, "v42", "v43")
#define TW_LD_CNT(C0, C1) TW_DG_CNT(C0, "%[n0]") TW_DG_CNT(C1, "%[n1]")
// the LDS reads of four images' words into a set (its pairs P0 .. P3)
#define TW_LD_READS(Z0, Z1, Z2, Z3, P0, P1, P2, P3) \
  TW_LD_RD(Z0, "v4", P0) TW_LD_RD(Z1, "v5", P1) TW_LD_RD(Z2, "v4", P2) TW_LD_RD(Z3, "v5", P3)
// the chains and popcounts of the four images whose words a set holds
#define TW_LD_CHAINS(Z0, Z1, Z2, Z3, C0, C1, C2, C3, C4, C5, C6, C7)          \
  "s_set_gpr_idx_on " Z0 ", 0x3\n\t" TW_LD_OPS(C0, C1)                        \
  "s_set_gpr_idx_idx " Z1 "\n\t" TW_LD_OPS(C2, C3)                            \
  "s_set_gpr_idx_idx " Z2 "\n\t" TW_LD_OPS(C4, C5)                            \
  "s_set_gpr_idx_idx " Z3 "\n\t" TW_LD_OPS(C6, C7) "s_set_gpr_idx_off\n\t"    \
  TW_LD_CNT(C0, C1) TW_LD_CNT(C2, C3) TW_LD_CNT(C4, C5) TW_LD_CNT(C6, C7)
#define TW_LD_ONE(Z)                                                          \
  TW_LD_RD(Z, "v4", "v[8:9]") "s_waitcnt lgkmcnt(0)\n\ts_set_gpr_idx_on " Z ", 0x3\n\t" \
  TW_LD_OPS("v8", "v9") "s_set_gpr_idx_off\n\t" TW_LD_CNT("v8", "v9")
#define TW_LD_W0 "s40", "s41", "s42", "s43"
#define TW_LD_W1 "s44", "s45", "s46", "s47"
#define TW_LD_N0 "s48", "s49", "s50", "s51"
#define TW_LD_SET_A "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15"
#define TW_LD_SET_B "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23"
#define TW_LD_PAIRS_A "v[8:9]", "v[10:11]", "v[12:13]", "v[14:15]"
#define TW_LD_PAIRS_B "v[16:17]", "v[18:19]", "v[20:21]", "v[22:23]"
#define TW_LD_X(M, ...) M(__VA_ARGS__)
#define TW_LD_W_FROM_N                                                        \
  "s_mov_b64 s[40:41], s[48:49]\n\ts_mov_b64 s[42:43], s[50:51]\n\t"          \
  "s_mov_b64 s[44:45], s[52:53]\n\ts_mov_b64 s[46:47], s[54:55]\n\t"
// rem: the images left (>= 1 on entry, 0 on exit); off: the byte offset of W's words from p
#define TW_LD_RUN                                                                          \
  "s_load_dwordx8 s[40:47], %[p], 0x0\n\ts_waitcnt lgkmcnt(0)\n\t"                         \
  "s_cmp_lt_u32 %[rem], 4\n\ts_cbranch_scc1 3f\n\t"                                        \
  TW_LD_X(TW_LD_READS, TW_LD_W0, TW_LD_PAIRS_A) "s_waitcnt lgkmcnt(0)\n\t"                 \
  "s_cmp_lt_u32 %[rem], 12\n\ts_cbranch_scc1 1f\n\t"                                       \
  "0:\n\t" /* >= 12 left: batches 0 and 1 and the next trip's batch 0 are whole */         \
  "s_load_dwordx8 s[48:55], %[p], %[off] offset:0x20\n\t"                                  \
  TW_LD_X(TW_LD_READS, TW_LD_W1, TW_LD_PAIRS_B) TW_LD_X(TW_LD_CHAINS, TW_LD_W0, TW_LD_SET_A) \
  "s_waitcnt lgkmcnt(0)\n\t"                                                               \
  TW_LD_X(TW_LD_READS, TW_LD_N0, TW_LD_PAIRS_A) TW_LD_X(TW_LD_CHAINS, TW_LD_W1, TW_LD_SET_B) \
  "s_waitcnt lgkmcnt(0)\n\t" TW_LD_W_FROM_N                                                \
  "s_add_u32 %[off], %[off], 32\n\ts_sub_u32 %[rem], %[rem], 8\n\t"                        \
  "s_cmp_ge_u32 %[rem], 12\n\ts_cbranch_scc1 0b\n\t"                                       \
  "1:\n\t" /* 4 .. 11 left, set A holds the words of W's batch 0 */                        \
  "s_cmp_lt_u32 %[rem], 8\n\ts_cbranch_scc1 2f\n\t"                                        \
  "s_load_dwordx8 s[48:55], %[p], %[off] offset:0x20\n\t"                                  \
  TW_LD_X(TW_LD_READS, TW_LD_W1, TW_LD_PAIRS_B) TW_LD_X(TW_LD_CHAINS, TW_LD_W0, TW_LD_SET_A) \
  "s_waitcnt lgkmcnt(0)\n\t" TW_LD_X(TW_LD_CHAINS, TW_LD_W1, TW_LD_SET_B) TW_LD_W_FROM_N   \
  "s_sub_u32 %[rem], %[rem], 8\n\ts_branch 3f\n\t"                                         \
  "2:\n\t" /* 4 .. 7 left */                                                               \
  TW_LD_X(TW_LD_CHAINS, TW_LD_W0, TW_LD_SET_A)                                             \
  "s_mov_b64 s[40:41], s[44:45]\n\ts_mov_b64 s[42:43], s[46:47]\n\t"                       \
  "s_sub_u32 %[rem], %[rem], 4\n\t"                                                        \
  "3:\n\t" /* 0 .. 3 left, their words in s40, s41, s42 */                                 \
  "s_cmp_eq_u32 %[rem], 0\n\ts_cbranch_scc1 4f\n\t" TW_LD_ONE("s40")                       \
  "s_cmp_eq_u32 %[rem], 1\n\ts_cbranch_scc1 4f\n\t" TW_LD_ONE("s41")                       \
  "s_cmp_eq_u32 %[rem], 2\n\ts_cbranch_scc1 4f\n\t" TW_LD_ONE("s42")                       \
  "4:\n\ts_mov_b32 %[rem], 0"
#define TW_LD_TAB(t16, t1)                                                    \
  "{v[24:39]}"(t16[0]), "{v40}"(t1[0]), "{v[42:57]}"(t16[1]), "{v58}"(t1[1])
#define TW_LD_CLOBBERS                                                                         \
  "scc", "v4", "v5", TW_LD_SET_A, TW_LD_SET_B, TW_LD_W0, TW_LD_W1, TW_LD_N0, "s52", "s53",     \
      "s54", "s55", "s56"

// One block's count of one (bag, x tile of two groups) on the LDS table.  lds: the byte address
// of the block's table of kClassLdsTableBytes (built by class_lds_build below, behind a
// barrier); pw: the tile's planes; zbag: the bag's class-ordered images (class_lds_encode);
// tab, cnt: the bag's run table and its entry count; next: an LDS counter, zero at the barrier,
// from which the block's waves draw runs — or null: wave wid of waves takes entries wid,
// wid + waves, ... (the striped assignment measured against the counter in DESIGN §4.1m).  ng:
// the tile's groups (1 or 2; a missing group's planes read as zero).  Returns the lane's count
// over the runs its wave took.
template <int NB, int K>
__device__ __forceinline__ unsigned long long bits_count_runs_lds(
    uint32_t lds, const uint32_t* __restrict__ pw, const uint32_t* __restrict__ zbag,
    const uint32_t* __restrict__ tab, int cnt, uint32_t* next, int lane, int ng, int wid = 0,
    int waves = 1) {
  constexpr int NL = NB - K, W = kClassWideBits, S = W * (kClassWideDigits - 1);
  static_assert(class_lds_fit(NL), "the table covers the low 8 planes of a 12-plane low field");
  typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
  const ConstWords ct = (ConstWords)(uintptr_t)tab;
  [[maybe_unused]] const ConstWords zc = (ConstWords)(uintptr_t)zbag;
  [[maybe_unused]] const uint32_t l8 = lds + 8u * (uint32_t)lane;
  ClassVec16 t16[kClassLdsGroups];
  uint32_t t1[kClassLdsGroups], acc[kClassLdsGroups] = {0u, 0u};
  uint32_t cg = 0;  // sum of len * popc(G) over the wave's runs
  for (int e = wid;; e += waves) {
    if (next != nullptr) {
      if (lane == 0) e = (int)atomicAdd(next, 1u);
      e = __builtin_amdgcn_readfirstlane(e);
    }
    if (e >= cnt) break;
    const ClassRun run = class_entry(ct[2 * e], ct[2 * e + 1]);
    // the class's G, P and E and the top digit's table under E (bits_count_span_wide's rebuild;
    // consecutive entries go to different waves: every run rebuilds)
    uint32_t ngp = 0;
    int ql = lane;  // (opaque per run: the reloads are not hoisted out of the loop)
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(ql));
#endif
#pragma unroll
    for (int r = 0; r < kClassLdsGroups; ++r) {
      uint32_t G, P, g[kClassWideEntries], tp[K], hp[W];
      const bool has = r < ng;  // wave-uniform
#pragma unroll
      for (int b = 0; b < K; ++b) tp[b] = has ? pw[(r * NB + NL + b) * 64 + ql] : 0u;
#pragma unroll
      for (int b = 0; b < W; ++b) hp[b] = has ? pw[(r * NB + S + b) * 64 + ql] : 0u;
      class_gp<K>(tp, run.cls, G, P);
      ngp = bits_popc_add(G, ngp);
      class_digit_table<W>(hp, class_equal_mask(G, P), g);
#pragma unroll
      for (int d = 0; d < (1 << W); ++d) t16[r][d] = g[d];
      t1[r] = g[1 << W];
    }
    cg += (uint32_t)run.len * ngp;  // the run's exact length
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t rem = (uint32_t)run.len, off = 0;  // >= 1: only non-empty classes have runs
    asm volatile(TW_LD_RUN
                 : [n0] "+v"(acc[0]), [n1] "+v"(acc[1]), [rem] "+s"(rem), [off] "+s"(off)
                 : [p] "s"(zc + run.z0), [l8] "v"(l8), TW_LD_TAB(t16, t1)
                 : TW_LD_CLOBBERS);
#endif
  }
  return (unsigned long long)cg + acc[0] + acc[1];
}

// The block's table: every wave builds digit tables 0 and 1 of both groups from the low 8
// planes; wave w (of 16) writes the 16 entries with d1 = w, one 8-byte store per entry and lane.
// The caller's barrier follows.  tab2: the table as {group 0, group 1} pairs, [entry][lane].
template <int NB>
__device__ __forceinline__ void class_lds_build(uint2* tab2, const uint32_t* __restrict__ pw,
                                                int wid, int lane, int ng) {
  ClassWideTables t[kClassLdsGroups];
#pragma unroll
  for (int r = 0; r < kClassLdsGroups; ++r) {
    uint32_t low[kClassWideNL];
#pragma unroll
    for (int b = 0; b < kClassLdsBits; ++b) low[b] = r < ng ? pw[(r * NB + b) * 64 + lane] : 0u;
#pragma unroll
    for (int b = kClassLdsBits; b < kClassWideNL; ++b) low[b] = 0u;
    class_wide_tables_one<0>(low, ~0u, t[r]);
    class_wide_tables_one<1>(low, ~0u, t[r]);
  }
  uint32_t a[kClassLdsGroups] = {0u, 0u}, b[kClassLdsGroups] = {0u, 0u};  // T1[w], T1[w + 1]
#pragma unroll
  for (int d = 0; d < kClassWideEntries; ++d)
#pragma unroll
    for (int r = 0; r < kClassLdsGroups; ++r) {
      a[r] = wid == d ? t[r].g[1][d] : a[r];
      b[r] = wid + 1 == d ? t[r].g[1][d] : b[r];
    }
#pragma unroll
  for (int d0 = 0; d0 < 16; ++d0)
    tab2[(wid * 16 + d0) * 64 + lane] =
        make_uint2(bits_carry(a[0], b[0], t[0].g[0][d0]), bits_carry(a[1], b[1], t[1].g[0][d0]));
}
#endif  // __HIPCC__

}  // namespace tw
