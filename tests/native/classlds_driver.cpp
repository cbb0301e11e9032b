// Host check of the LDS-table form of the class loop (csrc/chainclass.h class_lds_encode /
// class_lds_decode, class_lds_entry, class_gt32_lds, class_lds_runs), no GPU:
// tests/test_classlds_host.py compiles it under ASan + UBSan and runs it.
//  * encoding: class_lds_encode(zc) has its top digit < 16 in bits [3:0], an offset that is a
//    multiple of 512 and at most 255 * 512 in bits [16:9] and no other bit set; decode
//    reproduces the low 12 bits; the offset and top digit of ANY 32-bit word stay in range;
//  * table: 256 entries of two groups end at byte 131072, the last lane of the last entry ends
//    there, and the table with the epilogue's words fits the CU's 160 KiB;
//  * words: for (NB, K) = (16, 4), (18, 6), (20, 8), plane words random, all 0 (padded x slots),
//    all ones, one x per word, all x at the bound, all x equal to z and one off z, and z images
//    0, the bound, and m 16^j + {-1, 0, 1} for every j and m = 1 .. 15: class_lds_entry of the
//    encoded word's low byte, carried through the top-digit step (class_gt32_lds), equals
//    class_gt32_wide and class_gt32_masked word for word and the integer compare; a zero-plane
//    group counts nothing, whatever the class;
//  * plan: the launch's regions are those of the wide plan (the launcher only sets dbits), the
//    loop's over-read stays inside the count region, and class_lds_runs follows the setting,
//    the digit width, the tile and the swap.
// Prints one "ok <name>" line per check and exits non-zero at the first mismatch.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "chainclass.h"

using namespace tw;

static int fail(const char* what, long long a, long long b, long long c, long long d) {
  std::printf("FAIL %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
  return 1;
}

static int check_encoding(std::mt19937& g) {
  std::vector<uint32_t> zs = {0u, ~0u, 0xFFFu, ~0xFFFu, 1u, 0x80000000u, 0x55555555u, 0xAAAAAAAAu};
  for (int i = 0; i < 4000; ++i) zs.push_back(g());
  for (uint32_t v = 0; v <= 0xFFFu; ++v) zs.push_back(v), zs.push_back(v | 0xFFFFF000u);
  for (uint32_t zc : zs) {
    const uint32_t w = class_lds_encode(zc);
    if ((w & 0xFFu) >= 16u) return fail("index byte >= 16", zc, w, 0, 0);
    if (class_lds_top(w) != ((zc >> 8) & 15u)) return fail("top digit", zc, w, 0, 0);
    const uint32_t off = class_lds_offset(w);
    if (off % 512u || off > 255u * 512u) return fail("offset", zc, w, off, 0);
    if (off != (w & 0x1FE00u)) return fail("offset is not the masked word", zc, w, off, 0);
    if (off / 512u != (zc & 255u)) return fail("offset is not the low byte's entry", zc, w, off, 0);
    if (w & ~(0x1FE00u | 0xFu)) return fail("another bit set", zc, w, 0, 0);
    if (class_lds_decode(w) != (zc & 0xFFFu)) return fail("decode", zc, w, class_lds_decode(w), 0);
  }
  for (int i = 0; i < 100000; ++i) {  // any word: the loop's mask keeps the address in the table
    const uint32_t w = g();
    if (class_lds_offset(w) + 63u * 8u + 8u > (uint32_t)kClassLdsTableBytes) return fail("offset of any word", w, 0, 0, 0);
    if (class_lds_top(w) >= 16u) return fail("top of any word", w, 0, 0, 0);
  }
  std::printf("ok encoding\n");
  return 0;
}

static int check_table() {
  if (kClassLdsBits != 8 || kClassLdsGroups != 2 || kClassLdsEntries != 256 || kClassLdsEntryBytes != 512)
    return fail("constants", kClassLdsBits, kClassLdsGroups, kClassLdsEntries, kClassLdsEntryBytes);
  if (kClassLdsTableBytes != 131072) return fail("table bytes", kClassLdsTableBytes, 0, 0, 0);
  if (255 * 512 + 63 * 8 + 8 != kClassLdsTableBytes) return fail("last lane of the last entry", 0, 0, 0, 0);
  if (kClassLdsTableBytes + 16 * 8 + 8 > 160 * 1024) return fail("the CU's LDS", 0, 0, 0, 0);
  if (kClassLdsBits == kClassWideBits || kClassLdsBits == kClassDigitBits) return fail("dbits value", 0, 0, 0, 0);
  for (int nl = 1; nl <= 24; ++nl)
    if (class_lds_fit(nl) != (nl == 12)) return fail("lds fit", nl, 0, 0, 0);
  std::printf("ok table\n");
  return 0;
}

template <int NB>
static void planes_of(const uint32_t (&img)[32], uint32_t (&plane)[NB]) {
  uint32_t a[32];
  for (int k = 0; k < 32; ++k) a[k] = img[k];
  bits_transpose32(a);
  for (int b = 0; b < NB; ++b) plane[b] = a[b];
}

// one (group, z): the table form against the wide form, the masked form and the compare
template <int NB, int K>
static int check_word(const uint32_t (&img)[32], uint32_t z, bool padded) {
  constexpr int NL = NB - K;
  static_assert(class_lds_fit(NL), "the table form takes NB - K = 12");
  const uint32_t zc = ~z, D = class_of(zc, NB, K);
  uint32_t plane[NB], low[NL], low8[NL], top[K], masked[NL], G, P;
  planes_of<NB>(img, plane);
  for (int b = 0; b < NL; ++b) low[b] = plane[b];
  for (int b = 0; b < NL; ++b) low8[b] = b < kClassLdsBits ? plane[b] : 0u;  // (what the block reads)
  for (int b = 0; b < K; ++b) top[b] = plane[NL + b];
  class_gp<K>(top, D, G, P);
  const uint32_t E = class_equal_mask(G, P);
  class_mask_planes<NL>(low, E, masked);
  ClassWideTables t, tl{};
  class_wide_tables(low, E, t);
  class_wide_tables_one<0>(low8, ~0u, tl);  // the block's tables: digits 0 and 1 under ~0u
  class_wide_tables_one<1>(low8, ~0u, tl);
  uint32_t hp[kClassWideBits], g2[kClassWideEntries];  // the per-class rebuild: the top digit under E
  for (int b = 0; b < kClassWideBits; ++b) hp[b] = plane[8 + b];
  class_digit_table<kClassWideBits>(hp, E, g2);
  for (int d = 0; d < kClassWideEntries; ++d)
    if (g2[d] != t.g[2][d]) return fail("rebuilt top table", NB, K, d, g2[d]);
  const uint32_t word = class_lds_encode(zc);
  const uint32_t c_low = class_lds_entry(tl, class_lds_offset(word) / kClassLdsEntryBytes);
  // the wide loop's carry after its first two steps
  const uint32_t d0 = zc & 15u, d1 = (zc >> 4) & 15u;
  if (c_low != bits_carry(t.g[1][d1], t.g[1][d1 + 1], t.g[0][d0])) return fail("entry", NB, K, z, c_low);
  const ClassMasked got = class_gt32_lds(c_low, g2, G, word);
  const ClassMasked wide = class_gt32_wide(t, G, class_wide_encode(zc));
  const ClassMasked want = class_gt32_masked<NL>(masked, G, zc);
  if (got.constant != wide.constant || got.word != wide.word) return fail("wide lookup", NB, K, z, got.word);
  if (got.constant != want.constant || got.word != want.word) return fail("masked planes", NB, K, z, got.word);
  uint32_t gt = 0;
  for (int k = 0; k < 32; ++k) gt |= (uint32_t)(img[k] > z) << k;
  if ((got.constant | got.word) != gt || (got.constant & got.word)) return fail("compare", NB, K, z, gt);
  if (padded && (got.constant | got.word | c_low)) return fail("zero-plane group counted", NB, K, z, got.word);
  return 0;
}

template <int NB, int K>
static int check_k(std::mt19937& g) {
  constexpr int NL = NB - K;
  const uint32_t top = (uint32_t)(((uint64_t)1 << NB) - 1), lowmask = (1u << NL) - 1u;
  const uint32_t bound = top < 1000000u ? top : 1000000u;
  std::uniform_int_distribution<uint32_t> any(0, top);
  std::vector<uint32_t> zs = {0u, 1u, top, top - 1, bound, lowmask, lowmask + 1, top & ~lowmask};
  for (uint64_t e = 1; e <= top; e *= 16)  // m 16^j + {-1, 0, 1}: every j, m = 1 .. 15
    for (uint64_t m = 1; m < 16; ++m)
      for (int d = -1; d <= 1; ++d) {
        const uint64_t v = m * e + (uint64_t)(int64_t)d;
        if (v <= top) zs.push_back((uint32_t)v);
      }
  for (int i = 0; i < 40; ++i) zs.push_back(any(g));
  long long words = 0;
  for (uint32_t z : zs) {
    uint32_t img[32];
    for (int round = 0; round < 6; ++round) {  // random images; half of them share z's top field
      for (int k = 0; k < 32; ++k)
        img[k] = (g() & 1) ? any(g) : ((z & ~lowmask) | (any(g) & lowmask));
      if (check_word<NB, K>(img, z, false)) return 1;
    }
    for (int k = 0; k < 32; ++k) img[k] = z;  // all x equal to z
    if (check_word<NB, K>(img, z, false)) return 1;
    for (int k = 0; k < 32; ++k) {  // equal in the top field, -1 / 0 / +1 in the low field
      const uint32_t l = z & lowmask, d = (uint32_t)(k % 3);
      const uint32_t nl = d == 0 ? (l > 0 ? l - 1 : l) : d == 1 ? l : (l < lowmask ? l + 1 : l);
      img[k] = (z & ~lowmask) | nl;
    }
    if (check_word<NB, K>(img, z, false)) return 1;
    for (int k = 0; k < 32; ++k) img[k] = 0;  // plane words all 0: a tile's missing group
    if (check_word<NB, K>(img, z, true)) return 1;
    for (uint32_t b : {top, bound}) {  // plane words all ones / all x at the bound
      for (int k = 0; k < 32; ++k) img[k] = b;
      if (check_word<NB, K>(img, z, false)) return 1;
    }
    for (int one = 0; one < 32; one += 7) {  // one x per word
      for (int k = 0; k < 32; ++k) img[k] = k == one ? any(g) : 0u;
      if (check_word<NB, K>(img, z, false)) return 1;
    }
    words += 16;
  }
  std::printf("ok words NB=%d k=%d (%lld x 32 pairs)\n", NB, K, words);
  return 0;
}

static int check_plan() {
  const int64_t shapes[][3] = {{15625, 15625, 1280}, {15625, 15625, 64}, {31, 1, 1},
                               {4101, 130, 6},       {2048, 64, 33},     {1, 777, 3}};
  const int nbk[][2] = {{16, 4}, {18, 6}, {20, 8}};
  for (const auto& sh : shapes)
    for (const auto& q : nbk)
      for (int R : {1, 2})
        for (int swap : {0, 2})
          for (int64_t zc : {(int64_t)0, (int64_t)8, (int64_t)600}) {
            const int64_t nx = sh[0], nz = sh[1], bags = sh[2];
            const int nb = q[0], k = q[1];
            const int64_t sized = planes_work_words(nx, nz, bags, nb) + class_work_words(nz, bags);
            const PlanesPlan p = planes_plan(nx, nz, bags, R, zc, swap);
            const ClassPlan wide = class_plan(p, nx, nz, bags, nb, k, 8);
            ClassPlan lds = class_plan(p, nx, nz, bags, nb, k, 8);
            lds.digits = nb - k, lds.dbits = kClassLdsBits;  // (as the launcher does)
            if (lds.off_zs != wide.off_zs || lds.off_cnt != wide.off_cnt ||
                lds.off_tab != wide.off_tab || lds.zs_stride != wide.zs_stride ||
                lds.cap != wide.cap || class_plan_end(lds, bags) != class_plan_end(wide, bags))
              return fail("regions differ from the wide plan", nb, k, R, zc);
            if (class_plan_end(lds, bags) > sized) return fail("tables leave the workspace", nb, k, R, zc);
            const int64_t last = lds.off_zs + (bags - 1) * lds.zs_stride + nz + kClassLdsOverReadWords;
            if (last > lds.off_tab) return fail("over-read leaves the count region", nb, k, last, lds.off_tab);
            const bool fits = R == 2 && p.tiles_s * p.schunks == 0;
            if (class_lds_runs(1, kClassWideBits, p, bags)) return fail("runs under off", nb, k, R, swap);
            if (class_lds_runs(2, kClassWideBits, p, bags) != fits) return fail("runs under on", nb, k, R, swap);
            if (class_lds_runs(2, kClassDigitBits, p, bags)) return fail("runs under four digits", nb, k, R, swap);
            if (class_lds_runs(0, kClassWideBits, p, bags) !=
                (fits && class_lds_auto(bags * p.tiles_x)))
              return fail("automatic rule", nb, k, R, swap);
          }
  // the automatic rule at the sweep's block counts: off where the form lost
  const int64_t on[] = {192, 256, 384, 448, 512, 576, 640, 768, 832, 1024, 1280, 5120, 1 << 20};
  const int64_t off[] = {0, 1, 25, 128, 191, 257, 320, 383, 513, 575};
  for (int64_t b : on)
    if (!class_lds_auto(b)) return fail("automatic rule off", b, 0, 0, 0);
  for (int64_t b : off)
    if (class_lds_auto(b)) return fail("automatic rule on", b, 0, 0, 0);
  std::printf("ok plan\n");
  return 0;
}

int main() {
  std::mt19937 g(20261021u);
  if (check_encoding(g) || check_table() || check_plan()) return 1;
  if (check_k<16, 4>(g) || check_k<18, 6>(g) || check_k<20, 8>(g)) return 1;
  std::printf("done\n");
  return 0;
}
