// Host check of the wide-digit split of the class loop (csrc/chainclass.h class_wide_encode /
// class_wide_of, class_wide_tables, class_gt32_wide, the wide register map), no
// GPU: tests/test_classwide_host.py compiles it under ASan + UBSan and runs it.
//  * map: a group's tables are 16 + 17 + 17 = 50 registers, digit 0 at + 0, digits 1 and 2 at
//    + 16 and + 33, group g from v(24 + 50 g), two groups end at v123; the wide digits fit
//    exactly the 12-plane low field, and class_digit_bits answers 4 only there;
//  * encoding: every digit of class_wide_encode(zc) is < 16, byte 3 is 0, a byte holds nothing
//    but its digit, the digits reproduce the low 12 bits, and class_wide_of of ANY 32-bit word
//    is < 16;
//  * words: for (NB, K) = (16, 4), (18, 6), (20, 8), plane words random, all 0 (padded x slots),
//    all ones, one x per word, all x at the bound, all x equal to z and one off z, and z images
//    0, the bound, and m 16^j + {-1, 0, 1} for every j and m = 1 .. 15: class_gt32_wide equals
//    class_gt32_masked word for word — constant and word — equals class_gt32_digits, equals the
//    integer compare, and a padded x slot counts nothing;
//  * tables: entry 0 is 0, entry 16 is E (ones below the top digit), the entries are nested and
//    every top-digit entry is a subset of E;
//  * plan: class_plan's regions are disjoint, inside the sized workspace, the over-read of a
//    batch load stays inside the count region, and every region is where and as large as the
//    four-digit launch's (the plan does not depend on the digit width).
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

static int check_map() {
  if (kClassWideDigits != 3 || kClassWideBits != 4 || kClassWideNL != 12 || kClassWideEntries != 17)
    return fail("split constants", kClassWideDigits, kClassWideBits, kClassWideNL, kClassWideEntries);
  if (class_wide_table_regs() != 50 || kClassWideGroupRegs != 50)
    return fail("regs per group", class_wide_table_regs(), kClassWideGroupRegs, 0, 0);
  if (class_wide_reg(0, 0) != 0 || class_wide_reg(0, 15) != 15 || class_wide_reg(1, 0) != 16 ||
      class_wide_reg(1, 16) != 32 || class_wide_reg(2, 0) != 33 || class_wide_reg(2, 16) != 49)
    return fail("flat registers", class_wide_reg(1, 0), class_wide_reg(2, 0), class_wide_reg(2, 16), 0);
  if (class_wide_group_base(0) != 24 || class_wide_group_base(1) != 74)
    return fail("group bases", class_wide_group_base(0), class_wide_group_base(1), 0, 0);
  if (kClassWideMaxR != 2 || class_wide_last_reg(kClassWideMaxR) != 123)
    return fail("map end", kClassWideMaxR, class_wide_last_reg(kClassWideMaxR), 0, 0);
  // the digits' register ranges of one group are disjoint and in order
  for (int j = 0; j + 1 < kClassWideDigits; ++j)
    if (class_wide_reg(j, j == 0 ? 15 : 16) + 1 != class_wide_reg(j + 1, 0)) return fail("ranges", j, 0, 0, 0);
  for (int nl = 1; nl <= 24; ++nl)
    if (class_wide_fit(nl) != (nl == 12)) return fail("wide fit", nl, 0, 0, 0);
  for (int nb : {16, 18, 20, 22, 24})
    for (int k = 1; k <= 8; ++k) {
      const bool wide = nb - k == 12;
      if (class_digit_bits(nb, k, 4) != (wide ? 4 : 3)) return fail("bits under 4", nb, k, 0, 0);
      if (class_digit_bits(nb, k, 3) != 3) return fail("bits under 3", nb, k, 0, 0);
      if (class_digit_bits(nb, k, 0) != (wide && kClassDigitsAuto == 4 ? 4 : 3)) return fail("bits under 0", nb, k, 0, 0);
    }
  std::printf("ok map\n");
  return 0;
}

static int check_encoding(std::mt19937& g) {
  std::vector<uint32_t> zs = {0u, ~0u, 0xFFFu, ~0xFFFu, 1u, 0x80000000u, 0x55555555u, 0xAAAAAAAAu};
  for (int i = 0; i < 4000; ++i) zs.push_back(g());
  for (uint32_t v = 0; v <= 0xFFFu; ++v) zs.push_back(v), zs.push_back(v | 0xFFFFF000u);
  for (uint32_t zc : zs) {
    const uint32_t w = class_wide_encode(zc);
    if (w >> 24) return fail("byte 3 not zero", zc, w, 0, 0);
    uint32_t back = 0;
    for (int j = 0; j < kClassWideDigits; ++j) {
      const uint32_t d = class_wide_of(w, j);
      if (d >= 16u) return fail("digit >= 16", zc, j, d, 0);
      if (((w >> (8 * j)) & 0xFFu) != d) return fail("byte holds more than the digit", zc, j, w, 0);
      back |= d << (kClassWideBits * j);
    }
    if (back != (zc & 0xFFFu)) return fail("digits do not reproduce the low bits", zc, back, w, 0);
  }
  for (uint32_t w : {0xFFFFFFFFu, 0x10101010u, 0xF0F0F0F0u, 0x12345678u, 0x00FF11FFu})
    for (int j = 0; j < 4; ++j)
      if (class_wide_of(w, j) >= 16u) return fail("wide_of >= 16", w, j, 0, 0);
  for (int i = 0; i < 100000; ++i) {
    const uint32_t w = g();
    for (int j = 0; j < kClassWideDigits; ++j)
      if (class_wide_of(w, j) >= 16u) return fail("wide_of >= 16", w, j, 0, 0);
  }
  std::printf("ok encoding\n");
  return 0;
}

template <int NB>
static void planes_of(const uint32_t (&img)[32], uint32_t (&plane)[NB]) {
  uint32_t a[32];
  for (int k = 0; k < 32; ++k) a[k] = img[k];
  bits_transpose32(a);
  for (int b = 0; b < NB; ++b) plane[b] = a[b];
}

// one (group, z): the wide form against the masked form, the four-digit form and the compare
template <int NB, int K>
static int check_word(const uint32_t (&img)[32], uint32_t z, bool padded) {
  constexpr int NL = NB - K;
  static_assert(class_wide_fit(NL), "the wide digits take NB - K = 12");
  const uint32_t zc = ~z, D = class_of(zc, NB, K);
  uint32_t plane[NB], low[NL], top[K], masked[NL], G, P;
  planes_of<NB>(img, plane);
  for (int b = 0; b < NL; ++b) low[b] = plane[b];
  for (int b = 0; b < K; ++b) top[b] = plane[NL + b];
  class_gp<K>(top, D, G, P);
  const uint32_t E = class_equal_mask(G, P);
  class_mask_planes<NL>(low, E, masked);
  ClassWideTables t;
  class_wide_tables(low, E, t);
  for (int j = 0; j < kClassWideDigits; ++j) {
    const uint32_t full = j == kClassWideDigits - 1 ? E : ~0u;
    if (t.g[j][0] != 0u) return fail("entry 0", NB, K, j, t.g[j][0]);
    if (t.g[j][16] != full) return fail("entry 16", NB, K, j, t.g[j][16]);
    for (int d = 0; d < 16; ++d) {
      if (t.g[j][d] & ~t.g[j][d + 1]) return fail("entries not nested", NB, K, j, d);
      if (t.g[j][d] & ~full) return fail("top entry outside E", NB, K, j, d);
    }
  }
  const ClassMasked want = class_gt32_masked<NL>(masked, G, zc);
  const ClassMasked got = class_gt32_wide(t, G, class_wide_encode(zc));
  if (got.constant != want.constant) return fail("constant", NB, K, z, got.constant);
  if (got.word != want.word) return fail("word", NB, K, z, got.word);
  ClassDigitTables t3;
  class_digit_tables<NL>(low, E, t3);
  const ClassMasked four = class_gt32_digits(t3, G, class_digit_encode(zc, NL));
  if (got.constant != four.constant || got.word != four.word) return fail("four-digit lookup", NB, K, z, four.word);
  uint32_t gt = 0;
  for (int k = 0; k < 32; ++k) gt |= (uint32_t)(img[k] > z) << k;
  if ((got.constant | got.word) != gt || (got.constant & got.word)) return fail("compare", NB, K, z, gt);
  if (padded && (got.constant | got.word)) return fail("padded x slot counted", NB, K, z, got.word);
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
    for (int k = 0; k < 32; ++k) img[k] = 0;  // plane words all 0: padded x slots
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

// The plan of a wide launch is the four-digit launch's plan: class_plan does not see the digit
// width (the launcher sets dbits on its result), so the regions must be those of the sizing
// call — disjoint, in order, inside the workspace, the batch over-read inside the count region.
static int check_plan() {
  const int64_t shapes[][3] = {{15625, 15625, 1280}, {15625, 15625, 64}, {31, 1, 1},
                               {4101, 130, 6},       {2048, 64, 33},     {1, 777, 3}};
  const int nbk[][2] = {{16, 4}, {18, 6}, {20, 8}};
  for (const auto& sh : shapes)
    for (const auto& q : nbk)
      for (int R : {1, 2})
        for (int64_t zc : {(int64_t)0, (int64_t)8, (int64_t)600})
          for (int64_t runs : {(int64_t)1, (int64_t)8}) {
            const int64_t nx = sh[0], nz = sh[1], bags = sh[2];
            const int nb = q[0], k = q[1];
            const int64_t sized = planes_work_words(nx, nz, bags, nb) + class_work_words(nz, bags);
            const PlanesPlan p = planes_plan(nx, nz, bags, R, zc, 0);
            const ClassPlan four = class_plan(p, nx, nz, bags, nb, k, runs);
            ClassPlan wide = class_plan(p, nx, nz, bags, nb, k, runs);
            if (four.dbits != 0) return fail("class_plan sets dbits", nb, k, four.dbits, 0);
            wide.digits = nb - k, wide.dbits = kClassWideBits;  // (as the launcher does)
            if (wide.off_zs != four.off_zs || wide.off_cnt != four.off_cnt ||
                wide.off_tab != four.off_tab || wide.zs_stride != four.zs_stride ||
                wide.cap != four.cap || wide.per_bag != four.per_bag || wide.span != four.span ||
                class_plan_end(wide, bags) != class_plan_end(four, bags))
              return fail("regions differ from the four-digit plan", nb, k, R, zc);
            if (wide.off_zs != planes_work_words(nx, nz, bags, nb)) return fail("zs after the planes", nb, k, R, zc);
            if (wide.zs_stride < nz || wide.off_zs + bags * wide.zs_stride != wide.off_cnt)
              return fail("zs region", nb, k, R, zc);
            if (wide.off_tab - wide.off_cnt < 64 || wide.off_tab - wide.off_cnt < bags)
              return fail("count region", nb, k, R, zc);
            const int64_t last = wide.off_zs + (bags - 1) * wide.zs_stride + nz + 4;
            if (last > wide.off_tab) return fail("over-read leaves the count region", nb, k, last, wide.off_tab);
            if (class_plan_end(wide, bags) > sized) return fail("tables leave the workspace", nb, k, R, zc);
          }
  std::printf("ok plan\n");
  return 0;
}

int main() {
  std::mt19937 g(20261020u);
  if (check_map() || check_encoding(g) || check_plan()) return 1;
  if (check_k<16, 4>(g) || check_k<18, 6>(g) || check_k<20, 8>(g)) return 1;
  std::printf("done\n");
  return 0;
}
