// Host check of the digit-table form of the class loop (csrc/chainclass.h class_digit_table,
// class_digit_tables, class_digit_encode / class_digit_of, class_gt32_digits), no
// GPU: tests/test_classdigit_host.py compiles and runs it.
//  * split: for every low-field width the tables take, the digit widths are 1 .. 3, add up to
//    NL, the shifts are their running sum, and the table registers of a group fit the device
//    loop's map of 36 (35 at NL = 12); (NB, K) pairs the tables take are exactly those with
//    4 <= NB - K <= 12;
//  * encoding: class_digit_of(class_digit_encode(zc)) reproduces the low NL bits of zc for
//    random and extreme zc, and class_digit_of of ANY word (0xFFFFFFFF included) is < 8;
//  * words: for every such (NB, K) of NB in {16, 18, 20} and random and extreme plane words
//    (all 0, all ones, one x per word, all x equal to z, x one off z in the low field, all x at
//    the bound) and every z, class_gt32_digits equals class_gt32_masked word for word, constant
//    and word, and a padded x slot (plane words 0) contributes nothing;
//  * tables: entry 0 is 0, entry 2^w is E (ones below the top digit), the entries are nested
//    (G_d subset of G_(d+1)) and every top-digit entry is a subset of E;
//  * layout: the regions of a launch are disjoint and inside the sized workspace, and the four
//    words a whole batch's load reads past the last run of the last bag lie inside the count
//    region, for the bench's shape and small ones.
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

static int check_split() {
  for (int nl = 1; nl <= 24; ++nl) {
    if (class_digits_fit(nl) != (nl >= 4 && nl <= 12)) return fail("fit", nl, 0, 0, 0);
    if (!class_digits_fit(nl)) continue;
    int sum = 0, regs = 0;
    for (int j = 0; j < kClassDigits; ++j) {
      const int w = class_digit_width(nl, j);
      if (w < 1 || w > kClassDigitBits) return fail("digit width", nl, j, w, 0);
      if (class_digit_shift(nl, j) != sum) return fail("digit shift", nl, j, sum, 0);
      if (j > 0 && w > class_digit_width(nl, j - 1)) return fail("wider above", nl, j, w, 0);
      sum += w;
      regs += (1 << w) + (j > 0);
    }
    if (sum != nl) return fail("widths do not add up", nl, sum, 0, 0);
    if (class_digit_table_regs(nl) != regs || regs > 36) return fail("table regs", nl, regs, 0, 0);
  }
  if (class_digit_table_regs(12) != 35) return fail("regs at NL 12", class_digit_table_regs(12), 0, 0, 0);
  if (class_digit_table_regs(8) != 4 + 3 * 5) return fail("regs at NL 8", class_digit_table_regs(8), 0, 0, 0);
  std::printf("ok split\n");
  return 0;
}

static int check_encoding(std::mt19937& g) {
  for (int nl = 4; nl <= 12; ++nl) {
    const uint32_t lowmask = (1u << nl) - 1u;
    std::vector<uint32_t> zs = {0u, ~0u, lowmask, ~lowmask, 1u, 0x80000000u, 0x55555555u, 0xAAAAAAAAu};
    for (int i = 0; i < 2000; ++i) zs.push_back(g());
    for (uint32_t v = 0; v <= lowmask; v += 1 + (lowmask > 600 ? 5 : 0)) zs.push_back(v);
    for (uint32_t zc : zs) {
      const uint32_t w = class_digit_encode(zc, nl);
      uint32_t back = 0;
      for (int j = 0; j < kClassDigits; ++j) {
        const uint32_t d = class_digit_of(w, j);
        if (d >= (1u << class_digit_width(nl, j))) return fail("digit out of its width", nl, zc, j, d);
        if (((w >> (8 * j)) & 0xFFu) != d) return fail("byte holds more than the digit", nl, zc, j, w);
        back |= d << class_digit_shift(nl, j);
      }
      if (back != (zc & lowmask)) return fail("digits do not reproduce the low bits", nl, zc, back, w);
    }
  }
  for (uint32_t w : {0xFFFFFFFFu, 0x08080808u, 0xF8F8F8F8u, 0x12345678u})
    for (int j = 0; j < kClassDigits; ++j)
      if (class_digit_of(w, j) >= (1u << kClassDigitBits)) return fail("digit_of >= 8", w, j, 0, 0);
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

// one (group, z): the digit form against the masked form, and the tables' own properties
template <int NB, int K>
static int check_word(const uint32_t (&img)[32], uint32_t z, bool padded) {
  constexpr int NL = NB - K;
  const uint32_t zc = ~z, D = class_of(zc, NB, K);
  uint32_t plane[NB], low[NL], top[K], masked[NL], G, P;
  planes_of<NB>(img, plane);
  for (int b = 0; b < NL; ++b) low[b] = plane[b];
  for (int b = 0; b < K; ++b) top[b] = plane[NL + b];
  class_gp<K>(top, D, G, P);
  const uint32_t E = class_equal_mask(G, P);
  class_mask_planes<NL>(low, E, masked);
  ClassDigitTables t;
  class_digit_tables<NL>(low, E, t);
  for (int j = 0; j < kClassDigits; ++j) {
    const int n = 1 << class_digit_width(NL, j);
    const uint32_t full = j == kClassDigits - 1 ? E : ~0u;
    if (t.g[j][0] != 0u) return fail("entry 0", NB, K, j, t.g[j][0]);
    if (t.g[j][n] != full) return fail("entry 2^w", NB, K, j, t.g[j][n]);
    for (int d = 0; d < n; ++d) {
      if (t.g[j][d] & ~t.g[j][d + 1]) return fail("entries not nested", NB, K, j, d);
      if (t.g[j][d] & ~full) return fail("top entry outside E", NB, K, j, d);
    }
  }
  const ClassMasked want = class_gt32_masked<NL>(masked, G, zc);
  const ClassMasked got = class_gt32_digits(t, G, class_digit_encode(zc, NL));
  if (got.constant != want.constant) return fail("constant", NB, K, z, got.constant);
  if (got.word != want.word) return fail("word", NB, K, z, got.word);
  uint32_t gt = 0;
  for (int k = 0; k < 32; ++k) gt |= (uint32_t)(img[k] > z) << k;
  if ((got.constant | got.word) != gt || (got.constant & got.word)) return fail("compare", NB, K, z, gt);
  if (padded && (got.constant | got.word)) return fail("padded x slot counted", NB, K, z, got.word);
  return 0;
}

template <int NB, int K>
static int check_k(std::mt19937& g) {
  constexpr int NL = NB - K;
  if constexpr (!class_digits_fit(NL)) {
    std::printf("ok skip NB=%d k=%d (form 2)\n", NB, K);
    return 0;
  } else {
  const uint32_t top = (uint32_t)(((uint64_t)1 << NB) - 1), lowmask = (1u << NL) - 1u;
  const uint32_t bound = top < 1000000u ? top : 1000000u;
  std::uniform_int_distribution<uint32_t> any(0, top);
  std::vector<uint32_t> zs = {0u, 1u, top, top - 1, bound, lowmask, lowmask + 1, top & ~lowmask};
  for (int j = 0; j <= kClassDigits; ++j) {  // every digit boundary of the low field
    const uint32_t e = 1u << (j < kClassDigits ? class_digit_shift(NL, j) : NL);
    for (uint32_t m = 1; m < 8; m += 3)
      for (int d = -1; d <= 1; ++d) zs.push_back((m * e + (uint32_t)d) & top);
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
}

template <int NB>
static int check_nb(std::mt19937& g) {
  return check_k<NB, 1>(g) || check_k<NB, 2>(g) || check_k<NB, 3>(g) || check_k<NB, 4>(g) ||
         check_k<NB, 5>(g) || check_k<NB, 6>(g) || check_k<NB, 7>(g) || check_k<NB, 8>(g);
}

// The regions of a launch: disjoint, inside the sized workspace, and the over-read of the last
// run of the last bag (a whole batch's load: up to 4 words past the run's end) inside the
// count region.  The size does not depend on the plan or the class bits.
static int check_layout() {
  const int64_t shapes[][3] = {{15625, 15625, 1280}, {15625, 15625, 64}, {31, 1, 1},
                               {4101, 130, 6},       {2048, 64, 33},     {1, 777, 3}};
  for (const auto& sh : shapes) {
    const int64_t nx = sh[0], nz = sh[1], bags = sh[2];
    for (int nb : {16, 18, 20, 22, 24}) {
      const int64_t sized = planes_work_words(nx, nz, bags, nb) + class_work_words(nz, bags);
      for (int k = 1; k <= 8; ++k)
        for (int R : {1, 2, 3, 4})
          for (int64_t zc : {(int64_t)0, (int64_t)8, (int64_t)600}) {
            const PlanesPlan p = planes_plan(nx, nz, bags, R, zc, 0);
            const ClassPlan c = class_plan(p, nx, nz, bags, nb, k);
            if (c.off_zs != planes_work_words(nx, nz, bags, nb)) return fail("zs after the planes", nb, k, R, zc);
            const int64_t zs_end = c.off_zs + bags * c.zs_stride;
            if (c.zs_stride < nz || zs_end != c.off_cnt) return fail("zs region", nb, k, R, zc);
            if (c.off_tab - c.off_cnt < 64 || c.off_tab - c.off_cnt < bags) return fail("count region", nb, k, R, zc);
            // last run of the last bag ends at most at the bag's stride: + 4 words over-read
            const int64_t last = c.off_zs + (bags - 1) * c.zs_stride + nz + 4;
            if (last > c.off_tab) return fail("over-read leaves the count region", nb, k, last, c.off_tab);
            if (class_plan_end(c, bags) > sized) return fail("tables leave the workspace", nb, k, R, zc);
          }
    }
  }
  std::printf("ok layout\n");
  return 0;
}

int main() {
  std::mt19937 g(20261020u);
  if (check_split() || check_encoding(g) || check_layout()) return 1;
  if (check_nb<16>(g) || check_nb<18>(g) || check_nb<20>(g)) return 1;
  static_assert(!class_digits_fit(22 - 8) && !class_digits_fit(24 - 8), "NB >= 22: form 2");
  std::printf("done\n");
  return 0;
}
