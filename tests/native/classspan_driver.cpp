// Host check of the span items of the class count (csrc/chainclass.h class_span_clamp,
// class_spans, class_span_entries, class_span_item, class_span_auto, class_plan's span; DESIGN
// §4.1j), no GPU: tests/test_classspan_host.py compiles and runs it.
//  * decode: for entry counts 0, 1, M - 1, M, M + 1 and cap and every M in 1 .. cap, and for
//    launches of several bags whose tables come from class histograms (classes of several runs,
//    only class 0 or only class 2^k - 1 non-empty, an empty bag, bags of different counts), the
//    slots of a launch — per bag tiles_x * class_spans(cap, M), tile-major — visit every table
//    entry of every bag exactly once per tile and none at or past the bag's count;
//  * walk: one lane of an item — R plane-word groups of 32 x images — walks the spans of a bag
//    as the device does: digit tables 0 - 2 once per item, per run of a new class G, P, E and
//    the top digit by class_digit_table's own arithmetic, per image class_gt32_digits, per run
//    len * popc(G); the sum over the bag's spans is the brute-force count of x > z for random
//    and edge images, for every M, with u32 lane sums;
//  * plan: class_plan carries the clamped span and the items per bag; the automatic span is 1
//    for small launches, a power of two <= kClassSpanMax, never leaves fewer than
//    kClassSpanFill items per wave the chip holds, and is long at the bench's shape.
// Prints one "ok <name>" line per check and exits non-zero at the first mismatch.
#include <algorithm>
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

// every slot of one bag's part of a launch; seen[tx * cap + e] counts the visits
static int visit_bag(int tiles_x, int cap, int m, int cnt, std::vector<int>& seen) {
  const int spans = class_spans(cap, m);
  if ((int64_t)spans * m < cap || (int64_t)(spans - 1) * m >= cap) return fail("spans", cap, m, spans, 0);
  seen.assign((size_t)tiles_x * cap, 0);
  for (int rem = 0; rem < tiles_x * spans; ++rem) {
    const ClassSpanItem it = class_span_item(rem, spans);
    if (it.tx < 0 || it.tx >= tiles_x || it.q < 0 || it.q >= spans) return fail("item", rem, spans, it.tx, it.q);
    if (it.tx * spans + it.q != rem) return fail("item order", rem, spans, it.tx, it.q);
    const ClassSpan sp = class_span_entries(it.q, m, cnt);
    if (sp.e1 > cnt || sp.e1 - sp.e0 > m) return fail("span past the count", it.q, m, cnt, sp.e1);
    for (int e = sp.e0; e < sp.e1; ++e) ++seen[(size_t)it.tx * cap + e];
  }
  for (int tx = 0; tx < tiles_x; ++tx)
    for (int e = 0; e < cap; ++e)
      if (seen[(size_t)tx * cap + e] != (e < cnt ? 1 : 0)) return fail("visits", tx, e, cnt, m);
  return 0;
}

static int check_decode() {
  std::vector<int> seen;
  for (int cap : {1, 2, 7, 8, 9, 40, 308})
    for (int m = 1; m <= cap; ++m) {
      if (class_span_clamp(m, cap) != m) return fail("clamp inside", m, cap, 0, 0);
      for (int cnt : {0, 1, m - 1, m, m + 1, cap})
        if (cnt >= 0 && cnt <= cap)
          for (int tiles_x : {1, 3})
            if (visit_bag(tiles_x, cap, m, cnt, seen)) return 1;
    }
  for (int cap : {1, 5, 308}) {
    if (class_span_clamp(0, cap) != 1 || class_span_clamp(-3, cap) != 1) return fail("clamp low", cap, 0, 0, 0);
    if (class_span_clamp(cap + 7, cap) != cap || class_span_clamp((int64_t)1 << 40, cap) != cap)
      return fail("clamp high", cap, 0, 0, 0);
    if (class_spans(cap, cap) != 1) return fail("whole bag", cap, 0, 0, 0);
  }
  // launches of several bags from histograms: k class bits, runs of at most 8
  for (int k : {1, 3, 8}) {
    const int nc = 1 << k;
    std::vector<std::vector<uint32_t>> hists;
    auto hist = [&](auto f) {
      std::vector<uint32_t> h(nc);
      for (int c = 0; c < nc; ++c) h[c] = f(c);
      hists.push_back(h);
    };
    hist([&](int) { return 0u; });                               // no z
    hist([&](int c) { return c == 0 ? 1u : 0u; });               // one entry
    hist([&](int c) { return c == 0 ? 25u : 0u; });              // only class 0: four runs
    hist([&](int c) { return c == nc - 1 ? 17u : 0u; });         // only the last class: three
    hist([&](int c) { return (uint32_t)(c % 3 == 0 ? 9 + c % 5 : c % 3); });  // mixed
    hist([&](int) { return 8u; });                               // every class one full run
    hist([&](int) { return 1u; });
    int64_t max_nz = 0;
    for (auto& h : hists) {
      int64_t n = 0;
      for (uint32_t v : h) n += v;
      max_nz = std::max(max_nz, n);
    }
    const int cap = (int)class_capacity(max_nz, k, 8);
    std::vector<uint32_t> tab(2 * (size_t)cap);
    std::vector<int> cnts;
    for (auto& h : hists) {
      const int cnt = (int)class_table(h.data(), k, 8, tab.data());
      if (cnt > cap) return fail("count over the capacity", k, cnt, cap, 0);
      cnts.push_back(cnt);
    }
    if (*std::min_element(cnts.begin(), cnts.end()) != 0 || cnts[1] != 1 || cnts[2] != 4 || cnts[3] != 3)
      return fail("histogram counts", k, cnts[1], cnts[2], cnts[3]);
    for (int m = 1; m <= cap + 1; ++m) {
      const int mm = class_span_clamp(m, cap);
      for (int cnt : cnts)
        if (visit_bag(2, cap, mm, cnt, seen)) return 1;
    }
  }
  std::printf("ok decode\n");
  return 0;
}

// ---------------------------------------------------------------------------------- the walk
template <int NB>
static void planes_of(const uint32_t (&img)[32], uint32_t (&plane)[NB]) {
  uint32_t a[32];
  for (int k = 0; k < 32; ++k) a[k] = img[k];
  bits_transpose32(a);
  for (int b = 0; b < NB; ++b) plane[b] = a[b];
}

// The device's item on one lane: R groups against entries [e0, e1) of tab; zs: the bag's
// class-ordered images, digit-ready.  u32 lane sums, as on the device.
template <int NB, int K, int R>
static uint64_t walk_span(const uint32_t (&plane)[R][NB], const uint32_t* tab, const uint32_t* zs,
                          int e0, int e1) {
  constexpr int NL = NB - K, kTop = kClassDigits - 1;
  constexpr int W3 = class_digit_width(NL, kTop), S3 = class_digit_shift(NL, kTop);
  ClassDigitTables t[R];
  uint32_t top[R][K], hi[R][W3], acc[R], G[R];
  for (int r = 0; r < R; ++r) {
    uint32_t low[NL];
    for (int b = 0; b < NL; ++b) low[b] = plane[r][b];
    for (int b = 0; b < K; ++b) top[r][b] = plane[r][NL + b];
    for (int b = 0; b < W3; ++b) hi[r][b] = low[S3 + b];
    class_digit_tables_one<NL, 0>(low, ~0u, t[r]);
    class_digit_tables_one<NL, 1>(low, ~0u, t[r]);
    class_digit_tables_one<NL, 2>(low, ~0u, t[r]);
    for (int d = 0; d < kClassDigitEntries; ++d) t[r].g[kTop][d] = 0u;
    acc[r] = 0, G[r] = 0;
  }
  uint32_t ng = 0, cg = 0, cls = ~0u;
  for (int e = e0; e < e1; ++e) {
    const ClassRun run = class_entry(tab[2 * e], tab[2 * e + 1]);
    if (run.cls != cls) {
      cls = run.cls, ng = 0;
      for (int r = 0; r < R; ++r) {
        uint32_t P, g[(1 << W3) + 1];
        class_gp<K>(top[r], cls, G[r], P);
        ng += (uint32_t)__builtin_popcount(G[r]);
        class_digit_table<W3>(hi[r], class_equal_mask(G[r], P), g);
        for (int d = 1; d <= (1 << W3); ++d) t[r].g[kTop][d] = g[d];  // (entry 0 stays 0)
      }
    }
    cg += (uint32_t)run.len * ng;
    for (int64_t j = 0; j < run.len; ++j)
      for (int r = 0; r < R; ++r)
        acc[r] += (uint32_t)__builtin_popcount(class_gt32_digits(t[r], G[r], zs[run.z0 + j]).word);
  }
  uint64_t tot = cg;
  for (int r = 0; r < R; ++r) tot += acc[r];
  return tot;
}

template <int NB, int K>
static int check_walk(std::mt19937& g) {
  constexpr int NL = NB - K, R = 2;
  static_assert(class_digits_fit(NL), "a (NB, K) of the digit loop");
  const uint32_t top = (uint32_t)(((uint64_t)1 << NB) - 1), lowmask = (1u << NL) - 1u;
  std::uniform_int_distribution<uint32_t> any(0, top);
  for (int round = 0; round < 4; ++round) {
    // z images: random, with one long class, class 0 and the last class, digit boundaries
    std::vector<uint32_t> z;
    const int nz = round == 3 ? 1 : 150 + 37 * round;
    for (int i = 0; i < nz; ++i) z.push_back(any(g));
    if (round < 3) {
      for (int i = 0; i < 3 * 8 + 1; ++i) z.push_back((5u << NL) | (any(g) & lowmask));
      for (uint32_t v : {0u, 1u, top, top - 1, lowmask, lowmask + 1, top & ~lowmask}) z.push_back(v);
      for (int j = 1; j < kClassDigits; ++j) {
        const uint32_t e = 1u << class_digit_shift(NL, j);
        for (uint32_t v : {e - 1, e, e + 1, 7 * e}) z.push_back(v & top);
      }
    }
    // x images: random, ties with z, 0, the bound, a padded tail (plane words 0)
    uint32_t img[R][32], plane[R][NB];
    for (int r = 0; r < R; ++r) {
      for (int i = 0; i < 32; ++i) img[r][i] = (g() & 1) ? any(g) : z[g() % z.size()];
      img[r][0] = 0, img[r][1] = top;
      if (round == 1)
        for (int i = 20; i < 32; ++i) img[r][i] = 0;
      if (round == 2 && r == 1)
        for (int i = 0; i < 32; ++i) img[r][i] = top;  // G full in every class below the top
      planes_of<NB>(img[r], plane[r]);
    }
    uint64_t want = 0;
    for (int r = 0; r < R; ++r)
      for (int i = 0; i < 32; ++i)
        for (uint32_t v : z) want += img[r][i] > v;
    // pre-pass 2 on the host: complemented images by class, digit-ready, and the run table
    std::vector<uint32_t> hist(1u << K, 0u), cur(1u << K, 0u), zs(z.size());
    for (uint32_t v : z) ++hist[class_of(~v, NB, K)];
    for (uint32_t c = 1; c < (1u << K); ++c) cur[c] = cur[c - 1] + hist[c - 1];
    for (uint32_t v : z) zs[cur[class_of(~v, NB, K)]++] = class_digit_encode(~v, NL);
    const int cap = (int)class_capacity((int64_t)z.size(), K, 8);
    std::vector<uint32_t> tab(2 * (size_t)cap);
    const int cnt = (int)class_table(hist.data(), K, 8, tab.data());
    for (int m : {1, 2, 3, 5, 8, cnt > 1 ? cnt - 1 : 1, cnt, cap}) {
      m = class_span_clamp(m, cap);
      uint64_t got = 0;
      for (int q = 0; q < class_spans(cap, m); ++q) {
        const ClassSpan sp = class_span_entries(q, m, cnt);
        if (sp.e0 < sp.e1) got += walk_span<NB, K, R>(plane, tab.data(), zs.data(), sp.e0, sp.e1);
      }
      if (got != want) return fail("walk", NB, K, m, (long long)got - (long long)want);
    }
  }
  std::printf("ok walk NB=%d k=%d\n", NB, K);
  return 0;
}

static int check_plan() {
  const int64_t shapes[][3] = {{15625, 15625, 1280}, {15625, 15625, 256}, {4101, 130, 6},
                               {2048, 64, 33},       {1, 777, 3}};
  for (const auto& sh : shapes)
    for (int k : {1, 4, 8})
      for (int64_t runs : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)5, (int64_t)1 << 20}) {
        const PlanesPlan p = planes_plan(sh[0], sh[1], sh[2], 2, 0, 0);
        const ClassPlan c = class_plan(p, sh[0], sh[1], sh[2], 20, k, runs);
        const ClassPlan c1 = class_plan(p, sh[0], sh[1], sh[2], 20, k);
        if (c.span != class_span_clamp(runs, c.cap) || c.span < 1 || c.span > c.cap) return fail("plan span", k, runs, c.span, c.cap);
        if (c.per_bag != p.tiles_x * class_spans(c.cap, c.span) + p.tiles_s * p.schunks) return fail("per_bag", k, runs, c.per_bag, 0);
        if (c1.span != 1 || c1.per_bag != p.tiles_x * c1.cap + p.tiles_s * p.schunks) return fail("M = 1 is one item per entry", k, c1.per_bag, 0, 0);
        if (c.cap != c1.cap || c.off_tab != c1.off_tab || c.off_zs != c1.off_zs || c.off_cnt != c1.off_cnt)
          return fail("the span moves a region", k, runs, 0, 0);
      }
  for (int64_t bags : {(int64_t)1, (int64_t)32, (int64_t)128, (int64_t)256, (int64_t)1280, (int64_t)2048})
    for (int tiles : {1, 2, 4})
      for (int cap : {1, 9, 260, 308, 2000}) {
        const int m = class_span_auto(bags, tiles, cap);
        if (m < 1 || m > kClassSpanMax || m > std::max(cap, 1) || (m & (m - 1))) return fail("auto span", bags, tiles, cap, m);
        if (m > 1 && bags * tiles * class_spans(cap, m) < kClassSpanFill * kClassSpanChipWaves)
          return fail("auto span leaves a tail", bags, tiles, cap, m);
      }
  if (class_span_auto(4, 2, 260) != 1) return fail("small launches keep one entry per item", 0, 0, 0, 0);
  if (class_span_auto(1280, 4, 308) != kClassSpanMax) return fail("the bench's launch takes long spans", class_span_auto(1280, 4, 308), 0, 0, 0);
  if (class_span_auto(128, 2, 260) < 2) return fail("128 bags of two tiles", 0, 0, 0, 0);
  std::printf("ok plan\n");
  return 0;
}

int main() {
  std::mt19937 g(20261021u);
  if (check_decode() || check_plan()) return 1;
  if (check_walk<20, 8>(g) || check_walk<16, 4>(g) || check_walk<16, 8>(g) || check_walk<18, 6>(g)) return 1;
  std::printf("done\n");
  return 0;
}
