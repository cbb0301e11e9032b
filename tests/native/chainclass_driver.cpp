// Host check of csrc/chainclass.h (the class-run form of the plane-reading chain count), no GPU:
// tests/test_chainclass_host.py compiles and runs it.
//  * arithmetic, NB in {16, 20, 24} x k in {1, 2, 6, 8}: for random and boundary images (0,
//    2^NB - 1, multiples of 2^(NB - k) and one less, x = z) class_gt32 — bits_carry(G, P, c_low)
//    — equals bits_gt32's carry bit for bit and the integer compare; x slots of 0 count nothing
//    against every z; a padded SCALAR slot (complemented 0) would count G, which is why the
//    class loop never evaluates one;
//  * the run table: ragged class histograms (all z in one class, two classes, a class of size
//    1, odd sizes, empty classes, nz = 0) under forced z chunks of 8 and 600 and the automatic
//    one: the runs tile each class's range exactly once in class order, none is longer than
//    the chunk or empty, the entry count stays within class_capacity and the regions within
//    planes_work_words + class_work_words;
//  * a whole bag: z counting-sorted by class, the table built, every run counted with the
//    class loop's arithmetic on exactly its len images == the brute-force count.
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

static uint32_t popc(uint32_t v) { return bits_popc_add(v, 0u); }

// planes of 32 images
template <int NB>
static void planes_of(const uint32_t (&img)[32], uint32_t (&plane)[NB]) {
  uint32_t a[32];
  for (int k = 0; k < 32; ++k) a[k] = img[k];
  bits_transpose32(a);
  for (int b = 0; b < NB; ++b) plane[b] = a[b];
}

template <int NB, int K>
static uint32_t gt_class(const uint32_t (&plane)[NB], uint32_t zc, uint32_t* Gout = nullptr) {
  constexpr int NL = NB - K;
  uint32_t low[NL], top[K], G, P;
  for (int b = 0; b < NL; ++b) low[b] = plane[b];
  for (int b = 0; b < K; ++b) top[b] = plane[NL + b];
  class_gp<K>(top, class_of(zc, NB, K), G, P);
  if (Gout) *Gout = G;
  if (G & ~P) return ~bits_gt32<NB>(plane, zc);  // G must be a subset of P: force a mismatch
  return class_gt32<NL>(low, G, P, zc);
}

template <int NB, int K>
static int check_arith(std::mt19937& g) {
  const uint32_t top = (uint32_t)(((uint64_t)1 << NB) - 1);
  std::uniform_int_distribution<uint32_t> any(0, top);
  std::vector<uint32_t> edge = {0u, 1u, top, top - 1};
  for (uint32_t c = 1; c < (1u << K); ++c) {
    edge.push_back(c << (NB - K));
    edge.push_back((c << (NB - K)) - 1);
    edge.push_back((c << (NB - K)) + 1);
  }
  long long pairs = 0;
  for (int round = 0; round < 64; ++round) {
    uint32_t img[32], plane[NB];
    for (int k = 0; k < 32; ++k)
      img[k] = (round & 1) ? edge[(size_t)(any(g) % edge.size())] : any(g);
    if (round == 2)
      for (int k = 0; k < 32; ++k) img[k] = 0;  // padded x slots
    planes_of<NB>(img, plane);
    std::vector<uint32_t> zs(edge);
    for (int k = 0; k < 32; ++k) zs.push_back(img[k]);  // x = z
    for (int i = 0; i < 64; ++i) zs.push_back(any(g));
    for (uint32_t z : zs) {
      const uint32_t zc = ~z;
      uint32_t want = 0;
      for (int k = 0; k < 32; ++k) want |= (uint32_t)(img[k] > z) << k;
      const uint32_t full = bits_gt32<NB>(plane, zc), got = gt_class<NB, K>(plane, zc);
      if (full != want) return fail("bits_gt32", NB, K, z, full);
      if (got != want) return fail("class_gt32", NB, K, z, got);
      if (round == 2 && got != 0) return fail("padded x slot counted", NB, K, z, got);
      ++pairs;
    }
    // the trap: inside a run of class D a padded scalar slot (complemented 0) leaves
    // c_low = 0 and counts the run's G — the x whose top field is above the class's
    const uint32_t zr = any(g), ztop = zr >> (NB - K);
    uint32_t G, low[NB - K], above = 0;
    gt_class<NB, K>(plane, ~zr, &G);
    for (int b = 0; b < NB - K; ++b) low[b] = plane[b];
    for (int k = 0; k < 32; ++k) above |= (uint32_t)((img[k] >> (NB - K)) > ztop) << k;
    const uint32_t padded = class_gt32<NB - K>(low, G, ~0u, kBitsZNever);
    if (padded != G || G != above) return fail("padded scalar slot", NB, K, padded, above);
  }
  std::printf("ok arith NB=%d k=%d (%lld x 32 pairs)\n", NB, K, pairs);
  return 0;
}

// One histogram under one chunk: the table's invariants
static int check_table(const std::vector<uint32_t>& hist, int k, int64_t z_chunk, int64_t max_nz) {
  int64_t nz = 0;
  for (uint32_t n : hist) nz += n;
  const int64_t cap = class_capacity(max_nz, k, z_chunk), chunk = class_chunk(z_chunk);
  std::vector<uint32_t> tab((size_t)(2 * (cap + nz + 1)), 0xFFFFFFFFu);
  const int64_t e = class_table(hist.data(), k, z_chunk, tab.data());
  if (e > cap) return fail("capacity", k, z_chunk, e, cap);
  if (cap > class_capacity(max_nz, kClassMaxBits, kClassMinChunk))
    return fail("capacity above the sized one", k, z_chunk, cap, 0);
  int64_t at = 0, i = 0;
  for (uint32_t c = 0; c < (1u << k); ++c) {
    const int64_t end = at + hist[c];
    int64_t longest = 0, shortest = INT64_MAX;
    while (i < e) {
      const ClassRun r = class_entry(tab[2 * i], tab[2 * i + 1]);
      if (r.cls != c) break;
      if (r.z0 != at) return fail("run start", k, z_chunk, c, r.z0);
      if (r.len < 1 || r.len > chunk) return fail("run length", k, z_chunk, c, r.len);
      longest = std::max(longest, r.len);
      shortest = std::min(shortest, r.len);
      at += r.len;
      ++i;
    }
    if (at != end) return fail("class not tiled", k, z_chunk, c, at);
    if (hist[c] && longest - shortest > 1) return fail("runs not near-equal", k, z_chunk, c, 0);
  }
  if (i != e || at != nz) return fail("table end", k, z_chunk, i, e);
  return 0;
}

static int check_tables(std::mt19937& g) {
  long long tables = 0;
  for (int k : {1, 2, 6, 8}) {
    const size_t C = (size_t)1 << k;
    std::vector<std::vector<uint32_t>> hists;
    hists.push_back(std::vector<uint32_t>(C, 0));  // nz = 0
    for (uint32_t n : {1u, 7u, 8u, 9u, 601u, 15625u, 100000u}) {
      std::vector<uint32_t> h(C, 0);
      h[C - 1] = n;  // all z in one class
      hists.push_back(h);
      h[0] = 1;  // two classes, one of size 1
      hists.push_back(h);
      h[0] = n | 1u;  // two classes, odd
      hists.push_back(h);
    }
    for (int rep = 0; rep < 8; ++rep) {  // ragged: random sizes, about half the classes empty
      std::vector<uint32_t> h(C, 0);
      for (auto& n : h)
        if (g() & 1) n = g() % (rep < 4 ? 20 : 1300);
      hists.push_back(h);
    }
    for (const auto& h : hists) {
      int64_t nz = 0;
      for (uint32_t n : h) nz += n;
      for (int64_t max_nz : {nz, nz + 4321}) {
        if (max_nz == 0) max_nz = 1;
        for (int64_t zc : {(int64_t)8, (int64_t)600, (int64_t)0}) {
          for (int64_t n_bags : {(int64_t)1, (int64_t)1280}) {
            // the chunk as the launch gets it: from the plan, forced or automatic
            const PlanesPlan p = planes_plan(15625, max_nz, n_bags, 0, zc);
            if (check_table(h, k, p.z_chunk, max_nz)) return 1;
            for (int nb : {16, 20, 24}) {
              const ClassPlan cp = class_plan(p, 15625, max_nz, n_bags, nb, k);
              const int64_t have =
                  planes_work_words(15625, max_nz, n_bags, nb) + class_work_words(max_nz, n_bags);
              if (cp.chunk != class_chunk(p.z_chunk) || cp.zs_stride < max_nz ||
                  cp.off_zs != planes_work_words(15625, max_nz, n_bags, nb) ||
                  cp.off_cnt < cp.off_zs + n_bags * cp.zs_stride ||
                  cp.off_tab < cp.off_cnt + n_bags || class_plan_end(cp, n_bags) > have ||
                  cp.per_bag != p.tiles_x * cp.cap + p.tiles_s * p.schunks)
                return fail("regions", k, zc, nb, max_nz);
            }
            ++tables;
          }
        }
      }
    }
  }
  // the automatic class bits: 8 at the bench shape (mean run 61), never more than 8, fewer for
  // small bags, none in launches of few bags
  if (class_bits_auto(15625, 1280, 20) != 8 || class_bits_auto(15625, 32, 20) != 8 ||
      class_bits_auto(15625, 31, 20) != 0 || class_bits_auto(100000, 1, 18) != 0 ||
      class_bits_auto(100000, 64, 18) != 8 || class_bits_auto(1 << 23, 64, 24) != 8 ||
      class_bits_auto(4000, 64, 16) != 6 || class_bits_auto(96, 64, 16) != 1 ||
      class_bits_auto(95, 64, 16) != 0)
    return fail("automatic class bits", class_bits_auto(15625, 1280, 20),
                class_bits_auto(15625, 31, 20), class_bits_auto(4000, 64, 16), 0);
  std::printf("ok tables (%lld)\n", tables);
  return 0;
}

// A whole bag through the class form on the host
template <int NB, int K>
static int check_bag(std::mt19937& g, int nx, int nz, int64_t z_chunk, int mode) {
  const uint32_t top = (uint32_t)(((uint64_t)1 << NB) - 1);
  std::uniform_int_distribution<uint32_t> any(0, top);
  std::vector<uint32_t> x(nx), z(nz);
  for (auto& v : x) v = mode == 1 ? top : any(g);  // mode 1: every x the bound
  for (int i = 0; i < nz; ++i)                     // mode 1: an odd class and one of size 1
    z[i] = mode == 1 ? (i == 0 ? top : 5u) : mode == 2 ? 77u : any(g);
  long long want = 0;
  for (uint32_t a : x)
    for (uint32_t b : z) want += a > b;
  // pre-pass 2: histogram, scan, scatter
  std::vector<uint32_t> hist((size_t)1 << K, 0), cur((size_t)1 << K, 0), zs(nz);
  for (uint32_t b : z) ++hist[class_of(~b, NB, K)];
  for (size_t c = 1; c < hist.size(); ++c) cur[c] = cur[c - 1] + hist[c - 1];
  for (uint32_t b : z) zs[cur[class_of(~b, NB, K)]++] = ~b;
  const int64_t max_nz = nz > 0 ? nz : 1;
  std::vector<uint32_t> tab((size_t)(2 * class_capacity(max_nz, K, z_chunk)));
  const int64_t e = class_table(hist.data(), K, z_chunk, tab.data());
  long long got = 0;
  for (int x0 = 0; x0 < nx; x0 += 32) {  // one 32-image group per "lane"; slots past nx hold 0
    uint32_t img[32], plane[NB], low[NB - K], tp[K];
    for (int k = 0; k < 32; ++k) img[k] = x0 + k < nx ? x[x0 + k] : 0u;
    planes_of<NB>(img, plane);
    for (int b = 0; b < NB - K; ++b) low[b] = plane[b];
    for (int b = 0; b < K; ++b) tp[b] = plane[NB - K + b];
    for (int64_t i = 0; i < e; ++i) {
      const ClassRun r = class_entry(tab[2 * i], tab[2 * i + 1]);
      uint32_t G, P;
      class_gp<K>(tp, r.cls, G, P);
      for (int64_t j = 0; j < r.len; ++j) {  // exactly len images
        if (class_of(zs[r.z0 + j], NB, K) != r.cls) return fail("run class", NB, K, i, j);
        got += popc(class_gt32<NB - K>(low, G, P, zs[r.z0 + j]));
      }
    }
  }
  if (got != want) return fail("bag count", NB, K, got, want);
  return 0;
}

template <int NB, int K>
static int check_bags(std::mt19937& g) {
  for (int64_t zc : {(int64_t)8, (int64_t)600})
    for (int mode = 0; mode < 3; ++mode)
      for (int nx : {1, 31, 33, 100})
        for (int nz : {0, 1, 2, 7, 64, 65, 333})
          if (check_bag<NB, K>(g, nx, nz, zc, mode)) return 1;
  std::printf("ok bags NB=%d k=%d\n", NB, K);
  return 0;
}

template <int NB>
static int check_nb(std::mt19937& g) {
  return check_arith<NB, 1>(g) || check_arith<NB, 2>(g) || check_arith<NB, 6>(g) ||
         check_arith<NB, 8>(g) || check_bags<NB, 1>(g) || check_bags<NB, 2>(g) ||
         check_bags<NB, 6>(g) || check_bags<NB, 8>(g);
}

int main() {
  std::mt19937 g(20241020u);
  if (check_nb<16>(g) || check_nb<20>(g) || check_nb<24>(g)) return 1;
  if (check_tables(g)) return 1;
  std::printf("done\n");
  return 0;
}
