// Host check of the masked-plane form of the class loop (csrc/chainclass.h class_equal_mask,
// class_mask_planes, class_gt32_masked), no GPU: tests/test_classmask_host.py
// compiles and runs it.  With E = P & ~G and the low planes ANDed with E once per group,
//     popc(class_gt32(low, G, P, zc)) == popc(G) + popc(bits_gt32(masked, zc))
// for every z of the class, so a run of len images counts len * popc(G) + sum popc(word).
//  * words, NB in {16, 20, 24} x every k in 1 .. 8: random images and adversarial ones (all x
//    equal to z; x equal to z in the top field and -1 / +1 in the low field; x = 0 padded slots
//    against z image 0, where E is set and the planes are 0; all x at the bound): for every z
//    the constant and the word are disjoint, the word is E & c_low, constant | word is
//    class_gt32 bit for bit, and the popcounts add up to the per-image integer compare;
//  * runs of length 1, 2 and 3 (and longer) of one class, the class of three z beside the class
//    of one under x all at the bound included: len * popc(G) + the words == the integer count
//    with len the run's exact length, and one slot more in len is seen to over-count by popc(G).
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

static uint32_t popc(uint32_t v) { return bits_popc_add(v, 0u); }

template <int NB>
static void planes_of(const uint32_t (&img)[32], uint32_t (&plane)[NB]) {
  uint32_t a[32];
  for (int k = 0; k < 32; ++k) a[k] = img[k];
  bits_transpose32(a);
  for (int b = 0; b < NB; ++b) plane[b] = a[b];
}

// One x group prepared for class D as the device item prepares it
template <int NB, int K>
struct Group {
  static constexpr int NL = NB - K;
  uint32_t low[NL], masked[NL], G, P, E;
  Group(const uint32_t (&img)[32], uint32_t D) {
    uint32_t plane[NB], top[K];
    planes_of<NB>(img, plane);
    for (int b = 0; b < NL; ++b) low[b] = plane[b];
    for (int b = 0; b < K; ++b) top[b] = plane[NL + b];
    class_gp<K>(top, D, G, P);
    E = class_equal_mask(G, P);
    class_mask_planes<NL>(low, E, masked);
  }
};

// every property of one (group, z)
template <int NB, int K>
static int check_word(const uint32_t (&img)[32], uint32_t z) {
  constexpr int NL = NB - K;
  const uint32_t zc = ~z, D = class_of(zc, NB, K);
  const Group<NB, K> g(img, D);
  uint32_t want = 0, eq = 0;
  for (int k = 0; k < 32; ++k) {
    want |= (uint32_t)(img[k] > z) << k;
    eq |= (uint32_t)((img[k] >> NL) == (z >> NL)) << k;
  }
  if (g.G & ~g.P) return fail("G not a subset of P", NB, K, z, g.G);
  if (g.E != eq) return fail("E is not the equal-top mask", NB, K, z, g.E);
  const uint32_t full = class_gt32<NL>(g.low, g.G, g.P, zc);
  const ClassMasked m = class_gt32_masked<NL>(g.masked, g.G, zc);
  if (full != want) return fail("class_gt32", NB, K, z, full);
  if (m.constant != g.G) return fail("constant term", NB, K, z, m.constant);
  if (m.constant & m.word) return fail("constant and word overlap", NB, K, z, m.word);
  if (m.word != (g.E & bits_gt32<NL>(g.low, zc))) return fail("word != E & c", NB, K, z, m.word);
  if ((m.constant | m.word) != full) return fail("constant | word", NB, K, z, m.word);
  if (popc(m.constant) + popc(m.word) != popc(want)) return fail("popcounts", NB, K, z, m.word);
  return 0;
}

template <int NB, int K>
static int check_words(std::mt19937& g) {
  constexpr int NL = NB - K;
  const uint32_t top = (uint32_t)(((uint64_t)1 << NB) - 1), lowmask = (1u << NL) - 1u;
  std::uniform_int_distribution<uint32_t> any(0, top);
  long long pairs = 0;
  std::vector<uint32_t> zs = {0u, 1u, top, top - 1, lowmask, lowmask + 1, top & ~lowmask};
  for (uint32_t c = 1; c < (1u << K); c += (K > 4 ? 37 : 1)) {
    zs.push_back(c << NL);
    zs.push_back((c << NL) - 1);
    zs.push_back((c << NL) + 1);
  }
  for (int i = 0; i < 48; ++i) zs.push_back(any(g));
  const uint32_t bound = top < 1000000u ? top : 1000000u;
  for (uint32_t z : zs) {
    uint32_t img[32];
    // random images; half of them share z's top field
    for (int round = 0; round < 6; ++round) {
      for (int k = 0; k < 32; ++k)
        img[k] = (g() & 1) ? any(g) : ((z & ~lowmask) | (any(g) & lowmask));
      if (check_word<NB, K>(img, z)) return 1;
      ++pairs;
    }
    for (int k = 0; k < 32; ++k) img[k] = z;  // all x equal to z
    if (check_word<NB, K>(img, z)) return 1;
    for (int k = 0; k < 32; ++k) {  // equal in the top field, -1 / 0 / +1 in the low field
      const uint32_t l = z & lowmask, d = (uint32_t)(k % 3);
      const uint32_t nl = d == 0 ? (l > 0 ? l - 1 : l) : d == 1 ? l : (l < lowmask ? l + 1 : l);
      img[k] = (z & ~lowmask) | nl;
    }
    if (check_word<NB, K>(img, z)) return 1;
    for (int k = 0; k < 32; ++k) img[k] = 0;  // padded x slots (against z = 0: E set, planes 0)
    if (check_word<NB, K>(img, z)) return 1;
    {
      const Group<NB, K> pad(img, class_of(~z, NB, K));
      const ClassMasked m = class_gt32_masked<NL>(pad.masked, pad.G, ~z);
      if (m.constant != 0 || m.word != 0) return fail("padded x slot counted", NB, K, z, m.word);
      if (z == 0 && pad.E != ~0u) return fail("padded x against z 0: E", NB, K, z, pad.E);
    }
    for (uint32_t b : {top, bound}) {  // all x at the bound
      for (int k = 0; k < 32; ++k) img[k] = b;
      if (check_word<NB, K>(img, z)) return 1;
    }
    pairs += 5;
  }
  std::printf("ok words NB=%d k=%d (%lld x 32 pairs)\n", NB, K, pairs);
  return 0;
}

// One run: z images of one class against one group; len is the run's exact length
template <int NB, int K>
static int check_run(const uint32_t (&img)[32], const std::vector<uint32_t>& z) {
  constexpr int NL = NB - K;
  const uint32_t D = class_of(~z[0], NB, K);
  const Group<NB, K> g(img, D);
  long long want = 0, words = 0;
  for (uint32_t b : z) {
    if (class_of(~b, NB, K) != D) return fail("run of two classes", NB, K, b, D);
    for (int k = 0; k < 32; ++k) want += img[k] > b;
    words += popc(class_gt32_masked<NL>(g.masked, g.G, ~b).word);
  }
  const long long len = (long long)z.size();
  const long long got = len * popc(g.G) + words;
  if (got != want) return fail("run count", NB, K, got, want);
  // a padded slot past the run's end adds nothing to the words ...
  if (class_gt32_masked<NL>(g.masked, g.G, kBitsZNever).word != 0)
    return fail("padded scalar slot's word", NB, K, len, 0);
  // ... but one more in len over-counts by popc(G): len must be exact
  if ((len + 1) * popc(g.G) + words != want + popc(g.G))
    return fail("len + 1", NB, K, len, popc(g.G));
  return 0;
}

template <int NB, int K>
static int check_runs(std::mt19937& g) {
  constexpr int NL = NB - K;
  const uint32_t top = (uint32_t)(((uint64_t)1 << NB) - 1), lowmask = (1u << NL) - 1u;
  const uint32_t bound = top < 1000000u ? top : 1000000u;
  std::uniform_int_distribution<uint32_t> any(0, top);
  uint32_t img[32];
  int over = 0;
  // the trap input: x all at the bound, a class of three z and a class of one
  for (uint32_t b : {top, bound}) {
    for (int k = 0; k < 32; ++k) img[k] = b;
    if (check_run<NB, K>(img, {5u, 6u, 7u}) || check_run<NB, K>(img, {b})) return 1;
    const Group<NB, K> lowc(img, class_of(~5u, NB, K));
    // every x above the class of {5, 6, 7}: there an evaluated padded slot would show
    if ((b >> NL) > 0) over += popc(lowc.G) == 32 ? 1 : -64;
  }
  if (over < 1) return fail("the trap input does not set G", NB, K, over, 0);
  for (int round = 0; round < 200; ++round) {
    const uint32_t field = any(g) & ~lowmask;
    for (int k = 0; k < 32; ++k)
      img[k] = (g() % 3) ? any(g) : (field | (any(g) & lowmask));
    if (round == 7)
      for (int k = 0; k < 32; ++k) img[k] = 0;
    for (int len : {1, 2, 3, 4, 7, 9, 17}) {
      std::vector<uint32_t> z(len);
      for (auto& b : z) b = field | (any(g) & lowmask);
      if ((round & 1) && (img[round % 32] >> NL) == (field >> NL)) z[0] = img[round % 32];  // a tie
      if (check_run<NB, K>(img, z)) return 1;
    }
  }
  std::printf("ok runs NB=%d k=%d\n", NB, K);
  return 0;
}

template <int NB, int K>
static int check_k(std::mt19937& g) {
  return check_words<NB, K>(g) || check_runs<NB, K>(g);
}

template <int NB>
static int check_nb(std::mt19937& g) {
  return check_k<NB, 1>(g) || check_k<NB, 2>(g) || check_k<NB, 3>(g) || check_k<NB, 4>(g) ||
         check_k<NB, 5>(g) || check_k<NB, 6>(g) || check_k<NB, 7>(g) || check_k<NB, 8>(g);
}

int main() {
  std::mt19937 g(20261020u);
  if (check_nb<16>(g) || check_nb<20>(g) || check_nb<24>(g)) return 1;
  std::printf("done\n");
  return 0;
}
