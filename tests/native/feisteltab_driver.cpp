// Host check of the Feistel round tables (csrc/feistel.h feistel_round_table,
// feistel_once32_tab), no GPU: tests/test_feisteltab_host.py compiles it with
// the address and undefined-behaviour sanitizers and runs it.
//  * for half_bits 1 .. kEmTabMaxHB and keys {0, 1, 2^64 - 1, three fixed random} the table
//    has exactly 6 << half_bits entries (a heap block of that size: a lookup past it is the
//    address sanitizer's finding), every entry is <= mask, and the table-driven round network
//    equals feistel_once for EVERY v of the domain [0, 4^half_bits);
//  * the domain sizes around every boundary pick the half_bits the tables are sized by.
// Prints one "ok <name>" line per check and exits non-zero at the first mismatch.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "feistel.h"

using namespace tw;

static int fail(const char* what, long long a, long long b, long long c, long long d) {
  std::printf("FAIL %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
  return 1;
}

int main() {
  static_assert(kEmTabMaxHB == 11, "the test's range follows the largest tabulated half");
  const uint64_t keys[6] = {0ull, 1ull, ~0ull, 0x243F6A8885A308D3ull, 0x13198A2E03707344ull,
                            0xA4093822299F31D0ull};
  for (uint32_t hb = 1; hb <= kEmTabMaxHB; ++hb) {
    const int64_t domain = (int64_t)1 << (2 * hb);
    // the sizes that choose this half: (4^(hb-1), 4^hb]; one past it the next
    if (make_feistel(domain, 0).half_bits != hb) return fail("half_bits at 4^hb", hb, 0, 0, 0);
    if (make_feistel(domain + 1, 0).half_bits != hb + 1) return fail("half past", hb, 0, 0, 0);
    if (hb > 1 && make_feistel(domain / 4 + 1, 0).half_bits != hb)
      return fail("half_bits low end", hb, 0, 0, 0);
    for (int ki = 0; ki < 6; ++ki) {
      const Feistel f = make_feistel(domain, keys[ki]);
      if (f.mask != (1u << hb) - 1u) return fail("mask", hb, f.mask, 0, 0);
      std::vector<uint16_t> tab((size_t)6 << hb);
      feistel_round_table(f, tab.data());
      for (size_t e = 0; e < tab.size(); ++e)
        if (tab[e] > f.mask) return fail("entry above mask", hb, ki, (long long)e, tab[e]);
      for (uint32_t i = 0; i < 6; ++i)
        for (uint32_t R = 0; R <= f.mask; ++R)
          if (tab[(i << hb) + R] != (mix32(R * 0x9E3779B1u + f.k[i]) & f.mask))
            return fail("entry", hb, ki, i, R);
      for (int64_t v = 0; v < domain; ++v) {
        const uint64_t want = feistel_once(f, (uint64_t)v);
        const uint32_t got = feistel_once32_tab(tab.data(), hb, f.mask, (uint32_t)v);
        if (want != got) return fail("network", hb, ki, v, got);
      }
    }
    std::printf("ok tables half_bits=%u\n", hb);
  }
  std::printf("done\n");
  return 0;
}
