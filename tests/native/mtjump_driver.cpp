// Stand-alone driver of csrc/mtjump.cpp (tests/test_mt_jump.py compiles it with mtjump.cpp and
// numpy_rng.cpp under AddressSanitizer + UBSan and runs it as its own program): phi's degree,
// the polynomial arithmetic, and tw_mt_jump_host against plain stepping (tw_np_mt_next32).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/tuplewise.h"

namespace {

constexpr int kN = 624, kPW = 312;

void seed_key(uint32_t s, uint32_t* key) {  // init_genrand
  key[0] = s;
  for (int i = 1; i < kN; ++i) key[i] = 1812433253u * (key[i - 1] ^ (key[i - 1] >> 30)) + (uint32_t)i;
}

bool jump_matches(uint32_t seed, int pos0, int64_t J) {
  uint32_t a[kN], b[kN];
  seed_key(seed, a);
  int32_t pa = kN, pb;
  if (pos0 != kN) {  // a regenerated key (a true sequence word in key[0]) at position pos0
    uint32_t w;
    tw_np_mt_next32(a, &pa, 1, &w);
    pa = pos0;
  }
  memcpy(b, a, sizeof a);
  pb = pa;
  std::vector<uint32_t> out((size_t)J);
  tw_np_mt_next32(b, &pb, J, out.data());
  if (tw_mt_jump_host(a, &pa, J) != 0) return false;
  return pa == pb && memcmp(a, b, sizeof a) == 0;
}

}  // namespace

int main() {
  uint64_t phi[kPW], phi2[kPW];
  if (tw_mt_minpoly(phi) != 0 || tw_mt_minpoly(phi2) != 0) return 1;
  int deg = -1;
  for (int k = kPW * 64 - 1; k >= 0 && deg < 0; --k)
    if (phi[k >> 6] >> (k & 63) & 1) deg = k;
  if (deg != 19937 || !(phi[0] & 1) || memcmp(phi, phi2, sizeof phi) != 0) {
    printf("FAIL minpoly degree %d\n", deg);
    return 1;
  }
  printf("ok minpoly\n");

  // t^a * t^b == t^(a+b)
  const int64_t as[] = {1, 19936, 19937, 123456, 99999989}, bs[] = {0, 1, 40000, 7654321, 624};
  for (int i = 0; i < 5; ++i) {
    uint64_t pa[kPW], pb[kPW], pab[kPW], prod[kPW];
    if (tw_mt_jump_poly(as[i], pa) || tw_mt_jump_poly(bs[i], pb) ||
        tw_mt_jump_poly(as[i] + bs[i], pab) || tw_mt_poly_mulmod(pa, pb, prod) ||
        memcmp(prod, pab, sizeof prod) != 0) {
      printf("FAIL additivity %lld + %lld\n", (long long)as[i], (long long)bs[i]);
      return 1;
    }
  }
  printf("ok additivity\n");

  // argument errors
  uint32_t key[kN];
  seed_key(1, key);
  int32_t pos = 625;
  if (tw_mt_jump_host(key, &pos, 1) != 1 || tw_mt_jump_host(nullptr, &pos, 1) != 1 ||
      tw_mt_jump_poly(-1, phi2) != 1 || tw_mt_poly_mulmod(phi, phi, phi2) != 1) {
    printf("FAIL argument checks\n");
    return 1;
  }
  printf("ok arguments\n");

  const int64_t Js[] = {0, 1, 623, 624, 625, 1248, 65520, 2 * 65520 + 17, 1000000};
  const int poss[] = {kN, 0, 1, 623};
  for (int pi = 0; pi < 4; ++pi)
    for (int ji = 0; ji < 9; ++ji)
      if (!jump_matches(5489u + (uint32_t)pi, poss[pi], Js[ji])) {
        printf("FAIL jump pos=%d J=%lld\n", poss[pi], (long long)Js[ji]);
        return 1;
      }
  printf("ok jump\n");
  return 0;
}
