// Host check of csrc/bitcount.h (the bit-sliced compare-and-count's helpers), no GPU:
// tests/test_bitcount_host.py compiles and runs it.  Prints one "ok <name>" line per check and
// exits non-zero at the first mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "bitcount.h"

using namespace tw;

static int fail(const char* what, long a, long b) {
  std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
  return 1;
}

// 32 images -> planes, one z: the carry chain's 32 outcomes against x > z
template <int NB>
static int check_group(const uint32_t (&x)[32], uint32_t z, const char* what) {
  uint32_t a[32];
  for (int k = 0; k < 32; ++k) a[k] = x[k];
  bits_transpose32(a);
  uint32_t pl[NB];
  for (int b = 0; b < NB; ++b) pl[b] = a[b];
  const uint32_t c = bits_gt32<NB>(pl, ~z);
  uint32_t want = 0, n = 0;
  for (int k = 0; k < 32; ++k)
    if (x[k] > z) {
      want |= 1u << k;
      ++n;
    }
  if (c != want) return fail(what, (long)z, (long)c);
  if (bits_popc_add(c, 5u) != 5u + n) return fail("popcount", (long)c, (long)n);
  return 0;
}

template <int NB>
static int check_random(std::mt19937& g) {
  const uint32_t top = (uint32_t)(((uint64_t)1 << NB) - 1);
  std::uniform_int_distribution<uint32_t> any(0, top), small(0, 40);
  for (int it = 0; it < 4000; ++it) {
    uint32_t x[32];
    const uint32_t z = it % 7 == 0 ? 0u : it % 7 == 1 ? top : it % 7 == 2 ? small(g) : any(g);
    for (int k = 0; k < 32; ++k) {
      switch ((it + k) % 6) {
        case 0: x[k] = z; break;                       // ties
        case 1: x[k] = 0; break;
        case 2: x[k] = top; break;
        case 3: x[k] = z > 0 ? z - 1 : 0; break;
        case 4: x[k] = z < top ? z + 1 : top; break;
        default: x[k] = any(g);
      }
    }
    if (check_group<NB>(x, z, "carry chain (random)")) return 1;
  }
  std::printf("ok random NB=%d\n", NB);
  return 0;
}

int main() {
  std::mt19937 g(20240607u);
  {  // the transpose: bit k of a[b] = bit b of the former a[k]; twice = identity
    for (int it = 0; it < 200; ++it) {
      uint32_t a[32], t[32];
      for (int k = 0; k < 32; ++k) a[k] = t[k] = (uint32_t)g();
      bits_transpose32(t);
      for (int b = 0; b < 32; ++b)
        for (int k = 0; k < 32; ++k)
          if (((t[b] >> k) & 1u) != ((a[k] >> b) & 1u)) return fail("transpose", b, k);
      bits_transpose32(t);
      for (int k = 0; k < 32; ++k)
        if (t[k] != a[k]) return fail("transpose round trip", k, it);
    }
    std::printf("ok transpose\n");
  }
  {  // NB = 8, every (x, z) pair: x fills the 32 slots 32 values at a time
    for (uint32_t z = 0; z < 256; ++z)
      for (uint32_t x0 = 0; x0 < 256; x0 += 32) {
        uint32_t x[32];
        for (int k = 0; k < 32; ++k) x[k] = x0 + (uint32_t)k;
        if (check_group<8>(x, z, "carry chain (exhaustive NB=8)")) return 1;
      }
    std::printf("ok exhaustive NB=8\n");
  }
  if (check_random<16>(g) || check_random<18>(g) || check_random<20>(g) || check_random<22>(g) ||
      check_random<24>(g))
    return 1;
  {  // image conversion and the plane count chosen for a bound
    if (bits_x_image(-33554432.0f) != 0u || bits_x_image(0.0f) != 0u ||
        bits_x_image(std::nanf("")) != 0u || bits_x_image(16777215.0f) != 16777215u ||
        bits_x_image(7.0f) != 7u)
      return fail("x image", 0, 0);
    if (bits_z_image(-0.0f) != ~0u || bits_z_image(0.0f) != ~0u || bits_z_image(-7.0f) != ~7u ||
        bits_z_image(-16777215.0f) != ~16777215u)
      return fail("z image", 0, 0);
    const long bounds[] = {0, 65535, 65536, 262143, 262144, 1000000, 1048575, 1048576,
                           4194303, 4194304, 16777215, 16777216, -1};
    const int want[] = {16, 16, 18, 18, 20, 20, 20, 22, 22, 24, 24, 0, 0};
    for (int i = 0; i < 13; ++i)
      if (bits_pick_nb(bounds[i]) != want[i]) return fail("plane count", bounds[i], want[i]);
    // a padded z slot counts nothing, whatever the x images
    uint32_t pl[24];
    for (int b = 0; b < 24; ++b) pl[b] = ~0u;
    if (bits_gt32<24>(pl, kBitsZNever) != 0u) return fail("padded z", 0, 0);
    std::printf("ok images\n");
  }
  return 0;
}
