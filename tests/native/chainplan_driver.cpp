// Host check of csrc/chainplan.h (the work items of the plane-reading chain count), no GPU:
// tests/test_chainplan_host.py compiles and runs it.  For every plan it enumerates the items of
// a bag and checks that their rectangles tile nx x nz exactly once, that the swap rule picks
// the side with fewer slots, that the padded slots equal the closed form, that the plane
// layout is bits_transpose32's, and pins the bit-sliced-or-packed decision.  Prints one
// "ok <name>" line per check and exits non-zero at the first mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "chainplan.h"

using namespace tw;

static int fail(const char* what, long long a, long long b, long long c, long long d) {
  std::printf("FAIL %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
  return 1;
}

// One bag of nx x nz under plan p: exact tiling, slots, swap rule
static int check_bag(const PlanesPlan& p, int64_t nx, int64_t nz) {
  const PlanesBag b = planes_bag(nx, nz, p.swap != 0);
  const int64_t zg = (nz + kPlaneGroup - 1) / kPlaneGroup;
  const int64_t swapped_slots = (int64_t)b.rx * kPlaneGroup * zg;
  const int64_t padded_slots = (int64_t)kPlaneGroup * nz;
  if (b.swap != (p.swap && b.rx > 0 && swapped_slots < padded_slots))
    return fail("swap rule", nx, nz, swapped_slots, padded_slots);
  if ((int64_t)b.full * kPlaneGroup + b.rx != nx) return fail("split", nx, nz, b.full, b.rx);

  std::vector<PlanesRect> rects;
  int64_t area = 0, slots = 0;
  for (int rem = 0; rem < p.per_bag; ++rem) {
    const PlanesItem it = planes_item(p, nx, nz, rem);
    if (!it.active) continue;
    if (it.ng < 1 || it.ng > p.R || it.ng > 4) return fail("groups per item", nx, nz, rem, it.ng);
    if (it.g0 + it.ng > (it.swapped ? p.gz : p.gx)) return fail("workspace", nx, nz, rem, it.g0);
    if (it.s1 - it.s0 > p.z_chunk) return fail("chunk length", nx, nz, rem, it.s1 - it.s0);
    const PlanesRect r = planes_rect(it, nx, nz);
    if (r.x0 < 0 || r.x0 >= r.x1 || r.x1 > nx || r.z0 < 0 || r.z0 >= r.z1 || r.z1 > nz)
      return fail("rectangle bounds", nx, nz, rem, r.x0);
    if (it.swapped != (r.x0 >= (int64_t)b.full * kPlaneGroup && b.swap))
      return fail("swapped item outside the remainder", nx, nz, rem, r.x0);
    rects.push_back(r);
    area += (r.x1 - r.x0) * (r.z1 - r.z0);
    slots += (int64_t)it.ng * kPlaneGroup * (it.s1 - it.s0);
  }
  if (area != nx * nz) return fail("area", nx, nz, area, nx * nz);
  // exactly once: over every elementary x interval the z intervals tile [0, nz)
  std::vector<int64_t> xs;
  for (const auto& r : rects) {
    xs.push_back(r.x0);
    xs.push_back(r.x1);
  }
  std::sort(xs.begin(), xs.end());
  xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
  std::vector<std::vector<std::pair<int64_t, int64_t>>> cover(xs.size());
  for (const auto& r : rects) {
    size_t i = std::lower_bound(xs.begin(), xs.end(), r.x0) - xs.begin();
    for (; xs[i] < r.x1; ++i) cover[i].push_back({r.z0, r.z1});
  }
  if (nx > 0 && nz > 0 && (xs.empty() || xs.front() != 0 || xs.back() != nx))
    return fail("x cover", nx, nz, xs.empty() ? -1 : xs.front(), xs.empty() ? -1 : xs.back());
  for (size_t i = 0; i + 1 < xs.size(); ++i) {
    auto& c = cover[i];
    std::sort(c.begin(), c.end());
    int64_t at = 0;
    for (const auto& zz : c) {
      if (zz.first != at) return fail("z tiling", nx, nz, xs[i], zz.first);
      at = zz.second;
    }
    if (at != nz) return fail("z cover", nx, nz, xs[i], at);
  }
  // padded slots: the closed form of the chosen side, never more than the other side's
  const int64_t pad = slots - nx * nz;
  const int64_t pad_swap = (int64_t)b.rx * (kPlaneGroup * zg - nz);
  const int64_t pad_group = b.rx > 0 ? (int64_t)(kPlaneGroup - b.rx) * nz : 0;
  const int64_t want = b.swap ? pad_swap : pad_group;
  if (pad != want) return fail("padded slots", nx, nz, pad, want);
  if (p.swap && b.rx > 0 && nz > 0 &&
      pad > std::min(swapped_slots, padded_slots) - (int64_t)b.rx * nz)
    return fail("not the cheaper side", nx, nz, pad, 0);
  return 0;
}

static int check_plans() {
  const int64_t sizes[] = {0, 1, 63, 2047, 2048, 2049, 4101, 15625, 100000};
  long long bags = 0;
  for (int R : {2, 3, 4})
    for (int64_t zc : {(int64_t)8, (int64_t)600, (int64_t)0})
      for (int64_t nx : sizes)
        for (int64_t nz : sizes) {
          // the bag alone, and as a ragged bag of a launch whose largest is 100000 x 100000
          for (int ragged = 0; ragged < 2; ++ragged) {
            const int64_t mx = ragged ? 100000 : nx, mz = ragged ? 100000 : nz;
            for (int64_t n_bags : {(int64_t)1, (int64_t)64}) {
              if (zc != 0 && n_bags != 1) continue;  // (n_bags enters the automatic chunk only)
              const PlanesPlan p = planes_plan(mx, mz, n_bags, R, zc, 2);
              if (p.R != R || p.z_chunk < 2 || (p.z_chunk & 1) ||
                  p.per_bag != p.tiles_x * p.zchunks + p.tiles_s * p.schunks)
                return fail("plan", nx, nz, R, zc);
              if (zc != 0 && (p.z_chunk > zc || p.zchunks != (mz + zc - 1) / zc))
                return fail("forced chunk", nx, nz, R, zc);
              if (check_bag(p, nx, nz)) return 1;
              // (the A/B form without swapped items: every remainder a padded group)
              if (check_bag(planes_plan(mx, mz, n_bags, R, zc, 0), nx, nz)) return 1;
              if (check_bag(planes_plan(mx, mz, n_bags, R, zc, 1), nx, nz)) return 1;
              ++bags;
            }
          }
        }
  // the automatic plan: R = 4; the swap only in launches of many items
  if (planes_plan(15625, 15625, 1280, 0, 0).R != 4 || !planes_plan(15625, 15625, 1280, 0, 0).swap ||
      planes_plan(15625, 15625, 32, 0, 0).swap || planes_plan(15625, 15625, 1280, 0, 0, 0).swap ||
      !planes_plan(15625, 15625, 32, 0, 0, 2).swap)
    return fail("automatic plan", 0, 0, 0, 0);
  // the bench shape: 7 full groups as 4 + 3, the 1289-image remainder swapped
  {
    const PlanesBag b = planes_bag(15625, 15625);
    if (b.full != 7 || b.rx != 1289 || !b.swap || b.xgroups != 7 || b.zgroups != 8)
      return fail("bench bag", b.full, b.rx, b.swap, b.zgroups);
  }
  std::printf("ok plans (%lld bags)\n", bags);
  return 0;
}

// The pre-pass's layout: a lane's 32 images of a group transposed are its NB plane words
template <int NB>
static int check_layout(std::mt19937& g) {
  const int64_t n = 3 * kPlaneGroup + 777;  // a ragged last group
  const int groups = 4;
  std::uniform_int_distribution<uint32_t> any(0, (uint32_t)(((uint64_t)1 << NB) - 1));
  std::vector<uint32_t> img(n);
  for (auto& v : img) v = any(g);
  std::vector<uint32_t> work((size_t)groups * NB * 64, 0xFFFFFFFFu);
  for (int gr = 0; gr < groups; ++gr)
    for (int lane = 0; lane < 64; ++lane) {
      uint32_t a[32];
      for (int k = 0; k < 32; ++k) {
        const int64_t i = planes_image(gr, k, lane);
        a[k] = i < n ? img[i] : 0u;
      }
      bits_transpose32(a);
      for (int b = 0; b < NB; ++b) work[planes_word(NB, gr, b, lane)] = a[b];
    }
  std::vector<char> seen(n, 0);
  for (int gr = 0; gr < groups; ++gr)
    for (int b = 0; b < NB; ++b)
      for (int lane = 0; lane < 64; ++lane) {
        const uint32_t w = work[((size_t)gr * NB + b) * 64 + lane];  // [group][plane][lane]
        for (int k = 0; k < 32; ++k) {
          const int64_t i = (int64_t)gr * kPlaneGroup + k * 64 + lane;
          const uint32_t want = i < n ? (img[i] >> b) & 1u : 0u;
          if (((w >> k) & 1u) != want) return fail("plane layout", NB, gr, b, lane);
          if (i < n) seen[i] = 1;
        }
      }
  for (int64_t i = 0; i < n; ++i)
    if (!seen[i]) return fail("image not in any slot", NB, i, 0, 0);
  if (planes_work_words(n, 1, 1, NB) != (int64_t)(groups + 1) * NB * 64)
    return fail("workspace words", NB, 0, 0, 0);
  std::printf("ok layout NB=%d\n", NB);
  return 0;
}

// chain_count_sliced: which bounded launches run bit-sliced (true) and which packed
static int check_decision() {
  const int nb = bits_pick_nb(1000000);  // 20 planes
  const struct {
    int64_t max_nx;
    bool sliced;
  } automatic[] = {{3072, false}, {3073, true},  {4096, true},  {4097, false},  {4500, false},
                   {6144, false}, {6145, true},  {15625, true}, {100000, true}};
  for (const auto& c : automatic)
    if (chain_count_sliced(c.max_nx, 0, false, nb) != c.sliced)
      return fail("automatic decision", c.max_nx, c.sliced, nb, 0);
  for (int R : {2, 3, 4})  // the plane plans forced: sliced however small the bag
    if (!chain_count_sliced(1, R, false, nb)) return fail("forced planes", 1, R, nb, 0);
  for (int R : {8, 16})  // the packed plans forced
    if (chain_count_sliced(15625, R, false, nb)) return fail("forced packed", 15625, R, nb, 0);
  for (int R : {0, 2, 3, 4, 8, 16}) {
    if (chain_count_sliced(15625, R, true, nb)) return fail("half ties", 15625, R, nb, 1);
    // no bound below 2^24: no plane count holds the images
    if (chain_count_sliced(15625, R, false, bits_pick_nb((int64_t)1 << 24)))
      return fail("bound 2^24", 15625, R, 0, 0);
  }
  std::printf("ok decision\n");
  return 0;
}

int main() {
  std::mt19937 g(20240607u);
  if (check_plans() || check_decision()) return 1;
  if (check_layout<16>(g) || check_layout<18>(g) || check_layout<20>(g) || check_layout<22>(g) ||
      check_layout<24>(g))
    return 1;
  std::printf("done\n");
  return 0;
}
