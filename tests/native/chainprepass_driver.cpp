// Host check of the fused pre-pass grid (csrc/chainclass.h prepass_grid / prepass_role; DESIGN
// §4.1l): for bag counts 1, 2, 63, 64, 2048 and gx + gz of 1, 8 and 9, every (block, wave) of
// the computed grid maps to exactly one role; every bag has exactly one z-class block; every
// (bag, group, side) of k_chain_planes' own grid is covered exactly once, by the wave with the
// same workspace group as before; idle waves exist only in the last block.  The grid bound
// fires where the summed grid passes 2^31 - 1.  Also: the images per thread of the
// register-resident sort at its thresholds, the launch forms, and class_run32 against class_run.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

#include "chainclass.h"

using namespace tw;

#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAIL %s: ", #cond);         \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      std::exit(1);                            \
    }                                          \
  } while (0)

// k_chain_planes' mapping as it stood before planes_wave: wave w of its grid
struct OldWave {
  bool active, zside;
  int v, g;
  int64_t group;
};
static OldWave old_wave(int64_t block, int wid, int n_bags, int gx, int gz) {
  int64_t w = block * kPrepassWaves + wid;
  const int64_t x_waves = (int64_t)n_bags * gx;
  const bool zside = w >= x_waves;
  const int G = zside ? gz : gx;
  if (zside) w -= x_waves;
  if (G == 0 || w >= (int64_t)n_bags * G) return OldWave{false, zside, 0, 0, 0};
  const int v = (int)(w / G), g = (int)(w - (int64_t)v * G);
  return OldWave{true, zside, v, g, (zside ? x_waves : 0) + w};
}

static void check_roles(int n_bags, int gx, int gz) {
  const PrepassGrid grid = prepass_grid(n_bags, gx, gz);
  CHECK(grid.zblocks == n_bags && grid.blocks == grid.zblocks + grid.pblocks, "grid");
  CHECK(grid.pblocks == ((int64_t)n_bags * (gx + gz) + kPrepassWaves - 1) / kPrepassWaves,
        "plane blocks %lld", (long long)grid.pblocks);
  CHECK(prepass_grid_fits(n_bags, gx, gz), "fits");
  std::vector<int> zblocks_of(n_bags, 0);
  std::map<std::tuple<int, int, int>, int> seen;  // (bag, group, side) -> waves
  for (int64_t b = 0; b < grid.blocks; ++b) {
    int idle = 0;
    for (int w = 0; w < kPrepassWaves; ++w) {
      const PrepassRole r = prepass_role(b, w, n_bags, gx, gz);
      if (b < n_bags) {  // the whole block sorts bag b
        CHECK(r.role == kPrepassZClass && r.bag == b, "block %lld wave %d", (long long)b, w);
        if (w == 0) ++zblocks_of[r.bag];
        continue;
      }
      const OldWave o = old_wave(b - n_bags, w, n_bags, gx, gz);
      if (!o.active) {
        CHECK(r.role == kPrepassIdle, "block %lld wave %d", (long long)b, w);
        ++idle;
        continue;
      }
      CHECK(r.role == kPrepassPlanes && r.bag == o.v && r.g == o.g && r.zside == o.zside &&
                r.group == o.group,
            "block %lld wave %d: bag %d g %d side %d group %lld", (long long)b, w, r.bag, r.g,
            (int)r.zside, (long long)r.group);
      CHECK(r.bag >= 0 && r.bag < n_bags && r.g >= 0 && r.g < (r.zside ? gz : gx), "range");
      CHECK(r.group == (r.zside ? (int64_t)n_bags * gx + (int64_t)r.bag * gz + r.g
                                : (int64_t)r.bag * gx + r.g),
            "workspace group");
      ++seen[std::make_tuple(r.bag, r.g, (int)r.zside)];
    }
    CHECK(idle == 0 || b == grid.blocks - 1, "idle waves before the last block");
    CHECK(idle < kPrepassWaves, "a whole idle block");
  }
  for (int v = 0; v < n_bags; ++v) CHECK(zblocks_of[v] == 1, "bag %d: %d blocks", v, zblocks_of[v]);
  CHECK((int64_t)seen.size() == (int64_t)n_bags * (gx + gz), "groups covered: %zu", seen.size());
  for (const auto& kv : seen) CHECK(kv.second == 1, "a group built %d times", kv.second);
  // past the grid: no role
  for (int w = 0; w < kPrepassWaves; ++w)
    CHECK(prepass_role(grid.blocks, w, n_bags, gx, gz).role == kPrepassIdle, "past the grid");
  std::printf("ok roles bags=%d gx=%d gz=%d blocks=%lld\n", n_bags, gx, gz,
              (long long)grid.blocks);
}

static void check_bound() {
  const int64_t lim = ((int64_t)1 << 31) - 1;
  // one group per bag: the wave count stays below 2^31 where the summed grid passes it
  for (int gx = 0; gx <= 1; ++gx) {
    const int gz = 1 - gx;
    int64_t lo = 1, hi = lim;  // the largest n whose grid fits
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) / 2;
      if (prepass_grid(mid, gx, gz).blocks <= lim) lo = mid; else hi = mid - 1;
    }
    CHECK(prepass_grid(lo, gx, gz).blocks <= lim && prepass_grid(lo + 1, gx, gz).blocks > lim,
          "boundary %lld", (long long)lo);
    CHECK(prepass_grid_fits(lo, gx, gz), "fits at %lld", (long long)lo);
    CHECK(!prepass_grid_fits(lo + 1, gx, gz), "refused at %lld", (long long)(lo + 1));
    CHECK((lo + 1) * (gx + gz) < ((int64_t)1 << 31), "the plane waves alone would pass");
  }
  // many groups per bag: the wave count is the bound that fires
  CHECK(prepass_grid_fits(((int64_t)1 << 28) - 1, 4, 4), "2^31 - 8 waves");
  CHECK(!prepass_grid_fits((int64_t)1 << 28, 4, 4), "2^31 waves");
  std::printf("ok bound\n");
}

static void check_forms() {
  CHECK(kPrepassCap >= 16384, "the capacity covers bags of 16384 images");
  CHECK(kPrepassThreads == 256 && kPrepassCapSmall == 4096 && kPrepassCap == 16384, "sizes");
  CHECK(prepass_per_thread(0) == 0 && prepass_per_thread(-1) == 0, "an empty bag streams");
  CHECK(prepass_per_thread(1) == 16 && prepass_per_thread(4096) == 16, "small");
  CHECK(prepass_per_thread(4097) == 64 && prepass_per_thread(16384) == 64, "full");
  CHECK(prepass_per_thread(16385) == 0 && prepass_per_thread((int64_t)1 << 24) == 0, "stream");
  for (int64_t nz = 1; nz <= kPrepassCap; nz += 127)
    CHECK((int64_t)prepass_per_thread(nz) * kPrepassThreads >= nz, "capacity at %lld", (long long)nz);
  for (int mode = 0; mode <= 2; ++mode) {
    CHECK(prepass_form(mode, 0, 15625) == 1, "no class bits: the separate launches");
    CHECK(prepass_form(mode, 8, 16384) == (mode == 1 ? 1 : 2), "resident");
    CHECK(prepass_form(mode, 8, 16385) == (mode == 1 ? 1 : 3), "streaming");
  }
  std::printf("ok forms\n");
}

static void check_runs32() {
  const uint32_t ns[] = {1, 2, 7, 8, 9, 61, 255, 256, 257, 4096, 15625, 16383, 16384, 65535};
  for (uint32_t n : ns)
    for (int64_t chunk : {8, 9, 128, 600, 16384}) {
      const uint32_t nr = (uint32_t)class_runs(n, chunk);
      for (uint32_t j = 0; j < nr; ++j) {
        const ClassRun a = class_run(1000, n, nr, j, 5), b = class_run32(1000, n, nr, j, 5);
        CHECK(a.z0 == b.z0 && a.len == b.len && a.cls == b.cls, "n %u chunk %lld run %u", n,
              (long long)chunk, j);
      }
    }
  std::printf("ok runs32\n");
}

int main() {
  static_assert(kPrepassWaves == 4, "a pre-pass block is four waves");
  const int groups[][2] = {{1, 0}, {0, 1}, {8, 0}, {5, 3}, {8, 1}, {4, 5}};
  for (int n_bags : {1, 2, 63, 64, 2048})
    for (const auto& g : groups) check_roles(n_bags, g[0], g[1]);
  check_bound();
  check_forms();
  check_runs32();
  return 0;
}
