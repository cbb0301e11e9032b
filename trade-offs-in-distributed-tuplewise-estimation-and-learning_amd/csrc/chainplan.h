// chainplan.h — the work items of the plane-reading chain count (csrc/chain.hip's
// k_chain_planes + k_count_chain_planes).
//
// A bag's bit planes (bitcount.h) are built ONCE per launch by a pre-pass, in groups of
// kPlaneGroup images, and the count's items read them:
//  * a PLANE item: up to R consecutive x groups (lane side) against one z chunk (the
//    wave-uniform scalar side);
//  * a SWAPPED item, for the x remainder rx = nx mod kPlaneGroup: x > z is the carry out of
//    x + ~z, symmetric in its operands, so the remainder's x images are the scalars
//    (uncomplemented; NaN and "never" images 0, which carry against nothing) and up to R
//    groups of the bag's complemented z planes the lane side.
// The remainder is swapped where that takes fewer slots than padding it to a whole x group:
//     rx * kPlaneGroup * ceil(nz / kPlaneGroup)  <  kPlaneGroup * nz.
// Everything here is plain C++ (host and device): tests/native/chainplan_driver.cpp
// enumerates the items of a plan and checks that they tile nx x nz exactly once.
#pragma once
#include <stdint.h>

#include "bitcount.h"

namespace tw {

constexpr int kPlaneGroup = 64 * 32;  // images of one plane group: 32 per lane

// Plan constants (automatic plan).  Items no longer open with their transposes, so they can be
// short: z chunks of >= kPlanesMinZ images, as many as give ~kPlanesItems items (64 per wave
// slot of the device at 4 waves per SIMD) — the launch's tail is then a few percent of it
// whatever the items' mix of costs.  The remainder is swapped only in launches of at least
// kPlanesSwapItems plane items: in smaller ones the extra, shorter items lengthen the tail
// by more than the padding they save.  (Sweeps: DESIGN §4.1f, profiles/r09_count_planes_*.)
constexpr int64_t kPlanesItems = 256 * 4 * 4 * 64;
constexpr int64_t kPlanesMinZ = 128;
constexpr int64_t kPlanesSwapItems = 256 * 4 * 4 * 4;

// Workspace layout, u32 words: the x planes [bag][gx][NB][64], then the z planes
// [bag][gz][NB][64].  Group g, plane b, lane l; bit k of that word is bit b of image
// g * kPlaneGroup + k * 64 + l of the bag.
TW_BITS_HD int64_t planes_image(int g, int k, int lane) {
  return (int64_t)g * kPlaneGroup + k * 64 + lane;
}
TW_BITS_HD int64_t planes_word(int nb, int64_t group, int b, int lane) {
  return (group * nb + b) * 64 + lane;
}

struct PlanesPlan {
  int R;                 // largest groups per item (1..4)
  int gx, gz;            // groups per bag in the workspace: ceil(max_nx or max_nz / group)
  int tiles_x, zchunks;  // plane items per bag: x tiles of R groups x z chunks
  int tiles_s, schunks;  // swapped items per bag: z tiles of R groups x remainder chunks
  int per_bag;           // tiles_x * zchunks + tiles_s * schunks
  int64_t z_chunk;       // scalar-side images per item, even
  int swap;              // 1: remainders are swapped where planes_bag's rule says so
};

TW_BITS_HD int64_t planes_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Whether a launch counts bit-sliced (on planes) or with the packed kernel (k_count_chain).
// nb: bits_pick_nb of the caller's image bound (0: none promised, or none below 2^24); forced_R:
// tw_count_chain_set_plan's R (0 automatic; 8, 16 force the packed kernel, 2 .. 4 the planes).
// Bit-sliced needs the strict predicate and nb > 0.  Under the automatic plan a bag much
// smaller than a plane tile pads more slots than the bit-sliced loop gains (1.39x per slot,
// profiles/r07_mb_bits.log): the least slots of tiles of 2 or 4 groups — max_nx rounded up to
// the tile — past kBitsMaxPad x the least slots of the packed kernel's 16 or 8 images per lane
// keep the launch packed.  Interleaved A/B against the packed kernel (tools/count_bits_ab.py,
// profiles/r07_count_bits_ab.json): headline K = 20 8.48 -> 5.77 ms, K = 32 13.26 -> 9.07,
// K = 4 1.79 -> 1.19; per-rank shapes G = 2 / 4 / 8 at K = 20 0.66-0.67 of the packed time, C2
// (one 1e5 x 1e5 bag) 0.294 -> 0.260; none slower.
constexpr double kBitsMaxPad = 1.25;
TW_BITS_HD int64_t planes_padded(int64_t n, int64_t tile) {  // n rounded up to whole tiles
  return planes_ceil_div(n, tile) * tile;
}
TW_BITS_HD bool chain_count_sliced(int64_t max_nx, int forced_R, bool half, int nb) {
  if (half || nb <= 0 || forced_R == 8 || forced_R == 16) return false;
  if (forced_R != 0) return true;
  const int64_t p16 = planes_padded(max_nx, 64 * 16), p8 = planes_padded(max_nx, 64 * 8);
  const int64_t s2 = planes_padded(max_nx, 2 * kPlaneGroup);
  const int64_t s4 = planes_padded(max_nx, 4 * kPlaneGroup);
  return (double)(s2 < s4 ? s2 : s4) <= kBitsMaxPad * (double)(p16 < p8 ? p16 : p8);
}

// R, z_chunk: 0 = automatic (R = 4); swap: 0 never, 1 by the rule above, 2 always
TW_BITS_HD PlanesPlan planes_plan(int64_t max_nx, int64_t max_nz, int64_t n_bags, int R,
                                  int64_t z_chunk, int swap = 1) {
  PlanesPlan p{};
  p.gx = (int)planes_ceil_div(max_nx, kPlaneGroup);
  p.gz = (int)planes_ceil_div(max_nz, kPlaneGroup);
  if (R <= 0) R = 4;
  p.R = R;
  p.tiles_x = (int)planes_ceil_div(p.gx, R);
  p.tiles_s = (int)planes_ceil_div(p.gz, R);
  int64_t zc = z_chunk;
  if (zc <= 0) {
    const int64_t base = (int64_t)p.tiles_x * n_bags;
    const int64_t want = planes_ceil_div(kPlanesItems, base > 0 ? base : 1);
    zc = planes_ceil_div(max_nz, want > 0 ? want : 1);
    if (zc < kPlanesMinZ) zc = kPlanesMinZ;
  }
  if (zc > ((int64_t)1 << 24)) zc = (int64_t)1 << 24;  // u32 lane counters: 32 per scalar
  if (zc > max_nz) zc = max_nz;
  if (zc < 2) zc = 2;
  p.z_chunk = planes_ceil_div(zc, 2) * 2;
  p.zchunks = (int)planes_ceil_div(max_nz, p.z_chunk);
  if (p.zchunks > 0)  // the same number of chunks, of equal (even) length: no short last one
    p.z_chunk = planes_ceil_div(planes_ceil_div(max_nz, p.zchunks), 2) * 2;
  const int64_t max_rx = max_nx < kPlaneGroup ? max_nx : kPlaneGroup - 1;
  p.swap = swap == 2 ||
           (swap == 1 && (int64_t)p.tiles_x * p.zchunks * n_bags >= kPlanesSwapItems);
  p.schunks = p.swap ? (int)planes_ceil_div(max_rx, p.z_chunk) : 0;
  p.per_bag = p.tiles_x * p.zchunks + p.tiles_s * p.schunks;
  return p;
}

// One bag's split, from its own sizes (bags may be ragged)
struct PlanesBag {
  int full, rx;  // nx = full * kPlaneGroup + rx
  bool swap;     // the remainder goes through swapped items
  int xgroups;   // x groups the plane items read: full (+ 1: a padded remainder)
  int zgroups;   // z groups the swapped items read: ceil(nz / group), 0 without swap
};
TW_BITS_HD PlanesBag planes_bag(int64_t nx, int64_t nz, bool swap = true) {
  PlanesBag b{};
  b.full = (int)(nx / kPlaneGroup);
  b.rx = (int)(nx - (int64_t)b.full * kPlaneGroup);
  const int64_t zg = planes_ceil_div(nz, kPlaneGroup);
  b.swap = swap && b.rx > 0 && (int64_t)b.rx * zg < nz;
  b.xgroups = b.full + (b.rx > 0 && !b.swap ? 1 : 0);
  b.zgroups = b.swap ? (int)zg : 0;
  return b;
}

// Item `rem` in [0, per_bag) of a bag: the lane side is groups [g0, g0 + ng) of the x planes
// (swapped: of the z planes), the scalar side images [s0, s1) of the bag's z (swapped: x).
struct PlanesItem {
  bool active, swapped;
  int g0, ng;
  int64_t s0, s1;
};
TW_BITS_HD PlanesItem planes_item(const PlanesPlan& p, int64_t nx, int64_t nz, int rem) {
  PlanesItem it{};
  const PlanesBag b = planes_bag(nx, nz, p.swap != 0);
  const int n_plane = p.tiles_x * p.zchunks;
  if (rem < n_plane) {
    // tile-major: the waves of a block read the same planes and cost the same
    const int tx = rem / p.zchunks, cz = rem - tx * p.zchunks;
    it.g0 = tx * p.R;
    const int lim = b.xgroups < p.gx ? b.xgroups : p.gx;  // (never past the workspace)
    it.ng = lim - it.g0 < p.R ? lim - it.g0 : p.R;
    it.s0 = (int64_t)cz * p.z_chunk;
    it.s1 = it.s0 + p.z_chunk < nz ? it.s0 + p.z_chunk : nz;
  } else {
    rem -= n_plane;
    it.swapped = true;
    const int ts = rem / p.schunks, cs = rem - ts * p.schunks;
    it.g0 = ts * p.R;
    const int lim = b.zgroups < p.gz ? b.zgroups : p.gz;
    it.ng = lim - it.g0 < p.R ? lim - it.g0 : p.R;
    // the remainder in chunks of even, equal length (as few as z_chunk allows)
    const int64_t nsc = planes_ceil_div(b.rx, p.z_chunk);
    const int64_t len = nsc > 0 ? planes_ceil_div(planes_ceil_div(b.rx, nsc), 2) * 2 : 0;
    const int64_t x0 = (int64_t)b.full * kPlaneGroup;
    it.s0 = x0 + cs * len;
    it.s1 = it.s0 + len < nx ? it.s0 + len : nx;
  }
  it.active = it.ng > 0 && it.s0 < it.s1;
  return it;
}

// The pairs an item decides: x images [x0, x1) against z images [z0, z1) of the bag
struct PlanesRect {
  int64_t x0, x1, z0, z1;
};
TW_BITS_HD PlanesRect planes_rect(const PlanesItem& it, int64_t nx, int64_t nz) {
  const int64_t l0 = (int64_t)it.g0 * kPlaneGroup, l1 = l0 + (int64_t)it.ng * kPlaneGroup;
  if (it.swapped) return PlanesRect{it.s0, it.s1, l0, l1 < nz ? l1 : nz};
  return PlanesRect{l0, l1 < nx ? l1 : nx, it.s0, it.s1};
}

// Words of the workspace for n_bags bags of at most max_nx x max_nz images at nb planes
TW_BITS_HD int64_t planes_work_words(int64_t max_nx, int64_t max_nz, int64_t n_bags, int nb) {
  return n_bags * (planes_ceil_div(max_nx, kPlaneGroup) + planes_ceil_div(max_nz, kPlaneGroup)) *
         nb * 64;
}

}  // namespace tw
