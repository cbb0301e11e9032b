// chainclass.h — the class-run form of the plane-reading chain count (csrc/chain.hip's
// k_chain_zclasses + k_count_chain_classes), beside chainplan.h's items.
//
// With zc the complemented z image, x > z is the carry out of x + zc over NB bits (bitcount.h).
// Split the bits into the low bits [0, NB - k) and a TOP FIELD [NB - k, NB), and let D be the
// top field of zc — the z image's CLASS.  For a carry c into the top field the carry out is
//     G | (P & c),   G = the top field's own chain with carry-in 0    (x_top >  z_top)
//                    P = the same chain with carry-in all-ones         (x_top >= z_top)
// and G is a subset of P, so that is majority(G, P, c): one bits_carry with three VGPR sources.
// G and P depend on the x planes and D alone.  The scalar-side z of a bag are therefore grouped
// by class once per launch (a counting sort into a class-ordered region of the workspace) and
// an item compares its x groups against a RUN of z of one class: G and P once per item and
// group (2 k instructions), then (NB - k) + 1 + 1 per z and group instead of NB + 1.  Every
// pair still gets its own low-bit chain and its own popcount bit; only the subexpression
// common to a class is hoisted.
//
// Two properties the count depends on (tests/native/chainclass_driver.cpp checks both):
//  * a padded x slot (plane words 0) counts nothing: its low carry is 0 and its G is 0;
//  * a padded SCALAR slot is NOT harmless here — complemented 0 leaves c = 0 but counts G — so
//    the class loop takes exactly the run's images and never evaluates a slot past its end.
//
// The class-constant term.  G is a subset of P, so with E = P & ~G — the x whose
// top field EQUALS the class —
//     popc(G | (P & c)) = popc(G) + popc(E & c):
// popc(G) is the same for every z of a run and is counted once per item as len * popc(G), with
// len the run's exact length.  E & c needs no instruction of its own: a slot whose low planes
// are all 0 never carries from carry-in 0, so the low chain on the planes ANDed with E once per
// item yields exactly E & c.  Per z and group the lane side is then NL + 1 (the chain and one
// popcount).  Every pair still runs through its own low-bit chain.
//
// Everything here is plain C++ (host and device).
#pragma once
#include <stdint.h>

#include "bitcount.h"
#include "chainplan.h"

namespace tw {

constexpr int kClassMaxBits = 8;        // class bits k: 1 .. min(8, NB - 8)
constexpr int64_t kClassMinChunk = 8;   // shortest run length a plan may ask for

// The class of a complemented z image: the top k of its low nb bits
TW_BITS_HD uint32_t class_of(uint32_t zc, int nb, int k) {
  return (zc >> (nb - k)) & ((1u << k) - 1u);
}

// G and P of one x group against class D: top[b] is plane NB - K + b
template <int K>
TW_BITS_HD void class_gp(const uint32_t (&top)[K], uint32_t D, uint32_t& G, uint32_t& P) {
  const uint32_t m0 = bits_mask(D, 0);
  G = top[0] & m0;  // carry-in 0
  P = top[0] | m0;  // carry-in all-ones
#pragma unroll
  for (int b = 1; b < K; ++b) {
    const uint32_t m = bits_mask(D, b);
    G = bits_carry(top[b], m, G);
    P = bits_carry(top[b], m, P);
  }
}

// [x_k > z] for the 32 images of a group from its NL low planes, G and P of z's class
template <int NL>
TW_BITS_HD uint32_t class_gt32(const uint32_t (&low)[NL], uint32_t G, uint32_t P, uint32_t zc) {
  return bits_carry(G, P, bits_gt32<NL>(low, zc));
}

// E: the x of a group whose top field equals the class (G subset of P)
TW_BITS_HD uint32_t class_equal_mask(uint32_t G, uint32_t P) { return P & ~G; }

// The low planes of a group ANDed with E, once per item and group
template <int NL>
TW_BITS_HD void class_mask_planes(const uint32_t (&low)[NL], uint32_t E, uint32_t (&masked)[NL]) {
#pragma unroll
  for (int b = 0; b < NL; ++b) masked[b] = low[b] & E;
}

// The masked form of class_gt32: popc(class_gt32(low, G, P, zc)) == popc(constant) + popc(word)
// with constant = G for every z of the class and word = E & c_low from the MASKED planes
struct ClassMasked {
  uint32_t constant, word;  // disjoint: G and a subset of E
};
template <int NL>
TW_BITS_HD ClassMasked class_gt32_masked(const uint32_t (&masked)[NL], uint32_t G, uint32_t zc) {
  return ClassMasked{G, bits_gt32<NL>(masked, zc)};
}

// ---------------------------------------------------------------------------- the run table
// Per bag: for each non-empty class, ceil(n_c / chunk) runs of near-equal length over the
// class's range of the class-ordered region, classes in ascending order.  An entry is two u32
// words {z0 | class << 24, len} (z0 < 2^24: bags of < 2^24 z images; class < 2^8).
struct ClassRun {
  int64_t z0, len;
  uint32_t cls;
};

// Runs never ask for fewer than kClassMinChunk images, whatever the plan's z chunk: the
// workspace is sized without knowing the plan (the tuning hooks may change between the sizing
// call and the count).
TW_BITS_HD int64_t class_chunk(int64_t z_chunk) {
  return z_chunk < kClassMinChunk ? kClassMinChunk : z_chunk;
}
TW_BITS_HD int64_t class_runs(int64_t n, int64_t chunk) { return planes_ceil_div(n, chunk); }
// run j of the nr = class_runs(n, chunk) runs of a class whose range is [c0, c0 + n)
TW_BITS_HD ClassRun class_run(int64_t c0, int64_t n, int64_t nr, int64_t j, uint32_t cls) {
  const int64_t a = j * n / nr, b = (j + 1) * n / nr;
  return ClassRun{c0 + a, b - a, cls};
}
TW_BITS_HD uint32_t class_entry_lo(const ClassRun& r) { return (uint32_t)r.z0 | (r.cls << 24); }
TW_BITS_HD uint32_t class_entry_hi(const ClassRun& r) { return (uint32_t)r.len; }
TW_BITS_HD ClassRun class_entry(uint32_t lo, uint32_t hi) {
  return ClassRun{(int64_t)(lo & 0xFFFFFFu), (int64_t)hi, lo >> 24};
}

// Entries a bag's table can hold: every non-empty class has at most one run shorter than
// chunk, so sum ceil(n_c / chunk) <= 2^k + nz / chunk.
TW_BITS_HD int64_t class_capacity(int64_t max_nz, int k, int64_t z_chunk) {
  return ((int64_t)1 << k) + planes_ceil_div(max_nz, class_chunk(z_chunk));
}

// The whole table of one bag from its class histogram (the device builds the same entries with
// one thread per class: class_runs + class_run at the scanned offsets).  tab: 2 words per
// entry; returns the number of entries.
TW_BITS_HD int64_t class_table(const uint32_t* hist, int k, int64_t z_chunk, uint32_t* tab) {
  const int64_t chunk = class_chunk(z_chunk);
  int64_t c0 = 0, e = 0;
  for (uint32_t c = 0; c < (1u << k); ++c) {
    const int64_t n = hist[c], nr = class_runs(n, chunk);
    for (int64_t j = 0; j < nr; ++j, ++e) {
      const ClassRun r = class_run(c0, n, nr, j, c);
      tab[2 * e] = class_entry_lo(r);
      tab[2 * e + 1] = class_entry_hi(r);
    }
    c0 += n;
  }
  return e;
}

// ------------------------------------------------------------------------------ the regions
// u32 words after chainplan.h's planes: the class-ordered complemented z images
// [bag][zs_stride], the bags' entry counts [bag], the run tables [bag][cap][2].  Sized for the
// largest table any plan can ask for (k = kClassMaxBits, runs of kClassMinChunk); a launch
// lays its own, smaller table out at the stride of its own capacity.
TW_BITS_HD int64_t class_round64(int64_t n) { return planes_ceil_div(n, 64) * 64; }
TW_BITS_HD int64_t class_work_words(int64_t max_nz, int64_t n_bags) {
  return n_bags * (class_round64(max_nz) +
                   2 * class_capacity(max_nz, kClassMaxBits, kClassMinChunk)) +
         class_round64(n_bags);
}

struct ClassPlan {
  int k;              // class bits; 0: classes off (k_count_chain_planes)
  int cap;            // table entries per bag of this launch
  int per_bag;        // items per bag: tiles_x * cap + tiles_s * schunks
  int64_t chunk;      // longest run
  int64_t zs_stride;  // words per bag of the class-ordered region
  int64_t off_zs, off_cnt, off_tab;  // word offsets into the workspace
};

TW_BITS_HD ClassPlan class_plan(const PlanesPlan& p, int64_t max_nx, int64_t max_nz,
                                int64_t n_bags, int nb, int k) {
  ClassPlan c{};
  c.k = k;
  c.chunk = class_chunk(p.z_chunk);
  c.cap = (int)class_capacity(max_nz, k, p.z_chunk);
  c.per_bag = p.tiles_x * c.cap + p.tiles_s * p.schunks;
  c.zs_stride = class_round64(max_nz);
  c.off_zs = planes_work_words(max_nx, max_nz, n_bags, nb);
  c.off_cnt = c.off_zs + n_bags * c.zs_stride;
  c.off_tab = c.off_cnt + class_round64(n_bags);
  return c;
}
// words this launch's regions reach (<= planes_work_words + class_work_words)
TW_BITS_HD int64_t class_plan_end(const ClassPlan& c, int64_t n_bags) {
  return c.off_tab + n_bags * 2 * (int64_t)c.cap;
}

// The automatic class bits: the largest k <= min(8, NB - 8) whose mean run max_nz / 2^k stays
// >= kClassMinRun — the shortest measured (k = 8 at the bench's 15625-image bags, runs of 61)
// was the fastest at every multi-bag shape, so the bound only keeps tiny bags from runs of a
// few images that no longer amortise an item's plane loads and its G / P — and none in
// launches of fewer than kClassMinBags bags: pre-pass 2 sorts a bag per block, so with few
// bags it runs on a few CUs for as long as one bag takes (C2's single 1e5-image bag: 1.17x
// the time of k = 0 at best; 32 bags of 15625: 0.82x).  Sweeps: DESIGN §4.1g,
// profiles/r10_count_classes_sweep.json, profiles/r10_count_classes_ab.json.
constexpr int64_t kClassMinRun = 48;
constexpr int64_t kClassMinBags = 32;
TW_BITS_HD int class_bits_auto(int64_t max_nz, int64_t n_bags, int nb) {
  if (n_bags < kClassMinBags) return 0;
  int k = 0;
  while (k < kClassMaxBits && k < nb - 8 && max_nz / ((int64_t)2 << k) >= kClassMinRun) ++k;
  return k;
}

// The swap mode a launch plans with (0 never, 1 chainplan.h's rule, 2 always) from the hook's
// setting.  chainplan.h's automatic rule swaps the x remainder where it takes fewer SLOTS; under
// class runs a padded slot costs NL + 1 VALU per z and group and a swapped one NB + 1.25, so the
// automatic setting keeps the swap only where the swapped remainder of the largest bag is also
// the cheaper in instructions: rx * ceil(nz / 2048) * (NB + 1.25) < nz * (NL + 1).  At the bench
// shape (rx = 1289, nz = 15625, NB = 20, k = 8: 219 k against 203 k) that is no swap, measured
// 0.93-0.95 of the swapped launch's time; a remainder of a few images stays
// swapped.  Forced settings and launches without classes are left alone.
TW_BITS_HD int class_swap_mode(int swap, int64_t max_nx, int64_t max_nz, int nb, int k) {
  if (k == 0 || swap != 1) return swap;
  const int64_t rx = max_nx % kPlaneGroup, zg = planes_ceil_div(max_nz, kPlaneGroup);
  return rx * zg * (4 * nb + 5) < max_nz * 4 * (nb - k + 1) ? 1 : 0;
}

#if defined(__HIPCC__)
// Build-time forms of the class loop (csrc/Makefile ab-classform):
//   0  §4.1g's loop: bits_carry(G, P, c) per z, the images through a VGPR and v_readlane_b32
//   1  masked low planes: the chain's carry is counted as it is, len * popc(G) once per item
//   2  form 1 with the run read by scalar loads, TW_CLASS_BATCH images per load
#ifndef TW_CLASS_FORM
#define TW_CLASS_FORM 2
#endif
#ifndef TW_CLASS_BATCH
#define TW_CLASS_BATCH 4
#endif
static_assert(TW_CLASS_FORM >= 0 && TW_CLASS_FORM <= 2, "TW_CLASS_FORM: 0, 1 or 2");
static_assert(TW_CLASS_BATCH == 2 || TW_CLASS_BATCH == 4 || TW_CLASS_BATCH == 8 ||
                  TW_CLASS_BATCH == 16,
              "TW_CLASS_BATCH: a scalar load's width in words");
// A scalar batch starts inside its run and may read up to TW_CLASS_BATCH - 1 words past the
// run's end: into the same bag's later runs, the next bag's region or — from the last run of the
// last bag — the entry counts, class_round64(n_bags) >= 64 words that follow the class-ordered
// region (class_plan: off_cnt = off_zs + n_bags * zs_stride).  Always inside the workspace; the
// words read past the end are never compared.
static_assert(TW_CLASS_BATCH - 1 < 64, "the over-read must stay inside the count region");

// One wave item: R groups of NB plane words per lane at pw (bits_count_planes' layout) against
// the run's len >= 1 images at zs, complemented u32 of class cls (wave-uniform).  Exactly len
// images are compared: a padded scalar slot would count G (form 0) or be missed by the
// len * popc(G) term (forms 1, 2).
//  Forms 0, 1: the images go 64 at a time through one VGPR, the next 64 in flight, and reach
// the scalar side by v_readlane_b32 as in bits_scalar_loop; two per trip, an odd last one in a
// step of its own.
//  Form 2: zs is wave-uniform, so the run is read through the constant address space
// (s_load_dwordxN straight into SGPRs): whole batches in an unrolled trip with the next batch
// in flight, the last len mod TW_CLASS_BATCH images one at a time from the batch already loaded.
template <int NB, int K, int R>
__device__ __forceinline__ unsigned long long bits_count_class(const uint32_t* __restrict__ pw,
                                                               const uint32_t* __restrict__ zs,
                                                               int len, uint32_t cls, int lane) {
  constexpr int NL = NB - K;
  uint32_t lo[R][NL], acc[R];
#if TW_CLASS_FORM == 0
  uint32_t G[R], P[R];
#else
  uint32_t ng = 0;  // popc(G) over the groups: the class-constant term of one z
#endif
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint32_t top[K];
#pragma unroll
    for (int b = 0; b < NL; ++b) lo[r][b] = pw[(r * NB + b) * 64 + lane];
#pragma unroll
    for (int b = 0; b < K; ++b) top[b] = pw[(r * NB + NL + b) * 64 + lane];
#if TW_CLASS_FORM == 0
    class_gp<K>(top, cls, G[r], P[r]);
#else
    uint32_t g, p;
    class_gp<K>(top, cls, g, p);
    class_mask_planes<NL>(lo[r], class_equal_mask(g, p), lo[r]);
    ng = bits_popc_add(g, ng);
#endif
    acc[r] = 0;
  }
  auto step = [&](uint32_t sc) {
    uint32_t m[NL], c[R];
#pragma unroll
    for (int b = 0; b < NL; ++b) m[b] = bits_mask(sc, b);
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = lo[r][0] & m[0];
#pragma unroll
    for (int b = 1; b < NL; ++b)
#pragma unroll
      for (int r = 0; r < R; ++r) c[r] = bits_carry(lo[r][b], m[b], c[r]);
#pragma unroll
    for (int r = 0; r < R; ++r)
#if TW_CLASS_FORM == 0
      acc[r] = bits_popc_add(bits_carry(G[r], P[r], c[r]), acc[r]);
#else
      acc[r] = bits_popc_add(c[r], acc[r]);
#endif
  };
#if TW_CLASS_FORM == 2
  constexpr int B = TW_CLASS_BATCH;
  typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
  const ConstWords zc = (ConstWords)(uintptr_t)zs;
  uint32_t cur[B], next[B];
  auto load = [&](int j, uint32_t (&w)[B]) {
#pragma unroll
    for (int u = 0; u < B; ++u) w[u] = zc[j + u];
  };
  load(0, next);
  int j = 0;
  for (; j + B <= len; j += B) {
#pragma unroll
    for (int u = 0; u < B; ++u) cur[u] = next[u];
    load(min(j + B, len - 1), next);  // (starts inside the run; past a last whole batch: unused)
#pragma unroll
    for (int u = 0; u < B; ++u) step(cur[u]);
  }
  for (; j < len; ++j) {  // next holds the images from j on: never a word past the run's end
    step(next[0]);
#pragma unroll
    for (int u = 0; u + 1 < B; ++u) next[u] = next[u + 1];
  }
#else
  auto load = [&](int j) -> uint32_t { return zs[min(j + lane, len - 1)]; };  // (no branch)
  uint32_t next = load(0);
  for (int j = 0; j < len; j += 64) {
    const uint32_t sv = next;
    next = load(j + 64);
    const int cnt = min(64, len - j);
    int l = 0;
    for (; l + 2 <= cnt; l += 2) {
#pragma unroll
      for (int u = 0; u < 2; ++u) step((uint32_t)__builtin_amdgcn_readlane((int)sv, l + u));
    }
    if (l < cnt) step((uint32_t)__builtin_amdgcn_readlane((int)sv, l));  // never a padded slot
  }
#endif
  unsigned long long tot = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) tot += acc[r];
#if TW_CLASS_FORM != 0
  tot += (unsigned long long)(uint32_t)len * ng;  // the run's exact length
#endif
  return tot;
}
#endif  // __HIPCC__

}  // namespace tw
