// distselect.hip — exact order statistics of pairwise squared distances (tuplewise.bandwidth;
// DESIGN.md §4.16; an extension, not in the reference): a radix select over the bit patterns of
// the distance D of tripdist.h.  D is a non-negative double (never NaN, never -0 for finite rows),
// so key = __double_as_longlong(D) orders like an unsigned integer with bit 63 clear, and the k-th
// smallest D is found by integer histograms alone: nothing of size O(pairs) is stored.
//   tw_dist_hist    one pass over the pairs: for every pair whose key starts with a group's prefix,
//                   +1 in that group's bin of the key's next digit (kDselBits bits at most)
//   tw_dist_gather  the same walk: every key that starts with a group's prefix is appended to a key
//                   buffer through a wave-aggregated cursor (order unspecified, overflow dropped)
//   tw_keys_hist    the digit histogram of a 1-D key buffer (finishes a select after a gather)
// The host (tuplewise/bandwidth.py) drives the passes: it reads the histogram, narrows each target
// rank to its digit and extends the prefixes.
// The walk is k_mmd_sums' (mmd.hip): work items are tile pairs of kMmdT rows a side — the triangle
// for `within` (a diagonal tile counts anchor > point only), the rectangle for `cross` — kDselG
// consecutive items per workgroup, anchors staged in LDS, two points per lane, trip_chunk
// unchanged, so a D has the bits every other kernel gives it.  The tile, tail and diagonal masks
// PREDICATE the update: a masked pair touches no bin and appends no key.
// Counts are integers: a workgroup's bins are uint32 in LDS, its non-zero bins are added to the
// global uint64 histogram by integer atomics, so the result is exact and run-to-run identical
// whatever the schedule.  No float atomics.
#include "tw_common.h"
#include "selfreduce.h"  // self_tile_of
#include "tripdist.h"
#include "mmdtile.h"  // kMmdT, kMmdSA, mmd_load
#include <algorithm>

// How a lane's hit reaches the workgroup's LDS bins (a build flag of tools/time_bandwidth.py's
// attribution builds, never a runtime mode; the product is 0):
//   0  one LDS atomic per hitting lane, always: the kept form (measured the fastest in pass 1, where
//      nearly every lane of a wave hits the exponent's one bin, and in the later passes)
//   1  wave-combined: when every hitting lane of the wave has the same bin, one lane adds their
//      number; otherwise one LDS atomic per lane (slower than 0 in every pass measured)
//   2  the bin update compiled out (the walk and the matching stay): the update's share of a pass
#ifndef TW_DISTSEL_UPDATE
#define TW_DISTSEL_UPDATE 0
#endif

namespace tw {

constexpr int kDselBits = 11;                 // digit width: 8 KiB of uint32 bins per group
constexpr int kDselBins = 1 << kDselBits;
constexpr int kDselMaxGroups = 8;             // 64 KiB of dynamic LDS at most, beside the anchors
constexpr int kDselG = 2;                     // tile pairs per workgroup (k_mmd_sums' kMmdG)
constexpr int kDselKeysPerWG = kBlock * 64;   // keys of the buffer a workgroup of k_keys_hist owns
// A workgroup's uint32 bins cannot overflow: a pair (a key) adds at most 1 per group, and a
// workgroup owns at most kDselG * kMmdT * kMmdT = 32768 pairs (kDselKeysPerWG = 16384 keys).
static_assert((int64_t)kDselG * kMmdT * kMmdT < (1ll << 32) && kDselKeysPerWG < (1ll << 32),
              "a workgroup's items fit a uint32 bin");

// The prefix groups of a pass, by value in the kernel arguments: a key belongs to group g iff
// key >> shift[g] == prefix[g], shift = 63 - prefix bits (bit 63 of a key is 0, so an empty prefix
// is the value 0 at shift 63).
struct DselGroups {
  unsigned long long prefix[kDselMaxGroups];
  int32_t shift[kDselMaxGroups];
  int32_t n;
};

__device__ __forceinline__ void dsel_bin_add(uint32_t* __restrict__ bins, bool hit, uint32_t bin,
                                             int lane, uint32_t& sink) {
#if TW_DISTSEL_UPDATE == 2
  sink += hit ? bin + 1u : 0u;
#elif TW_DISTSEL_UPDATE == 0
  if (hit) atomicAdd(&bins[bin], 1u);
#else
  if (hit) {  // the lanes inside are the hitting lanes: ballots and readfirstlane see only them
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
    const unsigned long long act = __ballot(1);
    const unsigned long long same = __ballot(bin == first);
    if (same == act) {  // wave-uniform among the hitting lanes
      if ((act & ((1ull << lane) - 1ull)) == 0ull)
        atomicAdd(&bins[first], (uint32_t)__popcll(act));
    } else {
      atomicAdd(&bins[bin], 1u);
    }
  }
#endif
}

template <bool GATHER>
struct DselSink {
  const DselGroups& gr;
  int digit_shift;
  uint32_t digit_mask;
  uint32_t* __restrict__ bins;
  unsigned long long* __restrict__ keys;
  unsigned long long cap;
  unsigned long long* __restrict__ count;
  int lane;
  uint32_t sink;

  __device__ __forceinline__ void operator()(unsigned long long key, bool ok) {
    if constexpr (!GATHER) {
      const uint32_t digit = (uint32_t)(key >> digit_shift) & digit_mask;
      for (int g = 0; g < gr.n; ++g)
        dsel_bin_add(bins, ok && (key >> gr.shift[g]) == gr.prefix[g],
                     (uint32_t)g * kDselBins + digit, lane, sink);
    } else {
      bool hit = false;
      for (int g = 0; g < gr.n; ++g) hit = hit || (key >> gr.shift[g]) == gr.prefix[g];
      if (hit && ok) {  // one cursor step per wave: the lowest hitting lane takes the range
        const unsigned long long act = __ballot(1);
        const unsigned long long below = act & ((1ull << lane) - 1ull);
        unsigned long long base = 0ull;
        if (below == 0ull) base = atomicAdd(count, (unsigned long long)__popcll(act));
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
        const unsigned long long pos =
            (((unsigned long long)hi << 32) | lo) + (unsigned long long)__popcll(below);
        if (pos < cap) keys[pos] = key;   // an append past the capacity is dropped ...
        else atomicMax(count + 1, 1ull);  // ... and flagged
      }
    }
  }
};

// The wave's kTripTA x kTripR keys of a step, handed to the sink with their mask (mmd_fold's).
template <bool MASK, typename S>
__device__ __forceinline__ void dsel_visit(const double (&acc)[kTripTA][kTripR], int a_first,
                                           int na, int diag_shift, const bool (&valid)[kTripR],
                                           int lane, S& sink) {
#pragma unroll
  for (int a = 0; a < kTripTA; ++a) {
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      // diag_shift: 0 on a diagonal tile (anchor index above the point's), else past every point
      const bool ok = !MASK || (valid[r] && a_first + a < na &&
                                a_first + a + diag_shift > r * kWave + lane);
      sink((unsigned long long)__double_as_longlong(acc[a][r]), ok);
    }
  }
}

// within != 0: the pairs i < j of x (z, m unused).  Else all (x_i, z_k).  Workgroup blockIdx.x owns
// items [blockIdx.x * kDselG, ... + kDselG) of the triangle / rectangle of tiles.
template <bool GATHER>
__global__ __launch_bounds__(kBlock) void k_dist_walk(
    const double* __restrict__ x, int64_t n, const double* __restrict__ z, int64_t m, int d,
    int within, DselGroups gr, int digit_shift, uint32_t digit_mask,
    unsigned long long* __restrict__ hist, unsigned long long* __restrict__ keys,
    unsigned long long cap, unsigned long long* __restrict__ count) {
  __shared__ double sa[kMmdSA * kTripMaxD];
  extern __shared__ uint32_t bins[];  // !GATHER: gr.n * kDselBins
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if constexpr (!GATHER) {
    for (int q = threadIdx.x; q < gr.n * kDselBins; q += kBlock) bins[q] = 0u;
    __syncthreads();
  }
  DselSink<GATHER> sink{gr, digit_shift, digit_mask, bins, keys, cap, count, lane, 0u};
  const int64_t tx = (n + kMmdT - 1) / kMmdT, tz = (m + kMmdT - 1) / kMmdT;
  const int64_t items = within ? tx * (tx + 1) / 2 : tx * tz;
  const double* __restrict__ swave = sa + wid * kTripTA * kTripMaxD;
  const double* __restrict__ anc = within ? x : z;
  const int64_t nanc = within ? n : m;
  const int64_t it_end = std::min<int64_t>(items, ((int64_t)blockIdx.x + 1) * kDselG);
  for (int64_t it = (int64_t)blockIdx.x * kDselG; it < it_end; ++it) {
    int I, J;  // point tile I and anchor tile J: workgroup-uniform
    if (within) {
      self_tile_of(it, I, J);
    } else {
      I = (int)(it / tz);
      J = (int)(it - (int64_t)I * tz);
    }
    const int64_t p0 = (int64_t)I * kMmdT, a0 = (int64_t)J * kMmdT;
    const int na = (int)std::min<int64_t>(kMmdT, nanc - a0);  // >= 1: J is a tile of the sample
    const bool diag = within && I == J;
    bool valid[kTripR];
    const double* __restrict__ row[kTripR];
    bool all_valid = true;
#pragma unroll
    for (int r = 0; r < kTripR; ++r) {
      const int64_t p = p0 + r * kWave + lane;
      valid[r] = p < n;
      row[r] = x + (valid[r] ? p : p0) * d;  // a lane past the end reads the tile's first point
      all_valid = all_valid && p0 + r * kWave + kWave <= n;
    }
    const int n_full = d / kTripDC;  // whole chunks of coordinates; the rest is the tail chunk
    const bool tail = n_full * kTripDC < d;
    for (int s0 = 0; s0 < na; s0 += kMmdSA) {
      double pc[kTripR][kTripDC];
      if (n_full > 0) mmd_load<false>(row, 0, d, pc);
      else mmd_load<true>(row, 0, d, pc);
      __syncthreads();  // the previous step's readers
      for (int q = threadIdx.x; q < kMmdSA * d; q += kBlock) {
        const int a = q / d, cc = q - a * d;
        sa[a * kTripMaxD + cc] = s0 + a < na ? anc[(a0 + s0) * d + q] : 0.0;
      }
      __syncthreads();
      double acc[kTripTA][kTripR];
#pragma unroll
      for (int a = 0; a < kTripTA; ++a)
#pragma unroll
        for (int r = 0; r < kTripR; ++r) acc[a][r] = 0.0;
      for (int ch = 0; ch < n_full; ++ch) {
        double pn[kTripR][kTripDC];
        const int c1 = (ch + 1) * kTripDC;
        if (ch + 1 < n_full) mmd_load<false>(row, c1, d, pn);
        else if (tail) mmd_load<true>(row, c1, d, pn);
        trip_chunk<false>(swave, ch * kTripDC, d, pc, acc);
#pragma unroll
        for (int r = 0; r < kTripR; ++r)
#pragma unroll
          for (int cc = 0; cc < kTripDC; ++cc) pc[r][cc] = pn[r][cc];
      }
      if (tail) trip_chunk<true>(swave, n_full * kTripDC, d, pc, acc);
      const int a_first = s0 + wid * kTripTA;  // this wave's anchors of the step, tile-relative
      if (!diag && all_valid && s0 + kMmdSA <= na)  // workgroup-uniform
        dsel_visit<false>(acc, a_first, na, 0, valid, lane, sink);
      else
        dsel_visit<true>(acc, a_first, na, diag ? 0 : kMmdT, valid, lane, sink);
    }
  }
  if constexpr (!GATHER) {
#if TW_DISTSEL_UPDATE == 2
    if (sink.sink == 0xffffffffu) bins[0] = 1u;  // keeps the walk alive; the bins stay zero
#endif
    __syncthreads();
    for (int q = threadIdx.x; q < gr.n * kDselBins; q += kBlock) {
      const uint32_t v = bins[q];
      if (v != 0u) atomicAdd(&hist[q], (unsigned long long)v);
    }
  }
}

// Workgroup blockIdx.x owns keys [blockIdx.x * kDselKeysPerWG, ... + kDselKeysPerWG) of the buffer.
__global__ __launch_bounds__(kBlock) void k_keys_hist(
    const unsigned long long* __restrict__ keys, int64_t n_keys, DselGroups gr, int digit_shift,
    uint32_t digit_mask, unsigned long long* __restrict__ hist) {
  extern __shared__ uint32_t bins[];  // gr.n * kDselBins
  const int lane = threadIdx.x & (kWave - 1);
  for (int q = threadIdx.x; q < gr.n * kDselBins; q += kBlock) bins[q] = 0u;
  __syncthreads();
  DselSink<false> sink{gr, digit_shift, digit_mask, bins, nullptr, 0ull, nullptr, lane, 0u};
  const int64_t base = (int64_t)blockIdx.x * kDselKeysPerWG;
  for (int i = threadIdx.x; i < kDselKeysPerWG; i += kBlock) {
    const int64_t p = base + i;
    const bool ok = p < n_keys;
    sink(ok ? keys[p] : 0ull, ok);
  }
#if TW_DISTSEL_UPDATE == 2
  if (sink.sink == 0xffffffffu) bins[0] = 1u;
#endif
  __syncthreads();
  for (int q = threadIdx.x; q < gr.n * kDselBins; q += kBlock) {
    const uint32_t v = bins[q];
    if (v != 0u) atomicAdd(&hist[q], (unsigned long long)v);
  }
}

inline int64_t dsel_items(int64_t n, int64_t m, int32_t pairs) {
  const int64_t tx = ceil_div(n, kMmdT), tz = ceil_div(m, kMmdT);
  return pairs == TW_DIST_WITHIN ? tx * (tx + 1) / 2 : tx * tz;
}

// > 64 KiB of LDS (the anchors and eight groups' bins) must be opted into once per kernel
template <typename K>
inline hipError_t dsel_opt_in(K kernel, bool& done) {
  if (done) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(kDselMaxGroups * kDselBins * sizeof(uint32_t)));
  done = e == hipSuccess;
  return e;
}

}  // namespace tw

using namespace tw;

#define TW_DSEL_GROUP_CHECKS(fn)                                                                 \
  TW_ARG_CHECK(prefix && prefix_bits, fn ": null pointer");                                      \
  TW_ARG_CHECK(n_groups >= 1 && n_groups <= kDselMaxGroups, fn ": n_groups %d outside [1, %d]",  \
               n_groups, kDselMaxGroups);                                                        \
  DselGroups gr{};                                                                               \
  gr.n = n_groups;                                                                               \
  for (int g = 0; g < n_groups; ++g) {                                                           \
    TW_ARG_CHECK(prefix_bits[g] >= 0 && prefix_bits[g] <= 63,                                    \
                 fn ": prefix_bits[%d] = %d outside [0, 63]", g, prefix_bits[g]);                \
    TW_ARG_CHECK((prefix[g] >> prefix_bits[g]) == 0,                                             \
                 fn ": prefix[%d] has bits above its %d prefix bits", g, prefix_bits[g]);        \
    gr.prefix[g] = prefix[g];                                                                    \
    gr.shift[g] = 63 - prefix_bits[g];                                                           \
  }

#define TW_DSEL_DIGIT_CHECKS(fn)                                                                 \
  TW_ARG_CHECK(digit_bits >= 1 && digit_bits <= kDselBits && digit_shift >= 0 &&                 \
                   digit_shift + digit_bits <= 63,                                               \
               fn ": digit of %d bits at shift %d (1 .. %d bits inside bits 0 .. 62)", digit_bits, \
               digit_shift, kDselBits)

#define TW_DSEL_ROW_CHECKS(fn)                                                                   \
  TW_ARG_CHECK(pairs == TW_DIST_WITHIN || pairs == TW_DIST_CROSS, fn ": unknown pair set %d",    \
               pairs);                                                                           \
  TW_ARG_CHECK(d_x && (pairs == TW_DIST_WITHIN || d_z), fn ": null pointer");                    \
  TW_ARG_CHECK(d >= 1 && d <= kTripMaxD, fn ": d %d outside [1, %d]", d, kTripMaxD);             \
  if (pairs == TW_DIST_WITHIN) m = 0;                                                            \
  TW_ARG_CHECK(n >= 0 && m >= 0 && n < (1ll << 31) && m < (1ll << 31),                           \
               fn ": sizes outside [0, 2^31) (n %lld, m %lld)", (long long)n, (long long)m);     \
  const int64_t items = dsel_items(n, m, pairs);                                                 \
  const int64_t wgs = ceil_div(items, kDselG);                                                   \
  TW_ARG_CHECK(wgs < (1ll << 31), fn ": grid too large")

extern "C" int32_t tw_dist_select_digit_bits(void) { return kDselBits; }
extern "C" int32_t tw_dist_select_max_groups(void) { return kDselMaxGroups; }

extern "C" int64_t tw_dist_hist_bytes(int32_t n_groups) {
  if (n_groups < 1 || n_groups > kDselMaxGroups) return 0;
  return (int64_t)n_groups * kDselBins * 8;
}

extern "C" int tw_dist_hist(const double* d_x, int64_t n, const double* d_z, int64_t m, int32_t d,
                            int32_t pairs, const uint64_t* prefix, const int32_t* prefix_bits,
                            int32_t n_groups, int32_t digit_shift, int32_t digit_bits,
                            uint64_t* d_hist, void* stream) {
  TW_DSEL_ROW_CHECKS("tw_dist_hist");
  TW_ARG_CHECK(d_hist, "tw_dist_hist: null pointer");
  TW_DSEL_GROUP_CHECKS("tw_dist_hist");
  TW_DSEL_DIGIT_CHECKS("tw_dist_hist");
  hipStream_t st = (hipStream_t)stream;
  TW_HIP_CHECK(tw_zero_async(d_hist, 0, (size_t)tw_dist_hist_bytes(n_groups), st));
  if (wgs == 0) return TW_OK;
  static bool opted = false;
  TW_HIP_CHECK(dsel_opt_in(k_dist_walk<false>, opted));
  hipLaunchKernelGGL(k_dist_walk<false>, dim3((unsigned)wgs), dim3(kBlock),
                     (size_t)n_groups * kDselBins * sizeof(uint32_t), st, d_x, n, d_z, m, (int)d,
                     (int)(pairs == TW_DIST_WITHIN), gr, (int)digit_shift,
                     (uint32_t)((1u << digit_bits) - 1u), (unsigned long long*)d_hist,
                     (unsigned long long*)nullptr, 0ull, (unsigned long long*)nullptr);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int tw_dist_gather(const double* d_x, int64_t n, const double* d_z, int64_t m, int32_t d,
                              int32_t pairs, const uint64_t* prefix, const int32_t* prefix_bits,
                              int32_t n_groups, uint64_t* d_keys, int64_t capacity,
                              uint64_t* d_count, void* stream) {
  TW_DSEL_ROW_CHECKS("tw_dist_gather");
  TW_ARG_CHECK(d_count && capacity >= 0 && (d_keys || capacity == 0),
               "tw_dist_gather: null pointer or negative capacity %lld", (long long)capacity);
  TW_DSEL_GROUP_CHECKS("tw_dist_gather");
  hipStream_t st = (hipStream_t)stream;
  TW_HIP_CHECK(tw_zero_async(d_count, 0, 16, st));
  if (wgs == 0) return TW_OK;
  hipLaunchKernelGGL(k_dist_walk<true>, dim3((unsigned)wgs), dim3(kBlock), 0, st, d_x, n, d_z, m,
                     (int)d, (int)(pairs == TW_DIST_WITHIN), gr, 0, 0u,
                     (unsigned long long*)nullptr, (unsigned long long*)d_keys,
                     (unsigned long long)capacity, (unsigned long long*)d_count);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int tw_keys_hist(const uint64_t* d_keys, int64_t n_keys, const uint64_t* prefix,
                            const int32_t* prefix_bits, int32_t n_groups, int32_t digit_shift,
                            int32_t digit_bits, uint64_t* d_hist, void* stream) {
  TW_ARG_CHECK(d_hist && n_keys >= 0 && (d_keys || n_keys == 0),
               "tw_keys_hist: null pointer or negative size %lld", (long long)n_keys);
  TW_DSEL_GROUP_CHECKS("tw_keys_hist");
  TW_DSEL_DIGIT_CHECKS("tw_keys_hist");
  const int64_t wgs = ceil_div(n_keys, kDselKeysPerWG);
  TW_ARG_CHECK(wgs < (1ll << 31), "tw_keys_hist: grid too large");
  hipStream_t st = (hipStream_t)stream;
  TW_HIP_CHECK(tw_zero_async(d_hist, 0, (size_t)tw_dist_hist_bytes(n_groups), st));
  if (wgs == 0) return TW_OK;
  static bool opted = false;
  TW_HIP_CHECK(dsel_opt_in(k_keys_hist, opted));
  hipLaunchKernelGGL(k_keys_hist, dim3((unsigned)wgs), dim3(kBlock),
                     (size_t)n_groups * kDselBins * sizeof(uint32_t), st,
                     (const unsigned long long*)d_keys, n_keys, gr, (int)digit_shift,
                     (uint32_t)((1u << digit_bits) - 1u), (unsigned long long*)d_hist);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
