// mtdraw.hip — NumPy-order randint streams drawn on the device.
//
// cs.UB draws its B pairs with two legacy np.random.randint calls per block
// (compute_stats.py:37-42).  For a fixed bound that call is a masked rejection on consecutive
// 32-bit MT19937 words — word w is accepted iff (w & mask) <= high-1-low, whatever its position
// — so given the raw words the draws are a stream compaction.  The words themselves come from
// many sub-streams started in parallel: MT19937 is linear over GF(2), the state J words ahead is
// t^J mod phi applied to the current one (csrc/mtjump.cpp), and the states of sub-streams
// [2^v, 2^(v+1)) are one jump by 2^v L of the states [0, 2^v).
//
//   k_mt_jump      one workgroup per new state: the source's 20560 raw words in LDS (82 KB), the
//                  GF(2) convolution with a wave-uniform loop over the list of the polynomial's
//                  set coefficients, sixteen independent LDS reads a step
//   k_mt_generate  one workgroup per sub-stream: the key block regenerated in three dependent
//                  phases of <= 227 words, tempered words to HBM, per key block and (mask, range)
//                  configuration the number of accepted words (ballots; no atomics)
//   k_scan_counts  exclusive prefix sums of those counts, one workgroup per configuration
//   k_resolve      one workgroup walks the calls in order (call c starts after call c-1's last
//                  accepted word): a 256-ary search in the prefix, then a scan of one key block
//   k_compact      one pass over the words: call by binary search in the first-word table,
//                  slot = call base + accepted words since the call's first (deterministic)
//
// Word indices are aligned to the host key: word i is x[i] with x[0..623] = key, so NumPy's
// next word is word *pos and every group of 624 words is one of NumPy's key blocks.
#include <vector>

#include "tw_common.h"

namespace {
using namespace tw;

constexpr int kN = 624, kM = 397, kLag = kN - kM;  // 227 independent words per phase
constexpr int kDeg = 19937, kSeq = kDeg + kN - 1;
constexpr int kPolyCap = 19952, kPolyStride = 16 + kPolyCap;  // a listed polynomial (uint32)
constexpr int kMaxCfg = 4;
constexpr int kJumpThreads = 640;  // 10 waves: lanes are consecutive output words
constexpr size_t kJumpLds = (kSeq + kN) * sizeof(uint32_t);  // 84736 B of the 160 KB
constexpr int64_t kMaxWords = 1ll << 30;

struct Cfgs {
  uint32_t mask[kMaxCfg], rng[kMaxCfg];
  int n;
};

__host__ __device__ __forceinline__ uint32_t twist(uint32_t a, uint32_t b, uint32_t src) {
  const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
  return src ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
}

__device__ __forceinline__ uint32_t temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}

// Exclusive scan of v over a workgroup of NW waves (threads in order); *total = the sum.
template <int NW>
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* s_w, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t n = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += n;
  }
  __syncthreads();  // s_w's previous readers are done
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t s = s_w[i];
    off += i < wave ? s : 0u;
    tot += s;
  }
  *total = tot;
  return off + inc - v;
}

// table row first_dst + a = (a == 0 ? poly0 : polyk) applied to table row a: the row's raw
// sequence x[0, kSeq) by the recurrence (any kLag consecutive words are independent), then
// y[j] = XOR_{i : g_i = 1} x[i + j] — lanes are consecutive j, so every LDS read is
// conflict-free, and the loop over the polynomial's set coefficients is uniform.
__global__ __launch_bounds__(kJumpThreads) void k_mt_jump(uint32_t* __restrict__ table,
                                                          const uint32_t* __restrict__ poly0,
                                                          const uint32_t* __restrict__ polyk,
                                                          int first_dst) {
  extern __shared__ uint32_t x[];  // kSeq words, then kN zero words (kJumpLds bytes)
  const int a = blockIdx.x, t = threadIdx.x;
  const uint32_t* src = table + (size_t)a * kN;
  for (int i = t; i < kN; i += kJumpThreads) {
    x[i] = src[i];
    x[kSeq + i] = 0u;
  }
  __syncthreads();
  for (int k = kN; k < kSeq; k += kLag) {
    const int i = k + t;
    if (t < kLag && i < kSeq) x[i] = twist(x[i - kN], x[i - kN + 1], x[i - kLag]);
    __syncthreads();
  }
  if (t >= kN) return;
  // the polynomial as the list of its set coefficients (scalar loads; no bit scanning on the
  // scalar unit, which bound the bit-packed form at ~40 cycles a read): sixteen independent LDS
  // reads a step; the list is padded with kSeq, a zero word
  const uint32_t* g = a == 0 ? poly0 : polyk;
  const int n = min((int)__builtin_amdgcn_readfirstlane(g[0]), kPolyCap);
  const uint32_t* xs = x + t;
  uint32_t acc = 0;
  for (int i = 0; i < n; i += 16) {
    uint32_t v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint32_t p = __builtin_amdgcn_readfirstlane(g[16 + i + q]);
      v[q] = xs[min(p, (uint32_t)kSeq)];  // reads stay in x whatever the list holds
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) acc ^= v[q];
  }
  table[(size_t)(first_dst + a) * kN + t] = acc;
}

// Sub-stream k = blockIdx.x: words x[kL .. (k+1)L), L = 624 sb.  Its first key block is table
// row 0 itself (k = 0) or the row's words 1..623 plus one recurrence step (the row is the
// window at kL - 1: word 0 carries only the top bit); each further block is the twist of the
// previous one, new[i] from old words for i < 227, from new[i - 227] after (three phases).
__global__ __launch_bounds__(256) void k_mt_generate(const uint32_t* __restrict__ table, int sb,
                                                     Cfgs cf, uint32_t* __restrict__ words,
                                                     uint32_t* __restrict__ counts,
                                                     int ngroups) {
  __shared__ uint32_t s[2][kN];
  __shared__ uint32_t s_cnt[2][kMaxCfg][4];
  const int k = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const uint32_t* U = table + (size_t)k * kN;
  for (int i = t; i < kN; i += 256)
    s[0][i] = k == 0 ? U[i] : i < kN - 1 ? U[i + 1] : twist(U[0], U[1], U[kM]);
  __syncthreads();
  for (int b = 0; b < sb; ++b) {
    uint32_t* cur = s[b & 1];
    const uint32_t* prv = s[(b & 1) ^ 1];
    uint32_t* out = words + ((size_t)k * sb + b) * kN;
    uint32_t c[kMaxCfg] = {0u, 0u, 0u, 0u};
    for (int ph = 0; ph < 3; ++ph) {
      const int i = b == 0 ? ph * 256 + t : ph * kLag + t;
      const bool active = i < kN && (b == 0 || t < kLag);
      uint32_t w = 0;
      if (active) {
        uint32_t v;
        if (b == 0) {
          v = cur[i];
        } else {
          v = twist(prv[i], i == kN - 1 ? cur[0] : prv[i + 1], ph == 0 ? prv[i + kM] : cur[i - kLag]);
          cur[i] = v;
        }
        w = temper(v);
        out[i] = w;
      }
#pragma unroll
      for (int f = 0; f < kMaxCfg; ++f)
        if (f < cf.n) c[f] += (uint32_t)__popcll(__ballot(active && (w & cf.mask[f]) <= cf.rng[f]));
      if (ph == 2 && lane == 0) {
#pragma unroll
        for (int f = 0; f < kMaxCfg; ++f) s_cnt[b & 1][f][wave] = c[f];
      }
      if (b > 0 || ph == 2) __syncthreads();
    }
    if (t < cf.n) {
      const uint32_t* p = s_cnt[b & 1][t];
      counts[(size_t)t * ngroups + (size_t)k * sb + b] = p[0] + p[1] + p[2] + p[3];
    }
  }
}

// prefix[f][g] = accepted words of configuration f before group g; prefix[f][ng] = all
__global__ __launch_bounds__(1024) void k_scan_counts(const uint32_t* __restrict__ counts,
                                                      uint32_t* __restrict__ prefix, int ng) {
  __shared__ uint32_t s_w[16];
  const int t = threadIdx.x;
  const uint32_t* in = counts + (size_t)blockIdx.x * ng;
  uint32_t* out = prefix + (size_t)blockIdx.x * (ng + 1);
  const int per = (ng + 1023) / 1024;
  const int lo = min(t * per, ng), hi = min(lo + per, ng);
  uint32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += in[i];
  uint32_t total;
  uint32_t run = block_scan_excl<16>(sum, s_w, &total);
  for (int i = lo; i < hi; ++i) {
    out[i] = run;
    run += in[i];
  }
  if (t == 1023) out[ng] = total;
}

// One workgroup, the calls in order.  A(w) = accepted words of the call's configuration in
// [0, w); call c starts at wp with A(wp) = a and ends at the word e with A(e + 1) = a + cnt.
// result: calls completed, values of the first incomplete call, words consumed, calls with words.
__global__ __launch_bounds__(256) void k_resolve(const uint32_t* __restrict__ words,
                                                 const uint32_t* __restrict__ prefix, int ng,
                                                 Cfgs cf, int ncalls,
                                                 const int32_t* __restrict__ ccfg,
                                                 const int64_t* __restrict__ ccnt,
                                                 uint32_t* __restrict__ first,
                                                 uint32_t* __restrict__ last,
                                                 uint32_t* __restrict__ abase, uint32_t w0,
                                                 int64_t* __restrict__ result) {
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_pos;
  const int t = threadIdx.x;
  const uint32_t nwords = (uint32_t)ng * kN;
  uint32_t wp = w0, acur = 0;
  int lastcfg = -1, c = 0;
  int64_t partial = 0;
  for (; c < ncalls; ++c) {
    const int f = ccfg[c];
    const int64_t need = ccnt[c];
    const uint32_t* pf = prefix + (size_t)f * (ng + 1);
    const uint32_t mask = cf.mask[f], rng = cf.rng[f];
    if (f != lastcfg) {  // A(wp) afresh: the group's prefix plus the accepted words before wp
      const uint32_t g = wp / kN;
      if (g >= (uint32_t)ng) {
        acur = pf[ng];
      } else {
        uint32_t n = 0;
        for (int r = 0; r < 3; ++r) {
          const uint32_t i = 3 * t + r, wd = g * kN + i;
          if (i < kN && wd < wp) n += (words[wd] & mask) <= rng;
        }
        uint32_t tot;
        block_scan_excl<4>(n, s_w, &tot);
        acur = pf[g] + tot;
      }
      lastcfg = f;
    }
    const uint32_t total = pf[ng];
    if (t == 0) {
      first[c] = wp;
      abase[c] = acur;
    }
    if ((int64_t)acur + need > (int64_t)total) {  // the words run out inside this call
      partial = (int64_t)total - acur;
      if (t == 0) last[c] = nwords - 1;
      wp = nwords;
      break;
    }
    const uint32_t T = acur + (uint32_t)need;
    // the largest group g with pf[g] < T, by 256-ary search (pf[wp / 624] <= acur < T)
    uint32_t lo = wp / kN, hi = (uint32_t)ng;
    while (hi - lo > 1) {
      const uint32_t step = (hi - lo + 255) / 256, idx = lo + t * step;
      uint32_t ntrue;
      block_scan_excl<4>(idx < hi && pf[idx] < T ? 1u : 0u, s_w, &ntrue);
      lo += (ntrue - 1) * step;
      hi = min(lo + step, hi);
    }
    const uint32_t r = T - pf[lo];  // the r-th accepted word of group lo ends the call
    uint32_t n = 0;
    bool acc[3];
    for (int q = 0; q < 3; ++q) {
      const uint32_t i = 3 * t + q;
      acc[q] = i < kN && (words[lo * kN + i] & mask) <= rng;
      n += acc[q];
    }
    uint32_t tot;
    uint32_t ex = block_scan_excl<4>(n, s_w, &tot);
    if (ex < r && r <= ex + n) {
      for (int q = 0; q < 3; ++q)
        if (acc[q] && ++ex == r) s_pos = lo * kN + 3 * t + q;
    }
    __syncthreads();
    const uint32_t e = s_pos;
    if (t == 0) last[c] = e;
    wp = e + 1;
    acur = T;
  }
  if (t == 0) {
    result[0] = c;
    result[1] = partial;
    result[2] = wp;
    result[3] = c < ncalls ? c + 1 : ncalls;
  }
}

// Group g = blockIdx.x (one key block): every accepted word of a call's range goes to
// d_out[call_out + (A(w) - A(first word))] as call_base + (w & mask).
__global__ __launch_bounds__(256) void k_compact(const uint32_t* __restrict__ words,
                                                 const uint32_t* __restrict__ prefix, int ng,
                                                 Cfgs cf, const int32_t* __restrict__ ccfg,
                                                 const int64_t* __restrict__ ccnt,
                                                 const int32_t* __restrict__ cbase,
                                                 const int64_t* __restrict__ cout,
                                                 const uint32_t* __restrict__ first,
                                                 const uint32_t* __restrict__ last,
                                                 const uint32_t* __restrict__ abase,
                                                 const int64_t* __restrict__ result,
                                                 int32_t* __restrict__ out, int64_t out_len) {
  __shared__ uint32_t s_w[4];
  const int t = threadIdx.x, g = blockIdx.x;
  const int nlive = (int)result[3];
  if (nlive <= 0) return;
  const uint32_t gw0 = (uint32_t)g * kN, gw1 = gw0 + kN - 1;
  if (gw1 < first[0] || gw0 > last[nlive - 1]) return;  // uniform: before any barrier
  // the largest c in [lo, hi] with first[c] <= w (lo when there is none)
  auto find = [&](uint32_t w, int lo, int hi) {
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (first[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
  };
  const int clo = find(gw0, 0, nlive - 1), chi = find(gw1, clo, nlive - 1);
  uint32_t w[3];
  int c[3];
  for (int q = 0; q < 3; ++q) {
    const uint32_t i = 3 * t + q;
    w[q] = i < kN ? words[gw0 + i] : 0u;
    c[q] = -1;
    if (i < kN) {
      const int cc = clo == chi ? clo : find(gw0 + i, clo, chi);
      if (gw0 + i >= first[cc] && gw0 + i <= last[cc]) c[q] = cc;
    }
  }
  for (int f = 0; f < cf.n; ++f) {
    if (clo == chi && ccfg[clo] != f) continue;  // uniform
    const uint32_t mask = cf.mask[f], rng = cf.rng[f];
    bool acc[3];
    uint32_t n = 0;
    for (int q = 0; q < 3; ++q) {
      acc[q] = 3 * t + q < kN && (w[q] & mask) <= rng;
      n += acc[q];
    }
    uint32_t tot;
    uint32_t run = prefix[(size_t)f * (ng + 1) + g] + block_scan_excl<4>(n, s_w, &tot);
    for (int q = 0; q < 3; ++q) {
      if (!acc[q]) continue;
      const int cc = c[q];
      if (cc >= 0 && ccfg[cc] == f) {
        const int64_t rel = (int64_t)(run - abase[cc]);
        const int64_t slot = cout[cc] + rel;
        if (rel < ccnt[cc] && slot >= 0 && slot < out_len)
          out[slot] = (int32_t)((uint32_t)cbase[cc] + (w[q] & mask));
      }
      ++run;
    }
  }
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the carve-up of tw_np_randint_dev's d_work
struct Work {
  size_t words, counts, prefix, ccfg, ccnt, cbase, cout, first, last, abase, result, total;
  Work(int64_t nw, int64_t ng, int n_calls, int n_cfg) {
    size_t o = 0;
    auto take = [&](size_t bytes) {
      const size_t at = o;
      o += up256(bytes);
      return at;
    };
    words = take((size_t)nw * 4);
    counts = take((size_t)n_cfg * ng * 4);
    prefix = take((size_t)n_cfg * (ng + 1) * 4);
    ccfg = take((size_t)n_calls * 4);
    ccnt = take((size_t)n_calls * 8);
    cbase = take((size_t)n_calls * 4);
    cout = take((size_t)n_calls * 8);
    first = take((size_t)n_calls * 4);
    last = take((size_t)n_calls * 4);
    abase = take((size_t)n_calls * 4);
    result = take(4 * 8);
    total = o;
  }
};

int check_cfgs(const char* who, int32_t n_cfg, const uint32_t* cfg_mask, const uint32_t* cfg_rng,
               Cfgs* cf) {
  TW_ARG_CHECK(n_cfg >= 1 && n_cfg <= kMaxCfg && cfg_mask && cfg_rng,
               "%s: 1..%d (mask, range) configurations", who, kMaxCfg);
  *cf = Cfgs{};
  cf->n = n_cfg;
  for (int f = 0; f < n_cfg; ++f) {
    const uint32_t m = cfg_mask[f], r = cfg_rng[f];
    TW_ARG_CHECK(r >= 1 && r < 0xFFFFFFFFu && (m & (m + 1)) == 0 && m >= r && (m >> 1) < r,
                 "%s: configuration %d is not a masked-rejection (mask, range) pair", who, f);
    cf->mask[f] = m;
    cf->rng[f] = r;
  }
  return TW_OK;
}

int check_table(const char* who, int32_t n_states, int32_t stream_blocks) {
  TW_ARG_CHECK(n_states >= 1 && stream_blocks >= 1 &&
                   (int64_t)n_states * stream_blocks * kN <= kMaxWords,
               "%s: bad sizes (n_states=%d, stream_blocks=%d; at most 2^30 words)", who,
               n_states, stream_blocks);
  return TW_OK;
}

int launch_generate(const uint32_t* d_table, int32_t n_states, int32_t sb, const Cfgs& cf,
                    uint32_t* d_words, uint32_t* d_counts, hipStream_t st) {
  hipLaunchKernelGGL(k_mt_generate, dim3(n_states), dim3(256), 0, st, d_table, sb, cf, d_words,
                     d_counts, n_states * sb);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

}  // namespace

extern "C" {

int tw_mt_states(const uint32_t* key, int32_t n_states, const uint32_t* d_polys, int32_t levels,
                 uint32_t* d_table, void* stream) {
  TW_ARG_CHECK(key && d_table && n_states >= 1 && n_states <= (1 << 22) && levels >= 0 &&
                   levels <= 22 && (1ll << levels) >= n_states && (n_states == 1 || d_polys),
               "tw_mt_states: bad arguments (n_states=%d, levels=%d)", n_states, levels);
  hipStream_t st = (hipStream_t)stream;
  static bool attr = false;
  if (!attr) {
    TW_HIP_CHECK(hipFuncSetAttribute((const void*)k_mt_jump,
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)kJumpLds));
    attr = true;
  }
  TW_HIP_CHECK(hipMemcpyAsync(d_table, key, kN * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  for (int v = 0; (1 << v) < n_states; ++v) {
    const int have = 1 << v, napps = std::min(have, n_states - have);
    const uint32_t* p = d_polys + (size_t)v * 2 * kPolyStride;
    hipLaunchKernelGGL(k_mt_jump, dim3(napps), dim3(kJumpThreads), kJumpLds, st,
                       d_table, p, p + kPolyStride, have);
    TW_LAUNCH_CHECK();
  }
  return TW_OK;
}

int tw_mt_generate(const uint32_t* d_table, int32_t n_states, int32_t stream_blocks,
                   int32_t n_cfg, const uint32_t* cfg_mask, const uint32_t* cfg_rng,
                   uint32_t* d_words, uint32_t* d_counts, void* stream) {
  if (int rc = check_table("tw_mt_generate", n_states, stream_blocks)) return rc;
  Cfgs cf;
  if (int rc = check_cfgs("tw_mt_generate", n_cfg, cfg_mask, cfg_rng, &cf)) return rc;
  TW_ARG_CHECK(d_table && d_words && d_counts, "tw_mt_generate: null buffer");
  return launch_generate(d_table, n_states, stream_blocks, cf, d_words, d_counts,
                         (hipStream_t)stream);
}

int64_t tw_np_randint_dev_work_bytes(int32_t n_states, int32_t stream_blocks, int32_t n_calls,
                                     int32_t n_cfg) {
  if (n_states < 1 || stream_blocks < 1 || n_calls < 1 || n_cfg < 1 || n_cfg > kMaxCfg ||
      (int64_t)n_states * stream_blocks * kN > kMaxWords)
    return -1;
  const int64_t ng = (int64_t)n_states * stream_blocks;
  return (int64_t)Work(ng * kN, ng, n_calls, n_cfg).total;
}

int tw_np_randint_dev(uint32_t* key, int32_t* pos, const uint32_t* d_table, int32_t n_states,
                      int32_t stream_blocks, int32_t n_calls, const int32_t* call_cfg,
                      const int64_t* call_cnt, const int32_t* call_base, const int64_t* call_out,
                      int32_t n_cfg, const uint32_t* cfg_mask, const uint32_t* cfg_rng,
                      int32_t* d_out, int64_t out_len, void* d_work, int64_t* progress,
                      void* stream) {
  if (int rc = check_table("tw_np_randint_dev", n_states, stream_blocks)) return rc;
  Cfgs cf;
  if (int rc = check_cfgs("tw_np_randint_dev", n_cfg, cfg_mask, cfg_rng, &cf)) return rc;
  TW_ARG_CHECK(key && pos && *pos >= 0 && *pos <= kN, "tw_np_randint_dev: bad MT19937 state");
  TW_ARG_CHECK(n_calls >= 1 && call_cfg && call_cnt && call_base && call_out && progress &&
                   out_len >= 0,
               "tw_np_randint_dev: bad call tables (n_calls=%d)", n_calls);
  for (int32_t c = 0; c < n_calls; ++c)
    TW_ARG_CHECK(call_cfg[c] >= 0 && call_cfg[c] < n_cfg && call_cnt[c] >= 1 &&
                     call_cnt[c] <= kMaxWords && call_out[c] >= 0 &&
                     call_out[c] + call_cnt[c] <= out_len,
                 "tw_np_randint_dev: call %d is outside the output or its configuration", c);
  TW_ARG_CHECK(d_table && d_out && d_work, "tw_np_randint_dev: null device buffer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t L = (int64_t)stream_blocks * kN;
  const int ng = n_states * stream_blocks;
  const Work wk((int64_t)ng * kN, ng, n_calls, n_cfg);
  char* base = (char*)d_work;
  uint32_t* d_words = (uint32_t*)(base + wk.words);
  uint32_t* d_counts = (uint32_t*)(base + wk.counts);
  uint32_t* d_prefix = (uint32_t*)(base + wk.prefix);
  int32_t* d_ccfg = (int32_t*)(base + wk.ccfg);
  int64_t* d_ccnt = (int64_t*)(base + wk.ccnt);
  int32_t* d_cbase = (int32_t*)(base + wk.cbase);
  int64_t* d_cout = (int64_t*)(base + wk.cout);
  uint32_t* d_first = (uint32_t*)(base + wk.first);
  uint32_t* d_last = (uint32_t*)(base + wk.last);
  uint32_t* d_abase = (uint32_t*)(base + wk.abase);
  int64_t* d_result = (int64_t*)(base + wk.result);
  const size_t n = (size_t)n_calls;
  TW_HIP_CHECK(hipMemcpyAsync(d_ccfg, call_cfg, n * 4, hipMemcpyHostToDevice, st));
  TW_HIP_CHECK(hipMemcpyAsync(d_ccnt, call_cnt, n * 8, hipMemcpyHostToDevice, st));
  TW_HIP_CHECK(hipMemcpyAsync(d_cbase, call_base, n * 4, hipMemcpyHostToDevice, st));
  TW_HIP_CHECK(hipMemcpyAsync(d_cout, call_out, n * 8, hipMemcpyHostToDevice, st));
  if (int rc = launch_generate(d_table, n_states, stream_blocks, cf, d_words, d_counts, st))
    return rc;
  hipLaunchKernelGGL(k_scan_counts, dim3(n_cfg), dim3(1024), 0, st, d_counts, d_prefix, ng);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_resolve, dim3(1), dim3(256), 0, st, d_words, d_prefix, ng, cf, n_calls,
                     d_ccfg, d_ccnt, d_first, d_last, d_abase, (uint32_t)*pos, d_result);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_compact, dim3(ng), dim3(256), 0, st, d_words, d_prefix, ng, cf, d_ccfg,
                     d_ccnt, d_cbase, d_cout, d_first, d_last, d_abase, d_result, d_out, out_len);
  TW_LAUNCH_CHECK();
  int64_t res[4] = {0, 0, 0, 0};
  TW_HIP_CHECK(hipMemcpyAsync(res, d_result, sizeof res, hipMemcpyDeviceToHost, st));
  TW_HIP_CHECK(hipStreamSynchronize(st));
  const int64_t P = res[2];
  TW_ARG_CHECK(P >= *pos && P <= (int64_t)ng * kN && res[0] >= 0 && res[0] <= n_calls,
               "tw_np_randint_dev: the resolver returned an impossible position");
  progress[0] = res[0];
  progress[1] = res[1];
  progress[2] = P - *pos;
  if (P > *pos) {
    // NumPy's state after the word P - 1: the sub-stream holding it, as a whole key block (row
    // k >= 1 is the window at kL - 1: one recurrence step completes the block with the true
    // x[kL] in word 0), advanced by fewer than L + 1 words
    const int64_t k = (P - 1) / L;
    if (k > 0) {
      uint32_t U[kN];
      TW_HIP_CHECK(hipMemcpy(U, d_table + (size_t)k * kN, sizeof U, hipMemcpyDeviceToHost));
      for (int i = 0; i < kN - 1; ++i) key[i] = U[i + 1];
      key[kN - 1] = twist(U[0], U[1], U[kM]);
    }
    int32_t p = 0;
    std::vector<uint32_t> skipped((size_t)(P - k * L));
    tw_np_mt_next32(key, &p, P - k * L, skipped.data());
    *pos = p;
  }
  return TW_OK;
}

}  // extern "C"
