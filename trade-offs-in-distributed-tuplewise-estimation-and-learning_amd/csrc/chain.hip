// chain.hip — the T repartitions of one est.UnNT call as per-element CHAINS of positions, and
// the all-pairs counts of all T steps in ONE launch (round 4).
//
// Reference: est.UnN / UnNT  estimation-experiment/main.py:72-79 (repartition, count, repeat)
//            est.Un          estimation-experiment/main.py:29-31 (the strict predicate)
//
// The step structure of csrc/rankimage.hip (count step i, permute ALL records for step i+1 in
// the same launch) makes every step depend on the previous one through the whole array.  But a
// repartition is a keyed bijection of POSITIONS (csrc/feistel.h), so element e sits at step t
// at position P_t(e) = pi_t(P_{t-1}(e)), P_0(e) = e — a chain that depends on e alone.  And a
// step's count needs each shard's MULTISET of images, not their order.  So for a chunk of
// C <= 32 steps:
//  * k_chain_emit: every element walks its chain once (C forward Feistel evaluations, its
//    image in registers) and, per step, appends its image to the bag of the shard that holds
//    its position — an LDS histogram per block and round of steps, one cursor reservation per
//    (step, shard) and block, runs written coalesced (records.h's staging).  Over several ranks a
//    rank walks only ITS OWN elements and appends {image, local position} records to one
//    fixed-capacity bucket per (destination rank, step); ONE equal-split all-to-all per chunk
//    moves them and k_chain_unpack appends them to the receiver's (step, shard) bags (runs
//    reserved per block: a bag's multiset is what the count needs, not positions).
//  * k_count_chain: the C x N (step, shard) bags counted in one launch (k_count_rank's packed
//    f32 compare-and-count, its work items, XCD order and epilogue), counts [C][N].
//  * at the end of the call the scores in their final order: one scatter by the chains' last
//    positions (one process), or, over ranks, ONE all-to-all of the walked elements to the
//    ranks holding their final positions (k_chain_final_pack / k_chain_final_scatter).
// Work per element and step: one forward Feistel and a 4-B append, by exactly one rank — the
// repartitions no longer cost every rank the whole array.  The count launch has no random
// gathers, so its HBM traffic is the images themselves.  Same permutations (the keyed Feistel
// chain of est.UnNT's loop on the device), same counts, same final arrays as the step path.
//
// Half ties (tie_mode = "half"): an x image is the pair {g(x), h(x)}, h(x) = #{z : z <= x}
// (tw_rank_images_query with half = 1), and ONE clamped packed add gives [x > z] and [x >= z]
// for a z: clamp(h(x) - g(z)) == 1 <=> x >= z.  Half units = the sum of both lanes.
#include "bitcount.h"
#include "chainclass.h"
#include "chainplan.h"
#include "feistel.h"
#include "pkcount.h"
#include "records.h"

namespace tw {

constexpr int kChainMax = 32;            // steps per emission launch (keys in kernel args)
constexpr int kEmThreads = 256;
// tuning hooks (tw_chain_set_emit): elements per thread, steps per round; 0 = automatic
static int g_emit_epr = 0, g_emit_s = 0;
constexpr int kEmMaxB = 2 * kEmThreads;  // staged buckets (block_scan_excl's range)
constexpr int kEmMaxBig = 8192;          // buckets of the unstaged variant (LDS counters)

struct ChainKeys {
  uint64_t kx[kChainMax], kz[kChainMax];
};

struct ChainEmit {
  const uint64_t* xr;  // the emitting rank's X records (low word image; high word h when half)
  const uint64_t* zr;  // its Z records (low word: negated image)
  int64_t nx, nz;      // its element counts (every rank's local sizes)
  uint32_t* xpos;      // chain state: global position of each element at the last step done
  uint32_t* zpos;
  int first;           // no state yet: the position before step 0 is base + e
  int64_t xbase, zbase;
  int64_t NX, NZ;      // global sizes (the permutations' domains)
  int steps, half;
  // every rank's local prop-SWOR layout: shard s = [min(s k, n), min((s+1) k, n)), then the
  // tail that belongs to no shard
  int64_t kx, kz;
  FastDiv dkx, dkz;
  int nsh;
  // one process: bags [steps][nx] (4 B, or 8 B per x when half) and [steps][nz]; cursors
  // [steps][2][nsh + 1], zero on entry
  void* xbag;
  uint32_t* zbag;
  unsigned* cur;
  // the exchange (several ranks, or one rank forced through its collectives): per destination
  // g, steps buckets of 1 + cap records of W words (slot 0: the count), records {image
  // word(s), local position (z: nx + position)}
  int xchg, world, W;
  FastDiv dnx, dnz;
  uint64_t* send;
  int64_t cap;
  int* flag;
  int bx;  // blocks of X tiles; the rest are Z tiles
  // round tables (feistel.h; null: the arithmetic rounds): per (step, class) tab_stride
  // entries, class X first; hbx / hbz: the classes' half_bits
  const uint16_t* tab;
  uint32_t tab_stride, hbx, hbz;
};

// the round keys of a chunk's Feistel networks (host-made: k_chain_emit_prep's arguments)
struct ChainRounds {
  uint32_t k[kChainMax][2][6];
};

__device__ __forceinline__ int64_t em_region(int b, uint32_t k, int64_t n) {
  const int64_t o = (int64_t)b * k;
  return o < n ? o : n;
}

// next position of every element slot: one forward round set for all, then the cycle walks
// (4.6 % of the slots at n = 1e6 on a 2^20 domain) lane by lane — each lane takes ITS next
// walking slot, so a wave re-evaluates max-over-lanes times instead of once per slot with a
// walker anywhere in the wave (~0.95 of the slots)
// (once: one round set on a position — the arithmetic rounds or the table's)
template <int EPR, class Once>
__device__ __forceinline__ void chain_next(Once once, uint32_t Ntot, uint32_t (&pos)[EPR],
                                           unsigned valid) {
  unsigned walk = 0;
#pragma unroll
  for (int r = 0; r < EPR; ++r) {
    pos[r] = once(pos[r]);
    if (((valid >> r) & 1u) && pos[r] >= Ntot) walk |= 1u << r;
  }
  while (__any(walk != 0)) {
    if (walk) {
      const int r = __builtin_ctz(walk);
      uint32_t v = pos[0];
#pragma unroll
      for (int i = 1; i < EPR; ++i) v = i == r ? pos[i] : v;
      v = once(v);
#pragma unroll
      for (int i = 0; i < EPR; ++i) pos[i] = i == r ? v : pos[i];
      if (v < Ntot) walk &= ~(1u << r);
    }
  }
}

// The emission: each block walks its tile's chains through the chunk's steps, S steps per
// round: the positions of S steps (registers), ONE LDS histogram over the S x NB (step, bucket)
// counters, ONE reservation round of global adds and one staged write pass for all S steps.
// The per-round hand-offs (barriers, the cursor round trip) are a latency every block pays in
// sequence, so small problems (few blocks per CU) take several steps per round; large ones
// one (their blocks are issue-bound, and wider staging only costs occupancy).  A position walk
// kept in memory and placed by a second, fully parallel pass measured slower in both regimes
// (2e6 elements x 20 steps: 308 against 254 us; 250k: 59 against 52 us;
// profiles/r04_prof_parts3_stats.log) — it re-reads the images once per step.
//
// FULL: the staging of every mode (8-B values for half ties' {g, h} images, the exchange's
// position word).  One process with strict ties stages 4-B values only (FULL = false), which
// leaves the LDS for the round table below without costing a resident block.
//
// Round tables (em.tab, feistel.h): the block keeps the current step's table of its class in
// dynamic LDS, copied from the launch's workspace (k_chain_emit_prep) with 16-B loads.  A
// step's table is dead once every thread has left chain_next — after the round's first
// barrier — so the next step's copy is issued there and is visible after the round's later
// barriers: no barrier is added at one step per round.  With several steps per round each
// further step of the round pays two barriers around its copy.
//
// Destinations: the reservation loop has (step, bucket) of every counter anyway, so it leaves
// the counter's destination in LDS (dst: one process, the element offset c n + region(b) +
// reserved; the exchange, the record slot (b steps + c)(cap + 1) + 1 + reserved) and a staged
// record costs one LDS read, one add and the store — no division, no 64-bit multiply.
template <int EPR, int S, bool STAGED, bool FULL>
__global__ __launch_bounds__(kEmThreads) void k_chain_emit(ChainEmit em, ChainKeys keys) {
  constexpr int TILE = kEmThreads * EPR;
  constexpr int MB = STAGED ? kEmMaxB : kEmMaxBig;
  using SV = std::conditional_t<FULL, uint64_t, uint32_t>;
  extern __shared__ uint4 tabq[];
  __shared__ Feistel fs[kChainMax];
  __shared__ unsigned hist[MB], base[STAGED && !FULL ? 1 : MB], start[STAGED ? kEmMaxB : 1];
  __shared__ uint64_t dst[STAGED ? kEmMaxB : 1];
  __shared__ unsigned wave_tot[kEmThreads / kWave];
  __shared__ SV sv[STAGED ? TILE * S : 1];
  __shared__ uint32_t sq[STAGED && FULL ? TILE * S : 1];
  __shared__ uint16_t sb[STAGED ? TILE * S : 1];
  const bool isx = (int)blockIdx.x < em.bx;
  const int tile = isx ? (int)blockIdx.x : (int)blockIdx.x - em.bx;
  const int64_t n = isx ? em.nx : em.nz;
  const int64_t Ntot = isx ? em.NX : em.NZ;
  if ((int)threadIdx.x < em.steps)
    fs[threadIdx.x] = make_feistel(Ntot > 1 ? Ntot : 1, isx ? keys.kx[threadIdx.x]
                                                           : keys.kz[threadIdx.x]);
  const uint64_t* rec = isx ? em.xr : em.zr;
  uint32_t* posa = isx ? em.xpos : em.zpos;
  const int64_t gbase = isx ? em.xbase : em.zbase;
  const bool xchg = FULL && em.xchg;
  const bool wide = FULL && isx && em.half;  // 8-B x images {g, h}
  const uint16_t* tab = (const uint16_t*)tabq;
  const bool tabs = em.tab != nullptr;
  const uint32_t hb = isx ? em.hbx : em.hbz, hmask = (1u << hb) - 1;
  auto tab_load = [&](int c) {  // step c's table of this class (tab_stride covers the pad)
    const uint4* src =
        (const uint4*)(em.tab + ((size_t)c * 2 + (isx ? 0 : 1)) * em.tab_stride);
    const int nq = (int)(((6u << hb) + 7) / 8);
    for (int q = threadIdx.x; q < nq; q += kEmThreads) tabq[q] = src[q];
  };
  if (tabs) tab_load(0);
  SV val[EPR];
  uint32_t pos[EPR];
  unsigned valid = 0;
  const int64_t e0 = (int64_t)tile * TILE + threadIdx.x;
#pragma unroll
  for (int r = 0; r < EPR; ++r) {
    const int64_t e = e0 + (int64_t)r * kEmThreads;
    val[r] = 0;
    pos[r] = 0;
    if (e < n) {
      valid |= 1u << r;
      const uint64_t v = rec[e];
      val[r] = (SV)(wide ? v : (v & 0xFFFFFFFFull));
      pos[r] = em.first ? (uint32_t)(gbase + e) : posa[e];
    }
  }
  const int N = em.nsh;
  const int NB = xchg ? em.world : N + 1;
  const uint32_t kb = (uint32_t)(isx ? em.kx : em.kz);
  const FastDiv dk = isx ? em.dkx : em.dkz;
  const FastDiv dn = isx ? em.dnx : em.dnz;
  const int cnt = (int)min<int64_t>(TILE, n - (int64_t)tile * TILE);
  for (int i = threadIdx.x; i < S * NB && i < MB; i += kEmThreads) hist[i] = 0;
  __syncthreads();  // fs, hist
  for (int c0 = 0; c0 < em.steps; c0 += S) {
    const int ns = min(S, em.steps - c0);
    int bk[S][EPR];
    uint32_t aux[S][EPR];
    unsigned slot[S][EPR];
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
      for (int r = 0; r < EPR; ++r) {
        bk[s][r] = -1;
        aux[s][r] = 0;
        slot[s][r] = 0;
      }
      if (s < ns) {
        if (tabs) {
          if (S > 1 && s > 0) {  // (block-uniform) the round's further steps: their own copy
            __syncthreads();
            tab_load(c0 + s);
            __syncthreads();
          }
          chain_next<EPR>([&](uint32_t v) { return feistel_once32_tab(tab, hb, hmask, v); },
                          (uint32_t)Ntot, pos, valid);
        } else {
          const Feistel& F = fs[c0 + s];
          chain_next<EPR>([&](uint32_t v) { return feistel_once32(F, v); }, (uint32_t)Ntot, pos,
                          valid);
        }
#pragma unroll
        for (int r = 0; r < EPR; ++r) {
          if ((valid >> r) & 1u) {
            const uint32_t q = pos[r];
            int b;
            if (xchg) {
              const uint32_t g = fast_div32(q, dn);
              const uint32_t ql = q - g * (uint32_t)n;
              b = (int)g;
              aux[s][r] = isx ? ql : (uint32_t)em.nx + ql;
            } else {
              b = kb == 0 ? N : (int)min(fast_div32(q, dk), (uint32_t)N);
            }
            bk[s][r] = s * NB + b;
            slot[s][r] = atomicAdd(&hist[s * NB + b], 1u);
          }
        }
      }
    }
    __syncthreads();
    // every thread has left chain_next: the table is dead, the next round's first copy goes
    if (tabs && c0 + ns < em.steps) tab_load(c0 + ns);
    const int nc = ns * NB;
    for (int i = threadIdx.x; i < nc; i += kEmThreads) {
      const int s = S == 1 ? 0 : i / NB, b = i - s * NB;
      const int c = c0 + s;
      const unsigned h = hist[i];
      unsigned* cu;
      if (xchg)
        cu = (unsigned*)(em.send + ((int64_t)b * em.steps + c) * (em.cap + 1) * em.W);
      else
        cu = em.cur + ((int64_t)c * 2 + (isx ? 0 : 1)) * (N + 1) + b;
      const unsigned got = h ? atomicAdd(cu, h) : 0u;
      if constexpr (!STAGED || FULL) base[i] = got;
      if constexpr (STAGED) {
        start[i] = h;
        dst[i] = xchg ? (uint64_t)(((int64_t)b * em.steps + c) * (em.cap + 1) + 1 + got)
                      : (uint64_t)((int64_t)c * n + em_region(b, kb, n) + got);
      }
      hist[i] = 0;  // for the next round (its atomics come after the next barrier)
    }
    __syncthreads();
    // one record of the unstaged form: counter i = s * NB + b (step c0 + s, bucket b), slot u
    // in the bucket's run
    auto put = [&](int i, unsigned u, uint64_t v, uint32_t a) {
      const int s = S == 1 ? 0 : i / NB, b = i - s * NB;
      const int c = c0 + s;
      if (xchg) {
        if ((int64_t)u >= em.cap) {
          *em.flag = 1;  // dropped, never written out of place; the host raises
          return;
        }
        uint64_t* d = em.send + (((int64_t)b * em.steps + c) * (em.cap + 1) + 1 + u) * em.W;
        if (em.W == 1) {
          d[0] = v | ((uint64_t)a << 32);
        } else {
          d[0] = v;
          d[1] = a;
        }
      } else {
        const int64_t o = (int64_t)c * n + em_region(b, kb, n) + u;
        if (wide)
          ((uint64_t*)em.xbag)[o] = v;
        else
          (isx ? (uint32_t*)em.xbag : em.zbag)[o] = (uint32_t)v;
      }
    };
    if constexpr (STAGED) {
      block_scan_excl<kEmThreads>(start, nc, wave_tot);
#pragma unroll
      for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int r = 0; r < EPR; ++r) {
          if (bk[s][r] < 0) continue;
          const unsigned j = start[bk[s][r]] + slot[s][r];
          sv[j] = val[r];
          if constexpr (FULL) sq[j] = aux[s][r];
          sb[j] = (uint16_t)bk[s][r];
        }
      }
      __syncthreads();
      // a staged record: its counter's destination (dst) plus its place in the counter's run
      for (int j = threadIdx.x; j < cnt * ns; j += kEmThreads) {
        const int i = sb[j];
        const unsigned rel = (unsigned)j - start[i];
        const uint64_t o = dst[i] + rel;
        if (xchg) {
          if ((int64_t)base[i] + rel >= em.cap) {
            *em.flag = 1;  // dropped, never written out of place; the host raises
            continue;
          }
          const uint64_t v = sv[j];
          if (em.W == 1) {
            em.send[o] = v | ((uint64_t)sq[FULL ? j : 0] << 32);
          } else {
            em.send[2 * o] = v;
            em.send[2 * o + 1] = sq[FULL ? j : 0];
          }
        } else if (wide) {
          ((uint64_t*)em.xbag)[o] = sv[j];
        } else {
          (isx ? (uint32_t*)em.xbag : em.zbag)[o] = (uint32_t)sv[j];
        }
      }
      __syncthreads();  // staging, start[] and dst[] are reused by the next round
    } else {
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int r = 0; r < EPR; ++r)
          if (bk[s][r] >= 0) put(bk[s][r], base[bk[s][r]] + slot[s][r], val[r], aux[s][r]);
    }
  }
#pragma unroll
  for (int r = 0; r < EPR; ++r) {
    const int64_t e = e0 + (int64_t)r * kEmThreads;
    if (e < n) posa[e] = pos[r];
  }
}

// What an emission launch needs beforehand, in ONE launch: the cursors (one process: `words`
// 4-B words at `zero`) or the send heads (the exchange: `words` buckets of `stride` 8-B words)
// zeroed, and — with round tables — the chunk's tables: blockIdx.y = 2 step + class, F_i(R)
// at tab[blockIdx.y * tab_stride + (i << hb) + R] (the pad up to tab_stride is never looked up).
__global__ __launch_bounds__(kBlock) void k_chain_emit_prep(void* __restrict__ zero, int64_t words,
                                                            int64_t stride, ChainRounds rk,
                                                            uint16_t* __restrict__ tab,
                                                            uint32_t tab_stride, uint32_t hbx,
                                                            uint32_t hbz) {
  const int64_t t0 = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
  const int64_t nt = (int64_t)gridDim.x * gridDim.y * kBlock;
  if (stride == 0) {
    for (int64_t i = t0; i < words; i += nt) ((unsigned*)zero)[i] = 0;
  } else {
    for (int64_t i = t0; i < words; i += nt) ((uint64_t*)zero)[i * stride] = 0;
  }
  if (tab == nullptr) return;
  const int c = blockIdx.y >> 1, cls = blockIdx.y & 1;
  const uint32_t hb = cls ? hbz : hbx, mask = (1u << hb) - 1;
  uint16_t* out = tab + (size_t)blockIdx.y * tab_stride;
  for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < (6u << hb); e += gridDim.x * kBlock)
    out[e] = feistel_round_value(e & mask, rk.k[c][cls][e >> hb], mask);
}

// Receiver side: every record of bucket (source g, step c) appended to its (step, side, shard)
// bag region.  The count needs each bag's multiset, not the positions inside it, so a block
// histograms its records over the step's 2 (nsh + 1) regions in LDS, reserves one run per
// (block, region) with one global atomic on the step's cursors, and writes each record into
// its run — whole lines per run, where one scattered 4-B store per record at its position
// (round 4) made every line a partial write: 0.37 ms per 20 steps at G = 2, whose 4-MB step
// bags overflow an XCD's L2.  Region b of a side starts at min(b k, n) (em_region: shard b,
// and b = nsh the tail that belongs to no shard).  Logical blocks are step-major and dealt to
// the XCDs in contiguous ranges (xcd_block), so one step's runs meet in one L2.
constexpr int kUnpackPer = 4;  // records per thread and round
__global__ __launch_bounds__(kBlock) void k_chain_unpack(
    const uint64_t* __restrict__ recv, int world, int steps, int parts, int64_t cap, int W,
    int half, int64_t nx, int64_t nz, int64_t kx, int64_t kz, int nsh, void* __restrict__ xbag,
    uint32_t* __restrict__ zbag, unsigned* __restrict__ cursors, int* __restrict__ flag) {
  extern __shared__ unsigned un_lds[];  // hist[NB], base[NB]
  const int NB = 2 * (nsh + 1);
  unsigned* hist = un_lds;
  unsigned* base = un_lds + NB;
  const int lb = xcd_block(blockIdx.x, gridDim.x);
  const int c = lb / (world * parts);
  const int rem = lb - c * world * parts;
  const int g = rem / parts, part = rem - g * parts;
  const uint64_t* b = recv + ((int64_t)g * steps + c) * (cap + 1) * W;
  const int64_t cnt0 = (int64_t)(uint32_t)b[0];
  if (cnt0 > cap && part == 0 && threadIdx.x == 0) *flag = 1;
  const int64_t cnt = cnt0 < cap ? cnt0 : cap;
  unsigned* cur = cursors + (int64_t)c * NB;
  for (int j = threadIdx.x; j < NB; j += kBlock) hist[j] = 0;
  __syncthreads();
  constexpr int64_t kRound = (int64_t)kBlock * kUnpackPer;
  for (int64_t i0 = (int64_t)part * kRound; i0 < cnt; i0 += (int64_t)parts * kRound) {
    uint64_t v[kUnpackPer];
    int bk[kUnpackPer];
    unsigned slot[kUnpackPer];
#pragma unroll
    for (int u = 0; u < kUnpackPer; ++u) {
      const int64_t i = i0 + (int64_t)u * kBlock + threadIdx.x;
      bk[u] = -1;
      v[u] = 0;
      slot[u] = 0;
      if (i < cnt) {
        const uint64_t* r = b + (1 + i) * W;
        v[u] = W == 1 ? (r[0] & 0xFFFFFFFFull) : r[0];
        const int64_t p = W == 1 ? (int64_t)(r[0] >> 32) : (int64_t)r[1];
        if (p < nx) {
          bk[u] = kx > 0 ? (int)min<int64_t>(p / kx, nsh) : nsh;
        } else if (p < nx + nz) {
          const int64_t q = p - nx;
          bk[u] = (nsh + 1) + (kz > 0 ? (int)min<int64_t>(q / kz, nsh) : nsh);
        }
        if (bk[u] >= 0) slot[u] = atomicAdd(&hist[bk[u]], 1u);
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < NB; j += kBlock) {
      const unsigned h = hist[j];
      base[j] = h ? atomicAdd(cur + j, h) : 0u;
      hist[j] = 0;  // for the next round (its atomics come after the next barrier)
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kUnpackPer; ++u) {
      if (bk[u] < 0) continue;
      const bool isx = bk[u] <= nsh;
      const int rb = isx ? bk[u] : bk[u] - (nsh + 1);
      const int64_t o = em_region(rb, (uint32_t)(isx ? kx : kz), isx ? nx : nz) + base[bk[u]] +
                        slot[u];
      if (isx) {
        if (half)
          ((uint64_t*)xbag)[(int64_t)c * nx + o] = v[u];
        else
          ((uint32_t*)xbag)[(int64_t)c * nx + o] = (uint32_t)v[u];
      } else {
        zbag[(int64_t)c * nz + o] = (uint32_t)v[u];
      }
    }
    __syncthreads();  // base[] is rewritten by the next round
  }
}

// ----------------------------------------------------------------------------- the count
// One wave item: 64*R x-images (strict: R/2 packed pairs per lane; half: R {g, h} pairs) of
// one (step, shard) bag against z images [z0, z1) of it, z streamed through the scalar cache
// (16 images per s_load_dwordx16, the next group in flight while one is compared).
template <int R, bool HALF>
__device__ __forceinline__ unsigned long long count_chain_item(const void* __restrict__ xb,
                                                               int64_t x0, int64_t xe,
                                                               const float* __restrict__ zf,
                                                               int64_t z0, int64_t z1, int lane) {
  constexpr int P = HALF ? R : R / 2;
  f2 xv[P], acc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if constexpr (HALF) {
      const int64_t i = x0 + p * kWave + lane;
      xv[p] = i < xe ? ((const f2*)xb)[i] : f2{kImgNever, kImgNever};
    } else {
      const int64_t i0 = x0 + (2 * p) * kWave + lane, i1 = i0 + kWave;
      const float* xf = (const float*)xb;
      xv[p].x = i0 < xe ? xf[i0] : kImgNever;  // padded lanes: never greater
      xv[p].y = i1 < xe ? xf[i1] : kImgNever;
    }
    acc[p] = f2{0.f, 0.f};
  }
  // all compares of one z first, then the accumulations
  auto z_lo = [&](uint64_t zu) {
    f2 t[P];
#pragma unroll
    for (int p = 0; p < P; ++p) t[p] = gt_clamp(xv[p], zu);
#pragma unroll
    for (int p = 0; p < P; ++p) acc_add(acc[p], t[p]);
  };
  auto z_hi = [&](uint64_t zu) {
    f2 t[P];
#pragma unroll
    for (int p = 0; p < P; ++p) t[p] = gt_clamp_hi(xv[p], zu);
#pragma unroll
    for (int p = 0; p < P; ++p) acc_add(acc[p], t[p]);
  };
  auto z_pair = [&](uint64_t zu) {
    z_lo(zu);
    z_hi(zu);
  };
  const float* __restrict__ zp = zf + z0;
  const int nz = (int)(z1 - z0);
  int j = 0;
  if (nz > 0 && ((uintptr_t)zp & 7)) {  // an odd first image: alone, then aligned pairs
    z_lo((uint64_t)__float_as_uint(zp[0]));
    j = 1;
  }
  const uint64_t* __restrict__ q = (const uint64_t*)(zp + j);
  const int np = (nz - j) >> 1;
  int i = 0;
  if (np >= 16) {
    uint64_t za[8], zb[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) za[u] = q[u];
    const int last = np - 8;
    for (; i + 16 <= np; i += 16) {
      const uint64_t* qb = q + i + 8;
#pragma unroll
      for (int u = 0; u < 8; ++u) zb[u] = qb[u];
#pragma unroll
      for (int u = 0; u < 8; ++u) z_pair(za[u]);
      const uint64_t* qa = q + (i + 16 <= last ? i + 16 : last);
#pragma unroll
      for (int u = 0; u < 8; ++u) za[u] = qa[u];
#pragma unroll
      for (int u = 0; u < 8; ++u) z_pair(zb[u]);
    }
  }
  for (; i + 8 <= np; i += 8) {
    uint64_t zv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) zv[u] = q[i + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) z_pair(zv[u]);
  }
  for (; i < np; ++i) z_pair(q[i]);
  if ((nz - j) & 1) z_lo((uint64_t)__float_as_uint(zp[nz - 1]));
  unsigned long long tot = 0;
#pragma unroll
  for (int p = 0; p < P; ++p) tot += (unsigned)acc[p].x + (unsigned)acc[p].y;  // exact < 2^24
  return wave_sum_u64(tot);
}

// The count's epilogue: the block's wave totals, one u64 atomic per block and bag (v: the
// wave's bag; active: it counted one).
__device__ __forceinline__ void count_chain_epilogue(unsigned long long tot, bool active, int v,
                                                     int wid, int lane,
                                                     unsigned long long* __restrict__ out) {
  __shared__ unsigned long long part[kBlock / kWave];
  __shared__ int part_v[kBlock / kWave];
  if (lane == 0) {
    part[wid] = tot;
    part_v[wid] = active ? v : -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int cur = part_v[0];
    unsigned long long sum = part[0];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) {
      if (part_v[w] != cur) {
        if (cur >= 0 && sum) atomicAdd(out + cur, sum);
        cur = part_v[w];
        sum = 0;
      }
      sum += part[w];
    }
    if (cur >= 0 && sum) atomicAdd(out + cur, sum);
  }
}

// Work items as k_count_rank (csrc/rankimage.hip): per wave (bag v = step * N + shard, x tile,
// z chunk), shard-major logical order dealt to the XCDs in contiguous ranges, one u64 atomic
// per block and bag.  TILE: x images per item; item(x0, xe, z0, z1, lane) -> the lane's count.
template <int TILE, class Item>
__device__ __forceinline__ void count_chain_block(const int64_t* __restrict__ x_off,
                                                  int64_t x_stride,
                                                  const int64_t* __restrict__ z_off,
                                                  int64_t z_stride, int n_shards, int n_bags,
                                                  int tiles_x, int zchunks, int64_t z_chunk,
                                                  unsigned long long* __restrict__ out,
                                                  Item item_count) {
  const int per_bag = tiles_x * zchunks;
  const int lb = xcd_block(blockIdx.x, gridDim.x);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int item = lb * (kBlock / kWave) + wid;
  const int v = item / per_bag;
  bool active = v < n_bags;
  int64_t x0 = 0, xe = 0, z0 = 0, z1 = 0;
  if (active) {
    const int c = v / n_shards, s = v - c * n_shards;
    const int rem = item - v * per_bag;
    const int cz = rem / tiles_x;
    const int tx = rem - cz * tiles_x;
    const int64_t xo = (int64_t)c * x_stride, zo = (int64_t)c * z_stride;
    const int64_t xbg = xo + x_off[s], zbg = zo + z_off[s], ze = zo + z_off[s + 1];
    xe = xo + x_off[s + 1];
    x0 = xbg + (int64_t)tx * TILE;
    z0 = zbg + (int64_t)cz * z_chunk;
    z1 = (z0 + z_chunk < ze) ? z0 + z_chunk : ze;
    active = x0 < xe && z0 < ze;
  }
  unsigned long long tot = 0;
  if (active) tot = item_count(x0, xe, z0, z1, lane);
  count_chain_epilogue(tot, active, v, wid, lane, out);
}

template <int R, bool HALF>
__global__ __launch_bounds__(kBlock) void k_count_chain(
    const void* __restrict__ xb, const int64_t* __restrict__ x_off, int64_t x_stride,
    const float* __restrict__ zb, const int64_t* __restrict__ z_off, int64_t z_stride,
    int n_shards, int n_bags, int tiles_x, int zchunks, int64_t z_chunk,
    unsigned long long* __restrict__ out) {
  count_chain_block<kWave * R>(
      x_off, x_stride, z_off, z_stride, n_shards, n_bags, tiles_x, zchunks, z_chunk, out,
      [&](int64_t x0, int64_t xe, int64_t z0, int64_t z1, int lane) {
        return count_chain_item<R, HALF>(xb, x0, xe, zb, z0, z1, lane);
      });
}

// The bit-sliced count (bitcount.h; strict predicate, images in [0, 2^NB)) on planes built once
// per bag (chainplan.h): NB + 1 VALU instructions per 64 * 32 pairs where the
// packed form takes 32.  A pre-pass makes the planes once:
// one wave per (bag, group of 2048 images, side) loads the group's 32 images per lane (bit k
// of lane l: image g * 2048 + k * 64 + l), converts them (x: bits_x_image; z: complemented,
// bits_z_image), transposes and stores NB planes of 64 u32 — one 256-B store each.  Slots past
// the bag's end hold 0 on either side (z: kBitsZNever), so they count nothing in either role.
// Only the groups the bag's items read are written: its full x groups (and a padded last one
// where the remainder is not swapped), its z groups where it is.
template <int NB>
__device__ __forceinline__ void chain_planes_wave(
    int64_t block, const float* __restrict__ xb, const int64_t* __restrict__ x_off,
    int64_t x_stride, const float* __restrict__ zb, const int64_t* __restrict__ z_off,
    int64_t z_stride, int n_shards, int n_bags, int gx, int gz, int swap,
    uint32_t* __restrict__ work) {
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const PlanesWave pw = planes_wave(block * (kBlock / kWave) + wid, n_bags, gx, gz);
  if (!pw.active) return;
  const bool zside = pw.zside;
  const int v = pw.bag, g = pw.g;
  const int c = v / n_shards, s = v - c * n_shards;
  const int64_t nx = x_off[s + 1] - x_off[s], nz = z_off[s + 1] - z_off[s];
  const PlanesBag bag = planes_bag(nx, nz, swap != 0);
  if (g >= (zside ? bag.zgroups : bag.xgroups)) return;
  const float* __restrict__ src =
      zside ? zb + bits_uniform((int64_t)c * z_stride + z_off[s] + (int64_t)g * kPlaneGroup)
            : xb + bits_uniform((int64_t)c * x_stride + x_off[s] + (int64_t)g * kPlaneGroup);
  const int cnt =  // >= 1
      __builtin_amdgcn_readfirstlane((int)min((int64_t)kPlaneGroup,
                                              (zside ? nz : nx) - (int64_t)g * kPlaneGroup));
  float raw[32];
  uint32_t a[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) raw[k] = src[min(k * 64 + lane, cnt - 1)];
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const uint32_t img = zside ? bits_z_image(raw[k]) : bits_x_image(raw[k]);
    a[k] = k * 64 + lane < cnt ? img : (zside ? kBitsZNever : 0u);
  }
  bits_transpose32(a);
  uint32_t* __restrict__ dst = work + bits_uniform(planes_word(NB, pw.group, 0, 0));
#pragma unroll
  for (int b = 0; b < NB; ++b) dst[b * 64 + lane] = a[b];
}

template <int NB>
__global__ __launch_bounds__(kBlock) void k_chain_planes(
    const float* __restrict__ xb, const int64_t* __restrict__ x_off, int64_t x_stride,
    const float* __restrict__ zb, const int64_t* __restrict__ z_off, int64_t z_stride,
    int n_shards, int n_bags, int gx, int gz, int swap, uint32_t* __restrict__ work) {
  chain_planes_wave<NB>(blockIdx.x, xb, x_off, x_stride, zb, z_off, z_stride, n_shards, n_bags,
                        gx, gz, swap, work);
}

// The count on those planes: work items of chainplan.h (a plane item: up to p.R x groups
// against a z chunk; a swapped item: an x-remainder chunk against up to p.R z groups) in
// count_chain_block's XCD order and with its epilogue.  The groups of an item are
// wave-uniform, so it runs the instantiation for exactly that many: no group tests in the loop.
template <int NB>
__global__ __launch_bounds__(kBlock) void k_count_chain_planes(
    const float* __restrict__ xb, const int64_t* __restrict__ x_off, int64_t x_stride,
    const float* __restrict__ zb, const int64_t* __restrict__ z_off, int64_t z_stride,
    int n_shards, int n_bags, PlanesPlan p, const uint32_t* __restrict__ work,
    unsigned long long* __restrict__ out) {
  const int lb = xcd_block(blockIdx.x, gridDim.x);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int item = lb * (kBlock / kWave) + wid;
  const int v = item / p.per_bag;
  bool active = v < n_bags;
  unsigned long long tot = 0;
  if (active) {
    const int c = v / n_shards, s = v - c * n_shards;
    const int64_t nx = x_off[s + 1] - x_off[s], nz = z_off[s + 1] - z_off[s];
    const PlanesItem it = planes_item(p, nx, nz, item - v * p.per_bag);
    active = it.active;
    if (active) {
      const int64_t group = it.swapped ? (int64_t)n_bags * p.gx + (int64_t)v * p.gz + it.g0
                                       : (int64_t)v * p.gx + it.g0;
      const uint32_t* __restrict__ pw = work + bits_uniform(planes_word(NB, group, 0, 0));
      const float* __restrict__ sf =
          it.swapped ? xb + bits_uniform((int64_t)c * x_stride + x_off[s] + it.s0)
                     : zb + bits_uniform((int64_t)c * z_stride + z_off[s] + it.s0);
      const int ns = __builtin_amdgcn_readfirstlane((int)(it.s1 - it.s0));
      const int ng = __builtin_amdgcn_readfirstlane(it.ng);
      unsigned long long t;
      if (ng == 4)
        t = bits_count_planes<NB, 4>(pw, sf, ns, it.swapped, lane);
      else if (ng == 3)
        t = bits_count_planes<NB, 3>(pw, sf, ns, it.swapped, lane);
      else if (ng == 2)
        t = bits_count_planes<NB, 2>(pw, sf, ns, it.swapped, lane);
      else
        t = bits_count_planes<NB, 1>(pw, sf, ns, it.swapped, lane);
      tot = wave_sum_u64(t);
    }
  }
  count_chain_epilogue(tot, active, v, wid, lane, out);
}

// The class-run form of that count (chainclass.h).  Pre-pass 2, one block per
// bag: the bag's z images, complemented (bits_z_image), are counting-sorted by class — the top
// cp.k of their low nb bits — into the class-ordered region of the workspace, and the bag's run
// table is written: per non-empty class ceil(n_c / cp.chunk) runs of near-equal length.  Two
// passes over the images in global memory (histogram; scatter through LDS cursors), so a bag
// of any size goes through; the order inside a class is that of the cursors' atomics, which
// the counts — integer sums — do not see.  With cp.digits > 0 (the digit loop)
// an image is stored digit-ready (class_digit_encode; class_wide_encode where cp.dbits asks for
// the wide digits of §4.1k, class_lds_encode for the LDS-table form of §4.1m): one word per image
// in every form, written anew by every launch.
__device__ __forceinline__ uint32_t class_block_scan(uint32_t v, uint32_t* wsum, int lane,
                                                     int wid) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  if (lane == kWave - 1) wsum[wid] = v;
  __syncthreads();
  uint32_t add = 0;
  for (int w = 0; w < wid; ++w) add += wsum[w];
  __syncthreads();
  return v + add;  // inclusive
}

// the word pre-pass 2 stores for a complemented z image under the launch's loop
__device__ __forceinline__ uint32_t class_store_word(uint32_t zc, const ClassPlan& cp) {
  return cp.digits <= 0                 ? zc
         : cp.dbits == kClassLdsBits  ? class_lds_encode(zc)
         : cp.dbits == kClassWideBits ? class_wide_encode(zc)
                                      : class_digit_encode(zc, cp.digits);
}

// The same word from the launch's form spelled out once per block: field j is bits sh[j] ..
// of the image under mk[j], stored at bit at[j] (the digit loops: digit j in byte j; the
// LDS-table form: the top digit at bit 0, the low byte at bit 9)
struct ClassStoreForm {
  bool plain;  // the complemented image itself
  int sh[kClassDigits], at[kClassDigits];
  uint32_t mk[kClassDigits];
};
__device__ __forceinline__ ClassStoreForm class_store_form(const ClassPlan& cp) {
  ClassStoreForm e{};
  e.plain = cp.digits <= 0;
  const bool wide = cp.dbits == kClassWideBits, lds = cp.dbits == kClassLdsBits;
  const int nl = e.plain ? kClassDigitMaxNL : cp.digits;
#pragma unroll
  for (int j = 0; j < kClassDigits; ++j) {
    e.sh[j] = wide ? kClassWideBits * j : class_digit_shift(nl, j);
    e.mk[j] = wide ? (j < kClassWideDigits ? (1u << kClassWideBits) - 1u : 0u)
                   : (1u << class_digit_width(nl, j)) - 1u;
    e.at[j] = 8 * j;
  }
  if (lds) {  // class_lds_encode: two fields
    e.sh[0] = kClassLdsBits, e.mk[0] = (1u << kClassWideBits) - 1u, e.at[0] = 0;
    e.sh[1] = 0, e.mk[1] = (uint32_t)(kClassLdsEntries - 1), e.at[1] = 9;
#pragma unroll
    for (int j = 2; j < kClassDigits; ++j) e.sh[j] = 0, e.mk[j] = 0u, e.at[j] = 0;
  }
  return e;
}
__device__ __forceinline__ uint32_t class_store_word(uint32_t zc, const ClassStoreForm& e) {
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < kClassDigits; ++j) w |= ((zc >> e.sh[j]) & e.mk[j]) << e.at[j];
  return e.plain ? zc : w;
}

// From the bag's class histogram in hist (one thread per class, all of it written): the bag's
// entry count and run table go to the workspace and hist becomes the classes' first positions
// c0 in the class-ordered region.  Ends behind a barrier.  SMALL: a bag of at most kPrepassCap
// images, whose runs are cut in 32-bit arithmetic (class_run32: the same runs).
template <bool SMALL = false>
__device__ __forceinline__ void class_block_tables(uint32_t* hist, uint32_t* wsum, int v,
                                                   const ClassPlan& cp,
                                                   uint32_t* __restrict__ work) {
  const int t = threadIdx.x, lane = t & (kWave - 1), wid = t / kWave;
  const uint32_t n = hist[t];  // (classes >= 2^k: 0)
  const uint32_t nr = (uint32_t)class_runs(n, cp.chunk);
  const uint32_t c0 = class_block_scan(n, wsum, lane, wid) - n;
  const uint32_t e1 = class_block_scan(nr, wsum, lane, wid), e0 = e1 - nr;
  hist[t] = c0;  // (every thread read its own count above)
  if (t == kBlock - 1) work[cp.off_cnt + v] = e1;  // <= cp.cap (class_capacity)
  uint32_t* __restrict__ tab = work + (cp.off_tab + (int64_t)v * 2 * cp.cap);
  for (uint32_t j = 0; j < nr; ++j) {
    const ClassRun r =
        SMALL ? class_run32(c0, n, nr, j, (uint32_t)t) : class_run(c0, n, nr, j, (uint32_t)t);
    tab[2 * (e0 + j)] = class_entry_lo(r);
    tab[2 * (e0 + j) + 1] = class_entry_hi(r);
  }
  __syncthreads();
}

// A bag of any size: two passes over its images in global memory
__device__ __forceinline__ void chain_zclasses_stream(const float* __restrict__ src, int64_t nz,
                                                      int v, int nb, const ClassPlan& cp,
                                                      uint32_t* hist, uint32_t* wsum,
                                                      uint32_t* __restrict__ work) {
  const int t = threadIdx.x;
  hist[t] = 0;
  __syncthreads();
  constexpr int U = 8;  // loads in flight per thread: a block walks its whole bag
  for (int64_t i0 = t; i0 < nz; i0 += kBlock * U) {
    float f[U];
#pragma unroll
    for (int u = 0; u < U; ++u) f[u] = src[min(i0 + u * kBlock, nz - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + u * kBlock < nz) atomicAdd(&hist[class_of(bits_z_image(f[u]), nb, cp.k)], 1u);
  }
  __syncthreads();
  class_block_tables(hist, wsum, v, cp, work);  // hist: now the classes' cursors
  uint32_t* __restrict__ zs = work + (cp.off_zs + (int64_t)v * cp.zs_stride);
  for (int64_t i0 = t; i0 < nz; i0 += kBlock * U) {
    float f[U];
#pragma unroll
    for (int u = 0; u < U; ++u) f[u] = src[min(i0 + u * kBlock, nz - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t zc = bits_z_image(f[u]);
      if (i0 + u * kBlock < nz)
        zs[atomicAdd(&hist[class_of(zc, nb, cp.k)], 1u)] =  // < c0 + n <= nz
            class_store_word(zc, cp);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_chain_zclasses(
    const float* __restrict__ zb, const int64_t* __restrict__ z_off, int64_t z_stride,
    int n_shards, int n_bags, int nb, ClassPlan cp, uint32_t* __restrict__ work) {
  static_assert(kBlock == 1 << kClassMaxBits, "one thread per class");
  __shared__ uint32_t hist[kBlock], wsum[kBlock / kWave];
  const int v = blockIdx.x;  // < n_bags
  const int c = v / n_shards, s = v - c * n_shards;
  const int64_t nz = z_off[s + 1] - z_off[s];
  const float* __restrict__ src = zb + ((int64_t)c * z_stride + z_off[s]);
  chain_zclasses_stream(src, nz, v, nb, cp, hist, wsum, work);
}

// The same sort with the bag in registers: 1 <= nz <= kBlock * PER images, PER
// per thread, every load issued before the first use and every image read from global memory
// once.  The histogram's returning atomic is already the image's index inside its class: it
// stays beside the image (16 bits: below kPrepassCap), the classes' first positions come from
// the same scans as above, and the image goes to c0[class] + index.  hist: kBlock + 1 words.
template <int PER>
__device__ __forceinline__ void chain_zclasses_resident(const float* __restrict__ src, int nz,
                                                        int v, int nb, const ClassPlan& cp,
                                                        uint32_t* hist, uint32_t* wsum,
                                                        uint32_t* __restrict__ work) {
  static_assert(PER % 2 == 0 && (int64_t)kBlock * PER <= kPrepassCap, "chainclass.h's capacity");
  const int t = threadIdx.x;
  if (t == 0) hist[kBlock] = 0;
  hist[t] = 0;
  __syncthreads();
  float f[PER];
  uint32_t at[PER / 2];  // the indices of images 2 j and 2 j + 1
  // image u * kBlock + t exists: whole rows by a scalar test, one lane mask for the last row
  const int full = nz / kBlock;
  const bool tail = t < nz - full * kBlock;
  auto has = [&](int u) { return u < full || (u == full && tail); };
#pragma unroll
  for (int u = 0; u < PER; ++u)  // (u32 offsets from the uniform base: one register each)
    f[u] = src[min((uint32_t)(u * kBlock + t), (uint32_t)(nz - 1))];
  // (batches of kB images behind scheduling barriers: left to itself the compiler keeps every
  // image's class, index and address live at once, 242 VGPRs)
  constexpr int kB = 8;
  static_assert(PER % kB == 0 && kB % 2 == 0, "whole batches, whole index pairs");
#pragma unroll
  for (int u0 = 0; u0 < PER; u0 += kB) {
#pragma unroll
    for (int u = u0; u < u0 + kB; ++u) {
      // (no branch: a slot past the bag's end counts into the spare word behind the classes)
      const uint32_t cls = class_of(bits_z_image(f[u]), nb, cp.k);  // (f[u]: a clamped load)
      const uint32_t idx = atomicAdd(&hist[has(u) ? cls : kBlock], 1u);  // < kBlock * PER
      at[u / 2] = u % 2 ? at[u / 2] | (idx << 16) : idx;
      // (the pair is made here, not where the scatter reads it: one register per two images)
      if (u % 2) asm volatile("" : "+v"(at[u / 2]));
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  class_block_tables<true>(hist, wsum, v, cp, work);  // hist: now c0 of every class
  uint32_t* __restrict__ zs = work + (cp.off_zs + (int64_t)v * cp.zs_stride);
  const ClassStoreForm enc = class_store_form(cp);
#pragma unroll
  for (int u0 = 0; u0 < PER; u0 += kB) {
#pragma unroll
    for (int u = u0; u < u0 + kB; ++u) {
      float fu = f[u];  // (opaque: the class is computed again, not kept from the histogram)
      asm volatile("" : "+v"(fu));
      const uint32_t zc = bits_z_image(fu);
      const uint32_t idx = u % 2 ? at[u / 2] >> 16 : at[u / 2] & 0xFFFFu;
      if (has(u))
        zs[hist[class_of(zc, nb, cp.k)] + idx] = class_store_word(zc, enc);  // < c0 + n <= nz
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Both pre-passes of the class-run form in one launch (chainclass.h's prepass_grid; DESIGN
// §4.1l).  Blocks [0, n_bags): the z-class role of one bag — in registers where the bag fits
// (block-uniform), the streaming loop for any other size — and the bag's count zeroed, which
// the count kernels behind the launch add to.  The blocks after them: k_chain_planes' waves.
// The roles write disjoint regions and no block waits for another.
template <int NB>
__global__ __launch_bounds__(kBlock) void k_chain_prepass(
    const float* __restrict__ xb, const int64_t* __restrict__ x_off, int64_t x_stride,
    const float* __restrict__ zb, const int64_t* __restrict__ z_off, int64_t z_stride,
    int n_shards, int n_bags, int gx, int gz, int swap, ClassPlan cp,
    uint32_t* __restrict__ work, unsigned long long* __restrict__ out) {
  static_assert(kBlock == kPrepassThreads && kBlock == 1 << kClassMaxBits, "chainclass.h");
  __shared__ uint32_t hist[kBlock + 1], wsum[kBlock / kWave];
  if (blockIdx.x >= (unsigned)n_bags) {
    chain_planes_wave<NB>((int64_t)blockIdx.x - n_bags, xb, x_off, x_stride, zb, z_off, z_stride,
                          n_shards, n_bags, gx, gz, swap, work);
    return;
  }
  const int v = blockIdx.x;
  const int c = v / n_shards, s = v - c * n_shards;
  const int64_t nz = z_off[s + 1] - z_off[s];
  const float* __restrict__ src = zb + ((int64_t)c * z_stride + z_off[s]);
  if (threadIdx.x == 0) out[v] = 0ull;
  const int per = prepass_per_thread(nz);
  if (per == kPrepassPerSmall)
    chain_zclasses_resident<kPrepassPerSmall>(src, (int)nz, v, NB, cp, hist, wsum, work);
  else if (per == kPrepassPer)
    chain_zclasses_resident<kPrepassPer>(src, (int)nz, v, NB, cp, hist, wsum, work);
  else
    chain_zclasses_stream(src, nz, v, NB, cp, hist, wsum, work);
}

// The count on class runs: per bag p.tiles_x x class_spans(cp.cap, cp.span) class items
// (tile-major: a block's waves read the same planes), an item the cp.span consecutive table
// entries of one span (chainclass.h).  An item whose span starts past the bag's
// count exits at once; an active one reads its runs {z0, len, class} and counts its up to p.R
// x groups against exactly those len images each.  Under the digit loop an item keeps what
// depends on its x tile alone across the span; the masked-plane loop runs at cp.span = 1.
// The plan's swapped items run in a launch of their own (k_count_chain_swapped):
// their full-NB loop holds R * NB planes per lane, and without it this kernel allocates 89
// VGPRs at NB = 20, k = 8 (at most 94 at NB <= 20) — 5 waves per SIMD instead of 4 at the 105
// of the joint kernel.  Where the low field fits the digit tables (form 3, DESIGN
// §4.1i, §4.1j) the runs' images are digit-ready and the item runs bits_count_span_digits: 122
// VGPRs at NL = 12 (4 waves), 96 at narrower low fields (5 waves), as before the spans.
//  DW is the digit loop's planes per digit.  DW = kClassWideBits exists for
// NB - K = 12 alone — (16, 4), (18, 6), (20, 8) — and runs bits_count_span_wide on images
// pre-pass 2 wrote with class_wide_encode (cp.dbits): three 4-plane digits, 8 VALU + 5 SALU per
// z at two groups instead of 10 + 7, 124 - 126 VGPRs, no scratch, 4 waves.  The launcher picks
// it under tw_count_chain_class_digits' setting (automatic: wherever it fits); every other
// instantiation is the four-digit or masked-plane kernel it was, register for register.
template <int NB, int K, int DW = kClassDigitBits>
__global__ __launch_bounds__(kBlock) void k_count_chain_classes(
    const int64_t* __restrict__ x_off, const int64_t* __restrict__ z_off, int n_shards,
    int n_bags, PlanesPlan p, ClassPlan cp, const uint32_t* __restrict__ work,
    unsigned long long* __restrict__ out) {
  const int lb = xcd_block(blockIdx.x, gridDim.x);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int item = lb * (kBlock / kWave) + wid;
  const int spans = class_spans(cp.cap, cp.span);
  const int n_class = p.tiles_x * spans;
  const int v = item / n_class;
  bool active = v < n_bags;
  unsigned long long tot = 0;
  if (active) {
    const int s = v % n_shards;
    const int64_t nx = x_off[s + 1] - x_off[s], nz = z_off[s + 1] - z_off[s];
    const ClassSpanItem si = class_span_item(item - v * n_class, spans);
    const PlanesBag bag = planes_bag(nx, nz, p.swap != 0);
    const int lim = bag.xgroups < p.gx ? bag.xgroups : p.gx;
    const int g0 = si.tx * p.R;
    const int ng = __builtin_amdgcn_readfirstlane(lim - g0 < p.R ? lim - g0 : p.R);
    // (the bag's count is <= cp.cap: no entry past the bag's table is read)
    const ClassSpan sp = class_span_entries(
        si.q, cp.span, __builtin_amdgcn_readfirstlane((int)work[cp.off_cnt + v]));
    active = ng > 0 && sp.e0 < sp.e1;
    if (active) {
      const uint32_t* __restrict__ tab =
          work + bits_uniform(cp.off_tab + ((int64_t)v * cp.cap + sp.e0) * 2);
      const uint32_t* __restrict__ pw =
          work + bits_uniform(planes_word(NB, (int64_t)v * p.gx + g0, 0, 0));
      const uint32_t* __restrict__ zbag =
          work + bits_uniform(cp.off_zs + (int64_t)v * cp.zs_stride);
      unsigned long long t;
      if constexpr (DW == kClassWideBits) {  // the wide-digit loop: NB - K = 12, R <= 2
        static_assert(class_wide_fit(NB - K), "the wide digits take the 12-plane low field");
        t = bits_count_span_wide_of<NB, K, kClassDigitsMaxR>(pw, zbag, tab, sp.e1 - sp.e0, lane,
                                                             ng);
      } else if constexpr (class_loop_form(NB, K) == 3) {  // the digit loop: the launcher planned
        t = bits_count_span_digits_of<NB, K, kClassDigitsMaxR>(  // R <= kClassDigitsMaxR
            pw, zbag, tab, sp.e1 - sp.e0, lane, ng);
      } else {  // the masked-plane loop: one run per item (the launcher planned cp.span = 1)
        const ClassRun r = class_entry((uint32_t)__builtin_amdgcn_readfirstlane((int)tab[0]),
                                       (uint32_t)__builtin_amdgcn_readfirstlane((int)tab[1]));
        const uint32_t* __restrict__ zs = zbag + r.z0;
        const int len = (int)r.len;  // >= 1: only non-empty classes have runs
        if (ng == 4)
          t = bits_count_class<NB, K, 4>(pw, zs, len, r.cls, lane);
        else if (ng == 3)
          t = bits_count_class<NB, K, 3>(pw, zs, len, r.cls, lane);
        else if (ng == 2)
          t = bits_count_class<NB, K, 2>(pw, zs, len, r.cls, lane);
        else
          t = bits_count_class<NB, K, 1>(pw, zs, len, r.cls, lane);
      }
      tot = wave_sum_u64(t);
    }
  }
  count_chain_epilogue(tot, active, v, wid, lane, out);
}

// The count on class runs with the low field's carries tabulated in LDS (chainclass.h's
// class_lds_*): one block of kClassLdsThreads threads — 16 waves, one block per
// CU at 4 waves per SIMD — per (bag, x tile of two groups), grid = bags x p.tiles_x in
// xcd_block order.  The block tabulates the tile's 256 low-field carries per lane and group
// (128 KiB), then its waves draw the bag's runs from an LDS counter and count them with
// bits_count_runs_lds: 5 VALU per z instead of the wide loop's 8.  All waves belong to one bag:
// a block sum and one u64 atomic (the pre-pass zeroed the counts).  Exists for NB - K = 12;
// the launcher plans it with p.R = 2, no swapped items and images written by class_lds_encode
// (cp.dbits = kClassLdsBits).
constexpr int kClassLdsThreads = 1024;
constexpr int kClassLdsWaves = kClassLdsThreads / kWave;
static_assert(kClassLdsWaves * 16 == kClassLdsEntries, "wave w writes the 16 entries d1 = w");
static_assert(kClassLdsTableBytes + kClassLdsWaves * 8 + 8 <= 160 * 1024, "the CU's LDS");
template <int NB, int K>
__global__ __launch_bounds__(kClassLdsThreads) void k_count_chain_classes_lds(
    const int64_t* __restrict__ x_off, const int64_t* __restrict__ z_off, int n_shards,
    int n_bags, PlanesPlan p, ClassPlan cp, const uint32_t* __restrict__ work,
    unsigned long long* __restrict__ out) {
  __shared__ uint2 table[kClassLdsEntries * kWave];
  __shared__ unsigned long long part[kClassLdsWaves];
  __shared__ uint32_t next;
  static_assert(sizeof(table) == kClassLdsTableBytes, "chainclass.h's layout");
  const int lb = xcd_block(blockIdx.x, gridDim.x);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int v = lb / p.tiles_x, tx = lb - v * p.tiles_x;  // v < n_bags: the grid is exact
  const int s = v % n_shards;
  const int64_t nx = x_off[s + 1] - x_off[s], nz = z_off[s + 1] - z_off[s];
  const PlanesBag bag = planes_bag(nx, nz, p.swap != 0);
  const int lim = bag.xgroups < p.gx ? bag.xgroups : p.gx;
  const int g0 = tx * p.R;
  const int ng = __builtin_amdgcn_readfirstlane(lim - g0 < p.R ? lim - g0 : p.R);
  // (the bag's count is <= cp.cap: no entry past the bag's table is read)
  const int cnt = __builtin_amdgcn_readfirstlane((int)work[cp.off_cnt + v]);
  if (v >= n_bags || ng <= 0 || cnt <= 0) return;  // block-uniform, before the barriers
  const uint32_t* __restrict__ tab = work + bits_uniform(cp.off_tab + (int64_t)v * cp.cap * 2);
  const uint32_t* __restrict__ pw =
      work + bits_uniform(planes_word(NB, (int64_t)v * p.gx + g0, 0, 0));
  const uint32_t* __restrict__ zbag = work + bits_uniform(cp.off_zs + (int64_t)v * cp.zs_stride);
  if (threadIdx.x == 0) next = 0;
  class_lds_build<NB>(table, pw, wid, lane, ng);
  __syncthreads();
  const uint32_t lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint2*)table;
  const unsigned long long t =
      wave_sum_u64(bits_count_runs_lds<NB, K>(lds, pw, zbag, tab, cnt, &next, lane, ng));
  if (lane == 0) part[wid] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kClassLdsWaves; ++w) sum += part[w];
    if (sum) atomicAdd(out + v, sum);
  }
}

// The swapped items of a plan whose plane items went through class runs: per bag
// p.tiles_s x p.schunks items, the x remainder as scalars against the bag's z planes, the
// full-NB loop and the decode of k_count_chain_planes unchanged.  Adds to the same counts.
template <int NB>
__global__ __launch_bounds__(kBlock) void k_count_chain_swapped(
    const float* __restrict__ xb, const int64_t* __restrict__ x_off, int64_t x_stride,
    const int64_t* __restrict__ z_off, int n_shards, int n_bags, PlanesPlan p,
    const uint32_t* __restrict__ work, unsigned long long* __restrict__ out) {
  const int lb = xcd_block(blockIdx.x, gridDim.x);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int item = lb * (kBlock / kWave) + wid;
  const int n_swapped = p.tiles_s * p.schunks;  // > 0: not launched otherwise
  const int v = item / n_swapped;
  bool active = v < n_bags;
  unsigned long long tot = 0;
  if (active) {
    const int c = v / n_shards, s = v - c * n_shards;
    const int64_t nx = x_off[s + 1] - x_off[s], nz = z_off[s + 1] - z_off[s];
    const PlanesItem it =
        planes_item(p, nx, nz, p.tiles_x * p.zchunks + (item - v * n_swapped));
    active = it.active;  // (swapped: past the plan's plane items)
    if (active) {
      const int64_t group = (int64_t)n_bags * p.gx + (int64_t)v * p.gz + it.g0;
      const uint32_t* __restrict__ pw = work + bits_uniform(planes_word(NB, group, 0, 0));
      const float* __restrict__ sf = xb + bits_uniform((int64_t)c * x_stride + x_off[s] + it.s0);
      const int ns = __builtin_amdgcn_readfirstlane((int)(it.s1 - it.s0));
      const int ng = __builtin_amdgcn_readfirstlane(it.ng);
      unsigned long long t;
      if (ng == 4)
        t = bits_count_planes<NB, 4>(pw, sf, ns, true, lane);
      else if (ng == 3)
        t = bits_count_planes<NB, 3>(pw, sf, ns, true, lane);
      else if (ng == 2)
        t = bits_count_planes<NB, 2>(pw, sf, ns, true, lane);
      else
        t = bits_count_planes<NB, 1>(pw, sf, ns, true, lane);
      tot = wave_sum_u64(t);
    }
  }
  count_chain_epilogue(tot, active, v, wid, lane, out);
}

// ------------------------------------------- the call's final arrays over ranks: one exchange
// (round 6) Every rank walked its own elements to their final global positions (the chains'
// state after the call's last emission); each element's score and rank-image record travel
// ONCE to the rank that holds its final position — 24-B records {score, record, local
// position (z: n + position)} in G fixed-capacity buckets (k_exchange_pack_fixed's layout: a
// header record with the count, then up to cap records) through one equal-split all-to-all —
// and land at their positions: the rank's final arrays and the carried records of the next
// call.  This replaces the all-gathers of both samples and of both record arrays (G x the
// rank's bytes received per call) and the inverse-chain gathers from them.
constexpr int kFinMaxG = 1024, kFinPer = 8, kFinChunk = kBlock * kFinPer;

__global__ __launch_bounds__(kBlock) void k_chain_final_pack(
    const uint64_t* __restrict__ xv, const uint64_t* __restrict__ xr,
    const uint32_t* __restrict__ xpos, int64_t n, const uint64_t* __restrict__ zv,
    const uint64_t* __restrict__ zr, const uint32_t* __restrict__ zpos, int64_t m, int G,
    FastDiv dn, FastDiv dm, int64_t cap, unsigned long long* __restrict__ cursor,
    uint64_t* __restrict__ send, int* __restrict__ flag) {
  __shared__ unsigned lcnt[kFinMaxG];
  __shared__ int64_t lbase[kFinMaxG];
  const int64_t tot = n + m, bsz = cap + 1;
  for (int64_t c0 = (int64_t)blockIdx.x * kFinChunk; c0 < tot;
       c0 += (int64_t)gridDim.x * kFinChunk) {
    for (int i = threadIdx.x; i < G; i += kBlock) lcnt[i] = 0;
    __syncthreads();
    int dst[kFinPer];
    unsigned slot[kFinPer];
    int64_t pos[kFinPer];
#pragma unroll
    for (int k = 0; k < kFinPer; ++k) {
      const int64_t e = c0 + k * kBlock + threadIdx.x;
      dst[k] = -1;
      slot[k] = 0;
      pos[k] = 0;
      if (e < n) {
        const uint64_t p = xpos[e];
        const uint64_t g = fast_div(p, dn);
        dst[k] = (int)g;
        pos[k] = (int64_t)(p - g * (uint64_t)n);
      } else if (e < tot) {
        const uint64_t p = zpos[e - n];
        const uint64_t g = fast_div(p, dm);
        dst[k] = (int)g;
        pos[k] = (int64_t)(p - g * (uint64_t)m) + n;
      }
      if (dst[k] >= G) {  // a position past the sample (never, for a valid chain state)
        *flag = 1;
        dst[k] = -1;
      }
      if (dst[k] >= 0) slot[k] = atomicAdd(&lcnt[dst[k]], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < G; i += kBlock)
      if (lcnt[i]) lbase[i] = (int64_t)atomicAdd(cursor + i, (unsigned long long)lcnt[i]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kFinPer; ++k) {
      if (dst[k] >= 0) {
        const int64_t o = lbase[dst[k]] + slot[k];
        if (o < cap) {
          const int64_t e = c0 + k * kBlock + threadIdx.x;
          uint64_t* r = send + 3 * ((int64_t)dst[k] * bsz + 1 + o);
          r[0] = e < n ? xv[e] : zv[e - n];
          r[1] = e < n ? xr[e] : zr[e - n];
          r[2] = (uint64_t)pos[k];
        } else {
          *flag = 1;  // dropped, never written out of place; the host raises
        }
      }
    }
    __syncthreads();
  }
}

// the bucket headers from the cursors (then zeroed for the next call)
__global__ void k_chain_final_seal(int G, int64_t cap, unsigned long long* __restrict__ cursor,
                                   uint64_t* __restrict__ send, int* __restrict__ flag) {
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    const unsigned long long c = cursor[g];
    uint64_t* h = send + 3 * ((int64_t)g * (cap + 1));
    h[0] = c;
    h[1] = 0;
    h[2] = 0;
    cursor[g] = 0;
    if (c > (unsigned long long)cap) *flag = 1;
  }
}

// receive side: every record of every bucket at its position of the final arrays
__global__ __launch_bounds__(kBlock) void k_chain_final_scatter(
    const uint64_t* __restrict__ recv, int G, int64_t cap, int64_t n, int64_t m,
    uint64_t* __restrict__ xo, uint64_t* __restrict__ xro, uint64_t* __restrict__ zo,
    uint64_t* __restrict__ zro, int* __restrict__ flag) {
  const int64_t bsz = cap + 1, tot = (int64_t)G * cap;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < tot;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t g = i / cap, r = i - g * cap;
    const uint64_t c = recv[3 * (g * bsz)];
    if (c > (uint64_t)cap && r == 0) *flag = 1;
    if ((uint64_t)r < c && r < cap) {
      const uint64_t* q = recv + 3 * (g * bsz + 1 + r);
      const uint64_t p = q[2];
      if (p < (uint64_t)n) {
        xo[p] = q[0];
        xro[p] = q[1];
      } else if (p < (uint64_t)(n + m)) {
        zo[p - n] = q[0];
        zro[p - n] = q[1];
      } else {
        *flag = 1;
      }
    }
  }
}

// ----------------------------------------------------------------------------- final order
// One process: the scores at the chains' last positions, out[pos[e]] = in[e] (8-B values).
__global__ __launch_bounds__(kBlock) void k_chain_scatter(const uint64_t* __restrict__ xin,
                                                          const uint32_t* __restrict__ xpos,
                                                          int64_t nx,
                                                          const uint64_t* __restrict__ zin,
                                                          const uint32_t* __restrict__ zpos,
                                                          int64_t nz, uint64_t* __restrict__ xout,
                                                          uint64_t* __restrict__ zout) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nx + nz;
       e += (int64_t)gridDim.x * kBlock) {
    if (e < nx)
      xout[xpos[e]] = xin[e];
    else
      zout[zpos[e - nx]] = zin[e - nx];
  }
}

// ----------------------------------------------------------------------------- plan
struct ChainPlan {  // of the packed kernel
  int R, tiles_x, zchunks;
  int64_t z_chunk, blocks;
};
static int g_chain_R = 0;  // tuning hooks (tw_count_chain_set_plan); 0 = automatic
static int64_t g_chain_zchunk = 0;
static int g_planes_swap = 1;  // (tw_count_chain_set_swap: 0 never, 1 automatic, 2 always)
static int g_class_bits = -1;  // (tw_count_chain_set_class_bits: -1 automatic, 0 off, 1..8)
static int g_class_span = 0;   // (tw_count_chain_class_span: 0 automatic, >= 1 entries per item)
static int g_class_digits = 0;  // (tw_count_chain_class_digits: 0 automatic, 3 or 4 planes)
static int g_class_lds = 0;     // (tw_count_chain_class_lds: 0 automatic, 1 off, 2 on)
static int g_prepass = 0;  // (tw_count_chain_prepass: 0 automatic, 1 separate launches, 2 fused)
// class bits of a bit-sliced launch: forced (clamped to its planes), or chainclass.h's
// automatic rule
static int chain_class_bits(int64_t max_nz, int64_t bags, int nb) {
  return g_class_bits < 0 ? class_bits_auto(max_nz, bags, nb)
                          : std::min(g_class_bits, std::min(kClassMaxBits, nb - 8));
}

// strict: R in {16, 8} x-images per lane, least padded slots (ties to 16); half: R = 8 {g, h}
// pairs (the same 8 packed registers per lane).  z chunks: as many as give ~150 work items per
// SIMD (kChainItems), each of >= 600 images — long items amortise a wave's x loads and
// epilogue, enough of them keep the tail short.  Round 5 (tools/count_plan_ab.py, profiles/
// r05s49_count_plan_ab.log, interleaved A/B): against round 4's fixed 1024-image chunks the
// headline K = 20 launch 8.54 -> 8.31 ms, K = 32 13.68 -> 13.34, half ties 17.02 -> 16.54,
// every per-rank shape of the strong problem 0.3-2.4 % faster, C2 within 1 %
constexpr int64_t kChainItems = 256 * 4 * 150;
// (C2's single 1e5 x 1e5 bag: 600-image chunks 276.9 us, 512 282.3 us, profiles/
// r05s59_c2_plan.log; the large shapes are indifferent between 512 and 1024)
constexpr int64_t kChainMinZ = 600;
// (Whether a bounded launch runs this kernel or the bit-sliced count: chainplan.h's
// chain_count_sliced.)
static ChainPlan plan_chain(int64_t max_nx, int64_t max_nz, int64_t n_bags, bool half) {
  ChainPlan p{half ? 8 : 16, 1, 1, max_nz, 0};
  int64_t best = -1;
  if (!half) {
    for (int R : {16, 8}) {
      if (g_chain_R && R != g_chain_R) continue;
      const int64_t slots = ceil_div(max_nx, (int64_t)kWave * R) * kWave * R;
      if (best < 0 || slots < best) {
        best = slots;
        p.R = R;
      }
    }
  }
  p.tiles_x = (int)ceil_div(max_nx, (int64_t)kWave * p.R);
  const int64_t base = (int64_t)p.tiles_x * n_bags;
  int64_t zc = g_chain_zchunk;
  if (zc <= 0)
    zc = std::max<int64_t>(
        kChainMinZ, ceil_div(max_nz, std::max<int64_t>(1, ceil_div(kChainItems,
                                                                   std::max<int64_t>(1, base)))));
  zc = std::min<int64_t>(zc, (int64_t)1 << 24);  // f32 lane counters stay exact
  p.z_chunk = ceil_div(std::min<int64_t>(zc, max_nz), 8) * 8;
  p.zchunks = (int)ceil_div(max_nz, p.z_chunk);
  p.blocks = ceil_div((int64_t)p.tiles_x * p.zchunks * n_bags, kBlock / kWave);
  return p;
}

static ChainKeys chain_keys(const uint64_t* kx, const uint64_t* kz, int steps) {
  ChainKeys k{};
  for (int i = 0; i < steps; ++i) {
    k.kx[i] = kx[i];
    k.kz[i] = kz[i];
  }
  return k;
}

}  // namespace tw

using namespace tw;

// Round tables of the emission (tw_chain_set_emit_tables): 0 automatic, 1 off, 2 on wherever a
// table fits (both classes' half_bits <= kEmTabMaxHB)
static int g_emit_tables = 0;

static uint32_t em_half_bits(int64_t N) { return make_feistel(N > 1 ? N : 1, 0).half_bits; }
static bool em_tables_fit(int64_t NX, int64_t NZ) {
  return em_half_bits(NX) <= kEmTabMaxHB && em_half_bits(NZ) <= kEmTabMaxHB;
}
// entries per (step, class) slot: the larger class's table, padded to whole 16-B loads
static uint32_t em_tab_stride(int64_t NX, int64_t NZ) {
  return ((6u << std::max(em_half_bits(NX), em_half_bits(NZ))) + 7u) & ~7u;
}
// the launch plan: elements per thread and steps per round (tw_chain_set_emit or automatic)
// (profiles/r04_chain_parts.log: 2e6 elements, 20 steps: EPR 8 / 1 step per round 257 us,
// 8 / 2 296 us; 250k elements: 2 / 8 57 us, 2 / 1 79 us, 8 / 1 139 us)
// (round 5, profiles/r05s46_emit_sweep_ranks.log: a G = 4 rank's 500k elements, 4 per
// thread and 4 steps per round: 30 against 36 us at K = 4, 92 against 100 at K = 20)
static void em_plan(int64_t elems, int NB, int& epr, int& spr) {
  epr = g_emit_epr ? g_emit_epr : elems >= 1500000 ? 8 : elems >= 400000 ? 4 : 2;
  spr = g_emit_s ? g_emit_s : epr == 8 ? 1 : 16 / epr;
  while (spr > 1 && spr * NB > kEmMaxB) spr >>= 1;
}
// Whether a launch looks its rounds up.  Automatic (tools/emit_tables_ab.py, profiles/
// r15_emit_tables_ab.json): only one process with strict ties (the slim staging),
// 8 elements per thread, one step per round and half_bits <= 10 — 0.85 of the arithmetic
// rounds at 2e6 elements x 20 steps; every other form measured lost (the table's LDS costs the
// full staging a resident block, several steps per round pay two barriers per step) or was
// not measured (half_bits 11 in the slim form: 24 KB, three blocks per CU) and stays off.
static bool em_tables_on(int64_t NX, int64_t NZ, bool full, int epr, int spr) {
  if (g_emit_tables == 1 || !em_tables_fit(NX, NZ)) return false;
  if (g_emit_tables == 2) return true;
  return !full && epr == 8 && spr == 1 && em_half_bits(NX) <= 10 && em_half_bits(NZ) <= 10;
}
// the same for a launch by its arguments (chain_emit_impl and tw_chain_emit_tables_of share it)
static bool em_launch_tables(int64_t n_x, int64_t n_z, int world, bool half, bool xchg,
                             int n_shards) {
  const int NB = xchg ? world : n_shards + 1;
  int epr, spr;
  em_plan(n_x + n_z, NB, epr, spr);
  // (the unstaged form, > 512 buckets, was not swept: automatic leaves it as it was)
  return em_tables_on((int64_t)world * n_x, (int64_t)world * n_z,
                      xchg || half || NB > kEmMaxB, epr, spr);
}

static int chain_emit_impl(const uint64_t* d_x_rec, int64_t n_x, const uint64_t* d_z_rec,
                           int64_t n_z, int32_t half, uint32_t* d_x_pos, uint32_t* d_z_pos,
                           int32_t first, int32_t rank, int32_t world, const uint64_t* keys_x,
                           const uint64_t* keys_z, int32_t steps, int64_t x_shard,
                           int64_t z_shard, int32_t n_shards, void* d_x_bag, void* d_z_bag,
                           uint32_t* d_cursors, uint64_t* d_send, int64_t cap, int32_t* d_flag,
                           bool with_work, void* d_work, int64_t work_bytes, void* stream) {
  TW_ARG_CHECK(n_x >= 0 && n_z >= 0 && world >= 1 && rank >= 0 && rank < world &&
                   steps >= 0 && steps <= kChainMax && n_shards >= 0 && x_shard >= 0 &&
                   z_shard >= 0 && (half == 0 || half == 1) && (first == 0 || first == 1),
               "tw_chain_emit: bad sizes");
  TW_ARG_CHECK((int64_t)world * n_x < (1ll << 32) && (int64_t)world * n_z < (1ll << 32),
               "tw_chain_emit: positions must fit 32 bits");
  // the exchange mode is chosen by the send buffer, not by world > 1: a world-size-1 process
  // group can be forced through the collectives' path (ShardedSample(collectives=True))
  const bool xchg = d_send != nullptr;
  TW_ARG_CHECK((xchg ? world : n_shards + 1) <= kEmMaxBig,
               "tw_chain_emit: at most %d buckets (shards + 1, or ranks)", kEmMaxBig);
  TW_ARG_CHECK(steps == 0 || (keys_x != nullptr && keys_z != nullptr),
               "tw_chain_emit: keys missing");
  if (steps == 0 || n_x + n_z == 0) return TW_OK;
  TW_ARG_CHECK(d_x_pos != nullptr && d_z_pos != nullptr, "tw_chain_emit: position state missing");
  if (xchg)
    TW_ARG_CHECK(d_flag != nullptr && cap >= 1 && world <= 1024,
                 "tw_chain_emit: flag and cap >= 1 needed with a send buffer");
  else
    TW_ARG_CHECK(world == 1 && d_x_bag != nullptr && d_z_bag != nullptr && d_cursors != nullptr,
                 "tw_chain_emit: over ranks a send buffer, in one process bags and cursors");
  hipStream_t st = (hipStream_t)stream;
  ChainEmit em{};
  em.xr = d_x_rec;
  em.zr = d_z_rec;
  em.nx = n_x;
  em.nz = n_z;
  em.xpos = d_x_pos;
  em.zpos = d_z_pos;
  em.first = first;
  em.xbase = (int64_t)rank * n_x;
  em.zbase = (int64_t)rank * n_z;
  em.NX = (int64_t)world * n_x;
  em.NZ = (int64_t)world * n_z;
  em.steps = steps;
  em.half = half;
  em.kx = x_shard;
  em.kz = z_shard;
  em.dkx = make_fastdiv(x_shard > 0 ? x_shard : 1);
  em.dkz = make_fastdiv(z_shard > 0 ? z_shard : 1);
  em.nsh = n_shards;
  em.xbag = d_x_bag;
  em.zbag = (uint32_t*)d_z_bag;
  em.cur = d_cursors;
  em.xchg = xchg ? 1 : 0;
  em.world = world;
  em.W = half ? 2 : 1;
  em.dnx = make_fastdiv(n_x > 0 ? n_x : 1);
  em.dnz = make_fastdiv(n_z > 0 ? n_z : 1);
  em.send = d_send;
  em.cap = cap;
  em.flag = d_flag;
  // the workspace contract holds under every setting of the hook: a caller of the _ws entry
  // provides tw_chain_emit_work_bytes, checked before anything is launched
  const int NB = xchg ? world : n_shards + 1;
  const bool full = xchg || half;
  int epr, spr;
  em_plan(n_x + n_z, NB, epr, spr);
  const bool tabs = with_work && em_launch_tables(n_x, n_z, world, half != 0, xchg, n_shards);
  if (with_work) {
    const int64_t need = em_tables_fit(em.NX, em.NZ)
                             ? (int64_t)steps * 2 * em_tab_stride(em.NX, em.NZ) * 2 : 0;
    TW_ARG_CHECK(work_bytes >= need && (need == 0 || d_work != nullptr) &&
                     ((uintptr_t)d_work & 15) == 0,
                 "tw_chain_emit_ws: workspace of %lld bytes, 16-B aligned, needed",
                 (long long)need);
  }
  em.hbx = em_half_bits(em.NX);
  em.hbz = em_half_bits(em.NZ);
  em.tab_stride = tabs ? em_tab_stride(em.NX, em.NZ) : 0;
  em.tab = tabs ? (const uint16_t*)d_work : nullptr;
  {
    // the zeroing and the chunk's tables in one launch
    ChainRounds rk{};
    if (tabs)
      for (int c = 0; c < steps; ++c) {
        const Feistel fx = make_feistel(em.NX > 1 ? em.NX : 1, keys_x[c]);
        const Feistel fz = make_feistel(em.NZ > 1 ? em.NZ : 1, keys_z[c]);
        for (int i = 0; i < 6; ++i) {
          rk.k[c][0][i] = fx.k[i];
          rk.k[c][1][i] = fz.k[i];
        }
      }
    const int64_t words = xchg ? (int64_t)world * steps : (int64_t)steps * 2 * (n_shards + 1);
    const unsigned gy = tabs ? 2u * steps : 1u;
    const int64_t per = std::max<int64_t>(ceil_div(words, (int64_t)gy),
                                          tabs ? (int64_t)em.tab_stride : 1);
    const unsigned gx = (unsigned)std::min<int64_t>(64, ceil_div(per, kBlock));
    hipLaunchKernelGGL(k_chain_emit_prep, dim3(gx, gy), dim3(kBlock), 0, st,
                       xchg ? (void*)d_send : (void*)d_cursors, words,
                       xchg ? (cap + 1) * em.W : (int64_t)0, rk, (uint16_t*)em.tab,
                       em.tab_stride, em.hbx, em.hbz);
    TW_LAUNCH_CHECK();
  }
  const ChainKeys k = chain_keys(keys_x, keys_z, steps);
  const size_t dyn = tabs ? (size_t)em.tab_stride * sizeof(uint16_t) : 0;
  auto launch = [&](auto epr_c, auto spr_c, auto staged) {
    constexpr int EPR = decltype(epr_c)::value, S = decltype(spr_c)::value;
    constexpr bool ST = decltype(staged)::value;
    em.bx = (int)ceil_div(n_x, (int64_t)kEmThreads * EPR);
    const int64_t blocks = em.bx + ceil_div(n_z, (int64_t)kEmThreads * EPR);
    if (full)
      hipLaunchKernelGGL((k_chain_emit<EPR, S, ST, true>), dim3((unsigned)blocks),
                         dim3(kEmThreads), dyn, st, em, k);
    else
      hipLaunchKernelGGL((k_chain_emit<EPR, S, ST, false>), dim3((unsigned)blocks),
                         dim3(kEmThreads), dyn, st, em, k);
  };
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I4 = std::integral_constant<int, 4>;
  using I8 = std::integral_constant<int, 8>;
  using T_ = std::true_type;
  using F_ = std::false_type;
  if (NB > kEmMaxB) {
    if (epr == 8) launch(I8(), I1(), F_());
    else if (epr == 4) launch(I4(), I1(), F_());
    else launch(I2(), I1(), F_());
  } else if (epr == 8) {
    if (spr >= 2) launch(I8(), I2(), T_());
    else launch(I8(), I1(), T_());
  } else if (epr == 4) {
    if (spr >= 4) launch(I4(), I4(), T_());
    else launch(I4(), I1(), T_());
  } else {
    if (spr >= 8) launch(I2(), I8(), T_());
    else launch(I2(), I1(), T_());
  }
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int tw_chain_emit(const uint64_t* d_x_rec, int64_t n_x, const uint64_t* d_z_rec,
                             int64_t n_z, int32_t half, uint32_t* d_x_pos, uint32_t* d_z_pos,
                             int32_t first, int32_t rank, int32_t world, const uint64_t* keys_x,
                             const uint64_t* keys_z, int32_t steps, int64_t x_shard,
                             int64_t z_shard, int32_t n_shards, void* d_x_bag, void* d_z_bag,
                             uint32_t* d_cursors, uint64_t* d_send, int64_t cap,
                             int32_t* d_flag, void* stream) {
  return chain_emit_impl(d_x_rec, n_x, d_z_rec, n_z, half, d_x_pos, d_z_pos, first, rank, world,
                         keys_x, keys_z, steps, x_shard, z_shard, n_shards, d_x_bag, d_z_bag,
                         d_cursors, d_send, cap, d_flag, false, nullptr, 0, stream);
}

// tw_chain_emit with a workspace for the chunk's round tables (the caller's memory, as the
// planes workspace: written and read inside this one call on this one stream)
extern "C" int tw_chain_emit_ws(const uint64_t* d_x_rec, int64_t n_x, const uint64_t* d_z_rec,
                                int64_t n_z, int32_t half, uint32_t* d_x_pos, uint32_t* d_z_pos,
                                int32_t first, int32_t rank, int32_t world,
                                const uint64_t* keys_x, const uint64_t* keys_z, int32_t steps,
                                int64_t x_shard, int64_t z_shard, int32_t n_shards,
                                void* d_x_bag, void* d_z_bag, uint32_t* d_cursors,
                                uint64_t* d_send, int64_t cap, int32_t* d_flag, void* d_work,
                                int64_t work_bytes, void* stream) {
  return chain_emit_impl(d_x_rec, n_x, d_z_rec, n_z, half, d_x_pos, d_z_pos, first, rank, world,
                         keys_x, keys_z, steps, x_shard, z_shard, n_shards, d_x_bag, d_z_bag,
                         d_cursors, d_send, cap, d_flag, true, d_work, work_bytes, stream);
}

// bytes of tw_chain_emit_ws's workspace for `steps` steps over global sizes (NX, NZ); 0 where
// no table fits (the launch runs the arithmetic rounds)
extern "C" int64_t tw_chain_emit_work_bytes(int32_t steps, int64_t NX, int64_t NZ) {
  if (steps <= 0 || NX < 0 || NZ < 0 || !em_tables_fit(NX, NZ)) return 0;
  return (int64_t)steps * 2 * em_tab_stride(NX, NZ) * (int64_t)sizeof(uint16_t);
}

extern "C" int32_t tw_chain_set_emit_tables(int32_t mode) {
  const int32_t before = g_emit_tables;
  if (mode == -1) return before;
  TW_ARG_CHECK(mode >= 0 && mode <= 2,
               "tw_chain_set_emit_tables: 0 (automatic), 1 (off), 2 (on where a table fits) or -1 "
               "(report)");
  g_emit_tables = mode;
  return before;
}

// whether the tw_chain_emit_ws launch with these arguments (exchange: a send buffer is given)
// looks its rounds up under the current settings (this hook and tw_chain_set_emit): the
// launch's own decision
extern "C" int32_t tw_chain_emit_tables_of(int64_t n_x, int64_t n_z, int32_t world,
                                           int32_t half, int32_t exchange, int32_t n_shards) {
  if (n_x < 0 || n_z < 0 || world < 1 || n_shards < 0) return 0;
  return em_launch_tables(n_x, n_z, world, half != 0, exchange != 0, n_shards) ? 1 : 0;
}

extern "C" int tw_chain_set_emit(int32_t epr, int32_t steps_per_round) {
  TW_ARG_CHECK(epr == 0 || epr == 2 || epr == 4 || epr == 8,
               "tw_chain_set_emit: elements per thread 0, 2, 4 or 8");
  TW_ARG_CHECK(steps_per_round == 0 || steps_per_round == 1 || steps_per_round * epr == 16,
               "tw_chain_set_emit: steps per round 0, 1 or 16 / elements per thread");
  g_emit_epr = epr;
  g_emit_s = steps_per_round;
  return TW_OK;
}

extern "C" int tw_chain_unpack(const uint64_t* d_recv, int32_t world, int32_t steps, int64_t cap,
                               int32_t half, int64_t n_x, int64_t n_z, int64_t x_shard,
                               int64_t z_shard, int32_t n_shards, void* d_x_bag, void* d_z_bag,
                               uint32_t* d_cursors, int32_t* d_flag, void* stream) {
  TW_ARG_CHECK(world >= 1 && steps >= 0 && steps <= kChainMax && cap >= 1 && n_x >= 0 &&
                   n_z >= 0 && (half == 0 || half == 1) && (int64_t)world * steps < 65536 &&
                   x_shard >= 0 && z_shard >= 0 && n_shards >= 0 && n_shards < kEmMaxBig,
               "tw_chain_unpack: bad sizes");
  if (steps == 0 || n_x + n_z == 0) return TW_OK;
  TW_ARG_CHECK(d_cursors != nullptr && d_flag != nullptr, "tw_chain_unpack: cursors and flag");
  hipStream_t st = (hipStream_t)stream;
  const int NB = 2 * (n_shards + 1);
  TW_HIP_CHECK(tw_zero_async(d_cursors, 0, sizeof(uint32_t) * (size_t)NB * steps, st));
  const int parts = (int)std::max<int64_t>(
      1, std::min<int64_t>(ceil_div(cap, (int64_t)kBlock * kUnpackPer), 64));
  hipLaunchKernelGGL(k_chain_unpack, dim3((unsigned)(parts * world * steps)), dim3(kBlock),
                     sizeof(unsigned) * 2 * (size_t)NB, st, d_recv, (int)world, (int)steps, parts,
                     cap, half ? 2 : 1, (int)half, n_x, n_z, x_shard, z_shard, (int)n_shards,
                     d_x_bag, (uint32_t*)d_z_bag, (unsigned*)d_cursors, d_flag);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

// Receiver side at exact positions (the incomplete statistic over ranks, tw_chain_unpack_exact):
// a device-RNG draw addresses a POSITION of the step's permuted arrays, so every record {image,
// local position} lands at bag[c][position] — the step's permuted image arrays themselves, which
// tw_count_pairs_chain_rng reads.  Strict images only (one 8-B record word).
__global__ __launch_bounds__(kBlock) void k_chain_unpack_exact(
    const uint64_t* __restrict__ recv, int world, int steps, int parts, int64_t cap, int64_t nx,
    int64_t nz, uint32_t* __restrict__ xbag, uint32_t* __restrict__ zbag, int* __restrict__ flag) {
  const int lb = xcd_block(blockIdx.x, gridDim.x);
  const int c = lb / (world * parts);
  const int rem = lb - c * world * parts;
  const int g = rem / parts, part = rem - g * parts;
  const uint64_t* b = recv + ((int64_t)g * steps + c) * (cap + 1);
  const int64_t cnt0 = (int64_t)(uint32_t)b[0];
  if (cnt0 > cap && part == 0 && threadIdx.x == 0) *flag = 1;
  const int64_t cnt = cnt0 < cap ? cnt0 : cap;
  for (int64_t i = (int64_t)part * kBlock + threadIdx.x; i < cnt; i += (int64_t)parts * kBlock) {
    const uint64_t r = __builtin_nontemporal_load(b + 1 + i);
    const int64_t p = (int64_t)(r >> 32);
    const uint32_t v = (uint32_t)r;
    if (p < nx)
      xbag[(int64_t)c * nx + p] = v;
    else if (p < nx + nz)
      zbag[(int64_t)c * nz + (p - nx)] = v;
  }
}

extern "C" int tw_chain_unpack_exact(const uint64_t* d_recv, int32_t world, int32_t steps,
                                     int64_t cap, int64_t n_x, int64_t n_z, void* d_x_bag,
                                     void* d_z_bag, int32_t* d_flag, void* stream) {
  TW_ARG_CHECK(world >= 1 && steps >= 0 && steps <= kChainMax && cap >= 1 && n_x >= 0 &&
                   n_z >= 0 && (int64_t)world * steps < 65536 && n_x + n_z < (1ll << 32),
               "tw_chain_unpack_exact: bad sizes");
  if (steps == 0 || n_x + n_z == 0) return TW_OK;
  TW_ARG_CHECK(d_recv && d_x_bag && d_z_bag && d_flag, "tw_chain_unpack_exact: buffers");
  const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(cap, (int64_t)kBlock * 4), 64));
  hipLaunchKernelGGL(k_chain_unpack_exact, dim3((unsigned)(parts * world * steps)), dim3(kBlock),
                     0, (hipStream_t)stream, d_recv, (int)world, (int)steps, parts, cap, n_x, n_z,
                     (uint32_t*)d_x_bag, (uint32_t*)d_z_bag, d_flag);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

// The call's final arrays over ranks by one exchange (k_chain_final_pack / _seal / _scatter):
// tw_chain_final_pack packs this rank's walked elements (scores d_x / d_z, records d_x_rec /
// d_z_rec, final global positions d_x_pos / d_z_pos, each rank n_x / n_z of them) into world
// buckets of 1 + cap 24-B records (d_send: world * (cap + 1) * 3 u64; d_cursor: world u64,
// zero on entry and left zero); after an equal-split all-to-all, tw_chain_final_scatter writes
// every received record into d_x_out / d_x_rec_out / d_z_out / d_z_rec_out at its position.
extern "C" int tw_chain_final_pack(const void* d_x, const uint64_t* d_x_rec,
                                   const uint32_t* d_x_pos, int64_t n_x, const void* d_z,
                                   const uint64_t* d_z_rec, const uint32_t* d_z_pos, int64_t n_z,
                                   int32_t world, int64_t cap, uint64_t* d_cursor, void* d_send,
                                   int32_t* d_flag, void* stream) {
  TW_ARG_CHECK(world >= 1 && world <= kFinMaxG && n_x >= 1 && n_z >= 1 && cap >= 1 &&
                   (int64_t)world * n_x < (1ll << 32) && (int64_t)world * n_z < (1ll << 32),
               "tw_chain_final_pack: bad sizes");
  TW_ARG_CHECK(d_x && d_x_rec && d_x_pos && d_z && d_z_rec && d_z_pos && d_cursor && d_send &&
                   d_flag,
               "tw_chain_final_pack: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (int)std::min<int64_t>(2048, ceil_div(n_x + n_z, (int64_t)kFinChunk));
  hipLaunchKernelGGL(k_chain_final_pack, dim3(blocks), dim3(kBlock), 0, st,
                     (const uint64_t*)d_x, d_x_rec, d_x_pos, n_x, (const uint64_t*)d_z, d_z_rec,
                     d_z_pos, n_z, (int)world, make_fastdiv((uint64_t)n_x),
                     make_fastdiv((uint64_t)n_z), cap, (unsigned long long*)d_cursor,
                     (uint64_t*)d_send, (int*)d_flag);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_chain_final_seal, dim3(1), dim3(256), 0, st, (int)world, cap,
                     (unsigned long long*)d_cursor, (uint64_t*)d_send, (int*)d_flag);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int tw_chain_final_scatter(const void* d_recv, int32_t world, int64_t cap,
                                      int64_t n_x, int64_t n_z, void* d_x_out,
                                      void* d_x_rec_out, void* d_z_out, void* d_z_rec_out,
                                      int32_t* d_flag, void* stream) {
  TW_ARG_CHECK(world >= 1 && world <= kFinMaxG && cap >= 1 && n_x >= 0 && n_z >= 0 && d_recv &&
                   d_x_out && d_x_rec_out && d_z_out && d_z_rec_out && d_flag,
               "tw_chain_final_scatter: bad arguments");
  const int blocks = (int)std::max<int64_t>(
      1, std::min<int64_t>(2048, ceil_div((int64_t)world * cap, kBlock)));
  hipLaunchKernelGGL(k_chain_final_scatter, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint64_t*)d_recv, (int)world, cap, n_x, n_z, (uint64_t*)d_x_out,
                     (uint64_t*)d_x_rec_out, (uint64_t*)d_z_out, (uint64_t*)d_z_rec_out,
                     (int*)d_flag);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

namespace tw {
// the count launch of tw_count_pairs_chain on an output already zeroed
static int count_chain_launch(const void* d_x_bag, const int64_t* d_x_off, int64_t x_stride,
                              const void* d_z_bag, const int64_t* d_z_off, int64_t z_stride,
                              int32_t n_shards, int32_t steps, int64_t max_nx, int64_t max_nz,
                              int32_t half, uint64_t* d_out, hipStream_t st);
// ... and of the _planes entries (d_work: their plane workspace)
static int count_chain_launch_work(const void* d_x_bag, const int64_t* d_x_off, int64_t x_stride,
                                   const void* d_z_bag, const int64_t* d_z_off, int64_t z_stride,
                                   int32_t n_shards, int32_t steps, int64_t max_nx,
                                   int64_t max_nz, int32_t half, int64_t image_bound,
                                   uint64_t* d_out, void* d_work, hipStream_t st,
                                   bool zero_out);
}  // namespace tw

extern "C" int tw_count_pairs_chain(const void* d_x_bag, const int64_t* d_x_off,
                                    int64_t x_stride, const void* d_z_bag,
                                    const int64_t* d_z_off, int64_t z_stride, int32_t n_shards,
                                    int32_t steps, int64_t max_nx, int64_t max_nz, int32_t half,
                                    uint64_t* d_out, void* stream) {
  TW_ARG_CHECK(n_shards >= 0 && steps >= 0 && max_nx >= 0 && max_nz >= 0 && x_stride >= 0 &&
                   z_stride >= 0 && (half == 0 || half == 1),
               "tw_count_pairs_chain: bad sizes");
  TW_ARG_CHECK(max_nz < (1ll << 24), "tw_count_pairs_chain: shards of < 2^24 z-images");
  hipStream_t st = (hipStream_t)stream;
  const int64_t bags = (int64_t)n_shards * steps;
  if (bags == 0) return TW_OK;
  TW_HIP_CHECK(tw_zero_async(d_out, 0, sizeof(uint64_t) * (size_t)bags, st));
  return count_chain_launch(d_x_bag, d_x_off, x_stride, d_z_bag, d_z_off, z_stride, n_shards,
                            steps, max_nx, max_nz, half, d_out, st);
}

// Over ranks, a chunk's receive side in ONE call: the unpack's cursors and the counts zeroed by
// one launch, tw_chain_unpack's kernel, tw_count_pairs_chain's count — three launches
// back to back from the host instead of four from two calls (at G = 8 the chunk's device work
// is short and the host's launch gaps showed, profiles/r06s23_rank_call_timeline_G8_K4.log).
// Arguments: tw_chain_unpack's, then the count's shard offsets, largest shards and out
// [steps][n_shards] (bag strides n_x / n_z).
static __global__ __launch_bounds__(256) void k_zero_two(uint32_t* __restrict__ a, int64_t na,
                                                  uint64_t* __restrict__ b, int64_t nb) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < na + nb;
       i += (int64_t)gridDim.x * 256) {
    if (i < na)
      a[i] = 0u;
    else
      b[i - na] = 0ull;
  }
}

static int chain_unpack_count_impl(const uint64_t* d_recv, int32_t world, int32_t steps,
                                   int64_t cap, int32_t half, int64_t n_x, int64_t n_z,
                                     int64_t x_shard, int64_t z_shard, int32_t n_shards,
                                     void* d_x_bag, void* d_z_bag, uint32_t* d_cursors,
                                     int32_t* d_flag, const int64_t* d_x_off,
                                     const int64_t* d_z_off, int64_t max_nx, int64_t max_nz,
                                     int64_t image_bound, uint64_t* d_out, void* stream,
                                     void* d_work = nullptr) {  // (image_bound: with d_work)
  TW_ARG_CHECK(world >= 1 && steps >= 0 && steps <= kChainMax && cap >= 1 && n_x >= 0 &&
                   n_z >= 0 && (half == 0 || half == 1) && (int64_t)world * steps < 65536 &&
                   x_shard >= 0 && z_shard >= 0 && n_shards >= 0 && n_shards < kEmMaxBig &&
                   max_nx >= 0 && max_nz >= 0,
               "tw_chain_unpack_count: bad sizes");
  TW_ARG_CHECK(max_nz < (1ll << 24), "tw_chain_unpack_count: shards of < 2^24 z-images");
  const int64_t bags = (int64_t)n_shards * steps;
  if (bags == 0) return TW_OK;
  TW_ARG_CHECK(d_cursors != nullptr && d_flag != nullptr && d_out != nullptr,
               "tw_chain_unpack_count: cursors, flag and out");
  hipStream_t st = (hipStream_t)stream;
  const int NB = 2 * (n_shards + 1);
  const int64_t nc = (int64_t)NB * steps;
  hipLaunchKernelGGL(k_zero_two, dim3((unsigned)std::min<int64_t>(64, ceil_div(nc + bags, 256))),
                     dim3(256), 0, st, d_cursors, nc, d_out, bags);
  TW_LAUNCH_CHECK();
  if (n_x + n_z == 0) return TW_OK;
  const int parts = (int)std::max<int64_t>(
      1, std::min<int64_t>(ceil_div(cap, (int64_t)kBlock * kUnpackPer), 64));
  hipLaunchKernelGGL(k_chain_unpack, dim3((unsigned)(parts * world * steps)), dim3(kBlock),
                     sizeof(unsigned) * 2 * (size_t)NB, st, d_recv, (int)world, (int)steps, parts,
                     cap, half ? 2 : 1, (int)half, n_x, n_z, x_shard, z_shard, (int)n_shards,
                     d_x_bag, (uint32_t*)d_z_bag, (unsigned*)d_cursors, d_flag);
  TW_LAUNCH_CHECK();
  if (d_work != nullptr)  // (tw_chain_unpack_count_planes; its workspace checked there)
    return count_chain_launch_work(d_x_bag, d_x_off, n_x, d_z_bag, d_z_off, n_z, n_shards, steps,
                                   max_nx, max_nz, half, image_bound, d_out, d_work, st,
                                   /*zero_out=*/false);  // (k_zero_two above)
  return count_chain_launch(d_x_bag, d_x_off, n_x, d_z_bag, d_z_off, n_z, n_shards, steps,
                            max_nx, max_nz, half, d_out, st);
}

extern "C" int tw_chain_unpack_count(const uint64_t* d_recv, int32_t world, int32_t steps,
                                     int64_t cap, int32_t half, int64_t n_x, int64_t n_z,
                                     int64_t x_shard, int64_t z_shard, int32_t n_shards,
                                     void* d_x_bag, void* d_z_bag, uint32_t* d_cursors,
                                     int32_t* d_flag, const int64_t* d_x_off,
                                     const int64_t* d_z_off, int64_t max_nx, int64_t max_nz,
                                     uint64_t* d_out, void* stream) {
  return chain_unpack_count_impl(d_recv, world, steps, cap, half, n_x, n_z, x_shard, z_shard,
                                 n_shards, d_x_bag, d_z_bag, d_cursors, d_flag, d_x_off, d_z_off,
                                 max_nx, max_nz, -1, d_out, stream);
}

namespace tw {
// the packed kernel
static int count_chain_launch(const void* d_x_bag, const int64_t* d_x_off, int64_t x_stride,
                              const void* d_z_bag, const int64_t* d_z_off, int64_t z_stride,
                              int32_t n_shards, int32_t steps, int64_t max_nx, int64_t max_nz,
                              int32_t half, uint64_t* d_out, hipStream_t st) {
  const int64_t bags = (int64_t)n_shards * steps;
  if (max_nx == 0 || max_nz == 0) return TW_OK;
  const ChainPlan p = plan_chain(max_nx, max_nz, bags, half != 0);
  TW_ARG_CHECK(p.blocks * (kBlock / kWave) < (1ll << 31) && bags < (1ll << 31),
               "tw_count_pairs_chain: grid too large");
  dim3 g((unsigned)p.blocks), b(kBlock);
  auto* o = (unsigned long long*)d_out;
  const float* zb = (const float*)d_z_bag;
  if (half)
    hipLaunchKernelGGL((k_count_chain<8, true>), g, b, 0, st, d_x_bag, d_x_off, x_stride, zb,
                       d_z_off, z_stride, n_shards, (int)bags, p.tiles_x, p.zchunks, p.z_chunk,
                       o);
  else if (p.R == 16)
    hipLaunchKernelGGL((k_count_chain<16, false>), g, b, 0, st, d_x_bag, d_x_off, x_stride, zb,
                       d_z_off, z_stride, n_shards, (int)bags, p.tiles_x, p.zchunks, p.z_chunk,
                       o);
  else
    hipLaunchKernelGGL((k_count_chain<8, false>), g, b, 0, st, d_x_bag, d_x_off, x_stride, zb,
                       d_z_off, z_stride, n_shards, (int)bags, p.tiles_x, p.zchunks, p.z_chunk,
                       o);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

// The plane pre-pass and the count on its planes, back to back on st (out already zeroed);
// with class bits (cp.k > 0) pre-pass 2 between them, the plan's swapped items if it has any
// and the count on class runs.  fused (class bits only): one launch runs both pre-passes and
// zeroes out itself (k_chain_prepass).
template <int NB>
static void count_chain_launch_planes(const PlanesPlan& p, const ClassPlan& cp, bool fused,
                                      const float* xb,
                                      const int64_t* d_x_off, int64_t x_stride, const float* zb,
                                      const int64_t* d_z_off, int64_t z_stride, int n_shards,
                                      int bags, uint32_t* work, unsigned long long* o,
                                      hipStream_t st) {
  if (fused) {  // (cp.k > 0) both pre-passes and the zeroing of o in one launch
    hipLaunchKernelGGL((k_chain_prepass<NB>),
                       dim3((unsigned)prepass_grid(bags, p.gx, p.gz).blocks), dim3(kBlock), 0, st,
                       xb, d_x_off, x_stride, zb, d_z_off, z_stride, n_shards, bags, p.gx, p.gz,
                       p.swap, cp, work, o);
  } else {
    const int64_t pre = ceil_div((int64_t)bags * (p.gx + p.gz), kBlock / kWave);
    hipLaunchKernelGGL((k_chain_planes<NB>), dim3((unsigned)pre), dim3(kBlock), 0, st, xb,
                       d_x_off, x_stride, zb, d_z_off, z_stride, n_shards, bags, p.gx, p.gz,
                       p.swap, work);
  }
  if (cp.k > 0) {  // the class-run form: pre-pass 2, then the count on class runs
    if (!fused)
      hipLaunchKernelGGL(k_chain_zclasses, dim3((unsigned)bags), dim3(kBlock), 0, st, zb, d_z_off,
                         z_stride, n_shards, bags, NB, cp, work);
    const int n_swapped = p.tiles_s * p.schunks;
    if (n_swapped > 0)  // the plan's swapped items, in a launch of their own (same counts)
      hipLaunchKernelGGL((k_count_chain_swapped<NB>),
                         dim3((unsigned)ceil_div((int64_t)bags * n_swapped, kBlock / kWave)),
                         dim3(kBlock), 0, st, xb, d_x_off, x_stride, d_z_off, n_shards, bags, p,
                         (const uint32_t*)work, o);
    const dim3 g((unsigned)ceil_div(
                     (int64_t)bags * p.tiles_x * class_spans(cp.cap, cp.span), kBlock / kWave)),
        b(kBlock);
#define TW_CLASS_CASE(K)                                                                       \
  case K:                                                                                      \
    if constexpr (class_wide_fit(NB - K)) {                                                    \
      if (cp.dbits == kClassLdsBits) { /* one block per (bag, x tile): DESIGN §4.1m */         \
        hipLaunchKernelGGL((k_count_chain_classes_lds<NB, K>),                                 \
                           dim3((unsigned)((int64_t)bags * p.tiles_x)), dim3(kClassLdsThreads), \
                           0, st, d_x_off, d_z_off, n_shards, bags, p, cp,                     \
                           (const uint32_t*)work, o);                                          \
        break;                                                                                 \
      }                                                                                        \
      if (cp.dbits == kClassWideBits) {                                                        \
        hipLaunchKernelGGL((k_count_chain_classes<NB, K, kClassWideBits>), g, b, 0, st,        \
                           d_x_off, d_z_off, n_shards, bags, p, cp, (const uint32_t*)work, o); \
        break;                                                                                 \
      }                                                                                        \
    }                                                                                          \
    hipLaunchKernelGGL((k_count_chain_classes<NB, K>), g, b, 0, st, d_x_off, d_z_off,          \
                       n_shards, bags, p, cp, (const uint32_t*)work, o);                       \
    break;
    switch (cp.k) {
      TW_CLASS_CASE(1) TW_CLASS_CASE(2) TW_CLASS_CASE(3) TW_CLASS_CASE(4)
      TW_CLASS_CASE(5) TW_CLASS_CASE(6) TW_CLASS_CASE(7) TW_CLASS_CASE(8)
    }
#undef TW_CLASS_CASE
    return;
  }
  const int64_t blocks = ceil_div((int64_t)bags * p.per_bag, kBlock / kWave);
  hipLaunchKernelGGL((k_count_chain_planes<NB>), dim3((unsigned)blocks), dim3(kBlock), 0, st, xb,
                     d_x_off, x_stride, zb, d_z_off, z_stride, n_shards, bags, p,
                     (const uint32_t*)work, o);
}

// Bytes of plane workspace a bounded strict count of these bags may use (0: it runs packed)
static int64_t chain_planes_work_bytes(int64_t bags, int64_t max_nx, int64_t max_nz,
                                       int32_t half, int64_t image_bound) {
  const int nb = half ? 0 : bits_pick_nb(image_bound);
  if (nb == 0 || bags == 0 || max_nx == 0 || max_nz == 0) return 0;
  // (the class regions sized for any class bits and plan: chainclass.h's class_work_words)
  return (planes_work_words(max_nx, max_nz, bags, nb) + class_work_words(max_nz, bags)) *
         (int64_t)sizeof(uint32_t);
}

// The plan of a launch that runs a digit loop (form 3) of dbits planes per digit.  The digit
// loops' register maps hold kClassDigitsMaxR groups: the plan's tiles follow.  (A padded slot's
// price in the swap rule is that of the loop the launch runs; the LDS-table form plans as the
// wide loop it replaces.)
static PlanesPlan chain_digits_plan(int64_t max_nx, int64_t max_nz, int64_t bags, int nb, int k,
                                    int dbits) {
  int R = g_chain_R >= 1 && g_chain_R <= 4 ? g_chain_R : 0;
  R = R == 0 || R > kClassDigitsMaxR ? kClassDigitsMaxR : R;
  const int ndigits = dbits == kClassWideBits ? kClassWideDigits : kClassDigits;
  return planes_plan(max_nx, max_nz, bags, R, g_chain_zchunk,
                     class_swap_mode(g_planes_swap, max_nx, max_nz, nb, k, ndigits + 1));
}

// The count launch of the _planes entries on an output already zeroed (zero_out: zeroed here,
// by a launch of its own or inside the fused pre-pass): where chainplan.h's
// chain_count_sliced says so, the pre-pass and k_count_chain_planes (tuning hook: R = largest
// groups per item) or, with class bits, its class-run form (chainclass.h); everything else
// count_chain_launch's packed kernel.
static int count_chain_launch_work(const void* d_x_bag, const int64_t* d_x_off, int64_t x_stride,
                                   const void* d_z_bag, const int64_t* d_z_off, int64_t z_stride,
                                   int32_t n_shards, int32_t steps, int64_t max_nx,
                                   int64_t max_nz, int32_t half, int64_t image_bound,
                                   uint64_t* d_out, void* d_work, hipStream_t st,
                                   bool zero_out) {
  const int64_t bags = (int64_t)n_shards * steps;
  const int nb = bits_pick_nb(image_bound);
  const bool sliced =
      max_nx != 0 && max_nz != 0 && chain_count_sliced(max_nx, g_chain_R, half != 0, nb);
  const int k = sliced ? chain_class_bits(max_nz, bags, nb) : 0;
  // the fused pre-pass zeroes the counts itself; every other form adds to an output zeroed here
  const bool fused = prepass_form(g_prepass, k, max_nz) != 1;
  if (zero_out && !fused)
    TW_HIP_CHECK(tw_zero_async(d_out, 0, sizeof(uint64_t) * (size_t)bags, st));
  if (max_nx == 0 || max_nz == 0) return TW_OK;
  if (!sliced)
    return count_chain_launch(d_x_bag, d_x_off, x_stride, d_z_bag, d_z_off, z_stride, n_shards,
                              steps, max_nx, max_nz, half, d_out, st);
  // (under class runs the automatic swap also asks which remainder costs fewer instructions)
  // The digit loop's register map holds kClassDigitsMaxR groups: the plan's tiles follow
  const bool digits = k > 0 && class_loop_form(nb, k) == 3;
  // planes per digit: the wide split where it fits and the hook's setting asks for it
  const int dbits = digits ? class_digit_bits(nb, k, g_class_digits) : kClassDigitBits;
  const PlanesPlan p =
      digits ? chain_digits_plan(max_nx, max_nz, bags, nb, k, dbits)
             : planes_plan(max_nx, max_nz, bags, g_chain_R >= 1 && g_chain_R <= 4 ? g_chain_R : 0,
                           g_chain_zchunk,
                           class_swap_mode(g_planes_swap, max_nx, max_nz, nb, k, 0));
  // entries per item: the digit loop walks a span (forced, or chainclass.h's automatic rule);
  // the masked-plane loop's registers are class-dependent throughout: one run per item
  int64_t runs = 1;
  if (digits)
    runs = g_class_span > 0
               ? g_class_span
               : class_span_auto(bags, p.tiles_x, (int)class_capacity(max_nz, k, p.z_chunk));
  ClassPlan cp = class_plan(p, max_nx, max_nz, bags, nb, k, runs);
  cp.digits = digits ? nb - k : 0;
  // the LDS-table form where the launch would run the wide loop and the setting asks for it
  cp.dbits = !digits ? 0 : class_lds_runs(g_class_lds, dbits, p, bags) ? kClassLdsBits : dbits;
  TW_ARG_CHECK(bags * (int64_t)p.per_bag < (1ll << 31) &&
                   bags * (int64_t)(p.gx + p.gz) < (1ll << 31) &&
                   (!fused || prepass_grid_fits(bags, p.gx, p.gz)) &&
                   bags * (int64_t)cp.per_bag < (1ll << 31),
               "tw_count_pairs_chain_planes: grid too large");
  auto* o = (unsigned long long*)d_out;
  const float* xf = (const float*)d_x_bag;
  const float* zf = (const float*)d_z_bag;
  uint32_t* w = (uint32_t*)d_work;
  if (nb == 16)
    count_chain_launch_planes<16>(p, cp, fused, xf, d_x_off, x_stride, zf, d_z_off, z_stride, n_shards,
                                  (int)bags, w, o, st);
  else if (nb == 18)
    count_chain_launch_planes<18>(p, cp, fused, xf, d_x_off, x_stride, zf, d_z_off, z_stride, n_shards,
                                  (int)bags, w, o, st);
  else if (nb == 20)
    count_chain_launch_planes<20>(p, cp, fused, xf, d_x_off, x_stride, zf, d_z_off, z_stride, n_shards,
                                  (int)bags, w, o, st);
  else if (nb == 22)
    count_chain_launch_planes<22>(p, cp, fused, xf, d_x_off, x_stride, zf, d_z_off, z_stride, n_shards,
                                  (int)bags, w, o, st);
  else
    count_chain_launch_planes<24>(p, cp, fused, xf, d_x_off, x_stride, zf, d_z_off, z_stride, n_shards,
                                  (int)bags, w, o, st);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
}  // namespace tw

// The loop form the class count of a launch with nb planes and k class bits runs (chainclass.h
// class_loop_form; 3: the digit tables, where the low field fits them, 2: the masked planes)
extern "C" int32_t tw_count_chain_class_form(int32_t nb, int32_t k) {
  return class_loop_form(nb, k);
}

// The table entries an item of the digit loop walks (chainclass.h): runs >= 1
// forces that many (clamped to each launch's capacity), 0 restores the automatic rule, -1 only
// reports; any other value changes nothing.  Returns the setting in force before the call.
extern "C" int32_t tw_count_chain_class_span(int32_t runs) {
  const int32_t before = g_class_span;
  if (runs >= 0) g_class_span = runs;
  return before;
}

// The planes per digit of the digit loop (chainclass.h): 0 the automatic rule, 3
// the four-digit loop everywhere, 4 the wide digits where NB - K = 12 (anywhere else the
// four-digit loop runs), -1 only reports.  Returns the setting in force before the call;
// anything else changes nothing and returns TW_ERR_ARG.
extern "C" int32_t tw_count_chain_class_digits(int32_t w) {
  const int32_t before = g_class_digits;
  if (w == -1) return before;
  TW_ARG_CHECK(w == 0 || w == kClassDigitBits || w == kClassWideBits,
               "tw_count_chain_class_digits: 0 (automatic), 3, 4 or -1 (report)");
  g_class_digits = w;
  return before;
}

// The LDS-table form of the class count (chainclass.h): 0 the automatic rule, 1
// off — every launch is the digit loops' —, 2 on wherever the form fits (the launch would run
// the wide digits, two groups per tile, no swapped items), -1 only reports.  Returns the setting
// in force before the call; anything else changes nothing and returns TW_ERR_ARG.
// tw_count_chain_class_span has no effect on launches of this form.
extern "C" int32_t tw_count_chain_class_lds(int32_t mode) {
  const int32_t before = g_class_lds;
  if (mode == -1) return before;
  TW_ARG_CHECK(mode >= 0 && mode <= 2,
               "tw_count_chain_class_lds: 0 (automatic), 1 (off), 2 (on) or -1 (report)");
  g_class_lds = mode;
  return before;
}

// 1 if a strict launch of tw_count_pairs_chain_planes with these arguments runs the LDS-table
// form under the current settings, 0 otherwise
extern "C" int32_t tw_count_chain_class_lds_of(int32_t n_shards, int32_t steps, int64_t max_nx,
                                               int64_t max_nz, int64_t image_bound) {
  if (n_shards <= 0 || steps <= 0 || max_nx <= 0 || max_nz <= 0) return 0;
  const int64_t bags = (int64_t)n_shards * steps;
  const int nb = bits_pick_nb(image_bound);
  if (!chain_count_sliced(max_nx, g_chain_R, false, nb)) return 0;
  const int k = chain_class_bits(max_nz, bags, nb);
  if (k <= 0 || class_loop_form(nb, k) != 3) return 0;
  const int dbits = class_digit_bits(nb, k, g_class_digits);
  const PlanesPlan p = chain_digits_plan(max_nx, max_nz, bags, nb, k, dbits);
  return class_lds_runs(g_class_lds, dbits, p, bags) ? 1 : 0;
}

// The planes per digit a launch of (nb, k) runs under the current setting: 4 where it runs the
// wide digits, 3 everywhere else (where no digit loop runs the setting has no effect)
extern "C" int32_t tw_count_chain_class_digits_of(int32_t nb, int32_t k) {
  return k > 0 && class_loop_form(nb, k) == 3 ? class_digit_bits(nb, k, g_class_digits)
                                              : kClassDigitBits;
}

// How the pre-passes of the class-run form are launched: 0 automatic — fused
// wherever the class form runs —, 1 the separate launches (k_zero_fill, k_chain_planes,
// k_chain_zclasses), 2 fused wherever the class form runs, -1 only reports.  Returns the setting
// in force before the call; anything else changes nothing and returns TW_ERR_ARG.
extern "C" int32_t tw_count_chain_prepass(int32_t mode) {
  const int32_t before = g_prepass;
  if (mode == -1) return before;
  TW_ARG_CHECK(mode >= 0 && mode <= 2,
               "tw_count_chain_prepass: 0 (automatic), 1 (separate), 2 (fused) or -1 (report)");
  g_prepass = mode;
  return before;
}

// The form a strict launch of tw_count_pairs_chain_planes with these arguments runs under the
// current settings: 0 no pre-pass (the packed kernel), 1 separate launches, 2 the fused launch
// with every bag sorted in registers, 3 the fused launch with the streaming loop for bags past
// kPrepassCap images
extern "C" int32_t tw_count_chain_prepass_of(int32_t n_shards, int32_t steps, int64_t max_nx,
                                             int64_t max_nz, int64_t image_bound) {
  if (n_shards <= 0 || steps <= 0 || max_nx <= 0 || max_nz <= 0) return 0;
  const int nb = bits_pick_nb(image_bound);
  if (!chain_count_sliced(max_nx, g_chain_R, false, nb)) return 0;
  return prepass_form(g_prepass, chain_class_bits(max_nz, (int64_t)n_shards * steps, nb),
                      max_nz);
}

extern "C" int64_t tw_chain_planes_work_bytes(int32_t n_shards, int32_t steps, int64_t max_nx,
                                              int64_t max_nz, int32_t half,
                                              int64_t image_bound) {
  if (n_shards < 0 || steps < 0 || max_nx < 0 || max_nz < 0) return 0;
  return chain_planes_work_bytes((int64_t)n_shards * steps, max_nx, max_nz, half, image_bound);
}

// tw_count_pairs_chain with the caller's promise that every x and z image lies in
// [0, image_bound] (x also: the -2^25 "never" image): the strict predicate with
// image_bound < 2^24 runs bit-sliced where chain_count_sliced says so, on planes built once per
// bag, everything else packed.  Same counts either way.  Bit-sliced: the pre-pass
// (k_chain_planes) and the count (k_count_chain_planes or its class-run form) back to back on
// the stream.
// d_work: tw_chain_planes_work_bytes(...) bytes, written and read inside this call only.
extern "C" int tw_count_pairs_chain_planes(const void* d_x_bag, const int64_t* d_x_off,
                                           int64_t x_stride, const void* d_z_bag,
                                           const int64_t* d_z_off, int64_t z_stride,
                                           int32_t n_shards, int32_t steps, int64_t max_nx,
                                           int64_t max_nz, int32_t half, int64_t image_bound,
                                           uint64_t* d_out, void* stream, void* d_work,
                                           int64_t work_bytes) {
  TW_ARG_CHECK(image_bound >= 0, "tw_count_pairs_chain_planes: image_bound >= 0");
  TW_ARG_CHECK(n_shards >= 0 && steps >= 0 && max_nx >= 0 && max_nz >= 0 && x_stride >= 0 &&
                   z_stride >= 0 && (half == 0 || half == 1),
               "tw_count_pairs_chain_planes: bad sizes");
  TW_ARG_CHECK(max_nz < (1ll << 24), "tw_count_pairs_chain_planes: shards of < 2^24 z-images");
  const int64_t bags = (int64_t)n_shards * steps;
  if (bags == 0) return TW_OK;
  const int64_t need = chain_planes_work_bytes(bags, max_nx, max_nz, half, image_bound);
  TW_ARG_CHECK(work_bytes >= need && (need == 0 || d_work != nullptr),
               "tw_count_pairs_chain_planes: work_bytes %lld < %lld (tw_chain_planes_work_bytes)",
               (long long)work_bytes, (long long)need);
  return count_chain_launch_work(d_x_bag, d_x_off, x_stride, d_z_bag, d_z_off, z_stride,
                                 n_shards, steps, max_nx, max_nz, half, image_bound, d_out,
                                 d_work, (hipStream_t)stream, /*zero_out=*/true);
}

// tw_chain_unpack_count with tw_count_pairs_chain_planes' promise and count
extern "C" int tw_chain_unpack_count_planes(const uint64_t* d_recv, int32_t world, int32_t steps,
                                            int64_t cap, int32_t half, int64_t n_x, int64_t n_z,
                                            int64_t x_shard, int64_t z_shard, int32_t n_shards,
                                            void* d_x_bag, void* d_z_bag, uint32_t* d_cursors,
                                            int32_t* d_flag, const int64_t* d_x_off,
                                            const int64_t* d_z_off, int64_t max_nx,
                                            int64_t max_nz, int64_t image_bound, uint64_t* d_out,
                                            void* stream, void* d_work, int64_t work_bytes) {
  TW_ARG_CHECK(image_bound >= 0, "tw_chain_unpack_count_planes: image_bound >= 0");
  TW_ARG_CHECK(n_shards >= 0 && steps >= 0 && max_nx >= 0 && max_nz >= 0 &&
                   (half == 0 || half == 1),
               "tw_chain_unpack_count_planes: bad sizes");
  const int64_t need =
      chain_planes_work_bytes((int64_t)n_shards * steps, max_nx, max_nz, half, image_bound);
  TW_ARG_CHECK(work_bytes >= need && (need == 0 || d_work != nullptr),
               "tw_chain_unpack_count_planes: work_bytes %lld < %lld "
               "(tw_chain_planes_work_bytes)", (long long)work_bytes, (long long)need);
  return chain_unpack_count_impl(d_recv, world, steps, cap, half, n_x, n_z, x_shard, z_shard,
                                 n_shards, d_x_bag, d_z_bag, d_cursors, d_flag, d_x_off, d_z_off,
                                 max_nx, max_nz, image_bound, d_out, stream, d_work);
}

// ----------------------------------------------------------------------------- exact count
// The exact O(n + m) count of the bags (algo="sorted", row f4) on the rank images themselves:
// z images are integers g in [0, z_total], so a bag's z, bucketed by g >> shift into <= 16384
// LDS buckets (a counting sort in LDS), answer #{z : g(z) < t} as the z count of the lower
// buckets + a scan of t's own bucket (~1 z).  Per x: t = g(x) ([x > z] <=> g(z) < g(x)); half
// ties add t = h(x) ([x >= z] <=> g(z) < h(x)).  NaN x (image -2^25) count nothing; NaN z
// (g = #non-NaN z) are below no t.  One block per (step, shard) bag, bags of <= 16384 z.
namespace tw {

constexpr int kCbMaxZ = 16384;
constexpr int kCbBuckets = 16384;
constexpr int kCbThreads = 1024;
constexpr int kCbPer = kCbMaxZ / kCbThreads;  // z per thread

template <bool HALF>
__global__ __launch_bounds__(kCbThreads) void k_count_chain_bucket(
    const void* __restrict__ xbag, const int64_t* __restrict__ x_off, int64_t x_stride,
    const float* __restrict__ zbag, const int64_t* __restrict__ z_off, int64_t z_stride,
    int n_shards, int shift, int nbk, unsigned long long* __restrict__ out) {
  __shared__ uint32_t end[kCbBuckets];  // after the scatter: end of bucket b = start of b + 1
  __shared__ uint32_t zs[kCbMaxZ];
  __shared__ uint32_t wtot[kCbThreads / kWave];
  __shared__ unsigned long long bsum[kCbThreads / kWave];
  const int bag = xcd_block(blockIdx.x, gridDim.x);  // a step's shards on one XCD
  const int c = bag / n_shards, s = bag - c * n_shards;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  const int64_t z0 = z_off[s], x0 = x_off[s];
  const int nz = (int)(z_off[s + 1] - z0);
  const int64_t nx = x_off[s + 1] - x0;
  const float* zp = zbag + (int64_t)c * z_stride + z0;
  uint32_t zv[kCbPer];
#pragma unroll
  for (int u = 0; u < kCbPer; ++u) {  // all loads in flight before the first LDS atomic
    const int i = tid + u * kCbThreads;
    zv[u] = i < nz ? (uint32_t)(-zp[i]) : 0xFFFFFFFFu;  // z bags hold -g(z)
  }
  for (int b = tid; b < nbk; b += kCbThreads) end[b] = 0;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kCbPer; ++u)
    if (zv[u] != 0xFFFFFFFFu) atomicAdd(&end[zv[u] >> shift], 1u);
  __syncthreads();
  // exclusive prefix of the counts: kCbPer consecutive buckets per thread, wave scans, then
  // the wave totals
  {
    const int b0 = tid * kCbPer;
    uint32_t loc[kCbPer], sum = 0;
#pragma unroll
    for (int u = 0; u < kCbPer; ++u) {
      loc[u] = b0 + u < nbk ? end[b0 + u] : 0u;
      sum += loc[u];
    }
    uint32_t inc = sum;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint32_t t = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += t;
    }
    if (lane == kWave - 1) wtot[wid] = inc;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wid; ++w) wbase += wtot[w];
    uint32_t run = wbase + inc - sum;
#pragma unroll
    for (int u = 0; u < kCbPer; ++u) {
      if (b0 + u < nbk) end[b0 + u] = run;  // start of bucket b0 + u
      run += loc[u];
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kCbPer; ++u)  // counting-sort scatter: start -> end of every bucket
    if (zv[u] != 0xFFFFFFFFu) zs[atomicAdd(&end[zv[u] >> shift], 1u)] = zv[u];
  __syncthreads();
  auto below = [&](float tf) -> uint32_t {  // #{z of the bag : g(z) < t}
    if (!(tf > 0.0f)) return 0u;              // t <= 0 (or the NaN-x sentinel): none below
    const uint32_t t = (uint32_t)tf;
    const uint32_t b = t >> shift;            // < nbk: t <= z_total
    uint32_t lo = b ? end[b - 1] : 0u;
    // shift 0: every z of bucket t has image exactly t — none below it, no scan;
    // shift > 0: a bucket spans 2^shift images and is scanned (tie-heavy bags: long buckets)
    if (shift == 0) return lo;
    const uint32_t hi = end[b];
    uint32_t cnt = lo;
    for (; lo < hi; ++lo) cnt += zs[lo] < t ? 1u : 0u;
    return cnt;
  };
  unsigned long long acc = 0;
  if constexpr (HALF) {
    const uint64_t* xp = (const uint64_t*)xbag + (int64_t)c * x_stride + x0;
    for (int64_t i = tid; i < nx; i += kCbThreads) {
      const uint64_t v = xp[i];
      acc += below(__uint_as_float((uint32_t)v)) + below(__uint_as_float((uint32_t)(v >> 32)));
    }
  } else {
    const float* xp = (const float*)xbag + (int64_t)c * x_stride + x0;
    for (int64_t i = tid; i < nx; i += kCbThreads) acc += below(xp[i]);
  }
  acc = wave_sum_u64(acc);
  if (lane == 0) bsum[wid] = acc;
  __syncthreads();
  if (tid == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < kCbThreads / kWave; ++w) t += bsum[w];
    out[bag] = t;
  }
}

}  // namespace tw

extern "C" int tw_count_pairs_chain_bucket(const void* d_x_bag, const int64_t* d_x_off,
                                           int64_t x_stride, const void* d_z_bag,
                                           const int64_t* d_z_off, int64_t z_stride,
                                           int32_t n_shards, int32_t steps, int64_t max_nz,
                                           int64_t z_total, int32_t half, uint64_t* d_out,
                                           void* stream) {
  TW_ARG_CHECK(n_shards >= 0 && steps >= 0 && x_stride >= 0 && z_stride >= 0 &&
                   (half == 0 || half == 1) && z_total >= 0 && z_total < (1ll << 24),
               "tw_count_pairs_chain_bucket: bad sizes");
  TW_ARG_CHECK(max_nz >= 0 && max_nz <= kCbMaxZ,
               "tw_count_pairs_chain_bucket: bags of <= %d z (use tw_count_pairs_chain)",
               kCbMaxZ);
  const int64_t bags = (int64_t)n_shards * steps;
  TW_ARG_CHECK(bags < (1ll << 31), "tw_count_pairs_chain_bucket: too many bags");
  if (bags == 0) return TW_OK;
  int shift = 0;
  while ((z_total >> shift) >= kCbBuckets) ++shift;
  const int nbk = (int)(z_total >> shift) + 1;
  hipStream_t st = (hipStream_t)stream;
  auto* o = (unsigned long long*)d_out;
  if (half)
    hipLaunchKernelGGL((k_count_chain_bucket<true>), dim3((unsigned)bags), dim3(kCbThreads), 0,
                       st, d_x_bag, d_x_off, x_stride, (const float*)d_z_bag, d_z_off, z_stride,
                       n_shards, shift, nbk, o);
  else
    hipLaunchKernelGGL((k_count_chain_bucket<false>), dim3((unsigned)bags), dim3(kCbThreads), 0,
                       st, d_x_bag, d_x_off, x_stride, (const float*)d_z_bag, d_z_off, z_stride,
                       n_shards, shift, nbk, o);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int tw_count_chain_set_plan(int32_t R, int64_t z_chunk) {
  TW_ARG_CHECK(R == 0 || R == 8 || R == 16 || (R >= 2 && R <= 4),
               "tw_count_chain_set_plan: R in {0, 8, 16} (packed) or {2, 3, 4} (bit-sliced)");
  TW_ARG_CHECK(z_chunk >= 0 && z_chunk <= (1ll << 24), "tw_count_chain_set_plan: bad z_chunk");
  g_chain_R = R;
  g_chain_zchunk = z_chunk;
  return TW_OK;
}

extern "C" int tw_count_chain_set_swap(int32_t swap) {
  TW_ARG_CHECK(swap >= 0 && swap <= 2, "tw_count_chain_set_swap: 0, 1 or 2");
  g_planes_swap = swap;
  return TW_OK;
}

extern "C" int tw_count_chain_set_class_bits(int32_t k) {
  TW_ARG_CHECK(k >= -1 && k <= kClassMaxBits,
               "tw_count_chain_set_class_bits: -1 (automatic), 0 (off) or 1 .. 8");
  g_class_bits = k;
  return TW_OK;
}

extern "C" int tw_chain_scatter(const void* d_x, const uint32_t* d_x_pos, int64_t n_x,
                                const void* d_z, const uint32_t* d_z_pos, int64_t n_z,
                                void* d_x_out, void* d_z_out, void* stream) {
  TW_ARG_CHECK(n_x >= 0 && n_z >= 0, "tw_chain_scatter: bad sizes");
  TW_ARG_CHECK((n_x == 0 || d_x != d_x_out) && (n_z == 0 || d_z != d_z_out),
               "tw_chain_scatter: in and out must differ");
  if (n_x + n_z == 0) return TW_OK;
  const unsigned grid = (unsigned)std::min<int64_t>(4096, ceil_div(n_x + n_z, kBlock));
  hipLaunchKernelGGL(k_chain_scatter, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint64_t*)d_x, d_x_pos, n_x, (const uint64_t*)d_z, d_z_pos, n_z,
                     (uint64_t*)d_x_out, (uint64_t*)d_z_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
