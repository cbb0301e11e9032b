// triplet_grad.hip — triplet metric learning (tuplewise.triplet_learning; an
// extension, not in the reference): a linear map L (p, d) under the triplet hinge.  For a triplet
// (i, j, k), a = x_i - x_j, b = x_i - z_k, u = L a, v = L b:
//   S = margin + |u|^2 - |v|^2,  loss = max(S, 0),  G_t = 1{S > 0} 2 (u a^T - v b^T)
// tw_triplet_grad gives the mean over non-empty shards of the shard means of G_t, and per shard
// the mean loss and the count of S > 0.  No bit contract on G and the loss (explicit fma, a fixed
// summation order: no atomics, block partials added in block order); tw_triplet_project and
// tw_triplet_sgd_update are bit-exact (multiply and add separate; the build has
// -ffp-contract=off).
#include "tw_common.h"
#include "selfreduce.h"
#include <algorithm>

namespace tw {

constexpr int kTgMax = 64;     // d and p, at most
constexpr int kTgSlice = 128;  // triplets per workgroup
constexpr int kTgWaves = kBlock / kWave;
constexpr int kTgCC = 8;       // columns of G per pass of the block reduction

// LDS of one workgroup, in doubles: L^T ([DP][PP], rows r >= p and columns c >= d zero), then the
// (a, b) rows of the triplets in flight ([wave][group][DP][2]) — which the block reduction's
// [kTgCC][kBlock] image reuses after the loop.
template <int DP, int PP>
struct TgLds {
  static constexpr int G = kWave / PP;  // triplets side by side in a wave
  static constexpr int kLt = DP * PP;
  static constexpr int kAb = kTgWaves * G * DP * 2;
  static constexpr int kRed = kTgCC * kBlock;
  static constexpr int kTotal = kLt + (kAb > kRed ? kAb : kRed);
};

// One workgroup per (shard, slice of kTgSlice triplets).  Within a wave a group of PP lanes owns
// one triplet and lane r of the group the output row r: u_r and v_r take 2 d multiply-adds over
// wave-uniform (per group) LDS reads of a and b, two butterflies over the group give S, and an
// active triplet adds 2 (u_r a_c - v_r b_c) into the lane's row of G, DP doubles in registers.
// The rows of the next triplets are in flight (registers) while the current ones are used.
// GRAD = false (the evaluation's surrogate) keeps no row of G.
template <int DP, int PP, bool GRAD>
__global__ __launch_bounds__(kBlock) void k_triplet_grad(
    const double* __restrict__ x, const double* __restrict__ z, int d,
    const double* __restrict__ Lm, int p, const int32_t* __restrict__ ii,
    const int32_t* __restrict__ jj, const int32_t* __restrict__ kk,
    const int64_t* __restrict__ trip_off, int per, double margin, double* __restrict__ w_loss,
    unsigned long long* __restrict__ w_act, double* __restrict__ w_G) {
  using Lds = TgLds<DP, PP>;
  constexpr int G = Lds::G;
  constexpr int NL = (G * DP + kWave - 1) / kWave;  // (triplet, coordinate) entries per lane
  __shared__ double smem[Lds::kTotal];
  __shared__ unsigned long long part[kTgWaves];
  double* __restrict__ sLt = smem;
  double* __restrict__ sab = smem + Lds::kLt;

  const int sh = (int)blockIdx.x / per, bi = (int)blockIdx.x - sh * per;
  const int64_t te = trip_off[sh + 1];
  const int64_t t0 = trip_off[sh] + (int64_t)bi * kTgSlice;
  if (t0 >= te) return;  // block-uniform: this shard has no such slice
  const int cnt = (int)std::min<int64_t>(kTgSlice, te - t0);
  const int iters = (cnt + kTgWaves * G - 1) / (kTgWaves * G);

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  const int grp = lane / PP, r = lane - grp * PP;

  for (int q = tid; q < DP * PP; q += kBlock) {
    const int c = q / PP, rr = q - c * PP;
    sLt[q] = (c < d && rr < p) ? Lm[rr * d + c] : 0.0;
  }

  // entry e of a lane: (triplet e_g of the wave's G, coordinate e_c)
  double na[NL], nb[NL];
  auto fetch = [&](int it) {
#pragma unroll
    for (int e = 0; e < NL; ++e) {
      const int q = lane + e * kWave;
      const int eg = q / DP, ec = q - eg * DP;
      const int t = (it * kTgWaves + wid) * G + eg;
      na[e] = 0.0;
      nb[e] = 0.0;
      if (q < G * DP && ec < d && t < cnt) {
        const double* __restrict__ xi = x + (int64_t)ii[t0 + t] * d;
        const double v = xi[ec];
        na[e] = v - x[(int64_t)jj[t0 + t] * d + ec];
        nb[e] = v - z[(int64_t)kk[t0 + t] * d + ec];
      }
    }
  };

  double grow[GRAD ? DP : 1];
#pragma unroll
  for (int c = 0; c < (GRAD ? DP : 1); ++c) grow[c] = 0.0;
  double loss = 0.0;
  unsigned act = 0;
  double* __restrict__ my = sab + (wid * G + grp) * DP * 2;  // this lane's triplet

  fetch(0);
  for (int it = 0; it < iters; ++it) {
    __syncthreads();  // the previous triplets' readers (and, first, sLt's writers)
#pragma unroll
    for (int e = 0; e < NL; ++e) {
      const int q = lane + e * kWave;
      if (q < G * DP) {
        sab[wid * G * DP * 2 + 2 * q] = na[e];
        sab[wid * G * DP * 2 + 2 * q + 1] = nb[e];
      }
    }
    __syncthreads();
    if (it + 1 < iters) fetch(it + 1);

    // (a rolled loop: unrolled whole, the compiler keeps all of a and b in registers for the
    // second pass below, beside the lane's row of G, and the DP = 64 forms fall to one wave per
    // SIMD)
    double u = 0.0, v = 0.0;
#pragma unroll 8
    for (int c = 0; c < DP; ++c) {
      const double l = sLt[c * PP + r];
      u = fma(l, my[2 * c], u);
      v = fma(l, my[2 * c + 1], v);
    }
    double su = u * u, sv = v * v;
#pragma unroll
    for (int o = PP / 2; o > 0; o >>= 1) {
      su += __shfl_xor(su, o, kWave);
      sv += __shfl_xor(sv, o, kWave);
    }
    const double S = margin + su - sv;
    const bool live = (it * kTgWaves + wid) * G + grp < cnt;
    if (live && S > 0.0) {
      if (r == 0) {
        loss += S;
        act += 1u;
      }
      if constexpr (GRAD) {
        const double u2 = 2.0 * u, v2 = -2.0 * v;
#pragma unroll
        for (int c = 0; c < DP; ++c)
          grow[c] = fma(u2, my[2 * c], fma(v2, my[2 * c + 1], grow[c]));
      }
    }
  }

  // block partials: loss and active in the fixed order of selfreduce.h
  const double bl = self_block_sum_f64(loss, (double*)part);
  const unsigned long long ba = self_block_sum_u64(act, part);
  if (tid == 0) {
    w_loss[blockIdx.x] = bl;
    w_act[blockIdx.x] = ba;
  }
  if constexpr (GRAD) {
    // G: kTgCC columns at a time through LDS, the waves and groups added in a fixed order
    double* __restrict__ red = sab;
    double* __restrict__ out = w_G + (int64_t)blockIdx.x * p * d;
#pragma unroll
    for (int c0 = 0; c0 < DP; c0 += kTgCC) {
      __syncthreads();
#pragma unroll
      for (int cc = 0; cc < kTgCC; ++cc) red[cc * kBlock + tid] = grow[c0 + cc];
      __syncthreads();
      for (int o = tid; o < PP * kTgCC; o += kBlock) {
        const int rr = o / kTgCC, cc = o - rr * kTgCC;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < kTgWaves * G; ++q) s += red[cc * kBlock + q * PP + rr];
        if (rr < p && c0 + cc < d) out[rr * d + c0 + cc] = s;
      }
    }
  }
}

// the slices (workgroups) of a shard of t triplets: at most the `per` the launch gave each shard
__device__ __forceinline__ int tg_slices(int64_t t, int per) {
  return (int)std::min<int64_t>((t + kTgSlice - 1) / kTgSlice, per);
}

constexpr int kTgRedE = 16;                  // elements of G per block of the reduction
constexpr int kTgRedS = kBlock / kTgRedE;     // and the groups its shards are dealt to

// d_G[e] = (sum over non-empty shards of the shard's block partials added in block order / its
// triplets) / the number of non-empty shards.  A block owns kTgRedE elements; its shards are dealt
// round-robin to kTgRedS groups of threads, each adding its own in shard order, and the groups'
// sums are added in group order: a fixed order whatever the schedule.  d_loss[s] and d_active[s]
// likewise from their partials (an empty shard: 0).  Blocks [0, g_blocks) own the elements of G,
// the rest the shards.
__global__ __launch_bounds__(kBlock) void k_triplet_grad_reduce(
    const double* __restrict__ w_loss, const unsigned long long* __restrict__ w_act,
    const double* __restrict__ w_G, const int64_t* __restrict__ trip_off, int n_shards, int per,
    int pd, int g_blocks, double* __restrict__ G, double* __restrict__ loss,
    unsigned long long* __restrict__ active) {
  if ((int)blockIdx.x < g_blocks) {
    __shared__ double stot[kTgRedS][kTgRedE];
    __shared__ int snz[kTgRedS];
    const int el = threadIdx.x % kTgRedE, sg = threadIdx.x / kTgRedE;
    const int e = (int)blockIdx.x * kTgRedE + el;
    double total = 0.0;
    int nz = 0;
    for (int s = sg; s < n_shards; s += kTgRedS) {
      const int64_t t = trip_off[s + 1] - trip_off[s];
      if (t <= 0) continue;
      ++nz;
      if (e >= pd) continue;
      const int nb = tg_slices(t, per);
      const double* __restrict__ w = w_G + (int64_t)s * per * pd + e;
      double acc = 0.0;
#pragma unroll 4
      for (int b = 0; b < nb; ++b) acc += w[(int64_t)b * pd];
      total += acc / (double)t;
    }
    stot[sg][el] = total;
    if (el == 0) snz[sg] = nz;
    __syncthreads();
    if (sg == 0 && e < pd) {
      double sum = 0.0;
      int n = 0;
#pragma unroll
      for (int q = 0; q < kTgRedS; ++q) {
        sum += stot[q][el];
        n += snz[q];
      }
      G[e] = n ? sum / (double)n : 0.0;
    }
    return;
  }
  const int s = ((int)blockIdx.x - g_blocks) * kBlock + threadIdx.x;
  if (s >= n_shards) return;
  const int64_t t = trip_off[s + 1] - trip_off[s];
  double acc = 0.0;
  unsigned long long a = 0;
  if (t > 0) {
    const int nb = tg_slices(t, per);
    for (int b = 0; b < nb; ++b) {
      acc += w_loss[(int64_t)s * per + b];
      a += w_act[(int64_t)s * per + b];
    }
    acc = acc / (double)t;
  }
  loss[s] = acc;
  active[s] = a;
}

// NaN as THE quiet NaN (triplets.hip trip_canon: which NaN an operation returns is the
// hardware's choice).
__device__ __forceinline__ double tg_canon(double v) {
  return v != v ? __longlong_as_double(0x7ff8000000000000ll) : v;
}

// out[row, r] = acc over ascending c of acc + L[r, c] * A[row, c]: one thread per output.
__global__ __launch_bounds__(kBlock) void k_triplet_project(const double* __restrict__ A,
                                                            int64_t rows, int d,
                                                            const double* __restrict__ Lm, int p,
                                                            double* __restrict__ out) {
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (o >= rows * p) return;
  const int64_t row = o / p;
  const int r = (int)(o - row * p);
  const double* __restrict__ a = A + row * d;
  const double* __restrict__ l = Lm + r * d;
  double acc = 0.0;
#pragma unroll 4
  for (int c = 0; c < d; ++c) {
    const double t = l[c] * a[c];
    acc = acc + t;
  }
  out[o] = tg_canon(acc);
}

// g = G + reg L; delta = [0.9 delta +] lr g; L = L - delta, elementwise, multiply and add
// separate.
__global__ __launch_bounds__(kBlock) void k_triplet_sgd_update(const double* __restrict__ G,
                                                               double* __restrict__ Lm,
                                                               double* __restrict__ delta, int count,
                                                               double reg, double lr, int momentum) {
  const int e = (int)blockIdx.x * kBlock + threadIdx.x;
  if (e >= count) return;
  const double rl = reg * Lm[e];
  const double g = G[e] + rl;
  const double step = lr * g;
  double dl = step;
  if (momentum) {
    const double m = 0.9 * delta[e];
    dl = m + step;
  }
  delta[e] = dl;
  Lm[e] = Lm[e] - dl;
}

inline int64_t tg_blocks_per_shard(int64_t max_triplets) {
  return std::max<int64_t>(1, ceil_div(max_triplets, kTgSlice));
}

template <int DP, int PP>
static void tg_launch(bool grad, dim3 g, hipStream_t st, const double* x, const double* z, int d,
                      const double* Lm, int p, const int32_t* ii, const int32_t* jj,
                      const int32_t* kk, const int64_t* off, int per, double margin,
                      double* w_loss, unsigned long long* w_act, double* w_G) {
  if (grad)
    hipLaunchKernelGGL((k_triplet_grad<DP, PP, true>), g, dim3(kBlock), 0, st, x, z, d, Lm, p, ii,
                       jj, kk, off, per, margin, w_loss, w_act, w_G);
  else
    hipLaunchKernelGGL((k_triplet_grad<DP, PP, false>), g, dim3(kBlock), 0, st, x, z, d, Lm, p, ii,
                       jj, kk, off, per, margin, w_loss, w_act, w_G);
}

template <int DP, typename... A>
static void tg_launch_p(int p, A... a) {
  if (p <= 8) tg_launch<DP, 8>(a...);
  else if (p <= 16) tg_launch<DP, 16>(a...);
  else if (p <= 32) tg_launch<DP, 32>(a...);
  else tg_launch<DP, 64>(a...);
}

}  // namespace tw

using namespace tw;

extern "C" int32_t tw_triplet_grad_tile(void) { return kTgSlice; }

extern "C" int64_t tw_triplet_grad_work_bytes(int32_t n_shards, int64_t max_triplets, int32_t d,
                                              int32_t p) {
  if (n_shards < 0 || max_triplets < 0 || d < 1 || d > kTgMax || p < 1 || p > kTgMax) return 0;
  const int64_t blocks = tg_blocks_per_shard(max_triplets) * n_shards;
  return std::max<int64_t>(8, blocks * (16 + (int64_t)p * d * 8));
}

extern "C" int tw_triplet_grad(const double* d_x, const double* d_z, int32_t d, const double* d_L,
                               int32_t p, const int32_t* d_i, const int32_t* d_j,
                               const int32_t* d_k, const int64_t* d_trip_off, int32_t n_shards,
                               int64_t max_triplets, double margin, int32_t want_grad,
                               void* d_work, double* d_G, double* d_loss, uint64_t* d_active,
                               void* stream) {
  TW_ARG_CHECK(d_x && d_z && d_L && d_i && d_j && d_k && d_trip_off && d_work && d_loss &&
                   d_active && (d_G || !want_grad),
               "tw_triplet_grad: null pointer");
  TW_ARG_CHECK(d >= 1 && d <= kTgMax, "tw_triplet_grad: d %d outside [1, %d]", d, kTgMax);
  TW_ARG_CHECK(p >= 1 && p <= kTgMax, "tw_triplet_grad: p %d outside [1, %d]", p, kTgMax);
  TW_ARG_CHECK(n_shards >= 0, "tw_triplet_grad: n_shards %d < 0", n_shards);
  TW_ARG_CHECK(max_triplets >= 0, "tw_triplet_grad: max_triplets %lld < 0",
               (long long)max_triplets);
  TW_ARG_CHECK(want_grad == 0 || want_grad == 1, "tw_triplet_grad: want_grad %d (0 or 1)",
               want_grad);
  TW_ARG_CHECK(margin == margin, "tw_triplet_grad: margin is NaN");
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = tg_blocks_per_shard(max_triplets), blocks = per * n_shards;
  TW_ARG_CHECK(blocks < (1ll << 31), "tw_triplet_grad: grid too large");
  const int pd = p * d;
  double* w_loss = (double*)d_work;
  unsigned long long* w_act = (unsigned long long*)d_work + blocks;
  double* w_G = (double*)d_work + 2 * blocks;
  if (n_shards > 0) {
    const dim3 g((unsigned)blocks);
    const bool grad = want_grad != 0;
    if (d <= 8)
      tg_launch_p<8>(p, grad, g, st, d_x, d_z, (int)d, d_L, (int)p, d_i, d_j, d_k, d_trip_off,
                     (int)per, margin, w_loss, w_act, w_G);
    else if (d <= 16)
      tg_launch_p<16>(p, grad, g, st, d_x, d_z, (int)d, d_L, (int)p, d_i, d_j, d_k, d_trip_off,
                      (int)per, margin, w_loss, w_act, w_G);
    else if (d <= 32)
      tg_launch_p<32>(p, grad, g, st, d_x, d_z, (int)d, d_L, (int)p, d_i, d_j, d_k, d_trip_off,
                      (int)per, margin, w_loss, w_act, w_G);
    else
      tg_launch_p<64>(p, grad, g, st, d_x, d_z, (int)d, d_L, (int)p, d_i, d_j, d_k, d_trip_off,
                      (int)per, margin, w_loss, w_act, w_G);
    TW_LAUNCH_CHECK();
  }
  const int g_blocks = want_grad ? (int)ceil_div(pd, kTgRedE) : 0;
  const int s_blocks = (int)ceil_div(n_shards, kBlock);
  if (g_blocks + s_blocks == 0) return TW_OK;
  hipLaunchKernelGGL(k_triplet_grad_reduce, dim3((unsigned)(g_blocks + s_blocks)), dim3(kBlock), 0,
                     st, (const double*)w_loss, (const unsigned long long*)w_act,
                     (const double*)w_G, d_trip_off, (int)n_shards, (int)per, pd, g_blocks, d_G,
                     d_loss, (unsigned long long*)d_active);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int tw_triplet_project(const double* d_a, int64_t rows, int32_t d, const double* d_L,
                                  int32_t p, double* d_out, void* stream) {
  TW_ARG_CHECK(d_a && d_L && d_out, "tw_triplet_project: null pointer");
  TW_ARG_CHECK(d >= 1 && d <= kTgMax, "tw_triplet_project: d %d outside [1, %d]", d, kTgMax);
  TW_ARG_CHECK(p >= 1 && p <= kTgMax, "tw_triplet_project: p %d outside [1, %d]", p, kTgMax);
  TW_ARG_CHECK(rows >= 0, "tw_triplet_project: rows %lld < 0", (long long)rows);
  if (rows == 0) return TW_OK;
  const int64_t blocks = ceil_div(rows * p, kBlock);
  TW_ARG_CHECK(blocks < (1ll << 31), "tw_triplet_project: grid too large");
  hipLaunchKernelGGL(k_triplet_project, dim3((unsigned)blocks), dim3(kBlock), 0,
                     (hipStream_t)stream, d_a, rows, (int)d, d_L, (int)p, d_out);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

extern "C" int tw_triplet_sgd_update(const double* d_G, double* d_L, double* d_delta,
                                     int32_t count, double reg, double lr, int32_t momentum,
                                     void* stream) {
  TW_ARG_CHECK(d_G && d_L && d_delta, "tw_triplet_sgd_update: null pointer");
  TW_ARG_CHECK(count >= 1 && count <= kTgMax * kTgMax,
               "tw_triplet_sgd_update: count %d outside [1, %d]", count, kTgMax * kTgMax);
  TW_ARG_CHECK(momentum == 0 || momentum == 1, "tw_triplet_sgd_update: momentum %d (0 or 1)",
               momentum);
  hipLaunchKernelGGL(k_triplet_sgd_update, dim3((unsigned)ceil_div(count, kBlock)), dim3(kBlock),
                     0, (hipStream_t)stream, d_G, d_L, d_delta, (int)count, reg, lr,
                     (int)momentum);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
