// Microbenchmark (design probe for k_count_chain_bits): the bit-sliced
// compare-and-count of csrc/bitcount.h against the packed-f32 loop of tools/mb_pk.hip, on the
// bench's shard shape (64 shards of 15625 x 15625), both in one process, alternating per round.
//   packed:     2 v_pk_add_f32 per 128 pairs                      = 1 VALU / 64 pairs
//   bit-sliced: NB + 1 VALU per 64 * 32 pairs (+ 1 v_readlane_b32 per z and wave, NB s_bfe_i32
//               per z and wave on the scalar side), NB = 20 here   = 1 VALU / 97.5 pairs
// Printed per configuration: median and best ms over the rounds, pairs per inner-loop VALU
// instruction (the instruction count is the loops' own: items x z x instructions per z; an
// item's x loads, conversion and bit transpose are NOT in it, so they show as a lower issue
// rate), and those instructions per clock and CU at a nominal 2.4 GHz.
//   hipcc --offload-arch=gfx950 -O3 -o tools/mb_bits tools/mb_bits.hip && tools/mb_bits
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include "../trade-offs-in-distributed-tuplewise-estimation-and-learning_amd/csrc/bitcount.h"
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP %s @%d\n",hipGetErrorString(e),__LINE__); exit(1);}}while(0)

typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int kWave = 64, kBlock = 256, kNB = 20;

// ---- the packed-f32 loop of tools/mb_pk.hip
template <int HI>
__device__ __forceinline__ f2 gt_clamp(f2 x, unsigned long long nz2) {
  f2 t;
  if (HI)
    asm volatile("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] clamp" : "=v"(t) : "v"(x), "s"(nz2));
  else
    asm volatile("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] clamp" : "=v"(t) : "v"(x), "s"(nz2));
  return t;
}
__device__ __forceinline__ void acc_add(f2& a, f2 t) {
  asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(a) : "v"(t));
}

struct Shape {
  int n_shards, k, kp, tiles_x, zchunks, zc;
};

__device__ __forceinline__ bool item_of(const Shape& sh, int tile, int& s, int& x0, int& xe,
                                        int& z0, int& z1) {
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int item = blockIdx.x * (kBlock / kWave) + wid;
  const int per_shard = sh.tiles_x * sh.zchunks;
  s = item / per_shard;
  if (s >= sh.n_shards) return false;
  const int rem = item - s * per_shard, cz = rem / sh.tiles_x, tx = rem - cz * sh.tiles_x;
  x0 = s * sh.k + tx * tile;
  xe = (s + 1) * sh.k;
  z0 = s * sh.kp + cz * sh.zc;
  z1 = min(z0 + sh.zc, s * sh.kp + sh.k);
  return true;
}

template <int R>
__global__ __launch_bounds__(kBlock) void k_pk(const float* __restrict__ gx,
                                               const float* __restrict__ nzs, Shape sh,
                                               unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  int s, x0, xe, z0, z1;
  if (!item_of(sh, kWave * R, s, x0, xe, z0, z1)) return;
  f2 xv[R / 2], acc[R / 2];
#pragma unroll
  for (int p = 0; p < R / 2; ++p) {
    const int i0 = x0 + (2 * p) * kWave + lane, i1 = i0 + kWave;
    xv[p].x = i0 < xe ? gx[i0] : -3.0e7f;
    xv[p].y = i1 < xe ? gx[i1] : -3.0e7f;
    acc[p] = f2{0.f, 0.f};
  }
  const unsigned long long* __restrict__ zp = (const unsigned long long*)(nzs + z0);  // z0 even
  const int nz = z1 - z0;
  int j = 0;
  for (; j + 16 <= nz; j += 16) {
    unsigned long long zz[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) zz[u] = zp[j / 2 + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      f2 t[R / 2];
#pragma unroll
      for (int p = 0; p < R / 2; ++p) t[p] = gt_clamp<0>(xv[p], zz[u]);
#pragma unroll
      for (int p = 0; p < R / 2; ++p) acc_add(acc[p], t[p]);
#pragma unroll
      for (int p = 0; p < R / 2; ++p) t[p] = gt_clamp<1>(xv[p], zz[u]);
#pragma unroll
      for (int p = 0; p < R / 2; ++p) acc_add(acc[p], t[p]);
    }
  }
  for (; j < nz; ++j) {
    const unsigned long long zu = (unsigned long long)__float_as_uint(nzs[z0 + j]);
#pragma unroll
    for (int p = 0; p < R / 2; ++p) acc_add(acc[p], gt_clamp<0>(xv[p], zu));
  }
  unsigned long long tot = 0;
#pragma unroll
  for (int p = 0; p < R / 2; ++p) tot += (unsigned)acc[p].x + (unsigned)acc[p].y;
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, kWave);
  if (lane == 0 && tot) atomicAdd(out + s, tot);
}

// ---- the bit-sliced item of csrc/bitcount.h
template <int R>
__global__ __launch_bounds__(kBlock) void k_bits(const float* __restrict__ gx,
                                                 const float* __restrict__ nzs, Shape sh,
                                                 unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  int s, x0, xe, z0, z1;
  if (!item_of(sh, kWave * 32 * R, s, x0, xe, z0, z1)) return;
  unsigned long long tot = tw::bits_count_item<kNB, R>(gx, x0, xe, nzs, z0, z1, lane);
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, kWave);
  if (lane == 0 && tot) atomicAdd(out + s, tot);
}

// ---- pure issue probes: no loads, the z word from a loop-carried SGPR
__global__ __launch_bounds__(kBlock) void k_issue_bits(int iters, unsigned seed, unsigned* out) {
  uint32_t pl[4][kNB], acc[4] = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int b = 0; b < kNB; ++b) pl[r][b] = seed * (threadIdx.x + 7 * r + 31 * b + 1);
  unsigned z = __builtin_amdgcn_readfirstlane(seed);
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      z = z * 1664525u + 1013904223u;  // 2 SALU beside the NB s_bfe_i32
      uint32_t c[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) c[r] = pl[r][0] & tw::bits_mask(z, 0);
#pragma unroll
      for (int b = 1; b < kNB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] = tw::bits_carry(pl[r][b], tw::bits_mask(z, b), c[r]);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = tw::bits_popc_add(c[r], acc[r]);
    }
  }
  out[blockIdx.x * kBlock + threadIdx.x] = acc[0] + acc[1] + acc[2] + acc[3];
}
__global__ __launch_bounds__(kBlock) void k_issue_pk(int iters, float seed, float* out) {
  f2 x0 = {seed + threadIdx.x, seed}, x1 = x0 * 2.f, x2 = x0 * 3.f, x3 = x0 * 5.f;
  f2 a0 = {0, 0}, a1 = a0, a2 = a0, a3 = a0;
  unsigned long long z = (unsigned long long)__builtin_amdgcn_readfirstlane((int)seed) * 0x100000001ull;
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc_add(a0, gt_clamp<0>(x0, z)); acc_add(a1, gt_clamp<1>(x1, z));
      acc_add(a2, gt_clamp<0>(x2, z)); acc_add(a3, gt_clamp<1>(x3, z));
    }
  }
  out[blockIdx.x * kBlock + threadIdx.x] = a0.x + a1.y + a2.x + a3.y;
}

struct Config {
  const char* name;
  bool bits;
  int R, zc;
  std::vector<float> ms;
  bool ok = true;
};

static float launch(Config& c, const float* dx, const float* dz, int S, int k, int kp,
                    unsigned long long* dout, const std::vector<unsigned long long>& want,
                    hipEvent_t a, hipEvent_t b) {
  const int tile = c.bits ? kWave * 32 * c.R : kWave * c.R;
  Shape sh{S, k, kp, (k + tile - 1) / tile, (k + c.zc - 1) / c.zc, c.zc};
  const long items = (long)S * sh.tiles_x * sh.zchunks, blocks = (items + 3) / 4;
  float sum = 0;
  const int reps = 4;
  for (int r = -1; r < reps; ++r) {
    CK(hipMemsetAsync(dout, 0, S * 8));
    CK(hipEventRecord(a));
    if (c.bits && c.R == 2) hipLaunchKernelGGL(k_bits<2>, dim3(blocks), dim3(kBlock), 0, 0, dx, dz, sh, dout);
    else if (c.bits) hipLaunchKernelGGL(k_bits<4>, dim3(blocks), dim3(kBlock), 0, 0, dx, dz, sh, dout);
    else if (c.R == 8) hipLaunchKernelGGL(k_pk<8>, dim3(blocks), dim3(kBlock), 0, 0, dx, dz, sh, dout);
    else hipLaunchKernelGGL(k_pk<16>, dim3(blocks), dim3(kBlock), 0, 0, dx, dz, sh, dout);
    CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b));
    if (r >= 0) sum += ms;
  }
  std::vector<unsigned long long> got(S);
  CK(hipMemcpy(got.data(), dout, S * 8, hipMemcpyDeviceToHost));
  if (got != want) c.ok = false;
  return sum / reps;
}

int main() {
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  {  // issue probes, alternating
    const int blocks = 256 * 8, iters = 2048;
    void* o; CK(hipMalloc(&o, blocks * kBlock * 4));
    for (int rep = 0; rep < 3; ++rep) {
      float ms;
      CK(hipEventRecord(a));
      hipLaunchKernelGGL(k_issue_pk, dim3(blocks), dim3(kBlock), 0, 0, iters, 3.0f, (float*)o);
      CK(hipEventRecord(b)); CK(hipEventSynchronize(b)); CK(hipEventElapsedTime(&ms, a, b));
      double wi = (double)blocks * 4 * iters * 8 * 8;
      printf("issue probe packed: %.3f ms  %.3f VALU wave-instr/clk/CU @2.4GHz  %.3e pairs/s (64 per instr)\n",
             ms, wi / (ms * 1e-3) / 256 / 2.4e9, wi * 64 / (ms * 1e-3));
      CK(hipEventRecord(a));
      hipLaunchKernelGGL(k_issue_bits, dim3(blocks), dim3(kBlock), 0, 0, iters, 2654435761u, (unsigned*)o);
      CK(hipEventRecord(b)); CK(hipEventSynchronize(b)); CK(hipEventElapsedTime(&ms, a, b));
      wi = (double)blocks * 4 * iters * 2 * 4 * (kNB + 1);
      const double si = (double)blocks * 4 * iters * 2 * (kNB + 2);
      printf("issue probe bits R=4: %.3f ms  %.3f VALU + %.3f SALU wave-instr/clk/CU @2.4GHz  %.3e pairs/s (%.1f per VALU instr)\n",
             ms, wi / (ms * 1e-3) / 256 / 2.4e9, si / (ms * 1e-3) / 256 / 2.4e9,
             wi * 2048 / (kNB + 1) / (ms * 1e-3), 2048.0 / (kNB + 1));
    }
    CK(hipFree(o));
  }
  const int S = 64, k = 15625, n = S * k;
  const int kp = (k + 15) & ~15;
  std::vector<float> gx(n), nz((size_t)S * kp, 0.f);
  srand(7);
  for (int i = 0; i < n; ++i) gx[i] = (float)(rand() % 1000001);  // images in [0, 1e6]: 20 bits
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < k; ++i) nz[(size_t)s * kp + i] = -(float)(rand() % 1000001);
  gx[5] = -33554432.0f;                      // the "never" x image
  for (int i = 0; i < 64; ++i) gx[100 + i] = -nz[i];  // ties
  std::vector<unsigned long long> want(S, 0);
  for (int s = 0; s < S; ++s) {
    std::vector<float> zs(nz.begin() + (size_t)s * kp, nz.begin() + (size_t)s * kp + k);
    for (auto& v : zs) v = -v;
    std::sort(zs.begin(), zs.end());
    for (int i = 0; i < k; ++i)
      want[s] += std::lower_bound(zs.begin(), zs.end(), gx[s * k + i]) - zs.begin();
  }
  float *dx, *dz; unsigned long long* dout;
  CK(hipMalloc(&dx, n * 4)); CK(hipMalloc(&dz, (size_t)S * kp * 4)); CK(hipMalloc(&dout, S * 8));
  CK(hipMemcpy(dx, gx.data(), n * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dz, nz.data(), (size_t)S * kp * 4, hipMemcpyHostToDevice));
  std::vector<Config> cfg;
  cfg.push_back({"packed", false, 16, 528});
  cfg.push_back({"packed", false, 16, 1056});
  for (int R : {2, 4})
    for (int zc : {600, 1024, 2048, 4096}) cfg.push_back({"bits", true, R, zc});
  const int rounds = 7;
  for (int r = 0; r < rounds; ++r)  // every configuration once per round: packed and bits alternate
    for (auto& c : cfg) c.ms.push_back(launch(c, dx, dz, S, k, kp, dout, want, a, b));
  const double pairs = (double)S * k * k;
  double best_pk = 0, best_bits = 0;
  for (auto& c : cfg) {
    std::sort(c.ms.begin(), c.ms.end());
    const double med = c.ms[rounds / 2], lo = c.ms.front();
    const int tile = c.bits ? kWave * 32 * c.R : kWave * c.R;
    const long tiles_x = (k + tile - 1) / tile, zchunks = (k + c.zc - 1) / c.zc;
    // inner-loop VALU wave-instructions: per item and z, R/2 * 2 packed adds per z, or
    // R * (NB + 1) + 1 readlane (z rounded up to even per 64-group)
    double valu = 0;
    for (long cz = 0; cz < zchunks; ++cz) {
      const long nzc = std::min<long>(c.zc, k - cz * c.zc);
      valu += c.bits ? (double)((nzc + 1) / 2 * 2) * (c.R * (kNB + 1) + 1) : (double)nzc * c.R;
    }
    valu *= (double)S * tiles_x;
    const double rate = pairs / (med * 1e-3);
    (c.bits ? best_bits : best_pk) = std::max(c.bits ? best_bits : best_pk, rate);
    printf("%-6s R=%2d zc=%4d items=%6ld  median %.4f ms  best %.4f ms  %.3e pairs/s  %.1f pairs/VALU instr  %.3f VALU wave-instr/clk/CU @2.4GHz  %s\n",
           c.name, c.R, c.zc, (long)S * tiles_x * zchunks, med, lo, rate, pairs / valu,
           valu / (med * 1e-3) / 256 / 2.4e9, c.ok ? "counts OK" : "COUNTS DIFFER");
  }
  printf("g = best bit-sliced / best packed pairs/s = %.3f  (headline gain 1 / (0.06 + 0.94 / g) = %.3f)\n",
         best_bits / best_pk, 1.0 / (0.06 + 0.94 / (best_bits / best_pk)));
  return 0;
}
