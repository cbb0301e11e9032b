// Microbenchmark (design probe for csrc/chain.hip's class count): the wide-digit
// loop with its low tables in VGPRs against the same loop reading the low-field carry from a
// 128-KiB LDS table shared by a block.  Both run the product's own statements
// (csrc/chainclass.h: bits_count_span_wide — TW_WD_BATCH(2) — and bits_count_runs_lds) on the
// same synthetic bag: two x groups of random 20-bit images, 256 classes of 61 z images each,
// every (bag, tile) the same data.  16 waves per CU either way: (a) blocks of 4 waves, one span
// of 8 runs per wave; (b) one block of 16 waves per (bag, tile), runs drawn from an LDS counter.
// A third argument v > 0 makes the runs unequal — 61 - v .. 61 + v images — and adds (c): (b)
// with the runs striped over the waves by entry index instead of drawn from the counter.
// Counts are checked against the host's bits_gt32.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I <package>/csrc tools/mb_ldsdigit.hip -o tools/mb_ldsdigit
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tw_common.h"
#include "chainclass.h"

#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP %s @%d\n",hipGetErrorString(e),__LINE__); exit(1);}}while(0)

using namespace tw;
constexpr int NB = 20, K = 8, kRuns = 256, kRunLen = 61, kSpan = 8;

// (a) the parent's loop: one wave per span of kSpan runs
__global__ __launch_bounds__(kBlock) void k_wide(const uint32_t* __restrict__ pw,
                                                 const uint32_t* __restrict__ zs,
                                                 const uint32_t* __restrict__ tab,
                                                 unsigned long long* __restrict__ out, int) {
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int item = blockIdx.x * (kBlock / kWave) + wid;
  const int q = item % (kRuns / kSpan);
  const unsigned long long t =
      wave_sum_u64(bits_count_span_wide<NB, K, 2>(pw, zs, tab + 2 * q * kSpan, kSpan, lane));
  if (lane == 0) atomicAdd(out + (item & 1023), t);
}

// (b) the LDS table: one block of 16 waves per (bag, tile)
__global__ __launch_bounds__(1024) void k_lds(const uint32_t* __restrict__ pw,
                                              const uint32_t* __restrict__ zs,
                                              const uint32_t* __restrict__ tab,
                                              unsigned long long* __restrict__ out, int stripe) {
  __shared__ uint2 table[kClassLdsEntries * 64];
  __shared__ uint32_t next;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  if (threadIdx.x == 0) next = 0;
  class_lds_build<NB>(table, pw, wid, lane, 2);
  __syncthreads();
  const uint32_t lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint2*)table;
  const unsigned long long t =
      wave_sum_u64(bits_count_runs_lds<NB, K>(lds, pw, zs, tab, kRuns, stripe ? nullptr : &next,
                                              lane, 2, wid, 16));
  if (lane == 0) atomicAdd(out + ((blockIdx.x * 16 + wid) & 1023), t);
}

static unsigned long long total(unsigned long long* d_out) {
  unsigned long long hv[1024], h = 0;
  CK(hipMemcpy(hv, d_out, sizeof hv, hipMemcpyDeviceToHost));
  for (int i = 0; i < 1024; ++i) h += hv[i];
  return h;
}

int main(int argc, char** argv) {
  const int tiles = argc > 1 ? atoi(argv[1]) : 2048;  // (bag, tile) pairs: 8 per CU
  const int reps = argc > 2 ? atoi(argv[2]) : 5, it = 10;
  const int vary = argc > 3 ? std::min(atoi(argv[3]), kRunLen - 1) : 0;
  srand(7);
  std::vector<uint32_t> img(2 * 2048), planes(2 * NB * 64), zc, zw, zl, tab(2 * kRuns);
  for (auto& v : img) v = (uint32_t)(rand() & ((1 << NB) - 1));
  // planes_word's layout inside a tile: word (r * NB + b) * 64 + lane, bit i = image 32 lane + i
  for (int r = 0; r < 2; ++r)
    for (int b = 0; b < NB; ++b)
      for (int l = 0; l < 64; ++l) {
        uint32_t w = 0;
        for (int i = 0; i < 32; ++i) w |= ((img[r * 2048 + l * 32 + i] >> b) & 1u) << i;
        planes[(r * NB + b) * 64 + l] = w;
      }
  unsigned long long expect = 0;
  for (int c = 0; c < kRuns; ++c) {
    const int len = kRunLen + (vary ? rand() % (2 * vary + 1) - vary : 0);
    const ClassRun run{(int64_t)zc.size(), len, (uint32_t)c};
    tab[2 * c] = class_entry_lo(run), tab[2 * c + 1] = class_entry_hi(run);
    for (int j = 0; j < len; ++j) {
      const uint32_t z = ((uint32_t)c << (NB - K)) | (uint32_t)(rand() & 0xFFF);
      zc.push_back(z), zw.push_back(class_wide_encode(z)), zl.push_back(class_lds_encode(z));
    }
  }
  const int kZ = (int)zc.size();
  for (int r = 0; r < 2; ++r)
    for (int l = 0; l < 64; ++l) {
      uint32_t pl[NB];
      for (int b = 0; b < NB; ++b) pl[b] = planes[(r * NB + b) * 64 + l];
      for (int j = 0; j < kZ; ++j) expect += (unsigned)__builtin_popcount(bits_gt32<NB>(pl, zc[j]));
    }
  uint32_t *d_pw, *d_zw, *d_zl, *d_tab;
  unsigned long long* d_out;
  // (64 words behind the images: the loops' batches read a few words past a run's end)
  CK(hipMalloc(&d_pw, planes.size() * 4));
  CK(hipMalloc(&d_zw, (kZ + 64) * 4));
  CK(hipMalloc(&d_zl, (kZ + 64) * 4));
  CK(hipMalloc(&d_tab, tab.size() * 4));
  CK(hipMalloc(&d_out, 8 * 1024));
  CK(hipMemset(d_zw, 0, (kZ + 64) * 4));
  CK(hipMemset(d_zl, 0, (kZ + 64) * 4));
  CK(hipMemcpy(d_pw, planes.data(), planes.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_zw, zw.data(), kZ * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_zl, zl.data(), kZ * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const double cus = prop.multiProcessorCount, mhz = prop.clockRate / 1e3;
  printf("device: %s, %d CUs, %.0f MHz (nominal: the rates below assume it)\n", prop.name,
         prop.multiProcessorCount, mhz);
  const dim3 ga((unsigned)(tiles * (kRuns / kSpan) / (kBlock / kWave))), gb((unsigned)tiles);
  auto run = [&](int form, bool check) {  // 0: (a), 1: (b), 2: (c)
    const bool lds = form > 0;
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    CK(hipMemset(d_out, 0, 8 * 1024));
    CK(hipEventRecord(a));
    for (int i = 0; i < it; ++i) {
      if (lds)
        hipLaunchKernelGGL(k_lds, gb, dim3(1024), 0, 0, d_pw, d_zl, d_tab, d_out, form == 2);
      else
        hipLaunchKernelGGL(k_wide, ga, dim3(kBlock), 0, 0, d_pw, d_zw, d_tab, d_out, 0);
    }
    CK(hipGetLastError());
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    float ms;
    CK(hipEventElapsedTime(&ms, a, b));
    const unsigned long long h = total(d_out);
    const double per = ms / it, zwave = (double)tiles * kZ;  // z images x (bag, tile)
    const double ns_z = per * 1e6 / zwave * cus;              // per z and CU
    const int valu = lds ? 5 : 8;
    if (check)
      printf("%-18s %8.4f ms/launch  %6.3f ns per z and CU  loop VALU %d/z: %.3f wave-instr/clk/CU  %s\n",
             form == 2 ? "(c) lds, striped" : lds ? "(b) lds table" : "(a) wide VGPR", per, ns_z, valu,
             valu * zwave / cus / (per * 1e-3 * mhz * 1e6),
             h == expect * tiles * it ? "count ok" : "COUNT MISMATCH");
    return per;
  };
  run(0, false), run(1, false);  // warm-up
  std::vector<double> ta, tb, tc;
  for (int r = 0; r < reps; ++r) {
    ta.push_back(run(0, true));
    tb.push_back(run(1, true));
    if (vary) tc.push_back(run(2, true));
  }
  std::sort(ta.begin(), ta.end()), std::sort(tb.begin(), tb.end()), std::sort(tc.begin(), tc.end());
  if (vary)
    printf("runs of %d +- %d images: (c) striped median %.4f ms, spread %.4f; c/b = %.3f\n", kRunLen,
           vary, tc[reps / 2], tc.back() - tc.front(), tc[reps / 2] / tb[reps / 2]);
  printf("(a) median %.4f ms, spread %.4f; (b) median %.4f ms, spread %.4f; b/a = %.3f\n",
         ta[reps / 2], ta.back() - ta.front(), tb[reps / 2], tb.back() - tb.front(),
         tb[reps / 2] / ta[reps / 2]);
  return 0;
}
