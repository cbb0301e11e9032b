// Microbenchmark (design probe for csrc/mmd_perm.hip; not product code): the
// issue rate of v_mfma_f64_16x16x4_f64 on gfx950 with 1, 2, 4 and 8 independent accumulators,
// alone (one wave per SIMD) and beside a second wave per SIMD that runs eight independent
// v_fma_f64 chains — and that wave's v_fma_f64 rate alone and beside the matrix wave.
// One workgroup of 512 threads per CU: waves 0-3 (one per SIMD) issue the matrix instructions,
// waves 4-7 the vector ones; a role with 0 iterations returns at once.  Beside: the other role is
// given enough iterations to outlast the measured one.  Per configuration: the measured role's
// s_memtime ticks per instruction (wave 0 or 4 of every workgroup: median over workgroups) and
// the launch's event time per instruction of the measured role, in ns and in cycles at 2.4 GHz.
//   hipcc --offload-arch=gfx950 -O3 -o tools/mb_mfma_f64 tools/mb_mfma_f64.hip
//   tools/mb_mfma_f64 > profiles/mb_mfma_f64.log
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP %s @%d\n",hipGetErrorString(e),__LINE__); exit(1);}}while(0)

typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kWave = 64, kBlock = 512, kUnroll = 8, kChains = 8;

template <int NACC>
__global__ __launch_bounds__(kBlock) void k_mb(int mfma_iters, int fma_iters, double seed,
                                               double* __restrict__ out,
                                               long long* __restrict__ ticks) {
  const int wid = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  double res = 0.0;
  long long t0 = 0, t1 = 0;
  if (wid < 4) {
    if (mfma_iters == 0) return;
    const double a = seed + 1e-3 * lane, b = 1.0 - 1e-6 * lane;
    f64x4 acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
      acc[k] = f64x4{seed * k, 0.0, 1.0, 2.0};
      asm volatile("" : "+v"(acc[k]));
    }
    t0 = clock64();
    for (int i = 0; i < mfma_iters; ++i) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
#pragma unroll
        for (int k = 0; k < NACC; ++k)
          acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[k], 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < NACC; ++k) asm volatile("" : "+v"(acc[k]));
    t1 = clock64();
#pragma unroll
    for (int k = 0; k < NACC; ++k) res += acc[k][0] + acc[k][1] + acc[k][2] + acc[k][3];
  } else {
    if (fma_iters == 0) return;
    const double a = 0.999 + 1e-6 * lane, b = seed;
    double x[kChains];
#pragma unroll
    for (int k = 0; k < kChains; ++k) {
      x[k] = seed + k;
      asm volatile("" : "+v"(x[k]));
    }
    t0 = clock64();
    for (int i = 0; i < fma_iters; ++i) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
#pragma unroll
        for (int k = 0; k < kChains; ++k) x[k] = __builtin_fma(x[k], a, b);
    }
#pragma unroll
    for (int k = 0; k < kChains; ++k) asm volatile("" : "+v"(x[k]));
    t1 = clock64();
#pragma unroll
    for (int k = 0; k < kChains; ++k) res += x[k];
  }
  out[(size_t)blockIdx.x * kBlock + threadIdx.x] = res;
  if (lane == 0 && (wid == 0 || wid == 4)) ticks[blockIdx.x * 2 + wid / 4] = t1 - t0;
}

// The VALU form of the same product (lane = permutation, g a wave-uniform operand), at its best:
// no loads, the anchor's label bit hoisted, per pair one bit test of the point's label word, one
// select of 0.0 / 1.0 and one v_fma_f64 into one of four accumulators.  WAVES waves per SIMD.
__global__ __launch_bounds__(kBlock) void k_valu_form(int iters, int waves, double seed,
                                                      double* __restrict__ out,
                                                      long long* __restrict__ ticks) {
  const int wid = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  if (wid >= 4 * waves) return;
  const unsigned wp = 0x9E3779B9u * (lane + 1), wa = 0x85EBCA6Bu * (lane + 3);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const long long t0 = clock64();
  for (int i = 0; i < iters; ++i) {
    // g of the iteration's anchor row: wave-uniform (an SGPR pair)
    const double g = __longlong_as_double(((long long)__builtin_amdgcn_readfirstlane(
                         0x3FF00000 + (i & 1023)) << 32));
    const unsigned abit = (wa >> (i & 31)) & 1u;
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const unsigned b = (wp >> u) & abit;
      const double sdbl = __hiloint2double(b ? 0x3FF00000 : 0, 0);
      acc[u & 3] = __builtin_fma(g + 0.0 * u, sdbl, acc[u & 3]);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(acc[k]));
  const long long t1 = clock64();
  out[(size_t)blockIdx.x * kBlock + threadIdx.x] = (acc[0] + acc[1]) + (acc[2] + acc[3]) + seed;
  if (lane == 0 && wid == 0) ticks[blockIdx.x * 2] = t1 - t0;
}

struct Result { double ticks_per_instr, ns_per_instr; };

template <int NACC>
Result run(int cus, int mfma_iters, int fma_iters, bool measure_mfma, double* dout, long long* dticks) {
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  std::vector<long long> t(2 * cus);
  std::vector<double> per, ms_all;
  const double instr = measure_mfma ? (double)mfma_iters * kUnroll * NACC
                                    : (double)fma_iters * kUnroll * kChains;
  for (int rep = -1; rep < 5; ++rep) {
    CK(hipMemset(dticks, 0, 2 * cus * sizeof(long long)));
    CK(hipEventRecord(a));
    hipLaunchKernelGGL(k_mb<NACC>, dim3(cus), dim3(kBlock), 0, 0, mfma_iters, fma_iters, 1.5, dout, dticks);
    CK(hipGetLastError());
    CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b));
    if (rep < 0) continue;
    CK(hipMemcpy(t.data(), dticks, 2 * cus * sizeof(long long), hipMemcpyDeviceToHost));
    std::vector<long long> mine;
    for (int c = 0; c < cus; ++c) mine.push_back(t[2 * c + (measure_mfma ? 0 : 1)]);
    std::sort(mine.begin(), mine.end());
    per.push_back(mine[cus / 2] / instr);
    ms_all.push_back(ms);
  }
  std::sort(per.begin(), per.end()); std::sort(ms_all.begin(), ms_all.end());
  return {per[2], ms_all[2] * 1e6 / instr};
}

template <int NACC>
void config(int cus, double* dout, long long* dticks) {
  const int mi = 4096 / NACC, fi = 4096;  // about the same count of measured instructions
  // alone; beside a vector wave that outlasts it (4x the matrix wave's expected time)
  const Result alone = run<NACC>(cus, mi, 0, true, dout, dticks);
  const Result beside = run<NACC>(cus, mi, 8 * mi * NACC, true, dout, dticks);
  printf("mfma_f64_16x16x4 acc=%d  alone: %.2f ticks/instr, %.2f ns/instr (%.1f cyc @2.4GHz; launch incl.)"
         "  beside v_fma_f64: %.2f ticks/instr\n",
         NACC, alone.ticks_per_instr, alone.ns_per_instr, alone.ns_per_instr * 2.4, beside.ticks_per_instr);
  if (NACC == 4) {
    const Result falone = run<NACC>(cus, 0, fi, false, dout, dticks);
    const Result fbeside = run<NACC>(cus, 2 * fi / NACC, fi, false, dout, dticks);
    printf("v_fma_f64 (8 chains)  alone: %.2f ticks/instr, %.2f ns/instr (%.1f cyc @2.4GHz; launch incl.)"
           "  beside mfma acc=4: %.2f ticks/instr\n",
           falone.ticks_per_instr, falone.ns_per_instr, falone.ns_per_instr * 2.4, fbeside.ticks_per_instr);
  }
}

int main() {
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  printf("%s: %d CUs, clockRate %d kHz; one 512-thread workgroup per CU, waves 0-3 matrix, 4-7 vector\n",
         prop.name, cus, prop.clockRate);
  double* dout; long long* dticks;
  CK(hipMalloc(&dout, (size_t)cus * kBlock * 8)); CK(hipMalloc(&dticks, 2 * cus * sizeof(long long)));
  {  // what one s_memtime tick is: ticks of a known-length launch against its event time
    const Result r = run<4>(cus, 4096, 0, true, dout, dticks);
    printf("tick calibration: %.3f ticks/ns (s_memtime against device events, launch overhead incl.)\n",
           r.ticks_per_instr / r.ns_per_instr);
  }
  config<1>(cus, dout, dticks);
  config<2>(cus, dout, dticks);
  config<4>(cus, dout, dticks);
  config<8>(cus, dout, dticks);
  for (int waves = 1; waves <= 2; ++waves) {  // the VALU form: ticks per pair and 64 columns, per SIMD
    const int iters = 4096;
    std::vector<long long> t(2 * cus);
    std::vector<double> per;
    for (int rep = -1; rep < 5; ++rep) {
      hipLaunchKernelGGL(k_valu_form, dim3(cus), dim3(kBlock), 0, 0, iters, waves, 1.5, dout, dticks);
      CK(hipGetLastError()); CK(hipDeviceSynchronize());
      if (rep < 0) continue;
      CK(hipMemcpy(t.data(), dticks, 2 * cus * sizeof(long long), hipMemcpyDeviceToHost));
      std::vector<long long> mine;
      for (int c = 0; c < cus; ++c) mine.push_back(t[2 * c]);
      std::sort(mine.begin(), mine.end());
      per.push_back(mine[cus / 2] / ((double)iters * 32 * waves));
    }
    std::sort(per.begin(), per.end());
    printf("VALU form (lane = permutation: bit test, select, v_fma_f64 with a wave-uniform g), %d wave(s) per SIMD: "
           "%.2f ticks per pair and 64 columns per SIMD; the matrix form: 64 ticks per 1024 = 4.00\n",
           waves, per[2]);
  }
  printf("1024 multiply-adds per instruction: at T cycles per instruction a SIMD does 1024 / T a cycle\n");
  return 0;
}
