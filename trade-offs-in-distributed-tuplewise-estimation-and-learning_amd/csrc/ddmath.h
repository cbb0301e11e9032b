// ddmath.h — double-double sums (two-sum / fma two-product) shared by hingesort.hip (the sorted
// hinge sum) and selfsorted.hip (the sorted Gini sum): a value is hi + lo with |lo| <= ulp(hi)/2.
#pragma once
#include "tw_common.h"

namespace tw {

struct ddv {
  double hi, lo;
};
__device__ __forceinline__ ddv two_sum(double a, double b) {
  const double s = a + b;
  const double bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ ddv quick_two_sum(double a, double b) {
  const double s = a + b;
  return {s, b - (s - a)};
}
// a * b exactly: the rounded product and its error (no overflow / underflow)
__device__ __forceinline__ ddv two_prod(double a, double b) {
  const double p = a * b;
  return {p, __fma_rn(a, b, -p)};
}
__device__ __forceinline__ ddv dd_add(ddv a, ddv b) {
  ddv s = two_sum(a.hi, b.hi);
  const ddv t = two_sum(a.lo, b.lo);
  s.lo += t.hi;
  s = quick_two_sum(s.hi, s.lo);
  s.lo += t.lo;
  return quick_two_sum(s.hi, s.lo);
}
__device__ __forceinline__ ddv dd_neg(ddv a) { return {-a.hi, -a.lo}; }
// a * c for an exact small integer c (as a double)
__device__ __forceinline__ ddv dd_mul_d(ddv a, double c) {
  const double p = a.hi * c;
  const double e = __fma_rn(a.hi, c, -p);
  return quick_two_sum(p, e + a.lo * c);
}
__device__ __forceinline__ ddv dd_shfl_xor(ddv a, int m) {
  return {__shfl_xor(a.hi, m, kWave), __shfl_xor(a.lo, m, kWave)};
}

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

}  // namespace tw
