// Element access and launch grid shared by the block decompositions (mpse_qr.hip, mpse_qr2.hip, mpse_svd.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// one element of a real (double) or complex (double2) array, always handled as double2
template <bool CPLX>
struct Cx;
template <>
struct Cx<true> {
  static constexpr int E = 2;
  __device__ static double2 ld(const double* p, long long i) { return reinterpret_cast<const double2*>(p)[i]; }
  __device__ static void st(double* p, long long i, double2 v) { reinterpret_cast<double2*>(p)[i] = v; }
};
template <>
struct Cx<false> {
  static constexpr int E = 1;
  __device__ static double2 ld(const double* p, long long i) { return make_double2(p[i], 0.0); }
  __device__ static void st(double* p, long long i, double2 v) { p[i] = v.x; }
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) {  // conj(a) * b
  return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}

// workgroups of 256 threads for an elementwise grid-stride launch over n elements
inline int ew_blocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace
