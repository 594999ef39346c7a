// Vector kernels that both mpse_vec.hip (the exported BLAS-1 entry points) and mpse_lanczos.hip (the Lanczos drivers)
// launch, and the grid of their elementwise launches.
#pragma once
#include "mpse_device.h"

namespace {

// partial[b] = sum over this block's elements of conj(x) * y
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_dot_partial(const double* __restrict__ x, const double* __restrict__ y,
                                                             long long n, double* __restrict__ partial,
                                                             const int* __restrict__ done) {
  if (done && *done) return;
  double re = 0, im = 0;
  const long long stride = (long long)gridDim.x * RED_THREADS;
  if (CPLX) {
    // two 16-byte loads per operand in flight per thread (the loop is HBM-latency bound otherwise)
    const double2* x2 = reinterpret_cast<const double2*>(x);
    const double2* y2 = reinterpret_cast<const double2*>(y);
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += 2 * stride) {
      const long long i1 = i + stride;
      const bool h1 = i1 < n;
      const double2 a0 = x2[i], b0 = y2[i];
      const double2 a1 = h1 ? x2[i1] : make_double2(0.0, 0.0), b1 = h1 ? y2[i1] : make_double2(0.0, 0.0);
      re += a0.x * b0.x + a0.y * b0.y;
      im += a0.x * b0.y - a0.y * b0.x;
      re += a1.x * b1.x + a1.y * b1.y;
      im += a1.x * b1.y - a1.y * b1.x;
    }
  } else {
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) re += x[i] * y[i];
  }
  block_allsum2(re, im);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = re;
    partial[2 * blockIdx.x + 1] = im;
  }
}

__global__ __launch_bounds__(RED_THREADS) void k_reduce_final(const double* __restrict__ partial, int nb,
                                                              double* __restrict__ out, const int* __restrict__ done) {
  if (done && *done) return;
  double re = 0, im = 0;
  for (int i = threadIdx.x; i < nb; i += RED_THREADS) {
    re += partial[2 * i];
    im += partial[2 * i + 1];
  }
  block_allsum2(re, im);
  if (threadIdx.x == 0) {
    out[0] = re;
    out[1] = im;
  }
}

template <bool CPLX>
__global__ void k_scal(double* x, long long n, double ar, double ai) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (CPLX) {
      double2 v = reinterpret_cast<double2*>(x)[i];
      reinterpret_cast<double2*>(x)[i] = make_double2(ar * v.x - ai * v.y, ar * v.y + ai * v.x);
    } else {
      x[i] *= ar;
    }
  }
}

inline int ew_blocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace
