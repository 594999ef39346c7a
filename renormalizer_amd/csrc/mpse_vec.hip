// Vector algebra behind the exported BLAS-1 entry points (HBM-bound, wavefront-shuffle reductions).
//
// Reductions are two-stage with a grid size that depends on n only and fixed summation
// order, so dot products / norms are bitwise reproducible run to run.
#include <cmath>

#include "mpse_internal.h"
#include "mpse_vec_kernels.h"

namespace {

template <bool CPLX>
__global__ void k_axpy(double* y, const double* __restrict__ x, long long n, double ar, double ai) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (CPLX) {
      const double2 v = reinterpret_cast<const double2*>(x)[i];
      double2 o = reinterpret_cast<double2*>(y)[i];
      o.x += ar * v.x - ai * v.y;
      o.y += ar * v.y + ai * v.x;
      reinterpret_cast<double2*>(y)[i] = o;
    } else {
      y[i] += ar * x[i];
    }
  }
}

__global__ void k_cast(double* dst, const double* __restrict__ src, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    reinterpret_cast<double2*>(dst)[i] = make_double2(src[i], 0.0);
}

__global__ void k_conj(double* x, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[2 * i + 1] = -x[2 * i + 1];
}

// dst = src * s   (real scale)
__global__ void k_scale_into(double* dst, const double* __restrict__ src, long long n_doubles, double s) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_doubles; i += stride) dst[i] = src[i] * s;
}

// partial sums of |x_i|^2 / (atol + rtol max(|y1_i|, |y2_i|))^2  (error norm of an embedded Runge-Kutta pair)
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_scaled_sq(const double* __restrict__ x, const double* __restrict__ y1,
                                                           const double* __restrict__ y2, long long n, double rtol,
                                                           double atol, double* __restrict__ partial) {
  double s = 0, zero = 0;
  const long long stride = (long long)gridDim.x * RED_THREADS;
  for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) {
    double ax, a1, a2;
    if (CPLX) {
      ax = hypot(x[2 * i], x[2 * i + 1]);
      a1 = hypot(y1[2 * i], y1[2 * i + 1]);
      a2 = hypot(y2[2 * i], y2[2 * i + 1]);
    } else {
      ax = fabs(x[i]);
      a1 = fabs(y1[i]);
      a2 = fabs(y2[i]);
    }
    const double q = ax / (atol + rtol * fmax(a1, a2));
    s += q * q;
  }
  block_allsum2(s, zero);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = s;
    partial[2 * blockIdx.x + 1] = 0.0;
  }
}

// x[i] *= m[i]  (real mask / weights on a real or complex vector)
template <bool CPLX>
__global__ void k_mul_real(double* x, const double* __restrict__ m, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (CPLX) {
      double2 v = reinterpret_cast<double2*>(x)[i];
      v.x *= m[i];
      v.y *= m[i];
      reinterpret_cast<double2*>(x)[i] = v;
    } else {
      x[i] *= m[i];
    }
  }
}

// Davidson preconditioner out = r / (hdiag - e + shift), zero where mask == 0  (mps/gs.py:530-531)
template <bool CPLX>
__global__ void k_precond(double* out, const double* __restrict__ r, const double* __restrict__ hdiag,
                          const double* __restrict__ mask, long long n, double e, double shift) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double w = (mask && mask[i] == 0.0) ? 0.0 : 1.0 / (hdiag[i] - e + shift);
    if (CPLX) {
      const double2 v = reinterpret_cast<const double2*>(r)[i];
      reinterpret_cast<double2*>(out)[i] = make_double2(v.x * w, v.y * w);
    } else {
      out[i] = r[i] * w;
    }
  }
}

__global__ void k_real_part(double* out, const double* __restrict__ z, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = z[2 * i];
}

int read_scalar2(mpse_ctx* ctx, const double* dsrc, double* a, double* b) {
  MPSE_TRY(publish_and_wait(ctx, dsrc, 2, mpse_ctx::PIN_SCALAR2));
  if (ctx->prof_pending.size() > 2048) prof_drain(ctx);
  if (a) *a = ctx->pinned[mpse_ctx::PIN_SCALAR2];
  if (b) *b = ctx->pinned[mpse_ctx::PIN_SCALAR2 + 1];
  return MPSE_OK;
}

}  // namespace

int dotc_sync(mpse_ctx* ctx, int dtype, const void* x, const void* y, int64_t n, double* re, double* im) {
  const bool cplx = dtype == MPSE_C128;
  const int nb = red_blocks(n * (cplx ? 2 : 1));
  double* partial = ctx->dscratch;             // 2*nb doubles
  double* result = ctx->dscratch + 2 * RED_MAX_BLOCKS;
  MPSE_LAUNCH_TF(ctx, cplx, k_dot_partial, dim3(nb), dim3(RED_THREADS), (const double*)x, (const double*)y, (long long)n,
                 partial, (const int*)nullptr);
  hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(RED_THREADS), 0, ctx->stream, partial, nb, result, (const int*)nullptr);
  MPSE_HIP(ctx, hipGetLastError());
  return read_scalar2(ctx, result, re, im);
}

extern "C" {

int mpse_cast_f64_to_c128(mpse_ctx* ctx, void* dst, const void* src, int64_t n) {
  if (!ctx || (n && (!dst || !src))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (n <= 0) return MPSE_OK;
  wsite_written(ctx, dst, size_t(n) * 16);
  hipLaunchKernelGGL(k_cast, dim3(ew_blocks(n)), dim3(256), 0, ctx->stream, (double*)dst, (const double*)src,
                     (long long)n);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

int mpse_conj_inplace(mpse_ctx* ctx, void* x, int64_t n) {
  if (!ctx || (n && !x)) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (n <= 0) return MPSE_OK;
  wsite_written(ctx, x, size_t(n) * 16);
  hipLaunchKernelGGL(k_conj, dim3(ew_blocks(n)), dim3(256), 0, ctx->stream, (double*)x, (long long)n);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

int mpse_scal(mpse_ctx* ctx, int dtype, void* x, int64_t n, double a_re, double a_im) {
  if (!ctx || (n && !x)) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (n <= 0) return MPSE_OK;
  wsite_written(ctx, x, size_t(n) * dtype_size(dtype));
  // (the real kernels never read the imaginary part of the factor)
  MPSE_LAUNCH_TF_CHK(ctx, dtype == MPSE_C128, k_scal, dim3(ew_blocks(n)), dim3(256), (double*)x, (long long)n, a_re, a_im);
  return MPSE_OK;
}

int mpse_axpy(mpse_ctx* ctx, int dtype, void* y, const void* x, int64_t n, double a_re, double a_im) {
  if (!ctx || (n && (!x || !y))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (n <= 0) return MPSE_OK;
  wsite_written(ctx, y, size_t(n) * dtype_size(dtype));
  MPSE_LAUNCH_TF_CHK(ctx, dtype == MPSE_C128, k_axpy, dim3(ew_blocks(n)), dim3(256), (double*)y, (const double*)x,
                     (long long)n, a_re, a_im);
  return MPSE_OK;
}

int mpse_mul_real(mpse_ctx* ctx, int dtype, void* x, const void* m_f64, int64_t n) {
  if (!ctx || (n && (!x || !m_f64))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (n <= 0) return MPSE_OK;
  wsite_written(ctx, x, size_t(n) * dtype_size(dtype));
  MPSE_LAUNCH_TF_CHK(ctx, dtype == MPSE_C128, k_mul_real, dim3(ew_blocks(n)), dim3(256), (double*)x, (const double*)m_f64,
                     (long long)n);
  return MPSE_OK;
}

int mpse_davidson_precond(mpse_ctx* ctx, int dtype, void* out, const void* r, const void* hdiag_f64,
                          const void* mask_f64, int64_t n, double e, double shift) {
  if (!ctx || (n && (!out || !r || !hdiag_f64))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (n <= 0) return MPSE_OK;
  wsite_written(ctx, out, size_t(n) * dtype_size(dtype));
  MPSE_LAUNCH_TF_CHK(ctx, dtype == MPSE_C128, k_precond, dim3(ew_blocks(n)), dim3(256), (double*)out, (const double*)r,
                     (const double*)hdiag_f64, (const double*)mask_f64, (long long)n, e, shift);
  return MPSE_OK;
}

int mpse_real_part(mpse_ctx* ctx, void* out_f64, const void* z_c128, int64_t n) {
  if (!ctx || (n && (!out_f64 || !z_c128))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (n <= 0) return MPSE_OK;
  wsite_written(ctx, out_f64, size_t(n) * 8);
  hipLaunchKernelGGL(k_real_part, dim3(ew_blocks(n)), dim3(256), 0, ctx->stream, (double*)out_f64,
                     (const double*)z_c128, (long long)n);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

int mpse_dotc(mpse_ctx* ctx, int dtype, const void* x, const void* y, int64_t n, double* out_host) {
  if (!ctx || !out_host || (n && (!x || !y))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  out_host[0] = out_host[1] = 0.0;
  if (n <= 0) return MPSE_OK;
  return dotc_sync(ctx, dtype, x, y, n, &out_host[0], &out_host[1]);
}

int mpse_scaled_rms(mpse_ctx* ctx, int dtype, const void* x, const void* y1, const void* y2, int64_t n, double rtol,
                    double atol, double* out_host) {
  if (!ctx || !out_host || (n && (!x || !y1 || !y2))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  out_host[0] = 0.0;
  if (n <= 0) return MPSE_OK;
  const int nb = red_blocks(n);
  double* partial = ctx->dscratch;
  double* result = ctx->dscratch + 2 * RED_MAX_BLOCKS;
  MPSE_LAUNCH_TF(ctx, dtype == MPSE_C128, k_scaled_sq, dim3(nb), dim3(RED_THREADS), (const double*)x, (const double*)y1,
                 (const double*)y2, (long long)n, rtol, atol, partial);
  hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(RED_THREADS), 0, ctx->stream, partial, nb, result, (const int*)nullptr);
  MPSE_HIP(ctx, hipGetLastError());
  double re = 0, im = 0;
  MPSE_TRY(read_scalar2(ctx, result, &re, &im));
  out_host[0] = sqrt(re / double(n));
  return MPSE_OK;
}

int mpse_nrm2(mpse_ctx* ctx, int dtype, const void* x, int64_t n, double* out_host) {
  if (!ctx || !out_host || (n && !x)) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  out_host[0] = 0.0;
  if (n <= 0) return MPSE_OK;
  double re = 0, im = 0;
  MPSE_TRY(dotc_sync(ctx, dtype, x, x, n, &re, &im));
  out_host[0] = sqrt(re);
  return MPSE_OK;
}

}  // extern "C"
