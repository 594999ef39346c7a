// The device-resident Lanczos exponential that replaces lib/krylov/krylov.py:27-82: the synchronous solve, the
// asynchronous one (iterations enqueued ahead of a decision that falls on the device) and the batched one
// (mpse_expm_lanczos_batch), with their kernels.
#include <cmath>
#include <complex>
#include <cstdlib>
#include <utility>

#include "mpse_internal.h"
#include "mpse_lanczos_plan.h"
#include "mpse_vec_kernels.h"

namespace {

// member_ptr (mpse_internal.h) for the kernels of this file, as pointer arithmetic.  Through member_ptr's round trip
// over an integer the compiler no longer knows that a kernel argument points to global memory and issues flat loads and
// stores: with it the merged kernels were slower than the single forms they replace (k_lincomb_dev +13 %,
// k_lanczos_update_u +5 % at the headline's sizes, profiles/lanczos_one_driver.md).  Null stays null.
template <class T>
__device__ __forceinline__ T* lz_member(T* p, unsigned m, long long mstride) {
  using Byte = std::conditional_t<std::is_const<T>::value, const char, char>;
  return p ? reinterpret_cast<T*>(reinterpret_cast<Byte*>(p) + (long long)m * mstride) : p;
}

// dst = src / sqrt(b2) where b2 = sum of the nb partials of the preceding norm kernel; block 0 also stores b2
// (and the unused imaginary slot) to b2_out for the host and for the next recurrence step.
// VEC: 16-byte accesses, two per operand in flight per thread (needs 16-byte aligned vectors of even length - always
// the case for complex128); the plain path serves odd-length real vectors.
template <bool VEC>
__global__ __launch_bounds__(RED_THREADS) void k_scale_into_dev(double* dst, const double* __restrict__ src,
                                                                long long n_doubles,
                                                                const double* __restrict__ partial, int nb,
                                                                double* __restrict__ b2_out,
                                                                const int* __restrict__ done) {
  if (done && *done) return;
  double b2, im;
  sum_partials(partial, nb, b2, im);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    b2_out[0] = b2;
    b2_out[1] = im;
  }
  const double s = 1.0 / sqrt(b2);
  const long long stride = (long long)gridDim.x * blockDim.x;
  if (VEC) {
    const long long n2 = n_doubles >> 1;
    double2* d2 = reinterpret_cast<double2*>(dst);
    const double2* s2 = reinterpret_cast<const double2*>(src);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += 2 * stride) {
      const long long i1 = i + stride;
      const bool h1 = i1 < n2;
      const double2 a0 = s2[i];
      const double2 a1 = h1 ? s2[i1] : make_double2(0.0, 0.0);
      d2[i] = make_double2(a0.x * s, a0.y * s);
      if (h1) d2[i1] = make_double2(a1.x * s, a1.y * s);
    }
  } else {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_doubles; i += stride) dst[i] = src[i] * s;
  }
}

// Lanczos three-term update fused with the norm: w -= a*v1 + b*v0 ; partial = sum |w|^2
// (lib/krylov/krylov.py:70-71).  a = *ap and b = sqrt(*b2p) are read from device memory so that the
// recurrence never waits for the host.  VEC as above.
template <bool VEC>
__global__ __launch_bounds__(RED_THREADS) void k_lanczos_update(double* __restrict__ w, const double* __restrict__ v1,
                                                                const double* __restrict__ v0, long long n_doubles,
                                                                const double* __restrict__ a_partial, int a_nb,
                                                                double* __restrict__ a_out,
                                                                const double* __restrict__ b2p,
                                                                double* __restrict__ partial,
                                                                const int* __restrict__ done) {
  if (done && *done) return;
  // a = Re <w, v1>: summed here from the partials of the preceding k_dot_partial; block 0 records it
  double a, a_im;
  sum_partials(a_partial, a_nb, a, a_im);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a_out[0] = a;
    a_out[1] = a_im;
  }
  const double b = v0 ? sqrt(*b2p) : 0.0;
  double s = 0, zero = 0;
  const long long stride = (long long)gridDim.x * RED_THREADS;
  if (VEC) {
    const long long n2 = n_doubles >> 1;
    double2* w2 = reinterpret_cast<double2*>(w);
    const double2* p1 = reinterpret_cast<const double2*>(v1);
    const double2* p0 = reinterpret_cast<const double2*>(v0);
    const double2 z = make_double2(0.0, 0.0);
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n2; i += 2 * stride) {
      const long long i1 = i + stride;
      const bool h1 = i1 < n2;
      const double2 wa = w2[i], va = p1[i], ua = v0 ? p0[i] : z;
      const double2 wb = h1 ? w2[i1] : z, vb = h1 ? p1[i1] : z, ub = (h1 && v0) ? p0[i1] : z;
      const double2 xa = make_double2(wa.x - (a * va.x + b * ua.x), wa.y - (a * va.y + b * ua.y));
      const double2 xb = make_double2(wb.x - (a * vb.x + b * ub.x), wb.y - (a * vb.y + b * ub.y));
      w2[i] = xa;
      s += xa.x * xa.x + xa.y * xa.y;
      if (h1) {
        w2[i1] = xb;
        s += xb.x * xb.x + xb.y * xb.y;
      }
    }
  } else {
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n_doubles; i += stride) {
      double t = a * v1[i];
      if (v0) t += b * v0[i];
      const double x = w[i] - t;
      w[i] = x;
      s += x * x;
    }
  }
  block_allsum2(s, zero);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = s;
    partial[2 * blockIdx.x + 1] = 0.0;
  }
}

// Lanczos step on an UNNORMALISED basis (asynchronous solve): the Krylov vectors are kept as U_j = v_j / s_j with
// s_0 = 1 / |C|, s_{j+1} = 1 / beta_j, so that no separate normalisation pass over the vector is needed:
//   y = H U_j (in),  alpha_j = s_j^2 Re <y, U_j>,  w = s_j y - alpha_j s_j U_j - beta_{j-1} s_{j-1} U_{j-1} -> U_{j+1} (out)
// s_j^2 = 1 / sum(cur_partial) (the |U_j|^2 partials of the previous step; block 0 records the sum at cur_out),
// s_{j-1}^2 = 1 / *prev2 (recorded one step earlier).  Partials of |w|^2 go to `partial` (a different area than
// cur_partial: blocks read all of those before any block of the NEXT step overwrites them).
template <bool VEC>
// The matvec result arrives as the sum of nparts tensors y, y + part_stride, .. (doubles): the K slices of a split
// product or the halves of halved tiles (mpse_gemm.hip), added here in slice order instead of by a launch of their own
__device__ __forceinline__ void lanczos_update_u(double* __restrict__ u_next, const double* __restrict__ y, int nparts,
                                                 long long part_stride, const double* __restrict__ u1,
                                                 const double* __restrict__ u0, long long n_doubles,
                                                 const double* __restrict__ a_partial, int a_nb, double* __restrict__ a_out,
                                                 const double* __restrict__ cur_partial, int cur_nb,
                                                 double* __restrict__ cur_out, const double* __restrict__ prev2,
                                                 double* __restrict__ partial, const int* __restrict__ stop,
                                                 const unsigned long long* __restrict__ pmask, int prow, int ptiles,
                                                 const unsigned char* __restrict__ cmask, int crow, int ckw) {
  // pmask (complex vectors, VEC): the parts hold only some 16 x 16 tiles of the result viewed as rows of prow elements
  // (fused 0-site matvec, mpse_heff0.hip): word [tile row * ptiles + tile column], bit s = part s holds the tile; the
  // parts named there are added in part order, the others were never written.
  // cmask (complex vectors, VEC, no pmask): the caller's structural pattern of the centre (mpse_expm_centre_mask; rows of
  // crow elements, crow a multiple of 64, byte [(column / 64) * ckw + row / 16]): every vector of the solve is exactly
  // zero in the tiles it leaves out - nothing is read there and zeros are written (a wave works on 64 consecutive
  // elements of one row: the test is uniform over the wave)
  if (*stop) return;
  // The first pair of elements of this thread is requested BEFORE the scalars of the step are summed: its loads (mask
  // word, parts, U_j, U_{j-1}) do not depend on them, and the two block reductions of sum_partials otherwise stand in
  // front of every trip to memory of a kernel that is nothing but such trips.  Same arithmetic, same order.
  const long long stride = (long long)gridDim.x * RED_THREADS;
  const long long n2v = n_doubles >> 1;
  const double2 zz0 = make_double2(0.0, 0.0);
  struct Pair {
    double2 ya, yb, va, ua, vb, ub;
    bool h1;
  };
  auto fetch = [&](long long i) {
    Pair q;
    const double2* py = reinterpret_cast<const double2*>(y);
    const double2* p1 = reinterpret_cast<const double2*>(u1);
    const double2* p0 = reinterpret_cast<const double2*>(u0);
    const long long i1 = i + stride;
    q.h1 = i1 < n2v;
    bool la = true, lb = q.h1;      // element i / i1 lies in a tile the centre mask keeps (always, without a mask)
    if (pmask) {
      auto gather = [&](long long e) {
        const unsigned ee = (unsigned)e, row = ee / (unsigned)prow, col = ee - row * (unsigned)prow;
        unsigned long long m = pmask[(row >> 4) * ptiles + (col >> 4)];
        double2 acc = zz0;
        while (m) {          // four parts per round: their loads are in flight together, added in part order
          int sp[4];
          double2 t[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            sp[u] = m ? __builtin_ctzll(m) : -1;
            m &= m - (m ? 1 : 0);
            t[u] = sp[u] >= 0 ? py[(long long)sp[u] * (part_stride >> 1) + e] : zz0;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) acc.x += t[u].x, acc.y += t[u].y;
        }
        return acc;
      };
      q.ya = gather(i);
      q.yb = q.h1 ? gather(i1) : zz0;
    } else {
      // (one arithmetic path with and without the mask: the same expression trees, so the same fused multiply-adds)
      if (cmask) {
        auto live = [&](long long e) {
          const unsigned ee = (unsigned)e, row = ee / (unsigned)crow, col = ee - row * (unsigned)crow;
          return cmask[(col >> 6) * ckw + (row >> 4)] != 0;
        };
        la = live(i);
        lb = q.h1 && live(i1);
      }
      q.ya = la ? py[i] : zz0, q.yb = lb ? py[i1] : zz0;
      for (int s = 1; s < nparts; ++s) {
        const double2* ps = py + s * (part_stride >> 1);
        const double2 ta = la ? ps[i] : zz0, tb = lb ? ps[i1] : zz0;
        q.ya.x += ta.x, q.ya.y += ta.y, q.yb.x += tb.x, q.yb.y += tb.y;
      }
    }
    q.va = la ? p1[i] : zz0, q.ua = (la && u0) ? p0[i] : zz0;
    q.vb = lb ? p1[i1] : zz0, q.ub = (lb && u0) ? p0[i1] : zz0;
    return q;
  };
  const long long i_first = (long long)blockIdx.x * RED_THREADS + threadIdx.x;
  Pair first;
  first.h1 = false;
  if (VEC && i_first < n2v) first = fetch(i_first);
  asm volatile("" ::: "memory");
  double araw, a_im, cur2, z;
  sum_partials(a_partial, a_nb, araw, a_im);
  sum_partials(cur_partial, cur_nb, cur2, z);
  const double s1sq = 1.0 / cur2, s1 = sqrt(s1sq);
  const double a = araw * s1sq;                       // alpha_j
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a_out[0] = a;
    a_out[1] = a_im * s1sq;
    cur_out[0] = cur2;                                // |C|^2 (j == 0) or beta_{j-1}^2
    cur_out[1] = 0.0;
  }
  const double c_y = s1, c_1 = a * s1;
  const double c_0 = u0 ? sqrt(cur2) / sqrt(*prev2) : 0.0;   // beta_{j-1} s_{j-1}
  double s = 0, zero = 0;
  if (VEC) {
    double2* o2 = reinterpret_cast<double2*>(u_next);
    for (long long i = i_first; i < n2v; i += 2 * stride) {
      const Pair q = i == i_first ? first : fetch(i);
      const long long i1 = i + stride;
      const double2 xa = make_double2(c_y * q.ya.x - (c_1 * q.va.x + c_0 * q.ua.x), c_y * q.ya.y - (c_1 * q.va.y + c_0 * q.ua.y));
      const double2 xb = make_double2(c_y * q.yb.x - (c_1 * q.vb.x + c_0 * q.ub.x), c_y * q.yb.y - (c_1 * q.vb.y + c_0 * q.ub.y));
      o2[i] = xa;
      s += xa.x * xa.x + xa.y * xa.y;
      if (q.h1) {
        o2[i1] = xb;
        s += xb.x * xb.x + xb.y * xb.y;
      }
    }
  } else {
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n_doubles; i += stride) {
      double t = c_1 * u1[i];
      if (u0) t += c_0 * u0[i];
      double yv = y[i];
      for (int s = 1; s < nparts; ++s) yv += y[s * part_stride + i];
      const double x = c_y * yv - t;
      u_next[i] = x;
      s += x * x;
    }
  }
  block_allsum2(s, zero);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = s;
    partial[2 * blockIdx.x + 1] = 0.0;
  }
}
// Member blockIdx.y of a launch set (a single solve: one member): every per-member pointer at its member-0 address +
// blockIdx.y * mstride bytes (one slab per launch set).  The part and centre masks are the same for all members.
template <bool VEC>
__global__ __launch_bounds__(RED_THREADS) void k_lanczos_update_u(double* u_next, const double* y, int nparts,
                                                                  long long part_stride, const double* u1,
                                                                  const double* u0, long long n_doubles,
                                                                  const double* a_partial, int a_nb, double* a_out,
                                                                  const double* cur_partial, int cur_nb,
                                                                  double* cur_out, const double* prev2,
                                                                  double* partial, const int* stop,
                                                                  const unsigned long long* __restrict__ pmask,
                                                                  int prow, int ptiles,
                                                                  const unsigned char* __restrict__ cmask, int crow,
                                                                  int ckw, long long mstride) {
  const unsigned m = blockIdx.y;
  lanczos_update_u<VEC>(lz_member(u_next, m, mstride), lz_member(y, m, mstride), nparts, part_stride,
                        lz_member(u1, m, mstride), lz_member(u0, m, mstride), n_doubles,
                        lz_member(a_partial, m, mstride), a_nb, lz_member(a_out, m, mstride),
                        lz_member(cur_partial, m, mstride), cur_nb, lz_member(cur_out, m, mstride),
                        lz_member(prev2, m, mstride), lz_member(partial, m, mstride), lz_member(stop, m, mstride),
                        pmask, prow, ptiles, cmask, crow, ckw);
}

struct Coefs {
  double re[128];
  double im[128];
};

// res = sum_{i<m} coef_i V_i ; if prev != null also flag |res - prev| > atol + rtol |res| (numpy allclose): the flag
// word is raised to this check's generation stamp, so it never has to be cleared between checks
template <bool CPLX>
__global__ void k_lincomb(double* __restrict__ res, const double* __restrict__ V, long long n, int m, Coefs c,
                          const double* __restrict__ prev, double rtol, double atol, unsigned int* __restrict__ flag,
                          unsigned int gen) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (CPLX) {
      double xr = 0, xi = 0;
      for (int j = 0; j < m; ++j) {
        const double2 v = reinterpret_cast<const double2*>(V)[(long long)j * n + i];
        xr += c.re[j] * v.x - c.im[j] * v.y;
        xi += c.re[j] * v.y + c.im[j] * v.x;
      }
      if (prev) {
        const double2 p = reinterpret_cast<const double2*>(prev)[i];
        const double diff = hypot(p.x - xr, p.y - xi);
        if (!(diff <= atol + rtol * hypot(xr, xi))) bad = true;
      }
      reinterpret_cast<double2*>(res)[i] = make_double2(xr, xi);
    } else {
      double xr = 0;
      for (int j = 0; j < m; ++j) xr += c.re[j] * V[(long long)j * n + i];
      if (prev) {
        if (!(fabs(prev[i] - xr) <= atol + rtol * fabs(xr))) bad = true;
      }
      res[i] = xr;
    }
  }
  if (prev && bad) atomicMax(flag, gen);
}

// cyclic Jacobi eigen-decomposition of a small symmetric matrix (row-major a[m*m]);
// eigenvectors are the COLUMNS of u.  Used for the Lanczos tridiagonal matrix (m <= 128).
void sym_eig_jacobi(int m, std::vector<double>& a, std::vector<double>& w, std::vector<double>& u) {
  u.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) u[(size_t)i * m + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0, diag = 0;
    for (int i = 0; i < m; ++i) {
      diag += a[(size_t)i * m + i] * a[(size_t)i * m + i];
      for (int j = i + 1; j < m; ++j) off += a[(size_t)i * m + j] * a[(size_t)i * m + j];
    }
    if (off <= 1e-32 * (diag + off) || off == 0.0) break;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = a[(size_t)p * m + q];
        if (apq == 0.0) continue;
        const double app = a[(size_t)p * m + p], aqq = a[(size_t)q * m + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < m; ++k) {
          const double akp = a[(size_t)k * m + p], akq = a[(size_t)k * m + q];
          a[(size_t)k * m + p] = c * akp - s * akq;
          a[(size_t)k * m + q] = s * akp + c * akq;
        }
        for (int k = 0; k < m; ++k) {
          const double apk = a[(size_t)p * m + k], aqk = a[(size_t)q * m + k];
          a[(size_t)p * m + k] = c * apk - s * aqk;
          a[(size_t)q * m + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < m; ++k) {
          const double ukp = u[(size_t)k * m + p], ukq = u[(size_t)k * m + q];
          u[(size_t)k * m + p] = c * ukp - s * ukq;
          u[(size_t)k * m + q] = s * ukp + c * ukq;
        }
      }
  }
  w.resize(m);
  for (int i = 0; i < m; ++i) w[i] = a[(size_t)i * m + i];
}

// coef = U (nrm * exp(dt*w) .* U[0,:])   (lib/krylov/krylov.py:15-24)
void expm_coefs(int m, const std::vector<double>& alpha, const std::vector<double>& beta, double nrm,
                std::complex<double> dt, Coefs* out) {
  std::vector<double> a((size_t)m * m, 0.0), w, u;
  for (int i = 0; i < m; ++i) {
    a[(size_t)i * m + i] = alpha[i];
    if (i + 1 < m) a[(size_t)i * m + i + 1] = a[(size_t)(i + 1) * m + i] = beta[i];
  }
  sym_eig_jacobi(m, a, w, u);
  for (int i = 0; i < m; ++i) {
    std::complex<double> s = 0;
    for (int k = 0; k < m; ++k) s += u[(size_t)i * m + k] * (nrm * std::exp(dt * w[k]) * u[k]);  // u[0*m+k]
    out->re[i] = s.real();
    out->im[i] = s.imag();
  }
}

// ------------------------------------------------------------------------------------------------------------
// Asynchronous solve: the host enqueues Lanczos iterations ahead of the convergence decision, for a launch set of B
// members of one shape (a single solve: B = 1; mpse_expm_lanczos_batch: up to LZB_MAX, every launch of the chain covering
// all of them, blockIdx.y = member).  The small-matrix exponential, the closeness test of successive estimates and the
// decision itself run on the device; once a member's decision has fallen every later launch of that member
// (contractions included, SolveScope::skip) returns at once.  The host waits once per solve (when its guess of the
// Krylov dimension, taken from the last solve of the same problem class, was right), instead of twice per convergence
// check, and then for the control blocks of all members at once.
struct LzCtl {
  int done;       // decision has fallen
  int nvec;       // Krylov dimension of the answer
  int which;      // 0: answer in `out`, 1: in the spare buffer
  int bad;        // zero / non-finite start vector
  int need_host;  // |dt| * spectral bound too large for the on-device exponential: the host takes this check over
  int forced_m;   // breakdown: the estimate of this check is final, with this many vectors
  int stop;       // done || need_host || bad, raised by k_lz_decide: every later kernel of the member returns at once
  int pad;
};
using mpse_lz::LZ_MAXM;
static_assert(sizeof(LzCtl) == mpse_lz::LZ_CTL_DOUBLES * sizeof(double), "control block as the layout counts it");
static_assert(mpse_lz::LZ_NORM_CAP == RED_MAX_BLOCKS, "norm partials of the vector kernels fit their areas");
// |C|^2 of a start vector the unnormalised recurrence takes as it is: a normal double below 1e300 (1 / |C|^2 and the
// squares of the matvec stay finite and keep all their digits); other nonzero vectors are scaled by a power of two first
constexpr double LZ_N2_MIN = 2.2250738585072014e-308, LZ_N2_MAX = 1e300;

// coef = |v| exp(dt T_m) e_1 for the Lanczos tridiagonal T_m (alpha_0.., beta_0..) by a scaled Taylor series, one lane
// per component (lib/krylov/krylov.py:15-24 computes the same vector through eigh_tridiagonal).  Also applies the
// reference's breakdown rule retroactively: the first beta_i < tiny (i <= j) ends the space at i + 1 vectors.
// ``part`` / ``nb``: the |w|^2 partials of the update kernel launched just before; their sum beta_j^2 is formed
// here (in the order of k_reduce_final) and recorded at scal[6 + 4 j] - one launch less per convergence check.
// A launch with two workgroups also delivers the coefficients of the check two iterations earlier (workgroup 0:
// iteration j - 2, into coef + 2 LZ_MAXM; that check - the first of a solve - can never stop the iteration because there
// is no estimate before it, so it is evaluated together with the second one).
__device__ __forceinline__ void lz_coefs(double* __restrict__ scal, int j, double dt_re, double dt_im, double tiny,
                                         double* __restrict__ coef, LzCtl* ctl, const double* __restrict__ part, int nb) {
  const int lane = threadIdx.x;
  if (gridDim.x == 2 && blockIdx.x == 0) {   // the earlier check: its beta^2 is in scal already (summed by the update
    j -= 2;                                  // kernel of iteration j - 1)
    coef += 2 * LZ_MAXM;
    part = nullptr;
  }
  if (part) {
    double re = 0.0;
    for (int i = lane; i < nb; i += 64) re += part[2 * i];
    re = wave_sum(re);
    if (lane == 0) {
      scal[6 + 4 * j] = re;
      scal[6 + 4 * j + 1] = 0.0;
    }
    __threadfence_block();
    __syncthreads();
  }
  const double n2 = scal[0];
  if (!(n2 >= LZ_N2_MIN) || !(n2 < LZ_N2_MAX)) {
    if (lane == 0) {
      ctl->bad = 1;
      ctl->done = 1;
    }
    return;
  }
  int m = j + 1;
  // breakdown scan: beta_i = sqrt(scal[6 + 4 i]), i <= j (beta_j was reduced right before this launch)
  const double bi2 = lane <= j ? scal[6 + 4 * lane] : 1e300;
  const unsigned long long low = __ballot(!(sqrt(bi2) >= tiny));
  if (low) {
    m = __builtin_ctzll(low) + 1;
    if (lane == 0) ctl->forced_m = m;
  }
  const double a = lane < m ? scal[4 + 4 * lane] : 0.0;
  const double bup = lane + 1 < m ? sqrt(scal[6 + 4 * lane]) : 0.0;        // beta_lane couples lane and lane + 1
  double bdn = __shfl_up(bup, 1, 64);
  if (lane == 0) bdn = 0.0;
  // spectral bound (Gershgorin) -> scaling so that |dt| * bound / 2^s <= 1
  double g = lane < m ? fabs(a) + fabs(bup) + fabs(bdn) : 0.0;
  for (int o = 32; o > 0; o >>= 1) g = fmax(g, __shfl_xor(g, o, 64));
  const double rho = g * sqrt(dt_re * dt_re + dt_im * dt_im);
  // x = |dt| * bound / 2^s <= 2 per repetition (round 6; 1 and 22 terms before): the series of exp(x) to 1e-17 of the
  // result takes 16 / 19 / 26 terms for x <= 1/2, 1, 2 - half as many terms in all as 2^(s+1) repetitions of 22 at x <= 1 -
  // and its largest term is e^2: the cancellation costs a digit at most.
  int sq = 0;
  while (ldexp(rho, -sq) > 2.0 && sq < 40) ++sq;
  if (sq > 8) {      // would need more than 256 repetitions: let the host do this one with its eigen-decomposition
    if (lane == 0) ctl->need_host = 1;
    return;
  }
  const double xs = ldexp(rho, -sq);
  const int nterm = xs <= 0.5 ? 16 : xs <= 1.0 ? 19 : 26;
  const double sr = ldexp(dt_re, -sq), si = ldexp(dt_im, -sq);
  double yr = lane == 0 ? sqrt(n2) : 0.0, yi = 0.0;
  const int reps = 1 << sq;
  // neighbours by DPP wave shifts (lane 0 / lane 63 receive 0, which is what the tridiagonal matrix puts there): a
  // ds_bpermute round trip per neighbour was most of a term's latency
  auto from_below = [](double v) {   // value of lane - 1
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
  };
  auto from_above = [](double v) {   // value of lane + 1
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
  };
  // (dt / 2^s) T with the 1 / k of a term folded in at compile time
  const double ar = sr * a, ai = si * a, dnr = sr * bdn, dni = si * bdn, upr = sr * bup, upi = si * bup;
  for (int rep = 0; rep < reps; ++rep) {
    double tr = yr, ti = yi;     // current Taylor term
#pragma unroll
    for (int k = 1; k <= 26; ++k) {
      if (k <= nterm) {
        // t <- (dt / 2^s) T t / k
        const double ur = from_below(tr), ui = from_below(ti);
        const double dr = from_above(tr), di = from_above(ti);
        const double wr = (ar * tr - ai * ti) + (dnr * ur - dni * ui) + (upr * dr - upi * di);
        const double wi = (ar * ti + ai * tr) + (dnr * ui + dni * ur) + (upr * di + upi * dr);
        const double ik = 1.0 / (double)k;
        tr = wr * ik;
        ti = wi * ik;
        if (lane >= m) tr = ti = 0.0;
        yr += tr;
        yi += ti;
      }
    }
  }
  if (lane < LZ_MAXM) {
    // the stored basis is unnormalised: v_i = s_i U_i, s_0 = 1 / |C|, s_i = 1 / beta_{i-1}
    double sc = 0.0;
    if (lane < m) sc = lane == 0 ? 1.0 / sqrt(n2) : 1.0 / sqrt(scal[6 + 4 * (lane - 1)]);
    coef[lane] = lane < m ? yr * sc : 0.0;
    coef[LZ_MAXM + lane] = lane < m ? yi * sc : 0.0;
  }
}
// Member blockIdx.y (blockIdx.x / gridDim.x keep their meaning)
__global__ __launch_bounds__(64) void k_lz_coefs(double* scal, int j, double dt_re, double dt_im, double tiny,
                                                 double* coef, LzCtl* ctl, const double* part, int nb,
                                                 long long mstride) {
  const unsigned m = blockIdx.y;
  LzCtl* c = lz_member(ctl, m, mstride);
  if (c->stop) return;
  lz_coefs(lz_member(scal, m, mstride), j, dt_re, dt_im, tiny, lz_member(coef, m, mstride), c,
           lz_member(part, m, mstride), nb);
}

// The decisions of the check at iteration j (the estimates went to buffer `which`), one lane per member (B <= 64).  A
// member whose decision has fallen, or that needs the host (need_host, bad), raises its stop word.  ``pub`` != null: the
// host waits at this check - all B control blocks go to the mapped pinned buffer at pub + 4 m, then one sequence number
// (a k_publish launch did that before: one launch and its latency less per wait).
__global__ __launch_bounds__(64) void k_lz_decide(LzCtl* ctl, const unsigned int* flag, unsigned int gen, int has_prev,
                                                  int j, int which, int B, long long mstride, double* pub,
                                                  volatile double* seq_slot, double seq) {
  const int m = threadIdx.x;
  constexpr int W = int(sizeof(LzCtl) / sizeof(double));
  if (m < B) {
    LzCtl* c = lz_member(ctl, m, mstride);
    if (!c->stop) {
      if (!(c->done || c->need_host)) {     // (raised by k_lz_coefs of this check)
        if (c->forced_m > 0) {
          c->done = 1;
          c->nvec = c->forced_m;
          c->which = which;
        } else if (has_prev && *lz_member(flag, m, mstride) != gen) {
          c->done = 1;
          c->nvec = j + 1;
          c->which = which;
        }
      }
      if (c->done || c->need_host || c->bad) c->stop = 1;
    }
    if (pub) {
      const double* src = reinterpret_cast<const double*>(c);
      for (int i = 0; i < W; ++i) pub[m * W + i] = src[i];
    }
  }
  if (pub) {
    __threadfence_system();
    __syncthreads();
    if (m == 0) {
      *seq_slot = seq;
      __threadfence_system();
    }
  }
}

// res = sum_{i<m} coef_i V_i with the coefficients in device memory; optional closeness flag as in k_lincomb
// (Round 6, measured and dropped: the decision of the check riding on this launch - the workgroup that finishes last, by a
// counter in device memory, takes it - to save the k_lz_decide launch, ~4.6 us per check.  4 096 workgroups counting
// on one address cost far more than the launch: 539 -> 434 site-updates/s, profiles/r06_ab_lz_fuse.txt.)
// ``m_early`` > 0: the estimate of the (deferred) first check, sum_{i < m_early} coef2_i V_i with coef2 = coef + 2 LZ_MAXM,
// is formed in the same pass over the basis and takes the place of ``prev``.
template <bool CPLX>
__device__ __forceinline__ void lincomb_dev(double* __restrict__ res, const double* __restrict__ V, long long n, int m,
                                            const double* __restrict__ coef, const double* __restrict__ prev, double rtol,
                                            double atol, unsigned int* __restrict__ flag, unsigned int gen,
                                            const LzCtl* __restrict__ ctl, int m_early,
                                            const unsigned char* __restrict__ cmask, int crow, int ckw) {
  // cmask: as in k_lanczos_update_u - the basis vectors (and the earlier estimate) are exactly zero outside it
  // (a member that stopped has one of the two set; k_lz_coefs of this check may have raised them since)
  if (ctl->done || ctl->need_host) return;
  __shared__ double cr[LZ_MAXM], ci[LZ_MAXM], er[LZ_MAXM], ei[LZ_MAXM];
  if (threadIdx.x < LZ_MAXM) {
    cr[threadIdx.x] = coef[threadIdx.x];
    ci[threadIdx.x] = coef[LZ_MAXM + threadIdx.x];
    er[threadIdx.x] = m_early > 0 ? coef[2 * LZ_MAXM + threadIdx.x] : 0.0;
    ei[threadIdx.x] = m_early > 0 ? coef[3 * LZ_MAXM + threadIdx.x] : 0.0;
  }
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (CPLX) {
      if (cmask) {
        const unsigned ee = (unsigned)i, row = ee / (unsigned)crow, col = ee - row * (unsigned)crow;
        if (!cmask[(col >> 6) * ckw + (row >> 4)]) {
          reinterpret_cast<double2*>(res)[i] = make_double2(0.0, 0.0);
          continue;
        }
      }
      double xr = 0, xi = 0, pr = 0, pi = 0;
      for (int jj = 0; jj < m; ++jj) {
        if (cr[jj] == 0.0 && ci[jj] == 0.0 && !(jj < m_early)) continue;   // past a breakdown: never touched
        const double2 v = reinterpret_cast<const double2*>(V)[(long long)jj * n + i];
        if (cr[jj] != 0.0 || ci[jj] != 0.0) {
          xr += cr[jj] * v.x - ci[jj] * v.y;
          xi += cr[jj] * v.y + ci[jj] * v.x;
        }
        if (jj < m_early && (er[jj] != 0.0 || ei[jj] != 0.0)) {
          pr += er[jj] * v.x - ei[jj] * v.y;
          pi += er[jj] * v.y + ei[jj] * v.x;
        }
      }
      if (m_early > 0) {
        const double diff = hypot(pr - xr, pi - xi);
        if (!(diff <= atol + rtol * hypot(xr, xi))) bad = true;
      } else if (prev) {
        const double2 p = reinterpret_cast<const double2*>(prev)[i];
        const double diff = hypot(p.x - xr, p.y - xi);
        if (!(diff <= atol + rtol * hypot(xr, xi))) bad = true;
      }
      reinterpret_cast<double2*>(res)[i] = make_double2(xr, xi);
    } else {
      double xr = 0, pr = 0;
      for (int jj = 0; jj < m; ++jj) {
        if (cr[jj] == 0.0 && !(jj < m_early)) continue;
        const double v = V[(long long)jj * n + i];
        if (cr[jj] != 0.0) xr += cr[jj] * v;
        if (jj < m_early && er[jj] != 0.0) pr += er[jj] * v;
      }
      if (m_early > 0) {
        if (!(fabs(pr - xr) <= atol + rtol * fabs(xr))) bad = true;
      } else if (prev) {
        if (!(fabs(prev[i] - xr) <= atol + rtol * fabs(xr))) bad = true;
      }
      res[i] = xr;
    }
  }
  if ((prev || m_early > 0) && bad) atomicMax(flag, gen);
}
// Member blockIdx.y.  The estimate goes to the member's own result (res_sel 0: mem[m].out, or `out` itself when there is
// no member table - a single solve uploads none) or to its spare buffer (1: spare + m * mstride); ``prev_sel`` names the
// earlier estimate the same way (-1: none)
template <bool CPLX>
__global__ void k_lincomb_dev(const BatchMember* __restrict__ mem, double* out, double* spare, int res_sel, int prev_sel,
                              const double* V, long long n, int m, const double* coef, double rtol, double atol,
                              unsigned int* flag, unsigned int gen, const LzCtl* ctl, int m_early,
                              const unsigned char* __restrict__ cmask, int crow, int ckw, long long mstride) {
  const unsigned b = blockIdx.y;
  double* o = mem ? static_cast<double*>(mem[b].out) : out;
  double* sp = lz_member(spare, b, mstride);
  lincomb_dev<CPLX>(res_sel == 0 ? o : sp, lz_member(V, b, mstride), n, m, lz_member(coef, b, mstride),
                    prev_sel < 0 ? nullptr : (prev_sel == 0 ? o : sp), rtol, atol, lz_member(flag, b, mstride), gen,
                    lz_member(ctl, b, mstride), m_early, cmask, crow, ckw);
}

// Start of an asynchronous solve in one launch (three before: zero fill of the control block, copy of the start vector,
// its norm partials): U_0 = C, partial[b] = sum over block b of |C_i|^2 in the order of k_dot_partial(C, C), *ctl = 0.
template <bool CPLX>
__device__ __forceinline__ void lz_start(double* __restrict__ u0, const double* __restrict__ c, long long n,
                                         double* __restrict__ partial, LzCtl* ctl) {
  if (blockIdx.x == 0 && threadIdx.x < int(sizeof(LzCtl) / sizeof(int))) reinterpret_cast<int*>(ctl)[threadIdx.x] = 0;
  double re = 0, im = 0;
  const long long stride = (long long)gridDim.x * RED_THREADS;
  if (CPLX) {
    const double2* x2 = reinterpret_cast<const double2*>(c);
    double2* o2 = reinterpret_cast<double2*>(u0);
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += 2 * stride) {
      const long long i1 = i + stride;
      const bool h1 = i1 < n;
      const double2 a0 = x2[i];
      const double2 a1 = h1 ? x2[i1] : make_double2(0.0, 0.0);
      o2[i] = a0;
      if (h1) o2[i1] = a1;
      re += a0.x * a0.x + a0.y * a0.y;
      im += a0.x * a0.y - a0.y * a0.x;
      re += a1.x * a1.x + a1.y * a1.y;
      im += a1.x * a1.y - a1.y * a1.x;
    }
  } else {
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) {
      const double v = c[i];
      u0[i] = v;
      re += v * v;
    }
  }
  block_allsum2(re, im);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = re;
    partial[2 * blockIdx.x + 1] = im;
  }
}
// Member blockIdx.y starts from mem[m].C (without a member table: from `c`); its flag word is cleared with its control
// block (the region is fresh memory; lz_flag_stamp clears again only when the stamp wraps around)
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_lz_start(const BatchMember* __restrict__ mem, const double* c, double* u0,
                                                          long long n, double* partial, LzCtl* ctl, unsigned int* flag,
                                                          long long mstride) {
  const unsigned m = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) *lz_member(flag, m, mstride) = 0;
  lz_start<CPLX>(lz_member(u0, m, mstride), mem ? static_cast<const double*>(mem[m].C) : c, n,
                 lz_member(partial, m, mstride), lz_member(ctl, m, mstride));
}

inline bool lanczos_async_enabled() {
  static const bool on = [] {
    const char* e = getenv("MPSE_LANCZOS_ASYNC");
    return !(e && e[0] == '0');
  }();
  return on;
}

constexpr int LZ_CW = int(sizeof(LzCtl) / sizeof(double));
constexpr int LZB_MAX = 64;            // members per launch set (one lane each in k_lz_decide)
static_assert(mpse_ctx::PIN_BATCH_CTL + LZB_MAX * LZ_CW < mpse_ctx::PIN_QR_STATUS, "batch slot clear of the QR status word");

// The schedule and the region layout are integer rules of their own (mpse_lanczos_plan.h, tested on the host).  The
// run-ahead hint they start from is kept per problem class in the context (mpse_ctx::lz_hint)
using mpse_lz::LZ_DOT_CAP;
using LzSchedule = mpse_lz::Schedule;
inline unsigned long long lz_hint_key(int nsite, int64_t n, bool cplx) {
  return ((unsigned long long)nsite << 60) ^ ((unsigned long long)n << 1) ^ (cplx ? 1ull : 0ull);
}
inline int lz_hint(mpse_ctx* ctx, unsigned long long key) {
  const auto it = ctx->lz_hint.find(key);
  return it != ctx->lz_hint.end() ? it->second : 0;
}

// Generation stamp of a check that compares two estimates (0 for one that does not): the flag word is raised to the
// stamp, so it never has to be cleared between checks - only when the stamp wraps around (B words, `pitch` bytes apart)
int lz_flag_stamp(mpse_ctx* ctx, bool compares, unsigned int* flag, size_t pitch, int B, unsigned int* gen) {
  *gen = 0;
  if (!compares) return MPSE_OK;
  *gen = ++ctx->flag_gen;
  if (*gen != 0) return MPSE_OK;
  if (B == 1)
    MPSE_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(unsigned int), ctx->stream));
  else
    MPSE_HIP(ctx, hipMemset2DAsync(flag, pitch, 0, sizeof(unsigned int), size_t(B), ctx->stream));
  *gen = ++ctx->flag_gen;
  return MPSE_OK;
}

// the environments are constant over a Lanczos solve: their tile-occupancy masks are scanned once (mpse_gemm.hip)
void keep_env_masks(SolveScope& sc, const mpse_heff* h) {
  const mpse_dims& s = h->dims;
  const size_t lb = size_t(s.Dl_ket) * s.wl * s.Dl_ket * (h->l_dtype == MPSE_C128 ? 16 : 8);
  const size_t rb = size_t(s.Dr_ket) * s.wr * s.Dr_ket * (h->r_dtype == MPSE_C128 ? 16 : 8);
  sc.env_lo[0] = static_cast<const char*>(h->L), sc.env_hi[0] = sc.env_lo[0] + lb;
  sc.env_lo[1] = static_cast<const char*>(h->R), sc.env_hi[1] = sc.env_lo[1] + rb;
  sc.keeps_env_masks = true;
}

constexpr int LZ_FALLBACK = -77;   // internal: the asynchronous solve hands the problem to the synchronous one
constexpr int LZ_BADSTART = -78;   // internal: |C|^2 outside [LZ_N2_MIN, LZ_N2_MAX) (expm_lanczos_solve decides)

// What lz_async_run works on: a launch set of B members (1 <= B <= LZB_MAX) of n elements each
struct LzProblem {
  int dtype;
  int64_t n;
  int B;
  // start vectors and results: the device table of the members, or - null, B == 1 - the two pointers themselves (a
  // single solve uploads no table: the upload would stand on the dependent chain of every solve)
  const BatchMember* mem;
  const void* C;
  void* out;
  std::complex<double> dt;
  double rtol, atol;
  bool vec16;                    // 16-byte accesses: every Krylov vector starts on a 16-byte boundary and has even length
  // The structural mask of the centre (null: none): every vector of the solve is zero in the tiles it leaves out
  // (k_lanczos_update_u); the same for all members
  const unsigned char* vmask;
  int vm_row, vm_kw;
  int parts, dot_cap;            // result parts and dot partials the matvec may write (mpse_lz::layout)
};
// The set's areas: one slab, member m's region `lay.stride` doubles behind that of member m - 1.  The driver allocates
// it and replaces it when the basis grows; the caller finds C (bitwise, basis vector 0) and the spare estimate there.
struct LzSet {
  TmpBuf slab;
  mpse_lz::Layout lay{};
  explicit LzSet(mpse_ctx* ctx) : slab(ctx) {}
  double* at(int64_t off, int m = 0) { return slab.as<double>() + m * lay.stride + off; }
  long long mstride() const { return lay.stride * (long long)sizeof(double); }
};
// The one point where the callers of lz_async_run differ - y = H U_j for every member, iteration j.  The matvec gets
// member-0 addresses: U_j, the result parts, the dot partials, the members' stop word (its launches do nothing for a
// member whose word is set), the basis' range.  It says how the result came: as the sum of `nparts` tensors n elements
// apart (with `pmask`: tile-masked parts, MatvecReq::Parts), with a_nb partials of <H U_j, U_j>.
struct LzIter {
  int j;
  const double* u;
  double* parts;
  double* dot;
  const int* stop;
  long long mstride;
  const char *basis_lo, *basis_hi;
};
struct LzMatvecOut {
  int nparts = 1, a_nb = 0;
  const unsigned long long* pmask = nullptr;
  int prow = 0, ptiles = 0;
};
struct LzOutcome {
  enum Kind {
    RUNNING,   // (inside the driver only)
    DONE,      // the estimate with `nvec` vectors is the answer: in the member's `out` (which = 0) or in its spare area (1)
    BAD,       // |C|^2 outside what the recurrence takes; nothing went to `out`
    TO_SYNC    // the synchronous solve has to take over: need_host, or no decision within the 64-vector limit
  } kind = RUNNING;
  int which = 0, nvec = 0;
  bool breakdown = false;        // DONE by the breakdown rule, not by convergence
};
// What happened on the way, in the terms of mpse_ctx::lz_paths (LP_WAITS, LP_MERGED, LP_GROW, LP_PARTS, LP_VMASK,
// LP_UNVEC, LP_HOST_FIRST / LP_HOST_LATER, LP_LIMIT).  The driver reports, its callers count.
struct LzTally {
  long long paths[mpse_ctx::LP_COUNT] = {0};
  bool estimates = false;        // a check was enqueued: estimates may have gone to `out`
};

// The asynchronous iteration for one launch set; one outcome per member at oc[0 .. B).
template <class Matvec>
int lz_async_run(mpse_ctx* ctx, const LzProblem& p, LzSchedule sch, LzSet& set, Matvec&& matvec, LzOutcome* oc,
                 LzTally* tally) {
  const int B = p.B;
  const int64_t n = p.n;
  const bool cplx = p.dtype == MPSE_C128;
  const int64_t nd = n * (cplx ? 2 : 1);
  const double tiny = 100.0 * double(n) * 2.220446049250313e-16;
  const int nb = red_blocks(nd);
  const double vbytes = double(B) * double(n) * double(dtype_size(p.dtype));   // (the profiler's algorithmic bytes, variant 4)
  mpse_lz::Layout& L = set.lay;
  L = mpse_lz::layout(n, cplx, p.parts, p.dot_cap, sch.cap);
  MPSE_TRY(set.slab.alloc(size_t(B) * L.stride * sizeof(double)));
  // member-0 addresses, read again after the slab has grown
  auto vec = [&](int j) { return set.at(L.basis) + int64_t(j) * nd; };
  auto ctl = [&] { return reinterpret_cast<LzCtl*>(set.at(L.ctl)); };
  auto flag = [&] { return reinterpret_cast<unsigned int*>(set.at(L.flag)); };

  // U_0 = C itself (the Krylov basis is kept unnormalised, k_lanczos_update_u); |C|^2 partials feed the first step
  {
    ProfScope ps(ctx, 4, 0.0, 3.0 * vbytes);
    MPSE_LAUNCH_TF(ctx, cplx, k_lz_start, dim3(nb, B), dim3(RED_THREADS), p.mem, (const double*)p.C, vec(0), (long long)n,
                   set.at(L.norm[0]), ctl(), flag(), set.mstride());
    ps.end();
  }
  MPSE_HIP(ctx, hipGetLastError());

  int prev_sel = -1;    // where the earlier estimate went: -1 none, 0 the result, 1 the spare area (the same for all)
  bool waited = false;
  std::vector<LzCtl> hc(B);
  for (int m = 0; m < B; ++m) oc[m] = LzOutcome();
  for (int j = 0;; ++j) {
    if (j + 2 > sch.cap) {      // room for U_{j+1}: a new slab with a longer basis per member
      // In front of the matvec: the result parts are dead here (the update of iteration j - 1 has read them) and stay
      // behind; what lies in front of them and what lies behind them moves, section by section at the same offsets
      const int ncap = sch.grown();
      const mpse_lz::Layout G = mpse_lz::layout(n, cplx, p.parts, p.dot_cap, ncap);
      ++tally->paths[mpse_ctx::LP_GROW];
      TmpBuf s2(ctx);
      MPSE_TRY(s2.alloc(size_t(B) * G.stride * sizeof(double)));
      const int64_t span[2][2] = {{0, L.parts}, {L.spare, L.stride}};
      for (const auto& r : span)
        MPSE_HIP(ctx, hipMemcpy2DAsync(s2.as<double>() + r[0], size_t(G.stride) * 8, set.at(r[0]), size_t(L.stride) * 8,
                                       size_t(r[1] - r[0]) * 8, size_t(B), hipMemcpyDeviceToDevice, ctx->stream));
      std::swap(set.slab.p, s2.p);
      L = G;
      sch.cap = ncap;
    }
    const long long mstride = set.mstride();
    double* scal = set.at(L.scal);
    double* part_a = set.at(L.dot);
    const int* stop0 = &ctl()->stop;
    LzMatvecOut mv;
    MPSE_TRY(matvec(LzIter{j, vec(j), set.at(L.parts), part_a, stop0, mstride, reinterpret_cast<const char*>(vec(0)),
                           reinterpret_cast<const char*>(vec(sch.cap))},
                    &mv));
    // |U_j|^2 partials came from step j - 1 (or from |C|^2); this step's |w|^2 partials go to the other area
    double* cur_part = set.at(L.norm[j & 1]);
    double* new_part = set.at(L.norm[(j + 1) & 1]);
    double* cur_out = j == 0 ? scal : scal + 6 + 4 * (j - 1);
    const double* prev2 = j == 0 ? scal : (j == 1 ? scal : scal + 6 + 4 * (j - 2));
    if (mv.nparts > 1 || mv.pmask) ++tally->paths[mpse_ctx::LP_PARTS];
    if (!mv.pmask && p.vmask) ++tally->paths[mpse_ctx::LP_VMASK];
    if (!p.vec16) ++tally->paths[mpse_ctx::LP_UNVEC];
    {
      ProfScope ps(ctx, 4, 0.0, (j > 0 ? 4.0 : 3.0) * vbytes + (mv.nparts - 1) * vbytes);
      MPSE_LAUNCH_TF(ctx, p.vec16, k_lanczos_update_u, dim3(nb, B), dim3(RED_THREADS), vec(j + 1),
                     (const double*)set.at(L.parts), mv.nparts, (long long)nd, (const double*)vec(j),
                     j > 0 ? (const double*)vec(j - 1) : (const double*)nullptr, (long long)nd, (const double*)part_a,
                     mv.a_nb, scal + 4 + 4 * j, (const double*)cur_part, nb, cur_out, prev2, new_part, stop0, mv.pmask,
                     mv.prow, mv.ptiles, mv.pmask ? nullptr : p.vmask, p.vm_row, p.vm_kw, mstride);
      ps.end();
    }
    const LzSchedule::Step step = sch.at(j, prev_sel >= 0);
    const bool merged = step.merged, last = step.last;
    if (step.check) {
      if (merged) ++tally->paths[mpse_ctx::LP_MERGED];
      hipLaunchKernelGGL(k_lz_coefs, dim3(merged ? 2 : 1, B), dim3(64), 0, ctx->stream, scal, j, p.dt.real(), p.dt.imag(),
                         tiny, set.at(L.coef), ctl(), (const double*)new_part, nb, mstride);
      // successive estimates alternate between `out` and the spare area (no copies between checks)
      const int res_sel = prev_sel == 0 ? 1 : 0;
      const bool compares = prev_sel >= 0 || merged;
      unsigned int gen = 0;
      MPSE_TRY(lz_flag_stamp(ctx, compares, flag(), size_t(mstride), B, &gen));
      MPSE_LAUNCH_TF(ctx, cplx, k_lincomb_dev, dim3(ew_blocks(n), B), dim3(256), p.mem, (double*)p.out, set.at(L.spare),
                     res_sel, prev_sel, (const double*)vec(0), (long long)n, j + 1, (const double*)set.at(L.coef), p.rtol,
                     p.atol, flag(), gen, (const LzCtl*)ctl(), merged ? j - 1 : 0, p.vmask, p.vm_row, p.vm_kw, mstride);
      const bool wait_here = j >= sch.wait_from || waited || last;
      const PublishAt pa = publish_target(ctx, wait_here, mpse_ctx::PIN_BATCH_CTL);
      hipLaunchKernelGGL(k_lz_decide, dim3(1), dim3(64), 0, ctx->stream, ctl(), (const unsigned int*)flag(), gen,
                         compares ? 1 : 0, j, res_sel, B, mstride, pa.pub, pa.seq_slot, pa.seq);
      prev_sel = res_sel;
      tally->estimates = true;
      MPSE_HIP(ctx, hipGetLastError());
      if (wait_here) {
        MPSE_TRY(publish_collect(ctx, pa, ctl(), size_t(mstride), B, LZ_CW, mpse_ctx::PIN_BATCH_CTL, hc.data()));
        ++tally->paths[mpse_ctx::LP_WAITS];
        bool all = true;
        for (int m = 0; m < B; ++m) {
          LzOutcome& o = oc[m];
          if (o.kind != LzOutcome::RUNNING) continue;
          if (hc[m].bad) {             // (done was raised with it: nothing went to `out`)
            o.kind = LzOutcome::BAD;
          } else if (hc[m].need_host) {
            o.kind = LzOutcome::TO_SYNC;
            ++tally->paths[waited ? mpse_ctx::LP_HOST_LATER : mpse_ctx::LP_HOST_FIRST];
          } else if (hc[m].done) {
            o.kind = LzOutcome::DONE;
            o.which = hc[m].which, o.nvec = hc[m].nvec, o.breakdown = hc[m].forced_m > 0;
          } else {
            all = false;
          }
        }
        waited = true;
        if (all) return MPSE_OK;
      }
    }
    if (last) {     // beyond one wavefront of coefficients (or no convergence): the synchronous solve decides
      ++tally->paths[mpse_ctx::LP_LIMIT];
      for (int m = 0; m < B; ++m)
        if (oc[m].kind == LzOutcome::RUNNING) oc[m].kind = LzOutcome::TO_SYNC;
      return MPSE_OK;
    }
  }
}

// The single solve: a launch set of one member with the general matvec.
// hints: the caller's structural mask of the centre (empty: none; it describes the Krylov vectors of this solve) and its
// key of the solve's plan slot (0: none).  Only this solve uses them: the synchronous one it may hand over to has neither.
int expm_lanczos_async(mpse_ctx* ctx, int dtype, const mpse_heff* h, std::complex<double> dt, const void* Cin, void* out,
                       double rtol, double atol, int max_dim, int* nvec, int64_t n, const SolveHints& hints) {
  const bool cplx = dtype == MPSE_C128;
  const size_t es = dtype_size(dtype);
  const unsigned long long key = lz_hint_key(h->nsite, n, cplx);
  const bool vec16 = (cplx || n % 2 == 0) && (reinterpret_cast<uintptr_t>(Cin) & 15) == 0;
  // the matvec result, with room for a second part (MatvecReq::parts: halved tiles)
  int parts = n <= 65536 ? 4 : 2;   // (small centres: up to four slices, mpse_small.hip)
  const int f0_parts = (cplx && (reinterpret_cast<uintptr_t>(Cin) & 15) == 0) ? heff0_fused_parts(h, dtype) : 0;
  if (f0_parts > parts) parts = f0_parts;   // tile-masked parts of the fused 0-site matvec

  SolveScope scope(ctx);
  keep_env_masks(scope, h);
  scope.cmask = hints.cmask;
  scope.borrow_slot(hints.slot_key);

  // the structural mask of the centre also serves the vector kernels of this solve (square operators on complex vectors
  // whose rows are whole multiples of 64 elements)
  const unsigned char* vmask = nullptr;
  int vm_row = 0, vm_kw = 0;
  static const bool vmask_on = [] {
    const char* e = getenv("MPSE_VEC_MASK");
    return !(e && e[0] == '0');
  }();
  if (vmask_on && vec16 && cplx && scope.cmask.ptr && h->dims.Dl_ket > 0 && h->dims.Dl_bra == h->dims.Dl_ket &&
      h->dims.Dr_bra == h->dims.Dr_ket && n < (int64_t(1) << 31)) {
    const int64_t Dl = h->dims.Dl_ket, N = n / Dl;
    const int64_t nkw = ((Dl + 15) / 16 + 7) / 8;
    if (N * Dl == n && N % 64 == 0 && scope.cmask.bytes == (N / 64) * nkw * 8) {
      vmask = static_cast<const unsigned char*>(scope.cmask.ptr);
      vm_row = (int)N;
      vm_kw = (int)(nkw * 8);
    }
  }
  static const bool omask_on = [] {
    const char* e = getenv("MPSE_OUT_MASK");   // MPSE_OUT_MASK=0: the matvec writes every tile of its result
    return !(e && e[0] == '0');
  }();

  const int nb = red_blocks(n * (cplx ? 2 : 1));
  auto matvec = [&](const LzIter& it, LzMatvecOut* r) -> int {
    scope.skip = it.stop;
    scope.krylov_lo = it.basis_lo;   // (the basis moves when it grows)
    scope.krylov_hi = it.basis_hi;
    MatvecReq mv;
    // <H U_j, U_j> rides on the launch that completes H U_j; matvecs that cannot take it leave nb_out = 0 and the
    // reduction runs as a pass of its own
    mv.dot.y = it.u;
    mv.dot.part = it.dot;
    mv.dot.cap = LZ_DOT_CAP;
    // the result may come as W + W2 (the update reads both): the last product of a large one-site matvec then runs as
    // halved tiles, two workgroups per compute unit
    mv.parts.ptr = it.parts;
    mv.parts.cap_elems = (long long)parts * n;
    mv.parts.n = n;
    mv.parts.masked_ok = f0_parts > 0 && vec16;
    // the update reads the result only inside the structural mask (a matvec that answers with a part mask of its own is
    // one that does not look at this request)
    if (vmask && omask_on) mv.out_mask.mask = vmask, mv.out_mask.row = vm_row, mv.out_mask.pitch = vm_kw;
    MPSE_TRY(heff_apply(ctx, dtype, h, it.u, it.parts, &scope, &mv));
    const int used = mv.parts.used;
    r->pmask = mv.parts.mask, r->prow = mv.parts.mask_row, r->ptiles = mv.parts.mask_tiles;
    r->nparts = used > 0 ? used : (used == -2 ? 2 : 1);
    r->a_nb = mv.dot.nb_out > 0 ? mv.dot.nb_out : nb;
    if (mv.dot.nb_out > 0) return MPSE_OK;
    if (r->nparts > 1) return mpse_fail(ctx, MPSE_ERR_ARG, "expm_lanczos: a two-part matvec result without its dot partials");
    ProfScope ps(ctx, 4, 0.0, 2.0 * double(n) * double(es));
    MPSE_LAUNCH_TF(ctx, cplx, k_dot_partial, dim3(nb), dim3(RED_THREADS), (const double*)it.parts, it.u, (long long)n,
                   it.dot, it.stop);
    ps.end();
    return MPSE_OK;
  };

  const LzProblem p{dtype, n, 1, nullptr, Cin, out, dt, rtol, atol, vec16, vmask, vm_row, vm_kw, parts, LZ_DOT_CAP};
  LzSet set(ctx);
  LzOutcome oc;
  LzTally tally;
  const int st = lz_async_run(ctx, p, LzSchedule(lz_hint(ctx, key), max_dim), set, matvec, &oc, &tally);
  for (int i = 0; i < mpse_ctx::LP_COUNT; ++i) ctx->lz_paths[i] += tally.paths[i];
  MPSE_TRY(st);
  switch (oc.kind) {
    case LzOutcome::BAD:
      return LZ_BADSTART;
    case LzOutcome::DONE:
      ++ctx->lz_paths[mpse_ctx::LP_ASYNC_DONE];
      ++ctx->lz_paths[oc.breakdown ? mpse_ctx::LP_BD_ASYNC : mpse_ctx::LP_CONV];
      // the answer sits in the spare area (an even number of estimates): copied now - the host knows; before, a
      // conditional copy kernel was enqueued at every waited check
      if (oc.which == 1) MPSE_TRY(mpse_memcpy_d2d(ctx, out, set.at(set.lay.spare), size_t(n) * es));
      ctx->lz_hint[key] = oc.nvec;
      if (nvec) *nvec = oc.nvec;
      return MPSE_OK;
    default:
      // The synchronous solve restarts from Cin.  Estimates of this solve may have gone to `out` already: when `out` is
      // Cin, C is put back from its copy U_0 first (bitwise C; U_0 is never written after k_lz_start).
      if (tally.estimates && out == Cin) {
        ++ctx->lz_paths[mpse_ctx::LP_ALIAS_RESTART];
        MPSE_TRY(mpse_memcpy_d2d(ctx, out, set.at(set.lay.basis), size_t(n) * es));
      }
      return LZ_FALLBACK;
  }
}

// The synchronous solve: the host reads the recurrence scalars at every check and forms the coefficients itself.  It
// starts from Cin and takes no structural centre mask.
int expm_lanczos_sync(mpse_ctx* ctx, int dtype, const mpse_heff* h, std::complex<double> dt, const void* Cin, void* out,
                      double rtol, double atol, int max_dim, int* nvec, int64_t n) {
  const bool cplx = dtype == MPSE_C128;
  const size_t es = dtype_size(dtype);
  ++ctx->lz_paths[mpse_ctx::LP_SYNC];
  const int64_t nd = n * (cplx ? 2 : 1);  // doubles per vector
  const double tiny = 100.0 * double(n) * 2.220446049250313e-16;

  int cap = 16;
  TmpBuf V(ctx), W(ctx), RES(ctx), SCAL(ctx);
  MPSE_TRY(V.alloc(size_t(cap) * n * es));
  MPSE_TRY(W.alloc(size_t(n) * es));
  // device-resident recurrence scalars: [0..1] |v|^2 ; per j: alpha (re,im) at 4+4j, beta^2 at 6+4j ; flag at the end
  const int SC_FLAG = 4 + 4 * 130;
  MPSE_TRY(SCAL.alloc(size_t(SC_FLAG + 2) * sizeof(double)));
  double* scal = SCAL.as<double>();
  const int nb = red_blocks(nd);
  // two partial-sum areas: a kernel that consumes one set of partials writes its own into the other
  double* part_a = ctx->dscratch;                          // <w, v_j> partials
  double* part_b = ctx->dscratch + 4 * RED_MAX_BLOCKS;     // |.|^2 partials

  // optional HIP-event sampling of the HBM-bound vector kernels (mpse_prof_*, variant 4): algorithmic bytes
  const double vbytes = double(n) * double(es);
  auto dot_partials = [&](const void* x, const void* y, double* dst_partial) {
    ProfScope ps(ctx, 4, 0.0, 2.0 * vbytes);
    MPSE_LAUNCH_TF(ctx, cplx, k_dot_partial, dim3(nb), dim3(RED_THREADS), (const double*)x, (const double*)y, (long long)n,
                   dst_partial, (const int*)nullptr);
    ps.end();
  };

  // v0 = C / |C|
  dot_partials(Cin, Cin, part_b);
  // 16-byte vector accesses whenever every Krylov vector starts on a 16-byte boundary (always for complex128)
  const bool vec16 = (cplx || n % 2 == 0) && (reinterpret_cast<uintptr_t>(Cin) & 15) == 0;
  MPSE_LAUNCH_TF_CHK(ctx, vec16, k_scale_into_dev, dim3(nb), dim3(RED_THREADS), V.as<double>(), (const double*)Cin,
                     (long long)nd, (const double*)part_b, nb, scal, (const int*)nullptr);

  std::vector<double> alpha, beta;
  double nrmv = 0.0, nrm2 = 0.0;
  bool have_res = false;
  void* res_prev = nullptr;
  int pending_m = 0;   // Krylov dimension of a first estimate whose formation is postponed to the next check
  auto vec = [&](int j) { return V.as<char>() + size_t(j) * n * es; };
  // bring the scalars of iterations [alpha.size(), upto] to the host (one copy, one sync)
  auto fetch = [&](int upto) -> int {
    const int cnt = 4 + 4 * (upto + 1);
    MPSE_TRY(publish_and_wait(ctx, scal, cnt, mpse_ctx::PIN_LZ_SCAL));
    if (ctx->prof_pending.size() > 2048) prof_drain(ctx);
    const double* p = ctx->pinned + mpse_ctx::PIN_LZ_SCAL;
    nrm2 = p[0];
    nrmv = sqrt(p[0]);
    for (int j = (int)alpha.size(); j <= upto; ++j) {
      alpha.push_back(p[4 + 4 * j]);
      beta.push_back(sqrt(p[6 + 4 * j]));
    }
    return MPSE_OK;
  };
  auto finish = [&](int m, void* dst, const void* prev, int* flag_out) -> int {
    // dst = V[:m]^T coef ; optional closeness test against prev (numpy allclose semantics)
    Coefs c;
    expm_coefs(m, alpha, beta, nrmv, dt, &c);
    unsigned int* dflag = reinterpret_cast<unsigned int*>(ctx->dscratch + (size_t(1) << 16) - 8);
    unsigned int gen = 0;
    MPSE_TRY(lz_flag_stamp(ctx, prev != nullptr, dflag, 0, 1, &gen));
    MPSE_LAUNCH_TF_CHK(ctx, cplx, k_lincomb, dim3(ew_blocks(n)), dim3(256), (double*)dst, V.as<double>(), (long long)n, m,
                       c, (const double*)prev, rtol, atol, dflag, gen);
    if (prev && flag_out) {
      MPSE_TRY(publish_and_wait(ctx, reinterpret_cast<const double*>(dflag), 1, mpse_ctx::PIN_FLAG));
      *flag_out = (*reinterpret_cast<unsigned int*>(ctx->pinned + mpse_ctx::PIN_FLAG) == gen) ? 1 : 0;
    }
    return MPSE_OK;
  };
  // the reference stops at the first j with beta_j < tiny (krylov.py:72-74); scalars arrive late here, so the
  // test is applied retroactively: vectors past a breakdown are never used
  auto breakdown_at = [&](int upto) -> int {
    for (int j = 0; j <= upto && j < (int)beta.size(); ++j)
      if (!(beta[j] >= tiny)) return j;
    return -1;
  };

  SolveScope scope(ctx);
  keep_env_masks(scope, h);
  for (int j = 0;; ++j) {
    MPSE_TRY(heff_apply(ctx, dtype, h, vec(j), W.p, &scope, nullptr));
    dot_partials(W.p, vec(j), part_a);                             // alpha_j = Re <w, v_j> (partials)
    if (j == n - 1) {                                              // Krylov space == full space (krylov.py:59-61)
      hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(RED_THREADS), 0, ctx->stream, part_a, nb, scal + 4 + 4 * j,
                         (const int*)nullptr);
      MPSE_TRY(fetch(j));
      if (!(nrm2 >= LZ_N2_MIN && nrm2 < LZ_N2_MAX)) return LZ_BADSTART;
      int bd = breakdown_at(j - 1);
      const int m = bd >= 0 ? bd + 1 : j + 1;
      ++ctx->lz_paths[bd >= 0 ? mpse_ctx::LP_BD_SYNC : mpse_ctx::LP_FULL];
      MPSE_TRY(finish(m, out, nullptr, nullptr));
      if (nvec) *nvec = m;
      return MPSE_OK;
    }
    if (!vec16) ++ctx->lz_paths[mpse_ctx::LP_UNVEC];
    ProfScope ups(ctx, 4, 0.0, (j > 0 ? 4.0 : 3.0) * vbytes);
    MPSE_LAUNCH_TF(ctx, vec16, k_lanczos_update, dim3(nb), dim3(RED_THREADS), W.as<double>(), (const double*)vec(j),
                   j > 0 ? (const double*)vec(j - 1) : (const double*)nullptr, (long long)nd, (const double*)part_a, nb,
                   scal + 4 + 4 * j, (const double*)(scal + 6 + 4 * (j > 0 ? j - 1 : 0)), part_b, (const int*)nullptr);
    ups.end();
    // beta_j^2: needed by the host at a check and by the next update; k_scale_into_dev stores it when it runs
    // (every path that continues), the returning paths below read it through k_reduce_final
    const bool check = (j > 3 && j % 2 == 0);                      // krylov.py:76-81
    const bool last = (j + 1 >= max_dim);
    // The first estimate (j = 4) decides nothing - there is no earlier one to compare with - so it is not worth a
    // host round trip: it is formed at the next check, from the same alpha / beta / vectors it would have used,
    // right before the estimate it is compared with.  (A breakdown at j <= 4 is found at that next fetch and handled
    // retroactively like any other.)
    const bool defer = check && !have_res && pending_m == 0 && !last;
    const bool sync_now = (check && !defer) || last;
    if (sync_now)
      hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(RED_THREADS), 0, ctx->stream, part_b, nb, scal + 6 + 4 * j,
                         (const int*)nullptr);
    MPSE_HIP(ctx, hipGetLastError());
    if (sync_now) {
      MPSE_TRY(fetch(j));
      if (!(nrm2 >= LZ_N2_MIN && nrm2 < LZ_N2_MAX)) return LZ_BADSTART;
      const int bd = breakdown_at(j);
      if (bd >= 0) {
        ++ctx->lz_paths[mpse_ctx::LP_BD_SYNC];
        // what the reference would have returned at iteration bd - unless one of its convergence tests
        // (even jj > 3, jj < bd) had fired earlier: the deferred first estimate cannot fire (nothing to compare
        // with), later ones all ran here already and failed
        MPSE_TRY(finish(bd + 1, out, nullptr, nullptr));
        if (nvec) *nvec = bd + 1;
        return MPSE_OK;
      }
    }
    if (defer) {
      pending_m = j + 1;
    } else if (check) {
      // successive estimates alternate between `out` and a spare buffer (no copies between checks); the typical
      // solve converges on its third estimate, which lands in `out`
      if (pending_m > 0) {
        MPSE_TRY(RES.alloc(size_t(n) * es));
        MPSE_TRY(finish(pending_m, out, nullptr, nullptr));
        res_prev = out;
        have_res = true;
        pending_m = 0;
      }
      if (!have_res) {
        MPSE_TRY(RES.alloc(size_t(n) * es));
        MPSE_TRY(finish(j + 1, out, nullptr, nullptr));
        res_prev = out;
        have_res = true;
      } else {
        void* dst = (res_prev == out) ? RES.p : out;
        int flag = 1;
        MPSE_TRY(finish(j + 1, dst, res_prev, &flag));
        res_prev = dst;
        if (flag == 0) {
          ++ctx->lz_paths[mpse_ctx::LP_CONV];
          if (dst != out) MPSE_TRY(mpse_memcpy_d2d(ctx, out, dst, size_t(n) * es));
          if (nvec) *nvec = j + 1;
          return MPSE_OK;
        }
      }
    }
    if (last) {
      ++ctx->lz_paths[mpse_ctx::LP_NOCONV];
      if (nvec) *nvec = j + 1;
      if (res_prev && res_prev != out) MPSE_TRY(mpse_memcpy_d2d(ctx, out, res_prev, size_t(n) * es));
      return mpse_fail(ctx, MPSE_ERR_NOCONV, "expm_lanczos: no convergence within %d Krylov vectors", max_dim);
    }
    if (j + 2 > cap) {  // grow the Krylov basis (krylov.py:63-68)
      ++ctx->lz_paths[mpse_ctx::LP_GROW];
      int ncap = cap * 2;
      TmpBuf V2(ctx);
      MPSE_TRY(V2.alloc(size_t(ncap) * n * es));
      MPSE_TRY(mpse_memcpy_d2d(ctx, V2.p, V.p, size_t(cap) * n * es));
      std::swap(V.p, V2.p);
      cap = ncap;
    }
    ProfScope sps(ctx, 4, 0.0, 2.0 * vbytes);
    MPSE_LAUNCH_TF(ctx, vec16, k_scale_into_dev, dim3(nb), dim3(RED_THREADS), (double*)vec(j + 1), W.as<const double>(),
                   (long long)nd, (const double*)part_b, nb, scal + 6 + 4 * j, (const int*)nullptr);
    sps.end();
  }
}

// One attempt at C as it is: the asynchronous solve where it applies, behind it the synchronous one.  LZ_BADSTART: |C|^2
// is outside what the recurrence takes (expm_lanczos_solve decides); the arguments are checked there.
int lanczos_attempt(mpse_ctx* ctx, int dtype, const mpse_heff* h, double dt_re, double dt_im, const void* Cin, void* out,
                    double rtol, double atol, int max_dim, int* nvec, int64_t n, bool async_first, const SolveHints& hints) {
  const std::complex<double> dt(dt_re, dt_im);
  if (async_first && lanczos_async_enabled() && n > 256) {
    const int st = expm_lanczos_async(ctx, dtype, h, dt, Cin, out, rtol, atol, max_dim, nvec, n, hints);
    if (st != LZ_FALLBACK) return st;
  }
  return expm_lanczos_sync(ctx, dtype, h, dt, Cin, out, rtol, atol, max_dim, nvec, n);
}

// The solve behind mpse_expm_lanczos and the members of a batch that run alone.  A start vector whose |C|^2 the recurrence
// cannot take as it is (LZ_BADSTART) is zero or not finite - an error - or a nonzero C whose squared norm is subnormal or
// beyond 1e300.  That one is solved as 2^e C, its largest element in [1, 2), with atol scaled alike, and the result scaled
// back by 2^-e: the same stopping decisions, exact scalings.  Rare, and outside every iteration: C goes through the host once.
// hints: the caller's centre mask and slot key for this solve (SolveHints; empty: none) - both attempts receive them.
int expm_lanczos_solve(mpse_ctx* ctx, int dtype, const mpse_heff* h, double dt_re, double dt_im, const void* Cin, void* out,
                       double rtol, double atol, int max_dim, int* nvec, const SolveHints& hints, bool async_first = true) {
  const bool cplx = dtype == MPSE_C128;
  if (!cplx && dt_im != 0.0)
    return mpse_fail(ctx, MPSE_ERR_ARG, "expm_lanczos: complex time step needs a complex128 centre tensor");
  const mpse_dims& s = h->dims;
  if ((s.Dl_bra > 0 && s.Dl_bra != s.Dl_ket) || (s.Dr_bra > 0 && s.Dr_bra != s.Dr_ket))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "expm_lanczos: the effective Hamiltonian must be square (bra bonds == ket bonds)");
  const int64_t anc = s.danc > 0 ? s.danc : 1;
  int64_t n = s.Dl_ket * s.Dr_ket;
  if (h->nsite >= 1) n *= s.d0 * anc;
  if (h->nsite == 2) n *= s.d1 * (s.danc1 > 0 ? s.danc1 : anc);
  if (n <= 0) return mpse_fail(ctx, MPSE_ERR_SHAPE, "expm_lanczos: empty centre tensor");
  if (max_dim <= 0 || max_dim > 128) max_dim = 128;
  {   // out may be C itself (every path reads C before it writes out, or restores it first), not part of it
    const char *c0 = static_cast<const char*>(Cin), *o0 = static_cast<const char*>(out);
    const size_t bytes = size_t(n) * dtype_size(dtype);
    if (o0 != c0 && o0 < c0 + bytes && c0 < o0 + bytes)
      return mpse_fail(ctx, MPSE_ERR_ARG, "expm_lanczos: out overlaps C without being C");
  }
  int st = lanczos_attempt(ctx, dtype, h, dt_re, dt_im, Cin, out, rtol, atol, max_dim, nvec, n, async_first, hints);
  if (st != LZ_BADSTART) return st;
  const int64_t nd = n * (cplx ? 2 : 1);
  std::vector<double> hv(static_cast<size_t>(nd));
  MPSE_TRY(mpse_memcpy_d2h(ctx, hv.data(), Cin, size_t(nd) * sizeof(double)));
  double mx = 0.0;
  for (double x : hv) {
    if (!std::isfinite(x)) return mpse_fail(ctx, MPSE_ERR_ARG, "expm_lanczos: non-finite start vector");
    mx = std::max(mx, std::fabs(x));
  }
  if (!(mx > 0.0)) return mpse_fail(ctx, MPSE_ERR_ARG, "expm_lanczos: zero start vector");
  const int e = -std::ilogb(mx);
  for (double& x : hv) x = std::ldexp(x, e);
  TmpBuf S(ctx);
  MPSE_TRY(S.alloc(size_t(nd) * sizeof(double)));
  MPSE_TRY(mpse_memcpy_h2d(ctx, S.p, hv.data(), size_t(nd) * sizeof(double)));
  ++ctx->lz_paths[mpse_ctx::LP_RESCALE];
  st = lanczos_attempt(ctx, dtype, h, dt_re, dt_im, S.p, out, rtol, std::ldexp(atol, e), max_dim, nvec, n, true, hints);
  if (st == LZ_BADSTART) return mpse_fail(ctx, MPSE_ERR_ARG, "expm_lanczos: start vector out of range after scaling");
  if (st == MPSE_OK || st == MPSE_ERR_NOCONV) {   // (NOCONV leaves its last estimate in out as well)
    hipLaunchKernelGGL((k_scal<false>), dim3(ew_blocks(nd)), dim3(256), 0, ctx->stream, (double*)out, (long long)nd,
                       std::ldexp(1.0, -e), 0.0);
    MPSE_HIP(ctx, hipGetLastError());
  }
  return st;
}

// ------------------------------------------------------------------------------------------------------------
// Batched solve (mpse_expm_lanczos_batch): B members of one shape whose matvec takes the one-launch small-centre path
// run as one launch set of lz_async_run.  Each member does the arithmetic of its single solve in the same order - the
// same kernels with the same grids per member - and stops its own kernels when its decision has fallen (LzCtl::stop).
struct BatchSet {
  const mpse_heff* h0;        // the shape (every member has the same nsite / dims / dtypes)
  std::vector<int> idx;       // member -> position in the caller's arrays
  int64_t n;
  int nparts, nb_dot;
  size_t rt_bytes;
};

// solves one launch set; members the batch cannot finish (need_host, bad start vector, the 64-vector limit) are marked in
// `single` and left for the caller (their start vectors are untouched: out may alias C only for finished members)
int expm_lanczos_batch_set(mpse_ctx* ctx, int dtype, const BatchSet& bs, const mpse_heff* hs, const void* const* Cs,
                           void* const* outs, std::complex<double> dt, double rtol, double atol, int max_dim, int* nvec,
                           std::vector<char>& single, std::vector<int>& st_out, std::vector<std::string>& msg) {
  const int B = (int)bs.idx.size();
  const int64_t n = bs.n;
  const size_t es = dtype_size(dtype);
  const unsigned long long key = lz_hint_key(bs.h0->nsite, n, dtype == MPSE_C128);
  TmpBuf RT(ctx), MEM(ctx);
  MPSE_TRY(RT.alloc(size_t(B) * bs.rt_bytes));
  MPSE_TRY(MEM.alloc(size_t(B) * sizeof(BatchMember)));
  std::vector<BatchMember> mh(B);
  for (int m = 0; m < B; ++m) {
    const mpse_heff& h = hs[bs.idx[m]];
    mh[m] = BatchMember{h.L, h.R, h.W0, RT.as<char>() + size_t(m) * bs.rt_bytes, Cs[bs.idx[m]], outs[bs.idx[m]]};
  }
  MPSE_TRY(stage_h2d(ctx, MEM.p, mh.data(), mh.size() * sizeof(BatchMember)));
  const BatchMember* mem = MEM.as<const BatchMember>();
  auto matvec = [&](const LzIter& it, LzMatvecOut* r) -> int {
    // (the transposed environments wait for k_lz_start: it clears the stop words their launch looks at)
    if (it.j == 0) MPSE_TRY(heff_small_batch_rt(ctx, dtype, bs.h0, B, mem, it.stop, it.mstride));
    r->nparts = bs.nparts, r->a_nb = bs.nb_dot;
    return heff_small_batch_apply(ctx, dtype, bs.h0, B, mem, it.u, it.parts, n, it.dot, LZ_DOT_CAP, it.stop, it.mstride);
  };
  // (members are grouped only when every Krylov vector starts on a 16-byte boundary; no part or centre masks)
  const LzProblem p{dtype, n, B, mem, nullptr, nullptr, dt, rtol, atol, true, nullptr, 0, 0, bs.nparts, bs.nb_dot};
  LzSet set(ctx);
  std::vector<LzOutcome> oc(B);
  LzTally tally;   // (a batch counts its members, not their paths: mpse_expm_lanczos_batch_stats)
  MPSE_TRY(lz_async_run(ctx, p, LzSchedule(lz_hint(ctx, key), max_dim), set, matvec, oc.data(), &tally));
  int best = 0;
  for (int m = 0; m < B; ++m) {
    if (oc[m].kind != LzOutcome::DONE) {
      single[m] = 1;
      continue;
    }
    if (oc[m].which == 1)
      MPSE_TRY(mpse_memcpy_d2d(ctx, outs[bs.idx[m]], set.at(set.lay.spare, m), size_t(n) * es));
    if (nvec) nvec[bs.idx[m]] = oc[m].nvec;
    if (oc[m].nvec > best) best = oc[m].nvec;
    st_out[bs.idx[m]] = MPSE_OK;
  }
  if (best > 0) ctx->lz_hint[key] = best;
  // members the batch could not finish: the single solve from the copy of their start vector in the basis (bitwise C;
  // out may alias C).  Where their own asynchronous solve would hand over to the synchronous one (need_host, the vector
  // limit), that one runs directly - it starts from C and does not depend on the attempt before it
  for (int m = 0; m < B; ++m) {
    if (!single[m]) continue;
    const int i = bs.idx[m];
    int nv = 0;
    const int st = expm_lanczos_solve(ctx, dtype, &hs[i], dt.real(), dt.imag(), set.at(set.lay.basis, m), outs[i], rtol,
                                      atol, max_dim, &nv, SolveHints(), oc[m].kind == LzOutcome::BAD);
    if (nvec) nvec[i] = nv;
    st_out[i] = st;
    if (st != MPSE_OK) msg[i] = ctx->err;
  }
  return MPSE_OK;
}


}  // namespace

extern "C" {

int mpse_expm_centre_mask(mpse_ctx* ctx, const void* mask_dev, int64_t nbytes) {
  if (!ctx || (nbytes > 0 && !mask_dev) || nbytes < 0) return MPSE_ERR_ARG;
  ctx->cmask_pending = mpse_ctx::CMask();
  if (nbytes > 0) {
    ctx->cmask_pending.ptr = mask_dev;
    ctx->cmask_pending.bytes = nbytes;
  }
  return MPSE_OK;
}

int mpse_expm_lanczos(mpse_ctx* ctx, int dtype, const mpse_heff* h, double dt_re, double dt_im, const void* Cin,
                      void* out, double rtol, double atol, int max_dim, int* nvec) {
  if (!ctx || !h || !Cin || !out) return MPSE_ERR_ARG;
  if (MPSE_RECORDING(ctx)) return mpse_fail(ctx, MPSE_ERR_ARG, "expm_lanczos: cannot be recorded (mpse_defer_begin is open)");
  MPSE_BIND(ctx);
  // calls recorded by the caller for the time the result exists (QR of the new centre, environment update, absorption
  // of a bond factor) are issued here, before control goes back to the host language
  // a mask is good for the one solve it was set for, whatever path that takes: it leaves the context here
  SolveHints hints;
  hints.cmask = std::exchange(ctx->cmask_pending, mpse_ctx::CMask());
  hints.slot_key = std::exchange(ctx->slot_pending, 0LL);    // (the same rule for the key of the solve, mpse_solve_slot)
  const int st = expm_lanczos_solve(ctx, dtype, h, dt_re, dt_im, Cin, out, rtol, atol, max_dim, nvec, hints);
  return defer_replay(ctx, st);
}

int mpse_expm_lanczos_batch(mpse_ctx* ctx, int dtype, int count, const mpse_heff* h, double dt_re, double dt_im,
                            const void* const* C, void* const* out, double rtol, double atol, int max_dim, int* nvec) {
  if (!ctx || count < 0 || (count > 0 && (!h || !C || !out))) return MPSE_ERR_ARG;
  if (MPSE_RECORDING(ctx))
    return mpse_fail(ctx, MPSE_ERR_ARG, "expm_lanczos_batch: cannot be recorded (mpse_defer_begin is open)");
  if (count == 0) return MPSE_OK;
  MPSE_BIND(ctx);
  const int md = (max_dim <= 0 || max_dim > 128) ? 128 : max_dim;
  const bool cplx = dtype == MPSE_C128;
  std::vector<int> st(count, MPSE_OK);
  std::vector<std::string> msg(count);
  std::vector<char> grouped(count, 0);
  // launch sets: members of one shape, in the order of their first appearance, up to LZB_MAX each
  std::vector<BatchSet> sets;
  if (lanczos_async_enabled() && !(!cplx && dt_im != 0.0)) {
    std::vector<BatchSet> open;   // (the last set of each shape, while it has room)
    for (int i = 0; i < count; ++i) {
      const mpse_heff& hi = h[i];
      if (!C[i] || !out[i] || !hi.L || !hi.R) continue;
      const mpse_dims& s = hi.dims;
      if ((s.Dl_bra > 0 && s.Dl_bra != s.Dl_ket) || (s.Dr_bra > 0 && s.Dr_bra != s.Dr_ket)) continue;
      int64_t n = s.Dl_ket * s.Dr_ket;
      if (hi.nsite >= 1) n *= s.d0 * (s.danc > 0 ? s.danc : 1);
      if (hi.nsite != 0 && hi.nsite != 1) continue;
      if (n <= 256) continue;
      if (!((cplx || n % 2 == 0) && (reinterpret_cast<uintptr_t>(C[i]) & 15) == 0)) continue;
      {   // (an out that overlaps C without being C: the single solve refuses it)
        const char *c0 = static_cast<const char*>(C[i]), *o0 = static_cast<const char*>(out[i]);
        const size_t bytes = size_t(n) * (cplx ? 16 : 8);
        if (o0 != c0 && o0 < c0 + bytes && c0 < o0 + bytes) continue;
      }
      size_t rtb = 0;
      int np = 0, nbd = 0;
      if (!heff_small_batch_plan(&hi, dtype, n, LZ_DOT_CAP, &rtb, &np, &nbd)) continue;
      BatchSet* tgt = nullptr;
      for (auto& o : open) {
        const mpse_heff& h0 = *o.h0;
        if (h0.nsite == hi.nsite && memcmp(&h0.dims, &hi.dims, sizeof(mpse_dims)) == 0 && h0.l_dtype == hi.l_dtype &&
            h0.r_dtype == hi.r_dtype && h0.w_dtype == hi.w_dtype && (h0.W0 != nullptr) == (hi.W0 != nullptr)) {
          tgt = &o;
          break;
        }
      }
      if (tgt && (int)tgt->idx.size() == LZB_MAX) {
        sets.push_back(*tgt);
        tgt->idx.clear();
      }
      if (!tgt) {
        open.push_back(BatchSet{&hi, {}, n, np, nbd, rtb});
        tgt = &open.back();
      }
      tgt->idx.push_back(i);
    }
    for (auto& o : open) sets.push_back(o);
  }
  for (const BatchSet& bs : sets) {
    if (bs.idx.size() < 2) continue;    // (one member alone: its own solve)
    std::vector<char> single(bs.idx.size(), 0);
    MPSE_TRY(expm_lanczos_batch_set(ctx, dtype, bs, h, C, out, std::complex<double>(dt_re, dt_im), rtol, atol, md, nvec,
                                    single, st, msg));
    for (size_t m = 0; m < bs.idx.size(); ++m) {
      grouped[bs.idx[m]] = 1;
      if (single[m])
        ++ctx->lz_batch_single;
      else
        ++ctx->lz_batch_members;
    }
  }
  for (int i = 0; i < count; ++i) {
    if (grouped[i]) continue;
    ++ctx->lz_batch_single;
    if (!C[i] || !out[i]) {
      st[i] = mpse_fail(ctx, MPSE_ERR_ARG, "expm_lanczos: null vector");
      msg[i] = ctx->err;
      continue;
    }
    int nv = 0;
    st[i] = expm_lanczos_solve(ctx, dtype, &h[i], dt_re, dt_im, C[i], out[i], rtol, atol, max_dim, &nv, SolveHints());
    if (nvec) nvec[i] = nv;
    if (st[i] != MPSE_OK) msg[i] = ctx->err;
  }
  int status = MPSE_OK;
  for (int i = 0; i < count; ++i)
    if (st[i] != MPSE_OK) {
      status = mpse_fail(ctx, st[i], "expm_lanczos_batch: member %d: %s", i, msg[i].c_str());
      break;
    }
  return defer_replay(ctx, status);
}

int mpse_expm_lanczos_path_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  if (!ctx || n < 0 || (n > 0 && !counts)) return MPSE_ERR_ARG;
  for (int i = 0; i < n && i < mpse_ctx::LP_COUNT; ++i) counts[i] = ctx->lz_paths[i];
  return MPSE_OK;
}

int mpse_expm_lanczos_batch_stats(mpse_ctx* ctx, int64_t* batched_members, int64_t* single_members) {
  if (!ctx) return MPSE_ERR_ARG;
  if (batched_members) *batched_members = ctx->lz_batch_members;
  if (single_members) *single_members = ctx->lz_batch_single;
  return MPSE_OK;
}

}  // extern "C"
