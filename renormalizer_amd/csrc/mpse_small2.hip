// Two-layer effective-Hamiltonian matvec of SMALL one-site centres as ONE launch, for the batched conjugate gradients of
// mpse_pcg_batch (the correction-vector centre systems ((H - omega)^2 + eta^2) x = b of many frequencies at once).
//
//   out[d,h,k] = sum L[a,b,c,d] W[b,e,f,g] W[c,f,h,i] R[j,g,i,k] C[a,e,j]        (mps/hop_expr.py:24-38)
//
// At bond dimensions of a few tens the plans of mpse_heff_apply2 are several strided-GEMM launches on a vector of a few
// thousand elements.  Cut along the result bond d of L the chain needs no exchange between workgroups, and every step
// before the last is pointwise in the ket bond j of R, so the workgroup of row d walks over slices [j0, j0 + jh) of j:
//   T1[(b,c),(e,jj)] = sum_a Lt[d,b,c,a] C[a,e,j0+jj]              (wl^2 x d jh, LDS)
//   T2[c,f,g,jj]     = sum_{b,e} W[b,e,f,g] T1[(b,c),(e,jj)]        (LDS; W as a sparse list in LDS)
//   T3[h,(jj,g,i)]   = sum_{c,f} W[c,f,h,i] T2[c,f,g,jj]            (LDS, over T1)
//   acc[h,k]        += sum_q T3[h,q] R[(j0 wr^2 + q), k]            (registers; the rows (j,g,i) of R are contiguous in k)
// with FP64 vector FMAs (products a few rows tall).  The slice width jh is what the intermediates leave of the LDS budget,
// so the limit on the centre is set by the row of L and the sparse list, not by the intermediates.  Both W steps read ONE
// list: row (x, y) holds the non-zero W[u, v, x, y] as (u, v).  Lt[d,b,c,a] = L[a,b,c,d] (R needs no copy: its result bond
// is its last index) and the list are made once per solve by k_small2_prep_b.
//
// The launch ends with the first vector pass of a conjugate-gradient iteration: q = mask * y + shift * p and one partial
// sum of p^H q per workgroup, in a fixed order.  Member blockIdx.z takes everything from its entry of the member table.
#include <algorithm>

#include "mpse_device.h"
#include "mpse_internal.h"

namespace {

constexpr int S2_THREADS = RED_THREADS;
constexpr int S2_RB = 8;      // rows (b, c) of T1 per work item

template <bool CPLX>
struct El;
template <>
struct El<true> {
  using T = double2;
  static __device__ __forceinline__ T zero() { return make_double2(0.0, 0.0); }
  static __device__ __forceinline__ void mad(T& acc, const T a, const T b) {
    acc.x = fma(a.x, b.x, acc.x);
    acc.x = fma(-a.y, b.y, acc.x);
    acc.y = fma(a.x, b.y, acc.y);
    acc.y = fma(a.y, b.x, acc.y);
  }
  static __device__ __forceinline__ void mad_real(T& acc, const double w, const T b) {
    acc.x = fma(w, b.x, acc.x);
    acc.y = fma(w, b.y, acc.y);
  }
  static __device__ __forceinline__ void add(T& acc, const T b) { acc.x += b.x, acc.y += b.y; }
  static __device__ __forceinline__ T axpby(double m, const T y, double s, const T p) {
    return make_double2(m * y.x + s * p.x, m * y.y + s * p.y);
  }
  static __device__ __forceinline__ double re_dotc(const T a, const T b) { return a.x * b.x + a.y * b.y; }
};
template <>
struct El<false> {
  using T = double;
  static __device__ __forceinline__ T zero() { return 0.0; }
  static __device__ __forceinline__ void mad(T& acc, const T a, const T b) { acc = fma(a, b, acc); }
  static __device__ __forceinline__ void mad_real(T& acc, const double w, const T b) { acc = fma(w, b, acc); }
  static __device__ __forceinline__ void add(T& acc, const T b) { acc += b; }
  static __device__ __forceinline__ T axpby(double m, const T y, double s, const T p) { return m * y + s * p; }
  static __device__ __forceinline__ double re_dotc(const T a, const T b) { return a * b; }
};

// ---- once per solve: Lt[d,b,c,a] = L[a,b,c,d] and the sparse list of W (workgroup 0 of the member)
template <bool CPLX>
__global__ __launch_bounds__(S2_THREADS) void k_small2_prep_b(const Small2Plan g, const Pcg2Member* __restrict__ mem) {
  using T = typename El<CPLX>::T;
  const Pcg2Member mb = mem[blockIdx.z];
  const int Dl = g.Dl, ww = g.wl * g.wl;
  const T* L = reinterpret_cast<const T*>(mb.L);
  T* Lt = reinterpret_cast<T*>(mb.Lt);
  const long long n = (long long)Dl * ww * Dl;
  const long long stride = (long long)gridDim.x * S2_THREADS;
  for (long long i = (long long)blockIdx.x * S2_THREADS + threadIdx.x; i < n; i += stride) {
    const int a = (int)(i % Dl);
    const long long t = i / Dl;            // d * ww + bc
    const int bc = (int)(t % ww), dd = (int)(t / ww);
    Lt[i] = L[((long long)a * ww + bc) * Dl + dd];
  }
  if (blockIdx.x != 0) return;
  __shared__ int s_cnt[SM2_DMAX * SM2_WMAX + 1];
  const int d = g.d, wl = g.wl, wr = g.wr, rows = g.rows, pitch = g.pitch;
  const double* W = mb.W;
  const int r = threadIdx.x;
  int cnt = 0;
  if (r < rows) {
    const int x = r / wr, y = r - x * wr;
    for (int u = 0; u < wl; ++u)
      for (int v = 0; v < d; ++v)
        if (W[(((long long)u * d + v) * d + x) * wr + y] != 0.0) ++cnt;
    s_cnt[r] = cnt;
  }
  __syncthreads();
  if (r == 0) {
    int run = 0;
    for (int i = 0; i < rows; ++i) {
      const int c = s_cnt[i];
      s_cnt[i] = run;
      run += c;
    }
    s_cnt[rows] = run;
  }
  __syncthreads();
  if (r <= rows) mb.csr_ptr[r] = s_cnt[r];
  if (r < rows) {
    const int x = r / wr, y = r - x * wr;
    int o = s_cnt[r];
    for (int u = 0; u < wl; ++u)
      for (int v = 0; v < d; ++v) {
        const double w = W[(((long long)u * d + v) * d + x) * wr + y];
        if (w != 0.0) {
          mb.csr_idx[o] = (u << 8) | v;
          mb.csr_val[o] = w;
          ++o;
        }
      }
  }
  (void)pitch;
}

// last step of one slice: acc[x] += sum over q = grp, grp + G, .. < Kc of T3[x, q] R[row0 + q, k]
template <bool CPLX, int DX>
__device__ __forceinline__ void small2_last(typename El<CPLX>::T (&acc)[SM2_DMAX], const typename El<CPLX>::T* __restrict__ Rrow,
                                            const typename El<CPLX>::T* sT3, int K3, int Kc, int G, int grp, int Dr, int d) {
  using E = El<CPLX>;
  using T = typename E::T;
  int q = grp;
  for (; q + 3 * G < Kc; q += 4 * G) {
    T rv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) rv[u] = Rrow[(long long)(q + u * G) * Dr];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int x = 0; x < DX; ++x)
        if (x < d) E::mad(acc[x], sT3[x * K3 + q + u * G], rv[u]);
  }
  for (; q < Kc; q += G) {
    const T rv = Rrow[(long long)q * Dr];
#pragma unroll
    for (int x = 0; x < DX; ++x)
      if (x < d) E::mad(acc[x], sT3[x * K3 + q], rv);
  }
}

// mode 0: y = Heff2 x (the start residual's matvec); mode 1: q = mask * Heff2 p + shift * p and the partial of p^H q
template <bool CPLX>
__global__ __launch_bounds__(S2_THREADS) void k_heff2_small_b(const Small2Plan g, const Pcg2Member* __restrict__ mem, int mode) {
  using E = El<CPLX>;
  using T = typename E::T;
  const Pcg2Member mb = mem[blockIdx.z];
  if (*reinterpret_cast<const int*>(mb.ctl)) return;      // the member's decision has fallen
  extern __shared__ __attribute__((aligned(16))) double smem2[];
  const int tid = threadIdx.x;
  const int d0 = blockIdx.x;
  const int Dl = g.Dl, Dr = g.Dr, d = g.d, wl = g.wl, wr = g.wr, jh = g.jh;
  const int ww = wl * wl, N1 = d * Dr, N1h = d * jh, K3 = jh * wr * wr, rows = g.rows;
  int* s_ptr = reinterpret_cast<int*>(smem2);
  int* s_idx = reinterpret_cast<int*>(smem2 + g.ptr_dbl);
  double* s_val = smem2 + g.ptr_dbl + g.idx_dbl;
  T* s_el = reinterpret_cast<T*>(smem2 + g.csr_dbl);
  T* sL = s_el;
  T* sA = s_el + g.off_A;      // T1, then T3, at the end the K-group partials
  T* sB = s_el + g.off_B;      // T2

  // ---- the row of Lt and the sparse list (its head: what fits the LDS area; the tail is read from memory)
  {
    const T* Lrow = reinterpret_cast<const T*>(mb.Lt) + (long long)d0 * ww * Dl;
    for (int i = tid; i < ww * Dl; i += S2_THREADS) sL[i] = Lrow[i];
    for (int i = tid; i <= rows; i += S2_THREADS) s_ptr[i] = mb.csr_ptr[i];
  }
  __syncthreads();
  const int nnz = s_ptr[rows];
  const int nl = nnz < g.nnz_lds ? nnz : g.nnz_lds;
  for (int i = tid; i < nl; i += S2_THREADS) {
    s_idx[i] = mb.csr_idx[i];
    s_val[i] = mb.csr_val[i];
  }
  const int* __restrict__ g_idx = mb.csr_idx;
  const double* __restrict__ g_val = mb.csr_val;

  const T* __restrict__ Cm = reinterpret_cast<const T*>(mode ? mb.p : mb.x);
  const T* __restrict__ Rm = reinterpret_cast<const T*>(mb.R);
  const int G = g.G;
  const int grp = tid / Dr, kcol = tid - grp * Dr;
  const bool on = grp < G;
  T acc[SM2_DMAX];
#pragma unroll
  for (int x = 0; x < SM2_DMAX; ++x) acc[x] = E::zero();

  const int nrg = (ww + S2_RB - 1) / S2_RB;
  for (int j0 = 0; j0 < Dr; j0 += jh) {
    const int jc = Dr - j0 < jh ? Dr - j0 : jh;
    __syncthreads();      // the list is in place; the last slice's reads of T3 are done
    // ---- T1[(b,c),(e,jj)] = sum_a Lt[d0,b,c,a] C[a,e,j0+jj]   (columns beyond the slice: zero)
    for (int it = tid; it < nrg * N1h; it += S2_THREADS) {
      const int rg = it / N1h, col = it - rg * N1h;
      const int e = col / jh, jj = col - e * jh;
      const bool live = jj < jc;
      const int r0 = rg * S2_RB;
      T a8[S2_RB];
#pragma unroll
      for (int r = 0; r < S2_RB; ++r) a8[r] = E::zero();
      if (live) {
        const T* cp = Cm + e * Dr + j0 + jj;
        for (int a = 0; a < Dl; ++a) {
          const T cv = cp[(long long)a * N1];
#pragma unroll
          for (int r = 0; r < S2_RB; ++r) {
            const int row = r0 + r < ww ? r0 + r : ww - 1;
            E::mad(a8[r], sL[row * Dl + a], cv);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < S2_RB; ++r)
        if (r0 + r < ww) sA[(r0 + r) * N1h + col] = a8[r];
    }
    __syncthreads();
    // ---- T2[c,f,g,jj] = sum_{(b,e) in row (f,g)} W[b,e,f,g] T1[(b,c),(e,jj)]
    for (int o = tid; o < wl * d * wr * jh; o += S2_THREADS) {
      const int jj = o % jh;
      int t = o / jh;
      const int gg = t % wr;
      t /= wr;
      const int f = t % d, c = t / d;
      const int r = f * wr + gg;
      T s = E::zero();
      for (int q = s_ptr[r]; q < s_ptr[r + 1]; ++q) {
        const int id = q < nl ? s_idx[q] : g_idx[q];
        const double w = q < nl ? s_val[q] : g_val[q];
        const int b = id >> 8, e = id & 255;
        E::mad_real(s, w, sA[((b * wl + c) * d + e) * jh + jj]);
      }
      sB[o] = s;
    }
    __syncthreads();
    // ---- T3[h,(jj,g,i)] = sum_{(c,f) in row (h,i)} W[c,f,h,i] T2[c,f,g,jj]
    for (int o = tid; o < d * K3; o += S2_THREADS) {
      const int h = o / K3, q3 = o - h * K3;
      const int i = q3 % wr;
      int t = q3 / wr;
      const int gg = t % wr, jj = t / wr;
      const int r = h * wr + i;
      T s = E::zero();
      for (int q = s_ptr[r]; q < s_ptr[r + 1]; ++q) {
        const int id = q < nl ? s_idx[q] : g_idx[q];
        const double w = q < nl ? s_val[q] : g_val[q];
        const int c = id >> 8, f = id & 255;
        E::mad_real(s, w, sB[((c * d + f) * wr + gg) * jh + jj]);
      }
      sA[o] = s;
    }
    __syncthreads();
    // ---- acc[h,k] += sum_q T3[h,q] R[(j0,0,0) + q, k]
    if (on) {
      const T* Rrow = Rm + (long long)j0 * wr * wr * Dr + kcol;
      const int Kc = jc * wr * wr;
      if (d <= 2)
        small2_last<CPLX, 2>(acc, Rrow, sA, K3, Kc, G, grp, Dr, d);
      else if (d <= 4)
        small2_last<CPLX, 4>(acc, Rrow, sA, K3, Kc, G, grp, Dr, d);
      else if (d <= 8)
        small2_last<CPLX, 8>(acc, Rrow, sA, K3, Kc, G, grp, Dr, d);
      else
        small2_last<CPLX, 16>(acc, Rrow, sA, K3, Kc, G, grp, Dr, d);
    }
  }
  __syncthreads();
  if (on) {
#pragma unroll
    for (int x = 0; x < SM2_DMAX; ++x)
      if (x < d) sA[(grp * d + x) * Dr + kcol] = acc[x];
  }
  __syncthreads();
  // ---- the K groups in a fixed order, then the first vector pass of the iteration
  double pq = 0.0, zero = 0.0;
  const long long row = (long long)d0 * N1;
  T* yrow = reinterpret_cast<T*>(mode ? mb.q : mb.y) + row;
  const T* prow = Cm + row;
  const double* mrow = mb.mask ? mb.mask + row : nullptr;
  for (int i = tid; i < N1; i += S2_THREADS) {
    T s = sA[i];
    for (int q = 1; q < G; ++q) E::add(s, sA[q * N1 + i]);
    if (mode) {
      const T pv = prow[i];
      const T qv = E::axpby(mrow ? mrow[i] : 1.0, s, mb.shift, pv);
      yrow[i] = qv;
      pq += E::re_dotc(pv, qv);
    } else {
      yrow[i] = s;
    }
  }
  if (mode) {      // (uniform over the launch)
    block_allsum2(pq, zero);
    if (tid == 0) {
      mb.part_pq[2 * d0] = pq;
      mb.part_pq[2 * d0 + 1] = 0.0;
    }
  }
}

}  // namespace

bool small2_plan(int dtype, int64_t Dl, int64_t d, int64_t Dr, int64_t wl, int64_t wr, Small2Plan* p) {
  if (dtype != MPSE_F64 && dtype != MPSE_C128) return false;
  if (Dl < 1 || Dr < 1 || d < 1 || wl < 1 || wr < 1) return false;
  if (Dl > SM2_BMAX || Dr > SM2_BMAX || d > SM2_DMAX || wl > SM2_WMAX || wr > SM2_WMAX) return false;
  const int64_t es = dtype == MPSE_C128 ? 16 : 8;
  const int64_t rows = d * wr, pitch = wl * d;
  const int64_t nnz_lds = std::min<int64_t>(rows * pitch, SM2_NNZ_LDS);
  const int64_t ptr_dbl = (rows + 2) / 2, idx_dbl = (nnz_lds + 1) / 2;
  const int64_t csr_dbl = (ptr_dbl + idx_dbl + nnz_lds + 1) & ~int64_t(1);
  const int64_t wmax = std::max(wl, wr);
  const int64_t len_L = wl * wl * Dl;
  // elements of the working type left beside the sparse list and the row of Lt
  const int64_t avail = (SM2_LDS_MAX - 256 - csr_dbl * 8) / es - len_L;    // (256: the static words of the block reduction)
  const int64_t per_j = wmax * wmax * d + wl * d * wr;                     // T1 / T3 and T2 per ket-bond state of a slice
  if (avail < per_j) return false;
  int64_t jh = std::min<int64_t>(Dr, avail / per_j);
  const int64_t nslice = (Dr + jh - 1) / jh;
  jh = (Dr + nslice - 1) / nslice;
  // K groups of the last step: what the threads allow, the slice offers and the area for their partials holds
  const int64_t G = std::min<int64_t>(std::min<int64_t>(S2_THREADS / Dr, jh * wr * wr), avail / (d * Dr));
  if (G < 1) return false;
  const int64_t lenA = wmax * wmax * d * jh;
  const int64_t lds = csr_dbl * 8 + (len_L + std::max(per_j * jh, G * d * Dr)) * es;
  *p = Small2Plan{};
  p->Dl = (int)Dl, p->Dr = (int)Dr, p->d = (int)d, p->wl = (int)wl, p->wr = (int)wr;
  p->jh = (int)jh, p->nslice = (int)nslice, p->G = (int)G;
  p->rows = (int)rows, p->pitch = (int)pitch, p->nnz_lds = (int)nnz_lds;
  p->ptr_dbl = (int)ptr_dbl, p->idx_dbl = (int)idx_dbl, p->csr_dbl = (int)csr_dbl;
  p->off_A = (int)len_L, p->off_B = (int)(len_L + lenA);
  p->lds = (int)lds;
  return true;
}

int small2_prep(mpse_ctx* ctx, int dtype, const Small2Plan& p, int B, const Pcg2Member* mem) {
  const long long n = (long long)p.Dl * p.wl * p.wl * p.Dl;
  int nb = int((n + S2_THREADS - 1) / S2_THREADS);
  if (nb > 64) nb = 64;
  const dim3 grid((unsigned)nb, 1, (unsigned)B);
  if (dtype == MPSE_C128)
    hipLaunchKernelGGL((k_small2_prep_b<true>), grid, dim3(S2_THREADS), 0, ctx->stream, p, mem);
  else
    hipLaunchKernelGGL((k_small2_prep_b<false>), grid, dim3(S2_THREADS), 0, ctx->stream, p, mem);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

int small2_apply(mpse_ctx* ctx, int dtype, const Small2Plan& p, int B, const Pcg2Member* mem, int mode) {
  const dim3 grid((unsigned)p.Dl, 1, (unsigned)B);
  if (dtype == MPSE_C128)
    hipLaunchKernelGGL((k_heff2_small_b<true>), grid, dim3(S2_THREADS), (size_t)p.lds, ctx->stream, p, mem, mode);
  else
    hipLaunchKernelGGL((k_heff2_small_b<false>), grid, dim3(S2_THREADS), (size_t)p.lds, ctx->stream, p, mem, mode);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}
