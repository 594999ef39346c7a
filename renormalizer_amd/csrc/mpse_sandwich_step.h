// The site step of the transfer tensor with an MPO site in between, E (Db, w, Dk) -> E' (Db', w', Dk'), as one
// workgroup takes it with E in LDS: shared by k_sandwich_chain (mpse_sandwich.hip, every site of two chains) and
// k_expect_windows (mpse_expect.hip, the window of one operator on ONE chain); no other file includes this.
#pragma once
#include "mpse_chain.h"

// entries of the new E a thread accumulates in registers over (sigma, a): SW_PLANES entries (b', k') of the plane
// Dbr x Dkr, each in all of the up to SW_CHANNELS outgoing MPO channels g'
constexpr int SW_PLANES = 2;
constexpr int SW_CHANNELS = 8;
constexpr int SW_ACC = SW_PLANES * SW_CHANNELS;

struct SwSite {   // one row of the descriptor table (72 bytes, uploaded once per call)
  const void* bra;
  const void* ket;
  const void* w;
  int Dbl, Dkl, wl, d, danc, Dbr, Dkr, wr;
  int bra_c, ket_c, w_c;   // the tensor is complex128
  int pad;
};
static_assert(sizeof(SwSite) == 72, "descriptor rows are copied as 8-byte words");

// Per (sigma, a) in ascending order:
//   T[b, g, k'] = sum_k E[b, g, k] K[k, sigma, a, k']                                     (into LDS)
//   for every (sigma', g) whose row W[g, sigma', sigma, :] holds a non-zero entry:
//     S[b', k']       = sum_b op(B[b, sigma', a, b']) T[b, g, k']                          (register of the owner)
//     E'[b', g', k'] += W[g, sigma', sigma, g'] S[b', k']   for the non-zero entries g'    (registers of the owner)
// E' replaces E in LDS after the last (sigma, a).  Rows (b, g) of E are padded to Dk | 1 elements.  A thread owns the
// entries (b', k') = tid + jj * CHAIN_THREADS, jj < SW_PLANES, of every channel g' < SW_CHANNELS: SW_ACC accumulators,
// all indexed statically (the plan of the caller keeps a site inside them).  (b', k') runs with k' fastest: the reads
// of K are contiguous, those of T conflict free, B[b, sigma', a, b'] is one address per b' group.  The caller has
// passed a barrier behind the last write of E; ends with the barrier behind which the new E is read.
template <bool CPLX>
__device__ __forceinline__ void sw_site_step(const SwSite& s, int conj_bra, ChainT<CPLX>* E, ChainT<CPLX>* Ts) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int tid = threadIdx.x;
  const int Dbl = s.Dbl, Dkl = s.Dkl, wl = s.wl, d = s.d, danc = s.danc, Dbr = s.Dbr, Dkr = s.Dkr, wr = s.wr;
  const int pe = Dkl | 1, pe_new = Dkr | 1;
  const int nT = Dbl * wl * Dkr, P = Dbr * Dkr;
  const int p = d * danc;
  const int k_row = p * Dkr, b_row = p * Dbr, t_row = wl * Dkr;   // element strides of the left bond in K, B and T
  const bool cj = conj_bra != 0 && s.bra_c != 0;
  T acc[SW_PLANES][SW_CHANNELS];
#pragma unroll
  for (int jj = 0; jj < SW_PLANES; ++jj)
#pragma unroll
    for (int gp = 0; gp < SW_CHANNELS; ++gp) acc[jj][gp] = El::zero();
  for (int sa = 0; sa < p; ++sa) {
    const int sg = sa / danc, a = sa - sg * danc;
    for (int o = tid; o < nT; o += CHAIN_THREADS) {
      const int r = o / Dkr, kk = o - r * Dkr;
      const T* e_row = E + r * pe;
      const int k0 = sa * Dkr + kk;
      T sum = El::zero();
#pragma unroll 4
      for (int k = 0; k < Dkl; ++k) El::fma(sum, e_row[k], El::ld(s.ket, s.ket_c, k * k_row + k0));
      Ts[o] = sum;
    }
    __syncthreads();
    for (int sp = 0; sp < d; ++sp) {
      for (int g = 0; g < wl; ++g) {
        const int w0 = ((g * d + sp) * d + sg) * wr;
        bool any = false;
        for (int gp = 0; gp < wr; ++gp) any = any || El::nz(El::ldc(s.w, s.w_c, w0 + gp));
        if (!any) continue;
        const int b_base = (sp * danc + a) * Dbr;
#pragma unroll
        for (int jj = 0; jj < SW_PLANES; ++jj) {
          const int o = tid + jj * CHAIN_THREADS;
          if (jj * CHAIN_THREADS >= P) break;
          T S = El::zero();
          if (o < P) {
            const int bb = o / Dkr, kk = o - bb * Dkr;
            const T* t_col = Ts + g * Dkr + kk;
            const int b0 = b_base + bb;
#pragma unroll 2
            for (int b = 0; b < Dbl; ++b) {
              T v = El::ld(s.bra, s.bra_c, b * b_row + b0);
              if (cj) v = El::cj(v);
              El::fma(S, v, t_col[b * t_row]);
            }
          }
#pragma unroll
          for (int gp = 0; gp < SW_CHANNELS; ++gp) {
            if (gp < wr) {
              const T w = El::ldc(s.w, s.w_c, w0 + gp);
              if (El::nz(w)) El::fma(acc[jj][gp], w, S);
            }
          }
        }
      }
    }
    __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of E is done as well
  }
#pragma unroll
  for (int jj = 0; jj < SW_PLANES; ++jj) {
    const int o = tid + jj * CHAIN_THREADS;
    if (o < P) {
      const int bb = o / Dkr, kk = o - bb * Dkr;
      T* e_new = E + bb * wr * pe_new + kk;
#pragma unroll
      for (int gp = 0; gp < SW_CHANNELS; ++gp)
        if (gp < wr) e_new[gp * pe_new] = acc[jj][gp];
    }
  }
  __syncthreads();
}
