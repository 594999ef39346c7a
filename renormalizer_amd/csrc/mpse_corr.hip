// mpse_mps_corr: the matrix C[k, l] = <psi| X_k Y_l |psi> (k < l), C[k, k] = <psi| Z_k |psi> of one-site operators on
// selected sites of ONE chain as one engine call (the reference takes every entry as its own MPO expectation,
// mps/mps.py:1657-1687 calc_edof_rdm).  Two paths, chosen from the dims table alone (corr_plan):
//   chain      two launches, for chains whose bonds are at most CR_BOND_MAX.  k_corr_right: one workgroup walks right to
//              left with the identity environment R in LDS and leaves, at every selected site l, the closed
//              environments G_l (with Y_l) and Gd_l (with Z_l) in pooled memory.  k_corr_rows: workgroup k walks left to right with the transfer matrix E in LDS, opens with X_k at
//              site sel[k] and closes against G_l at every later selected site.  A workgroup reads only what the launch
//              before it wrote: no flag, no spin wait, no atomic.
//   enqueued   the same two passes as products of the contraction kernel; the open rows are one stack of environments
//              that grows by a row per selected site - every other chain
// The host reads once, at the end.  A fixed summation order: the same inputs give the same bits.
#include "mpse_chain.h"

namespace {

constexpr int CR_WAVES = CHAIN_THREADS / 64;
constexpr int CR_OUT_PER_THREAD = 4;      // entries of a new environment a thread accumulates in registers
// rows of E / R and of the slice T are padded (chain_pitch)
constexpr int64_t cr_lds_bytes(int64_t D, int64_t es) { return (2 * D * chain_pitch(D) + CR_WAVES) * es; }
constexpr int64_t cr_bond_limit() {
  // the largest power-of-two bond D whose complex environment and T slice (both D rows, padded) and the reduction
  // words fit, and whose environment has one entry per accumulator of the workgroup
  int64_t D = 1;
  while (cr_lds_bytes(2 * D, 16) <= CHAIN_LDS_MAX && 4 * D * D <= int64_t(CHAIN_THREADS) * CR_OUT_PER_THREAD) D *= 2;
  return D;
}
constexpr int64_t CR_BOND_FIT = cr_bond_limit();
static_assert(CR_BOND_FIT == 64, "2 x 64 x 65 complex128 + 16 = 130 KB of 160 KB; 128 would need 516 KB");
// Largest bond up to which the two launches are faster than the enqueued products: measured with tools/corr_bench.py,
// profiles/corr_matrix.md (ahead at 16, behind at 32 and, one workgroup per row being one compute unit per row, far
// behind at 64).  Chains between this and CR_BOND_FIT take the kernels only under MPSE_CORR_CHAIN=1.
constexpr int64_t CR_BOND_MAX = 16;
static_assert(CR_BOND_MAX <= CR_BOND_FIT, "the measured limit lies inside what fits");
// d danc <= CHAIN_EXT_MAX keeps the site offsets inside 32 bits: 64 * 65536 * 64 = 2^28 elements
constexpr int64_t CR_NSEL_MAX = 256;      // grid cap of k_corr_rows: one workgroup per compute unit of the chip

struct CrSite {   // one row of the descriptor table (40 bytes, uploaded once per call)
  const void* a;
  int Dl, d, danc, Dr;
  int cplx;       // the tensor is complex128
  int sel;        // position in the selection, -1: not selected
  int moff;       // complex elements before X of this site in the matrix buffer; Y at + d d, Z at + 2 d d
  int goff;       // working elements before G of this site in the pooled buffer; Gd at + Dl Dl
};
static_assert(sizeof(CrSite) == 40, "descriptor rows are copied as 8-byte words");

struct CrPlan {
  bool chain;            // the chain kernels take it
  bool fit;              // they could: LDS, grid cap and offsets allow the launches, whatever the measured bond limit says
  int64_t max_bond;
  int64_t e_elems;       // LDS elements of the environment (padded rows), largest over the bonds
  int64_t t_elems;       // LDS elements of one (sigma, ancilla) slice of T (padded rows), largest over the sites
  int64_t lds;           // bytes of either launch, working dtype
};

bool corr_table_ok(int nsite, const int64_t* dims) { return chain_table_ok(nsite, dims, 4, {0}, {3}); }

// the sizing of a table that is a chain
CrPlan corr_plan(int nsite, const int64_t* dims, int nsel, bool cplx) {
  CrPlan pl{false, false, 0, 0, 0, 0};
  bool fits = true;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + 4 * i;
    for (int j : {0, 3}) pl.max_bond = d[j] > pl.max_bond ? d[j] : pl.max_bond;
    if (pl.max_bond > CR_BOND_FIT || d[1] > CHAIN_EXT_MAX || d[2] > CHAIN_EXT_MAX ||
        d[1] * d[2] > CHAIN_EXT_MAX) {
      fits = false;
      continue;
    }
    const int64_t e_l = d[0] * chain_pitch(d[0]), e_r = d[3] * chain_pitch(d[3]), t = d[0] * chain_pitch(d[3]);
    pl.e_elems = e_l > pl.e_elems ? e_l : pl.e_elems;
    pl.e_elems = e_r > pl.e_elems ? e_r : pl.e_elems;
    pl.t_elems = t > pl.t_elems ? t : pl.t_elems;
  }
  if (!fits || nsel < 1 || nsel > CR_NSEL_MAX) {
    pl.e_elems = pl.t_elems = 0;
    return pl;
  }
  pl.lds = (pl.e_elems + pl.t_elems + CR_WAVES) * (cplx ? 16 : 8);
  pl.fit = pl.lds <= CHAIN_LDS_MAX;
  if (!pl.fit) pl.lds = pl.e_elems = pl.t_elems = 0;
  pl.chain = pl.fit && pl.max_bond <= CR_BOND_MAX;
  return pl;
}

// R_N = 1.  Per site from the right, per (sigma, a) in ascending order:
//   T[c, b'] = sum_c' A[c, sigma, a, c'] R[b', c']                                          (into LDS)
//   R'[b, c] += sum_b' conj(A[b, sigma, a, b']) T[c, b']                                    (registers of the owner)
// and at a selected site, for every sigma' whose Y[sigma', sigma] or Z[sigma', sigma] is not zero,
//   S = sum_b' conj(A[b, sigma', a, b']) T[c, b'],  G[b, c] += Y[sigma', sigma] S,  Gd[b, c] += Z[sigma', sigma] S.
// R' replaces R in LDS after the last (sigma, a); G and Gd go to gbuf.  A thread owns the entries (b, c) = tid + j *
// CHAIN_THREADS, c fastest: A[b, ..] is one address per b group, the reads of T run down a column of padded rows.  The
// walk ends at the first selected site.
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_corr_right(const CrSite* __restrict__ sites, int nsite, int first,
                                                              int e_elems, const double* __restrict__ mats,
                                                              void* gbuf) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double cr_lds[];
  T* R = reinterpret_cast<T*>(cr_lds);
  T* Ts = R + e_elems;
  T* G = static_cast<T*>(gbuf);
  const int tid = threadIdx.x;
  if (tid == 0) R[0] = El::one();
  __syncthreads();
  for (int i = nsite - 1; i >= first; --i) {
    const CrSite s = sites[i];
    const int Dl = s.Dl, d = s.d, danc = s.danc, Dr = s.Dr;
    const int p = d * danc, row = p * Dr;   // element stride of the left bond
    const int pr = Dr | 1, pn = Dl | 1;
    const int nT = Dl * Dr, nE = Dl * Dl;
    const bool selected = s.sel >= 0;
    const double* Ym = mats + 2 * (s.moff + d * d);
    const double* Zm = mats + 2 * (s.moff + 2 * d * d);
    T acc_r[CR_OUT_PER_THREAD], acc_g[CR_OUT_PER_THREAD], acc_d[CR_OUT_PER_THREAD];
#pragma unroll
    for (int j = 0; j < CR_OUT_PER_THREAD; ++j) acc_r[j] = acc_g[j] = acc_d[j] = El::zero();
    for (int sa = 0; sa < p; ++sa) {
      const int sg = sa / danc, a = sa - sg * danc;
      for (int o = tid; o < nT; o += CHAIN_THREADS) {
        const int c = o / Dr, bp = o - c * Dr;
        const T* r_row = R + bp * pr;
        const int a0 = c * row + sa * Dr;
        T sum = El::zero();
#pragma unroll 4
        for (int cp = 0; cp < Dr; ++cp) El::fma(sum, El::ld(s.a, s.cplx, a0 + cp), r_row[cp]);
        Ts[c * pr + bp] = sum;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < CR_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          const int b = o / Dl, c = o - b * Dl;
          const T* t_row = Ts + c * pr;
          const int b0 = b * row + sa * Dr;
          T S = El::zero();
#pragma unroll 4
          for (int bp = 0; bp < Dr; ++bp) El::fma(S, El::cj(El::ld(s.a, s.cplx, b0 + bp)), t_row[bp]);
          El::add(acc_r[j], S);
          if (selected) {
            for (int sp = 0; sp < d; ++sp) {
              const T y = El::ldm(Ym, sp * d + sg), z = El::ldm(Zm, sp * d + sg);
              if (!El::nz(y) && !El::nz(z)) continue;
              T S2 = S;
              if (sp != sg) {
                const int b1 = b * row + (sp * danc + a) * Dr;
                S2 = El::zero();
#pragma unroll 4
                for (int bp = 0; bp < Dr; ++bp) El::fma(S2, El::cj(El::ld(s.a, s.cplx, b1 + bp)), t_row[bp]);
              }
              El::fma(acc_g[j], y, S2);
              El::fma(acc_d[j], z, S2);
            }
          }
        }
      }
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of R is done as well
    }
#pragma unroll
    for (int j = 0; j < CR_OUT_PER_THREAD; ++j) {
      const int o = tid + j * CHAIN_THREADS;
      if (o < nE) {
        const int b = o / Dl, c = o - b * Dl;
        R[b * pn + c] = acc_r[j];
        if (selected) {
          G[s.goff + o] = acc_g[j];
          G[s.goff + nE + o] = acc_d[j];
        }
      }
    }
    __syncthreads();
  }
}

// sum of v over the workgroup in a fixed order: down the lanes of each wave, then a tree over the waves through LDS;
// the value is valid in thread 0
template <bool CPLX>
__device__ typename ChainEl<CPLX>::T cr_block_sum(typename ChainEl<CPLX>::T v, typename ChainEl<CPLX>::T* red,
                                                  int tid) {
  using El = ChainEl<CPLX>;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) El::add(v, El::shfl_down(v, off));
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  for (int st = CR_WAVES / 2; st > 0; st >>= 1) {
    if (tid < st) El::add(red[tid], red[tid + st]);
    __syncthreads();
  }
  const typename El::T r = red[0];
  __syncthreads();   // red is written again by the next sum
  return r;
}

// Workgroup k: E_0 = 1, then from site 0 to the last selected site.  At a selected site l >= k first the closing
//   C[k, l] = sum_{b, c} E[b, c] (l == k ? Gd_l : G_l)[b, c],
// then (not behind the last selected site) the transfer, per (sigma, a) in ascending order:
//   T[b, c'] = sum_c E[b, c] A[c, sigma, a, c']                                             (into LDS)
//   E'[b', c'] += O[sigma', sigma] sum_b conj(A[b, sigma', a, b']) T[b, c']                 (registers of the owner)
// with O = X_k at site sel[k] (its non-zero entries) and the identity elsewhere.  Threads take (b', c') with c'
// fastest, as in k_overlap_chain.
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_corr_rows(const CrSite* __restrict__ sites, int last, int nsel,
                                                             int e_elems, int t_elems, const double* __restrict__ mats,
                                                             const void* __restrict__ gbuf, double* __restrict__ out) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double cr_lds[];
  T* E = reinterpret_cast<T*>(cr_lds);
  T* Ts = E + e_elems;
  T* red = Ts + t_elems;
  const T* G = static_cast<const T*>(gbuf);
  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  if (tid == 0) E[0] = El::one();
  __syncthreads();
  for (int i = 0; i <= last; ++i) {
    const CrSite s = sites[i];
    const int Dl = s.Dl, d = s.d, danc = s.danc, Dr = s.Dr;
    const int p = d * danc, row = p * Dr;
    const int pe = Dl | 1, pe_new = Dr | 1;
    const int nT = Dl * Dr, nE = Dr * Dr;
    const int l = s.sel;
    if (l >= k) {
      const T* g = G + s.goff + (l == k ? Dl * Dl : 0);
      T part = El::zero();
      for (int o = tid; o < Dl * Dl; o += CHAIN_THREADS) {
        const int b = o / Dl, c = o - b * Dl;
        El::fma(part, E[b * pe + c], g[o]);
      }
      const T tot = cr_block_sum<CPLX>(part, red, tid);
      if (tid == 0) {
        out[2 * (k * nsel + l)] = El::re(tot);
        out[2 * (k * nsel + l) + 1] = El::im(tot);
      }
      if (i == last) break;
    }
    const bool open = l == k;
    const double* Xm = mats + 2 * s.moff;
    T acc[CR_OUT_PER_THREAD];
#pragma unroll
    for (int j = 0; j < CR_OUT_PER_THREAD; ++j) acc[j] = El::zero();
    for (int sa = 0; sa < p; ++sa) {
      const int sg = sa / danc, a = sa - sg * danc;
      for (int o = tid; o < nT; o += CHAIN_THREADS) {
        const int b = o / Dr, cc = o - b * Dr;
        const T* e_row = E + b * pe;
        const int a0 = sa * Dr + cc;
        T sum = El::zero();
#pragma unroll 4
        for (int c = 0; c < Dl; ++c) El::fma(sum, e_row[c], El::ld(s.a, s.cplx, c * row + a0));
        Ts[o] = sum;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < CR_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          const int bb = o / Dr, cc = o - bb * Dr;
          for (int sp = open ? 0 : sg; sp < (open ? d : sg + 1); ++sp) {
            T x = El::one();
            if (open) {
              x = El::ldm(Xm, sp * d + sg);
              if (!El::nz(x)) continue;
            }
            const int b0 = (sp * danc + a) * Dr + bb;
            T S = El::zero();
#pragma unroll 4
            for (int b = 0; b < Dl; ++b) El::fma(S, El::cj(El::ld(s.a, s.cplx, b * row + b0)), Ts[b * Dr + cc]);
            if (open)
              El::fma(acc[j], x, S);
            else
              El::add(acc[j], S);
          }
        }
      }
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of E is done as well
    }
#pragma unroll
    for (int j = 0; j < CR_OUT_PER_THREAD; ++j) {
      const int o = tid + j * CHAIN_THREADS;
      if (o < nE) {
        const int bb = o / Dr, cc = o - bb * Dr;
        E[bb * pe_new + cc] = acc[j];
      }
    }
    __syncthreads();
  }
}

struct CrArgs {
  int nsite;
  const void* const* sites;
  const int* dtype;
  const int64_t* dims;
  int nsel;
  const int* sel;
  const double* X;   // per selected site d x d complex pairs, one after the other
  const double* Y;
  const double* Z;
};

// the three local matrices of every selected site as one host array: X_0 Y_0 Z_0 X_1 ..; moff[k] = complex elements
// before X_k.  Complex pairs, or the real parts alone (real_only: the enqueued path of an all-real call).
std::vector<double> corr_mats(const CrArgs& a, bool real_only, std::vector<int64_t>* moff) {
  std::vector<double> m;
  moff->assign((size_t)a.nsel, 0);
  int64_t src = 0;
  for (int k = 0; k < a.nsel; ++k) {
    const int64_t dd = a.dims[4 * a.sel[k] + 1] * a.dims[4 * a.sel[k] + 1];
    (*moff)[k] = (int64_t)(m.size() / (real_only ? 1 : 2));
    for (const double* M : {a.X, a.Y, a.Z})
      for (int64_t e = 0; e < dd; ++e) {
        m.push_back(M[2 * (src + e)]);
        if (!real_only) m.push_back(M[2 * (src + e) + 1]);
      }
    src += dd;
  }
  return m;
}

int corr_chain(mpse_ctx* ctx, const CrArgs& a, bool cplx, const CrPlan& pl, double* out_host) {
  std::vector<int64_t> moff;
  const std::vector<double> mats = corr_mats(a, false, &moff);
  std::vector<CrSite> rows((size_t)a.nsite);
  int64_t g_elems = 0;
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const bool is_sel = k < a.nsel && a.sel[k] == i;
    rows[i] = CrSite{a.sites[i], (int)d[0], (int)d[1], (int)d[2], (int)d[3], a.dtype[i] == MPSE_C128,
                     is_sel ? k : -1, is_sel ? (int)moff[k] : 0, is_sel ? (int)g_elems : 0};
    if (is_sel) {
      g_elems += 2 * d[0] * d[0];
      ++k;
    }
  }
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_corr_right), CHAIN_KERNELS(k_corr_rows)}, CHAIN_LDS_MAX));
  const size_t es = cplx ? 16 : 8, n_out = (size_t)a.nsel * a.nsel * 2;
  TmpBuf tab(ctx), mbuf(ctx), gbuf(ctx), res(ctx);
  MPSE_TRY(chain_stage_rows(ctx, tab, rows));
  MPSE_TRY(mbuf.alloc(mats.size() * sizeof(double)));
  MPSE_TRY(gbuf.alloc((size_t)g_elems * es));
  MPSE_TRY(res.alloc(n_out * sizeof(double)));
  MPSE_TRY(stage_h2d(ctx, mbuf.p, mats.data(), mats.size() * sizeof(double)));
  MPSE_TRY(device_zero(ctx, res.p, n_out * sizeof(double)));
  const int first = a.sel[0], last = a.sel[a.nsel - 1];
  CHAIN_LAUNCH(ctx, cplx, k_corr_right, 1, pl.lds, tab.as<const CrSite>(), a.nsite, first, (int)pl.e_elems,
               mbuf.as<const double>(), gbuf.p);
  CHAIN_LAUNCH(ctx, cplx, k_corr_rows, a.nsel, pl.lds, tab.as<const CrSite>(), last, a.nsel, (int)pl.e_elems,
               (int)pl.t_elems, mbuf.as<const double>(), (const void*)gbuf.p, res.as<double>());
  MPSE_HIP(ctx, hipGetLastError());
  return mpse_memcpy_d2h(ctx, out_host, res.p, n_out * sizeof(double));
}

// Both passes as products of the contraction kernel, in one dtype: complex as soon as any site or local matrix is (real
// sites are widened into pooled copies first, widen_site).
//   right pass, site i from the last one down to sel[0], R (D_r, D_r) = [b', c']:
//     Y1[(c, s, a), b'] = sum_c' A[(c, s, a), c'] R[b', c']
//     R'[b, c] = sum_(s, a, b') conj(A[b, (s, a, b')]) Y1[c, (s, a, b')]
//     selected:  Y2[c, s', a, b'] = sum_s M[s', s] Y1[c, s, a, b'] (batched over c),  G resp. Gd = conj(A) . Y2 like R'
//   left pass, site i from 0 to sel[nsel - 1], stack S[k][b][c]: row 0 is the identity transfer E, row 1 + k the row
//   opened at sel[k]:
//     selected site l:  C[k, l] = S[1 + k] . vec(G_l) for the open rows (one product), C[l, l] = S[0] . vec(Gd_l)
//     X1[(k, b), (s, a, c')] = sum_c S[(k, b), c] A[c, (s, a, c')]         (one product for the whole stack)
//     selected:  X1[1 + l][b, s', a, c'] = sum_s X_l[s', s] X1[0][b, s, a, c'] (batched over b): the stack grows
//     S'[k][b', c'] = sum_(b, s, a) conj(A[(b, s, a), b']) X1[k][(b, s, a), c']          (batched over k)
int corr_enqueued(mpse_ctx* ctx, const CrArgs& a, bool cplx, double* out_host) {
  const int dt = cplx ? MPSE_C128 : MPSE_F64;
  const int cj = cplx ? 1 : 0;
  const size_t es = cplx ? 16 : 8;
  const int nsel = a.nsel, first = a.sel[0], last = a.sel[nsel - 1];
  std::vector<int64_t> moff;
  const std::vector<double> mats = corr_mats(a, !cplx, &moff);
  int64_t e_max = 1, x_max = 1, g_elems = 0;
  std::vector<int64_t> goff((size_t)nsel);
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const int64_t* d = a.dims + 4 * i;
    e_max = d[3] * d[3] > e_max ? d[3] * d[3] : e_max;
    const int64_t x = d[0] * d[1] * d[2] * d[3];
    x_max = x > x_max ? x : x_max;
    if (k < nsel && a.sel[k] == i) {
      goff[k++] = g_elems;
      g_elems += 2 * d[0] * d[0];
    }
  }
  // widened copies of the real sites of a complex call live to the end of the call
  std::vector<std::unique_ptr<TmpBuf>> wide;
  std::vector<const void*> site;
  MPSE_TRY(chain_widen_sites(ctx, a.nsite, a.sites, a.dtype, a.dims, cplx, &wide, &site));
  TmpBuf mbuf(ctx), gbuf(ctx), res(ctx), r0(ctx), r1(ctx), y1(ctx), y2(ctx);
  MPSE_TRY(mbuf.alloc(mats.size() * sizeof(double)));
  MPSE_TRY(gbuf.alloc((size_t)g_elems * es));
  MPSE_TRY(res.alloc((size_t)nsel * nsel * es));
  MPSE_TRY(r0.alloc((size_t)e_max * es));
  MPSE_TRY(r1.alloc((size_t)e_max * es));
  MPSE_TRY(y1.alloc((size_t)x_max * es));
  MPSE_TRY(y2.alloc((size_t)x_max * es));
  MPSE_TRY(stage_h2d(ctx, mbuf.p, mats.data(), mats.size() * sizeof(double)));
  MPSE_TRY(device_zero(ctx, res.p, (size_t)nsel * nsel * es));
  const double one[2] = {1.0, 0.0};
  MPSE_TRY(stage_h2d(ctx, r0.p, one, es));
  char* G = static_cast<char*>(gbuf.p);
  const char* M = static_cast<const char*>(mbuf.p);
  // ---- right pass
  {
    void* R = r0.p;
    void* Rn = r1.p;
    int k = nsel - 1;
    for (int i = a.nsite - 1; i >= first; --i) {
      const int64_t* d = a.dims + 4 * i;
      const int64_t Dl = d[0], dd = d[1], da = d[2], Dr = d[3], p = dd * da;
      MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(Dl * p, Dr), idx1(Dr, 1), idx1(Dr, 1), idx1(Dr, Dr), idx1(Dl * p, Dr),
                         idx1(Dr, 1), 1, 0, 0, 0, site[i], R, y1.p));
      if (k >= 0 && a.sel[k] == i) {
        // which = 1: Y -> G (not needed for the first selected site), 2: Z -> Gd
        for (int which = (k == 0 ? 2 : 1); which <= 2; ++which) {
          const char* Mk = M + (size_t)(moff[k] + which * dd * dd) * es;
          MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(dd, dd), idx1(dd, 1), idx1(dd, da * Dr), idx1(da * Dr, 1),
                             idx1(dd, da * Dr), idx1(da * Dr, 1), Dl, 0, p * Dr, p * Dr, Mk, y1.p, y2.p));
          MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(Dl, p * Dr), idx1(p * Dr, 1), idx1(p * Dr, 1), idx1(Dl, p * Dr),
                             idx1(Dl, Dl), idx1(Dl, 1), 1, 0, 0, 0, site[i], y2.p,
                             G + (size_t)(goff[k] + (which == 2 ? Dl * Dl : 0)) * es));
        }
        --k;
      }
      if (i == first) break;
      MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(Dl, p * Dr), idx1(p * Dr, 1), idx1(p * Dr, 1), idx1(Dl, p * Dr),
                         idx1(Dl, Dl), idx1(Dl, 1), 1, 0, 0, 0, site[i], y1.p, Rn));
      void* t = R;
      R = Rn, Rn = t;
    }
  }
  // ---- left pass
  {
    TmpBuf s0(ctx), s1(ctx), x1(ctx);
    MPSE_TRY(s0.alloc((size_t)(nsel + 1) * e_max * es));
    MPSE_TRY(s1.alloc((size_t)(nsel + 1) * e_max * es));
    MPSE_TRY(x1.alloc((size_t)(nsel + 1) * x_max * es));
    MPSE_TRY(stage_h2d(ctx, s0.p, one, es));
    char* S = static_cast<char*>(s0.p);
    char* Sn = static_cast<char*>(s1.p);
    char* X1 = static_cast<char*>(x1.p);
    char* C = static_cast<char*>(res.p);
    int64_t n_open = 0;
    for (int i = 0; i <= last; ++i) {
      const int64_t* d = a.dims + 4 * i;
      const int64_t Dl = d[0], dd = d[1], da = d[2], Dr = d[3], p = dd * da;
      const bool is_sel = a.sel[n_open] == i;
      if (is_sel) {
        const int64_t l = n_open;
        if (n_open > 0)
          MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(n_open, Dl * Dl), idx1(Dl * Dl, 1), idx1(Dl * Dl, 1), idx1(1, 1),
                             idx1(n_open, nsel), idx1(1, 1), 1, 0, 0, 0, S + (size_t)(Dl * Dl) * es,
                             G + (size_t)goff[l] * es, C + (size_t)l * es));
        MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(1, Dl * Dl), idx1(Dl * Dl, 1), idx1(Dl * Dl, 1), idx1(1, 1),
                           idx1(1, nsel), idx1(1, 1), 1, 0, 0, 0, S, G + (size_t)(goff[l] + Dl * Dl) * es,
                           C + (size_t)(l * nsel + l) * es));
        if (i == last) break;
      }
      const int64_t nrow = n_open + 1;
      MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(nrow * Dl, Dl), idx1(Dl, 1), idx1(Dl, p * Dr), idx1(p * Dr, 1),
                         idx1(nrow * Dl, p * Dr), idx1(p * Dr, 1), 1, 0, 0, 0, S, site[i], X1));
      if (is_sel) {
        const char* Xk = M + (size_t)moff[n_open] * es;
        MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(dd, dd), idx1(dd, 1), idx1(dd, da * Dr), idx1(da * Dr, 1),
                           idx1(dd, da * Dr), idx1(da * Dr, 1), Dl, 0, p * Dr, p * Dr, Xk, X1,
                           X1 + (size_t)(nrow * Dl * p * Dr) * es));
        ++n_open;
      }
      MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(Dr, 1), idx1(Dl * p, Dr), idx1(Dl * p, Dr), idx1(Dr, 1), idx1(Dr, Dr),
                         idx1(Dr, 1), n_open + 1, 0, Dl * p * Dr, Dr * Dr, site[i], X1, Sn));
      char* t = S;
      S = Sn, Sn = t;
    }
  }
  std::vector<double> host((size_t)nsel * nsel * (cplx ? 2 : 1));
  MPSE_TRY(mpse_memcpy_d2h(ctx, host.data(), res.p, host.size() * sizeof(double)));
  for (size_t e = 0; e < (size_t)nsel * nsel; ++e) {
    out_host[2 * e] = cplx ? host[2 * e] : host[e];
    out_host[2 * e + 1] = cplx ? host[2 * e + 1] : 0.0;
  }
  return MPSE_OK;
}

}  // namespace

extern "C" {

int mpse_mps_corr_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n) {
  const bool valid = corr_table_ok(nsite, dims);
  const CrPlan pl = valid ? corr_plan(nsite, dims, nsel, any_complex != 0) : CrPlan{false, false, 0, 0, 0, 0};
  const int64_t v[12] = {CR_BOND_MAX, CHAIN_LDS_MAX, pl.chain ? pl.lds : 0, pl.fit ? pl.e_elems : 0,
                         pl.fit ? pl.t_elems : 0, CHAIN_THREADS, pl.max_bond, valid ? 1 : 0,
                         CR_NSEL_MAX, CHAIN_EXT_MAX, CR_BOND_FIT, pl.fit ? pl.lds : 0};
  plan_info_out(info, n, v, 12);
  return pl.chain ? 1 : 0;
}

int mpse_mps_corr_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::corr_stats, counts, n);
}

int mpse_mps_corr(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims, int nsel,
                  const int* sel, const double* X, const double* Y, const double* Z, double* out_host) {
  if (!ctx) return MPSE_ERR_ARG;
  if (nsite < 1 || !sites || !dtype || !dims || nsel < 1 || !sel || !X || !Y || !Z || !out_host)
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_corr: null argument, no sites or no selection");
  bool cplx = false;
  MPSE_TRY(chain_scan_sites(ctx, "mps_corr", nsite, {sites}, {dtype}, &cplx));
  for (int k = 0; k < nsel; ++k)
    if (sel[k] < 0 || sel[k] >= nsite || (k > 0 && sel[k] <= sel[k - 1]))
      return mpse_fail(ctx, MPSE_ERR_SHAPE, "mps_corr: the selection is not strictly ascending inside [0, %d)", nsite);
  if (!corr_table_ok(nsite, dims))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "mps_corr: dims is not a chain (extents >= 1, matching neighbours, first and last bond 1)");
  if (MPSE_RECORDING(ctx))
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_corr: synchronous, not available while a deferred list is recorded");
  int64_t n_mat = 0;
  for (int k = 0; k < nsel; ++k) n_mat += dims[4 * sel[k] + 1] * dims[4 * sel[k] + 1];
  for (int64_t e = 0; e < n_mat && !cplx; ++e) cplx = X[2 * e + 1] != 0.0 || Y[2 * e + 1] != 0.0 || Z[2 * e + 1] != 0.0;
  CrPlan pl = corr_plan(nsite, dims, nsel, cplx);
  MPSE_BIND(ctx);
  // MPSE_CORR_CHAIN=0 sends every chain through the enqueued products; =1 sends every chain whose launches fit through
  // the kernels, above the measured bond limit as well (measurements of that limit: tools/corr_bench.py)
  const char env = chain_env_switch("MPSE_CORR_CHAIN");
  if (env == '0') pl.chain = false;
  if (env == '1') pl.chain = pl.fit;
  const CrArgs args{nsite, sites, dtype, dims, nsel, sel, X, Y, Z};
  std::vector<double> res((size_t)nsel * nsel * 2, 0.0);
  if (pl.chain)
    MPSE_TRY(corr_chain(ctx, args, cplx, pl, res.data()));
  else
    MPSE_TRY(corr_enqueued(ctx, args, cplx, res.data()));
  ctx->corr_stats[pl.chain ? mpse_ctx::CR_CHAIN : mpse_ctx::CR_ENQUEUED] += 1;
  ctx->corr_stats[mpse_ctx::CR_SITES] += nsite;
  ctx->corr_stats[mpse_ctx::CR_ENTRIES] += (long long)nsel * (nsel + 1) / 2;
  memcpy(out_host, res.data(), res.size() * sizeof(double));
  return MPSE_OK;
}

}  // extern "C"
