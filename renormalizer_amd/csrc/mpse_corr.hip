// mpse_mps_corr: the matrix C[k, l] = <psi| X_k Y_l |psi> (k < l), C[k, k] = <psi| Z_k |psi> of one-site operators on
// selected sites of ONE chain as one engine call (the reference takes every entry as its own MPO expectation,
// mps/mps.py:1657-1687 calc_edof_rdm).  Two paths, chosen from the dims table alone (corr_plan):
//   chain      two launches, for chains whose bonds are at most CR_BOND_MAX.  k_corr_right: one workgroup walks right to
//              left with the identity environment R in LDS and leaves, at every selected site l, the closed
//              environments G_l (with Y_l) and Gd_l (with Z_l) in pooled memory.  k_corr_rows: workgroup k walks left
//              to right with the transfer matrix E in LDS, opens with X_k at site sel[k] and closes against G_l at
//              every later selected site.
//   enqueued   the same two passes as products of the contraction kernel; the open rows are one stack of environments
//              that grows by a row per selected site - every other chain
// The walk, the sizing, the entry checks and the plain products of the enqueued passes are those of mpse_chain_walk.h,
// which also says what holds for all three calls: launch order instead of flags, one host read, a fixed summation order.
#include "mpse_chain_walk.h"

namespace {

// the regions of mpse_chain_walk.h plus one word per wave for cr_block_sum (mpse_chain_walk.h)
static_assert(chain_walk_lds(CHAIN_BOND_FIT, 16, CHAIN_WAVES) <= CHAIN_LDS_MAX,
              "2 x 64 x 65 complex128 + 16 = 130 KB of 160 KB");
// Largest bond up to which the two launches are faster than the enqueued products: measured with tools/corr_bench.py,
// profiles/corr_matrix.md (ahead at 16, behind at 32 and, one workgroup per row being one compute unit per row, far
// behind at 64).  Chains between this and CHAIN_BOND_FIT take the kernels only under MPSE_CORR_CHAIN=1.
constexpr int64_t CR_BOND_MAX = 16;
static_assert(CR_BOND_MAX <= CHAIN_BOND_FIT, "the measured limit lies inside what fits");
constexpr int64_t CR_NSEL_MAX = 256;      // grid cap of k_corr_rows: one workgroup per compute unit of the chip

struct CrSite : ChainSelRow {   // one row of the descriptor table (40 bytes, uploaded once per call)
  int moff;       // complex elements before X of this site in the matrix buffer; Y at + d d, Z at + 2 d d
  int goff;       // working elements before G of this site in the pooled buffer; Gd at + Dl Dl
};
static_assert(sizeof(CrSite) == 40, "descriptor rows are copied as 8-byte words");

// the sizing of a table that is a chain: the grid cap on the selection, the reduction words in LDS
ChainSelPlan corr_plan(int nsite, const int64_t* dims, int nsel, bool cplx) {
  return chain_sel_plan(nsite, dims, nsel >= 1 && nsel <= CR_NSEL_MAX, CHAIN_WAVES, cplx, CR_BOND_MAX);
}

// R_N = 1.  Per site from the right, per (sigma, a) in ascending order the transfer to the right (walk_right_slice: T =
// A[sigma, a] . R into LDS; walk_right_sum: R' += S in the registers of the owner), and at a selected site, for every
// sigma' whose Y[sigma', sigma] or Z[sigma', sigma] is not zero,
//   S = sum_b' conj(A[b, sigma', a, b']) T[c, b'],  G[b, c] += Y[sigma', sigma] S,  Gd[b, c] += Z[sigma', sigma] S.
// R' replaces R in LDS after the last (sigma, a); G and Gd go to gbuf.  The walk ends at the first selected site.
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
  walk_env_one<CPLX>(R);
  for (int i = nsite - 1; i >= first; --i) {
    const CrSite s = sites[i];
    const int d = s.d, danc = s.danc, Dr = s.Dr;
    const int p = d * danc, row = p * Dr, nE = s.Dl * s.Dl;
    const bool selected = s.sel >= 0;
    const double* Ym = mats + 2 * (s.moff + d * d);
    const double* Zm = mats + 2 * (s.moff + 2 * d * d);
    T acc_r[CHAIN_OUT_PER_THREAD], acc_g[CHAIN_OUT_PER_THREAD], acc_d[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc_r);
    walk_acc_zero<CPLX>(acc_g);
    walk_acc_zero<CPLX>(acc_d);
    for (int sa = 0; sa < p; ++sa) {
      const int sg = sa / danc, a = sa - sg * danc;
      walk_right_slice<CPLX>(s, row, sa * Dr, R, Ts);
#pragma unroll
      for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          T S;
          walk_right_sum<CPLX>(s, row, sa * Dr, o, Ts, S);
          El::add(acc_r[j], S);
          if (selected) {
            for (int sp = 0; sp < d; ++sp) {
              const T y = El::ldm(Ym, sp * d + sg), z = El::ldm(Zm, sp * d + sg);
              if (!El::nz(y) && !El::nz(z)) continue;
              T S2 = S;
              if (sp != sg) walk_right_sum<CPLX>(s, row, (sp * danc + a) * Dr, o, Ts, S2);
              El::fma(acc_g[j], y, S2);
              El::fma(acc_d[j], z, S2);
            }
          }
        }
      }
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of R is done as well
    }
    if (selected) {
#pragma unroll
      for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          G[s.goff + o] = acc_g[j];
          G[s.goff + nE + o] = acc_d[j];
        }
      }
    }
    walk_acc_store<CPLX>(acc_r, s.Dl, s.Dl, R);
  }
}

// Workgroup k: E_0 = 1, then from site 0 to the last selected site.  At a selected site l >= k first the closing
//   C[k, l] = sum_{b, c} E[b, c] (l == k ? Gd_l : G_l)[b, c],
// then (not behind the last selected site) the transfer to the left, per (sigma, a) in ascending order: T = E .
// A[sigma, a] into LDS (walk_left_slice), E'[b', c'] += O[sigma', sigma] S, S of the bra slice sigma' (walk_left_sum),
// with O = X_k at site sel[k] (its non-zero entries) and the identity elsewhere.
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
  walk_env_one<CPLX>(E);
  for (int i = 0; i <= last; ++i) {
    const CrSite s = sites[i];
    const int Dl = s.Dl, d = s.d, danc = s.danc, Dr = s.Dr;
    const int p = d * danc, row = p * Dr, nE = Dr * Dr;
    const int l = s.sel;
    if (l >= k) {
      const T part = walk_env_dot<CPLX>(E, Dl, G + s.goff + (l == k ? Dl * Dl : 0), tid, CHAIN_THREADS);
      const T tot = cr_block_sum<CPLX>(part, red, tid);
      if (tid == 0) {
        out[2 * (k * nsel + l)] = El::re(tot);
        out[2 * (k * nsel + l) + 1] = El::im(tot);
      }
      if (i == last) break;
    }
    const bool open = l == k;
    const double* Xm = mats + 2 * s.moff;
    T acc[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc);
    for (int sa = 0; sa < p; ++sa) {
      const int sg = sa / danc, a = sa - sg * danc;
      walk_left_slice<CPLX>(s, row, sa * Dr, E, Dl | 1, Ts, Dr);
#pragma unroll
      for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          for (int sp = open ? 0 : sg; sp < (open ? d : sg + 1); ++sp) {
            T x = El::one();
            if (open) {
              x = El::ldm(Xm, sp * d + sg);
              if (!El::nz(x)) continue;
            }
            T S;
            walk_left_sum<CPLX>(s, row, (sp * danc + a) * Dr, o, Ts, S);
            if (open)
              El::fma(acc[j], x, S);
            else
              El::add(acc[j], S);
          }
        }
      }
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of E is done as well
    }
    walk_acc_store<CPLX>(acc, Dr, Dr, E);
  }
}

struct CrArgs : ChainSelArgs {
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

int corr_chain(mpse_ctx* ctx, const CrArgs& a, bool cplx, const ChainSelPlan& pl, double* out_host) {
  std::vector<int64_t> moff;
  const std::vector<double> mats = corr_mats(a, false, &moff);
  std::vector<CrSite> rows((size_t)a.nsite);
  int64_t g_elems = 0;
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const bool is_sel = k < a.nsel && a.sel[k] == i;
    rows[i] = CrSite{chain_sel_row(a, i, is_sel ? k : -1), is_sel ? (int)moff[k] : 0, is_sel ? (int)g_elems : 0};
    if (is_sel) g_elems += 2 * a.dims[4 * i] * a.dims[4 * i], ++k;
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
// sites are widened into pooled copies first, widen_site).  The plain products: ChainSelEnq of mpse_chain_walk.h.
//   right pass, site i from the last one down to sel[0], R (D_r, D_r) = [b', c']:  Y1 = A . R (a_r),  R' = conj(A) . Y1
//   (ca_y)
//     selected:  Y2[c, s', a, b'] = sum_s M[s', s] Y1[c, s, a, b'] (batched over c),  G resp. Gd = conj(A) . Y2 like R'
//   left pass, site i from 0 to sel[nsel - 1], stack S[k][b][c]: row 0 is the identity transfer E, row 1 + k the row
//   opened at sel[k]:
//     selected site l:  C[k, l] = S[1 + k] . vec(G_l) for the open rows (one product), C[l, l] = S[0] . vec(Gd_l)
//     X1 = S . A, one product for the whole stack (l_a);  S' = conj(A) . X1, batched over k (ca_x)
//     selected:  X1[1 + l][b, s', a, c'] = sum_s X_l[s', s] X1[0][b, s, a, c'] (batched over b): the stack grows
int corr_enqueued(mpse_ctx* ctx, const CrArgs& a, bool cplx, double* out_host) {
  ChainSelEnq q(ctx, cplx);
  MPSE_TRY(q.init(a));
  const size_t es = q.es;
  const int nsel = a.nsel, first = a.sel[0], last = a.sel[nsel - 1];
  std::vector<int64_t> moff;
  const std::vector<double> mats = corr_mats(a, !cplx, &moff);
  int64_t g_elems = 0;
  std::vector<int64_t> goff((size_t)nsel);
  for (int k = 0; k < nsel; ++k) goff[k] = g_elems, g_elems += 2 * a.dims[4 * a.sel[k]] * a.dims[4 * a.sel[k]];
  TmpBuf mbuf(ctx), gbuf(ctx), res(ctx), r0(ctx), r1(ctx), y1(ctx), y2(ctx);
  MPSE_TRY(mbuf.alloc(mats.size() * sizeof(double)));
  MPSE_TRY(q.alloc({{&gbuf, g_elems}, {&res, (int64_t)nsel * nsel}, {&r0, q.e_max}, {&r1, q.e_max}, {&y1, q.x_max},
                    {&y2, q.x_max}}));
  MPSE_TRY(stage_h2d(ctx, mbuf.p, mats.data(), mats.size() * sizeof(double)));
  MPSE_TRY(device_zero(ctx, res.p, (size_t)nsel * nsel * es));
  const double one[2] = {1.0, 0.0};
  MPSE_TRY(stage_h2d(ctx, r0.p, one, es));
  char* G = static_cast<char*>(gbuf.p);
  const char* M = static_cast<const char*>(mbuf.p);
  // the mix of the physical leg of Y with the local matrix Mk, batched over the rows of the left bond
  auto mix = [&](const int64_t* d, const char* Mk, const void* Y, void* Y2) {
    const int64_t dd = d[1], k = d[2] * d[3];
    return q.gemm(0, idx1(dd, dd), idx1(dd, 1), idx1(dd, k), idx1(k, 1), idx1(dd, k), idx1(k, 1), d[0], 0, dd * k,
                  dd * k, Mk, Y, Y2);
  };
  // ---- right pass
  {
    void* R = r0.p;
    void* Rn = r1.p;
    int k = nsel - 1;
    for (int i = a.nsite - 1; i >= first; --i) {
      const int64_t* d = a.dims + 4 * i;
      const int64_t Dl = d[0], dd = d[1], Dr = d[3], p = dd * d[2];
      MPSE_TRY(q.a_r(Dl * p, Dr, Dr, q.site[i], R, y1.p));
      if (k >= 0 && a.sel[k] == i) {
        // which = 1: Y -> G (not needed for the first selected site), 2: Z -> Gd
        for (int which = (k == 0 ? 2 : 1); which <= 2; ++which) {
          MPSE_TRY(mix(d, M + (size_t)(moff[k] + which * dd * dd) * es, y1.p, y2.p));
          MPSE_TRY(q.ca_y(Dl, Dl, p * Dr, q.site[i], y2.p, G + (size_t)(goff[k] + (which == 2 ? Dl * Dl : 0)) * es));
        }
        --k;
      }
      if (i == first) break;
      MPSE_TRY(q.ca_y(Dl, Dl, p * Dr, q.site[i], y1.p, Rn));
      std::swap(R, Rn);
    }
  }
  // ---- left pass
  {
    TmpBuf s0(ctx), s1(ctx), x1(ctx);
    MPSE_TRY(q.alloc({{&s0, (nsel + 1) * q.e_max}, {&s1, (nsel + 1) * q.e_max}, {&x1, (nsel + 1) * q.x_max}}));
    MPSE_TRY(stage_h2d(ctx, s0.p, one, es));
    char* S = static_cast<char*>(s0.p);
    char* Sn = static_cast<char*>(s1.p);
    char* X1 = static_cast<char*>(x1.p);
    char* C = static_cast<char*>(res.p);
    int64_t n_open = 0;
    for (int i = 0; i <= last; ++i) {
      const int64_t* d = a.dims + 4 * i;
      const int64_t Dl = d[0], Dr = d[3], p = d[1] * d[2];
      const bool is_sel = a.sel[n_open] == i;
      if (is_sel) {
        const int64_t l = n_open, nE = Dl * Dl;
        if (n_open > 0)
          MPSE_TRY(q.gemm(0, idx1(n_open, nE), idx1(nE, 1), idx1(nE, 1), idx1(1, 1), idx1(n_open, nsel), idx1(1, 1), 1,
                          0, 0, 0, S + (size_t)nE * es, G + (size_t)goff[l] * es, C + (size_t)l * es));
        MPSE_TRY(q.gemm(0, idx1(1, nE), idx1(nE, 1), idx1(nE, 1), idx1(1, 1), idx1(1, nsel), idx1(1, 1), 1, 0, 0, 0, S,
                        G + (size_t)(goff[l] + nE) * es, C + (size_t)(l * nsel + l) * es));
        if (i == last) break;
      }
      const int64_t nrow = n_open + 1;
      MPSE_TRY(q.l_a(nrow, Dl, Dl, p * Dr, S, q.site[i], X1));
      if (is_sel) {
        MPSE_TRY(mix(d, M + (size_t)moff[n_open] * es, X1, X1 + (size_t)(nrow * Dl * p * Dr) * es));
        ++n_open;
      }
      MPSE_TRY(q.ca_x(n_open + 1, Dl * p, Dr, Dr, q.site[i], X1, Sn));
      std::swap(S, Sn);
    }
  }
  return chain_read_pairs(ctx, res.p, (int64_t)nsel * nsel, cplx, {{0, (int64_t)nsel * nsel, 0}}, out_host);
}

}  // namespace

extern "C" {

int mpse_mps_corr_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n) {
  const bool valid = chain_sel_table_ok(nsite, dims);
  const ChainSelPlan pl = valid ? corr_plan(nsite, dims, nsel, any_complex != 0) : ChainSelPlan{};
  return chain_sel_plan_out(pl, valid, CR_BOND_MAX, CR_NSEL_MAX, {}, info, n);
}

int mpse_mps_corr_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::corr_stats, counts, n);
}

int mpse_mps_corr(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims, int nsel,
                  const int* sel, const double* X, const double* Y, const double* Z, double* out_host) {
  const CrArgs args{{nsite, sites, dtype, dims, nsel, sel}, X, Y, Z};
  bool cplx = false;
  MPSE_TRY(chain_sel_prologue(ctx, "mps_corr", args, 1, X && Y && Z && out_host, &cplx));
  int64_t n_mat = 0;
  for (int k = 0; k < nsel; ++k) n_mat += dims[4 * sel[k] + 1] * dims[4 * sel[k] + 1];
  for (int64_t e = 0; e < n_mat && !cplx; ++e) cplx = X[2 * e + 1] != 0.0 || Y[2 * e + 1] != 0.0 || Z[2 * e + 1] != 0.0;
  ChainSelPlan pl = corr_plan(nsite, dims, nsel, cplx);
  MPSE_BIND(ctx);
  chain_sel_plan_switch("MPSE_CORR_CHAIN", &pl);
  std::vector<double> res((size_t)nsel * nsel * 2, 0.0);
  if (pl.chain)
    MPSE_TRY(corr_chain(ctx, args, cplx, pl, res.data()));
  else
    MPSE_TRY(corr_enqueued(ctx, args, cplx, res.data()));
  return chain_sel_done(ctx->corr_stats, pl.chain, nsite, (long long)nsel * (nsel + 1) / 2, res, out_host);
}

}  // extern "C"
