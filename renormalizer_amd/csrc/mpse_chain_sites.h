// The call "environments of selected sites, then close each site", which mpse_rdm1.hip makes for ONE chain (rows that
// begin with ChainSelRow: the chain is its own conjugated bra) and mpse_trdm1.hip for a bra and a ket that differ (rows
// that begin with Chain2Row); no other file includes this.  Written once, for two chains, on the stages and the walks
// of mpse_chain_walk.h.  A file keeps its kernels (two lines each around the bodies here), the bond limits of its path
// rule and its exports.
//   M_i[p, p'] = sum_{b,k,g,b',k'} op(B_i)[b,p,g,b'] L_i[b,k] K_i[k,p',g,k'] R_i[b',k']
// L_i / R_i: the environments left / right of site i, bra index first: Db rows, Dk columns.
// LDS plan of either launch, working elements (8 or 16 bytes), rows padded to an odd pitch (chain_pitch):
//   region E   max over the bonds of Db * pitch(Dk) and over the sites of Db_l * Db_r
//              the walks: the environment;  chain_close_site: U (Db_l x Db_r, unpadded)
//   region T   max over the sites of Db_l * pitch(Dk_r) and Dk_l * pitch(Db_r)
//              the walks: the slice T from the left resp. from the right;  chain_close_site: V (Db_l rows)
// For ONE chain U fits in the environment's region by itself (D_l * D_r <= max(D_l, D_r) * pitch(max(D_l, D_r))); for
// rectangular environments it does not (Db = 64, Dk = 1: U has 4096 elements, an environment 64), so region E is sized
// for U as well; the closing takes the one order ket first, bra last, whatever the bonds.  L and R of the closing stay
// in the pooled buffer and are read through L2: with them in LDS a complex bond of 64 would need 4 x 64 x 65 x 16 = 260 KB.
#pragma once
#include "mpse_chain_walk.h"

template <class Base>
struct ChainSiteRow : Base {   // one row of the table: nsite rows, then the selected sites' rows again
  int64_t eoff;   // working elements before L of this site in the pooled buffer; R (transposed) at + Db_l Dk_l
  int64_t ooff;   // complex elements before M of this site in the result
};

// --------------------------------------------------------------------------------------------------------- device side
// Body of a *_sites kernel: workgroup j closes the environments of site sel[j] (row nsite + j of the table).  Per
// (sigma', a) in ascending order:
//   V[b, k'] = sum_k L[b, k] K[k, sigma', a, k']                            (into LDS, region T: walk_left_slice with the
//                                                                            packed L as E and padded rows of V)
//   U[b, b'] = sum_k' V[b, k'] R[b', k']                                                       (into LDS, region E)
//   M[sigma, sigma'] += sum_{b, b'} op(B[b, sigma, a, b']) U[b, b']        for sigma = wave, wave + 16, ..: one wave per
// sigma, its lanes stride over (b, b') in ascending order and are summed with shuffles, lane 0 adds the ancilla values
// in ascending order into the result - no barrier per sigma.  L[b, .] is one address per b group; R is stored
// transposed, so the lanes (b') read R[b', k'] side by side; the reads of V are one address per b group.
template <bool CPLX, class Row>
__device__ __forceinline__ void chain_close_site(const Row* __restrict__ sites, int nsite, int e_elems,
                                                 const void* __restrict__ pool, double* __restrict__ out) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double walk_lds[];
  T* U = reinterpret_cast<T*>(walk_lds);
  T* V = U + e_elems;
  const Row s = sites[nsite + blockIdx.x];
  const int Dbl = walk_Dbl(s), Dkl = walk_Dkl(s), d = s.d, danc = s.danc, Dbr = walk_Dbr(s), Dkr = walk_Dkr(s);
  const int krow = d * danc * Dkr, brow = d * danc * Dbr;
  const int pv = Dkr | 1, nU = Dbl * Dbr;
  const T* L = static_cast<const T*>(pool) + s.eoff;
  const T* Rt = L + Dbl * Dkl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int sp = 0; sp < d; ++sp) {
    for (int g = 0; g < danc; ++g) {
      walk_left_slice<CPLX>(s, krow, (sp * danc + g) * Dkr, L, Dkl, V, pv);
      for (int o = tid; o < nU; o += CHAIN_THREADS) {
        const int b = o / Dbr, bp = o - b * Dbr;
        const T* v_row = V + b * pv;
        T sum = El::zero();
#pragma unroll 4
        for (int kp = 0; kp < Dkr; ++kp) El::fma(sum, v_row[kp], Rt[kp * Dbr + bp]);
        U[o] = sum;
      }
      __syncthreads();   // the next U is written behind the barrier after the next V: every wave is through its sums then
      for (int sg = wave; sg < d; sg += CHAIN_WAVES) {
        const int b0 = (sg * danc + g) * Dbr;
        T part = El::zero();
        for (int o = lane; o < nU; o += 64) {
          const int b = o / Dbr, bp = o - b * Dbr;
          El::fma(part, walk_ld_bra<CPLX>(s, b * brow + b0 + bp), U[o]);
        }
        part = walk_wave_sum<CPLX>(part);
        if (lane == 0) {
          double* dst = out + 2 * (s.ooff + (int64_t)sg * d + sp);
          dst[0] = (g ? dst[0] : 0.0) + El::re(part);
          dst[1] = (g ? dst[1] : 0.0) + El::im(part);
        }
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- host side
// descriptor row i of the table, `sel` its position in the selection or -1
template <class Row>
static Row chain_site_row(const ChainSelArgs& a, int i, int sel, int64_t eoff, int64_t ooff) {
  if constexpr (walk_two_chains<Row>) {
    const ChainExt x = a.ext(i);
    const int bra_c = a.bra_dtype[i] == MPSE_C128, ket_c = a.dtype[i] == MPSE_C128;
    return Row{Chain2Row{a.bra[i], a.sites[i], (int)x.Dbl, (int)x.Dkl, (int)x.d, (int)x.danc, (int)x.Dbr, (int)x.Dkr,
                         bra_c, ket_c, (a.conj_bra != 0 && bra_c) ? 1 : 0, sel},
               eoff, ooff};
  } else {
    return Row{chain_sel_row(a, i, sel), eoff, ooff};
  }
}

// The chain path: stages the rows, runs launch(table, pooled environments, result) - the CHAIN_LAUNCH of the *_envs
// kernel on two workgroups and of the *_sites kernel on nsel, chain_lds_attr first - and reads the result, once
template <class Row, class Launch>
static int chain_sites_launch(mpse_ctx* ctx, const ChainSelArgs& a, bool cplx, Launch&& launch, double* out_host) {
  std::vector<Row> rows((size_t)a.nsite + a.nsel);
  int64_t e_elems = 0, o_elems = 0;
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const ChainExt x = a.ext(i);
    const bool is_sel = k < a.nsel && a.sel[k] == i;
    rows[i] = chain_site_row<Row>(a, i, is_sel ? k : -1, is_sel ? e_elems : 0, is_sel ? o_elems : 0);
    if (is_sel) {
      rows[(size_t)a.nsite + k] = rows[i];
      e_elems += x.Dbl * x.Dkl + x.Dbr * x.Dkr;
      o_elems += x.d * x.d;
      ++k;
    }
  }
  const size_t es = cplx ? 16 : 8, n_out = (size_t)o_elems * 2;
  TmpBuf tab(ctx), pool(ctx), res(ctx);
  MPSE_TRY(chain_stage_rows(ctx, tab, rows));
  MPSE_TRY(pool.alloc((size_t)e_elems * es));
  MPSE_TRY(res.alloc(n_out * sizeof(double)));
  MPSE_TRY(launch(tab.as<const Row>(), pool.p, res.as<double>()));
  MPSE_HIP(ctx, hipGetLastError());
  return mpse_memcpy_d2h(ctx, out_host, res.p, n_out * sizeof(double));
}

// The same contractions as products of the contraction kernel, in one dtype: complex as soon as any tensor is (real
// sites are widened into pooled copies first).  The plain products: ChainSelEnq of mpse_chain_walk.h.
//   right pass, site i from the last one down to sel[0] + 1, R (Db_r, Dk_r):  Y = K . R^T (a_r),  R' = op(B) . Y^T
//     (ca_y).  R of a selected site is written straight into its place in the pooled buffer, the others alternate
//     between two scratch buffers.
//   left pass, site i from 0 to sel[nsel - 1], L (Db_l, Dk_l):  X = L . K (l_a),  L' = op(B)^T . X (ca_x)
//     selected:  Z[(b, s, a), b'] = sum_k' X[(b, s, a), k'] R_i[b', k']
//                M[s', s] = sum_(b, a, b') op(B[b, s', (a, b')]) Z[b, s, (a, b')]          (into the packed result)
static inline int chain_sites_enqueued(mpse_ctx* ctx, const ChainSelArgs& a, bool cplx, double* out_host) {
  ChainSelEnq q(ctx, cplx, a.conj_bra);
  MPSE_TRY(q.init(a));
  const size_t es = q.es;
  const int nsel = a.nsel, first = a.sel[0], last = a.sel[nsel - 1];
  int64_t r_elems = 0, o_elems = 0;
  std::vector<int64_t> roff((size_t)nsel), ooff((size_t)nsel);
  for (int k = 0; k < nsel; ++k) {
    const ChainExt x = a.ext(a.sel[k]);
    roff[k] = r_elems, ooff[k] = o_elems;
    r_elems += x.Dbr * x.Dkr;
    o_elems += x.d * x.d;
  }
  TmpBuf rbuf(ctx), res(ctx), e0(ctx), e1(ctx), x1(ctx), z(ctx);
  MPSE_TRY(q.alloc({{&rbuf, r_elems}, {&res, o_elems}, {&e0, q.e_max}, {&e1, q.e_max}, {&x1, q.x_max}, {&z, q.x_max}}));
  const double one[2] = {1.0, 0.0};
  void* scratch[2] = {e0.p, e1.p};
  // where R_i (the environment right of site i) lives
  auto r_at = [&](int i) -> void* {
    return q.pos[i] >= 0 ? static_cast<char*>(rbuf.p) + (size_t)roff[q.pos[i]] * es : scratch[i & 1];
  };
  // ---- right pass
  MPSE_TRY(stage_h2d(ctx, r_at(a.nsite - 1), one, es));
  for (int i = a.nsite - 1; i > first; --i) {
    const ChainExt x = a.ext(i);
    const int64_t p = x.d * x.danc;
    MPSE_TRY(q.a_r(x.Dkl * p, x.Dbr, x.Dkr, q.site[i], r_at(i), x1.p));
    MPSE_TRY(q.ca_y(x.Dbl, x.Dkl, p * x.Dbr, q.bra[i], x1.p, r_at(i - 1)));
  }
  // ---- left pass
  void* L = scratch[0];
  void* Ln = scratch[1];
  MPSE_TRY(stage_h2d(ctx, L, one, es));
  for (int i = 0; i <= last; ++i) {
    const ChainExt x = a.ext(i);
    const int64_t dd = x.d, da = x.danc, p = dd * da;
    MPSE_TRY(q.l_a(1, x.Dbl, x.Dkl, p * x.Dkr, L, q.site[i], x1.p));
    if (q.pos[i] >= 0) {
      MPSE_TRY(q.a_r(x.Dbl * p, x.Dbr, x.Dkr, x1.p, r_at(i), z.p));
      MPSE_TRY(q.gemm(1, idx1(dd, da * x.Dbr), idx2(x.Dbl, da * x.Dbr, p * x.Dbr, 1),
                      idx2(x.Dbl, da * x.Dbr, p * x.Dbr, 1), idx1(dd, da * x.Dbr), idx1(dd, dd), idx1(dd, 1), 1, 0, 0, 0,
                      q.bra[i], z.p, static_cast<char*>(res.p) + (size_t)ooff[q.pos[i]] * es));
    }
    if (i == last) break;
    MPSE_TRY(q.ca_x(1, x.Dbl * p, x.Dbr, x.Dkr, q.bra[i], x1.p, Ln));
    std::swap(L, Ln);
  }
  return chain_read_pairs(ctx, res.p, o_elems, cplx, {{0, o_elems, 0}}, out_host);
}

// Tail of the two entry points behind the prologue and the plan: the path the plan chose, the call counted in `stats`
template <class Row, class Launch>
static int chain_sites_call(mpse_ctx* ctx, const ChainSelArgs& a, bool cplx, bool chain, long long* stats,
                            Launch&& launch, double* out_host) {
  int64_t n_out = 0;
  for (int k = 0; k < a.nsel; ++k) n_out += a.ext(a.sel[k]).d * a.ext(a.sel[k]).d;
  std::vector<double> res((size_t)n_out * 2, 0.0);
  if (chain)
    MPSE_TRY(chain_sites_launch<Row>(ctx, a, cplx, launch, res.data()));
  else
    MPSE_TRY(chain_sites_enqueued(ctx, a, cplx, res.data()));
  return chain_sel_done(stats, chain, a.nsite, a.nsel, res, out_host);
}
