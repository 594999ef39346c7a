// mpse_mps_rdm1: the one-site reduced density matrices
//   rho_i[p, p'] = sum_{a,a',g,b,b'} conj(A[a,p,g,b]) L_i[a,a'] A[a',p',g,b'] R_i[b,b']
// of selected sites of ONE chain as one engine call (the reference closes every site with three products and a host
// read of its own, mps/mps.py:1547-1598 calc_1site_rdm; local expectation values <O> = sum O[p,p'] rho_i[p,p'] take one
// operator window and one host read each).  L_i / R_i: the identity-operator environments left / right of site i, first
// index from the conjugated tensor.  Two paths, chosen from the dims table alone (rdm1_plan):
//   chain      two launches, for chains whose bonds are at most RD_BOND_MAX.  k_rdm1_envs: workgroup 0 walks right to
//              left with R in LDS, workgroup 1 left to right with L in LDS (chain_walk_left); each leaves its
//              environment of every selected site in pooled memory (R transposed, so that k_rdm1_sites reads it along
//              the lanes).  k_rdm1_sites: one workgroup per selected site closes L_i and R_i around the site.
//   enqueued   the same contractions as products of the contraction kernel - every other chain
// LDS plan of either launch, working elements (8 or 16 bytes), rows padded to an odd pitch (chain_pitch):
//   region E   max over the bonds D of D * pitch(D)                 k_rdm1_envs: the environment;  k_rdm1_sites: U
//   region T   max over the sites of D_l * pitch(D_r)               k_rdm1_envs: the slice T;      k_rdm1_sites: V
// (U is D_l x D_r unpadded, D_l * D_r <= max(D_l, D_r) * pitch(max(D_l, D_r)) <= E.)  L and R of k_rdm1_sites stay in
// the pooled buffer and are read through L2: with them in LDS a complex bond of 64 would need 4 x 64 x 65 x 16 = 260 KB.
// The walk, the sizing, the entry checks and the plain products of the enqueued passes are those of mpse_chain_walk.h,
// which also says what holds for all three calls: launch order instead of flags, one host read, a fixed summation order.
#include "mpse_chain_walk.h"

namespace {

// Largest bond up to which the two launches are faster than the enqueued products: measured with tools/rdm1_bench.py,
// profiles/rdm1.md (ahead at 8 and 16 on both models; at 32 ahead with 4 phonon levels, behind with 16; each walk being
// one workgroup on one compute unit, far behind at 64).  Chains between this and CHAIN_BOND_FIT take the kernels only
// under MPSE_RDM1_CHAIN=1.
constexpr int64_t RD_BOND_MAX = 16;
static_assert(1 <= RD_BOND_MAX && RD_BOND_MAX <= CHAIN_BOND_FIT, "the measured limit lies inside what fits");
// The grid of k_rdm1_sites is one workgroup per selected site, whatever their number: no cap on nsel.

struct RdSite : ChainSelRow {   // one row of the table (48 bytes): nsite rows, then the selected sites' rows again
  int64_t eoff;   // working elements before L of this site in the pooled buffer; R (transposed) at + Dl Dl
  int64_t ooff;   // complex elements before rho of this site in the result
};
static_assert(sizeof(RdSite) == 48, "descriptor rows are copied as 8-byte words");

// the sizing of a table that is a chain
ChainSelPlan rdm1_plan(int nsite, const int64_t* dims, int nsel, bool cplx) {
  return chain_sel_plan(nsite, dims, nsel >= 1, 0, cplx, RD_BOND_MAX);
}

// Workgroup 0 of k_rdm1_envs.  R_N = 1.  At a selected site R goes to the pooled buffer, transposed; the walk ends at
// the first selected site.  Else per site from the right, per (sigma, a) in ascending order the transfer to the right:
// T = A[sigma, a] . R into LDS (walk_right_slice), R' += S in the owner's registers (walk_acc_add).  R' replaces R in
// LDS after the last (sigma, a).
template <bool CPLX>
__device__ void rd_walk_right(const RdSite* __restrict__ sites, int nsite, int first, ChainT<CPLX>* R,
                              ChainT<CPLX>* Ts, ChainT<CPLX>* pool) {
  walk_env_one<CPLX>(R);
  for (int i = nsite - 1; i >= first; --i) {
    const RdSite s = sites[i];
    const int p = s.d * s.danc, row = p * s.Dr, nE = s.Dl * s.Dl;
    if (s.sel >= 0) walk_env_to_pool<CPLX, true>(R, s.Dr, pool + s.eoff + nE);
    if (i == first) break;
    ChainT<CPLX> acc[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc);
    for (int sa = 0; sa < p; ++sa) {
      walk_right_slice<CPLX>(s, row, sa * s.Dr, R, Ts);
      walk_acc_add<CPLX, false>(s, row, sa * s.Dr, Ts, nE, acc);
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of R is done as well
    }
    walk_acc_store<CPLX>(acc, s.Dl, R);
  }
}

template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_rdm1_envs(const RdSite* __restrict__ sites, int nsite, int first,
                                                             int last, int e_elems, void* pool) {
  using T = ChainT<CPLX>;
  extern __shared__ __attribute__((aligned(16))) double rd_lds[];
  T* E = reinterpret_cast<T*>(rd_lds);
  T* Ts = E + e_elems;
  if (blockIdx.x == 0)
    rd_walk_right<CPLX>(sites, nsite, first, E, Ts, static_cast<T*>(pool));
  else
    chain_walk_left<CPLX>(sites, last, E, Ts, static_cast<T*>(pool));
}

// Workgroup k closes the environments of site sel[k] (row nsite + k of the table).  Per (sigma', a) in ascending order:
//   V[a, b'] = sum_a' L[a, a'] A[a', sigma', a, b']                       (into LDS, region T: walk_left_slice with the
//                                                                          packed L as E and padded rows of V)
//   U[a, b]  = sum_b' V[a, b'] R[b, b']                                                      (into LDS, region E)
//   rho[sigma, sigma'] += sum_{a, b} conj(A[a, sigma, a, b]) U[a, b]     for sigma = wave, wave + 16, ..: one wave per
// sigma, its lanes stride over (a, b) in ascending order and are summed with shuffles, lane 0 adds the ancilla values
// in ascending order into the result - no barrier per sigma.  L[a, .] is one address per a group; R is stored
// transposed, so the lanes (b) read R[b, b'] side by side; the reads of V are one address per a group.
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_rdm1_sites(const RdSite* __restrict__ sites, int nsite, int e_elems,
                                                              const void* __restrict__ pool, double* __restrict__ out) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double rd_lds[];
  T* U = reinterpret_cast<T*>(rd_lds);
  T* V = U + e_elems;
  const RdSite s = sites[nsite + blockIdx.x];
  const int Dl = s.Dl, d = s.d, danc = s.danc, Dr = s.Dr;
  const int row = d * danc * Dr;
  const int pv = Dr | 1, nU = Dl * Dr;
  const T* L = static_cast<const T*>(pool) + s.eoff;
  const T* Rt = L + Dl * Dl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int sp = 0; sp < d; ++sp) {
    for (int g = 0; g < danc; ++g) {
      walk_left_slice<CPLX>(s, row, (sp * danc + g) * Dr, L, Dl, V, pv);
      for (int o = tid; o < nU; o += CHAIN_THREADS) {
        const int a = o / Dr, b = o - a * Dr;
        const T* v_row = V + a * pv;
        T sum = El::zero();
#pragma unroll 4
        for (int bp = 0; bp < Dr; ++bp) El::fma(sum, v_row[bp], Rt[bp * Dr + b]);
        U[o] = sum;
      }
      __syncthreads();   // the next U is written behind the barrier after the next V: every wave is through its sums then
      for (int sg = wave; sg < d; sg += CHAIN_WAVES) {
        const int s0 = (sg * danc + g) * Dr;
        T part = El::zero();
        for (int o = lane; o < nU; o += 64) {
          const int a = o / Dr, b = o - a * Dr;
          El::fma(part, El::cj(El::ld(s.a, s.cplx, a * row + s0 + b)), U[o]);
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

int rdm1_chain(mpse_ctx* ctx, const ChainSelArgs& a, bool cplx, const ChainSelPlan& pl, double* out_host) {
  std::vector<RdSite> rows((size_t)a.nsite + a.nsel);
  int64_t e_elems = 0, o_elems = 0;
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const bool is_sel = k < a.nsel && a.sel[k] == i;
    rows[i] = RdSite{chain_sel_row(a, i, is_sel ? k : -1), is_sel ? e_elems : 0, is_sel ? o_elems : 0};
    if (is_sel) {
      rows[(size_t)a.nsite + k] = rows[i];
      e_elems += d[0] * d[0] + d[3] * d[3];
      o_elems += d[1] * d[1];
      ++k;
    }
  }
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_rdm1_envs), CHAIN_KERNELS(k_rdm1_sites)}, CHAIN_LDS_MAX));
  const size_t es = cplx ? 16 : 8, n_out = (size_t)o_elems * 2;
  TmpBuf tab(ctx), pool(ctx), res(ctx);
  MPSE_TRY(chain_stage_rows(ctx, tab, rows));
  MPSE_TRY(pool.alloc((size_t)e_elems * es));
  MPSE_TRY(res.alloc(n_out * sizeof(double)));
  CHAIN_LAUNCH(ctx, cplx, k_rdm1_envs, 2, pl.lds, tab.as<const RdSite>(), a.nsite, a.sel[0], a.sel[a.nsel - 1],
               (int)pl.e_elems, pool.p);
  CHAIN_LAUNCH(ctx, cplx, k_rdm1_sites, a.nsel, pl.lds, tab.as<const RdSite>(), a.nsite, (int)pl.e_elems,
               (const void*)pool.p, res.as<double>());
  MPSE_HIP(ctx, hipGetLastError());
  return mpse_memcpy_d2h(ctx, out_host, res.p, n_out * sizeof(double));
}

// The same contractions as products of the contraction kernel, in one dtype: complex as soon as any site is (real sites
// are widened into pooled copies first, widen_site).  The plain products: ChainSelEnq of mpse_chain_walk.h.
//   right pass, site i from the last one down to sel[0] + 1, R (D_r, D_r) = [b', c']:  Y1 = A . R (a_r),  R' = conj(A) .
//   Y1 (ca_y).  R of a selected site is written straight into its place in the pooled buffer, the others alternate
//   between two scratch buffers.
//   left pass, site i from 0 to sel[nsel - 1], L (D_l, D_l) = [b, c]:  X1 = L . A (l_a),  L' = conj(A) . X1 (ca_x)
//     selected:  Y[(b, s, a), c] = sum_c' X1[(b, s, a), c'] R_i[c, c']
//                rho[s', s] = sum_(b, a, c) conj(A[b, s', (a, c)]) Y[b, s, (a, c)]       (into the packed result)
int rdm1_enqueued(mpse_ctx* ctx, const ChainSelArgs& a, bool cplx, double* out_host) {
  ChainSelEnq q(ctx, cplx);
  MPSE_TRY(q.init(a));
  const size_t es = q.es;
  const int nsel = a.nsel, first = a.sel[0], last = a.sel[nsel - 1];
  int64_t r_elems = 0, o_elems = 0;
  std::vector<int64_t> roff((size_t)nsel), ooff((size_t)nsel);
  for (int k = 0; k < nsel; ++k) {
    const int64_t* d = a.dims + 4 * a.sel[k];
    roff[k] = r_elems, ooff[k] = o_elems;
    r_elems += d[3] * d[3];
    o_elems += d[1] * d[1];
  }
  TmpBuf rbuf(ctx), res(ctx), e0(ctx), e1(ctx), x1(ctx), y(ctx);
  MPSE_TRY(q.alloc({{&rbuf, r_elems}, {&res, o_elems}, {&e0, q.e_max}, {&e1, q.e_max}, {&x1, q.x_max}, {&y, q.x_max}}));
  const double one[2] = {1.0, 0.0};
  void* scratch[2] = {e0.p, e1.p};
  // where R_i (the environment right of site i) lives
  auto r_at = [&](int i) -> void* {
    return q.pos[i] >= 0 ? static_cast<char*>(rbuf.p) + (size_t)roff[q.pos[i]] * es : scratch[i & 1];
  };
  // ---- right pass
  MPSE_TRY(stage_h2d(ctx, r_at(a.nsite - 1), one, es));
  for (int i = a.nsite - 1; i > first; --i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], p = d[1] * d[2], Dr = d[3];
    MPSE_TRY(q.a_r(Dl * p, Dr, q.site[i], r_at(i), x1.p));
    MPSE_TRY(q.ca_y(Dl, p * Dr, q.site[i], x1.p, r_at(i - 1)));
  }
  // ---- left pass
  void* L = scratch[0];
  void* Ln = scratch[1];
  MPSE_TRY(stage_h2d(ctx, L, one, es));
  for (int i = 0; i <= last; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], dd = d[1], da = d[2], Dr = d[3], p = dd * da;
    MPSE_TRY(q.l_a(1, Dl, p * Dr, L, q.site[i], x1.p));
    if (q.pos[i] >= 0) {
      MPSE_TRY(q.a_r(Dl * p, Dr, x1.p, r_at(i), y.p));
      MPSE_TRY(q.gemm(1, idx1(dd, da * Dr), idx2(Dl, da * Dr, p * Dr, 1), idx2(Dl, da * Dr, p * Dr, 1),
                      idx1(dd, da * Dr), idx1(dd, dd), idx1(dd, 1), 1, 0, 0, 0, q.site[i], y.p,
                      static_cast<char*>(res.p) + (size_t)ooff[q.pos[i]] * es));
    }
    if (i == last) break;
    MPSE_TRY(q.ca_x(1, Dl * p, Dr, q.site[i], x1.p, Ln));
    std::swap(L, Ln);
  }
  return chain_read_pairs(ctx, res.p, o_elems, cplx, {{0, o_elems, 0}}, out_host);
}

}  // namespace

extern "C" {

int mpse_mps_rdm1_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n) {
  const bool valid = chain_sel_table_ok(nsite, dims);
  const ChainSelPlan pl = valid ? rdm1_plan(nsite, dims, nsel, any_complex != 0) : ChainSelPlan{};
  return chain_sel_plan_out(pl, valid, RD_BOND_MAX, 0, {}, info, n);
}

int mpse_mps_rdm1_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::rdm1_stats, counts, n);
}

int mpse_mps_rdm1(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims, int nsel,
                  const int* sel, double* out_host) {
  const ChainSelArgs args{nsite, sites, dtype, dims, nsel, sel};
  bool cplx = false;
  MPSE_TRY(chain_sel_prologue(ctx, "mps_rdm1", args, 1, out_host != nullptr, &cplx));
  ChainSelPlan pl = rdm1_plan(nsite, dims, nsel, cplx);
  MPSE_BIND(ctx);
  chain_sel_plan_switch("MPSE_RDM1_CHAIN", &pl);
  int64_t n_out = 0;
  for (int k = 0; k < nsel; ++k) n_out += dims[4 * sel[k] + 1] * dims[4 * sel[k] + 1];
  std::vector<double> res((size_t)n_out * 2, 0.0);
  if (pl.chain)
    MPSE_TRY(rdm1_chain(ctx, args, cplx, pl, res.data()));
  else
    MPSE_TRY(rdm1_enqueued(ctx, args, cplx, res.data()));
  return chain_sel_done(ctx->rdm1_stats, pl.chain, nsite, nsel, res, out_host);
}

}  // extern "C"
