// mpse_mps_trdm1: the one-site transition density matrices
//   T_i[p, p'] = sum_{b,k,g,b',k'} op(B_i)[b,p,g,b'] L_i[b,k] K_i[k,p',g,k'] R_i[b',k']
// of selected sites of TWO chains, a bra B and a ket K, as one engine call (the reference's spectral function takes
// <gs| a_i |ket(t)> for every i with one operator window, one closing product and one host read per i plus a conjugated
// copy of the bra, transport/spectral_function.py:106-117; <bra| O_i |ket> = sum O[p,p'] T_i[p,p']).  L_i / R_i: the
// overlap environments left / right of site i, bra index first: Db rows, Dk columns - rectangular.  op: the complex
// conjugate when conj_bra is set, as in mpse_mps_overlap.  With bra == ket and conj_bra it is rho_i of mpse_mps_rdm1.
// Two paths, chosen from the dims table alone (trdm1_plan):
//   chain      two launches.  k_trdm1_envs: workgroup 0 walks right to left with R in LDS, workgroup 1 left to right with
//              L in LDS; each leaves its environment of every selected site in pooled memory (R transposed, so that
//              k_trdm1_sites reads it along the lanes).  k_trdm1_sites: one workgroup per selected site closes L_i and
//              R_i around the site.
//   enqueued   the same contractions as products of the contraction kernel - every other chain
// LDS plan of either launch, working elements (8 or 16 bytes), rows padded to an odd pitch (chain_pitch):
//   region E   max over the bonds of Db * pitch(Dk) and over the sites of Db_l * Db_r
//              k_trdm1_envs: the environment;  k_trdm1_sites: U (Db_l x Db_r, unpadded)
//   region T   max over the sites of Db_l * pitch(Dk_r) and Dk_l * pitch(Db_r)
//              k_trdm1_envs: the slice T of the walk from the left resp. from the right;  k_trdm1_sites: V (Db_l rows)
// The argument of mpse_rdm1.hip that U fits in the environment's region does not hold for rectangular environments (Db
// = 64, Dk = 1: U has 4096 elements, an environment 64), so region E is sized for U as well; k_trdm1_sites closes in
// the one order ket first, bra last, whatever the bonds.  L and R of k_trdm1_sites stay in the pooled buffer and are
// read through L2.  The launches FIT when the plan is within CHAIN_LDS_MAX, Db * Dk <= CHAIN_THREADS *
// CHAIN_OUT_PER_THREAD at every bond (one accumulator per entry of an environment), d, danc and d * danc <=
// CHAIN_EXT_MAX and every site tensor has fewer than 2^31 elements (the offsets into a site are 32-bit).  Launch order
// instead of flags, one host read, a fixed summation order: as said in mpse_chain_walk.h, whose walk2_* stages these
// kernels use.
#include "mpse_chain_walk.h"

namespace {

// Largest bond of either chain up to which the two launches are faster than the enqueued products: measured with
// tools/trdm1_bench.py, profiles/trdm1.md (bra and ket of one bond: ahead at 8 and 16 on both models; at 32 ahead with 4
// phonon levels, behind with 16 - the limit profiles/rdm1.md found for the square walk).  Chains above it that fit
// take the kernels only under MPSE_TRDM1_CHAIN=1.
constexpr int64_t TR_BOND_MAX = 16;
// The ket's limit when every bond of the bra is 1 (a product-state bra: the environments are rows): ahead at 16 and 32
// on both models; at 64 ahead with 4 phonon levels, behind with 16; each walk being one workgroup of which Dk threads
// work, far behind at 256
constexpr int64_t TR_BOND_MAX_BRA1 = 32;
static_assert(1 <= TR_BOND_MAX && TR_BOND_MAX <= TR_BOND_MAX_BRA1, "a bond-1 bra is the cheaper case");
constexpr int64_t TR_ACC_MAX = int64_t(CHAIN_THREADS) * CHAIN_OUT_PER_THREAD;
constexpr int64_t TR_SITE_ELEMS_MAX = (int64_t(1) << 31) - 1;

static_assert(mpse_ctx::TR_SITES == 2 && mpse_ctx::TR_MATRICES == 3, "chain_sel_done: chain, enqueued, sites, results");

struct TrSite : Chain2Row {   // one row of the table (72 bytes): nsite rows, then the selected sites' rows again
  int64_t eoff;   // working elements before L of this site in the pooled buffer; R (transposed) at + Db_l Dk_l
  int64_t ooff;   // complex elements before T of this site in the result
};
static_assert(sizeof(TrSite) == 72, "descriptor rows are copied as 8-byte words");

struct TrArgs {
  int nsite;
  const void* const* bra;
  const int* bra_dtype;
  const void* const* ket;
  const int* ket_dtype;
  const int64_t* dims;   // nsite rows (Db_l, Dk_l, d, danc, Db_r, Dk_r)
  int conj_bra;
  int nsel;
  const int* sel;
};

struct TrPlan {
  bool chain;            // the chain kernels take it
  bool fit;              // they could, whatever the bond limits of the rule say
  int64_t max_bra, max_ket;
  int64_t e_elems;       // LDS elements of region E
  int64_t t_elems;       // LDS elements of region T
  int64_t lds;           // bytes of either launch, working dtype
};

bool trdm1_table_ok(int nsite, const int64_t* dims) { return chain_table_ok(nsite, dims, 6, {0, 1}, {4, 5}); }

// the sizing of a table that is a chain
TrPlan trdm1_plan(int nsite, const int64_t* dims, int nsel, bool cplx) {
  TrPlan pl{false, false, 0, 0, 0, 0, 0};
  bool fits = nsel >= 1;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + 6 * i;
    pl.max_bra = std::max({pl.max_bra, d[0], d[4]});
    pl.max_ket = std::max({pl.max_ket, d[1], d[5]});
    bool ok = d[2] <= CHAIN_EXT_MAX && d[3] <= CHAIN_EXT_MAX && d[2] * d[3] <= CHAIN_EXT_MAX;
    for (int j : {0, 4}) ok = ok && d[j] <= TR_ACC_MAX && d[j + 1] <= TR_ACC_MAX && d[j] * d[j + 1] <= TR_ACC_MAX;
    ok = ok && d[0] * d[2] * d[3] * d[4] <= TR_SITE_ELEMS_MAX && d[1] * d[2] * d[3] * d[5] <= TR_SITE_ELEMS_MAX;
    if (!ok) {
      fits = false;
      continue;
    }
    pl.e_elems = std::max({pl.e_elems, d[0] * chain_pitch(d[1]), d[4] * chain_pitch(d[5]), d[0] * d[4]});
    pl.t_elems = std::max({pl.t_elems, d[0] * chain_pitch(d[5]), d[1] * chain_pitch(d[4])});
  }
  if (fits) {
    pl.lds = (pl.e_elems + pl.t_elems) * (cplx ? 16 : 8);
    pl.fit = pl.lds <= CHAIN_LDS_MAX;
  }
  if (!pl.fit) pl.lds = pl.e_elems = pl.t_elems = 0;
  const bool in_rule = (pl.max_bra <= TR_BOND_MAX && pl.max_ket <= TR_BOND_MAX) ||
                       (pl.max_bra == 1 && pl.max_ket <= TR_BOND_MAX_BRA1);
  pl.chain = pl.fit && in_rule;
  return pl;
}

// Workgroup 0 of k_trdm1_envs.  R_N = 1.  At a selected site R goes to the pooled buffer, transposed; the walk ends at
// the first selected site.  Else per site from the right, per (sigma, a) in ascending order: T = K[sigma, a] . R^T into
// LDS (walk2_right_slice), R' += op(B[sigma, a]) . T^T in the owner's registers.  R' replaces R in LDS after the last
// (sigma, a).
template <bool CPLX>
__device__ void tr_walk_right(const TrSite* __restrict__ sites, int nsite, int first, ChainT<CPLX>* R, ChainT<CPLX>* Ts,
                              ChainT<CPLX>* pool) {
  walk_env_one<CPLX>(R);
  for (int i = nsite - 1; i >= first; --i) {
    const TrSite s = sites[i];
    const int p = s.d * s.danc, krow = p * s.Dkr, brow = p * s.Dbr, nE = s.Dbl * s.Dkl;
    if (s.sel >= 0) walk2_env_to_pool<CPLX, true>(R, s.Dbr, s.Dkr, pool + s.eoff + nE);
    if (i == first) break;
    ChainT<CPLX> acc[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc);
    for (int sa = 0; sa < p; ++sa) {
      walk2_right_slice<CPLX>(s, krow, sa * s.Dkr, R, Ts);
#pragma unroll
      for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) {
        const int o = threadIdx.x + j * CHAIN_THREADS;
        if (o < nE) {
          ChainT<CPLX> S;
          walk2_right_sum<CPLX>(s, brow, sa * s.Dbr, o, Ts, S);
          ChainEl<CPLX>::add(acc[j], S);
        }
      }
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of R is done as well
    }
    walk2_acc_store<CPLX>(acc, s.Dbl, s.Dkl, R);
  }
}

// Workgroup 1.  L_0 = 1.  At a selected site L goes to the pooled buffer; the walk ends at the last selected site.  Else
// per site from the left, per (sigma, a) in ascending order: T = L . K[sigma, a] into LDS (packed rows), L' +=
// op(B[sigma, a])^T . T in the owner's registers.
template <bool CPLX>
__device__ void tr_walk_left(const TrSite* __restrict__ sites, int last, ChainT<CPLX>* L, ChainT<CPLX>* Ts,
                             ChainT<CPLX>* pool) {
  walk_env_one<CPLX>(L);
  for (int i = 0; i <= last; ++i) {
    const TrSite s = sites[i];
    const int p = s.d * s.danc, krow = p * s.Dkr, brow = p * s.Dbr, nE = s.Dbr * s.Dkr;
    if (s.sel >= 0) walk2_env_to_pool<CPLX, false>(L, s.Dbl, s.Dkl, pool + s.eoff);
    if (i == last) break;
    ChainT<CPLX> acc[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc);
    for (int sa = 0; sa < p; ++sa) {
      walk2_left_slice<CPLX>(s, krow, sa * s.Dkr, L, s.Dkl | 1, Ts, s.Dkr);
#pragma unroll
      for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) {
        const int o = threadIdx.x + j * CHAIN_THREADS;
        if (o < nE) {
          ChainT<CPLX> S;
          walk2_left_sum<CPLX>(s, brow, sa * s.Dbr, o, Ts, s.Dkr, S);
          ChainEl<CPLX>::add(acc[j], S);
        }
      }
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of L is done as well
    }
    walk2_acc_store<CPLX>(acc, s.Dbr, s.Dkr, L);
  }
}

template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_trdm1_envs(const TrSite* __restrict__ sites, int nsite, int first,
                                                              int last, int e_elems, void* pool) {
  using T = ChainT<CPLX>;
  extern __shared__ __attribute__((aligned(16))) double tr_lds[];
  T* E = reinterpret_cast<T*>(tr_lds);
  T* Ts = E + e_elems;
  if (blockIdx.x == 0)
    tr_walk_right<CPLX>(sites, nsite, first, E, Ts, static_cast<T*>(pool));
  else
    tr_walk_left<CPLX>(sites, last, E, Ts, static_cast<T*>(pool));
}

// Workgroup j closes the environments of site sel[j] (row nsite + j of the table).  Per (sigma', a) in ascending order:
//   V[b, k'] = sum_k L[b, k] K[k, sigma', a, k']                            (into LDS, region T: walk2_left_slice with the
//                                                                            packed L as E and padded rows of V)
//   U[b, b'] = sum_k' V[b, k'] R[b', k']                                                       (into LDS, region E)
//   T[sigma, sigma'] += sum_{b, b'} op(B[b, sigma, a, b']) U[b, b']        for sigma = wave, wave + 16, ..: one wave per
// sigma, its lanes stride over (b, b') in ascending order and are summed with shuffles, lane 0 adds the ancilla values
// in ascending order into the result - no barrier per sigma.  R is stored transposed, so the lanes (b') read R[b', k']
// side by side; the reads of V are one address per b group.
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_trdm1_sites(const TrSite* __restrict__ sites, int nsite, int e_elems,
                                                               const void* __restrict__ pool, double* __restrict__ out) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double tr_lds[];
  T* U = reinterpret_cast<T*>(tr_lds);
  T* V = U + e_elems;
  const TrSite s = sites[nsite + blockIdx.x];
  const int Dbl = s.Dbl, Dkl = s.Dkl, d = s.d, danc = s.danc, Dbr = s.Dbr, Dkr = s.Dkr;
  const int krow = d * danc * Dkr, brow = d * danc * Dbr;
  const int pv = Dkr | 1, nU = Dbl * Dbr;
  const T* L = static_cast<const T*>(pool) + s.eoff;
  const T* Rt = L + Dbl * Dkl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int sp = 0; sp < d; ++sp) {
    for (int g = 0; g < danc; ++g) {
      walk2_left_slice<CPLX>(s, krow, (sp * danc + g) * Dkr, L, Dkl, V, pv);
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
          El::fma(part, walk2_ld_bra<CPLX>(s, b * brow + b0 + bp), U[o]);
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

int trdm1_chain(mpse_ctx* ctx, const TrArgs& a, bool cplx, const TrPlan& pl, double* out_host) {
  std::vector<TrSite> rows((size_t)a.nsite + a.nsel);
  int64_t e_elems = 0, o_elems = 0;
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const int64_t* d = a.dims + 6 * i;
    const bool is_sel = k < a.nsel && a.sel[k] == i;
    const int bra_c = a.bra_dtype[i] == MPSE_C128, ket_c = a.ket_dtype[i] == MPSE_C128;
    rows[i] = TrSite{Chain2Row{a.bra[i], a.ket[i], (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5],
                               bra_c, ket_c, (a.conj_bra != 0 && bra_c) ? 1 : 0, is_sel ? k : -1},
                     is_sel ? e_elems : 0, is_sel ? o_elems : 0};
    if (is_sel) {
      rows[(size_t)a.nsite + k] = rows[i];
      e_elems += d[0] * d[1] + d[4] * d[5];
      o_elems += d[2] * d[2];
      ++k;
    }
  }
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_trdm1_envs), CHAIN_KERNELS(k_trdm1_sites)}, CHAIN_LDS_MAX));
  const size_t es = cplx ? 16 : 8, n_out = (size_t)o_elems * 2;
  TmpBuf tab(ctx), pool(ctx), res(ctx);
  MPSE_TRY(chain_stage_rows(ctx, tab, rows));
  MPSE_TRY(pool.alloc((size_t)e_elems * es));
  MPSE_TRY(res.alloc(n_out * sizeof(double)));
  CHAIN_LAUNCH(ctx, cplx, k_trdm1_envs, 2, pl.lds, tab.as<const TrSite>(), a.nsite, a.sel[0], a.sel[a.nsel - 1],
               (int)pl.e_elems, pool.p);
  CHAIN_LAUNCH(ctx, cplx, k_trdm1_sites, a.nsel, pl.lds, tab.as<const TrSite>(), a.nsite, (int)pl.e_elems,
               (const void*)pool.p, res.as<double>());
  MPSE_HIP(ctx, hipGetLastError());
  return mpse_memcpy_d2h(ctx, out_host, res.p, n_out * sizeof(double));
}

// The same contractions as products of the contraction kernel, in one dtype: complex as soon as any tensor of either
// chain is (real sites are widened into pooled copies first, widen_site).  The four products of ChainSelEnq are square;
// these are their rectangular counterparts, B (Db_l, p, Db_r) and K (Dk_l, p, Dk_r) with p = d danc, op(B) through the
// conjugation flag of the product:
//   right pass, site i from the last one down to sel[0] + 1, R (Db_r, Dk_r):  Y[(k, s), b'] = sum_k' K[(k, s), k'] R[b',
//     k'],  R'[b, k] = sum_(s, b') op(B[b, (s, b')]) Y[k, (s, b')].  R of a selected site is written straight into its
//     place in the pooled buffer, the others alternate between two scratch buffers.
//   left pass, site i from 0 to sel[nsel - 1], L (Db_l, Dk_l):  X[b, (s, k')] = sum_k L[b, k] K[k, (s, k')],
//     L'[b', k'] = sum_(b, s) op(B[(b, s), b']) X[(b, s), k']
//     selected:  Z[(b, s, a), b'] = sum_k' X[(b, s, a), k'] R_i[b', k']
//                T[s', s] = sum_(b, a, b') op(B[b, s', (a, b')]) Z[b, s, (a, b')]          (into the packed result)
struct TrEnq {
  mpse_ctx* ctx;
  int dt, cj;   // cj: conjugate B, set for a complex call that conjugates the bra
  size_t es;
  std::vector<const void*> bra, ket;
  std::vector<std::unique_ptr<TmpBuf>> wide;

  TrEnq(mpse_ctx* c, bool cplx, int conj_bra)
      : ctx(c), dt(cplx ? MPSE_C128 : MPSE_F64), cj(cplx && conj_bra ? 1 : 0), es(cplx ? 16 : 8) {}
  int init(const TrArgs& a) {
    bra.assign(a.bra, a.bra + a.nsite);
    ket.assign(a.ket, a.ket + a.nsite);
    for (int i = 0; i < a.nsite && dt == MPSE_C128; ++i) {
      const int64_t* d = a.dims + 6 * i;
      const int64_t p = d[2] * d[3];
      if (a.bra_dtype[i] != MPSE_C128) {
        wide.emplace_back(new TmpBuf(ctx));
        MPSE_TRY(widen_site(ctx, *wide.back(), &bra[i], d[0] * p * d[4], d[0] * p * d[4]));
      }
      if (a.ket_dtype[i] != MPSE_C128) {
        wide.emplace_back(new TmpBuf(ctx));
        MPSE_TRY(widen_site(ctx, *wide.back(), &ket[i], d[1] * p * d[5], d[1] * p * d[5]));
      }
    }
    return MPSE_OK;
  }
  int gemm(int conj_a, mpse_index ma, mpse_index ka, mpse_index kb, mpse_index nb, mpse_index mc, mpse_index nc,
           const void* A, const void* B, void* C) const {
    return gemm_call(ctx, dt, dt, conj_a ? cj : 0, 0, ma, ka, kb, nb, mc, nc, 1, 0, 0, 0, A, B, C);
  }
  //   Y[r, b'] = sum_k' A[r, k'] R[b', k']: n rows of Dk_r elements against R (Db_r, Dk_r)
  int a_rt(int64_t n, int64_t Dbr, int64_t Dkr, const void* A, const void* R, void* Y) const {
    return gemm(0, idx1(n, Dkr), idx1(Dkr, 1), idx1(Dkr, 1), idx1(Dbr, Dkr), idx1(n, Dbr), idx1(Dbr, 1), A, R, Y);
  }
  //   R'[b, k] = sum_j op(B[b, j]) Y[k, j],  j = (s, a, b'): kk = p Db_r
  int b_yt(int64_t Dbl, int64_t Dkl, int64_t kk, const void* B, const void* Y, void* Rn) const {
    return gemm(1, idx1(Dbl, kk), idx1(kk, 1), idx1(kk, 1), idx1(Dkl, kk), idx1(Dbl, Dkl), idx1(Dkl, 1), B, Y, Rn);
  }
  //   X[b, j] = sum_k L[b, k] K[k, j],  j = (s, a, k'): n = p Dk_r
  int l_k(int64_t Dbl, int64_t Dkl, int64_t n, const void* L, const void* K, void* X) const {
    return gemm(0, idx1(Dbl, Dkl), idx1(Dkl, 1), idx1(Dkl, n), idx1(n, 1), idx1(Dbl, n), idx1(n, 1), L, K, X);
  }
  //   L'[b', k'] = sum_r op(B[r, b']) X[r, k'],  r = (b, s, a): m = Db_l p
  int bt_x(int64_t m, int64_t Dbr, int64_t Dkr, const void* B, const void* X, void* Ln) const {
    return gemm(1, idx1(Dbr, 1), idx1(m, Dbr), idx1(m, Dkr), idx1(Dkr, 1), idx1(Dbr, Dkr), idx1(Dkr, 1), B, X, Ln);
  }
};

int trdm1_enqueued(mpse_ctx* ctx, const TrArgs& a, bool cplx, double* out_host) {
  TrEnq q(ctx, cplx, a.conj_bra);
  MPSE_TRY(q.init(a));
  const size_t es = q.es;
  const int nsel = a.nsel, first = a.sel[0], last = a.sel[nsel - 1];
  std::vector<int> pos((size_t)a.nsite, -1);
  int64_t r_elems = 0, o_elems = 0, e_max = 1, x_max = 1;
  std::vector<int64_t> roff((size_t)nsel), ooff((size_t)nsel);
  for (int k = 0; k < nsel; ++k) {
    const int64_t* d = a.dims + 6 * a.sel[k];
    pos[a.sel[k]] = k;
    roff[k] = r_elems, ooff[k] = o_elems;
    r_elems += d[4] * d[5];
    o_elems += d[2] * d[2];
  }
  for (int i = 0; i < a.nsite; ++i) {
    const int64_t* d = a.dims + 6 * i;
    const int64_t p = d[2] * d[3];
    e_max = std::max({e_max, d[0] * d[1], d[4] * d[5]});
    x_max = std::max({x_max, d[1] * p * d[4], d[0] * p * d[5], d[0] * p * d[4]});
  }
  TmpBuf rbuf(ctx), res(ctx), e0(ctx), e1(ctx), x1(ctx), z(ctx);
  const std::initializer_list<std::pair<TmpBuf*, int64_t>> bufs = {{&rbuf, r_elems}, {&res, o_elems}, {&e0, e_max},
                                                                   {&e1, e_max},    {&x1, x_max},  {&z, x_max}};
  for (const auto& b : bufs) MPSE_TRY(b.first->alloc((size_t)b.second * es));
  const double one[2] = {1.0, 0.0};
  void* scratch[2] = {e0.p, e1.p};
  // where R_i (the environment right of site i) lives
  auto r_at = [&](int i) -> void* {
    return pos[i] >= 0 ? static_cast<char*>(rbuf.p) + (size_t)roff[pos[i]] * es : scratch[i & 1];
  };
  // ---- right pass
  MPSE_TRY(stage_h2d(ctx, r_at(a.nsite - 1), one, es));
  for (int i = a.nsite - 1; i > first; --i) {
    const int64_t* d = a.dims + 6 * i;
    const int64_t Dbl = d[0], Dkl = d[1], p = d[2] * d[3], Dbr = d[4], Dkr = d[5];
    MPSE_TRY(q.a_rt(Dkl * p, Dbr, Dkr, q.ket[i], r_at(i), x1.p));
    MPSE_TRY(q.b_yt(Dbl, Dkl, p * Dbr, q.bra[i], x1.p, r_at(i - 1)));
  }
  // ---- left pass
  void* L = scratch[0];
  void* Ln = scratch[1];
  MPSE_TRY(stage_h2d(ctx, L, one, es));
  for (int i = 0; i <= last; ++i) {
    const int64_t* d = a.dims + 6 * i;
    const int64_t Dbl = d[0], Dkl = d[1], dd = d[2], da = d[3], Dbr = d[4], Dkr = d[5], p = dd * da;
    MPSE_TRY(q.l_k(Dbl, Dkl, p * Dkr, L, q.ket[i], x1.p));
    if (pos[i] >= 0) {
      MPSE_TRY(q.a_rt(Dbl * p, Dbr, Dkr, x1.p, r_at(i), z.p));
      MPSE_TRY(q.gemm(1, idx1(dd, da * Dbr), idx2(Dbl, da * Dbr, p * Dbr, 1), idx2(Dbl, da * Dbr, p * Dbr, 1),
                      idx1(dd, da * Dbr), idx1(dd, dd), idx1(dd, 1), q.bra[i], z.p,
                      static_cast<char*>(res.p) + (size_t)ooff[pos[i]] * es));
    }
    if (i == last) break;
    MPSE_TRY(q.bt_x(Dbl * p, Dbr, Dkr, q.bra[i], x1.p, Ln));
    std::swap(L, Ln);
  }
  return chain_read_pairs(ctx, res.p, o_elems, cplx, {{0, o_elems, 0}}, out_host);
}

// What the entry point refuses before any device work, in the order of chain_sel_prologue
int trdm1_prologue(mpse_ctx* ctx, const TrArgs& a, bool out, bool* cplx) {
  if (!ctx) return MPSE_ERR_ARG;
  if (a.nsite < 1 || !a.bra || !a.bra_dtype || !a.ket || !a.ket_dtype || !a.dims || a.nsel < 1 || !a.sel || !out)
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_trdm1: null argument, no sites or no selection");
  MPSE_TRY(chain_scan_sites(ctx, "mps_trdm1", a.nsite, {a.bra, a.ket}, {a.bra_dtype, a.ket_dtype}, cplx));
  if (!chain_sel_ok(a.nsite, a.nsel, a.sel))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "mps_trdm1: the selection is not strictly ascending inside [0, %d)", a.nsite);
  if (!trdm1_table_ok(a.nsite, a.dims))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "mps_trdm1: dims is not a chain (extents >= 1, matching neighbours, first and last bonds 1)");
  if (MPSE_RECORDING(ctx))
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_trdm1: synchronous, not available while a deferred list is recorded");
  return MPSE_OK;
}

}  // namespace

extern "C" {

int mpse_mps_trdm1_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n) {
  const bool valid = trdm1_table_ok(nsite, dims);
  const TrPlan pl = valid ? trdm1_plan(nsite, dims, nsel, any_complex != 0) : TrPlan{};
  const int64_t v[14] = {TR_BOND_MAX, CHAIN_LDS_MAX, pl.chain ? pl.lds : 0, pl.e_elems, pl.t_elems, CHAIN_THREADS,
                         pl.max_bra, pl.max_ket, valid ? 1 : 0, 0, CHAIN_EXT_MAX, TR_ACC_MAX, pl.lds, TR_BOND_MAX_BRA1};
  plan_info_out(info, n, v, 14);
  return pl.chain ? 1 : 0;
}

int mpse_mps_trdm1_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::trdm1_stats, counts, n);
}

int mpse_mps_trdm1(mpse_ctx* ctx, int nsite, const void* const* bra, const int* bra_dtype, const void* const* ket,
                   const int* ket_dtype, const int64_t* dims, int conj_bra, int nsel, const int* sel, double* out_host) {
  const TrArgs args{nsite, bra, bra_dtype, ket, ket_dtype, dims, conj_bra, nsel, sel};
  bool cplx = false;
  MPSE_TRY(trdm1_prologue(ctx, args, out_host != nullptr, &cplx));
  TrPlan pl = trdm1_plan(nsite, dims, nsel, cplx);
  MPSE_BIND(ctx);
  const char env = chain_env_switch("MPSE_TRDM1_CHAIN");   // as chain_sel_plan_switch
  if (env == '0') pl.chain = false;
  if (env == '1') pl.chain = pl.fit;
  int64_t n_out = 0;
  for (int k = 0; k < nsel; ++k) n_out += dims[6 * sel[k] + 2] * dims[6 * sel[k] + 2];
  std::vector<double> res((size_t)n_out * 2, 0.0);
  if (pl.chain)
    MPSE_TRY(trdm1_chain(ctx, args, cplx, pl, res.data()));
  else
    MPSE_TRY(trdm1_enqueued(ctx, args, cplx, res.data()));
  return chain_sel_done(ctx->trdm1_stats, pl.chain, nsite, nsel, res, out_host);
}

}  // extern "C"
