// mpse_mps_expect_many: <psi| O_m |psi> of a LIST of MPOs against ONE chain as one engine call with one host read (the
// reference takes every operator as its own Environ walk, mps/mp.py expectations; a polaron-structure job asks for
// nmol^2 of them after every step).  Operator m is the identity outside its window [first_m, last_m]; only the MPO
// sites of the window are given.  Bond j lies left of site j (j = 0 .. nsite); L_j (D_j x D_j, first index from the
// conjugated tensor) is the identity environment of the sites before it, R_j that of the sites from j on, and
//   <O_m> = sum_{b, k} E_m[b, 0, k] R_{last_m + 1}[b, k],   E_m = L_{first_m} carried through the window with the MPO.
// L_0 and R_nsite are the 1 x 1 sentinel.  Two paths, chosen from the dims tables alone (expect_plan):
//   chain      two launches.  k_expect_envs: the two walks of k_bondspec_envs, one workgroup from either end; they leave
//              L and R of every distinct window edge in pooled memory.  k_expect_windows: one workgroup per operator
//              loads its L into LDS as the transfer tensor E (D, 1, D), walks its window with the site step of
//              k_sandwich_chain (sw_site_step) and closes against its R with cr_block_sum.  More operators than
//              EX_GRID_MAX: the second kernel is launched again, within the call.
//   enqueued   the same environments as products of the contraction kernel (ChainSelEnq), each window with the
//              environment-update plan that mpse_mps_sandwich enqueues, every closing as a product into one device
//              result - every other call
// A workgroup reads only what the launch before it wrote: no atomics, no flags; a fixed summation order.
#include "mpse_chain_walk.h"
#include "mpse_sandwich_step.h"

namespace {

// Largest state bond up to which the two launches are faster than the enqueued path on both Holstein chains of
// tools/expect_many_bench.py for both of its operator lists (profiles/expect_many.md): ahead at 8 and 16 (1.2x .. 3.1x),
// at 32 ahead for the pair operators (MPO bond 1) but behind for the bond-4 MPOs of the chain with 16 phonon levels
// (0.63x, and behind Mps.expectations too: a workgroup is one compute unit and meets 16 slices of 32 x 4 x 32 per site).
// The accumulators of the site step hold SW_PLANES x CHAIN_THREADS entries of a bond plane, so nothing above a bond of
// 45 fits whatever this says; chains between this and what fits take the kernels only under MPSE_EXPECT_CHAIN=1.
constexpr int64_t EX_BOND_MAX = 16;
static_assert(1 <= EX_BOND_MAX && EX_BOND_MAX <= CHAIN_BOND_FIT, "the limit lies inside what fits");
constexpr int64_t EX_GRID_MAX = 256;   // workgroups of one k_expect_windows launch: one per compute unit of the chip

struct ExSite : ChainSelRow {   // one row per site (56 bytes)
  // sel (of ChainSelRow): >= 0 when L of the bond RIGHT of this site is a window edge - leave it at loff
  int rsel;       // >= 0 when R of the bond LEFT of this site is a window edge - leave it at roff
  int pad;
  int64_t loff;   // working elements before L of the bond right of this site in the pooled buffer
  int64_t roff;   // working elements before R of the bond left of this site
};
static_assert(sizeof(ExSite) == 56, "descriptor rows are copied as 8-byte words");

struct ExW {   // one row per MPO site of a window (24 bytes), the windows one after the other
  const void* w;
  int wl, wr;
  int w_c;     // the tensor is complex128
  int pad;
};
static_assert(sizeof(ExW) == 24, "descriptor rows are copied as 8-byte words");

struct ExOp {   // one row per operator (32 bytes)
  int first, last;
  int woff;       // rows of the ExW table before its window
  int pad;
  int64_t loff;   // working elements before L of bond `first` in the pooled buffer
  int64_t roff;   // working elements before R of bond `last + 1`
};
static_assert(sizeof(ExOp) == 32, "descriptor rows are copied as 8-byte words");

struct ExArgs : ChainSelArgs {   // nsel, sel of the base are not used
  int nop;
  const int* first;
  const int* last;
  const void* const* W;     // the MPO sites of the windows, one window after the other
  const int* w_dtype;
  const int64_t* wdims;     // (wl, wr) per MPO site
};

struct ExPlan : ChainSelPlan {
  int64_t we_elems;   // LDS elements of E (D, w, D) with padded rows, largest over the window bonds
  int64_t wt_elems;   // LDS elements of one (sigma, a) slice of T, largest over the window sites
  int64_t w_max;      // largest MPO bond
  int64_t acc;        // accumulators per thread the widest window site needs: SW_CHANNELS * ceil(Dr Dr / threads)
};

// the windows lie inside the chain, first <= last, and the MPO bonds of each form a chain that starts and ends at 1;
// *nw: the MPO sites of all windows
bool expect_windows_ok(int nsite, int nop, const int* first, const int* last, const int64_t* wdims, int64_t* nw) {
  *nw = 0;
  if (nop < 1 || !first || !last || !wdims) return false;
  for (int m = 0; m < nop; ++m) {
    if (first[m] < 0 || last[m] >= nsite || first[m] > last[m]) return false;
    const int64_t* w = wdims + 2 * *nw;
    const int len = last[m] - first[m] + 1;
    for (int j = 0; j < len; ++j) {
      if (w[2 * j] < 1 || w[2 * j + 1] < 1) return false;
      if (j + 1 < len && w[2 * j + 1] != w[2 * j + 2]) return false;
    }
    if (w[0] != 1 || w[2 * len - 1] != 1) return false;
    *nw += len;
  }
  return true;
}

// The sizing of a table that is a chain with windows that are valid: that of the walks (chain_sel_plan), and the
// regions of k_expect_windows, E, one slice of T and a word per wave for cr_block_sum
ExPlan expect_plan(int nsite, const int64_t* dims, int nop, const int* first, const int* last, const int64_t* wdims,
                   bool cplx) {
  ExPlan pl{chain_sel_plan(nsite, dims, true, 0, cplx, EX_BOND_MAX), 0, 0, 0, 0};
  int64_t row = 0;
  for (int m = 0; m < nop; ++m)
    for (int i = first[m]; i <= last[m]; ++i, ++row) {
      const int64_t Dl = dims[4 * i], Dr = dims[4 * i + 3], wl = wdims[2 * row], wr = wdims[2 * row + 1];
      pl.w_max = std::max({pl.w_max, wl, wr});
      if (!pl.fit) continue;   // bonds above CHAIN_BOND_FIT: no sizes
      pl.we_elems = std::max({pl.we_elems, Dl * wl * chain_pitch(Dl), Dr * wr * chain_pitch(Dr)});
      pl.wt_elems = std::max(pl.wt_elems, Dl * wl * Dr);
      pl.acc = std::max(pl.acc, SW_CHANNELS * ((Dr * Dr + CHAIN_THREADS - 1) / CHAIN_THREADS));
    }
  if (pl.fit) {
    const int64_t lds_win = (pl.we_elems + pl.wt_elems + CHAIN_WAVES) * (cplx ? 16 : 8);
    pl.lds = std::max(pl.lds, lds_win);
    if (pl.lds > CHAIN_LDS_MAX || pl.w_max > SW_CHANNELS || pl.acc > SW_ACC) pl.fit = false;
  }
  if (!pl.fit) pl.lds = pl.e_elems = pl.t_elems = pl.we_elems = pl.wt_elems = 0;
  pl.chain = pl.fit && pl.max_bond <= EX_BOND_MAX;
  return pl;
}

// Launch 1.  Workgroup 0 walks right to left and leaves R of every window edge, workgroup 1 left to right and leaves L.
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_expect_envs(const ExSite* __restrict__ sites, int nsite, int first,
                                                               int last, int e_elems, void* pool) {
  walk_envs<CPLX, true>(sites, nsite, first, last, e_elems, pool);
}

// Launch 2.  Workgroup x takes operator op0 + x: L of its first bond from pooled memory into E (D rows of D | 1
// elements: the transfer tensor (D, 1, D)), the site step of k_sandwich_chain over its window with the chain as bra
// (conjugated) and ket, and the closing sum_{b, k} E[b, 0, k] R[b, k] in the fixed order of cr_block_sum.
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_expect_windows(const ExSite* __restrict__ sites,
                                                                  const ExOp* __restrict__ ops,
                                                                  const ExW* __restrict__ ws, int op0, int e_elems,
                                                                  int t_elems, const void* __restrict__ pool,
                                                                  double* __restrict__ out) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double ex_lds[];
  T* E = reinterpret_cast<T*>(ex_lds);
  T* Ts = E + e_elems;
  T* red = Ts + t_elems;
  const T* P = static_cast<const T*>(pool);
  const int tid = threadIdx.x;
  const int m = op0 + blockIdx.x;
  const ExOp op = ops[m];
  walk_env_from_pool<CPLX>(P + op.loff, sites[op.first].Dl, E);
  int Dr = 1;
  for (int i = op.first; i <= op.last; ++i) {
    const ExSite a = sites[i];
    const ExW w = ws[op.woff + (i - op.first)];
    const SwSite s{a.a, a.a, w.w, a.Dl, a.Dl, w.wl, a.d, a.danc, a.Dr, a.Dr, w.wr, a.cplx, a.cplx, w.w_c, 0};
    sw_site_step<CPLX>(s, 1, E, Ts);
    Dr = a.Dr;
  }
  const T part = walk_env_dot<CPLX>(E, Dr, P + op.roff, tid, CHAIN_THREADS);
  const T tot = cr_block_sum<CPLX>(part, red, tid);
  if (tid == 0) {
    out[2 * m] = El::re(tot);
    out[2 * m + 1] = El::im(tot);
  }
}

// Where the environments of the bonds live in the pooled buffer, for both paths: L_j at boff[j], R_j at tot + boff[j],
// every bond with room for D_j D_j working elements; which of them a window needs; the range of the walks
struct ExEdges {
  std::vector<int64_t> boff;
  int64_t tot = 0;
  std::vector<char> need_l, need_r;
  int max_l = 0, min_r = 0;   // the largest bond whose L, the smallest whose R is needed

  ExEdges(const ExArgs& a) : boff((size_t)a.nsite + 1), need_l((size_t)a.nsite + 1, 0), need_r((size_t)a.nsite + 1, 0) {
    for (int j = 0; j <= a.nsite; ++j) {
      const int64_t D = j < a.nsite ? a.dims[4 * j] : 1;
      boff[j] = tot;
      tot += D * D;
    }
    min_r = a.nsite;
    for (int m = 0; m < a.nop; ++m) {
      need_l[a.first[m]] = 1, need_r[a.last[m] + 1] = 1;
      max_l = std::max(max_l, a.first[m]);
      min_r = std::min(min_r, a.last[m] + 1);
    }
  }
};

// the sentinel L_0 = R_nsite = 1 into their places
int expect_sentinels(mpse_ctx* ctx, const ExArgs& a, const ExEdges& e, void* pool, size_t es) {
  const double one[2] = {1.0, 0.0};
  char* p = static_cast<char*>(pool);
  MPSE_TRY(stage_h2d(ctx, p + (size_t)e.boff[0] * es, one, es));
  return stage_h2d(ctx, p + (size_t)(e.tot + e.boff[a.nsite]) * es, one, es);
}

int expect_chain(mpse_ctx* ctx, const ExArgs& a, bool cplx, const ExPlan& pl, int64_t nw, double* out_host) {
  const ExEdges e(a);
  std::vector<ExSite> rows((size_t)a.nsite);
  for (int i = 0; i < a.nsite; ++i) {
    ExSite r{chain_sel_row(a, i, e.need_l[i + 1] && i + 1 < a.nsite ? 0 : -1), e.need_r[i] && i > 0 ? 0 : -1, 0,
             e.boff[i + 1], e.tot + e.boff[i]};
    rows[i] = r;
  }
  std::vector<ExW> wrows((size_t)nw);
  std::vector<ExOp> ops((size_t)a.nop);
  int64_t row = 0;
  for (int m = 0; m < a.nop; ++m) {
    ops[m] = ExOp{a.first[m], a.last[m], (int)row, 0, e.boff[a.first[m]], e.tot + e.boff[a.last[m] + 1]};
    for (int i = a.first[m]; i <= a.last[m]; ++i, ++row)
      wrows[row] = ExW{a.W[row], (int)a.wdims[2 * row], (int)a.wdims[2 * row + 1], a.w_dtype[row] == MPSE_C128, 0};
  }
  // the window kernel has no static LDS; both launches may use all of a compute unit's
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_expect_envs), CHAIN_KERNELS(k_expect_windows)}, CHAIN_LDS_MAX));
  const size_t es = cplx ? 16 : 8, n_out = 2 * (size_t)a.nop;
  TmpBuf tab(ctx), wtab(ctx), otab(ctx), pool(ctx), res(ctx);
  MPSE_TRY(chain_stage_rows(ctx, tab, rows));
  MPSE_TRY(chain_stage_rows(ctx, wtab, wrows));
  MPSE_TRY(chain_stage_rows(ctx, otab, ops));
  MPSE_TRY(pool.alloc(2 * (size_t)e.tot * es));
  MPSE_TRY(res.alloc(n_out * sizeof(double)));
  MPSE_TRY(expect_sentinels(ctx, a, e, pool.p, es));
  CHAIN_LAUNCH(ctx, cplx, k_expect_envs, 2, (pl.e_elems + pl.t_elems) * (int64_t)es, tab.as<const ExSite>(), a.nsite,
               e.min_r - 1, e.max_l - 1, (int)pl.e_elems, pool.p);
  const int64_t lds_win = (pl.we_elems + pl.wt_elems + CHAIN_WAVES) * (int64_t)es;
  for (int64_t op0 = 0; op0 < a.nop; op0 += EX_GRID_MAX)
    CHAIN_LAUNCH(ctx, cplx, k_expect_windows, std::min<int64_t>(EX_GRID_MAX, a.nop - op0), lds_win,
                 tab.as<const ExSite>(), otab.as<const ExOp>(), wtab.as<const ExW>(), (int)op0, (int)pl.we_elems,
                 (int)pl.wt_elems, (const void*)pool.p, res.as<double>());
  MPSE_HIP(ctx, hipGetLastError());
  return mpse_memcpy_d2h(ctx, out_host, res.p, n_out * sizeof(double));
}

// The environments as the products of bondspec_enqueued in one dtype (complex as soon as any site or MPO site is; real
// sites are widened into pooled copies), every bond a walk passes kept in the pooled buffer.  Then per operator the
// update of mpse_env_update (left domain, no unit channel) site after site of its window, from L (D, 1, D) of its first
// bond on two pooled environments, and res[m] = vec(E) . vec(R) of its last bond as one product.
int expect_enqueued(mpse_ctx* ctx, const ExArgs& a, bool cplx, double* out_host) {
  ChainSelEnq q(ctx, cplx);
  MPSE_TRY(q.init(a));
  const ExEdges e(a);
  const size_t es = q.es;
  int64_t e_max = 1, row = 0;
  for (int m = 0; m < a.nop; ++m)
    for (int i = a.first[m]; i <= a.last[m]; ++i, ++row)
      e_max = std::max(e_max, a.dims[4 * i + 3] * a.wdims[2 * row + 1] * a.dims[4 * i + 3]);
  TmpBuf pool(ctx), x1(ctx), e0(ctx), e1(ctx), res(ctx);
  MPSE_TRY(q.alloc({{&pool, 2 * e.tot}, {&x1, q.x_max}, {&e0, e_max}, {&e1, e_max}, {&res, a.nop}}));
  MPSE_TRY(expect_sentinels(ctx, a, e, pool.p, es));
  char* P = static_cast<char*>(pool.p);
  auto L = [&](int j) -> void* { return P + (size_t)e.boff[j] * es; };
  auto R = [&](int j) -> void* { return P + (size_t)(e.tot + e.boff[j]) * es; };
  for (int i = a.nsite - 1; i >= e.min_r; --i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], p = d[1] * d[2], Dr = d[3];
    MPSE_TRY(q.a_r(Dl * p, Dr, Dr, q.site[i], R(i + 1), x1.p));
    MPSE_TRY(q.ca_y(Dl, Dl, p * Dr, q.site[i], x1.p, R(i)));
  }
  for (int i = 0; i < e.max_l; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], p = d[1] * d[2], Dr = d[3];
    MPSE_TRY(q.l_a(1, Dl, Dl, p * Dr, L(i), q.site[i], x1.p));
    MPSE_TRY(q.ca_x(1, Dl * p, Dr, Dr, q.site[i], x1.p, L(i + 1)));
  }
  row = 0;
  for (int m = 0; m < a.nop; ++m) {
    const void* env = L(a.first[m]);
    void* nxt = e0.p;
    for (int i = a.first[m]; i <= a.last[m]; ++i, ++row) {
      const int64_t* d = a.dims + 4 * i;
      mpse_dims dm{};
      dm.Dl_bra = dm.Dl_ket = d[0], dm.Dr_bra = dm.Dr_ket = d[3];
      dm.d0 = d[1], dm.d1 = 1, dm.danc = d[2];
      dm.wl = a.wdims[2 * row], dm.wm = 1, dm.wr = a.wdims[2 * row + 1];
      dm.env_unit = 0, dm.danc1 = 0;
      MPSE_TRY(mpse_env_update(ctx, q.dt, MPSE_DOMAIN_L, &dm, env, q.dt, q.site[i], q.site[i], q.cj, a.W[row],
                               a.w_dtype[row], nxt));
      env = nxt;
      nxt = nxt == e0.p ? e1.p : e0.p;
    }
    const int64_t Dr = a.dims[4 * a.last[m] + 3], nE = Dr * Dr;
    MPSE_TRY(q.gemm(0, idx1(1, nE), idx1(nE, 1), idx1(nE, 1), idx1(1, 1), idx1(1, 1), idx1(1, 1), 1, 0, 0, 0, env,
                    R(a.last[m] + 1), static_cast<char*>(res.p) + (size_t)m * es));
  }
  return chain_read_pairs(ctx, res.p, a.nop, cplx, {{0, a.nop, 0}}, out_host);
}

}  // namespace

extern "C" {

int mpse_mps_expect_many_plan(int nsite, const int64_t* dims, int nop, const int* first, const int* last,
                              const int64_t* wdims, int any_complex, int64_t* info, int n) {
  int64_t nw = 0;
  const bool valid = chain_sel_table_ok(nsite, dims) && expect_windows_ok(nsite, nop, first, last, wdims, &nw);
  const ExPlan pl = valid ? expect_plan(nsite, dims, nop, first, last, wdims, any_complex != 0) : ExPlan{};
  return chain_sel_plan_out(pl, valid, EX_BOND_MAX, EX_GRID_MAX,
                            {pl.we_elems, pl.wt_elems, pl.w_max, SW_CHANNELS, pl.acc, SW_ACC, any_complex ? 16 : 8},
                            info, n);
}

int mpse_mps_expect_many_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::expect_stats, counts, n);
}

int mpse_mps_expect_many(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims,
                         int nop, const int* first, const int* last, const void* const* W, const int* w_dtype,
                         const int64_t* wdims, double* out_host) {
  if (!ctx) return MPSE_ERR_ARG;
  if (nsite < 1 || !sites || !dtype || !dims || nop < 1 || !first || !last || !W || !w_dtype || !wdims || !out_host)
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_expect_many: null argument, no sites or no operators");
  bool cplx = false, w_cplx = false;
  MPSE_TRY(chain_scan_sites(ctx, "mps_expect_many", nsite, {sites}, {dtype}, &cplx));
  int64_t nw = 0;
  if (!expect_windows_ok(nsite, nop, first, last, wdims, &nw))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "mps_expect_many: a window is not first <= last inside [0, %d), or its MPO bonds are no chain "
                     "from 1 to 1", nsite);
  if (nw > INT32_MAX) return mpse_fail(ctx, MPSE_ERR_SHAPE, "mps_expect_many: too many MPO sites");
  MPSE_TRY(chain_scan_sites(ctx, "mps_expect_many (MPO sites)", (int)nw, {W}, {w_dtype}, &w_cplx));
  cplx = cplx || w_cplx;
  if (!chain_sel_table_ok(nsite, dims))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "mps_expect_many: dims is not a chain (extents >= 1, matching neighbours, first and last bond 1)");
  if (MPSE_RECORDING(ctx))
    return mpse_fail(ctx, MPSE_ERR_ARG,
                     "mps_expect_many: synchronous, not available while a deferred list is recorded");
  const ExArgs args{{nsite, sites, dtype, dims, 0, nullptr}, nop, first, last, W, w_dtype, wdims};
  ExPlan pl = expect_plan(nsite, dims, nop, first, last, wdims, cplx);
  MPSE_BIND(ctx);
  chain_sel_plan_switch("MPSE_EXPECT_CHAIN", &pl);
  std::vector<double> res(2 * (size_t)nop, 0.0);
  if (pl.chain)
    MPSE_TRY(expect_chain(ctx, args, cplx, pl, nw, res.data()));
  else
    MPSE_TRY(expect_enqueued(ctx, args, cplx, res.data()));
  return chain_sel_done(ctx->expect_stats, pl.chain, nsite, nop, res, out_host);
}

}  // extern "C"
