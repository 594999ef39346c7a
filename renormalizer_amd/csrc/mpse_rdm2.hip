// mpse_mps_rdm2: the two-site reduced density matrices
//   rho_kl[(p,q),(p',q')] = sum conj(A_k)[.,p,g,.] conj(A_l)[.,q,g',.] A_k[.,p',g,.] A_l[.,q',g',.]
// of every pair k < l of selected sites of ONE chain as one engine call, identity environments outside the pair and
// identity transfer matrices in between, the ancilla legs g, g' traced (the reference pushes a running object one site
// at a time per pair and reads every pair back on its own, mps/mps.py:1600-1655 calc_2site_rdm).  It is the walk of
// mpse_mps_corr with every elementary matrix |p><p'| opened at k and every |q><q'| closed at l, sharing the walk.  Two
// paths, chosen from the dims table and the selection alone (rdm2_plan):
//   chain      two launches, for chains whose bonds are at most RD2_BOND_MAX.  k_rdm2_envs: workgroup 0 walks right to
//              left with R in LDS and leaves, at every selected site l but the first, the d_l^2 closed environments
//              G_l^{qq'}[b, c] in pooled memory; workgroup 1 walks left to right (walk_left) and leaves L_k at
//              every selected site but the last.  k_rdm2_rows: one workgroup per unit (k, p, p') starts at sel[k] from
//              L_k, opens with the slices sigma = p' and the bra rows sigma' = p, carries E to the right and closes
//              against all G_l^{qq'} at every later selected site.
//   enqueued   the same passes as products of the contraction kernel; the open rows are one stack that grows by d_k^2
//              rows per opening site and is walked in chunks under a byte bound - every other chain
// The walk, the sizing, the entry checks and the plain products of the enqueued passes are those of mpse_chain_walk.h,
// which also says what holds for all three calls: launch order instead of flags, one host read, a fixed summation order.
#include "mpse_chain_walk.h"

namespace {

// Largest bond up to which the kernels take a call that fits: measured with tools/rdm2_bench.py, profiles/rdm2.md.  On
// the band-limit chain (d = 2 / 4) the two launches are ahead of the enqueued products at 8, 16 and 32; on the Holstein
// chain with 16 phonon levels (256 units and 16 slices per phonon site, each unit one workgroup on one compute unit)
// they are behind at 16, 32 and 64.  8 is the largest bond of the measurement plan at which they won on every chain
// measured there; an extra row, that Holstein chain at 8, has them behind as well (profiles/rdm2.md names it).  Chains
// between this and CHAIN_BOND_FIT take the kernels only under MPSE_RDM2_CHAIN=1.
constexpr int64_t RD2_BOND_MAX = 8;
static_assert(1 <= RD2_BOND_MAX && RD2_BOND_MAX <= CHAIN_BOND_FIT, "the limit of the rule lies inside what fits");
// Device offsets into the pooled environments and into the result are 32-bit inside the kernels
constexpr int64_t RD2_ELEMS_MAX = int64_t(1) << 31;
// Byte bound of one chunk of the enqueued path: its two stacks of open rows plus X1.  A memory choice, not a
// measurement: a quarter of a GiB next to the pooled G_l of the call.  MPSE_RDM2_STACK_BYTES in the environment
// overrides it, read per call (for tests and measurements).
constexpr int64_t RD2_STACK_BYTES_MAX = int64_t(256) << 20;
// what the host can hold of a result at all; a larger request is MPSE_ERR_OOM before any device work
constexpr int64_t RD2_OUT_ELEMS_CAP = int64_t(1) << 40;

struct Rd2Site : ChainSelRow {   // one row of the descriptor table (56 bytes)
  int64_t eoff;   // working elements before L of this site in the pooled buffer (selected sites but the last)
  int64_t goff;   // working elements before G^{qq'} of this site in the pooled buffer: d d matrices [b][c], (q, q') major
  int64_t csum;   // sum of d^2 over the selected sites before this one
};
static_assert(sizeof(Rd2Site) == 56, "descriptor rows are copied as 8-byte words");

struct Rd2Unit {   // one workgroup of k_rdm2_rows (32 bytes); the table follows the site rows
  int site;        // the opening site sel[k]
  int p, pp;       // the row |p><p'|: bra index p, ket index p'
  int row;         // p d_k + p'
  int64_t dk2;     // d_k^2
  int64_t obase;   // complex elements before the block of pair (k, l) in the result, less dk2 * csum of site sel[l]
};
static_assert(sizeof(Rd2Unit) == 32, "unit rows are copied as 8-byte words");

struct Rd2Plan : ChainSelPlan {
  int64_t units;         // workgroups of k_rdm2_rows: sum of d_k^2 over the selected sites but the last
  int64_t out_elems;     // complex elements of the result: sum over k < l of d_k^2 d_l^2 (saturates at INT64_MAX)
  int64_t pool_elems;    // working elements of the pooled L_k and G_l
};

int64_t sat_add(int64_t a, int64_t b) { return a > INT64_MAX - b ? INT64_MAX : a + b; }
int64_t sat_mul(int64_t a, int64_t b) { return a != 0 && b > INT64_MAX / a ? INT64_MAX : a * b; }

// the sizing of a table that is a chain with a selection that is one: at least a pair, the pooled environments and the
// result inside the 32-bit offsets of the kernels
Rd2Plan rdm2_plan(int nsite, const int64_t* dims, int nsel, const int* sel, bool cplx) {
  Rd2Plan pl{};
  int64_t before = 0;   // sum of d^2 over the selected sites walked so far
  for (int k = 0; k < nsel; ++k) {
    const int64_t* d = dims + 4 * sel[k];
    const int64_t dd = sat_mul(d[1], d[1]), bb = sat_mul(d[0], d[0]);
    pl.out_elems = sat_add(pl.out_elems, sat_mul(before, dd));
    before = sat_add(before, dd);
    if (k < nsel - 1) {
      pl.units = sat_add(pl.units, dd);
      pl.pool_elems = sat_add(pl.pool_elems, bb);
    }
    if (k > 0) pl.pool_elems = sat_add(pl.pool_elems, sat_mul(dd, bb));
  }
  const bool allowed = nsel >= 2 && pl.pool_elems < RD2_ELEMS_MAX && pl.out_elems < RD2_ELEMS_MAX;
  static_cast<ChainSelPlan&>(pl) = chain_sel_plan(nsite, dims, allowed, 0, cplx, RD2_BOND_MAX);
  return pl;
}

// Workgroup 0 of k_rdm2_envs.  R_N = 1.  Per site from the right down to `stop`, the second selected site, per (q', g)
// in ascending order the transfer to the right (walk_right_slice, walk_right_dot):
//   T[c, b'] = sum_c' A[c, q', g, c'] R[b', c']                                             (into LDS)
//   S_q[b, c] = sum_b' conj(A[b, q, g, b']) T[c, b']
//   R'[b, c] += S_q'[b, c]                                                                  (registers of the owner)
// and at a selected site, for every q, G^{qq'}[b, c] (+)= S_q[b, c] in pooled memory: one slice T yields G^{qq'} for
// every q; with an ancilla leg the owner of (b, c) adds the values of g = 1, 2, .. in ascending order to its own word
// (nobody else touches it: no atomic).  R' replaces R in LDS after the last (q', g).
template <bool CPLX>
__device__ void rd2_walk_right(const Rd2Site* __restrict__ sites, int nsite, int stop, ChainT<CPLX>* R,
                               ChainT<CPLX>* Ts, ChainT<CPLX>* pool) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int tid = threadIdx.x;
  walk_env_one<CPLX>(R);
  for (int i = nsite - 1; i >= stop; --i) {
    const Rd2Site s = sites[i];
    const int d = s.d, danc = s.danc, Dr = s.Dr;
    const int p = d * danc, row = p * Dr, nE = s.Dl * s.Dl;
    const bool closes = s.sel >= 0;         // every selected site this walk reaches is a closing one
    T* G = pool + s.goff;
    T acc[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc);
    for (int sa = 0; sa < p; ++sa) {
      const int qp = sa / danc, g = sa - qp * danc;
      walk_right_slice<CPLX>(s, row, sa * Dr, R, Ts);
#pragma unroll
      for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          const int b = o / s.Dl, c = o - b * s.Dl;
          const T* t_row = Ts + c * (Dr | 1);
          for (int q = closes ? 0 : qp; q < (closes ? d : qp + 1); ++q) {
            T S;
            walk_right_dot<CPLX>(s, b * row + (q * danc + g) * Dr, t_row, S);
            if (q == qp) El::add(acc[j], S);
            if (closes) {
              T* w = G + (q * d + qp) * nE + o;
              if (g) El::add(S, *w);
              *w = S;
            }
          }
        }
      }
      __syncthreads();   // T is overwritten by the next (q', g); after the last one every read of R is done as well
    }
    if (i == stop) break;
    walk_acc_store<CPLX>(acc, s.Dl, s.Dl, R);
  }
}

template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_rdm2_envs(const Rd2Site* __restrict__ sites, int nsite, int stop,
                                                             int last, int e_elems, void* pool) {
  using T = ChainT<CPLX>;
  extern __shared__ __attribute__((aligned(16))) double rd2_lds[];
  T* E = reinterpret_cast<T*>(rd2_lds);
  T* Ts = E + e_elems;
  if (blockIdx.x == 0)
    rd2_walk_right<CPLX>(sites, nsite, stop, E, Ts, static_cast<T*>(pool));
  else
    walk_left<CPLX, false>(sites, last, E, Ts, static_cast<T*>(pool));
}

// Workgroup u: the row |p><p'| opened at site sel[k] = units[u].site.  E = L_k from the pooled buffer, then from that
// site to the last selected one.  At a later selected site l first the closing against all d_l^2 environments,
//   out[k, l][p][p'][q][q'] = sum_{b, c} E[b, c] G_l^{qq'}[b, c]:
// wave w takes the entries (q, q') = w, w + 16, .., its lanes stride over (b, c) in ascending order and are summed with
// shuffles - no barrier per entry.  Then (not behind the last selected site) the transfer to the left, per slice in
// ascending order: T = E . A[sigma, g] into LDS (walk_left_slice), E' += S of the bra slice (sigma', g) (walk_acc_add),
// with (sigma', sigma) = (p, p') for every g at the opening site and sigma' = sigma over all (sigma, g) elsewhere.
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_rdm2_rows(const Rd2Site* __restrict__ sites,
                                                             const Rd2Unit* __restrict__ units, int last, int e_elems,
                                                             const void* __restrict__ pool, double* __restrict__ out) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double rd2_lds[];
  T* E = reinterpret_cast<T*>(rd2_lds);
  T* Ts = E + e_elems;
  const T* P = static_cast<const T*>(pool);
  const Rd2Unit u = units[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = u.site; i <= last; ++i) {
    const Rd2Site s = sites[i];
    const int Dl = s.Dl, d = s.d, danc = s.danc, Dr = s.Dr;
    const int p = d * danc, row = p * Dr;
    const int nE = Dr * Dr, nL = Dl * Dl;
    const bool open = i == u.site;
    if (open) {
      walk_env_from_pool<CPLX>(P + s.eoff, Dl, E);
    } else if (s.sel >= 0) {
      const T* G = P + s.goff;
      const int dl2 = d * d;
      double* dst = out + 2 * (u.obase + u.dk2 * s.csum + (int64_t)u.row * dl2);
      for (int qq = wave; qq < dl2; qq += CHAIN_WAVES) {
        const T part = walk_wave_sum<CPLX>(walk_env_dot<CPLX>(E, Dl, G + qq * nL, lane, 64));
        if (lane == 0) {
          dst[2 * qq] = El::re(part);
          dst[2 * qq + 1] = El::im(part);
        }
      }
      if (i == last) break;
    }
    T acc[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc);
    const int nslice = open ? danc : p;
    for (int t = 0; t < nslice; ++t) {
      const int ket = (open ? u.pp * danc + t : t) * Dr, bra = (open ? u.p * danc + t : t) * Dr;
      walk_left_slice<CPLX>(s, row, ket, E, Dl | 1, Ts, Dr);
      walk_acc_add<CPLX, true>(s, row, bra, Ts, nE, acc);
      __syncthreads();   // T is overwritten by the next slice; after the last one every read of E is done as well
    }
    walk_acc_store<CPLX>(acc, Dr, Dr, E);
  }
}

// d^2 of selected site k
int64_t rd2_dd(const ChainSelArgs& a, int k) { return a.dims[4 * a.sel[k] + 1] * a.dims[4 * a.sel[k] + 1]; }

// complex elements before the block of pair (k, l) for every k, l = k + 1: the pairs of one k follow each other with
// ascending l, so the block of (k, l) starts at obase[k] + d_k^2 * (csum[l] - csum[k + 1]), csum[m] the sum of d^2 over
// the selected sites before m
void rd2_offsets(const ChainSelArgs& a, std::vector<int64_t>* csum, std::vector<int64_t>* obase) {
  csum->assign((size_t)a.nsel + 1, 0);
  obase->assign((size_t)a.nsel, 0);
  for (int k = 0; k < a.nsel; ++k) (*csum)[k + 1] = (*csum)[k] + rd2_dd(a, k);
  for (int k = 0; k + 1 < a.nsel; ++k)
    (*obase)[k + 1] = (*obase)[k] + rd2_dd(a, k) * ((*csum)[a.nsel] - (*csum)[k + 1]);
}

int rdm2_chain(mpse_ctx* ctx, const ChainSelArgs& a, bool cplx, const Rd2Plan& pl, double* out_host) {
  std::vector<int64_t> csum, obase;
  rd2_offsets(a, &csum, &obase);
  static_assert(sizeof(Rd2Site) % 8 == 0 && sizeof(Rd2Unit) % 8 == 0, "one table of 8-byte words");
  const size_t site_words = sizeof(Rd2Site) / 8, unit_words = sizeof(Rd2Unit) / 8;
  std::vector<uint64_t> table((size_t)a.nsite * site_words + (size_t)pl.units * unit_words);
  Rd2Site* rows = reinterpret_cast<Rd2Site*>(table.data());
  Rd2Unit* units = reinterpret_cast<Rd2Unit*>(table.data() + (size_t)a.nsite * site_words);
  int64_t pool_elems = 0, nunit = 0;
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const bool is_sel = k < a.nsel && a.sel[k] == i;
    rows[i] = Rd2Site{chain_sel_row(a, i, is_sel ? k : -1), 0, 0, is_sel ? csum[k] : 0};
    if (!is_sel) continue;
    if (k < a.nsel - 1) {
      rows[i].eoff = pool_elems;
      pool_elems += d[0] * d[0];
      for (int p = 0; p < (int)d[1]; ++p)
        for (int pp = 0; pp < (int)d[1]; ++pp)
          units[nunit++] = Rd2Unit{i, p, pp, p * (int)d[1] + pp, d[1] * d[1], obase[k] - d[1] * d[1] * csum[k + 1]};
    }
    if (k > 0) {
      rows[i].goff = pool_elems;
      pool_elems += d[1] * d[1] * d[0] * d[0];
    }
    ++k;
  }
  if (nunit != pl.units || pool_elems != pl.pool_elems)
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_rdm2: the tables disagree with the plan");
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_rdm2_envs), CHAIN_KERNELS(k_rdm2_rows)}, CHAIN_LDS_MAX));
  const size_t es = cplx ? 16 : 8, n_out = (size_t)pl.out_elems * 2;
  TmpBuf tab(ctx), pool(ctx), res(ctx);
  MPSE_TRY(chain_stage_rows(ctx, tab, table));
  MPSE_TRY(pool.alloc((size_t)pool_elems * es));
  MPSE_TRY(res.alloc(n_out * sizeof(double)));
  const Rd2Site* drows = tab.as<const Rd2Site>();
  const Rd2Unit* dunits = reinterpret_cast<const Rd2Unit*>(tab.as<const uint64_t>() + (size_t)a.nsite * site_words);
  CHAIN_LAUNCH(ctx, cplx, k_rdm2_envs, 2, pl.lds, drows, a.nsite, a.sel[1], a.sel[a.nsel - 2], (int)pl.e_elems, pool.p);
  CHAIN_LAUNCH(ctx, cplx, k_rdm2_rows, pl.units, pl.lds, drows, dunits, a.sel[a.nsel - 1], (int)pl.e_elems,
               (const void*)pool.p, res.as<double>());
  MPSE_HIP(ctx, hipGetLastError());
  return mpse_memcpy_d2h(ctx, out_host, res.p, n_out * sizeof(double));
}

// the byte bound of a chunk: RD2_STACK_BYTES_MAX, or MPSE_RDM2_STACK_BYTES from the environment when it is a positive
// number
int64_t rd2_stack_bytes() {
  const char* env = getenv("MPSE_RDM2_STACK_BYTES");
  const long long v = env ? strtoll(env, nullptr, 10) : 0;
  return v > 0 ? (int64_t)v : RD2_STACK_BYTES_MAX;
}

// The same contractions as products of the contraction kernel, in one dtype: complex as soon as any site is (real sites
// are widened into pooled copies first).  The plain products: ChainSelEnq of mpse_chain_walk.h.
//   right pass, site i from the last one down to sel[1], R (D_r, D_r) = [b', c']:  Y1 = A . R,  R' = conj(A) . Y1
//     selected:  G_i[(b, c), (q, q')] = sum_(g, b') conj(A[b, q, (g, b')]) Y1[c, q', (g, b')]      (one product)
//   left pass, site i from 0 to sel[nsel - 2] - 1, L (D_l, D_l) = [b, c]:  X1 = L . A,  L' = conj(A) . X1; L of a
//   selected site is written straight into its place in the pooled buffer, the others alternate between two buffers
//   open rows, a stack S[r][b][c] walked from the first opening site of a CHUNK to the last selected site:
//     selected site l with open rows:  C[r, (q, q')] = sum_(b, c) S[r, (b, c)] G_l[(b, c), (q, q')]   (one product)
//     X1 = S . A, one product for the whole stack (l_a);  S' = conj(A) . X1, batched over r (ca_x)
//     opening site k of the chunk:  XL = L_k . A as X1 above, and d_k^2 new rows
//       S'[(p, p')][b', c'] = sum_(a, g) conj(A[a, p, g, b']) XL[a, p', g, c']                        (one product)
// A chunk is a run of whole opening sites whose rows keep the two stacks plus X1 inside rd2_stack_bytes(); one opening
// site that alone exceeds the bound is split by rows (then one product per p of the range).  C of one closing is
// contiguous on the device, rows in stack order; the one host read at the end copies every (k, l) run of rows to its
// place in the pair blocks, with 64-bit offsets.
int rdm2_enqueued(mpse_ctx* ctx, const ChainSelArgs& a, bool cplx, int64_t out_elems, double* out_host) {
  ChainSelEnq q(ctx, cplx);
  MPSE_TRY(q.init(a));
  const size_t es = q.es;
  const int nsel = a.nsel, last = a.sel[nsel - 1];
  std::vector<int64_t> csum, obase;
  rd2_offsets(a, &csum, &obase);
  int64_t l_elems = 0, g_elems = 0;
  std::vector<int64_t> loff((size_t)nsel, 0), goff((size_t)nsel, 0);
  for (int k = 0; k < nsel; ++k) {
    const int64_t* d = a.dims + 4 * a.sel[k];
    if (k < nsel - 1) loff[k] = l_elems, l_elems += d[0] * d[0];
    if (k > 0) goff[k] = g_elems, g_elems += d[0] * d[0] * d[1] * d[1];
  }
  // ---- the chunks: opening sites [k0, k1], rows [r0, r1) of every one of them (a part only when k0 == k1)
  struct Chunk {
    int k0, k1;
    int64_t r0, r1;
  };
  const int64_t row_bytes = (2 * q.e_max + q.x_max) * (int64_t)es;
  const int64_t rows_max = std::max<int64_t>(1, rd2_stack_bytes() / row_bytes);
  std::vector<Chunk> chunks;
  int64_t rows_cap = 1;
  for (int k = 0; k < nsel - 1;) {
    const int64_t dd = rd2_dd(a, k);
    if (dd > rows_max) {
      for (int64_t r = 0; r < dd; r += rows_max) chunks.push_back(Chunk{k, k, r, std::min(dd, r + rows_max)});
      rows_cap = std::max(rows_cap, rows_max);
      ++k;
      continue;
    }
    int k1 = k;
    int64_t rows = dd;
    while (k1 + 1 < nsel - 1 && rows + rd2_dd(a, k1 + 1) <= rows_max) rows += rd2_dd(a, ++k1);
    chunks.push_back(Chunk{k, k1, 0, 0});
    rows_cap = std::max(rows_cap, rows);
    k = k1 + 1;
  }
  TmpBuf lbuf(ctx), gbuf(ctx), res(ctx), e0(ctx), e1(ctx), xl(ctx), s0(ctx), s1(ctx), x1(ctx);
  MPSE_TRY(q.alloc({{&lbuf, l_elems}, {&gbuf, g_elems}, {&res, out_elems}, {&e0, q.e_max}, {&e1, q.e_max},
                    {&xl, q.x_max}, {&s0, rows_cap * q.e_max}, {&s1, rows_cap * q.e_max}, {&x1, rows_cap * q.x_max}}));
  const double one[2] = {1.0, 0.0};
  void* scratch[2] = {e0.p, e1.p};
  char* G = static_cast<char*>(gbuf.p);
  // ---- right pass
  {
    void* R = scratch[0];
    void* Rn = scratch[1];
    MPSE_TRY(stage_h2d(ctx, R, one, es));
    for (int i = a.nsite - 1; i >= a.sel[1]; --i) {
      const int64_t* d = a.dims + 4 * i;
      const int64_t Dl = d[0], dd = d[1], da = d[2], Dr = d[3], p = dd * da;
      MPSE_TRY(q.a_r(Dl * p, Dr, Dr, q.site[i], R, xl.p));
      if (q.pos[i] >= 0)
        MPSE_TRY(q.gemm(1, idx1(Dl * dd, da * Dr), idx1(da * Dr, 1), idx1(da * Dr, 1), idx1(Dl * dd, da * Dr),
                        idx2(Dl, dd, Dl * dd * dd, dd), idx2(Dl, dd, dd * dd, 1), 1, 0, 0, 0, q.site[i], xl.p,
                        G + (size_t)goff[q.pos[i]] * es));
      if (i == a.sel[1]) break;
      MPSE_TRY(q.ca_y(Dl, Dl, p * Dr, q.site[i], xl.p, Rn));
      std::swap(R, Rn);
    }
  }
  // ---- left pass; where L_i (the environment left of site i) lives
  auto l_at = [&](int i) -> void* {
    const int k = q.pos[i];
    return k >= 0 && k < nsel - 1 ? static_cast<char*>(lbuf.p) + (size_t)loff[k] * es : scratch[i & 1];
  };
  MPSE_TRY(stage_h2d(ctx, l_at(0), one, es));
  for (int i = 0; i < a.sel[nsel - 2]; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], p = d[1] * d[2], Dr = d[3];
    MPSE_TRY(q.l_a(1, Dl, Dl, p * Dr, l_at(i), q.site[i], xl.p));
    MPSE_TRY(q.ca_x(1, Dl * p, Dr, Dr, q.site[i], xl.p, l_at(i + 1)));
  }
  // ---- open rows, chunk by chunk
  struct Run {   // rows [r0, r0 + n) of the opening site sel[k] lie behind `before` rows of the stack
    int64_t before, r0, n;
    int k;
  };
  std::vector<ChainRun> runs;   // a run of a closing, where it lies in res and where in the pair blocks
  int64_t filled = 0;
  for (const Chunk& ch : chunks) {
    char* S = static_cast<char*>(s0.p);
    char* Sn = static_cast<char*>(s1.p);
    int64_t nrow = 0;
    std::vector<Run> open_runs;
    for (int i = a.sel[ch.k0]; i <= last; ++i) {
      const int64_t* d = a.dims + 4 * i;
      const int64_t Dl = d[0], dd = d[1], da = d[2], Dr = d[3], p = dd * da;
      const int k = q.pos[i];
      if (k >= 0 && nrow > 0) {
        MPSE_TRY(q.gemm(0, idx1(nrow, Dl * Dl), idx1(Dl * Dl, 1), idx1(Dl * Dl, dd * dd), idx1(dd * dd, 1),
                        idx1(nrow, dd * dd), idx1(dd * dd, 1), 1, 0, 0, 0, S, G + (size_t)goff[k] * es,
                        static_cast<char*>(res.p) + (size_t)filled * es));
        for (const Run& r : open_runs)
          runs.push_back({filled + r.before * dd * dd, r.n * dd * dd,
                          obase[r.k] + rd2_dd(a, r.k) * (csum[k] - csum[r.k + 1]) + r.r0 * dd * dd});
        filled += nrow * dd * dd;
      }
      if (i == last) break;
      if (nrow > 0) {
        MPSE_TRY(q.l_a(nrow, Dl, Dl, p * Dr, S, q.site[i], x1.p));
        MPSE_TRY(q.ca_x(nrow, Dl * p, Dr, Dr, q.site[i], x1.p, Sn));
      }
      if (k >= ch.k0 && k <= ch.k1) {
        const bool part = ch.r1 > ch.r0;
        const int64_t ra = part ? ch.r0 : 0, rb = part ? ch.r1 : dd * dd;
        char* dest = Sn + (size_t)(nrow * Dr * Dr) * es;
        MPSE_TRY(q.l_a(1, Dl, Dl, p * Dr, l_at(i), q.site[i], xl.p));
        // the rows (p, p') of [ra, rb): for every p its range [lo, hi) of p'; M = (p, b'), K = (a, g), N = (p', c')
        for (int64_t pr = ra / dd; pr * dd < rb; ++pr) {
          int64_t np = 1, lo = std::max(ra, pr * dd) - pr * dd, hi = std::min(rb, (pr + 1) * dd) - pr * dd;
          if (!part) np = dd, lo = 0, hi = dd;   // the whole site in one product
          const char* Ap = static_cast<const char*>(q.site[i]) + (size_t)(pr * da * Dr) * es;
          const char* Bp = static_cast<const char*>(xl.p) + (size_t)(lo * da * Dr) * es;
          MPSE_TRY(q.gemm(1, idx2(np, Dr, da * Dr, 1), idx2(Dl, da, p * Dr, Dr), idx2(Dl, da, p * Dr, Dr),
                          idx2(hi - lo, Dr, da * Dr, 1), idx2(np, Dr, dd * Dr * Dr, Dr), idx2(hi - lo, Dr, Dr * Dr, 1),
                          1, 0, 0, 0, Ap, Bp, dest + (size_t)((pr * dd + lo - ra) * Dr * Dr) * es));
          if (!part) break;
        }
        open_runs.push_back(Run{nrow, ra, rb - ra, k});
        nrow += rb - ra;
      }
      std::swap(S, Sn);
    }
  }
  if (filled != out_elems) return mpse_fail(ctx, MPSE_ERR_ARG, "mps_rdm2: the chunks do not cover the result");
  return chain_read_pairs(ctx, res.p, out_elems, cplx, runs, out_host);
}

}  // namespace

extern "C" {

int mpse_mps_rdm2_plan(int nsite, const int64_t* dims, int nsel, const int* sel, int any_complex, int64_t* info, int n) {
  const bool valid = chain_sel_table_ok(nsite, dims);
  Rd2Plan pl{};
  if (valid && chain_sel_ok(nsite, nsel, sel))
    pl = rdm2_plan(nsite, dims, nsel, sel, any_complex != 0);
  else if (valid)
    pl.max_bond = chain_sel_plan(nsite, dims, false, 0, false, RD2_BOND_MAX).max_bond;
  return chain_sel_plan_out(pl, valid, RD2_BOND_MAX, 0, {pl.units, pl.out_elems, RD2_STACK_BYTES_MAX}, info, n);
}

int mpse_mps_rdm2_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::rdm2_stats, counts, n);
}

int mpse_mps_rdm2(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims, int nsel,
                  const int* sel, double* out_host) {
  const ChainSelArgs args{nsite, sites, dtype, dims, nsel, sel};
  bool cplx = false;
  MPSE_TRY(chain_sel_prologue(ctx, "mps_rdm2", args, 2, out_host != nullptr, &cplx));
  Rd2Plan pl = rdm2_plan(nsite, dims, nsel, sel, cplx);
  if (pl.out_elems > RD2_OUT_ELEMS_CAP)
    return mpse_fail(ctx, MPSE_ERR_OOM, "mps_rdm2: a result of %lld complex elements", (long long)pl.out_elems);
  MPSE_BIND(ctx);
  chain_sel_plan_switch("MPSE_RDM2_CHAIN", &pl);
  std::vector<double> res((size_t)pl.out_elems * 2, 0.0);
  if (pl.chain)
    MPSE_TRY(rdm2_chain(ctx, args, cplx, pl, res.data()));
  else
    MPSE_TRY(rdm2_enqueued(ctx, args, cplx, pl.out_elems, res.data()));
  return chain_sel_done(ctx->rdm2_stats, pl.chain, nsite, (long long)nsel * (nsel - 1) / 2, res, out_host);
}

}  // extern "C"
