// mpse_mps_rdm2: the two-site reduced density matrices
//   rho_kl[(p,q),(p',q')] = sum conj(A_k)[.,p,g,.] conj(A_l)[.,q,g',.] A_k[.,p',g,.] A_l[.,q',g',.]
// of every pair k < l of selected sites of ONE chain as one engine call, identity environments outside the pair and
// identity transfer matrices in between, the ancilla legs g, g' traced (the reference pushes a running object one site
// at a time per pair and reads every pair back on its own, mps/mps.py:1600-1655 calc_2site_rdm).  It is the walk of
// mpse_mps_corr with every elementary matrix |p><p'| opened at k and every |q><q'| closed at l, sharing the walk.  Two
// paths, chosen from the dims table and the selection alone (rdm2_plan):
//   chain      two launches, for chains whose bonds are at most RD2_BOND_MAX.  k_rdm2_envs: workgroup 0 walks right to
//              left with R in LDS and leaves, at every selected site l but the first, the d_l^2 closed environments
//              G_l^{qq'}[b, c] in pooled memory; workgroup 1 walks left to right (chain_walk_left) and leaves L_k at
//              every selected site but the last.  k_rdm2_rows: one workgroup per unit (k, p, p') starts at sel[k] from
//              L_k, opens with the slices sigma = p' and the bra rows sigma' = p, carries E to the right and closes
//              against all G_l^{qq'} at every later selected site.  A workgroup reads only what the launch before it
//              wrote: no flag, no spin wait, no atomic.
//   enqueued   the same passes as products of the contraction kernel; the open rows are one stack that grows by d_k^2
//              rows per opening site and is walked in chunks under a byte bound - every other chain
// LDS plan of either launch as for mpse_mps_rdm1: region E (max D * pitch(D)) plus region T (max D_l * pitch(D_r)).
// The host reads once, at the end.  A fixed summation order: the same inputs give the same bits.
#include "mpse_chain.h"

namespace {

constexpr int RD2_WAVES = CHAIN_THREADS / 64;
constexpr int RD2_OUT_PER_THREAD = 4;     // entries of a new environment a thread accumulates in registers (CR_OUT_PER_THREAD)
constexpr int64_t rd2_lds_bytes(int64_t D, int64_t es) { return 2 * D * chain_pitch(D) * es; }
constexpr int64_t rd2_bond_limit() {
  // the largest power-of-two bond D whose complex regions E and T (both D rows, padded) fit, and whose environment has
  // one entry per accumulator of the workgroup
  int64_t D = 1;
  while (rd2_lds_bytes(2 * D, 16) <= CHAIN_LDS_MAX && 4 * D * D <= int64_t(CHAIN_THREADS) * RD2_OUT_PER_THREAD) D *= 2;
  return D;
}
constexpr int64_t RD2_BOND_FIT = rd2_bond_limit();
static_assert(RD2_BOND_FIT == 64, "2 x 64 x 65 complex128 = 130 KB of 160 KB; 128 would need 516 KB");
// Largest bond up to which the kernels take a call that fits: measured with tools/rdm2_bench.py, profiles/rdm2.md.  On
// the band-limit chain (d = 2 / 4) the two launches are ahead of the enqueued products at 8, 16 and 32; on the Holstein
// chain with 16 phonon levels (256 units and 16 slices per phonon site, each unit one workgroup on one compute unit)
// they are behind at 16, 32 and 64.  8 is the largest bond of the measurement plan at which they won on every chain
// measured there; an extra row, that Holstein chain at 8, has them behind as well (profiles/rdm2.md names it).  Chains
// between this and RD2_BOND_FIT take the kernels only under MPSE_RDM2_CHAIN=1.
constexpr int64_t RD2_BOND_MAX = 8;
static_assert(1 <= RD2_BOND_MAX && RD2_BOND_MAX <= RD2_BOND_FIT, "the limit of the rule lies inside what fits");
// Device offsets into the pooled environments and into the result are 32-bit inside the kernels
constexpr int64_t RD2_ELEMS_MAX = int64_t(1) << 31;
// Byte bound of one chunk of the enqueued path: its two stacks of open rows plus X1.  A memory choice, not a
// measurement: a quarter of a GiB next to the pooled G_l of the call.  MPSE_RDM2_STACK_BYTES in the environment
// overrides it, read per call (for tests and measurements).
constexpr int64_t RD2_STACK_BYTES_MAX = int64_t(256) << 20;
// what the host can hold of a result at all; a larger request is MPSE_ERR_OOM before any device work
constexpr int64_t RD2_OUT_ELEMS_CAP = int64_t(1) << 40;

struct Rd2Site {   // one row of the descriptor table (56 bytes)
  const void* a;
  int Dl, d, danc, Dr;
  int cplx;       // the tensor is complex128
  int sel;        // position in the selection, -1: not selected
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

struct Rd2Plan {
  bool chain;            // the chain kernels take it
  bool fit;              // they could: LDS and offsets allow the launches, whatever the bond limit of the rule says
  int64_t max_bond;
  int64_t e_elems;       // LDS elements of region E
  int64_t t_elems;       // LDS elements of region T
  int64_t lds;           // bytes of either launch, working dtype
  int64_t units;         // workgroups of k_rdm2_rows: sum of d_k^2 over the selected sites but the last
  int64_t out_elems;     // complex elements of the result: sum over k < l of d_k^2 d_l^2 (saturates at INT64_MAX)
  int64_t pool_elems;    // working elements of the pooled L_k and G_l
};

bool rdm2_table_ok(int nsite, const int64_t* dims) { return chain_table_ok(nsite, dims, 4, {0}, {3}); }
bool rdm2_sel_ok(int nsite, int nsel, const int* sel) {
  if (nsel < 1 || !sel) return false;
  for (int k = 0; k < nsel; ++k)
    if (sel[k] < 0 || sel[k] >= nsite || (k > 0 && sel[k] <= sel[k - 1])) return false;
  return true;
}

int64_t sat_add(int64_t a, int64_t b) { return a > INT64_MAX - b ? INT64_MAX : a + b; }
int64_t sat_mul(int64_t a, int64_t b) { return a != 0 && b > INT64_MAX / a ? INT64_MAX : a * b; }

// the sizing of a table that is a chain with a selection that is one
Rd2Plan rdm2_plan(int nsite, const int64_t* dims, int nsel, const int* sel, bool cplx) {
  Rd2Plan pl{false, false, 0, 0, 0, 0, 0, 0, 0};
  bool fits = true;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + 4 * i;
    for (int j : {0, 3}) pl.max_bond = d[j] > pl.max_bond ? d[j] : pl.max_bond;
    if (pl.max_bond > RD2_BOND_FIT || d[1] > CHAIN_EXT_MAX || d[2] > CHAIN_EXT_MAX || d[1] * d[2] > CHAIN_EXT_MAX) {
      fits = false;
      continue;
    }
    const int64_t e_l = d[0] * chain_pitch(d[0]), e_r = d[3] * chain_pitch(d[3]), t = d[0] * chain_pitch(d[3]);
    pl.e_elems = e_l > pl.e_elems ? e_l : pl.e_elems;
    pl.e_elems = e_r > pl.e_elems ? e_r : pl.e_elems;
    pl.t_elems = t > pl.t_elems ? t : pl.t_elems;
  }
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
  if (!fits || nsel < 2 || pl.pool_elems >= RD2_ELEMS_MAX || pl.out_elems >= RD2_ELEMS_MAX) {
    pl.e_elems = pl.t_elems = 0;
    return pl;
  }
  pl.lds = (pl.e_elems + pl.t_elems) * (cplx ? 16 : 8);
  pl.fit = pl.lds <= CHAIN_LDS_MAX;
  if (!pl.fit) pl.lds = pl.e_elems = pl.t_elems = 0;
  pl.chain = pl.fit && pl.max_bond <= RD2_BOND_MAX;
  return pl;
}

// Workgroup 0 of k_rdm2_envs.  R_N = 1.  Per site from the right down to `stop`, the second selected site, per (q', g)
// in ascending order:
//   T[c, b'] = sum_c' A[c, q', g, c'] R[b', c']                                             (into LDS)
//   S_q[b, c] = sum_b' conj(A[b, q, g, b']) T[c, b']
//   R'[b, c] += S_q'[b, c]                                                                  (registers of the owner)
// and at a selected site, for every q, G^{qq'}[b, c] (+)= S_q[b, c] in pooled memory: one slice T yields G^{qq'} for
// every q; with an ancilla leg the owner of (b, c) adds the values of g = 1, 2, .. in ascending order to its own word
// (nobody else touches it: no atomic).  R' replaces R in LDS after the last (q', g).  A thread owns the entries (b, c)
// = tid + j * CHAIN_THREADS, c fastest: A[b, ..] is one address per b group, the reads of T run down a column of padded
// rows.
template <bool CPLX>
__device__ void rd2_walk_right(const Rd2Site* __restrict__ sites, int nsite, int stop, typename ChainEl<CPLX>::T* R,
                               typename ChainEl<CPLX>::T* Ts, typename ChainEl<CPLX>::T* pool) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int tid = threadIdx.x;
  if (tid == 0) R[0] = El::one();
  __syncthreads();
  for (int i = nsite - 1; i >= stop; --i) {
    const Rd2Site s = sites[i];
    const int Dl = s.Dl, d = s.d, danc = s.danc, Dr = s.Dr;
    const int p = d * danc, row = p * Dr;   // element stride of the left bond
    const int pr = Dr | 1, pn = Dl | 1;
    const int nT = Dl * Dr, nE = Dl * Dl;
    const bool closes = s.sel >= 0;         // every selected site this walk reaches is a closing one
    T* G = pool + s.goff;
    T acc[RD2_OUT_PER_THREAD];
#pragma unroll
    for (int j = 0; j < RD2_OUT_PER_THREAD; ++j) acc[j] = El::zero();
    for (int sa = 0; sa < p; ++sa) {
      const int qp = sa / danc, g = sa - qp * danc;
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
      for (int j = 0; j < RD2_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          const int b = o / Dl, c = o - b * Dl;
          const T* t_row = Ts + c * pr;
          for (int q = closes ? 0 : qp; q < (closes ? d : qp + 1); ++q) {
            const int b0 = b * row + (q * danc + g) * Dr;
            T S = El::zero();
#pragma unroll 4
            for (int bp = 0; bp < Dr; ++bp) El::fma(S, El::cj(El::ld(s.a, s.cplx, b0 + bp)), t_row[bp]);
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
#pragma unroll
    for (int j = 0; j < RD2_OUT_PER_THREAD; ++j) {
      const int o = tid + j * CHAIN_THREADS;
      if (o < nE) {
        const int b = o / Dl, c = o - b * Dl;
        R[b * pn + c] = acc[j];
      }
    }
    __syncthreads();
  }
}

template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_rdm2_envs(const Rd2Site* __restrict__ sites, int nsite, int stop,
                                                             int last, int e_elems, void* pool) {
  using T = typename ChainEl<CPLX>::T;
  extern __shared__ __attribute__((aligned(16))) double rd2_lds[];
  T* E = reinterpret_cast<T*>(rd2_lds);
  T* Ts = E + e_elems;
  if (blockIdx.x == 0)
    rd2_walk_right<CPLX>(sites, nsite, stop, E, Ts, static_cast<T*>(pool));
  else
    chain_walk_left<CPLX, RD2_OUT_PER_THREAD>(sites, last, E, Ts, static_cast<T*>(pool));
}

// Workgroup u: the row |p><p'| opened at site sel[k] = units[u].site.  E = L_k from the pooled buffer, then from that
// site to the last selected one.  At a later selected site l first the closing against all d_l^2 environments,
//   out[k, l][p][p'][q][q'] = sum_{b, c} E[b, c] G_l^{qq'}[b, c]:
// wave w takes the entries (q, q') = w, w + 16, .., its lanes stride over (b, c) in ascending order and are summed with
// shuffles - no barrier per entry.  Then (not behind the last selected site) the transfer, per slice in ascending order:
//   T[b, c'] = sum_c E[b, c] A[c, sigma, g, c']                                             (into LDS)
//   E'[b', c'] += sum_b conj(A[b, sigma', g, b']) T[b, c']                                  (registers of the owner)
// with (sigma', sigma) = (p, p') for every g at the opening site and sigma' = sigma over all (sigma, g) elsewhere.
// Threads take (b', c') with c' fastest, as in k_corr_rows.
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
    const int pe = Dl | 1, pe_new = Dr | 1;
    const int nT = Dl * Dr, nE = Dr * Dr, nL = Dl * Dl;
    const bool open = i == u.site;
    if (open) {
      const T* L = P + s.eoff;
      for (int o = tid; o < nL; o += CHAIN_THREADS) {
        const int b = o / Dl, c = o - b * Dl;
        E[b * pe + c] = L[o];
      }
      __syncthreads();
    } else if (s.sel >= 0) {
      const T* G = P + s.goff;
      const int dl2 = d * d;
      double* dst = out + 2 * (u.obase + u.dk2 * s.csum + (int64_t)u.row * dl2);
      for (int qq = wave; qq < dl2; qq += RD2_WAVES) {
        const T* g = G + qq * nL;
        T part = El::zero();
        for (int o = lane; o < nL; o += 64) {
          const int b = o / Dl, c = o - b * Dl;
          El::fma(part, E[b * pe + c], g[o]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) El::add(part, El::shfl_down(part, off));
        if (lane == 0) {
          dst[2 * qq] = El::re(part);
          dst[2 * qq + 1] = El::im(part);
        }
      }
      if (i == last) break;
    }
    T acc[RD2_OUT_PER_THREAD];
#pragma unroll
    for (int j = 0; j < RD2_OUT_PER_THREAD; ++j) acc[j] = El::zero();
    const int nslice = open ? danc : p;
    for (int t = 0; t < nslice; ++t) {
      const int ket = (open ? u.pp * danc + t : t) * Dr, bra = (open ? u.p * danc + t : t) * Dr;
      for (int o = tid; o < nT; o += CHAIN_THREADS) {
        const int b = o / Dr, cc = o - b * Dr;
        const T* e_row = E + b * pe;
        const int a0 = ket + cc;
        T sum = El::zero();
#pragma unroll 4
        for (int c = 0; c < Dl; ++c) El::fma(sum, e_row[c], El::ld(s.a, s.cplx, c * row + a0));
        Ts[o] = sum;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < RD2_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          const int bb = o / Dr, cc = o - bb * Dr;
          const int b0 = bra + bb;
          T S = El::zero();
#pragma unroll 4
          for (int b = 0; b < Dl; ++b) El::fma(S, El::cj(El::ld(s.a, s.cplx, b * row + b0)), Ts[b * Dr + cc]);
          El::add(acc[j], S);
        }
      }
      __syncthreads();   // T is overwritten by the next slice; after the last one every read of E is done as well
    }
#pragma unroll
    for (int j = 0; j < RD2_OUT_PER_THREAD; ++j) {
      const int o = tid + j * CHAIN_THREADS;
      if (o < nE) {
        const int bb = o / Dr, cc = o - bb * Dr;
        E[bb * pe_new + cc] = acc[j];
      }
    }
    __syncthreads();
  }
}

struct Rd2Args {
  int nsite;
  const void* const* sites;
  const int* dtype;
  const int64_t* dims;
  int nsel;
  const int* sel;
};

// d^2 of selected site k
int64_t rd2_dd(const Rd2Args& a, int k) { return a.dims[4 * a.sel[k] + 1] * a.dims[4 * a.sel[k] + 1]; }

// complex elements before the block of pair (k, l) for every k, l = k + 1: the pairs of one k follow each other with
// ascending l, so the block of (k, l) starts at obase[k] + d_k^2 * (csum[l] - csum[k + 1]), csum[m] the sum of d^2 over
// the selected sites before m
void rd2_offsets(const Rd2Args& a, std::vector<int64_t>* csum, std::vector<int64_t>* obase) {
  csum->assign((size_t)a.nsel + 1, 0);
  obase->assign((size_t)a.nsel, 0);
  for (int k = 0; k < a.nsel; ++k) (*csum)[k + 1] = (*csum)[k] + rd2_dd(a, k);
  for (int k = 0; k + 1 < a.nsel; ++k)
    (*obase)[k + 1] = (*obase)[k] + rd2_dd(a, k) * ((*csum)[a.nsel] - (*csum)[k + 1]);
}

int rdm2_chain(mpse_ctx* ctx, const Rd2Args& a, bool cplx, const Rd2Plan& pl, double* out_host) {
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
    rows[i] = Rd2Site{a.sites[i], (int)d[0], (int)d[1], (int)d[2], (int)d[3], a.dtype[i] == MPSE_C128,
                      is_sel ? k : -1, 0, 0, is_sel ? csum[k] : 0};
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
// are widened into pooled copies first, chain_widen_sites).
//   right pass, site i from the last one down to sel[1], R (D_r, D_r) = [b', c']:
//     Y1[(c, s, g), b'] = sum_c' A[(c, s, g), c'] R[b', c']
//     selected:  G_i[(b, c), (q, q')] = sum_(g, b') conj(A[b, q, (g, b')]) Y1[c, q', (g, b')]      (one product)
//     R'[b, c] = sum_(s, g, b') conj(A[b, (s, g, b')]) Y1[c, (s, g, b')]
//   left pass, site i from 0 to sel[nsel - 2] - 1, L (D_l, D_l) = [b, c]; L of a selected site is written straight
//   into its place in the pooled buffer, the others alternate between two scratch buffers:
//     X1[b, (s, g, c')] = sum_c L[b, c] A[c, (s, g, c')],  L'[b', c'] = sum_(b, s, g) conj(A[(b, s, g), b']) X1[(b, s, g), c']
//   open rows, a stack S[r][b][c] walked from the first opening site of a CHUNK to the last selected site:
//     selected site l with open rows:  C[r, (q, q')] = sum_(b, c) S[r, (b, c)] G_l[(b, c), (q, q')]   (one product)
//     X1[(r, b), (s, g, c')] = sum_c S[(r, b), c] A[c, (s, g, c')]                     (one product for the whole stack)
//     S'[r][b', c'] = sum_(b, s, g) conj(A[(b, s, g), b']) X1[r][(b, s, g), c']                       (batched over r)
//     opening site k of the chunk:  XL = L_k . A as X1 above, and d_k^2 new rows
//       S'[(p, p')][b', c'] = sum_(a, g) conj(A[a, p, g, b']) XL[a, p', g, c']                        (one product)
// A chunk is a run of whole opening sites whose rows keep the two stacks plus X1 inside rd2_stack_bytes(); one opening
// site that alone exceeds the bound is split by rows (then one product per p of the range).  C of one closing is
// contiguous on the device, rows in stack order; the one host read at the end copies every (k, l) run of rows to its
// place in the pair blocks, with 64-bit offsets.
int rdm2_enqueued(mpse_ctx* ctx, const Rd2Args& a, bool cplx, int64_t out_elems, double* out_host) {
  const int dt = cplx ? MPSE_C128 : MPSE_F64;
  const int cj = cplx ? 1 : 0;
  const size_t es = cplx ? 16 : 8;
  const int nsel = a.nsel, last = a.sel[nsel - 1];
  std::vector<int64_t> csum, obase;
  rd2_offsets(a, &csum, &obase);
  int64_t e_max = 1, x_max = 1, l_elems = 0, g_elems = 0;
  std::vector<int64_t> loff((size_t)nsel, 0), goff((size_t)nsel, 0);
  std::vector<int> pos((size_t)a.nsite, -1);
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const int64_t* d = a.dims + 4 * i;
    e_max = d[3] * d[3] > e_max ? d[3] * d[3] : e_max;
    const int64_t x = d[0] * d[1] * d[2] * d[3];
    x_max = x > x_max ? x : x_max;
    if (k < nsel && a.sel[k] == i) {
      pos[i] = k;
      if (k < nsel - 1) loff[k] = l_elems, l_elems += d[0] * d[0];
      if (k > 0) goff[k] = g_elems, g_elems += d[0] * d[0] * d[1] * d[1];
      ++k;
    }
  }
  // ---- the chunks: opening sites [k0, k1], rows [r0, r1) of every one of them (a part only when k0 == k1)
  struct Chunk {
    int k0, k1;
    int64_t r0, r1;
  };
  const int64_t row_bytes = (2 * e_max + x_max) * (int64_t)es;
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
  std::vector<std::unique_ptr<TmpBuf>> wide;
  std::vector<const void*> site;
  MPSE_TRY(chain_widen_sites(ctx, a.nsite, a.sites, a.dtype, a.dims, cplx, &wide, &site));
  TmpBuf lbuf(ctx), gbuf(ctx), res(ctx), e0(ctx), e1(ctx), xl(ctx), s0(ctx), s1(ctx), x1(ctx);
  MPSE_TRY(lbuf.alloc((size_t)l_elems * es));
  MPSE_TRY(gbuf.alloc((size_t)g_elems * es));
  MPSE_TRY(res.alloc((size_t)out_elems * es));
  MPSE_TRY(e0.alloc((size_t)e_max * es));
  MPSE_TRY(e1.alloc((size_t)e_max * es));
  MPSE_TRY(xl.alloc((size_t)x_max * es));
  MPSE_TRY(s0.alloc((size_t)rows_cap * e_max * es));
  MPSE_TRY(s1.alloc((size_t)rows_cap * e_max * es));
  MPSE_TRY(x1.alloc((size_t)rows_cap * x_max * es));
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
      MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(Dl * p, Dr), idx1(Dr, 1), idx1(Dr, 1), idx1(Dr, Dr), idx1(Dl * p, Dr),
                         idx1(Dr, 1), 1, 0, 0, 0, site[i], R, xl.p));
      if (pos[i] >= 0)
        MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(Dl * dd, da * Dr), idx1(da * Dr, 1), idx1(da * Dr, 1),
                           idx1(Dl * dd, da * Dr), idx2(Dl, dd, Dl * dd * dd, dd), idx2(Dl, dd, dd * dd, 1), 1, 0, 0, 0,
                           site[i], xl.p, G + (size_t)goff[pos[i]] * es));
      if (i == a.sel[1]) break;
      MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(Dl, p * Dr), idx1(p * Dr, 1), idx1(p * Dr, 1), idx1(Dl, p * Dr),
                         idx1(Dl, Dl), idx1(Dl, 1), 1, 0, 0, 0, site[i], xl.p, Rn));
      std::swap(R, Rn);
    }
  }
  // ---- left pass; where L_i (the environment left of site i) lives
  auto l_at = [&](int i) -> void* {
    return pos[i] >= 0 && pos[i] < nsel - 1 ? static_cast<char*>(lbuf.p) + (size_t)loff[pos[i]] * es : scratch[i & 1];
  };
  MPSE_TRY(stage_h2d(ctx, l_at(0), one, es));
  for (int i = 0; i < a.sel[nsel - 2]; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], p = d[1] * d[2], Dr = d[3];
    MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(Dl, Dl), idx1(Dl, 1), idx1(Dl, p * Dr), idx1(p * Dr, 1),
                       idx1(Dl, p * Dr), idx1(p * Dr, 1), 1, 0, 0, 0, l_at(i), site[i], xl.p));
    MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(Dr, 1), idx1(Dl * p, Dr), idx1(Dl * p, Dr), idx1(Dr, 1), idx1(Dr, Dr),
                       idx1(Dr, 1), 1, 0, 0, 0, site[i], xl.p, l_at(i + 1)));
  }
  // ---- open rows, chunk by chunk
  struct Run {   // rows [r0, r0 + n) of pair (k, l) lie at `dev` complex elements into res
    int64_t dev, r0, n;
    int k, l;
  };
  std::vector<Run> runs;
  int64_t filled = 0;
  for (const Chunk& ch : chunks) {
    char* S = static_cast<char*>(s0.p);
    char* Sn = static_cast<char*>(s1.p);
    int64_t nrow = 0;
    std::vector<Run> open_runs;   // dev: rows before the run in the stack
    for (int i = a.sel[ch.k0]; i <= last; ++i) {
      const int64_t* d = a.dims + 4 * i;
      const int64_t Dl = d[0], dd = d[1], da = d[2], Dr = d[3], p = dd * da;
      const int k = pos[i];
      if (k >= 0 && nrow > 0) {
        MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(nrow, Dl * Dl), idx1(Dl * Dl, 1), idx1(Dl * Dl, dd * dd),
                           idx1(dd * dd, 1), idx1(nrow, dd * dd), idx1(dd * dd, 1), 1, 0, 0, 0, S,
                           G + (size_t)goff[k] * es, static_cast<char*>(res.p) + (size_t)filled * es));
        for (const Run& r : open_runs) runs.push_back(Run{filled + r.dev * dd * dd, r.r0, r.n, r.k, k});
        filled += nrow * dd * dd;
      }
      if (i == last) break;
      if (nrow > 0) {
        MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(nrow * Dl, Dl), idx1(Dl, 1), idx1(Dl, p * Dr), idx1(p * Dr, 1),
                           idx1(nrow * Dl, p * Dr), idx1(p * Dr, 1), 1, 0, 0, 0, S, site[i], x1.p));
        MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(Dr, 1), idx1(Dl * p, Dr), idx1(Dl * p, Dr), idx1(Dr, 1),
                           idx1(Dr, Dr), idx1(Dr, 1), nrow, 0, Dl * p * Dr, Dr * Dr, site[i], x1.p, Sn));
      }
      if (k >= ch.k0 && k <= ch.k1) {
        const bool part = ch.r1 > ch.r0;
        const int64_t ra = part ? ch.r0 : 0, rb = part ? ch.r1 : dd * dd;
        char* dest = Sn + (size_t)(nrow * Dr * Dr) * es;
        MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(Dl, Dl), idx1(Dl, 1), idx1(Dl, p * Dr), idx1(p * Dr, 1),
                           idx1(Dl, p * Dr), idx1(p * Dr, 1), 1, 0, 0, 0, l_at(i), site[i], xl.p));
        // the rows (p, p') of [ra, rb): for every p its range [lo, hi) of p'; M = (p, b'), K = (a, g), N = (p', c')
        for (int64_t pr = ra / dd; pr * dd < rb; ++pr) {
          int64_t np = 1, lo = std::max(ra, pr * dd) - pr * dd, hi = std::min(rb, (pr + 1) * dd) - pr * dd;
          if (!part) np = dd, lo = 0, hi = dd;   // the whole site in one product
          const char* Ap = static_cast<const char*>(site[i]) + (size_t)(pr * da * Dr) * es;
          const char* Bp = static_cast<const char*>(xl.p) + (size_t)(lo * da * Dr) * es;
          MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx2(np, Dr, da * Dr, 1), idx2(Dl, da, p * Dr, Dr),
                             idx2(Dl, da, p * Dr, Dr), idx2(hi - lo, Dr, da * Dr, 1), idx2(np, Dr, dd * Dr * Dr, Dr),
                             idx2(hi - lo, Dr, Dr * Dr, 1), 1, 0, 0, 0, Ap, Bp,
                             dest + (size_t)((pr * dd + lo - ra) * Dr * Dr) * es));
          if (!part) break;
        }
        open_runs.push_back(Run{nrow, ra, rb - ra, k, -1});
        nrow += rb - ra;
      }
      std::swap(S, Sn);
    }
  }
  if (filled != out_elems) return mpse_fail(ctx, MPSE_ERR_ARG, "mps_rdm2: the chunks do not cover the result");
  std::vector<double> host((size_t)out_elems * (cplx ? 2 : 1));
  MPSE_TRY(mpse_memcpy_d2h(ctx, host.data(), res.p, host.size() * sizeof(double)));
  for (const Run& r : runs) {
    const int64_t dl2 = rd2_dd(a, r.l);
    const int64_t dst = obase[r.k] + rd2_dd(a, r.k) * (csum[r.l] - csum[r.k + 1]) + r.r0 * dl2;
    for (int64_t e = 0; e < r.n * dl2; ++e) {
      out_host[2 * (dst + e)] = cplx ? host[2 * (r.dev + e)] : host[r.dev + e];
      out_host[2 * (dst + e) + 1] = cplx ? host[2 * (r.dev + e) + 1] : 0.0;
    }
  }
  return MPSE_OK;
}

}  // namespace

extern "C" {

int mpse_mps_rdm2_plan(int nsite, const int64_t* dims, int nsel, const int* sel, int any_complex, int64_t* info, int n) {
  const bool valid = rdm2_table_ok(nsite, dims);
  const bool sel_ok = valid && rdm2_sel_ok(nsite, nsel, sel);
  const Rd2Plan pl = sel_ok ? rdm2_plan(nsite, dims, nsel, sel, any_complex != 0)
                            : Rd2Plan{false, false, valid ? rdm2_plan(nsite, dims, 0, nullptr, false).max_bond : 0,
                                      0, 0, 0, 0, 0, 0};
  const int64_t v[15] = {RD2_BOND_MAX, CHAIN_LDS_MAX, pl.chain ? pl.lds : 0, pl.fit ? pl.e_elems : 0,
                         pl.fit ? pl.t_elems : 0, CHAIN_THREADS, pl.max_bond, valid ? 1 : 0,
                         0, CHAIN_EXT_MAX, RD2_BOND_FIT, pl.fit ? pl.lds : 0,
                         pl.units, pl.out_elems, RD2_STACK_BYTES_MAX};
  plan_info_out(info, n, v, 15);
  return pl.chain ? 1 : 0;
}

int mpse_mps_rdm2_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::rdm2_stats, counts, n);
}

int mpse_mps_rdm2(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims, int nsel,
                  const int* sel, double* out_host) {
  if (!ctx) return MPSE_ERR_ARG;
  if (nsite < 1 || !sites || !dtype || !dims || nsel < 2 || !sel || !out_host)
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_rdm2: null argument, no sites or fewer than two selected sites");
  bool cplx = false;
  MPSE_TRY(chain_scan_sites(ctx, "mps_rdm2", nsite, {sites}, {dtype}, &cplx));
  if (!rdm2_sel_ok(nsite, nsel, sel))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "mps_rdm2: the selection is not strictly ascending inside [0, %d)", nsite);
  if (!rdm2_table_ok(nsite, dims))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "mps_rdm2: dims is not a chain (extents >= 1, matching neighbours, first and last bond 1)");
  if (MPSE_RECORDING(ctx))
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_rdm2: synchronous, not available while a deferred list is recorded");
  Rd2Plan pl = rdm2_plan(nsite, dims, nsel, sel, cplx);
  if (pl.out_elems > RD2_OUT_ELEMS_CAP)
    return mpse_fail(ctx, MPSE_ERR_OOM, "mps_rdm2: a result of %lld complex elements", (long long)pl.out_elems);
  MPSE_BIND(ctx);
  // MPSE_RDM2_CHAIN=0 sends every chain through the enqueued products; =1 sends every chain whose launches fit through
  // the kernels, above the bond limit of the rule as well (measurements of that limit: tools/rdm2_bench.py)
  const char env = chain_env_switch("MPSE_RDM2_CHAIN");
  if (env == '0') pl.chain = false;
  if (env == '1') pl.chain = pl.fit;
  const Rd2Args args{nsite, sites, dtype, dims, nsel, sel};
  std::vector<double> res((size_t)pl.out_elems * 2, 0.0);
  if (pl.chain)
    MPSE_TRY(rdm2_chain(ctx, args, cplx, pl, res.data()));
  else
    MPSE_TRY(rdm2_enqueued(ctx, args, cplx, pl.out_elems, res.data()));
  ctx->rdm2_stats[pl.chain ? mpse_ctx::RD2_CHAIN : mpse_ctx::RD2_ENQUEUED] += 1;
  ctx->rdm2_stats[mpse_ctx::RD2_SITES] += nsite;
  ctx->rdm2_stats[mpse_ctx::RD2_PAIRS] += (long long)nsel * (nsel - 1) / 2;
  memcpy(out_host, res.data(), res.size() * sizeof(double));
  return MPSE_OK;
}

}  // extern "C"
