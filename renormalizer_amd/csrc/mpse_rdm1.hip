// mpse_mps_rdm1: the one-site reduced density matrices
//   rho_i[p, p'] = sum_{a,a',g,b,b'} conj(A[a,p,g,b]) L_i[a,a'] A[a',p',g,b'] R_i[b,b']
// of selected sites of ONE chain as one engine call (the reference closes every site with three products and a host
// read of its own, mps/mps.py:1547-1598 calc_1site_rdm; local expectation values <O> = sum O[p,p'] rho_i[p,p'] take one
// operator window and one host read each).  L_i / R_i: the identity-operator environments left / right of site i, first
// index from the conjugated tensor.  Two paths, chosen from the dims table alone (rdm1_plan):
//   chain      two launches, for chains whose bonds are at most RD_BOND_MAX.  k_rdm1_envs: workgroup 0 walks right to
//              left with R in LDS, workgroup 1 left to right with L in LDS (chain_walk_left); each leaves its environment of every
//              selected site in pooled memory (R transposed, so that k_rdm1_sites reads it along the lanes).
//              k_rdm1_sites: one workgroup per selected site closes L_i and R_i around the site.  A workgroup reads
//              only what the launch before it wrote: no flag, no spin wait, no atomic.
//   enqueued   the same contractions as products of the contraction kernel - every other chain
// LDS plan of either launch, working elements (8 or 16 bytes), rows padded to an odd pitch (chain_pitch):
//   region E   max over the bonds D of D * pitch(D)                 k_rdm1_envs: the environment;  k_rdm1_sites: U
//   region T   max over the sites of D_l * pitch(D_r)               k_rdm1_envs: the slice T;      k_rdm1_sites: V
// (U is D_l x D_r unpadded, D_l * D_r <= max(D_l, D_r) * pitch(max(D_l, D_r)) <= E.)  L and R of k_rdm1_sites stay in
// the pooled buffer and are read through L2: with them in LDS a complex bond of 64 would need 4 x 64 x 65 x 16 = 260 KB.
// The host reads once, at the end.  A fixed summation order: the same inputs give the same bits.
#include "mpse_chain.h"

namespace {

constexpr int RD_WAVES = CHAIN_THREADS / 64;
constexpr int RD_OUT_PER_THREAD = 4;      // entries of a new environment a thread accumulates in registers
constexpr int64_t rd_lds_bytes(int64_t D, int64_t es) { return 2 * D * chain_pitch(D) * es; }
constexpr int64_t rd_bond_limit() {
  // the largest power-of-two bond D whose complex regions E and T (both D rows, padded) fit, and whose environment has
  // one entry per accumulator of the workgroup
  int64_t D = 1;
  while (rd_lds_bytes(2 * D, 16) <= CHAIN_LDS_MAX && 4 * D * D <= int64_t(CHAIN_THREADS) * RD_OUT_PER_THREAD) D *= 2;
  return D;
}
constexpr int64_t RD_BOND_FIT = rd_bond_limit();
static_assert(RD_BOND_FIT == 64, "2 x 64 x 65 complex128 = 130 KB of 160 KB; 128 would need 516 KB");
// Largest bond up to which the two launches are faster than the enqueued products: measured with tools/rdm1_bench.py,
// profiles/rdm1.md (ahead at 8 and 16 on both models; at 32 ahead with 4 phonon levels, behind with 16; each walk being
// one workgroup on one compute unit, far behind at 64).  Chains between this and RD_BOND_FIT take the kernels only
// under MPSE_RDM1_CHAIN=1.
constexpr int64_t RD_BOND_MAX = 16;
static_assert(1 <= RD_BOND_MAX && RD_BOND_MAX <= RD_BOND_FIT, "the measured limit lies inside what fits");
// d danc <= CHAIN_EXT_MAX keeps the site offsets inside 32 bits: 64 * 65536 * 64 = 2^28 elements.  The grid of
// k_rdm1_sites is one workgroup per selected site, whatever their number: no cap on nsel.

struct RdSite {   // one row of the descriptor table (48 bytes): nsite rows, then the rows of the selected sites again
  const void* a;
  int Dl, d, danc, Dr;
  int cplx;       // the tensor is complex128
  int sel;        // position in the selection, -1: not selected
  int64_t eoff;   // working elements before L of this site in the pooled buffer; R (transposed) at + Dl Dl
  int64_t ooff;   // complex elements before rho of this site in the result
};
static_assert(sizeof(RdSite) == 48, "descriptor rows are copied as 8-byte words");

struct RdPlan {
  bool chain;            // the chain kernels take it
  bool fit;              // they could: LDS and offsets allow the launches, whatever the measured bond limit says
  int64_t max_bond;
  int64_t e_elems;       // LDS elements of region E
  int64_t t_elems;       // LDS elements of region T
  int64_t lds;           // bytes of either launch, working dtype
};

bool rdm1_table_ok(int nsite, const int64_t* dims) { return chain_table_ok(nsite, dims, 4, {0}, {3}); }

// the sizing of a table that is a chain
RdPlan rdm1_plan(int nsite, const int64_t* dims, int nsel, bool cplx) {
  RdPlan pl{false, false, 0, 0, 0, 0};
  bool fits = true;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + 4 * i;
    for (int j : {0, 3}) pl.max_bond = d[j] > pl.max_bond ? d[j] : pl.max_bond;
    if (pl.max_bond > RD_BOND_FIT || d[1] > CHAIN_EXT_MAX || d[2] > CHAIN_EXT_MAX || d[1] * d[2] > CHAIN_EXT_MAX) {
      fits = false;
      continue;
    }
    const int64_t e_l = d[0] * chain_pitch(d[0]), e_r = d[3] * chain_pitch(d[3]), t = d[0] * chain_pitch(d[3]);
    pl.e_elems = e_l > pl.e_elems ? e_l : pl.e_elems;
    pl.e_elems = e_r > pl.e_elems ? e_r : pl.e_elems;
    pl.t_elems = t > pl.t_elems ? t : pl.t_elems;
  }
  if (!fits || nsel < 1) {
    pl.e_elems = pl.t_elems = 0;
    return pl;
  }
  pl.lds = (pl.e_elems + pl.t_elems) * (cplx ? 16 : 8);
  pl.fit = pl.lds <= CHAIN_LDS_MAX;
  if (!pl.fit) pl.lds = pl.e_elems = pl.t_elems = 0;
  pl.chain = pl.fit && pl.max_bond <= RD_BOND_MAX;
  return pl;
}

// Workgroup 0 of k_rdm1_envs.  R_N = 1.  At a selected site R goes to the pooled buffer, transposed; the walk ends at
// the first selected site.  Else per site from the right, per (sigma, a) in ascending order:
//   T[c, b'] = sum_c' A[c, sigma, a, c'] R[b', c']                                          (into LDS)
//   R'[b, c] += sum_b' conj(A[b, sigma, a, b']) T[c, b']                                    (registers of the owner)
// R' replaces R in LDS after the last (sigma, a).  A thread owns the entries (b, c) = tid + j * CHAIN_THREADS, c
// fastest: A[b, ..] is one address per b group, the reads of T run down a column of padded rows.
template <bool CPLX>
__device__ void rd_walk_right(const RdSite* __restrict__ sites, int nsite, int first, typename ChainEl<CPLX>::T* R,
                              typename ChainEl<CPLX>::T* Ts, typename ChainEl<CPLX>::T* pool) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int tid = threadIdx.x;
  if (tid == 0) R[0] = El::one();
  __syncthreads();
  for (int i = nsite - 1; i >= first; --i) {
    const RdSite s = sites[i];
    const int Dl = s.Dl, Dr = s.Dr;
    const int p = s.d * s.danc, row = p * Dr;   // element stride of the left bond
    const int pr = Dr | 1, pn = Dl | 1;
    const int nT = Dl * Dr, nE = Dl * Dl;
    if (s.sel >= 0) {
      T* Rt = pool + s.eoff + nE;
      for (int o = tid; o < Dr * Dr; o += CHAIN_THREADS) {
        const int bp = o / Dr, b = o - bp * Dr;
        Rt[o] = R[b * pr + bp];
      }
    }
    if (i == first) break;
    T acc[RD_OUT_PER_THREAD];
#pragma unroll
    for (int j = 0; j < RD_OUT_PER_THREAD; ++j) acc[j] = El::zero();
    for (int sa = 0; sa < p; ++sa) {
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
      for (int j = 0; j < RD_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          const int b = o / Dl, c = o - b * Dl;
          const T* t_row = Ts + c * pr;
          const int b0 = b * row + sa * Dr;
          T S = El::zero();
#pragma unroll 4
          for (int bp = 0; bp < Dr; ++bp) El::fma(S, El::cj(El::ld(s.a, s.cplx, b0 + bp)), t_row[bp]);
          El::add(acc[j], S);
        }
      }
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of R is done as well
    }
#pragma unroll
    for (int j = 0; j < RD_OUT_PER_THREAD; ++j) {
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
__global__ __launch_bounds__(CHAIN_THREADS) void k_rdm1_envs(const RdSite* __restrict__ sites, int nsite, int first,
                                                             int last, int e_elems, void* pool) {
  using T = typename ChainEl<CPLX>::T;
  extern __shared__ __attribute__((aligned(16))) double rd_lds[];
  T* E = reinterpret_cast<T*>(rd_lds);
  T* Ts = E + e_elems;
  if (blockIdx.x == 0)
    rd_walk_right<CPLX>(sites, nsite, first, E, Ts, static_cast<T*>(pool));
  else
    chain_walk_left<CPLX, RD_OUT_PER_THREAD>(sites, last, E, Ts, static_cast<T*>(pool));   // workgroup 1: mpse_chain.h
}

// Workgroup k closes the environments of site sel[k] (row nsite + k of the table).  Per (sigma', a) in ascending order:
//   V[a, b'] = sum_a' L[a, a'] A[a', sigma', a, b']                                          (into LDS, region T)
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
      const int sa = (sp * danc + g) * Dr;
      for (int o = tid; o < nU; o += CHAIN_THREADS) {
        const int a = o / Dr, bp = o - a * Dr;
        const T* l_row = L + a * Dl;
        T sum = El::zero();
#pragma unroll 4
        for (int ap = 0; ap < Dl; ++ap) El::fma(sum, l_row[ap], El::ld(s.a, s.cplx, ap * row + sa + bp));
        V[a * pv + bp] = sum;
      }
      __syncthreads();
      for (int o = tid; o < nU; o += CHAIN_THREADS) {
        const int a = o / Dr, b = o - a * Dr;
        const T* v_row = V + a * pv;
        T sum = El::zero();
#pragma unroll 4
        for (int bp = 0; bp < Dr; ++bp) El::fma(sum, v_row[bp], Rt[bp * Dr + b]);
        U[o] = sum;
      }
      __syncthreads();   // the next U is written behind the barrier after the next V: every wave is through its sums then
      for (int sg = wave; sg < d; sg += RD_WAVES) {
        const int s0 = (sg * danc + g) * Dr;
        T part = El::zero();
        for (int o = lane; o < nU; o += 64) {
          const int a = o / Dr, b = o - a * Dr;
          El::fma(part, El::cj(El::ld(s.a, s.cplx, a * row + s0 + b)), U[o]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) El::add(part, El::shfl_down(part, off));
        if (lane == 0) {
          double* dst = out + 2 * (s.ooff + (int64_t)sg * d + sp);
          dst[0] = (g ? dst[0] : 0.0) + El::re(part);
          dst[1] = (g ? dst[1] : 0.0) + El::im(part);
        }
      }
    }
  }
}

struct RdArgs {
  int nsite;
  const void* const* sites;
  const int* dtype;
  const int64_t* dims;
  int nsel;
  const int* sel;
};

int64_t rdm1_out_elems(const RdArgs& a) {
  int64_t n = 0;
  for (int k = 0; k < a.nsel; ++k) n += a.dims[4 * a.sel[k] + 1] * a.dims[4 * a.sel[k] + 1];
  return n;
}

int rdm1_chain(mpse_ctx* ctx, const RdArgs& a, bool cplx, const RdPlan& pl, double* out_host) {
  std::vector<RdSite> rows((size_t)a.nsite + a.nsel);
  int64_t e_elems = 0, o_elems = 0;
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const bool is_sel = k < a.nsel && a.sel[k] == i;
    rows[i] = RdSite{a.sites[i], (int)d[0], (int)d[1], (int)d[2], (int)d[3], a.dtype[i] == MPSE_C128,
                     is_sel ? k : -1, is_sel ? e_elems : 0, is_sel ? o_elems : 0};
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
// are widened into pooled copies first, widen_site).
//   right pass, site i from the last one down to sel[0] + 1, R (D_r, D_r) = [b', c']:
//     Y1[(c, s, a), b'] = sum_c' A[(c, s, a), c'] R[b', c']
//     R'[b, c] = sum_(s, a, b') conj(A[b, (s, a, b')]) Y1[c, (s, a, b')]
//   R of a selected site is written straight into its place in the pooled buffer, the others alternate between two
//   scratch buffers.
//   left pass, site i from 0 to sel[nsel - 1], L (D_l, D_l) = [b, c]:
//     X1[b, (s, a, c')] = sum_c L[b, c] A[c, (s, a, c')]
//     selected:  Y[(b, s, a), c] = sum_c' X1[(b, s, a), c'] R_i[c, c']
//                rho[s', s] = sum_(b, a, c) conj(A[b, s', (a, c)]) Y[b, s, (a, c)]       (into the packed result)
//     L'[b', c'] = sum_(b, s, a) conj(A[(b, s, a), b']) X1[(b, s, a), c']
int rdm1_enqueued(mpse_ctx* ctx, const RdArgs& a, bool cplx, double* out_host) {
  const int dt = cplx ? MPSE_C128 : MPSE_F64;
  const int cj = cplx ? 1 : 0;
  const size_t es = cplx ? 16 : 8;
  const int nsel = a.nsel, first = a.sel[0], last = a.sel[nsel - 1];
  int64_t e_max = 1, x_max = 1, r_elems = 0, o_elems = 0;
  std::vector<int64_t> roff((size_t)nsel), ooff((size_t)nsel);
  std::vector<int> pos((size_t)a.nsite, -1);
  for (int i = 0, k = 0; i < a.nsite; ++i) {
    const int64_t* d = a.dims + 4 * i;
    e_max = d[3] * d[3] > e_max ? d[3] * d[3] : e_max;
    const int64_t x = d[0] * d[1] * d[2] * d[3];
    x_max = x > x_max ? x : x_max;
    if (k < nsel && a.sel[k] == i) {
      pos[i] = k;
      roff[k] = r_elems, ooff[k] = o_elems;
      r_elems += d[3] * d[3];
      o_elems += d[1] * d[1];
      ++k;
    }
  }
  // widened copies of the real sites of a complex call live to the end of the call
  std::vector<std::unique_ptr<TmpBuf>> wide;
  std::vector<const void*> site;
  MPSE_TRY(chain_widen_sites(ctx, a.nsite, a.sites, a.dtype, a.dims, cplx, &wide, &site));
  TmpBuf rbuf(ctx), res(ctx), e0(ctx), e1(ctx), x1(ctx), y(ctx);
  MPSE_TRY(rbuf.alloc((size_t)r_elems * es));
  MPSE_TRY(res.alloc((size_t)o_elems * es));
  MPSE_TRY(e0.alloc((size_t)e_max * es));
  MPSE_TRY(e1.alloc((size_t)e_max * es));
  MPSE_TRY(x1.alloc((size_t)x_max * es));
  MPSE_TRY(y.alloc((size_t)x_max * es));
  const double one[2] = {1.0, 0.0};
  void* scratch[2] = {e0.p, e1.p};
  // where R_i (the environment right of site i) lives
  auto r_at = [&](int i) -> void* {
    return pos[i] >= 0 ? static_cast<char*>(rbuf.p) + (size_t)roff[pos[i]] * es : scratch[i & 1];
  };
  // ---- right pass
  MPSE_TRY(stage_h2d(ctx, r_at(a.nsite - 1), one, es));
  for (int i = a.nsite - 1; i > first; --i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], p = d[1] * d[2], Dr = d[3];
    MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(Dl * p, Dr), idx1(Dr, 1), idx1(Dr, 1), idx1(Dr, Dr), idx1(Dl * p, Dr),
                       idx1(Dr, 1), 1, 0, 0, 0, site[i], r_at(i), x1.p));
    MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(Dl, p * Dr), idx1(p * Dr, 1), idx1(p * Dr, 1), idx1(Dl, p * Dr),
                       idx1(Dl, Dl), idx1(Dl, 1), 1, 0, 0, 0, site[i], x1.p, r_at(i - 1)));
  }
  // ---- left pass
  void* L = scratch[0];
  void* Ln = scratch[1];
  MPSE_TRY(stage_h2d(ctx, L, one, es));
  for (int i = 0; i <= last; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], dd = d[1], da = d[2], Dr = d[3], p = dd * da;
    MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(Dl, Dl), idx1(Dl, 1), idx1(Dl, p * Dr), idx1(p * Dr, 1),
                       idx1(Dl, p * Dr), idx1(p * Dr, 1), 1, 0, 0, 0, L, site[i], x1.p));
    if (pos[i] >= 0) {
      MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(Dl * p, Dr), idx1(Dr, 1), idx1(Dr, 1), idx1(Dr, Dr), idx1(Dl * p, Dr),
                         idx1(Dr, 1), 1, 0, 0, 0, x1.p, r_at(i), y.p));
      MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(dd, da * Dr), idx2(Dl, da * Dr, p * Dr, 1),
                         idx2(Dl, da * Dr, p * Dr, 1), idx1(dd, da * Dr), idx1(dd, dd), idx1(dd, 1), 1, 0, 0, 0, site[i],
                         y.p, static_cast<char*>(res.p) + (size_t)ooff[pos[i]] * es));
    }
    if (i == last) break;
    MPSE_TRY(gemm_call(ctx, dt, dt, cj, 0, idx1(Dr, 1), idx1(Dl * p, Dr), idx1(Dl * p, Dr), idx1(Dr, 1), idx1(Dr, Dr),
                       idx1(Dr, 1), 1, 0, 0, 0, site[i], x1.p, Ln));
    void* t = L;
    L = Ln, Ln = t;
  }
  std::vector<double> host((size_t)o_elems * (cplx ? 2 : 1));
  MPSE_TRY(mpse_memcpy_d2h(ctx, host.data(), res.p, host.size() * sizeof(double)));
  for (size_t e = 0; e < (size_t)o_elems; ++e) {
    out_host[2 * e] = cplx ? host[2 * e] : host[e];
    out_host[2 * e + 1] = cplx ? host[2 * e + 1] : 0.0;
  }
  return MPSE_OK;
}

}  // namespace

extern "C" {

int mpse_mps_rdm1_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n) {
  const bool valid = rdm1_table_ok(nsite, dims);
  const RdPlan pl = valid ? rdm1_plan(nsite, dims, nsel, any_complex != 0) : RdPlan{false, false, 0, 0, 0, 0};
  const int64_t v[12] = {RD_BOND_MAX, CHAIN_LDS_MAX, pl.chain ? pl.lds : 0, pl.fit ? pl.e_elems : 0,
                         pl.fit ? pl.t_elems : 0, CHAIN_THREADS, pl.max_bond, valid ? 1 : 0,
                         0, CHAIN_EXT_MAX, RD_BOND_FIT, pl.fit ? pl.lds : 0};
  plan_info_out(info, n, v, 12);
  return pl.chain ? 1 : 0;
}

int mpse_mps_rdm1_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::rdm1_stats, counts, n);
}

int mpse_mps_rdm1(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims, int nsel,
                  const int* sel, double* out_host) {
  if (!ctx) return MPSE_ERR_ARG;
  if (nsite < 1 || !sites || !dtype || !dims || nsel < 1 || !sel || !out_host)
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_rdm1: null argument, no sites or no selection");
  bool cplx = false;
  MPSE_TRY(chain_scan_sites(ctx, "mps_rdm1", nsite, {sites}, {dtype}, &cplx));
  for (int k = 0; k < nsel; ++k)
    if (sel[k] < 0 || sel[k] >= nsite || (k > 0 && sel[k] <= sel[k - 1]))
      return mpse_fail(ctx, MPSE_ERR_SHAPE, "mps_rdm1: the selection is not strictly ascending inside [0, %d)", nsite);
  if (!rdm1_table_ok(nsite, dims))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "mps_rdm1: dims is not a chain (extents >= 1, matching neighbours, first and last bond 1)");
  if (MPSE_RECORDING(ctx))
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_rdm1: synchronous, not available while a deferred list is recorded");
  RdPlan pl = rdm1_plan(nsite, dims, nsel, cplx);
  MPSE_BIND(ctx);
  // MPSE_RDM1_CHAIN=0 sends every chain through the enqueued products; =1 sends every chain whose launches fit through
  // the kernels, above the bond limit of the rule as well (measurements of that limit: tools/rdm1_bench.py)
  const char env = chain_env_switch("MPSE_RDM1_CHAIN");
  if (env == '0') pl.chain = false;
  if (env == '1') pl.chain = pl.fit;
  const RdArgs args{nsite, sites, dtype, dims, nsel, sel};
  std::vector<double> res((size_t)rdm1_out_elems(args) * 2, 0.0);
  if (pl.chain)
    MPSE_TRY(rdm1_chain(ctx, args, cplx, pl, res.data()));
  else
    MPSE_TRY(rdm1_enqueued(ctx, args, cplx, res.data()));
  ctx->rdm1_stats[pl.chain ? mpse_ctx::RD_CHAIN : mpse_ctx::RD_ENQUEUED] += 1;
  ctx->rdm1_stats[mpse_ctx::RD_SITES] += nsite;
  ctx->rdm1_stats[mpse_ctx::RD_MATRICES] += nsel;
  memcpy(out_host, res.data(), res.size() * sizeof(double));
  return MPSE_OK;
}

}  // extern "C"
