// mpse_mps_bond_spectra: the Schmidt weights p = sigma^2 of selected bonds of ONE chain as one engine call, from the two
// identity-operator environments of a bond instead of a canonical form (the reference copies the state, sweeps it into
// right-canonical form with a blocked QR per site and sweeps back with a blocked SVD per bond, mps/mps.py:1759-1773
// calc_bond_singular_values).  Bond k lies between the sites k and k + 1; L (D x D) is the environment of the sites
// 0 .. k, R that of the sites k + 1 .., first index from the conjugated tensor.  With the state cut at the bond,
// psi = X Y (X: left part x D, Y: D x right part), L = X^H X and R^T = Y Y^H, and the weights are the non-zero
// eigenvalues of (X Y)(X Y)^H, which are those of R^T L and of the Hermitian L^(1/2) R^T L^(1/2).  With L = U Lambda U^H:
//   M = Lambda^(1/2) U^H R^T U Lambda^(1/2),   p = eig(M)
// No inverse: a rank-deficient L (a padded bond) only puts zero rows and columns into M.  Two paths, chosen from the dims
// table alone (bondspec_plan):
//   chain      two launches, for chains whose bonds are at most BS_BOND_MAX.  k_bondspec_envs: the two walks of
//              k_rdm1_envs as mpse_chain_walk.h has them for bonds (walk_envs with AT_BOND); workgroup 0 walks right to
//              left and leaves R of every selected bond in pooled memory, workgroup 1 left to right and leaves L.  k_bondspec_eig: one workgroup per selected bond, two Hermitian
//              eigensolves in LDS by a cyclic two-sided Jacobi (bs_jacobi).
//   enqueued   the two passes as products of the contraction kernel, the two solves of a bond through the block SVD
//              (a Hermitian positive semidefinite matrix has its eigenvalues as singular values and the eigenvectors of
//              its non-zero values as left vectors; the columns of the null space meet sqrt(0)) - every other chain;
//              two host reads per bond, no speed claimed
// LDS plan of k_bondspec_eig at bond D, working elements (8 or 16 bytes), rows padded to chain_pitch(D):
//   region A   D * pitch   L, then W = R^T U, then M
//   region V   D * pitch   U
//   strip      D           the rotations of a Jacobi step (c and sigma of each pair: 2 or 3 doubles); between the solves
//                          Lambda^(1/2); at the end the weights
// A third region for M does not fit at a complex bond of 64 (3 x 64 x 65 x 16 B = 200 KB of 160 KB): M is formed from
// W and U entry by entry, staged through the D D pooled elements that held L, and read back behind a barrier.  R stays
// in pooled memory: in W[a, j] = sum_b R[b, a] U[b, j] the lanes run over j (U along a row of LDS) and, for D < 64, over
// a, which R as the walk leaves it has side by side.  k_bondspec_envs has the plan of k_rdm1_envs (mpse_rdm1.hip).
#include "mpse_chain_walk.h"

namespace {

// Largest bond up to which the two launches are faster than the enqueued path on both Holstein chains of
// tools/bond_spectra_bench.py, profiles/bond_spectra.md: ahead at 8, 16, 32 and 64 (22x .. 4.6x with 4 phonon levels,
// 16x .. 1.8x with 16), so the limit is all that fits.  (Against calc_bond_entropy the kernels are 17x .. 2.2x ahead
// except at bond 64 with 16 levels, 0.8x: each walk is one workgroup.)  Were the limit below CHAIN_BOND_FIT, chains
// between the two would take the kernels only under MPSE_BOND_SPECTRA_CHAIN=1.
constexpr int64_t BS_BOND_MAX = 64;
static_assert(1 <= BS_BOND_MAX && BS_BOND_MAX <= CHAIN_BOND_FIT, "the limit lies inside what fits");
// Sweep cap of one Jacobi solve.  A safety condition: a solve that reaches it fails the call.  More than twice the
// largest count seen: 13 over tests/test_bond_spectra_gpu.py, 10 over tools/bond_spectra_bench.py (stats slot 4).
constexpr int BS_SWEEP_CAP = 40;
constexpr double BS_EPS = 2.220446049250313e-16;

struct BsSite : ChainSelRow {   // one row of the table (64 bytes): nsite rows, then the rows left of the selected bonds
  // sel (of ChainSelRow): position of the bond RIGHT of this site in the selection, -1: not selected - leave L here
  int rsel;       // position of the bond LEFT of this site in the selection, -1: not selected - leave R here
  int pad;
  int64_t loff;   // working elements before L of the bond right of this site in the pooled buffer; its R at + D D
  int64_t roff;   // working elements before R of the bond left of this site
  int64_t ooff;   // doubles before the weights of the bond right of this site in the result
};
static_assert(sizeof(BsSite) == 64, "descriptor rows are copied as 8-byte words");

struct BsPlan : ChainSelPlan {
  int64_t eig_elems;   // LDS elements of k_bondspec_eig at the largest bond of the table
};

// The sizing of a table that is a chain: that of the walks, and the three regions of k_bondspec_eig, which are the larger
BsPlan bondspec_plan(int nsite, const int64_t* dims, int nsel, bool cplx) {
  BsPlan pl{chain_sel_plan(nsite, dims, nsel >= 1 && nsite >= 2, 0, cplx, BS_BOND_MAX), 0};
  if (pl.fit) {
    pl.eig_elems = 2 * pl.max_bond * chain_pitch(pl.max_bond) + pl.max_bond;
    pl.lds = std::max(pl.lds, pl.eig_elems * (cplx ? 16 : 8));
    if (pl.lds > CHAIN_LDS_MAX) {
      pl.fit = pl.chain = false;
      pl.lds = pl.e_elems = pl.t_elems = pl.eig_elems = 0;
    }
  }
  return pl;
}

template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_bondspec_envs(const BsSite* __restrict__ sites, int nsite, int first,
                                                                 int last, int e_elems, void* pool) {
  walk_envs<CPLX, true>(sites, nsite, first, last, e_elems, pool);
}

// ------------------------------------------------------------------------------------------ the Hermitian eigensolver
__device__ __forceinline__ double bs_abs2(double a) { return a * a; }
__device__ __forceinline__ double bs_abs2(double2 a) { return a.x * a.x + a.y * a.y; }
__device__ __forceinline__ double bs_scale(double a, double f) { return a * f; }
__device__ __forceinline__ double2 bs_scale(double2 a, double f) { return make_double2(a.x * f, a.y * f); }
__device__ __forceinline__ double bs_real(double a) { return a; }
__device__ __forceinline__ double2 bs_real(double2 a) { return make_double2(a.x, 0.0); }
__device__ __forceinline__ bool bs_is_zero(double a) { return a == 0.0; }
__device__ __forceinline__ bool bs_is_zero(double2 a) { return a.x == 0.0 && a.y == 0.0; }

// (x, y) <- (c x - g y, conj(g) x + c y): the rows p, q of J^H A for J = [[c, g], [-conj(g), c]]; with conj(g) in the
// place of g the columns p, q of A J
template <bool CPLX>
__device__ __forceinline__ void bs_rot(ChainT<CPLX>& x, ChainT<CPLX>& y, double c, ChainT<CPLX> g) {
  using El = ChainEl<CPLX>;
  ChainT<CPLX> nx = bs_scale(x, c), ny = bs_scale(y, c);
  El::fma(nx, bs_scale(g, -1.0), y);
  El::fma(ny, El::cj(g), x);
  x = nx, y = ny;
}

// Pair k of step t of the round-robin tournament of n2 players (n2 even): player n2 - 1 stays and meets t, the others
// meet across the circle, (t + k, t - k) mod (n2 - 1).  p < q.  The n2 / 2 pairs of a step are disjoint, and over the
// n2 - 1 steps every pair meets once.  For an odd matrix n2 = D + 1 and player D is the bye: q == D, always pair 0.
__device__ __forceinline__ void bs_pair(int k, int t, int n2, int* p, int* q) {
  const int m = n2 - 1;
  int a = m, b = t;
  if (k > 0) {
    a = t + k;
    a = a >= m ? a - m : a;
    b = t - k;
    b = b < 0 ? b + m : b;
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

// the rotation of pair k from the strip; the bye of an odd matrix has no slot and is the identity
template <bool CPLX>
__device__ __forceinline__ void bs_rot_of(const double* rot, int k, int odd, bool live, double* c, ChainT<CPLX>* g) {
  constexpr int RS = CPLX ? 3 : 2;
  *c = 1.0;
  *g = ChainEl<CPLX>::zero();
  if (!live) return;
  const double* r = rot + RS * (k - odd);
  *c = r[0];
  if constexpr (CPLX) *g = make_double2(r[1], r[2]);
  else *g = r[1];
}

// Cyclic two-sided Jacobi for the Hermitian D x D matrix A in LDS (rows of chain_pitch(D)); VECS: V <- the eigenvectors
// as columns (A_in = V diag V^H), else V is not touched.  On return the diagonal of A holds the eigenvalues and what is
// left off it is below the thresholds.  One sweep is the n2 - 1 steps of the round-robin ordering; the rotations of a
// step are disjoint: first one thread per pair decides and leaves (c, sigma) in the strip `rot`, then every 2 x 2 block
// (pair of rows) x (pair of columns) is J_P^H . block . J_Q by one thread, and the columns of V follow.  A pair is
// rotated unless |a_pq|^2 <= eps^2 |a_pp a_qq| or |a_pq|^2 <= (eps |A|_F / D)^2 (so that zero and rank-deficient
// matrices stop; NaN rotates and runs into the cap).  The solve ends with the first sweep that rotates nothing: the
// decision is taken here, by every thread from the same LDS word.  Returns the number of sweeps, that one included, or
// -1 at the cap; the same value in every thread.  Ends with a barrier.
template <bool CPLX, bool VECS>
__device__ int bs_jacobi(int D, ChainT<CPLX>* A, ChainT<CPLX>* V, double* rot, int* flag, double* red) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  constexpr int RS = CPLX ? 3 : 2;
  const int pitch = D | 1, odd = D & 1, n2 = D + odd, npairs = n2 / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double part = 0.0;
  for (int o = tid; o < D * D; o += CHAIN_THREADS) {
    const int r = o / D, c = o - r * D;
    part += bs_abs2(A[r * pitch + c]);
    if constexpr (VECS) V[r * pitch + c] = r == c ? El::one() : El::zero();
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if (lane == 0) red[wave] = part;
  if (tid == 0) *flag = 0;
  __syncthreads();
  double nrm2 = 0.0;
  for (int w = 0; w < CHAIN_WAVES; ++w) nrm2 += red[w];
  const double eps2 = BS_EPS * BS_EPS, floor2 = nrm2 * eps2 / ((double)D * (double)D);
  for (int sweep = 1; sweep <= BS_SWEEP_CAP; ++sweep) {
    for (int t = 0; t < n2 - 1; ++t) {
      if (tid < npairs) {
        int p, q;
        bs_pair(tid, t, n2, &p, &q);
        if (q < D) {
          const double app = El::re(A[p * pitch + p]), aqq = El::re(A[q * pitch + q]);
          const T apq = A[p * pitch + q];
          const double g2 = bs_abs2(apq);
          double c = 1.0;
          T g = El::zero();
          if (!(g2 <= floor2) && !(g2 <= eps2 * fabs(app * aqq))) {
            const double ga = sqrt(g2), tau = (aqq - app) / (2.0 * ga);
            const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + tt * tt);
            g = bs_scale(apq, tt * c / ga);
            *flag = 1;
          }
          double* r = rot + RS * (tid - odd);
          r[0] = c;
          r[1] = El::re(g);
          if constexpr (CPLX) r[2] = El::im(g);
        }
      }
      __syncthreads();
      for (int it = tid; it < npairs * npairs; it += CHAIN_THREADS) {
        const int P = it / npairs, Q = it - P * npairs;
        int p, q, p2, q2;
        bs_pair(P, t, n2, &p, &q);
        bs_pair(Q, t, n2, &p2, &q2);
        const bool lp = q < D, lq = q2 < D;
        double cp, cq;
        T gp, gq;
        bs_rot_of<CPLX>(rot, P, odd, lp, &cp, &gp);
        bs_rot_of<CPLX>(rot, Q, odd, lq, &cq, &gq);
        if (bs_is_zero(gp) && bs_is_zero(gq)) continue;   // both the identity (c = 1 with sigma = 0)
        T x00 = A[p * pitch + p2], x01 = lq ? A[p * pitch + q2] : El::zero();
        T x10 = lp ? A[q * pitch + p2] : El::zero(), x11 = lp && lq ? A[q * pitch + q2] : El::zero();
        bs_rot<CPLX>(x00, x01, cq, El::cj(gq));   // columns
        bs_rot<CPLX>(x10, x11, cq, El::cj(gq));
        bs_rot<CPLX>(x00, x10, cp, gp);           // rows
        bs_rot<CPLX>(x01, x11, cp, gp);
        if (P == Q) {   // the rotated pair itself: what the rotation annihilates is zero, the diagonal real
          x01 = x10 = El::zero();
          x00 = bs_real(x00), x11 = bs_real(x11);
        }
        A[p * pitch + p2] = x00;
        if (lq) A[p * pitch + q2] = x01;
        if (lp) A[q * pitch + p2] = x10;
        if (lp && lq) A[q * pitch + q2] = x11;
      }
      if constexpr (VECS) {
        for (int it = tid; it < D * npairs; it += CHAIN_THREADS) {
          const int r = it / npairs, Q = it - r * npairs;
          int p2, q2;
          bs_pair(Q, t, n2, &p2, &q2);
          if (q2 >= D) continue;
          double cq;
          T gq;
          bs_rot_of<CPLX>(rot, Q, odd, true, &cq, &gq);
          if (bs_is_zero(gq)) continue;
          T x = V[r * pitch + p2], y = V[r * pitch + q2];
          bs_rot<CPLX>(x, y, cq, El::cj(gq));
          V[r * pitch + p2] = x;
          V[r * pitch + q2] = y;
        }
      }
      __syncthreads();
    }
    const int rotated = *flag;
    __syncthreads();
    if (tid == 0) *flag = 0;
    __syncthreads();
    if (!rotated) return sweep;
  }
  return -1;
}

// the Hermitian part of the D D packed elements at P into the padded rows of A; ends with the barrier behind which A is
// read
template <bool CPLX>
__device__ __forceinline__ void bs_load_herm(const ChainT<CPLX>* P, int D, ChainT<CPLX>* A) {
  using El = ChainEl<CPLX>;
  const int pitch = D | 1;
  for (int o = threadIdx.x; o < D * D; o += CHAIN_THREADS) {
    const int r = o / D, c = o - r * D;
    ChainT<CPLX> v = P[o];
    El::add(v, El::cj(P[c * D + r]));
    A[r * pitch + c] = bs_scale(v, 0.5);
  }
  __syncthreads();
}

// Workgroup k takes the selected bond k (row nsite + k of the table: the site left of it).  L into A; first solve with
// the vectors; Lambda^(1/2) (negative rounding noise of Lambda as 0) into the strip; W = R^T U into A; M entry by entry
// to where L was in pooled memory and back as its Hermitian part; second solve, values only; clamped at 0, ranked in
// descending order (ties by index) and written.  sweeps[2 k], [2 k + 1]: the sweeps of the two solves, -1 at the cap.
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_bondspec_eig(const BsSite* __restrict__ sites, int nsite, void* pool,
                                                                double* __restrict__ out, double* __restrict__ sweeps) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double bs_lds[];
  __shared__ int flag;
  __shared__ double red[CHAIN_WAVES];
  const BsSite s = sites[nsite + blockIdx.x];
  const int D = s.Dr, pitch = D | 1, nA = D * pitch, tid = threadIdx.x;
  T* A = reinterpret_cast<T*>(bs_lds);
  T* V = A + nA;
  double* strip = reinterpret_cast<double*>(V + nA);
  T* Lp = static_cast<T*>(pool) + s.loff;
  const T* Rp = Lp + D * D;
  bs_load_herm<CPLX>(Lp, D, A);
  const int sw1 = bs_jacobi<CPLX, true>(D, A, V, strip, &flag, red);
  for (int i = tid; i < D; i += CHAIN_THREADS) {
    const double lam = El::re(A[i * pitch + i]);
    strip[i] = lam > 0.0 ? sqrt(lam) : 0.0;
  }
  __syncthreads();
  for (int o = tid; o < D * D; o += CHAIN_THREADS) {
    const int a = o / D, j = o - a * D;
    T sum = El::zero();
#pragma unroll 4
    for (int b = 0; b < D; ++b) El::fma(sum, Rp[b * D + a], V[b * pitch + j]);
    A[a * pitch + j] = sum;
  }
  __syncthreads();
  for (int o = tid; o < D * D; o += CHAIN_THREADS) {
    const int i = o / D, j = o - i * D;
    T sum = El::zero();
#pragma unroll 4
    for (int a = 0; a < D; ++a) El::fma(sum, El::cj(V[a * pitch + i]), A[a * pitch + j]);
    Lp[o] = bs_scale(sum, strip[i] * strip[j]);
  }
  __syncthreads();   // M is complete in pooled memory, every read of W and of Lambda is done
  bs_load_herm<CPLX>(Lp, D, A);
  const int sw2 = bs_jacobi<CPLX, false>(D, A, V, strip, &flag, red);
  for (int i = tid; i < D; i += CHAIN_THREADS) {
    const double w = El::re(A[i * pitch + i]);
    strip[i] = w > 0.0 ? w : 0.0;
  }
  __syncthreads();
  for (int i = tid; i < D; i += CHAIN_THREADS) {
    const double w = strip[i];
    int rank = 0;
    for (int j = 0; j < D; ++j) rank += (strip[j] > w || (strip[j] == w && j < i)) ? 1 : 0;
    out[s.ooff + rank] = w;
  }
  if (tid == 0) {
    sweeps[2 * blockIdx.x] = sw1;
    sweeps[2 * blockIdx.x + 1] = sw2;
  }
}

int bondspec_chain(mpse_ctx* ctx, const ChainSelArgs& a, bool cplx, const BsPlan& pl, int64_t n_out, double* out_host) {
  std::vector<BsSite> rows((size_t)a.nsite + a.nsel);
  for (int i = 0; i < a.nsite; ++i) rows[i] = BsSite{chain_sel_row(a, i, -1), -1, 0, 0, 0, 0};
  int64_t e_elems = 0, o_elems = 0;
  for (int j = 0; j < a.nsel; ++j) {
    const int k = a.sel[j];
    const int64_t D = a.dims[4 * k + 3];
    rows[k].sel = j, rows[k].loff = e_elems, rows[k].ooff = o_elems;
    rows[k + 1].rsel = j, rows[k + 1].roff = e_elems + D * D;
    e_elems += 2 * D * D;
    o_elems += D;
  }
  for (int j = 0; j < a.nsel; ++j) rows[(size_t)a.nsite + j] = rows[a.sel[j]];
  // the eig kernel has a few words of static LDS next to its regions
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_bondspec_envs)}, CHAIN_LDS_MAX));
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_bondspec_eig)}, CHAIN_LDS_MAX - 1024));
  const size_t es = cplx ? 16 : 8, n_res = (size_t)n_out + 2 * (size_t)a.nsel;
  TmpBuf tab(ctx), pool(ctx), res(ctx);
  MPSE_TRY(chain_stage_rows(ctx, tab, rows));
  MPSE_TRY(pool.alloc((size_t)e_elems * es));
  MPSE_TRY(res.alloc(n_res * sizeof(double)));
  CHAIN_LAUNCH(ctx, cplx, k_bondspec_envs, 2, (pl.e_elems + pl.t_elems) * (int64_t)es, tab.as<const BsSite>(), a.nsite,
               a.sel[0], a.sel[a.nsel - 1], (int)pl.e_elems, pool.p);
  CHAIN_LAUNCH(ctx, cplx, k_bondspec_eig, a.nsel, pl.eig_elems * (int64_t)es, tab.as<const BsSite>(), a.nsite, pool.p,
               res.as<double>(), res.as<double>() + n_out);
  MPSE_HIP(ctx, hipGetLastError());
  std::vector<double> host(n_res);
  MPSE_TRY(mpse_memcpy_d2h(ctx, host.data(), res.p, n_res * sizeof(double)));
  long long top = 0;
  for (int j = 0; j < a.nsel; ++j)
    for (int w = 0; w < 2; ++w) {
      const long long sw = (long long)host[(size_t)n_out + 2 * j + w];
      if (sw < 1)
        return mpse_fail(ctx, MPSE_ERR_NOCONV, "mps_bond_spectra: the Jacobi solve of %s at bond %d did not end in %d sweeps",
                         w ? "M" : "L", a.sel[j], BS_SWEEP_CAP);
      top = std::max(top, sw);
    }
  ctx->bondspec_stats[mpse_ctx::BS_MAX_SWEEPS] = std::max(ctx->bondspec_stats[mpse_ctx::BS_MAX_SWEEPS], top);
  memcpy(out_host, host.data(), (size_t)n_out * sizeof(double));
  return MPSE_OK;
}

// The eigenvalues of the Hermitian positive semidefinite D x D matrix at `mat` as its singular values (descending) into
// s_host, the left vectors into U (D x D); one dense block.  Synchronous (mpse_block_svd reads the values).
int bs_psd_svd(mpse_ctx* ctx, int dt, int64_t D, const void* mat, void* U, void* Vt, double* s_host) {
  std::vector<int64_t> idx((size_t)D);
  for (int64_t i = 0; i < D; ++i) idx[i] = i;
  const int64_t off[2] = {0, D};
  return mpse_block_svd(ctx, dt, mat, D, D, 1, idx.data(), off, idx.data(), off, U, Vt, s_host, D);
}

// The same two passes as products of the contraction kernel in one dtype (ChainSelEnq; the passes of rdm1_enqueued), L
// and R of the selected bonds into pooled buffers, then per selected bond:
//   L = U S V^H (block SVD)          US[b, j] = U[b, j] sqrt(S_j) (column gather with a scale)
//   T1[a, j] = sum_b R[b, a] US[b, j]          M[i, j] = sum_a conj(US[a, i]) T1[a, j]          p = the singular values of M
int bondspec_enqueued(mpse_ctx* ctx, const ChainSelArgs& a, bool cplx, double* out_host) {
  ChainSelEnq q(ctx, cplx);
  MPSE_TRY(q.init(a));   // pos[k] >= 0: the bond right of site k is selected
  const size_t es = q.es;
  const int nsel = a.nsel, first = a.sel[0], last = a.sel[nsel - 1];
  int64_t b_elems = 0, d_max = 1;
  std::vector<int64_t> boff((size_t)nsel), ooff((size_t)nsel);
  int64_t o_elems = 0;
  for (int k = 0; k < nsel; ++k) {
    const int64_t D = a.dims[4 * a.sel[k] + 3];
    boff[k] = b_elems, ooff[k] = o_elems;
    b_elems += D * D;
    o_elems += D;
    d_max = std::max(d_max, D);
  }
  TmpBuf lbuf(ctx), rbuf(ctx), e0(ctx), e1(ctx), x1(ctx), u(ctx), vt(ctx), us(ctx), t1(ctx), m(ctx);
  MPSE_TRY(q.alloc({{&lbuf, b_elems}, {&rbuf, b_elems}, {&e0, q.e_max}, {&e1, q.e_max}, {&x1, q.x_max},
                    {&u, d_max * d_max}, {&vt, d_max * d_max}, {&us, d_max * d_max}, {&t1, d_max * d_max},
                    {&m, d_max * d_max}}));
  const double one[2] = {1.0, 0.0};
  void* scratch[2] = {e0.p, e1.p};
  auto at = [&](TmpBuf& buf, int bond) -> void* {   // where the environment of bond `bond` lives
    return bond >= 0 && bond < a.nsite - 1 && q.pos[bond] >= 0
               ? static_cast<char*>(buf.p) + (size_t)boff[q.pos[bond]] * es
               : scratch[bond & 1];
  };
  // ---- right pass: R of bond i - 1 from R of bond i and site i
  MPSE_TRY(stage_h2d(ctx, at(rbuf, a.nsite - 1), one, es));
  for (int i = a.nsite - 1; i > first; --i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], p = d[1] * d[2], Dr = d[3];
    MPSE_TRY(q.a_r(Dl * p, Dr, Dr, q.site[i], at(rbuf, i), x1.p));
    MPSE_TRY(q.ca_y(Dl, Dl, p * Dr, q.site[i], x1.p, at(rbuf, i - 1)));
  }
  // ---- left pass: L of bond i from L of bond i - 1 and site i (bond -1 shares the parity of bond 1: scratch[1])
  MPSE_TRY(stage_h2d(ctx, scratch[1], one, es));
  for (int i = 0; i <= last; ++i) {
    const int64_t* d = a.dims + 4 * i;
    const int64_t Dl = d[0], p = d[1] * d[2], Dr = d[3];
    const void* L = i == 0 ? scratch[1] : at(lbuf, i - 1);
    MPSE_TRY(q.l_a(1, Dl, Dl, p * Dr, L, q.site[i], x1.p));
    MPSE_TRY(q.ca_x(1, Dl * p, Dr, Dr, q.site[i], x1.p, at(lbuf, i)));
  }
  // ---- the two solves of every selected bond
  std::vector<double> s_host((size_t)d_max), root((size_t)d_max);
  std::vector<int64_t> cols((size_t)d_max);
  for (int64_t i = 0; i < d_max; ++i) cols[i] = i;
  for (int k = 0; k < nsel; ++k) {
    const int64_t D = a.dims[4 * a.sel[k] + 3];
    const void* L = at(lbuf, a.sel[k]);
    const void* R = at(rbuf, a.sel[k]);
    MPSE_TRY(bs_psd_svd(ctx, q.dt, D, L, u.p, vt.p, s_host.data()));
    for (int64_t i = 0; i < D; ++i) root[i] = s_host[i] > 0.0 ? sqrt(s_host[i]) : 0.0;
    MPSE_TRY(mpse_gather_cols(ctx, q.dt, us.p, u.p, D, D, cols.data(), root.data(), D));
    MPSE_TRY(q.gemm(0, idx1(D, 1), idx1(D, D), idx1(D, D), idx1(D, 1), idx1(D, D), idx1(D, 1), 1, 0, 0, 0, R, us.p,
                    t1.p));
    MPSE_TRY(q.ca_x(1, D, D, D, us.p, t1.p, m.p));
    MPSE_TRY(bs_psd_svd(ctx, q.dt, D, m.p, u.p, vt.p, s_host.data()));
    for (int64_t i = 0; i < D; ++i) out_host[ooff[k] + i] = s_host[i] > 0.0 ? s_host[i] : 0.0;
  }
  return MPSE_OK;
}

}  // namespace

extern "C" {

int mpse_mps_bond_spectra_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n) {
  const bool valid = chain_sel_table_ok(nsite, dims);
  const BsPlan pl = valid ? bondspec_plan(nsite, dims, nsel, any_complex != 0) : BsPlan{};
  return chain_sel_plan_out(pl, valid, BS_BOND_MAX, 0, {pl.eig_elems, BS_SWEEP_CAP}, info, n);
}

int mpse_mps_bond_spectra_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::bondspec_stats, counts, n);
}

int mpse_mps_bond_spectra(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims,
                          int nsel, const int* sel, double* out_host) {
  const ChainSelArgs args{nsite, sites, dtype, dims, nsel, sel};
  bool cplx = false;
  if (ctx && nsite == 1) return mpse_fail(ctx, MPSE_ERR_ARG, "mps_bond_spectra: a chain of one site has no bond");
  MPSE_TRY(chain_sel_prologue(ctx, "mps_bond_spectra", args, 1, out_host != nullptr, &cplx, nsite - 1));
  BsPlan pl = bondspec_plan(nsite, dims, nsel, cplx);
  MPSE_BIND(ctx);
  chain_sel_plan_switch("MPSE_BOND_SPECTRA_CHAIN", &pl);
  int64_t n_out = 0;
  for (int k = 0; k < nsel; ++k) n_out += dims[4 * sel[k] + 3];
  std::vector<double> res((size_t)n_out, 0.0);
  if (pl.chain)
    MPSE_TRY(bondspec_chain(ctx, args, cplx, pl, n_out, res.data()));
  else
    MPSE_TRY(bondspec_enqueued(ctx, args, cplx, res.data()));
  return chain_sel_done(ctx->bondspec_stats, pl.chain, nsite, nsel, res, out_host);
}

}  // extern "C"
