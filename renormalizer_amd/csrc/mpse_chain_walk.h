// What the chain calls with a selection share beyond mpse_chain.h (mpse_corr.hip, mpse_rdm2.hip, mpse_bondspec.hip and
// mpse_expect.hip include this; mpse_rdm1.hip and mpse_trdm1.hip through mpse_chain_sites.h, which adds the call those
// two share; no other file includes either).  Five of them take dims rows (D_l, d, danc, D_r) of ONE chain, which is
// its own conjugated bra, and a strictly ascending selection (of bonds in mpse_bondspec.hip, of windows in
// mpse_expect.hip); mpse_trdm1.hip takes rows (Db_l, Dk_l, d, danc, Db_r, Dk_r) of a bra and a ket that differ, with
// rectangular environments.  All walk with the identity transfer matrix: the environment in LDS, one (sigma, ancilla)
// slice of a site at a time.  Everything here is written once, for two chains; ONE chain is the case of equal bonds
// and B = K, decided while compiling on the device side and by the dims table on the host side.  Here are
//   device   the two stages of the transfer per direction (walk_right_slice, walk_right_sum with walk_right_dot,
//            walk_left_slice, walk_left_sum), the owners' accumulators (walk_acc_zero / _add / _store), the moves of an
//            environment between LDS and pooled memory (walk_env_to_pool / _from_pool), walk_env_dot, the two sums over
//            a wave and over the workgroup; on them one site of a walk that only carries an environment on (walk_site),
//            the two walks that leave environments at selected sites or at selected bonds (walk_left, walk_right) and
//            the body of the *_envs kernels with a grid of two (walk_envs)
//   host     the sizing of the launches (chain_sel_plan), the checks of the entry points (chain_sel_prologue), the tail
//            of an entry point and of a *_plan export, and what the enqueued passes share (ChainSelEnq)
// A call keeps its descriptor row and what it does with the sums; the walks of mpse_corr.hip and rd2_walk_right of
// mpse_rdm2.hip, which accumulate several environments per slice, keep their loop over the slices as well.  In all six a
// workgroup reads only what the launch before it wrote (no flag, no spin wait, no atomic), the host reads once, at the
// end, and the order of every sum is fixed: the same inputs give the same bits.
#pragma once
#include <type_traits>

#include "mpse_chain.h"

constexpr int CHAIN_WAVES = CHAIN_THREADS / 64;
constexpr int CHAIN_OUT_PER_THREAD = 4;   // entries of a new environment a thread accumulates in registers

// --------------------------------------------------------------------------------------------------------- device side
// A descriptor row `Row` starts with ChainSelRow (ONE chain, which is its own conjugated bra) or with Chain2Row (a bra B
// (Db_l, d, danc, Db_r) and a ket K (Dk_l, d, danc, Dk_r) that differ).  The stages below are written once, for two
// chains, and reach the row through the accessors walk_Dbl .. walk_Dkr, walk_ld_ket and walk_ld_bra: for ONE chain Db =
// Dk, B = K and op(B) is the conjugate, decided while compiling.  (The accessors are functions called where a value is
// used, not one struct of the four bonds filled per site: that changed the code of the walks,
// profiles/chain_walk_refactor.md.)  An environment at a bond is Db rows of chain_pitch(Dk) elements in LDS, bra index
// first.  `krow` / `brow`: the elements of K / B per index of its left bond, d danc Dk_r / d danc Db_r, computed once
// per site by the kernel; a slice of a site is named by the elements before it in such a row, `ket` = (sigma danc + a)
// Dk_r in K and `bra` = (sigma danc + a) Db_r in B.  Every sum runs over its inner index in ascending order.
struct ChainSelRow {   // what a descriptor row of a call on one chain begins with (32 bytes)
  const void* a;
  int Dl, d, danc, Dr;
  int cplx;            // the tensor is complex128
  int sel;             // position in the selection, -1: not selected
};
struct Chain2Row {   // what a descriptor row of a two-chain call begins with (56 bytes)
  const void* bra;
  const void* ket;
  int Dbl, Dkl, d, danc, Dbr, Dkr;
  int bra_c, ket_c;    // the side's tensor is complex128
  int bra_cj;          // conjugate the bra tensor: the call conjugates the bra and this tensor is complex
  int sel;             // position in the selection, -1: not selected
};

template <class Row>
constexpr bool walk_two_chains = std::is_base_of<Chain2Row, Row>::value;
// the four bonds of a site
template <class Row>
__device__ __forceinline__ int walk_Dbl(const Row& s) {
  if constexpr (walk_two_chains<Row>) return s.Dbl;
  else return s.Dl;
}
template <class Row>
__device__ __forceinline__ int walk_Dkl(const Row& s) {
  if constexpr (walk_two_chains<Row>) return s.Dkl;
  else return s.Dl;
}
template <class Row>
__device__ __forceinline__ int walk_Dbr(const Row& s) {
  if constexpr (walk_two_chains<Row>) return s.Dbr;
  else return s.Dr;
}
template <class Row>
__device__ __forceinline__ int walk_Dkr(const Row& s) {
  if constexpr (walk_two_chains<Row>) return s.Dkr;
  else return s.Dr;
}
template <bool CPLX, class Row>
__device__ __forceinline__ ChainT<CPLX> walk_ld_ket(const Row& s, int i) {
  if constexpr (walk_two_chains<Row>) return ChainEl<CPLX>::ld(s.ket, s.ket_c, i);
  else return ChainEl<CPLX>::ld(s.a, s.cplx, i);
}
template <bool CPLX, class Row>
__device__ __forceinline__ ChainT<CPLX> walk_ld_bra(const Row& s, int i) {   // op(B)
  if constexpr (walk_two_chains<Row>) {
    const ChainT<CPLX> v = ChainEl<CPLX>::ld(s.bra, s.bra_c, i);
    return s.bra_cj ? ChainEl<CPLX>::cj(v) : v;
  } else {
    return ChainEl<CPLX>::cj(ChainEl<CPLX>::ld(s.a, s.cplx, i));
  }
}

// the identity environment of the bond 1 at either end
template <bool CPLX>
__device__ __forceinline__ void walk_env_one(ChainT<CPLX>* E) {
  if (threadIdx.x == 0) E[0] = ChainEl<CPLX>::one();
  __syncthreads();
}

// Rightwards (the walk from the right), first stage: T[k, b'] = sum_k' K[k, ket, k'] R[b', k'] into LDS, R with rows of
// chain_pitch(Dk_r), T (Dk_l rows) with rows of chain_pitch(Db_r); ends with the barrier behind which T is read
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_right_slice(const Row& s, int krow, int ket, const ChainT<CPLX>* R,
                                                 ChainT<CPLX>* Ts) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int Dbr = walk_Dbr(s), Dkr = walk_Dkr(s), pr = Dkr | 1, pt = Dbr | 1, nT = walk_Dkl(s) * Dbr;
  for (int o = threadIdx.x; o < nT; o += CHAIN_THREADS) {
    const int k = o / Dbr, bp = o - k * Dbr;
    const T* r_row = R + bp * pr;
    const int k0 = k * krow + ket;
    T sum = El::zero();
#pragma unroll 4
    for (int kp = 0; kp < Dkr; ++kp) El::fma(sum, walk_ld_ket<CPLX>(s, k0 + kp), r_row[kp]);
    Ts[k * pt + bp] = sum;
  }
  __syncthreads();
}

// Rightwards, second stage: S = sum_b' op(B[b, bra, b']) T[k, b'] of the entry o = b Dk_l + k of the new environment
// (Db_l x Dk_l).  Owners take o = tid + j * CHAIN_THREADS: B[b, ..] is one address per b group, the reads of T run down
// a column of padded rows.  walk_right_dot is the sum itself, for rd2_walk_right, which meets an owned entry with d bra
// slices and takes (b, k) once.  S leaves through a reference and `brow` comes from the kernel on purpose:
// DESIGN_HISTORY.md.
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_right_dot(const Row& s, int b0, const ChainT<CPLX>* t_row, ChainT<CPLX>& S) {
  using El = ChainEl<CPLX>;
  const int Dbr = walk_Dbr(s);
  S = El::zero();
#pragma unroll 4
  for (int bp = 0; bp < Dbr; ++bp) El::fma(S, walk_ld_bra<CPLX>(s, b0 + bp), t_row[bp]);
}
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_right_sum(const Row& s, int brow, int bra, int o, const ChainT<CPLX>* Ts,
                                               ChainT<CPLX>& S) {
  const int b = o / walk_Dkl(s), k = o - b * walk_Dkl(s);
  walk_right_dot<CPLX>(s, b * brow + bra, Ts + k * (walk_Dbr(s) | 1), S);
}

// Leftwards (the walk from the left), first stage: T[b, k'] = sum_k E[b, k] K[k, ket, k'] with rows of E `pe` and rows
// of T `pt` elements apart (the walks: E padded in LDS, T packed; chain_close_site: E packed in pooled memory, T
// padded); ends with the barrier behind which T is read
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_left_slice(const Row& s, int krow, int ket, const ChainT<CPLX>* E, int pe,
                                                ChainT<CPLX>* Ts, int pt) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int Dkl = walk_Dkl(s), Dkr = walk_Dkr(s), nT = walk_Dbl(s) * Dkr;
  for (int o = threadIdx.x; o < nT; o += CHAIN_THREADS) {
    const int b = o / Dkr, kk = o - b * Dkr;
    const T* e_row = E + b * pe;
    const int k0 = ket + kk;
    T sum = El::zero();
#pragma unroll 4
    for (int k = 0; k < Dkl; ++k) El::fma(sum, e_row[k], walk_ld_ket<CPLX>(s, k * krow + k0));
    Ts[b * pt + kk] = sum;
  }
  __syncthreads();
}

// Leftwards, second stage: S = sum_b op(B[b, bra, b']) T[b, k'] of the entry o = b' Dk_r + k' of the new environment
// (Db_r x Dk_r), T packed.  Owners take o = tid + j * CHAIN_THREADS, k' fastest.
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_left_sum(const Row& s, int brow, int bra, int o, const ChainT<CPLX>* Ts,
                                              ChainT<CPLX>& S) {
  using El = ChainEl<CPLX>;
  const int Dbl = walk_Dbl(s), Dkr = walk_Dkr(s);
  const int bb = o / Dkr, kk = o - bb * Dkr;
  const int b0 = bra + bb;
  S = El::zero();
#pragma unroll 4
  for (int b = 0; b < Dbl; ++b) El::fma(S, walk_ld_bra<CPLX>(s, b * brow + b0), Ts[b * Dkr + kk]);
}

// acc[j] += S of the owned entries o < n against ONE bra slice, S summed first: the walks that only carry an
// environment on
template <bool CPLX, bool LEFT, class Row>
__device__ __forceinline__ void walk_acc_add(const Row& s, int row, int bra, const ChainT<CPLX>* Ts, int n,
                                             ChainT<CPLX> (&acc)[CHAIN_OUT_PER_THREAD]) {
#pragma unroll
  for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) {
    const int o = threadIdx.x + j * CHAIN_THREADS;
    if (o < n) {
      ChainT<CPLX> S;
      if constexpr (LEFT) walk_left_sum<CPLX>(s, row, bra, o, Ts, S);
      else walk_right_sum<CPLX>(s, row, bra, o, Ts, S);
      ChainEl<CPLX>::add(acc[j], S);
    }
  }
}

template <bool CPLX>
__device__ __forceinline__ void walk_acc_zero(ChainT<CPLX> (&acc)[CHAIN_OUT_PER_THREAD]) {
#pragma unroll
  for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) acc[j] = ChainEl<CPLX>::zero();
}

// The accumulators of the owners become the rows x cols environment in LDS.  The caller has passed the barrier behind
// the last slice, so every read of the old environment is done; ends with the barrier behind which the new one is read.
template <bool CPLX>
__device__ __forceinline__ void walk_acc_store(const ChainT<CPLX> (&acc)[CHAIN_OUT_PER_THREAD], int rows, int cols,
                                               ChainT<CPLX>* E) {
  const int pitch = cols | 1;
#pragma unroll
  for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) {
    const int o = threadIdx.x + j * CHAIN_THREADS;
    if (o < rows * cols) {
      const int r = o / cols, c = o - r * cols;
      E[r * pitch + c] = acc[j];
    }
  }
  __syncthreads();
}

// the rows x cols environment in LDS to rows cols packed elements of pooled memory, as it is or transposed (cols x rows)
template <bool CPLX, bool TRANSPOSED>
__device__ __forceinline__ void walk_env_to_pool(const ChainT<CPLX>* E, int rows, int cols, ChainT<CPLX>* P) {
  const int pitch = cols | 1;
  for (int o = threadIdx.x; o < rows * cols; o += CHAIN_THREADS) {
    int r, c;
    if (TRANSPOSED) c = o / rows, r = o - c * rows;
    else r = o / cols, c = o - r * cols;
    P[o] = E[r * pitch + c];
  }
}

// and back; ends with the barrier behind which the environment is read
template <bool CPLX>
__device__ __forceinline__ void walk_env_from_pool(const ChainT<CPLX>* P, int D, ChainT<CPLX>* E) {
  const int pitch = D | 1;
  for (int o = threadIdx.x; o < D * D; o += CHAIN_THREADS) {
    const int r = o / D, c = o - r * D;
    E[r * pitch + c] = P[o];
  }
  __syncthreads();
}

// the share of one thread in sum_o E[o] G[o], E of bond D in LDS, G packed: o = first, first + step, ..
template <bool CPLX>
__device__ __forceinline__ ChainT<CPLX> walk_env_dot(const ChainT<CPLX>* E, int D, const ChainT<CPLX>* G, int first,
                                                     int step) {
  using El = ChainEl<CPLX>;
  const int pitch = D | 1;
  ChainT<CPLX> part = El::zero();
  for (int o = first; o < D * D; o += step) {
    const int r = o / D, c = o - r * D;
    El::fma(part, E[r * pitch + c], G[o]);
  }
  return part;
}

// sum over the lanes of a wave, down the shuffle tree 32 .. 1; the value is valid in lane 0
template <bool CPLX>
__device__ __forceinline__ ChainT<CPLX> walk_wave_sum(ChainT<CPLX> v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ChainEl<CPLX>::add(v, ChainEl<CPLX>::shfl_down(v, off));
  return v;
}

// One site of a walk that only carries an environment on.  From the left: E (Db_l x Dk_l) in LDS becomes E' (Db_r x
// Dk_r): per (sigma, a) in ascending order T = E . K[sigma, a] into LDS, E' += op(B[sigma, a])^T . T in the owner's
// registers; E' replaces E in LDS after the last (sigma, a).  From the right: R (Db_r x Dk_r) becomes R' (Db_l x Dk_l)
// through T = K[sigma, a] . R^T and R' += op(B[sigma, a]) . T^T.
template <bool CPLX, bool LEFT, class Row>
__device__ __forceinline__ void walk_site(const Row& s, ChainT<CPLX>* E, ChainT<CPLX>* Ts) {
  const int p = s.d * s.danc, krow = p * walk_Dkr(s), brow = p * walk_Dbr(s);
  const int rows = LEFT ? walk_Dbr(s) : walk_Dbl(s), cols = LEFT ? walk_Dkr(s) : walk_Dkl(s);
  ChainT<CPLX> acc[CHAIN_OUT_PER_THREAD];
  walk_acc_zero<CPLX>(acc);
  for (int sa = 0; sa < p; ++sa) {
    if constexpr (LEFT) walk_left_slice<CPLX>(s, krow, sa * walk_Dkr(s), E, walk_Dkl(s) | 1, Ts, walk_Dkr(s));
    else walk_right_slice<CPLX>(s, krow, sa * walk_Dkr(s), E, Ts);
    walk_acc_add<CPLX, LEFT>(s, brow, sa * walk_Dbr(s), Ts, rows * cols, acc);
    __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of E is done as well
  }
  walk_acc_store<CPLX>(acc, rows, cols, E);
}

// The two walks that leave environments in pooled memory; E_0 = 1 resp. R behind the last site = 1.  AT_BOND says where:
//   false  at a selected SITE (`sel` >= 0), before its transfer: L as it is at `eoff` working elements of `pool`, R
//          transposed behind it, at eoff + Db_l Dk_l (chain_close_site reads it along the lanes).  The walk ends AT site
//          `last` resp. `first`, whose transfer is not taken.  (k_rdm1_envs, k_trdm1_envs; from the left k_rdm2_envs)
//   true   at a selected BOND, after the transfer of the site next to it, as it is: L of the bond right of a site with
//          `sel` >= 0 at `loff`, R of the bond left of a site with `rsel` >= 0 at `roff`.  The walk ends behind site
//          `last`, the one left of the last selected bond, resp. `first`, the one left of the first selected bond, whose
//          transfer is not taken.  (k_bondspec_envs, k_expect_envs)
template <bool CPLX, bool AT_BOND, class Row>
__device__ void walk_left(const Row* __restrict__ sites, int last, ChainT<CPLX>* E, ChainT<CPLX>* Ts,
                          ChainT<CPLX>* pool) {
  walk_env_one<CPLX>(E);
  for (int i = 0; i <= last; ++i) {
    const Row s = sites[i];
    if constexpr (!AT_BOND) {
      if (s.sel >= 0) walk_env_to_pool<CPLX, false>(E, walk_Dbl(s), walk_Dkl(s), pool + s.eoff);
      if (i == last) break;
    }
    walk_site<CPLX, true>(s, E, Ts);
    if constexpr (AT_BOND)
      if (s.sel >= 0) walk_env_to_pool<CPLX, false>(E, walk_Dbr(s), walk_Dkr(s), pool + s.loff);
  }
}
template <bool CPLX, bool AT_BOND, class Row>
__device__ void walk_right(const Row* __restrict__ sites, int nsite, int first, ChainT<CPLX>* R, ChainT<CPLX>* Ts,
                           ChainT<CPLX>* pool) {
  walk_env_one<CPLX>(R);
  for (int i = nsite - 1; AT_BOND ? i > first : i >= first; --i) {
    const Row s = sites[i];
    if constexpr (!AT_BOND) {
      if (s.sel >= 0)
        walk_env_to_pool<CPLX, true>(R, walk_Dbr(s), walk_Dkr(s), pool + s.eoff + walk_Dbl(s) * walk_Dkl(s));
      if (i == first) break;
    }
    walk_site<CPLX, false>(s, R, Ts);
    if constexpr (AT_BOND)
      if (s.rsel >= 0) walk_env_to_pool<CPLX, false>(R, walk_Dbl(s), walk_Dkl(s), pool + s.roff);
  }
}

// Body of an *_envs kernel with a grid of two: workgroup 0 walks right to left, workgroup 1 left to right, each with its
// environment in the first e_elems working elements of the dynamic LDS and the slice T behind them
template <bool CPLX, bool AT_BOND, class Row>
__device__ __forceinline__ void walk_envs(const Row* __restrict__ sites, int nsite, int first, int last, int e_elems,
                                          void* pool) {
  using T = ChainT<CPLX>;
  extern __shared__ __attribute__((aligned(16))) double walk_lds[];
  T* E = reinterpret_cast<T*>(walk_lds);
  T* Ts = E + e_elems;
  if (blockIdx.x == 0)
    walk_right<CPLX, AT_BOND>(sites, nsite, first, E, Ts, static_cast<T*>(pool));
  else
    walk_left<CPLX, AT_BOND>(sites, last, E, Ts, static_cast<T*>(pool));
}

// sum of v over the workgroup in a fixed order: down the lanes of each wave, then a tree over the waves through LDS;
// the value is valid in thread 0 (k_corr_rows of mpse_corr.hip, k_expect_windows of mpse_expect.hip)
template <bool CPLX>
__device__ ChainT<CPLX> cr_block_sum(ChainT<CPLX> v, ChainT<CPLX>* red, int tid) {
  using El = ChainEl<CPLX>;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) El::add(v, El::shfl_down(v, off));
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  for (int st = CHAIN_WAVES / 2; st > 0; st >>= 1) {
    if (tid < st) El::add(red[tid], red[tid + st]);
    __syncthreads();
  }
  const ChainT<CPLX> r = red[0];
  __syncthreads();   // red is written again by the next sum
  return r;
}

// ----------------------------------------------------------------------------------------------------------- host side
// the two LDS regions of a launch at bond D, environment and slice (both D rows, padded), plus `extra` elements
constexpr int64_t chain_walk_lds(int64_t D, int64_t es, int64_t extra = 0) {
  return (2 * D * chain_pitch(D) + extra) * es;
}
// the largest power-of-two bond D whose complex regions fit and whose environment has one entry per accumulator
constexpr int64_t chain_bond_fit() {
  int64_t D = 1;
  constexpr int64_t acc = int64_t(CHAIN_THREADS) * CHAIN_OUT_PER_THREAD;
  while (chain_walk_lds(2 * D, 16) <= CHAIN_LDS_MAX && 4 * D * D <= acc) D *= 2;
  return D;
}
constexpr int64_t CHAIN_BOND_FIT = chain_bond_fit();
static_assert(CHAIN_BOND_FIT == 64, "2 x 64 x 65 complex128 = 130 KB of 160 KB; 128 would need 516 KB");
// one accumulator per entry of an environment: Db * Dk <= CHAIN_ACC_MAX at every bond.  d danc <= CHAIN_EXT_MAX and fewer
// than 2^31 elements per site tensor keep the site offsets inside 32 bits (ONE chain: 64 * 65536 * 64 = 2^28 elements).
constexpr int64_t CHAIN_ACC_MAX = int64_t(CHAIN_THREADS) * CHAIN_OUT_PER_THREAD;
constexpr int64_t CHAIN_SITE_ELEMS_MAX = (int64_t(1) << 31) - 1;
static_assert(CHAIN_BOND_FIT * CHAIN_BOND_FIT == CHAIN_ACC_MAX, "ONE chain: a bond fits up to CHAIN_BOND_FIT");

// Row i of a dims table as the extents of a bra and a ket: the table has rows (D_l, d, danc, D_r) of ONE chain, which
// is its own bra, or (`two`) rows (Db_l, Dk_l, d, danc, Db_r, Dk_r) of two chains
struct ChainExt {
  int64_t Dbl, Dkl, d, danc, Dbr, Dkr;
};
static inline ChainExt chain_ext(const int64_t* dims, bool two, int i) {
  const int64_t* r = dims + (two ? 6 : 4) * i;
  return two ? ChainExt{r[0], r[1], r[2], r[3], r[4], r[5]} : ChainExt{r[0], r[0], r[1], r[2], r[3], r[3]};
}

struct ChainSelArgs {
  int nsite;
  const void* const* sites;   // the chain; with a bra, the ket
  const int* dtype;
  const int64_t* dims;
  int nsel;
  const int* sel;
  // A bra that differs from the chain (mpse_trdm1.hip): dims then has the six-column rows.  Without one the chain is
  // its own bra, conjugated.
  const void* const* bra = nullptr;
  const int* bra_dtype = nullptr;
  int conj_bra = 1;

  bool two() const { return bra != nullptr; }
  ChainExt ext(int i) const { return chain_ext(dims, two(), i); }
};

// the common part of descriptor row i, `sel` its position in the selection or -1
static inline ChainSelRow chain_sel_row(const ChainSelArgs& a, int i, int sel) {
  const int64_t* d = a.dims + 4 * i;
  return ChainSelRow{a.sites[i], (int)d[0], (int)d[1], (int)d[2], (int)d[3], a.dtype[i] == MPSE_C128, sel};
}

struct ChainSelPlan {
  bool chain;            // the chain kernels take it
  bool fit;              // they could: LDS and offsets allow the launches, whatever the bond limit of the rule says
  int64_t max_bond;      // largest bond of either chain
  int64_t e_elems;       // LDS elements of region E: the largest environment (padded rows) and Db_l Db_r of a site
  int64_t t_elems;       // LDS elements of region T: the largest (sigma, ancilla) slice of T (padded rows)
  int64_t lds;           // bytes of either launch, working dtype
  int64_t max_bra, max_ket;
};

static inline bool chain_sel_table_ok(int nsite, const int64_t* dims, bool two = false) {
  return two ? chain_table_ok(nsite, dims, 6, {0, 1}, {4, 5}) : chain_table_ok(nsite, dims, 4, {0}, {3});
}
static inline bool chain_sel_ok(int nsite, int nsel, const int* sel) {
  if (nsel < 1 || !sel) return false;
  for (int k = 0; k < nsel; ++k)
    if (sel[k] < 0 || sel[k] >= nsite || (k > 0 && sel[k] <= sel[k - 1])) return false;
  return true;
}

// The sizing of a table that is a chain (`two`: of a bra and a ket, chain_ext).  `allowed`: the conditions of the call
// itself (number of selected sites, offsets) hold; `extra`: LDS elements of the call next to the two regions;
// `bond_max`: the bond limit of its rule.  Region E holds an environment, Db rows of pitch(Dk), and for the calls that
// close a site U (Db_l x Db_r, unpadded), which ONE chain has room for anyway: D_l D_r <= D pitch(D) at its larger
// bond.  Region T holds a slice of either walk: Db_l rows of pitch(Dk_r) from the left, Dk_l rows of pitch(Db_r) from
// the right.
static inline ChainSelPlan chain_sel_plan(int nsite, const int64_t* dims, bool allowed, int64_t extra, bool cplx,
                                          int64_t bond_max, bool two = false) {
  ChainSelPlan pl{false, false, 0, 0, 0, 0, 0, 0};
  bool fits = allowed;
  for (int i = 0; i < nsite; ++i) {
    const ChainExt x = chain_ext(dims, two, i);
    pl.max_bra = std::max({pl.max_bra, x.Dbl, x.Dbr});
    pl.max_ket = std::max({pl.max_ket, x.Dkl, x.Dkr});
    bool ok = x.d <= CHAIN_EXT_MAX && x.danc <= CHAIN_EXT_MAX && x.d * x.danc <= CHAIN_EXT_MAX;
    for (int64_t D : {x.Dbl, x.Dkl, x.Dbr, x.Dkr}) ok = ok && D <= CHAIN_ACC_MAX;
    ok = ok && x.Dbl * x.Dkl <= CHAIN_ACC_MAX && x.Dbr * x.Dkr <= CHAIN_ACC_MAX;
    for (int64_t n : {x.Dbl * x.d * x.danc * x.Dbr, x.Dkl * x.d * x.danc * x.Dkr}) ok = ok && n <= CHAIN_SITE_ELEMS_MAX;
    if (!ok) {
      fits = false;
      continue;
    }
    pl.e_elems = std::max({pl.e_elems, x.Dbl * chain_pitch(x.Dkl), x.Dbr * chain_pitch(x.Dkr), x.Dbl * x.Dbr});
    pl.t_elems = std::max({pl.t_elems, x.Dbl * chain_pitch(x.Dkr), x.Dkl * chain_pitch(x.Dbr)});
  }
  pl.max_bond = std::max(pl.max_bra, pl.max_ket);
  if (fits) {
    pl.lds = (pl.e_elems + pl.t_elems + extra) * (cplx ? 16 : 8);
    pl.fit = pl.lds <= CHAIN_LDS_MAX;
  }
  if (!pl.fit) pl.lds = pl.e_elems = pl.t_elems = 0;
  pl.chain = pl.fit && pl.max_bond <= bond_max;
  return pl;
}

// Body of a *_plan export: the twelve values that the three calls share, `more` behind them; returns the path
static inline int chain_sel_plan_out(const ChainSelPlan& pl, bool valid, int64_t bond_max, int64_t nsel_max,
                                     std::initializer_list<int64_t> more, int64_t* info, int n) {
  std::vector<int64_t> v{bond_max, CHAIN_LDS_MAX, pl.chain ? pl.lds : 0, pl.e_elems, pl.t_elems, CHAIN_THREADS,
                         pl.max_bond, valid ? 1 : 0, nsel_max, CHAIN_EXT_MAX, CHAIN_BOND_FIT, pl.lds};
  v.insert(v.end(), more);
  plan_info_out(info, n, v.data(), (int)v.size());
  return pl.chain ? 1 : 0;
}

static_assert(mpse_ctx::CR_SITES == 2 && mpse_ctx::RD_SITES == 2 && mpse_ctx::RD2_SITES == 2 &&
              mpse_ctx::BS_SITES == 2 && mpse_ctx::CR_ENTRIES == 3 && mpse_ctx::RD_MATRICES == 3 &&
              mpse_ctx::RD2_PAIRS == 3 && mpse_ctx::BS_BONDS == 3,
              "chain_sel_done: chain, enqueued, sites, results");
// Tail of an entry point: counts the call (stats: by path, sites walked, results) and hands the result to the caller
static inline int chain_sel_done(long long* stats, bool chain, int nsite, long long results,
                                 const std::vector<double>& res, double* out_host) {
  stats[chain ? 0 : 1] += 1, stats[2] += nsite, stats[3] += results;
  memcpy(out_host, res.data(), res.size() * sizeof(double));
  return MPSE_OK;
}

// MPSE_*_CHAIN=0 sends every chain through the enqueued products; =1 sends every chain whose launches fit through the
// kernels, above the bond limit of the rule as well (measurements of the limits: tools/*_bench.py)
static inline void chain_sel_plan_switch(const char* name, ChainSelPlan* pl) {
  const char env = chain_env_switch(name);
  if (env == '0') pl->chain = false;
  if (env == '1') pl->chain = pl->fit;
}

// What an entry point refuses before any device work, in this order: a null argument (`rest`: the pointer arguments of
// the call beyond the chain, its dims and its selection are all there) or fewer than nsel_min selected sites, a null
// site or an unknown dtype (of the bra first, where there is one), a selection that is not strictly ascending, a table
// that is no chain, a deferred list being recorded.  *cplx: some tensor is complex128.  `sel_end`: the selection lies in
// [0, sel_end); -1: in [0, nsite), a selection of sites (the bonds of mpse_bondspec.hip end one earlier).
static inline int chain_sel_prologue(mpse_ctx* ctx, const char* call, const ChainSelArgs& a, int nsel_min, bool rest,
                                     bool* cplx, int sel_end = -1) {
  if (!ctx) return MPSE_ERR_ARG;
  if (a.nsite < 1 || !a.sites || !a.dtype || !a.dims || a.nsel < nsel_min || !a.sel || !rest)
    return mpse_fail(ctx, MPSE_ERR_ARG, "%s: null argument, no sites or %s", call,
                     nsel_min > 1 ? "fewer than two selected sites" : "no selection");
  MPSE_TRY(a.two() ? chain_scan_sites(ctx, call, a.nsite, {a.bra, a.sites}, {a.bra_dtype, a.dtype}, cplx)
                   : chain_scan_sites(ctx, call, a.nsite, {a.sites}, {a.dtype}, cplx));
  if (sel_end < 0) sel_end = a.nsite;
  if (!chain_sel_ok(sel_end, a.nsel, a.sel))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "%s: the selection is not strictly ascending inside [0, %d)", call, sel_end);
  if (!chain_sel_table_ok(a.nsite, a.dims, a.two()))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "%s: dims is not a chain (extents >= 1, matching neighbours, first and last %s 1)", call,
                     a.two() ? "bonds" : "bond");
  if (MPSE_RECORDING(ctx))
    return mpse_fail(ctx, MPSE_ERR_ARG, "%s: synchronous, not available while a deferred list is recorded", call);
  return MPSE_OK;
}

// The n working elements at `dev` read by the host, once, and every run of them (src, count, dst in elements) written
// as complex pairs into out
struct ChainRun {
  int64_t src, n, dst;
};
static inline int chain_read_pairs(mpse_ctx* ctx, const void* dev, int64_t n, bool cplx,
                                   const std::vector<ChainRun>& runs, double* out) {
  std::vector<double> host((size_t)n * (cplx ? 2 : 1));
  MPSE_TRY(mpse_memcpy_d2h(ctx, host.data(), dev, host.size() * sizeof(double)));
  for (const ChainRun& r : runs)
    for (int64_t e = 0; e < r.n; ++e) {
      out[2 * (r.dst + e)] = cplx ? host[2 * (r.src + e)] : host[r.src + e];
      out[2 * (r.dst + e) + 1] = cplx ? host[2 * (r.src + e) + 1] : 0.0;
    }
  return MPSE_OK;
}

// What the enqueued path of a call works with: the working dtype (complex as soon as any operand is), every site of the
// ket K (Dk_l, p, Dk_r) and of the bra B (Db_l, p, Db_r), p = d danc, in it (real sites of a complex call as widened
// copies in pooled buffers that live as long as this; ONE chain is widened once and is both), the position of every
// site in the selection (-1: not selected; the correlation matrix does not need it), the largest environment and the
// largest site or intermediate in elements, a product in that dtype and the four products of the transfer, op(B)
// through the conjugation flag of the product.  The calls on ONE chain pass equal bonds.
struct ChainSelEnq {
  mpse_ctx* ctx;
  int dt, cj;    // cj: conjugate B, set for a complex call that conjugates the bra
  size_t es;
  int64_t e_max = 1, x_max = 1;
  std::vector<int> pos;
  std::vector<const void*> site, bra;   // K and B
  std::vector<std::unique_ptr<TmpBuf>> wide;

  ChainSelEnq(mpse_ctx* c, bool cplx, int conj_bra = 1)
      : ctx(c), dt(cplx ? MPSE_C128 : MPSE_F64), cj(cplx && conj_bra ? 1 : 0), es(cplx ? 16 : 8) {}
  int widen(const void** t, int64_t n) {
    wide.emplace_back(new TmpBuf(ctx));
    return widen_site(ctx, *wide.back(), t, n, n);
  }
  int init(const ChainSelArgs& a) {
    pos.assign((size_t)a.nsite, -1);
    for (int k = 0; k < a.nsel; ++k) pos[a.sel[k]] = k;
    site.assign(a.sites, a.sites + a.nsite);
    if (a.two()) bra.assign(a.bra, a.bra + a.nsite);
    for (int i = 0; i < a.nsite; ++i) {
      const ChainExt x = a.ext(i);
      const int64_t p = x.d * x.danc;
      e_max = std::max(e_max, x.Dbr * x.Dkr);
      x_max = std::max({x_max, x.Dkl * p * x.Dbr, x.Dbl * p * x.Dkr, x.Dbl * p * x.Dbr});
      if (dt != MPSE_C128) continue;
      if (a.two() && a.bra_dtype[i] != MPSE_C128) MPSE_TRY(widen(&bra[i], x.Dbl * p * x.Dbr));
      if (a.dtype[i] != MPSE_C128) MPSE_TRY(widen(&site[i], x.Dkl * p * x.Dkr));
    }
    if (!a.two()) bra = site;
    return MPSE_OK;
  }
  int alloc(std::initializer_list<std::pair<TmpBuf*, int64_t>> bufs) const {   // each buffer with its working elements
    for (const auto& b : bufs) MPSE_TRY(b.first->alloc((size_t)b.second * es));
    return MPSE_OK;
  }
  int gemm(int conj_a, mpse_index ma, mpse_index ka, mpse_index kb, mpse_index nb, mpse_index mc, mpse_index nc,
           int64_t batch, int64_t sba, int64_t sbb, int64_t sbc, const void* A, const void* B, void* C) const {
    return gemm_call(ctx, dt, dt, conj_a ? cj : 0, 0, ma, ka, kb, nb, mc, nc, batch, sba, sbb, sbc, A, B, C);
  }
  //   Y[r, b'] = sum_k' A[r, k'] R[b', k'],  r = (k, s, a): n = Dk_l p rows (or any stack of rows of Dk_r elements)
  int a_r(int64_t n, int64_t Dbr, int64_t Dkr, const void* A, const void* R, void* Y) const {
    return gemm(0, idx1(n, Dkr), idx1(Dkr, 1), idx1(Dkr, 1), idx1(Dbr, Dkr), idx1(n, Dbr), idx1(Dbr, 1), 1, 0, 0, 0, A, R,
                Y);
  }
  //   R'[b, k] = sum_(s, a, b') op(B[b, (s, a, b')]) Y[k, (s, a, b')],  kk = p Db_r
  int ca_y(int64_t Dbl, int64_t Dkl, int64_t kk, const void* B, const void* Y, void* Rn) const {
    return gemm(1, idx1(Dbl, kk), idx1(kk, 1), idx1(kk, 1), idx1(Dkl, kk), idx1(Dbl, Dkl), idx1(Dkl, 1), 1, 0, 0, 0, B, Y,
                Rn);
  }
  //   X[(r, b), (s, a, k')] = sum_k L[(r, b), k] K[k, (s, a, k')] for a stack of nrow environments,  n = p Dk_r
  int l_a(int64_t nrow, int64_t Dbl, int64_t Dkl, int64_t n, const void* L, const void* K, void* X) const {
    return gemm(0, idx1(nrow * Dbl, Dkl), idx1(Dkl, 1), idx1(Dkl, n), idx1(n, 1), idx1(nrow * Dbl, n), idx1(n, 1), 1, 0, 0,
                0, L, K, X);
  }
  //   L'[r][b', k'] = sum_(b, s, a) op(B[(b, s, a), b']) X[r][(b, s, a), k'] batched over the nrow environments of a
  //   stack,  m = Db_l p.  The batch strides are passed for nrow = 1 too: a product of one batch never reads them.
  int ca_x(int64_t nrow, int64_t m, int64_t Dbr, int64_t Dkr, const void* B, const void* X, void* Ln) const {
    return gemm(1, idx1(Dbr, 1), idx1(m, Dbr), idx1(m, Dkr), idx1(Dkr, 1), idx1(Dbr, Dkr), idx1(Dkr, 1), nrow, 0, m * Dkr,
                Dbr * Dkr, B, X, Ln);
  }
};
