// What the chain calls with a site selection share beyond mpse_chain.h (mpse_corr.hip, mpse_rdm1.hip, mpse_rdm2.hip,
// mpse_trdm1.hip, mpse_bondspec.hip, mpse_expect.hip; no other file includes this).  The first three and
// mpse_bondspec.hip (whose selection names bonds) take dims rows (D_l, d, danc, D_r) of ONE chain and a strictly ascending selection, and walk the chain with
// the identity transfer matrix: the environment in LDS, one (sigma,
// ancilla) slice of a site at a time.  mpse_trdm1.hip walks TWO chains with rectangular environments: its stages are
// the walk2_* ones below, next to the square ones, which it leaves alone.  Here are the two stages of that transfer,
// once per direction, the moves of an environment between LDS and pooled memory, the sizing of the launches, the
// checks of the entry points and what the enqueued passes share.  A call keeps its descriptor row, its loop over the
// slices and what it does with the sums.  In all four a workgroup reads only what the launch before it wrote (no flag,
// no spin wait, no atomic), the host reads once, at the end, and the order of every sum is fixed: the same inputs give
// the same bits.
#pragma once
#include "mpse_chain.h"

constexpr int CHAIN_WAVES = CHAIN_THREADS / 64;
constexpr int CHAIN_OUT_PER_THREAD = 4;   // entries of a new environment a thread accumulates in registers

// --------------------------------------------------------------------------------------------------------- device side
// `Row`: a descriptor row that starts with ChainSelRow.  `row`: the elements of A per index of its left bond, d danc
// D_r, computed once per site by the kernel.  An environment of bond D in LDS has D rows of chain_pitch(D) elements.  A
// slice of a site is named by the elements before it in a row of the left bond: (sigma danc + a) D_r.  Every sum runs
// over its inner index in ascending order.
struct ChainSelRow {   // what the descriptor rows of the three calls begin with (32 bytes)
  const void* a;
  int Dl, d, danc, Dr;
  int cplx;            // the tensor is complex128
  int sel;             // position in the selection, -1: not selected
};

// the identity environment of the bond 1 at either end
template <bool CPLX>
__device__ __forceinline__ void walk_env_one(ChainT<CPLX>* E) {
  if (threadIdx.x == 0) E[0] = ChainEl<CPLX>::one();
  __syncthreads();
}

// Rightwards, first stage: T[c, b'] = sum_c' A[c, ket, c'] R[b', c'] into LDS, rows of T padded like those of R; ends
// with the barrier behind which T is read
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_right_slice(const Row& s, int row, int ket, const ChainT<CPLX>* R,
                                                 ChainT<CPLX>* Ts) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int Dr = s.Dr, pr = Dr | 1, nT = s.Dl * Dr;
  for (int o = threadIdx.x; o < nT; o += CHAIN_THREADS) {
    const int c = o / Dr, bp = o - c * Dr;
    const T* r_row = R + bp * pr;
    const int a0 = c * row + ket;
    T sum = El::zero();
#pragma unroll 4
    for (int cp = 0; cp < Dr; ++cp) El::fma(sum, El::ld(s.a, s.cplx, a0 + cp), r_row[cp]);
    Ts[c * pr + bp] = sum;
  }
  __syncthreads();
}

// Rightwards, second stage: S = sum_b' conj(A[b, bra, b']) T[c, b'] of the entry o = b D_l + c of the new environment.
// Owners take o = tid + j * CHAIN_THREADS: A[b, ..] is one address per b group, the reads of T run down a column of
// padded rows.  walk_right_dot is the sum itself, for rd2_walk_right, which meets an owned entry with d bra slices and
// takes (b, c) once.  S leaves through a reference and `row` comes from the kernel on purpose: DESIGN_HISTORY.md.
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_right_dot(const Row& s, int b0, const ChainT<CPLX>* t_row, ChainT<CPLX>& S) {
  using El = ChainEl<CPLX>;
  const int Dr = s.Dr;
  S = El::zero();
#pragma unroll 4
  for (int bp = 0; bp < Dr; ++bp) El::fma(S, El::cj(El::ld(s.a, s.cplx, b0 + bp)), t_row[bp]);
}
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_right_sum(const Row& s, int row, int bra, int o, const ChainT<CPLX>* Ts,
                                               ChainT<CPLX>& S) {
  const int b = o / s.Dl, c = o - b * s.Dl;
  walk_right_dot<CPLX>(s, b * row + bra, Ts + c * (s.Dr | 1), S);
}

// Leftwards, first stage: T[b, c'] = sum_c E[b, c] A[c, ket, c'] with rows of E `pe` and rows of T `pt` elements apart
// (the walks: E padded in LDS, T packed; k_rdm1_sites: E packed in pooled memory, T padded); ends with the barrier
// behind which T is read
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_left_slice(const Row& s, int row, int ket, const ChainT<CPLX>* E, int pe,
                                                ChainT<CPLX>* Ts, int pt) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int Dl = s.Dl, Dr = s.Dr, nT = Dl * Dr;
  for (int o = threadIdx.x; o < nT; o += CHAIN_THREADS) {
    const int b = o / Dr, cc = o - b * Dr;
    const T* e_row = E + b * pe;
    const int a0 = ket + cc;
    T sum = El::zero();
#pragma unroll 4
    for (int c = 0; c < Dl; ++c) El::fma(sum, e_row[c], El::ld(s.a, s.cplx, c * row + a0));
    Ts[b * pt + cc] = sum;
  }
  __syncthreads();
}

// Leftwards, second stage: S = sum_b conj(A[b, bra, b']) T[b, c'] of the entry o = b' D_r + c' of the new environment,
// T packed.  Owners take o = tid + j * CHAIN_THREADS, c' fastest.
template <bool CPLX, class Row>
__device__ __forceinline__ void walk_left_sum(const Row& s, int row, int bra, int o, const ChainT<CPLX>* Ts,
                                              ChainT<CPLX>& S) {
  using El = ChainEl<CPLX>;
  const int Dl = s.Dl, Dr = s.Dr;
  const int bb = o / Dr, cc = o - bb * Dr;
  const int b0 = bra + bb;
  S = El::zero();
#pragma unroll 4
  for (int b = 0; b < Dl; ++b) El::fma(S, El::cj(El::ld(s.a, s.cplx, b * row + b0)), Ts[b * Dr + cc]);
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

// The accumulators of the owners become the environment of bond D in LDS.  The caller has passed the barrier behind the
// last slice, so every read of the old environment is done; ends with the barrier behind which the new one is read.
template <bool CPLX>
__device__ __forceinline__ void walk_acc_store(const ChainT<CPLX> (&acc)[CHAIN_OUT_PER_THREAD], int D,
                                               ChainT<CPLX>* E) {
  const int pitch = D | 1;
#pragma unroll
  for (int j = 0; j < CHAIN_OUT_PER_THREAD; ++j) {
    const int o = threadIdx.x + j * CHAIN_THREADS;
    if (o < D * D) {
      const int r = o / D, c = o - r * D;
      E[r * pitch + c] = acc[j];
    }
  }
  __syncthreads();
}

// the environment of bond D in LDS to D D packed elements of pooled memory, as it is or transposed
template <bool CPLX, bool TRANSPOSED>
__device__ __forceinline__ void walk_env_to_pool(const ChainT<CPLX>* E, int D, ChainT<CPLX>* P) {
  const int pitch = D | 1;
  for (int o = threadIdx.x; o < D * D; o += CHAIN_THREADS) {
    const int r = o / D, c = o - r * D;
    P[o] = TRANSPOSED ? E[c * pitch + r] : E[r * pitch + c];
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

// The walk from the left that leaves the identity environment L of selected sites in pooled memory: workgroup 1 of
// k_rdm1_envs and of k_rdm2_envs.  `Row` has eoff (working elements before L of the site in `pool`) as well.  L_0 = 1.
// At a selected site L goes to the pooled buffer; the walk ends at site `last`.  Else per site from the left, per
// (sigma, a) in ascending order, the transfer to the left: T = L . A[sigma, a] into LDS, L' += S in the owner's
// registers.
template <bool CPLX, class Row>
__device__ void chain_walk_left(const Row* __restrict__ sites, int last, ChainT<CPLX>* E, ChainT<CPLX>* Ts,
                                ChainT<CPLX>* pool) {
  walk_env_one<CPLX>(E);
  for (int i = 0; i <= last; ++i) {
    const Row s = sites[i];
    const int p = s.d * s.danc, row = p * s.Dr, nE = s.Dr * s.Dr;
    if (s.sel >= 0) walk_env_to_pool<CPLX, false>(E, s.Dl, pool + s.eoff);
    if (i == last) break;
    ChainT<CPLX> acc[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc);
    for (int sa = 0; sa < p; ++sa) {
      walk_left_slice<CPLX>(s, row, sa * s.Dr, E, s.Dl | 1, Ts, s.Dr);
      walk_acc_add<CPLX, true>(s, row, sa * s.Dr, Ts, nE, acc);
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of L is done as well
    }
    walk_acc_store<CPLX>(acc, s.Dr, E);
  }
}

// The walks that leave the identity environments of selected BONDS in pooled memory: the two workgroups of
// k_bondspec_envs (mpse_bondspec.hip) and of k_expect_envs (mpse_expect.hip).  `Row` has, beyond ChainSelRow, rsel (the
// bond LEFT of the site is selected: leave R there), roff and loff (working elements before that R, and before L of the
// bond RIGHT of the site, which `sel` selects, in `pool`).
// From the right: R behind the last site is 1.  Per site from the right down to the one right of the first selected
// bond, the transfer of rd_walk_right (mpse_rdm1.hip); R of a selected bond goes to the pooled buffer as it is.
template <bool CPLX, class Row>
__device__ void walk_bonds_right(const Row* __restrict__ sites, int nsite, int first, ChainT<CPLX>* R, ChainT<CPLX>* Ts,
                                 ChainT<CPLX>* pool) {
  walk_env_one<CPLX>(R);
  for (int i = nsite - 1; i > first; --i) {
    const Row s = sites[i];
    const int p = s.d * s.danc, row = p * s.Dr, nE = s.Dl * s.Dl;
    ChainT<CPLX> acc[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc);
    for (int sa = 0; sa < p; ++sa) {
      walk_right_slice<CPLX>(s, row, sa * s.Dr, R, Ts);
      walk_acc_add<CPLX, false>(s, row, sa * s.Dr, Ts, nE, acc);
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of R is done as well
    }
    walk_acc_store<CPLX>(acc, s.Dl, R);
    if (s.rsel >= 0) walk_env_to_pool<CPLX, false>(R, s.Dl, pool + s.roff);
  }
}

// From the left: the sibling of chain_walk_left that leaves L BEHIND a site (the bond right of it) and ends behind
// site `last`, the one left of the last selected bond
template <bool CPLX, class Row>
__device__ void walk_bonds_left(const Row* __restrict__ sites, int last, ChainT<CPLX>* E, ChainT<CPLX>* Ts,
                                ChainT<CPLX>* pool) {
  walk_env_one<CPLX>(E);
  for (int i = 0; i <= last; ++i) {
    const Row s = sites[i];
    const int p = s.d * s.danc, row = p * s.Dr, nE = s.Dr * s.Dr;
    ChainT<CPLX> acc[CHAIN_OUT_PER_THREAD];
    walk_acc_zero<CPLX>(acc);
    for (int sa = 0; sa < p; ++sa) {
      walk_left_slice<CPLX>(s, row, sa * s.Dr, E, s.Dl | 1, Ts, s.Dr);
      walk_acc_add<CPLX, true>(s, row, sa * s.Dr, Ts, nE, acc);
      __syncthreads();   // T is overwritten by the next (sigma, a); after the last one every read of L is done as well
    }
    walk_acc_store<CPLX>(acc, s.Dr, E);
    if (s.sel >= 0) walk_env_to_pool<CPLX, false>(E, s.Dr, pool + s.loff);
  }
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

// ------------------------------------------------------------------------------------------- device side, two chains
// The same two stages for a bra B (Db_l, d, danc, Db_r) and a ket K (Dk_l, d, danc, Dk_r) that differ: an environment at
// a bond is Db rows of chain_pitch(Dk) elements, bra index first.  `Row`: a descriptor row that starts with Chain2Row.
// `krow` / `brow`: the elements of K / B per index of its left bond, d danc Dk_r / d danc Db_r; a slice is named by the
// elements before it in such a row, `ket` = (sigma danc + a) Dk_r in K and `bra` = (sigma danc + a) Db_r in B.  op(B) is
// the conjugate when the row says so (bra_cj: the call conjugates the bra and this tensor is complex).
struct Chain2Row {   // what a descriptor row of a two-chain call begins with (56 bytes)
  const void* bra;
  const void* ket;
  int Dbl, Dkl, d, danc, Dbr, Dkr;
  int bra_c, ket_c;    // the side's tensor is complex128
  int bra_cj;          // conjugate the bra tensor
  int sel;             // position in the selection, -1: not selected
};

template <bool CPLX, class Row>
__device__ __forceinline__ ChainT<CPLX> walk2_ld_bra(const Row& s, int i) {
  const ChainT<CPLX> v = ChainEl<CPLX>::ld(s.bra, s.bra_c, i);
  return s.bra_cj ? ChainEl<CPLX>::cj(v) : v;
}

// Leftwards (the walk from the left), first stage: T[b, k'] = sum_k E[b, k] K[k, ket, k'] with rows of E `pe` and rows
// of T `pt` elements apart; ends with the barrier behind which T is read
template <bool CPLX, class Row>
__device__ __forceinline__ void walk2_left_slice(const Row& s, int krow, int ket, const ChainT<CPLX>* E, int pe,
                                                 ChainT<CPLX>* Ts, int pt) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int Dkl = s.Dkl, Dkr = s.Dkr, nT = s.Dbl * Dkr;
  for (int o = threadIdx.x; o < nT; o += CHAIN_THREADS) {
    const int b = o / Dkr, kk = o - b * Dkr;
    const T* e_row = E + b * pe;
    const int k0 = ket + kk;
    T sum = El::zero();
#pragma unroll 4
    for (int k = 0; k < Dkl; ++k) El::fma(sum, e_row[k], El::ld(s.ket, s.ket_c, k * krow + k0));
    Ts[b * pt + kk] = sum;
  }
  __syncthreads();
}

// Leftwards, second stage: S = sum_b op(B[b, bra, b']) T[b, k'] of the entry o = b' Dk_r + k' of the new environment
// (Db_r x Dk_r), rows of T `pt` apart.  Owners take o = tid + j * CHAIN_THREADS, k' fastest.
template <bool CPLX, class Row>
__device__ __forceinline__ void walk2_left_sum(const Row& s, int brow, int bra, int o, const ChainT<CPLX>* Ts, int pt,
                                               ChainT<CPLX>& S) {
  using El = ChainEl<CPLX>;
  const int Dbl = s.Dbl, Dkr = s.Dkr;
  const int bb = o / Dkr, kk = o - bb * Dkr;
  const int b0 = bra + bb;
  S = El::zero();
#pragma unroll 4
  for (int b = 0; b < Dbl; ++b) El::fma(S, walk2_ld_bra<CPLX>(s, b * brow + b0), Ts[b * pt + kk]);
}

// Rightwards (the walk from the right), first stage: T[k, b'] = sum_k' K[k, ket, k'] R[b', k'] into LDS, R with rows
// of chain_pitch(Dk_r), T (Dk_l rows) with rows of chain_pitch(Db_r); ends with the barrier behind which T is read
template <bool CPLX, class Row>
__device__ __forceinline__ void walk2_right_slice(const Row& s, int krow, int ket, const ChainT<CPLX>* R,
                                                  ChainT<CPLX>* Ts) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  const int Dbr = s.Dbr, Dkr = s.Dkr, pr = Dkr | 1, pt = Dbr | 1, nT = s.Dkl * Dbr;
  for (int o = threadIdx.x; o < nT; o += CHAIN_THREADS) {
    const int k = o / Dbr, bp = o - k * Dbr;
    const T* r_row = R + bp * pr;
    const int k0 = k * krow + ket;
    T sum = El::zero();
#pragma unroll 4
    for (int kp = 0; kp < Dkr; ++kp) El::fma(sum, El::ld(s.ket, s.ket_c, k0 + kp), r_row[kp]);
    Ts[k * pt + bp] = sum;
  }
  __syncthreads();
}

// Rightwards, second stage: S = sum_b' op(B[b, bra, b']) T[k, b'] of the entry o = b Dk_l + k of the new environment
// (Db_l x Dk_l).  Owners take o = tid + j * CHAIN_THREADS: B[b, ..] is one address per b group.
template <bool CPLX, class Row>
__device__ __forceinline__ void walk2_right_sum(const Row& s, int brow, int bra, int o, const ChainT<CPLX>* Ts,
                                                ChainT<CPLX>& S) {
  using El = ChainEl<CPLX>;
  const int Dkl = s.Dkl, Dbr = s.Dbr;
  const int b = o / Dkl, k = o - b * Dkl;
  const int b0 = b * brow + bra;
  const ChainT<CPLX>* t_row = Ts + k * (Dbr | 1);
  S = El::zero();
#pragma unroll 4
  for (int bp = 0; bp < Dbr; ++bp) El::fma(S, walk2_ld_bra<CPLX>(s, b0 + bp), t_row[bp]);
}

// The accumulators of the owners become the rows x cols environment in LDS; barriers as walk_acc_store
template <bool CPLX>
__device__ __forceinline__ void walk2_acc_store(const ChainT<CPLX> (&acc)[CHAIN_OUT_PER_THREAD], int rows, int cols,
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
__device__ __forceinline__ void walk2_env_to_pool(const ChainT<CPLX>* E, int rows, int cols, ChainT<CPLX>* P) {
  const int pitch = cols | 1;
  for (int o = threadIdx.x; o < rows * cols; o += CHAIN_THREADS) {
    int r, c;
    if (TRANSPOSED) c = o / rows, r = o - c * rows;
    else r = o / cols, c = o - r * cols;
    P[o] = E[r * pitch + c];
  }
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
// d danc <= CHAIN_EXT_MAX keeps the site offsets inside 32 bits: 64 * 65536 * 64 = 2^28 elements

struct ChainSelArgs {
  int nsite;
  const void* const* sites;
  const int* dtype;
  const int64_t* dims;
  int nsel;
  const int* sel;
};

// the common part of descriptor row i, `sel` its position in the selection or -1
static inline ChainSelRow chain_sel_row(const ChainSelArgs& a, int i, int sel) {
  const int64_t* d = a.dims + 4 * i;
  return ChainSelRow{a.sites[i], (int)d[0], (int)d[1], (int)d[2], (int)d[3], a.dtype[i] == MPSE_C128, sel};
}

struct ChainSelPlan {
  bool chain;            // the chain kernels take it
  bool fit;              // they could: LDS and offsets allow the launches, whatever the bond limit of the rule says
  int64_t max_bond;
  int64_t e_elems;       // LDS elements of the environment (padded rows), largest over the bonds
  int64_t t_elems;       // LDS elements of one (sigma, ancilla) slice of T (padded rows), largest over the sites
  int64_t lds;           // bytes of either launch, working dtype
};

static inline bool chain_sel_table_ok(int nsite, const int64_t* dims) {
  return chain_table_ok(nsite, dims, 4, {0}, {3});
}
static inline bool chain_sel_ok(int nsite, int nsel, const int* sel) {
  if (nsel < 1 || !sel) return false;
  for (int k = 0; k < nsel; ++k)
    if (sel[k] < 0 || sel[k] >= nsite || (k > 0 && sel[k] <= sel[k - 1])) return false;
  return true;
}

// The sizing of a table that is a chain.  `allowed`: the conditions of the call itself (number of selected sites,
// offsets) hold; `extra`: LDS elements of the call next to the two regions; `bond_max`: the bond limit of its rule.
static inline ChainSelPlan chain_sel_plan(int nsite, const int64_t* dims, bool allowed, int64_t extra, bool cplx,
                                          int64_t bond_max) {
  ChainSelPlan pl{false, false, 0, 0, 0, 0};
  bool fits = true;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + 4 * i;
    for (int j : {0, 3}) pl.max_bond = d[j] > pl.max_bond ? d[j] : pl.max_bond;
    if (pl.max_bond > CHAIN_BOND_FIT || d[1] > CHAIN_EXT_MAX || d[2] > CHAIN_EXT_MAX || d[1] * d[2] > CHAIN_EXT_MAX) {
      fits = false;
      continue;
    }
    const int64_t e_l = d[0] * chain_pitch(d[0]), e_r = d[3] * chain_pitch(d[3]), t = d[0] * chain_pitch(d[3]);
    pl.e_elems = std::max({pl.e_elems, e_l, e_r});
    pl.t_elems = std::max(pl.t_elems, t);
  }
  if (fits && allowed) {
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
// the call beyond `a` are all there) or fewer than nsel_min selected sites, a null site or an unknown dtype, a
// selection that is not strictly ascending, a table that is no chain, a deferred list being recorded.  *cplx: some
// tensor is complex128.  `sel_end`: the selection lies in [0, sel_end); -1: in [0, nsite), a selection of sites (the
// bonds of mpse_bondspec.hip end one earlier).
static inline int chain_sel_prologue(mpse_ctx* ctx, const char* call, const ChainSelArgs& a, int nsel_min, bool rest,
                                     bool* cplx, int sel_end = -1) {
  if (!ctx) return MPSE_ERR_ARG;
  if (a.nsite < 1 || !a.sites || !a.dtype || !a.dims || a.nsel < nsel_min || !a.sel || !rest)
    return mpse_fail(ctx, MPSE_ERR_ARG, "%s: null argument, no sites or %s", call,
                     nsel_min > 1 ? "fewer than two selected sites" : "no selection");
  MPSE_TRY(chain_scan_sites(ctx, call, a.nsite, {a.sites}, {a.dtype}, cplx));
  if (sel_end < 0) sel_end = a.nsite;
  if (!chain_sel_ok(sel_end, a.nsel, a.sel))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "%s: the selection is not strictly ascending inside [0, %d)", call, sel_end);
  if (!chain_sel_table_ok(a.nsite, a.dims))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "%s: dims is not a chain (extents >= 1, matching neighbours, first and last bond 1)", call);
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

// What the enqueued path of a call works with: the working dtype (complex as soon as any operand is), every site in it
// (real sites of a complex call as widened copies in pooled buffers that live as long as this), the position of every
// site in the selection (-1: not selected; the correlation matrix does not need it), the largest environment and the
// largest site in elements, a product in that dtype and the four products of the identity transfer.  A (D_l, p, D_r)
// with p = d danc.
struct ChainSelEnq {
  mpse_ctx* ctx;
  int dt, cj;    // cj: conjugate A, set for a complex call
  size_t es;
  int64_t e_max = 1, x_max = 1;
  std::vector<int> pos;
  std::vector<const void*> site;
  std::vector<std::unique_ptr<TmpBuf>> wide;

  ChainSelEnq(mpse_ctx* c, bool cplx) : ctx(c), dt(cplx ? MPSE_C128 : MPSE_F64), cj(cplx ? 1 : 0), es(cplx ? 16 : 8) {}
  int init(const ChainSelArgs& a) {
    pos.assign((size_t)a.nsite, -1);
    for (int k = 0; k < a.nsel; ++k) pos[a.sel[k]] = k;
    for (int i = 0; i < a.nsite; ++i) {
      const int64_t* d = a.dims + 4 * i;
      e_max = std::max(e_max, d[3] * d[3]);
      x_max = std::max(x_max, d[0] * d[1] * d[2] * d[3]);
    }
    return chain_widen_sites(ctx, a.nsite, a.sites, a.dtype, a.dims, cj != 0, &wide, &site);
  }
  int alloc(std::initializer_list<std::pair<TmpBuf*, int64_t>> bufs) const {   // each buffer with its working elements
    for (const auto& b : bufs) MPSE_TRY(b.first->alloc((size_t)b.second * es));
    return MPSE_OK;
  }
  int gemm(int conj_a, mpse_index ma, mpse_index ka, mpse_index kb, mpse_index nb, mpse_index mc, mpse_index nc,
           int64_t batch, int64_t sba, int64_t sbb, int64_t sbc, const void* A, const void* B, void* C) const {
    return gemm_call(ctx, dt, dt, conj_a ? cj : 0, 0, ma, ka, kb, nb, mc, nc, batch, sba, sbb, sbc, A, B, C);
  }
  //   Y[r, b'] = sum_c' A[r, c'] R[b', c'],  r = (c, s, a): n = D_l p rows (or any stack of rows of D_r elements)
  int a_r(int64_t n, int64_t Dr, const void* A, const void* R, void* Y) const {
    return gemm(0, idx1(n, Dr), idx1(Dr, 1), idx1(Dr, 1), idx1(Dr, Dr), idx1(n, Dr), idx1(Dr, 1), 1, 0, 0, 0, A, R, Y);
  }
  //   R'[b, c] = sum_(s, a, b') conj(A[b, (s, a, b')]) Y[c, (s, a, b')],  k = p D_r
  int ca_y(int64_t Dl, int64_t k, const void* A, const void* Y, void* Rn) const {
    return gemm(1, idx1(Dl, k), idx1(k, 1), idx1(k, 1), idx1(Dl, k), idx1(Dl, Dl), idx1(Dl, 1), 1, 0, 0, 0, A, Y, Rn);
  }
  //   X[(r, b), (s, a, c')] = sum_c L[(r, b), c] A[c, (s, a, c')] for a stack of nrow environments,  k = p D_r
  int l_a(int64_t nrow, int64_t Dl, int64_t k, const void* L, const void* A, void* X) const {
    return gemm(0, idx1(nrow * Dl, Dl), idx1(Dl, 1), idx1(Dl, k), idx1(k, 1), idx1(nrow * Dl, k), idx1(k, 1), 1, 0, 0, 0,
                L, A, X);
  }
  //   L'[r][b', c'] = sum_(b, s, a) conj(A[(b, s, a), b']) X[r][(b, s, a), c'] batched over the nrow environments of a
  //   stack,  m = D_l p.  The batch strides are passed for nrow = 1 too (the unbatched calls passed zeros; a product
  //   of one batch never reads them).
  int ca_x(int64_t nrow, int64_t m, int64_t Dr, const void* A, const void* X, void* Ln) const {
    return gemm(1, idx1(Dr, 1), idx1(m, Dr), idx1(m, Dr), idx1(Dr, 1), idx1(Dr, Dr), idx1(Dr, 1), nrow, 0, m * Dr,
                Dr * Dr, A, X, Ln);
  }
};
