// FP64-MFMA strided tensor-contraction kernel (the one dense kernel every hot-path
// contraction is built from) and its launcher mpse_gemm.
//
//   C[b](i,j) = alpha * sum_k opA(A[b](i,k)) opB(B[b](k,j)) + beta * C[b](i,j)
//
// Design for gfx950 (MI355X):
//   * v_mfma_f64_16x16x4_f64 (64 cycles/SIMD): a wave owns a 32x32 output tile = 2x2 MFMA tiles on planar
//     (re / im) operand fragments.  complex x complex uses the 3M scheme (three real products per complex
//     product: Ar Br, Ai Bi, (Ar + Ai)(Br + Bi)), complex x real = 2 MFMAs, real x real = 1.
//   * a 256-thread workgroup (4 waves, 2x2) owns a 64x64 tile; K advances 16 at a time:
//     global -> registers (issued one tile ahead through running pointers when both K maps are single level)
//     -> LDS as planar (re / im) panels whose layout follows the operand's memory order ([i][k] rows of 17
//     doubles when k is the contiguous index, [k][i] rows of 80 doubles otherwise, so that both the staging
//     ds_write_b64 and the fragment ds_read_b64 are bank-conflict free) -> register fragments, double buffered
//     per k-group of 4.
//   * operands are read straight through two-level strides (no transpose copies: the reference's tensordot
//     materialises a transposed copy before every ?gemm); complex128 elements are 16-byte loads; the
//     thread->element map follows whichever logical index is contiguous in memory so wave loads coalesce.
//   * split-K with a fixed-order reduction kernel when there are fewer output tiles than CUs.
//   * optional structural-zero skipping: a scan kernel flags the 64 x 16 operand tiles that hold data, the K loop
//     visits only K tiles with data on both sides (block-sparse tensors of the quantum-number-conserving sweeps).
//   * launches with at most one workgroup per compute unit put eight waves on the tile (16 x 32 per wave) so that
//     every SIMD has a second wave to fill its MFMA gaps.
//   * workgroups are placed by die: the dispatcher deals launch positions to the eight dies (XCDs, one L2 each) round
//     robin - die = blockIdx mod 8 - so the position -> (tile, K slice) map decides what each L2 has to hold and how
//     evenly block-sparse work spreads.  Split products run slice-fastest (a die = a K range of both operands);
//     unsplit ones give a die whole tile rows or columns of the larger operand; block-sparse ones with more tiles than
//     slots are launched in a die-aware, heaviest-first order computed from the occupancy masks (k_tile_order), the
//     others with their tile columns skewed by the tile row.  (tools/gemm_balance.py on MPSE_GEMM_TRACE timelines.)
//   * accumulation order over k is fixed and independent of the launch order => bitwise reproducible results.
#include <cstdlib>
#include <type_traits>

#include "mpse_device.h"
#include "mpse_gemm_tiles.h"
#include "mpse_internal.h"
#include "mpse_plans.h"

typedef double v4d __attribute__((ext_vector_type(4)));

// debug timeline buffer of the contraction kernel: only inside the profiled (timed) region; MPSE_GEMM_TRACE_ONLY=f0
// leaves the buffer to the records of the fused bond / two-level-site matvec (mpse_heff0.hip)
static unsigned long long* gemm_trace_ptr(const mpse_ctx* ctx) {
  static const bool f0_only = [] {
    const char* e = getenv("MPSE_GEMM_TRACE_ONLY");
    return e && e[0] == 'f';
  }();
  return (ctx->prof_on && !f0_only) ? ctx->gemm_trace : nullptr;
}

namespace {

struct IdxMap {
  long long s_hi, s_lo;
  int ext, lo;
};

// Grouped launch (folded one-site matvec, mpse_plans.h): the tile rows of the launch are divided among up to GMAX_GRP
// groups of equal height; a group has its own result and up to GMAX_SEG (A, B) operand pairs whose products are summed
// - the K loop runs over the segments one after the other.  All pairs share the index maps of GemmArgs (M = rows of
// one group, K = length of one segment).  am / bm: byte flags of the 64 x 16 tiles of the segment's operands (row of
// tile t at t * pitch), null = all occupied.
constexpr int GMAX_GRP = 8, GMAX_SEG = 4, GMAX_MIX = 8;
struct GMix {             // epilogue mix term (GroupedMixTerm)
  const double* src;
  int b, f, delta, pad;
};
struct GSeg {
  const double* A;
  const double* B;
  const unsigned char* am;
  const unsigned char* bm;
};
struct GGrp {
  GSeg seg[GMAX_SEG];
  double* C;
  int nseg;
  int use_beta;
};
struct GemmGroups {
  GGrp g[GMAX_GRP];
  int ngrp, tiles_m_grp, nkt_seg, am_pitch, bm_pitch;
  // split2: every output tile is computed by TWO workgroups, each over half of the tile's OCCUPIED K tiles: the first
  // half (with the beta term) is stored to C, the second to C2, laid out like C - the CONSUMER of the result adds the
  // two (the Lanczos update reads both; floating-point atomics onto one result measured slower than the launch they
  // were to speed up: 16 K eight-byte atomics per workgroup).  For block-sparse products with one tile per compute
  // unit: such a launch is as slow as its fullest tile, and a lone workgroup leaves the matrix pipe idle between its
  // MFMAs; the halves of heavy and light tiles are paired per compute unit through the launch order (cpd = compute
  // units per die, perm = tiles by decreasing weight).  DESIGN.md 4.1.
  int split2, cpd;
  double* C2;
  // optional: the flags of every tile's concatenated K range, assembled once (k_tile_order, kept with the launch order
  // for the solve): nkw words per tile, tile = (group's tile row, tile column) in launch-independent order
  const unsigned long long* flags;
  // epilogue mix (complex x complex; mpse_internal.h GroupedDesc): group mix_grp takes as its beta term
  //   sum_t W[b_t, x, x + delta_t, f_t] src_t[row + delta_t, column],  x = row mod mix_d (64 % mix_d == 0)
  // - a plane of the folded one-site matvec that is only ever accumulated onto, formed where it is consumed
  int nmix, mix_grp, mix_d, mix_wr;
  long long mix_ld;
  const double* mix_w;
  GMix mix[GMAX_MIX];
  // result mask (MatvecReq::OutMask; one group, the launch carries the dot request): the caller reads the result only
  // where omask says - rows of om_d * N elements, the product's rows being (a, sigma), sigma < om_d.  k_tile_order marks
  // the tiles that lie wholly outside (mpse_plans.h out_tile_live) in the launch order as ~tile: their workgroups store
  // a zero dot partial and nothing else.
  const unsigned char* omask;
  int om_pitch, om_d;
  int dot4;     // eight-wave form: the dot partial in the summation order of the four-wave form (see the epilogue)
};

struct GemmArgs {
  const double* A;
  const double* B;
  double* C;
  IdxMap mA, kA, kB, nB, mC, nC;
  long long sbA, sbB, sbC;  // batch strides in elements
  int M, N, K;
  int tiles_m, tiles_n;     // workgroup tiles
  int mtiles_m, mtiles_n;   // 64 x 64 tiles (granularity of the occupancy masks)
  int a_kfast, b_kfast;
  int conjA, conjB;
  int use_beta;
  double alpha_re, alpha_im, beta_re, beta_im;
  int skew;            // tile column = (column of the linear index + tile row) mod tiles_n
  int die_group;       // 0: off, 1: a die owns whole tile rows, 2: whole tile columns (see the kernel)
  int slice_fast;      // split-K, batch == 1: launch position = tile * ksplit + slice
  const int* perm;     // optional: linear tile index by launch position, tiles with the most K tiles first
  int ksplit;          // number of K slices (1 = none)
  int kt_per_split;    // k-tiles per slice
  double* ws;          // split-K partial sums: [batch][ksplit][M][N] compact, dtype of C
  // structural-zero skipping (optional, single-level K maps only): byte kt of amask[(b * tiles_m + tm) * nkw * 8 ..]
  // is 1 if tile (tm, k-tile kt) of A holds a non-zero element, 0 otherwise; bmask likewise per column tile.
  // (nkw 64-bit words of 8 flags per tile row.)  K tiles where either operand tile is entirely zero are never
  // loaded or multiplied.
  const unsigned long long* amask;
  const unsigned long long* bmask;
  int nkw;
  unsigned long long* kt_counter;   // profiling only: every workgroup adds the number of K tiles it multiplied
  const int* skip;                  // optional device flag: non-zero -> the launch does nothing (SolveScope::skip)
  // optional (batch == 1): the kernel that stores the final values of C also accumulates sum conj(C) . y over its
  // share of C (y laid out like C) and stores one (re, im) partial per workgroup at dot_part - the Lanczos
  // coefficient alpha_j = <H v_j, v_j> without a pass of its own over the two vectors
  const double* dot_y;
  double* dot_part;
  // optional (batch == 1): the beta term is read from here (own index maps) instead of from C - a product that
  // accumulates onto a slice of another tensor needs no copy of that slice into C first
  const double* Cin;
  IdxMap mCin, nCin;
  unsigned long long* trace;        // debug timeline (mpse_ctx::gemm_trace), null normally
  GemmGroups gg;                    // GRP instantiations only
};


// (re, im) += conj(c) * y
__device__ __forceinline__ void dot_acc(double& re, double& im, double2 c, double2 y) {
  re += c.x * y.x + c.y * y.y;
  im += c.x * y.y - c.y * y.x;
}

__device__ __forceinline__ long long idx_off(const IdxMap& m, int i) {
  // single-level maps are canonicalised on the host to lo == INT_MAX: skip the integer division (uniform branch)
  if (m.lo == 0x7fffffff) return (long long)i * m.s_lo;
  const int hi = i / m.lo;
  const int l = i - hi * m.lo;
  return (long long)hi * m.s_hi + (long long)l * m.s_lo;
}

// One element of the result, shared by the kernel's epilogue and the split-K reduction: o = alpha x, o += beta c0
__device__ __forceinline__ double2 alpha_times(const GemmArgs& g, double xr, double xi) {
  double2 o;
  o.x = g.alpha_re * xr - g.alpha_im * xi;
  o.y = g.alpha_re * xi + g.alpha_im * xr;
  return o;
}
__device__ __forceinline__ void add_beta(const GemmArgs& g, double2& o, double2 c0) {
  o.x += g.beta_re * c0.x - g.beta_im * c0.y;
  o.y += g.beta_re * c0.y + g.beta_im * c0.x;
}

// one element of an operand or of a partial sum: complex as one 16-byte load, real with a zero imaginary part
template <bool CPLX>
__device__ __forceinline__ double2 load_elem(const double* p) {
  if constexpr (CPLX) return *reinterpret_cast<const double2*>(p);
  return make_double2(*p, 0.0);
}

// one record of the debug timeline (MPSE_GEMM_TRACE), written by one thread of a workgroup as it leaves the kernel
__device__ __forceinline__ void trace_record(const GemmArgs& g, bool ca, bool cb, unsigned long long t0,
                                             unsigned long long rt0, unsigned long long t1, unsigned long long t2,
                                             unsigned long long t3, int ktd) {
  const unsigned long long slot = atomicAdd(g.trace, 1ull);
  if (slot >= GEMM_TRACE_CAP) return;
  unsigned long long* r = g.trace + 1 + slot * GEMM_TRACE_WORDS;
  r[0] = ((unsigned long long)gridDim.x << 32) | (unsigned long long)blockIdx.x;
  r[1] = ((unsigned long long)(ca ? 1 : 0) << 62) | ((unsigned long long)(cb ? 1 : 0) << 61) |
         ((unsigned long long)g.ksplit << 40) | ((unsigned long long)(unsigned)g.K << 8);
  // where the workgroup ran: HW_ID (wave / SIMD / CU / SH / SE fields) and the die (XCC_ID)
  const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
  r[2] = (unsigned long long)(unsigned)ktd | ((unsigned long long)(((xc & 0xf) << 16) | (hw & 0xffff)) << 32);
  r[3] = t0;
  r[4] = t1;
  r[5] = t2;
  r[6] = t3;
  r[7] = __builtin_readcyclecounter();
  r[8] = rt0;
  r[9] = __builtin_amdgcn_s_memrealtime();
}

constexpr int BM = 64, BN = 64, BK = 16, LDK = BK + 1;   // BM x BN: granularity of the tile-occupancy masks

// The MFMAs of one 16 x 16 sub-tile on one k-group (4 of K).  complex x complex uses the 3M scheme (three real products
// per complex product instead of four):
//   T1 = Ar Br, T2 = Ai Bi, T3 = (Ar + Ai)(Br + Bi)  =>  re = T1 - T2, im = T3 - T1 - T2
// re holds T1, im holds T3, t2 holds T2 until the epilogue combines them; as / bs: the sums, formed once per k-group.
// complex x real: two products, real x real: one.
template <bool CA, bool CB>
__device__ __forceinline__ void mfma_subtile(const double& ar, const double& ai, const double& br, const double& bi,
                                             const double& as, const double& bs, v4d& re, v4d& im, v4d& t2) {
  re = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, re, 0, 0, 0);
  if constexpr (CA && CB) {
    t2 = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, t2, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f64_16x16x4f64(as, bs, im, 0, 0, 0);
  } else if constexpr (CA) {
    im = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, im, 0, 0, 0);
  } else if constexpr (CB) {
    im = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, im, 0, 0, 0);
  }
}

// KS: both K maps are single level -> no integer division in the K loop
// WI: 16-row blocks of the 64 x 64 output tile per wave.  2: four waves of 32 x 32 (the default).  1: eight
// waves of 16 x 32 on the same tile - for launches that put ONE workgroup on a compute unit, so that every
// SIMD still has two waves to overlap fragment reads, staging and address arithmetic with the other's MFMAs.
// GRP: grouped launch (GemmGroups; batch == 1, unsplit, KS, K a multiple of BK, M a multiple of the tile height).
template <bool CA, bool CB, bool KS, int WI = 2, bool GRP = false>
__global__ __launch_bounds__(256 * (2 / WI), WI == 1 ? 4 : ((CA && CB) ? 2 : 3)) void k_gemm(const GemmArgs g) {
  static_assert(!GRP || KS, "grouped launches use the single-level kernel");
  static_assert(WI == 1 || WI == 2, "four or eight waves");
  constexpr int NT = 256 * (2 / WI);
  constexpr int LD = 80;                         // [k][i] panel rows; LD mod 32 == 16 keeps the fragment reads conflict free
  constexpr int NLD = BM * BK / NT;              // staged elements per thread and operand (panel = BK*LD >= BM*LDK doubles)
  constexpr bool CC = CA || CB;
  constexpr int EA = CA ? 2 : 1, EB = CB ? 2 : 1, EC = CC ? 2 : 1;
  // one LDS object: [Are | Aim? | Bre | Bim?], each BK x LD doubles
  __shared__ double smem[(2 + (CA ? 1 : 0) + (CB ? 1 : 0)) * BK * LD];
  if (g.skip && *g.skip) return;   // workgroup-uniform
  const unsigned long long tr0 = g.trace ? __builtin_readcyclecounter() : 0ull;
  const unsigned long long rt0 = g.trace ? __builtin_amdgcn_s_memrealtime() : 0ull;   // device-wide 100 MHz clock
  unsigned long long tr1 = 0, tr2 = 0, tr3 = 0;
  double* sAr = smem;
  double* sAi = sAr + BK * LD;  // only meaningful if CA
  double* sBr = smem + (CA ? 2 : 1) * BK * LD;
  double* sBi = sBr + BK * LD;  // only meaningful if CB

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;   // WI == 1: wm = 0 .. 3
  constexpr int WROWS = 16 * WI;         // rows of the output tile per wave

  const int ntile = g.tiles_m * g.tiles_n;
  const int bid = blockIdx.x;
  // ---- tile of this position: launch position -> (batch, K slice, tile, half of a halved tile), mpse_gemm_tiles.h
  int bs, t, half;
  mpse_tiles::launch_position(g, GRP, bid, ntile, bs, t, half);
  const int b = bs / g.ksplit;
  const int ks_id = bs - b * g.ksplit;
  bool dead = false;                     // grouped launch with a result mask: nobody reads this tile
  if (g.perm) {                          // heaviest tiles first (k_tile_order)
    t = g.perm[mpse_tiles::order_index(t, ks_id, ntile)];
    if constexpr (GRP) mpse_tiles::order_decode(t, t, dead);
  }
  int tm = t / g.tiles_n;
  int tn = t - tm * g.tiles_n;
  if constexpr (GRP) {
    // (workgroup-uniform; before anything of the operands, the beta term, the mix or the dot partner is asked for.
    // The partial's slot is the tile's, as in the epilogue: the sum over the slots keeps its order.)
    if (dead) {
      if (g.dot_y && tid == 0) {
        const long long slot = (long long)bs * ntile + t;
        g.dot_part[2 * slot] = 0.0;
        g.dot_part[2 * slot + 1] = 0.0;
      }
      if (g.trace && tid == 0) trace_record(g, CA, CB, tr0, rt0, tr0, tr0, tr0, 0);   // (an empty workgroup of the timeline)
      return;
    }
  }
  MPSE_TILES_PLACE(g, t, tm, tn);       // die groups, skew
  // grouped launch: the tile row picks the group, the rest of the kernel sees the group's own rows
  int grp = 0;
  if constexpr (GRP) {
    grp = mpse_tiles::group_of_row(tm, g.gg.tiles_m_grp);
    tm -= grp * g.gg.tiles_m_grp;
  }
  // ---- operands of the batch element / of the group
  const GGrp& gp = g.gg.g[grp];          // (kernel-argument memory; touched by GRP instantiations only)
  const double* A = GRP ? gp.seg[0].A : g.A + (long long)b * g.sbA * EA;
  const double* B = GRP ? gp.seg[0].B : g.B + (long long)b * g.sbB * EB;
  // (halved tiles: the second half of every tile goes to the second result, without the beta term)
  double* C = GRP ? (half ? g.gg.C2 : gp.C) : g.C + (long long)b * g.sbC * EC;

  // ---- per-thread staging coordinates (4 elements of each operand tile)
  int ai[NLD], ak[NLD], bj[NLD], bk[NLD];
  long long aoff[NLD], boff[NLD];
#pragma unroll
  for (int r = 0; r < NLD; ++r) {
    if (g.a_kfast) {
      ak[r] = tid % BK;
      ai[r] = tid / BK + (NT / BK) * r;
    } else {
      ai[r] = tid % BM;
      ak[r] = tid / BM + (NT / BM) * r;
    }
    if (g.b_kfast) {
      bk[r] = tid % BK;
      bj[r] = tid / BK + (NT / BK) * r;
    } else {
      bj[r] = tid % BN;
      bk[r] = tid / BN + (NT / BN) * r;
    }
    // rows / columns past the edge read a clamped (valid) address: they only feed outputs that
    // are never stored, so no predication is needed and every load below is unconditional
    int gi = min(tm * BM + ai[r], g.M - 1);
    int gj = min(tn * BN + bj[r], g.N - 1);
    aoff[r] = idx_off(g.mA, gi);
    boff[r] = idx_off(g.nB, gj);
  }

  double2 ra[NLD], rb[NLD];
  bool ka_in[NLD], kb_in[NLD];
  const int nkt_seg = GRP ? g.gg.nkt_seg : 0;
  const int nkt_all = GRP ? gp.nseg * nkt_seg : (g.K + BK - 1) / BK;
  int kt_begin = GRP ? 0 : ks_id * g.kt_per_split;
  int kt_end = GRP ? nkt_all : min(nkt_all, kt_begin + g.kt_per_split);
  // fast path (single-level K maps; the launcher guarantees non-negative strides and operand spans below 4 GB):
  // a uniform tile base (scalar registers, recomputed from the tile number) plus one 32-bit byte offset per lane and
  // staged element - the global_load saddr + voffset form: no per-lane 64-bit pointers to keep and to advance
  unsigned int loa[NLD], lob[NLD];
  const char* a_row0 = nullptr;
  const char* b_col0 = nullptr;
  long long step_a = 0, step_b = 0;
  if constexpr (KS) {
    // tile bases = the smallest row / column offset of the tile.  Inside one group of a two-level map the offset
    // grows with the index (strides >= 0), so the minimum sits at the first row or at the first row of a later group:
    // a short uniform loop over the group starts inside the tile (scalar code, no LDS, no barrier)
    auto tile_min = [&](const IdxMap& m, int first, int count, int ext) -> long long {
      const int last = min(first + count, ext);          // exclusive
      long long best = idx_off(m, min(first, ext - 1));
      if (m.lo != 0x7fffffff) {
        for (int r = (first / m.lo + 1) * m.lo; r < last; r += m.lo) best = min(best, idx_off(m, r));
      }
      return best;
    };
    const long long a0 = tile_min(g.mA, tm * BM, BM, g.M), b0 = tile_min(g.nB, tn * BN, BN, g.N);
    a_row0 = reinterpret_cast<const char*>(A + a0 * EA);
    b_col0 = reinterpret_cast<const char*>(B + b0 * EB);
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      loa[r] = (unsigned int)((aoff[r] - a0 + (long long)ak[r] * g.kA.s_lo) * EA * 8);
      lob[r] = (unsigned int)((boff[r] - b0 + (long long)bk[r] * g.kB.s_lo) * EB * 8);
    }
    step_a = (long long)BK * g.kA.s_lo * EA * 8;   // bytes per K tile
    step_b = (long long)BK * g.kB.s_lo * EB * 8;
  }
  // grouped launch: tile bases of every segment's operands (uniform), selected by the segment a K tile falls into
  const char* seg_a[GMAX_SEG];
  const char* seg_b[GMAX_SEG];
  if constexpr (GRP) {
#pragma unroll
    for (int q = 0; q < GMAX_SEG; ++q) {
      const int qq = q < gp.nseg ? q : 0;
      seg_a[q] = a_row0 + (reinterpret_cast<const char*>(gp.seg[qq].A) - reinterpret_cast<const char*>(A));
      seg_b[q] = b_col0 + (reinterpret_cast<const char*>(gp.seg[qq].B) - reinterpret_cast<const char*>(B));
    }
  }
  auto seg_pick = [&](const char* const(&arr)[GMAX_SEG], int q) {
    return q == 0 ? arr[0] : q == 1 ? arr[1] : q == 2 ? arr[2] : arr[3];
  };
  // every k of the tile is < K
  auto load_full = [&](int kt) {
    const char* at = a_row0 + (long long)kt * step_a;
    const char* bt = b_col0 + (long long)kt * step_b;
    if constexpr (GRP) {
      const int q = kt / nkt_seg, l = kt - q * nkt_seg;
      at = seg_pick(seg_a, q) + (long long)l * step_a;
      bt = seg_pick(seg_b, q) + (long long)l * step_b;
    }
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      if constexpr (CA) {
        ra[r] = *reinterpret_cast<const double2*>(at + loa[r]);
      } else {
        ra[r].x = *reinterpret_cast<const double*>(at + loa[r]);
        ra[r].y = 0.0;
      }
      if constexpr (CB) {
        rb[r] = *reinterpret_cast<const double2*>(bt + lob[r]);
      } else {
        rb[r].x = *reinterpret_cast<const double*>(bt + lob[r]);
        rb[r].y = 0.0;
      }
    }
  };
  // ---- loader: K tile kt of both operands -> staging registers
  auto load_tile = [&](int kt) {
    if constexpr (GRP) {
      load_full(kt);
    } else if constexpr (KS) {
      if ((kt + 1) * BK <= g.K) {
        load_full(kt);
      } else {   // (at most the last K tile of a product) lanes past K skip the load and stage zeros
        const char* at = a_row0 + (long long)kt * step_a;
        const char* bt = b_col0 + (long long)kt * step_b;
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
          const bool ina = kt * BK + ak[r] < g.K, inb = kt * BK + bk[r] < g.K;
          ra[r] = make_double2(0.0, 0.0);
          rb[r] = make_double2(0.0, 0.0);
          if (ina) {
            if constexpr (CA)
              ra[r] = *reinterpret_cast<const double2*>(at + loa[r]);
            else
              ra[r].x = *reinterpret_cast<const double*>(at + loa[r]);
          }
          if (inb) {
            if constexpr (CB)
              rb[r] = *reinterpret_cast<const double2*>(bt + lob[r]);
            else
              rb[r].x = *reinterpret_cast<const double*>(bt + lob[r]);
          }
        }
      }
    } else {     // general maps: an offset per element, also for the (only possibly partial) last K tile
#pragma unroll
      for (int r = 0; r < NLD; ++r) {
        {
          const int k = kt * BK + ak[r];
          const bool kin = k < g.K;
          const int kc = kin ? k : g.K - 1;
          const long long ko = idx_off(g.kA, kc);
          const double* p = A + (aoff[r] + ko) * EA;
          double2 v;
          if constexpr (CA) {
            v = *reinterpret_cast<const double2*>(p);
          } else {
            v.x = *p;
            v.y = 0.0;
          }
          ra[r] = v;       // zeroing of k >= K happens at LDS-write time: nothing here consumes the load,
          ka_in[r] = kin;  // so the waitcnt for it lands after the MFMA block of the current tile
        }
        {
          const int k = kt * BK + bk[r];
          const bool kin = k < g.K;
          const int kc = kin ? k : g.K - 1;
          const long long ko = idx_off(g.kB, kc);
          const double* p = B + (boff[r] + ko) * EB;
          double2 v;
          if constexpr (CB) {
            v = *reinterpret_cast<const double2*>(p);
          } else {
            v.x = *p;
            v.y = 0.0;
          }
          rb[r] = v;
          kb_in[r] = kin;
        }
      }
    }
  };
  const double sgn_a = g.conjA ? -1.0 : 1.0, sgn_b = g.conjB ? -1.0 : 1.0;

  // accumulators (complex x complex: the three products of the 3M scheme, mfma_subtile)
  constexpr bool M3 = CA && CB;
  v4d acc_re[WI][2], acc_im[WI][2], acc_t2[WI][2];
#pragma unroll
  for (int i = 0; i < WI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      acc_re[i][j] = v4d{0, 0, 0, 0};
      acc_im[i][j] = v4d{0, 0, 0, 0};
      acc_t2[i][j] = v4d{0, 0, 0, 0};
    }

  // ---- flags into LDS.  The flag words of this workgroup's tile row / column are fetched once (up to MASKW words each): read
  // from global memory inside the K loop they put an L2 round trip in front of every tile's loads.
  constexpr int MASKW = 64;
  __shared__ unsigned long long s_mask[2][MASKW];
  const unsigned long long* am = nullptr;
  const unsigned long long* bm = nullptr;
  bool mlds = false;   // the flag words are in LDS (read with ds_read: a generic pointer would make every look-up a
                       // flat load, whose wait drains the operand loads in flight as well)
  if constexpr (GRP) {
    // flags of the concatenated K range of this tile, assembled from the segments' operand masks (g.nkw = words of
    // that range when any segment has a mask, else 0)
    if (g.nkw > 0 && g.nkw <= MASKW && g.gg.flags) {
      if (tid < g.nkw) {
        s_mask[0][tid] = g.gg.flags[((long long)(grp * g.gg.tiles_m_grp + tm) * g.tiles_n + tn) * g.nkw + tid];
        s_mask[1][tid] = 0x0101010101010101ull;
      }
      __syncthreads();
      mlds = true;
      am = s_mask[0];
    } else if (g.nkw > 0 && g.nkw <= MASKW) {
      unsigned char* f0 = reinterpret_cast<unsigned char*>(s_mask[0]);
      for (int t = tid; t < g.nkw * 8; t += NT) {
        unsigned char v = 0;
        if (t < nkt_all) {
          const int q = t / nkt_seg, l = t - q * nkt_seg;
          const GSeg& sg = gp.seg[q];
          v = 1;
          if (sg.am) v &= sg.am[(long long)tm * g.gg.am_pitch + l];
          if (sg.bm) v &= sg.bm[(long long)tn * g.gg.bm_pitch + l];
        }
        f0[t] = v;
      }
      if (tid < g.nkw) s_mask[1][tid] = 0x0101010101010101ull;
      __syncthreads();
      mlds = true;
      am = s_mask[0];       // (non-null: look-ups go through the LDS copy)
    }
    if (g.gg.split2) {
      // this workgroup's half: occupied K tiles [n half / 2, n (half + 1) / 2) of the tile (every thread walks the
      // same flag words); without masks the K range itself is halved
      if (mlds) {
        auto word_at = [&](int w) { return mpse_tiles::trim_flags(s_mask[0][w], w, nkt_all); };
        int n = 0;
        for (int w = 0; w < g.nkw; ++w) n += __popcll(word_at(w));
        const mpse_tiles::FlaggedPos<decltype(word_at)> pos_of{n, g.nkw, nkt_all, word_at};
        kt_begin = half == 0 ? 0 : pos_of(n / 2);
        kt_end = half == 0 ? pos_of(n / 2) : nkt_all;
      } else {
        kt_begin = half == 0 ? 0 : nkt_all / 2;
        kt_end = half == 0 ? nkt_all / 2 : nkt_all;
      }
    }
  } else if constexpr (KS) {
    // masks are kept per 64 rows / columns whatever the workgroup tile
    if (g.amask) am = g.amask + ((long long)b * g.mtiles_m + tm) * g.nkw;
    if (g.bmask) bm = g.bmask + ((long long)b * g.mtiles_n + tn) * g.nkw;
    if ((am || bm) && g.nkw <= MASKW) {
      if (tid < g.nkw) {
        s_mask[0][tid] = am ? am[tid] : 0x0101010101010101ull;
        s_mask[1][tid] = bm ? bm[tid] : 0x0101010101010101ull;
      }
      __syncthreads();
      mlds = true;
    }
  }
  auto next_kt = [&](int from) -> int {
    if (!am && !bm) return from;
    return mpse_tiles::next_flagged(from, kt_end, [&](int w) {
      unsigned long long word = mpse_tiles::FLAGS_ALL;
      if (mlds) {
        word &= s_mask[0][w] & s_mask[1][w];
      } else {
        if (am) word &= am[w];
        if (bm) word &= bm[w];
      }
      return word;
    });
  };
  int kt = next_kt(kt_begin);
  if (g.trace) tr1 = __builtin_readcyclecounter();
  if (kt < kt_end) load_tile(kt);
  const int frow = lane & 15, fk = lane >> 4;
  // LDS strides (in doubles) of element (i, k) of each panel
  const int sai = g.a_kfast ? LDK : 1, sak = g.a_kfast ? 1 : LD;
  const int sbj = g.b_kfast ? LDK : 1, sbk = g.b_kfast ? 1 : LD;
  int wofa[NLD], wofb[NLD], rofa[WI], rofb[2];
#pragma unroll
  for (int r = 0; r < NLD; ++r) {
    wofa[r] = ai[r] * sai + ak[r] * sak;
    wofb[r] = bj[r] * sbj + bk[r] * sbk;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (i < WI) rofa[i] = (wm * WROWS + i * 16 + frow) * sai + fk * sak;
    rofb[i] = (wn * 32 + i * 16 + frow) * sbj + fk * sbk;
  }

  // operand fragments of one k-group (4 of K): double buffered so that the ds_reads of group kk+1 are in
  // flight under the 16 MFMAs of group kk
  double f_ar[2][WI], f_ai[2][WI], f_br[2][2], f_bi[2][2];
  auto read_frag = [&](int buf, int kk) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i < WI) {
        f_ar[buf][i] = sAr[rofa[i] + kk * 4 * sak];
        if constexpr (CA) f_ai[buf][i] = sAi[rofa[i] + kk * 4 * sak];
      }
      f_br[buf][i] = sBr[rofb[i] + kk * 4 * sbk];
      if constexpr (CB) f_bi[buf][i] = sBi[rofb[i] + kk * 4 * sbk];
    }
  };
  // staged registers -> LDS panels
  auto stage_to_lds = [&]() {
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      if constexpr (KS) {  // out-of-range k were staged as zeros by load_tile
        sAr[wofa[r]] = ra[r].x;
        if constexpr (CA) sAi[wofa[r]] = sgn_a * ra[r].y;
        sBr[wofb[r]] = rb[r].x;
        if constexpr (CB) sBi[wofb[r]] = sgn_b * rb[r].y;
      } else {
        sAr[wofa[r]] = ka_in[r] ? ra[r].x : 0.0;
        if constexpr (CA) sAi[wofa[r]] = ka_in[r] ? sgn_a * ra[r].y : 0.0;
        sBr[wofb[r]] = kb_in[r] ? rb[r].x : 0.0;
        if constexpr (CB) sBi[wofb[r]] = kb_in[r] ? sgn_b * rb[r].y : 0.0;
      }
    }
  };
  // The 16 (x3 / x2 / x1) MFMAs of a k-group on fragment buffer cb.  `staging` (the last k-group of a tile, KS
  // variants): with the staging stores of the next tile between them, one register of each operand per output sub-tile.
  auto mfma_group = [&](int cb, auto staging) {
    double as[WI], bs[2];
    if constexpr (M3) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (i < WI) as[i] = f_ar[cb][i] + f_ai[cb][i];
        bs[i] = f_br[cb][i] + f_bi[cb][i];
      }
    }
#pragma unroll
    for (int i = 0; i < WI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        mfma_subtile<CA, CB>(f_ar[cb][i], f_ai[cb][i], f_br[cb][j], f_bi[cb][j], as[i], bs[j], acc_re[i][j], acc_im[i][j],
                             acc_t2[i][j]);
        if constexpr (decltype(staging)::value) {
          constexpr int PER = NLD / 4 > 0 ? NLD / 4 : 1;
#pragma unroll
          for (int q = 0; q < PER; ++q) {
            const int r = (2 * i + j) * PER + q;
            if (r < NLD) {
            sAr[wofa[r]] = ra[r].x;
            if constexpr (CA) sAi[wofa[r]] = sgn_a * ra[r].y;
            sBr[wofb[r]] = rb[r].x;
            if constexpr (CB) sBi[wofb[r]] = sgn_b * rb[r].y;
            }
          }
          // pin the interleave: the MFMAs of this sub-tile, then its staging stores (left alone the scheduler issues
          // the MFMAs first and the stores in a block behind them)
          constexpr int NM = M3 ? 3 : (CA || CB) ? 2 : 1;
          __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
          __builtin_amdgcn_sched_group_barrier(0x200, (2 + (CA ? 1 : 0) + (CB ? 1 : 0)) * PER, 0);
        }
      }
  };
  constexpr std::false_type plain{};
  constexpr std::true_type with_staging{};

  // ---- K loop
  int kt_done = 0;
  if constexpr (KS) {
    // Software-pipelined K loop.  A wave issues in order: every instruction that is not an MFMA and sits between the
    // last MFMA of one K tile and the first of the next (barrier, staging stores, barrier, mask look-up, pointer
    // updates, loads, first fragment reads) is time the matrix pipe idles unless a second workgroup on the CU fills it
    // - 1460 of 4530 cycles per tile for a workgroup alone on its CU (tools/gemm_trace.py).  So the last k-group of a
    // tile is multiplied AFTER the barrier that frees the panels, interleaved with the staging stores of the next
    // tile; the loads of the tile after that are issued under the first k-group of the next iteration.
    int nk = kt_end;
    if (kt < kt_end) {
      stage_to_lds();
      nk = next_kt(kt + 1);
      if (nk < kt_end) load_tile(nk);
      lds_barrier();
      if (g.trace) tr2 = __builtin_readcyclecounter();
      read_frag(0, 0);
    }
    const bool any = kt < kt_end;
    while (nk < kt_end) {          // tile kt has a successor (single-exit loop: an exit in the middle made the
      ++kt_done;                   // compiler keep two copies of the accumulators and spill)
      read_frag(1, 1);
      mfma_group(0, plain);
      read_frag(0, 2);
      mfma_group(1, plain);
      read_frag(1, 3);
      mfma_group(0, plain);
      lds_barrier();               // every wave holds its last fragments: the panels may be overwritten
      mfma_group(1, with_staging); // the MFMAs of the last k-group, the staging stores of tile nk between them
      // the tile after nk (mask words in LDS: no global load is waited for); its loads stay in flight across the
      // barrier (lds_barrier does not wait for them) and across the next iteration's MFMAs
      const int after = next_kt(nk + 1);
      if (after < kt_end) load_tile(after);
      kt = nk;
      nk = after;
      lds_barrier();               // panels of the next tile complete
      read_frag(0, 0);
    }
    if (any) {                     // last tile: nothing left to stage
      ++kt_done;
      read_frag(1, 1);
      mfma_group(0, plain);
      read_frag(0, 2);
      mfma_group(1, plain);
      read_frag(1, 3);
      mfma_group(0, plain);
      mfma_group(1, plain);
    }
  } else {
  while (kt < kt_end) {
    ++kt_done;
    __syncthreads();
    if (g.trace && kt_done == 1) tr2 = __builtin_readcyclecounter();
    stage_to_lds();
    __syncthreads();
    const int nk = next_kt(kt + 1);
    if (nk < kt_end) load_tile(nk);
    kt = nk;

    read_frag(0, 0);
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      const int cb = kk & 1;
      if (kk + 1 < BK / 4) read_frag(cb ^ 1, kk + 1);
      mfma_group(cb, plain);
    }
  }
  }

  if (g.trace) tr3 = __builtin_readcyclecounter();
  struct TraceEnd {     // the record is written when the workgroup leaves the kernel, whichever way
    const GemmArgs& g;
    unsigned long long t0, rt0, &t1, &t2, &t3;
    int tid;
    int& ktd;
    __device__ ~TraceEnd() {
      if (g.trace && tid == 0) trace_record(g, CA, CB, t0, rt0, t1, t2, t3, ktd);
    }
  } trace_end{g, tr0, rt0, tr1, tr2, tr3, tid, kt_done};
  if (g.kt_counter && tid == 0 && kt_done) atomicAdd(g.kt_counter, (unsigned long long)kt_done);
  if constexpr (M3) {   // ---- 3M combine
#pragma unroll
    for (int i = 0; i < WI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc_im[i][j] = acc_im[i][j] - acc_re[i][j] - acc_t2[i][j];
        acc_re[i][j] = acc_re[i][j] - acc_t2[i][j];
      }
  }
  // ---- epilogue (split-K store, or: beta source, store with dot and hand-off, block dot): lane holds rows (lane>>4)+4r, column lane&15 of each 16x16 tile
  if (g.ksplit > 1) {
    // raw partial sums; alpha/beta and the strided store happen in k_splitk_reduce
    double* wsb = g.ws + (long long)bs * g.M * g.N * EC;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gj = tn * BN + wn * 32 + j * 16 + (lane & 15);
      if (gj >= g.N) continue;
#pragma unroll
      for (int i = 0; i < WI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = tm * BM + wm * WROWS + i * 16 + (lane >> 4) + 4 * r;
          if (gi >= g.M) continue;
          double* p = wsb + ((long long)gi * g.N + gj) * EC;
          if constexpr (CC)
            *reinterpret_cast<double2*>(p) = make_double2(acc_re[i][j][r], acc_im[i][j][r]);
          else
            *p = acc_re[i][j][r];
        }
    }
    return;
  }
  double dre = 0.0, dim = 0.0;
  // Two passes: first every load of the beta term and of the dot partner is issued (16 elements per lane, nothing
  // stored yet, so the loads are in flight together), then the results are formed and stored.  Interleaved with the
  // stores, the loads went out one by one (they may alias C for all the compiler knows): 30 000 cycles of epilogue
  // on the C-step of the one-site matvec, a quarter of that workgroup's life (tools/gemm_trace.py).
  // (complex x complex only: the mixed variants run three waves per SIMD on 168 registers, where the 128 registers
  // of the preloads spill; their beta / dot terms are read inside the store loop as before)
  constexpr bool PRE = CA && CB;
  double2 pre_c[PRE ? WI : 1][2][4], pre_y[PRE ? WI : 1][2][4];
  const bool need_c = GRP ? (gp.use_beta != 0 && half == 0) : g.use_beta != 0, need_y = g.dot_y != nullptr;
  // Epilogue mix: the beta term of this group is a sum of band-diagonal taps on up to GMAX_MIX tensors laid out like C
  // (rows (a, x), x = row mod d; the tile's 64 rows hold whole runs of x, so row + delta stays inside the tile where the
  // weight is not zero).  Weights per (term, tile row) are put into the LDS the K loop has left, out of range = 0.
  // A zero weight SELECTS zero - never multiplies: a source may hold anything where its own product was not asked for.
  // Loads are unconditional at clamped addresses.  One term at a time, its loads in flight together: the terms of a
  // sub-tile all at once would not fit the registers next to the accumulators.
  bool mix_on = false;
  if constexpr (GRP && PRE) mix_on = need_c && g.gg.nmix > 0 && grp == g.gg.mix_grp;   // workgroup-uniform
  if constexpr (GRP && PRE) {
    if (mix_on) {
      const int d = g.gg.mix_d;
      __syncthreads();                   // every wave has read its last fragments: the panels are free
      for (int x = tid; x < g.gg.nmix * BM; x += NT) {
        const GMix& m = g.gg.mix[x / BM];
        const int sg = (x % BM) % d, e = sg + m.delta;
        double w = 0.0;
        if (e >= 0 && e < d) w = g.gg.mix_w[(((long long)m.b * d + sg) * d + e) * g.gg.mix_wr + m.f];
        smem[x] = w;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < WI; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) pre_c[i][j][r] = make_double2(0.0, 0.0);
      for (int t = 0; t < g.gg.nmix; ++t) {
        const double* src = g.gg.mix[t].src;
        const int delta = g.gg.mix[t].delta;
        double2 v[WI][2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int gj = min(tn * BN + wn * 32 + j * 16 + (lane & 15), g.N - 1);
#pragma unroll
          for (int i = 0; i < WI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int gi = tm * BM + wm * WROWS + i * 16 + (lane >> 4) + 4 * r + delta;
              const int gc = min(max(gi, 0), g.M - 1);
              v[i][j][r] = *reinterpret_cast<const double2*>(src + ((long long)gc * g.gg.mix_ld + gj) * 2);
            }
        }
#pragma unroll
        for (int i = 0; i < WI; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double w = smem[t * BM + wm * WROWS + i * 16 + (lane >> 4) + 4 * r];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              // (one fused multiply-add per tap, taps in the order of the elementwise pass: the same bits as k_wmix)
              pre_c[i][j][r].x = w != 0.0 ? fma(w, v[i][j][r].x, pre_c[i][j][r].x) : pre_c[i][j][r].x;
              pre_c[i][j][r].y = w != 0.0 ? fma(w, v[i][j][r].y, pre_c[i][j][r].y) : pre_c[i][j][r].y;
            }
          }
      }
    }
  }
  if (PRE && (need_c || need_y)) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gj = min(tn * BN + wn * 32 + j * 16 + (lane & 15), g.N - 1);     // clamped: never stored past the edge
      const long long coffn = idx_off(g.nC, gj);
      const long long cinn = g.Cin ? idx_off(g.nCin, gj) : 0;
#pragma unroll
      for (int i = 0; i < WI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = min(tm * BM + wm * WROWS + i * 16 + (lane >> 4) + 4 * r, g.M - 1);
          const long long co = idx_off(g.mC, gi) + coffn;
          if (need_c && !mix_on) {
            const double* pin = g.Cin ? g.Cin + (idx_off(g.mCin, gi) + cinn) * EC : C + co * EC;
            if constexpr (CC)
              pre_c[i][j][r] = *reinterpret_cast<const double2*>(pin);
            else
              pre_c[i][j][r] = make_double2(*pin, 0.0);
          }
          if (need_y) {
            if constexpr (CC)
              pre_y[i][j][r] = reinterpret_cast<const double2*>(g.dot_y)[co];
            else
              pre_y[i][j][r] = make_double2(g.dot_y[co], 0.0);
          }
        }
    }
  }
  // Eight waves with the dot partial of the four-wave form (GemmGroups::dot4; whole tiles only).  There a lane sums its
  // 16 products in the order (j, i, r); here the rows i = 0 / 1 of that lane belong to the same lane of the waves
  // wm = 2 m / 2 m + 1.  The running sum goes from one to the other through LDS - even wave columns j = 0, odd wave
  // j = 0, even j = 1, odd j = 1 - so the odd waves end with the four-wave lanes' values; the even ones count as zero.
  constexpr bool HAND = GRP && PRE && WI == 1;
  bool hand = false;
  auto hslot = [&]() { return smem + 1024 + (((wm >> 1) * 2 + wn) * 64 + lane) * 2; };   // (behind the weights of the mix)
  if constexpr (HAND) {
    hand = g.gg.dot4 != 0 && need_y;   // workgroup-uniform
    if (hand) __syncthreads();         // every wave has left the K loop and the mix: the panels are free
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gj = tn * BN + wn * 32 + j * 16 + (lane & 15);
    if (gj >= g.N) continue;
    if constexpr (HAND) {
      if (hand) {
        if (wm & 1) __syncthreads();                       // the even wave's columns j are in
        if ((wm & 1) || j > 0) dre = hslot()[0], dim = hslot()[1];
      }
    }
    const long long coffn = idx_off(g.nC, gj);
#pragma unroll
    for (int i = 0; i < WI; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = tm * BM + wm * WROWS + i * 16 + (lane >> 4) + 4 * r;
        if (gi >= g.M) continue;
        const long long co = idx_off(g.mC, gi) + coffn;
        double* p = C + co * EC;
        const double xr = acc_re[i][j][r];
        if constexpr (CC) {
          const double xi = acc_im[i][j][r];
          double2 o = alpha_times(g, xr, xi);
          if (need_c) {
            double2 c0;
            if constexpr (PRE)
              c0 = pre_c[i][j][r];
            else
              c0 = *reinterpret_cast<const double2*>(g.Cin ? g.Cin + (idx_off(g.mCin, gi) + idx_off(g.nCin, gj)) * EC : C + co * EC);
            add_beta(g, o, c0);
          }
          *reinterpret_cast<double2*>(p) = o;
          if (need_y) {
            if constexpr (PRE)
              dot_acc(dre, dim, o, pre_y[i][j][r]);
            else
              dot_acc(dre, dim, o, reinterpret_cast<const double2*>(g.dot_y)[co]);
          }
        } else {
          double o = g.alpha_re * xr;
          if (need_c) o += g.beta_re * (g.Cin ? g.Cin[idx_off(g.mCin, gi) + idx_off(g.nCin, gj)] : *p);
          *p = o;
          if (need_y) dre += o * g.dot_y[co];
        }
      }
    }
    if constexpr (HAND) {
      if (hand) {
        if (!((wm & 1) && j == 1)) hslot()[0] = dre, hslot()[1] = dim;
        if (!(wm & 1)) {
          __syncthreads();
          if (j == 0) __syncthreads();                     // the odd wave's columns 0 are in
        } else if (j == 0) {
          __syncthreads();
        }
      }
    }
  }
  if constexpr (HAND) {
    if (hand && !(wm & 1)) dre = dim = 0.0;
  }
  if (g.dot_y) {   // workgroup-uniform
    // (block-wide sum for NT threads, totals to every thread; fixed order)
    __shared__ double s_dot[2 * (NT / 64)];
    dre = wave_sum(dre);
    dim = wave_sum(dim);
    if (lane == 0) {
      s_dot[2 * wave] = dre;
      s_dot[2 * wave + 1] = dim;
    }
    __syncthreads();
    dre = dim = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
      dre += s_dot[2 * w];
      dim += s_dot[2 * w + 1];
    }
    if (tid == 0) {   // slot = the tile, not the launch position: the sum order does not depend on the tile order
      const long long slot = (long long)bs * ntile + (long long)tm * g.tiles_n + tn;
      g.dot_part[2 * slot] = dre;
      g.dot_part[2 * slot + 1] = dim;
    }
  }
}

// Launch order of the output tiles of a block-sparse product.  The dispatcher hands workgroups to the eight dies
// round robin (die = launch position mod 8, checked with tools/gemm_balance.py) and to free slots in launch order.
//  * Tiles are sorted by the number of K tiles both operands occupy, most first: longest-processing-time-first
//    scheduling.  In storage order the full tiles of a quantum-number sector sit next to each other and pile up on
//    the same dies and compute units (30 K tiles on the fullest CU against 21 on average for the d = 16 A-step).
//  * Where the tile columns divide evenly among the dies, every die owns whole tile columns (chosen in a snake over
//    the columns sorted by weight, so that the dies carry equal work): its L2 then holds the column panels of B it
//    needs instead of streaming all of B (the plain sorted order raised the HBM-side traffic of the A-step by 2.5x).
// One workgroup, bitonic sorts of <= 2048 keys in LDS.
// (n: power of two <= 2048, the keys beyond the data are zero; 1024 threads, n / 2 compare-exchange pairs per step)
__device__ __forceinline__ void bitonic_desc(unsigned* key, int tid, int n) {
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < (n >> 1)) {
        const int lo = 2 * tid - (tid & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned a = key[lo], b = key[hi];
        if ((a < b) == desc) {
          key[lo] = b;
          key[hi] = a;
        }
      }
      __syncthreads();
    }
}
__device__ __forceinline__ int pow2_at_least(int x) {
  int n = 2;
  while (n < x) n <<= 1;
  return n;
}
__global__ __launch_bounds__(1024) void k_tile_order(const unsigned long long* __restrict__ amask,
                                                       const unsigned long long* __restrict__ bmask, int nkw, int nkt,
                                                       int tiles_m, int tiles_n, int by_die, int* __restrict__ perm,
                                                       const int* __restrict__ skip, const GemmGroups gg,
                                                       unsigned char* __restrict__ flags_out, int flags_pitch,
                                                       int om_M, int om_N) {
  if (skip && *skip) return;
  __shared__ unsigned key[2048], ckey[2048];
  __shared__ int colw[2048];
  __shared__ unsigned char die_of[2048], dead[2048];
  const int ntile = tiles_m * tiles_n, tid = threadIdx.x;
  const bool part = by_die && tiles_n % 8 == 0 && tiles_n <= 2048;
  for (int c = tid; c < 2048; c += 1024) colw[c] = 0;
  __syncthreads();
  for (int i = tid; i < 2048; i += 1024) {
    unsigned cnt = 0;
    dead[i] = 0;
    if (i < ntile) {
      const int tm = i / tiles_n, tn = i - tm * tiles_n;
      if (gg.ngrp > 0) {   // grouped launch: the segments of the tile row's group, byte flags per operand
        const int grp = mpse_tiles::group_of_row(tm, gg.tiles_m_grp), tml = tm - grp * gg.tiles_m_grp;
        const GGrp& G = gg.g[grp];
        // a tile outside the result mask (one group): no flags - weight 0, last in the order - and marked there
        const bool off = gg.omask && !mpse_plan::out_tile_live(gg.omask, gg.om_pitch, gg.om_d, om_N, om_M, tm, tn);
        dead[i] = off ? 1 : 0;
        for (int q = 0; q < G.nseg; ++q)
          for (int l = 0; l < gg.nkt_seg; ++l) {
            unsigned v = off ? 0 : 1;
            if (G.seg[q].am) v &= G.seg[q].am[(long long)tml * gg.am_pitch + l];
            if (G.seg[q].bm) v &= G.seg[q].bm[(long long)tn * gg.bm_pitch + l];
            cnt += v;
            if (flags_out) flags_out[(long long)i * flags_pitch + q * gg.nkt_seg + l] = (unsigned char)v;
          }
        if (flags_out)
          for (int l = G.nseg * gg.nkt_seg; l < flags_pitch; ++l) flags_out[(long long)i * flags_pitch + l] = 0;
      } else {
        for (int w = 0; w < nkw; ++w) {
          unsigned long long x = 0x0101010101010101ull;
          if (amask) x &= amask[(long long)tm * nkw + w];
          if (bmask) x &= bmask[(long long)tn * nkw + w];
          const int valid = nkt - 8 * w;                    // flag bytes past the last K tile are never written
          if (valid < 8) x &= (1ull << (8 * valid)) - 1ull;
          cnt += __popcll(x);
        }
      }
      if (part) atomicAdd(&colw[tn], (int)cnt);
    }
    key[i] = cnt;      // (<= 512 K tiles)
  }
  __syncthreads();
  if (part) {
    for (int c = tid; c < 2048; c += 1024) ckey[c] = c < tiles_n ? ((unsigned)colw[c] << 11) | (unsigned)(2047 - c) : 0u;
    __syncthreads();
    bitonic_desc(ckey, tid, pow2_at_least(tiles_n));
    for (int r = tid; r < tiles_n; r += 1024) {
      const int c = 2047 - (int)(ckey[r] & 2047u), r16 = r & 15;
      die_of[c] = (unsigned char)(r16 < 8 ? r16 : 15 - r16);          // snake over the columns by weight
    }
    __syncthreads();
  }
  for (int i = tid; i < 2048; i += 1024) {
    unsigned k = 0;
    if (i < ntile) {
      const unsigned die = part ? die_of[i % tiles_n] : 0u;
      k = (die << 28) | (key[i] << 16) | (unsigned)(0xFFFF - i);
    }
    key[i] = k;
  }
  __syncthreads();
  bitonic_desc(key, tid, pow2_at_least(ntile));
  const int per_die = ntile / 8;           // part: every die owns tiles_n / 8 columns of tiles_m tiles
  for (int i = tid; i < ntile; i += 1024) {
    const int s = part ? (7 - (i & 7)) * per_die + (i >> 3) : i;
    const int t = 0xFFFF - (int)(key[s] & 0xFFFFu);
    perm[i] = dead[t] ? ~t : t;           // (mpse_tiles::order_decode reads it)
  }
}

// C(i,j) = alpha * sum_s ws[b][s][i][j] + beta * C(i,j); slices summed in fixed order.
// One output row per blockIdx.y step (row index arithmetic is wave-uniform), threads run along j.
template <bool CC>
__global__ __launch_bounds__(256) void k_splitk_reduce(const GemmArgs g, int batch) {
  constexpr int EC = CC ? 2 : 1;
  if (g.skip && *g.skip) return;
  const long long mn = (long long)g.M * g.N;
  const int rows = g.M * batch;
  double dre = 0.0, dim = 0.0;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int b = row / g.M;
    const int i = row - b * g.M;
    const double* wrow = g.ws + ((long long)b * g.ksplit * mn + (long long)i * g.N) * EC;
    double* crow = g.C + ((long long)b * g.sbC + idx_off(g.mC, i)) * EC;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < g.N; j += gridDim.x * 256) {
      const double* w = wrow + (long long)j * EC;
      double xr = 0, xi = 0;
      int s = 0;
      // four slices in flight per thread (the loads are independent, the additions keep their fixed order)
      for (; s + 4 <= g.ksplit; s += 4) {
        const double2 v0 = load_elem<CC>(w + (long long)s * mn * EC), v1 = load_elem<CC>(w + (long long)(s + 1) * mn * EC);
        const double2 v2 = load_elem<CC>(w + (long long)(s + 2) * mn * EC), v3 = load_elem<CC>(w + (long long)(s + 3) * mn * EC);
        xr += v0.x, xi += v0.y;
        xr += v1.x, xi += v1.y;
        xr += v2.x, xi += v2.y;
        xr += v3.x, xi += v3.y;
      }
      for (; s < g.ksplit; ++s) {
        const double2 v = load_elem<CC>(w + (long long)s * mn * EC);
        xr += v.x, xi += v.y;
      }
      const long long co = idx_off(g.nC, j);
      double* p = crow + co * EC;
      const double* pin = g.Cin ? g.Cin + (idx_off(g.mCin, i) + idx_off(g.nCin, j)) * EC : p;
      if constexpr (CC) {
        double2 o = alpha_times(g, xr, xi);
        if (g.use_beta) add_beta(g, o, *reinterpret_cast<const double2*>(pin));
        *reinterpret_cast<double2*>(p) = o;
        if (g.dot_y) dot_acc(dre, dim, o, reinterpret_cast<const double2*>(g.dot_y)[idx_off(g.mC, i) + co]);
      } else {
        double o = g.alpha_re * xr;
        if (g.use_beta) o += g.beta_re * (*pin);
        *p = o;
        if (g.dot_y) dre += o * g.dot_y[idx_off(g.mC, i) + co];
      }
    }
  }
  if (g.dot_y) {   // grid-uniform; batch == 1
    block_allsum2(dre, dim);
    if (threadIdx.x == 0) {
      const long long bid = (long long)blockIdx.y * gridDim.x + blockIdx.x;
      g.dot_part[2 * bid] = dre;
      g.dot_part[2 * bid + 1] = dim;
    }
  }
}

// Tile occupancy of both GEMM operands in one launch: one wave per (k tile, 64-row tile, batch x operand); lane r
// scans the 16 k of its row and the wave stores the byte flag of the tile (1 = something non-zero).  "Rows" are
// the M index for A and the N index for B.  The sweeps' tensors are block sparse by quantum number and every
// kernel keeps their structural zeros exact, so whole tiles vanish.
struct OccOperand {
  const double* base;
  IdxMap rmap, kmap;
  int nrows, tiles, cplx, kfast;
  long long sb;
  unsigned char* flags;   // [batch][tiles][nkw * 8]
};
__global__ __launch_bounds__(256) void k_tile_occ(OccOperand oa, OccOperand ob, int K, int nkw, int batch,
                                                  const int* skip) {
  if (skip && *skip) return;
  // one wave per k tile (4 per workgroup); 16 independent loads per lane, lanes along whichever index is contiguous
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kt = blockIdx.x * 4 + wave, t = blockIdx.y;
  const bool second = (int)blockIdx.z >= batch;
  const OccOperand& o = second ? ob : oa;
  const int b = second ? blockIdx.z - batch : blockIdx.z;
  if (t >= o.tiles || kt * BK >= K) return;
  const int E = o.cplx ? 2 : 1;
  const double* base = o.base + (long long)b * o.sb * E;
  bool nz = false;
  if (o.kfast) {   // k contiguous: 16 lanes span the 16 k of a row, 4 rows per pass
    const int k = kt * BK + (lane & 15);
    const bool kin = k < K;
    const long long ko = idx_off(o.kmap, kin ? k : K - 1);
    // all 16 loads are issued before the first compare (clamped addresses instead of predicated loads)
    double v0[16], v1[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = min(t * BM + i * 4 + (lane >> 4), o.nrows - 1);
      const double* q = base + (idx_off(o.rmap, r) + ko) * E;
      v0[i] = q[0];
      v1[i] = o.cplx ? q[1] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool in = (t * BM + i * 4 + (lane >> 4)) < o.nrows && kin;
      nz |= in && (v0[i] != 0.0 || v1[i] != 0.0);
    }
  } else {         // rows contiguous: one row per lane, 16 k per lane
    const int r = t * BM + lane;
    if (r < o.nrows) {
      const double* p = base + idx_off(o.rmap, r) * E;
      double v0[16], v1[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = min(kt * BK + i, K - 1);
        const double* q = p + idx_off(o.kmap, k) * E;
        v0[i] = q[0];
        v1[i] = o.cplx ? q[1] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) nz |= (kt * BK + i < K) && (v0[i] != 0.0 || v1[i] != 0.0);
    }
  }
  const bool any = __ballot(nz) != 0ull;
  if (lane == 0) o.flags[((long long)b * o.tiles + t) * nkw * 8 + kt] = any ? 1 : 0;
}

bool to_map(const mpse_index& s, IdxMap* m) {
  if (s.ext < 0 || s.ext > 0x7fffffffLL) return false;
  m->ext = (int)s.ext;
  long long lo = s.lo_ext <= 0 ? 1 : s.lo_ext;
  m->s_hi = s.s_hi;
  m->s_lo = s.s_lo;
  // canonical single-level forms: lo >= ext ; lo == 1 (only the hi level moves) ; contiguous levels
  if (lo >= s.ext) {
    m->s_hi = 0;
  } else if (lo == 1) {
    m->s_lo = s.s_hi;
    m->s_hi = 0;
    lo = s.ext;
  } else if (s.s_hi == lo * s.s_lo) {
    m->s_hi = 0;
    lo = s.ext;
  }
  if (lo >= s.ext) lo = 0x7fffffffLL;
  m->lo = (int)lo;
  return true;
}

inline bool is_single(const IdxMap& m) { return m.lo == 0x7fffffff; }

// ---- (d0,d1,d2) -> (d0,d2,d1) copy through a 32x32 LDS tile
template <bool CPLX>
__global__ __launch_bounds__(256) void k_transpose_inner(double* out, const double* in, long long d0, int d1,
                                                         int d2, int conj) {
  constexpr int E = CPLX ? 2 : 1;
  __shared__ double tile[32][33 * E];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int t1 = (d1 + 31) / 32, t2 = (d2 + 31) / 32;
  long long bid = blockIdx.x;
  const long long b0 = bid / ((long long)t1 * t2);
  const int rem = (int)(bid - b0 * t1 * t2);
  const int by = rem / t2, bx = rem - by * t2;
  const double* src = in + b0 * (long long)d1 * d2 * E;
  double* dst = out + b0 * (long long)d1 * d2 * E;
  for (int yy = ty; yy < 32; yy += 8) {
    int y = by * 32 + yy, x = bx * 32 + tx;
    if (y < d1 && x < d2) {
      const double* p = src + ((long long)y * d2 + x) * E;
      tile[yy][tx * E] = p[0];
      if (CPLX) tile[yy][tx * E + 1] = conj ? -p[1] : p[1];
    }
  }
  __syncthreads();
  for (int yy = ty; yy < 32; yy += 8) {
    int x = bx * 32 + yy, y = by * 32 + tx;  // output row = old column
    if (y < d1 && x < d2) {
      double* p = dst + ((long long)x * d1 + y) * E;
      p[0] = tile[tx][yy * E];
      if (CPLX) p[1] = tile[tx][yy * E + 1];
    }
  }
}

// ---- pieces shared by the launchers (gemm_impl, occ_mask_get, gemm_grouped)
inline int n_cu_of(const mpse_ctx* ctx) { return ctx->n_cu > 0 ? ctx->n_cu : 256; }

// stride of the index as it moves through memory, for "which index of an operand is the contiguous one"
long long fastest(const IdxMap& m) { return m.ext <= 1 ? (long long)1 << 60 : (m.s_lo < 0 ? -m.s_lo : m.s_lo); }

// the fast kernel addresses its operands as uniform base + 32-bit lane offset: non-negative strides, spans < 4 GB
bool span_ok(const IdxMap& m, const IdxMap& k, bool cplx) {
  if (m.s_hi < 0 || m.s_lo < 0 || k.s_hi < 0 || k.s_lo < 0) return false;
  auto span = [](const IdxMap& x) {
    if (x.ext <= 1) return 0.0;
    if (x.lo == 0x7fffffff) return double(x.ext - 1) * double(x.s_lo);
    return double((x.ext - 1) / x.lo) * double(x.s_hi) + double(x.lo - 1) * double(x.s_lo);
  };
  return (span(m) + span(k) + 1.0) * (cplx ? 16.0 : 8.0) < 4.0e9;
}
bool fast_ok(const GemmArgs& g, bool ca, bool cb) { return span_ok(g.mA, g.kA, ca) && span_ok(g.nB, g.kB, cb); }

// The six index maps of a product with what follows from them: extents, tiles, staging orientation.  false: an extent
// is out of range.
// Workgroup tile: 64 x 64.  (A 32 x 32 one-wave tile for products whose 64 x 64 tiles cannot fill the chip lost to
// split-K by 17 % on the headline run - one wave walking the whole K is a longer latency chain than many workgroups
// walking two K tiles each plus a reduction pass - and was removed.)
bool fill_maps(GemmArgs& g, const mpse_index& ma, const mpse_index& ka, const mpse_index& kb, const mpse_index& nb,
               const mpse_index& mc, const mpse_index& nc) {
  if (!to_map(ma, &g.mA) || !to_map(ka, &g.kA) || !to_map(kb, &g.kB) || !to_map(nb, &g.nB) || !to_map(mc, &g.mC) ||
      !to_map(nc, &g.nC))
    return false;
  g.M = g.mA.ext, g.N = g.nB.ext, g.K = g.kA.ext;
  g.tiles_m = g.mtiles_m = (g.M + BM - 1) / BM;
  g.tiles_n = g.mtiles_n = (g.N + BN - 1) / BN;
  g.a_kfast = fastest(g.kA) <= fastest(g.mA);
  g.b_kfast = fastest(g.kB) <= fastest(g.nB);
  return true;
}

// ---- occupancy masks: flags of the 64 x 16 tiles of one operand (`batch` matrices sb elements apart, rows through
// rm, K through km), [batch][tile][nkw * 8] bytes
SolveScope::OccKey occ_key(const void* p, const IdxMap& rm, const IdxMap& km, long long sb, long long batch, bool cplx) {
  SolveScope::OccKey k;
  memset(&k, 0, sizeof(k));
  k.ptr = p;
  k.r_ext = rm.ext, k.r_lo = rm.lo, k.r_shi = rm.s_hi, k.r_slo = rm.s_lo;
  k.k_ext = km.ext, k.k_lo = km.lo, k.k_shi = km.s_hi, k.k_slo = km.s_lo;
  k.sb = sb, k.nrows = rm.ext, k.tiles = (rm.ext + BM - 1) / BM, k.nkw = ((km.ext + BK - 1) / BK + 7) / 8;
  k.batch = (int)batch, k.K = km.ext, k.cplx = cplx ? 1 : 0;
  return k;
}
size_t occ_bytes(const SolveScope::OccKey& k) { return size_t(k.batch) * k.tiles * k.nkw * 8; }

struct OccMask {
  void* mask = nullptr;
  bool scan = false;     // the flags are still to be written (k_tile_occ)
  bool stable = true;    // the mask (or its absence) outlives the call: cached or the solve's
};
// Where the mask of an operand comes from.  Inside a Krylov solve the environments do not change: the mask of an
// operand inside them (`keep` = the solve's scope where SolveScope::in_env, else null) is looked up in the scope's
// occ_cache and on a miss stored there until the scope ends.  Any other operand takes the mask the caller already has
// (`given`, null = none) or, to be scanned, `tmp` in a temporary of the caller.
int occ_mask_source(mpse_ctx* ctx, SolveScope* keep, const SolveScope::OccKey& key, const void* given, void* tmp,
                    OccMask* m) {
  m->stable = keep || given;
  if (keep)
    for (const auto& e : keep->occ_cache)
      if (memcmp(&e.key, &key, sizeof(key)) == 0) {
        m->mask = e.mask;
        return MPSE_OK;
      }
  m->scan = !given;
  if (given) {
    m->mask = const_cast<void*>(given);
  } else if (keep) {
    MPSE_TRY(mpse_malloc(ctx, occ_bytes(key), &m->mask));
    keep->occ_cache.push_back({key, m->mask});
  } else {
    m->mask = tmp;
  }
  return MPSE_OK;
}
OccOperand occ_operand(const SolveScope::OccKey& k, const IdxMap& rm, const IdxMap& km, int kfast, const OccMask& m) {
  return OccOperand{static_cast<const double*>(k.ptr), rm, km, k.nrows, m.scan ? k.tiles : 0, k.cplx, kfast, k.sb,
                    static_cast<unsigned char*>(m.mask)};
}

// ---- launch order (k_tile_order).  keep: the scope of the solve whose masks it is computed from, else null - the
// order is looked up in the scope's perm_cache (key: every field but perm) and on a miss stored there like the masks;
// otherwise it goes to `tmp`.  *sort: the order is still to be computed.
int perm_source(mpse_ctx* ctx, SolveScope* keep, SolveScope::PermEntry key, size_t bytes, TmpBuf& tmp, int** perm,
                bool* sort) {
  *sort = false;
  if (keep)
    for (const auto& e : keep->perm_cache)
      if (e.amask == key.amask && e.bmask == key.bmask && e.tiles_m == key.tiles_m && e.tiles_n == key.tiles_n &&
          e.nkt == key.nkt) {
        *perm = static_cast<int*>(e.perm);
        return MPSE_OK;
      }
  *sort = true;
  if (keep) {
    MPSE_TRY(mpse_malloc(ctx, bytes, &key.perm));
    keep->perm_cache.push_back(key);
    *perm = static_cast<int*>(key.perm);
  } else {
    MPSE_TRY(tmp.alloc(bytes));
    *perm = tmp.as<int>();
  }
  return MPSE_OK;
}

// ---- the one place where k_gemm and k_splitk_reduce are instantiated and launched: for every operand type pair the
// fast kernel with eight (`wide`) and four waves and the general kernel; for a complex second operand the two grouped
// forms of the fast kernel.  A split product whose slices are not left to its consumer is followed by its reduction
// (rgrid.x != 0).
void launch_gemm(mpse_ctx* ctx, const GemmArgs& g, long long nwg, bool ca, bool cb, bool fast, bool wide, bool grouped,
                 dim3 rgrid = dim3(0), int batch = 1) {
  using Kern = void (*)(const GemmArgs);
  static const Kern plain[4][3] = {   // [complex operands first][eight waves, four waves, general]
      {k_gemm<true, true, true, 1>, k_gemm<true, true, true>, k_gemm<true, true, false>},
      {k_gemm<true, false, true, 1>, k_gemm<true, false, true>, k_gemm<true, false, false>},
      {k_gemm<false, true, true, 1>, k_gemm<false, true, true>, k_gemm<false, true, false>},
      {k_gemm<false, false, true, 1>, k_gemm<false, false, true>, k_gemm<false, false, false>}};
  static void (*const reduce[2])(const GemmArgs, int) = {k_splitk_reduce<true>, k_splitk_reduce<false>};
  static const Kern groups[2][2] = {   // [complex first operand first][eight waves, four waves]
      {k_gemm<true, true, true, 1, true>, k_gemm<true, true, true, 2, true>},
      {k_gemm<false, true, true, 1, true>, k_gemm<false, true, true, 2, true>}};
  const int form = fast && wide ? 0 : fast ? 1 : 2;
  const Kern k = grouped ? groups[ca ? 0 : 1][form] : plain[(ca ? 0 : 2) + (cb ? 0 : 1)][form];
  hipLaunchKernelGGL(k, dim3((unsigned)nwg), dim3(form == 0 ? 512 : 256), 0, ctx->stream, g);
  if (rgrid.x) hipLaunchKernelGGL(reduce[(ca || cb) ? 0 : 1], rgrid, dim3(256), 0, ctx->stream, g, batch);
}

// the path counters of mpse_gemm_path_stats
void count_paths(long long* gp, const mpse_plan::GemmPlan& p, bool batched) {
  const bool masked = p.fast && p.masks;   // (the general kernel visits every K tile)
  ++gp[mpse_ctx::GP_LAUNCH];
  gp[mpse_ctx::GP_GENERAL] += !p.fast;
  gp[mpse_ctx::GP_WIDE] += p.wide;
  gp[mpse_ctx::GP_SPLIT_B1] += p.ksplit > 1 && !batched;
  gp[mpse_ctx::GP_SPLIT_BN] += p.ksplit > 1 && batched;
  gp[mpse_ctx::GP_DIE1] += p.die_group == 1;
  gp[mpse_ctx::GP_DIE2] += p.die_group == 2;
  gp[mpse_ctx::GP_SKEW] += !p.order && !p.die_group;
  gp[mpse_ctx::GP_ORDER] += p.order;
  gp[mpse_ctx::GP_MASK] += masked;
  gp[mpse_ctx::GP_MASK_GLOBAL] += masked && p.nkw > 64;
}
void count_paths(long long* gp, const GroupedDesc& d) {
  ++gp[mpse_ctx::GP_GROUPED];
  gp[mpse_ctx::GP_GROUPED_SPLIT2] += d.split2;
  gp[mpse_ctx::GP_GROUPED_MIX] += d.nmix > 0;
}

}  // namespace

// sc: the solve the product runs in, rq: what run_plan asks of it beyond the descriptor (both may be null)
static int gemm_impl(mpse_ctx* ctx, const mpse_gemm_desc* d, const void* A, const void* B, void* C, int skip_zero,
                     SolveScope* sc, ProductReq* rq) {
  // ---- check
  if (!ctx || !d) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if ((d->dtype_a != MPSE_F64 && d->dtype_a != MPSE_C128) || (d->dtype_b != MPSE_F64 && d->dtype_b != MPSE_C128))
    return mpse_fail(ctx, MPSE_ERR_ARG, "mpse_gemm: unknown dtype");
  if (d->m_a.ext != d->m_c.ext || d->n_b.ext != d->n_c.ext || d->k_a.ext != d->k_b.ext)
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "mpse_gemm: extents disagree (M %lld/%lld N %lld/%lld K %lld/%lld)",
                     (long long)d->m_a.ext, (long long)d->m_c.ext, (long long)d->n_b.ext, (long long)d->n_c.ext,
                     (long long)d->k_a.ext, (long long)d->k_b.ext);
  if (d->m_a.ext == 0 || d->n_b.ext == 0 || d->batch <= 0) return MPSE_OK;
  if (!A || !B || !C) return mpse_fail(ctx, MPSE_ERR_ARG, "mpse_gemm: null operand");
  GemmArgs g = {};
  g.A = (const double*)A;
  g.B = (const double*)B;
  g.C = (double*)C;
  if (!fill_maps(g, d->m_a, d->k_a, d->k_b, d->n_b, d->m_c, d->n_c))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "mpse_gemm: extent out of range");
  g.sbA = d->sb_a;
  g.sbB = d->sb_b;
  g.sbC = d->sb_c;
  const bool ca = d->dtype_a == MPSE_C128, cb = d->dtype_b == MPSE_C128;
  g.conjA = d->conj_a && ca;
  g.conjB = d->conj_b && cb;
  g.alpha_re = d->alpha_re;
  g.alpha_im = d->alpha_im;
  g.beta_re = d->beta_re;
  g.beta_im = d->beta_im;
  g.use_beta = (d->beta_re != 0.0 || d->beta_im != 0.0);
  // beta source of the caller (ProductReq::cin)
  if (rq && rq->cin) {
    if (d->batch != 1 || !g.use_beta || !to_map(rq->cin_m, &g.mCin) || !to_map(rq->cin_n, &g.nCin) ||
        g.mCin.ext != g.mC.ext || g.nCin.ext != g.nC.ext)
      return mpse_fail(ctx, MPSE_ERR_ARG, "mpse_gemm: beta source needs batch == 1, beta != 0 and the extents of C");
    g.Cin = static_cast<const double*>(rq->cin);
  }
  g.skip = sc ? sc->skip : nullptr;
  g.skew = 1;
  if (!ctx->gemm_trace_checked) {
    ctx->gemm_trace_checked = true;
    if (getenv("MPSE_GEMM_TRACE")) {
      void* pt = nullptr;
      if (hipMalloc(&pt, (1 + GEMM_TRACE_CAP * GEMM_TRACE_WORDS) * sizeof(unsigned long long)) == hipSuccess) {
        (void)hipMemsetAsync(pt, 0, sizeof(unsigned long long), ctx->stream);
        ctx->gemm_trace = static_cast<unsigned long long*>(pt);
      }
    }
  }
  g.trace = gemm_trace_ptr(ctx);

  // ---- plan
  // dot request of the caller (ProductReq::dot: run_plan passes it to the step that completes the result); slices
  // for a consumer that adds them itself (ProductReq::slices): plain product into a compact result
  MatvecReq::Dot* dot = rq ? rq->dot : nullptr;
  const bool compact = is_single(g.mC) && is_single(g.nC) && g.mC.s_lo == g.N && (g.nC.s_lo == 1 || g.N == 1);
  const bool slices = rq && rq->slices && compact && d->alpha_re == 1.0 && d->alpha_im == 0.0;
  const mpse_plan::GemmPlan p = mpse_plan::launch_plan(
      {g.M, g.N, g.K, d->batch, n_cu_of(ctx), ca, cb, skip_zero, is_single(g.kA) && is_single(g.kB), fast_ok(g, ca, cb),
       dot != nullptr, dot ? dot->cap : 0, slices, slices ? rq->slices_cap : 0, g.use_beta != 0});
  if (p.nwg > 0x7fffffffLL) return mpse_fail(ctx, MPSE_ERR_SHAPE, "mpse_gemm: grid too large");
  g.ksplit = p.ksplit;
  g.kt_per_split = p.kt_per_split;
  g.slice_fast = g.ksplit > 1 && d->batch == 1;
  g.die_group = p.die_group;
  TmpBuf WSB(ctx), MSK(ctx), PERM(ctx);
  if (p.leave_slices) {
    g.ws = static_cast<double*>(rq->slices);
    rq->slices_used = g.ksplit;
  } else if (g.ksplit > 1) {
    MPSE_TRY(WSB.alloc(p.ws_bytes));
    g.ws = WSB.as<double>();
  }
  if (p.dot_producers) {
    g.dot_y = static_cast<const double*>(dot->y);
    g.dot_part = dot->part;
    dot->nb_out = (int)p.dot_producers;
  }
  mpse_ctx::ProfRec rec;
  const int variant = (ca ? 1 : 0) + (cb ? 2 : 0);
  const double mnk = double(g.M) * double(g.N) * double(g.K) * double(d->batch);
  // algorithmic (dense-equivalent) flops; compulsory traffic: read A and B once, write C once (+ read C when beta != 0)
  const bool prof_this = prof_begin(
      ctx, variant, mnk * ((ca && cb) ? 8.0 : (ca || cb) ? 4.0 : 2.0),
      double(d->batch) * (double(g.M) * g.K * (ca ? 16 : 8) + double(g.K) * g.N * (cb ? 16 : 8) +
                          double(g.M) * g.N * ((ca || cb) ? 16 : 8) * (g.use_beta ? 2 : 1)),
      &rec);
  g.kt_counter = prof_this && ctx->prof_ktiles ? ctx->prof_ktiles + variant : nullptr;

  // ---- masks: tile occupancy of the operands the hint names (bit 0: A, bit 1: B - an operand that is as large as the
  // product itself is not worth a pass), then only K tiles with data on both sides are visited
  OccMask ma, mb;
  if (p.masks) {
    g.nkw = p.nkw;
    const bool sa = skip_zero & 1, sb = skip_zero & 2;
    const SolveScope::OccKey ka = occ_key(g.A, g.mA, g.kA, g.sbA, d->batch, ca);
    const SolveScope::OccKey kb = occ_key(g.B, g.nB, g.kB, g.sbB, d->batch, cb);
    SolveScope* const keep_a = sa && sc && sc->in_env(g.A) ? sc : nullptr;
    SolveScope* const keep_b = sb && sc && sc->in_env(g.B) ? sc : nullptr;
    // B is a Krylov vector of a solve whose caller supplied the structural mask of the centre tensor: no scan
    const void* centre = (sb && sc && sc->in_krylov(g.B) && d->batch == 1 && (long long)occ_bytes(kb) == sc->cmask.bytes)
                             ? sc->cmask.ptr : nullptr;
    // (one temporary for the masks that are not kept)
    const size_t tmp_a = sa && !keep_a ? occ_bytes(ka) : 0, tmp_b = sb && !keep_b && !centre ? occ_bytes(kb) : 0;
    if (tmp_a + tmp_b) MPSE_TRY(MSK.alloc(tmp_a + tmp_b));
    if (sa) MPSE_TRY(occ_mask_source(ctx, keep_a, ka, nullptr, MSK.p, &ma));
    if (sb) MPSE_TRY(occ_mask_source(ctx, keep_b, kb, centre, MSK.as<char>() + tmp_a, &mb));
    // (flag bytes past the last k tile stay unwritten: next_kt never looks beyond kt_end)
    if (ma.scan || mb.scan) {
      const OccOperand oa = occ_operand(ka, g.mA, g.kA, g.a_kfast, ma), ob = occ_operand(kb, g.nB, g.kB, g.b_kfast, mb);
      const dim3 og((p.nkt + 3) / 4, oa.tiles > ob.tiles ? oa.tiles : ob.tiles, (unsigned)(2 * d->batch));
      hipLaunchKernelGGL(k_tile_occ, og, dim3(256), 0, ctx->stream, oa, ob, g.K, g.nkw, (int)d->batch, g.skip);
    }
    g.amask = static_cast<const unsigned long long*>(ma.mask);
    g.bmask = static_cast<const unsigned long long*>(mb.mask);
  }

  // ---- order
  if (p.order) {
    // inside a Krylov solve both masks are the solve's (cached environment mask, structural centre mask): one sort
    // serves every matvec of the solve
    SolveScope* const keep = sc && sc->keeps_env_masks && ma.stable && mb.stable ? sc : nullptr;
    int* pp = nullptr;
    bool sort = false;
    MPSE_TRY(perm_source(ctx, keep, {g.amask, g.bmask, g.tiles_m, g.tiles_n, p.nkt, nullptr},
                         size_t(g.tiles_m) * g.tiles_n * sizeof(int), PERM, &pp, &sort));
    if (sort)
      hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, ctx->stream, g.amask, g.bmask, g.nkw, p.nkt, g.tiles_m,
                         g.tiles_n, 1, pp, g.skip, GemmGroups(), (unsigned char*)nullptr, 0, 0, 0);
    g.perm = pp;
  }

  // ---- launch
  count_paths(ctx->gemm_paths, p, d->batch > 1);
  const bool reduce = g.ksplit > 1 && !p.leave_slices;
  launch_gemm(ctx, g, p.nwg, ca, cb, p.fast, p.wide, false, reduce ? dim3((unsigned)p.rgx, (unsigned)p.rgy) : dim3(0),
              (int)d->batch);
  if (prof_this) prof_end(ctx, rec);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Tile-occupancy flags of one operand (rows through `r`, K through `k`, both from `ptr`): from the cache of the
// Krylov solve's scope, else scanned now - into that cache when the operand lies inside the solve's environment
// ranges, into `tmp` otherwise.  flags[t * pitch + kt], 64 rows per tile t.
int occ_mask_get(mpse_ctx* ctx, SolveScope* sc, const void* ptr, int dtype, mpse_index r, mpse_index k,
                 TmpBuf& tmp, const unsigned char** flags, int* pitch, bool* stable) {
  IdxMap rm, km;
  if (!to_map(r, &rm) || !to_map(k, &km) || !is_single(km))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "occupancy scan: K index must be single level");
  const SolveScope::OccKey key = occ_key(ptr, rm, km, 0, 1, dtype == MPSE_C128);
  SolveScope* const keep = sc && sc->in_env(ptr) ? sc : nullptr;
  OccMask m;
  if (!keep) MPSE_TRY(tmp.alloc(occ_bytes(key)));
  MPSE_TRY(occ_mask_source(ctx, keep, key, nullptr, tmp.p, &m));
  if (m.scan) {
    const OccOperand oa = occ_operand(key, rm, km, fastest(km) <= fastest(rm), m);
    OccOperand ob = oa;
    ob.tiles = 0;
    hipLaunchKernelGGL(k_tile_occ, dim3(((key.K + BK - 1) / BK + 3) / 4, key.tiles, 2), dim3(256), 0, ctx->stream, oa, ob,
                       key.K, key.nkw, 1, sc ? sc->skip : nullptr);
    MPSE_HIP(ctx, hipGetLastError());
  }
  *flags = static_cast<const unsigned char*>(m.mask);
  *pitch = key.nkw * 8;
  *stable = m.stable;
  return MPSE_OK;
}

// Compulsory traffic of a grouped launch (M x K first operands, K x N second, M x N results): every DISTINCT operand
// read once - the groups of the products with L share the centre tensor, which used to be counted once per group -
// every result written once, the beta term of a group read once; a group with an epilogue mix reads, in the place of
// its beta term, the distinct sources of the mix that are not operands of the launch already (the centre tensor is
// both where a plane is the centre itself).
static double grouped_bytes(const GroupedDesc& d, double M, double N, double K, bool ca) {
  const void* seen[3][GMAX_GRP * GMAX_SEG + GMAX_MIX];
  int n[3] = {0, 0, 0};
  auto fresh = [&](int w, const void* p) {
    for (int i = 0; i < n[w]; ++i)
      if (seen[w][i] == p) return false;
    seen[w][n[w]++] = p;
    return true;
  };
  double bytes = 0.0, betas = 0.0;
  for (int i = 0; i < d.ngrp; ++i) {
    for (int q = 0; q < d.grp[i].nseg; ++q) {
      if (fresh(0, d.grp[i].seg[q].A)) bytes += M * K * (ca ? 16.0 : 8.0);
      if (fresh(1, d.grp[i].seg[q].B)) bytes += K * N * 16.0;
    }
    bytes += M * N * 16.0;
    betas += d.grp[i].beta != 0.0 ? 1.0 : 0.0;
  }
  if (d.nmix > 0) {
    betas -= 1.0;
    const int w = (K == N && ca) ? 0 : 2;      // (a source is laid out like the result: the extent of a first operand when K = N)
    for (int t = 0; t < d.nmix; ++t)
      if (fresh(w, d.mix[t].src)) bytes += M * N * 16.0;
  }
  return bytes + betas * M * N * 16.0;
}

// Grouped launch of the contraction kernel (mpse_internal.h GroupedDesc; folded one-site matvec of mpse_plans.h).
// dot: the caller's dot request when this launch completes a matvec result (one group only), else null.
int gemm_grouped(mpse_ctx* ctx, const GroupedDesc& d, SolveScope* sc, MatvecReq::Dot* dot,
                 const MatvecReq::OutMask* om) {
  // ---- check
  GemmArgs g = {};
  if (d.ngrp < 1 || d.ngrp > GMAX_GRP) return mpse_fail(ctx, MPSE_ERR_ARG, "grouped product: 1 .. %d groups", GMAX_GRP);
  if (!fill_maps(g, d.ma, d.ka, d.kb, d.nb, d.mc, d.nc))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "grouped product: extent out of range");
  if (g.M != g.mC.ext || g.N != g.nC.ext || g.K != g.kB.ext) return mpse_fail(ctx, MPSE_ERR_SHAPE, "grouped product: extents disagree");
  if (g.M == 0 || g.N == 0) return MPSE_OK;
  const bool ca = d.dta == MPSE_C128, cb = d.dtb == MPSE_C128;
  if (!is_single(g.kA) || !is_single(g.kB) || !fast_ok(g, ca, cb) || g.K % BK != 0 || g.K < BK ||
      (d.ngrp > 1 && g.M % BM != 0) || !cb)
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "grouped product: needs single-level K indices, K a multiple of %d, group "
                     "heights a multiple of %d and a complex second operand", BK, BM);
  if (d.split2 && (d.ngrp != 1 || !d.c2 || g.M % BM != 0))
    return mpse_fail(ctx, MPSE_ERR_ARG, "grouped product: halved tiles need one group, whole tile rows and a second result");
  g.alpha_re = 1.0, g.beta_re = 1.0;
  g.ksplit = 1;
  g.skip = sc ? sc->skip : nullptr;
  g.skew = 1;
  g.trace = gemm_trace_ptr(ctx);
  GemmGroups& gg = g.gg;
  gg.ngrp = d.ngrp, gg.tiles_m_grp = g.mtiles_m, gg.nkt_seg = g.K / BK;
  gg.am_pitch = d.am_pitch, gg.bm_pitch = d.bm_pitch;
  gg.split2 = d.split2 ? 1 : 0;
  gg.C2 = static_cast<double*>(d.c2);
  gg.cpd = n_cu_of(ctx) / 8;
  int max_seg = 0;
  double segs = 0;
  bool any_mask = false, any_beta = false;
  for (int i = 0; i < d.ngrp; ++i) {
    const GroupedGrp& s = d.grp[i];
    if (s.nseg < 1 || s.nseg > GMAX_SEG || !s.C) return mpse_fail(ctx, MPSE_ERR_ARG, "grouped product: bad group");
    gg.g[i].C = static_cast<double*>(s.C);
    gg.g[i].nseg = s.nseg;
    gg.g[i].use_beta = s.beta != 0.0 ? 1 : 0;
    if (s.beta != 0.0 && s.beta != 1.0) return mpse_fail(ctx, MPSE_ERR_ARG, "grouped product: beta must be 0 or 1");
    any_beta = any_beta || s.beta != 0.0;
    for (int q = 0; q < s.nseg; ++q) {
      if (!s.seg[q].A || !s.seg[q].B) return mpse_fail(ctx, MPSE_ERR_ARG, "grouped product: null operand");
      gg.g[i].seg[q] = GSeg{static_cast<const double*>(s.seg[q].A), static_cast<const double*>(s.seg[q].B), s.seg[q].am, s.seg[q].bm};
      any_mask = any_mask || s.seg[q].am || s.seg[q].bm;
    }
    max_seg = s.nseg > max_seg ? s.nseg : max_seg;
    segs += s.nseg;
  }
  g.A = gg.g[0].seg[0].A, g.B = gg.g[0].seg[0].B, g.C = gg.g[0].C;
  g.use_beta = any_beta;
  if (d.nmix > 0) {
    // (the sources are read through 32-bit row numbers of C's own row space; the rows of a tile keep their a)
    if (!ca || d.nmix > GMAX_MIX || d.mix_grp < 0 || d.mix_grp >= d.ngrp || d.grp[d.mix_grp].beta != 1.0 || !d.mix_w ||
        d.mix_d < 1 || BM % d.mix_d != 0 || g.M % BM != 0 || d.mix_wr < 1 || d.mix_ld < g.N)
      return mpse_fail(ctx, MPSE_ERR_ARG, "grouped product: bad epilogue mix");
    gg.nmix = d.nmix, gg.mix_grp = d.mix_grp, gg.mix_d = d.mix_d, gg.mix_wr = d.mix_wr, gg.mix_ld = d.mix_ld;
    gg.mix_w = static_cast<const double*>(d.mix_w);
    for (int t = 0; t < d.nmix; ++t) {
      if (!d.mix[t].src || d.mix[t].delta <= -d.mix_d || d.mix[t].delta >= d.mix_d)
        return mpse_fail(ctx, MPSE_ERR_ARG, "grouped product: bad epilogue mix term");
      gg.mix[t] = GMix{static_cast<const double*>(d.mix[t].src), d.mix[t].b, d.mix[t].f, d.mix[t].delta, 0};
    }
  }

  // ---- plan
  const int nkt_max = max_seg * gg.nkt_seg;
  // The result mask is taken by a launch that completes the result of one group WITH the dot request riding - else a
  // reduction of its own would read the tiles left unwritten - and whose rows are whole (a, sigma) runs of the mask's
  // layout.  Which tiles are left out is recorded in the launch order.
  const long long nwg_all = (long long)((g.M + BM - 1) / BM) * g.tiles_n * (d.split2 ? 2 : 1);
  const int om_d = om && om->mask && om->row > 0 && om->row % g.N == 0 ? om->row / g.N : 0;
  const bool om_fits = om_d > 0 && d.ngrp == 1 && dot && nwg_all <= dot->cap && g.M % om_d == 0 &&
                       (g.M / om_d + 15) / 16 <= om->pitch && om->row % 64 == 0;
  const mpse_plan::GroupedPlan p =
      mpse_plan::grouped_plan(g.M, g.N, d.ngrp, nkt_max, any_mask, d.split2, ca, n_cu_of(ctx), om_fits);
  const long long ntile = (long long)p.tiles_m * p.tiles_n;
  if (ntile > 0x7fffffffLL) return mpse_fail(ctx, MPSE_ERR_SHAPE, "grouped product: grid too large");
  g.tiles_m = p.tiles_m;
  g.nkw = p.nkw;
  g.die_group = p.die_group;
  if (dot && d.ngrp == 1 && p.nwg >= 1 && p.nwg <= dot->cap) {
    g.dot_y = static_cast<const double*>(dot->y);
    g.dot_part = dot->part;
    dot->nb_out = (int)p.nwg;
  }
  const bool out_mask = om_fits && p.order && g.dot_y;
  if (out_mask) gg.omask = om->mask, gg.om_pitch = om->pitch, gg.om_d = om_d;
  mpse_ctx::ProfRec rec;
  const int variant = (ca ? 1 : 0) + (cb ? 2 : 0);
  const double mnk = double(g.M) * double(g.N) * double(g.K) * segs;
  const bool prof_this = prof_begin(ctx, variant, mnk * ((ca && cb) ? 8.0 : 4.0),
                                    grouped_bytes(d, double(g.M), double(g.N), double(g.K), ca),
                                    &rec);
  g.kt_counter = prof_this && ctx->prof_ktiles ? ctx->prof_ktiles + variant : nullptr;

  // ---- order (the masks are the segments' own)
  TmpBuf PERM(ctx);
  if (p.order) {
    // (one buffer: the launch order, then the assembled flags of every tile - 8-byte aligned; grouped entries of the
    // cache never collide with plain ones)
    const size_t perm_bytes = (size_t(ntile) * sizeof(int) + 7) & ~size_t(7), flag_pitch = size_t(g.nkw) * 8;
    int* pp = nullptr;
    bool sort = false;
    MPSE_TRY(perm_source(ctx, sc && sc->keeps_env_masks && d.masks_stable ? sc : nullptr,
                         {gg.g[0].seg[0].am, gg.g[0].seg[0].bm, g.tiles_m, g.tiles_n,
                          nkt_max + 1000 * d.ngrp + (out_mask ? 1000000 : 0), nullptr},
                         perm_bytes + size_t(ntile) * flag_pitch, PERM, &pp, &sort));
    if (sort)
      hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long*)nullptr,
                         (const unsigned long long*)nullptr, 0, nkt_max, g.tiles_m, g.tiles_n, d.split2 ? 0 : 1, pp,
                         g.skip, gg, reinterpret_cast<unsigned char*>(pp) + perm_bytes, (int)flag_pitch, g.M, g.N);
    g.perm = pp;
    g.gg.flags = reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(pp) + perm_bytes);
  }

  // ---- launch
  count_paths(ctx->gemm_paths, d);
  ctx->gemm_paths[mpse_ctx::GP_GROUPED_OUTMASK] += out_mask;
  // With the dead tiles gone a compute unit mostly holds ONE working workgroup of a halved launch: eight waves on it,
  // as for launches of one workgroup per unit - with the dot partial of the four-wave form, so that the switch does not
  // change a bit of the solve.
  const bool om_wide = out_mask && d.split2 && ca && !p.wide && g.N % BN == 0;
  gg.dot4 = om_wide ? 1 : 0;
  launch_gemm(ctx, g, p.nwg, ca, cb, true, p.wide || om_wide, true);
  if (prof_this) prof_end(ctx, rec);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

extern "C" int mpse_gemm(mpse_ctx* ctx, const mpse_gemm_desc* d, const void* A, const void* B, void* C) {
  if (ctx && d && MPSE_RECORDING(ctx)) {
    const mpse_gemm_desc dc = *d;
    ctx->defer_ops[ctx->defer_recording].push_back([ctx, dc, A, B, C] { return mpse_gemm(ctx, &dc, A, B, C); });
    return MPSE_OK;
  }
  return gemm_impl(ctx, d, A, B, C, d ? (d->skip_zero_tiles & 3) : 0, nullptr, nullptr);
}

extern "C" int mpse_gemm_path_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  if (!ctx || n < 0 || (n > 0 && !counts)) return MPSE_ERR_ARG;
  for (int i = 0; i < n && i < mpse_ctx::GP_COUNT; ++i) counts[i] = ctx->gemm_paths[i];
  return MPSE_OK;
}

int gemm_call(mpse_ctx* ctx, int dta, int dtb, int conja, int conjb, mpse_index ma, mpse_index ka, mpse_index kb,
              mpse_index nb, mpse_index mc, mpse_index nc, int64_t batch, int64_t sba, int64_t sbb, int64_t sbc,
              const void* A, const void* B, void* C, double alpha, double beta, int skip_zero, SolveScope* sc,
              ProductReq* rq) {
  mpse_gemm_desc d;
  d.dtype_a = dta;
  d.dtype_b = dtb;
  d.conj_a = conja;
  d.conj_b = conjb;
  d.m_a = ma;
  d.k_a = ka;
  d.k_b = kb;
  d.n_b = nb;
  d.m_c = mc;
  d.n_c = nc;
  d.batch = batch;
  d.sb_a = sba;
  d.sb_b = sbb;
  d.sb_c = sbc;
  d.alpha_re = alpha;
  d.alpha_im = 0.0;
  d.beta_re = beta;
  d.beta_im = 0.0;
  d.skip_zero_tiles = skip_zero;
  return gemm_impl(ctx, &d, A, B, C, skip_zero, sc, rq);
}

extern "C" int mpse_transpose_inner(mpse_ctx* ctx, int dtype, void* out, const void* in, int64_t d0, int64_t d1,
                                    int64_t d2, int conj) {
  if (!ctx) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (d0 <= 0 || d1 <= 0 || d2 <= 0) return MPSE_OK;
  if (!out || !in) return MPSE_ERR_ARG;
  long long nblk = d0 * ((d1 + 31) / 32) * ((d2 + 31) / 32);
  if (nblk > 0x7fffffffLL) return mpse_fail(ctx, MPSE_ERR_SHAPE, "transpose grid too large");
  wsite_written(ctx, out, size_t(d0) * size_t(d1) * size_t(d2) * dtype_size(dtype));
  if (dtype == MPSE_C128)
    hipLaunchKernelGGL((k_transpose_inner<true>), dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (double*)out,
                       (const double*)in, (long long)d0, (int)d1, (int)d2, conj);
  else
    hipLaunchKernelGGL((k_transpose_inner<false>), dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (double*)out,
                       (const double*)in, (long long)d0, (int)d1, (int)d2, 0);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}
