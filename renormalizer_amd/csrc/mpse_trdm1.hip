// mpse_mps_trdm1: the one-site transition density matrices
//   T_i[p, p'] = sum_{b,k,g,b',k'} op(B_i)[b,p,g,b'] L_i[b,k] K_i[k,p',g,k'] R_i[b',k']
// of selected sites of TWO chains, a bra B and a ket K, as one engine call (the reference's spectral function takes
// <gs| a_i |ket(t)> for every i with one operator window, one closing product and one host read per i plus a conjugated
// copy of the bra, transport/spectral_function.py:106-117; <bra| O_i |ket> = sum O[p,p'] T_i[p,p']).  L_i / R_i: the
// overlap environments left / right of site i, bra index first: Db rows, Dk columns - rectangular.  op: the complex
// conjugate when conj_bra is set, as in mpse_mps_overlap.  With bra == ket and conj_bra it is rho_i of mpse_mps_rdm1,
// and both are the call of mpse_chain_sites.h: the kernels, the LDS plan and the enqueued passes are written there,
// once.  Two paths, chosen from the dims table alone (trdm1_plan):
//   chain      two launches.  k_trdm1_envs: workgroup 0 walks right to left with R in LDS, workgroup 1 left to right with
//              L in LDS (walk_envs); each leaves its environment of every selected site in pooled memory (R transposed,
//              so that k_trdm1_sites reads it along the lanes).  k_trdm1_sites: one workgroup per selected site closes
//              L_i and R_i around the site (chain_close_site).
//   enqueued   the same contractions as products of the contraction kernel - every other chain
// The launches FIT when the plan is within CHAIN_LDS_MAX, Db * Dk <= CHAIN_ACC_MAX at every bond (one accumulator per
// entry of an environment), d, danc and d * danc <= CHAIN_EXT_MAX and every site tensor has fewer than 2^31 elements
// (the offsets into a site are 32-bit): chain_sel_plan.  Launch order instead of flags, one host read, a fixed
// summation order: as said in mpse_chain_walk.h.
#include "mpse_chain_sites.h"

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

static_assert(mpse_ctx::TR_SITES == 2 && mpse_ctx::TR_MATRICES == 3, "chain_sel_done: chain, enqueued, sites, results");

using TrSite = ChainSiteRow<Chain2Row>;   // 72 bytes
static_assert(sizeof(TrSite) == 72, "descriptor rows are copied as 8-byte words");

// The sizing of a table that is a chain: that of chain_sel_plan for two chains, under the rule of the two limits
ChainSelPlan trdm1_plan(int nsite, const int64_t* dims, int nsel, bool cplx) {
  ChainSelPlan pl = chain_sel_plan(nsite, dims, nsel >= 1, 0, cplx, TR_BOND_MAX, true);
  pl.chain = pl.fit && (pl.max_bond <= TR_BOND_MAX || (pl.max_bra == 1 && pl.max_ket <= TR_BOND_MAX_BRA1));
  return pl;
}

template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_trdm1_envs(const TrSite* __restrict__ sites, int nsite, int first,
                                                              int last, int e_elems, void* pool) {
  walk_envs<CPLX, false>(sites, nsite, first, last, e_elems, pool);
}

template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_trdm1_sites(const TrSite* __restrict__ sites, int nsite, int e_elems,
                                                               const void* __restrict__ pool, double* __restrict__ out) {
  chain_close_site<CPLX>(sites, nsite, e_elems, pool, out);
}

// the two launches of the chain path (chain_sites_launch)
int trdm1_launch(mpse_ctx* ctx, bool cplx, const ChainSelPlan& pl, const ChainSelArgs& a, const TrSite* tab, void* pool,
                 double* res) {
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_trdm1_envs), CHAIN_KERNELS(k_trdm1_sites)}, CHAIN_LDS_MAX));
  CHAIN_LAUNCH(ctx, cplx, k_trdm1_envs, 2, pl.lds, tab, a.nsite, a.sel[0], a.sel[a.nsel - 1], (int)pl.e_elems, pool);
  CHAIN_LAUNCH(ctx, cplx, k_trdm1_sites, a.nsel, pl.lds, tab, a.nsite, (int)pl.e_elems, (const void*)pool, res);
  return MPSE_OK;
}

}  // namespace

extern "C" {

int mpse_mps_trdm1_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n) {
  const bool valid = chain_sel_table_ok(nsite, dims, true);
  const ChainSelPlan pl = valid ? trdm1_plan(nsite, dims, nsel, any_complex != 0) : ChainSelPlan{};
  const int64_t v[14] = {TR_BOND_MAX, CHAIN_LDS_MAX, pl.chain ? pl.lds : 0, pl.e_elems, pl.t_elems, CHAIN_THREADS,
                         pl.max_bra, pl.max_ket, valid ? 1 : 0, 0, CHAIN_EXT_MAX, CHAIN_ACC_MAX, pl.lds, TR_BOND_MAX_BRA1};
  plan_info_out(info, n, v, 14);
  return pl.chain ? 1 : 0;
}

int mpse_mps_trdm1_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::trdm1_stats, counts, n);
}

int mpse_mps_trdm1(mpse_ctx* ctx, int nsite, const void* const* bra, const int* bra_dtype, const void* const* ket,
                   const int* ket_dtype, const int64_t* dims, int conj_bra, int nsel, const int* sel, double* out_host) {
  const ChainSelArgs args{nsite, ket, ket_dtype, dims, nsel, sel, bra, bra_dtype, conj_bra};
  bool cplx = false;
  MPSE_TRY(chain_sel_prologue(ctx, "mps_trdm1", args, 1, out_host != nullptr && bra && bra_dtype, &cplx));
  ChainSelPlan pl = trdm1_plan(nsite, dims, nsel, cplx);
  MPSE_BIND(ctx);
  chain_sel_plan_switch("MPSE_TRDM1_CHAIN", &pl);
  return chain_sites_call<TrSite>(
      ctx, args, cplx, pl.chain, ctx->trdm1_stats,
      [&](const TrSite* tab, void* pool, double* res) { return trdm1_launch(ctx, cplx, pl, args, tab, pool, res); },
      out_host);
}

}  // extern "C"
