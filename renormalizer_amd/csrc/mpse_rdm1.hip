// mpse_mps_rdm1: the one-site reduced density matrices
//   rho_i[p, p'] = sum_{a,a',g,b,b'} conj(A[a,p,g,b]) L_i[a,a'] A[a',p',g,b'] R_i[b,b']
// of selected sites of ONE chain as one engine call (the reference closes every site with three products and a host
// read of its own, mps/mps.py:1547-1598 calc_1site_rdm; local expectation values <O> = sum O[p,p'] rho_i[p,p'] take one
// operator window and one host read each).  L_i / R_i: the identity-operator environments left / right of site i, first
// index from the conjugated tensor.  It is the call of mpse_chain_sites.h with the chain as its own conjugated bra:
// the kernels, the LDS plan and the enqueued passes are written there, once, for this file and for mpse_trdm1.hip.  Two
// paths, chosen from the dims table alone (rdm1_plan):
//   chain      two launches, for chains whose bonds are at most RD_BOND_MAX.  k_rdm1_envs: workgroup 0 walks right to
//              left with R in LDS, workgroup 1 left to right with L in LDS (walk_envs); each leaves its environment of
//              every selected site in pooled memory (R transposed, so that k_rdm1_sites reads it along the lanes).
//              k_rdm1_sites: one workgroup per selected site closes L_i and R_i around the site (chain_close_site).
//   enqueued   the same contractions as products of the contraction kernel - every other chain
// Launch order instead of flags, one host read, a fixed summation order: as said in mpse_chain_walk.h.
#include "mpse_chain_sites.h"

namespace {

// Largest bond up to which the two launches are faster than the enqueued products: measured with tools/rdm1_bench.py,
// profiles/rdm1.md (ahead at 8 and 16 on both models; at 32 ahead with 4 phonon levels, behind with 16; each walk being
// one workgroup on one compute unit, far behind at 64).  Chains between this and CHAIN_BOND_FIT take the kernels only
// under MPSE_RDM1_CHAIN=1.
constexpr int64_t RD_BOND_MAX = 16;
static_assert(1 <= RD_BOND_MAX && RD_BOND_MAX <= CHAIN_BOND_FIT, "the measured limit lies inside what fits");
// The grid of k_rdm1_sites is one workgroup per selected site, whatever their number: no cap on nsel.

using RdSite = ChainSiteRow<ChainSelRow>;   // 48 bytes
static_assert(sizeof(RdSite) == 48, "descriptor rows are copied as 8-byte words");

// the sizing of a table that is a chain
ChainSelPlan rdm1_plan(int nsite, const int64_t* dims, int nsel, bool cplx) {
  return chain_sel_plan(nsite, dims, nsel >= 1, 0, cplx, RD_BOND_MAX);
}

template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_rdm1_envs(const RdSite* __restrict__ sites, int nsite, int first,
                                                             int last, int e_elems, void* pool) {
  walk_envs<CPLX, false>(sites, nsite, first, last, e_elems, pool);
}

template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_rdm1_sites(const RdSite* __restrict__ sites, int nsite, int e_elems,
                                                              const void* __restrict__ pool, double* __restrict__ out) {
  chain_close_site<CPLX>(sites, nsite, e_elems, pool, out);
}

// the two launches of the chain path (chain_sites_launch)
int rdm1_launch(mpse_ctx* ctx, bool cplx, const ChainSelPlan& pl, const ChainSelArgs& a, const RdSite* tab, void* pool,
                double* res) {
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_rdm1_envs), CHAIN_KERNELS(k_rdm1_sites)}, CHAIN_LDS_MAX));
  CHAIN_LAUNCH(ctx, cplx, k_rdm1_envs, 2, pl.lds, tab, a.nsite, a.sel[0], a.sel[a.nsel - 1], (int)pl.e_elems, pool);
  CHAIN_LAUNCH(ctx, cplx, k_rdm1_sites, a.nsel, pl.lds, tab, a.nsite, (int)pl.e_elems, (const void*)pool, res);
  return MPSE_OK;
}

}  // namespace

extern "C" {

int mpse_mps_rdm1_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n) {
  const bool valid = chain_sel_table_ok(nsite, dims);
  const ChainSelPlan pl = valid ? rdm1_plan(nsite, dims, nsel, any_complex != 0) : ChainSelPlan{};
  return chain_sel_plan_out(pl, valid, RD_BOND_MAX, 0, {}, info, n);
}

int mpse_mps_rdm1_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::rdm1_stats, counts, n);
}

int mpse_mps_rdm1(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims, int nsel,
                  const int* sel, double* out_host) {
  const ChainSelArgs args{nsite, sites, dtype, dims, nsel, sel};
  bool cplx = false;
  MPSE_TRY(chain_sel_prologue(ctx, "mps_rdm1", args, 1, out_host != nullptr, &cplx));
  ChainSelPlan pl = rdm1_plan(nsite, dims, nsel, cplx);
  MPSE_BIND(ctx);
  chain_sel_plan_switch("MPSE_RDM1_CHAIN", &pl);
  return chain_sites_call<RdSite>(
      ctx, args, cplx, pl.chain, ctx->rdm1_stats,
      [&](const RdSite* tab, void* pool, double* res) { return rdm1_launch(ctx, cplx, pl, args, tab, pool, res); },
      out_host);
}

}  // extern "C"
