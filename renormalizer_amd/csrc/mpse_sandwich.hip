// mpse_mps_sandwich: <bra| O |ket> of two different chains with an MPO between them as ONE engine call (the value a
// Green-Kubo job records after every step; the reference builds an Environ and walks it, mps/mp.py expectation).  Two
// paths, chosen from the dims table alone (sandwich_plan):
//   k_sandwich_chain  one launch, one workgroup walks every site; the transfer tensor E (Db, w, Dk) and one
//                     (sigma, ancilla) slice of T = E . K[:, sigma, a, :] live in LDS, the new E in registers
//   enqueued          the environment-update plan of mpse_env_update (left domain, no unit channel) site after site on
//                     two pooled environments, enqueued back to back from here
// Either way the host reads once, at the end.  No atomics, a fixed summation order: the same inputs give the same bits.
#include "mpse_sandwich_step.h"

namespace {

constexpr int64_t SW_SITE_ELEMS_MAX = 1ll << 30;   // elements of one site tensor: offsets stay inside 32 bits
// Multiply-adds (of the working type) of the heaviest site above which the enqueued products are faster than one
// workgroup although the chain still fits: measured with tools/sandwich_bench.py, profiles/sandwich.md
constexpr int64_t SW_WORK_MAX = 1ll << 62;
constexpr int64_t SW_WORK_CLAMP = INT64_MAX;   // what the work of an absurd table is reported as

struct SwPlan {
  bool chain;         // the chain kernel takes it
  int64_t e_elems;    // LDS elements of E (padded rows), largest over the bonds
  int64_t t_elems;    // LDS elements of one (sigma, a) slice of T, largest over the sites
  int64_t lds;        // bytes of the launch, working dtype (0: not eligible)
  int64_t lds_fit;    // the same when LDS, accumulators and channels allow the launch, whatever the work (else 0)
  int64_t acc;        // accumulators per thread the widest site needs: SW_CHANNELS * ceil(Dbr Dkr / threads)
  int64_t w_max;      // largest MPO bond
  int64_t work;       // multiply-adds of the heaviest site, dense: d danc (Dbl wl Dkl Dkr + d wl Dbl Dbr Dkr)
};

bool sandwich_table_ok(int nsite, const int64_t* dims) { return chain_table_ok(nsite, dims, 8, {0, 1, 2}, {5, 6, 7}); }

// the sizing of a table that is a chain
SwPlan sandwich_plan(int nsite, const int64_t* dims, bool cplx) {
  SwPlan pl{false, 0, 0, 0, 0, 0, 0, 0};
  bool fits = true, bonds_ok = true;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* s = dims + 8 * i;
    const int64_t Dbl = s[0], Dkl = s[1], wl = s[2], d = s[3], danc = s[4], Dbr = s[5], Dkr = s[6], wr = s[7];
    const double work = double(d) * double(danc) *
                        (double(Dbl) * double(wl) * double(Dkl) * double(Dkr) +
                         double(d) * double(wl) * double(Dbl) * double(Dbr) * double(Dkr));
    const int64_t wk = work >= 9.0e18 ? SW_WORK_CLAMP : int64_t(work);
    pl.work = wk > pl.work ? wk : pl.work;
    // what the launch needs depends on the bonds alone; the physical extents only have to keep offsets inside 32 bits
    bool small = true;
    for (int j : {0, 1, 2, 5, 6, 7}) small = small && s[j] <= CHAIN_EXT_MAX;
    if (!small) {
      bonds_ok = false;
      continue;
    }
    const double site_max = double(SW_SITE_ELEMS_MAX);
    if (d > CHAIN_EXT_MAX || danc > CHAIN_EXT_MAX || double(Dbl) * d * danc * Dbr > site_max ||
        double(Dkl) * d * danc * Dkr > site_max || double(wl) * d * d * wr > site_max)
      fits = false;
    const int64_t e_l = Dbl * wl * chain_pitch(Dkl), e_r = Dbr * wr * chain_pitch(Dkr), t = Dbl * wl * Dkr;
    const int64_t acc = SW_CHANNELS * ((Dbr * Dkr + CHAIN_THREADS - 1) / CHAIN_THREADS);
    pl.w_max = wr > pl.w_max ? wr : pl.w_max;
    pl.e_elems = e_l > pl.e_elems ? e_l : pl.e_elems;
    pl.e_elems = e_r > pl.e_elems ? e_r : pl.e_elems;
    pl.t_elems = t > pl.t_elems ? t : pl.t_elems;
    pl.acc = acc > pl.acc ? acc : pl.acc;
  }
  if (!bonds_ok) {
    pl.e_elems = pl.t_elems = pl.acc = 0;
    return pl;
  }
  const int64_t lds = (pl.e_elems + pl.t_elems) * (cplx ? 16 : 8);
  pl.lds_fit = fits && lds <= CHAIN_LDS_MAX && pl.acc <= SW_ACC && pl.w_max <= SW_CHANNELS ? lds : 0;
  pl.chain = pl.lds_fit > 0 && pl.work <= SW_WORK_MAX;
  pl.lds = pl.chain ? lds : 0;
  return pl;
}

// E_0 = 1 (1 x 1 x 1), then the site step of mpse_sandwich_step.h (sw_site_step) site after site.  The result
// E_N[0, 0, 0] goes to out[0..1] and, when pub is set, to the mapped host buffer followed by the sequence number
// (publish_collect).
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_sandwich_chain(const SwSite* __restrict__ sites, int nsite,
                                                                  int conj_bra, int e_elems, double* out, double* pub,
                                                                  volatile double* seq_slot, double seq) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double sw_lds[];
  T* E = reinterpret_cast<T*>(sw_lds);
  T* Ts = E + e_elems;
  const int tid = threadIdx.x;
  if (tid == 0) E[0] = El::one();
  __syncthreads();
  for (int i = 0; i < nsite; ++i) {
    const SwSite s = sites[i];
    sw_site_step<CPLX>(s, conj_bra, E, Ts);
  }
  if (tid == 0) chain_publish2(out, pub, seq_slot, seq, El::re(E[0]), El::im(E[0]));
}

struct SwArgs {
  int nsite;
  const void* const* bra;
  const int* bra_dtype;
  const void* const* ket;
  const int* ket_dtype;
  const void* const* W;
  const int* w_dtype;
  const int64_t* dims;
  int conj_bra;
};

int sandwich_chain(mpse_ctx* ctx, const SwArgs& a, bool cplx, const SwPlan& pl, double* out2) {
  std::vector<SwSite> rows((size_t)a.nsite);
  for (int i = 0; i < a.nsite; ++i) {
    const int64_t* s = a.dims + 8 * i;
    rows[i] = SwSite{a.bra[i], a.ket[i], a.W[i], (int)s[0], (int)s[1], (int)s[2], (int)s[3], (int)s[4], (int)s[5],
                     (int)s[6], (int)s[7], a.bra_dtype[i] == MPSE_C128, a.ket_dtype[i] == MPSE_C128,
                     a.w_dtype[i] == MPSE_C128, 0};
  }
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_sandwich_chain)}, CHAIN_LDS_MAX));
  return chain_scalar_launch(ctx, rows, [&](const SwSite* tab, double* res, const PublishAt& at) {
    CHAIN_LAUNCH(ctx, cplx, k_sandwich_chain, 1, pl.lds, tab, a.nsite, a.conj_bra, (int)pl.e_elems, res, at.pub,
                 at.seq_slot, at.seq);
  }, out2);
}

// mpse_env_update (left domain, env_unit = 0) per site on two pooled environments.  The update works in one dtype per
// site - complex from the first complex operand on - so a real site next to complex operands is widened into a pooled
// copy first (what lib.py contract_one_site does with to_complex).
int sandwich_enqueued(mpse_ctx* ctx, const SwArgs& a, double* out2) {
  int64_t e_max = 2, site_max = 1;
  for (int i = 0; i < a.nsite; ++i) {
    const int64_t* s = a.dims + 8 * i;
    const int64_t e = s[5] * s[7] * s[6], nb = s[0] * s[3] * s[4] * s[5], nk = s[1] * s[3] * s[4] * s[6];
    e_max = e > e_max ? e : e_max;
    site_max = nb > site_max ? nb : site_max;
    site_max = nk > site_max ? nk : site_max;
  }
  TmpBuf e0(ctx), e1(ctx), cb(ctx), ck(ctx);
  MPSE_TRY(e0.alloc((size_t)e_max * 16));
  MPSE_TRY(e1.alloc((size_t)e_max * 16));
  const double one[2] = {1.0, 0.0};
  MPSE_TRY(stage_h2d(ctx, e0.p, one, sizeof(one)));
  void* env = e0.p;
  void* nxt = e1.p;
  int e_dt = MPSE_F64;
  for (int i = 0; i < a.nsite; ++i) {
    const int64_t* s = a.dims + 8 * i;
    const bool cx = e_dt == MPSE_C128 || a.bra_dtype[i] == MPSE_C128 || a.ket_dtype[i] == MPSE_C128 ||
                    a.w_dtype[i] == MPSE_C128;
    const int dt = cx ? MPSE_C128 : MPSE_F64;
    const void* bra = a.bra[i];
    const void* ket = a.ket[i];
    if (cx && a.bra_dtype[i] != MPSE_C128) MPSE_TRY(widen_site(ctx, cb, &bra, s[0] * s[3] * s[4] * s[5], site_max));
    if (cx && a.ket_dtype[i] != MPSE_C128) MPSE_TRY(widen_site(ctx, ck, &ket, s[1] * s[3] * s[4] * s[6], site_max));
    mpse_dims dm{};
    dm.Dl_bra = s[0], dm.Dl_ket = s[1], dm.Dr_bra = s[5], dm.Dr_ket = s[6];
    dm.d0 = s[3], dm.d1 = 1, dm.danc = s[4];
    dm.wl = s[2], dm.wm = 1, dm.wr = s[7];
    dm.env_unit = 0, dm.danc1 = 0;
    const int cj = (a.conj_bra != 0 && a.bra_dtype[i] == MPSE_C128) ? 1 : 0;
    MPSE_TRY(mpse_env_update(ctx, dt, MPSE_DOMAIN_L, &dm, env, e_dt, ket, bra, cj, a.W[i], a.w_dtype[i], nxt));
    void* t = env;
    env = nxt, nxt = t;
    e_dt = dt;
  }
  return chain_scalar_result(ctx, env, e_dt == MPSE_C128, out2);   // E_N is 1 x 1 x 1
}

}  // namespace

extern "C" {

int mpse_mps_sandwich_plan(int nsite, const int64_t* dims, int any_complex, int64_t* info, int n) {
  const bool valid = sandwich_table_ok(nsite, dims);
  const SwPlan pl = valid ? sandwich_plan(nsite, dims, any_complex != 0) : SwPlan{false, 0, 0, 0, 0, 0, 0, 0};
  const int64_t v[12] = {CHAIN_LDS_MAX, pl.lds,      pl.e_elems, pl.t_elems,    CHAIN_THREADS,        SW_ACC,
                         pl.acc,        SW_WORK_MAX, pl.work,    valid ? 1 : 0, any_complex ? 16 : 8, SW_CHANNELS};
  plan_info_out(info, n, v, 12);
  return pl.chain ? 1 : 0;
}

int mpse_mps_sandwich_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::sandwich_stats, counts, n);
}

int mpse_mps_sandwich(mpse_ctx* ctx, int nsite, const void* const* bra, const int* bra_dtype, const void* const* ket,
                      const int* ket_dtype, const void* const* W, const int* w_dtype, const int64_t* dims,
                      int conj_bra, double* out_re_im_host) {
  if (!ctx) return MPSE_ERR_ARG;
  if (nsite < 1 || !bra || !bra_dtype || !ket || !ket_dtype || !W || !w_dtype || !dims || !out_re_im_host)
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_sandwich: null argument or no sites");
  bool cplx = false;
  MPSE_TRY(chain_scan_sites(ctx, "mps_sandwich", nsite, {bra, ket, W}, {bra_dtype, ket_dtype, w_dtype}, &cplx));
  if (!sandwich_table_ok(nsite, dims))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "mps_sandwich: dims is not a chain (extents >= 1, matching neighbours, first and last bonds 1)");
  if (MPSE_RECORDING(ctx))
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_sandwich: synchronous, not available while a deferred list is recorded");
  SwPlan pl = sandwich_plan(nsite, dims, cplx);
  MPSE_BIND(ctx);
  // MPSE_SANDWICH_CHAIN=0 sends every chain through the enqueued updates; =1 sends every chain that fits the launch
  // through the kernel, over the work bound as well (measurements of that bound: tools/sandwich_bench.py)
  const char env = chain_env_switch("MPSE_SANDWICH_CHAIN");
  if (env == '0') pl.chain = false;
  if (env == '1' && pl.lds_fit > 0) pl.chain = true, pl.lds = pl.lds_fit;
  const SwArgs args{nsite, bra, bra_dtype, ket, ket_dtype, W, w_dtype, dims, conj_bra};
  double res[2] = {0.0, 0.0};
  if (pl.chain)
    MPSE_TRY(sandwich_chain(ctx, args, cplx, pl, res));
  else
    MPSE_TRY(sandwich_enqueued(ctx, args, res));
  ctx->sandwich_stats[pl.chain ? mpse_ctx::SW_CHAIN : mpse_ctx::SW_ENQUEUED] += 1;
  ctx->sandwich_stats[mpse_ctx::SW_SITES] += nsite;
  out_re_im_host[0] = res[0];
  out_re_im_host[1] = res[1];
  return MPSE_OK;
}

}  // extern "C"
