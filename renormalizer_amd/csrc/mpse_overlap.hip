// mpse_mps_overlap: <bra|ket> of two different chains as ONE engine call (the reference walks the chain with two
// tensordots per site, mps/mp.py:933-956).  Two paths, chosen from the dims table alone (overlap_plan):
//   k_overlap_chain  one launch, one workgroup walks every site; the transfer matrix E and one sigma slice of
//                    T = E . K[:, sigma, :] live in LDS - chains whose bonds are all <= OV_BOND_MAX
//   enqueued         2 N products through the contraction kernel, enqueued back to back from here with two pooled
//                    temporaries (the products of Mps.dot, without its host round trips) - every other chain
// Either way the host reads once, at the end.  No atomics, a fixed summation order: the same inputs give the same bits.
#include "mpse_chain.h"

namespace {

constexpr int OV_OUT_PER_THREAD = 4;      // entries of the new E a thread accumulates in registers over sigma
constexpr int64_t ov_lds_bytes(int64_t D, int64_t es) { return (D * chain_pitch(D) + D * D) * es; }
constexpr int64_t ov_bond_limit() {
  // the largest power-of-two bond D whose complex E (D x D, padded) and T slice (D x D) fit, and whose E has one entry
  // per accumulator of the workgroup
  int64_t D = 1;
  while (ov_lds_bytes(2 * D, 16) <= CHAIN_LDS_MAX && 4 * D * D <= int64_t(CHAIN_THREADS) * OV_OUT_PER_THREAD) D *= 2;
  return D;
}
constexpr int64_t OV_BOND_MAX = ov_bond_limit();
static_assert(OV_BOND_MAX == 64, "64 x 65 + 64 x 64 complex128 = 129 KB of 160 KB; 128 would need 516 KB");
// p <= CHAIN_EXT_MAX keeps the site offsets inside 32 bits: 64 * 65536 * 64 = 2^28 elements

struct OvSite {   // one row of the descriptor table (48 bytes, uploaded once per call)
  const void* bra;
  const void* ket;
  int Dbl, Dkl, p, Dbr, Dkr;
  int bra_c, ket_c;   // the side's tensor is complex128
  int pad;
};
static_assert(sizeof(OvSite) == 48, "descriptor rows are copied as 8-byte words");

struct OvPlan {
  bool chain;            // the chain kernel takes it
  int64_t max_bond;      // largest bond of either side
  int64_t e_elems;       // LDS elements of E (padded rows), largest over the bonds
  int64_t t_elems;       // LDS elements of one sigma slice of T, largest over the sites
  int64_t lds;           // bytes, working dtype
};

bool overlap_table_ok(int nsite, const int64_t* dims) { return chain_table_ok(nsite, dims, 5, {0, 1}, {3, 4}); }

// the sizing of a table that is a chain
OvPlan overlap_plan(int nsite, const int64_t* dims, bool cplx) {
  OvPlan pl{false, 0, 0, 0, 0};
  bool fits = true;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + 5 * i;
    for (int j : {0, 1, 3, 4}) pl.max_bond = d[j] > pl.max_bond ? d[j] : pl.max_bond;
    if (pl.max_bond > OV_BOND_MAX || d[2] > CHAIN_EXT_MAX) {
      fits = false;
      continue;
    }
    const int64_t e_l = d[0] * chain_pitch(d[1]), e_r = d[3] * chain_pitch(d[4]), t = d[0] * d[4];
    pl.e_elems = e_l > pl.e_elems ? e_l : pl.e_elems;
    pl.e_elems = e_r > pl.e_elems ? e_r : pl.e_elems;
    pl.t_elems = t > pl.t_elems ? t : pl.t_elems;
  }
  if (!fits) return pl;
  pl.lds = (pl.e_elems + pl.t_elems) * (cplx ? 16 : 8);
  pl.chain = pl.lds <= CHAIN_LDS_MAX;
  if (!pl.chain) pl.lds = 0;
  return pl;
}

// E_0 = 1;  per site, per sigma in ascending order:  T[b, k'] = sum_k E[b, k] K[k, sigma, k']  (into LDS), then
// E'[b', k'] += sum_b op(B[b, sigma, b']) T[b, k']  (registers of the thread that owns (b', k')); E' replaces E in LDS
// after the last sigma.  Threads take entries with k' fastest: the reads of K are contiguous, those of T conflict free,
// B[b, sigma, b'] is one address per b' group.  The result E_N[0, 0] goes to out[0..1] and, when pub is set, to the
// mapped host buffer followed by the sequence number (publish_collect).
template <bool CPLX>
__global__ __launch_bounds__(CHAIN_THREADS) void k_overlap_chain(const OvSite* __restrict__ sites, int nsite,
                                                                 int conj_bra, int e_elems, double* out, double* pub,
                                                                 volatile double* seq_slot, double seq) {
  using El = ChainEl<CPLX>;
  using T = typename El::T;
  extern __shared__ __attribute__((aligned(16))) double ov_lds[];
  T* E = reinterpret_cast<T*>(ov_lds);
  T* Ts = E + e_elems;
  const int tid = threadIdx.x;
  if (tid == 0) E[0] = El::one();
  __syncthreads();
  for (int i = 0; i < nsite; ++i) {
    const OvSite s = sites[i];
    const int Dbl = s.Dbl, Dkl = s.Dkl, p = s.p, Dbr = s.Dbr, Dkr = s.Dkr;
    const int pe = Dkl | 1, pe_new = Dkr | 1;
    const int nT = Dbl * Dkr, nE = Dbr * Dkr;
    const int k_row = p * Dkr, b_row = p * Dbr;   // element strides of the left bond in K and B
    const bool cj = conj_bra != 0 && s.bra_c != 0;
    T acc[OV_OUT_PER_THREAD];
#pragma unroll
    for (int j = 0; j < OV_OUT_PER_THREAD; ++j) acc[j] = El::zero();
    for (int sg = 0; sg < p; ++sg) {
      for (int o = tid; o < nT; o += CHAIN_THREADS) {
        const int b = o / Dkr, kk = o - b * Dkr;
        const T* e_row = E + b * pe;
        const int k0 = sg * Dkr + kk;
        T sum = El::zero();
#pragma unroll 8
        for (int k = 0; k < Dkl; ++k) El::fma(sum, e_row[k], El::ld(s.ket, s.ket_c, k * k_row + k0));
        Ts[o] = sum;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < OV_OUT_PER_THREAD; ++j) {
        const int o = tid + j * CHAIN_THREADS;
        if (o < nE) {
          const int bb = o / Dkr, kk = o - bb * Dkr;
          const int b0 = sg * Dbr + bb;
          T sum = acc[j];
#pragma unroll 8
          for (int b = 0; b < Dbl; ++b) {
            T v = El::ld(s.bra, s.bra_c, b * b_row + b0);
            if (cj) v = El::cj(v);
            El::fma(sum, v, Ts[b * Dkr + kk]);
          }
          acc[j] = sum;
        }
      }
      __syncthreads();   // T is overwritten by the next sigma; after the last one every read of E is done as well
    }
#pragma unroll
    for (int j = 0; j < OV_OUT_PER_THREAD; ++j) {
      const int o = tid + j * CHAIN_THREADS;
      if (o < nE) {
        const int bb = o / Dkr, kk = o - bb * Dkr;
        E[bb * pe_new + kk] = acc[j];
      }
    }
    __syncthreads();
  }
  if (tid == 0) chain_publish2(out, pub, seq_slot, seq, El::re(E[0]), El::im(E[0]));
}

int overlap_chain(mpse_ctx* ctx, int nsite, const void* const* bra, const int* bra_dtype, const void* const* ket,
                  const int* ket_dtype, const int64_t* dims, bool cplx, int conj_bra, const OvPlan& pl, double* out2) {
  std::vector<OvSite> rows((size_t)nsite);
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + 5 * i;
    rows[i] = OvSite{bra[i], ket[i], (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4],
                     bra_dtype[i] == MPSE_C128, ket_dtype[i] == MPSE_C128, 0};
  }
  MPSE_TRY(chain_lds_attr(ctx, {CHAIN_KERNELS(k_overlap_chain)}, CHAIN_LDS_MAX));
  return chain_scalar_launch(ctx, rows, [&](const OvSite* tab, double* res, const PublishAt& at) {
    CHAIN_LAUNCH(ctx, cplx, k_overlap_chain, 1, pl.lds, tab, nsite, conj_bra, (int)pl.e_elems, res, at.pub, at.seq_slot,
                 at.seq);
  }, out2);
}

// the two products per site of Mps.dot, enqueued from here: T = E . K as (Db_l, p Dk_r), E' = op(B)^T . T with B as
// (Db_l p, Db_r) and T as (Db_l p, Dk_r).  E and T are complex from the first complex operand on, as in mpse_gemm.
int overlap_enqueued(mpse_ctx* ctx, int nsite, const void* const* bra, const int* bra_dtype, const void* const* ket,
                     const int* ket_dtype, const int64_t* dims, int conj_bra, double* out2) {
  int64_t e_max = 2, t_max = 1;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + 5 * i;
    e_max = d[3] * d[4] > e_max ? d[3] * d[4] : e_max;
    t_max = d[0] * d[2] * d[4] > t_max ? d[0] * d[2] * d[4] : t_max;
  }
  TmpBuf ebuf(ctx), tbuf(ctx);
  MPSE_TRY(ebuf.alloc((size_t)e_max * 16));
  MPSE_TRY(tbuf.alloc((size_t)t_max * 16));
  const double one[2] = {1.0, 0.0};
  MPSE_TRY(stage_h2d(ctx, ebuf.p, one, sizeof(one)));
  int e_dt = MPSE_F64;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + 5 * i;
    const int64_t Dbl = d[0], Dkl = d[1], p = d[2], Dbr = d[3], Dkr = d[4];
    const int t_dt = (e_dt == MPSE_C128 || ket_dtype[i] == MPSE_C128) ? MPSE_C128 : MPSE_F64;
    MPSE_TRY(gemm_call(ctx, e_dt, ket_dtype[i], 0, 0, idx1(Dbl, Dkl), idx1(Dkl, 1), idx1(Dkl, p * Dkr),
                       idx1(p * Dkr, 1), idx1(Dbl, p * Dkr), idx1(p * Dkr, 1), 1, 0, 0, 0, ebuf.p, ket[i], tbuf.p));
    const int cj = (conj_bra != 0 && bra_dtype[i] == MPSE_C128) ? 1 : 0;
    MPSE_TRY(gemm_call(ctx, bra_dtype[i], t_dt, cj, 0, idx1(Dbr, 1), idx1(Dbl * p, Dbr), idx1(Dbl * p, Dkr),
                       idx1(Dkr, 1), idx1(Dbr, Dkr), idx1(Dkr, 1), 1, 0, 0, 0, bra[i], tbuf.p, ebuf.p));
    e_dt = (t_dt == MPSE_C128 || bra_dtype[i] == MPSE_C128) ? MPSE_C128 : MPSE_F64;
  }
  return chain_scalar_result(ctx, ebuf.p, e_dt == MPSE_C128, out2);   // E_N is 1 x 1
}

}  // namespace

extern "C" {

int mpse_mps_overlap_plan(int nsite, const int64_t* dims, int any_complex, int64_t* info, int n) {
  const bool valid = overlap_table_ok(nsite, dims);
  const OvPlan pl = valid ? overlap_plan(nsite, dims, any_complex != 0) : OvPlan{false, 0, 0, 0, 0};
  const int64_t v[8] = {OV_BOND_MAX, CHAIN_LDS_MAX, pl.lds, pl.chain ? pl.e_elems : 0, pl.chain ? pl.t_elems : 0,
                        CHAIN_THREADS, pl.max_bond, valid ? 1 : 0};
  plan_info_out(info, n, v, 8);
  return pl.chain ? 1 : 0;
}

int mpse_mps_overlap_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::overlap_stats, counts, n);
}

int mpse_mps_overlap(mpse_ctx* ctx, int nsite, const void* const* bra, const int* bra_dtype, const void* const* ket,
                     const int* ket_dtype, const int64_t* dims, int conj_bra, double* out_re_im_host) {
  if (!ctx) return MPSE_ERR_ARG;
  if (nsite < 1 || !bra || !bra_dtype || !ket || !ket_dtype || !dims || !out_re_im_host)
    return mpse_fail(ctx, MPSE_ERR_ARG, "mps_overlap: null argument or no sites");
  bool cplx = false;
  MPSE_TRY(chain_scan_sites(ctx, "mps_overlap", nsite, {bra, ket}, {bra_dtype, ket_dtype}, &cplx));
  if (!overlap_table_ok(nsite, dims))
    return mpse_fail(ctx, MPSE_ERR_SHAPE,
                     "mps_overlap: dims is not a chain (extents >= 1, matching neighbours, first and last bond 1)");
  // No refusal while a deferred list is recorded, unlike mpse_mps_sandwich and mpse_mps_corr: the enqueued path goes
  // through gemm_call, which does not record, so the call runs at once on either path
  OvPlan pl = overlap_plan(nsite, dims, cplx);
  MPSE_BIND(ctx);
  // MPSE_OVERLAP_CHAIN=0 sends every chain through the enqueued products (measurements: tools/overlap_bench.py)
  if (chain_env_switch("MPSE_OVERLAP_CHAIN") == '0') pl.chain = false;
  double res[2] = {0.0, 0.0};
  if (pl.chain)
    MPSE_TRY(overlap_chain(ctx, nsite, bra, bra_dtype, ket, ket_dtype, dims, cplx, conj_bra, pl, res));
  else
    MPSE_TRY(overlap_enqueued(ctx, nsite, bra, bra_dtype, ket, ket_dtype, dims, conj_bra, res));
  ctx->overlap_stats[pl.chain ? mpse_ctx::OV_CHAIN : mpse_ctx::OV_ENQUEUED] += 1;
  ctx->overlap_stats[mpse_ctx::OV_SITES] += nsite;
  out_re_im_host[0] = res[0];
  out_re_im_host[1] = res[1];
  return MPSE_OK;
}

}  // extern "C"
