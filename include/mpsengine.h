/*
 * mpsengine.h - C ABI of the MI355X (gfx950) matrix-product-state sweep engine.
 *
 * This is the drop-in boundary for the per-site hot path of Renormalizer's
 * DMRG (optimize_mps) and TDVP (Mps.evolve) loops.  Each entry point names the
 * reference call site(s) it replaces (paths relative to renormalizer/ in
 * shuaigroup/Renormalizer v0.0.11).  The reference reaches all of this
 * arithmetic through `xp.tensordot`, `opt_einsum` and SciPy LAPACK; here it is
 * hand-written HIP (FP64 MFMA contraction kernel, wavefront reductions,
 * Householder / one-sided Jacobi factorizations), device resident.
 *
 * Conventions
 *   - plain C types only; every function returns an int status (MPSE_OK == 0)
 *     and never throws; mpse_last_error(ctx) gives a message for the last failure;
 *   - `void*` tensor arguments are DEVICE pointers obtained from mpse_malloc
 *     unless the name ends in `_host`;
 *   - tensors are dense, C-order (last index fastest), dtype MPSE_F64 (8 B) or
 *     MPSE_C128 (interleaved re,im; 16 B);
 *   - index roles follow the reference: environment (bra bond, mpo bond, ket bond),
 *     mps site (D_l, d[, d_anc], D_r), mpo site (w_l, d_up, d_down, w_r);
 *   - all work is enqueued on the context's HIP stream; only the functions
 *     documented as synchronous (downloads, scalar results) wait for it;
 *   - one context per GPU per process (mirrors mps/backend.py:129-132).
 */
#ifndef MPSENGINE_H
#define MPSENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpse_ctx mpse_ctx;

enum {
  MPSE_OK = 0,
  MPSE_ERR_OOM = 1,      /* device allocation failed (reference: MEMORY_ERRORS, mps/backend.py:89-94) */
  MPSE_ERR_SHAPE = 2,    /* inconsistent extents / "Invalid quantum number" (mps/svd_qn.py:219-220) */
  MPSE_ERR_NOCONV = 3,   /* iterative routine hit its iteration limit */
  MPSE_ERR_HIP = 4,      /* a HIP runtime call failed */
  MPSE_ERR_ARG = 5       /* bad argument (null pointer, unknown dtype, ...) */
};

enum { MPSE_F64 = 0, MPSE_C128 = 1 };
enum { MPSE_DOMAIN_L = 0, MPSE_DOMAIN_R = 1 };

/* ---------------------------------------------------------------- context */

/* Replaces backend selection / device binding, mps/backend.py:29-62 (RENO_GPU). */
int mpse_ctx_create(int device, mpse_ctx** out);
int mpse_ctx_destroy(mpse_ctx* ctx);
/* mps/backend.py:129-132 Backend.sync() */
int mpse_sync(mpse_ctx* ctx);
const char* mpse_last_error(const mpse_ctx* ctx);
const char* mpse_version(void);
/* device name, compute-unit count and the HIP stream handle (as void*) for callers that time with HIP events */
int mpse_device_info(mpse_ctx* ctx, char* name, size_t name_len, int* n_cu, void** stream);

/* ------------------------------------------------------------- profiling */
/* Optional per-launch timing of the contraction kernel with HIP events on the context stream
 * (no reference counterpart; used by bench.py for the roofline figures).  variant indexes the
 * operand types of mpse_gemm: 0 = f64 x f64, 1 = c128 x f64, 2 = f64 x c128, 3 = c128 x c128.
 * Totals cover the TIMED launches since the last reset; algorithmic flops use 2/4/4/8 per MAC.
 * on == 1 times every launch, on == N > 1 every N-th launch (sampling: two HIP events per timed launch
 * cost a few microseconds of stream time each). */
/* variants 4 and 5 of mpse_prof_get: 4 = the HBM-bound Lanczos vector kernels inside mpse_expm_lanczos (algorithmic
 * bytes in total_bytes), 5 = whole mpse_block_qr calls (Householder flops in total_flops).  The sampling counter is
 * shared by all variants.  mpse_prof_get_ktiles: 64 x 64 x 16 multiply-add blocks the timed contraction launches of a
 * variant (0-3) actually multiplied - with structural-zero skipping fewer than the dense count; the MFMA work issued
 * is ktiles x 65536 MACs x {2, 4, 4, 6} real flops (complex x complex uses three real products per complex one). */
int mpse_prof_get_ktiles(mpse_ctx* ctx, int variant, int64_t* ktiles);
/* variant 6 of mpse_prof_get = whole batched mpse_block_svd[_full] calls (one-sided Jacobi): total_bytes / total_flops are
 * the traffic and the arithmetic of sweeps x all column pairs (an upper bound: converged pairs are not rotated);
 * mpse_prof_get_svd_sweeps: Jacobi sweeps summed over the timed calls. */
int mpse_prof_get_svd_sweeps(mpse_ctx* ctx, int64_t* sweeps);
/* variant 7 of mpse_prof_get = the fused bond / two-level-site matvec launches (k_heff0_fused): total_flops are the
 * algorithmic flops of the matvec (dense formula of the contraction, no credit for skipped zero blocks), total_bytes the
 * operands read once plus the result written once. */
int mpse_prof_enable(mpse_ctx* ctx, int on);
int mpse_prof_reset(mpse_ctx* ctx);
int mpse_prof_get(mpse_ctx* ctx, int variant, double* total_ms, double* total_flops, double* total_bytes,
                  int64_t* launches);

/* --------------------------------------------------------- device memory */

/* Pooled device allocator (mps/backend.py:116-127 free_all_blocks/log_memory_usage). */
int mpse_malloc(mpse_ctx* ctx, size_t bytes, void** dptr);
int mpse_free(mpse_ctx* ctx, void* dptr);
int mpse_pool_trim(mpse_ctx* ctx);
int mpse_mem_info(mpse_ctx* ctx, size_t* pool_bytes, size_t* in_use_bytes, size_t* device_free, size_t* device_total);
/* mps/matrix.py:298-322 asnumpy/asxp. h2d/d2h are synchronous with respect to the host buffer. */
int mpse_memcpy_h2d(mpse_ctx* ctx, void* dst, const void* src_host, size_t bytes);
int mpse_memcpy_d2h(mpse_ctx* ctx, void* dst_host, const void* src, size_t bytes);
int mpse_memcpy_d2d(mpse_ctx* ctx, void* dst, const void* src, size_t bytes);
int mpse_memset_zero(mpse_ctx* ctx, void* dst, size_t bytes);
/* strided block copy (height rows of width_bytes; pitches in bytes): the sub-block assignments of
 * MatrixProduct.add (mps/mp.py:386-398) and dstack/vstack of the edge sites. */
int mpse_memcpy_2d(mpse_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
                   size_t height);

/* ------------------------------------------------------ vector primitives */
/* The Lanczos / Davidson vector algebra of lib/krylov/krylov.py:54-82 and
 * lib/davidson/davidson.py.  n counts elements of the given dtype.          */
int mpse_cast_f64_to_c128(mpse_ctx* ctx, void* dst, const void* src, int64_t n);
int mpse_conj_inplace(mpse_ctx* ctx, void* x, int64_t n);                       /* C128 only */
int mpse_scal(mpse_ctx* ctx, int dtype, void* x, int64_t n, double a_re, double a_im);
int mpse_axpy(mpse_ctx* ctx, int dtype, void* y, const void* x, int64_t n, double a_re, double a_im);
/* x_i *= m_i with real weights m (quantum-number mask of mps/gs.py:236-237, 520-523 kept as a dense 0/1 vector) */
int mpse_mul_real(mpse_ctx* ctx, int dtype, void* x, const void* m_f64, int64_t n);
/* Davidson preconditioner out = r / (hdiag - e + shift), zero where mask == 0 (mps/gs.py:530-531; mask may be NULL) */
int mpse_davidson_precond(mpse_ctx* ctx, int dtype, void* out, const void* r, const void* hdiag_f64,
                          const void* mask_f64, int64_t n, double e, double shift);
/* out_i = Re z_i */
int mpse_real_part(mpse_ctx* ctx, void* out_f64, const void* z_c128, int64_t n);
/* out_host[0..1] = sum conj(x_i) y_i  (xp.vdot); synchronous */
int mpse_dotc(mpse_ctx* ctx, int dtype, const void* x, const void* y, int64_t n, double* out_host);
/* out_host[0] = ||x||_2 (xp.linalg.norm); synchronous */
int mpse_nrm2(mpse_ctx* ctx, int dtype, const void* x, int64_t n, double* out_host);

/* out_host[0] = sqrt(mean_i |x_i|^2 / (atol + rtol max(|y1_i|, |y2_i|))^2): the error norm and the initial-step
 * norms of the embedded Runge-Kutta pairs that propagate single sites (ivp_solver = "RK45", mps/mps.py:1299-1315, and
 * the per-site integrations of TDVP-CMF, :1096-1265, where the reference calls scipy.integrate.solve_ivp).  Synchronous. */
int mpse_scaled_rms(mpse_ctx* ctx, int dtype, const void* x, const void* y1, const void* y2, int64_t n, double rtol,
                    double atol, double* out_host);

/* ------------------------------------------- deferred calls
 * A sweep knows what follows a local solve before the solve has converged: the QR of the new centre and the
 * environment update after a site step (mps/mps.py:1316-1378), the absorption of the bond factor into the next site
 * after a bond step (:1379-1395).  The host can only issue them once the solve has returned - and while the host
 * language gets there the GPU idles.  Between mpse_defer_begin and mpse_defer_end the calls mpse_gemm, mpse_block_qr
 * and mpse_env_update on this context are stored (scalar arguments and host index arrays copied, device pointers as
 * given - the buffers must exist) instead of executed; mpse_defer_arm(list) makes the next mpse_expm_lanczos run the
 * stored calls of that list, in order, right after it has enqueued the end of the solve, before it returns.  Two
 * lists (0, 1) so that the calls following the next-but-one solve can be recorded while one list waits.  Device blocks
 * freed while a list is open or waiting are released only after it has run.  Any other entry point called while a
 * list is being recorded executes at once, as usual (it must not depend on results of stored calls).
 * mpse_defer_run executes a list immediately; mpse_defer_discard drops everything (error paths). */
int mpse_defer_begin(mpse_ctx* ctx, int list);
int mpse_defer_end(mpse_ctx* ctx);
int mpse_defer_arm(mpse_ctx* ctx, int list);
int mpse_defer_run(mpse_ctx* ctx, int list);
int mpse_defer_discard(mpse_ctx* ctx);

/* ------------------------------------------- general tensor contraction */

/* A logical matrix index that addresses memory through up to two levels:
 *   offset(i) = (i / lo_ext) * s_hi + (i % lo_ext) * s_lo      (strides in elements)
 * Single-level indices use lo_ext >= ext (s_hi ignored). */
typedef struct {
  int64_t ext;
  int64_t lo_ext;
  int64_t s_hi;
  int64_t s_lo;
} mpse_index;

/* C[b](i,j) = alpha * sum_k opA(A[b](i,k)) * opB(B[b](k,j)) + beta * C[b](i,j)
 * Replaces mps/matrix.py:210-211 tensordot and :283-295 pair_tensor_contract
 * (transpose-copy + ?gemm in the reference) with one FP64-MFMA kernel that reads
 * the operands through their strides.  C is C128 if either operand is.       */
typedef struct {
  int dtype_a, dtype_b;
  int conj_a, conj_b;
  mpse_index m_a, k_a;      /* A(i,k) */
  mpse_index k_b, n_b;      /* B(k,j) */
  mpse_index m_c, n_c;      /* C(i,j) */
  int64_t batch;
  int64_t sb_a, sb_b, sb_c; /* batch strides, elements */
  double alpha_re, alpha_im;
  double beta_re, beta_im;
  int skip_zero_tiles;      /* hint for block-sparse operands: bit 0 scan A, bit 1 scan B for all-zero 64 x 16
                               tiles and skip them in the K loop (same result; pays from ~1e8 multiply-adds);
                               0 = plain dense GEMM */
} mpse_gemm_desc;

int mpse_gemm(mpse_ctx* ctx, const mpse_gemm_desc* desc, const void* A, const void* B, void* C);

/* How the contraction kernel was launched: cumulative counts of this context, counted on the host where the launcher
 * decides (a call that returns early or is refused counts nothing; a deferred call counts when it runs).  counts[i]
 * for i < min(n, 16), in this order:
 *    0  launches of the kernel by mpse_gemm and the contraction plans (grouped launches excepted)
 *    1  of them through the general kernel (a two-level K index, a negative stride or an operand span of 4 GB or more)
 *    2  eight waves per workgroup (one workgroup per compute unit or fewer, at least two K tiles)
 *    3  split-K, batch == 1 (slices of one product run slice-fastest; a reduction launch follows)
 *    4  split-K, batch > 1
 *    5  die grouping 1: the workgroups of one die own whole tile rows
 *    6  die grouping 2: whole tile columns
 *    7  tile columns skewed by the tile row (unsplit, unsorted, not die grouped)
 *    8  tile launch order sorted from the occupancy masks (block-sparse, batch == 1, many tiles)
 *    9  occupancy masks read by the kernel (skip_zero_tiles; the general kernel visits every K tile)
 *   10  of them read from global memory instead of LDS (more than 64 mask words, K > 8192)
 *   11  grouped launches (the folded one-site matvec)
 *   12  of them with every tile halved between two workgroups
 *   13  of them that form their beta term in the epilogue from blocks of the MPO site (epilogue mix)
 *   14  launches of the elementwise MPO pass (k_wmix) by the contraction plans
 *   15  grouped launches that left the result tiles outside the solve's structural mask unwritten (MPSE_OUT_MASK)
 * Diagnostics for tests (which path ran); no device work. */
int mpse_gemm_path_stats(mpse_ctx* ctx, int64_t* counts, int n);

/* out = transpose of `in` viewed as (d0,d1,d2) -> (d0,d2,d1); optional conjugation. */
int mpse_transpose_inner(mpse_ctx* ctx, int dtype, void* out, const void* in,
                         int64_t d0, int64_t d1, int64_t d2, int conj);

/* --------------------------------------------------- hot-path contractions */

/* Extents of a (one- or two-site) centre and its surroundings. */
typedef struct {
  int64_t Dl_bra, Dl_ket;   /* left bond of bra / ket (equal for an effective Hamiltonian used by Lanczos / Davidson;
                               mpse_heff_apply alone accepts bra != ket: H C projected onto another state's bonds) */
  int64_t Dr_bra, Dr_ket;
  int64_t d0, d1;           /* physical dims of the centre site(s); d1 unused for 0/1-site */
  int64_t danc;             /* ancilla dim of an MPDM site, 1 for an MPS */
  int64_t wl, wm, wr;       /* mpo bonds: left, middle (2-site only), right */
  int64_t env_unit;         /* mpse_env_update only: 1-based MPO-bond channel b with env[:, b, :] == identity
                               (see mpse_env_unit_channel); 0 = none / unknown */
  int64_t danc1;            /* ancilla dim of the second site of a two-site MPDM centre; 0 = same as danc */
} mpse_dims;

/* Environment update, replaces mps/lib.py:169-250 contract_one_site
 * (L: abc,adf->bcdf; bcdf,bdeg->cfeg; cfeg,ceh->fgh   R: fda,abc->fdbc; fdbc,gdeb->fcge; fcge,hec->fgh,
 * ancilla variants lib.py:207-211/239-243).
 *   env : (Dl_bra,wl,Dl_ket) for L, (Dr_bra,wr,Dr_ket) for R;  ket : (Dl_ket,d0[,danc],Dr_ket)
 *   bra : same layout with the bra extents, or NULL to use ket; bra_conj!=0 -> conjugate it here
 *         (pass 0 when the buffer already holds the conjugated tensor, like the reference's ms_conj)
 *   W   : (wl,d0,d0,wr), dtype w_dtype
 *   out : (Dr_bra,wr,Dr_ket) for L, (Dl_bra,wl,Dl_ket) for R; dtype `dtype`
 * env_dtype may be MPSE_F64 for the all-ones sentinel (lib.py:25). */
int mpse_env_update(mpse_ctx* ctx, int dtype, int domain, const mpse_dims* dims,
                    const void* env, int env_dtype, const void* ket, const void* bra, int bra_conj,
                    const void* W, int w_dtype, void* out);

/* Environment update through a stack of n_mpo MPO sites, replaces mps/lib.py:121-166 contract_one_site_multi_mpo
 * (used by optimize_mps(omega=...), mps/gs.py:106-112, for the (H - omega)^2 functional: Environ(mps, [mpo, mpo])).
 *   env : (D_bra, w_1, .., w_n, D_ket) - layer 1 touches the bra, layer n the ket;  W[i] : (wl[i], d0, d0, wr[i]), device
 *   out : (D'_bra, w'_1, .., w'_n, D'_ket);  dims->wl / wr / wm / env_unit are ignored.  1 <= n_mpo <= 4. */
int mpse_env_update_multi(mpse_ctx* ctx, int dtype, int domain, const mpse_dims* dims, int n_mpo,
                          const int64_t* wl, const int64_t* wr, const void* env, int env_dtype,
                          const void* ket, const void* bra, int bra_conj, const void* const* W, int w_dtype, void* out);

/* Finds an MPO-bond channel b of a square environment env (D, w, D) with max|env[:, b, :] - 1| <= tol: the
 * channel in which no operator has acted yet is the identity matrix when the sites behind it are canonical
 * (the reference contracts it like any other, mps/lib.py:200-205).  *unit_host = b + 1 for the first such channel, or 0
 * if there is none; a channel that holds a NaN or an infinity, in either part of a complex element, never qualifies,
 * and w > 2048 answers 0 without looking.
 * The result is passed as mpse_dims.env_unit / mpse_heff.l_unit / r_unit so that the big GEMMs skip that channel.
 * Synchronous (one small read-back). */
int mpse_env_unit_channel(mpse_ctx* ctx, int dtype, const void* env, int64_t D, int64_t w, double tol,
                          int64_t* unit_host);

/* Effective Hamiltonian applied to the centre, replaces the closures built by
 * mps/hop_expr.py:57-115 (0-site abc,lbk,ck->al ; 1-site abc,bdef,lfk,cek->adl ;
 * 2-site abc,bdef,fghj,ljk,cehk->adgl ; ancilla variants), order (L.C).W.R.
 *   L (Dl,wl,Dl)  R (Dr,wr,Dr)  W0 (wl,d0,d0,wm|wr)  W1 (wm,d1,d1,wr)  C (Dl_ket,d0[,danc][,d1[,danc1]],Dr_ket), out the same with the bra bonds
 * nsite in {0,1,2}; for nsite==0 wl==wr is the shared mpo bond. */
typedef struct {
  int nsite;
  mpse_dims dims;
  const void* L; int l_dtype;
  const void* R; int r_dtype;
  const void* W0; const void* W1; int w_dtype;
  int64_t l_unit, r_unit;   /* 1-based channel along which L (resp. R) is the identity matrix, 0 = none:
                               that slice of the contraction is a copy instead of a GEMM */
} mpse_heff;

int mpse_heff_apply(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, void* out);

/* Optional: tells the engine the values of a real MPO site W (wl, d, d, wr) that lives at W_dev, from a host copy
 * (row major, the same numbers).  The engine keeps the block structure W[b, :, :, f] (which channel pairs are non-zero,
 * which are the identity) and, for large one-site centres on that site, absorbs the MPO step of mpse_heff_apply /
 * mpse_expm_lanczos / mpse_davidson into the operands of the two large products instead of running it as a step of
 * its own (same result: the reference's single expression mps/hop_expr.py:75-79).  The contents of W_dev must not
 * change while the hint stands: mpse_free(W_dev), a call with W_host == NULL, and every element-level entry point that
 * writes into the described range (mpse_memcpy_h2d / _d2d / _2d, mpse_memset_zero, mpse_scal, mpse_conj_inplace,
 * mpse_axpy, mpse_mul_real, mpse_real_part, mpse_cast_f64_to_c128, mpse_davidson_precond, mpse_gather_cols / _rows,
 * mpse_transpose_inner, the solution vectors of mpse_pcg / _sum / _batch) drop it; a caller that uses W_dev as the
 * OUTPUT of anything else (mpse_gemm, a contraction, a decomposition, another solver) has to drop it itself.
 * mpse_env_update on a described site with d >= 8 runs its MPO step as an elementwise pass over the site's non-zero
 * blocks as well.  No device work. */
int mpse_mpo_site_hint(mpse_ctx* ctx, const void* W_dev, const double* W_host_f64, int64_t wl, int64_t d, int64_t wr);

/* How many effective-Hamiltonian applications of this context ran as the single fused launch of mpse_heff0.hip (inside
 * mpse_expm_lanczos: bond matrices, mps/hop_expr.py:63-67, and one-site centres with a two-level physical index,
 * :75-79) instead of through the contraction plans.  Diagnostics; tests use it to see that the path they mean to check
 * is the one that ran.  Either pointer may be NULL. */
int mpse_heff_fused_stats(mpse_ctx* ctx, int64_t* bond_launches, int64_t* site_launches);

/* Two-layer effective Hamiltonian of the (H - omega)^2 functional, replaces the twolayer=True closures of
 * mps/hop_expr.py:24-52 (1-site abcd,befg,cfhi,jgik,aej->dhk ; 2-site abcd,befg,cfhi,gjkl,ikmn,olnp,aejo->dhmp).
 *   L (Dl, wl, wl, Dl), R (Dr, wr, wr, Dr); W0 / W1 serve both layers; no ancilla; nsite in {1, 2}; the unit-channel
 *   fields are ignored. */
int mpse_heff_apply2(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, void* out);

/* Two MPO layers on a centre with TWO physical legs, each layer on the leg it names: one term of the finite-temperature
 * correction-vector operator (omega - Liou)^2 X = a a X + 2 a X H + X H H, a = omega - H, on a site of an operator in
 * MPS form (replaces the hop closure and the path1 environment chains of cv/finitet.py:215-299, 585-716).
 *   C, out (Dl, d_up, d_down, Dr);  L (Dl, wl1, wl2, Dl), R (Dr, wr1, wr2, Dr): (bond of C, layer 1, layer 2, bond of out)
 *   W1 (wl1, d, d, wr1), W2 (wl2, d, d, wr2), d the extent of the leg the layer acts on; layer 1 acts first
 *   trans == 0: leg'[x] = sum_y W[., x, y, .] leg[y];  trans != 0: leg'[y] = sum_x W[., x, y, .] leg[x]
 * Both layers MPSE_LEG_UP (d_down passes through), both MPSE_LEG_DOWN, or layer 1 up and layer 2 down, side by side
 * (the other order is refused with MPSE_ERR_SHAPE: such layers commute).  One-site centres only.  With d_down == 1,
 * both layers up, transposed, on the same site this is mpse_heff_apply2 step by step. */
enum { MPSE_LEG_UP = 0, MPSE_LEG_DOWN = 1 };
typedef struct {
  int64_t Dl, Dr, d_up, d_down;
  int64_t wl1, wr1, wl2, wr2;
  int leg1, leg2;
  int trans1, trans2;
  const void* L; int l_dtype;
  const void* R; int r_dtype;
  const void* W1; const void* W2; int w_dtype;
} mpse_heff_ft;

int mpse_heff_apply_ft(mpse_ctx* ctx, int dtype, const mpse_heff_ft* h, const void* C, void* out);

/* The environment of such a term moved over one site X (Dl, d_up, d_down, Dr): the bra is conj(X), the ket X, each
 * layer contracts its own leg between them and the leg no layer touches is contracted directly.
 *   MPSE_DOMAIN_L: env (Dl, wl1, wl2, Dl) -> out (Dr, wr1, wr2, Dr);  MPSE_DOMAIN_R: env (Dr, wr1, wr2, Dr) ->
 *   out (Dl, wl1, wl2, Dl); index order as L / R above.  h->L, h->R and their dtypes are not read. */
int mpse_env_update_ft(mpse_ctx* ctx, int dtype, int domain, const mpse_heff_ft* h, const void* env, int env_dtype,
                       const void* X, void* out);

/* Lanczos exponential out = expm(dt*Heff) C, replaces lib/krylov/krylov.py:27-82
 * expm_krylov as called at mps/mps.py:1300-1303, 1343-1346, 1377-1380 (same
 * recurrence without re-orthogonalisation, same stopping rule: successive
 * approximations allclose(rtol,atol) on even j > 3, breakdown at beta < 100 n eps).
 * Synchronous; *nvec receives the Krylov dimension.
 * `out` may be `C` itself (the result then replaces the start vector on every path); an `out` that overlaps `C`
 * without starting at the same address is refused with MPSE_ERR_ARG.  A zero or non-finite C is MPSE_ERR_ARG.  A
 * nonzero C whose |C|^2 is subnormal or at least 1e300 is solved as 2^e C with its largest element in [1, 2) (atol
 * scaled alike) and the result scaled back; inside that range the result for 2^k C is bitwise 2^k times the one for C
 * with atol = 0, as long as no element involved leaves the normal range. */
/* Optional, for the NEXT mpse_expm_lanczos on this context only: the tile-occupancy pattern of the centre tensor as
 * the sweep knows it from the quantum numbers (mps/mp.py:308-352: entry (a, sigma, b) can be non-zero only where the
 * bond and physical quantum numbers add up to the total) - the same for every Krylov vector of the solve, so the
 * engine need not scan each vector for empty tiles before multiplying it by the left environment.  Layout: for the
 * centre tensor viewed as the matrix C[a, (sigma.., b)] (Dl rows, N columns): byte [tn * nkw * 8 + kt] is 1 if any
 * entry with a in [16 kt, 16 kt + 16) and column in [64 tn, 64 tn + 64) may be non-zero, nkw = ceil(ceil(Dl / 16) / 8),
 * tn < ceil(N / 64); nbytes = ceil(N / 64) * nkw * 8.  A mask of another size is ignored.  The mask must mark every
 * tile that holds a non-zero (a superset is fine, a missing tile drops its contribution). */
int mpse_expm_centre_mask(mpse_ctx* ctx, const void* mask_dev, int64_t nbytes);
/* Optional, for the NEXT mpse_expm_lanczos on this context only (a pending key is left alone by
 * mpse_expm_lanczos_batch, like the centre mask): a non-zero key that names this solve among the solves the caller
 * repeats - in a sweep, (site or bond, direction, site-or-bond solve).  The context keeps the launch plan of the fused
 * bond / two-level-site matvec of a keyed solve in a slot of that key; the next solve under the key re-uses it when
 * nothing it was built from differs: shapes and MPO terms are compared on the host, the tile-occupancy flags of the
 * environments and the centre mask on the device by the scan that computes them anyway.  Whatever differs, the plan is
 * rebuilt before the first matvec, so the key never changes a result: every solve is bitwise its keyless self.  Key 0
 * (or no call): no slot.  MPSE_PLAN_REUSE=0 in the environment: keys are ignored.  The key serves the asynchronous solve
 * (the one that runs the fused matvec); a solve that takes or falls back to the synchronous path runs without it. */
int mpse_solve_slot(mpse_ctx* ctx, int64_t key);
/* Byte budget of the slots (default 64 MiB); beyond it the least recently used slots go, at once and whenever a slot
 * grows.  A hook for tests, not part of the integration surface. */
int mpse_plan_store_budget(mpse_ctx* ctx, int64_t bytes);
/* Cumulative counts[i], i < n (zeros beyond 6): 0 keyed solves, 1 of them whose slot matched on the host, 2 host-side
 * mismatches (shape, MPO terms, plan parameters), 3 slots evicted, 4 rebuilds of the fused matvec's plan decided on the
 * device (first builds included), 5 rebuilds of launch orders (none is kept yet: 0).  Reads two device words back:
 * synchronous, diagnostics only. */
int mpse_plan_reuse_stats(mpse_ctx* ctx, int64_t* counts, int n);

int mpse_expm_lanczos(mpse_ctx* ctx, int dtype, const mpse_heff* h, double dt_re, double dt_im,
                      const void* C, void* out, double rtol, double atol, int max_dim, int* nvec);
/* out[i] = expm(dt * Heff_i) C[i] for count independent members: h, C, out, nvec are arrays of count entries (C / out
 * hold device pointers).  Every member's result and Krylov dimension are bitwise what mpse_expm_lanczos gives for it
 * alone.  Members with equal (nsite, dims, dtypes) whose matvec takes the small-centre path and whose centre has more
 * than 256 elements are solved together, up to 64 per launch set; every other member runs through mpse_expm_lanczos,
 * one after another.  A pending mpse_expm_centre_mask is left for the next mpse_expm_lanczos.  On an error the status is
 * that of the first failing member, named in mpse_last_error; the outputs are then unspecified.  Synchronous. */
int mpse_expm_lanczos_batch(mpse_ctx* ctx, int dtype, int count, const mpse_heff* h, double dt_re, double dt_im,
                            const void* const* C, void* const* out, double rtol, double atol, int max_dim, int* nvec);
/* Cumulative counts of members solved by the batched kernels and of members that went through the single solve
 * (grouping, size, need_host, 64-vector limit).  Diagnostics for tests; either pointer may be NULL. */
int mpse_expm_lanczos_batch_stats(mpse_ctx* ctx, int64_t* batched_members, int64_t* single_members);
/* How the Lanczos solves of this context ran: cumulative counts, counted on the host where the solve decides (members
 * solved by the batched kernels of mpse_expm_lanczos_batch count nothing here; the rest of a batch counts as single
 * solves).  counts[i] for i < min(n, 18), in this order:
 *    0  runs of the synchronous solve (centres of 256 elements or fewer, and every hand-over from the asynchronous
 *       solve; a synchronous run that meets an out-of-range |C|^2 and restarts on the rescaled vector, 16, counts twice)
 *    1  asynchronous solves (centres of more than 256 elements) finished on the device
 *    2  hand-overs to the synchronous solve: need_host (|dt| * Gershgorin bound > 512) at the first check the host read
 *    3  the same at a later check read by the host (an estimate of the solve was in `out` already)
 *    4  hand-overs at the 64-vector limit of the asynchronous solve (or at max_dim below it)
 *    5  solves ended by a breakdown (beta < 100 n eps) on the asynchronous path
 *    6  the same on the synchronous path
 *    7  synchronous solves that reached the full space (Krylov dimension == n) without a breakdown
 *    8  solves ended by the convergence test (either path)
 *    9  MPSE_ERR_NOCONV (max_dim reached)
 *   10  merged first checks (the estimates of j = 4 and j = 6 formed in one pass; asynchronous path)
 *   11  host waits of the asynchronous path
 *   12  growths of the Krylov basis (either path)
 *   13  asynchronous update launches that added a matvec result of two or more parts, or read a part mask
 *   14  asynchronous update launches that applied the centre mask (mpse_expm_centre_mask) to the vectors
 *   15  update launches with 8-byte accesses (an odd real length or a start vector off a 16-byte boundary; either path)
 *   16  solves restarted on a start vector scaled by a power of two (|C|^2 out of the normal range)
 *   17  hand-overs with out == C: C put back from its copy in the Krylov basis before the synchronous solve
 * Diagnostics for tests (which path ran); no device work. */
int mpse_expm_lanczos_path_stats(mpse_ctx* ctx, int64_t* counts, int n);

/* Davidson eigensolver for the lowest nroots eigenpairs of the effective Hamiltonian, replaces
 * lib/davidson/davidson.py:154-441 as called at mps/gs.py:533-538 (diagonal preconditioner r / (hdiag - e + shift),
 * Gram-Schmidt twice, restart from the Ritz vectors when max_space vectors are held, convergence of a root when
 * |de| < tol and |r| < sqrt(tol), new directions dropped when their squared norm falls under lindep; tol < 0: the
 * residual alone decides, |r| < -tol - the convergence test of the reference's algo = "primme", gs.py:552-569).
 *   h         : the projected operator (mpse_heff_apply; twolayer != 0: mpse_heff_apply2, the (H - omega)^2 form)
 *   hdiag_f64 : its diagonal (n doubles, device);  mask_f64: 0/1 weights of the symmetry-allowed entries or NULL
 *               (the reference compresses vectors to those entries on the host, mps/gs.py:260, 520-523)
 *   guess     : nguess start vectors of n elements each, contiguous (device);  x_out: nroots vectors (device)
 *   e_host    : nroots eigenvalues;  max_space <= 0 selects 12 + 3 (nroots - 1), max_cycle <= 0 selects 100
 *   1 <= nroots <= 16 and max_space + nroots + 1 <= 80, else MPSE_ERR_ARG (both default spaces fit every nroots)
 * When fewer than nroots eigenpairs exist in the masked space, the missing ones come back as NaN in e_host and zero
 * vectors in x_out.  No start vector left after the mask and the lindep test: MPSE_ERR_ARG.
 * The subspace matrix grows by one batched reduction per new vector; subspace eigenproblems run on the host.
 * Synchronous. */
int mpse_davidson(mpse_ctx* ctx, int dtype, const mpse_heff* h, int twolayer, const void* hdiag_f64,
                  const void* mask_f64, int nroots, int nguess, const void* guess, double tol, int max_cycle,
                  int max_space, double lindep, double shift, double* e_host, void* x_out, int* ncycle, int* nmatvec);

/* Preconditioned conjugate gradients for a Hermitian positive definite projected operator, replaces the
 * scipy.sparse.linalg.cg call of cv/zerot.py:231-290 (host vectors, one Python closure per matvec) for the correction
 * vector ((H - e0 - omega)^2 + eta^2) x = b.  Vectors, scalars and the convergence decision stay on the device; the host
 * enqueues iterations ahead and reads a pinned copy of the control block every fourth iteration.
 *   A v       = mask * (Heff v) + shift * v, Heff applied by mpse_heff_apply2 (twolayer != 0) or mpse_heff_apply
 *   diag_f64  : preconditioner z = r / diag (n doubles, device; the caller has added `shift`; every entry > 0, else
 *               MPSE_ERR_ARG); NULL: plain conjugate gradients
 *   mask_f64  : 0/1 weights of the symmetry-allowed entries or NULL (as mpse_davidson); b is read through the mask
 *               and the start vector is masked in place on entry
 *   x         : start vector on entry, solution on return (device); must not overlap b
 *   tol       : stop when |r| <= tol |b| (scipy's rule with atol = 0, cv/zerot.py:288)
 *   max_iter  : <= 0 selects 10 n (scipy's default).  Not converged within it: MPSE_ERR_NOCONV, x is the last iterate
 *               and the three outputs are filled
 *   iters_host, relres_host (|r| / |b| of the recurrence), lvalue_host (Re(x^H A x) - 2 Re(b^H x) of the returned x,
 *               formed as -Re(b^H x) - Re(r^H x) in the last update pass: the reference spends one more matvec on it,
 *               cv/zerot.py:296, which its hop count, taken before, does not include: that count is the matvec of
 *               the start residual plus the iterations, *iters_host + 1 here); each may be NULL
 * b == 0 under the mask: x = 0, zero iterations, MPSE_OK.  A curvature p^H A p that is not positive (operator not
 * positive definite, or NaN) stops the solve with MPSE_ERR_ARG; x is the iterate before that step.  Once the decision
 * has fallen on the device every launch the host has enqueued past it returns at once, so x is the iterate of the
 * deciding iteration.  MPSE_F64 and MPSE_C128 (conjugated dot products).  Synchronous. */
int mpse_pcg(mpse_ctx* ctx, int dtype, const mpse_heff* h, int twolayer, double shift, const void* diag_f64,
             const void* mask_f64, const void* b, void* x, double tol, int max_iter, int* iters_host,
             double* relres_host, double* lvalue_host);
/* What the mpse_pcg solves of this context did, cumulative: counts[i], i < n, receives
 *    0  solves that reached a decision on the device (a call that fails on an argument check of the host, an
 *       allocation or the runtime is not counted; one refused for its diagonal is counted here and under no ending)
 *    1  iterations (sum of the reported iteration counts)
 *    2  matvecs issued by iterations (the one of the start residual b - A x0 is not counted): iterations plus what the
 *       host had enqueued past the decision
 *    3  host waits (reads of the pinned control block)
 *    4  solves ended by the tolerance (b == 0 included)
 *    5  solves ended by max_iter (MPSE_ERR_NOCONV)
 *    6  solves ended by a non-positive curvature (MPSE_ERR_ARG)
 *    7  two-layer solves
 *    8  masked solves
 *    9  not a count: the number of iterations between two host waits (the compile-time constant of mpse_pcg.hip;
 *       entry 2 exceeds entry 1 by at most this number - 1 per solve that ended by the tolerance or max_iter)
 * Diagnostics for tests; no device work. */
int mpse_pcg_stats(mpse_ctx* ctx, int64_t* counts, int n);

/* count independent systems with the semantics of mpse_pcg, member by member: h, shift_host, b, x and the four outputs
 * are arrays of count entries (b / x hold device pointers; diag_f64 / mask_f64 arrays of device pointers, the array or
 * single entries may be NULL); dtype, twolayer, tol and max_iter serve all members (max_iter <= 0: 10 n of each member).
 * The stopping rule, the b == 0 ending, the curvature and diagonal refusals and lvalue are mpse_pcg's.
 *   status_host[i] : the member's own MPSE_OK / MPSE_ERR_NOCONV / MPSE_ERR_ARG (MPSE_ERR_SHAPE for a member mpse_pcg
 *                    refuses for its shape); a member that does not converge or is refused does not disturb the others
 *   return value   : non-zero only for argument, allocation or runtime errors of the call as a whole
 * Members with twolayer != 0 on a one-site centre whose shape passes the rule of mpse_pcg_batch_plan (bra bonds == ket
 * bonds, no ancilla, L and R of the working dtype, real W) are solved together, members of equal (Dl, d, Dr, wl, wr) in
 * launch sets of up to 32: the matvec is ONE launch for the whole set (mpse_small2.hip; it also forms q = mask * y +
 * shift * p and the partial sums of p^H q), every vector kernel of the iteration carries a member index, each member has
 * its own control block and partials, a member whose decision has fallen does nothing in later launches, and the host
 * reads the pinned mirrors of all control blocks every fourth iteration until every member has decided.  Every other
 * member (one layer, two sites, outside the rule) runs through mpse_pcg unchanged, one after another, and returns bit
 * for bit what mpse_pcg returns.
 * Determinism: a member's x, iters, relres and lvalue are bitwise the same whatever else is in the batch - alone
 * (count == 1), with any neighbours, at any position, on either side of a launch-set boundary; its path depends on its
 * own shape only.  The batched path uses another matvec than mpse_pcg (other summation order), so a batched member
 * agrees with mpse_pcg on the same system to the solver tolerance, not bitwise.  Synchronous. */
int mpse_pcg_batch(mpse_ctx* ctx, int dtype, int count, const mpse_heff* h, int twolayer, const double* shift_host,
                   const void* const* diag_f64, const void* const* mask_f64, const void* const* b, void* const* x,
                   double tol, int max_iter, int* status_host, int* iters_host, double* relres_host,
                   double* lvalue_host);
/* counts[i], i < n, cumulative:
 *    0  members solved by the batched kernels
 *    1  members handed to mpse_pcg
 *    2  launch sets
 *    3  batched matvec launches issued by iterations (one per iteration of a launch set, whatever its size; the one of
 *       the start residuals is not counted; past the last decision the host has enqueued up to 3 more)
 *    4  host waits of the launch sets
 *    5  not a count: the member limit per launch set
 * mpse_pcg_stats does not count the members solved by the batched kernels; members handed to mpse_pcg count there as
 * any other solve.  Diagnostics for tests; no device work. */
int mpse_pcg_batch_stats(mpse_ctx* ctx, int64_t* counts, int n);
/* The eligibility rule of the one-launch two-layer matvec, on the shape alone: returns 1 when a one-site two-layer
 * centre (Dl, d, Dr) with MPO bonds wl, wr of working type dtype takes it, else 0.  Eligible: wl, wr <= info[0],
 * d <= info[1], Dl, Dr <= info[2], and the launch plan (row of the transposed L, sparse W list, the intermediates of a
 * slice of at least one ket-bond state of R) within info[3] bytes of LDS.  info[i], i < n (may be NULL):
 *    0 - 3  the limits: MPO bond channels, physical dimension, bond dimension, LDS bytes per workgroup
 *    4      LDS bytes of the plan (0: not eligible)    5  its slice width    6  its number of slices
 *    7      entries of the sparse W list kept in LDS
 * No context, no device work. */
int mpse_pcg_batch_plan(int dtype, int64_t Dl, int64_t d, int64_t Dr, int64_t wl, int64_t wr, int64_t* info, int n);

/* mpse_pcg over a weighted sum of mpse_heff_ft terms: (mask * sum_t weight[t] * A_t + shift) x = b with 1 <= nterms <= 4,
 * the centre system of the finite-temperature correction vector (weights 1, 2, 1; replaces scipy.sparse.linalg.cg of
 * cv/finitet.py:306-311).  All terms share Dl, Dr, d_up, d_down.  Every term writes a result vector of its own and the
 * launch that forms q = mask * sum_t weight[t] y_t + shift * p reads them all (no pass per term); everything else -
 * control block, host waits, endings, outputs - is mpse_pcg's.  A solve with one term of weight 1 that mpse_heff_apply2
 * can express returns bit for bit what mpse_pcg (twolayer != 0) returns.  Counted in mpse_pcg_stats like any solve
 * (entry 2 counts one matvec per iteration, not per term) and in mpse_pcg_sum_stats. */
int mpse_pcg_sum(mpse_ctx* ctx, int dtype, int nterms, const mpse_heff_ft* terms, const double* weights_host,
                 double shift, const void* diag_f64, const void* mask_f64, const void* b, void* x, double tol,
                 int max_iter, int* iters_host, double* relres_host, double* lvalue_host);
/* counts[i], i < n:  0 summed solves that reached a decision, 1 their iterations, 2 term applications issued by
 * iterations (terms x matvecs), 3 their host waits, 4 preconditioner diagonals started by mpse_diag_ft
 * (calls with accumulate == 0). */
int mpse_pcg_sum_stats(mpse_ctx* ctx, int64_t* counts, int n);

/* diag (Dl, d_up, d_down, Dr) (+)= weight * the diagonal of one mpse_heff_ft term (the pre_M1 / pre_M2 / pre_M4 of
 * cv/finitet.py:233-275), formed on the device:
 *   diag[a, u, v, j] += weight * sum_{b, c, g, i} L[a, b, c, a] S[b, c, u, v, g, i] R[j, g, i, j]
 *   S (wl1, wl2, d_up, d_down, wr1, wr2), real: the per-site factor of the two MPO sites, the same for every centre on
 *   that site (both layers on one leg: sum_y W1[b, x, y, g] W2[c, y, x, i] resp. its transposed-order twin, constant
 *   along the other leg; one layer per leg: W1[b, u, u, g] W2[c, v, v, i]); mpse_site_factor_ft forms it from h->W1 /
 *   h->W2 once per site and frequency.  accumulate == 0 overwrites diag and adds `shift` first. */
int mpse_site_factor_ft(mpse_ctx* ctx, const mpse_heff_ft* h, void* S_f64);
int mpse_diag_ft(mpse_ctx* ctx, const mpse_heff_ft* h, const void* S_f64, double weight, double shift, int accumulate,
                 void* diag_f64);

/* ------------------------------------------------------ overlap of two chains */

/* <bra|ket> of two different matrix product states (or density operators) in one call, replaces the per-site
 * tensordot pair of mps/mp.py:933-956 (MatrixProduct.dot):
 *   E_0 = 1,  E_{i+1}[b', k'] = sum_{b, sigma, k} op(B_i)[b, sigma, b'] E_i[b, k] K_i[k, sigma, k'],  result E_N[0, 0]
 *   bra[i], ket[i]   : device site tensors, contiguous (D_l, p, D_r), each MPSE_F64 or MPSE_C128 (bra_dtype[i] /
 *                      ket_dtype[i]; any mixture); an MpDm site (D_l, d_up, d_down, D_r) passes p = d_up * d_down
 *   dims             : nsite rows (Db_l, Dk_l, p, Db_r, Dk_r), host
 *   conj_bra != 0    : op = complex conjugate (the bra buffers hold the state itself); 0: they hold the conjugate already
 *   out_re_im_host   : two doubles
 * Rows with an extent < 1, neighbours whose bonds differ, or a first / last bond != 1: MPSE_ERR_SHAPE before any
 * device work.  Chains that pass mpse_mps_overlap_plan run as ONE launch (k_overlap_chain: one workgroup walks the
 * sites, E and one sigma slice of T = E . K[:, sigma, :] in LDS, working dtype complex as soon as any site is); every
 * other chain as the 2 nsite products of the reference enqueued back to back through the contraction kernel, with two
 * pooled temporaries.  No atomics, no host read between sites, a fixed summation order: the same inputs give the same
 * bits on every call (the two paths sum in different orders and agree to rounding).  MPSE_OVERLAP_CHAIN=0 in the
 * environment sends every chain through the enqueued products (for measurements).  Synchronous. */
int mpse_mps_overlap(mpse_ctx* ctx, int nsite, const void* const* bra, const int* bra_dtype, const void* const* ket,
                     const int* ket_dtype, const int64_t* dims /* nsite x 5 */, int conj_bra, double* out_re_im_host);
/* counts[i], i < n, cumulative:  0 chains taken by the chain kernel, 1 chains taken by the enqueued path, 2 sites
 * walked (both paths).  A refused call counts nothing.  Diagnostics for tests; no device work. */
int mpse_mps_overlap_stats(mpse_ctx* ctx, int64_t* counts, int n);
/* The path rule, on the dims table alone: returns 1 when the chain kernel takes the chain, else 0 (also for a table
 * mpse_mps_overlap refuses).  Eligible: every bond of either side <= info[0], every p <= 65536, and E (rows padded to
 * an odd length against bank conflicts) plus the largest T slice within info[1] bytes of LDS in the working dtype
 * (complex when any_complex != 0).  info[i], i < n (may be NULL):
 *    0  the bond limit: the largest power of two D with a complex D x D E and T slice inside info[1]
 *    1  LDS bytes a workgroup may use (the 160 KiB of a gfx950 compute unit)
 *    2  LDS bytes of this chain's launch (0: not eligible)    3  its elements of E    4  its elements of T
 *    5  threads of the workgroup    6  the largest bond of the table (0: refused)    7  1 when the table is a chain
 * No context, no device work. */
int mpse_mps_overlap_plan(int nsite, const int64_t* dims, int any_complex, int64_t* info, int n);

/* ------------------------------------------- <bra| O |ket> of two chains and an MPO */

/* <bra| O |ket> of two different matrix product states (or density operators) with a matrix product operator between
 * them in one call, replaces the Environ walk behind mps/mp.py expectation(mpo, self_conj):
 *   E_0 = 1 (1 x 1 x 1),
 *   E_{i+1}[b', g', k'] = sum_{b, g, k, s', s, a} op(B_i[b, s', a, b']) W_i[g, s', s, g'] E_i[b, g, k] K_i[k, s, a, k'],
 *   result E_N[0, 0, 0]
 *   bra[i], ket[i]   : device site tensors, contiguous (D_l, d, danc, D_r); a is the ancilla leg of a density-operator
 *                      site (danc = 1 for an MPS), each MPSE_F64 or MPSE_C128 (any mixture per site and per side)
 *   W[i]             : device MPO site (wl, d, d, wr), MPSE_F64 or MPSE_C128 (w_dtype[i]); its FIRST physical leg meets
 *                      the bra, as in mpse_env_update and Mpo.apply
 *   dims             : nsite rows (Db_l, Dk_l, wl, d, danc, Db_r, Dk_r, wr), host
 *   conj_bra != 0    : op = complex conjugate (the bra buffers hold the state itself); 0: they hold the conjugate already
 *   out_re_im_host   : two doubles
 * Rows with an extent < 1, neighbours whose bonds or MPO bonds differ, or a first / last bond or MPO bond != 1:
 * MPSE_ERR_SHAPE before any device work.  Null pointers and unknown dtypes: MPSE_ERR_ARG.  Chains that pass
 * mpse_mps_sandwich_plan run as ONE launch (k_sandwich_chain: one workgroup walks the sites, E and one (s, a) slice of
 * T = E . K[:, s, a, :] in LDS, the new E in registers, W read through the scalar path with its zero entries skipped,
 * working dtype complex as soon as any tensor is); every other chain as the environment-update plan of
 * mpse_env_update (left domain, env_unit = 0) site after site on two pooled environments.  No atomics, no host read
 * between sites, a fixed summation order: the same inputs give the same bits on every call (the two paths sum in
 * different orders and agree to rounding).  MPSE_SANDWICH_CHAIN=0 in the environment sends every chain through the
 * enqueued updates, =1 every chain whose launch fits through the kernel whatever its work (both for measurements).
 * Synchronous; refused while a deferred list is being recorded. */
int mpse_mps_sandwich(mpse_ctx* ctx, int nsite, const void* const* bra, const int* bra_dtype, const void* const* ket,
                      const int* ket_dtype, const void* const* W, const int* w_dtype, const int64_t* dims /* nsite x 8 */,
                      int conj_bra, double* out_re_im_host);
/* counts[i], i < n, cumulative:  0 chains taken by the chain kernel, 1 chains taken by the enqueued path, 2 sites
 * walked (both paths).  A refused call counts nothing.  Diagnostics for tests; no device work. */
int mpse_mps_sandwich_stats(mpse_ctx* ctx, int64_t* counts, int n);
/* The path rule, on the dims table alone: returns 1 when the chain kernel takes the chain, else 0 (also for a table
 * mpse_mps_sandwich refuses).  Eligible: E (Db x w rows of Dk elements, padded to an odd length against bank
 * conflicts; the largest over the bonds) plus the largest T slice (Db_l wl Dk_r elements) within info[0] bytes of LDS
 * in the working dtype (complex when any_complex != 0); wr * ceil(Db_r Dk_r / info[4]) <= info[5] accumulators per
 * thread at every site; and the dense multiply-add count of the heaviest site,
 * d danc (Db_l wl Dk_l Dk_r + d wl Db_l Db_r Dk_r), at most info[7].  info[i], i < n (may be NULL):
 *    0  LDS bytes a workgroup may use (the 160 KiB of a gfx950 compute unit)
 *    1  LDS bytes of this chain's launch (0: not eligible)    2  its elements of E    3  its elements of T
 *    4  threads of the workgroup    5  accumulators a thread has    6  accumulators the heaviest site needs
 *    7  the work bound (measured, profiles/sandwich.md)    8  multiply-adds of the heaviest site
 *    9  1 when the table is a chain    10  bytes of a working element (8 or 16)
 * No context, no device work. */
int mpse_mps_sandwich_plan(int nsite, const int64_t* dims, int any_complex, int64_t* info, int n);

/* ------------------------------- matrix of two-point functions of one-site operators */

/* C[k, l] = <psi| X_k Y_l |psi> for k < l and C[k, k] = <psi| Z_k |psi> of one-site operators on the selected sites
 * sel[0] < sel[1] < .. of ONE chain, the bra being the conjugate of the state itself, in one call; replaces the
 * n (n + 1) / 2 MPO expectations of mps/mps.py:1657-1687 (calc_edof_rdm):
 *   sites[i]    : device site tensors, contiguous (D_l, d, danc, D_r); a is the ancilla leg of a density-operator site,
 *                 which is traced (danc = 1 for an MPS); each MPSE_F64 or MPSE_C128 (dtype[i]; any mixture)
 *   dims        : nsite rows (D_l, d, danc, D_r), host
 *   sel         : nsel site indices, strictly ascending, host
 *   X, Y, Z     : host; for every selected site in turn a d x d matrix of complex pairs (2 d d doubles): X_k opens,
 *                 Y_k closes, Z_k is the operator of the diagonal entry.  The FIRST index of a matrix meets the bra, as
 *                 W[g, s', s, g'] does in mpse_env_update
 *   out_host    : nsel x nsel complex pairs, row k column l; the lower triangle is left zero
 * Rows with an extent < 1, neighbours whose bonds differ, a first / last bond != 1, or a selection that is not strictly
 * ascending inside [0, nsite): MPSE_ERR_SHAPE before any device work.  Null pointers, an empty selection and unknown
 * dtypes: MPSE_ERR_ARG.  Chains that pass mpse_mps_corr_plan (bonds up to a measured limit) run as TWO launches on the context stream with no host
 * read between them: k_corr_right (one workgroup walks from the right with the identity environment in LDS and leaves
 * the environments closed with Y_l and with Z_l at every selected site l in pooled memory) and k_corr_rows (workgroup k
 * walks from the left, opens with X_k at sel[k] and closes at every later selected site); no flag, spin wait or atomic
 * between workgroups.  Every other chain runs the same two passes as products of the contraction kernel, the open rows
 * as one stack that grows by a row per selected site, all temporaries pooled (MPSE_ERR_OOM when they do not fit; the
 * context stays usable).  The working dtype is complex as soon as any site or local matrix is.  A fixed summation
 * order: the same inputs give the same bits on every call (the two paths sum in different orders and agree to
 * rounding).  MPSE_CORR_CHAIN=0 in the environment sends every chain through the enqueued products, =1 every chain
 * whose launches fit through the kernels, above the measured bond limit as well (both for measurements).  Synchronous;
 * refused while a deferred list is being recorded. */
int mpse_mps_corr(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims /* nsite x 4 */,
                  int nsel, const int* sel, const double* X, const double* Y, const double* Z, double* out_host);
/* counts[i], i < n, cumulative:  0 calls taken by the chain kernels, 1 calls taken by the enqueued path, 2 sites walked
 * (nsite per call), 3 matrix entries produced (nsel (nsel + 1) / 2 per call).  A refused call counts nothing.
 * Diagnostics for tests; no device work. */
int mpse_mps_corr_stats(mpse_ctx* ctx, int64_t* counts, int n);
/* The path rule, on the dims table and the number of selected sites alone: returns 1 when the chain kernels take the
 * call, else 0 (also for a table mpse_mps_corr refuses).  The launches FIT when every bond <= info[10], d * danc <=
 * info[9], 1 <= nsel <= info[8], and the environment plus the largest T slice (rows padded to an odd length against bank
 * conflicts) plus 16 reduction words lie within info[1] bytes of LDS in the working dtype (complex when any_complex !=
 * 0).  The kernels TAKE a call that fits when every bond is also <= info[0], the measured limit up to which they are
 * faster than the enqueued products (profiles/corr_matrix.md).  info[i], i < n (may be NULL):
 *    0  the bond limit of the rule (measured)
 *    1  LDS bytes a workgroup may use (the 160 KiB of a gfx950 compute unit)
 *    2  LDS bytes of either launch (0: not taken)    3  its elements of E (0: does not fit)    4  its elements of T
 *    5  threads of a workgroup    6  the largest bond of the table (0: refused)    7  1 when the table is a chain
 *    8  the grid cap: the largest nsel the chain kernels take    9  the largest d * danc they take
 *   10  the bond limit of the LDS: the largest power of two D with a complex D x D environment and T slice inside info[1]
 *   11  LDS bytes of either launch when it fits, whatever info[0] says (0: does not fit)
 * No context, no device work. */
int mpse_mps_corr_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n);

/* ------------------------------- one-site reduced density matrices of selected sites */

/* rho_i[p, p'] = sum_{a,a',g,b,b'} conj(A[a,p,g,b]) L_i[a,a'] A[a',p',g,b'] R_i[b,b'] for every selected site i of ONE
 * chain in one call, L_i and R_i the identity-operator environments of the sites left and right of i (their first index
 * comes from the conjugated tensor), the ancilla leg g traced; replaces the per-site products and host reads of
 * mps/mps.py:1547-1598 (calc_1site_rdm) and, traced against a one-site operator O (first index on the bra side), <O> =
 * sum_{p,p'} O[p,p'] rho_i[p,p'], the per-operator windows of expectations:
 *   sites[i]    : device site tensors, contiguous (D_l, d, danc, D_r), each MPSE_F64 or MPSE_C128 (dtype[i]; any mixture)
 *   dims        : nsite rows (D_l, d, danc, D_r), host
 *   sel         : nsel site indices, strictly ascending, host
 *   out_host    : the nsel matrices one after the other, each d x d row-major complex pairs: 2 * sum_k d_k^2 doubles
 * Refusals as mpse_mps_corr: rows with an extent < 1, neighbours whose bonds differ, a first / last bond != 1, or a
 * selection that is not strictly ascending inside [0, nsite): MPSE_ERR_SHAPE before any device work.  Null pointers, an
 * empty selection and unknown dtypes: MPSE_ERR_ARG.  A refused call counts nothing, enqueues nothing and leaves out_host
 * as it was.  Chains that pass mpse_mps_rdm1_plan run as TWO launches with no host read between them: k_rdm1_envs (two
 * workgroups; one walks from the right with R in LDS, the other from the left with L in LDS, and each leaves its
 * environment of every selected site in pooled memory) and k_rdm1_sites (one workgroup per selected site closes the two
 * environments around the site; each p of rho[p, p'] is summed by one wave with lane shuffles); no flag, spin wait or
 * atomic between workgroups.  Every other chain runs the same contractions as products of the contraction kernel, all
 * temporaries pooled (MPSE_ERR_OOM when they do not fit; the context stays usable).  The working dtype is complex as
 * soon as any site is; a real chain returns zero imaginary parts.  A fixed summation order: the same inputs give the same
 * bits on every call (the two paths sum in different orders and agree to rounding).  MPSE_RDM1_CHAIN=0 in the
 * environment sends every chain through the enqueued products, =1 every chain whose launches fit through the kernels,
 * above the bond limit of the rule as well (both for measurements).  Synchronous, one host read at the end; refused
 * while a deferred list is being recorded. */
int mpse_mps_rdm1(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims /* nsite x 4 */,
                  int nsel, const int* sel, double* out_host);
/* counts[i], i < n, cumulative:  0 calls taken by the chain kernels, 1 calls taken by the enqueued path, 2 sites walked
 * (nsite per call), 3 matrices produced (nsel per call).  A refused call counts nothing.  Diagnostics for tests; no
 * device work. */
int mpse_mps_rdm1_stats(mpse_ctx* ctx, int64_t* counts, int n);
/* The path rule, on the dims table and the number of selected sites alone: returns 1 when the chain kernels take the
 * call, else 0 (also for a table mpse_mps_rdm1 refuses).  The launches FIT when every bond <= info[10], d, danc and d *
 * danc <= info[9], nsel >= 1, and the environment plus the largest (sigma, ancilla) slice (rows padded to an odd length
 * against bank conflicts) lie within info[1] bytes of LDS in the working dtype (complex when any_complex != 0).  The
 * kernels TAKE a call that fits when every bond is also <= info[0] (profiles/rdm1.md).  info[i], i < n (may be NULL):
 *    0  the bond limit of the rule
 *    1  LDS bytes a workgroup may use (the 160 KiB of a gfx950 compute unit)
 *    2  LDS bytes of either launch (0: not taken)    3  its elements of the environment (0: does not fit)
 *    4  its elements of a slice    5  threads of a workgroup    6  the largest bond of the table (0: refused)
 *    7  1 when the table is a chain    8  the cap on nsel (0: none, one workgroup per selected site)
 *    9  the largest d * danc the kernels take
 *   10  the bond limit of the LDS: the largest power of two D with a complex D x D environment and slice inside info[1]
 *   11  LDS bytes of either launch when it fits, whatever info[0] says (0: does not fit)
 * No context, no device work. */
int mpse_mps_rdm1_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n);

/* ------------------------------- two-site reduced density matrices of all pairs of selected sites */

/* rho_kl[(p,q),(p',q')] = sum conj(A_k)[.,p,g,.] conj(A_l)[.,q,g',.] A_k[.,p',g,.] A_l[.,q',g',.] for every pair k < l of
 * the selected sites of ONE chain in one call: identity environments outside the pair, identity transfer matrices in
 * between, the ancilla legs g, g' traced wherever a site meets its conjugate; replaces the per-pair products and host
 * reads of mps/mps.py:1600-1655 (calc_2site_rdm).  It is the walk of mpse_mps_corr with every elementary matrix |p><p'|
 * opened at k and every |q><q'| closed at l, sharing the walk:
 *   sites[i]    : device site tensors, contiguous (D_l, d, danc, D_r), each MPSE_F64 or MPSE_C128 (dtype[i]; any mixture)
 *   dims        : nsite rows (D_l, d, danc, D_r), host
 *   sel         : nsel >= 2 site indices, strictly ascending, host
 *   out_host    : the pairs of the selection in the order (0,1), (0,2), .., (0,nsel-1), (1,2), .., each one block
 *                 [p][p'][q][q'] of row-major complex pairs: 2 * sum_{k<l} d_k^2 d_l^2 doubles
 * Refusals as mpse_mps_corr / mpse_mps_rdm1, with the same codes: rows with an extent < 1, neighbours whose bonds differ,
 * a first / last bond != 1, or a selection that is not strictly ascending inside [0, nsite): MPSE_ERR_SHAPE before any
 * device work.  Null pointers, nsel < 2 and unknown dtypes: MPSE_ERR_ARG.  A refused call counts nothing, enqueues
 * nothing and leaves out_host as it was.  Chains that pass mpse_mps_rdm2_plan run as TWO launches with no host read
 * between them: k_rdm2_envs (two workgroups; one walks from the right with R in LDS and leaves the d_l^2 closed
 * environments G_l^{qq'} of every selected site but the first in pooled memory, the other walks from the left and leaves
 * L_k of every selected site but the last) and k_rdm2_rows (one workgroup per (k, p, p') starts from L_k at sel[k],
 * carries the opened state to the right and closes against all G_l^{qq'} at every later selected site, one wave per
 * entry (q, q'), summed with lane shuffles); no flag, spin wait or atomic between workgroups.  Every other chain runs
 * the same passes as products of the contraction kernel, the open rows as one stack that grows by d_k^2 rows per opening
 * site and is walked in chunks of whole opening sites (one that alone exceeds the bound: split by rows) whose two stacks
 * plus X1 stay under 256 MiB (info[14] of the plan; MPSE_RDM2_STACK_BYTES in the environment overrides it, read per
 * call); all temporaries pooled (MPSE_ERR_OOM when they do not fit; the context stays usable).  The working dtype is
 * complex as soon as any site is; a real chain returns zero imaginary parts.  A fixed summation order: the same inputs
 * give the same bits on every call (the two paths sum in different orders and agree to rounding).  MPSE_RDM2_CHAIN=0 in
 * the environment sends every chain through the enqueued products, =1 every chain whose launches fit through the
 * kernels, above the bond limit of the rule as well (both for measurements).  Synchronous, one host read at the end;
 * refused while a deferred list is being recorded. */
int mpse_mps_rdm2(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype, const int64_t* dims /* nsite x 4 */,
                  int nsel, const int* sel, double* out_host);
/* counts[i], i < n, cumulative:  0 calls taken by the chain kernels, 1 calls taken by the enqueued path, 2 sites walked
 * (nsite per call), 3 pairs produced (nsel (nsel - 1) / 2 per call).  A refused call counts nothing.  Diagnostics for
 * tests; no device work. */
int mpse_mps_rdm2_stats(mpse_ctx* ctx, int64_t* counts, int n);
/* The path rule, on the dims table and the selection alone (the grid and the size of the result depend on the
 * selection): returns 1 when the chain kernels take the call, else 0 (also for a table or a selection mpse_mps_rdm2
 * refuses).  The launches FIT under the bond, extent and LDS conditions of mpse_mps_rdm1_plan when nsel >= 2 and the
 * pooled environments and the result each stay below 2^31 elements (device offsets are 32-bit).  The kernels TAKE a
 * call that fits when every bond is also <= info[0], a measured limit (profiles/rdm2.md: ahead of the enqueued products
 * up to bond 32 on a chain with d = 2 / 4, behind on a chain with d = 16 at every bond).  info[i], i < n (may be NULL): 0
 * to 11 as for mpse_mps_rdm1_plan, then
 *   12  workgroups of the second launch: sum of d_k^2 over the selected sites but the last
 *   13  complex elements of the result: sum over k < l of d_k^2 d_l^2
 *   14  the byte bound of a chunk of the enqueued path
 * 12 and 13 are 0 for a table or a selection that is refused.  No context, no device work. */
int mpse_mps_rdm2_plan(int nsite, const int64_t* dims, int nsel, const int* sel, int any_complex, int64_t* info, int n);

/* ------------------------------- one-site transition density matrices of selected sites of two chains */

/* T_i[p, p'] = sum_{b,k,g,b',k'} op(B_i)[b,p,g,b'] L_i[b,k] K_i[k,p',g,k'] R_i[b',k'] for every selected site i of TWO
 * chains, a bra B and a ket K, in one call: L_i and R_i the overlap environments of the sites left and right of i (bra
 * index first: Db rows, Dk columns), the ancilla leg g traced, op the complex conjugate when conj_bra != 0, exactly the
 * convention of mpse_mps_overlap.  sum_p T_i[p, p] = <bra|ket> for every i; with bra == ket and conj_bra = 1, T_i is
 * rho_i of mpse_mps_rdm1 with the same index order; traced against a one-site operator O (first index on the bra side),
 * <bra| O_i |ket> = sum_{p,p'} O[p,p'] T_i[p,p'], which replaces the per-operator windows, closing products and host
 * reads of expectations(opers, bra) (transport/spectral_function.py:106-117: G_i(t) = <gs| a_i |ket(t)> / 1j):
 *   bra[i], ket[i] : device site tensors, contiguous (Db_l, d, danc, Db_r) resp. (Dk_l, d, danc, Dk_r), each MPSE_F64
 *                    or MPSE_C128 (bra_dtype[i], ket_dtype[i]; any mixture, across the two chains as well)
 *   dims           : nsite rows (Db_l, Dk_l, d, danc, Db_r, Dk_r), host
 *   sel            : nsel site indices, strictly ascending, host
 *   out_host       : the nsel matrices one after the other, each d x d row-major complex pairs: 2 * sum_k d_k^2 doubles
 * Refusals as mpse_mps_rdm1, with the same codes and in the same order: null pointers, an empty selection, a null site
 * and unknown dtypes: MPSE_ERR_ARG; a selection that is not strictly ascending inside [0, nsite), rows with an extent <
 * 1, neighbours whose bonds differ or a first / last bond != 1 in the bond columns of either chain: MPSE_ERR_SHAPE
 * before any device work.  A refused call counts nothing, enqueues nothing and leaves out_host as it was.  Chains that
 * pass mpse_mps_trdm1_plan run as TWO launches with no host read between them: k_trdm1_envs (two workgroups; one walks
 * from the right with R in LDS, the other from the left with L in LDS, and each leaves its environment of every
 * selected site in pooled memory) and k_trdm1_sites (one workgroup per selected site closes the two environments around
 * the site; each p of T[p, p'] is summed by one wave with lane shuffles); no flag, spin wait or atomic between
 * workgroups.  Every other chain runs the same contractions as products of the contraction kernel, all temporaries
 * pooled (MPSE_ERR_OOM when they do not fit; the context stays usable).  The working dtype is complex as soon as any
 * tensor of either chain is; two real chains return zero imaginary parts.  A fixed summation order: the same inputs
 * give the same bits on every call (the two paths sum in different orders and agree to rounding).  MPSE_TRDM1_CHAIN=0 in
 * the environment sends every chain through the enqueued products, =1 every chain whose launches fit through the
 * kernels, above the bond limits of the rule as well (both for measurements).  Synchronous, one host read at the end;
 * refused while a deferred list is being recorded. */
int mpse_mps_trdm1(mpse_ctx* ctx, int nsite, const void* const* bra, const int* bra_dtype, const void* const* ket,
                   const int* ket_dtype, const int64_t* dims /* nsite x 6 */, int conj_bra, int nsel, const int* sel,
                   double* out_host);
/* counts[i], i < n, cumulative:  0 calls taken by the chain kernels, 1 calls taken by the enqueued path, 2 sites walked
 * (nsite per call), 3 matrices produced (nsel per call).  A refused call counts nothing.  Diagnostics for tests; no
 * device work. */
int mpse_mps_trdm1_stats(mpse_ctx* ctx, int64_t* counts, int n);
/* The path rule, on the dims table and the number of selected sites alone: returns 1 when the chain kernels take the
 * call, else 0 (also for a table mpse_mps_trdm1 refuses).  LDS plan of either launch, in working elements of 8 (real)
 * or 16 bytes (complex when any_complex != 0), rows padded to an odd length (x | 1) against bank conflicts:
 *   region E  the largest of Db * (Dk | 1) over the bonds and Db_l * Db_r over the sites (the environment of the walks;
 *             the intermediate of the closing, which contracts the ket first and is Db_l x Db_r whatever the bonds)
 *   region T  the largest of Db_l * (Dk_r | 1) and Dk_l * (Db_r | 1) over the sites (one (sigma, ancilla) slice of the
 *             walk from the left resp. from the right)
 * The launches FIT when (E + T) elements lie within info[1] bytes, Db * Dk <= info[11] at every bond (one accumulator
 * per entry of an environment), d, danc and d * danc <= info[10], every site tensor of either chain has fewer than 2^31
 * elements (32-bit offsets) and nsel >= 1: there is no cap on a single bond, a bra of bond 1 against a ket of bond 256
 * fits and so does the reverse.  The kernels TAKE a call that fits when the largest bond of either chain is <= info[0],
 * or when every bond of the bra is 1 and the largest bond of the ket is <= info[13] (profiles/trdm1.md).  info[i], i <
 * n (may be NULL):
 *    0  the bond limit of the rule
 *    1  LDS bytes a workgroup may use (the 160 KiB of a gfx950 compute unit)
 *    2  LDS bytes of either launch (0: not taken)    3  its elements of region E (0: does not fit)
 *    4  its elements of region T    5  threads of a workgroup
 *    6  the largest bond of the bra (0: refused)    7  the largest bond of the ket (0: refused)
 *    8  1 when the table is a chain    9  the cap on nsel (0: none, one workgroup per selected site)
 *   10  the largest d * danc the kernels take   11  the largest Db * Dk of a bond they take
 *   12  LDS bytes of either launch when it fits, whatever the rule says (0: does not fit)
 *   13  the bond limit of the rule for the ket of a call whose bra has bond 1 throughout
 * No context, no device work. */
int mpse_mps_trdm1_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n);

/* ------------------------------- Schmidt weights of selected bonds */

/* The Schmidt weights p = sigma^2 of selected bonds of ONE chain in one call, without a canonical form, a quantum-number
 * table or a copy of the state (replaces, for the weights and the entropies, the two sweeps of
 * mps/mps.py:1759-1773 calc_bond_singular_values).  Bond k lies between the sites k and k + 1, 0 <= k <= nsite - 2, and
 * has the dimension D_k = dims[k][3].  With L_k (D_k x D_k) the identity-operator environment of the sites 0 .. k and
 * R_k that of the sites k + 1 .. nsite - 1 (first index from the conjugated tensor, as in mpse_mps_rdm1), the non-zero
 * weights are the eigenvalues of L^(1/2) R^T L^(1/2): with L = U Lambda U^H, of the Hermitian matrix
 *   M = Lambda^(1/2) U^H R^T U Lambda^(1/2).
 * No inverse appears: a rank-deficient bond is no special case.
 *   sites, dtype, dims : as for mpse_mps_rdm1 (the ancilla leg of density-operator sites is traced with the bonds)
 *   sel                : nsel bond indices, strictly ascending inside [0, nsite - 1), host
 *   out_host           : packed, for every selected bond D_k doubles: its weights in descending order, negative
 *                        rounding noise clamped to 0; not normalised (they sum to <psi|psi>): sum_k D_k doubles
 * The weights are exact to about eps * (the largest weight), not relatively: singular values below sqrt(eps) of the
 * largest are not resolved.  Refusals as mpse_mps_rdm1, with the same codes and in the same order; a chain of one site
 * has no bond and is refused like an empty selection (MPSE_ERR_ARG).  A refused call counts nothing, enqueues nothing
 * and leaves out_host as it was.  Chains that pass mpse_mps_bond_spectra_plan run as TWO launches with no host read
 * between them: k_bondspec_envs (two workgroups, the walks of k_rdm1_envs; the one from the left leaves L_k of every
 * selected bond in pooled memory, the one from the right R_k) and k_bondspec_eig (one workgroup per selected bond: a
 * cyclic two-sided Jacobi for Hermitian matrices in LDS, round-robin ordering, first on L with the vectors, then on M
 * for the values; the stopping decision is taken on the device, a solve that reaches its sweep cap fails the call with
 * MPSE_ERR_NOCONV and a message, no weight is returned); no flag, spin wait or atomic between workgroups.  Every other
 * chain runs the two passes as products of the contraction kernel and the two solves of a bond through mpse_block_svd
 * (a Hermitian positive semidefinite matrix has its eigenvalues as singular values), with a host read per solve; no
 * speed is claimed for it.  A fixed summation order: the same inputs give the same bits on every call.
 * MPSE_BOND_SPECTRA_CHAIN=0 / =1 as MPSE_RDM1_CHAIN.  Synchronous; refused while a deferred list is being recorded. */
int mpse_mps_bond_spectra(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype,
                          const int64_t* dims /* nsite x 4 */, int nsel, const int* sel, double* out_host);
/* counts[i], i < n, cumulative:  0 calls taken by the chain kernels, 1 calls taken by the enqueued path, 2 sites walked
 * (nsite per call), 3 bonds returned (nsel per call), 4 the largest number of Jacobi sweeps any solve of k_bondspec_eig
 * has taken on this context (the sweep that finds nothing to rotate included).  A refused call counts nothing.
 * Diagnostics for tests; no device work. */
int mpse_mps_bond_spectra_stats(mpse_ctx* ctx, int64_t* counts, int n);
/* The path rule, on the dims table and the number of selected bonds alone: returns 1 when the chain kernels take the
 * call, else 0 (also for a table mpse_mps_bond_spectra refuses, a chain of one site and nsel < 1).  The launches FIT
 * under the conditions of mpse_mps_rdm1_plan; the kernels TAKE a call that fits when every bond is also <= info[0]
 * (profiles/bond_spectra.md).  info[i], i < n (may be NULL): 0 to 11 as for mpse_mps_rdm1_plan, with 2 and 11 the larger
 * of the two launches, then
 *   12  LDS elements of k_bondspec_eig: 2 D (D | 1) + D, the matrix, the vectors and a strip for Lambda and the
 *       rotations, at the largest bond D of the table (the selection is no argument here; 0: does not fit)
 *   13  the sweep cap of a solve
 * No context, no device work. */
int mpse_mps_bond_spectra_plan(int nsite, const int64_t* dims, int nsel, int any_complex, int64_t* info, int n);

/* ------------------------------- expectation values of a list of MPOs against one chain */

/* out[m] = <psi| O_m |psi>, m < nop, for MPOs O_m against ONE chain (the bra is the conjugate of the ket) in one call
 * with one host read; replaces the loop of mps/mp.py expectations.  O_m is the identity outside its window
 * [first[m], last[m]] and is given by the MPO sites of the window alone.
 *   sites, dtype, dims  : as mpse_mps_rdm1 (rows D_l, d, danc, D_r; the ancilla leg of density-operator sites is traced)
 *   first, last         : nop windows, 0 <= first[m] <= last[m] < nsite; windows may repeat and overlap
 *   W, w_dtype          : the device MPO sites (wl, d, d, wr) of the windows, one window after the other (sum of the
 *                         window lengths entries); the first physical leg meets the conjugated tensor
 *   wdims               : (wl, wr) per MPO site; per window a chain of bonds that starts and ends at 1
 *   out_host            : 2 nop doubles, (re, im) per operator
 * An operator that is the identity everywhere is passed as a window of one site holding the identity and returns
 * <psi|psi>.  Null pointers, nop < 1 and unknown dtypes: MPSE_ERR_ARG; a window outside the chain or with first > last,
 * MPO bonds that do not match, a table that is no chain: MPSE_ERR_SHAPE; all before any device work, out_host as it
 * was.  Calls that pass mpse_mps_expect_many_plan run as TWO kernels with no host read between them: k_expect_envs (two
 * workgroups, the walks of k_bondspec_envs; they leave the identity environments L and R of every distinct window edge
 * in pooled memory; the edges of the chain are the 1 x 1 sentinel) and k_expect_windows (one workgroup per operator: L
 * into LDS as the transfer tensor (D, 1, D), the site step of k_sandwich_chain over the window, the closing against R
 * as a block sum in a fixed order; launched again within the call when there are more operators than info[8]).  Every
 * other call runs the same environments as enqueued products, each window as the environment updates that
 * mpse_mps_sandwich enqueues and every closing as a product into one device result.  Working dtype complex as soon as
 * any tensor is; an all-real call returns exact zero imaginary parts.  No atomics, no flags, a fixed summation order:
 * the same inputs give the same bits on every call (the two paths sum in different orders and agree to rounding).
 * MPSE_EXPECT_CHAIN=0 / =1 as MPSE_CORR_CHAIN.  Synchronous; refused while a deferred list is being recorded. */
int mpse_mps_expect_many(mpse_ctx* ctx, int nsite, const void* const* sites, const int* dtype,
                         const int64_t* dims /* nsite x 4 */, int nop, const int* first, const int* last,
                         const void* const* W, const int* w_dtype, const int64_t* wdims /* MPO sites x 2 */,
                         double* out_host);
/* counts[i], i < n, cumulative:  0 calls taken by the chain kernels, 1 calls taken by the enqueued path, 2 sites walked
 * (nsite per call), 3 values returned (nop per call).  A refused call counts nothing.  Diagnostics for tests; no device
 * work. */
int mpse_mps_expect_many_stats(mpse_ctx* ctx, int64_t* counts, int n);
/* The path rule, on the dims tables alone: returns 1 when the chain kernels take the call, else 0 (also for tables
 * mpse_mps_expect_many refuses).  The launches FIT when the walks fit (mpse_mps_rdm1_plan), every MPO bond is
 * <= info[15], the widest window site needs at most info[17] accumulators per thread, info[15] * ceil(D_r D_r /
 * info[5]), and E (D w rows of D | 1 elements, the largest over the window bonds) plus the largest slice of T (D_l wl
 * D_r) plus a word per wave are within info[1] bytes in the working dtype; the kernels TAKE a call that fits when every
 * bond of the state is also <= info[0] (profiles/expect_many.md).  info[i], i < n (may be NULL): 0 to 11 as for
 * mpse_mps_rdm1_plan (7: table AND windows are valid; 8: the workgroups of one k_expect_windows launch; 2 and 11 the
 * larger of the two launches), then
 *   12  LDS elements of E in k_expect_windows    13  of its slice of T    14  the largest MPO bond
 *   15  MPO channels a thread holds    16  accumulators the widest window site needs    17  accumulators a thread has
 *   18  bytes of a working element (8 or 16)
 * No context, no device work. */
int mpse_mps_expect_many_plan(int nsite, const int64_t* dims, int nop, const int* first, const int* last,
                              const int64_t* wdims, int any_complex, int64_t* info, int n);

/* Which renormalised basis states to keep, replaces select_basis of mps/lib.py:253-322 (the index selection; the
 * column copies are mpse_gather_cols / mpse_gather_rows): an equal quota int(m_max * percent / nblocks) per
 * quantum-number block (ascending block id, descending weight inside a block), the remaining slots by descending
 * weight; stable on ties.  block_id_host[i] = rank of state i's quantum number among the distinct ones (may be NULL
 * when percent == 0).  picked_host receives min(count, m_max) indices.  Host-side integer logic, no device work. */
int mpse_truncate_select(const double* sigma_host, const int64_t* block_id_host, int64_t count, int64_t m_max,
                         double percent, int64_t* picked_host, int64_t* npicked);

/* ------------------------------------------------ block decompositions */

/* Quantum-number blocked QR (system 'L') / RQ (system 'R') of the centre matrix
 * coef (nrow x ncol), replaces mps/svd_qn.py:99-227 with QR=True, full_matrices=False
 * (scipy.linalg.qr / rq per block + blockrecover).  The integer bookkeeping stays
 * with the caller: block b owns rows row_idx_host[row_off_host[b]..row_off_host[b+1])
 * and columns col_idx_host[col_off_host[b]..col_off_host[b+1]); it contributes
 * min(rows,cols) columns.  Outputs (device, zero outside the blocks):
 *   U  (nrow x K)  and  Vt (K x ncol),  K = sum_b min(m_b,n_b),  coef == U @ Vt on the blocks;
 *   system 'L': U has orthonormal columns;  system 'R': Vt has orthonormal rows.
 * system_is_R: bit 0 = system 'R'; bit 1 = this decomposition by the Householder kernels whatever the context's scheme
 * (mpse_block_qr_scheme) says - for a caller that knows the blocks to be rank deficient (a sweep that has seen this site
 * break the Cholesky-QR path before). */
int mpse_block_qr(mpse_ctx* ctx, int dtype, const void* coef, int64_t nrow, int64_t ncol,
                  int nblocks, const int64_t* row_idx_host, const int64_t* row_off_host,
                  const int64_t* col_idx_host, const int64_t* col_off_host,
                  int system_is_R, void* U, void* Vt, int64_t K);

/* How many mpse_block_qr decompositions this context has run, how many of them went through the Cholesky-QR kernels
 * (tall blocks of up to 256 columns: three Gram / Cholesky / triangular-solve passes on MFMA, all compute units) and how
 * many of those were redone by the Householder kernels because a block was rank deficient or too ill conditioned for
 * the scheme (device-side flag).  No reference counterpart (diagnostics; bench.py reports the rates).  Any pointer may
 * be NULL. */
int mpse_block_qr_stats(mpse_ctx* ctx, int64_t* calls, int64_t* chol_calls, int64_t* chol_fallbacks);

/* Optimistic mode of the Cholesky-QR path, for callers that can repeat a whole step (the TDVP-PS sweep, whose input
 * state stays untouched until the step returns): while it is on, mpse_block_qr does not read the breakdown flag back
 * after each decomposition - the read-back stalls the host exactly where it should be enqueueing the next local solve -
 * a breakdown raises a sticky device word instead and the results of that decomposition are NOT an isometry.
 * mpse_block_qr_check (synchronous) says whether any decomposition since the mode was switched on broke down: the caller
 * then discards the step and repeats it with the mode off (every decomposition verified, Householder where needed).
 * Switching the mode on OR off clears the word - ask before switching off - and while the mode is off
 * mpse_block_qr_check reports 0 without touching the device.  No reference counterpart. */
int mpse_block_qr_optimistic(mpse_ctx* ctx, int on);
int mpse_block_qr_check(mpse_ctx* ctx, int* tripped);

/* Pass counts of the Cholesky-QR path since the context was created (synchronous read of two device counters): quantum-
 * number blocks factorised by those kernels, and how many of them ended after TWO passes - the kernels decide per block,
 * on the device, whether the Gram matrix of the second pass is close enough to the identity for its factor to leave an
 * isometry to rounding (n max|G - I| <= 0.1); the third pass of such a block is skipped.  No reference counterpart
 * (diagnostics; bench.py reports the rate).  Either pointer may be NULL. */
int mpse_block_qr_pass_stats(mpse_ctx* ctx, int64_t* blocks, int64_t* two_pass);

/* Which decisions the Cholesky-QR path of mpse_block_qr took on this context, cumulative.  Per call: the whole call is
 * factorised by the right-looking Cholesky kernel when its widest block has at most 160 columns, by the left-looking one
 * otherwise.  Per block, on the device: pass 2 is the last pass when n max|G - I| <= 0.1 (as above); the factor of pass 2
 * or 3 is the first-order one, R = I + striu(E) + diag(E) / 2 with E = G - I, when n max|G - I| <= 1e-9 (the triangular
 * solve is then a product).  counts[i], i < n, receives (zeros beyond the last entry)
 *    0  decompositions tried by the Cholesky-QR kernels (chol_calls of mpse_block_qr_stats)
 *    1  of those, factorised by the right-looking kernel
 *    2  of those, factorised by the left-looking kernel
 *    3  of those, redone by the Householder kernels (chol_fallbacks of mpse_block_qr_stats)
 *    4  blocks factorised (blocks of mpse_block_qr_pass_stats; the blocks of a decomposition that was redone count)
 *    5  blocks that ended after two passes (two_pass of mpse_block_qr_pass_stats)
 *    6  two-pass blocks whose pass-2 factor was the first-order one
 *    7  three-pass blocks whose pass-3 factor was the first-order one
 * Entries 0 - 3 are host counters, 4 - 7 device words summed by the scatter kernel of each decomposition and read here
 * (synchronous).  Diagnostics for tests (tests/test_block_qr_chol_gpu.py); no reference counterpart. */
int mpse_block_qr_path_stats(mpse_ctx* ctx, int64_t* counts, int n);

/* Which kernels mpse_block_qr uses on this context: 0 Householder only (the column-by-column elimination of LAPACK's
 * geqrf, mps/svd_qn.py:171-185 calls scipy.linalg.qr: the SAME isometry as the reference up to rounding, also in the
 * directions of numerically zero singular values, where a QR factorisation is not unique), 1 Cholesky-QR for tall blocks
 * from 256 rows on (default), 2 Cholesky-QR for every block shape it supports, -1 back to the MPSE_CHOLQR environment
 * setting.  Both schemes return U @ Vt == coef and an isometry to rounding; they may differ by a rotation inside the
 * numerical null space of a block.  No reference counterpart. */
int mpse_block_qr_scheme(mpse_ctx* ctx, int scheme);

/* Quantum-number blocked economic SVD by one-sided Jacobi, replaces mps/svd_qn.py:99-240
 * with QR=False, full_matrices=False (scipy.linalg.svd gesdd per block).  Same block
 * description; outputs U (nrow x K), Vt (K x ncol) (block order, NOT globally sorted) and
 * the singular values S_host[K] (descending inside each block).  Synchronous. */
int mpse_block_svd(mpse_ctx* ctx, int dtype, const void* coef, int64_t nrow, int64_t ncol,
                   int nblocks, const int64_t* row_idx_host, const int64_t* row_off_host,
                   const int64_t* col_idx_host, const int64_t* col_off_host,
                   void* U, void* Vt, double* S_host, int64_t K);

/* full_matrices=True variant (mps/svd_qn.py:65-86, 187-213 as called by MatrixProduct._update_mps, mps/mp.py:693-695):
 * after the K singular triplets, block b contributes extra_host[b] null-space vectors of its taller side (zero
 * singular value; 0 <= extra <= |m_b - n_b|): extra columns of U (nrow x KU) for m_b >= n_b, extra rows of
 * Vt (KV x ncol) otherwise, appended after column/row K in block order.  extra_host == NULL means none. */
int mpse_block_svd_full(mpse_ctx* ctx, int dtype, const void* coef, int64_t nrow, int64_t ncol,
                        int nblocks, const int64_t* row_idx_host, const int64_t* row_off_host,
                        const int64_t* col_idx_host, const int64_t* col_off_host, const int64_t* extra_host,
                        void* U, int64_t KU, void* Vt, int64_t KV, double* S_host, int64_t K);

/* Which block step ran the Jacobi sweeps of the mpse_block_svd / mpse_block_svd_full calls of this context, cumulative:
 * the column kernel (pairs of 8-column blocks in LDS) takes a call whose widest block fits the dynamic LDS the runtime
 * grants it - 512 bytes per complex column, 256 per real one: 300 / 600 columns at 150 KB - the Gram-matrix kernel every
 * other call and, with MPSE_SVD_GRAM=2 in the environment, every call.  counts[i], i < n, receives (zeros beyond the
 * last entry)
 *    0  decompositions that reached the sweeps (a call refused for its arguments or shapes counts nothing)
 *    1  of those, sweeps run by the column kernel
 *    2  of those, sweeps run by the Gram kernel
 *    3  sweeps
 *    4  launches of the two sweep kernels
 *    5  not a count: the row slabs per pair of column blocks (gram_R) of the most recent Gram decomposition, 0: none yet
 *    6  not a count: bytes of dynamic LDS the column kernel may use in this process (150 KB, or 64 KB where the runtime
 *       refused the attribute); 0 before the first decomposition of the context
 * Diagnostics for tests; no device work.  No reference counterpart. */
int mpse_block_svd_stats(mpse_ctx* ctx, int64_t* counts, int n);

/* out[:, j] = in[:, cols_host[j]] * scale_host[j]  (column gather of a row-major matrix,
 * replaces the per-column copies of mps/lib.py:303-316 select_basis; scale_host may be NULL). */
int mpse_gather_cols(mpse_ctx* ctx, int dtype, void* out, const void* in, int64_t nrow, int64_t ncol_in,
                     const int64_t* cols_host, const double* scale_host, int64_t ncol_out);
/* out[i, :] = in[rows_host[i], :] * scale_host[i] */
int mpse_gather_rows(mpse_ctx* ctx, int dtype, void* out, const void* in, int64_t ncol,
                     const int64_t* rows_host, const double* scale_host, int64_t nrow_out);

/* ------------------------------------------- tangent-space (TDA) excited states */

/* The Hamiltonian projected onto the first-order tangent space of a matrix product state, replaces the closures hop and
 * hdiag of mps/tda.py:152-247 (TDA.kernel).  With B_j the right-canonical sites of the normalised state, A_j the
 * left-canonical sites of the left-to-right SVD sweep (tda.py:98-121), U_j (Dl, d, n_j) the trailing columns of the full
 * left factor of site j (absent where n_j = 0) and T_j = U_j X_j, one application is
 *   L_0 = 1, L_{j+1} = updL(L_j; A_j, W_j, A_j);  R_N = 1, R_j = updR(R_{j+1}; B_j, W_j, B_j)        (once per handle)
 *   F_0 = 0, F_{j+1} = updL(F_j; A_j, W_j, B_j) + updL(L_j; A_j, W_j, T_j)                           j = 0 .. N-2
 *   G_N = 0, G_j     = updR(G_{j+1}; B_j, W_j, A_j) + updR(R_{j+1}; B_j, W_j, T_j)                   j = N-1 .. 1
 *   O_j = heff(L_j, W_j, R_{j+1}) T_j + heff(F_j, W_j, R_{j+1}) B_j + heff(L_j, W_j, G_{j+1}) A_j
 *   Y_j[l, r] = sum_{a, s} conj(U_j[a, s, l]) O_j[a, s, r]
 * (upd(E; bra, W, ket) = mpse_env_update with the bra conjugated, heff = the one-site mpse_heff_apply): 4 (N - 1)
 * environment updates and 3 N effective-Hamiltonian applications at most, where the reference rebuilds an environment
 * chain per site that carries coefficients (about N^2 updates).  Terms that vanish (F_0, G_N, T_j of a site without U_j)
 * are not issued.  The vector x is the concatenation, over the sites that have a U_j, of X_j (n_j, Dr_j), row major
 * (the reference's reshape_x); its element type is the handle's working dtype: MPSE_C128 as soon as any operand is
 * complex, MPSE_F64 otherwise.
 *
 * mpse_tda_create: the handle borrows the caller's device pointers - they must stay valid and unchanged while it lives -
 *   A[i], B[i] (Dl, d, Dr), U[i] (Dl, d, n) or NULL, W[i] (wl, d, d, wr), each MPSE_F64 or MPSE_C128 (u_dtype[i] of an
 *   absent U[i] is not read), dims: nsite rows (Dl, d, Dr, wl, wr, n), host; n == 0 <=> U[i] == NULL.
 *   Rows with an extent < 1 (n < 0), neighbours whose bonds or MPO bonds differ, a first / last bond or MPO bond != 1, or
 *   n > Dl d: MPSE_ERR_SHAPE before any device work; null sites or dtypes out of range: MPSE_ERR_ARG.  It owns L_j, R_j
 *   (one enqueued update each; their unit channels are looked up once with mpse_env_unit_channel), widened copies of
 *   real sites of a complex handle, the offsets of x and the work buffers F, G, T, O.  *xsize_out = sum_j n_j Dr_j,
 *   *dtype_out = the working dtype (either may be NULL).  An empty tangent space (xsize == 0) is MPSE_ERR_SHAPE.
 * mpse_tda_apply: y = P^H H P x, enqueued on the context stream, no host synchronisation; x is not modified and must
 *   not overlap y.
 * mpse_tda_hdiag: out_f64[xsize] = Re diag(P^H H P) (tda.py:154-170, "abc,ded,bghe,agl,chl->ld"), per site
 *   X[b,c,(g,l)] = sum_a L[a,b,c] conj(U[a,(g,l)]) as a product, Q[(b,g,h),l] = sum_c X[b,c,g,l] U[c,h,l] by the
 *   column-wise dot kernel k_tda_qdiag, then the products with W and with the strided diagonal of R; the columns l are
 *   walked in chunks that keep X under 256 MiB (MPSE_TDA_X_BYTES in the environment overrides the bound, read per call).
 * mpse_tda_davidson: mpse_davidson with the handle as the operator, on vectors of xsize elements of the working dtype
 *   (`dtype` must be it): same iteration, arguments, limits and results; no mask.  Synchronous.
 * mpse_tda_stats: counts[i], i < n, cumulative:  0 handles created, 1 applications, 2 environment updates and 3
 *   effective-Hamiltonian applications issued by applications, 4 sites through k_tda_qdiag, 5 Davidson calls.
 *   Diagnostics for tests; no device work. */
typedef struct mpse_tda mpse_tda;
int mpse_tda_create(mpse_ctx* ctx, int nsite, const void* const* A, const int* a_dtype, const void* const* B,
                    const int* b_dtype, const void* const* U, const int* u_dtype, const void* const* W,
                    const int* w_dtype, const int64_t* dims /* nsite x 6 */, mpse_tda** out, int64_t* xsize_out,
                    int* dtype_out);
int mpse_tda_destroy(mpse_ctx* ctx, mpse_tda* h);
int mpse_tda_apply(mpse_ctx* ctx, mpse_tda* h, const void* x, void* y);
int mpse_tda_hdiag(mpse_ctx* ctx, mpse_tda* h, void* out_f64);
int mpse_tda_davidson(mpse_ctx* ctx, int dtype, mpse_tda* h, const void* hdiag_f64, int nroots, int nguess,
                      const void* guess, double tol, int max_cycle, int max_space, double lindep, double shift,
                      double* e_host, void* x_out, int* ncycle, int* nmatvec);
int mpse_tda_stats(mpse_ctx* ctx, int64_t* counts, int n);

#ifdef __cplusplus
}
#endif
#endif /* MPSENGINE_H */
