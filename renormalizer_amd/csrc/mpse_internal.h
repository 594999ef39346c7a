// Internal declarations shared by the translation units of libmpsengine.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mpsengine.h"
#include "mpse_plan_store.h"

struct mpse_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int n_cu = 0;
  char err[512] = {0};
  char dev_name[128] = {0};

  // size-bucketed caching allocator: hipMalloc/hipFree synchronise the device, the
  // sweep allocates per site.  Single in-order stream => a freed block may be handed
  // out again immediately.
  std::mutex pool_mu;                       // mpse_malloc / mpse_free may be called from a GC pass on another thread
  std::multimap<size_t, void*> free_blocks;
  std::unordered_map<void*, size_t> live;   // ptr -> bucket size
  size_t pool_bytes = 0;
  size_t in_use_bytes = 0;
  unsigned long long n_device_allocs = 0;   // hipMalloc calls (pool misses)

  // optional HIP-event profiling of the contraction kernel (mpse_prof_*)
  struct ProfRec {
    hipEvent_t e0, e1;
    int variant;
    double flops, bytes;
  };
  bool prof_on = false;
  int prof_stride = 1;      // time every prof_stride-th contraction launch (sampling keeps the overhead small)
  long long prof_counter = 0;
  std::vector<ProfRec> prof_pending;
  std::vector<hipEvent_t> prof_free_events;
  static constexpr int PROF_NVAR = 8;     // 0-3: contraction kernel by operand types, 4: Lanczos vector kernels, 5: block QR, 6: block SVD,
                                          // 7: fused bond / two-level-site matvec (k_heff0_fused)
  int64_t prof_svd_sweeps = 0;            // Jacobi sweeps of the timed mpse_block_svd calls (largest block of each call)
  double prof_ms[PROF_NVAR] = {0};
  double prof_flops[PROF_NVAR] = {0};
  double prof_bytes[PROF_NVAR] = {0};
  int64_t prof_launches[PROF_NVAR] = {0};
  // K tiles (64 x 64 x 16 multiply-add blocks) actually multiplied by the timed contraction launches, per variant:
  // structural-zero skipping makes this smaller than the dense count (device counters, one atomic per workgroup)
  unsigned long long* prof_ktiles = nullptr;

  // pinned ring for small host->device uploads that must not stall the stream (index lists, descriptors)
  char* stage = nullptr;
  char* stage_dev = nullptr;   // the ring as the device sees it (mapped), null: copies go through the runtime
  size_t stage_size = 0, stage_pos = 0;

  // Small pinned staging buffer for scalar read-backs, and its map (offsets in doubles).  The slots overlap; that is
  // harmless because a reader copies its values out before the next enqueue on that context.
  enum PinnedSlot {
    PIN_SCALAR2 = 0,       // [0, 2): read_scalar2 (dot products, norms)
    PIN_FLAG = 8,          // [8, 9): Lanczos closeness flag; block SVD: done words of nblk blocks, (nblk + 1) / 2 doubles
    PIN_LZ_SCAL = 16,      // [16, 540): recurrence scalars of the synchronous Lanczos solve, up to 4 + 4 * 130 doubles
    PIN_ENV_UNIT = 32,        // [32, 32 + w): deviation from the unit per MPO channel of an environment, w <= 2048
    PIN_DAVIDSON = 64,     // [64, 64 + count): subspace products and norms of the Davidson solver, count <= 1024
    // [3700, 3956): control blocks of a launch set, up to 64 x LzCtl (the asynchronous Lanczos solve, single or batched)
    // or 32 x PcgCtl (mpse_pcg, mpse_pcg_sum: one block; mpse_pcg_batch), never both at once
    PIN_BATCH_CTL = 3700,
    PIN_QR_STATUS = 3990,  // [3990, 3991): breakdown word of the Cholesky-QR
    PIN_SLOTS_END = 4000,  // slots of publish_and_wait end here
    PIN_DOUBLES = 4096,
    PIN_SEQ = PIN_DOUBLES - 1   // the last double: sequence word of the published read-backs
  };
  double* pinned = nullptr;     // PIN_DOUBLES doubles
  double* pinned_dev = nullptr; // the same buffer as the device sees it (mapped, host coherent)
  unsigned long long publish_seq = 0;
  double* dscratch = nullptr;   // device scratch for reductions (1<<16 doubles); the last 8 hold flag words
  unsigned int flag_gen = 0;    // generation stamp of the Lanczos convergence flag (no per-check memset)
  // Krylov dimension of the last solve per problem class (number of sites, vector length): how far to run ahead
  std::unordered_map<unsigned long long, int> lz_hint;
  // Block structure of MPO sites the caller has described (mpse_mpo_site_hint), by device pointer: large one-site
  // matvecs on such a site take the folded plan (mpse_plans.h).  Dropped when the buffer is freed, and when one of
  // these entry points write into it (wsite_written): mpse_memcpy_h2d, mpse_memcpy_d2d, mpse_memcpy_2d,
  // mpse_memset_zero, mpse_scal, mpse_conj_inplace, mpse_axpy, mpse_mul_real, mpse_real_part, mpse_cast_f64_to_c128,
  // mpse_davidson_precond, mpse_gather_cols, mpse_gather_rows, mpse_transpose_inner, and the solution vectors of
  // mpse_pcg, mpse_pcg_sum and mpse_pcg_batch.  No other writer looks at the map: results of mpse_gemm and the
  // contractions, the factors of the decompositions and the outputs of the other solvers must not target a described
  // buffer.
  struct WSiteEntry {
    std::shared_ptr<void> info;      // -> mpse_plan::WSiteInfo
    size_t bytes = 0;                // extent of the described site on the device
  };
  std::unordered_map<const void*, WSiteEntry> wsite_info;
  // Deferred calls (mpse_defer_*): mpse_gemm / mpse_block_qr / mpse_env_update issued while a list is being recorded
  // are stored with copies of their arguments; an armed list runs at the end of the next mpse_expm_lanczos, right
  // after the solve has been enqueued to its end.  While a list is recorded or waiting, freed device blocks are held
  // back (a recorded call may still read them).
  std::vector<std::function<int()>> defer_ops[2];
  int defer_recording = -1;
  int defer_armed = -1;
  bool defer_hold = false;                  // guarded by pool_mu
  std::vector<void*> defer_frees;           // guarded by pool_mu
  // Tile-occupancy mask of the centre tensor as operand B of the first products of a matvec, supplied by the caller
  // (mpse_expm_centre_mask: the structural pattern of the quantum numbers, the same for every Krylov vector).  It waits
  // here for the next mpse_expm_lanczos, which takes it out on entry and hands it down as an argument to the scope of
  // its solve (SolveScope::cmask); nothing else reads it.
  struct CMask {
    const void* ptr = nullptr;
    long long bytes = 0;
  } cmask_pending;
  // Plan store: device data of a local solve that the NEXT solve under the same caller's key (mpse_solve_slot) finds
  // unchanged when the tile structure of its operands is unchanged - the plan of the fused matvec (mpse_heff0.hip: tile
  // flags, term table, part mask, launch records).  A slot owns one device buffer, [0, 16) of it the word `changed`
  // that the scan kernels raise and the planner clears; the host remembers what it compares itself (mpse_plan_store.h).
  // Slots go least recently used first under plan_store.budget bytes, and with the context.  slot_pending waits for the
  // next mpse_expm_lanczos like cmask_pending.  MPSE_PLAN_REUSE=0: keys are ignored.
  struct PlanSlotData {
    void* buf = nullptr;
    bool have_f0 = false;
    mpse_store::F0Sig sig;
    std::vector<char> terms;       // term table | term counts as uploaded
  };
  using PlanSlot = mpse_store::Table<PlanSlotData>::Slot;
  mpse_store::Table<PlanSlotData> plan_store;
  long long slot_pending = 0;
  // two device words, bumped by the planners when they do run: [0] k_f0_plan / k_f0_valid of keyed solves (diagnostics,
  // mpse_plan_reuse_stats; context-wide, so that the sum outlives evicted slots); allocated by plan_words()
  int* plan_words_dev = nullptr;
  enum PlanStat { PR_KEYED, PR_HITS, PR_MISMATCH, PR_EVICT, PR_COUNT };
  long long plan_stats[PR_COUNT] = {0};
  // Debug: per-workgroup timeline of the contraction kernel (MPSE_GEMM_TRACE=<file>): every workgroup appends one
  // record (grid, K tiles multiplied, s_memtime stamps of its phases); mpse_prof_get writes the file.
  unsigned long long* gemm_trace = nullptr;   // [1 + GEMM_TRACE_CAP * GEMM_TRACE_WORDS] words: counter, then records
  bool gemm_trace_checked = false;
  long long f0_launches[2] = {0, 0};   // fused matvec launches: bond matrices, two-level sites
  // launch decisions of the contraction kernel (mpse_gemm_path_stats; the order of include/mpsengine.h)
  enum GemmPath {
    GP_LAUNCH, GP_GENERAL, GP_WIDE, GP_SPLIT_B1, GP_SPLIT_BN, GP_DIE1, GP_DIE2, GP_SKEW, GP_ORDER, GP_MASK,
    GP_MASK_GLOBAL, GP_GROUPED, GP_GROUPED_SPLIT2, GP_GROUPED_MIX, GP_WMIX, GP_GROUPED_OUTMASK, GP_COUNT
  };
  long long gemm_paths[GP_COUNT] = {0};
  // mpse_block_qr: decompositions that took the Cholesky-QR path / that fell back from it to Householder
  long long qr_chol_calls = 0, qr_chol_fallbacks = 0, qr_calls = 0;
  // of qr_chol_calls: factorised by the right-looking / the left-looking Cholesky kernel (mpse_block_qr_path_stats)
  long long qr_chol_rl = 0, qr_chol_ll = 0;
  // mpse_block_svd[_full]: which block step ran the sweeps (mpse_block_svd_stats; the order of include/mpsengine.h).
  // The last two are no counts: gram_R of the latest Gram decomposition, the dynamic LDS granted to the column kernel
  enum SvdStat { SV_DECOMP, SV_COLUMN, SV_GRAM, SV_SWEEPS, SV_LAUNCHES, SV_GRAM_R, SV_COL_LDS, SV_COUNT };
  long long svd_stats[SV_COUNT] = {0};
  // optimistic mode of the Cholesky-QR path (mpse_block_qr_optimistic): breakdowns raise this sticky device word
  // instead of being read back per decomposition
  bool qr_optimistic = false;
  int qr_scheme = -1;            // mpse_block_qr_scheme: -1 environment default, 0 Householder only, 1 default rule, 2 every eligible shape
  // device words of the block QR (QR_WORDS of them): [0] sticky breakdown flag of the optimistic mode, [2] blocks
  // factorised by the Cholesky-QR kernels, [3] of them finished after two passes (mpse_block_qr_pass_stats), [4] two-pass
  // blocks whose pass-2 factor was the first-order one, [5] three-pass blocks whose pass-3 factor was
  // (mpse_block_qr_path_stats); allocated by qr_words()
  static constexpr int QR_WORDS = 8;
  int* qr_words_dev = nullptr;
  // mpse_expm_lanczos_batch: members solved by the batched kernels / through the single solve (mpse_expm_lanczos_batch_stats)
  long long lz_batch_members = 0, lz_batch_single = 0;
  // how the Lanczos solves of this context ran (mpse_expm_lanczos_path_stats; the order of include/mpsengine.h)
  enum LzPath {
    LP_SYNC, LP_ASYNC_DONE, LP_HOST_FIRST, LP_HOST_LATER, LP_LIMIT, LP_BD_ASYNC, LP_BD_SYNC, LP_FULL, LP_CONV,
    LP_NOCONV, LP_MERGED, LP_WAITS, LP_GROW, LP_PARTS, LP_VMASK, LP_UNVEC, LP_RESCALE, LP_ALIAS_RESTART, LP_COUNT
  };
  long long lz_paths[LP_COUNT] = {0};
  // what the conjugate-gradient solves of this context did (mpse_pcg_stats; the order of include/mpsengine.h)
  enum PcgStat {
    PS_SOLVES, PS_ITERS, PS_MATVECS, PS_WAITS, PS_END_TOL, PS_END_MAXITER, PS_END_CURVATURE, PS_TWOLAYER, PS_MASKED,
    PS_COUNT
  };
  long long pcg_stats[PS_COUNT] = {0};
  // the summed solves among them (mpse_pcg_sum_stats)
  enum PcgSumStat { PSS_SOLVES, PSS_ITERS, PSS_TERM_APPLIES, PSS_WAITS, PSS_DIAGS, PSS_COUNT };
  long long pcg_sum_stats[PSS_COUNT] = {0};
  // mpse_pcg_batch (mpse_pcg_batch_stats; the order of include/mpsengine.h)
  enum PcgBatchStat { PB_MEMBERS, PB_SINGLE, PB_SETS, PB_MATVEC_LAUNCHES, PB_WAITS, PB_COUNT };
  long long pcg_batch_stats[PB_COUNT] = {0};
  // mpse_mps_overlap (mpse_mps_overlap_stats; the order of include/mpsengine.h)
  enum OverlapStat { OV_CHAIN, OV_ENQUEUED, OV_SITES, OV_COUNT };
  long long overlap_stats[OV_COUNT] = {0};
  // mpse_mps_sandwich (mpse_mps_sandwich_stats; the order of include/mpsengine.h)
  enum SandwichStat { SW_CHAIN, SW_ENQUEUED, SW_SITES, SW_COUNT };
  long long sandwich_stats[SW_COUNT] = {0};
  // mpse_mps_corr (mpse_mps_corr_stats; the order of include/mpsengine.h)
  enum CorrStat { CR_CHAIN, CR_ENQUEUED, CR_SITES, CR_ENTRIES, CR_COUNT };
  long long corr_stats[CR_COUNT] = {0};
  // mpse_mps_rdm1 (mpse_mps_rdm1_stats; the order of include/mpsengine.h)
  enum Rdm1Stat { RD_CHAIN, RD_ENQUEUED, RD_SITES, RD_MATRICES, RD_COUNT };
  long long rdm1_stats[RD_COUNT] = {0};
  // mpse_mps_rdm2 (mpse_mps_rdm2_stats; the order of include/mpsengine.h)
  enum Rdm2Stat { RD2_CHAIN, RD2_ENQUEUED, RD2_SITES, RD2_PAIRS, RD2_COUNT };
  long long rdm2_stats[RD2_COUNT] = {0};
  // mpse_mps_trdm1 (mpse_mps_trdm1_stats; the order of include/mpsengine.h)
  enum Trdm1Stat { TR_CHAIN, TR_ENQUEUED, TR_SITES, TR_MATRICES, TR_COUNT };
  long long trdm1_stats[TR_COUNT] = {0};
  // mpse_mps_bond_spectra (mpse_mps_bond_spectra_stats; the order of include/mpsengine.h)
  enum BondSpecStat { BS_CHAIN, BS_ENQUEUED, BS_SITES, BS_BONDS, BS_MAX_SWEEPS, BS_COUNT };
  long long bondspec_stats[BS_COUNT] = {0};
  // mpse_mps_expect_many (mpse_mps_expect_many_stats; the order of include/mpsengine.h)
  enum ExpectStat { EX_CHAIN, EX_ENQUEUED, EX_SITES, EX_ENTRIES, EX_COUNT };
  long long expect_stats[EX_COUNT] = {0};
  // mpse_tda_* (mpse_tda_stats; the order of include/mpsengine.h)
  enum TdaStat { TD_HANDLES, TD_APPLIES, TD_ENV_UPDATES, TD_HEFF_APPLIES, TD_QDIAG_SITES, TD_DAVIDSON, TD_COUNT };
  long long tda_stats[TD_COUNT] = {0};
};
// What the caller of mpse_expm_lanczos said about the one solve that follows (mpse_expm_centre_mask, mpse_solve_slot):
// taken out of the context on entry and handed down as an argument to the scope of the asynchronous solve
struct SolveHints {
  mpse_ctx::CMask cmask;
  long long slot_key = 0;
};
int qr_words(mpse_ctx* ctx);     // allocate + zero ctx->qr_words_dev once (mpse_qr.hip)
int plan_words(mpse_ctx* ctx);   // allocate + zero ctx->plan_words_dev once (mpse_core.hip)
// The slot's device buffer becomes one of `bytes` bytes (its first 16 the zeroed word `changed`): room is made under the
// budget by evicting other slots; *ok = false when that cannot be done (the caller goes on as without a key).
int plan_slot_buffer(mpse_ctx* ctx, mpse_ctx::PlanSlot* slot, size_t bytes, bool* ok);

int mpse_fail(mpse_ctx* ctx, int code, const char* fmt, ...);
// Makes ctx->device the calling thread's current HIP device (a new thread starts on device 0; allocations and
// launches follow the CURRENT device, not the stream's).  Every entry point that allocates or launches calls it.
inline int mpse_bind(mpse_ctx* ctx) {
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur == ctx->device) return MPSE_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return mpse_fail(ctx, MPSE_ERR_HIP, "hipSetDevice(%d) failed", ctx->device);
  return MPSE_OK;
}
// asynchronous upload of a small host array through the pinned ring (the host buffer may be reused at once)
int stage_h2d(mpse_ctx* ctx, void* dst, const void* src_host, size_t bytes);
// zero fill as a plain kernel on the context stream (8-byte aligned ranges; others go through hipMemsetAsync)
int device_zero(mpse_ctx* ctx, void* dst, size_t bytes);
// an entry point is about to write `bytes` at `dst`: a described MPO site (mpse_mpo_site_hint) that overlaps the range no
// longer holds the values that were analysed - its description goes
inline void wsite_written(mpse_ctx* ctx, const void* dst, size_t bytes) {
  if (!dst || !bytes) return;
  std::lock_guard<std::mutex> lock(ctx->pool_mu);   // (before the first look at the map: mpse_free may run on a GC thread)
  if (ctx->wsite_info.empty()) return;
  const char* lo = static_cast<const char*>(dst);
  for (auto it = ctx->wsite_info.begin(); it != ctx->wsite_info.end();) {
    const char* w = static_cast<const char*>(it->first);
    if (lo < w + it->second.bytes && w < lo + bytes)
      it = ctx->wsite_info.erase(it);
    else
      ++it;
  }
}
// fold finished profiling records into the totals; call only when the stream is idle
void prof_drain(mpse_ctx* ctx);
// HIP-event bracket around a group of launches on the context stream; begin returns false when this call is not
// sampled (profiling off or not the N-th call) or no event could be had
bool prof_begin(mpse_ctx* ctx, int variant, double flops, double bytes, mpse_ctx::ProfRec* rec);
void prof_end(mpse_ctx* ctx, const mpse_ctx::ProfRec& rec);
// bracket that cannot leak its event pair: a scope left without end() (error return) hands the events back
struct ProfScope {
  mpse_ctx* ctx;
  mpse_ctx::ProfRec rec;
  bool on;
  ProfScope(mpse_ctx* c, int variant, double flops, double bytes) : ctx(c), on(prof_begin(c, variant, flops, bytes, &rec)) {}
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;
  void end() {
    if (on) prof_end(ctx, rec);
    on = false;
  }
  ~ProfScope() {
    if (!on) return;
    ctx->prof_free_events.push_back(rec.e0);
    ctx->prof_free_events.push_back(rec.e1);
  }
};

#define MPSE_HIP(ctx, call)                                                              \
  do {                                                                                   \
    hipError_t _e = (call);                                                              \
    if (_e != hipSuccess)                                                                \
      return mpse_fail((ctx), (_e == hipErrorOutOfMemory) ? MPSE_ERR_OOM : MPSE_ERR_HIP, \
                       "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(_e)); \
  } while (0)

#define MPSE_TRY(call)            \
  do {                            \
    int _s = (call);              \
    if (_s != MPSE_OK) return _s; \
  } while (0)

#define MPSE_BIND(ctx) MPSE_TRY(mpse_bind(ctx))

// Body of a *_stats export: counts[i], i < n, are the counters `src` of the context, zeros behind them
template <int COUNT>
static inline int stats_out(const mpse_ctx* ctx, long long (mpse_ctx::*src)[COUNT], int64_t* counts, int n) {
  if (!ctx || n < 0 || (n > 0 && !counts)) return MPSE_ERR_ARG;
  for (int i = 0; i < n; ++i) counts[i] = i < COUNT ? (ctx->*src)[i] : 0;
  return MPSE_OK;
}

// One launch of kern<true> or kern<false> on the context stream, picked by a host bool (complex / real vectors, 16-byte
// accesses), with one argument list.  MPSE_LAUNCH_TF leaves the error check to the call site (one check after a group
// of launches); MPSE_LAUNCH_TF_CHK checks at once; MPSE_LAUNCH_TF_LDS is MPSE_LAUNCH_TF with `lds` bytes of dynamic LDS.
#define MPSE_LAUNCH_TF_LDS(ctx, flag, kern, grid, block, lds, ...)                      \
  do {                                                                                  \
    if (flag)                                                                           \
      hipLaunchKernelGGL((kern<true>), grid, block, lds, (ctx)->stream, __VA_ARGS__);   \
    else                                                                                \
      hipLaunchKernelGGL((kern<false>), grid, block, lds, (ctx)->stream, __VA_ARGS__);  \
  } while (0)
#define MPSE_LAUNCH_TF(ctx, flag, kern, grid, block, ...) \
  MPSE_LAUNCH_TF_LDS(ctx, flag, kern, grid, block, 0, __VA_ARGS__)
#define MPSE_LAUNCH_TF_CHK(ctx, ...)     \
  do {                                   \
    MPSE_LAUNCH_TF(ctx, __VA_ARGS__);    \
    MPSE_HIP(ctx, hipGetLastError());    \
  } while (0)

// Entry points that may be recorded start with this: true -> the call was stored, return MPSE_OK.
#define MPSE_RECORDING(ctx) ((ctx)->defer_recording >= 0)
// runs and empties the armed list (no-op when none is armed); `status` of the solve it follows: a failed solve
// drops the list
int defer_replay(mpse_ctx* ctx, int status);

// RAII temporary from the pool
struct TmpBuf {
  mpse_ctx* ctx;
  void* p = nullptr;
  TmpBuf(mpse_ctx* c) : ctx(c) {}
  int alloc(size_t bytes) { return mpse_malloc(ctx, bytes ? bytes : 16, &p); }
  ~TmpBuf() {
    if (p) mpse_free(ctx, p);
  }
  template <class T>
  T* as() { return reinterpret_cast<T*>(p); }
};

static inline size_t dtype_size(int dt) { return dt == MPSE_C128 ? 16 : 8; }
static inline mpse_index idx1(int64_t ext, int64_t stride) { return mpse_index{ext, ext > 0 ? ext : 1, 0, stride}; }
static inline mpse_index idx2(int64_t hi_ext, int64_t lo_ext, int64_t s_hi, int64_t s_lo) {
  return mpse_index{hi_ext * lo_ext, lo_ext > 0 ? lo_ext : 1, s_hi, s_lo};
}

// What a solver fixes and keeps for the length of one solve (the Lanczos drivers of mpse_lanczos.hip, Davidson, PCG),
// handed by pointer to every matvec of it; null outside a solve.  The scope owns the device data that the matvecs of its
// solve compute once and share - masks, launch orders, the transposed right environment, the data of the fused matvec:
// a matvec fills them through the pointer it was given, and the end of the scope frees exactly these and nothing else.
// The context keeps one thing across solves: the plan data of a KEYED solve (mpse_solve_slot), in the slot of that key
// (mpse_ctx::plan_store).  The scope borrows the slot for its lifetime and hands it back, never frees it.  A stale slot
// cannot be observed: what the plan was built from is compared again at every solve - shapes and term table on the
// host, every flag byte on the device by the scan that writes it - and the planner, next on the stream, rebuilds the
// plan before the first matvec whenever one of them differs.  Without a key the scope keeps everything itself, as before.
struct SolveScope {
  mpse_ctx* ctx;
  mpse_ctx::PlanSlot* slot = nullptr;   // borrowed (borrow_slot), null: keyless
  bool slot_f0_taken = false;           // the slot serves the FIRST fused-matvec plan of the solve (mpse_heff0.hip)
  // device word that turns every contraction launch into a no-op once it is non-zero: the stop word of the asynchronous
  // Lanczos solve (LzCtl::stop: decision fallen, or the host has to take over), whose iterations are enqueued ahead of
  // the convergence decision
  const int* skip = nullptr;
  // Lanczos: the environments [env_lo, env_hi), constant over the solve - the tile-occupancy masks of operands inside
  // them are scanned once and kept (occ_cache), and so are the launch orders built on such masks (perm_cache)
  bool keeps_env_masks = false;
  const char* env_lo[2] = {nullptr, nullptr};
  const char* env_hi[2] = {nullptr, nullptr};
  // the caller's structural mask of the centre (mpse_expm_centre_mask, handed down by mpse_expm_lanczos): it describes
  // the operands inside the Krylov basis [krylov_lo, krylov_hi)
  mpse_ctx::CMask cmask;
  const char* krylov_lo = nullptr;
  const char* krylov_hi = nullptr;

  // Tile-occupancy masks of the operands inside the environment ranges: computed by the first matvec, reused by the
  // others (mpse_gemm.hip)
  struct OccKey {
    const void* ptr;
    long long r_ext, r_lo, r_shi, r_slo, k_ext, k_lo, k_shi, k_slo, sb;
    int nrows, tiles, nkw, batch, K, cplx;
  };
  struct OccEntry {
    OccKey key;
    void* mask;
  };
  std::vector<OccEntry> occ_cache;
  // launch orders of block-sparse products (k_tile_order), kept like the masks they were computed from
  struct PermEntry {
    const void *amask, *bmask;
    int tiles_m, tiles_n, nkt;
    void* perm;
  };
  std::vector<PermEntry> perm_cache;
  // Transposed right environment of the small-centre matvec (mpse_small.hip); another R replaces it
  struct SmallRt {
    const void* src = nullptr;
    void* rt = nullptr;
    size_t bytes = 0;
  } small_rt;
  // Data of the fused 0-site matvec (mpse_heff0.hip): transposed right environment, tile flags, part mask; other
  // operands replace it
  struct F0Cache {
    void* buf = nullptr;
    void* plan = nullptr;      // flags, terms, part mask, launch records: inside buf, or the slot's buffer past its word
    const void *L = nullptr, *R = nullptr, *W = nullptr, *cmask = nullptr;
    int Dl = 0, Dr = 0, w = 0, nsite = -1;
  } f0;

  explicit SolveScope(mpse_ctx* c) : ctx(c) {}
  SolveScope(const SolveScope&) = delete;
  SolveScope& operator=(const SolveScope&) = delete;
  ~SolveScope() {
    for (auto& e : occ_cache) mpse_free(ctx, e.mask);
    for (auto& e : perm_cache) mpse_free(ctx, e.perm);
    if (f0.buf) mpse_free(ctx, f0.buf);
    if (small_rt.rt) mpse_free(ctx, small_rt.rt);
    if (slot) slot->borrowed = false;
  }
  // takes the slot of `key` for this solve (0, MPSE_PLAN_REUSE=0 or a slot in use: none); mpse_core.hip
  void borrow_slot(long long key);
  bool in_env(const void* p) const {
    const char* c = static_cast<const char*>(p);
    return keeps_env_masks && ((c >= env_lo[0] && c < env_hi[0]) || (c >= env_lo[1] && c < env_hi[1]));
  }
  bool in_krylov(const void* p) const {
    const char* c = static_cast<const char*>(p);
    return cmask.ptr && c && c >= krylov_lo && c < krylov_hi;
  }
};

// One matvec's requests from its caller (the asynchronous Lanczos solve), and what the callee made of them
struct MatvecReq {
  // also accumulate sum conj(result) . y, as per-workgroup partials at `part` (room for `cap` of them); nb_out = number
  // written (0: the matvec could not take it, the caller runs its own reduction)
  struct Dot {
    const void* y = nullptr;
    double* part = nullptr;
    int cap = 0;
    int nb_out = 0;
  } dot;
  // The caller can take the result as the SUM of several tensors (the Lanczos update adds them while it reads): it
  // offers a buffer of cap_elems elements of the working dtype, n of them per part.  The last product of the plan may
  // then leave its K slices there instead of reducing them (mpse_gemm.hip: split products, halved tiles).  used =
  // number of parts written at ptr, ptr + n, .. (0: the result is complete in `out`, as usual; -2: `out` and the
  // second slot).
  struct Parts {
    void* ptr = nullptr;
    long long cap_elems = 0, n = 0;
    int used = 0;
    // The caller can also take parts that hold only SOME 16 x 16 tiles of the result (mpse_heff0.hip): the callee then
    // sets `mask` (device; one 64-bit word per tile of the result viewed as a matrix with rows of mask_row elements,
    // mask_tiles tiles per tile row: bit s = part s holds the tile) and the consumer adds exactly the parts named there
    bool masked_ok = false;
    const unsigned long long* mask = nullptr;
    int mask_row = 0, mask_tiles = 0;
  } parts;
  // Only these tiles of the result are needed: the caller reads the result nowhere else (the Lanczos update under the
  // structural mask of the centre, with the same three quantities: the result as rows of `row` elements, byte
  // [(column / 64) * pitch + row / 16], zero = never read).  The launch that completes the result may leave the tiles
  // that lie wholly outside unwritten - only together with the dot request, whose partials of such tiles are (0, 0).
  struct OutMask {
    const unsigned char* mask = nullptr;
    int row = 0, pitch = 0;
  } out_mask;
};

// What run_plan asks of one product beyond its descriptor (gemm_call; gemm_grouped takes the dot request and the
// result mask as arguments)
struct ProductReq {
  MatvecReq::Dot* dot = nullptr;   // the product completes the matvec result: it carries the caller's dot request
  // beta source: C = A.B + beta * Cin(i, j) with Cin's own index maps
  const void* cin = nullptr;
  mpse_index cin_m{}, cin_n{};
  // the CONSUMER adds the K slices of a split product while it reads them (the elementwise MPO step of the small
  // sites): the product leaves its raw slices at `slices` (slice s at slices + s * M * N elements, compact like C) and
  // launches no reduction; slices_used = number of slices (0: the product stored C as usual)
  void* slices = nullptr;
  size_t slices_cap = 0;
  int slices_used = 0;
};

// The matvec behind mpse_heff_apply, for a caller inside a solve (sc) and / or with requests (mv); both may be null
int heff_apply(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, void* out, SolveScope* sc,
               MatvecReq* mv);
// The two-layer matvec behind mpse_heff_apply2, for a caller inside a solve (sc may be null)
int heff_apply2(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, void* out, SolveScope* sc);
// One term of the finite-temperature correction-vector operator (mpse_heff_apply_ft), inside a solve (sc may be null)
int heff_apply_ft(mpse_ctx* ctx, int dtype, const mpse_heff_ft* h, const void* C, void* out, SolveScope* sc);
// extents and leg order of such a term; refuses with "<who>: ..." (hidden: the dynamic symbol table stays what it was)
__attribute__((visibility("hidden"))) int ft_shape_ok(mpse_ctx* ctx, const mpse_heff_ft& h, const char* who);
// One-launch matvec of small 0- / 1-site centres (mpse_small.hip); *taken says whether it ran (else: the plans)
int heff_small_try(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, void* out, SolveScope* sc,
                   MatvecReq* mv, bool* taken);

// Batched small-centre Krylov solves (mpse_expm_lanczos_batch, mpse_lanczos.hip): what differs between the members of one
// launch set beyond their region of the slab (mpse_lanczos_plan.h: vectors, scalars, partials, flag word and control
// block at member-0 addresses + m * mstride bytes).  The kernels of the asynchronous solve take the table as a nullable
// pointer: a single solve is a launch set of one member that passes its C and out directly and uploads no table.
struct BatchMember {
  const void* L;    // environments and MPO site of the member's effective Hamiltonian
  const void* R;
  const void* W;
  void* Rt;         // its transposed right environment (mpse_small.hip)
  const void* C;    // start vector
  void* out;        // result
};
template <class T>
__host__ __device__ inline T* member_ptr(T* p, unsigned m, long long mstride) {
  return p ? reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + uintptr_t(m) * uintptr_t(mstride)) : p;
}
// The plan of the one-launch matvec for the request of the asynchronous Lanczos solve (result parts of up to 4 n
// elements, dot_cap partials): false when h does not take that path with its dot request; else the bytes of a transposed
// right environment, the number of result parts and the dot partials the launch writes
bool heff_small_batch_plan(const mpse_heff* h, int dtype, int64_t n, int dot_cap, size_t* rt_bytes, int* nparts,
                           int* nb_dot);
// B transposed right environments (mem[m].R -> mem[m].Rt) in one launch; member m is skipped while its word is set
int heff_small_batch_rt(mpse_ctx* ctx, int dtype, const mpse_heff* h, int B, const BatchMember* mem, const int* skip0,
                        long long mstride);
// H_m C_m for B members with the shape of h in one launch: result parts at parts0, <H C, C> partials at dot_part0
int heff_small_batch_apply(mpse_ctx* ctx, int dtype, const mpse_heff* h, int B, const BatchMember* mem,
                           const void* C0, void* parts0, int64_t n, double* dot_part0, int dot_cap, const int* skip0,
                           long long mstride);
// One-launch two-layer matvec of small one-site centres (mpse_small2.hip), the matvec of mpse_pcg_batch.  Eligibility is
// a rule on the member's own shape: every extent within these limits and the launch plan within the LDS budget.
constexpr int SM2_WMAX = 8;            // MPO bond channels per layer (wl, wr)
constexpr int SM2_DMAX = 16;           // physical dimension
constexpr int SM2_BMAX = 64;           // bond dimensions Dl, Dr
constexpr int SM2_LDS_MAX = 65536;     // bytes of LDS per workgroup (a second workgroup per compute unit stays possible)
constexpr int SM2_NNZ_LDS = 1024;      // entries of the sparse W list kept in LDS (the rest is read from memory)
struct Small2Plan {
  int Dl, Dr, d, wl, wr;
  int jh, nslice, G;                   // slice width of the ket bond of R, number of slices, K groups of the last step
  int rows, pitch, nnz_lds;            // sparse W list: rows (x, y), capacity per row, entries held in LDS
  int ptr_dbl, idx_dbl, csr_dbl;       // LDS doubles of the row pointers, the indices, the whole list (even)
  int off_A, off_B;                    // LDS offsets (elements of the working type) behind the row of Lt
  int lds;                             // dynamic LDS bytes
};
// one member of a launch set: operator parts, per-solve copies, vectors, partials and control block
struct Pcg2Member {
  const double *L, *R, *W;
  double* Lt;                          // (Dl, wl, wl, Dl): [d][b][c][a] = L[a][b][c][d]
  int *csr_ptr, *csr_idx;              // rows + 1 offsets; (u << 8) | v per entry
  double* csr_val;
  const double *mask, *diag, *b;
  double *x, *y, *q, *r, *p;
  double *part_bb, *part_pq, *part_bx, *part_rz0, *part_rz1;
  void* ctl;                           // PcgCtl (mpse_pcg.hip); its first word is `done`
  double shift;
};
// false: the shape does not take the one-launch two-layer matvec
bool small2_plan(int dtype, int64_t Dl, int64_t d, int64_t Dr, int64_t wl, int64_t wr, Small2Plan* p);
// per solve: transposed left environments and sparse W lists of B members in one launch
int small2_prep(mpse_ctx* ctx, int dtype, const Small2Plan& p, int B, const Pcg2Member* mem);
// one launch for B members; mode 0: y = Heff2 x, mode 1: q = mask * Heff2 p + shift * p with the partials of p^H q
int small2_apply(mpse_ctx* ctx, int dtype, const Small2Plan& p, int B, const Pcg2Member* mem, int mode);
// Fused 0-site matvec for large complex bond matrices (mpse_heff0.hip): number of parts it would deliver (0 = not
// eligible) and the attempt itself (needs a solve, which keeps its data, and MatvecReq::Parts::masked_ok)
int heff0_fused_parts(const mpse_heff* h, int dtype);
int heff0_fused_try(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, const double* w_host,
                    SolveScope* sc, MatvecReq* mv, bool* taken);

// convenience wrapper over mpse_gemm used by the contraction entry points
int gemm_call(mpse_ctx* ctx, int dta, int dtb, int conja, int conjb, mpse_index ma, mpse_index ka,
              mpse_index kb, mpse_index nb, mpse_index mc, mpse_index nc, int64_t batch, int64_t sba,
              int64_t sbb, int64_t sbc, const void* A, const void* B, void* C, double alpha = 1.0,
              double beta = 0.0, int skip_zero = 0, SolveScope* sc = nullptr, ProductReq* rq = nullptr);

// Grouped launch of the contraction kernel (mpse_gemm.hip): up to 8 groups of equal height dividing the tile rows, each
// with its own result C (same index maps) and up to 4 (A, B) operand pairs whose products are summed (+ beta C, beta 0
// or 1).  am / bm: tile-occupancy flags of the operands (occ_mask_get layout, row pitches below), null = dense.
struct GroupedSeg {
  const void* A = nullptr;
  const void* B = nullptr;
  const unsigned char* am = nullptr;
  const unsigned char* bm = nullptr;
};
struct GroupedMixTerm {       // one diagonal of one block of an MPO site applied to a tensor laid out like C's rows
  const void* src = nullptr;  // (complex128, rows (a, x) at stride ld, columns contiguous)
  int b = 0, f = 0, delta = 0;
};
struct GroupedGrp {
  GroupedSeg seg[4];
  void* C = nullptr;
  int nseg = 0;
  double beta = 0.0;
};
struct GroupedDesc {
  int dta = MPSE_F64, dtb = MPSE_F64;
  mpse_index ma{}, ka{}, kb{}, nb{}, mc{}, nc{};
  int ngrp = 0;
  GroupedGrp grp[8];
  int am_pitch = 0, bm_pitch = 0;
  bool masks_stable = false;   // the flags live as long as the running solve's caches: the launch order is kept with them
  // one group only: two workgroups per output tile, each over half of its occupied K tiles; the first half (+ beta C)
  // goes to C, the second to c2 (laid out like C): the consumer adds them
  bool split2 = false;
  void* c2 = nullptr;
  // epilogue mix (mpse_plans.h EpiTerm; complex x complex only): the beta term of group mix_grp (beta = 1) is
  //   sum_t W[b_t, x, x + delta_t, f_t] src_t[(a, x + delta_t), j]   for output row (a, x), x = row mod d, 64 % d == 0
  // instead of C itself.  W: the real site (., d, d, wr) on the device.
  int nmix = 0, mix_grp = 0;
  GroupedMixTerm mix[8];
  const void* mix_w = nullptr;
  int mix_d = 0, mix_wr = 0;
  long long mix_ld = 0;
};
// om: MatvecReq::out_mask of the caller when this launch completes a matvec result, else null; taken only with `dot`
int gemm_grouped(mpse_ctx* ctx, const GroupedDesc& d, SolveScope* sc, MatvecReq::Dot* dot,
                 const MatvecReq::OutMask* om = nullptr);
int occ_mask_get(mpse_ctx* ctx, SolveScope* sc, const void* ptr, int dtype, mpse_index r, mpse_index k,
                 TmpBuf& tmp, const unsigned char** flags, int* pitch, bool* stable);

// Low-latency read-back of a few device doubles: a one-wave kernel copies them into the mapped pinned buffer
// and then publishes a sequence number; the host spins on that number instead of going through a copy-engine
// transfer plus hipStreamSynchronize (the gap the GPU idles after every convergence check shrinks from ~25 us to
// the launch latency).  count <= 1024; the values land at ctx->pinned + slot, below PIN_SLOTS_END.
int publish_and_wait(mpse_ctx* ctx, const double* dsrc, int count, int slot);
// The waiting half alone, for a kernel that publishes by itself (writes `count` doubles at pinned_dev + slot, then the
// sequence number `seq` at pinned_dev + PIN_SEQ, each followed by __threadfence_system()).
int publish_wait_seq(mpse_ctx* ctx, double seq, const double* dsrc, int count, int slot);
// The wait path of the solvers whose deciding kernel publishes its control block(s).  publish_target says where to:
// `wait_here` = the host waits at this launch; all null / zero when it does not or when there is no mapped view (the
// kernel then publishes nothing).  publish_collect, after the launch: waits for the sequence number - or, when none was
// handed out or it never arrives, copies the B blocks of W doubles, `stride` bytes apart at dsrc, to the slot (B == 1: a
// plain copy, else a 2-D copy) - drains the profiler queue and copies the blocks from the slot to `host_out`.
// (hidden: the dynamic symbol table of the library stays what it was)
struct PublishAt {
  double* pub;
  volatile double* seq_slot;
  double seq;
};
__attribute__((visibility("hidden"))) PublishAt publish_target(mpse_ctx* ctx, bool wait_here, int slot);
__attribute__((visibility("hidden"))) int publish_collect(mpse_ctx* ctx, const PublishAt& at, const void* dsrc, size_t stride,
                                                          int B, int W, int slot, void* host_out);

// The Davidson iteration of mpse_davidson (mpse_davidson.hip) on vectors of n elements of `dtype` under an operator the
// caller supplies: fn(self, x, y) enqueues y = H x on the context stream.  Everything else - arguments, limits, results -
// as mpse_davidson documents it.
struct DavOp {
  int (*fn)(void* self, const void* x, void* y);
  void* self;
};
__attribute__((visibility("hidden"))) int davidson_solve(mpse_ctx* ctx, int dtype, int64_t n, const DavOp& op,
                                                         const void* hdiag_f64, const void* mask_f64, int nroots,
                                                         int nguess, const void* guess, double tol, int max_cycle,
                                                         int max_space, double lindep, double shift, double* e_host,
                                                         void* x_out, int* ncycle, int* nmatvec);

// reductions (mpse_vec.hip): results land in ctx->pinned after a stream sync
int dotc_sync(mpse_ctx* ctx, int dtype, const void* x, const void* y, int64_t n, double* re, double* im);

// Householder QR on column-major workspaces (mpse_qr2.hip), shared by mpse_block_qr and the SVD
struct HhParam {  // per reflector: H = I - tau v v^H, v = (1, scale * tail)
  double tau_re, tau_im;
  double scale_re, scale_im;
  // panel-blocked kernels (mpse_qr2.hip): inner products u_i^H u_l with the earlier reflectors i of the same
  // four-column panel (re, im; i = 0 .. l-1), by-products of the panel factorisation that the compact-WY
  // applications need for T
  double g[6];
};
// one block of a QR: the blocks of a call live in one column-major workspace
struct QrBlk {
  long long ws_off;  // element offset of the mm x nn block inside the workspace
  long long q_off;   // element offset of its mm x k Q inside the Q buffer
  int mm, nn, k;
  int prm_off;       // offset of its reflector parameters
  int nq = 0;        // columns of Q to form (0 -> k); columns beyond k complete the basis (full_matrices SVD)
  long long row_off = 0, col_off = 0;   // block_qr: where the block's row / column index lists start (device lists)
};
constexpr int HH_BATCH_MAX_ROWS = 4096;                      // taller blocks: unblocked kernels, one block at a time
constexpr unsigned long long GEMM_TRACE_CAP = 1ull << 21;   // records
constexpr int GEMM_TRACE_WORDS = 10;                         // 64-bit words per record
// any block height; ``blks_dev``: the same descriptors already on the device (else they are uploaded here)
int hh_qr(mpse_ctx* ctx, bool cplx, double* ws, double* q, HhParam* prm, const QrBlk* blks_host, int nblk, bool form_q,
          const QrBlk* blks_dev = nullptr);
// Shifted Cholesky-QR of tall blocks on MFMA (mpse_cholqr.hip).  The blocks are factorised in place in their column-major
// workspaces and scattered to U / Vt like mpse_block_qr does; *ok = false when a block was rank deficient or too ill
// conditioned for the scheme (device flag, one read-back): the caller then runs the Householder path on fresh copies.
bool cholqr_eligible(const mpse_ctx* ctx, const QrBlk* blks, int nblk);
int cholqr_blocks(mpse_ctx* ctx, bool cplx, double* ws, const QrBlk* blks, int nblk, const long long* drows,
                  const long long* dcols, int herm, void* U, void* Vt, long long K, long long ncol, bool* ok);
// zero fill of two ranges in one launch (8-byte aligned)
int device_zero2(mpse_ctx* ctx, void* a, size_t abytes, void* b, size_t bbytes);
