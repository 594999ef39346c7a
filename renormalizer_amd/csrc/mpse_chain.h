// What the "whole chain in one engine call" entry points share (mpse_overlap.hip includes this, mpse_sandwich.hip through
// mpse_sandwich_step.h, the site step it shares with mpse_expect.hip; the calls with a selection include it through
// mpse_chain_walk.h, which adds the stages and walks that those six share: mpse_corr.hip, mpse_rdm2.hip,
// mpse_bondspec.hip and mpse_expect.hip directly, mpse_rdm1.hip and mpse_trdm1.hip through mpse_chain_sites.h, the one
// call those two are; no other file includes any of the four).  Each call walks a chain of site tensors either with its
// own one-workgroup kernel(s), the environment in LDS, or as products enqueued back to back; which one, its plan decides
// from the dims table alone.  A call supplies its descriptor row, its plan (the sizing behind chain_table_ok), its
// kernel(s) with their loop nests and its enqueued fallback; the element type, the limits of a launch, the publishing
// tail, the staging, the dispatch and the bookkeeping of the exports are here.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "mpse_internal.h"

// -------------------------------------------------------------------------------------------------- limits of a launch
constexpr int CHAIN_THREADS = 1024;               // one workgroup, 16 waves: the largest a launch may have
constexpr int64_t CHAIN_LDS_MAX = 160 * 1024;     // LDS of a gfx950 compute unit; one workgroup may use all of it
constexpr int64_t CHAIN_EXT_MAX = 1 << 16;        // extents above this never take a chain kernel (32-bit offsets)
// rows of an environment in LDS are padded to an odd number of elements: the threads of a wave that work on different
// rows b of T[b, k'] = sum_k E[b, k] K[k, k'] read E[b, k] for one k at a time, a column, and an even pitch would put a
// column on few banks
constexpr int64_t chain_pitch(int64_t d) { return d | 1; }

// --------------------------------------------------------------------------------------------------------- device side
// Small operands read at addresses that are the same for the whole workgroup: through the constant address space the
// loads are scalar, and a branch on the value is taken by the wave, not by its lanes
using cdouble_p = const __attribute__((address_space(4))) double*;

// working element of the chain kernels
template <bool CPLX>
struct ChainEl;
template <>
struct ChainEl<false> {
  using T = double;
  __device__ static T zero() { return 0.0; }
  __device__ static T one() { return 1.0; }
  __device__ static T ld(const void* p, int /*cplx*/, int i) { return static_cast<const double*>(p)[i]; }
  __device__ static T ldc(const void* p, int /*cplx*/, int i) { return ((cdouble_p)p)[i]; }
  __device__ static T ldm(const double* m, int i) { return m[2 * i]; }   // local matrices are complex pairs
  __device__ static bool nz(T a) { return a != 0.0; }
  __device__ static T cj(T a) { return a; }
  __device__ static void add(T& acc, T a) { acc += a; }
  __device__ static void fma(T& acc, T a, T b) { acc += a * b; }
  __device__ static T shfl_down(T a, int off) { return __shfl_down(a, off, 64); }
  __device__ static double re(T a) { return a; }
  __device__ static double im(T) { return 0.0; }
};
template <>
struct ChainEl<true> {
  using T = double2;
  __device__ static T zero() { return make_double2(0.0, 0.0); }
  __device__ static T one() { return make_double2(1.0, 0.0); }
  __device__ static T ld(const void* p, int cplx, int i) {
    return cplx ? static_cast<const double2*>(p)[i] : make_double2(static_cast<const double*>(p)[i], 0.0);
  }
  __device__ static T ldc(const void* p, int cplx, int i) {
    cdouble_p q = (cdouble_p)p;
    return cplx ? make_double2(q[2 * i], q[2 * i + 1]) : make_double2(q[i], 0.0);
  }
  __device__ static T ldm(const double* m, int i) { return make_double2(m[2 * i], m[2 * i + 1]); }
  __device__ static bool nz(T a) { return a.x != 0.0 || a.y != 0.0; }
  __device__ static T cj(T a) { return make_double2(a.x, -a.y); }
  __device__ static void add(T& acc, T a) {
    acc.x += a.x;
    acc.y += a.y;
  }
  __device__ static void fma(T& acc, T a, T b) {
    acc.x += a.x * b.x - a.y * b.y;
    acc.y += a.x * b.y + a.y * b.x;
  }
  __device__ static T shfl_down(T a, int off) {
    return make_double2(__shfl_down(a.x, off, 64), __shfl_down(a.y, off, 64));
  }
  __device__ static double re(T a) { return a.x; }
  __device__ static double im(T a) { return a.y; }
};

template <bool CPLX>
using ChainT = typename ChainEl<CPLX>::T;

// Tail of a kernel whose result is one complex scalar, for its one deciding thread: the value goes to out[0..1] and,
// when pub is set, to the mapped host buffer followed by the sequence number (publish_collect)
__device__ __forceinline__ void chain_publish2(double* out, double* pub, volatile double* seq_slot, double seq,
                                               double re, double im) {
  out[0] = re;
  out[1] = im;
  if (pub) {
    pub[0] = re;
    pub[1] = im;
    __threadfence_system();
    *seq_slot = seq;
    __threadfence_system();
  }
}

// ----------------------------------------------------------------------------------------------------------- host side
// Is the dims table (nsite rows of row_len extents) a chain: every extent >= 1, the bonds in the columns `left` of the
// first row and `right` of the last row 1, and right[j] of a row equal to left[j] of the next one
static inline bool chain_table_ok(int nsite, const int64_t* dims, int row_len, std::initializer_list<int> left,
                                  std::initializer_list<int> right) {
  if (nsite < 1 || !dims) return false;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* d = dims + (int64_t)row_len * i;
    for (int j = 0; j < row_len; ++j)
      if (d[j] < 1) return false;
    if (i == 0)
      for (int c : left)
        if (d[c] != 1) return false;
    if (i == nsite - 1)
      for (int c : right)
        if (d[c] != 1) return false;
    if (i + 1 < nsite)
      for (auto l = left.begin(), r = right.begin(); l != left.end(); ++l, ++r)
        if (d[*r] != d[row_len + *l]) return false;
  }
  return true;
}

// info[i], i < n, of a *_plan export: the nv values of the call, zeros behind them
static inline void plan_info_out(int64_t* info, int n, const int64_t* v, int nv) {
  for (int i = 0; i < n && info; ++i) info[i] = i < nv ? v[i] : 0;
}

// The MPSE_*_CHAIN switch of a call, read per call: '0' (every chain through the enqueued path), '1' (every chain that
// fits through the kernels), 0 when it is unset or anything else
static inline char chain_env_switch(const char* name) {
  const char* env = getenv(name);
  return env && (env[0] == '0' || env[0] == '1') ? env[0] : 0;
}

// The site lists of a call (`call`: its name in the messages): a null site or an unknown dtype is MPSE_ERR_ARG;
// *cplx: some tensor is complex128
static inline int chain_scan_sites(mpse_ctx* ctx, const char* call, int nsite,
                                   std::initializer_list<const void* const*> ptrs,
                                   std::initializer_list<const int*> dtypes, bool* cplx) {
  *cplx = false;
  for (int i = 0; i < nsite; ++i) {
    for (const void* const* p : ptrs)
      if (!p[i]) return mpse_fail(ctx, MPSE_ERR_ARG, "%s: null site %d", call, i);
    for (const int* dt : dtypes) {
      if (dt[i] != MPSE_F64 && dt[i] != MPSE_C128)
        return mpse_fail(ctx, MPSE_ERR_ARG, "%s: unknown dtype at site %d", call, i);
      *cplx = *cplx || dt[i] == MPSE_C128;
    }
  }
  return MPSE_OK;
}

// Lets the kernels use `bytes` of dynamic LDS; once per kernel, whichever thread comes first (the list of kernels that
// are done is per translation unit, a handful each; one that no longer fits is merely set again)
static inline int chain_lds_attr(mpse_ctx* ctx, std::initializer_list<const void*> kernels, int64_t bytes) {
  static std::mutex mu;
  static const void* done[16];
  static int ndone = 0;
  std::lock_guard<std::mutex> lock(mu);
  for (const void* f : kernels) {
    if (std::find(done, done + ndone, f) != done + ndone) continue;
    MPSE_HIP(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (ndone < 16) done[ndone++] = f;
  }
  return MPSE_OK;
}

// kern<cplx> of the <true> / <false> pair of a chain kernel on `grid` workgroups of CHAIN_THREADS threads with `lds` bytes
// of dynamic LDS (chain_lds_attr first); the error check is left to the call site, as with MPSE_LAUNCH_TF
#define CHAIN_LAUNCH(ctx, cplx, kern, grid, lds, ...) \
  MPSE_LAUNCH_TF_LDS(ctx, cplx, kern, dim3((unsigned)(grid)), dim3(CHAIN_THREADS), (size_t)(lds), __VA_ARGS__)
#define CHAIN_KERNELS(kern) reinterpret_cast<const void*>(&kern<true>), reinterpret_cast<const void*>(&kern<false>)

// the descriptor rows of a call as a pooled device table, uploaded through the pinned ring
template <class Row>
static int chain_stage_rows(mpse_ctx* ctx, TmpBuf& tab, const std::vector<Row>& rows) {
  MPSE_TRY(tab.alloc(rows.size() * sizeof(Row)));
  return stage_h2d(ctx, tab.p, rows.data(), rows.size() * sizeof(Row));
}

// One workgroup, result = one complex scalar: stages the rows, runs launch(table, result, publish target) - a
// CHAIN_LAUNCH of a kernel that ends with chain_publish2 - and collects the two doubles into out2
template <class Row, class Launch>
static int chain_scalar_launch(mpse_ctx* ctx, const std::vector<Row>& rows, Launch&& launch, double* out2) {
  TmpBuf tab(ctx), res(ctx);
  MPSE_TRY(chain_stage_rows(ctx, tab, rows));
  MPSE_TRY(res.alloc(2 * sizeof(double)));
  const PublishAt at = publish_target(ctx, true, mpse_ctx::PIN_SCALAR2);
  launch(tab.as<const Row>(), res.as<double>(), at);
  MPSE_HIP(ctx, hipGetLastError());
  return publish_collect(ctx, at, res.p, 0, 1, 2, mpse_ctx::PIN_SCALAR2, out2);
}

// End of an enqueued path whose last environment is one element at `dev`: the host reads it here.  The word behind a
// real one is inside the buffer and not used.
static inline int chain_scalar_result(mpse_ctx* ctx, const void* dev, bool is_complex, double* out2) {
  MPSE_TRY(publish_and_wait(ctx, static_cast<const double*>(dev), 2, mpse_ctx::PIN_SCALAR2));
  out2[0] = ctx->pinned[mpse_ctx::PIN_SCALAR2];
  out2[1] = is_complex ? ctx->pinned[mpse_ctx::PIN_SCALAR2 + 1] : 0.0;
  return MPSE_OK;
}

// A real site of n elements next to complex operands: widened into the pooled buffer `buf` (allocated here on first
// use, with room for `cap` elements; it lives as long as its owner, to the end of the call), *site then points there
static inline int widen_site(mpse_ctx* ctx, TmpBuf& buf, const void** site, int64_t n, int64_t cap) {
  if (!buf.p) MPSE_TRY(buf.alloc((size_t)cap * 16));
  MPSE_TRY(mpse_cast_f64_to_c128(ctx, buf.p, *site, n));
  *site = buf.p;
  return MPSE_OK;
}
