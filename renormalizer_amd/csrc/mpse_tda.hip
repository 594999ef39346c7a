// mpse_tda_*: the Hamiltonian projected onto the first-order tangent space of a matrix product state (replaces the
// closures hop and hdiag of mps/tda.py:152-247 of the reference).  One application walks the chain twice - G from the
// right, F from the left - with the environment updates and one-site matvecs every sweep uses (mpse_env_update,
// heff_apply), 4 (N - 1) updates and 3 N matvecs at most; the reference rebuilds an environment chain for every site that
// carries coefficients.  The recursion is stated in include/mpsengine.h.  The two sums per site are taken as separate
// products followed by mpse_axpy (DESIGN.md says why).  The only kernel of this file is k_tda_qdiag, the column-wise dot
// of the preconditioner that no product expresses.
#include <algorithm>
#include <vector>

#include "mpse_device.h"
#include "mpse_internal.h"

struct mpse_tda {
  int nsite = 0;
  int dtype = MPSE_F64;               // working dtype: complex as soon as any operand is
  size_t es = 8;
  std::vector<int64_t> dims;          // nsite rows (Dl, d, Dr, wl, wr, n)
  std::vector<const void*> A, B, U, W;   // sites in the working dtype (the caller's, or widened copies in `owned`)
  std::vector<int> wdt;
  std::vector<void*> owned;           // everything the handle frees
  std::vector<void*> L, R;            // L_0 .. L_N, R_0 .. R_N (L_N and R_0 are not built: null)
  std::vector<int64_t> lunit, runit;  // their unit channels (1-based, 0 = none)
  std::vector<int64_t> xoff, toff, goff;   // elements before X_j in x, T_j in Tb, G_j in Gb
  std::vector<char> has_f, has_g;     // F_j / G_j is not identically zero
  int64_t xsize = 0;
  void *Tb = nullptr, *Gb = nullptr, *F0 = nullptr, *F1 = nullptr, *Etmp = nullptr, *O = nullptr, *Otmp = nullptr;

  const int64_t* row(int j) const { return dims.data() + 6 * j; }
  int64_t Dl(int j) const { return row(j)[0]; }
  int64_t d(int j) const { return row(j)[1]; }
  int64_t Dr(int j) const { return row(j)[2]; }
  int64_t wl(int j) const { return row(j)[3]; }
  int64_t wr(int j) const { return row(j)[4]; }
  int64_t n(int j) const { return row(j)[5]; }
};

namespace {

// Byte bound of X[b, c, (g, l)] of one chunk of columns l in mpse_tda_hdiag.  A memory choice, not a measurement;
// MPSE_TDA_X_BYTES in the environment overrides it, read per call (for tests and measurements).
constexpr int64_t TDA_X_BYTES_MAX = int64_t(256) << 20;
// environments below this bond are not searched for a unit channel: the contraction plans use one only where the
// product it saves pays (mpse_plans.h unit_pays), and the search is a host round trip
constexpr int64_t TDA_UNIT_MIN_BOND = 128;
constexpr double TDA_UNIT_TOL = 1e-12;

int64_t tda_x_bytes() {
  const char* env = getenv("MPSE_TDA_X_BYTES");
  const long long v = env ? strtoll(env, nullptr, 10) : 0;
  return v > 0 ? (int64_t)v : TDA_X_BYTES_MAX;
}

// Q[(b, g, h), l] = sum_c X[b, c, g, l] U[c, h, l0 + l]: a dot over c for every column l, which no product expresses
// (l is shared by both operands and the result).  X (wl, Dl, d, nl) is the chunk of columns [l0, l0 + nl), U (Dl, d, n)
// the whole tangent factor.  One thread per (row, l), threads along l: every load and store of a wave is contiguous
// (16 bytes per lane when complex); memory bound: X is read once, U once per (b, g).
template <bool CPLX>
__global__ __launch_bounds__(256) void k_tda_qdiag(const double* __restrict__ X, const double* __restrict__ U,
                                                   double* __restrict__ Q, int wl, int Dl, int d, long long n,
                                                   long long l0, long long nl) {
  const long long total = (long long)wl * d * d * nl;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    const long long r = t / nl, l = t - r * nl;
    const int h = (int)(r % d), g = (int)((r / d) % d), b = (int)(r / ((long long)d * d));
    const long long x0 = ((long long)b * Dl * d + g) * nl + l, xs = (long long)d * nl;
    const long long u0 = (long long)h * n + l0 + l, us = (long long)d * n;
    if (CPLX) {
      const double2* x2 = reinterpret_cast<const double2*>(X);
      const double2* u2 = reinterpret_cast<const double2*>(U);
      double re = 0, im = 0;
      for (int c = 0; c < Dl; ++c) {
        const double2 a = x2[x0 + c * xs], v = u2[u0 + c * us];
        re += a.x * v.x - a.y * v.y;
        im += a.x * v.y + a.y * v.x;
      }
      reinterpret_cast<double2*>(Q)[t] = make_double2(re, im);
    } else {
      double re = 0;
      for (int c = 0; c < Dl; ++c) re += X[x0 + c * xs] * U[u0 + c * us];
      Q[t] = re;
    }
  }
}

// Is the table a chain with tangent widths that fit: the check of chain_table_ok (mpse_chain.h) for rows
// (Dl, d, Dr, wl, wr, n) with 0 <= n <= Dl d
bool tda_table_ok(int nsite, const int64_t* dims) {
  if (nsite < 1 || !dims) return false;
  for (int i = 0; i < nsite; ++i) {
    const int64_t* r = dims + 6 * i;
    for (int j = 0; j < 5; ++j)
      if (r[j] < 1) return false;
    if (r[5] < 0 || r[5] > r[0] * r[1]) return false;
    if (i == 0 && (r[0] != 1 || r[3] != 1)) return false;
    if (i == nsite - 1 && (r[2] != 1 || r[4] != 1)) return false;
    if (i + 1 < nsite && (r[2] != r[6] || r[4] != r[6 + 3])) return false;
  }
  return true;
}

mpse_dims site_dims(const mpse_tda& h, int j, int64_t env_unit) {
  mpse_dims s{};
  s.Dl_bra = s.Dl_ket = h.Dl(j);
  s.Dr_bra = s.Dr_ket = h.Dr(j);
  s.d0 = h.d(j), s.d1 = 1, s.danc = 1;
  s.wl = h.wl(j), s.wm = 1, s.wr = h.wr(j);
  s.env_unit = env_unit;
  return s;
}

int tda_alloc(mpse_ctx* ctx, mpse_tda* h, int64_t elems, void** p) {
  MPSE_TRY(mpse_malloc(ctx, size_t(elems > 0 ? elems : 1) * h->es, p));
  h->owned.push_back(*p);
  return MPSE_OK;
}

// the site in the working dtype: the caller's buffer, or a widened copy the handle owns
int tda_site(mpse_ctx* ctx, mpse_tda* h, const void* src, int dt, int64_t elems, const void** out) {
  *out = src;
  if (dt == h->dtype) return MPSE_OK;
  void* p = nullptr;
  MPSE_TRY(tda_alloc(ctx, h, elems, &p));
  MPSE_TRY(mpse_cast_f64_to_c128(ctx, p, src, elems));
  *out = p;
  return MPSE_OK;
}

// out = upd(env; bra, W_j, ket), bra conjugated; env_unit: the unit channel of env (0: none / unknown)
int tda_env(mpse_ctx* ctx, const mpse_tda& h, int domain, int j, const void* env, int64_t env_unit, const void* ket,
            const void* bra, void* out, bool count) {
  const mpse_dims s = site_dims(h, j, env_unit);
  if (count) ++ctx->tda_stats[mpse_ctx::TD_ENV_UPDATES];
  return mpse_env_update(ctx, h.dtype, domain, &s, env, h.dtype, ket, bra, 1, h.W[j], h.wdt[j], out);
}

// out = heff(Lenv, W_j, Renv) C
int tda_heff(mpse_ctx* ctx, const mpse_tda& h, int j, const void* Lenv, int64_t l_unit, const void* Renv, int64_t r_unit,
             const void* C, void* out) {
  mpse_heff e{};
  e.nsite = 1;
  e.dims = site_dims(h, j, 0);
  e.L = Lenv, e.l_dtype = h.dtype;
  e.R = Renv, e.r_dtype = h.dtype;
  e.W0 = h.W[j], e.W1 = nullptr, e.w_dtype = h.wdt[j];
  e.l_unit = l_unit, e.r_unit = r_unit;
  ++ctx->tda_stats[mpse_ctx::TD_HEFF_APPLIES];
  return heff_apply(ctx, h.dtype, &e, C, out, nullptr, nullptr);
}

void tda_release(mpse_ctx* ctx, mpse_tda* h) {
  for (void* p : h->owned) mpse_free(ctx, p);
  delete h;
}

int tda_build(mpse_ctx* ctx, mpse_tda* h, const void* const* A, const int* a_dtype, const void* const* B,
              const int* b_dtype, const void* const* U, const int* u_dtype) {
  const int N = h->nsite;
  for (int j = 0; j < N; ++j) {
    const int64_t se = h->Dl(j) * h->d(j) * h->Dr(j);
    MPSE_TRY(tda_site(ctx, h, A[j], a_dtype[j], se, &h->A[j]));
    MPSE_TRY(tda_site(ctx, h, B[j], b_dtype[j], se, &h->B[j]));
    if (U[j]) MPSE_TRY(tda_site(ctx, h, U[j], u_dtype[j], h->Dl(j) * h->d(j) * h->n(j), &h->U[j]));
  }
  // constant environments: L_0 .. L_{N-1} from the A, R_N .. R_1 from the B
  const double one[2] = {1.0, 0.0};
  MPSE_TRY(tda_alloc(ctx, h, 1, &h->L[0]));
  MPSE_TRY(stage_h2d(ctx, h->L[0], one, h->es));
  MPSE_TRY(tda_alloc(ctx, h, 1, &h->R[N]));
  MPSE_TRY(stage_h2d(ctx, h->R[N], one, h->es));
  for (int j = 0; j + 1 < N; ++j) {
    MPSE_TRY(tda_alloc(ctx, h, h->Dr(j) * h->wr(j) * h->Dr(j), &h->L[j + 1]));
    MPSE_TRY(tda_env(ctx, *h, MPSE_DOMAIN_L, j, h->L[j], h->lunit[j], h->A[j], h->A[j], h->L[j + 1], false));
    if (h->Dr(j) >= TDA_UNIT_MIN_BOND)
      MPSE_TRY(mpse_env_unit_channel(ctx, h->dtype, h->L[j + 1], h->Dr(j), h->wr(j), TDA_UNIT_TOL, &h->lunit[j + 1]));
  }
  for (int j = N - 1; j >= 1; --j) {
    MPSE_TRY(tda_alloc(ctx, h, h->Dl(j) * h->wl(j) * h->Dl(j), &h->R[j]));
    MPSE_TRY(tda_env(ctx, *h, MPSE_DOMAIN_R, j, h->R[j + 1], h->runit[j + 1], h->B[j], h->B[j], h->R[j], false));
    if (h->Dl(j) >= TDA_UNIT_MIN_BOND)
      MPSE_TRY(mpse_env_unit_channel(ctx, h->dtype, h->R[j], h->Dl(j), h->wl(j), TDA_UNIT_TOL, &h->runit[j]));
  }
  // work buffers
  int64_t t_elems = 0, g_elems = 0, e_max = 1, s_max = 1;
  for (int j = 0; j < N; ++j) {
    const int64_t se = h->Dl(j) * h->d(j) * h->Dr(j), le = h->Dl(j) * h->wl(j) * h->Dl(j);
    h->toff[j] = t_elems;
    if (h->U[j]) t_elems += se;
    h->goff[j] = g_elems;
    if (j >= 1) g_elems += le;
    e_max = std::max(e_max, le);
    s_max = std::max(s_max, se);
  }
  MPSE_TRY(tda_alloc(ctx, h, t_elems, &h->Tb));
  MPSE_TRY(tda_alloc(ctx, h, g_elems, &h->Gb));
  MPSE_TRY(tda_alloc(ctx, h, e_max, &h->F0));
  MPSE_TRY(tda_alloc(ctx, h, e_max, &h->F1));
  MPSE_TRY(tda_alloc(ctx, h, e_max, &h->Etmp));
  MPSE_TRY(tda_alloc(ctx, h, s_max, &h->O));
  MPSE_TRY(tda_alloc(ctx, h, s_max, &h->Otmp));
  return MPSE_OK;
}

int tda_apply(mpse_ctx* ctx, mpse_tda* h, const void* x, void* y) {
  const int N = h->nsite, dt = h->dtype;
  const size_t es = h->es;
  ++ctx->tda_stats[mpse_ctx::TD_APPLIES];
  auto T = [&](int j) { return static_cast<char*>(h->Tb) + size_t(h->toff[j]) * es; };
  auto G = [&](int j) { return static_cast<char*>(h->Gb) + size_t(h->goff[j]) * es; };
  // T_j = U_j X_j
  for (int j = 0; j < N; ++j) {
    if (!h->U[j]) continue;
    const int64_t rows = h->Dl(j) * h->d(j), n = h->n(j), Dr = h->Dr(j);
    MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(rows, n), idx1(n, 1), idx1(n, Dr), idx1(Dr, 1), idx1(rows, Dr),
                       idx1(Dr, 1), 1, 0, 0, 0, h->U[j], static_cast<const char*>(x) + size_t(h->xoff[j]) * es, T(j)));
  }
  // G_j = updR(G_{j+1}; B_j, W_j, A_j) + updR(R_{j+1}; B_j, W_j, T_j), j = N-1 .. 1
  for (int j = N - 1; j >= 1; --j) {
    if (!h->has_g[j]) continue;
    const int64_t le = h->Dl(j) * h->wl(j) * h->Dl(j);
    bool have = false;
    if (h->has_g[j + 1]) {
      MPSE_TRY(tda_env(ctx, *h, MPSE_DOMAIN_R, j, G(j + 1), 0, h->A[j], h->B[j], G(j), true));
      have = true;
    }
    if (h->U[j]) {
      MPSE_TRY(tda_env(ctx, *h, MPSE_DOMAIN_R, j, h->R[j + 1], h->runit[j + 1], T(j), h->B[j], have ? h->Etmp : G(j), true));
      if (have) MPSE_TRY(mpse_axpy(ctx, dt, G(j), h->Etmp, le, 1.0, 0.0));
    }
  }
  // left to right: O_j and Y_j, then F_{j+1} = updL(F_j; A_j, W_j, B_j) + updL(L_j; A_j, W_j, T_j)
  void* F = h->F0;
  void* Fn = h->F1;
  for (int j = 0; j < N; ++j) {
    const int64_t rows = h->Dl(j) * h->d(j), n = h->n(j), Dr = h->Dr(j), se = rows * Dr;
    if (h->U[j]) {
      MPSE_TRY(tda_heff(ctx, *h, j, h->L[j], h->lunit[j], h->R[j + 1], h->runit[j + 1], T(j), h->O));
      if (h->has_f[j]) {
        MPSE_TRY(tda_heff(ctx, *h, j, F, 0, h->R[j + 1], h->runit[j + 1], h->B[j], h->Otmp));
        MPSE_TRY(mpse_axpy(ctx, dt, h->O, h->Otmp, se, 1.0, 0.0));
      }
      if (h->has_g[j + 1]) {
        MPSE_TRY(tda_heff(ctx, *h, j, h->L[j], h->lunit[j], G(j + 1), 0, h->A[j], h->Otmp));
        MPSE_TRY(mpse_axpy(ctx, dt, h->O, h->Otmp, se, 1.0, 0.0));
      }
      // Y_j[l, r] = sum_(a, s) conj(U_j[(a, s), l]) O_j[(a, s), r]
      MPSE_TRY(gemm_call(ctx, dt, dt, 1, 0, idx1(n, 1), idx1(rows, n), idx1(rows, Dr), idx1(Dr, 1), idx1(n, Dr),
                         idx1(Dr, 1), 1, 0, 0, 0, h->U[j], h->O, static_cast<char*>(y) + size_t(h->xoff[j]) * es));
    }
    if (j + 1 < N && h->has_f[j + 1]) {
      const int64_t re = Dr * h->wr(j) * Dr;
      bool have = false;
      if (h->has_f[j]) {
        MPSE_TRY(tda_env(ctx, *h, MPSE_DOMAIN_L, j, F, 0, h->B[j], h->A[j], Fn, true));
        have = true;
      }
      if (h->U[j]) {
        MPSE_TRY(tda_env(ctx, *h, MPSE_DOMAIN_L, j, h->L[j], h->lunit[j], T(j), h->A[j], have ? h->Etmp : Fn, true));
        if (have) MPSE_TRY(mpse_axpy(ctx, dt, Fn, h->Etmp, re, 1.0, 0.0));
      }
      std::swap(F, Fn);
    }
  }
  return MPSE_OK;
}

struct TdaOp {
  mpse_ctx* ctx;
  mpse_tda* h;
  static int apply(void* self, const void* x, void* y) {
    TdaOp* o = static_cast<TdaOp*>(self);
    return tda_apply(o->ctx, o->h, x, y);
  }
};

}  // namespace

extern "C" {

int mpse_tda_create(mpse_ctx* ctx, int nsite, const void* const* A, const int* a_dtype, const void* const* B,
                    const int* b_dtype, const void* const* U, const int* u_dtype, const void* const* W,
                    const int* w_dtype, const int64_t* dims, mpse_tda** out, int64_t* xsize_out, int* dtype_out) {
  if (!ctx || !out) return MPSE_ERR_ARG;
  *out = nullptr;
  if (!A || !a_dtype || !B || !b_dtype || !U || !u_dtype || !W || !w_dtype || !dims)
    return mpse_fail(ctx, MPSE_ERR_ARG, "tda_create: null argument");
  if (MPSE_RECORDING(ctx)) return mpse_fail(ctx, MPSE_ERR_ARG, "tda_create: refused while a deferred list is recorded");
  if (!tda_table_ok(nsite, dims))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "tda_create: the dims table (Dl, d, Dr, wl, wr, n) is not a chain");
  auto dt_ok = [](int dt) { return dt == MPSE_F64 || dt == MPSE_C128; };
  bool cplx = false;
  int64_t xsize = 0;
  for (int j = 0; j < nsite; ++j) {
    const int64_t n = dims[6 * j + 5];
    if (!A[j] || !B[j] || !W[j] || (n > 0) != (U[j] != nullptr))
      return mpse_fail(ctx, MPSE_ERR_ARG, "tda_create: site %d: null tensor, or U and n disagree", j);
    if (!dt_ok(a_dtype[j]) || !dt_ok(b_dtype[j]) || !dt_ok(w_dtype[j]) || (U[j] && !dt_ok(u_dtype[j])))
      return mpse_fail(ctx, MPSE_ERR_ARG, "tda_create: site %d: unknown dtype", j);
    cplx = cplx || a_dtype[j] == MPSE_C128 || b_dtype[j] == MPSE_C128 || w_dtype[j] == MPSE_C128 ||
           (U[j] && u_dtype[j] == MPSE_C128);
    xsize += n * dims[6 * j + 2];
  }
  if (xsize == 0) return mpse_fail(ctx, MPSE_ERR_SHAPE, "tda_create: the tangent space is empty");
  MPSE_BIND(ctx);
  mpse_tda* h = new (std::nothrow) mpse_tda;
  if (!h) return mpse_fail(ctx, MPSE_ERR_OOM, "tda_create: host allocation failed");
  const int N = nsite;
  h->nsite = N;
  h->dtype = cplx ? MPSE_C128 : MPSE_F64;
  h->es = dtype_size(h->dtype);
  h->dims.assign(dims, dims + 6 * (size_t)N);
  h->A.assign(N, nullptr), h->B.assign(N, nullptr), h->U.assign(N, nullptr);
  h->W.assign(W, W + N);
  h->wdt.assign(w_dtype, w_dtype + N);
  h->L.assign(N + 1, nullptr), h->R.assign(N + 1, nullptr);
  h->lunit.assign(N + 1, 0), h->runit.assign(N + 1, 0);
  h->xoff.assign(N, 0), h->toff.assign(N, 0), h->goff.assign(N + 1, 0);
  h->has_f.assign(N + 1, 0), h->has_g.assign(N + 2, 0);
  for (int j = 0; j < N; ++j) {
    h->xoff[j] = h->xsize;
    h->xsize += h->n(j) * h->Dr(j);
    h->has_f[j + 1] = h->has_f[j] || U[j] != nullptr;
  }
  for (int j = N - 1; j >= 0; --j) h->has_g[j] = h->has_g[j + 1] || U[j] != nullptr;
  const int st = tda_build(ctx, h, A, a_dtype, B, b_dtype, U, u_dtype);
  if (st != MPSE_OK) {
    tda_release(ctx, h);
    return st;
  }
  ++ctx->tda_stats[mpse_ctx::TD_HANDLES];
  *out = h;
  if (xsize_out) *xsize_out = h->xsize;
  if (dtype_out) *dtype_out = h->dtype;
  return MPSE_OK;
}

int mpse_tda_destroy(mpse_ctx* ctx, mpse_tda* h) {
  if (!ctx) return MPSE_ERR_ARG;
  if (h) tda_release(ctx, h);
  return MPSE_OK;
}

int mpse_tda_apply(mpse_ctx* ctx, mpse_tda* h, const void* x, void* y) {
  if (!ctx || !h || !x || !y) return MPSE_ERR_ARG;
  if (MPSE_RECORDING(ctx)) return mpse_fail(ctx, MPSE_ERR_ARG, "tda_apply: refused while a deferred list is recorded");
  const char *xb = static_cast<const char*>(x), *yb = static_cast<const char*>(y);
  const size_t bytes = size_t(h->xsize) * h->es;
  if (xb < yb + bytes && yb < xb + bytes) return mpse_fail(ctx, MPSE_ERR_ARG, "tda_apply: x and y overlap");
  MPSE_BIND(ctx);
  return tda_apply(ctx, h, x, y);
}

int mpse_tda_hdiag(mpse_ctx* ctx, mpse_tda* h, void* out_f64) {
  if (!ctx || !h || !out_f64) return MPSE_ERR_ARG;
  if (MPSE_RECORDING(ctx)) return mpse_fail(ctx, MPSE_ERR_ARG, "tda_hdiag: refused while a deferred list is recorded");
  MPSE_BIND(ctx);
  const int dt = h->dtype;
  const bool cplx = dt == MPSE_C128;
  const size_t es = h->es;
  const int64_t bound = tda_x_bytes();
  double* out = static_cast<double*>(out_f64);
  for (int j = 0; j < h->nsite; ++j) {
    if (!h->U[j]) continue;
    const int64_t Dl = h->Dl(j), d = h->d(j), Dr = h->Dr(j), wl = h->wl(j), wr = h->wr(j), n = h->n(j);
    const int64_t per_col = wl * Dl * d * (int64_t)es;
    const int64_t nl_max = std::min(n, std::max<int64_t>(1, bound / per_col));
    TmpBuf X(ctx), Q(ctx), V(ctx), Hd(ctx);
    MPSE_TRY(X.alloc(size_t(per_col) * nl_max));
    MPSE_TRY(Q.alloc(size_t(wl * d * d * nl_max) * es));
    MPSE_TRY(V.alloc(size_t(wr * nl_max) * es));
    if (cplx) MPSE_TRY(Hd.alloc(size_t(nl_max * Dr) * es));
    for (int64_t l0 = 0; l0 < n; l0 += nl_max) {
      const int64_t nl = std::min(nl_max, n - l0);
      // X[(b, c), (g, l)] = sum_a L[a, (b, c)] conj(U[a, (g, l0 + l)])
      MPSE_TRY(gemm_call(ctx, dt, dt, 0, 1, idx1(wl * Dl, 1), idx1(Dl, wl * Dl), idx1(Dl, d * n), idx2(d, nl, n, 1),
                         idx1(wl * Dl, d * nl), idx1(d * nl, 1), 1, 0, 0, 0, h->L[j],
                         static_cast<const char*>(h->U[j]) + size_t(l0) * es, X.p));
      const long long total = (long long)wl * d * d * nl;
      const int blocks = (int)std::min<long long>((total + 255) / 256, 4096);
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_tda_qdiag, dim3(blocks), dim3(256), X.as<const double>(),
                         static_cast<const double*>(h->U[j]), Q.as<double>(), (int)wl, (int)Dl, (int)d, (long long)n,
                         (long long)l0, (long long)nl);
      // V[e, l] = sum_(b, g, h) W[(b, g, h), e] Q[(b, g, h), l]
      MPSE_TRY(gemm_call(ctx, h->wdt[j], dt, 0, 0, idx1(wr, 1), idx1(wl * d * d, wr), idx1(wl * d * d, nl), idx1(nl, 1),
                         idx1(wr, nl), idx1(nl, 1), 1, 0, 0, 0, h->W[j], Q.p, V.p));
      // hdiag[l, r] = sum_e V[e, l] R[r, e, r]: the diagonal of R through the stride wr Dr + 1 of its column index
      void* dst = cplx ? Hd.p : static_cast<void*>(out + h->xoff[j] + l0 * Dr);
      MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(nl, 1), idx1(wr, nl), idx1(wr, Dr), idx1(Dr, wr * Dr + 1), idx1(nl, Dr),
                         idx1(Dr, 1), 1, 0, 0, 0, V.p, h->R[j + 1], dst));
      if (cplx) MPSE_TRY(mpse_real_part(ctx, out + h->xoff[j] + l0 * Dr, Hd.p, nl * Dr));
    }
    ++ctx->tda_stats[mpse_ctx::TD_QDIAG_SITES];
  }
  return MPSE_OK;
}

int mpse_tda_davidson(mpse_ctx* ctx, int dtype, mpse_tda* h, const void* hdiag_f64, int nroots, int nguess,
                      const void* guess, double tol, int max_cycle, int max_space, double lindep, double shift,
                      double* e_host, void* x_out, int* ncycle, int* nmatvec) {
  if (!ctx || !h || !hdiag_f64 || !guess || !e_host || !x_out) return MPSE_ERR_ARG;
  if (MPSE_RECORDING(ctx)) return mpse_fail(ctx, MPSE_ERR_ARG, "tda_davidson: refused while a deferred list is recorded");
  MPSE_BIND(ctx);
  if (dtype != h->dtype) return mpse_fail(ctx, MPSE_ERR_ARG, "tda_davidson: dtype is not the working dtype of the handle");
  if (nroots < 1 || nguess < 1 || nroots > 16)
    return mpse_fail(ctx, MPSE_ERR_ARG, "tda_davidson: 1 <= nroots <= 16 and at least one guess");
  ++ctx->tda_stats[mpse_ctx::TD_DAVIDSON];
  TdaOp op{ctx, h};
  return davidson_solve(ctx, dtype, h->xsize, DavOp{&TdaOp::apply, &op}, hdiag_f64, nullptr, nroots, nguess, guess, tol,
                        max_cycle, max_space, lindep, shift, e_host, x_out, ncycle, nmatvec);
}

int mpse_tda_stats(mpse_ctx* ctx, int64_t* counts, int n) { return stats_out(ctx, &mpse_ctx::tda_stats, counts, n); }

}  // extern "C"
