// Contraction plans for the hot path: each environment update / effective-Hamiltonian
// matvec is a short list of strided-GEMM steps (see mpse_gemm.hip) over named buffers.
// Pure host C++ with no HIP dependency, so the index algebra can be exercised on a CPU
// (tests/host_emu) with a naive loop executor; the product executes the same plans
// with the FP64-MFMA kernel (mpse_contract.hip).
//
// Contraction order is (env . site) . W . (other side) - the order opt_einsum's
// optimal path picks for D >> w, d (mps/hop_expr.py via mps/oe_contract_wrap.py:24-35) -
// i.e. two large GEMMs around a small batched contraction with the MPO site tensor.
// All index permutations are absorbed in operand strides; nothing is transposed in memory.
//
// One idiom: every planner declares its tensors as labelled views and states each product as one `contract` call
// (see "Labelled views" below, which also says how to add a product); the strides of every index map are derived from
// the declared layouts, never multiplied out by hand.  tests/test_plans_pin_host.py pins every plan.
#pragma once
#include <cassert>
#include <cstdint>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/mpsengine.h"

namespace mpse_plan {

enum Buf { B_L = 0, B_R, B_W0, B_W1, B_C, B_BRA, B_OUT, B_T1, B_T2, B_T3, B_W2, B_W3, B_OUT2, B_COUNT };
inline int w_buf(int layer) { return layer == 0 ? B_W0 : layer == 1 ? B_W1 : layer == 2 ? B_W2 : B_W3; }

enum Kind { K_GEMM = 0, K_COPY = 1, K_WMIX = 2, K_GGEMM = 3 };


// ---------------------------------------------------------------------------------------------------------------
// Folded one-site matvec: the MPO step shrinks to what the block structure of the MPO site needs, so most of the
// intermediates T1 = L . C and T2 = W T1 (Dl wl d Dr elements each) and the launches that only move them (MPO step as a
// batched product, unit-channel copy) disappear.
//   out[a,dd,l] = sum_f P_f[a,dd,k] R[l,f,k],   P_f = sum_b W[b,dd,:,f] (L[:,b,:] . C)
// An MPO site is a sparse matrix of d x d blocks W[b,:,:,f]; for sum-of-products Hamiltonians most non-zero blocks are
// the identity (channels that pass through the site).
//   * a channel b whose only block is an identity into a channel f that receives nothing else: the product
//     L[:,b,:] . C IS the plane P_f - written there directly;
//   * the other channels b write temporary planes T_b = L[:,b,:] . C, and one elementwise pass (K_WMIX) forms every
//     remaining plane P_f = sum_b W[b,:,:,f] T_b, with the centre tensor itself in the place of T_b for the unit channel
//     of L (d x d blocks out of LDS; an identity block is a plain add);
//   * a plane that is only the unit channel's identity block is the centre tensor itself (no copy), and the plane of
//     R's unit channel is `out`;
//   * all products L[:,b,:] . C of a site are ONE grouped launch (K_GGEMM: a group = the tile rows of one channel), and
//     out (+)= sum_{f != ru} P_f . R[:,f,:]^T is one more: one group whose K loop runs over the channels (segments).
// Every channel keeps its own product, so the quantum-number zero blocks of L[:,b,:] stay whole empty tiles.
constexpr int G_MAXGRP = 8, G_MAXSEG = 4, WM_MAXDST = 4, WM_MAXTERM = 4;
// Epilogue mix: the plane of R's unit channel (f = ru) is never an operand of the products with R - it is what they
// accumulate onto.  Where its blocks are bands of half-width <= EPI_MAXBAND, the first product with R forms it in its
// epilogue instead of reading it back from `out`: a term = one diagonal of one block,
//   mix[(a, x), k] = sum_terms W[b, x, x + delta, f] src[(a, x + delta), k],
// and a 64-row output tile holds whole runs of x (64 % d == 0), so the taps never leave the tile's rows of a.
constexpr int EPI_MAXTERM = 8, EPI_MAXBAND = 2;

struct WBlock {
  int b, f;
  bool ident;   // W[b, :, :, f] is the d x d identity
};
struct WSiteInfo {
  int64_t wl = 0, d = 0, wr = 0;
  std::vector<WBlock> blocks;   // the non-zero blocks, ordered by (f, b)
  std::vector<double> w;        // the site itself (wl, d, d, wr), row major
};
inline WSiteInfo analyse_mpo_site(const double* w, int64_t wl, int64_t d, int64_t wr) {
  WSiteInfo r;
  r.wl = wl, r.d = d, r.wr = wr;
  r.w.assign(w, w + wl * d * d * wr);
  for (int64_t f = 0; f < wr; ++f)
    for (int64_t b = 0; b < wl; ++b) {
      bool any = false, ident = true;
      for (int64_t x = 0; x < d; ++x)
        for (int64_t e = 0; e < d; ++e) {
          const double v = w[((b * d + x) * d + e) * wr + f];
          if (v != 0.0) any = true;
          if (v != (x == e ? 1.0 : 0.0)) ident = false;
        }
      if (any) r.blocks.push_back(WBlock{(int)b, (int)f, ident});
    }
  return r;
}

// K_WMIX: dst[a, dd, k] = sum_terms sum_e W[b, dd, e, f] src[a, e, k]; element (a, x, k) of a tensor at off + a s_a + x s_d + k
constexpr int WM_CHUNK = 4, WM_MAXCHUNKS = 8;     // a thread forms WM_CHUNK consecutive dd; d <= 32
struct WMixTerm {
  int b = 0, f = 0;
  bool ident = false;
  int src = 0;
  int64_t src_off = 0, s_a = 0, s_d = 0;
  unsigned char e_lo[WM_MAXCHUNKS] = {0}, e_hi[WM_MAXCHUNKS] = {0};   // columns e the rows of a chunk need: [e_lo, e_hi)
};
struct WMixDst {
  int dst = 0;
  int64_t dst_off = 0, s_a = 0, s_d = 0;
  int nterm = 0;
  WMixTerm term[WM_MAXTERM];
};
enum BMaskKind { BM_NONE = 0, BM_SCAN = 1, BM_CENTRE = 2 };
struct GSegPlan {
  int abuf = 0;
  int64_t a_off = 0;
  int bbuf = 0;
  int64_t b_off = 0;
  int64_t am_row0 = -1;   // >= 0: occupancy of A from the step's scan_a: first tile row of this segment there
  int bm_kind = BM_NONE;  // BM_SCAN: from scan_b, K tiles from bm_kt0 on; BM_CENTRE: B is the centre tensor (structural
  int64_t bm_kt0 = 0;     // mask of the solve)
};
struct EpiTerm {
  int src = 0;            // tensor (rows (a, x), columns k) the diagonal is applied to: the centre, a temporary or `out`
  int64_t src_off = 0;
  int b = 0, f = 0;       // block W[b, :, :, f] of the site in wbuf ...
  int delta = 0;          // ... and its diagonal e = x + delta
};
struct GGroupPlan {
  int nseg = 0;
  GSegPlan seg[G_MAXSEG];
  int cbuf = 0;
  int64_t c_off = 0;
  double beta = 0.0;
  // epilogue mix (nmix > 0; beta == 1): the beta term is the sum of these terms instead of C itself
  int nmix = 0;
  EpiTerm mix[EPI_MAXTERM];
  int wbuf = B_W0;
  int64_t mix_d = 0, mix_wr = 0, mix_ld = 0;   // site (., d, d, wr); row stride of the sources
  // split2 (single-group steps): two workgroups per output tile, each over half of the tile's occupied K tiles; the
  // first half (+ beta C) is stored to C, the second to B_OUT2, laid out like C: the caller of the plan adds the two
  bool split2 = false;
};
struct ScanDesc {   // an operand whose tile occupancy is scanned once for all segments that read parts of it
  bool on = false;
  int buf = 0, dt = MPSE_F64;
  int64_t off = 0;
  mpse_index r{}, k{};
};

struct Step {
  int a, b, c;                 // buffer ids
  int64_t a_off, b_off, c_off; // element offsets into the buffers
  int dta, dtb;
  int conja, conjb;
  mpse_index ma, ka, kb, nb, mc, nc;
  int64_t batch, sba, sbb, sbc;
  int kind = K_GEMM;           // K_COPY: C(i,j) = A(i,j) with A indexed by (ma, ka), C by (mc, nc); b unused
  double beta = 0.0;           // K_GEMM: C = A.B + beta C
  int skip_zero = 0;           // K_GEMM: scan both operands for all-zero tiles and skip them (block-sparse sweeps)
  // K_GEMM steps written by push_w also carry the sizes of the MPO step they are (Da = batch of bond states, N =
  // trailing block): the executor runs small ones (d = 2 sites) through an elementwise kernel instead of MFMA tiles
  bool is_wstep = false;
  int64_t w_Da = 0, w_wl = 0, w_d = 0, w_wr = 0, w_N = 0;
  // K_WMIX / K_GGEMM (folded one-site matvec, above)
  std::vector<WMixDst> mix;    // K_WMIX: b = MPO site; tensors (wp_Da, wp_d, wp_Dk)
  int64_t wp_Da = 0, wp_d = 0, wp_Dk = 0, wp_wr = 0;
  std::vector<GGroupPlan> groups;   // K_GGEMM: ma .. nc describe ONE segment's product (rows of one group, K of one segment)
  ScanDesc scan_a, scan_b;
  int cin = -1;                // K_GEMM with beta != 0: buffer the beta term is read from (-1: C itself) ...
  int64_t cin_off = 0;         // ... at this element offset, through these index maps
  mpse_index mcin{}, ncin{};
  // Marks (set by `marked`, below, for every plan a planner returns): what the step is within its plan, so that the
  // executors read it instead of inferring it from the step list
  bool elementwise_w = false;  // a small-site MPO step: runs as the elementwise kernel (k_wsmall), not as MFMA tiles
  int slices_to = -1;          // a product that may leave its K slices to that elementwise step (index; -1: none) ...
  int64_t slice_b_lo = 0, slice_b_hi = 0;   // ... on that step: the channels of its input the slices form, [b_lo, b_hi),
  int64_t slice_elems = 0;                  // and the elements of one slice (mc.ext * nc.ext of the product)
  bool completes = false;      // the step finishes the caller's result: it may carry MatvecReq::dot / out_mask
};

struct Plan {
  std::vector<Step> steps;
  int64_t tmp_elems[3] = {0, 0, 0};  // T1, T2, T3 sizes (elements of the working dtype)
  bool two_results = false;          // the result is B_OUT + B_OUT2 (GGroupPlan::split2)
  const char* error = nullptr;
};

inline mpse_index i1(int64_t ext, int64_t stride) { return mpse_index{ext, ext > 0 ? ext : 1, 0, stride}; }
inline mpse_index i2(int64_t hi, int64_t lo, int64_t s_hi, int64_t s_lo) {
  return mpse_index{hi * lo, lo > 0 ? lo : 1, s_hi, s_lo};
}

// ---------------------------------------------------------------------------------------------------------------
// Labelled views: the one idiom every planner below is written in.  A tensor is a View - buffer, dtype, element offset
// and per dimension a one-letter label, an extent and a stride; a product is ONE `contract` call that names the labels
// of its row, contracted and column index (outer -> inner) and derives every index map from the views.  No planner
// multiplies out a stride: i1 / i2 are called by labels_index alone.  Nothing here allocates (heff_apply plans at every
// Krylov iteration); the only heap traffic of a plan is p.steps.push_back.
//   * a view is built from its row-major extents; `sub` narrows a dimension (a channel range around a unit channel, one
//     plane of a stack of planes), `as` renames the dimensions by position (K[c, n] read as rows a of X[a, b, n]);
//   * an index is the listed labels with extent-1 labels dropped and contiguous neighbours merged; at most two levels
//     per operand - what is left over goes to `batch` (one level) or `loops` (one step per value);
//   * `copy` is the strided copy (K_COPY) in the same terms.
// To add a product: declare the views of its operands with the layouts they have in memory, give them shared labels,
// call contract(p, A, B, C, m, k, n); set what is policy (skip_zero, beta, cin, is_wstep) on the step it returns; add
// the planner's cases to tests/host_emu/plan_dump.cpp and its numbers to a host emulator test.
constexpr int VIEW_MAXDIM = 8;
struct View {
  int buf = 0, dt = MPSE_F64;
  int64_t off = 0;
  int n = 0;
  char lab[VIEW_MAXDIM] = {0};
  int64_t ex[VIEW_MAXDIM] = {0}, st[VIEW_MAXDIM] = {0};
  View() {}
  View(int b, int d, std::initializer_list<std::pair<char, int64_t>> l) : buf(b), dt(d) {   // memory order, row major
    assert(l.size() <= size_t(VIEW_MAXDIM));
    for (auto& q : l) lab[n] = q.first, ex[n] = q.second, ++n;
    int64_t s = 1;
    for (int i = n; i-- > 0;) st[i] = s, s *= ex[i];
  }
  int find(char c) const {
    for (int i = 0; i < n; ++i)
      if (lab[i] == c) return i;
    return -1;
  }
  int64_t ext(char c) const {      // -1 if the label is absent
    const int i = find(c);
    return i < 0 ? -1 : ex[i];
  }
  int64_t stride(char c) const {   // 0 if the label is absent
    const int i = find(c);
    return i < 0 ? 0 : st[i];
  }
  View sub(char c, int64_t first, int64_t count) const {   // values [first, first + count) of one dimension
    View v = *this;
    const int i = find(c);
    assert(i >= 0);
    v.off += first * st[i], v.ex[i] = count;
    return v;
  }
  View as(const char* labels) const {   // the same memory, dimensions renamed by position
    View v = *this;
    for (int i = 0; i < n && labels[i]; ++i) v.lab[i] = labels[i];
    return v;
  }
};

inline bool labels_index(const View& v, const char* labels, mpse_index* out) {
  int64_t le[2], ls[2], total = 1;   // (ext, stride), outer -> inner, merged
  int nl = 0;
  for (const char* c = labels; *c; ++c) {
    const int i = v.find(*c);
    if (i < 0) return false;
    const int64_t e = v.ex[i], st = v.st[i];
    total *= e;
    if (e == 1) continue;
    if (nl > 0 && ls[nl - 1] == e * st) {
      le[nl - 1] *= e, ls[nl - 1] = st;
    } else {
      if (nl == 2) return false;
      le[nl] = e, ls[nl] = st, ++nl;
    }
  }
  *out = nl == 0 ? i1(total, 1) : nl == 1 ? i1(le[0], ls[0]) : i2(le[0], le[1], ls[0], ls[1]);
  return true;
}

// the six index maps of C[m, n] = sum_k A[m, k] B[k, n]
inline bool product_maps(Step& s, const View& A, const View& B, const View& C, const char* m, const char* k, const char* n) {
  return labels_index(A, m, &s.ma) && labels_index(A, k, &s.ka) && labels_index(B, k, &s.kb) && labels_index(B, n, &s.nb) &&
         labels_index(C, m, &s.mc) && labels_index(C, n, &s.nc);
}

// C[batch][m, n] = sum_k A[batch][m, k] B[batch][k, n] for every value of the `loops` labels.  Returns the last step it
// pushed (valid until the next push), nullptr when it pushed none.
inline Step* contract(Plan& p, const View& A, const View& B, const View& C, const char* m, const char* k, const char* n,
                      const char* batch = "", const char* loops = "", int conja = 0) {
  if (p.error) return nullptr;
  Step s{};
  if (!product_maps(s, A, B, C, m, k, n)) {
    p.error = "plan: an index of a stacked-MPO contraction needs more than two stride levels";
    return nullptr;
  }
  s.a = A.buf, s.b = B.buf, s.c = C.buf, s.dta = A.dt, s.dtb = B.dt, s.conja = conja, s.batch = 1;
  if (batch[0]) {
    // a batch label may be absent from A or B (stride 0) but must be a single level where present
    auto one = [&](const View& v, int64_t* st) {
      int present = 0, all = 0;
      for (const char* c = batch; *c; ++c) ++all, present += v.find(*c) >= 0 ? 1 : 0;
      if (present == 0) {
        *st = 0;
        return true;
      }
      mpse_index ix;
      if (present != all || !labels_index(v, batch, &ix) || (ix.lo_ext < ix.ext && ix.ext > 1)) return false;
      *st = ix.s_lo;
      return true;
    };
    if (!one(A, &s.sba) || !one(B, &s.sbb) || !one(C, &s.sbc)) {
      p.error = "plan: batch labels of a stacked-MPO contraction do not form one level";
      return nullptr;
    }
    for (const char* c = batch; *c; ++c) s.batch *= C.ext(*c);
  }
  int64_t ext[VIEW_MAXDIM], cnt[VIEW_MAXDIM] = {0}, nloop = 1;
  int nl = 0;
  for (const char* c = loops; *c && nl < VIEW_MAXDIM; ++c, ++nl) {
    ext[nl] = C.ext(*c) >= 0 ? C.ext(*c) : (A.ext(*c) >= 0 ? A.ext(*c) : B.ext(*c));
    nloop *= ext[nl];
  }
  for (int64_t it = 0; it < nloop; ++it) {
    s.a_off = A.off, s.b_off = B.off, s.c_off = C.off;
    for (int l = 0; l < nl; ++l) {
      s.a_off += cnt[l] * A.stride(loops[l]);
      s.b_off += cnt[l] * B.stride(loops[l]);
      s.c_off += cnt[l] * C.stride(loops[l]);
    }
    p.steps.push_back(s);
    for (int l = nl; l-- > 0;) {
      if (++cnt[l] < ext[l]) break;
      cnt[l] = 0;
    }
  }
  return nloop > 0 ? &p.steps.back() : nullptr;
}

// dst[rows, cols] = src[rows, cols] (K_COPY), both sides through the same labels
inline void copy(Plan& p, const View& src, const View& dst, const char* rows, const char* cols) {
  mpse_index mi, ni, mo, no;
  if (!labels_index(src, rows, &mi) || !labels_index(src, cols, &ni) || !labels_index(dst, rows, &mo) ||
      !labels_index(dst, cols, &no)) {
    p.error = "plan: an index of a copy needs more than two stride levels";
    return;
  }
  Step s{src.buf, src.buf, dst.buf, src.off, 0, dst.off, src.dt, src.dt, 0, 0, mi, ni, ni, no, mo, no, 1, 0, 0, 0};
  s.kind = K_COPY;
  p.steps.push_back(s);
}

// Skipping a unit channel trades a (m x k x n) slice of a GEMM for a strided copy kernel: below ~1e8 multiply-adds
// the slice costs less than the extra launch, so small centres keep the plain GEMM.
inline int64_t& unit_threshold() {   // multiply-adds; a test hook lowers it so that small cases take the copy path
  static int64_t v = int64_t(1) << 27;
  return v;
}
inline bool unit_pays(int64_t m, int64_t k, int64_t n) { return m * k * n >= unit_threshold(); }
inline bool& beta_source_flag() {
  static bool v = true;     // (test hook: the emulator also runs the plans with the copy instead)
  return v;
}
inline bool beta_source_on() { return beta_source_flag(); }
// Scanning the operands of a GEMM for structurally zero tiles costs two small launches and one pass over the
// operands; worth it from ~3e7 multiply-adds on.
// The result says which operands to scan: bit 0 = A, bit 1 = B.
inline int skip_pays(int64_t m, int64_t k, int64_t n, int which = 3) {
  return m * k * n >= (int64_t(1) << 28) ? which : 0;
}

// The channels of an environment around its unit channel u (-1: none): at most two ranges [lo, hi)
struct ChannelRanges {
  int64_t lo[2], hi[2];
  ChannelRanges(int64_t u, int64_t w) : lo{0, u + 1}, hi{u >= 0 ? u : w, u >= 0 ? w : 0} {}
};

// X[a,b,n] = sum_c E[a,b,c] K[c,n] for an environment E (rows, w, cols) and a matrix K (cols, N).
// `unit` (1-based, 0 = none) names an MPO-bond channel b along which E[:, b, :] is the identity matrix (what a
// canonical MPS gives for the channel in which no operator has acted yet): that slice of X is a copy of K and
// the GEMM runs over the remaining channels only.
// Layout of X: (rows, w, N) when b_outer == false; (w, rows, N) when b_outer == true.  With the channel as the
// outer index every 64-row tile of the GEMM belongs to one MPO channel and one run of bond states, so the
// quantum-number zero blocks of E show up as whole empty tiles (structural-zero skipping, mpse_gemm.hip).
inline void push_env_times(Plan& p, int ebuf, int e_dtype, int kbuf, int k_dtype, int xbuf, int64_t rows, int64_t w,
                           int64_t cols, int64_t N, int64_t unit, bool b_outer) {
  const int64_t u = (unit >= 1 && unit <= w && rows == cols && unit_pays(rows, cols, N)) ? unit - 1 : -1;
  const View E(ebuf, e_dtype, {{'a', rows}, {'b', w}, {'c', cols}}), K(kbuf, k_dtype, {{'c', cols}, {'n', N}});
  const View X = b_outer ? View(xbuf, k_dtype, {{'b', w}, {'a', rows}, {'n', N}})
                         : View(xbuf, k_dtype, {{'a', rows}, {'b', w}, {'n', N}});
  if (u >= 0) copy(p, K.as("an"), X.sub('b', u, 1), "a", "n");
  const ChannelRanges cr(u, w);
  for (int r = 0; r < 2; ++r) {
    const int64_t b0 = cr.lo[r], nb = cr.hi[r] - cr.lo[r];
    if (nb <= 0) continue;
    if (Step* s = contract(p, E.sub('b', b0, nb), K, X.sub('b', b0, nb), b_outer ? "ba" : "ab", "c", "n"))
      s->skip_zero = skip_pays(rows * nb, cols, N);
  }
}

// out[(m,g),l] = sum_{f,k} T[m,f,g,k] E[l,f,k] for T (M1, w, anc, Dk) and an environment E (Dout, w, Dk).
// `unit` as above: E[:, f, :] = identity contributes T[m,f,g,l] itself (needs Dout == Dk).
inline void push_times_env(Plan& p, int tbuf, int t_dtype, int ebuf, int e_dtype, int obuf, int64_t M1, int64_t anc,
                           int64_t w, int64_t Dk, int64_t Dout, int64_t unit) {
  const int64_t u = (unit >= 1 && unit <= w && Dout == Dk && unit_pays(M1 * anc, Dk, Dout)) ? unit - 1 : -1;
  const View T(tbuf, t_dtype, {{'m', M1}, {'f', w}, {'g', anc}, {'k', Dk}}), E(ebuf, e_dtype, {{'l', Dout}, {'f', w}, {'k', Dk}});
  const View O(obuf, t_dtype, {{'m', M1}, {'g', anc}, {'l', Dout}});
  double beta = 0.0;
  // The unit channel contributes T[m, u, g, l] itself: the first product reads it as its beta term straight from T
  // (no copy into `out` first), unless there is no product at all (w == 1) or MPSE_BETA_SOURCE=0.
  const bool direct = u >= 0 && w > 1 && beta_source_on();
  const View Tu = u >= 0 ? T.sub('f', u, 1).as("mfgl") : T;
  if (u >= 0 && !direct) {
    copy(p, Tu, O, "mg", "l");
    beta = 1.0;
  }
  bool first = true;
  const ChannelRanges cr(u, w);
  for (int r = 0; r < 2; ++r) {
    const int64_t f0 = cr.lo[r], nf = cr.hi[r] - cr.lo[r];
    if (nf <= 0) continue;
    Step* s = contract(p, T.sub('f', f0, nf), E.sub('f', f0, nf), O, "mg", "fk", "l");
    if (!s) return;
    if (direct && first) {
      s->cin = Tu.buf, s->cin_off = Tu.off;
      labels_index(Tu, "mg", &s->mcin), labels_index(Tu, "l", &s->ncin);
      beta = 1.0;
    }
    first = false;
    s->beta = beta;
    s->skip_zero = skip_pays(M1 * anc, nf * Dk, Dout, 2);   // A = the big intermediate: environment side only
    beta = 1.0;
  }
}

// T_out[a, d, f, n] = sum_{b,e} W[b,d,e,f] T_in[b, a, e, n]   (W (wl,d,d,wr) row-major; batch over a;
// T_in in the channel-outer layout written by push_env_times(b_outer = true))
inline void push_w(Plan& p, int wbuf, int w_dtype, int tin, int tout, int t_dtype, int64_t na, int64_t wl, int64_t d,
                   int64_t wr, int64_t N) {
  const View W(wbuf, w_dtype, {{'b', wl}, {'y', d}, {'e', d}, {'f', wr}});
  const View Tin(tin, t_dtype, {{'b', wl}, {'a', na}, {'e', d}, {'n', N}}), Tout(tout, t_dtype, {{'a', na}, {'y', d}, {'f', wr}, {'n', N}});
  if (Step* s = contract(p, W, Tin, Tout, "yf", "be", "n", "a")) {
    s->is_wstep = true;
    s->w_Da = na, s->w_wl = wl, s->w_d = d, s->w_wr = wr, s->w_N = N;
  }
}


// The marks of a plan (Step::elementwise_w .. completes); every planner returns its plan through this.
//   * elementwise: the MPO step of a small real site (wl d <= 16 inputs, d wr <= 16 outputs) over whole tensors;
//   * hand-off: the first elementwise step that reads T1 adds the K slices of the ONE product that forms its input
//     channels itself (no reduction launch between them), when that product's rows are (channel | bra bond) over whole
//     channels of T1, compactly stored.  Whether the product really leaves slices is decided when it runs;
//   * completes: the last step, when it is a plain product, or a grouped one of a single group, into the whole of `out`.
inline Plan marked(Plan p) {
  Step *prod = nullptr, *cons = nullptr;
  int n_t1 = 0;
  for (Step& s : p.steps) {
    s.elementwise_w = s.kind == K_GEMM && s.is_wstep && s.dta == MPSE_F64 && s.a_off == 0 && s.b_off == 0 &&
                      s.c_off == 0 && s.beta == 0.0 && s.w_wl * s.w_d <= 16 && s.w_d * s.w_wr <= 16;
    s.slices_to = -1, s.slice_b_lo = s.slice_b_hi = s.slice_elems = 0, s.completes = false;
    if (s.elementwise_w && s.b == B_T1 && !cons) cons = &s;
    if (!cons && s.kind == K_GEMM && !s.is_wstep && s.c == B_T1) ++n_t1, prod = &s;
  }
  if (cons && n_t1 == 1 && prod->batch == 1 && prod->beta == 0.0 && prod->cin < 0 && cons->w_Da > 0 &&
      prod->nc.ext == cons->w_d * cons->w_N && prod->mc.ext % cons->w_Da == 0 &&
      prod->c_off % (cons->w_Da * cons->w_d * cons->w_N) == 0) {
    prod->slices_to = int(cons - p.steps.data());
    cons->slice_b_lo = prod->c_off / (cons->w_Da * cons->w_d * cons->w_N);
    cons->slice_b_hi = cons->slice_b_lo + prod->mc.ext / cons->w_Da;
    cons->slice_elems = prod->mc.ext * prod->nc.ext;
  }
  if (!p.steps.empty()) {
    Step& s = p.steps.back();
    s.completes = s.kind == K_GEMM ? s.c == B_OUT && s.c_off == 0 && s.batch == 1
                                   : s.kind == K_GGEMM && s.groups.size() == 1 && s.groups[0].cbuf == B_OUT &&
                                         s.groups[0].c_off == 0;
  }
  return p;
}

// The operands of a plan by buffer id, one helper per operator family (bufs: B_COUNT entries, zeroed by the caller)
inline void bind_heff(const void** bufs, const mpse_heff& h, const void* C, void* out) {
  bufs[B_L] = h.L, bufs[B_R] = h.R, bufs[B_W0] = h.W0, bufs[B_W1] = h.W1, bufs[B_C] = C, bufs[B_OUT] = out;
}
inline void bind_heff_ft(const void** bufs, const mpse_heff_ft& h, const void* C, void* out) {
  bufs[B_L] = h.L, bufs[B_R] = h.R, bufs[B_W0] = h.W1, bufs[B_W1] = h.W2, bufs[B_C] = C, bufs[B_OUT] = out;
}
inline void bind_env(const void** bufs, const void* env, const void* ket, const void* bra, void* out, int n_mpo,
                     const void* const* W) {
  bufs[B_L] = env, bufs[B_C] = ket, bufs[B_BRA] = bra, bufs[B_OUT] = out;
  for (int i = 0; i < n_mpo; ++i) bufs[w_buf(i)] = W[i];
}

// Effective Hamiltonian matvec, mps/hop_expr.py:57-115.  The bra-side bonds (rows of L / R, bonds of `out`) may
// differ from the ket-side bonds (columns of L / R, bonds of C): that is the projection of H C onto another
// state's bond spaces used by the variational compression (mps/mp.py:513-650); the Krylov / Davidson drivers
// require them equal.
inline Plan plan_heff1_fold(int dtype, const mpse_heff& h, const WSiteInfo& wi, bool two_results, bool mix_epilogue);

// `wi`: block structure of the MPO site where the caller knows it (mpse_mpo_site_hint): large one-site centres then
// take the folded plan.  `two_results`: the caller accepts the result as the sum of B_OUT and B_OUT2 (Plan::two_results
// says whether the plan made use of it).  `mix_epilogue`: the folded plan may form the plane of R's unit channel in the
// epilogue of the first product with R (EpiTerm); the caller's executor must understand GGroupPlan::nmix.
inline Plan plan_heff(int dtype, const mpse_heff& h, const WSiteInfo* wi = nullptr, bool two_results = false,
                      bool mix_epilogue = false) {
  Plan p;
  const mpse_dims& s = h.dims;
  const int64_t Dl = s.Dl_ket, Dr = s.Dr_ket, wl = s.wl, wr = s.wr;
  const int64_t Dlb = s.Dl_bra > 0 ? s.Dl_bra : Dl, Drb = s.Dr_bra > 0 ? s.Dr_bra : Dr;
  const int64_t anc = s.danc > 0 ? s.danc : 1;
  if (h.nsite == 0) {
    // abc,lbk,ck->al (hop_expr.py:63-67): T[a,b,k] = L[(a,b),c] S[c,k] ; out[a,l] = T[a,(b,k)] R[l,(b,k)]
    if (wl != wr) {
      p.error = "heff(0-site): wl != wr";
      return p;
    }
    p.tmp_elems[0] = Dlb * wl * Dr;
    push_env_times(p, B_L, h.l_dtype, B_C, dtype, B_T1, Dlb, wl, Dl, Dr, h.l_unit, false);
    push_times_env(p, B_T1, dtype, B_R, h.r_dtype, B_OUT, Dlb, 1, wr, Dr, Drb, h.r_unit);
    return marked(std::move(p));
  }
  if (h.nsite == 1) {
    if (wi) {
      Plan f = plan_heff1_fold(dtype, h, *wi, two_results, mix_epilogue);
      if (!f.error) return f;
    }
    // abc,bdef,lfk,cek->adl (hop_expr.py:75-79); ancilla cegk->adgl (87-91)
    const int64_t d = s.d0, N = d * anc * Dr, Nb = anc * Dr;
    p.tmp_elems[0] = Dlb * wl * N;
    p.tmp_elems[1] = Dlb * d * wr * Nb;
    // T1[a,b,(e,g,k)] = sum_c L[(a,b),c] C[c,(e,g,k)]
    push_env_times(p, B_L, h.l_dtype, B_C, dtype, B_T1, Dlb, wl, Dl, N, h.l_unit, true);
    // T2[a,d,f,(g,k)] = sum_{b,e} W[b,d,e,f] T1[a,b,e,(g,k)]
    push_w(p, B_W0, h.w_dtype, B_T1, B_T2, dtype, Dlb, wl, d, wr, Nb);
    // out[(a,d,g),l] = sum_{f,k} T2[a,d,f,g,k] R[l,f,k]
    push_times_env(p, B_T2, dtype, B_R, h.r_dtype, B_OUT, Dlb * d, anc, wr, Dr, Drb, h.r_unit);
    return marked(std::move(p));
  }
  if (h.nsite == 2) {
    // abc,bdef,fghj,ljk,cehk->adgl (hop_expr.py:99-103); ancilla cemhnk->admgnl (111-115): the two ancilla legs m, n
    // have the sizes of their own sites (a0, a1)
    const int64_t d0 = s.d0, d1 = s.d1, wm = s.wm;
    const int64_t a0 = anc, a1 = s.danc1 > 0 ? s.danc1 : anc;
    const int64_t n2 = a1 * Dr;             // (n,k): trailing block after h
    const int64_t n1 = a0 * d1 * n2;        // (m,h,n,k): trailing block after e
    const int64_t N = d0 * n1;
    p.tmp_elems[0] = Dlb * wl * N;
    p.tmp_elems[1] = Dlb * d0 * wm * n1;
    p.tmp_elems[2] = Dlb * d0 * a0 * d1 * wr * n2;
    // T1[a,b,(e,m,h,n,k)]
    push_env_times(p, B_L, h.l_dtype, B_C, dtype, B_T1, Dlb, wl, Dl, N, h.l_unit, true);
    // T2[a,d,f,(m,h,n,k)]
    push_w(p, B_W0, h.w_dtype, B_T1, B_T2, dtype, Dlb, wl, d0, wm, n1);
    // T3[A,m,g,j,N] = sum_{f,h} W1[f,g,h,j] T2[A,f,m,h,N]   batch A = (a,d), N = (n,k); one step per m
    const View W1(B_W1, h.w_dtype, {{'f', wm}, {'g', d1}, {'h', d1}, {'j', wr}});
    const View T2(B_T2, dtype, {{'A', Dlb * d0}, {'f', wm}, {'m', a0}, {'h', d1}, {'N', n2}});
    const View T3(B_T3, dtype, {{'A', Dlb * d0}, {'m', a0}, {'g', d1}, {'j', wr}, {'N', n2}});
    contract(p, W1, T2, T3, "gj", "fh", "N", "A", "m");
    // out[(a,d,m,g,n),l] = sum_{j,k} T3[a,d,m,g,j,n,k] R[l,j,k]
    push_times_env(p, B_T3, dtype, B_R, h.r_dtype, B_OUT, Dlb * d0 * a0 * d1, a1, wr, Dr, Drb, h.r_unit);
    return marked(std::move(p));
  }
  p.error = "heff: nsite must be 0, 1 or 2";
  return p;
}


// smallest Dl * d * Dr * Dl (multiply-adds of one channel's product) from which the folded plan is used
inline int64_t& fold_min() {
  static int64_t v = [] {
    const char* e = getenv("MPSE_WFOLD");      // MPSE_WFOLD=0: the three-step chain everywhere
    return (e && e[0] == '0') ? (int64_t(1) << 62) : (int64_t(1) << 28);
  }();
  return v;
}

inline int64_t& fold_cus() {    // compute units of the device (mpse_ctx_create sets it): products with at most one
  static int64_t v = 256;       // 64 x 64 tile per unit are halved along K (GGroupPlan::split2)
  return v;
}
inline bool& fold_split2() {
  static bool v = [] {
    const char* e = getenv("MPSE_SPLIT2");     // MPSE_SPLIT2=0: one workgroup per tile
    return !(e && e[0] == '0');
  }();
  return v;
}
inline bool& fold_epi() {
  static bool v = [] {
    const char* e = getenv("MPSE_WFOLD_EPI");  // MPSE_WFOLD_EPI=0: every mixed plane through the elementwise pass
    return !(e && e[0] == '0');
  }();
  return v;
}
inline int64_t& fold_split2_min_kt() {   // fewest K tiles of a product worth halving (test hook)
  static int64_t v = 8;
  return v;
}
inline int64_t& fold_align() {   // bra-bond multiple the device needs (a 64-row tile = one channel); a test hook lowers it
  static int64_t v = 64;
  return v;
}

// One term of the elementwise pass: block `k` of the site applied to src[a, x, k], with the columns e that the rows of
// each chunk of WM_CHUNK rows need
inline WMixTerm wmix_term(const WSiteInfo& wi, const WBlock& k, const View& src) {
  WMixTerm t;
  t.b = k.b, t.f = k.f, t.ident = k.ident;
  t.src = src.buf, t.src_off = src.off, t.s_a = src.stride('a'), t.s_d = src.stride('x');
  const int64_t d = wi.d, nchunk = (d + WM_CHUNK - 1) / WM_CHUNK;
  for (int64_t c = 0; c < nchunk; ++c) {
    int64_t lo = d, hi = 0;
    for (int64_t x = c * WM_CHUNK; x < std::min<int64_t>(d, (c + 1) * WM_CHUNK); ++x)
      for (int64_t e = 0; e < d; ++e)
        if (wi.w[((k.b * d + x) * d + e) * wi.wr + k.f] != 0.0) lo = std::min(lo, e), hi = std::max(hi, e + 1);
    t.e_lo[c] = (unsigned char)(hi > lo ? lo : 0), t.e_hi[c] = (unsigned char)(hi > lo ? hi : 0);
  }
  return t;
}
inline bool wmix_fits_lds(int64_t nslot, int64_t d) { return nslot * d * d <= 8192; }   // 64 KB of LDS for the dense blocks

// Folded one-site matvec (see above), analysis: what becomes of every channel of the site - no step yet.  `error` is
// set when the site does not qualify (the caller then takes the three-step chain of plan_heff).
struct FoldAnalysis {
  const char* error = nullptr;
  const WSiteInfo* wi = nullptr;
  int64_t lu = -1, ru = -1;                                   // unit channels of L / R (0-based, -1: none)
  std::vector<std::vector<const WBlock*>> by_f, by_b;        // the blocks per channel of R / of L
  // where the product of channel b goes: straight into the plane of its channel f (direct_f), or into a temporary
  // (tmp_of, ntmp of them); planes: storage for every channel f != ru that is not the centre tensor itself (plane_of,
  // nplanes of them; alias: it is); mixed: the planes the elementwise pass forms, in its order
  std::vector<int64_t> direct_f, tmp_of, plane_of, mixed;
  std::vector<char> alias, present;
  int64_t ntmp = 0, nplanes = 0;
  // epilogue mix: the plane f = ru as diagonals (block, delta) applied by the first product with R; epi_direct_b: the
  // channel whose product is written straight into `out` and read back as a term
  bool epi = false, split2 = false, out_init = false;         // out_init: `out` holds a plane before the products with R
  int64_t epi_direct_b = -1;
  std::vector<std::pair<const WBlock*, int>> epi_diag;
  // the operands; T1 / T2 are stacks of planes [a, x, k] like the centre, and so is `out` where it serves as one
  View L, C, R, T1, T2, OUT;
  View dest(int64_t f) const { return f == ru ? OUT.as("axk") : T2.sub('p', plane_of[f], 1); }
  View src(int64_t b) const { return b == lu ? C.as("axk") : b == epi_direct_b ? OUT.as("axk") : T1.sub('t', tmp_of[b], 1); }
};

inline FoldAnalysis fold_analyse(int dtype, const mpse_heff& h, const WSiteInfo& wi, bool two_results, bool mix_epilogue) {
  FoldAnalysis a;
  a.wi = &wi;
  const mpse_dims& s = h.dims;
  const int64_t Dl = s.Dl_ket, Dr = s.Dr_ket, wl = s.wl, wr = s.wr, d = s.d0;
  const int64_t Dlb = s.Dl_bra > 0 ? s.Dl_bra : Dl, Drb = s.Dr_bra > 0 ? s.Dr_bra : Dr;
  if (h.nsite != 1 || s.danc > 1 || h.w_dtype != MPSE_F64 || wi.wl != wl || wi.d != d || wi.wr != wr ||
      ((dtype != MPSE_C128 || h.r_dtype != MPSE_C128) && fold_align() == 64)) {   // (the grouped kernel is built for a
                                                    // complex second operand: centre and R; host emulation: any)
    a.error = "fold: not a plain complex one-site centre with a real MPO site";
    return a;
  }
  if (Dlb % fold_align() != 0 || Dl % std::min<int64_t>(16, fold_align()) != 0 ||
      Dr % std::min<int64_t>(16, fold_align()) != 0 || d > WM_CHUNK * WM_MAXCHUNKS || Dl * d * Dr * Dlb < fold_min()) {
    a.error = "fold: centre too small or not tile aligned";
    return a;
  }
  const int64_t lu = a.lu = (h.l_unit >= 1 && h.l_unit <= wl && Dlb == Dl) ? h.l_unit - 1 : -1;
  const int64_t ru = a.ru = (h.r_unit >= 1 && h.r_unit <= wr && Drb == Dr) ? h.r_unit - 1 : -1;
  auto &by_f = a.by_f, &by_b = a.by_b;
  by_f.resize(wr), by_b.resize(wl);
  for (const WBlock& k : wi.blocks) by_f[k.f].push_back(&k), by_b[k.b].push_back(&k);
  // Epilogue mix: the plane f = ru, where it is a sum of narrow bands and a product with R follows to carry it.  One
  // identity block whose channel b feeds nothing else is written straight into `out` by the product with L (nothing
  // else writes `out` before the products with R) and read back as a term of its own.
  if (mix_epilogue && ru >= 0 && !by_f[ru].empty() && d > 0 && 64 % d == 0) {
    bool sum = true, follows = false;
    {
      const WBlock* k = by_f[ru][0];
      if (by_f[ru].size() == 1 && k->ident && k->b != lu && by_b[k->b].size() == 1) sum = false;   // already direct
    }
    for (int64_t f = 0; f < wr; ++f)
      if (f != ru && !by_f[f].empty()) follows = true;
    bool narrow = true;
    for (const WBlock* k : by_f[ru]) {
      if (k->ident) {
        a.epi_diag.push_back({k, 0});
        continue;
      }
      bool diag[2 * EPI_MAXBAND + 1] = {false};
      for (int64_t x = 0; x < d; ++x)
        for (int64_t e = 0; e < d; ++e)
          if (wi.w[((k->b * d + x) * d + e) * wr + k->f] != 0.0) {
            if (std::abs(e - x) > EPI_MAXBAND)
              narrow = false;
            else
              diag[e - x + EPI_MAXBAND] = true;
          }
      for (int q = 0; q <= 2 * EPI_MAXBAND; ++q)
        if (diag[q]) a.epi_diag.push_back({k, q - EPI_MAXBAND});
    }
    a.epi = sum && follows && narrow && (int)a.epi_diag.size() <= EPI_MAXTERM;
    if (a.epi)
      for (const WBlock* k : by_f[ru])
        if (k->ident && k->b != lu && by_b[k->b].size() == 1) {
          a.epi_direct_b = k->b;
          break;
        }
  }
  a.direct_f.assign(wl, -1), a.tmp_of.assign(wl, -1);
  int64_t ngemm = 0;
  for (int64_t b = 0; b < wl; ++b) {
    if (b == lu || by_b[b].empty()) continue;
    ++ngemm;
    if (b == a.epi_direct_b)
      a.direct_f[b] = ru;
    else if (by_b[b].size() == 1 && by_b[b][0]->ident && by_f[by_b[b][0]->f].size() == 1)
      a.direct_f[b] = by_b[b][0]->f;
    else
      a.tmp_of[b] = a.ntmp++;
  }
  if (ngemm > G_MAXGRP) {
    a.error = "fold: too many channels";
    return a;
  }
  a.plane_of.assign(wr, -1), a.alias.assign(wr, 0), a.present.assign(wr, 0);
  int64_t ncseg = 0;      // channels the products with R run over
  for (int64_t f = 0; f < wr; ++f) {
    if (by_f[f].empty()) continue;
    a.present[f] = 1;
    if (f == ru) continue;
    ++ncseg;
    if (by_f[f].size() == 1 && by_f[f][0]->b == lu && by_f[f][0]->ident)
      a.alias[f] = 1;
    else
      a.plane_of[f] = a.nplanes++;
  }
  // The products with R as halved tiles (split2) when the caller takes the result in two parts, they have at most one
  // tile per compute unit and fit one launch.
  const int64_t ctiles = ((Dlb * d + 63) / 64) * ((Drb + 63) / 64);
  a.split2 = two_results && fold_split2() && ncseg >= 1 && ncseg <= G_MAXSEG && ctiles <= fold_cus() &&
             ncseg * ((Dr + 15) / 16) >= fold_split2_min_kt() && (Dlb * d) % 64 == 0 && Drb == Dr && dtype == MPSE_C128;
  // the planes that are sums of blocks: the elementwise pass
  int64_t nslot = 0;
  for (int64_t f = 0; f < wr; ++f) {
    if (!a.present[f] || a.alias[f]) continue;
    if (a.epi && f == ru) continue;        // formed by the first product with R
    bool is_direct = false;
    for (const WBlock* k : by_f[f])
      if (k->b != lu && a.direct_f[k->b] == f) is_direct = true;
    if (is_direct) continue;
    if ((int)a.mixed.size() >= WM_MAXDST || (int)by_f[f].size() > WM_MAXTERM) {
      a.error = "fold: too many blocks per channel";
      return a;
    }
    a.mixed.push_back(f);
    for (const WBlock* k : by_f[f]) nslot += k->ident ? 0 : 1;
  }
  if (!wmix_fits_lds(nslot, d)) {
    a.error = "fold: blocks too large for the elementwise pass";
    return a;
  }
  a.out_init = ru >= 0 && a.present[ru];
  if (ncseg == 0 && !a.out_init) {
    a.error = "fold: the MPO site is zero";
    return a;
  }
  a.L = View(B_L, h.l_dtype, {{'a', Dlb}, {'b', wl}, {'c', Dl}}), a.R = View(B_R, h.r_dtype, {{'l', Drb}, {'f', wr}, {'k', Dr}});
  a.C = View(B_C, dtype, {{'c', Dl}, {'x', d}, {'k', Dr}}), a.OUT = View(B_OUT, dtype, {{'a', Dlb}, {'x', d}, {'l', Drb}});
  a.T1 = View(B_T1, dtype, {{'t', a.ntmp}, {'a', Dlb}, {'x', d}, {'k', Dr}});
  a.T2 = View(B_T2, dtype, {{'p', a.nplanes}, {'a', Dlb}, {'x', d}, {'k', Dr}});
  return a;
}

// L products: all L[:, b, :] . C in one grouped launch, each into its plane or its temporary
inline void fold_emit_l(Plan& p, const FoldAnalysis& a) {
  Step ga{};
  ga.kind = K_GGEMM;
  ga.dta = a.L.dt, ga.dtb = a.C.dt;
  product_maps(ga, a.L, a.C, a.T1, "a", "c", "xk");
  ga.batch = 1;
  ga.scan_a.on = true;        // L as (channel | bra bond) rows: every 64-row tile belongs to one channel
  ga.scan_a.buf = a.L.buf, ga.scan_a.dt = a.L.dt, ga.scan_a.off = a.L.off;
  labels_index(a.L, "ba", &ga.scan_a.r), labels_index(a.L, "c", &ga.scan_a.k);
  for (int64_t b = 0; b < (int64_t)a.tmp_of.size(); ++b) {
    if (a.direct_f[b] < 0 && a.tmp_of[b] < 0) continue;
    const View Lb = a.L.sub('b', b, 1), dst = a.direct_f[b] >= 0 ? a.dest(a.direct_f[b]) : a.T1.sub('t', a.tmp_of[b], 1);
    GGroupPlan g;
    g.nseg = 1;
    g.seg[0].abuf = Lb.buf, g.seg[0].a_off = Lb.off, g.seg[0].am_row0 = b * (a.L.ext('a') / 64);
    g.seg[0].bbuf = a.C.buf, g.seg[0].b_off = a.C.off, g.seg[0].bm_kind = BM_CENTRE;
    g.cbuf = dst.buf, g.c_off = dst.off;
    ga.groups.push_back(g);
  }
  if (!ga.groups.empty()) p.steps.push_back(ga);
}

// elementwise mix: the planes that are sums of blocks
inline void fold_emit_mix(Plan& p, const FoldAnalysis& a) {
  Step mix{};
  mix.kind = K_WMIX;
  mix.b = B_W0;
  mix.dta = a.C.dt, mix.dtb = MPSE_F64;   // (a real MPO site: fold_analyse refuses any other)
  mix.wp_Da = a.L.ext('a'), mix.wp_d = a.C.ext('x'), mix.wp_Dk = a.C.ext('k'), mix.wp_wr = a.R.ext('f');
  for (int64_t f : a.mixed) {
    const View dst = a.dest(f);
    WMixDst q;
    q.dst = dst.buf, q.dst_off = dst.off, q.s_a = dst.stride('a'), q.s_d = dst.stride('x');
    for (const WBlock* k : a.by_f[f]) q.term[q.nterm++] = wmix_term(*a.wi, *k, a.src(k->b));
    mix.mix.push_back(q);
  }
  if (!mix.mix.empty()) p.steps.push_back(mix);
}

// R products: out (+)= sum_{f != ru} P_f . R[:, f, :]^T, one group, at most G_MAXSEG channels per launch
inline void fold_emit_r(Plan& p, const FoldAnalysis& a) {
  Step gc{};
  gc.kind = K_GGEMM;
  gc.dta = a.C.dt, gc.dtb = a.R.dt;
  product_maps(gc, a.T2, a.R, a.OUT, "ax", "k", "l");
  gc.batch = 1;
  gc.scan_b.on = true;        // R as (bra bond) x (channel | ket bond)
  gc.scan_b.buf = a.R.buf, gc.scan_b.dt = a.R.dt, gc.scan_b.off = a.R.off;
  labels_index(a.R, "l", &gc.scan_b.r), labels_index(a.R, "fk", &gc.scan_b.k);
  std::vector<GSegPlan> segs;
  for (int64_t f = 0; f < (int64_t)a.present.size(); ++f) {
    if (!a.present[f] || f == a.ru) continue;
    const View P = a.alias[f] ? a.C : a.T2.sub('p', a.plane_of[f], 1), Rf = a.R.sub('f', f, 1);
    GSegPlan sg;
    sg.abuf = P.buf, sg.a_off = P.off;
    sg.bbuf = Rf.buf, sg.b_off = Rf.off;
    sg.bm_kind = BM_SCAN, sg.bm_kt0 = f * (a.R.ext('k') / 16);
    segs.push_back(sg);
  }
  for (size_t i = 0; i < segs.size(); i += G_MAXSEG) {
    Step st = gc;
    GGroupPlan g;
    g.cbuf = a.OUT.buf, g.c_off = a.OUT.off;
    g.beta = (a.out_init || i > 0) ? 1.0 : 0.0;     // the first launch starts `out` unless a plane is there already
    if (a.split2) g.split2 = true, p.two_results = true;
    for (size_t j = i; j < segs.size() && j < i + G_MAXSEG; ++j) g.seg[g.nseg++] = segs[j];
    if (a.epi && i == 0) {
      g.wbuf = B_W0, g.mix_d = a.C.ext('x'), g.mix_wr = a.R.ext('f'), g.mix_ld = a.T2.stride('x');
      for (const auto& kd : a.epi_diag) {
        const View src = a.src(kd.first->b);
        EpiTerm& t = g.mix[g.nmix++];
        t.b = kd.first->b, t.f = kd.first->f, t.delta = kd.second;
        t.src = src.buf, t.src_off = src.off;
      }
    }
    st.groups.push_back(g);
    p.steps.push_back(st);
  }
}

// Folded one-site matvec; p.error is set when the site does not qualify and the caller takes plan_heff.
inline Plan plan_heff1_fold(int dtype, const mpse_heff& h, const WSiteInfo& wi, bool two_results = false,
                            bool mix_epilogue = false) {
  Plan p;
  const FoldAnalysis a = fold_analyse(dtype, h, wi, two_results, mix_epilogue);
  if ((p.error = a.error)) return p;
  p.tmp_elems[0] = a.ntmp * a.T1.stride('t');
  p.tmp_elems[1] = a.nplanes * a.T2.stride('p');
  fold_emit_l(p, a);
  fold_emit_mix(p, a);
  fold_emit_r(p, a);
  return marked(std::move(p));
}


// Environment update, mps/lib.py:169-250.  Buffers: B_L = incoming environment (either
// domain), B_C = ket site, B_BRA = bra site, B_W0 = mpo site, B_OUT = new environment.
// MPO step of an environment update as the elementwise pass of the folded matvec (K_WMIX) instead of a batched
// real x complex product: for a large physical index and a site the caller has described (mpse_mpo_site_hint) the
// product moves ~130 MB to apply a handful of identity / diagonal / tridiagonal blocks.  in_left: the incoming channel is
// the LEFT index of W (domain L); otherwise the right one (domain R).  Tensors: src[a, c, x, k] / dst[a, c, x, k] with c
// the channel and x the physical index, in whatever order the views hold them.  Returns false (nothing pushed) when the
// site does not fit the pass.
inline bool push_env_wmix(Plan& p, const WSiteInfo& wi, bool in_left, int w_dtype, const View& src, const View& dst) {
  const int64_t d = wi.d, nout = in_left ? wi.wr : wi.wl;
  if (d > 32 || (d + WM_CHUNK - 1) / WM_CHUNK > WM_MAXCHUNKS) return false;
  std::vector<std::vector<const WBlock*>> by_out(nout);
  int64_t nslot = 0;
  for (const WBlock& k : wi.blocks) {
    by_out[in_left ? k.f : k.b].push_back(&k);
    nslot += k.ident ? 0 : 1;
  }
  for (auto& v : by_out)
    if ((int)v.size() > WM_MAXTERM) return false;
  if (!wmix_fits_lds(nslot, d)) return false;
  Step mix{};
  mix.kind = K_WMIX;
  mix.b = B_W0;
  mix.dta = src.dt, mix.dtb = w_dtype;
  mix.wp_Da = src.ext('a'), mix.wp_d = d, mix.wp_Dk = src.ext('k'), mix.wp_wr = wi.wr;
  Step part = mix;
  for (int64_t o = 0; o < nout; ++o) {
    const View dv = dst.sub('c', o, 1);
    WMixDst q;
    q.dst = dv.buf, q.dst_off = dv.off, q.s_a = dv.stride('a'), q.s_d = dv.stride('x');
    for (const WBlock* k : by_out[o]) q.term[q.nterm++] = wmix_term(wi, *k, src.sub('c', in_left ? k->b : k->f, 1));
    part.mix.push_back(q);         // (a channel without blocks: nterm = 0, the pass writes zeros)
    if ((int)part.mix.size() == WM_MAXDST) {
      p.steps.push_back(part);
      part = mix;
    }
  }
  if (!part.mix.empty()) p.steps.push_back(part);
  return true;
}

// The products with the bra that close an environment update (Y = the last intermediate, K = everything contracted):
//   L: out[p,(f,h)] = sum_{A,g} bra*[(A,g),p] Y[A,f,g,h]      A = (bra bond, physical), g = traced ancilla
//   R: out[p,(q,h)] = sum_K bra*[p,K] Y[h,q,K]                K = (physical, ancilla, bra bond)
inline Step* push_bra_l(Plan& p, int ybuf, int dtype, int bra_conj, int64_t A, int64_t anc, int64_t wr, int64_t Drk, int64_t Drb) {
  const View BRA(B_BRA, dtype, {{'A', A}, {'g', anc}, {'p', Drb}}), Y(ybuf, dtype, {{'A', A}, {'f', wr}, {'g', anc}, {'h', Drk}});
  return contract(p, BRA, Y, View(B_OUT, dtype, {{'p', Drb}, {'f', wr}, {'h', Drk}}), "p", "Ag", "fh", "", "", bra_conj);
}
inline Step* push_bra_r(Plan& p, int ybuf, int dtype, int bra_conj, int64_t K, int64_t wl, int64_t Dlk, int64_t Dlb) {
  const View BRA(B_BRA, dtype, {{'p', Dlb}, {'K', K}}), Y(ybuf, dtype, {{'h', Dlk}, {'q', wl}, {'K', K}});
  return contract(p, BRA, Y, View(B_OUT, dtype, {{'p', Dlb}, {'q', wl}, {'h', Dlk}}), "p", "K", "qh", "", "", bra_conj);
}

inline Plan plan_env(int dtype, int domain, const mpse_dims& s, int env_dtype, int w_dtype, int bra_conj,
                     const WSiteInfo* wi = nullptr) {
  Plan p;
  // the described site takes the elementwise MPO step where the batched product is the expensive way (large d, no ancilla)
  const bool wfold = wi && dtype == MPSE_C128 && w_dtype == MPSE_F64 && s.d0 >= 8 && (s.danc <= 1) && wi->wl == s.wl &&
                     wi->d == s.d0 && wi->wr == s.wr;
  const int64_t d = s.d0, wl = s.wl, wr = s.wr;
  const int64_t anc = s.danc > 0 ? s.danc : 1;
  const int64_t Dlb = s.Dl_bra, Dlk = s.Dl_ket, Drb = s.Dr_bra, Drk = s.Dr_ket;
  if (domain == MPSE_DOMAIN_L) {
    // env L[a,b,c] ; ket A[c,e,g,h] ; W[b,d,e,f] ; bra Ab[a,d,g,p] -> out[p,f,h]  (g = traced ancilla)
    const int64_t N = d * anc * Drk;
    p.tmp_elems[0] = Dlb * wl * N;
    p.tmp_elems[1] = Dlb * d * wr * anc * Drk;
    // X[b,a,(e,g,h)] = sum_c L[(a,b),c] A[c,(e,g,h)]
    push_env_times(p, B_L, env_dtype, B_C, dtype, B_T1, Dlb, wl, Dlk, N, s.env_unit, true);
    // Y[a,d,f,(g,h)] = sum_{b,e} W[b,d,e,f] X[b,a,e,(g,h)]
    if (!(wfold && push_env_wmix(p, *wi, true, w_dtype, View(B_T1, dtype, {{'c', wl}, {'a', Dlb}, {'x', d}, {'k', Drk}}),
                                 View(B_T2, dtype, {{'a', Dlb}, {'x', d}, {'c', wr}, {'k', Drk}}))))
      push_w(p, B_W0, w_dtype, B_T1, B_T2, dtype, Dlb, wl, d, wr, anc * Drk);
    // out[p,(f,h)] = sum_{a,d,g} bra*[(a,d,g),p] Y[a,d,f,g,h]
    if (Step* st = push_bra_l(p, B_T2, dtype, bra_conj, Dlb * d, anc, wr, Drk, Drb))
      st->skip_zero = skip_pays(Drb, Dlb * d * anc, wr * Drk, 1);   // B = the big intermediate: bra side only
    return marked(std::move(p));
  }
  if (domain == MPSE_DOMAIN_R) {
    // env R[a,b,c] ; ket A[h,e,g,c] ; W[q,d,e,b] ; bra Ab[p,d,g,a] -> out[p,q,h]
    p.tmp_elems[0] = Dlk * d * anc * wr * Drb;
    p.tmp_elems[1] = Dlk * wl * d * anc * Drb;
    // X[m,b,a] = sum_c A[m,c] R[a,b,c]   m = (h,e,g); columns ordered (b | a) through the strides of R
    const int64_t M = Dlk * d * anc;
    const int64_t u = (s.env_unit >= 1 && s.env_unit <= wr && Drb == Drk && unit_pays(M, Drk, Drb)) ? s.env_unit - 1 : -1;
    const View A(B_C, dtype, {{'m', M}, {'c', Drk}}), R(B_L, env_dtype, {{'a', Drb}, {'b', wr}, {'c', Drk}});
    const View X(B_T1, dtype, {{'m', M}, {'b', wr}, {'a', Drb}});
    // unit channel: R[a,u,c] = delta(a,c)  =>  X[m,u,a] = A[m,a]
    if (u >= 0) copy(p, A.as("ma"), X.sub('b', u, 1), "m", "a");
    const ChannelRanges cr(u, wr);
    for (int r = 0; r < 2; ++r) {
      const int64_t b0 = cr.lo[r], nb = cr.hi[r] - cr.lo[r];
      if (nb <= 0) continue;
      if (Step* st = contract(p, A, R.sub('b', b0, nb), X.sub('b', b0, nb), "m", "c", "ba"))
        st->skip_zero = skip_pays(M, Drk, nb * Drb);
    }
    // Y[h,q,y,g,a] = sum_{e,b} W[q,y,e,b] X[h,e,g,b,a] ; batch h ; one step per ancilla value g
    if (!(wfold && push_env_wmix(p, *wi, false, w_dtype, View(B_T1, dtype, {{'a', Dlk}, {'x', d}, {'c', wr}, {'k', Drb}}),
                                 View(B_T2, dtype, {{'a', Dlk}, {'c', wl}, {'x', d}, {'k', Drb}}))))
      contract(p, View(B_W0, w_dtype, {{'q', wl}, {'y', d}, {'e', d}, {'b', wr}}),
               View(B_T1, dtype, {{'h', Dlk}, {'e', d}, {'g', anc}, {'b', wr}, {'a', Drb}}),
               View(B_T2, dtype, {{'h', Dlk}, {'q', wl}, {'y', d}, {'g', anc}, {'a', Drb}}), "qy", "eb", "a", "h", "g");
    // out[p,(q,h)] = sum_{d,g,a} bra*[p,(d,g,a)] Y[h,q,(d,g,a)]
    if (Step* st = push_bra_r(p, B_T2, dtype, bra_conj, d * anc * Drb, wl, Dlk, Dlb))
      st->skip_zero = skip_pays(Dlb, d * anc * Drb, wl * Dlk, 1);
    return marked(std::move(p));
  }
  p.error = "env: bad domain";
  return p;
}


// Environment update with a stack of n MPO sites (mps/lib.py:121-166 contract_one_site_multi_mpo), n >= 1:
//   L: env E[a, b_1..b_n, c], bra[a, x_0, g, p], W_i[b_i, x_{i-1}, x_i, f_i], ket[c, x_n, g, h] -> out[p, f_1..f_n, h]
//   R: env E[a, b_1..b_n, c], bra[p, x_0, g, a], W_i[q_i, x_{i-1}, x_i, b_i], ket[h, x_n, g, c] -> out[p, q_1..q_n, h]
// (layer 1 touches the bra, layer n the ket; g = traced ancilla).  Buffers: B_L env, B_C ket, B_BRA bra, B_OUT out,
// MPO sites w_buf(layer) = B_W0, B_W1, B_W2, B_W3; intermediates alternate between B_T1 and B_T2.
inline Plan plan_env_multi(int dtype, int domain, const mpse_dims& s, int n, const int64_t* wl, const int64_t* wr,
                           int env_dtype, int w_dtype, int bra_conj) {
  Plan p;
  if (n < 1 || n > 4) {
    p.error = "env_multi: 1 to 4 MPO layers";
    return p;
  }
  const int64_t d = s.d0, anc = s.danc > 0 ? s.danc : 1;
  const int64_t Dlb = s.Dl_bra, Dlk = s.Dl_ket, Drb = s.Dr_bra, Drk = s.Dr_ket;
  int64_t WL = 1, WR = 1;
  for (int i = 0; i < n; ++i) WL *= wl[i], WR *= wr[i];
  const bool left = domain == MPSE_DOMAIN_L;
  if (!left && domain != MPSE_DOMAIN_R) {
    p.error = "env: bad domain";
    return p;
  }
  // sizes of the intermediates: after the first GEMM the channels still carry the incoming bonds; layer by layer
  // (ket side first) they are replaced by the outgoing ones
  int64_t win[4], wout[4];
  for (int i = 0; i < n; ++i) win[i] = left ? wl[i] : wr[i], wout[i] = left ? wr[i] : wl[i];
  const int64_t Da = left ? Dlb : Drb;      // bond of the environment row that stays open until the last step
  const int64_t Dh = left ? Drk : Dlk;      // open ket bond
  int64_t cur = Da * d * anc * Dh;
  for (int i = 0; i < n; ++i) cur *= win[i];
  int64_t maxsz = cur;
  {
    int64_t t = cur;
    for (int i = n - 1; i >= 0; --i) {
      t = t / win[i] * wout[i];
      if (t > maxsz) maxsz = t;
    }
  }
  p.tmp_elems[0] = p.tmp_elems[1] = maxsz;
  int tb = B_T1;
  if (left) {
    // T_n[(b_1..b_n), a, x, g, h] = sum_c E[a, (b), c] ket[c, (x, g, h)]   (channel-outer layout)
    push_env_times(p, B_L, env_dtype, B_C, dtype, tb, Dlb, WL, Dlk, d * anc * Drk, 0, true);
    // layer i = n..1: T_{i-1}[P, a, y, f_i, F, g, h] = sum_{b_i, x} W_i[b_i, y, x, f_i] T_i[P, b_i, a, x, F, g, h]
    int64_t P = WL, F = 1;
    for (int i = n - 1; i >= 0; --i) {
      P /= wl[i];
      View W(w_buf(i), w_dtype, {{'b', wl[i]}, {'y', d}, {'x', d}, {'f', wr[i]}});
      View Tin(tb, dtype, {{'P', P}, {'b', wl[i]}, {'a', Dlb}, {'x', d}, {'N', F * anc * Drk}});
      const int to = tb == B_T1 ? B_T2 : B_T1;
      View Tout(to, dtype, {{'P', P}, {'a', Dlb}, {'y', d}, {'f', wr[i]}, {'N', F * anc * Drk}});
      contract(p, W, Tin, Tout, "yf", "bx", "N", "a", "P");
      tb = to;
      F *= wr[i];
    }
    // out[p, (F, h)] = sum_{a, y, g} bra*[(a, y, g), p] T_0[(a, y), F, g, h]
    push_bra_l(p, tb, dtype, bra_conj, Dlb * d, anc, WR, Drk, Drb);
    return marked(std::move(p));
  }
  // R: T_n[h, x, g, (b_1..b_n), a] = sum_c ket[(h, x, g), c] E[a, (b), c]
  contract(p, View(B_C, dtype, {{'m', Dlk * d * anc}, {'c', Drk}}), View(B_L, env_dtype, {{'a', Drb}, {'b', WR}, {'c', Drk}}),
           View(tb, dtype, {{'m', Dlk * d * anc}, {'b', WR}, {'a', Drb}}), "m", "c", "ba");
  // layer i = n..1: T_{i-1}[h, q_i, Q, y, g, P, a] = sum_{x, b_i} W_i[q_i, y, x, b_i] T_i[h, Q, x, g, P, b_i, a]
  int64_t P = WR, Q = 1;
  for (int i = n - 1; i >= 0; --i) {
    P /= wr[i];
    View W(w_buf(i), w_dtype, {{'q', wl[i]}, {'y', d}, {'x', d}, {'b', wr[i]}});
    View Tin(tb, dtype, {{'h', Dlk}, {'Q', Q}, {'x', d}, {'g', anc}, {'P', P}, {'b', wr[i]}, {'a', Drb}});
    const int to = tb == B_T1 ? B_T2 : B_T1;
    View Tout(to, dtype, {{'h', Dlk}, {'q', wl[i]}, {'Q', Q}, {'y', d}, {'g', anc}, {'P', P}, {'a', Drb}});
    contract(p, W, Tin, Tout, "qy", "xb", "Pa", "h", "Qg");
    tb = to;
    Q *= wl[i];
  }
  // out[p, (Q, h)] = sum_{y, g, a} bra*[p, (y, g, a)] T_0[h, Q, (y, g, a)]
  push_bra_r(p, tb, dtype, bra_conj, d * anc * Drb, WL, Dlk, Dlb);
  return marked(std::move(p));
}

// Two-layer effective Hamiltonian of the (H - omega)^2 functional, mps/hop_expr.py:24-52 (same MPO sites in both
// layers, no ancilla):
//   1-site  abcd, befg, cfhi, jgik, aej -> dhk          L (Dl, wl, wl, Dl), R (Dr, wr, wr, Dr), W0 (wl, d0, d0, wr)
//   2-site  abcd, befg, cfhi, gjkl, ikmn, olnp, aejo -> dhmp         W0 (wl, d0, d0, wm), W1 (wm, d1, d1, wr)
// The centre enters through the FIRST bond index of L / R and the upper physical legs, the result leaves through
// the last one - exactly the reference's index placement.
inline Plan plan_heff2(int dtype, const mpse_heff& h) {
  Plan p;
  const mpse_dims& s = h.dims;
  const int64_t Dl = s.Dl_ket, Dr = s.Dr_ket, wl = s.wl, wr = s.wr, d0 = s.d0;
  if (h.nsite != 1 && h.nsite != 2) {
    p.error = "heff (two layers): one- or two-site centres only";
    return p;
  }
  if ((s.Dl_bra > 0 && s.Dl_bra != Dl) || (s.Dr_bra > 0 && s.Dr_bra != Dr)) {
    p.error = "heff (two layers): bra bonds must equal ket bonds";
    return p;
  }
  // z: a pure batch index next to the right bond (several centres at once - the columns of the identity when the
  // dense projected operator is wanted, mps/gs.py:307-369); 1-site: C (Dl, d0, z, Dr) with z = danc,
  // 2-site: C (Dl, d0, d1, z, Dr) with z = danc1 (danc must be 1)
  if (h.nsite == 1) {
    const int64_t nz = s.danc > 0 ? s.danc : 1;
    const int64_t big = std::max(wl * wl, std::max(wl * wr, wr * wr)) * Dl * d0 * nz * Dr;
    p.tmp_elems[0] = p.tmp_elems[1] = p.tmp_elems[2] = big;
    View L(B_L, h.l_dtype, {{'a', Dl}, {'b', wl}, {'c', wl}, {'d', Dl}});
    View R(B_R, h.r_dtype, {{'j', Dr}, {'g', wr}, {'i', wr}, {'k', Dr}});
    View W(B_W0, h.w_dtype, {{'b', wl}, {'e', d0}, {'f', d0}, {'g', wr}});       // layer 1 labels
    View W2(B_W0, h.w_dtype, {{'c', wl}, {'f', d0}, {'h', d0}, {'i', wr}});      // layer 2 labels
    View C(B_C, dtype, {{'a', Dl}, {'e', d0}, {'z', nz}, {'j', Dr}});
    View T1(B_T1, dtype, {{'b', wl}, {'c', wl}, {'d', Dl}, {'e', d0}, {'z', nz}, {'j', Dr}});
    contract(p, L, C, T1, "bcd", "a", "ezj");
    View T2(B_T2, dtype, {{'c', wl}, {'d', Dl}, {'f', d0}, {'g', wr}, {'z', nz}, {'j', Dr}});
    contract(p, W, T1, T2, "fg", "be", "zj", "cd");
    View T3(B_T3, dtype, {{'d', Dl}, {'h', d0}, {'z', nz}, {'j', Dr}, {'g', wr}, {'i', wr}});
    contract(p, W2, T2, T3, "hi", "cf", "zjg", "d");
    View O(B_OUT, dtype, {{'d', Dl}, {'h', d0}, {'z', nz}, {'k', Dr}});
    contract(p, T3, R, O, "dhz", "jgi", "k");
    return marked(std::move(p));
  }
  if (s.danc > 1) {
    p.error = "heff (two layers, 2-site): the batch index is danc1, danc must be 1";
    return p;
  }
  const int64_t d1 = s.d1, wm = s.wm, nz = s.danc1 > 0 ? s.danc1 : 1;
  {
    int64_t big = 0;
    const int64_t cand[5] = {wl * wl, wl * wm, wm * wm, wm * wr, wr * wr};
    for (int64_t c : cand) big = c > big ? c : big;
    p.tmp_elems[0] = p.tmp_elems[1] = p.tmp_elems[2] = big * d0 * d1 * nz * Dl * Dr;
  }
  View L(B_L, h.l_dtype, {{'a', Dl}, {'b', wl}, {'c', wl}, {'d', Dl}});
  View R(B_R, h.r_dtype, {{'o', Dr}, {'l', wr}, {'n', wr}, {'p', Dr}});
  View C(B_C, dtype, {{'a', Dl}, {'e', d0}, {'j', d1}, {'z', nz}, {'o', Dr}});
  View Wa(B_W0, h.w_dtype, {{'b', wl}, {'e', d0}, {'f', d0}, {'g', wm}});
  View Wb(B_W0, h.w_dtype, {{'c', wl}, {'f', d0}, {'h', d0}, {'i', wm}});
  View Wc(B_W1, h.w_dtype, {{'g', wm}, {'j', d1}, {'k', d1}, {'l', wr}});
  View Wd(B_W1, h.w_dtype, {{'i', wm}, {'k', d1}, {'m', d1}, {'n', wr}});
  View T1(B_T1, dtype, {{'b', wl}, {'c', wl}, {'d', Dl}, {'e', d0}, {'j', d1}, {'z', nz}, {'o', Dr}});
  contract(p, L, C, T1, "bcd", "a", "ejzo");
  View T2(B_T2, dtype, {{'c', wl}, {'d', Dl}, {'f', d0}, {'g', wm}, {'j', d1}, {'z', nz}, {'o', Dr}});
  contract(p, Wa, T1, T2, "fg", "be", "jzo", "cd");
  View T3(B_T3, dtype, {{'d', Dl}, {'h', d0}, {'i', wm}, {'g', wm}, {'j', d1}, {'z', nz}, {'o', Dr}});
  contract(p, Wb, T2, T3, "hi", "cf", "gjzo", "d");
  View T4(B_T1, dtype, {{'d', Dl}, {'h', d0}, {'i', wm}, {'k', d1}, {'l', wr}, {'z', nz}, {'o', Dr}});
  contract(p, Wc, T3, T4, "kl", "gj", "zo", "dhi");
  View T5(B_T2, dtype, {{'d', Dl}, {'h', d0}, {'m', d1}, {'z', nz}, {'o', Dr}, {'l', wr}, {'n', wr}});
  contract(p, Wd, T4, T5, "mn", "ik", "zol", "dh");
  View O(B_OUT, dtype, {{'d', Dl}, {'h', d0}, {'m', d1}, {'z', nz}, {'p', Dr}});
  contract(p, T5, R, O, "dhmz", "oln", "p");
  return marked(std::move(p));
}

// Two MPO layers on a centre with two physical legs (a site of an operator in MPS form: C (Dl, d_up, d_down, Dr)),
// each layer on a leg of its own choice: the three terms of ((omega - Liou)^2) X = a a X + 2 a X H + X H H with
// a = omega - H (cv/finitet.py:215-299).  Labels:
//   L (a, b, c, d)  a = bond towards the centre (ket), b / c = MPO bonds of layer 1 / 2, d = bond of the result (bra)
//   R (j, g, i, k)  the same on the right;   C (a, u, v, j);   out (d, u', v', k)
//   layer n, MPO site W_n (wl_n, d, d, wr_n): trans == 0: leg'[x] = sum_y W_n[., x, y, .] leg[y]; trans != 0:
//   leg'[y] = sum_x W_n[., x, y, .] leg[x].  The leg no layer touches passes through.
// Both layers up is plan_heff2 with d_down as its batch index (the same steps, so the same bits); both down moves the
// spectator into the batch of the MPO steps; one on each leg (up first) runs the second layer as a batch over
// (bond, MPO bond, up leg).  Nothing is transposed in memory: every permutation is in the views.
inline View ft_w_view(int buf, int dt, bool trans, char lb, int64_t wl, char in, char out, int64_t d, char rb,
                      int64_t wr) {
  return trans ? View(buf, dt, {{lb, wl}, {in, d}, {out, d}, {rb, wr}}) : View(buf, dt, {{lb, wl}, {out, d}, {in, d}, {rb, wr}});
}

inline const char* ft_check(const mpse_heff_ft& h) {
  if (h.Dl <= 0 || h.Dr <= 0 || h.d_up <= 0 || h.d_down <= 0 || h.wl1 <= 0 || h.wr1 <= 0 || h.wl2 <= 0 || h.wr2 <= 0)
    return "heff_ft: empty extent";
  if ((h.leg1 != MPSE_LEG_UP && h.leg1 != MPSE_LEG_DOWN) || (h.leg2 != MPSE_LEG_UP && h.leg2 != MPSE_LEG_DOWN))
    return "heff_ft: a layer acts on MPSE_LEG_UP or MPSE_LEG_DOWN";
  if (h.leg1 == MPSE_LEG_DOWN && h.leg2 == MPSE_LEG_UP)
    return "heff_ft: layers on different legs commute - give the one on the up leg first";
  return nullptr;
}

// largest intermediate of a chain: left to right T1 (b, c), T2 (c, g), T3 (g, i); right to left T1 (g, i), T2 (b, i), T3 (b, c)
inline int64_t ft_tmp_elems(const mpse_heff_ft& h, bool right_to_left = false) {
  const int64_t mid = right_to_left ? h.wl1 * h.wr2 : h.wl2 * h.wr1;
  return std::max(h.wl1 * h.wl2, std::max(mid, h.wr1 * h.wr2)) * h.Dl * h.d_up * h.d_down * h.Dr;
}

// Left-to-right part shared by the matvec and the left environment update: T3 = W_2 W_1 (L . C); *up / *down receive
// the labels of the two legs in T3, *kr the order in which the last product runs over (j, g, i).
inline View ft_chain_l(Plan& p, int dtype, const mpse_heff_ft& h, char* up, char* down, const char** kr) {
  const int64_t Dl = h.Dl, Dr = h.Dr, du = h.d_up, dv = h.d_down;
  View L(B_L, h.l_dtype, {{'a', Dl}, {'b', h.wl1}, {'c', h.wl2}, {'d', Dl}});
  View C(B_C, dtype, {{'a', Dl}, {'u', du}, {'v', dv}, {'j', Dr}});
  View T1(B_T1, dtype, {{'b', h.wl1}, {'c', h.wl2}, {'d', Dl}, {'u', du}, {'v', dv}, {'j', Dr}});
  contract(p, L, C, T1, "bcd", "a", "uvj");
  const bool t1 = h.trans1 != 0, t2 = h.trans2 != 0;
  if (h.leg1 == MPSE_LEG_UP && h.leg2 == MPSE_LEG_UP) {
    View W1 = ft_w_view(B_W0, h.w_dtype, t1, 'b', h.wl1, 'u', 'x', du, 'g', h.wr1);
    View W2 = ft_w_view(B_W1, h.w_dtype, t2, 'c', h.wl2, 'x', 'y', du, 'i', h.wr2);
    View T2(B_T2, dtype, {{'c', h.wl2}, {'d', Dl}, {'x', du}, {'g', h.wr1}, {'v', dv}, {'j', Dr}});
    contract(p, W1, T1, T2, "xg", "bu", "vj", "cd");
    View T3(B_T3, dtype, {{'d', Dl}, {'y', du}, {'v', dv}, {'j', Dr}, {'g', h.wr1}, {'i', h.wr2}});
    contract(p, W2, T2, T3, "yi", "cx", "vjg", "d");
    *up = 'y', *down = 'v', *kr = "jgi";
    return T3;
  }
  if (h.leg1 == MPSE_LEG_DOWN && h.leg2 == MPSE_LEG_DOWN) {
    View W1 = ft_w_view(B_W0, h.w_dtype, t1, 'b', h.wl1, 'v', 's', dv, 'g', h.wr1);
    View W2 = ft_w_view(B_W1, h.w_dtype, t2, 'c', h.wl2, 's', 't', dv, 'i', h.wr2);
    View T2(B_T2, dtype, {{'c', h.wl2}, {'d', Dl}, {'u', du}, {'s', dv}, {'g', h.wr1}, {'j', Dr}});
    contract(p, W1, T1, T2, "sg", "bv", "j", "cdu");
    View T3(B_T3, dtype, {{'d', Dl}, {'u', du}, {'t', dv}, {'j', Dr}, {'g', h.wr1}, {'i', h.wr2}});
    contract(p, W2, T2, T3, "ti", "cs", "jg", "du");
    *up = 'u', *down = 't', *kr = "jgi";
    return T3;
  }
  // layer 1 on the up leg, layer 2 on the down leg, side by side
  View W1 = ft_w_view(B_W0, h.w_dtype, t1, 'b', h.wl1, 'u', 'x', du, 'g', h.wr1);
  View W2 = ft_w_view(B_W1, h.w_dtype, t2, 'c', h.wl2, 'v', 's', dv, 'i', h.wr2);
  View T2(B_T2, dtype, {{'c', h.wl2}, {'d', Dl}, {'g', h.wr1}, {'x', du}, {'v', dv}, {'j', Dr}});
  contract(p, W1, T1, T2, "xg", "bu", "vj", "cd");
  View T3(B_T3, dtype, {{'d', Dl}, {'g', h.wr1}, {'x', du}, {'s', dv}, {'i', h.wr2}, {'j', Dr}});
  contract(p, W2, T2, T3, "si", "cv", "j", "dgx");
  *up = 'x', *down = 's', *kr = "gij";
  return T3;
}

// out (Dl, d_up, d_down, Dr) = term applied to C
inline Plan plan_heff_ft(int dtype, const mpse_heff_ft& h) {
  Plan p;
  if ((p.error = ft_check(h))) return p;
  p.tmp_elems[0] = p.tmp_elems[1] = p.tmp_elems[2] = ft_tmp_elems(h);
  char dud[4] = "d";     // (d, up, down): the rows of the last product
  const char* kr;
  View T3 = ft_chain_l(p, dtype, h, &dud[1], &dud[2], &kr);
  View R(B_R, h.r_dtype, {{'j', h.Dr}, {'g', h.wr1}, {'i', h.wr2}, {'k', h.Dr}});
  View O(B_OUT, dtype, {{'d', h.Dl}, {dud[1], h.d_up}, {dud[2], h.d_down}, {'k', h.Dr}});
  contract(p, T3, R, O, dud, kr, "k");
  return marked(std::move(p));
}

// Environment of a term moved over one site X (Dl, d_up, d_down, Dr): bra = conj(X), ket = X, every layer contracts its
// own leg between them, the untouched leg is contracted directly.  Buffers: B_L = incoming environment (L (Dl, wl1, wl2,
// Dl) for MPSE_DOMAIN_L, R (Dr, wr1, wr2, Dr) for MPSE_DOMAIN_R; h.L / h.R are not read), B_C = B_BRA = X,
// B_OUT = (Dr, wr1, wr2, Dr) resp. (Dl, wl1, wl2, Dl), index order (ket bond, layer 1, layer 2, bra bond).
inline Plan plan_env_ft(int dtype, int domain, const mpse_heff_ft& h, int env_dtype) {
  Plan p;
  if ((p.error = ft_check(h))) return p;
  p.tmp_elems[0] = p.tmp_elems[1] = p.tmp_elems[2] = ft_tmp_elems(h, domain == MPSE_DOMAIN_R);
  const int64_t Dl = h.Dl, Dr = h.Dr, du = h.d_up, dv = h.d_down;
  const int conj = dtype == MPSE_C128 ? 1 : 0;
  if (domain == MPSE_DOMAIN_L) {
    mpse_heff_ft hl = h;
    hl.l_dtype = env_dtype;
    char dud[4] = "d";
    const char* kr;
    View T3 = ft_chain_l(p, dtype, hl, &dud[1], &dud[2], &kr);
    View BRA(B_BRA, dtype, {{'d', Dl}, {dud[1], du}, {dud[2], dv}, {'k', Dr}});
    View O(B_OUT, dtype, {{'j', Dr}, {'g', h.wr1}, {'i', h.wr2}, {'k', Dr}});
    contract(p, BRA, T3, O, "k", dud, kr, "", "", conj);
    return marked(std::move(p));
  }
  if (domain != MPSE_DOMAIN_R) {
    p.error = "env: bad domain";
    return p;
  }
  const bool t1 = h.trans1 != 0, t2 = h.trans2 != 0;
  View X(B_C, dtype, {{'a', Dl}, {'u', du}, {'v', dv}, {'j', Dr}});
  View R(B_L, env_dtype, {{'j', Dr}, {'g', h.wr1}, {'i', h.wr2}, {'k', Dr}});
  View T1(B_T1, dtype, {{'a', Dl}, {'u', du}, {'v', dv}, {'g', h.wr1}, {'i', h.wr2}, {'k', Dr}});
  contract(p, X, R, T1, "auv", "j", "gik");
  View O(B_OUT, dtype, {{'a', Dl}, {'b', h.wl1}, {'c', h.wl2}, {'d', Dl}});
  if (h.leg1 == MPSE_LEG_UP && h.leg2 == MPSE_LEG_UP) {
    View W1 = ft_w_view(B_W0, h.w_dtype, t1, 'b', h.wl1, 'u', 'x', du, 'g', h.wr1);
    View W2 = ft_w_view(B_W1, h.w_dtype, t2, 'c', h.wl2, 'x', 'y', du, 'i', h.wr2);
    View T2(B_T2, dtype, {{'a', Dl}, {'b', h.wl1}, {'x', du}, {'v', dv}, {'i', h.wr2}, {'k', Dr}});
    contract(p, W1, T1, T2, "bx", "ug", "vik", "a");
    View T3(B_T3, dtype, {{'a', Dl}, {'b', h.wl1}, {'c', h.wl2}, {'y', du}, {'v', dv}, {'k', Dr}});
    contract(p, W2, T2, T3, "cy", "xi", "vk", "ab");
    View BRA(B_BRA, dtype, {{'d', Dl}, {'y', du}, {'v', dv}, {'k', Dr}});
    contract(p, BRA, T3, O, "d", "yvk", "abc", "", "", conj);
    return marked(std::move(p));
  }
  if (h.leg1 == MPSE_LEG_DOWN && h.leg2 == MPSE_LEG_DOWN) {
    View W1 = ft_w_view(B_W0, h.w_dtype, t1, 'b', h.wl1, 'v', 's', dv, 'g', h.wr1);
    View W2 = ft_w_view(B_W1, h.w_dtype, t2, 'c', h.wl2, 's', 't', dv, 'i', h.wr2);
    View T2(B_T2, dtype, {{'a', Dl}, {'u', du}, {'b', h.wl1}, {'s', dv}, {'i', h.wr2}, {'k', Dr}});
    contract(p, W1, T1, T2, "bs", "vg", "ik", "au");
    View T3(B_T3, dtype, {{'a', Dl}, {'u', du}, {'b', h.wl1}, {'c', h.wl2}, {'t', dv}, {'k', Dr}});
    contract(p, W2, T2, T3, "ct", "si", "k", "aub");
    View BRA(B_BRA, dtype, {{'d', Dl}, {'u', du}, {'t', dv}, {'k', Dr}});
    contract(p, BRA, T3, O, "d", "utk", "abc", "", "", conj);
    return marked(std::move(p));
  }
  View W1 = ft_w_view(B_W0, h.w_dtype, t1, 'b', h.wl1, 'u', 'x', du, 'g', h.wr1);
  View W2 = ft_w_view(B_W1, h.w_dtype, t2, 'c', h.wl2, 'v', 's', dv, 'i', h.wr2);
  View T2(B_T2, dtype, {{'a', Dl}, {'b', h.wl1}, {'x', du}, {'v', dv}, {'i', h.wr2}, {'k', Dr}});
  contract(p, W1, T1, T2, "bx", "ug", "vik", "a");
  View T3(B_T3, dtype, {{'a', Dl}, {'b', h.wl1}, {'x', du}, {'c', h.wl2}, {'s', dv}, {'k', Dr}});
  contract(p, W2, T2, T3, "cs", "vi", "k", "abx");
  View BRA(B_BRA, dtype, {{'d', Dl}, {'x', du}, {'s', dv}, {'k', Dr}});
  contract(p, BRA, T3, O, "d", "xsk", "abc", "", "", conj);
  return marked(std::move(p));
}

// ---------------------------------------------------------------------------------------------------------------
// Launch plans of the contraction kernel (mpse_gemm.hip): everything its launchers decide from sizes and flags alone -
// pure integer arithmetic, so the policy is checked on a CPU (tests/test_gemm_plan_host.py).  64 x 64 output tiles,
// K tiles of 16.

// Unsplit products without a sorted order, from 64 tiles on: a die owns whole tile rows (1) or tile columns (2) of
// the larger operand (size_a, size_b: doubles per unit of K), where their number divides among the eight dies; 0: off
inline int die_group_rule(long long ntile, int tiles_m, int tiles_n, double size_a, double size_b) {
  if (ntile < 64) return 0;
  if (size_a >= size_b && tiles_m % 8 == 0) return 1;
  if (tiles_n % 8 == 0) return 2;
  return tiles_m % 8 == 0 ? 1 : 0;
}
// A launch order by weight (k_tile_order) pays for block-sparse products with more workgroups than two per compute
// unit (`always`: halved tiles are paired through it whatever their number); the sort holds 2048 tiles.
inline bool order_pays(long long ntile, long long nwg, int n_cu, bool always = false) {
  return (always || nwg > 2LL * n_cu) && ntile <= 2048;
}

struct GemmShape {         // a plain product as launch_plan sees it; M, N, batch > 0
  long long M, N, K, batch;
  int n_cu;
  bool ca, cb;             // complex operands
  int skip_hint;           // bit 0 / bit 1: skip the structurally zero tiles of A / B
  bool k_single;           // both K maps are single level
  bool fast_ok;            // non-negative strides and operand spans below 4 GB (what the fast kernel addresses)
  bool dot;                // the caller wants sum conj(C) . y as partials, with room for dot_cap of them
  long long dot_cap;
  bool slices;             // the caller offers to add the K slices itself (compact result, alpha = 1), slices_cap bytes
  unsigned long long slices_cap;
  bool use_beta;
};
struct GemmPlan {
  int tiles_m, tiles_n, nkt;
  int ksplit, kt_per_split;    // K slices (1 = none), K tiles per slice
  unsigned long long ws_bytes; // partial sums of a split product
  bool leave_slices;           // ... stay in the caller's buffer: no reduction launch
  long long nwg;               // workgroups
  bool fast, wide;             // single-level kernel; its eight-wave form
  bool masks;                  // occupancy masks are used, nkw 64-bit words of 8 flags per tile row
  int nkw;
  bool order;                  // launch order by weight
  int die_group;
  long long rgx, rgy;          // reduction grid of a split product
  long long dot_producers;     // workgroups that store a dot partial; 0: the request is not taken
};
inline GemmPlan launch_plan(const GemmShape& s) {
  GemmPlan p{};
  p.tiles_m = int((s.M + 63) / 64), p.tiles_n = int((s.N + 63) / 64), p.nkt = int((s.K + 15) / 16);
  const long long ntile = (long long)p.tiles_m * p.tiles_n, base = ntile * s.batch;
  p.ksplit = 1;
  p.kt_per_split = p.nkt > 0 ? p.nkt : 1;
  // split-K when the output tiles alone cannot fill the compute units (skinny results with long K)
  if (base < s.n_cu && p.nkt >= 4) {
    // fewer output tiles than CUs: slice K until ~1 workgroup per CU exists (policy sweeps of the headline run,
    // DESIGN.md 4.1.  2 per CU: equal to 1.7 % slower depending on the box - the reduction pass reads twice the
    // slices; 3 per CU: -3 %; 0.5 per CU: -7 %).  (One tile per CU runs as fast unsplit as split in two + reduction
    // pass since the K loop prefetches fragments: measured, 4096x256 C-step.)
    const long long want = (s.n_cu + base - 1) / base, maxs = p.nkt / 2;   // at least two K tiles per slice
    const int S = int(want < maxs ? want : maxs);
    if (S > 1) {
      p.kt_per_split = (p.nkt + S - 1) / S;
      p.ksplit = (p.nkt + p.kt_per_split - 1) / p.kt_per_split;
      p.ws_bytes = (unsigned long long)s.batch * p.ksplit * s.M * s.N * ((s.ca || s.cb) ? 16 : 8);
      // (Leaving the slices to the consumer of a matvec result - the Lanczos update adding them while it reads -
      // instead of the reduction launch measured 1.4 % slower on the headline run: every slice's workgroups then load
      // the dot partner, and the update kernel streams 16 slices with a fraction of the reduction kernel's blocks.)
      p.leave_slices = s.slices && !s.dot && s.batch == 1 && !s.use_beta && p.ws_bytes <= s.slices_cap;
    }
  }
  p.nwg = base * p.ksplit;
  p.rgx = (s.N + 255) / 256 > 64 ? 64 : (s.N + 255) / 256;
  p.rgy = s.M * s.batch > 32768 ? 32768 : s.M * s.batch;
  if (s.dot && s.batch == 1) {
    // the kernel that stores the final values forms the partials: the product's workgroups, or the reduction's
    long long producers = base;
    if (p.ksplit > 1) {
      const long long cap_y = s.dot_cap / p.rgx;
      if (cap_y >= 1 && p.rgy > cap_y) p.rgy = cap_y;
      producers = p.rgx * p.rgy;
    }
    if (producers >= 1 && producers <= s.dot_cap) p.dot_producers = producers;
  }
  p.masks = (s.skip_hint & 3) && s.k_single && p.nkt >= 2 && s.batch <= 16384;
  p.nkw = p.masks ? (p.nkt + 7) / 8 : 0;
  p.order = s.batch == 1 && p.masks && order_pays(ntile, ntile * p.ksplit, s.n_cu);
  if (!p.order && p.ksplit == 1 && s.batch == 1)
    p.die_group = die_group_rule(ntile, p.tiles_m, p.tiles_n, double(s.M) * (s.ca ? 2 : 1), double(s.N) * (s.cb ? 2 : 1));
  p.fast = s.k_single && s.fast_ok;
  // one workgroup per compute unit (or fewer): eight waves on the tile instead of four
  p.wide = p.fast && p.nwg <= s.n_cu && p.nkt >= 2;
  return p;
}

// Result tiles of the products with R against the structural mask of the centre.  The result is the centre's layout:
// rows a, columns (sigma, l), row length d * Dr; mask byte [(column / 64) * pitch + a / 16], zero = nothing of that
// 16 x 64 block is ever read.  The product's own tile (tm, tn) covers rows (a, sigma) in [64 tm, 64 tm + 64) of its M
// rows and columns l in [64 tn, 64 tn + 64): it is live when any byte it touches is set.  Any d: a tile may hold several
// a (also across a 16-row boundary of the mask) or a part of one.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool out_tile_live(const unsigned char* mask, int pitch, int d, int Dr, int M, int tm, int tn) {
  const int r1 = 64 * tm + 64 < M ? 64 * tm + 64 : M, l0 = 64 * tn, l1 = 64 * tn + 63 < Dr - 1 ? 64 * tn + 63 : Dr - 1;
  for (int r = 64 * tm; r < r1; ++r) {
    const int a = r / d, sg = r - a * d;
    for (int ct = (sg * Dr + l0) >> 6; ct <= (sg * Dr + l1) >> 6; ++ct)
      if (mask[(long long)ct * pitch + (a >> 4)]) return true;
  }
  return false;
}

// Grouped launch: ngrp groups of M rows each, complex second operand, nkt_max = K tiles of the longest group.
struct GroupedPlan {
  int tiles_m, tiles_n, nkw, die_group;
  bool order, wide;
  long long nwg;
};
// out_mask: the launch would leave the result tiles outside the caller's mask unwritten (out_tile_live) - which tiles
// those are is recorded with the launch order, so such a launch is ordered whatever its size
inline GroupedPlan grouped_plan(long long M, long long N, int ngrp, int nkt_max, bool any_mask, bool split2, bool ca,
                                int n_cu, bool out_mask = false) {
  GroupedPlan p{};
  p.tiles_m = int((M + 63) / 64) * ngrp, p.tiles_n = int((N + 63) / 64);
  const long long ntile = (long long)p.tiles_m * p.tiles_n;
  p.nwg = ntile * (split2 ? 2 : 1);
  p.nkw = (any_mask && (nkt_max + 7) / 8 <= 64) ? (nkt_max + 7) / 8 : 0;   // (a tile's flag words must fit its LDS copy)
  // products with more tiles than slots (heaviest first, die aware), and halved products (their position -> (tile,
  // half) map pairs heavy and light halves per compute unit through the order; plain sorted order)
  p.order = p.nkw > 0 && order_pays(ntile, ntile, n_cu, split2 || out_mask);
  if (!p.order) p.die_group = die_group_rule(ntile, p.tiles_m, p.tiles_n, double(M) * ngrp * (ca ? 2 : 1), double(N) * 2);
  p.wide = p.nwg <= n_cu;
  return p;
}

}  // namespace mpse_plan
