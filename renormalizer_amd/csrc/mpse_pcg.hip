// Preconditioned conjugate gradients on the projected centre problem, vectors and decision resident on the device:
// replaces the scipy.sparse.linalg.cg call of cv/zerot.py:231-290 (a Python closure per matvec on host vectors).
//
//   A v = mask * (Heff v) + shift * v          (Heff: mpse_heff_apply, or mpse_heff_apply2 for the (H - omega)^2 form)
//   z   = r / diag                             (diag == NULL: z = r)
//
// One iteration is the matvec plus three vector launches:
//   k_pcg_q     q = mask * y + shift * p, partial sums of p^H q
//   k_pcg_step  alpha = (r^H z) / (p^H q) from the partials; x += alpha p; r -= alpha q; partial sums of r^H z, r^H r
//               (z = r / diag formed on the fly, never stored) and of b^H x, r^H x for the functional
//   k_pcg_dir   beta from the partials; p = z + beta p; workgroup 0 takes the decision (tolerance, iteration limit)
//               and, at the iterations the host waits for, copies the control block to its pinned mirror
// Every consumer re-sums the producer's per-block partials in the same order (sum_partials, mpse_device.h), so all
// workgroups of a launch agree bitwise on alpha, beta and on a non-positive curvature, and no scalar leaves the device
// between iterations.  Once PcgCtl::done is raised every later launch of the solve returns at once (the contractions of
// the matvec through SolveScope::skip): x is final at the deciding iteration whatever the host has enqueued since.
#include <cmath>

#include "mpse_cx.h"
#include "mpse_device.h"
#include "mpse_internal.h"

namespace {

constexpr int PCG_K = 4;        // the host reads the pinned control block every PCG_K iterations: at most PCG_K - 1
                                // matvecs are enqueued past the decision

enum { PCG_WHY_NONE = 0, PCG_WHY_TOL = 1, PCG_WHY_MAXITER = 2, PCG_WHY_CURVATURE = 3, PCG_WHY_DIAG = 4, PCG_WHY_ZERO_B = 5 };

struct PcgCtl {
  int done;        // decision has fallen: later launches do nothing
  int status;      // MPSE_OK / MPSE_ERR_NOCONV / MPSE_ERR_ARG
  int iters;       // iterations behind the x that is returned
  int why;         // PCG_WHY_*
  double relres2;  // |r|^2 / |b|^2 of that x
  double lvalue;   // Re(x^H A x) - 2 Re(b^H x) = -Re(b^H x) - Re(r^H x) with r = b - A x
  double bb;       // |mask * b|^2
  double pad[3];
};
static_assert(sizeof(PcgCtl) == 8 * sizeof(double), "control block = 8 doubles");
constexpr int PCG_CW = int(sizeof(PcgCtl) / sizeof(double));

__device__ __forceinline__ void pcg_publish(const PcgCtl* ctl, double* pub, volatile double* seq_slot, double seq) {
  const double* src = reinterpret_cast<const double*>(ctl);
  for (int i = 0; i < PCG_CW; ++i) pub[i] = src[i];
  __threadfence_system();
  *seq_slot = seq;
  __threadfence_system();
}

__device__ __forceinline__ double2 scale2(double2 v, double s) { return make_double2(v.x * s, v.y * s); }
__device__ __forceinline__ double re_dotc(double2 a, double2 b) { return a.x * b.x + a.y * b.y; }   // Re conj(a) b

// Entry: clears the control block, masks the start vector in place, partial sums of |mask * b|^2 and the number of
// diagonal entries that are not positive (second slot of the pair).
template <bool CPLX>
__device__ __forceinline__ void pcg_prep_body(double* __restrict__ x, const double* __restrict__ b,
                                              const double* __restrict__ mask, const double* __restrict__ diag,
                                              long long n, double* __restrict__ part_bb, PcgCtl* ctl) {
  if (blockIdx.x == 0 && threadIdx.x < PCG_CW) reinterpret_cast<double*>(ctl)[threadIdx.x] = 0.0;
  double bb = 0, bad = 0;
  const long long stride = (long long)gridDim.x * RED_THREADS;
  for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) {
    const double m = mask ? mask[i] : 1.0;
    const double2 bv = scale2(Cx<CPLX>::ld(b, i), m);
    bb += re_dotc(bv, bv);
    if (mask) Cx<CPLX>::st(x, i, scale2(Cx<CPLX>::ld(x, i), m));
    if (diag && !(diag[i] > 0.0)) bad += 1.0;
  }
  block_allsum2(bb, bad);
  if (threadIdx.x == 0) {
    part_bb[2 * blockIdx.x] = bb;
    part_bb[2 * blockIdx.x + 1] = bad;
  }
}
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_prep(double* __restrict__ x, const double* __restrict__ b,
                                                          const double* __restrict__ mask,
                                                          const double* __restrict__ diag, long long n,
                                                          double* __restrict__ part_bb, PcgCtl* ctl) {
  pcg_prep_body<CPLX>(x, b, mask, diag, n, part_bb, ctl);
}

// r = b - A x0 from y = Heff x0, p = z = r / diag; partial sums (r^H z, r^H r) and (b^H x, r^H x).  A right-hand side
// that vanishes under the mask ends the solve here with x = 0; a diagonal entry that is not positive with MPSE_ERR_ARG.
template <bool CPLX>
__device__ __forceinline__ void pcg_start_body(const double* __restrict__ y, const double* __restrict__ b,
                                               const double* __restrict__ mask, const double* __restrict__ diag,
                                               double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                               double shift, long long n, const double* __restrict__ part_bb, int nb,
                                               double* __restrict__ part_rz, double* __restrict__ part_bx, PcgCtl* ctl) {
  double bb, bad;
  sum_partials(part_bb, nb, bb, bad);
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  const long long stride = (long long)gridDim.x * RED_THREADS;
  if (bad > 0.0) {
    if (lead) ctl->done = 1, ctl->status = MPSE_ERR_ARG, ctl->why = PCG_WHY_DIAG;
    return;
  }
  if (bb == 0.0) {
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride)
      Cx<CPLX>::st(x, i, make_double2(0.0, 0.0));
    if (lead) ctl->done = 1, ctl->status = MPSE_OK, ctl->why = PCG_WHY_ZERO_B;
    return;
  }
  if (lead) ctl->bb = bb;
  double rz = 0, rr = 0, bx = 0, rx = 0;
  for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) {
    const double m = mask ? mask[i] : 1.0;
    const double2 bv = scale2(Cx<CPLX>::ld(b, i), m), yv = Cx<CPLX>::ld(y, i), xv = Cx<CPLX>::ld(x, i);
    const double2 rv = make_double2(bv.x - (m * yv.x + shift * xv.x), bv.y - (m * yv.y + shift * xv.y));
    const double2 zv = diag ? scale2(rv, 1.0 / diag[i]) : rv;
    Cx<CPLX>::st(r, i, rv);
    Cx<CPLX>::st(p, i, zv);
    rz += re_dotc(rv, zv);
    rr += re_dotc(rv, rv);
    bx += re_dotc(bv, xv);
    rx += re_dotc(rv, xv);
  }
  block_allsum2(rz, rr);
  block_allsum2(bx, rx);
  if (threadIdx.x == 0) {
    part_rz[2 * blockIdx.x] = rz;
    part_rz[2 * blockIdx.x + 1] = rr;
    part_bx[2 * blockIdx.x] = bx;
    part_bx[2 * blockIdx.x + 1] = rx;
  }
}
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_start(const double* __restrict__ y, const double* __restrict__ b,
                                                           const double* __restrict__ mask,
                                                           const double* __restrict__ diag, double* __restrict__ x,
                                                           double* __restrict__ r, double* __restrict__ p,
                                                           double shift, long long n,
                                                           const double* __restrict__ part_bb, int nb,
                                                           double* __restrict__ part_rz, double* __restrict__ part_bx,
                                                           PcgCtl* ctl) {
  pcg_start_body<CPLX>(y, b, mask, diag, x, r, p, shift, n, part_bb, nb, part_rz, part_bx, ctl);
}

// (a) q = mask * y + shift * p with y = Heff p; partial sums of p^H q (real for a Hermitian operator: the real part is kept)
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_q(const double* __restrict__ y, const double* __restrict__ p,
                                                       const double* __restrict__ mask, double shift,
                                                       double* __restrict__ q, long long n,
                                                       double* __restrict__ part_pq, const PcgCtl* __restrict__ ctl) {
  if (ctl->done) return;
  double pq = 0, zero = 0;
  const long long stride = (long long)gridDim.x * RED_THREADS;
  for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) {
    const double m = mask ? mask[i] : 1.0;
    const double2 yv = Cx<CPLX>::ld(y, i), pv = Cx<CPLX>::ld(p, i);
    const double2 qv = make_double2(m * yv.x + shift * pv.x, m * yv.y + shift * pv.y);
    Cx<CPLX>::st(q, i, qv);
    pq += re_dotc(pv, qv);
  }
  block_allsum2(pq, zero);
  if (threadIdx.x == 0) {
    part_pq[2 * blockIdx.x] = pq;
    part_pq[2 * blockIdx.x + 1] = 0.0;
  }
}

// (a) for a weighted sum of operators: q = mask * (sum_t w_t y_t) + shift * p from the results of all terms in ONE pass,
// where accumulating products (beta = 1) would tie the bits of q to how the contraction kernel splits its K loop and a
// pass per term would read and write the vectors three times over.  The partial sums are those of k_pcg_q.
struct PcgTerms {
  const double* y[4];
  double w[4];
  int n;
};
template <bool CPLX>
__device__ __forceinline__ double2 pcg_term_sum(const PcgTerms& t, long long i) {
  double2 s = scale2(Cx<CPLX>::ld(t.y[0], i), t.w[0]);
  for (int k = 1; k < t.n; ++k) {
    const double2 v = Cx<CPLX>::ld(t.y[k], i);
    s.x += t.w[k] * v.x, s.y += t.w[k] * v.y;
  }
  return s;
}
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_q_sum(const PcgTerms t, const double* __restrict__ p,
                                                           const double* __restrict__ mask, double shift,
                                                           double* __restrict__ q, long long n,
                                                           double* __restrict__ part_pq, const PcgCtl* __restrict__ ctl) {
  if (ctl->done) return;
  double pq = 0, zero = 0;
  const long long stride = (long long)gridDim.x * RED_THREADS;
  for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) {
    const double m = mask ? mask[i] : 1.0;
    const double2 yv = pcg_term_sum<CPLX>(t, i), pv = Cx<CPLX>::ld(p, i);
    const double2 qv = make_double2(m * yv.x + shift * pv.x, m * yv.y + shift * pv.y);
    Cx<CPLX>::st(q, i, qv);
    pq += re_dotc(pv, qv);
  }
  block_allsum2(pq, zero);
  if (threadIdx.x == 0) {
    part_pq[2 * blockIdx.x] = pq;
    part_pq[2 * blockIdx.x + 1] = 0.0;
  }
}
// the same sum written into the first term's vector: the start residual (once per solve) goes through k_pcg_start
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_combine(const PcgTerms t, double* y, long long n) {
  const long long stride = (long long)gridDim.x * RED_THREADS;
  for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride)
    Cx<CPLX>::st(y, i, pcg_term_sum<CPLX>(t, i));
}

// (b) alpha = (r^H z) / (p^H q); x += alpha p; r -= alpha q; partial sums for the next beta, the residual test and the
// functional.  part_cur holds the (r^H z, r^H r) of the residual this step starts from, part_new receives the new ones
// (another area: workgroups read all of part_cur while others already write).  A curvature p^H q that is not positive
// (operator not positive definite, or NaN) ends the solve: every workgroup sees the same sum and leaves x alone.
// (nbq: the number of p^H q partials - those of k_pcg_q, or one per workgroup of the one-launch two-layer matvec)
template <bool CPLX>
__device__ __forceinline__ void pcg_step_body(const double* __restrict__ p, const double* __restrict__ q,
                                              const double* __restrict__ b, const double* __restrict__ mask,
                                              const double* __restrict__ diag, double* __restrict__ x,
                                              double* __restrict__ r, long long n, const double* __restrict__ part_pq,
                                              int nbq, const double* __restrict__ part_cur,
                                              double* __restrict__ part_new, double* __restrict__ part_bx, int nb,
                                              PcgCtl* ctl) {
  // (a workgroup that starts after workgroup 0 has raised `done` for the curvature below leaves here instead of through
  // its own test of p^H q: the same outcome, x and r untouched)
  if (ctl->done) return;
  // the first element of this thread is requested before the scalars are summed: its loads do not depend on them, and
  // the block reductions otherwise stand in front of every trip to memory (as k_lanczos_update_u does)
  const long long stride = (long long)gridDim.x * RED_THREADS;
  const long long i0 = (long long)blockIdx.x * RED_THREADS + threadIdx.x;
  struct Elem {
    double2 p, q, x, r, b;
    double d;
  };
  auto fetch = [&](long long i) {
    Elem e;
    e.p = Cx<CPLX>::ld(p, i), e.q = Cx<CPLX>::ld(q, i), e.x = Cx<CPLX>::ld(x, i), e.r = Cx<CPLX>::ld(r, i);
    e.b = scale2(Cx<CPLX>::ld(b, i), mask ? mask[i] : 1.0);
    e.d = diag ? diag[i] : 1.0;
    return e;
  };
  Elem first;
  if (i0 < n) first = fetch(i0);
  asm volatile("" ::: "memory");
  double pq, rz_cur, t0, t1;
  sum_partials(part_pq, nbq, pq, t0);
  sum_partials(part_cur, nb, rz_cur, t1);
  if (!(pq > 0.0)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->done = 1, ctl->status = MPSE_ERR_ARG, ctl->why = PCG_WHY_CURVATURE;
    return;
  }
  const double alpha = rz_cur / pq;
  double rz = 0, rr = 0, bx = 0, rx = 0;
  for (long long i = i0; i < n; i += stride) {
    const Elem e = i == i0 ? first : fetch(i);
    const double2 xv = make_double2(e.x.x + alpha * e.p.x, e.x.y + alpha * e.p.y);
    const double2 rv = make_double2(e.r.x - alpha * e.q.x, e.r.y - alpha * e.q.y);
    const double2 zv = diag ? scale2(rv, 1.0 / e.d) : rv;
    Cx<CPLX>::st(x, i, xv);
    Cx<CPLX>::st(r, i, rv);
    rz += re_dotc(rv, zv);
    rr += re_dotc(rv, rv);
    bx += re_dotc(e.b, xv);
    rx += re_dotc(rv, xv);
  }
  block_allsum2(rz, rr);
  block_allsum2(bx, rx);
  if (threadIdx.x == 0) {
    part_new[2 * blockIdx.x] = rz;
    part_new[2 * blockIdx.x + 1] = rr;
    part_bx[2 * blockIdx.x] = bx;
    part_bx[2 * blockIdx.x + 1] = rx;
  }
}
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_step(const double* __restrict__ p, const double* __restrict__ q,
                                                          const double* __restrict__ b,
                                                          const double* __restrict__ mask,
                                                          const double* __restrict__ diag, double* __restrict__ x,
                                                          double* __restrict__ r, long long n,
                                                          const double* __restrict__ part_pq,
                                                          const double* __restrict__ part_cur,
                                                          double* __restrict__ part_new, double* __restrict__ part_bx,
                                                          int nb, PcgCtl* ctl) {
  pcg_step_body<CPLX>(p, q, b, mask, diag, x, r, n, part_pq, nb, part_cur, part_new, part_bx, nb, ctl);
}

// (c) after k iterations: beta = (r^H z)_new / (r^H z)_old, p = z + beta p (k == 0: p = z stands from k_pcg_start);
// workgroup 0 decides - |r|^2 <= tol^2 |b|^2, then the iteration limit - and publishes the control block when the host
// waits at this iteration (pub != null), also when the decision fell earlier.
template <bool CPLX>
__device__ __forceinline__ void pcg_dir_body(const double* __restrict__ r, const double* __restrict__ diag,
                                             double* __restrict__ p, long long n, const double* __restrict__ part_new,
                                             const double* __restrict__ part_old, const double* __restrict__ part_bx,
                                             int nb, double tol2, int k, int max_iter, PcgCtl* ctl, double* pub,
                                             volatile double* seq_slot, double seq) {
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  // Workgroup 0 raises `done` inside this launch, possibly before other workgroups have started: those leave here and
  // skip their part of p = z + beta p.  That is harmless because p is never read again once `done` is set (every later
  // launch returns at its top), and this kernel writes neither x nor r: the returned x does not depend on the race.
  if (ctl->done) {
    if (pub && lead) pcg_publish(ctl, pub, seq_slot, seq);
    return;
  }
  double rz_new, rr;
  sum_partials(part_new, nb, rz_new, rr);
  if (k > 0) {
    double rz_old, t;
    sum_partials(part_old, nb, rz_old, t);
    const double beta = rz_new / rz_old;
    const long long stride = (long long)gridDim.x * RED_THREADS;
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) {
      const double2 rv = Cx<CPLX>::ld(r, i), pv = Cx<CPLX>::ld(p, i);
      const double2 zv = diag ? scale2(rv, 1.0 / diag[i]) : rv;
      Cx<CPLX>::st(p, i, make_double2(zv.x + beta * pv.x, zv.y + beta * pv.y));
    }
  }
  if (blockIdx.x != 0) return;
  const double bb = ctl->bb;
  const bool conv = rr <= tol2 * bb;
  const bool stop = conv || k >= max_iter;     // (uniform over the workgroup: every thread holds the same sums)
  double bx = 0, rx = 0;
  if (stop) sum_partials(part_bx, nb, bx, rx);
  if (lead) {
    ctl->iters = k;
    ctl->relres2 = rr / bb;
    if (stop) {
      ctl->lvalue = -bx - rx;
      ctl->status = conv ? MPSE_OK : MPSE_ERR_NOCONV;
      ctl->why = conv ? PCG_WHY_TOL : PCG_WHY_MAXITER;
      ctl->done = 1;
    }
    if (pub) pcg_publish(ctl, pub, seq_slot, seq);
  }
}
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_dir(const double* __restrict__ r, const double* __restrict__ diag,
                                                         double* __restrict__ p, long long n,
                                                         const double* __restrict__ part_new,
                                                         const double* __restrict__ part_old,
                                                         const double* __restrict__ part_bx, int nb, double tol2, int k,
                                                         int max_iter, PcgCtl* ctl, double* pub,
                                                         volatile double* seq_slot, double seq) {
  pcg_dir_body<CPLX>(r, diag, p, n, part_new, part_old, part_bx, nb, tol2, k, max_iter, ctl, pub, seq_slot, seq);
}

// ---- batched forms (mpse_pcg_batch): member blockIdx.z of a launch set runs the bodies above on its own vectors,
// partials and control block from the member table, with the grid its single launch would have: what a member computes
// does not depend on the others
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_prep_b(const Pcg2Member* __restrict__ mem, long long n) {
  const Pcg2Member mb = mem[blockIdx.z];
  pcg_prep_body<CPLX>(mb.x, mb.b, mb.mask, mb.diag, n, mb.part_bb, static_cast<PcgCtl*>(mb.ctl));
}
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_start_b(const Pcg2Member* __restrict__ mem, long long n, int nb) {
  const Pcg2Member mb = mem[blockIdx.z];
  pcg_start_body<CPLX>(mb.y, mb.b, mb.mask, mb.diag, mb.x, mb.r, mb.p, mb.shift, n, mb.part_bb, nb, mb.part_rz0,
                       mb.part_bx, static_cast<PcgCtl*>(mb.ctl));
}
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_step_b(const Pcg2Member* __restrict__ mem, long long n, int nbq,
                                                            int nb, int k) {
  const Pcg2Member mb = mem[blockIdx.z];
  pcg_step_body<CPLX>(mb.p, mb.q, mb.b, mb.mask, mb.diag, mb.x, mb.r, n, mb.part_pq, nbq,
                      (k - 1) & 1 ? mb.part_rz1 : mb.part_rz0, k & 1 ? mb.part_rz1 : mb.part_rz0, mb.part_bx, nb,
                      static_cast<PcgCtl*>(mb.ctl));
}
template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_dir_b(const Pcg2Member* __restrict__ mem, long long n, int nb,
                                                           double tol2, int k, int max_iter) {
  const Pcg2Member mb = mem[blockIdx.z];
  pcg_dir_body<CPLX>(mb.r, mb.diag, mb.p, n, k & 1 ? mb.part_rz1 : mb.part_rz0, (k + 1) & 1 ? mb.part_rz1 : mb.part_rz0,
                     mb.part_bx, nb, tol2, k, max_iter, static_cast<PcgCtl*>(mb.ctl), nullptr, nullptr, 0.0);
}
// the control blocks of all members to the pinned mirror, then the sequence number (one workgroup, after k_pcg_dir_b)
__global__ __launch_bounds__(RED_THREADS) void k_pcg_publish_b(const Pcg2Member* __restrict__ mem, int B, double* pub,
                                                               volatile double* seq_slot, double seq) {
  for (int i = threadIdx.x; i < B * PCG_CW; i += RED_THREADS)
    pub[i] = static_cast<const double*>(mem[i / PCG_CW].ctl)[i % PCG_CW];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    *seq_slot = seq;
    __threadfence_system();
  }
}

template <bool CPLX>
int pcg_run(mpse_ctx* ctx, int dtype, const mpse_heff* h, int twolayer, double shift, const double* diag,
            const double* mask, const double* b, double* x, double tol, int max_iter, int64_t n, PcgCtl* hc,
            int nterms = 0, const mpse_heff_ft* terms = nullptr, const double* weights = nullptr) {
  const size_t es = dtype_size(dtype);
  const int64_t nd = n * (CPLX ? 2 : 1);
  const int nb = red_blocks(nd);
  // one slab: control block, five areas of partials (|b|^2; p^H q; r^H z twice, by iteration parity; b^H x), then y, q, r, p
  // (a summed solve: one more y per further term, behind p)
  const size_t head = size_t(PCG_CW + 5 * 2 * nb) * sizeof(double);
  const size_t head_al = (head + 255) & ~size_t(255);
  TmpBuf slab(ctx);
  MPSE_TRY(slab.alloc(head_al + (4 + size_t(nterms > 1 ? nterms - 1 : 0)) * size_t(n) * es));
  PcgCtl* ctl = slab.as<PcgCtl>();
  double* part = slab.as<double>() + PCG_CW;
  double *part_bb = part, *part_pq = part + 2 * nb, *part_bx = part + 4 * nb;
  double* part_rz[2] = {part + 6 * nb, part + 8 * nb};
  char* vecs = slab.as<char>() + head_al;
  double* y = reinterpret_cast<double*>(vecs);
  double* q = reinterpret_cast<double*>(vecs + size_t(n) * es);
  double* r = reinterpret_cast<double*>(vecs + 2 * size_t(n) * es);
  double* p = reinterpret_cast<double*>(vecs + 3 * size_t(n) * es);

  SolveScope scope(ctx);
  scope.skip = &ctl->done;
  // a single term of weight one is the plain solve on that term's result
  const bool summed = nterms > 1 || (nterms == 1 && weights[0] != 1.0);
  PcgTerms ts;
  memset(&ts, 0, sizeof(ts));
  ts.n = nterms;
  for (int t = 0; t < nterms; ++t) {
    ts.y[t] = t == 0 ? y : reinterpret_cast<double*>(vecs + (3 + size_t(t)) * size_t(n) * es);
    ts.w[t] = weights[t];
  }
  auto matvec = [&](const void* in) -> int {
    if (nterms > 0) {
      for (int t = 0; t < nterms; ++t)
        MPSE_TRY(heff_apply_ft(ctx, dtype, &terms[t], in, const_cast<double*>(ts.y[t]), &scope));
      return MPSE_OK;
    }
    return twolayer ? heff_apply2(ctx, dtype, h, in, y, &scope) : heff_apply(ctx, dtype, h, in, y, &scope, nullptr);
  };
  const dim3 grid(nb), block(RED_THREADS);
  const long long nn = (long long)n;
  const double tol2 = tol * tol;
  memset(hc, 0, sizeof(*hc));

  hipLaunchKernelGGL(k_pcg_prep<CPLX>, grid, block, 0, ctx->stream, x, b, mask, diag, nn, part_bb, ctl);
  MPSE_HIP(ctx, hipGetLastError());
  MPSE_TRY(matvec(x));
  if (summed) {
    hipLaunchKernelGGL(k_pcg_combine<CPLX>, grid, block, 0, ctx->stream, ts, y, nn);
    MPSE_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(k_pcg_start<CPLX>, grid, block, 0, ctx->stream, (const double*)y, b, mask, diag, x, r, p, shift, nn,
                     (const double*)part_bb, nb, part_rz[0], part_bx, ctl);
  MPSE_HIP(ctx, hipGetLastError());
  for (int k = 0;; ++k) {
    if (k > 0) {
      MPSE_TRY(matvec(p));
      ++ctx->pcg_stats[mpse_ctx::PS_MATVECS];
      ctx->pcg_sum_stats[mpse_ctx::PSS_TERM_APPLIES] += nterms;
      if (summed)
        hipLaunchKernelGGL(k_pcg_q_sum<CPLX>, grid, block, 0, ctx->stream, ts, (const double*)p, mask, shift, q, nn,
                           part_pq, (const PcgCtl*)ctl);
      else
        hipLaunchKernelGGL(k_pcg_q<CPLX>, grid, block, 0, ctx->stream, (const double*)y, (const double*)p, mask, shift, q,
                           nn, part_pq, (const PcgCtl*)ctl);
      MPSE_HIP(ctx, hipGetLastError());
      hipLaunchKernelGGL(k_pcg_step<CPLX>, grid, block, 0, ctx->stream, (const double*)p, (const double*)q, b, mask, diag,
                         x, r, nn, (const double*)part_pq, (const double*)part_rz[(k - 1) & 1], part_rz[k & 1], part_bx,
                         nb, ctl);
      MPSE_HIP(ctx, hipGetLastError());
    }
    const bool wait_here = (k % PCG_K == PCG_K - 1) || k >= max_iter;
    const PublishAt at = publish_target(ctx, wait_here, mpse_ctx::PIN_PCG_CTL);
    hipLaunchKernelGGL(k_pcg_dir<CPLX>, grid, block, 0, ctx->stream, (const double*)r, diag, p, nn,
                       (const double*)part_rz[k & 1], (const double*)part_rz[(k + 1) & 1], (const double*)part_bx, nb,
                       tol2, k, max_iter, ctl, at.pub, at.seq_slot, at.seq);
    MPSE_HIP(ctx, hipGetLastError());
    if (wait_here) {
      // the control block that this k_pcg_dir published, or a copy of it
      MPSE_TRY(publish_collect(ctx, at, ctl, 0, 1, PCG_CW, mpse_ctx::PIN_PCG_CTL, hc));
      ++ctx->pcg_stats[mpse_ctx::PS_WAITS];
      if (nterms > 0) ++ctx->pcg_sum_stats[mpse_ctx::PSS_WAITS];
      if (hc->done) break;
      if (k >= max_iter) return mpse_fail(ctx, MPSE_ERR_HIP, "pcg: no decision at the iteration limit");
    }
  }
  return MPSE_OK;
}
template <class... A>
int pcg_run_dtype(mpse_ctx* ctx, int dtype, A... a) {
  return dtype == MPSE_C128 ? pcg_run<true>(ctx, dtype, a...) : pcg_run<false>(ctx, dtype, a...);
}

// ---- preconditioner of the summed solve: the diagonal of each term from the environment diagonals and a per-site factor
// element of an MPO site W (wl, d, d, wr) that takes leg value `in` to `out` under the layer's transposition flag
__device__ __forceinline__ double ft_w_elem(const double* W, int trans, long long d, long long wr, long long b, long long in,
                                            long long out, long long f) {
  return trans ? W[((b * d + in) * d + out) * wr + f] : W[((b * d + out) * d + in) * wr + f];
}

struct FtShape {
  long long Dl, Dr, du, dv, wl1, wr1, wl2, wr2;
  int leg1, leg2, trans1, trans2;
};

// S[b, c, u, v, g, i]: both layers on one leg: sum_x W1(leg -> x)[b, g] W2(x -> leg)[c, i]; one per leg: the two diagonals
__global__ __launch_bounds__(256) void k_site_factor_ft(const FtShape h, const double* __restrict__ W1,
                                                        const double* __restrict__ W2, double* __restrict__ S) {
  const long long total = h.wl1 * h.wl2 * h.du * h.dv * h.wr1 * h.wr2;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  long long r = idx;
  const long long i = r % h.wr2; r /= h.wr2;
  const long long g = r % h.wr1; r /= h.wr1;
  const long long v = r % h.dv; r /= h.dv;
  const long long u = r % h.du; r /= h.du;
  const long long c = r % h.wl2;
  const long long b = r / h.wl2;
  double acc = 0.0;
  if (h.leg1 == h.leg2) {
    const long long d = h.leg1 == MPSE_LEG_UP ? h.du : h.dv, e = h.leg1 == MPSE_LEG_UP ? u : v;
    for (long long x = 0; x < d; ++x)
      acc += ft_w_elem(W1, h.trans1, d, h.wr1, b, e, x, g) * ft_w_elem(W2, h.trans2, d, h.wr2, c, x, e, i);
  } else {
    acc = ft_w_elem(W1, h.trans1, h.du, h.wr1, b, u, u, g) * ft_w_elem(W2, h.trans2, h.dv, h.wr2, c, v, v, i);
  }
  S[idx] = acc;
}

// diag[a, u, v, j] (+)= weight * sum_{b, c, g, i} Re(L[a, b, c, a] R[j, g, i, j]) S[b, c, u, v, g, i]; one thread per entry
template <bool LC, bool RC>
__global__ __launch_bounds__(256) void k_diag_ft(const FtShape h, const double* __restrict__ L,
                                                 const double* __restrict__ R, const double* __restrict__ S, double weight,
                                                 double shift, int accumulate, double* __restrict__ diag) {
  const long long total = h.Dl * h.du * h.dv * h.Dr;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  long long r = idx;
  const long long j = r % h.Dr; r /= h.Dr;
  const long long v = r % h.dv; r /= h.dv;
  const long long u = r % h.du;
  const long long a = r / h.du;
  double acc = 0.0;
  for (long long b = 0; b < h.wl1; ++b)
    for (long long c = 0; c < h.wl2; ++c) {
      const long long lo = ((a * h.wl1 + b) * h.wl2 + c) * h.Dl + a;
      const double lr = LC ? L[2 * lo] : L[lo], li = LC ? L[2 * lo + 1] : 0.0;
      for (long long g = 0; g < h.wr1; ++g)
        for (long long i = 0; i < h.wr2; ++i) {
          const long long ro = ((j * h.wr1 + g) * h.wr2 + i) * h.Dr + j;
          const double rr = RC ? R[2 * ro] : R[ro], ri = RC ? R[2 * ro + 1] : 0.0;
          acc += (lr * rr - li * ri) * S[((((b * h.wl2 + c) * h.du + u) * h.dv + v) * h.wr1 + g) * h.wr2 + i];
        }
    }
  diag[idx] = (accumulate ? diag[idx] : shift) + weight * acc;
}

FtShape ft_shape(const mpse_heff_ft& h) {
  return FtShape{h.Dl, h.Dr, h.d_up, h.d_down, h.wl1, h.wr1, h.wl2, h.wr2, h.leg1, h.leg2, h.trans1, h.trans2};
}
int ft_shape_ok(mpse_ctx* ctx, const mpse_heff_ft& h, const char* who) {
  if (h.Dl <= 0 || h.Dr <= 0 || h.d_up <= 0 || h.d_down <= 0 || h.wl1 <= 0 || h.wr1 <= 0 || h.wl2 <= 0 || h.wr2 <= 0)
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "%s: empty extent", who);
  if ((h.leg1 != MPSE_LEG_UP && h.leg1 != MPSE_LEG_DOWN) || (h.leg2 != MPSE_LEG_UP && h.leg2 != MPSE_LEG_DOWN) ||
      (h.leg1 == MPSE_LEG_DOWN && h.leg2 == MPSE_LEG_UP))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "%s: layers act up/up, down/down or up/down", who);
  return MPSE_OK;
}

}  // namespace

// counts a solve that reached its decision and turns the control block into outputs and status
static int pcg_report(mpse_ctx* ctx, const PcgCtl& hc, bool masked, double tol, int* iters_host, double* relres_host,
                      double* lvalue_host) {
  ++ctx->pcg_stats[mpse_ctx::PS_SOLVES];
  if (masked) ++ctx->pcg_stats[mpse_ctx::PS_MASKED];
  ctx->pcg_stats[mpse_ctx::PS_ITERS] += hc.iters;
  if (iters_host) *iters_host = hc.iters;
  if (relres_host) *relres_host = std::sqrt(hc.relres2);
  if (lvalue_host) *lvalue_host = hc.lvalue;
  switch (hc.why) {
    case PCG_WHY_TOL:
    case PCG_WHY_ZERO_B:
      ++ctx->pcg_stats[mpse_ctx::PS_END_TOL];
      return MPSE_OK;
    case PCG_WHY_MAXITER:
      ++ctx->pcg_stats[mpse_ctx::PS_END_MAXITER];
      return mpse_fail(ctx, MPSE_ERR_NOCONV, "pcg: |r| / |b| = %.3e after %d iterations (tol %.3e)", std::sqrt(hc.relres2),
                       hc.iters, tol);
    case PCG_WHY_CURVATURE:
      ++ctx->pcg_stats[mpse_ctx::PS_END_CURVATURE];
      return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: curvature p^H A p <= 0 (or not a number) after %d iterations: the operator "
                       "is not positive definite", hc.iters);
    case PCG_WHY_DIAG:
      return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: the preconditioner diagonal has entries that are not positive");
    default:
      return mpse_fail(ctx, MPSE_ERR_HIP, "pcg: control block without a decision");
  }
}

// ---- mpse_pcg_batch: launch sets of members with one shape that takes the one-launch two-layer matvec
namespace {

constexpr int PCGB_MAX = 32;         // members per launch set
static_assert(mpse_ctx::PIN_BATCH_CTL + PCGB_MAX * PCG_CW < mpse_ctx::PIN_QR_STATUS, "batch slot clear of the QR status word");

// the member's own shape decides: one-site, two layers, square, no ancilla, operands of the working type, real W
bool pcg_batch_eligible(int dtype, const mpse_heff& h, int twolayer, Small2Plan* plan) {
  if (!twolayer || h.nsite != 1) return false;
  const mpse_dims& s = h.dims;
  if ((s.Dl_bra > 0 && s.Dl_bra != s.Dl_ket) || (s.Dr_bra > 0 && s.Dr_bra != s.Dr_ket) || s.danc > 1) return false;
  if (h.l_dtype != dtype || h.r_dtype != dtype || h.w_dtype != MPSE_F64) return false;
  return small2_plan(dtype, s.Dl_ket, s.d0, s.Dr_ket, s.wl, s.wr, plan);
}

struct PcgSet {
  Small2Plan plan;
  std::vector<int> idx;      // member -> position in the caller's arrays
};

int pcg_batch_set(mpse_ctx* ctx, int dtype, const PcgSet& ps, const mpse_heff* hs, const double* shifts,
                  const void* const* diags, const void* const* masks, const void* const* bs, void* const* xs, double tol,
                  int max_iter, std::vector<PcgCtl>& hc) {
  const int B = (int)ps.idx.size();
  const Small2Plan& pl = ps.plan;
  const bool cplx = dtype == MPSE_C128;
  const size_t es = dtype_size(dtype);
  const int64_t n = int64_t(pl.Dl) * pl.d * pl.Dr;
  const int64_t nd = n * (cplx ? 2 : 1);
  const int nb = red_blocks(nd), nbq = pl.Dl;
  // per-member region of the slab (256-byte aligned sections): control block, partials (|b|^2; p^H q; b^H x; r^H z twice),
  // y, q, r, p, the transposed left environment, the sparse W list
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t o_part = al(sizeof(PcgCtl));
  const size_t o_vec = o_part + al(size_t(8 * nb + 2 * nbq) * sizeof(double));
  const size_t vb = al(size_t(n) * es);
  const size_t o_lt = o_vec + 4 * vb;
  const size_t o_ptr = o_lt + al(size_t(pl.Dl) * pl.wl * pl.wl * pl.Dl * es);
  const size_t cap = size_t(pl.rows) * pl.pitch;
  const size_t o_idx = o_ptr + al(size_t(pl.rows + 1) * sizeof(int));
  const size_t o_val = o_idx + al(cap * sizeof(int));
  const size_t ms = o_val + al(cap * sizeof(double));
  TmpBuf SLAB(ctx), MEM(ctx);
  MPSE_TRY(SLAB.alloc(size_t(B) * ms));
  MPSE_TRY(MEM.alloc(size_t(B) * sizeof(Pcg2Member)));
  std::vector<Pcg2Member> mh(B);
  for (int m = 0; m < B; ++m) {
    const int i = ps.idx[m];
    char* base = SLAB.as<char>() + size_t(m) * ms;
    double* part = reinterpret_cast<double*>(base + o_part);
    Pcg2Member& mb = mh[m];
    mb.L = static_cast<const double*>(hs[i].L), mb.R = static_cast<const double*>(hs[i].R);
    mb.W = static_cast<const double*>(hs[i].W0);
    mb.Lt = reinterpret_cast<double*>(base + o_lt);
    mb.csr_ptr = reinterpret_cast<int*>(base + o_ptr), mb.csr_idx = reinterpret_cast<int*>(base + o_idx);
    mb.csr_val = reinterpret_cast<double*>(base + o_val);
    mb.mask = masks ? static_cast<const double*>(masks[i]) : nullptr;
    mb.diag = diags ? static_cast<const double*>(diags[i]) : nullptr;
    mb.b = static_cast<const double*>(bs[i]);
    mb.x = static_cast<double*>(xs[i]);
    mb.y = reinterpret_cast<double*>(base + o_vec), mb.q = reinterpret_cast<double*>(base + o_vec + vb);
    mb.r = reinterpret_cast<double*>(base + o_vec + 2 * vb), mb.p = reinterpret_cast<double*>(base + o_vec + 3 * vb);
    mb.part_bb = part, mb.part_bx = part + 2 * nb, mb.part_rz0 = part + 4 * nb, mb.part_rz1 = part + 6 * nb;
    mb.part_pq = part + 8 * nb;
    mb.ctl = base;
    mb.shift = shifts[i];
    wsite_written(ctx, xs[i], size_t(n) * es);
  }
  MPSE_TRY(stage_h2d(ctx, MEM.p, mh.data(), mh.size() * sizeof(Pcg2Member)));
  const Pcg2Member* mem = MEM.as<const Pcg2Member>();
  const dim3 grid(nb, 1, B), block(RED_THREADS);
  const long long nn = (long long)n;
  const double tol2 = tol * tol;
  if (max_iter <= 0) max_iter = int(10 * n);      // (n <= 64 * 16 * 64)

  MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_prep_b, grid, block, mem, nn);
  MPSE_TRY(small2_prep(ctx, dtype, pl, B, mem));
  MPSE_TRY(small2_apply(ctx, dtype, pl, B, mem, 0));
  MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_start_b, grid, block, mem, nn, nb);
  ++ctx->pcg_batch_stats[mpse_ctx::PB_SETS];
  for (int k = 0;; ++k) {
    if (k > 0) {
      MPSE_TRY(small2_apply(ctx, dtype, pl, B, mem, 1));
      ++ctx->pcg_batch_stats[mpse_ctx::PB_MATVEC_LAUNCHES];
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_step_b, grid, block, mem, nn, nbq, nb, k);
    }
    MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_dir_b, grid, block, mem, nn, nb, tol2, k, max_iter);
    const bool wait_here = (k % PCG_K == PCG_K - 1) || k >= max_iter;
    if (!wait_here) continue;
    const PublishAt at = publish_target(ctx, true, mpse_ctx::PIN_BATCH_CTL);
    if (at.pub) {
      hipLaunchKernelGGL(k_pcg_publish_b, dim3(1), block, 0, ctx->stream, mem, B, at.pub, at.seq_slot, at.seq);
      MPSE_HIP(ctx, hipGetLastError());
    }
    MPSE_TRY(publish_collect(ctx, at, SLAB.p, ms, B, PCG_CW, mpse_ctx::PIN_BATCH_CTL, hc.data()));
    ++ctx->pcg_batch_stats[mpse_ctx::PB_WAITS];
    bool all = true;
    for (int m = 0; m < B; ++m) all = all && hc[m].done;
    if (all) break;
    if (k >= max_iter) return mpse_fail(ctx, MPSE_ERR_HIP, "pcg_batch: no decision at the iteration limit");
  }
  return MPSE_OK;
}

}  // namespace

extern "C" {

int mpse_pcg_batch(mpse_ctx* ctx, int dtype, int count, const mpse_heff* h, int twolayer, const double* shift_host,
                   const void* const* diag_f64, const void* const* mask_f64, const void* const* b, void* const* x,
                   double tol, int max_iter, int* status_host, int* iters_host, double* relres_host,
                   double* lvalue_host) {
  if (!ctx) return MPSE_ERR_ARG;
  if (count < 0 || (count > 0 && (!h || !shift_host || !b || !x || !status_host)))
    return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_batch: null argument");
  if (dtype != MPSE_F64 && dtype != MPSE_C128) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_batch: unknown dtype");
  if (!(tol >= 0.0)) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_batch: tol must be >= 0");
  if (count == 0) return MPSE_OK;
  MPSE_BIND(ctx);
  const size_t es = dtype_size(dtype);
  // launch sets: eligible members of one shape, in the order of their first appearance, up to PCGB_MAX each
  std::vector<PcgSet> sets, open;
  std::vector<char> grouped(count, 0);
  for (int i = 0; i < count; ++i) {
    const mpse_heff& hi = h[i];
    Small2Plan pl;
    if (!b[i] || !x[i] || !hi.L || !hi.R || !hi.W0 || !std::isfinite(shift_host[i])) continue;   // (mpse_pcg refuses it)
    if (!pcg_batch_eligible(dtype, hi, twolayer, &pl)) continue;
    const size_t bytes = size_t(pl.Dl) * pl.d * pl.Dr * es;
    const char *xb = static_cast<const char*>(x[i]), *bb = static_cast<const char*>(b[i]);
    if (xb < bb + bytes && bb < xb + bytes) continue;
    PcgSet* tgt = nullptr;
    for (auto& o : open)
      if (o.plan.Dl == pl.Dl && o.plan.d == pl.d && o.plan.Dr == pl.Dr && o.plan.wl == pl.wl && o.plan.wr == pl.wr) {
        tgt = &o;
        break;
      }
    if (tgt && (int)tgt->idx.size() == PCGB_MAX) {
      sets.push_back(*tgt);
      tgt->idx.clear();
    }
    if (!tgt) {
      open.push_back(PcgSet{pl, {}});
      tgt = &open.back();
    }
    tgt->idx.push_back(i);
    grouped[i] = 1;
  }
  for (auto& o : open) sets.push_back(o);
  for (const PcgSet& ps : sets) {
    std::vector<PcgCtl> hc(ps.idx.size());
    MPSE_TRY(pcg_batch_set(ctx, dtype, ps, h, shift_host, diag_f64, mask_f64, b, x, tol, max_iter, hc));
    for (size_t m = 0; m < ps.idx.size(); ++m) {
      const int i = ps.idx[m];
      ++ctx->pcg_batch_stats[mpse_ctx::PB_MEMBERS];
      if (iters_host) iters_host[i] = hc[m].iters;
      if (relres_host) relres_host[i] = std::sqrt(hc[m].relres2);
      if (lvalue_host) lvalue_host[i] = hc[m].lvalue;
      status_host[i] = hc[m].status;
    }
  }
  for (int i = 0; i < count; ++i) {
    if (grouped[i]) continue;
    ++ctx->pcg_batch_stats[mpse_ctx::PB_SINGLE];
    int it = 0;
    double rel = 0.0, lv = 0.0;
    const int st = mpse_pcg(ctx, dtype, &h[i], twolayer, shift_host[i], diag_f64 ? diag_f64[i] : nullptr,
                            mask_f64 ? mask_f64[i] : nullptr, b[i], x[i], tol, max_iter, &it, &rel, &lv);
    if (st != MPSE_OK && st != MPSE_ERR_NOCONV && st != MPSE_ERR_ARG && st != MPSE_ERR_SHAPE) return st;
    status_host[i] = st;
    if (iters_host) iters_host[i] = it;
    if (relres_host) relres_host[i] = rel;
    if (lvalue_host) lvalue_host[i] = lv;
  }
  return MPSE_OK;
}

int mpse_pcg_batch_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  MPSE_TRY(stats_out(ctx, &mpse_ctx::pcg_batch_stats, counts, n));
  if (n > mpse_ctx::PB_COUNT) counts[mpse_ctx::PB_COUNT] = PCGB_MAX;
  return MPSE_OK;
}

int mpse_pcg_batch_plan(int dtype, int64_t Dl, int64_t d, int64_t Dr, int64_t wl, int64_t wr, int64_t* info, int n) {
  Small2Plan pl;
  const bool ok = small2_plan(dtype, Dl, d, Dr, wl, wr, &pl);
  const int64_t v[8] = {SM2_WMAX, SM2_DMAX, SM2_BMAX, SM2_LDS_MAX, ok ? pl.lds : 0, ok ? pl.jh : 0, ok ? pl.nslice : 0,
                        SM2_NNZ_LDS};
  for (int i = 0; i < n && info; ++i) info[i] = i < 8 ? v[i] : 0;
  return ok ? 1 : 0;
}

int mpse_pcg(mpse_ctx* ctx, int dtype, const mpse_heff* h, int twolayer, double shift, const void* diag_f64,
             const void* mask_f64, const void* b, void* x, double tol, int max_iter, int* iters_host,
             double* relres_host, double* lvalue_host) {
  if (!ctx) return MPSE_ERR_ARG;
  if (!h || !b || !x || !h->L || !h->R || !h->W0) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: null argument");
  MPSE_BIND(ctx);
  if (dtype != MPSE_F64 && dtype != MPSE_C128) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: unknown dtype");
  if (dtype != MPSE_C128 && (h->l_dtype == MPSE_C128 || h->r_dtype == MPSE_C128 || h->w_dtype == MPSE_C128))
    return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: real vectors with complex operator parts");
  if (!(tol >= 0.0) || !std::isfinite(shift)) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: tol must be >= 0 and shift finite");
  const mpse_dims& s = h->dims;
  if ((s.Dl_bra > 0 && s.Dl_bra != s.Dl_ket) || (s.Dr_bra > 0 && s.Dr_bra != s.Dr_ket))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "pcg: the projected operator must be square (bra bonds == ket bonds)");
  if (h->nsite != 1 && h->nsite != 2) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: one- or two-site centres");
  if (twolayer && (s.danc > 1 || s.danc1 > 1)) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: two-layer operators take no ancilla");
  const int64_t anc = s.danc > 0 ? s.danc : 1;
  int64_t n = s.Dl_ket * s.Dr_ket * s.d0 * anc;
  if (h->nsite == 2) n *= s.d1 * (s.danc1 > 0 ? s.danc1 : anc);
  if (n <= 0) return mpse_fail(ctx, MPSE_ERR_SHAPE, "pcg: empty centre tensor");
  const size_t bytes = size_t(n) * dtype_size(dtype);
  const char *xb = static_cast<const char*>(x), *bb = static_cast<const char*>(b);
  if (xb < bb + bytes && bb < xb + bytes) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: x must not overlap b");
  if (max_iter <= 0) max_iter = n > (int64_t(1) << 27) ? (1 << 30) : int(10 * n);   // scipy's default, 10 n
  wsite_written(ctx, x, bytes);

  PcgCtl hc;
  const double *diag = static_cast<const double*>(diag_f64), *mask = static_cast<const double*>(mask_f64);
  const int st = pcg_run_dtype(ctx, dtype, h, twolayer, shift, diag, mask, static_cast<const double*>(b),
                               static_cast<double*>(x), tol, max_iter, n, &hc);
  if (st != MPSE_OK) return st;      // (allocation or runtime failure: no solve is counted)
  if (twolayer) ++ctx->pcg_stats[mpse_ctx::PS_TWOLAYER];
  return pcg_report(ctx, hc, mask_f64 != nullptr, tol, iters_host, relres_host, lvalue_host);
}

int mpse_pcg_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  if (!ctx || n < 0 || (n > 0 && !counts)) return MPSE_ERR_ARG;
  for (int i = 0; i < n && i < mpse_ctx::PS_COUNT; ++i) counts[i] = ctx->pcg_stats[i];
  if (n > mpse_ctx::PS_COUNT) counts[mpse_ctx::PS_COUNT] = PCG_K;
  return MPSE_OK;
}

int mpse_pcg_sum(mpse_ctx* ctx, int dtype, int nterms, const mpse_heff_ft* terms, const double* weights_host,
                 double shift, const void* diag_f64, const void* mask_f64, const void* b, void* x, double tol,
                 int max_iter, int* iters_host, double* relres_host, double* lvalue_host) {
  if (!ctx) return MPSE_ERR_ARG;
  if (!terms || !weights_host || !b || !x) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: null argument");
  MPSE_BIND(ctx);
  if (nterms < 1 || nterms > 4) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: 1 to 4 terms, got %d", nterms);
  if (dtype != MPSE_F64 && dtype != MPSE_C128) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: unknown dtype");
  if (!(tol >= 0.0) || !std::isfinite(shift)) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: tol must be >= 0 and shift finite");
  for (int t = 0; t < nterms; ++t) {
    const mpse_heff_ft& h = terms[t];
    if (!h.L || !h.R || !h.W1 || !h.W2) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: null operator part in term %d", t);
    MPSE_TRY(ft_shape_ok(ctx, h, "pcg_sum"));
    if (!std::isfinite(weights_host[t])) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: weight %d is not finite", t);
    if (dtype != MPSE_C128 && (h.l_dtype == MPSE_C128 || h.r_dtype == MPSE_C128 || h.w_dtype == MPSE_C128))
      return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: real vectors with complex operator parts");
    if (h.Dl != terms[0].Dl || h.Dr != terms[0].Dr || h.d_up != terms[0].d_up || h.d_down != terms[0].d_down)
      return mpse_fail(ctx, MPSE_ERR_SHAPE, "pcg_sum: term %d acts on another centre shape", t);
  }
  const int64_t n = terms[0].Dl * terms[0].d_up * terms[0].d_down * terms[0].Dr;
  const size_t bytes = size_t(n) * dtype_size(dtype);
  const char *xb = static_cast<const char*>(x), *bb = static_cast<const char*>(b);
  if (xb < bb + bytes && bb < xb + bytes) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: x must not overlap b");
  if (max_iter <= 0) max_iter = n > (int64_t(1) << 27) ? (1 << 30) : int(10 * n);
  wsite_written(ctx, x, bytes);

  PcgCtl hc;
  const double *diag = static_cast<const double*>(diag_f64), *mask = static_cast<const double*>(mask_f64);
  const int st = pcg_run_dtype(ctx, dtype, nullptr, 0, shift, diag, mask, static_cast<const double*>(b),
                               static_cast<double*>(x), tol, max_iter, n, &hc, nterms, terms, weights_host);
  if (st != MPSE_OK) return st;
  ++ctx->pcg_sum_stats[mpse_ctx::PSS_SOLVES];
  ctx->pcg_sum_stats[mpse_ctx::PSS_ITERS] += hc.iters;
  return pcg_report(ctx, hc, mask_f64 != nullptr, tol, iters_host, relres_host, lvalue_host);
}

int mpse_pcg_sum_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::pcg_sum_stats, counts, n);
}

int mpse_site_factor_ft(mpse_ctx* ctx, const mpse_heff_ft* h, void* S_f64) {
  if (!ctx) return MPSE_ERR_ARG;
  if (!h || !S_f64 || !h->W1 || !h->W2) return mpse_fail(ctx, MPSE_ERR_ARG, "site_factor_ft: null argument");
  MPSE_BIND(ctx);
  MPSE_TRY(ft_shape_ok(ctx, *h, "site_factor_ft"));
  if (h->w_dtype != MPSE_F64) return mpse_fail(ctx, MPSE_ERR_ARG, "site_factor_ft: real MPO sites only");
  const long long total = h->wl1 * h->wl2 * h->d_up * h->d_down * h->wr1 * h->wr2;
  hipLaunchKernelGGL(k_site_factor_ft, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, ft_shape(*h),
                     static_cast<const double*>(h->W1), static_cast<const double*>(h->W2), static_cast<double*>(S_f64));
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

int mpse_diag_ft(mpse_ctx* ctx, const mpse_heff_ft* h, const void* S_f64, double weight, double shift, int accumulate,
                 void* diag_f64) {
  if (!ctx) return MPSE_ERR_ARG;
  if (!h || !S_f64 || !diag_f64 || !h->L || !h->R) return mpse_fail(ctx, MPSE_ERR_ARG, "diag_ft: null argument");
  MPSE_BIND(ctx);
  MPSE_TRY(ft_shape_ok(ctx, *h, "diag_ft"));
  const long long total = h->Dl * h->d_up * h->d_down * h->Dr;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const FtShape fs = ft_shape(*h);
  const double *L = static_cast<const double*>(h->L), *R = static_cast<const double*>(h->R);
  const double* S = static_cast<const double*>(S_f64);
  double* dg = static_cast<double*>(diag_f64);
  const bool lc = h->l_dtype == MPSE_C128, rc = h->r_dtype == MPSE_C128;
  if (lc && rc)
    hipLaunchKernelGGL((k_diag_ft<true, true>), grid, block, 0, ctx->stream, fs, L, R, S, weight, shift, accumulate, dg);
  else if (lc)
    hipLaunchKernelGGL((k_diag_ft<true, false>), grid, block, 0, ctx->stream, fs, L, R, S, weight, shift, accumulate, dg);
  else if (rc)
    hipLaunchKernelGGL((k_diag_ft<false, true>), grid, block, 0, ctx->stream, fs, L, R, S, weight, shift, accumulate, dg);
  else
    hipLaunchKernelGGL((k_diag_ft<false, false>), grid, block, 0, ctx->stream, fs, L, R, S, weight, shift, accumulate, dg);
  MPSE_HIP(ctx, hipGetLastError());
  if (!accumulate) ++ctx->pcg_sum_stats[mpse_ctx::PSS_DIAGS];
  return MPSE_OK;
}

}  // extern "C"
