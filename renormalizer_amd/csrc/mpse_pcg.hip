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
#include "mpse_pcg_plan.h"

namespace {

using namespace mpse_pcg_plan;   // PCG_K, PCG_CW, PCG_WHY_*, waits_at, default_max_iter, layout

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
static_assert(sizeof(PcgCtl) == PCG_CW * sizeof(double), "control block = PCG_CW doubles");

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

// ---- the host side: one driver (pcg_drive) for mpse_pcg, mpse_pcg_sum and the launch sets of mpse_pcg_batch

// A launch set: B >= 1 members of one shape.  mh[m] holds the caller's b, x, mask, diag and shift of member m and the
// vectors, partials and control block of its region of the slab (mpse_pcg_plan::layout, regions `stride` bytes apart).
// mem: the same table on the device, or null (B == 1): a single solve uploads nothing and launches the direct-pointer
// kernels on mh[0] - its launches and its global accesses are what they always were.
struct PcgSet {
  int dtype;
  int64_t n;
  int nb, nbq;                   // partial pairs per reduction of the vector kernels / of p^H q
  double tol;
  int max_iter;
  int B;
  const Pcg2Member *mh, *mem;
  size_t stride;
  const char* who;
};
void pcg_place(Pcg2Member& mb, char* base, const Layout& l) {
  auto at = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  mb.ctl = base + l.ctl;
  mb.part_bb = at(l.part_bb), mb.part_bx = at(l.part_bx), mb.part_pq = at(l.part_pq);
  mb.part_rz0 = at(l.part_rz[0]), mb.part_rz1 = at(l.part_rz[1]);
  mb.y = at(l.y), mb.q = at(l.q), mb.r = at(l.r), mb.p = at(l.p);
}

// The stages as launches, one method per stage: the table form when the set has a device table, else the direct form.
struct PcgLaunch {
  mpse_ctx* ctx;
  const PcgSet& s;
  const bool cplx = s.dtype == MPSE_C128;
  const long long n = (long long)s.n;
  const Pcg2Member& m = s.mh[0];
  const dim3 grid{(unsigned)s.nb, 1, (unsigned)(s.mem ? s.B : 1)}, block{RED_THREADS};
  PcgCtl* ctl() const { return static_cast<PcgCtl*>(m.ctl); }
  double* rz(int k) const { return k & 1 ? m.part_rz1 : m.part_rz0; }      // r^H z partials by iteration parity

  int prep() const {
    if (s.mem)
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_prep_b, grid, block, s.mem, n);
    else
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_prep, grid, block, m.x, m.b, m.mask, m.diag, n, m.part_bb, ctl());
    return MPSE_OK;
  }
  int start() const {
    if (s.mem)
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_start_b, grid, block, s.mem, n, s.nb);
    else
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_start, grid, block, m.y, m.b, m.mask, m.diag, m.x, m.r, m.p, m.shift, n, m.part_bb,
                         s.nb, m.part_rz0, m.part_bx, ctl());
    return MPSE_OK;
  }
  // q and the partials of p^H q from the product in y, or from the results of the terms of a summed solve
  int q(const PcgTerms* sum) const {
    if (s.mem) return mpse_fail(ctx, MPSE_ERR_ARG, "%s: the q kernel has no table form", s.who);
    if (sum)
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_q_sum, grid, block, *sum, m.p, m.mask, m.shift, m.q, n, m.part_pq, ctl());
    else
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_q, grid, block, m.y, m.p, m.mask, m.shift, m.q, n, m.part_pq, ctl());
    return MPSE_OK;
  }
  int step(int k) const {
    if (s.mem)
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_step_b, grid, block, s.mem, n, s.nbq, s.nb, k);
    else
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_step, grid, block, m.p, m.q, m.b, m.mask, m.diag, m.x, m.r, n, m.part_pq,
                         rz(k - 1), rz(k), m.part_bx, s.nb, ctl());
    return MPSE_OK;
  }
  // the direction update with the decision.  `at`: where the control blocks go when the host waits here - the direct
  // form publishes by itself, the table form in a launch of one workgroup behind it
  int dir(int k, const PublishAt& at) const {
    const double tol2 = s.tol * s.tol;
    if (s.mem) {
      MPSE_LAUNCH_TF_CHK(ctx, cplx, k_pcg_dir_b, grid, block, s.mem, n, s.nb, tol2, k, s.max_iter);
      if (at.pub) hipLaunchKernelGGL(k_pcg_publish_b, dim3(1), block, 0, ctx->stream, s.mem, s.B, at.pub, at.seq_slot, at.seq);
    } else {
      MPSE_LAUNCH_TF(ctx, cplx, k_pcg_dir, grid, block, m.r, m.diag, m.p, n, rz(k), rz(k + 1), m.part_bx, s.nb, tol2, k,
                     s.max_iter, ctl(), at.pub, at.seq_slot, at.seq);
    }
    MPSE_HIP(ctx, hipGetLastError());
    return MPSE_OK;
  }
};

// what the driver enqueued, for the counters of its callers (valid also when the run fails part-way)
struct PcgTally {
  long long products = 0, waits = 0;
};

// Runs a launch set to the decisions of all its members: hc[0 .. B).  The matvec is the one point where the callers
// differ: mv.start() enqueues y = A x0 for every member, mv.product() the product with p of an iteration, which either
// leaves q and the partials of p^H q (mv.makes_q) or y - then the q kernel follows, on mv.sum() when y is a sum of terms.
template <class Matvec>
int pcg_drive(mpse_ctx* ctx, const PcgSet& s, Matvec& mv, PcgCtl* hc, PcgTally* tally) {
  const PcgLaunch go{ctx, s};
  memset(hc, 0, size_t(s.B) * sizeof(PcgCtl));
  MPSE_TRY(go.prep());
  MPSE_TRY(mv.start());
  MPSE_TRY(go.start());
  for (int k = 0;; ++k) {
    if (k > 0) {
      MPSE_TRY(mv.product());
      ++tally->products;
      if (!mv.makes_q) MPSE_TRY(go.q(mv.sum()));
      MPSE_TRY(go.step(k));
    }
    const bool wait_here = waits_at(k, s.max_iter);
    const PublishAt at = publish_target(ctx, wait_here, mpse_ctx::PIN_BATCH_CTL);
    MPSE_TRY(go.dir(k, at));
    if (!wait_here) continue;
    // the control blocks that this launch published, or a copy of them
    MPSE_TRY(publish_collect(ctx, at, s.mh[0].ctl, s.stride, s.B, PCG_CW, mpse_ctx::PIN_BATCH_CTL, hc));
    ++tally->waits;
    bool all = true;
    for (int m = 0; m < s.B; ++m) all = all && hc[m].done;
    if (all) return MPSE_OK;
    if (k >= s.max_iter) return mpse_fail(ctx, MPSE_ERR_HIP, "%s: no decision at the iteration limit", s.who);
  }
}

// ---- the three matvecs
// Heff or its two-layer form on the pointers of a single solve; contractions return at once after the decision
struct PcgGeneral {
  static constexpr bool makes_q = false;
  mpse_ctx* ctx;
  int dtype;
  const mpse_heff* h;
  int twolayer;
  const Pcg2Member& m;
  SolveScope scope{ctx};         // (the caller sets scope.skip to the control block's `done`)
  int apply(const void* in) {
    return twolayer ? heff_apply2(ctx, dtype, h, in, m.y, &scope) : heff_apply(ctx, dtype, h, in, m.y, &scope, nullptr);
  }
  int start() { return apply(m.x); }
  int product() { return apply(m.p); }
  const PcgTerms* sum() const { return nullptr; }
};
// a weighted sum of finite-temperature terms, each into a y of its own (ts.y: m.y, then the layout's further vectors);
// a single term of weight one is the plain solve on that term's result
struct PcgSummed {
  static constexpr bool makes_q = false;
  mpse_ctx* ctx;
  const PcgSet& s;
  const mpse_heff_ft* terms;
  PcgTerms ts;
  SolveScope scope{ctx};
  int apply(const void* in) {
    for (int t = 0; t < ts.n; ++t)
      MPSE_TRY(heff_apply_ft(ctx, s.dtype, &terms[t], in, const_cast<double*>(ts.y[t]), &scope));
    return MPSE_OK;
  }
  int start() {
    MPSE_TRY(apply(s.mh[0].x));
    if (sum())      // the start residual goes through k_pcg_start: the sum into the first term's vector
      MPSE_LAUNCH_TF_CHK(ctx, s.dtype == MPSE_C128, k_pcg_combine, dim3(s.nb), dim3(RED_THREADS), ts, s.mh[0].y, (long long)s.n);
    return MPSE_OK;
  }
  int product() { return apply(s.mh[0].p); }
  const PcgTerms* sum() const { return ts.n > 1 || ts.w[0] != 1.0 ? &ts : nullptr; }
};
// the one-launch two-layer matvec of a launch set (mpse_small2.hip): members from the device table, q by itself
struct PcgSmall2 {
  static constexpr bool makes_q = true;
  mpse_ctx* ctx;
  const Small2Plan& pl;
  const PcgSet& s;
  int start() {
    MPSE_TRY(small2_prep(ctx, s.dtype, pl, s.B, s.mem));
    return small2_apply(ctx, s.dtype, pl, s.B, s.mem, 0);
  }
  int product() { return small2_apply(ctx, s.dtype, pl, s.B, s.mem, 1); }
  const PcgTerms* sum() const { return nullptr; }
};

// a single solve (mpse_pcg, mpse_pcg_sum, a batch member outside the one-launch rule): its slab and its set of one
struct PcgSingle {
  TmpBuf slab;
  Layout lay{};
  Pcg2Member m{};
  PcgSet set{};
  explicit PcgSingle(mpse_ctx* ctx) : slab(ctx) {}
  int init(int dtype, int64_t n, int extra_y, double shift, const void* diag, const void* mask, const void* b, void* x,
           double tol, int max_iter) {
    const bool cplx = dtype == MPSE_C128;
    const int nb = red_blocks(n * (cplx ? 2 : 1));
    lay = layout(n, cplx, nb, nb, extra_y);
    MPSE_TRY(slab.alloc(lay.stride));
    pcg_place(m, slab.as<char>(), lay);
    m.diag = static_cast<const double*>(diag), m.mask = static_cast<const double*>(mask);
    m.b = static_cast<const double*>(b), m.x = static_cast<double*>(x);
    m.shift = shift;
    set = PcgSet{dtype, n, nb, nb, tol, max_iter > 0 ? max_iter : default_max_iter(n), 1, &m, nullptr, 0, "pcg"};
    return MPSE_OK;
  }
};

// ---- argument rules shared by the entry points (`who` heads the message), and those of mpse_pcg
int pcg_check_dtype(mpse_ctx* ctx, const char* who, int dtype) {
  return dtype != MPSE_F64 && dtype != MPSE_C128 ? mpse_fail(ctx, MPSE_ERR_ARG, "%s: unknown dtype", who) : MPSE_OK;
}
int pcg_check_parts(mpse_ctx* ctx, const char* who, int dtype, int l_dtype, int r_dtype, int w_dtype) {
  if (dtype != MPSE_C128 && (l_dtype == MPSE_C128 || r_dtype == MPSE_C128 || w_dtype == MPSE_C128))
    return mpse_fail(ctx, MPSE_ERR_ARG, "%s: real vectors with complex operator parts", who);
  return MPSE_OK;
}
int pcg_check_tol_shift(mpse_ctx* ctx, const char* who, double tol, double shift) {
  if (!(tol >= 0.0) || !std::isfinite(shift)) return mpse_fail(ctx, MPSE_ERR_ARG, "%s: tol must be >= 0 and shift finite", who);
  return MPSE_OK;
}
int pcg_check_overlap(mpse_ctx* ctx, const char* who, int dtype, int64_t n, const void* b, const void* x) {
  const size_t bytes = size_t(n) * dtype_size(dtype);
  const char *xb = static_cast<const char*>(x), *bb = static_cast<const char*>(b);
  return xb < bb + bytes && bb < xb + bytes ? mpse_fail(ctx, MPSE_ERR_ARG, "%s: x must not overlap b", who) : MPSE_OK;
}
// The rules of mpse_pcg in the order they fire; it touches nothing but the message, so that mpse_pcg_batch can ask for
// a member's status without running it.  *n: the vector length of a member that passes.
int pcg_check_member(mpse_ctx* ctx, int dtype, const mpse_heff* h, int twolayer, double shift, const void* b,
                     const void* x, double tol, int64_t* n) {
  if (!h || !b || !x || !h->L || !h->R || !h->W0) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: null argument");
  MPSE_TRY(pcg_check_dtype(ctx, "pcg", dtype));
  MPSE_TRY(pcg_check_parts(ctx, "pcg", dtype, h->l_dtype, h->r_dtype, h->w_dtype));
  MPSE_TRY(pcg_check_tol_shift(ctx, "pcg", tol, shift));
  const mpse_dims& s = h->dims;
  if ((s.Dl_bra > 0 && s.Dl_bra != s.Dl_ket) || (s.Dr_bra > 0 && s.Dr_bra != s.Dr_ket))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "pcg: the projected operator must be square (bra bonds == ket bonds)");
  if (h->nsite != 1 && h->nsite != 2) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: one- or two-site centres");
  if (twolayer && (s.danc > 1 || s.danc1 > 1)) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg: two-layer operators take no ancilla");
  const int64_t anc = s.danc > 0 ? s.danc : 1;
  *n = s.Dl_ket * s.Dr_ket * s.d0 * anc;
  if (h->nsite == 2) *n *= s.d1 * (s.danc1 > 0 ? s.danc1 : anc);
  if (*n <= 0) return mpse_fail(ctx, MPSE_ERR_SHAPE, "pcg: empty centre tensor");
  return pcg_check_overlap(ctx, "pcg", dtype, *n, b, x);
}

// ---- outcomes: a control block as outputs and status (one without a decision is a failure of the engine)
int pcg_outcome(const PcgCtl& hc, int* iters_host, double* relres_host, double* lvalue_host) {
  if (iters_host) *iters_host = hc.iters;
  if (relres_host) *relres_host = std::sqrt(hc.relres2);
  if (lvalue_host) *lvalue_host = hc.lvalue;
  return hc.why == PCG_WHY_NONE ? MPSE_ERR_HIP : hc.status;
}
// in a batch these belong to the member; any other status fails the call
bool pcg_members_own(int status) {
  return status == MPSE_OK || status == MPSE_ERR_NOCONV || status == MPSE_ERR_ARG || status == MPSE_ERR_SHAPE;
}
// a single solve that reached its decision: counted, written out, with the message of one that failed
int pcg_single_end(mpse_ctx* ctx, const PcgCtl& hc, bool masked, double tol, int* iters_host, double* relres_host,
                   double* lvalue_host) {
  const int st = pcg_outcome(hc, iters_host, relres_host, lvalue_host);
  ++ctx->pcg_stats[mpse_ctx::PS_SOLVES];
  if (masked) ++ctx->pcg_stats[mpse_ctx::PS_MASKED];
  ctx->pcg_stats[mpse_ctx::PS_ITERS] += hc.iters;
  switch (hc.why) {
    case PCG_WHY_TOL:
    case PCG_WHY_ZERO_B:
      ++ctx->pcg_stats[mpse_ctx::PS_END_TOL];
      return st;
    case PCG_WHY_MAXITER:
      ++ctx->pcg_stats[mpse_ctx::PS_END_MAXITER];
      return mpse_fail(ctx, st, "pcg: |r| / |b| = %.3e after %d iterations (tol %.3e)", std::sqrt(hc.relres2), hc.iters, tol);
    case PCG_WHY_CURVATURE:
      ++ctx->pcg_stats[mpse_ctx::PS_END_CURVATURE];
      return mpse_fail(ctx, st, "pcg: curvature p^H A p <= 0 (or not a number) after %d iterations: the operator "
                       "is not positive definite", hc.iters);
    case PCG_WHY_DIAG:
      return mpse_fail(ctx, st, "pcg: the preconditioner diagonal has entries that are not positive");
    default:
      return mpse_fail(ctx, st, "pcg: control block without a decision");
  }
}

// mpse_pcg behind its argument rules (n from pcg_check_member); also a batch member outside the one-launch rule
int pcg_solve_general(mpse_ctx* ctx, int dtype, const mpse_heff* h, int twolayer, double shift, const void* diag,
                      const void* mask, const void* b, void* x, double tol, int max_iter, int64_t n, int* iters_host,
                      double* relres_host, double* lvalue_host) {
  wsite_written(ctx, x, size_t(n) * dtype_size(dtype));
  PcgSingle one(ctx);
  MPSE_TRY(one.init(dtype, n, 0, shift, diag, mask, b, x, tol, max_iter));
  PcgGeneral mv{ctx, dtype, h, twolayer, one.m};
  mv.scope.skip = static_cast<const int*>(one.m.ctl);      // PcgCtl::done
  PcgCtl hc;
  PcgTally t;
  const int st = pcg_drive(ctx, one.set, mv, &hc, &t);
  ctx->pcg_stats[mpse_ctx::PS_MATVECS] += t.products;
  ctx->pcg_stats[mpse_ctx::PS_WAITS] += t.waits;
  if (st != MPSE_OK) return st;      // (allocation or runtime failure: no solve is counted)
  if (twolayer) ++ctx->pcg_stats[mpse_ctx::PS_TWOLAYER];
  return pcg_single_end(ctx, hc, mask != nullptr, tol, iters_host, relres_host, lvalue_host);
}

// ---- mpse_pcg_batch: launch sets of members with one shape that takes the one-launch two-layer matvec
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

struct PcgGroup {
  Small2Plan plan;
  std::vector<int> idx;      // member -> position in the caller's arrays
};

int pcg_batch_set(mpse_ctx* ctx, int dtype, const PcgGroup& ps, const mpse_heff* hs, const double* shifts,
                  const void* const* diags, const void* const* masks, const void* const* bs, void* const* xs, double tol,
                  int max_iter, PcgCtl* hc) {
  const int B = (int)ps.idx.size();
  const Small2Plan& pl = ps.plan;
  const bool cplx = dtype == MPSE_C128;
  const size_t es = dtype_size(dtype);
  const int64_t n = int64_t(pl.Dl) * pl.d * pl.Dr;
  const int nb = red_blocks(n * (cplx ? 2 : 1)), nbq = pl.Dl;
  // behind the solver's sections of a member: the transposed left environment and the sparse W list of its matvec
  Layout lay = layout(n, cplx, nb, nbq, 0);
  const size_t cap = size_t(pl.rows) * pl.pitch;
  const size_t o_lt = lay.end;
  const size_t o_ptr = o_lt + align256(size_t(pl.Dl) * pl.wl * pl.wl * pl.Dl * es);
  const size_t o_idx = o_ptr + align256(size_t(pl.rows + 1) * sizeof(int));
  const size_t o_val = o_idx + align256(cap * sizeof(int));
  lay.stride = o_val + align256(cap * sizeof(double));
  TmpBuf SLAB(ctx), MEM(ctx);
  MPSE_TRY(SLAB.alloc(size_t(B) * lay.stride));
  MPSE_TRY(MEM.alloc(size_t(B) * sizeof(Pcg2Member)));
  std::vector<Pcg2Member> mh(B);
  for (int m = 0; m < B; ++m) {
    const int i = ps.idx[m];
    char* base = SLAB.as<char>() + size_t(m) * lay.stride;
    Pcg2Member& mb = mh[m];
    pcg_place(mb, base, lay);
    mb.L = static_cast<const double*>(hs[i].L), mb.R = static_cast<const double*>(hs[i].R);
    mb.W = static_cast<const double*>(hs[i].W0);
    mb.Lt = reinterpret_cast<double*>(base + o_lt);
    mb.csr_ptr = reinterpret_cast<int*>(base + o_ptr), mb.csr_idx = reinterpret_cast<int*>(base + o_idx);
    mb.csr_val = reinterpret_cast<double*>(base + o_val);
    mb.mask = masks ? static_cast<const double*>(masks[i]) : nullptr;
    mb.diag = diags ? static_cast<const double*>(diags[i]) : nullptr;
    mb.b = static_cast<const double*>(bs[i]);
    mb.x = static_cast<double*>(xs[i]);
    mb.shift = shifts[i];
    wsite_written(ctx, xs[i], size_t(n) * es);
  }
  MPSE_TRY(stage_h2d(ctx, MEM.p, mh.data(), mh.size() * sizeof(Pcg2Member)));
  const PcgSet set{dtype, n, nb, nbq, tol, max_iter > 0 ? max_iter : default_max_iter(n), B, mh.data(),
                   MEM.as<const Pcg2Member>(), lay.stride, "pcg_batch"};
  PcgSmall2 mv{ctx, pl, set};
  PcgTally t;
  const int st = pcg_drive(ctx, set, mv, hc, &t);
  ++ctx->pcg_batch_stats[mpse_ctx::PB_SETS];
  ctx->pcg_batch_stats[mpse_ctx::PB_MATVEC_LAUNCHES] += t.products;
  ctx->pcg_batch_stats[mpse_ctx::PB_WAITS] += t.waits;
  return st;
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
  MPSE_TRY(pcg_check_dtype(ctx, "pcg_batch", dtype));
  if (!(tol >= 0.0)) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_batch: tol must be >= 0");
  if (count == 0) return MPSE_OK;
  MPSE_BIND(ctx);
  auto out = [](auto* arr, int i) { return arr ? arr + i : nullptr; };
  // launch sets: members that pass the rules of mpse_pcg and are eligible, of one shape, in the order of their first
  // appearance, up to PCGB_MAX each
  std::vector<PcgGroup> sets, open;
  std::vector<char> grouped(count, 0);
  for (int i = 0; i < count; ++i) {
    Small2Plan pl;
    int64_t n;
    if (pcg_check_member(ctx, dtype, &h[i], twolayer, shift_host[i], b[i], x[i], tol, &n) != MPSE_OK) continue;
    if (!pcg_batch_eligible(dtype, h[i], twolayer, &pl)) continue;
    PcgGroup* tgt = nullptr;
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
      open.push_back(PcgGroup{pl, {}});
      tgt = &open.back();
    }
    tgt->idx.push_back(i);
    grouped[i] = 1;
  }
  for (auto& o : open) sets.push_back(o);
  PcgCtl hc[PCGB_MAX];
  for (const PcgGroup& ps : sets) {
    MPSE_TRY(pcg_batch_set(ctx, dtype, ps, h, shift_host, diag_f64, mask_f64, b, x, tol, max_iter, hc));
    for (size_t m = 0; m < ps.idx.size(); ++m) {
      const int i = ps.idx[m];
      status_host[i] = pcg_outcome(hc[m], out(iters_host, i), out(relres_host, i), out(lvalue_host, i));
      if (!pcg_members_own(status_host[i])) return mpse_fail(ctx, status_host[i], "pcg_batch: control block without a decision");
      ++ctx->pcg_batch_stats[mpse_ctx::PB_MEMBERS];
    }
  }
  // the others one by one as mpse_pcg solves them; one that its rules refuse has that status, the message and zeros
  for (int i = 0; i < count; ++i) {
    if (grouped[i]) continue;
    ++ctx->pcg_batch_stats[mpse_ctx::PB_SINGLE];
    int64_t n;
    int st = pcg_check_member(ctx, dtype, &h[i], twolayer, shift_host[i], b[i], x[i], tol, &n);
    if (st == MPSE_OK)
      st = pcg_solve_general(ctx, dtype, &h[i], twolayer, shift_host[i], diag_f64 ? diag_f64[i] : nullptr,
                             mask_f64 ? mask_f64[i] : nullptr, b[i], x[i], tol, max_iter, n, out(iters_host, i),
                             out(relres_host, i), out(lvalue_host, i));
    else
      pcg_outcome(PcgCtl{}, out(iters_host, i), out(relres_host, i), out(lvalue_host, i));
    if (!pcg_members_own(st)) return st;
    status_host[i] = st;
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
  int64_t n;
  MPSE_TRY(pcg_check_member(ctx, dtype, h, twolayer, shift, b, x, tol, &n));
  MPSE_BIND(ctx);
  return pcg_solve_general(ctx, dtype, h, twolayer, shift, diag_f64, mask_f64, b, x, tol, max_iter, n, iters_host,
                           relres_host, lvalue_host);
}

int mpse_pcg_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  MPSE_TRY(stats_out(ctx, &mpse_ctx::pcg_stats, counts, n));
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
  MPSE_TRY(pcg_check_dtype(ctx, "pcg_sum", dtype));
  MPSE_TRY(pcg_check_tol_shift(ctx, "pcg_sum", tol, shift));
  for (int t = 0; t < nterms; ++t) {
    const mpse_heff_ft& h = terms[t];
    if (!h.L || !h.R || !h.W1 || !h.W2) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: null operator part in term %d", t);
    MPSE_TRY(ft_shape_ok(ctx, h, "pcg_sum"));
    if (!std::isfinite(weights_host[t])) return mpse_fail(ctx, MPSE_ERR_ARG, "pcg_sum: weight %d is not finite", t);
    MPSE_TRY(pcg_check_parts(ctx, "pcg_sum", dtype, h.l_dtype, h.r_dtype, h.w_dtype));
    if (h.Dl != terms[0].Dl || h.Dr != terms[0].Dr || h.d_up != terms[0].d_up || h.d_down != terms[0].d_down)
      return mpse_fail(ctx, MPSE_ERR_SHAPE, "pcg_sum: term %d acts on another centre shape", t);
  }
  const int64_t n = terms[0].Dl * terms[0].d_up * terms[0].d_down * terms[0].Dr;
  MPSE_TRY(pcg_check_overlap(ctx, "pcg_sum", dtype, n, b, x));
  wsite_written(ctx, x, size_t(n) * dtype_size(dtype));

  PcgSingle one(ctx);
  MPSE_TRY(one.init(dtype, n, nterms - 1, shift, diag_f64, mask_f64, b, x, tol, max_iter));
  PcgSummed mv{ctx, one.set, terms};
  mv.scope.skip = static_cast<const int*>(one.m.ctl);
  memset(&mv.ts, 0, sizeof(mv.ts));
  mv.ts.n = nterms;
  for (int t = 0; t < nterms; ++t) {
    mv.ts.y[t] = t == 0 ? one.m.y : reinterpret_cast<double*>(one.slab.as<char>() + one.lay.extra_y + size_t(t - 1) * one.lay.vec);
    mv.ts.w[t] = weights_host[t];
  }
  PcgCtl hc;
  PcgTally t;
  const int st = pcg_drive(ctx, one.set, mv, &hc, &t);
  ctx->pcg_stats[mpse_ctx::PS_MATVECS] += t.products;
  ctx->pcg_stats[mpse_ctx::PS_WAITS] += t.waits;
  ctx->pcg_sum_stats[mpse_ctx::PSS_TERM_APPLIES] += t.products * nterms;
  ctx->pcg_sum_stats[mpse_ctx::PSS_WAITS] += t.waits;
  if (st != MPSE_OK) return st;
  ++ctx->pcg_sum_stats[mpse_ctx::PSS_SOLVES];
  ctx->pcg_sum_stats[mpse_ctx::PSS_ITERS] += hc.iters;
  return pcg_single_end(ctx, hc, mask_f64 != nullptr, tol, iters_host, relres_host, lvalue_host);
}

int mpse_pcg_sum_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::pcg_sum_stats, counts, n);
}

}  // extern "C"
