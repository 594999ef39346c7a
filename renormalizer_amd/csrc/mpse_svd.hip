// Quantum-number blocked economic SVD by one-sided (Hestenes) Jacobi on the device.
// Replaces scipy.linalg.svd(gesdd) per block in mps/svd_qn.py:12-49,177-213.
//
// All quantum-number blocks of a decomposition share every launch (blockIdx.y = block; mm >= nn, wide blocks are
// processed as their adjoint):
//   * the block is gathered column-major and QR factorised (hh_qr; Q1 gets the null-space columns the caller asked for);
//   * one-sided Jacobi on the square problem X = R^H, V = I: every launch is a block step over pairs of column blocks
//     (k_jacobi_block in LDS where the column blocks fit, k_jacobi_gram otherwise); a sweep without rotations ends the
//     iteration of a block, and the convergence of a sweep is read once for all blocks;
//   * sigma_j = |x_j| are read back, sorted on the host (descending, like LAPACK);
//   * columns are normalised; numerically null columns are zeroed and the basis is completed to an exact isometry by
//     a Householder QR of the normalised matrix (Q R with |R_jj| = 1 on the non-null columns), which is what LAPACK's
//     economic U guarantees and what the sweep algorithms above this layer rely on;
//   * the tall side's vectors are Q1[:, :nn] V.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "mpse_cx.h"
#include "mpse_device.h"
#include "mpse_internal.h"

namespace {

struct SvdBlk {
  long long ws_off, v_off, q_off;   // element offsets: column-major block (mm x nn), V (nn x nn), completed Q (mm x nq)
  long long row_off, col_off;       // into the concatenated row / column index lists
  long long koff, null_off;         // where its singular triplets / null vectors go in U / Vt
  int mm, nn, N, herm, extra, sig_off;
  double tol;
  int mm0, pad;                     // rows of the block the thresholds refer to (the tall block behind a square one)
  long long q1_off;                 // square stage: the tall block's Q factor, mm0 x (nn + extra)
};

template <bool CPLX>
__global__ void k_gather_blocks(double* ws, const double* __restrict__ coef, long long ncol,
                                const long long* __restrict__ rows_all, const long long* __restrict__ cols_all,
                                const SvdBlk* __restrict__ blks) {
  const SvdBlk B = blks[blockIdx.y];
  const long long* rows = rows_all + B.row_off;
  const long long* cols = cols_all + B.col_off;
  double* w = ws + B.ws_off * Cx<CPLX>::E;
  const int mm = B.mm, nn = B.nn;
  const long long total = (long long)mm * nn;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    if (!B.herm) {
      const int c = (int)(t % nn), r = (int)(t / nn);
      Cx<CPLX>::st(w, r + (long long)c * mm, Cx<CPLX>::ld(coef, rows[r] * ncol + cols[c]));
    } else {
      const int r = (int)(t % mm), c = (int)(t / mm);
      double2 v = Cx<CPLX>::ld(coef, rows[c] * ncol + cols[r]);
      v.y = -v.y;
      Cx<CPLX>::st(w, r + (long long)c * mm, v);
    }
  }
}

template <bool CPLX>
__global__ void k_identity_blocks(double* vbase, const SvdBlk* __restrict__ blks) {
  const SvdBlk B = blks[blockIdx.y];
  double* v = vbase + B.v_off * Cx<CPLX>::E;
  const long long total = (long long)B.nn * B.nn;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride)
    Cx<CPLX>::st(v, t, make_double2((t % B.nn) == (t / B.nn) ? 1.0 : 0.0, 0.0));
}

template <bool CPLX>
__global__ __launch_bounds__(RED_THREADS) void k_col_norms_b(const double* __restrict__ ws,
                                                             const SvdBlk* __restrict__ blks, double* sig) {
  const SvdBlk B = blks[blockIdx.y];
  if ((int)blockIdx.x >= B.nn) return;
  const double* col = ws + (B.ws_off + (long long)blockIdx.x * B.mm) * Cx<CPLX>::E;
  double s = 0, z = 0;
  for (int r = threadIdx.x; r < B.mm; r += RED_THREADS) {
    const double2 x = Cx<CPLX>::ld(col, r);
    s += x.x * x.x + x.y * x.y;
  }
  block_allsum2(s, z);
  if (threadIdx.x == 0) sig[B.sig_off + blockIdx.x] = sqrt(s);
}

// null2[b] = (largest column norm * eps * mm)^2 ; also resets the sweep state of the block
__global__ void k_null2(const SvdBlk* __restrict__ blks, const double* __restrict__ sig, double* null2, int* nrot,
                        int* done) {
  const SvdBlk B = blks[blockIdx.x];
  double m = 0.0;
  for (int j = threadIdx.x; j < B.nn; j += 64) m = fmax(m, sig[B.sig_off + j]);
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if (threadIdx.x == 0) {
    const double nn = m * 2.220446049250313e-16 * (double)B.mm0;
    null2[blockIdx.x] = nn * nn;
    nrot[blockIdx.x] = 0;
    done[blockIdx.x] = B.nn > 1 ? 0 : 1;
  }
}

// after a sweep: a block without rotations is converged; counters restart
__global__ void k_sweep_end(int nblk, int* nrot, int* done) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblk) return;
  if (nrot[b] == 0) done[b] = 1;
  nrot[b] = 0;
}

// Block step of the iteration on the square problems: a workgroup takes a PAIR OF COLUMN BLOCKS (JB_COLS columns
// each) of X and of V into LDS and runs a complete round-robin sweep over all pairs of those 2 JB_COLS columns there -
// one wave per pair, LDS-only barriers between the 2 JB_COLS - 1 inner steps - before it writes them back.  The
// launches of a sweep are the nb - 1 steps of the round robin over the nb column blocks: 31 launches instead of 255
// for 256 columns, each of them dozens of dependent rotations deep (a launch per rotation step costs ~6 us on this
// part whatever it does).  The pairs INSIDE a block are rotated in the first launch of a sweep only (full inner round
// robin over the 2 JB_COLS columns); the other launches rotate the JB_COLS x JB_COLS cross pairs (JB_COLS inner
// steps).  Needs 2 x 2 JB_COLS x nn elements of LDS (512 bytes per complex column, 256 per real one): whatever fits the
// dynamic LDS the runtime grants - nn <= 300 (complex) / 600 (real) at 150 KB, 128 / 256 at the default 64 KB.
constexpr int JB_COLS = 8;
constexpr int JB_KEEP = 4;          // x 64 rows of a column pair kept in registers through an inner step
template <bool CPLX>
__global__ __launch_bounds__(64 * JB_COLS) void k_jacobi_block(double* ws, double* vbase, const SvdBlk* __restrict__ blks,
                                                              int step, const double* __restrict__ null2v, int* nrot,
                                                              const int* __restrict__ done) {
  constexpr int E = Cx<CPLX>::E, NC = 2 * JB_COLS, NT = 64 * JB_COLS;
  extern __shared__ double s_cols[];            // X columns [NC][nn], then V columns [NC][nn]
  const int b = blockIdx.y;
  if (done[b]) return;
  const SvdBlk B = blks[b];
  const int nn = B.nn;
  const int nb = ((nn + JB_COLS - 1) / JB_COLS + 1) & ~1;      // column blocks, padded to an even number
  const int kk = blockIdx.x;
  if (step >= nb - 1 || kk >= nb / 2) return;
  int bp, bq;
  if (kk == 0) {
    bp = step % (nb - 1);
    bq = nb - 1;
  } else {
    bp = (step + kk) % (nb - 1);
    bq = (step - kk + (nb - 1)) % (nb - 1);
  }
  if (bp > bq) {
    const int t = bp;
    bp = bq;
    bq = t;
  }
  if (bp * JB_COLS >= nn) return;               // both blocks are padding
  double* x = ws + B.ws_off * E;
  double* v = vbase + B.v_off * E;
  double* sx = s_cols;
  double* sv = s_cols + (long long)NC * nn * E;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto gcol = [&](int c) { return (c < JB_COLS ? bp : bq) * JB_COLS + (c % JB_COLS); };   // local column -> column of X
  for (int t = tid; t < NC * nn; t += NT) {
    const int c = t / nn, r = t - c * nn, g = gcol(c);
    double2 a = make_double2(0.0, 0.0), w = a;
    if (g < nn) {
      a = Cx<CPLX>::ld(x, r + (long long)g * nn);
      w = Cx<CPLX>::ld(v, r + (long long)g * nn);
    }
    Cx<CPLX>::st(sx, t, a);
    Cx<CPLX>::st(sv, t, w);
  }
  __syncthreads();
  const double null2 = null2v[b], tol = B.tol;
  int rotations = 0;
  const bool full = step == 0;                  // (workgroup-uniform)
  for (int st = 0; st < (full ? NC - 1 : JB_COLS); ++st) {
    int p, q;
    if (full) {    // pair of this wave in inner step st (circle method on NC local columns)
      if (wave == 0) {
        p = st % (NC - 1);
        q = NC - 1;
      } else {
        p = (st + wave) % (NC - 1);
        q = (st - wave + (NC - 1)) % (NC - 1);
      }
      if (p > q) {
        const int t = p;
        p = q;
        q = t;
      }
    } else {       // cross pairs only: column `wave` of the first block with a rotating column of the second
      p = wave;
      q = JB_COLS + (wave + st) % JB_COLS;
    }
    if (gcol(p) < nn && gcol(q) < nn) {          // wave-uniform
      double* ap = sx + (long long)p * nn * E;
      double* aq = sx + (long long)q * nn * E;
      double alpha = 0, beta = 0, gr = 0, gi = 0;
      // (round 6: the first JB_KEEP x 64 rows of the two columns stay in registers between the Gram pass and the rotation,
      // and the same rows of the two V columns are requested before the rotation parameters exist - the step is bound
      // by its LDS traffic, 40 KB per wave, and by the round trips in front of and behind the scalar chain: 28.1 -> 25.8 us
      // per launch at 256 columns.  Keeping the wave's own column resident over all the cross steps of a launch was
      // built as well and measured slower, 28.2 us)
      double2 xa[JB_KEEP], xy[JB_KEEP], va[JB_KEEP], vy[JB_KEEP];
      double* vp = sv + (long long)p * nn * E;
      double* vq = sv + (long long)q * nn * E;
#pragma unroll
      for (int i = 0; i < JB_KEEP; ++i) {
        const int r = lane + 64 * i;
        xa[i] = xy[i] = va[i] = vy[i] = make_double2(0.0, 0.0);
        if (r < nn) {
          xa[i] = Cx<CPLX>::ld(ap, r);
          xy[i] = Cx<CPLX>::ld(aq, r);
        }
        alpha += xa[i].x * xa[i].x + xa[i].y * xa[i].y;
        beta += xy[i].x * xy[i].x + xy[i].y * xy[i].y;
        gr += xa[i].x * xy[i].x + xa[i].y * xy[i].y;
        gi += xa[i].x * xy[i].y - xa[i].y * xy[i].x;
      }
      for (int r = lane + 64 * JB_KEEP; r < nn; r += 64) {
        const double2 a = Cx<CPLX>::ld(ap, r), y = Cx<CPLX>::ld(aq, r);
        alpha += a.x * a.x + a.y * a.y;
        beta += y.x * y.x + y.y * y.y;
        gr += a.x * y.x + a.y * y.y;
        gi += a.x * y.y - a.y * y.x;
      }
#pragma unroll
      for (int i = 0; i < JB_KEEP; ++i) {
        const int r = lane + 64 * i;
        if (r < nn) {
          va[i] = Cx<CPLX>::ld(vp, r);
          vy[i] = Cx<CPLX>::ld(vq, r);
        }
      }
      alpha = wave_sum(alpha);
      beta = wave_sum(beta);
      gr = wave_sum(gr);
      gi = wave_sum(gi);
      // (every lane forms the same rotation: the chain of long-latency operations is kept short - one reciprocal square
      // root gives |g| and the phase, the convergence test compares squares; alpha, beta > null2 rules out underflow of
      // their product at any realistic scale)
      const double g2 = gr * gr + gi * gi;
      if (g2 != 0.0 && alpha > null2 && beta > null2 && g2 > (tol * tol) * alpha * beta) {
        // tan 2 theta = 2 |g| / (beta - alpha), the smaller angle, with two long operations in series instead of four
        // (round 6; the form of k_jacobi_gram): d = beta - alpha, r = sqrt(d^2 + 4 |g|^2), w = |d| + r,
        // c = w / sqrt(w^2 + 4 |g|^2), s = sign(d) 2 |g| / sqrt(w^2 + 4 |g|^2); the three Gram entries scaled by a power
        // of two first (squares of squared norms)
        const int ex = -__builtin_amdgcn_frexp_exp(alpha + beta);
        const double gxs = __builtin_amdgcn_ldexp(gr, ex), gys = __builtin_amdgcn_ldexp(gi, ex);
        const double d = __builtin_amdgcn_ldexp(beta, ex) - __builtin_amdgcn_ldexp(alpha, ex);
        const double g2s = gxs * gxs + gys * gys;
        const double ig = fast_rsqrt(g2s);
        const double pr = gxs * ig, pi = gys * ig;
        const double f = d * d + 4.0 * g2s;
        const double w = fabs(d) + f * fast_rsqrt(f);
        const double qn = fast_rsqrt(w * w + 4.0 * g2s);
        const double c = w * qn, sn = (d >= 0.0 ? 2.0 : -2.0) * (g2s * ig) * qn;
#pragma unroll
        for (int i = 0; i < JB_KEEP; ++i) {
          const int r = lane + 64 * i;
          if (r < nn) {
            const double2 a = xa[i], y0 = xy[i];
            const double2 y = make_double2(y0.x * pr + y0.y * pi, y0.y * pr - y0.x * pi);
            Cx<CPLX>::st(ap, r, make_double2(c * a.x - sn * y.x, c * a.y - sn * y.y));
            Cx<CPLX>::st(aq, r, make_double2(sn * a.x + c * y.x, sn * a.y + c * y.y));
            const double2 w2 = va[i], z0 = vy[i];
            const double2 z = make_double2(z0.x * pr + z0.y * pi, z0.y * pr - z0.x * pi);
            Cx<CPLX>::st(vp, r, make_double2(c * w2.x - sn * z.x, c * w2.y - sn * z.y));
            Cx<CPLX>::st(vq, r, make_double2(sn * w2.x + c * z.x, sn * w2.y + c * z.y));
          }
        }
        for (int r = lane + 64 * JB_KEEP; r < nn; r += 64) {
          const double2 a = Cx<CPLX>::ld(ap, r), y0 = Cx<CPLX>::ld(aq, r);
          const double2 y = make_double2(y0.x * pr + y0.y * pi, y0.y * pr - y0.x * pi);
          Cx<CPLX>::st(ap, r, make_double2(c * a.x - sn * y.x, c * a.y - sn * y.y));
          Cx<CPLX>::st(aq, r, make_double2(sn * a.x + c * y.x, sn * a.y + c * y.y));
          const double2 w = Cx<CPLX>::ld(vp, r), z0 = Cx<CPLX>::ld(vq, r);
          const double2 z = make_double2(z0.x * pr + z0.y * pi, z0.y * pr - z0.x * pi);
          Cx<CPLX>::st(vp, r, make_double2(c * w.x - sn * z.x, c * w.y - sn * z.y));
          Cx<CPLX>::st(vq, r, make_double2(sn * w.x + c * z.x, sn * w.y + c * z.y));
        }
        ++rotations;
      }
    }
    __syncthreads();
  }
  for (int t = tid; t < NC * nn; t += NT) {
    const int c = t / nn, r = t - c * nn, g = gcol(c);
    if (g < nn) {
      Cx<CPLX>::st(x, r + (long long)g * nn, Cx<CPLX>::ld(sx, t));
      Cx<CPLX>::st(v, r + (long long)g * nn, Cx<CPLX>::ld(sv, t));
    }
  }
  if (lane == 0 && rotations) atomicAdd(nrot + b, rotations);
}

// Block step on the Gram matrix (round 6): a pair of JG-column blocks of X and V is rotated through its 2 JG x 2 JG Gram
// matrix instead of through its columns - the step for blocks too wide for the column kernel above (its LDS holds
// 4 JB_COLS columns of nn rows: nn <= 300 complex / 600 real in 150 KB), where the alternative was one launch per
// rotation step.
//   1. G = Y^H Y of the 2 JG = 32 columns Y of the pair, on MFMA straight from memory (rows dealt to the 4 waves, partial
//      sums added through LDS in a fixed order).  Only the first launch of a sweep forms all three tiles: the diagonal
//      tiles of a column block travel with it (dgin / dgout: what the rotations of the previous launch made of them),
//      the later launches form the tile of the cross products;
//   2. the inner round robin runs on G alone: two-sided rotations G <- J^H G J in LDS (thread (k, l) owns the 2 x 2 block
//      of column pair k against column pair l and forms both rotations itself from the diagonal blocks - one barrier per
//      inner step, two copies of G by parity), U <- U J accumulated one step behind.  The rotation of a pair is the one
//      the column kernels form from the same three Gram entries; what differs is that the entries are carried through
//      the inner steps by the rotation formulas instead of being recomputed from the columns - two-sided Jacobi on a
//      positive definite matrix keeps the accuracy relative to the scaled matrix (Demmel / Veselic, SIAM J. Matrix
//      Anal. Appl. 13 (1992) 1204), and every sweep starts from fresh entries;
//   3. [X; V](:, pair) <- [X; V](:, pair) U on MFMA, 16-row tiles, transposed form so that loads and stores run along
//      the columns.
// The products are 6 nn 32^2 complex multiply-adds per launch and FP64 MFMA runs at the vector rate on this part
// (64 cycles per 16 x 16 x 4 step): ~20 us on ONE compute unit at nn = 256, so the rows of step 3 are dealt to R
// workgroups per pair (each repeats steps 1 - 2: same inputs, same bits).  That needs the launch to read one copy of
// X, V and write another (a workgroup must not overwrite rows a neighbour still reads for its Gram matrix): every
// workgroup writes its rows of its columns in EVERY launch - converged blocks, steps past a block's last one and pairs
// without a rotation copy them - so that the current copy is the same for all blocks.
// Measured (profiles/r06_svd_gram_step.md): an inner step with all 16 rotations live costs ~4 600 cycles (rotation
// parameters ~1 100, the 2 x 2 blocks ~1 600, U ~1 000, barrier ~400: one wave per SIMD, every LDS round trip and FP64
// chain exposed), a launch at nn = 256 ~50 us for 256 cross pairs where the column kernel takes 28 us for 64: the sweep
// costs the same (17 launches against 33) and whole runs are within +-2 %, so the column kernel keeps the blocks it
// fits; at nn = 512 (one block of a 512 x 4096 centre) the decomposition takes 28 ms against 58 with a launch per step.
constexpr int JG = 16;
typedef double jg_v4d __attribute__((ext_vector_type(4)));
template <bool CPLX>
__global__ __launch_bounds__(256) void k_jacobi_gram(const double* __restrict__ xin, double* __restrict__ xout,
                                                     const double* __restrict__ vin, double* __restrict__ vout,
                                                     const double2* __restrict__ dgin, double2* __restrict__ dgout,
                                                     int nbmax, const SvdBlk* __restrict__ blks, int step, int R,
                                                     const double* __restrict__ null2v, int* nrot,
                                                     const int* __restrict__ done) {
  constexpr int NC = 2 * JG;
  extern __shared__ double s_dyn[];
  double2* sG0 = reinterpret_cast<double2*>(s_dyn);     // G by parity of the inner step: 2 x [32][32]
  double2* sG1 = sG0 + NC * NC;
  constexpr int NCP = NC + 1;                           // pitch of U: stored by COLUMN (a rotation step reads two columns
  double2* sU = sG1 + NC * NC;                          // at 32 consecutive rows), padded against bank conflicts in step 3
  double* sPart = reinterpret_cast<double*>(sU + NC * NCP);   // 2 slots x 3 tiles x (re, im) x 4 x 64
  __shared__ int s_cnt;
  const int b = blockIdx.y;
  const SvdBlk B = blks[b];
  const int nn = B.nn;
  const int nb = ((nn + JG - 1) / JG + 1) & ~1;         // column blocks, padded to an even number
  const int kk = blockIdx.x / R, slab = blockIdx.x - kk * R;
  if (kk >= nb / 2) return;
  const bool active = !done[b] && step < nb - 1;
  const int pstep = active ? step : 0;                  // (idle launches copy by the pairing of step 0)
  int bp, bq;
  if (kk == 0) {
    bp = pstep % (nb - 1);
    bq = nb - 1;
  } else {
    bp = (pstep + kk) % (nb - 1);
    bq = (pstep - kk + (nb - 1)) % (nb - 1);
  }
  if (bp > bq) {
    const int t = bp;
    bp = bq;
    bq = t;
  }
  if (bp * JG >= nn) return;                            // both blocks are padding
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), x = lane & 15, kq = lane >> 4;
  const double* X = xin + B.ws_off * Cx<CPLX>::E;
  const double* V = vin + B.v_off * Cx<CPLX>::E;
  double* Xo = xout + B.ws_off * Cx<CPLX>::E;
  double* Vo = vout + B.v_off * Cx<CPLX>::E;
  const double2* dgp_in = dgin + ((long long)b * nbmax + bp) * 256;
  const double2* dgq_in = dgin + ((long long)b * nbmax + bq) * 256;
  double2* dgp_out = dgout + ((long long)b * nbmax + bp) * 256;
  double2* dgq_out = dgout + ((long long)b * nbmax + bq) * 256;
  auto gcol = [&](int c) { return (c < JG ? bp : bq) * JG + (c & (JG - 1)); };   // local column -> column of X
  if (tid == 0) s_cnt = 0;
  for (int t = tid; t < NC * NC; t += 256) sU[(t >> 5) * NCP + (t & 31)] = make_double2((t >> 5) == (t & 31) ? 1.0 : 0.0, 0.0);
  int rotated = 0;
  if (active) {
    // ---- 1. Gram matrix.  First launch of a sweep: all three tiles from the columns.  Later launches: the tile of the
    // cross products only - the diagonal tiles are what the previous launch's rotations made of them (dgin: every
    // launch leaves the diagonal tiles of its final G for the two column blocks it rotated).  Wave w takes the row
    // steps w, w + 4, .. (four rows each); all loads of a wave go out before its first MFMA.
    const bool fresh = step == 0;
    double2 dg_p = make_double2(0.0, 0.0), dg_q = dg_p;
    if (!fresh) {
      dg_p = dgp_in[tid];
      dg_q = dgq_in[tid];
    }
    jg_v4d gr[3], gi[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) gr[i] = gi[i] = jg_v4d{0, 0, 0, 0};
    {
      const int c0 = gcol(x), c1 = gcol(JG + x);
      const bool ok0 = c0 < nn, ok1 = c1 < nn;
      const long long o0 = (long long)(ok0 ? c0 : 0) * nn, o1 = (long long)(ok1 ? c1 : 0) * nn;
      const int nks = (nn + 3) >> 2;
      for (int base = wave; base < nks; base += 64) {
        double2 va[16], vb[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int ks = base + 4 * i;
          va[i] = vb[i] = make_double2(0.0, 0.0);
          if (ks < nks) {
            const int r = min(4 * ks + kq, nn - 1);
            va[i] = Cx<CPLX>::ld(X, o0 + r);
            vb[i] = Cx<CPLX>::ld(X, o1 + r);
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int ks = base + 4 * i;
          if (ks >= nks) break;
          const bool okr = 4 * ks + kq < nn;
          const double ar = okr && ok0 ? va[i].x : 0.0, ai = okr && ok0 ? va[i].y : 0.0;
          const double br = okr && ok1 ? vb[i].x : 0.0, bi = okr && ok1 ? vb[i].y : 0.0;
          // conj(a) b = (ar br + ai bi) + i (ar bi - ai br)
          gr[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, gr[1], 0, 0, 0);
          if constexpr (CPLX) {
            gr[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, gr[1], 0, 0, 0);
            gi[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, gi[1], 0, 0, 0);
            gi[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, br, gi[1], 0, 0, 0);
          }
          if (fresh) {
            gr[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, ar, gr[0], 0, 0, 0);
            gr[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(br, br, gr[2], 0, 0, 0);
            if constexpr (CPLX) {
              gr[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, ai, gr[0], 0, 0, 0);
              gr[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(bi, bi, gr[2], 0, 0, 0);
              gi[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, ai, gi[0], 0, 0, 0);
              gi[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, ar, gi[0], 0, 0, 0);
              gi[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(br, bi, gi[2], 0, 0, 0);
              gi[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(-bi, br, gi[2], 0, 0, 0);
            }
          }
        }
      }
    }
    // partial sums of the 4 waves in a fixed tree: (w, w + 2), then (0, 1); wave 1 writes into the slot it has consumed
    auto put = [&](int slot) {
      double* p = sPart + slot * 1536;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[(i * 8 + r) * 64 + lane] = gr[i][r];
          p[(i * 8 + 4 + r) * 64 + lane] = gi[i][r];
        }
    };
    auto add = [&](int slot) {
      const double* p = sPart + slot * 1536;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gr[i][r] += p[(i * 8 + r) * 64 + lane];
          gi[i][r] += p[(i * 8 + 4 + r) * 64 + lane];
        }
    };
    if (wave >= 2) put(wave - 2);
    if (!fresh) {          // the carried diagonal tiles
      const int row = tid >> 4, col = tid & 15;
      sG0[row * NC + col] = dg_p;
      sG0[(JG + row) * NC + JG + col] = dg_q;
    }
    __syncthreads();
    if (wave < 2) add(wave);
    if (wave == 1) put(1);
    __syncthreads();
    if (wave == 0) {
      add(1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = kq + 4 * r;
        // tiles (0,0), (0,1), (1,1); the lower tile is the adjoint of (0,1); the diagonal is real
        sG0[row * NC + JG + x] = make_double2(gr[1][r], gi[1][r]);
        sG0[(JG + x) * NC + row] = make_double2(gr[1][r], -gi[1][r]);
        if (fresh) {
          sG0[row * NC + x] = make_double2(gr[0][r], row == x ? 0.0 : gi[0][r]);
          sG0[(JG + row) * NC + JG + x] = make_double2(gr[2][r], row == x ? 0.0 : gi[2][r]);
        }
      }
    }
    __syncthreads();
    // ---- 2. inner round robin on G
    const double null2 = null2v[b], tol2 = B.tol * B.tol;
    const bool full = step == 0;                        // (pairs inside a block: in the first launch of a sweep only)
    const int nst = full ? NC - 1 : JG;
    struct Rot {
      double c, s, er, ei;
      bool on;
    };
    auto pair_of = [&](int m, int st, int& p, int& q) {
      if (full) {                                       // circle method on the 32 local columns
        if (m == 0) {
          p = st;                                       // (st < NC - 1)
          q = NC - 1;
        } else {
          p = st + m;
          if (p >= NC - 1) p -= NC - 1;
          q = st - m + (NC - 1);
          if (q >= NC - 1) q -= NC - 1;
        }
        if (p > q) {
          const int t = p;
          p = q;
          q = t;
        }
      } else {                                          // cross pairs only
        p = m;
        q = JG + ((m + st) & (JG - 1));
      }
    };
    // The rotation of the pair (p, q) from alpha = G_pp, beta = G_qq, g = G_pq - the one the column kernels form
    // (tan 2 theta = 2 |g| / (beta - alpha), the smaller angle), arranged so that two long operations sit in series instead
    // of four (every thread of the workgroup waits for this chain in every inner step): with d = beta - alpha,
    // r = sqrt(d^2 + 4 |g|^2), w = |d| + r:  t = sign(d) 2 |g| / w,  c = w / sqrt(w^2 + 4 |g|^2),  s = c t;  the phase
    // e = g / |g| comes from a reciprocal square root that runs beside the chain.  The three entries are scaled by a
    // power of two first (squares of squared norms would leave the exponent range at column norms ~1e+-77).
    // (Branch-free: the two rotations a thread forms are independent chains of ~30 dependent FP64 operations each and
    // must overlap - behind a branch they ran one after the other, 4 900 cycles per inner step against 2 600 with every
    // pair skipped.  Square root and reciprocal square root by the coupled iteration g -> sqrt, h -> 1 / (2 sqrt): two
    // dependent levels per step instead of four.)
    auto sqrt_pair = [](double xv, double& sq, double& rs) {
      const double y = __builtin_amdgcn_rsq(xv);
      double g = xv * y, h = 0.5 * y;
      double e = __builtin_fma(-h, g, 0.5);
      g = __builtin_fma(g, e, g);
      h = __builtin_fma(h, e, h);
      e = __builtin_fma(-h, g, 0.5);
      sq = __builtin_fma(g, e, g);
      rs = 2.0 * __builtin_fma(h, e, h);
    };
    auto rot_of = [&](const double2* G, int p, int q) {
      const double alpha = G[p * NC + p].x, beta = G[q * NC + q].x;
      const double2 g = G[p * NC + q];
      const int ex = -__builtin_amdgcn_frexp_exp(alpha + beta);
      const double as = __builtin_amdgcn_ldexp(alpha, ex), bs = __builtin_amdgcn_ldexp(beta, ex);
      const double gx = __builtin_amdgcn_ldexp(g.x, ex), gy = __builtin_amdgcn_ldexp(g.y, ex);
      const double g2 = gx * gx + gy * gy;
      const bool on = alpha > null2 && beta > null2 && g2 != 0.0 && g2 > tol2 * as * bs;
      const double g2s = on ? g2 : 1.0;                 // (a skipped pair runs the arithmetic on harmless numbers)
      const double d = on ? bs - as : 0.0, f = __builtin_fma(d, d, 4.0 * g2s);
      double absg, ig, r, ir;
      sqrt_pair(g2s, absg, ig);
      sqrt_pair(f, r, ir);
      const double w = fabs(d) + r, f2 = __builtin_fma(w, w, 4.0 * g2s);
      double r2, qn;
      sqrt_pair(f2, r2, qn);
      Rot rr;
      rr.on = on;
      rr.c = on ? w * qn : 1.0;
      rr.s = on ? (d >= 0.0 ? 2.0 : -2.0) * absg * qn : 0.0;
      rr.er = on ? gx * ig : 1.0;
      rr.ei = on ? gy * ig : 0.0;
      return rr;
    };
    // [a b] <- [a b] J,  J = [[c, s], [-s conj(e), c conj(e)]]  (the rotation of the column kernels: y = conj(e) b)
    auto cols = [&](const Rot& r, double2& a, double2& bb) {
      const double2 y = make_double2(bb.x * r.er + bb.y * r.ei, bb.y * r.er - bb.x * r.ei);
      const double2 na = make_double2(r.c * a.x - r.s * y.x, r.c * a.y - r.s * y.y);
      bb = make_double2(r.s * a.x + r.c * y.x, r.s * a.y + r.c * y.y);
      a = na;
    };
    // [a; b] <- J^H [a; b]:  a' = c a - s e b,  b' = s a + c e b
    auto rows = [&](const Rot& r, double2& a, double2& bb) {
      const double2 y = make_double2(bb.x * r.er - bb.y * r.ei, bb.y * r.er + bb.x * r.ei);
      const double2 na = make_double2(r.c * a.x - r.s * y.x, r.c * a.y - r.s * y.y);
      bb = make_double2(r.s * a.x + r.c * y.x, r.s * a.y + r.c * y.y);
      a = na;
    };
    const int k = tid >> 4, l = tid & 15;               // thread (k, l): the 2 x 2 block of pair k against pair l
    // U <- U J_k (rows l, l + 16 of the column pair k) runs one step behind: it does not feed the next rotations, so its
    // LDS round trips overlap the chain of the next step's rotation parameters instead of standing in front of the barrier
    Rot ru{1.0, 0.0, 1.0, 0.0, false};
    int pu = 0, qu = 0;
    auto u_update = [&]() {
      if (ru.on) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          double2 a = sU[pu * NCP + l + 16 * i], c = sU[qu * NCP + l + 16 * i];
          cols(ru, a, c);
          sU[pu * NCP + l + 16 * i] = a;
          sU[qu * NCP + l + 16 * i] = c;
        }
      }
    };
    for (int st = 0; st < nst; ++st) {
      const double2* Gc = (st & 1) ? sG1 : sG0;
      double2* Gn = (st & 1) ? sG0 : sG1;
      int pk, qk, pl, ql;
      pair_of(k, st, pk, qk);
      pair_of(l, st, pl, ql);
      double2 b00 = Gc[pk * NC + pl], b01 = Gc[pk * NC + ql], b10 = Gc[qk * NC + pl], b11 = Gc[qk * NC + ql];
      const Rot rk = rot_of(Gc, pk, qk), rl = rot_of(Gc, pl, ql);
      u_update();                                       // (of the previous step)
      cols(rl, b00, b01);
      cols(rl, b10, b11);
      rows(rk, b00, b10);
      rows(rk, b01, b11);
      if (k == l) {
        b00.y = b11.y = 0.0;
        if (rk.on) {
          b01 = b10 = make_double2(0.0, 0.0);
          ++rotated;
        }
      }
      Gn[pk * NC + pl] = b00;
      Gn[pk * NC + ql] = b01;
      Gn[qk * NC + pl] = b10;
      Gn[qk * NC + ql] = b11;
      ru = rk;
      pu = pk;
      qu = qk;
      __syncthreads();
    }
    u_update();
    if (rotated) atomicAdd(&s_cnt, rotated);
    if (slab == 0) {       // the diagonal tiles of the final G travel with the column blocks
      const double2* Gf = ((nst - 1) & 1) ? sG0 : sG1;
      const int row = tid >> 4, col = tid & 15;
      dgp_out[tid] = Gf[row * NC + col];
      dgq_out[tid] = Gf[(JG + row) * NC + JG + col];
    }
  } else if (slab == 0) {
    dgp_out[tid] = dgp_in[tid];
    dgq_out[tid] = dgq_in[tid];
  }
  __syncthreads();
  const int cnt = s_cnt;
  if (cnt && slab == 0 && tid == 0) atomicAdd(nrot + b, cnt);
  // ---- 3. the rows of this workgroup: 16-row tiles slab, slab + R, .. of [X; V], dealt to the waves
  const int nt = (nn + 15) >> 4;
  double ur[2][8], ui[2][8];
  if (cnt) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int k4 = 0; k4 < 8; ++k4) {
        const double2 w = sU[(JG * ct + x) * NCP + 4 * k4 + kq];
        ur[ct][k4] = w.x;
        ui[ct][k4] = w.y;
      }
  }
  int gc[8];
#pragma unroll
  for (int k4 = 0; k4 < 8; ++k4) gc[k4] = gcol(4 * k4 + kq);
  for (int ti = slab + R * wave; ti < 2 * nt; ti += 4 * R) {
    const bool isx = ti < nt;
    const double* src = isx ? X : V;
    double* dst = isx ? Xo : Vo;
    const int row = 16 * (isx ? ti : ti - nt) + x;
    const bool okr = row < nn;
    double2 y[8];
#pragma unroll
    for (int k4 = 0; k4 < 8; ++k4) {
      y[k4] = make_double2(0.0, 0.0);
      if (okr && gc[k4] < nn) y[k4] = Cx<CPLX>::ld(src, (long long)gc[k4] * nn + row);
    }
    if (!cnt) {                                         // nothing rotated: the rows pass through
#pragma unroll
      for (int k4 = 0; k4 < 8; ++k4)
        if (okr && gc[k4] < nn) Cx<CPLX>::st(dst, (long long)gc[k4] * nn + row, y[k4]);
      continue;
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      // out^T[col][row] = sum_k U[k][col] Y[row][k]
      jg_v4d ore = {0, 0, 0, 0}, oim = {0, 0, 0, 0};
#pragma unroll
      for (int k4 = 0; k4 < 8; ++k4) {
        ore = __builtin_amdgcn_mfma_f64_16x16x4f64(ur[ct][k4], y[k4].x, ore, 0, 0, 0);
        if constexpr (CPLX) {
          ore = __builtin_amdgcn_mfma_f64_16x16x4f64(-ui[ct][k4], y[k4].y, ore, 0, 0, 0);
          oim = __builtin_amdgcn_mfma_f64_16x16x4f64(ui[ct][k4], y[k4].x, oim, 0, 0, 0);
          oim = __builtin_amdgcn_mfma_f64_16x16x4f64(ur[ct][k4], y[k4].y, oim, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int g = gcol(JG * ct + kq + 4 * r);
        if (okr && g < nn) Cx<CPLX>::st(dst, (long long)g * nn + row, make_double2(ore[r], oim[r]));
      }
    }
  }
}

template <bool CPLX>
__global__ void k_normalise_perm_b(double* un_base, const double* __restrict__ ws, const SvdBlk* __restrict__ blks,
                                   const double* __restrict__ sig, const long long* __restrict__ perm,
                                   const double* __restrict__ thresh) {
  const SvdBlk B = blks[blockIdx.y];
  const int mm = B.mm, nn = B.nn;
  double* dst = un_base + B.ws_off * Cx<CPLX>::E;
  const double* src = ws + B.ws_off * Cx<CPLX>::E;
  const double th = thresh[blockIdx.y];
  const long long total = (long long)mm * nn;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int j = (int)(t / mm), r = (int)(t % mm);
    const int pj = (int)perm[B.sig_off + j];
    const double sg = sig[B.sig_off + pj];
    double2 x = Cx<CPLX>::ld(src, r + (long long)pj * mm);
    if (sg > th) {
      x.x /= sg;
      x.y /= sg;
    } else {
      x = make_double2(0.0, 0.0);
    }
    Cx<CPLX>::st(dst, t, x);
  }
}

// X = R^H (nn x nn, column major, lower triangular) from the factored tall block (R on and above the diagonal of the
// mm0 x nn workspace): the one-sided Jacobi iteration runs on the rows of R - Drmac / Veselic preconditioning: the
// rotations see nn-row columns instead of mm0-row ones and the sweeps needed drop several-fold.
template <bool CPLX>
__global__ void k_rh_blocks(double* x_base, const double* __restrict__ ws, const SvdBlk* __restrict__ tall,
                            const SvdBlk* __restrict__ sq) {
  const SvdBlk T = tall[blockIdx.y], S = sq[blockIdx.y];
  const int nn = T.nn, mm0 = T.mm;
  const double* r = ws + T.ws_off * Cx<CPLX>::E;
  double* x = x_base + S.ws_off * Cx<CPLX>::E;
  const long long total = (long long)nn * nn;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int i = (int)(t % nn), j = (int)(t / nn);          // X(i, j) = conj(R(j, i)), zero above the diagonal
    double2 v = make_double2(0.0, 0.0);
    if (j <= i) {
      v = Cx<CPLX>::ld(r, j + (long long)i * mm0);
      v.y = -v.y;
    }
    Cx<CPLX>::st(x, t, v);
  }
}

// de Rijk's ordering: the sweeps start from the columns of X sorted by decreasing norm (dst[:, j] = src[:, p[j]]), V
// from the matching permutation matrix - one-sided Jacobi then needs fewer sweeps
template <bool CPLX>
__global__ void k_sort_cols_b(double* dst_base, double* v_base, const double* __restrict__ src_base,
                              const long long* __restrict__ perm_all, const SvdBlk* __restrict__ sq) {
  const SvdBlk S = sq[blockIdx.y];
  const int nn = S.nn;
  const double* src = src_base + S.ws_off * Cx<CPLX>::E;
  double* dst = dst_base + S.ws_off * Cx<CPLX>::E;
  double* v = v_base + S.v_off * Cx<CPLX>::E;
  const long long* perm = perm_all + S.sig_off;
  const long long total = (long long)nn * nn;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int i = (int)(t % nn), j = (int)(t / nn);
    const int pj = (int)perm[j];
    Cx<CPLX>::st(dst, t, Cx<CPLX>::ld(src, i + (long long)pj * nn));
    Cx<CPLX>::st(v, t, make_double2(i == pj ? 1.0 : 0.0, 0.0));
  }
}

// A = Q1 R = Q1 X^H with X = Ux S Vx^H  =>  A = (Q1 Vx) S Ux^H: left vectors ut = Q1 Vx (mm0 x nn, column pj of it for
// the j-th largest value), right vectors the columns of the completed Ux (q, with the phase of the completion's
// diagonal).  herm blocks were factorised as their adjoint: the roles swap and both sides are conjugated.
template <bool CPLX>
__global__ void k_scatter_svd2_b(double* U, double* Vt, const double* __restrict__ ut_base,
                                 const double* __restrict__ un_base, const double* __restrict__ q_base,
                                 const long long* __restrict__ perm_all, long long K, long long ncol,
                                 const long long* __restrict__ rows_all, const long long* __restrict__ cols_all,
                                 const SvdBlk* __restrict__ tall, const SvdBlk* __restrict__ sq) {
  constexpr int E = Cx<CPLX>::E;
  const SvdBlk T = tall[blockIdx.y], S = sq[blockIdx.y];
  const int mm = T.mm, nn = T.nn, herm = T.herm;
  const double* ut = ut_base + T.ws_off * E;
  const double* un = un_base + S.ws_off * E;
  const double* q = q_base + S.q_off * E;
  const long long* perm = perm_all + S.sig_off;
  const long long* rows = rows_all + T.row_off;
  const long long* cols = cols_all + T.col_off;
  const long long koff = T.koff;
  const long long tott = (long long)mm * nn, totv = (long long)nn * nn;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < tott + totv; t += stride) {
    if (t < tott) {                 // tall side: column perm[j] of Q1 Vx
      int j, r;
      if (!herm) {
        j = (int)(t % nn);
        r = (int)(t / nn);
      } else {
        r = (int)(t % mm);
        j = (int)(t / mm);
      }
      double2 y = Cx<CPLX>::ld(ut, r + (long long)perm[j] * mm);
      if (!herm) {
        Cx<CPLX>::st(U, rows[r] * K + koff + j, y);
      } else {
        y.y = -y.y;
        Cx<CPLX>::st(Vt, (koff + j) * ncol + cols[r], y);
      }
    } else {                        // square side: column j of the completed Ux, times the phase of R_jj of the completion
      const long long t2 = t - tott;
      int j, c;
      if (!herm) {
        c = (int)(t2 % nn);
        j = (int)(t2 / nn);
      } else {
        j = (int)(t2 % nn);
        c = (int)(t2 / nn);
      }
      double2 d = Cx<CPLX>::ld(un, j + (long long)j * nn);
      if (d.x == 0.0 && d.y == 0.0) d = make_double2(1.0, 0.0);
      const double2 x = Cx<CPLX>::ld(q, c + (long long)j * nn);
      double2 y = make_double2(x.x * d.x - x.y * d.y, x.x * d.y + x.y * d.x);
      if (!herm) {
        y.y = -y.y;
        Cx<CPLX>::st(Vt, (koff + j) * ncol + cols[c], y);
      } else {
        Cx<CPLX>::st(U, rows[c] * K + koff + j, y);
      }
    }
  }
}

// null-space vectors of the taller side: the columns nn .. nn + extra of the tall block's Q factor
template <bool CPLX>
__global__ void k_scatter_null2_b(double* U, double* Vt, const double* __restrict__ q1_base, long long ldU,
                                  long long ncol, const long long* __restrict__ rows_all,
                                  const long long* __restrict__ cols_all, const SvdBlk* __restrict__ tall) {
  const SvdBlk B = tall[blockIdx.y];
  if (B.extra <= 0) return;
  const int mm = B.mm, nn = B.nn, extra = B.extra;
  const double* q = q1_base + B.q1_off * Cx<CPLX>::E;
  const long long* rows = rows_all + B.row_off;
  const long long* cols = cols_all + B.col_off;
  const long long total = (long long)mm * extra;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    if (!B.herm) {
      const int e = (int)(t % extra), r = (int)(t / extra);
      Cx<CPLX>::st(U, rows[r] * ldU + B.null_off + e, Cx<CPLX>::ld(q, r + (long long)(nn + e) * mm));
    } else {
      const int r = (int)(t % mm), e = (int)(t / mm);
      double2 x = Cx<CPLX>::ld(q, r + (long long)(nn + e) * mm);
      x.y = -x.y;
      Cx<CPLX>::st(Vt, (B.null_off + e) * ncol + cols[r], x);
    }
  }
}

template <bool CPLX>
int block_svd_batched(mpse_ctx* ctx, const void* coef, int64_t nrow, int64_t ncol, int nblocks, const int64_t* row_idx,
                      const int64_t* row_off, const int64_t* col_idx, const int64_t* col_off, void* U, void* Vt,
                      double* S_host, int64_t K, const int64_t* extra_host, int64_t KU, int64_t KV) {
  constexpr size_t es = CPLX ? 16 : 8;
  constexpr int E = CPLX ? 2 : 1;
  // tall[b]: the gathered block (mm x nn, mm >= nn; wide blocks as their adjoint) - QR factorised first;
  // sq[b]: the nn x nn problem X = R^H the Jacobi sweeps run on
  std::vector<SvdBlk> tall, sq;
  long long ws_tot = 0, q1_tot = 0, x_tot = 0, sig_tot = 0, koff = 0, uoff = K, voff = K;
  int maxN = 0, maxnn = 0;
  long long max_tall = 1, max_sq = 1;
  for (int b = 0; b < nblocks; ++b) {
    const int m = (int)(row_off[b + 1] - row_off[b]), n = (int)(col_off[b + 1] - col_off[b]);
    const int k = std::min(m, n);
    if (k == 0) continue;
    SvdBlk B;
    memset(&B, 0, sizeof(B));
    B.herm = m < n ? 1 : 0;
    B.mm = B.herm ? n : m;
    B.nn = B.herm ? m : n;
    B.mm0 = B.mm;
    B.N = (B.nn + 1) & ~1;
    B.extra = extra_host ? (int)extra_host[b] : 0;
    B.ws_off = ws_tot, B.q1_off = q1_tot, B.sig_off = (int)sig_tot;
    B.row_off = row_off[b], B.col_off = col_off[b];
    B.koff = koff;
    B.null_off = B.herm ? voff : uoff;
    (B.herm ? voff : uoff) += B.extra;
    SvdBlk S = B;
    S.mm = S.nn;                      // (thresholds keep the tall dimension: mm0)
    S.extra = 0;
    S.ws_off = x_tot, S.v_off = x_tot, S.q_off = x_tot;
    S.tol = 2.220446049250313e-16 * std::sqrt((double)B.mm0);
    ws_tot += (long long)B.mm * B.nn;
    q1_tot += (long long)B.mm * (B.nn + B.extra);
    x_tot += (long long)B.nn * B.nn;
    sig_tot += B.nn;
    koff += k;
    maxN = std::max(maxN, B.N);
    maxnn = std::max(maxnn, B.nn);
    max_tall = std::max(max_tall, (long long)B.mm * (B.nn + B.extra) + (long long)B.nn * B.nn);
    max_sq = std::max(max_sq, (long long)B.nn * B.nn);
    tall.push_back(B);
    sq.push_back(S);
  }
  const int nblk = (int)tall.size();
  // whole-call timing for bench.py (variant 6): the algorithmic bytes depend on the sweep count, filled in below
  ProfScope sprof(ctx, 6, 0.0, 0.0);
  const bool spt = sprof.on;
  int sweeps_done = 0;
  MPSE_TRY(mpse_memset_zero(ctx, U, size_t(nrow * KU) * es));
  MPSE_TRY(mpse_memset_zero(ctx, Vt, size_t(KV * ncol) * es));
  const int64_t nri = row_off[nblocks], nci = col_off[nblocks];
  TmpBuf IDX(ctx), DB(ctx), WS(ctx), Q1(ctx), PRM1(ctx), X(ctx), UN(ctx), QX(ctx), VM(ctx), PRM2(ctx), SIG(ctx), PERM(ctx),
      ST(ctx);
  MPSE_TRY(IDX.alloc(size_t(nri + nci) * 8));
  MPSE_TRY(DB.alloc(size_t(2 * nblk) * sizeof(SvdBlk)));
  MPSE_TRY(WS.alloc(size_t(ws_tot) * es));
  MPSE_TRY(Q1.alloc(size_t(q1_tot) * es));
  MPSE_TRY(PRM1.alloc(size_t(sig_tot + 1) * sizeof(HhParam)));
  MPSE_TRY(X.alloc(size_t(x_tot) * es));
  MPSE_TRY(UN.alloc(size_t(x_tot) * es));
  MPSE_TRY(QX.alloc(size_t(x_tot) * es));
  MPSE_TRY(VM.alloc(size_t(x_tot) * es));
  MPSE_TRY(PRM2.alloc(size_t(sig_tot + 1) * sizeof(HhParam)));
  MPSE_TRY(SIG.alloc(size_t(sig_tot) * 8));
  MPSE_TRY(PERM.alloc(size_t(sig_tot) * 8));
  // per block: null2 (double), thresh (double), nrot (int), done (int)
  const int nblk_pad = (nblk + 1) & ~1;     // `done` is read back as doubles: keep it 8-byte aligned
  MPSE_TRY(ST.alloc(size_t(nblk_pad) * (8 + 8 + 4 + 4) + 64));
  double* null2 = ST.as<double>();
  double* thresh = null2 + nblk_pad;
  int* nrot = reinterpret_cast<int*>(thresh + nblk_pad);
  int* done = nrot + nblk_pad;
  MPSE_TRY(stage_h2d(ctx, IDX.p, row_idx, size_t(nri) * 8));
  MPSE_TRY(stage_h2d(ctx, IDX.as<char>() + size_t(nri) * 8, col_idx, size_t(nci) * 8));
  MPSE_TRY(stage_h2d(ctx, DB.p, tall.data(), size_t(nblk) * sizeof(SvdBlk)));
  MPSE_TRY(stage_h2d(ctx, DB.as<SvdBlk>() + nblk, sq.data(), size_t(nblk) * sizeof(SvdBlk)));
  const long long* drows = IDX.as<long long>();
  const long long* dcols = IDX.as<long long>() + nri;
  const SvdBlk* dtall = DB.as<SvdBlk>();
  const SvdBlk* dsq = DB.as<SvdBlk>() + nblk;
  double* ws = WS.as<double>();
  double* xs = X.as<double>();
  double* vm = VM.as<double>();
  double* sigd = SIG.as<double>();
  int gt = ew_blocks(max_tall), gs = ew_blocks(max_sq);
  if (gt > 256) gt = 256;
  if (gs > 256) gs = 256;
  // ---- 1. gather, QR of every tall block (R in place, Q1 with the null-space columns the caller asked for)
  hipLaunchKernelGGL((k_gather_blocks<CPLX>), dim3(gt, nblk), dim3(256), 0, ctx->stream, ws, (const double*)coef,
                     (long long)ncol, drows, dcols, dtall);
  MPSE_HIP(ctx, hipGetLastError());
  {
    std::vector<QrBlk> qb((size_t)nblk);
    for (int b = 0; b < nblk; ++b) {
      const SvdBlk& B = tall[b];
      qb[b] = QrBlk{B.ws_off, B.q1_off, B.mm, B.nn, B.nn, B.sig_off, B.nn + B.extra};
    }
    MPSE_TRY(hh_qr(ctx, CPLX, ws, Q1.as<double>(), PRM1.as<HhParam>(), qb.data(), nblk, true));
  }
  // ---- 2. X = R^H, V = I, one-sided Jacobi on the square problems
  // (X is formed in the buffer of the normalised copy and sorted into its own: columns by decreasing norm)
  double* xraw = UN.as<double>();
  hipLaunchKernelGGL((k_rh_blocks<CPLX>), dim3(gs, nblk), dim3(256), 0, ctx->stream, xraw, (const double*)ws, dtall, dsq);
  hipLaunchKernelGGL((k_col_norms_b<CPLX>), dim3(maxnn, nblk), dim3(RED_THREADS), 0, ctx->stream, (const double*)xraw, dsq,
                     sigd);
  hipLaunchKernelGGL(k_null2, dim3(nblk), dim3(64), 0, ctx->stream, dsq, (const double*)sigd, null2, nrot, done);
  MPSE_HIP(ctx, hipGetLastError());
  {
    std::vector<double> sig0((size_t)sig_tot);
    MPSE_TRY(mpse_memcpy_d2h(ctx, sig0.data(), sigd, size_t(sig_tot) * 8));
    std::vector<long long> p0((size_t)sig_tot);
    for (const SvdBlk& B : sq) {
      long long* p = p0.data() + B.sig_off;
      const double* sg = sig0.data() + B.sig_off;
      std::iota(p, p + B.nn, 0LL);
      std::stable_sort(p, p + B.nn, [&](long long x, long long y) { return sg[x] > sg[y]; });
    }
    MPSE_TRY(stage_h2d(ctx, PERM.p, p0.data(), size_t(sig_tot) * 8));
    hipLaunchKernelGGL((k_sort_cols_b<CPLX>), dim3(gs, nblk), dim3(256), 0, ctx->stream, xs, vm, (const double*)xraw,
                       PERM.as<const long long>(), dsq);
    MPSE_HIP(ctx, hipGetLastError());
  }
  // Which block step runs the sweeps: the column kernel in LDS (k_jacobi_block) where the column blocks of X and V fit
  // the granted dynamic LDS (4 JB_COLS columns of the widest block: nn <= 300 complex, 600 real at 150 KB; 128 / 256
  // where the runtime keeps the kernel to 64 KB), the Gram kernel (k_jacobi_gram) for wider blocks.  MPSE_SVD_GRAM=2:
  // the Gram kernel for every size (read per call: tests switch it).  mpse_block_svd_stats says which one ran.
  const bool gram_all = [] {
    const char* e = getenv("MPSE_SVD_GRAM");
    return e && atoi(e) >= 2;
  }();
  const int gram_r_env = [] {
    const char* e = getenv("MPSE_SVD_GRAM_R");     // row slabs per column-block pair (default: a 16-row tile per wave)
    return e ? atoi(e) : 0;
  }();
  TmpBuf X2(ctx), VM2(ctx), DG(ctx);
  double2* dgbuf[2] = {nullptr, nullptr};
  double* xbuf[2] = {xs, nullptr};
  double* vbuf[2] = {vm, nullptr};
  int cur = 0;                      // which copy of X, V holds the state (Gram kernel: every launch writes the other)
  if (maxN > 1) {
    std::vector<int> hdone(nblk, 0);
    bool all = false;
    const size_t gram_lds = size_t(2) * 32 * 32 * 16 + size_t(32) * 33 * 16 + size_t(2) * 1536 * 8;
    static const bool gram_attr = [&] {
      const hipError_t a = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_jacobi_gram<true>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)gram_lds);
      const hipError_t b = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_jacobi_gram<false>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)gram_lds);
      (void)hipGetLastError();
      return a == hipSuccess && b == hipSuccess;
    }();
    const size_t blk_lds = size_t(4) * JB_COLS * maxnn * es;      // X and V columns of a pair of column blocks
    // beyond the default 64 KB of dynamic LDS (the CU has 160 KB): asked for once; a runtime that refuses keeps the
    // column kernel to the problems that fit 64 KB
    static const bool lds_attr = [] {
      const hipError_t a = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_jacobi_block<true>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
      const hipError_t b = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_jacobi_block<false>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
      (void)hipGetLastError();
      return a == hipSuccess && b == hipSuccess;
    }();
    const size_t col_lds = (lds_attr ? size_t(150) : size_t(64)) * 1024;
    const bool cols_fit = blk_lds <= col_lds;
    const bool use_gram = gram_all || !cols_fit;
    ctx->svd_stats[mpse_ctx::SV_COL_LDS] = (long long)col_lds;
    if (use_gram && !gram_attr)
      return mpse_fail(ctx, MPSE_ERR_HIP, "block_svd: the runtime refused %zu bytes of dynamic LDS to the Gram step",
                       gram_lds);
    int gram_R = 1;
    if (use_gram) {
      MPSE_TRY(X2.alloc(size_t(x_tot) * es));
      MPSE_TRY(VM2.alloc(size_t(x_tot) * es));
      xbuf[1] = X2.as<double>();
      vbuf[1] = VM2.as<double>();
      // the diagonal Gram tiles that travel with the column blocks (two copies like X and V)
      const size_t dg_elems = size_t(nblk) * size_t((((maxnn + JG - 1) / JG + 1) & ~1)) * 256;
      MPSE_TRY(DG.alloc(2 * dg_elems * 16));
      dgbuf[0] = DG.as<double2>();
      dgbuf[1] = DG.as<double2>() + dg_elems;
      const int tiles = 2 * ((maxnn + 15) / 16), pairs = (((maxnn + JG - 1) / JG + 1) & ~1) / 2;
      gram_R = gram_r_env > 0 ? gram_r_env : (tiles + 3) / 4;      // (a 16-row tile per wave)
      while (gram_R > 1 && (long long)gram_R * pairs * nblk > 1024) gram_R >>= 1;
      if (gram_R < 1) gram_R = 1;
      if (gram_R > 16) gram_R = 16;
      ctx->svd_stats[mpse_ctx::SV_GRAM_R] = gram_R;
    }
    ++ctx->svd_stats[mpse_ctx::SV_DECOMP];
    ++ctx->svd_stats[use_gram ? mpse_ctx::SV_GRAM : mpse_ctx::SV_COLUMN];
    for (int sweep = 0; sweep < 60 && !all; ++sweep) {
      if (use_gram) {
        const int nbmax = ((maxnn + JG - 1) / JG + 1) & ~1;
        for (int step = 0; step < nbmax - 1; ++step) {
          hipLaunchKernelGGL((k_jacobi_gram<CPLX>), dim3(nbmax / 2 * gram_R, nblk), dim3(256), gram_lds, ctx->stream,
                             (const double*)xbuf[cur], xbuf[cur ^ 1], (const double*)vbuf[cur], vbuf[cur ^ 1],
                             (const double2*)dgbuf[cur], dgbuf[cur ^ 1], nbmax, dsq, step, gram_R, (const double*)null2, nrot,
                             (const int*)done);
          cur ^= 1;
        }
        ctx->svd_stats[mpse_ctx::SV_LAUNCHES] += nbmax - 1;
      } else {
        const int nbmax = ((maxnn + JB_COLS - 1) / JB_COLS + 1) & ~1;
        for (int step = 0; step < nbmax - 1; ++step)
          hipLaunchKernelGGL((k_jacobi_block<CPLX>), dim3(nbmax / 2, nblk), dim3(64 * JB_COLS), blk_lds, ctx->stream, xs,
                             vm, dsq, step, (const double*)null2, nrot, (const int*)done);
        ctx->svd_stats[mpse_ctx::SV_LAUNCHES] += nbmax - 1;
      }
      hipLaunchKernelGGL(k_sweep_end, dim3((nblk + 255) / 256), dim3(256), 0, ctx->stream, nblk, nrot, done);
      MPSE_HIP(ctx, hipGetLastError());
      // one read-back per sweep for all blocks
      if (nblk <= 2000) {
        MPSE_TRY(publish_and_wait(ctx, reinterpret_cast<const double*>(done), (nblk + 1) / 2, mpse_ctx::PIN_FLAG));
        memcpy(hdone.data(), ctx->pinned + mpse_ctx::PIN_FLAG, size_t(nblk) * sizeof(int));
      } else {
        MPSE_TRY(mpse_memcpy_d2h(ctx, hdone.data(), done, size_t(nblk) * sizeof(int)));
      }
      all = true;
      for (int b = 0; b < nblk; ++b) all = all && hdone[b];
      ++sweeps_done;
      ++ctx->svd_stats[mpse_ctx::SV_SWEEPS];
    }
    if (!all) return mpse_fail(ctx, MPSE_ERR_NOCONV, "block_svd: Jacobi did not converge within 60 sweeps");
  }
  xs = xbuf[cur];
  vm = vbuf[cur];
  hipLaunchKernelGGL((k_col_norms_b<CPLX>), dim3(maxnn, nblk), dim3(RED_THREADS), 0, ctx->stream, (const double*)xs, dsq,
                     sigd);
  std::vector<double> sig((size_t)sig_tot), th((size_t)nblk);
  MPSE_TRY(mpse_memcpy_d2h(ctx, sig.data(), sigd, size_t(sig_tot) * 8));
  std::vector<long long> perm((size_t)sig_tot);
  for (int b = 0; b < nblk; ++b) {
    const SvdBlk& B = sq[b];
    long long* p = perm.data() + B.sig_off;
    const double* sg = sig.data() + B.sig_off;
    std::iota(p, p + B.nn, 0LL);
    std::stable_sort(p, p + B.nn, [&](long long x, long long y) { return sg[x] > sg[y]; });
    for (int j = 0; j < B.nn; ++j) S_host[B.koff + j] = sg[p[j]];
    th[b] = sg[p[0]] * 2.220446049250313e-16 * (double)B.mm0;
  }
  MPSE_TRY(stage_h2d(ctx, PERM.p, perm.data(), size_t(sig_tot) * 8));
  MPSE_TRY(stage_h2d(ctx, thresh, th.data(), size_t(nblk) * 8));
  // ---- 3. Ux: the normalised columns of X, null columns zeroed, completed to an isometry (Householder QR of the
  // normalised matrix, all blocks in the same launches)
  double* un = UN.as<double>();
  hipLaunchKernelGGL((k_normalise_perm_b<CPLX>), dim3(gs, nblk), dim3(256), 0, ctx->stream, un, (const double*)xs, dsq,
                     (const double*)sigd, PERM.as<const long long>(), (const double*)thresh);
  MPSE_HIP(ctx, hipGetLastError());
  {
    std::vector<QrBlk> qb((size_t)nblk);
    for (int b = 0; b < nblk; ++b) {
      const SvdBlk& B = sq[b];
      qb[b] = QrBlk{B.ws_off, B.q_off, B.nn, B.nn, B.nn, B.sig_off, B.nn};
    }
    MPSE_TRY(hh_qr(ctx, CPLX, un, QX.as<double>(), PRM2.as<HhParam>(), qb.data(), nblk, true));
  }
  // ---- 4. left vectors of the tall blocks: Q1[:, :nn] Vx through the contraction kernel (into the workspace the
  // factored block no longer needs), then both sides to their places
  for (int b = 0; b < nblk; ++b) {
    const SvdBlk& B = tall[b];
    const SvdBlk& S = sq[b];
    const int dt = CPLX ? MPSE_C128 : MPSE_F64;
    MPSE_TRY(gemm_call(ctx, dt, dt, 0, 0, idx1(B.mm, 1), idx1(B.nn, B.mm), idx1(B.nn, 1), idx1(B.nn, B.nn), idx1(B.mm, 1),
                       idx1(B.nn, B.mm), 1, 0, 0, 0, Q1.as<char>() + size_t(B.q1_off) * es, reinterpret_cast<char*>(vm) + size_t(S.v_off) * es,
                       WS.as<char>() + size_t(B.ws_off) * es));
  }
  hipLaunchKernelGGL((k_scatter_svd2_b<CPLX>), dim3(gt, nblk), dim3(256), 0, ctx->stream, (double*)U, (double*)Vt,
                     (const double*)ws, (const double*)un, (const double*)QX.as<double>(), PERM.as<const long long>(),
                     (long long)KU, (long long)ncol, drows, dcols, dtall, dsq);
  if (uoff > K || voff > K)
    hipLaunchKernelGGL((k_scatter_null2_b<CPLX>), dim3(gt, nblk), dim3(256), 0, ctx->stream, (double*)U, (double*)Vt,
                       (const double*)Q1.as<double>(), (long long)KU, (long long)ncol, drows, dcols, dtall);
  MPSE_HIP(ctx, hipGetLastError());
  if (spt) {
    // one sweep = nn (nn - 1) / 2 pairs on nn-row columns of X and V: a pair reads its two columns (Gram entries), reads
    // and writes them again (rotation): 3 passes over 4 nn elements.  Rotations that are skipped (converged pairs, null
    // columns) make the real traffic smaller: an upper bound, like the flops (dots 3 x 8 + rotation 2 x 12 real flops
    // per complex row pair); the QR of the tall blocks and the final product are counted as well.
    double bytes = 0.0, flops = 0.0;
    for (const SvdBlk& B : tall) {
      const double pairs = 0.5 * B.nn * (B.nn - 1.0) * sweeps_done, rows = 2.0 * B.nn;
      bytes += pairs * 3.0 * 2.0 * rows * double(es) + 3.0 * double(B.mm) * B.nn * double(es);
      flops += pairs * rows * (CPLX ? 48.0 : 12.0) +
               (CPLX ? 4.0 : 1.0) * (4.0 * B.mm * double(B.nn) * B.nn - 4.0 * double(B.nn) * B.nn * B.nn / 3.0) +
               (CPLX ? 8.0 : 2.0) * double(B.mm) * B.nn * B.nn;
    }
    sprof.rec.bytes = bytes;
    sprof.rec.flops = flops;
    ctx->prof_svd_sweeps += sweeps_done;
    sprof.end();
  }
  (void)E;
  return MPSE_OK;
}

// argument and shape checks; every block height then takes the path above
template <bool CPLX>
int block_svd_impl(mpse_ctx* ctx, const void* coef, int64_t nrow, int64_t ncol, int nblocks, const int64_t* row_idx,
                   const int64_t* row_off, const int64_t* col_idx, const int64_t* col_off, void* U, void* Vt,
                   double* S_host, int64_t K, const int64_t* extra_host, int64_t KU, int64_t KV) {
  int64_t ktot = 0, nu = 0, nv = 0;
  for (int b = 0; b < nblocks; ++b) {
    const int64_t m = row_off[b + 1] - row_off[b], n = col_off[b + 1] - col_off[b];
    if (m < 0 || n < 0) return mpse_fail(ctx, MPSE_ERR_SHAPE, "block_svd: negative block extent");
    const int64_t k = std::min(m, n);
    ktot += k;
    int64_t ex = extra_host ? extra_host[b] : 0;
    if (ex < 0 || ex > std::max(m, n) - k) return mpse_fail(ctx, MPSE_ERR_SHAPE, "block_svd: bad extra count");
    if (k == 0) ex = 0;
    if (m >= n) nu += ex; else nv += ex;
  }
  if (KU != ktot + nu || KV != ktot + nv)
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "block_svd: KU/KV (%lld,%lld) do not match the blocks (%lld,%lld)",
                     (long long)KU, (long long)KV, (long long)(ktot + nu), (long long)(ktot + nv));
  if (ktot != K) return mpse_fail(ctx, MPSE_ERR_SHAPE, "block_svd: K=%lld but blocks give %lld", (long long)K, (long long)ktot);
  if (ktot == 0) return mpse_fail(ctx, MPSE_ERR_SHAPE, "Invalid quantum number");
  return block_svd_batched<CPLX>(ctx, coef, nrow, ncol, nblocks, row_idx, row_off, col_idx, col_off, U, Vt, S_host, K,
                                 extra_host, KU, KV);
}

}  // namespace

extern "C" int mpse_block_svd_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  return stats_out(ctx, &mpse_ctx::svd_stats, counts, n);
}

extern "C" int mpse_block_svd_full(mpse_ctx* ctx, int dtype, const void* coef, int64_t nrow, int64_t ncol, int nblocks,
                                   const int64_t* row_idx_host, const int64_t* row_off_host,
                                   const int64_t* col_idx_host, const int64_t* col_off_host,
                                   const int64_t* extra_host, void* U, int64_t KU, void* Vt, int64_t KV,
                                   double* S_host, int64_t K) {
  if (!ctx || !coef || !U || !Vt || !S_host || !row_idx_host || !row_off_host || !col_idx_host || !col_off_host)
    return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (nblocks <= 0) return mpse_fail(ctx, MPSE_ERR_SHAPE, "Invalid quantum number");
  if (dtype == MPSE_C128)
    return block_svd_impl<true>(ctx, coef, nrow, ncol, nblocks, row_idx_host, row_off_host, col_idx_host,
                                col_off_host, U, Vt, S_host, K, extra_host, KU, KV);
  if (dtype == MPSE_F64)
    return block_svd_impl<false>(ctx, coef, nrow, ncol, nblocks, row_idx_host, row_off_host, col_idx_host,
                                 col_off_host, U, Vt, S_host, K, extra_host, KU, KV);
  return mpse_fail(ctx, MPSE_ERR_ARG, "block_svd: unknown dtype");
}

extern "C" int mpse_block_svd(mpse_ctx* ctx, int dtype, const void* coef, int64_t nrow, int64_t ncol, int nblocks,
                              const int64_t* row_idx_host, const int64_t* row_off_host, const int64_t* col_idx_host,
                              const int64_t* col_off_host, void* U, void* Vt, double* S_host, int64_t K) {
  return mpse_block_svd_full(ctx, dtype, coef, nrow, ncol, nblocks, row_idx_host, row_off_host, col_idx_host,
                             col_off_host, nullptr, U, K, Vt, K, S_host, K);
}
