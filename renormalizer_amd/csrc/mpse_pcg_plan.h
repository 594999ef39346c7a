// The integer rules of the conjugate-gradient solver (mpse_pcg.hip): when the host waits for the decision, the default
// iteration limit, and the layout of a member's region of the slab - one layout for mpse_pcg, mpse_pcg_sum and the
// members of mpse_pcg_batch.  Host code only, no HIP: tests/host_emu/pcg_plan_emu.cpp compiles this header with g++.
// (namespace mpse_pcg_plan: `mpse_pcg` itself is the exported function)
#pragma once
#include <cstddef>
#include <cstdint>

namespace mpse_pcg_plan {

constexpr int PCG_K = 4;        // the host reads the pinned control block every PCG_K iterations: at most PCG_K - 1
                                // matvecs are enqueued past the decision
constexpr int PCG_CW = 8;       // doubles of the control block (PcgCtl, mpse_pcg.hip)

enum { PCG_WHY_NONE = 0, PCG_WHY_TOL = 1, PCG_WHY_MAXITER = 2, PCG_WHY_CURVATURE = 3, PCG_WHY_DIAG = 4, PCG_WHY_ZERO_B = 5 };

// does the host wait for the control block behind the direction update of iteration k
inline bool waits_at(int k, int max_iter) { return (k % PCG_K == PCG_K - 1) || k >= max_iter; }

// scipy's default, 10 n
inline int default_max_iter(int64_t n) { return n > (int64_t(1) << 27) ? (1 << 30) : int(10 * n); }

// A member's region of the slab, offsets in bytes.  Every section starts on a 256-byte boundary, in this order:
//   control block | partials: |b|^2, b^H x, r^H z twice (by iteration parity), p^H q | y, q, r, p | further y vectors
// Member m of a launch set has every section `stride` bytes behind member m - 1.  A caller with sections of its own
// (the one-launch matvec: transposed left environment, sparse W list) puts them at `end` and moves `stride` behind them.
struct Layout {
  size_t ctl, part_bb, part_bx, part_rz[2], part_pq;
  size_t y, q, r, p;
  size_t extra_y, vec;      // further y vector t (a summed solve's term t + 1) at extra_y + t * vec
  size_t end, stride;
};
inline size_t align256(size_t bytes) { return (bytes + 255) & ~size_t(255); }
// n elements per vector (complex: 16 bytes each), nb partial pairs per reduction of the vector kernels, nbq pairs of
// p^H q (nb from k_pcg_q, one per workgroup of the one-launch matvec), extra_y vectors behind p
inline Layout layout(int64_t n, bool cplx, int nb, int nbq, int extra_y) {
  const size_t pairs = align256(2 * size_t(nb) * sizeof(double));
  Layout l;
  l.vec = align256(size_t(n) * (cplx ? 16 : 8));
  l.ctl = 0;
  l.part_bb = align256(PCG_CW * sizeof(double));
  l.part_bx = l.part_bb + pairs;
  l.part_rz[0] = l.part_bx + pairs;
  l.part_rz[1] = l.part_rz[0] + pairs;
  l.part_pq = l.part_rz[1] + pairs;
  l.y = l.part_pq + align256(2 * size_t(nbq > nb ? nbq : nb) * sizeof(double));
  l.q = l.y + l.vec;
  l.r = l.q + l.vec;
  l.p = l.r + l.vec;
  l.extra_y = l.p + l.vec;
  l.end = l.extra_y + size_t(extra_y) * l.vec;
  l.stride = l.end;
  return l;
}

}  // namespace mpse_pcg_plan
