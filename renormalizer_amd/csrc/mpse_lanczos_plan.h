// The integer rules of the asynchronous Lanczos solve (mpse_lanczos.hip): its schedule - how far the host runs ahead of
// the decision, how the basis grows, which iterations carry a check - and the layout of a member's region of the slab.
// Host code only, no HIP: tests/host_emu/lanczos_plan_emu.cpp compiles this header with g++.
#pragma once
#include <cstdint>

namespace mpse_lz {

constexpr int LZ_MAXM = 64;       // one wavefront holds the Krylov coefficients
// <H U_j, U_j> partials a matvec may write: room for 4096 producers (the fused bond / two-level-site matvec has up to
// (D / 16) w (D / 64) d workgroups per unit share, mpse_heff0.hip)
constexpr int LZ_DOT_CAP = 4096;
constexpr int LZ_NORM_CAP = 512;  // |.|^2 partials of the vector kernels (RED_MAX_BLOCKS, mpse_device.h)
// recurrence scalars as in the synchronous solve: [0..1] |v|^2 ; per j: alpha at 4 + 4 j, beta^2 at 6 + 4 j
constexpr int LZ_SCALARS = 4 + 4 * 130;
constexpr int LZ_CTL_DOUBLES = 4;   // sizeof(LzCtl) / 8

// A single solve and the members of a batch share the schedule: a batched member returns the bits of its single solve.
// ``hint``: Krylov dimension of the last solve of the same problem class (0: none, mpse_ctx::lz_hint).
struct Schedule {
  int limit;                // iterations the decision on the device covers: one wavefront of coefficients
  int wait_from;            // first wait at the check that can confirm the hinted dimension (or the first that can decide at all)
  int cap;                  // capacity of the basis, vectors
  Schedule(int hint, int max_dim) : limit(max_dim < LZ_MAXM ? max_dim : LZ_MAXM) {
    wait_from = hint - 1 > 6 ? hint - 1 : 6;
    cap = hint + 4 > 16 ? hint + 4 : 16;
    if (cap > limit + 1) cap = limit + 1;
  }
  int grown() const { return cap * 2 < limit + 1 ? cap * 2 : limit + 1; }
  // Iteration j: does it carry a check (krylov.py:76-81), is it the last one.  The first check of a solve (j = 4) cannot
  // stop it - there is no earlier estimate to compare with - so it is evaluated together with the second one (j = 6,
  // `merged`): one pass over the basis forms both estimates, and a solve has three small launches and ~25 us of
  // dependent latency less.
  struct Step {
    bool check, last, merged;
  };
  Step at(int j, bool have_prev) const {
    Step st{j > 3 && j % 2 == 0, j + 1 >= limit, false};
    if (st.check && !have_prev && j == 4 && j + 3 < limit) st.check = false;   // (its turn comes at j = 6)
    if (st.check && !have_prev && j == 6) st.merged = true;
    return st;
  }
};

// A member's region of the slab, offsets in doubles.  Sections start on 256-byte boundaries, in this order:
//   scalars | control block | coefficients, flag word, dot partials, two norm-partial areas, result parts, spare
//   estimate, basis
// The basis comes last so that it can grow: a larger capacity moves nothing in front of it.  Member m of a launch set
// has every section `stride` doubles behind member m - 1.
struct Layout {
  int64_t scal, ctl, coef;       // one section: LZ_SCALARS doubles, the control block, 4 LZ_MAXM coefficients
  int64_t flag, dot, norm[2], parts, spare, basis;
  int64_t stride;
};
inline int64_t align32(int64_t doubles) { return (doubles + 31) & ~int64_t(31); }
// n elements per vector (complex: two doubles each), `parts` result parts of n elements, room for dot_cap dot partials
// and `cap` basis vectors
inline Layout layout(int64_t n, bool cplx, int parts, int dot_cap, int cap) {
  const int64_t nd = n * (cplx ? 2 : 1);
  Layout l;
  l.scal = 0;
  l.ctl = LZ_SCALARS;
  l.coef = l.ctl + 8;
  l.flag = align32(l.coef + 4 * LZ_MAXM);
  l.dot = l.flag + 32;
  l.norm[0] = l.dot + align32(2 * int64_t(dot_cap));
  l.norm[1] = l.norm[0] + align32(2 * int64_t(LZ_NORM_CAP));
  l.parts = l.norm[1] + align32(2 * int64_t(LZ_NORM_CAP));
  l.spare = l.parts + align32(parts * nd);
  l.basis = l.spare + align32(nd);
  l.stride = l.basis + align32(cap * nd);
  return l;
}

}  // namespace mpse_lz
