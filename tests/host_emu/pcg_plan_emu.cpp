// Host view of the integer rules of the conjugate-gradient solver (renormalizer_amd/csrc/mpse_pcg_plan.h), for
// tests/test_pcg_plan_host.py.
#include "../../renormalizer_amd/csrc/mpse_pcg_plan.h"

extern "C" {

int emu_waits_at(int k, int max_iter) { return mpse_pcg_plan::waits_at(k, max_iter) ? 1 : 0; }

int emu_default_max_iter(long long n) { return mpse_pcg_plan::default_max_iter(n); }

// out = {ctl, part_bb, part_bx, part_rz[0], part_rz[1], part_pq, y, q, r, p, extra_y, end, stride, vec} in bytes
void emu_layout(long long n, int cplx, int nb, int nbq, int extra_y, long long* out) {
  const mpse_pcg_plan::Layout l = mpse_pcg_plan::layout(n, cplx != 0, nb, nbq, extra_y);
  const size_t v[14] = {l.ctl, l.part_bb, l.part_bx, l.part_rz[0], l.part_rz[1], l.part_pq, l.y,
                        l.q,   l.r,       l.p,       l.extra_y,    l.end,        l.stride,  l.vec};
  for (int i = 0; i < 14; ++i) out[i] = (long long)v[i];
}

// {PCG_K, PCG_CW}
void emu_constants(int* out) { out[0] = mpse_pcg_plan::PCG_K, out[1] = mpse_pcg_plan::PCG_CW; }

}  // extern "C"
