// Host view of the integer rules of the asynchronous Lanczos solve (renormalizer_amd/csrc/mpse_lanczos_plan.h), for
// tests/test_lanczos_plan_host.py.
#include "../../renormalizer_amd/csrc/mpse_lanczos_plan.h"

extern "C" {

// out = {limit, wait_from, cap, grown()}
void emu_schedule(int hint, int max_dim, int* out) {
  const mpse_lz::Schedule s(hint, max_dim);
  out[0] = s.limit, out[1] = s.wait_from, out[2] = s.cap, out[3] = s.grown();
}

// bit 0: check, bit 1: last, bit 2: merged
int emu_step(int hint, int max_dim, int j, int have_prev) {
  const mpse_lz::Schedule::Step st = mpse_lz::Schedule(hint, max_dim).at(j, have_prev != 0);
  return (st.check ? 1 : 0) | (st.last ? 2 : 0) | (st.merged ? 4 : 0);
}

// out = {scal, flag, dot, norm[0], norm[1], parts, spare, basis, stride, ctl, coef} in doubles
void emu_layout(long long n, int cplx, int parts, int dot_cap, int cap, long long* out) {
  const mpse_lz::Layout l = mpse_lz::layout(n, cplx != 0, parts, dot_cap, cap);
  const int64_t v[11] = {l.scal, l.flag, l.dot, l.norm[0], l.norm[1], l.parts, l.spare, l.basis, l.stride, l.ctl, l.coef};
  for (int i = 0; i < 11; ++i) out[i] = v[i];
}

// {LZ_MAXM, LZ_DOT_CAP, LZ_NORM_CAP, LZ_SCALARS, LZ_CTL_DOUBLES}
void emu_constants(int* out) {
  out[0] = mpse_lz::LZ_MAXM, out[1] = mpse_lz::LZ_DOT_CAP, out[2] = mpse_lz::LZ_NORM_CAP, out[3] = mpse_lz::LZ_SCALARS;
  out[4] = mpse_lz::LZ_CTL_DOUBLES;
}

}  // extern "C"
