// TEST INFRASTRUCTURE: the plans of the two-leg, two-layer operator (mpse_plans.h: plan_heff_ft, plan_env_ft) through the
// naive executor of plan_emu.cpp, for tests/test_plans_ft_host.py.  Never linked into libmpsengine.so.
#include "plan_emu.cpp"

// largest element offset an index map reaches
static int64_t span(const mpse_index& m) {
  if (m.ext <= 0) return 0;
  if (m.lo_ext >= m.ext) return (m.ext - 1) * m.s_lo;
  return ((m.ext - 1) / m.lo_ext) * m.s_hi + (m.lo_ext - 1) * m.s_lo;
}
// every access of a step to an intermediate (B_T1 .. B_T3) must stay inside the plan's tmp_elems: the executor
// allocates exactly that much on the device.  (All strides of these plans are non-negative.)
static bool temporaries_fit(const Plan& p) {
  for (const Step& s : p.steps) {
    const int64_t nb = s.batch > 1 ? s.batch - 1 : 0;
    const int buf[3] = {s.a, s.b, s.c};
    const int64_t last[3] = {s.a_off + nb * s.sba + span(s.ma) + span(s.ka), s.b_off + nb * s.sbb + span(s.kb) + span(s.nb),
                             s.c_off + nb * s.sbc + span(s.mc) + span(s.nc)};
    for (int i = 0; i < 3; ++i)
      if (buf[i] >= B_T1 && buf[i] <= B_T3 && last[i] >= p.tmp_elems[buf[i] - B_T1]) return false;
  }
  return true;
}

extern "C" int emu_heff_apply_ft(int dtype, const mpse_heff_ft* h, const void* C, void* out) {
  Plan p = plan_heff_ft(dtype, *h);
  if (!p.error && !temporaries_fit(p)) return -1;
  const void* bufs[B_COUNT] = {nullptr};
  bind_heff_ft(bufs, *h, C, out);
  return run(dtype, p, bufs);
}

extern "C" int emu_env_update_ft(int dtype, int domain, const mpse_heff_ft* h, const void* env, int env_dtype,
                                 const void* X, void* out) {
  Plan p = plan_env_ft(dtype, domain, *h, env_dtype);
  if (!p.error && !temporaries_fit(p)) return -1;
  const void* const W[2] = {h->W1, h->W2};
  const void* bufs[B_COUNT] = {nullptr};
  bind_env(bufs, env, X, X, out, 2, W);
  return run(dtype, p, bufs);
}

// number of plan steps and whether they equal those of plan_heff2 on the same operands (d_down == 1, both layers up,
// transposed, one MPO site): the reason a one-term summed solve reproduces the two-layer solve bit for bit
extern "C" int emu_ft_steps_equal_heff2(int dtype, const mpse_heff_ft* h) {
  mpse_heff g;
  memset(&g, 0, sizeof(g));
  g.nsite = 1;
  g.dims.Dl_ket = h->Dl, g.dims.Dr_ket = h->Dr, g.dims.d0 = h->d_up, g.dims.danc = 1;
  g.dims.wl = h->wl1, g.dims.wr = h->wr1;
  g.L = h->L, g.R = h->R, g.W0 = h->W1, g.l_dtype = h->l_dtype, g.r_dtype = h->r_dtype, g.w_dtype = h->w_dtype;
  Plan a = plan_heff_ft(dtype, *h), b = plan_heff2(dtype, g);
  if (a.error || b.error || a.steps.size() != b.steps.size()) return 0;
  auto same = [](const mpse_index& x, const mpse_index& y) {
    return x.ext == y.ext && x.lo_ext == y.lo_ext && x.s_hi == y.s_hi && x.s_lo == y.s_lo;
  };
  for (size_t i = 0; i < a.steps.size(); ++i) {
    const Step &s = a.steps[i], &t = b.steps[i];
    const bool w2 = i == 2;      // the second layer reads B_W1 here, B_W0 there: the same site in this comparison
    if (s.a != (w2 && t.a == B_W0 ? B_W1 : t.a) || s.b != t.b || s.c != t.c || s.a_off != t.a_off || s.b_off != t.b_off ||
        s.c_off != t.c_off || s.dta != t.dta || s.dtb != t.dtb || s.conja != t.conja || s.conjb != t.conjb ||
        !same(s.ma, t.ma) || !same(s.ka, t.ka) || !same(s.kb, t.kb) || !same(s.nb, t.nb) || !same(s.mc, t.mc) ||
        !same(s.nc, t.nc) || s.batch != t.batch || s.sba != t.sba || s.sbb != t.sbb || s.sbc != t.sbc ||
        s.kind != t.kind || s.beta != t.beta)
      return 0;
  }
  return (int)a.steps.size();
}
