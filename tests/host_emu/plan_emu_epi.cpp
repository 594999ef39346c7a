// TEST INFRASTRUCTURE: host twin of the folded one-site matvec plan with the epilogue mix (renormalizer_amd/csrc/
// mpse_plans.h: plan_heff1_fold(..., mix_epilogue), GGroupPlan::nmix) through the naive executor of plan_emu.cpp, for
// tests/test_plans_epi_host.py.  Never linked into libmpsengine.so.
#include "plan_emu.cpp"

static void hooks() {
  fold_min() = 1;
  fold_align() = 4;
  fold_split2_min_kt() = 1;
}

// info: steps, K_WMIX steps, K_WMIX destinations, terms on the first product into `out`, terms on later ones, products
// into `out`, two results, temporary elements T1
extern "C" int emu_epi_apply(int dtype, const mpse_heff* h, const void* C, void* out, int mix_epilogue, long long* info) {
  hooks();
  const WSiteInfo wi = analyse_mpo_site((const double*)h->W0, h->dims.wl, h->dims.d0, h->dims.wr);
  Plan p = plan_heff1_fold(dtype, *h, wi, true, mix_epilogue != 0);
  if (p.error) return MPSE_ERR_SHAPE;
  long long r[8] = {(long long)p.steps.size(), 0, 0, 0, 0, 0, p.two_results ? 1 : 0, p.tmp_elems[0]};
  for (const Step& s : p.steps) {
    if (s.kind == K_WMIX) ++r[1], r[2] += (long long)s.mix.size();
    if (s.kind == K_GGEMM && s.groups.size() == 1 && s.groups[0].cbuf == B_OUT && s.groups[0].seg[0].bbuf == B_R) {
      r[r[5] == 0 ? 3 : 4] += s.groups[0].nmix;
      ++r[5];
    }
  }
  memcpy(info, r, sizeof(r));
  return run_fold(dtype, p, h, C, out);
}

// The step list as flat integers: kinds, buffers, offsets (and what else decides what a step does).
// which: 0 = the plan as existing callers ask for it (no trailing argument), 1 = mix_epilogue false, 2 = true.
// Returns the number of integers (or -1: no plan, -2: does not fit).
extern "C" long long emu_epi_steps(int dtype, const mpse_heff* h, int which, long long* rec, long long cap) {
  hooks();
  const WSiteInfo wi = analyse_mpo_site((const double*)h->W0, h->dims.wl, h->dims.d0, h->dims.wr);
  Plan p = which == 0 ? plan_heff1_fold(dtype, *h, wi, true) : plan_heff1_fold(dtype, *h, wi, true, which == 2);
  if (p.error) return -1;
  std::vector<long long> v;
  v.push_back(p.two_results), v.push_back(p.tmp_elems[0]), v.push_back(p.tmp_elems[1]);
  for (const Step& s : p.steps) {
    v.push_back(-1), v.push_back(s.kind);
    for (const GGroupPlan& g : s.groups) {
      v.push_back(-2), v.push_back(g.cbuf), v.push_back(g.c_off), v.push_back((long long)g.beta), v.push_back(g.split2),
          v.push_back(g.nseg), v.push_back(g.nmix);
      for (int q = 0; q < g.nseg; ++q)
        v.push_back(g.seg[q].abuf), v.push_back(g.seg[q].a_off), v.push_back(g.seg[q].bbuf), v.push_back(g.seg[q].b_off);
      for (int u = 0; u < g.nmix; ++u)
        v.push_back(g.mix[u].src), v.push_back(g.mix[u].src_off), v.push_back(g.mix[u].b), v.push_back(g.mix[u].f),
            v.push_back(g.mix[u].delta);
    }
    for (const WMixDst& q : s.mix) {
      v.push_back(-3), v.push_back(q.dst), v.push_back(q.dst_off), v.push_back(q.nterm);
      for (int u = 0; u < q.nterm; ++u)
        v.push_back(q.term[u].src), v.push_back(q.term[u].src_off), v.push_back(q.term[u].b), v.push_back(q.term[u].f),
            v.push_back(q.term[u].ident);
    }
  }
  if ((long long)v.size() > cap) return -2;
  memcpy(rec, v.data(), v.size() * sizeof(long long));
  return (long long)v.size();
}
