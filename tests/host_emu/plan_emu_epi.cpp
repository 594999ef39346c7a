// TEST INFRASTRUCTURE: host twin of the folded one-site matvec plan with the epilogue mix (renormalizer_amd/csrc/
// mpse_plans.h: plan_heff1_fold(..., mix_epilogue), GGroupPlan::nmix).  A small runner of its own for the two step kinds
// of that plan, with naive loops on host memory (tests/test_plans_epi_host.py).  Never linked into libmpsengine.so.
#include <complex>
#include <cstring>
#include <vector>

#include "../../renormalizer_amd/csrc/mpse_plans.h"

using namespace mpse_plan;
typedef std::complex<double> cd;

static inline int64_t off(const mpse_index& m, int64_t i) {
  if (m.lo_ext >= m.ext) return i * m.s_lo;
  return (i / m.lo_ext) * m.s_hi + (i % m.lo_ext) * m.s_lo;
}
static inline cd ld(const void* p, int dt, int64_t o) {
  return dt == MPSE_C128 ? ((const cd*)p)[o] : cd(((const double*)p)[o], 0.0);
}
static inline void st(void* p, int dt, int64_t o, cd v) {
  if (dt == MPSE_C128)
    ((cd*)p)[o] = v;
  else
    ((double*)p)[o] = v.real();
}

// Temporaries are poisoned (every byte 0x7f: huge finite numbers), so a term that multiplies where it has to select, or
// reads a row of another bond state, shows in the result.
static int run(int dtype, const Plan& p, const void* bufs_in[B_COUNT]) {
  if (p.error) return MPSE_ERR_SHAPE;
  const void* bufs[B_COUNT];
  for (int i = 0; i < B_COUNT; ++i) bufs[i] = bufs_in[i];
  const size_t es = dtype == MPSE_C128 ? 16 : 8;
  std::vector<char> t[3];
  for (int i = 0; i < 3; ++i) {
    t[i].assign(size_t(p.tmp_elems[i]) * es + 16, 0x7f);
    bufs[B_T1 + i] = t[i].data();
  }
  for (const Step& s : p.steps) {
    if (s.kind == K_WMIX) {   // dst[a, dd, k] = sum_terms sum_e W[b, dd, e, f] src[a, e, k]
      const double* W = (const double*)bufs[s.b];
      for (const WMixDst& q : s.mix)
        for (int64_t a = 0; a < s.wp_Da; ++a)
          for (int64_t dd = 0; dd < s.wp_d; ++dd)
            for (int64_t k = 0; k < s.wp_Dk; ++k) {
              cd acc = 0;
              for (int u = 0; u < q.nterm; ++u) {
                const WMixTerm& tm = q.term[u];
                const int64_t c = dd / WM_CHUNK;
                for (int64_t e = tm.e_lo[c]; e < tm.e_hi[c]; ++e) {
                  const double v = tm.ident ? (e == dd ? 1.0 : 0.0) : W[((tm.b * s.wp_d + dd) * s.wp_d + e) * s.wp_wr + tm.f];
                  if (v != 0.0) acc += v * ld(bufs[tm.src], dtype, tm.src_off + a * tm.s_a + e * tm.s_d + k);
                }
              }
              st(const_cast<void*>(bufs[q.dst]), dtype, q.dst_off + a * q.s_a + dd * q.s_d + k, acc);
            }
      continue;
    }
    if (s.kind != K_GGEMM) return MPSE_ERR_ARG;
    for (const GGroupPlan& g : s.groups) {
      void* Cg = const_cast<void*>(bufs[g.cbuf]);
      if (g.nmix > 0 && (g.beta != 1.0 || g.mix_d < 1 || 64 % g.mix_d != 0 || g.nmix > EPI_MAXTERM)) return MPSE_ERR_ARG;
      const double* W = (const double*)bufs[g.wbuf];
      for (int64_t i = 0; i < s.ma.ext; ++i)
        for (int64_t jn = 0; jn < s.nb.ext; ++jn) {
          cd acc = 0;
          for (int q = 0; q < g.nseg; ++q) {
            const GSegPlan& sg = g.seg[q];
            for (int64_t k = 0; k < s.ka.ext; ++k)
              acc += ld(bufs[sg.abuf], s.dta, sg.a_off + off(s.ma, i) + off(s.ka, k)) *
                     ld(bufs[sg.bbuf], s.dtb, sg.b_off + off(s.kb, k) + off(s.nb, jn));
          }
          const int64_t o = g.c_off + off(s.mc, i) + off(s.nc, jn);
          if (g.split2) {   // the second result receives a part of the sum, the caller adds the two
            st(const_cast<void*>(bufs[B_OUT2]), dtype, o, 0.25 * acc);
            acc *= 0.75;
          }
          cd c0 = 0;
          if (g.nmix > 0) {
            // output row i = (a, x): the rows of a 64-row tile that the device may touch are those of the same a, and
            // the address is clamped to the tensor whatever the weight
            const int64_t d = g.mix_d, x = i % d;
            for (int u = 0; u < g.nmix; ++u) {
              const EpiTerm& m = g.mix[u];
              const int64_t e = x + m.delta;
              const double w = (e >= 0 && e < d) ? W[((m.b * d + x) * d + e) * g.mix_wr + m.f] : 0.0;
              const int64_t row = std::min<int64_t>(std::max<int64_t>(i + m.delta, 0), s.ma.ext - 1);
              const cd v = ld(bufs[m.src], dtype, m.src_off + row * g.mix_ld + jn);
              if (w != 0.0) c0 += w * v;
            }
          } else if (g.beta != 0.0) {
            c0 = g.beta * ld(Cg, dtype, o);
          }
          st(Cg, dtype, o, acc + c0);
        }
    }
  }
  return MPSE_OK;
}

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
  const size_t es = dtype == MPSE_C128 ? 16 : 8;
  const int64_t n = (h->dims.Dl_bra > 0 ? h->dims.Dl_bra : h->dims.Dl_ket) * h->dims.d0 *
                    (h->dims.Dr_bra > 0 ? h->dims.Dr_bra : h->dims.Dr_ket);
  std::vector<char> out2(size_t(n) * es + 16, 0x7f);
  const void* bufs[B_COUNT] = {nullptr};
  bufs[B_L] = h->L, bufs[B_R] = h->R, bufs[B_W0] = h->W0, bufs[B_C] = C, bufs[B_OUT] = out, bufs[B_OUT2] = out2.data();
  const int rc = run(dtype, p, bufs);
  if (rc == MPSE_OK && p.two_results)
    for (int64_t i = 0; i < n * (int64_t)(es / 8); ++i) ((double*)out)[i] += ((const double*)out2.data())[i];
  return rc;
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
