// TEST INFRASTRUCTURE: executes the product's contraction plans (renormalizer_amd/csrc/
// mpse_plans.h) on HOST memory with a naive loop implementation of the strided-GEMM
// contract, so the index algebra of the hot-path contractions is checked on a CPU-only
// machine against numpy (tests/test_plans_host.py).  Never linked into libmpsengine.so.
// One executor for every plan (plan_emu_epi.cpp and plan_emu_ft.cpp include this file); like the device it reads the
// marks of the steps (Step::elementwise_w, slices_to, ...) instead of inferring them.
#include <complex>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../renormalizer_amd/csrc/mpse_plans.h"

using namespace mpse_plan;
typedef std::complex<double> cd;

static inline int64_t off(const mpse_index& m, int64_t i) {
  if (m.lo_ext >= m.ext) return i * m.s_lo;
  return (i / m.lo_ext) * m.s_hi + (i % m.lo_ext) * m.s_lo;
}

static inline cd ld(const void* p, int dt, int64_t o, int conj = 0) {
  if (dt == MPSE_C128) {
    cd v = ((const cd*)p)[o];
    return conj ? std::conj(v) : v;
  }
  return cd(((const double*)p)[o], 0.0);
}
static inline void st(void* p, int dt, int64_t o, cd v) {
  if (dt == MPSE_C128)
    ((cd*)p)[o] = v;
  else
    ((double*)p)[o] = v.real();
}

// Test hook: S >= 2 forces the hand-off of K slices that the device decides per launch (0: never, as a product that does
// not split).  A product marked slices_to then stores its result as S K slices in a side buffer (slice q at q * M * N,
// compact like C) and leaves its range of C untouched - poisoned, where C is a temporary.
static int g_handoff = 0;
extern "C" void emu_set_slice_handoff(int S) { g_handoff = S; }

static void naive_gemm(const Step& s, const void* A, const void* B, void* C, const void* Cin, void* slices, int S) {
  const int dtc = (s.dta == MPSE_C128 || s.dtb == MPSE_C128) ? MPSE_C128 : MPSE_F64;
  const int64_t K = s.ka.ext, nq = slices ? S : 1, per = (K + nq - 1) / nq;
  for (int64_t b = 0; b < s.batch; ++b)
    for (int64_t i = 0; i < s.ma.ext; ++i)
      for (int64_t j = 0; j < s.nb.ext; ++j) {
        cd acc = 0;
        for (int64_t q = 0; q < nq; ++q) {      // (a slice may be empty: it holds zeros)
          for (int64_t k = q * per; k < std::min(K, (q + 1) * per); ++k)
            acc += ld(A, s.dta, b * s.sba + off(s.ma, i) + off(s.ka, k), s.conja) *
                   ld(B, s.dtb, b * s.sbb + off(s.kb, k) + off(s.nb, j), s.conjb);
          if (slices) st(slices, dtc, (q * s.mc.ext + i) * s.nc.ext + j, acc), acc = 0;
        }
        if (slices) continue;
        int64_t o = b * s.sbc + off(s.mc, i) + off(s.nc, j);
        // the beta term comes from C itself or, for steps with a beta source, from that tensor through its own maps
        const void* src = Cin ? Cin : C;
        const int64_t oi = Cin ? off(s.mcin, i) + off(s.ncin, j) : o;
        st(C, dtc, o, acc + (s.beta != 0.0 ? s.beta * ld(src, dtc, oi) : cd(0)));
      }
}

static void naive_copy(const Step& s, int dt, const void* A, void* C) {
  for (int64_t i = 0; i < s.ma.ext; ++i)
    for (int64_t j = 0; j < s.ka.ext; ++j) st(C, dt, off(s.mc, i) + off(s.nc, j), ld(A, dt, off(s.ma, i) + off(s.ka, j)));
}

// The MPO step of a small site as the device runs it (Step::elementwise_w, k_wsmall), in the tensors' own layouts:
//   T2[a, dd, f, n] = sum_{b,e} W[b, dd, e, f] T1[b, a, e, n]
// with the channels [slice_b_lo, slice_b_hi) of T1 summed from `nslices` K slices of the product that forms them, by the
// address formula of WsmArgs::slices (mpse_contract.hip); nslices == 0: everything is read from T1.
static void naive_wsmall(const Step& s, int dt, const double* W, const void* T1, void* T2, const void* slices, int nslices) {
  const int64_t Da = s.w_Da, d = s.w_d, wl = s.w_wl, wr = s.w_wr, N = s.w_N;
  for (int64_t a = 0; a < Da; ++a)
    for (int64_t dd = 0; dd < d; ++dd)
      for (int64_t f = 0; f < wr; ++f)
        for (int64_t n = 0; n < N; ++n) {
          cd acc = 0;
          for (int64_t b = 0; b < wl; ++b)
            for (int64_t e = 0; e < d; ++e) {
              cd x = 0;
              if (nslices > 0 && b >= s.slice_b_lo && b < s.slice_b_hi)
                for (int q = 0; q < nslices; ++q)
                  x += ld(slices, dt, q * s.slice_elems + (((b - s.slice_b_lo) * Da + a) * d + e) * N + n);
              else
                x = ld(T1, dt, ((b * Da + a) * d + e) * N + n);
              acc += W[((b * d + dd) * d + e) * wr + f] * x;
            }
          st(T2, dt, ((a * d + dd) * wr + f) * N + n, acc);
        }
}

// dst[a, dd, k] = sum_terms sum_e W[b, dd, e, f] src[a, e, k]
static int naive_wmix(const Step& s, int dtype, const void* const* bufs) {
  const double* W = (const double*)bufs[s.b];
  const int64_t nchunk = (s.wp_d + WM_CHUNK - 1) / WM_CHUNK;
  for (const WMixDst& q : s.mix)
    for (int64_t a = 0; a < s.wp_Da; ++a)
      for (int64_t dd = 0; dd < s.wp_d; ++dd)
        for (int64_t k = 0; k < s.wp_Dk; ++k) {
          cd acc = 0;
          for (int t = 0; t < q.nterm; ++t) {
            const WMixTerm& tm = q.term[t];
            const int64_t c = dd / WM_CHUNK;
            if (c >= nchunk) return MPSE_ERR_ARG;
            // only the columns the plan declares for this chunk are read - as on the device
            for (int64_t e = tm.e_lo[c]; e < tm.e_hi[c]; ++e) {
              const double v = tm.ident ? (e == dd ? 1.0 : 0.0) : W[((tm.b * s.wp_d + dd) * s.wp_d + e) * s.wp_wr + tm.f];
              if (v != 0.0) acc += v * ld(bufs[tm.src], dtype, tm.src_off + a * tm.s_a + e * tm.s_d + k);
            }
          }
          st(const_cast<void*>(bufs[q.dst]), dtype, q.dst_off + a * q.s_a + dd * q.s_d + k, acc);
        }
  return MPSE_OK;
}

// every group: C = sum over its segments of A_seg . B_seg + (beta C, or the epilogue mix: GGroupPlan::nmix)
static int naive_ggemm(const Step& s, int dtype, const void* const* bufs) {
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
  return MPSE_OK;
}

// Temporaries are poisoned (every byte 0x7f: huge finite numbers): every element must be written before use, and a
// term that multiplies where it has to select, or reads a row of another bond state, shows in the result.
static int run(int dtype, const Plan& p, const void* bufs_in[B_COUNT]) {
  if (p.error) return MPSE_ERR_SHAPE;
  const void* bufs[B_COUNT];
  for (int i = 0; i < B_COUNT; ++i) bufs[i] = bufs_in[i];
  const size_t es = dtype == MPSE_C128 ? 16 : 8;
  std::vector<char> t[3], slices;
  int slices_used = 0;
  for (int i = 0; i < 3; ++i) {
    t[i].assign(size_t(p.tmp_elems[i]) * es + 16, 0x7f);
    bufs[B_T1 + i] = t[i].data();
  }
  for (const Step& s : p.steps) {
    const size_t ea = s.dta == MPSE_C128 ? 16 : 8, eb = s.dtb == MPSE_C128 ? 16 : 8;
    const int dtc = (s.dta == MPSE_C128 || s.dtb == MPSE_C128) ? MPSE_C128 : MPSE_F64;
    if (dtc != dtype && s.kind != K_WMIX) return MPSE_ERR_ARG;
    int rc = MPSE_OK;
    if (s.elementwise_w) {
      naive_wsmall(s, dtype, (const double*)bufs[s.a], bufs[s.b], const_cast<void*>(bufs[s.c]), slices.data(), slices_used);
      slices_used = 0;
    } else if (s.kind == K_WMIX) {
      rc = naive_wmix(s, dtype, bufs);
    } else if (s.kind == K_GGEMM) {
      rc = naive_ggemm(s, dtype, bufs);
    } else if (s.kind == K_COPY) {
      naive_copy(s, dtc, (const char*)bufs[s.a] + s.a_off * ea, (char*)const_cast<void*>(bufs[s.c]) + s.c_off * es);
    } else {
      const bool hand = g_handoff >= 2 && s.slices_to >= 0;
      if (hand) slices.assign(size_t(g_handoff) * s.mc.ext * s.nc.ext * es, 0x7f), slices_used = g_handoff;
      naive_gemm(s, (const char*)bufs[s.a] + s.a_off * ea, (const char*)bufs[s.b] + s.b_off * eb,
                 (char*)const_cast<void*>(bufs[s.c]) + s.c_off * es,
                 s.cin >= 0 ? (const char*)bufs[s.cin] + s.cin_off * es : nullptr, hand ? slices.data() : nullptr, g_handoff);
    }
    if (rc != MPSE_OK) return rc;
  }
  return MPSE_OK;
}

extern "C" int emu_heff_apply(int dtype, const mpse_heff* h, const void* C, void* out) {
  const void* bufs[B_COUNT] = {nullptr};
  bind_heff(bufs, *h, C, out);
  return run(dtype, plan_heff(dtype, *h), bufs);
}

extern "C" int emu_env_update(int dtype, int domain, const mpse_dims* dims, const void* env, int env_dtype,
                              const void* ket, const void* bra, int bra_conj, const void* W, int w_dtype, void* out) {
  const void* bufs[B_COUNT] = {nullptr};
  bind_env(bufs, env, ket, bra ? bra : ket, out, 1, &W);
  return run(dtype, plan_env(dtype, domain, *dims, env_dtype, w_dtype, bra_conj), bufs);
}

extern "C" int emu_env_update_multi(int dtype, int domain, const mpse_dims* dims, int n, const int64_t* wl,
                                    const int64_t* wr, const void* env, int env_dtype, const void* ket, const void* bra,
                                    int bra_conj, const void* const* W, int w_dtype, void* out) {
  const void* bufs[B_COUNT] = {nullptr};
  bind_env(bufs, env, ket, bra ? bra : ket, out, n, W);
  return run(dtype, plan_env_multi(dtype, domain, *dims, n, wl, wr, env_dtype, w_dtype, bra_conj), bufs);
}

extern "C" int emu_heff_apply2(int dtype, const mpse_heff* h, const void* C, void* out) {
  const void* bufs[B_COUNT] = {nullptr};
  bind_heff(bufs, *h, C, out);
  return run(dtype, plan_heff2(dtype, *h), bufs);
}

extern "C" void emu_set_unit_threshold(long long macs) { unit_threshold() = macs; }

// runs a folded one-site plan; its result in two parts (Plan::two_results) is added up here, as the caller would
static int run_fold(int dtype, const Plan& p, const mpse_heff* h, const void* C, void* out) {
  const size_t es = dtype == MPSE_C128 ? 16 : 8;
  const int64_t n = (h->dims.Dl_bra > 0 ? h->dims.Dl_bra : h->dims.Dl_ket) * h->dims.d0 *
                    (h->dims.Dr_bra > 0 ? h->dims.Dr_bra : h->dims.Dr_ket);
  std::vector<char> out2(size_t(n) * es + 16, 0x7f);
  const void* bufs[B_COUNT] = {nullptr};
  bind_heff(bufs, *h, C, out);
  bufs[B_OUT2] = out2.data();
  const int st = run(dtype, p, bufs);
  if (st == MPSE_OK && p.two_results)
    for (int64_t i = 0; i < n * (int64_t)(es / 8); ++i) ((double*)out)[i] += ((const double*)out2.data())[i];
  return st;
}
// one-site matvec through the folded plan (the block structure of the MPO site read from the host copy of W);
// returns MPSE_ERR_SHAPE when the site does not qualify.  *nsteps receives the number of plan steps.
extern "C" int emu_heff_apply_fold(int dtype, const mpse_heff* h, const void* C, void* out, int* nsteps) {
  const WSiteInfo wi = analyse_mpo_site((const double*)h->W0, h->dims.wl, h->dims.d0, h->dims.wr);
  // the result in two parts where the plan makes use of it (complex centres whose rows fill whole tiles)
  Plan p = plan_heff1_fold(dtype, *h, wi, true);
  if (nsteps) *nsteps = (int)p.steps.size() + (p.two_results ? 100 : 0);
  return run_fold(dtype, p, h, C, out);
}
extern "C" void emu_set_fold_min(long long macs, long long align, long long split2_min_kt) {
  fold_min() = macs;
  fold_align() = align;
  fold_split2_min_kt() = split2_min_kt;
}
extern "C" void emu_set_beta_source(int on) { beta_source_flag() = on != 0; }

// The marks of a plan as flat integers (tests/test_plans_marks_host.py), per step: kind, elementwise_w, slices_to,
// slice_b_lo, slice_b_hi, slice_elems, completes.  Returns the number of integers (-1: no plan, -2: does not fit).
static long long marks_of(const Plan& p, long long* rec, long long cap) {
  if (p.error) return -1;
  if ((long long)p.steps.size() * 7 > cap) return -2;
  for (const Step& s : p.steps) {
    const long long r[7] = {s.kind, s.elementwise_w, s.slices_to, s.slice_b_lo, s.slice_b_hi, s.slice_elems, s.completes};
    memcpy(rec, r, sizeof(r));
    rec += 7;
  }
  return (long long)p.steps.size() * 7;
}
// fold: 0 = plan_heff, 1 / 2 = plan_heff1_fold without / with the epilogue mix (site structure from the host copy of W0)
extern "C" long long emu_heff_marks(int dtype, const mpse_heff* h, int fold, long long* rec, long long cap) {
  if (!fold) return marks_of(plan_heff(dtype, *h), rec, cap);
  const WSiteInfo wi = analyse_mpo_site((const double*)h->W0, h->dims.wl, h->dims.d0, h->dims.wr);
  return marks_of(plan_heff1_fold(dtype, *h, wi, true, fold == 2), rec, cap);
}
extern "C" long long emu_env_marks(int dtype, int domain, const mpse_dims* dims, int env_dtype, int w_dtype,
                                   long long* rec, long long cap) {
  return marks_of(plan_env(dtype, domain, *dims, env_dtype, w_dtype, 1), rec, cap);
}

// The launch plans of the contraction kernel as flat integer records (tests/test_gemm_plan_host.py).
// in: M, N, K, batch, n_cu, ca, cb, skip_hint, k_single, fast_ok, dot, dot_cap, slices, slices_cap, use_beta
// out: tiles_m, tiles_n, nkt, ksplit, kt_per_split, ws_bytes, leave_slices, nwg, fast, wide, masks, nkw, order, die_group,
//      rgx, rgy, dot_producers
extern "C" void emu_gemm_launch_plan(const long long* in, long long* out) {
  const GemmPlan p = launch_plan({in[0], in[1], in[2], in[3], (int)in[4], in[5] != 0, in[6] != 0, (int)in[7], in[8] != 0,
                                  in[9] != 0, in[10] != 0, in[11], in[12] != 0, (unsigned long long)in[13], in[14] != 0});
  const long long r[17] = {p.tiles_m, p.tiles_n, p.nkt, p.ksplit, p.kt_per_split, (long long)p.ws_bytes, p.leave_slices,
                           p.nwg, p.fast, p.wide, p.masks, p.nkw, p.order, p.die_group, p.rgx, p.rgy, p.dot_producers};
  memcpy(out, r, sizeof(r));
}
// in: M, N, ngrp, nkt_max, any_mask, split2, ca, n_cu;  out: tiles_m, tiles_n, nkw, die_group, order, wide, nwg
extern "C" void emu_gemm_grouped_plan(const long long* in, long long* out) {
  const GroupedPlan p = grouped_plan(in[0], in[1], (int)in[2], (int)in[3], in[4] != 0, in[5] != 0, in[6] != 0, (int)in[7]);
  const long long r[7] = {p.tiles_m, p.tiles_n, p.nkw, p.die_group, p.order, p.wide, p.nwg};
  memcpy(out, r, sizeof(r));
}
