// TEST INFRASTRUCTURE: a pin of every contraction plan (renormalizer_amd/csrc/mpse_plans.h) for
// tests/test_plans_pin_host.py.  Enumerates planner calls, prints per case a key and a 64-bit hash of a canonical dump
// of the plan (every field of Plan, Step, GGroupPlan, GSegPlan, EpiTerm, ScanDesc, WMixDst, WMixTerm and the error),
// then a tally of the planner branches the cases took.  An mpse_index is dumped in the canonical form the device gives
// it (to_map, mpse_gemm.hip; strides dropped where the extent is <= 1, batch strides likewise), so two representations no
// executor can tell apart compare equal; everything else compares exactly.  `--case KEY` prints the full dump of one case.
// Uses only the planners' public entry points and the Plan / Step structs.  Never linked into libmpsengine.so.
#include <cstdarg>
#include <cstdio>
#include <map>
#include <sstream>

#include "../../renormalizer_amd/csrc/mpse_plans.h"

using namespace mpse_plan;

static std::ostringstream* g_os;
static const char* g_want = nullptr;   // --case KEY
static bool g_found = false;
static std::map<std::string, long long> g_tally;
static const char* const TALLIES[] = {
    "unit_copy", "beta_source", "two_ranges", "kind_gemm", "kind_copy", "kind_wmix", "kind_ggemm", "env_wmix_taken",
    "env_wmix_refused", "epi", "split2", "direct_plane", "alias", "temporary", "second_r_launch"};

static void put_index(const char* name, const mpse_index& s) {
  long long ext = s.ext, lo = s.lo_ext <= 0 ? 1 : s.lo_ext, s_hi = s.s_hi, s_lo = s.s_lo;
  if (lo >= ext) {
    s_hi = 0;
  } else if (lo == 1) {
    s_lo = s_hi, s_hi = 0, lo = ext;
  } else if (s_hi == lo * s_lo) {
    s_hi = 0, lo = ext;
  }
  if (lo >= ext) lo = 0x7fffffffLL;
  if (ext <= 1) s_hi = s_lo = 0;
  *g_os << ' ' << name << "=(" << ext << ',' << lo << ',' << s_hi << ',' << s_lo << ')';
}

static void put_scan(const char* name, const ScanDesc& d) {
  *g_os << "  " << name << " on=" << d.on << " buf=" << d.buf << " dt=" << d.dt << " off=" << d.off;
  put_index("r", d.r), put_index("k", d.k);
  *g_os << '\n';
}

static std::string dump(const Plan& p) {
  std::ostringstream os;
  g_os = &os;
  os << "error=" << (p.error ? p.error : "-") << " tmp=" << p.tmp_elems[0] << ',' << p.tmp_elems[1] << ',' << p.tmp_elems[2]
     << " two_results=" << p.two_results << " steps=" << p.steps.size() << '\n';
  for (const Step& s : p.steps) {
    os << " step kind=" << s.kind << " a=" << s.a << '+' << s.a_off << " b=" << s.b << '+' << s.b_off << " c=" << s.c << '+'
       << s.c_off << " dt=" << s.dta << ',' << s.dtb << " conj=" << s.conja << ',' << s.conjb;
    put_index("ma", s.ma), put_index("ka", s.ka), put_index("kb", s.kb), put_index("nb", s.nb), put_index("mc", s.mc),
        put_index("nc", s.nc);
    const bool nb1 = s.batch <= 1;     // the batch is an index too: its strides are never read where it has one value
    os << " batch=" << s.batch << ',' << (nb1 ? 0 : s.sba) << ',' << (nb1 ? 0 : s.sbb) << ',' << (nb1 ? 0 : s.sbc) << " beta=" << s.beta << " skip=" << s.skip_zero
       << " w=" << s.is_wstep << ',' << s.w_Da << ',' << s.w_wl << ',' << s.w_d << ',' << s.w_wr << ',' << s.w_N
       << " wp=" << s.wp_Da << ',' << s.wp_d << ',' << s.wp_Dk << ',' << s.wp_wr << " cin=" << s.cin << '+' << s.cin_off;
    put_index("mcin", s.mcin), put_index("ncin", s.ncin);
    os << " marks=" << s.elementwise_w << ',' << s.slices_to << ',' << s.slice_b_lo << ',' << s.slice_b_hi << ','
       << s.slice_elems << ',' << s.completes << '\n';
    put_scan("scan_a", s.scan_a), put_scan("scan_b", s.scan_b);
    for (const WMixDst& q : s.mix) {
      os << "  dst " << q.dst << '+' << q.dst_off << " s=" << q.s_a << ',' << q.s_d << " nterm=" << q.nterm << '\n';
      for (int t = 0; t < q.nterm; ++t) {
        const WMixTerm& u = q.term[t];
        os << "   term b=" << u.b << " f=" << u.f << " ident=" << u.ident << " src=" << u.src << '+' << u.src_off
           << " s=" << u.s_a << ',' << u.s_d << " e=";
        for (int c = 0; c < WM_MAXCHUNKS; ++c) os << int(u.e_lo[c]) << ':' << int(u.e_hi[c]) << ' ';
        os << '\n';
      }
    }
    for (const GGroupPlan& g : s.groups) {
      os << "  group nseg=" << g.nseg << " c=" << g.cbuf << '+' << g.c_off << " beta=" << g.beta << " nmix=" << g.nmix
         << " wbuf=" << g.wbuf << " mix=" << g.mix_d << ',' << g.mix_wr << ',' << g.mix_ld << " split2=" << g.split2 << '\n';
      for (int q = 0; q < g.nseg; ++q) {
        const GSegPlan& sg = g.seg[q];
        os << "   seg a=" << sg.abuf << '+' << sg.a_off << " b=" << sg.bbuf << '+' << sg.b_off << " am_row0=" << sg.am_row0
           << " bm=" << sg.bm_kind << ',' << sg.bm_kt0 << '\n';
      }
      for (int q = 0; q < g.nmix; ++q) {
        const EpiTerm& t = g.mix[q];
        os << "   epi src=" << t.src << '+' << t.src_off << " b=" << t.b << " f=" << t.f << " delta=" << t.delta << '\n';
      }
    }
  }
  return os.str();
}

static bool is_w(int buf) { return buf == B_W0 || buf == B_W1 || buf == B_W2 || buf == B_W3; }

// env_pre: 1 = an environment update whose caller described the site and whose sizes ask for the elementwise step
static void emit(const std::string& key, const Plan& p, int env_pre = 0) {
  const std::string d = dump(p);
  unsigned long long h = 1469598103934665603ULL;
  for (unsigned char c : d) h = (h ^ c) * 1099511628211ULL;
  if (g_want) {
    if (key == g_want) printf("%s\n%s", key.c_str(), d.c_str()), g_found = true;
  } else {
    printf("%s %016llx\n", key.c_str(), h);
  }
  if (p.error) ++g_tally[std::string("error: ") + p.error];
  static const char* const kinds[] = {"kind_gemm", "kind_copy", "kind_wmix", "kind_ggemm"};
  bool t[16] = {false}, wmix = false;
  int r_launches = 0;
  for (size_t i = 0; i < p.steps.size(); ++i) {
    const Step& s = p.steps[i];
    ++g_tally[kinds[s.kind]];
    if (s.kind == K_COPY) t[0] = true;
    if (s.kind == K_GEMM && s.cin >= 0) t[1] = true;
    if (i > 0) {
      const Step& q = p.steps[i - 1];
      if (s.kind == K_GEMM && q.kind == K_GEMM && !s.is_wstep && !is_w(s.a) && s.a == q.a && s.b == q.b && s.c == q.c) t[2] = true;
    }
    if (s.kind == K_WMIX) wmix = true;
    if (s.kind == K_GGEMM && s.scan_b.on) ++r_launches;
    for (const GGroupPlan& g : s.groups) {
      if (g.nmix > 0) t[3] = true;
      if (g.split2) t[4] = true;
      if (s.scan_a.on && (g.cbuf == B_T2 || g.cbuf == B_OUT)) t[5] = true;
      if (s.scan_a.on && g.cbuf == B_T1) t[7] = true;
      for (int q = 0; q < g.nseg; ++q)
        if (s.scan_b.on && g.seg[q].abuf == B_C) t[6] = true;
    }
  }
  static const char* const names[] = {"unit_copy", "beta_source", "two_ranges", "epi", "split2", "direct_plane", "alias", "temporary"};
  for (int i = 0; i < 8; ++i)
    if (t[i]) ++g_tally[names[i]];
  if (r_launches >= 2) ++g_tally["second_r_launch"];
  if (env_pre && !p.error) ++g_tally[wmix ? "env_wmix_taken" : "env_wmix_refused"];
}

static std::string key(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}

static void hooks(int64_t thr, bool beta, int64_t fmin, int64_t align, int64_t min_kt, bool split2 = true, int64_t cus = 256) {
  unit_threshold() = thr, beta_source_flag() = beta, fold_min() = fmin, fold_align() = align, fold_split2_min_kt() = min_kt;
  fold_split2() = split2, fold_cus() = cus, fold_epi() = true;
}
static void default_hooks() { hooks(int64_t(1) << 27, true, int64_t(1) << 28, 64, 8); }

// ---- MPO sites of named block structure (tests/test_plans_epi_host.py builds the same family): (wr + 1, d, d, wr), channel
// 0 is L's unit channel, wr - 1 R's; channels 1, 2, 5 .. pass through; the plane of R's unit channel receives `kind`
static void band(std::vector<double>& w, int64_t d, int64_t wr, int64_t b, int64_t f, std::initializer_list<int> offs) {
  for (int o : offs)
    for (int64_t x = 0; x < d; ++x) {
      const int64_t e = x + o;
      if (e >= 0 && e < d) w[((b * d + x) * d + e) * wr + f] = 1.5 + 0.125 * double(x + 2 * e) + 0.25 * o;
    }
}
static void eye(std::vector<double>& w, int64_t d, int64_t wr, int64_t b, int64_t f) {
  for (int64_t x = 0; x < d; ++x) w[((b * d + x) * d + x) * wr + f] = 1.0;
}
static void full(std::vector<double>& w, int64_t d, int64_t wr, int64_t b, int64_t f) {
  for (int64_t x = 0; x < d; ++x)
    for (int64_t e = 0; e < d; ++e) w[((b * d + x) * d + e) * wr + f] = 0.5 + 0.0625 * double(3 * x + e);
}
struct Site {
  int64_t wl, d, wr;
  std::vector<double> w;
  WSiteInfo info() const { return analyse_mpo_site(w.data(), wl, d, wr); }
};
static const char* const SITE_KINDS[] = {"plain", "ident", "diag", "tri", "penta", "second", "wide", "dense", "passonly", "zero",
                                         "fanout", "manyblk", "manydst", "bigblk", "manych", "eonly"};
static Site make_site(const std::string& kind, int64_t d, int64_t wr = 4) {
  Site s;
  if (kind == "bigblk") {           // nine dense blocks: more than the elementwise pass holds at d = 32
    s.wl = 3, s.d = d, s.wr = 3, s.w.assign(3 * d * d * 3, 0.0);
    for (int b = 0; b < 3; ++b)
      for (int f = 0; f < 3; ++f) full(s.w, d, 3, b, f);
    return s;
  }
  if (kind == "manych") {           // ten channels of L that each need a product
    s.wl = 10, s.d = d, s.wr = 10, s.w.assign(10 * d * d * 10, 0.0);
    for (int b = 0; b < 10; ++b) eye(s.w, d, 10, b, b);
    return s;
  }
  if (kind == "manyblk") {          // five blocks into one plane
    s.wl = 6, s.d = d, s.wr = 3, s.w.assign(6 * d * d * 3, 0.0);
    eye(s.w, d, 3, 0, 0);
    for (int b = 1; b < 6; ++b) band(s.w, d, 3, b, 1, {0});
    eye(s.w, d, 3, 5, 2);
    return s;
  }
  if (kind == "manydst") {          // five mixed planes
    s.wl = 3, s.d = d, s.wr = 6, s.w.assign(3 * d * d * 6, 0.0);
    for (int f = 0; f < 6; ++f) band(s.w, d, 6, 0, f, {0}), band(s.w, d, 6, 1 + f % 2, f, {-1, 1});
    return s;
  }
  if (kind == "eonly") {            // nothing but the plane of R's unit channel: no product with R follows
    s.wl = 2, s.d = d, s.wr = 2, s.w.assign(2 * d * d * 2, 0.0);
    eye(s.w, d, 2, 0, 1), band(s.w, d, 2, 1, 1, {-1, 1});
    return s;
  }
  const int64_t wl = wr + 1, ru = wr - 1;
  s.wl = wl, s.d = d, s.wr = wr, s.w.assign(wl * d * d * wr, 0.0);
  std::vector<double>& w = s.w;
  if (kind == "zero") return s;
  eye(w, d, wr, 0, 0), eye(w, d, wr, 1, 1), eye(w, d, wr, 2, 2);
  for (int64_t f = 3; f < ru; ++f) eye(w, d, wr, f + 2, f);
  if (kind == "passonly") return s;      // identity blocks only, nothing into R's unit channel
  eye(w, d, wr, 4, ru);
  if (kind == "plain") return s;         // the plane of R's unit channel is one product's result: already direct
  if (kind == "ident")
    eye(w, d, wr, 0, ru);
  else if (kind == "diag")
    band(w, d, wr, 0, ru, {0});
  else if (kind == "tri")
    band(w, d, wr, 0, ru, {0}), band(w, d, wr, 3, ru, {-1, 1});
  else if (kind == "penta" || kind == "second" || kind == "fanout") {
    band(w, d, wr, 0, ru, {-2, 0, 2}), band(w, d, wr, 3, ru, {-1, 0, 1});
    if (kind == "second") band(w, d, wr, 3, 1, {-1, 1});
    if (kind == "fanout") band(w, d, wr, 3, 1, {-1, 1}), band(w, d, wr, 3, 2, {0}), eye(w, d, wr, 1, 0);
  } else if (kind == "wide")
    band(w, d, wr, 0, ru, {-3, 0});
  else if (kind == "dense")
    band(w, d, wr, 0, ru, {0}), full(w, d, wr, 3, ru);
  return s;
}

static const int DT[4][4] = {   // working dtype, L / env, R, W
    {MPSE_F64, MPSE_F64, MPSE_F64, MPSE_F64}, {MPSE_C128, MPSE_F64, MPSE_C128, MPSE_F64}, {MPSE_C128, MPSE_C128, MPSE_C128, MPSE_C128},
    {MPSE_C128, MPSE_F64, MPSE_F64, MPSE_F64}};

static mpse_heff heff(int nsite, int dt, int64_t Dl, int64_t Dr, int64_t Dlb, int64_t Drb, int64_t d0, int64_t d1, int64_t wl,
                      int64_t wm, int64_t wr, int64_t danc, int64_t danc1, int64_t lu, int64_t ru) {
  mpse_heff h{};
  h.nsite = nsite;
  h.dims.Dl_ket = Dl, h.dims.Dr_ket = Dr, h.dims.Dl_bra = Dlb, h.dims.Dr_bra = Drb, h.dims.d0 = d0, h.dims.d1 = d1;
  h.dims.wl = wl, h.dims.wm = wm, h.dims.wr = wr, h.dims.danc = danc, h.dims.danc1 = danc1;
  h.l_dtype = DT[dt][1], h.r_dtype = DT[dt][2], h.w_dtype = DT[dt][3];
  h.l_unit = lu, h.r_unit = ru;
  return h;
}
static int64_t unit_of(int which, int64_t w) { return which == 0 ? 0 : which == 1 ? 1 : which == 2 ? (w + 1) / 2 : w; }

struct Shape {
  int64_t Dl, Dr, d0, d1, wl, wm, wr;
};
static const Shape SHAPES[3] = {{6, 5, 3, 2, 4, 2, 3}, {1, 4, 1, 2, 1, 1, 3}, {4, 1, 2, 1, 3, 3, 1}};

static void cases_heff() {
  for (int ns = 0; ns <= 2; ++ns)
    for (int dt = 0; dt < 3; ++dt)
      for (int sh = 0; sh < 3; ++sh)
        for (int bra = 0; bra < 2; ++bra)
          for (int64_t danc = 0; danc <= 2; ++danc)
            for (int64_t danc1 = 0; danc1 <= (ns == 2 ? 3 : 0); danc1 += 3)
              for (int thr = 0; thr < 2; ++thr)
                for (int lu = 0; lu < 4; ++lu)
                  for (int ru = 0; ru < 4; ++ru)
                    for (int beta = 1; beta >= 0; --beta) {
                      // thinned where a switch cannot matter: units need equal bonds and a threshold they pass; the
                      // beta source needs a unit channel of R
                      const bool diag3 = (lu == 0 && ru == 0) || (lu == 1 && ru == 3) || (lu == 2 && ru == 2);
                      if ((bra == 1 || thr == 1 || dt != 1 || sh != 0) && !diag3) continue;
                      if (bra == 1 && thr == 1) continue;
                      if (!beta && (ru == 0 || lu == 1 || lu == 3)) continue;
                      const Shape& s = SHAPES[sh];
                      const int64_t wl = ns == 0 ? s.wr : s.wl;
                      hooks(thr ? int64_t(1) << 27 : 0, beta != 0, int64_t(1) << 28, 64, 8);
                      const mpse_heff h = heff(ns, dt, s.Dl, s.Dr, bra ? s.Dl + 2 : 0, bra ? s.Dr + 1 : 0, s.d0, s.d1, wl, s.wm,
                                               s.wr, danc, danc1, unit_of(lu, wl), unit_of(ru, s.wr));
                      emit(key("heff.n%dt%ds%db%d.a%lld%lld.thr%d.u%d%d.bs%d", ns, dt, sh, bra, (long long)danc,
                               (long long)danc1, thr, lu, ru, beta),
                           plan_heff(DT[dt][0], h));
                    }
  default_hooks();
  emit("heff.n0.wl_ne_wr", plan_heff(MPSE_F64, heff(0, 0, 4, 4, 0, 0, 1, 1, 2, 1, 3, 1, 0, 0, 0)));
  emit("heff.n3", plan_heff(MPSE_F64, heff(3, 0, 4, 4, 0, 0, 2, 2, 2, 2, 2, 1, 0, 0, 0)));
  // mixed operand dtypes the grid above does not hold
  for (int l = 0; l < 2; ++l)
    for (int r = 0; r < 2; ++r)
      for (int w = 0; w < 2; ++w)
        for (int ns = 0; ns <= 2; ++ns) {
          mpse_heff h = heff(ns, 1, 6, 5, 0, 0, 3, 2, ns == 0 ? 3 : 4, 2, 3, 1, 0, 1, 3);
          h.l_dtype = l ? MPSE_C128 : MPSE_F64, h.r_dtype = r ? MPSE_C128 : MPSE_F64, h.w_dtype = w ? MPSE_C128 : MPSE_F64;
          hooks(0, true, int64_t(1) << 28, 64, 8);
          emit(key("heff.mixed.n%d.l%dr%dw%d", ns, l, r, w), plan_heff(MPSE_C128, h));
        }
}

static mpse_dims env_dims(int64_t Dlk, int64_t Drk, int64_t Dlb, int64_t Drb, int64_t d, int64_t wl, int64_t wr, int64_t danc,
                          int64_t unit) {
  mpse_dims s{};
  s.Dl_ket = Dlk, s.Dr_ket = Drk, s.Dl_bra = Dlb, s.Dr_bra = Drb, s.d0 = d, s.wl = wl, s.wr = wr, s.danc = danc, s.env_unit = unit;
  return s;
}

static void cases_env() {
  for (int dom = 0; dom < 2; ++dom)
    for (int dt = 0; dt < 3; ++dt)
      for (int sh = 0; sh < 3; ++sh)
        for (int bra = 0; bra < 2; ++bra)
          for (int64_t danc = 0; danc <= 2; ++danc)
            for (int thr = 0; thr < 2; ++thr)
              for (int u = 0; u < 4; ++u)
                for (int cj = 0; cj < 2; ++cj) {
                  if ((bra == 1 || thr == 1 || sh != 0) && u != 0 && u != 2) continue;
                  if ((bra == 1 && thr == 1) || (dt != 1 && cj == 0)) continue;
                  const Shape& s = SHAPES[sh];
                  hooks(thr ? int64_t(1) << 27 : 0, true, int64_t(1) << 28, 64, 8);
                  // the incoming environment carries (bra, channel, ket) of the bond it comes from
                  const int64_t w_in = dom == 0 ? s.wl : s.wr;
                  const mpse_dims m = env_dims(s.Dl, s.Dr, bra ? s.Dl + 2 : s.Dl, bra ? s.Dr + 1 : s.Dr, s.d0, s.wl, s.wr, danc,
                                               unit_of(u, w_in));
                  emit(key("env.%ct%ds%db%d.a%lld.thr%d.u%d.cj%d", dom ? 'R' : 'L', dt, sh, bra, (long long)danc, thr, u, cj),
                       plan_env(DT[dt][0], dom ? MPSE_DOMAIN_R : MPSE_DOMAIN_L, m, DT[dt][1], DT[dt][3], cj));
                }
  default_hooks();
  emit("env.bad_domain", plan_env(MPSE_C128, 77, env_dims(4, 4, 4, 4, 2, 2, 2, 1, 0), MPSE_C128, MPSE_F64, 1));
  // a described site: the elementwise MPO step where it fits
  for (int dom = 0; dom < 2; ++dom)
    for (const char* kind : {"penta", "dense", "tri", "zero", "manyblk", "manydst", "bigblk"})
      for (int64_t d : {8, 16, 32})
        for (int var = 0; var < 5; ++var) {
          if (var > 0 && (d != 16 || std::string(kind) != "penta")) continue;
          const Site st = make_site(kind, d);
          const WSiteInfo wi = st.info();
          hooks(0, true, int64_t(1) << 28, 64, 8);
          // var 1: ancilla; 2: real working dtype; 3: the description is of another site; 4: unit channel + bra bonds differ
          const int64_t danc = var == 1 ? 2 : 1;
          const int dt = var == 2 ? 0 : 1;
          mpse_dims m = env_dims(12, 20, var == 4 ? 16 : 12, var == 4 ? 24 : 20, d, st.wl + (var == 3), st.wr, danc,
                                 var == 4 ? 1 : 0);
          if (var != 4) m.env_unit = dom == 0 ? st.wl : 1;
          emit(key("envw.%c.%s.d%lld.v%d", dom ? 'R' : 'L', kind, (long long)d, var),
               plan_env(DT[dt][0], dom ? MPSE_DOMAIN_R : MPSE_DOMAIN_L, m, DT[dt][1], DT[dt][3], 1, &wi), var == 0 || var == 4);
        }
  // a small site (d < 8) keeps the batched product
  {
    const Site st = make_site("tri", 4);
    const WSiteInfo wi = st.info();
    emit("envw.L.tri.d4", plan_env(MPSE_C128, MPSE_DOMAIN_L, env_dims(12, 20, 12, 20, 4, st.wl, st.wr, 1, 0), MPSE_F64, MPSE_F64, 1, &wi));
  }
}

static void cases_env_multi() {
  const int64_t wl[4] = {3, 2, 1, 4}, wr[4] = {2, 3, 2, 1};
  for (int n = 0; n <= 5; ++n)
    for (int dom = 0; dom < 3; ++dom)
      for (int dt = 0; dt < 3; ++dt)
        for (int64_t danc = 0; danc <= 2; ++danc)
          for (int sh = 0; sh < 2; ++sh)
            for (int cj = 0; cj < 2; ++cj) {
              if ((n == 0 || n == 5 || dom == 2) && (dt || danc || sh || cj)) continue;
              default_hooks();
              const mpse_dims m = sh ? env_dims(1, 5, 3, 1, 1, 0, 0, danc, 0) : env_dims(6, 5, 7, 4, 3, 0, 0, danc, 0);
              emit(key("envm.n%d.%c.t%d.a%lld.s%d.cj%d", n, dom == 0 ? 'L' : dom == 1 ? 'R' : 'X', dt, (long long)danc, sh, cj),
                   plan_env_multi(DT[dt][0], dom == 0 ? MPSE_DOMAIN_L : dom == 1 ? MPSE_DOMAIN_R : 77, m, n, wl, wr, DT[dt][1],
                                  DT[dt][3], cj));
            }
}

static void cases_heff2() {
  default_hooks();
  for (int ns = 0; ns <= 2; ++ns)
    for (int dt = 0; dt < 3; ++dt)
      for (int sh = 0; sh < 3; ++sh)
        for (int64_t danc = 0; danc <= 2; ++danc)
          for (int64_t danc1 = 0; danc1 <= 3; danc1 += 3)
            for (int bra = 0; bra < 3; ++bra) {
              if (bra && (dt || sh || danc || danc1)) continue;
              const Shape& s = SHAPES[sh];
              const mpse_heff h = heff(ns, dt, s.Dl, s.Dr, bra == 1 ? s.Dl : bra == 2 ? s.Dl + 1 : 0, bra == 1 ? s.Dr : 0, s.d0, s.d1,
                                       s.wl, s.wm, s.wr, danc, danc1, 0, 0);
              emit(key("heff2.n%d.t%d.s%d.a%lld.%lld.b%d", ns, dt, sh, (long long)danc, (long long)danc1, bra),
                   plan_heff2(DT[dt][0], h));
            }
}

static void cases_ft() {
  default_hooks();
  const int legs[5][2] = {{MPSE_LEG_UP, MPSE_LEG_UP}, {MPSE_LEG_DOWN, MPSE_LEG_DOWN}, {MPSE_LEG_UP, MPSE_LEG_DOWN},
                          {MPSE_LEG_DOWN, MPSE_LEG_UP}, {MPSE_LEG_UP, 99}};
  for (int lg = 0; lg < 5; ++lg)
    for (int tr = 0; tr < 4; ++tr)
      for (int dt = 0; dt < 3; ++dt)
        for (int sh = 0; sh < 2; ++sh) {
          if (lg >= 3 && (tr || dt || sh)) continue;
          mpse_heff_ft h{};
          if (sh == 0) h.Dl = 6, h.Dr = 5, h.d_up = 3, h.d_down = 2, h.wl1 = 2, h.wr1 = 3, h.wl2 = 4, h.wr2 = 2;
          if (sh == 1) h.Dl = 1, h.Dr = 4, h.d_up = 1, h.d_down = 3, h.wl1 = 1, h.wr1 = 2, h.wl2 = 3, h.wr2 = 1;
          h.leg1 = legs[lg][0], h.leg2 = legs[lg][1], h.trans1 = tr & 1, h.trans2 = tr >> 1;
          h.l_dtype = DT[dt][1], h.r_dtype = DT[dt][2], h.w_dtype = DT[dt][3];
          emit(key("ft.heff.l%d.tr%d.t%d.s%d", lg, tr, dt, sh), plan_heff_ft(DT[dt][0], h));
          for (int dom = 0; dom < 3; ++dom) {
            if (dom == 2 && (lg || tr || dt || sh)) continue;
            emit(key("ft.env%c.l%d.tr%d.t%d.s%d", dom == 0 ? 'L' : dom == 1 ? 'R' : 'X', lg, tr, dt, sh),
                 plan_env_ft(DT[dt][0], dom == 0 ? MPSE_DOMAIN_L : dom == 1 ? MPSE_DOMAIN_R : 77, h, DT[dt][1]));
          }
        }
  mpse_heff_ft h{};
  h.Dl = 4, h.Dr = 4, h.d_up = 0, h.d_down = 2, h.wl1 = h.wr1 = h.wl2 = h.wr2 = 2, h.leg1 = h.leg2 = MPSE_LEG_UP;
  emit("ft.heff.empty", plan_heff_ft(MPSE_C128, h));
}

static void cases_fold() {
  for (const char* kind : SITE_KINDS)
    for (int64_t d : {4, 16, 32, 3, 36})
      for (int64_t wr : {4, 7})
        for (int units = 0; units < 4; ++units)        // bit 0: l_unit, bit 1: r_unit
          for (int epi = 0; epi < 2; ++epi)
            for (int two = 0; two < 3; ++two) {         // 2: the caller takes two results, the split2 switch is off
              const std::string k = kind;
              const bool sized = k == "plain" || k == "ident" || k == "diag" || k == "tri" || k == "penta" || k == "second" ||
                                 k == "wide" || k == "dense" || k == "passonly" || k == "zero" || k == "fanout";
              if (wr == 7 && (!sized || d != 4)) continue;
              if ((d == 3 || d == 36) && (k != "penta" || units != 3)) continue;
              if (d == 32 && k != "bigblk" && k != "penta") continue;
              if (k == "bigblk" && d != 32 && d != 4) continue;
              if (two == 2 && (k != "penta" || d != 4)) continue;
              const Site st = make_site(k, d, wr);
              const WSiteInfo wi = st.info();
              hooks(int64_t(1) << 27, true, 1, 4, 1, two != 2);
              const int64_t lu = (units & 1) ? 1 : 0, ru = (units & 2) ? st.wr : 0;
              const mpse_heff h = heff(1, 1, 8, 12, 0, 0, d, 1, st.wl, 1, st.wr, 1, 0, lu, ru);
              emit(key("fold.%s.d%lld.w%lld.u%d.e%d.r%d", kind, (long long)d, (long long)wr, units, epi, two),
                   plan_heff1_fold(MPSE_C128, h, wi, two != 0, epi != 0));
            }
  // refusals and switches around one site; plan_heff with a described site (folded, or the chain where it is refused)
  const Site st = make_site("penta", 4);
  const WSiteInfo wi = st.info();
  const Site other = make_site("penta", 4, 5);
  const WSiteInfo wo = other.info();
  struct Var {
    const char* name;
    int ns, dt;
    int64_t Dl, Dr, Dlb, Drb, danc, fmin, align, min_kt, cus;
    bool other;
  };
  const Var vars[] = {
      {"ok", 1, 1, 8, 12, 0, 0, 1, 1, 4, 1, 256, false},        {"real", 1, 0, 8, 12, 0, 0, 1, 1, 4, 1, 256, false},
      {"real_r", 1, 3, 8, 12, 0, 0, 1, 1, 4, 1, 256, false},    {"real64", 1, 0, 64, 64, 0, 0, 1, 1, 64, 1, 256, false},
      {"real_r64", 1, 3, 64, 64, 0, 0, 1, 1, 64, 1, 256, false}, {"c64", 1, 1, 64, 64, 0, 0, 1, 1, 64, 1, 256, false},
      {"anc", 1, 1, 8, 12, 0, 0, 2, 1, 4, 1, 256, false},       {"danc0", 1, 1, 8, 12, 0, 0, 0, 1, 4, 1, 256, false},
      {"nsite2", 2, 1, 8, 12, 0, 0, 1, 1, 4, 1, 256, false},    {"othersite", 1, 1, 8, 12, 0, 0, 1, 1, 4, 1, 256, true},
      {"small", 1, 1, 8, 12, 0, 0, 1, int64_t(1) << 28, 4, 1, 256, false},
      {"unaligned_bra", 1, 1, 8, 12, 6, 0, 1, 1, 4, 1, 256, false}, {"unaligned_l", 1, 1, 6, 12, 8, 0, 1, 1, 4, 1, 256, false},
      {"unaligned_r", 1, 1, 8, 10, 0, 0, 1, 1, 4, 1, 256, false},   {"bra_l", 1, 1, 8, 12, 12, 0, 1, 1, 4, 1, 256, false},
      {"bra_r", 1, 1, 8, 12, 0, 16, 1, 1, 4, 1, 256, false},        {"min_kt", 1, 1, 8, 12, 0, 0, 1, 1, 4, 8, 256, false},
      {"few_cus", 1, 1, 8, 12, 0, 0, 1, 1, 4, 1, 0, false},         {"rows", 1, 1, 4, 12, 0, 0, 1, 1, 4, 1, 256, false},
      {"wide64", 1, 1, 64, 128, 0, 0, 1, 1, 64, 1, 256, false},   {"complex_w", 1, 2, 8, 12, 0, 0, 1, 1, 4, 1, 256, false},
  };
  for (const Var& v : vars)
    for (int via = 0; via < 2; ++via)
      for (int epi = 0; epi < 2; ++epi) {
        hooks(int64_t(1) << 27, true, v.fmin, v.align, v.min_kt, true, v.cus);
        const mpse_heff h = heff(v.ns, v.dt, v.Dl, v.Dr, v.Dlb, v.Drb, 4, 4, st.wl, st.wr, st.wr, v.danc, 0, 1, st.wr);
        const WSiteInfo& w = v.other ? wo : wi;
        emit(key("foldvar.%s.via%d.e%d", v.name, via, epi),
             via ? plan_heff(DT[v.dt][0], h, &w, true, epi != 0) : plan_heff1_fold(DT[v.dt][0], h, w, true, epi != 0));
      }
}

// The benchmark's own shapes: bonds of 256, d = 2 (electronic sites) and 16 (phonon sites), MPO bonds 4 and 5; every
// hook at the value the product runs with
static void cases_full_size() {
  default_hooks();
  const int64_t D = 256;
  const int64_t wlr[4][2] = {{4, 5}, {5, 4}, {5, 5}, {4, 4}};
  for (int dt = 1; dt < 3; ++dt)
    for (int64_t Dl : {256, 64})
      for (const auto& w : wlr)
        for (int units = 0; units < 2; ++units) {
          const int64_t wl = w[0], wr = w[1], lu = units ? 1 : 0, ru = units ? wr : 0;
          if (wl == wr) emit(key("full.heff0.t%d.D%lld.w%lld.u%d", dt, (long long)Dl, (long long)wl, units),
                             plan_heff(MPSE_C128, heff(0, dt, Dl, Dl, 0, 0, 1, 1, wl, 1, wr, 1, 0, lu, ru)));
          for (int64_t d : {2, 16}) {
            emit(key("full.heff1.t%d.D%lld.d%lld.w%lld%lld.u%d", dt, (long long)Dl, (long long)d, (long long)wl, (long long)wr, units),
                 plan_heff(MPSE_C128, heff(1, dt, Dl, D, 0, 0, d, 1, wl, 1, wr, 1, 0, lu, ru)));
            emit(key("full.heff2.t%d.D%lld.d%lld.w%lld%lld.u%d", dt, (long long)Dl, (long long)d, (long long)wl, (long long)wr, units),
                 plan_heff(MPSE_C128, heff(2, dt, Dl, D, 0, 0, d, 18 - d, wl, 5, wr, 1, 0, lu, ru)));
            for (int dom = 0; dom < 2; ++dom) {
              const mpse_dims m = env_dims(Dl, D, Dl, D, d, wl, wr, 1, units ? (dom ? wr : 1) : 0);
              emit(key("full.env%c.t%d.D%lld.d%lld.w%lld%lld.u%d", dom ? 'R' : 'L', dt, (long long)Dl, (long long)d, (long long)wl,
                       (long long)wr, units),
                   plan_env(MPSE_C128, dom ? MPSE_DOMAIN_R : MPSE_DOMAIN_L, m, DT[dt][1], MPSE_F64, 1));
            }
          }
        }
  // the phonon site with its block structure described: folded matvec, elementwise environment step
  for (const char* kind : {"penta", "tri", "plain", "second"})
    for (int64_t Dl : {256, 128, 64})
      for (int units = 0; units < 4; ++units)
        for (int epi = 0; epi < 2; ++epi)
          for (int two = 0; two < 2; ++two) {
            const Site st = make_site(kind, 16);
            const WSiteInfo wi = st.info();
            const int64_t lu = (units & 1) ? 1 : 0, ru = (units & 2) ? st.wr : 0;
            emit(key("full.fold.%s.D%lld.u%d.e%d.r%d", kind, (long long)Dl, units, epi, two),
                 plan_heff(MPSE_C128, heff(1, 1, Dl, D, 0, 0, 16, 1, st.wl, 1, st.wr, 1, 0, lu, ru), &wi, two != 0, epi != 0));
            if (epi || two) continue;
            for (int dom = 0; dom < 2; ++dom) {
              const mpse_dims m = env_dims(Dl, D, Dl, D, 16, st.wl, st.wr, 1, (units & 1) ? (dom ? st.wr : 1) : 0);
              emit(key("full.envw%c.%s.D%lld.u%d", dom ? 'R' : 'L', kind, (long long)Dl, units),
                   plan_env(MPSE_C128, dom ? MPSE_DOMAIN_R : MPSE_DOMAIN_L, m, MPSE_C128, MPSE_F64, 1, &wi), 1);
            }
          }
}

int main(int argc, char** argv) {
  if (argc == 3 && std::string(argv[1]) == "--case") g_want = argv[2];
  cases_heff();
  cases_env();
  cases_env_multi();
  cases_heff2();
  cases_ft();
  cases_fold();
  cases_full_size();
  if (g_want) {
    if (!g_found) fprintf(stderr, "no such case: %s\n", g_want);
    return g_found ? 0 : 1;
  }
  for (const char* t : TALLIES) printf("tally %s %lld\n", t, g_tally[t]);
  for (const auto& kv : g_tally)
    if (kv.first.rfind("error: ", 0) == 0) printf("tally %s = %lld\n", kv.first.c_str(), kv.second);
  return 0;
}
