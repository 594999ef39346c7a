// Hot-path contractions: environment update and effective-Hamiltonian matvec.
// The index algebra lives in mpse_plans.h (a list of strided-GEMM steps); this file
// executes a plan on the device with the FP64-MFMA contraction kernel.
#include <deque>

#include "mpse_internal.h"
#include "mpse_plans.h"

using namespace mpse_plan;

namespace {

__device__ __forceinline__ long long off2(const mpse_index m, long long i) {
  if (m.lo_ext >= m.ext) return i * m.s_lo;
  const long long hi = i / m.lo_ext;
  return hi * m.s_hi + (i - hi * m.lo_ext) * m.s_lo;
}

// dst(i,j) = src(i,j) through two-level row / column maps; one 16 B (complex) or 8 B element per thread,
// threads run along j so contiguous columns coalesce
template <typename T>
__global__ __launch_bounds__(256) void k_copy_strided(T* dst, const T* src, mpse_index mi, mpse_index ni, mpse_index mo,
                                                      mpse_index no, const int* skip) {
  if (skip && *skip) return;
  const long long nn = ni.ext;
  const long long total = mi.ext * nn;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const long long i = t / nn, j = t - i * nn;
    dst[off2(mo, i) + off2(no, j)] = src[off2(mi, i) + off2(ni, j)];
  }
}

// dev[b] = max_{a,c} | E[a,b,c] - delta(a,c) | for an environment E (D, w, D); doubles are non-negative, so
// their bit patterns order like integers and atomicMax on the 64-bit pattern is an exact max
template <bool CPLX>
__global__ __launch_bounds__(256) void k_unit_deviation(const double* env, int D, int w, unsigned long long* dev) {
  constexpr int E = CPLX ? 2 : 1;
  const int a = blockIdx.x;
  __shared__ double red[4];
  for (int b = 0; b < w; ++b) {
    const double* row = env + ((long long)a * w + b) * D * E;
    double m = 0.0;
    for (int c = threadIdx.x; c < D; c += 256) {
      double re = row[c * E] - (c == a ? 1.0 : 0.0);
      double v = fabs(re);
      if (!(v <= 1e300)) v = 1e300;  // NaN / inf never pass for a unit channel; each part on its own, because
      if (CPLX) {                    // fmax returns its other argument when one is NaN
        double vi = fabs(row[c * E + 1]);
        if (!(vi <= 1e300)) vi = 1e300;
        v = fmax(v, vi);
      }
      m = fmax(m, v);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
      atomicMax(dev + b, (unsigned long long)__double_as_longlong(m));
    }
    __syncthreads();
  }
}

// ---- MPO step of a small site (wl d <= 16 inputs, d wr <= 16 outputs per bond state and trailing index: the d = 2
// sites of a Holstein chain):  T2[a, dd, f, n] = sum_{b,e} W[b, dd, e, f] T1[b, a, e, n].  As a batched MFMA product
// this is 8 x 8 x 256 per bond state padded to 64 x 64 tiles (14 us); here one thread owns one (a, n), reads its
// inputs (coalesced along n), multiplies by W out of LDS and stores its outputs: two passes over 18 MB.
struct WsmArgs {
  const double* T1;
  double* T2;
  const double* W;
  int Da, d, wl, wr, N;
  const int* skip;
  // channels [b_lo, b_hi) of T1 arrive as `nslices` K slices of the product that forms them (slice s of channel b, row
  // a at slices + s * slice_stride + (((b - b_lo) * Da + a) * d + e) * N + n): added here instead of by a launch of
  // their own (nslices == 0: everything is read from T1)
  const double* slices;
  long long slice_stride;
  int nslices, b_lo, b_hi;
};

template <bool CPLX>
__global__ __launch_bounds__(256) void k_wsmall(const WsmArgs g) {
  if (g.skip && *g.skip) return;
  constexpr int E = CPLX ? 2 : 1;
  __shared__ double s_w[16][16];   // [o = dd * wr + f][be = b * d + e]
  const int nrow = g.wl * g.d, no = g.d * g.wr;
  {
    const int o = threadIdx.x >> 4, be = threadIdx.x & 15;
    double v = 0.0;
    if (o < no && be < nrow) {
      const int dd = o / g.wr, f = o - dd * g.wr, b = be / g.d, e = be - b * g.d;
      v = g.W[(((long long)b * g.d + dd) * g.d + e) * g.wr + f];
    }
    s_w[o][be] = v;
  }
  __syncthreads();
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)g.Da * g.N) return;
  const int a = (int)(idx / g.N), n = (int)(idx - (long long)a * g.N);
  double xr[16], xi[16];
#pragma unroll
  for (int be = 0; be < 16; ++be) {
    xr[be] = 0.0;
    xi[be] = 0.0;
    if (be < nrow) {
      const int b = be / g.d, e = be - b * g.d;
      if (g.nslices > 0 && b >= g.b_lo && b < g.b_hi) {
        const double* src = g.slices + ((((long long)(b - g.b_lo) * g.Da + a) * g.d + e) * g.N + n) * E;
        for (int sl = 0; sl < g.nslices; ++sl) {      // slice order: the same sum as the reduction launch forms
          xr[be] += src[0];
          if constexpr (CPLX) xi[be] += src[1];
          src += g.slice_stride * E;
        }
      } else {
        const double* src = g.T1 + ((((long long)b * g.Da + a) * g.d + e) * g.N + n) * E;
        xr[be] = src[0];
        if constexpr (CPLX) xi[be] = src[1];
      }
    }
  }
#pragma unroll
  for (int o = 0; o < 16; ++o) {
    if (o >= no) break;
    double ar = 0.0, ai = 0.0;
#pragma unroll
    for (int be = 0; be < 16; ++be) {
      const double w = s_w[o][be];   // zero beyond nrow
      ar += w * xr[be];
      if constexpr (CPLX) ai += w * xi[be];
    }
    double* dst = g.T2 + (((long long)a * no + o) * g.N + n) * E;
    dst[0] = ar;
    if constexpr (CPLX) dst[1] = ai;
  }
}

// ---- elementwise MPO step of the folded one-site matvec (mpse_plans.h: K_WMIX):
//   dst_j[a, dd, k] = sum_terms sum_e W[b_t, dd, e, f_t] src_t[a, e, k]
// A thread owns one (a, k) and WM_CHUNK consecutive dd (lanes run along k: every load / store of a wave is 1 KB
// contiguous; the chunks of one (a, k) sit in neighbouring waves and share their loads in L2); it reads only the
// columns e its rows touch ([e_lo, e_hi) per term and chunk, from the host copy of the site: a tridiagonal block
// costs six loads per chunk, an identity block is a plain add).  Non-identity blocks sit in LDS as dense d x d matrices.
struct WmixTermDev {
  const double* src;
  long long s_a, s_d;
  int b, f, ident, slot;
  unsigned char e_lo[WM_MAXCHUNKS], e_hi[WM_MAXCHUNKS];
};
struct WmixDstDev {
  double* dst;
  long long s_a, s_d;
  int nterm, pad;
  WmixTermDev term[WM_MAXTERM];
};
struct WmixArgs {
  WmixDstDev dst[WM_MAXDST];
  const double* W;
  int ndst, Da, d, wr, Dk, nchunk, nslot;
  const int* skip;
};

template <bool CPLX>
__global__ __launch_bounds__(256) void k_wmix(const WmixArgs g) {
  if (g.skip && *g.skip) return;
  constexpr int E = CPLX ? 2 : 1;
  extern __shared__ double s_blk[];               // [slot][dd][e]
  const int d = g.d, dd2 = d * d;
  for (int j = 0; j < g.ndst; ++j)
    for (int t = 0; t < g.dst[j].nterm; ++t) {
      const WmixTermDev& tm = g.dst[j].term[t];
      if (tm.ident) continue;
      for (int r = threadIdx.x; r < dd2; r += 256) {
        const int x = r / d, e = r - x * d;
        s_blk[tm.slot * dd2 + r] = g.W[(((long long)tm.b * d + x) * d + e) * g.wr + tm.f];
      }
    }
  __syncthreads();
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)g.Da * g.nchunk * g.Dk) return;
  const int k = (int)(idx % g.Dk);
  const long long rest = idx / g.Dk;
  const int q = (int)(rest % g.nchunk), a = (int)(rest / g.nchunk);
  const int x0 = q * WM_CHUNK;
  for (int j = 0; j < g.ndst; ++j) {
    const WmixDstDev& D = g.dst[j];
    double ar[WM_CHUNK], ai[WM_CHUNK];
#pragma unroll
    for (int i = 0; i < WM_CHUNK; ++i) ar[i] = 0.0, ai[i] = 0.0;
    for (int t = 0; t < D.nterm; ++t) {
      const WmixTermDev& tm = D.term[t];
      const double* src = tm.src + ((long long)a * tm.s_a + k) * E;
      if (tm.ident) {
#pragma unroll
        for (int i = 0; i < WM_CHUNK; ++i)
          if (x0 + i < d) {
            const double* p = src + (long long)(x0 + i) * tm.s_d * E;
            ar[i] += p[0];
            if constexpr (CPLX) ai[i] += p[1];
          }
        continue;
      }
      const double* blk = s_blk + tm.slot * dd2;
      const int lo = tm.e_lo[q], hi = tm.e_hi[q];
      for (int e0 = lo; e0 < hi; e0 += 8) {
        double vr[8], vi[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {      // the loads of a batch are issued together
          vr[u] = 0.0, vi[u] = 0.0;
          if (e0 + u < hi) {
            const double* p = src + (long long)(e0 + u) * tm.s_d * E;
            vr[u] = p[0];
            if constexpr (CPLX) vi[u] = p[1];
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (e0 + u < hi) {
#pragma unroll
            for (int i = 0; i < WM_CHUNK; ++i)
              if (x0 + i < d) {
                const double w = blk[(x0 + i) * d + e0 + u];
                ar[i] += w * vr[u];
                if constexpr (CPLX) ai[i] += w * vi[u];
              }
          }
      }
    }
    double* dst = D.dst + ((long long)a * D.s_a + k) * E;
#pragma unroll
    for (int i = 0; i < WM_CHUNK; ++i)
      if (x0 + i < d) {
        double* p = dst + (long long)(x0 + i) * D.s_d * E;
        if constexpr (CPLX)
          *reinterpret_cast<double2*>(p) = make_double2(ar[i], ai[i]);
        else
          p[0] = ar[i];
      }
  }
}

int copy_call(mpse_ctx* ctx, int dtype, const void* src, void* dst, mpse_index mi, mpse_index ni, mpse_index mo,
              mpse_index no, const int* skip) {
  const long long total = mi.ext * ni.ext;
  if (total <= 0) return MPSE_OK;
  long long nb = (total + 255) / 256;
  if (nb > 65536) nb = 65536;
  if (dtype == MPSE_C128)
    hipLaunchKernelGGL((k_copy_strided<double2>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, (double2*)dst,
                       (const double2*)src, mi, ni, mo, no, skip);
  else
    hipLaunchKernelGGL((k_copy_strided<double>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, (double*)dst,
                       (const double*)src, mi, ni, mo, no, skip);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

// One run of a plan: what the executors of its steps share
struct PlanRun {
  mpse_ctx* ctx;
  int dtype;
  size_t es;                   // element size of the working dtype
  const void* bufs[B_COUNT];   // operands and temporaries by buffer id
  SolveScope* sc;              // the solve the plan runs in (may be null) ...
  MatvecReq* mv;               // ... and the requests of the matvec it computes (may be null)
  const int* skip;             // sc->skip
  MatvecReq::Dot* dot;         // mv->dot where the caller gave a partner, else null
  TmpBuf slices;               // K slices that a product (Step::slices_to) left to the elementwise MPO step ...
  int slices_used = 0;         // ... and how many (0: none; whether it leaves any is the product's decision when it runs)
  PlanRun(mpse_ctx* c, int dt, const void* const* b, SolveScope* s, MatvecReq* m)
      : ctx(c), dtype(dt), es(dtype_size(dt)), sc(s), mv(m), skip(s ? s->skip : nullptr),
        dot(m && m->dot.y ? &m->dot : nullptr), slices(c) {
    for (int i = 0; i < B_COUNT; ++i) bufs[i] = b[i];
  }
  // *p = element `off` of buffer `buf`, whose elements are of dtype `dt`
  template <class T>
  int resolve(int buf, int64_t off, int dt, T** p) const {
    if (!bufs[buf]) return mpse_fail(ctx, MPSE_ERR_ARG, "plan: missing buffer");
    *p = (T*)((char*)const_cast<void*>(bufs[buf]) + size_t(off) * dtype_size(dt));
    return MPSE_OK;
  }
};

// MPO step of a small site (Step::elementwise_w): it adds the K slices that the product of its input channels left it
int run_wsmall(PlanRun& r, const Step& s) {
  WsmArgs g;
  MPSE_TRY(r.resolve(s.a, s.a_off, s.dta, &g.W));
  MPSE_TRY(r.resolve(s.b, s.b_off, s.dtb, &g.T1));
  MPSE_TRY(r.resolve(s.c, s.c_off, s.dtb, &g.T2));
  g.Da = (int)s.w_Da, g.d = (int)s.w_d, g.wl = (int)s.w_wl, g.wr = (int)s.w_wr, g.N = (int)s.w_N;
  g.skip = r.skip;
  g.slices = r.slices_used > 0 ? r.slices.as<const double>() : nullptr;
  g.nslices = r.slices_used, g.slice_stride = s.slice_elems, g.b_lo = (int)s.slice_b_lo, g.b_hi = (int)s.slice_b_hi;
  r.slices_used = 0;
  const long long total = s.w_Da * s.w_N;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (s.dtb == MPSE_C128)
    hipLaunchKernelGGL((k_wsmall<true>), grid, dim3(256), 0, r.ctx->stream, g);
  else
    hipLaunchKernelGGL((k_wsmall<false>), grid, dim3(256), 0, r.ctx->stream, g);
  MPSE_HIP(r.ctx, hipGetLastError());
  return MPSE_OK;
}

int run_wmix(PlanRun& r, const Step& s) {
  WmixArgs g;
  memset(&g, 0, sizeof(g));
  MPSE_TRY(r.resolve(s.b, 0, MPSE_F64, &g.W));
  g.ndst = (int)s.mix.size();
  g.Da = (int)s.wp_Da, g.d = (int)s.wp_d, g.wr = (int)s.wp_wr, g.Dk = (int)s.wp_Dk;
  g.nchunk = (g.d + WM_CHUNK - 1) / WM_CHUNK;
  g.skip = r.skip;
  int nslot = 0;
  for (int j = 0; j < g.ndst; ++j) {
    const WMixDst& q = s.mix[j];
    MPSE_TRY(r.resolve(q.dst, q.dst_off, r.dtype, &g.dst[j].dst));
    g.dst[j].s_a = q.s_a, g.dst[j].s_d = q.s_d, g.dst[j].nterm = q.nterm;
    for (int t = 0; t < q.nterm; ++t) {
      const WMixTerm& tm = q.term[t];
      WmixTermDev& o = g.dst[j].term[t];
      MPSE_TRY(r.resolve(tm.src, tm.src_off, r.dtype, &o.src));
      o.s_a = tm.s_a, o.s_d = tm.s_d, o.b = tm.b, o.f = tm.f, o.ident = tm.ident ? 1 : 0;
      o.slot = tm.ident ? 0 : nslot++;
      memcpy(o.e_lo, tm.e_lo, sizeof(o.e_lo));
      memcpy(o.e_hi, tm.e_hi, sizeof(o.e_hi));
    }
  }
  g.nslot = nslot;
  const size_t lds = size_t(nslot > 0 ? nslot : 1) * g.d * g.d * sizeof(double);
  if (lds > 64 * 1024) return mpse_fail(r.ctx, MPSE_ERR_SHAPE, "plan: MPO blocks of the elementwise step exceed the LDS");
  const long long total = (long long)s.wp_Da * g.nchunk * s.wp_Dk;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (r.dtype == MPSE_C128)
    hipLaunchKernelGGL((k_wmix<true>), grid, dim3(256), lds, r.ctx->stream, g);
  else
    hipLaunchKernelGGL((k_wmix<false>), grid, dim3(256), lds, r.ctx->stream, g);
  ++r.ctx->gemm_paths[mpse_ctx::GP_WMIX];
  MPSE_HIP(r.ctx, hipGetLastError());
  return MPSE_OK;
}

// Occupancy of an operand that is scanned once for all segments reading parts of it: the environments, by a scan that
// the solve keeps (one scan serves every channel).  *flags stays null where the plan asks for none.
int scan_flags(PlanRun& r, const ScanDesc& sd, TmpBuf& tmp, const unsigned char** flags, int* pitch, bool* stable) {
  if (!sd.on || !r.bufs[sd.buf]) return MPSE_OK;
  const char* ptr;
  MPSE_TRY(r.resolve(sd.buf, sd.off, sd.dt, &ptr));
  bool st = false;
  MPSE_TRY(occ_mask_get(r.ctx, r.sc, ptr, sd.dt, sd.r, sd.k, tmp, flags, pitch, &st));
  *stable = *stable && st;
  return MPSE_OK;
}

// Structural mask of the centre (B_C) as operand B of a grouped step: K = its left bond, columns = (e, k); null where
// the solve has none that fits (prepared operands: pushed through the MPO block)
const unsigned char* centre_mask(const PlanRun& r, const Step& s, int* pitch) {
  const int64_t K = s.kb.ext, N = s.nb.ext;
  const int64_t nkw = ((K + 15) / 16 + 7) / 8, ntn = (N + 63) / 64;
  if (!r.sc || !r.sc->in_krylov(r.bufs[B_C]) || r.sc->cmask.bytes != ntn * nkw * 8) return nullptr;
  *pitch = (int)(nkw * 8);
  return static_cast<const unsigned char*>(r.sc->cmask.ptr);
}

// the beta term of group `i` formed in the epilogue from the blocks of the MPO site (GGroupPlan::nmix)
int bind_epilogue_mix(PlanRun& r, const GGroupPlan& g, int i, GroupedDesc& gd) {
  if (gd.nmix > 0 || !r.bufs[g.wbuf]) return mpse_fail(r.ctx, MPSE_ERR_ARG, "plan: bad epilogue mix");
  gd.nmix = g.nmix, gd.mix_grp = i;
  gd.mix_w = r.bufs[g.wbuf];
  gd.mix_d = (int)g.mix_d, gd.mix_wr = (int)g.mix_wr, gd.mix_ld = g.mix_ld;
  for (int t = 0; t < g.nmix; ++t) {
    const EpiTerm& m = g.mix[t];
    MPSE_TRY(r.resolve(m.src, m.src_off, r.dtype, &gd.mix[t].src));
    gd.mix[t].b = m.b, gd.mix[t].f = m.f, gd.mix[t].delta = m.delta;
  }
  return MPSE_OK;
}

int run_ggemm(PlanRun& r, const Step& s) {
  GroupedDesc gd;
  gd.dta = s.dta, gd.dtb = s.dtb;
  gd.ma = s.ma, gd.ka = s.ka, gd.kb = s.kb, gd.nb = s.nb, gd.mc = s.mc, gd.nc = s.nc;
  gd.ngrp = (int)s.groups.size();
  TmpBuf MA(r.ctx), MB(r.ctx);
  const unsigned char *fa = nullptr, *fb = nullptr;
  bool stable = true;
  MPSE_TRY(scan_flags(r, s.scan_a, MA, &fa, &gd.am_pitch, &stable));
  MPSE_TRY(scan_flags(r, s.scan_b, MB, &fb, &gd.bm_pitch, &stable));
  int cm_pitch = 0;
  const unsigned char* cm = centre_mask(r, s, &cm_pitch);
  for (int i = 0; i < gd.ngrp; ++i) {
    const GGroupPlan& g = s.groups[i];
    GroupedGrp& o = gd.grp[i];
    MPSE_TRY(r.resolve(g.cbuf, g.c_off, r.dtype, &o.C));
    o.nseg = g.nseg;
    o.beta = g.beta;
    if (g.nmix > 0) MPSE_TRY(bind_epilogue_mix(r, g, i, gd));
    for (int q = 0; q < g.nseg; ++q) {
      const GSegPlan& sg = g.seg[q];
      MPSE_TRY(r.resolve(sg.abuf, sg.a_off, s.dta, &o.seg[q].A));
      MPSE_TRY(r.resolve(sg.bbuf, sg.b_off, s.dtb, &o.seg[q].B));
      if (fa && sg.am_row0 >= 0) o.seg[q].am = fa + size_t(sg.am_row0) * gd.am_pitch;
      if (sg.bm_kind == BM_SCAN && fb) {
        o.seg[q].bm = fb + sg.bm_kt0;
      } else if (sg.bm_kind == BM_CENTRE && cm) {
        o.seg[q].bm = cm;
        gd.bm_pitch = cm_pitch;
      }
    }
  }
  gd.masks_stable = stable;
  if (gd.ngrp == 1 && s.groups[0].split2) {
    if (!r.bufs[B_OUT2]) return mpse_fail(r.ctx, MPSE_ERR_ARG, "plan: missing second result");
    gd.split2 = true;
    gd.c2 = const_cast<void*>(r.bufs[B_OUT2]);
  }
  // the step that completes the result carries the caller's dot request and result mask
  MPSE_TRY(gemm_grouped(r.ctx, gd, r.sc, s.completes ? r.dot : nullptr,
                        s.completes && r.mv && r.mv->out_mask.mask ? &r.mv->out_mask : nullptr));
  return MPSE_OK;
}

// plain product (K_GEMM) or copy (K_COPY)
int run_product(PlanRun& r, const Step& s) {
  const int dtc = (s.dta == MPSE_C128 || s.dtb == MPSE_C128) ? MPSE_C128 : MPSE_F64;
  if (dtc != r.dtype)  // every step of a plan must produce the working dtype
    return mpse_fail(r.ctx, MPSE_ERR_ARG, "plan step dtype mismatch (got %d want %d)", dtc, r.dtype);
  const char *a, *b;
  char* c;
  MPSE_TRY(r.resolve(s.a, s.a_off, s.dta, &a));
  MPSE_TRY(r.resolve(s.b, s.b_off, s.dtb, &b));
  MPSE_TRY(r.resolve(s.c, s.c_off, dtc, &c));
  if (s.kind == K_COPY) return copy_call(r.ctx, dtc, a, c, s.ma, s.ka, s.mc, s.nc, r.skip);
  ProductReq rq;
  if (s.completes) rq.dot = r.dot;   // a plain product into the whole of `out` takes the caller's dot request along
  if (s.cin >= 0) {
    if (!r.bufs[s.cin]) return mpse_fail(r.ctx, MPSE_ERR_ARG, "plan: missing beta source");
    rq.cin = (const char*)r.bufs[s.cin] + size_t(s.cin_off) * dtype_size(dtc);
    rq.cin_m = s.mcin;
    rq.cin_n = s.ncin;
  }
  if (s.slices_to >= 0) {
    // room for four slices of this product's result (more: the product reduces them itself, as usual); without the
    // room the offer is withdrawn
    const size_t blk = size_t(s.mc.ext) * size_t(s.nc.ext) * dtype_size(dtc);
    if (r.slices.alloc(4 * blk) == MPSE_OK) {
      rq.slices = r.slices.p;
      rq.slices_cap = 4 * blk;
    }
  }
  MPSE_TRY(gemm_call(r.ctx, s.dta, s.dtb, s.conja, s.conjb, s.ma, s.ka, s.kb, s.nb, s.mc, s.nc, s.batch, s.sba, s.sbb,
                     s.sbc, a, b, c, 1.0, s.beta, s.skip_zero, r.sc, &rq));
  if (rq.slices_used > 0) r.slices_used = rq.slices_used;
  return MPSE_OK;
}

}  // namespace

// sc: the solve the plan runs in, mv: the requests of the matvec it computes (both may be null)
static int run_plan(mpse_ctx* ctx, int dtype, const Plan& p, const void* bufs_in[B_COUNT],
                    SolveScope* sc = nullptr, MatvecReq* mv = nullptr) {
  if (p.error) return mpse_fail(ctx, MPSE_ERR_SHAPE, "%s", p.error);
  TmpBuf t1(ctx), t2(ctx), t3(ctx);
  TmpBuf* tmp[3] = {&t1, &t2, &t3};
  PlanRun r(ctx, dtype, bufs_in, sc, mv);
  for (int i = 0; i < 3; ++i)
    if (p.tmp_elems[i]) {
      MPSE_TRY(tmp[i]->alloc(size_t(p.tmp_elems[i]) * r.es));
      r.bufs[B_T1 + i] = tmp[i]->p;
    }
  for (const Step& s : p.steps)
    MPSE_TRY(s.elementwise_w ? run_wsmall(r, s)
             : s.kind == K_WMIX ? run_wmix(r, s)
             : s.kind == K_GGEMM ? run_ggemm(r, s)
                                 : run_product(r, s));
  return MPSE_OK;
}

int heff_apply(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, void* out, SolveScope* sc,
               MatvecReq* mv) {
  if (!ctx || !h || !C || !out || !h->L || !h->R) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (dtype != MPSE_C128 && (h->l_dtype == MPSE_C128 || h->r_dtype == MPSE_C128 || h->w_dtype == MPSE_C128))
    return mpse_fail(ctx, MPSE_ERR_ARG, "heff_apply: real centre with complex operator parts");
  std::shared_ptr<void> wi_keep;     // (the map is also touched by mpse_free, possibly from another thread)
  if (h->nsite == 1 && h->W0) {
    std::lock_guard<std::mutex> lock(ctx->pool_mu);
    auto it = ctx->wsite_info.find(h->W0);
    if (it != ctx->wsite_info.end()) wi_keep = it->second.info;
  }
  {
    bool taken = false;
    MPSE_TRY(heff_small_try(ctx, dtype, h, C, out, sc, mv, &taken));
    if (taken) return MPSE_OK;     // (parts.used is set there: the result may be a sum of parts)
    const WSiteInfo* wi0 = static_cast<const WSiteInfo*>(wi_keep.get());
    const bool wi_ok = wi0 && h->nsite == 1 && wi0->wl == h->dims.wl && wi0->d == h->dims.d0 && wi0->wr == h->dims.wr;
    MPSE_TRY(heff0_fused_try(ctx, dtype, h, C, wi_ok ? wi0->w.data() : nullptr, sc, mv, &taken));
    if (taken) return MPSE_OK;     // (tile-masked parts: parts.used, parts.mask)
  }
  // a caller that takes the result in two parts (the Lanczos solve) lets the last product run as halved tiles; `used`
  // tells it whether the second part holds anything
  MatvecReq::Parts* pr = mv && mv->parts.ptr ? &mv->parts : nullptr;
  const bool two_ok = pr && pr->cap_elems >= 2 * pr->n;
  Plan p = plan_heff(dtype, *h, static_cast<const WSiteInfo*>(wi_keep.get()), two_ok, fold_epi());
  if (pr) pr->used = 0;
  const void* bufs[B_COUNT] = {nullptr};
  bind_heff(bufs, *h, C, out);
  // halved tiles: part 0 is `out` itself (it holds the beta term), part 1 the second slot of the caller's buffer;
  // split products: all parts in the caller's buffer (mpse_gemm.hip sets `used`)
  if (p.two_results) bufs[B_OUT2] = static_cast<char*>(pr->ptr) + size_t(pr->n) * dtype_size(dtype);
  MPSE_TRY(run_plan(ctx, dtype, p, bufs, sc, mv));
  if (p.two_results) pr->used = -2;     // (out, part 1)
  return MPSE_OK;
}

extern "C" int mpse_heff_apply(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, void* out) {
  return heff_apply(ctx, dtype, h, C, out, nullptr, nullptr);
}

extern "C" int mpse_mpo_site_hint(mpse_ctx* ctx, const void* W_dev, const double* W_host, int64_t wl, int64_t d,
                                  int64_t wr) {
  if (!ctx || !W_dev) return MPSE_ERR_ARG;
  if (!W_host) {
    std::lock_guard<std::mutex> lock(ctx->pool_mu);
    ctx->wsite_info.erase(W_dev);
    return MPSE_OK;
  }
  if (wl <= 0 || d <= 0 || wr <= 0) return mpse_fail(ctx, MPSE_ERR_SHAPE, "mpo_site_hint: empty MPO site");
  std::shared_ptr<void> info = std::make_shared<WSiteInfo>(analyse_mpo_site(W_host, wl, d, wr));
  std::lock_guard<std::mutex> lock(ctx->pool_mu);
  ctx->wsite_info[W_dev] = mpse_ctx::WSiteEntry{info, size_t(wl) * size_t(d) * size_t(d) * size_t(wr) * sizeof(double)};
  return MPSE_OK;
}

extern "C" int mpse_env_update(mpse_ctx* ctx, int dtype, int domain, const mpse_dims* dims, const void* env,
                               int env_dtype, const void* ket, const void* bra, int bra_conj, const void* W,
                               int w_dtype, void* out) {
  if (!ctx || !dims || !env || !ket || !W || !out) return MPSE_ERR_ARG;
  if (MPSE_RECORDING(ctx)) {
    const mpse_dims dc = *dims;
    ctx->defer_ops[ctx->defer_recording].push_back([=] {
      return mpse_env_update(ctx, dtype, domain, &dc, env, env_dtype, ket, bra, bra_conj, W, w_dtype, out);
    });
    return MPSE_OK;
  }
  MPSE_BIND(ctx);
  if (dtype != MPSE_C128 && (env_dtype == MPSE_C128 || w_dtype == MPSE_C128))
    return mpse_fail(ctx, MPSE_ERR_ARG, "env_update: real sites with complex env/mpo");
  if (!bra) {
    bra = ket;
    if (dims->Dl_bra != dims->Dl_ket || dims->Dr_bra != dims->Dr_ket)
      return mpse_fail(ctx, MPSE_ERR_SHAPE, "env_update: bra==NULL needs equal bonds");
  }
  std::shared_ptr<void> wi_keep;     // the site as the caller described it (mpse_mpo_site_hint): elementwise MPO step
  {
    static const bool fold_on = [] {
      const char* e = getenv("MPSE_ENV_WFOLD");
      return !(e && e[0] == '0');
    }();
    std::lock_guard<std::mutex> lock(ctx->pool_mu);
    auto it = ctx->wsite_info.find(W);
    if (fold_on && it != ctx->wsite_info.end()) wi_keep = it->second.info;
  }
  Plan p = plan_env(dtype, domain, *dims, env_dtype, w_dtype, bra_conj, static_cast<const WSiteInfo*>(wi_keep.get()));
  const void* bufs[B_COUNT] = {nullptr};
  bind_env(bufs, env, ket, bra, out, 1, &W);
  return run_plan(ctx, dtype, p, bufs);
}

extern "C" int mpse_env_update_multi(mpse_ctx* ctx, int dtype, int domain, const mpse_dims* dims, int n_mpo,
                                     const int64_t* wl, const int64_t* wr, const void* env, int env_dtype,
                                     const void* ket, const void* bra, int bra_conj, const void* const* W, int w_dtype,
                                     void* out) {
  if (!ctx || !dims || !env || !ket || !W || !wl || !wr || !out) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (n_mpo < 1 || n_mpo > 4) return mpse_fail(ctx, MPSE_ERR_ARG, "env_update_multi: 1 to 4 MPO layers, got %d", n_mpo);
  if (dtype != MPSE_C128 && (env_dtype == MPSE_C128 || w_dtype == MPSE_C128))
    return mpse_fail(ctx, MPSE_ERR_ARG, "env_update_multi: real sites with complex env/mpo");
  if (!bra) {
    bra = ket;
    if (dims->Dl_bra != dims->Dl_ket || dims->Dr_bra != dims->Dr_ket)
      return mpse_fail(ctx, MPSE_ERR_SHAPE, "env_update_multi: bra==NULL needs equal bonds");
  }
  Plan p = plan_env_multi(dtype, domain, *dims, n_mpo, wl, wr, env_dtype, w_dtype, bra_conj);
  for (int i = 0; i < n_mpo; ++i)
    if (!W[i]) return MPSE_ERR_ARG;
  const void* bufs[B_COUNT] = {nullptr};
  bind_env(bufs, env, ket, bra, out, n_mpo, W);
  return run_plan(ctx, dtype, p, bufs);
}

int heff_apply2(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, void* out, SolveScope* sc) {
  if (!ctx || !h || !C || !out || !h->L || !h->R || !h->W0) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (dtype != MPSE_C128 && (h->l_dtype == MPSE_C128 || h->r_dtype == MPSE_C128 || h->w_dtype == MPSE_C128))
    return mpse_fail(ctx, MPSE_ERR_ARG, "heff_apply2: real centre with complex operator parts");
  Plan p = plan_heff2(dtype, *h);
  const void* bufs[B_COUNT] = {nullptr};
  bind_heff(bufs, *h, C, out);
  return run_plan(ctx, dtype, p, bufs, sc);
}

extern "C" int mpse_heff_apply2(mpse_ctx* ctx, int dtype, const mpse_heff* h, const void* C, void* out) {
  return heff_apply2(ctx, dtype, h, C, out, nullptr);
}

// ---- two layers on a two-leg centre (finite-temperature correction vector): plans of mpse_plans.h
int heff_apply_ft(mpse_ctx* ctx, int dtype, const mpse_heff_ft* h, const void* C, void* out, SolveScope* sc) {
  if (!ctx || !h || !C || !out || !h->L || !h->R || !h->W1 || !h->W2) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (dtype != MPSE_C128 && (h->l_dtype == MPSE_C128 || h->r_dtype == MPSE_C128 || h->w_dtype == MPSE_C128))
    return mpse_fail(ctx, MPSE_ERR_ARG, "heff_apply_ft: real centre with complex operator parts");
  Plan p = plan_heff_ft(dtype, *h);
  const void* bufs[B_COUNT] = {nullptr};
  bind_heff_ft(bufs, *h, C, out);
  return run_plan(ctx, dtype, p, bufs, sc);
}

extern "C" int mpse_heff_apply_ft(mpse_ctx* ctx, int dtype, const mpse_heff_ft* h, const void* C, void* out) {
  return heff_apply_ft(ctx, dtype, h, C, out, nullptr);
}

extern "C" int mpse_env_update_ft(mpse_ctx* ctx, int dtype, int domain, const mpse_heff_ft* h, const void* env,
                                  int env_dtype, const void* X, void* out) {
  if (!ctx || !h || !env || !X || !out || !h->W1 || !h->W2) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (dtype != MPSE_C128 && (env_dtype == MPSE_C128 || h->w_dtype == MPSE_C128))
    return mpse_fail(ctx, MPSE_ERR_ARG, "env_update_ft: real site with complex env/mpo");
  Plan p = plan_env_ft(dtype, domain, *h, env_dtype);
  const void* const W[2] = {h->W1, h->W2};
  const void* bufs[B_COUNT] = {nullptr};
  bind_env(bufs, env, X, X, out, 2, W);
  return run_plan(ctx, dtype, p, bufs);
}

int ft_shape_ok(mpse_ctx* ctx, const mpse_heff_ft& h, const char* who) {
  if (h.Dl <= 0 || h.Dr <= 0 || h.d_up <= 0 || h.d_down <= 0 || h.wl1 <= 0 || h.wr1 <= 0 || h.wl2 <= 0 || h.wr2 <= 0)
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "%s: empty extent", who);
  if ((h.leg1 != MPSE_LEG_UP && h.leg1 != MPSE_LEG_DOWN) || (h.leg2 != MPSE_LEG_UP && h.leg2 != MPSE_LEG_DOWN) ||
      (h.leg1 == MPSE_LEG_DOWN && h.leg2 == MPSE_LEG_UP))
    return mpse_fail(ctx, MPSE_ERR_SHAPE, "%s: layers act up/up, down/down or up/down", who);
  return MPSE_OK;
}

// ---- preconditioner of the summed solve: the diagonal of each term from the environment diagonals and a per-site factor
namespace {

// element of an MPO site W (wl, d, d, wr) that takes leg value `in` to `out` under the layer's transposition flag
__device__ __forceinline__ double ft_w_elem(const double* W, int trans, long long d, long long wr, long long b, long long in,
                                            long long out, long long f) {
  return trans ? W[((b * d + in) * d + out) * wr + f] : W[((b * d + out) * d + in) * wr + f];
}

struct FtShape {
  long long Dl, Dr, du, dv, wl1, wr1, wl2, wr2;
  int leg1, leg2, trans1, trans2;
};

// S[b, c, u, v, g, i]: both layers on one leg: sum_x W1(leg -> x)[b, g] W2(x -> leg)[c, i]; one per leg: the two diagonals
__global__ __launch_bounds__(256) void k_site_factor_ft(const FtShape h, const double* __restrict__ W1,
                                                        const double* __restrict__ W2, double* __restrict__ S) {
  const long long total = h.wl1 * h.wl2 * h.du * h.dv * h.wr1 * h.wr2;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  long long r = idx;
  const long long i = r % h.wr2; r /= h.wr2;
  const long long g = r % h.wr1; r /= h.wr1;
  const long long v = r % h.dv; r /= h.dv;
  const long long u = r % h.du; r /= h.du;
  const long long c = r % h.wl2;
  const long long b = r / h.wl2;
  double acc = 0.0;
  if (h.leg1 == h.leg2) {
    const long long d = h.leg1 == MPSE_LEG_UP ? h.du : h.dv, e = h.leg1 == MPSE_LEG_UP ? u : v;
    for (long long x = 0; x < d; ++x)
      acc += ft_w_elem(W1, h.trans1, d, h.wr1, b, e, x, g) * ft_w_elem(W2, h.trans2, d, h.wr2, c, x, e, i);
  } else {
    acc = ft_w_elem(W1, h.trans1, h.du, h.wr1, b, u, u, g) * ft_w_elem(W2, h.trans2, h.dv, h.wr2, c, v, v, i);
  }
  S[idx] = acc;
}

// diag[a, u, v, j] (+)= weight * sum_{b, c, g, i} Re(L[a, b, c, a] R[j, g, i, j]) S[b, c, u, v, g, i]; one thread per entry
template <bool LC, bool RC>
__global__ __launch_bounds__(256) void k_diag_ft(const FtShape h, const double* __restrict__ L,
                                                 const double* __restrict__ R, const double* __restrict__ S, double weight,
                                                 double shift, int accumulate, double* __restrict__ diag) {
  const long long total = h.Dl * h.du * h.dv * h.Dr;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  long long r = idx;
  const long long j = r % h.Dr; r /= h.Dr;
  const long long v = r % h.dv; r /= h.dv;
  const long long u = r % h.du;
  const long long a = r / h.du;
  double acc = 0.0;
  for (long long b = 0; b < h.wl1; ++b)
    for (long long c = 0; c < h.wl2; ++c) {
      const long long lo = ((a * h.wl1 + b) * h.wl2 + c) * h.Dl + a;
      const double lr = LC ? L[2 * lo] : L[lo], li = LC ? L[2 * lo + 1] : 0.0;
      for (long long g = 0; g < h.wr1; ++g)
        for (long long i = 0; i < h.wr2; ++i) {
          const long long ro = ((j * h.wr1 + g) * h.wr2 + i) * h.Dr + j;
          const double rr = RC ? R[2 * ro] : R[ro], ri = RC ? R[2 * ro + 1] : 0.0;
          acc += (lr * rr - li * ri) * S[((((b * h.wl2 + c) * h.du + u) * h.dv + v) * h.wr1 + g) * h.wr2 + i];
        }
    }
  diag[idx] = (accumulate ? diag[idx] : shift) + weight * acc;
}

FtShape ft_shape(const mpse_heff_ft& h) {
  return FtShape{h.Dl, h.Dr, h.d_up, h.d_down, h.wl1, h.wr1, h.wl2, h.wr2, h.leg1, h.leg2, h.trans1, h.trans2};
}

}  // namespace

extern "C" int mpse_site_factor_ft(mpse_ctx* ctx, const mpse_heff_ft* h, void* S_f64) {
  if (!ctx) return MPSE_ERR_ARG;
  if (!h || !S_f64 || !h->W1 || !h->W2) return mpse_fail(ctx, MPSE_ERR_ARG, "site_factor_ft: null argument");
  MPSE_BIND(ctx);
  MPSE_TRY(ft_shape_ok(ctx, *h, "site_factor_ft"));
  if (h->w_dtype != MPSE_F64) return mpse_fail(ctx, MPSE_ERR_ARG, "site_factor_ft: real MPO sites only");
  const long long total = h->wl1 * h->wl2 * h->d_up * h->d_down * h->wr1 * h->wr2;
  hipLaunchKernelGGL(k_site_factor_ft, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, ft_shape(*h),
                     static_cast<const double*>(h->W1), static_cast<const double*>(h->W2), static_cast<double*>(S_f64));
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

extern "C" int mpse_diag_ft(mpse_ctx* ctx, const mpse_heff_ft* h, const void* S_f64, double weight, double shift,
                            int accumulate, void* diag_f64) {
  if (!ctx) return MPSE_ERR_ARG;
  if (!h || !S_f64 || !diag_f64 || !h->L || !h->R) return mpse_fail(ctx, MPSE_ERR_ARG, "diag_ft: null argument");
  MPSE_BIND(ctx);
  MPSE_TRY(ft_shape_ok(ctx, *h, "diag_ft"));
  const long long total = h->Dl * h->d_up * h->d_down * h->Dr;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const FtShape fs = ft_shape(*h);
  const double *L = static_cast<const double*>(h->L), *R = static_cast<const double*>(h->R);
  const double* S = static_cast<const double*>(S_f64);
  double* dg = static_cast<double*>(diag_f64);
  const bool lc = h->l_dtype == MPSE_C128, rc = h->r_dtype == MPSE_C128;
  if (lc && rc)
    hipLaunchKernelGGL((k_diag_ft<true, true>), grid, block, 0, ctx->stream, fs, L, R, S, weight, shift, accumulate, dg);
  else if (lc)
    hipLaunchKernelGGL((k_diag_ft<true, false>), grid, block, 0, ctx->stream, fs, L, R, S, weight, shift, accumulate, dg);
  else if (rc)
    hipLaunchKernelGGL((k_diag_ft<false, true>), grid, block, 0, ctx->stream, fs, L, R, S, weight, shift, accumulate, dg);
  else
    hipLaunchKernelGGL((k_diag_ft<false, false>), grid, block, 0, ctx->stream, fs, L, R, S, weight, shift, accumulate, dg);
  MPSE_HIP(ctx, hipGetLastError());
  if (!accumulate) ++ctx->pcg_sum_stats[mpse_ctx::PSS_DIAGS];
  return MPSE_OK;
}

extern "C" int mpse_env_unit_channel(mpse_ctx* ctx, int dtype, const void* env, int64_t D, int64_t w, double tol,
                                     int64_t* unit_host) {
  if (!ctx || !env || !unit_host) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  *unit_host = 0;
  if (D <= 0 || w <= 0 || w > 2048) return MPSE_OK;
  unsigned long long* dev = reinterpret_cast<unsigned long long*>(ctx->dscratch);
  MPSE_HIP(ctx, hipMemsetAsync(dev, 0, size_t(w) * sizeof(double), ctx->stream));
  if (dtype == MPSE_C128)
    hipLaunchKernelGGL((k_unit_deviation<true>), dim3((unsigned)D), dim3(256), 0, ctx->stream, (const double*)env, (int)D,
                       (int)w, dev);
  else
    hipLaunchKernelGGL((k_unit_deviation<false>), dim3((unsigned)D), dim3(256), 0, ctx->stream, (const double*)env,
                       (int)D, (int)w, dev);
  MPSE_HIP(ctx, hipGetLastError());
  if (w <= 1024) {
    MPSE_TRY(publish_and_wait(ctx, reinterpret_cast<const double*>(dev), (int)w, mpse_ctx::PIN_ENV_UNIT));
  } else {
    MPSE_HIP(ctx, hipMemcpyAsync(ctx->pinned + mpse_ctx::PIN_ENV_UNIT, dev, size_t(w) * sizeof(double), hipMemcpyDeviceToHost,
                                 ctx->stream));
    MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  for (int64_t b = 0; b < w; ++b)
    if (ctx->pinned[mpse_ctx::PIN_ENV_UNIT + b] <= tol) {
      *unit_host = b + 1;
      break;
    }
  return MPSE_OK;
}
