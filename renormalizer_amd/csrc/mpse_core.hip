// Context, pooled device memory and host<->device transfers of libmpsengine.so.
#include "mpse_internal.h"
#include "mpse_plans.h"

int mpse_fail(mpse_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

// 8-byte words: zero fill, and copy out of the mapped pinned staging ring.  Plain kernels queue like any other
// launch; the runtime's fill / copy operations leave 6-13 us of idle time behind them on the stream (rocprofv3 trace
// of the headline run: 640 of them per step).
__global__ __launch_bounds__(256) void k_zero8(unsigned long long* dst, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = 0ull;
}
__global__ __launch_bounds__(256) void k_copy8(unsigned long long* dst, const unsigned long long* __restrict__ src,
                                               long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_zero8x2(unsigned long long* a, long long na, unsigned long long* b, long long nb) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (long long)gridDim.x * 256) {
    if (i < na)
      a[i] = 0ull;
    else
      b[i - na] = 0ull;
  }
}

int device_zero2(mpse_ctx* ctx, void* a, size_t abytes, void* b, size_t bbytes) {
  if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | abytes | bbytes) & 7) != 0 || !abytes || !bbytes) {
    MPSE_TRY(device_zero(ctx, a, abytes));
    return device_zero(ctx, b, bbytes);
  }
  const long long na = (long long)(abytes / 8), nb = (long long)(bbytes / 8);
  long long blocks = (na + nb + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_zero8x2, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, static_cast<unsigned long long*>(a), na,
                     static_cast<unsigned long long*>(b), nb);
  MPSE_HIP(ctx, hipGetLastError());
  return MPSE_OK;
}

int device_zero(mpse_ctx* ctx, void* dst, size_t bytes) {
  if (!bytes) return MPSE_OK;
  if ((reinterpret_cast<uintptr_t>(dst) & 7) == 0 && (bytes & 7) == 0) {
    const long long n = (long long)(bytes / 8);
    long long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_zero8, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, static_cast<unsigned long long*>(dst), n);
    MPSE_HIP(ctx, hipGetLastError());
    return MPSE_OK;
  }
  MPSE_HIP(ctx, hipMemsetAsync(dst, 0, bytes, ctx->stream));
  return MPSE_OK;
}

int stage_h2d(mpse_ctx* ctx, void* dst, const void* src_host, size_t bytes) {
  if (!bytes) return MPSE_OK;
  if (!ctx->stage || bytes > ctx->stage_size / 4) return mpse_memcpy_h2d(ctx, dst, src_host, bytes);
  const size_t need = (bytes + 255) & ~size_t(255);
  if (ctx->stage_pos + need > ctx->stage_size) {
    // wrap: every copy enqueued so far must have consumed its slice
    MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stage_pos = 0;
  }
  char* slot = ctx->stage + ctx->stage_pos;
  memcpy(slot, src_host, bytes);
  if (ctx->stage_dev && (reinterpret_cast<uintptr_t>(dst) & 7) == 0 && (bytes & 7) == 0 && bytes <= (size_t(1) << 20)) {
    // the device reads the ring itself (mapped pinned memory), whole 8-byte words (index lists, descriptors)
    const size_t words = bytes / 8;
    ctx->stage_pos += need;
    __sync_synchronize();
    long long blocks = (long long)((words + 255) / 256);
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(k_copy8, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, static_cast<unsigned long long*>(dst),
                       reinterpret_cast<const unsigned long long*>(ctx->stage_dev + (slot - ctx->stage)),
                       (long long)words);
    MPSE_HIP(ctx, hipGetLastError());
    return MPSE_OK;
  }
  ctx->stage_pos += need;
  MPSE_HIP(ctx, hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
  return MPSE_OK;
}

void prof_drain(mpse_ctx* ctx) {
  for (auto& r : ctx->prof_pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
      ctx->prof_ms[r.variant] += ms;
      ctx->prof_flops[r.variant] += r.flops;
      ctx->prof_bytes[r.variant] += r.bytes;
      ctx->prof_launches[r.variant] += 1;
    }
    ctx->prof_free_events.push_back(r.e0);
    ctx->prof_free_events.push_back(r.e1);
  }
  ctx->prof_pending.clear();
}

bool prof_begin(mpse_ctx* ctx, int variant, double flops, double bytes, mpse_ctx::ProfRec* rec) {
  // (whole block-SVD calls, variant 6, last milliseconds and are few: every one of them is timed)
  if (!ctx->prof_on || (variant != 6 && ctx->prof_counter++ % ctx->prof_stride != 0)) return false;
  auto get_event = [&](hipEvent_t* e) {
    if (!ctx->prof_free_events.empty()) {
      *e = ctx->prof_free_events.back();
      ctx->prof_free_events.pop_back();
      return true;
    }
    return hipEventCreate(e) == hipSuccess;
  };
  if (!get_event(&rec->e0)) return false;
  if (!get_event(&rec->e1)) {
    ctx->prof_free_events.push_back(rec->e0);
    return false;
  }
  rec->variant = variant;
  rec->flops = flops;
  rec->bytes = bytes;
  if (hipEventRecord(rec->e0, ctx->stream) != hipSuccess) {
    ctx->prof_free_events.push_back(rec->e0);
    ctx->prof_free_events.push_back(rec->e1);
    return false;
  }
  return true;
}

void prof_end(mpse_ctx* ctx, const mpse_ctx::ProfRec& rec) {
  (void)hipEventRecord(rec.e1, ctx->stream);
  ctx->prof_pending.push_back(rec);
}

namespace {
__global__ void k_copy16(double2* __restrict__ dst, const double2* __restrict__ src, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}
}  // namespace

static void defer_update_hold(mpse_ctx* ctx) {
  const bool hold = ctx->defer_recording >= 0 || !ctx->defer_ops[0].empty() || !ctx->defer_ops[1].empty();
  std::lock_guard<std::mutex> lock(ctx->pool_mu);
  ctx->defer_hold = hold;
  if (hold) return;
  for (void* p : ctx->defer_frees) {
    auto it = ctx->live.find(p);
    if (it == ctx->live.end()) continue;
    ctx->free_blocks.emplace(it->second, p);
    ctx->in_use_bytes -= it->second;
    ctx->live.erase(it);
  }
  ctx->defer_frees.clear();
}

int defer_replay(mpse_ctx* ctx, int status) {
  const int list = ctx->defer_armed;
  if (list < 0) return status;
  ctx->defer_armed = -1;
  std::vector<std::function<int()>> ops;
  ops.swap(ctx->defer_ops[list]);
  if (status == MPSE_OK)
    for (auto& f : ops) {
      status = f();
      if (status != MPSE_OK) break;
    }
  ops.clear();
  defer_update_hold(ctx);
  return status;
}

// ---- plan store (mpse_internal.h) ---------------------------------------------------------------------------------

static bool plan_reuse_on() {
  static const bool on = [] {
    const char* e = getenv("MPSE_PLAN_REUSE");
    return !(e && e[0] == '0');
  }();
  return on;
}

int plan_words(mpse_ctx* ctx) {
  if (ctx->plan_words_dev) return MPSE_OK;
  void* p = nullptr;
  MPSE_TRY(mpse_malloc(ctx, 16, &p));
  ctx->plan_words_dev = static_cast<int*>(p);
  return device_zero(ctx, ctx->plan_words_dev, 16);
}

void SolveScope::borrow_slot(long long key) {
  if (slot || key == 0 || !plan_reuse_on()) return;
  ++ctx->plan_stats[mpse_ctx::PR_KEYED];
  mpse_ctx::PlanSlot* s = ctx->plan_store.find(key);
  if (!s) s = ctx->plan_store.insert(key);
  if (s->borrowed) return;
  s->borrowed = true;
  slot = s;
}

int plan_slot_buffer(mpse_ctx* ctx, mpse_ctx::PlanSlot* slot, size_t bytes, bool* ok) {
  *ok = false;
  if (slot->data.buf) {
    mpse_free(ctx, slot->data.buf);
    slot->data = mpse_ctx::PlanSlotData();
    ctx->plan_store.charge(slot, 0);
  }
  int ev = 0;
  const bool room = ctx->plan_store.make_room(bytes, slot, [ctx](mpse_ctx::PlanSlotData& d) {
    if (d.buf) mpse_free(ctx, d.buf);
  }, &ev);
  ctx->plan_stats[mpse_ctx::PR_EVICT] += ev;
  if (!room) return MPSE_OK;
  MPSE_TRY(plan_words(ctx));
  void* p = nullptr;
  MPSE_TRY(mpse_malloc(ctx, bytes, &p));
  slot->data.buf = p;
  ctx->plan_store.charge(slot, bytes);
  MPSE_TRY(device_zero(ctx, p, 16));
  *ok = true;
  return MPSE_OK;
}

extern "C" {

int mpse_solve_slot(mpse_ctx* ctx, int64_t key) {
  if (!ctx) return MPSE_ERR_ARG;
  ctx->slot_pending = key;
  return MPSE_OK;
}

int mpse_plan_store_budget(mpse_ctx* ctx, int64_t bytes) {
  if (!ctx || bytes < 0) return MPSE_ERR_ARG;
  ctx->plan_store.budget = (size_t)bytes;
  int ev = 0;     // slots beyond the new budget go now, least recently used first
  ctx->plan_store.make_room(0, nullptr, [ctx](mpse_ctx::PlanSlotData& d) {
    if (d.buf) mpse_free(ctx, d.buf);
  }, &ev);
  ctx->plan_stats[mpse_ctx::PR_EVICT] += ev;
  return MPSE_OK;
}

int mpse_plan_reuse_stats(mpse_ctx* ctx, int64_t* counts, int n) {
  if (!ctx || n < 0 || (n > 0 && !counts)) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  int v[4] = {0, 0, 0, 0};
  if (ctx->plan_words_dev) MPSE_TRY(mpse_memcpy_d2h(ctx, v, ctx->plan_words_dev, 16));
  for (int i = 0; i < n; ++i)
    counts[i] = i < mpse_ctx::PR_COUNT ? ctx->plan_stats[i] : i < mpse_ctx::PR_COUNT + 2 ? v[i - mpse_ctx::PR_COUNT] : 0;
  return MPSE_OK;
}

int mpse_prof_enable(mpse_ctx* ctx, int on) {
  if (!ctx) return MPSE_ERR_ARG;
  MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  prof_drain(ctx);
  ctx->prof_on = on != 0;
  ctx->prof_stride = on > 1 ? on : 1;
  ctx->prof_counter = 0;
  return MPSE_OK;
}

int mpse_prof_reset(mpse_ctx* ctx) {
  if (!ctx) return MPSE_ERR_ARG;
  MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  prof_drain(ctx);
  for (int i = 0; i < mpse_ctx::PROF_NVAR; ++i) {
    ctx->prof_ms[i] = ctx->prof_flops[i] = ctx->prof_bytes[i] = 0;
    ctx->prof_launches[i] = 0;
  }
  ctx->prof_svd_sweeps = 0;
  if (ctx->prof_ktiles) {
    MPSE_HIP(ctx, hipMemsetAsync(ctx->prof_ktiles, 0, 4 * sizeof(unsigned long long), ctx->stream));
    MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MPSE_OK;
}

int mpse_prof_get_ktiles(mpse_ctx* ctx, int variant, int64_t* ktiles) {
  if (!ctx || !ktiles || variant < 0 || variant > 3) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  *ktiles = 0;
  if (!ctx->prof_ktiles) return MPSE_OK;
  unsigned long long v[4];
  MPSE_HIP(ctx, hipMemcpyAsync(v, ctx->prof_ktiles, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
  MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *ktiles = (int64_t)v[variant];
  return MPSE_OK;
}

int mpse_prof_get_svd_sweeps(mpse_ctx* ctx, int64_t* sweeps) {
  if (!ctx || !sweeps) return MPSE_ERR_ARG;
  *sweeps = ctx->prof_svd_sweeps;
  return MPSE_OK;
}

int mpse_prof_get(mpse_ctx* ctx, int variant, double* total_ms, double* total_flops, double* total_bytes,
                  int64_t* launches) {
  if (!ctx || variant < 0 || variant >= mpse_ctx::PROF_NVAR) return MPSE_ERR_ARG;
  MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  prof_drain(ctx);
  if (variant == 0 && ctx->gemm_trace) {     // debug timeline of the contraction kernel (MPSE_GEMM_TRACE=<file>)
    const char* path = getenv("MPSE_GEMM_TRACE");
    unsigned long long n = 0;
    if (path && hipMemcpy(&n, ctx->gemm_trace, sizeof(n), hipMemcpyDeviceToHost) == hipSuccess) {
      if (n > GEMM_TRACE_CAP) n = GEMM_TRACE_CAP;
      std::vector<unsigned long long> rec(size_t(n) * GEMM_TRACE_WORDS);
      if (n && hipMemcpy(rec.data(), ctx->gemm_trace + 1, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
        if (FILE* fh = fopen(path, "wb")) {
          fwrite(rec.data(), sizeof(unsigned long long), rec.size(), fh);
          fclose(fh);
        }
      }
    }
  }
  if (total_ms) *total_ms = ctx->prof_ms[variant];
  if (total_flops) *total_flops = ctx->prof_flops[variant];
  if (total_bytes) *total_bytes = ctx->prof_bytes[variant];
  if (launches) *launches = ctx->prof_launches[variant];
  return MPSE_OK;
}

const char* mpse_version(void) { return "mpsengine 0.1 (gfx950)"; }

const char* mpse_last_error(const mpse_ctx* ctx) { return ctx ? ctx->err : "null context"; }

int mpse_ctx_create(int device, mpse_ctx** out) {
  if (!out) return MPSE_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MPSE_ERR_HIP;
  if (device < 0 || device >= ndev) return MPSE_ERR_ARG;
  mpse_ctx* ctx = new mpse_ctx();
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    delete ctx;
    return MPSE_ERR_HIP;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    ctx->n_cu = prop.multiProcessorCount;
    if (ctx->n_cu > 0) mpse_plan::fold_cus() = ctx->n_cu;
    snprintf(ctx->dev_name, sizeof(ctx->dev_name), "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipHostMalloc((void**)&ctx->pinned, mpse_ctx::PIN_DOUBLES * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&ctx->dscratch, (size_t(1) << 16) * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&ctx->prof_ktiles, 4 * sizeof(unsigned long long)) != hipSuccess ||
      hipHostMalloc((void**)&ctx->stage, size_t(8) << 20) != hipSuccess) {
    delete ctx;
    return MPSE_ERR_HIP;
  }
  // on the context's own stream: touching the null stream would make the runtime open one more hardware queue,
  // and with four trajectories per GPU (four streams) two of them would then share a queue and serialise
  (void)hipMemsetAsync(ctx->dscratch + (size_t(1) << 16) - 8, 0, 8 * sizeof(double), ctx->stream);
  (void)hipMemsetAsync(ctx->prof_ktiles, 0, 4 * sizeof(unsigned long long), ctx->stream);
  (void)hipStreamSynchronize(ctx->stream);
  // MPSE_PINNED_MAP=0: no mapped view of the pinned buffer - every read-back takes the copy path
  const char* pin_map = getenv("MPSE_PINNED_MAP");
  if ((pin_map && pin_map[0] == '0') || hipHostGetDevicePointer((void**)&ctx->pinned_dev, ctx->pinned, 0) != hipSuccess)
    ctx->pinned_dev = nullptr;
  {
    if (hipHostGetDevicePointer((void**)&ctx->stage_dev, ctx->stage, 0) != hipSuccess)
      ctx->stage_dev = nullptr;
    (void)hipGetLastError();
  }
  ctx->pinned[mpse_ctx::PIN_SEQ] = 0.0;
  ctx->stage_size = size_t(8) << 20;
  *out = ctx;
  return MPSE_OK;
}

static int pool_trim_locked(mpse_ctx* ctx) {
  MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (auto& kv : ctx->free_blocks) {
    (void)hipFree(kv.second);
    ctx->pool_bytes -= kv.first;
  }
  ctx->free_blocks.clear();
  return MPSE_OK;
}

int mpse_pool_trim(mpse_ctx* ctx) {
  if (!ctx) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  std::lock_guard<std::mutex> lock(ctx->pool_mu);
  return pool_trim_locked(ctx);
}

int mpse_ctx_destroy(mpse_ctx* ctx) {
  if (!ctx) return MPSE_ERR_ARG;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  prof_drain(ctx);
  ctx->plan_store.clear([ctx](mpse_ctx::PlanSlotData& d) {
    if (d.buf) mpse_free(ctx, d.buf);
  });
  for (auto e : ctx->prof_free_events) (void)hipEventDestroy(e);
  for (auto& kv : ctx->free_blocks) (void)hipFree(kv.second);
  for (auto& kv : ctx->live) (void)hipFree(kv.first);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->stage) (void)hipHostFree(ctx->stage);
  if (ctx->dscratch) (void)hipFree(ctx->dscratch);
  if (ctx->prof_ktiles) (void)hipFree(ctx->prof_ktiles);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return MPSE_OK;
}

int mpse_sync(mpse_ctx* ctx) {
  if (!ctx) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!ctx->prof_pending.empty()) prof_drain(ctx);
  return MPSE_OK;
}

int mpse_device_info(mpse_ctx* ctx, char* name, size_t name_len, int* n_cu, void** stream) {
  if (!ctx) return MPSE_ERR_ARG;
  if (name && name_len) snprintf(name, name_len, "%s", ctx->dev_name);
  if (n_cu) *n_cu = ctx->n_cu;
  if (stream) *stream = (void*)ctx->stream;
  return MPSE_OK;
}

static size_t bucket_of(size_t bytes) {
  // 256 B granularity below 1 MiB, then 1/8-octave size classes (<= 12.5 % slack)
  if (bytes < 256) return 256;
  if (bytes <= (size_t(1) << 20)) return (bytes + 255) & ~size_t(255);
  size_t p = size_t(1) << 20;
  while ((p << 1) <= bytes) p <<= 1;
  size_t step = p >> 3;
  return ((bytes + step - 1) / step) * step;
}

int mpse_malloc(mpse_ctx* ctx, size_t bytes, void** dptr) {
  if (!ctx || !dptr) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  std::lock_guard<std::mutex> lock(ctx->pool_mu);
  size_t b = bucket_of(bytes);
  auto it = ctx->free_blocks.find(b);
  void* p = nullptr;
  if (it != ctx->free_blocks.end()) {
    p = it->second;
    ctx->free_blocks.erase(it);
  } else {
    hipError_t e = hipMalloc(&p, b);
    ++ctx->n_device_allocs;
    if (e != hipSuccess) {
      // give cached blocks back to the driver and retry once
      (void)hipGetLastError();  // the failed call leaves a sticky error that later hipGetLastError() checks would see
      pool_trim_locked(ctx);
      e = hipMalloc(&p, b);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        *dptr = nullptr;
        return mpse_fail(ctx, MPSE_ERR_OOM, "hipMalloc(%zu) failed: %s (pool %zu B, in use %zu B)", b,
                         hipGetErrorString(e), ctx->pool_bytes, ctx->in_use_bytes);
      }
    }
    ctx->pool_bytes += b;
  }
  ctx->live[p] = b;
  ctx->in_use_bytes += b;
  *dptr = p;
  return MPSE_OK;
}

int mpse_free(mpse_ctx* ctx, void* dptr) {
  if (!ctx) return MPSE_ERR_ARG;
  if (!dptr) return MPSE_OK;
  std::lock_guard<std::mutex> lock(ctx->pool_mu);
  auto it = ctx->live.find(dptr);
  if (it == ctx->live.end()) return mpse_fail(ctx, MPSE_ERR_ARG, "mpse_free: unknown pointer %p", dptr);
  if (!ctx->wsite_info.empty()) ctx->wsite_info.erase(dptr);   // a described MPO site (mpse_mpo_site_hint) goes with its buffer
  if (ctx->defer_hold) {   // a recorded call may still read this block: released after the replay
    ctx->defer_frees.push_back(dptr);
    return MPSE_OK;
  }
  ctx->free_blocks.emplace(it->second, dptr);
  ctx->in_use_bytes -= it->second;
  ctx->live.erase(it);
  return MPSE_OK;
}

// ---- deferred calls ---------------------------------------------------------------------------------------------

int mpse_defer_begin(mpse_ctx* ctx, int list) {
  if (!ctx || list < 0 || list > 1) return MPSE_ERR_ARG;
  if (ctx->defer_recording >= 0) return mpse_fail(ctx, MPSE_ERR_ARG, "mpse_defer_begin: already recording");
  if (ctx->defer_armed == list) return mpse_fail(ctx, MPSE_ERR_ARG, "mpse_defer_begin: list %d is armed", list);
  ctx->defer_ops[list].clear();
  ctx->defer_recording = list;
  defer_update_hold(ctx);
  return MPSE_OK;
}

int mpse_defer_end(mpse_ctx* ctx) {
  if (!ctx) return MPSE_ERR_ARG;
  if (ctx->defer_recording < 0) return mpse_fail(ctx, MPSE_ERR_ARG, "mpse_defer_end: not recording");
  ctx->defer_recording = -1;
  defer_update_hold(ctx);
  return MPSE_OK;
}

int mpse_defer_arm(mpse_ctx* ctx, int list) {
  if (!ctx || list < 0 || list > 1) return MPSE_ERR_ARG;
  if (ctx->defer_recording >= 0) return mpse_fail(ctx, MPSE_ERR_ARG, "mpse_defer_arm: still recording");
  ctx->defer_armed = list;
  return MPSE_OK;
}

int mpse_defer_discard(mpse_ctx* ctx) {
  if (!ctx) return MPSE_ERR_ARG;
  ctx->defer_ops[0].clear();
  ctx->defer_ops[1].clear();
  ctx->defer_recording = ctx->defer_armed = -1;
  defer_update_hold(ctx);
  return MPSE_OK;
}

int mpse_defer_run(mpse_ctx* ctx, int list) {
  if (!ctx || list < 0 || list > 1) return MPSE_ERR_ARG;
  if (ctx->defer_recording >= 0) return mpse_fail(ctx, MPSE_ERR_ARG, "mpse_defer_run: still recording");
  MPSE_BIND(ctx);
  ctx->defer_armed = list;
  return defer_replay(ctx, MPSE_OK);
}


int mpse_mem_info(mpse_ctx* ctx, size_t* pool_bytes, size_t* in_use_bytes, size_t* device_free,
                  size_t* device_total) {
  if (!ctx) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (pool_bytes) *pool_bytes = ctx->pool_bytes;
  if (in_use_bytes) *in_use_bytes = ctx->in_use_bytes;
  size_t f = 0, t = 0;
  MPSE_HIP(ctx, hipMemGetInfo(&f, &t));
  if (device_free) *device_free = f;
  if (device_total) *device_total = t;
  return MPSE_OK;
}

int mpse_memcpy_h2d(mpse_ctx* ctx, void* dst, const void* src_host, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src_host))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (!bytes) return MPSE_OK;
  wsite_written(ctx, dst, bytes);
  MPSE_HIP(ctx, hipMemcpyAsync(dst, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MPSE_OK;
}

int mpse_memcpy_d2h(mpse_ctx* ctx, void* dst_host, const void* src, size_t bytes) {
  if (!ctx || (bytes && (!dst_host || !src))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (!bytes) return MPSE_OK;
  MPSE_HIP(ctx, hipMemcpyAsync(dst_host, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MPSE_OK;
}

int mpse_memcpy_d2d(mpse_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (!bytes) return MPSE_OK;
  wsite_written(ctx, dst, bytes);
  // tensors are 16-byte aligned multiples of 8 bytes: a plain grid-stride kernel queues like any other launch, while
  // the runtime's device-to-device copy leaves ~15 us of idle time behind it on the stream (rocprofv3 trace)
  if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0 && (bytes & 15) == 0) {
    const size_t n = bytes / 16;
    size_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_copy16, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, reinterpret_cast<double2*>(dst),
                       reinterpret_cast<const double2*>(src), (long long)n);
    MPSE_HIP(ctx, hipGetLastError());
    return MPSE_OK;
  }
  MPSE_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return MPSE_OK;
}

int mpse_memcpy_2d(mpse_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
                   size_t height) {
  if (!ctx || ((width_bytes && height) && (!dst || !src))) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  if (!width_bytes || !height) return MPSE_OK;
  wsite_written(ctx, dst, dpitch * (height - 1) + width_bytes);
  MPSE_HIP(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, height, hipMemcpyDeviceToDevice, ctx->stream));
  return MPSE_OK;
}

int mpse_memset_zero(mpse_ctx* ctx, void* dst, size_t bytes) {
  if (!ctx || (bytes && !dst)) return MPSE_ERR_ARG;
  MPSE_BIND(ctx);
  wsite_written(ctx, dst, bytes);
  return device_zero(ctx, dst, bytes);
}

}  // extern "C"

namespace {
__global__ void k_publish(const double* __restrict__ src, double* dst, int count, volatile double* seq_slot, double seq) {
  for (int i = threadIdx.x; i < count; i += blockDim.x) dst[i] = src[i];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    *seq_slot = seq;
    __threadfence_system();
  }
}
}  // namespace

int publish_wait_seq(mpse_ctx* ctx, double seq, const double* dsrc, int count, int slot) {
  volatile double* flag = ctx->pinned + mpse_ctx::PIN_SEQ;
  for (long long spins = 0; *flag != seq; ++spins) {
    if (spins > 2000000000LL || ((spins & 0xfffff) == 0xfffff && hipStreamQuery(ctx->stream) == hipSuccess && *flag != seq)) {
      // the kernel is gone but the number never arrived: fall back to the ordinary path (also surfaces errors)
      MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
      MPSE_HIP(ctx, hipMemcpy(ctx->pinned + slot, dsrc, size_t(count) * sizeof(double), hipMemcpyDeviceToHost));
      return MPSE_OK;
    }
  }
  __sync_synchronize();
  return MPSE_OK;
}

PublishAt publish_target(mpse_ctx* ctx, bool wait_here, int slot) {
  if (!wait_here || !ctx->pinned_dev) return PublishAt{nullptr, nullptr, 0.0};
  return PublishAt{ctx->pinned_dev + slot, ctx->pinned_dev + mpse_ctx::PIN_SEQ, double(++ctx->publish_seq)};
}

// the waiting half: the values are at ctx->pinned + slot when it returns
static int publish_wait(mpse_ctx* ctx, const PublishAt& at, const void* dsrc, size_t stride, int B, int W, int slot) {
  if (at.seq != 0.0) {
    MPSE_TRY(publish_wait_seq(ctx, at.seq, static_cast<const double*>(dsrc), W, slot));   // (rescues the first block itself)
    if (B == 1 || ctx->pinned[mpse_ctx::PIN_SEQ] == at.seq) return MPSE_OK;
  }
  // no mapped view, or the number never arrived: plain copies
  const size_t row = size_t(W) * sizeof(double);
  if (B == 1)
    MPSE_HIP(ctx, hipMemcpyAsync(ctx->pinned + slot, dsrc, row, hipMemcpyDeviceToHost, ctx->stream));
  else
    MPSE_HIP(ctx, hipMemcpy2DAsync(ctx->pinned + slot, row, dsrc, stride, row, size_t(B), hipMemcpyDeviceToHost, ctx->stream));
  MPSE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MPSE_OK;
}

int publish_collect(mpse_ctx* ctx, const PublishAt& at, const void* dsrc, size_t stride, int B, int W, int slot,
                    void* host_out) {
  MPSE_TRY(publish_wait(ctx, at, dsrc, stride, B, W, slot));
  if (ctx->prof_pending.size() > 2048) prof_drain(ctx);
  memcpy(host_out, ctx->pinned + slot, size_t(B) * W * sizeof(double));
  return MPSE_OK;
}

int publish_and_wait(mpse_ctx* ctx, const double* dsrc, int count, int slot) {
  if (count < 0 || count > 1024 || slot < 0 || slot + count > mpse_ctx::PIN_SLOTS_END)
    return mpse_fail(ctx, MPSE_ERR_ARG, "publish: range");
  const PublishAt at = publish_target(ctx, true, slot);
  if (at.pub) {
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, ctx->stream, dsrc, at.pub, count, at.seq_slot, at.seq);
    MPSE_HIP(ctx, hipGetLastError());
  }
  return publish_wait(ctx, at, dsrc, 0, 1, count, slot);
}
