// C ABI of libpyloo_amd.so (see include/pyloo_amd.h).  Host code only: argument checks,
// host<->device staging for PLA_HOST callers, kernel launches on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/pyloo_amd.h"
#include "pla_launch.h"
#include "pla_nonfactor.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define PLA_HIP(call)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(e_ == hipErrorOutOfMemory ? PLA_ERR_NOMEM : PLA_ERR_HIP, "%s: %s", #call, \
                  hipGetErrorString(e_));                                                 \
  } while (0)

int pow2_at_least(int64_t n) {
  int p = 8;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace

struct pla_engine {
  int device = 0;
  // One engine = one workspace: every entry point that takes an engine holds this lock for the whole call, so
  // concurrent callers (ctypes releases the GIL) are serialised instead of racing on the buffers below.
  std::mutex mu;
  // frozen: the workspace may be referenced by a captured HIP graph; a call that would have to reallocate any of
  // it returns PLA_ERR_FROZEN instead (pla_engine_set_frozen)
  bool frozen = false;
  unsigned long long* counters = nullptr;  // [pla::kCountersTotal] device (layout: pla_launch.h): [0..15] per call, [16..] engine statistics
  double* d_red = nullptr;                 // reduction partials
  // staging for PLA_HOST callers (grown on demand)
  void* d_in = nullptr;
  size_t d_in_bytes = 0;
  void* d_lw = nullptr;
  size_t d_lw_bytes = 0;
  double* d_pw = nullptr;  // 3 * n doubles + agg
  size_t d_pw_elems = 0;
  void* d_slow = nullptr;  // [n] row list of the fast path
  size_t d_slow_bytes = 0;
  // quantile tables log1p(-(j+0.5)/M), one immutable device buffer per tail count M seen so far (never rewritten
  // or freed before the engine is destroyed: enqueued launches and captured graphs keep valid pointers)
  struct L1Table { int64_t M; double* d; };
  std::vector<L1Table> l1_tables;
  void* d_ws = nullptr;    // hand-over buffers of the split LOO pass: [n][stride] tail values + [n][8] scalars
  size_t d_ws_bytes = 0;
  void* d_col = nullptr;   // observations-fastest LOO (pla_col.h): candidate lists + scalars of one block of observations
  size_t d_col_bytes = 0;
  void* d_probs = nullptr;  // quantile levels of pla_e_loo_quantiles
  size_t d_probs_bytes = 0;
  void* d_rows = nullptr;  // clamped copy of a caller's device row-index list
  void* d_slab = nullptr;  // host path, observations-fastest input: (n_draws, block of observations) slab before the transpose
  void* d_grp = nullptr;   // group sums of one block of groups (pla_psis_loo_groups; pla_group_sum from the host)
  size_t d_grp_bytes = 0;
  void* d_gidx = nullptr;  // host path of the group calls: [0] replaced-entry counter, then the uploaded offsets and members
  size_t d_gidx_bytes = 0;
  size_t d_slab_bytes = 0;
  size_t d_rows_bytes = 0;
  void* d_cmp = nullptr;  // model comparison: per-tile partials (pla_compare.h)
  size_t d_cmp_bytes = 0;
  void* d_cmp_out = nullptr;  // ... and the outputs of host calls / of the stacking evaluation
  size_t d_cmp_out_bytes = 0;
  int compare_grid = 0;  // pla_engine_set_compare_grid: workgroup cap of the comparison passes (0: the library's choice)
  void* d_nf = nullptr;  // non-factorised LOO: slots of the blocked / general routes (pla_nonfactor.h)
  size_t d_nf_bytes = 0;
  void* d_nf_in = nullptr;  // ... staging of a host call: one block of draws (mu, matrices, df) and y
  size_t d_nf_in_bytes = 0;
  void* d_nf_out = nullptr;  // ... and its outputs (ll block, flags)
  size_t d_nf_out_bytes = 0;
  void* d_kf = nullptr;  // k-fold: the source table of the last pla_kfold_lme call ...
  size_t d_kf_bytes = 0;
  // ... its pinned host copy (the upload reads it after the call has returned), two of them used in turn, and the event behind
  // each upload: a call waits for the upload of the call before the previous one before it rewrites that copy
  void* h_kf[2] = {nullptr, nullptr};
  size_t h_kf_bytes[2] = {0, 0};
  hipEvent_t kf_event[2] = {nullptr, nullptr};
  int kf_turn = 0;
  void* d_mm = nullptr;  // moment matching: per-tile partials of pla_mm_moments (pla_mm.h)
  size_t d_mm_bytes = 0;
  void* d_mix = nullptr;  // Mix-IS-LOO (pla_mixis.h): the slab of pass 1, c, the unscaled pointwise values, the finishing pass's partials
  size_t d_mix_bytes = 0;
  int mixis_grid = 0;  // pla_engine_set_mixis_grid (0: the library's choice)
  void* d_pit = nullptr;  // LOO-PIT (pla_pit.h): one block of predictive draws, draws fastest (transposed or staged from the host)
  size_t d_pit_bytes = 0;
  void* d_lfo = nullptr;  // leave-future-out CV (pla_lfo.h): the carry into a block of steps [n_draws], then the carries of its chunks
  size_t d_lfo_bytes = 0;
  void* d_ess = nullptr;  // relative efficiency (pla_ess.h): a slot of centred draws per workgroup of the long-row route
  size_t d_ess_bytes = 0;
  int ess_grid = 0;  // pla_engine_set_ess_grid (0: the library's choice)
  std::string kf_label;  // the routes of the last pla_kfold_lme, for the text pla_kfold_reduce leaves in last_kernels
  int nonfactor_route = 0;  // pla_engine_set_nonfactor_route
  int nonfactor_grid = 0;   // pla_engine_set_nonfactor_grid (0: the library's choice)
  // timing of the main kernel
  bool timing = false;
  static constexpr int kTimingRing = 64;  // launches timed without a host-side wait in between
  hipEvent_t ev0[kTimingRing] = {}, ev1[kTimingRing] = {}, evm[kTimingRing] = {};  // evm: after the first kernel of a split pass
  bool has_mid[kTimingRing] = {};
  double acc_ms = 0.0;
  double acc_first_ms = 0.0;  // first (dominant) kernel of split passes only
  long long first_launches = 0;
  int64_t launches = 0;
  int pending = 0;  // event pairs recorded and not yet read back
  // streamed split pass (psis_loo_impl, pla_kernels.hip launch_wave): two internal streams forked from / joined to the
  // caller's stream -- the wave kernel on one, the fit kernel beside it on the other -- and the flags between them
  hipStream_t pipe_first = nullptr, pipe_second = nullptr;
  hipEvent_t pipe_fork = nullptr, pipe_join1 = nullptr, pipe_join2 = nullptr;
  void* d_sync = nullptr;
  size_t d_sync_bytes = 0;
  // timing of the first kernel alone (bench roofline: average duration of one launch of the dominant kernel)
  static constexpr int kPipeTimed = 64;
  hipEvent_t pipe_t0[kPipeTimed] = {}, pipe_t1[kPipeTimed] = {};
  int pipe_timed = 0;
  std::string last_kernels;  // pla_engine_last_kernels
  // ordering of the calls ACROSS streams: every call that enqueues work on the workspace records `order_event` behind it, and a
  // call on another stream makes that stream wait for it first (EngineCall)
  hipEvent_t order_event = nullptr;
  hipStream_t order_stream = nullptr;
  bool order_valid = false;
};

namespace {

thread_local bool g_frozen = false;  // set from the engine at the start of every entry point (EngineCall)

int grow(void** p, size_t* have, size_t want) {
  if (*have >= want) return PLA_OK;
  if (g_frozen)
    return fail(PLA_ERR_FROZEN, "the engine workspace is frozen (pla_engine_set_frozen) and this call needs %zu more bytes of it",
                want - *have);
  // hipFree waits for the device: launches already enqueued on any stream have finished with the old buffer
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  hipError_t e = hipMalloc(p, want);
  if (e != hipSuccess) return fail(PLA_ERR_NOMEM, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
  *have = want;
  return PLA_OK;
}

int check_common(pla_engine* eng, const void* in, int dtype, int64_t n_obs, int64_t n_draws,
                 int64_t stride_obs, int64_t stride_draw, int method, int64_t tail_count, int mem_space) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (method != PLA_PSIS && method != PLA_SIS && method != PLA_TIS) return fail(PLA_ERR_ARG, "bad method");
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (n_obs > 0 && !in) return fail(PLA_ERR_ARG, "input pointer is NULL");
  if (n_draws < 1 || n_draws > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_draws out of range");
  if (stride_draw == 0 || stride_obs < 0 || stride_draw < 0) return fail(PLA_ERR_ARG, "bad strides");
  if (method == PLA_PSIS) {
    // x_sorted[-M-1] must exist (numpy raises IndexError otherwise: psis.py:136)
    if (tail_count < 1 || tail_count + 1 > n_draws)
      return fail(PLA_ERR_ARG, "tail_count %lld needs at least %lld draws, got %lld", (long long)tail_count,
                  (long long)tail_count + 1, (long long)n_draws);
    if (tail_count > pla::max_tail_count())
      return fail(PLA_ERR_UNSUPPORTED, "tail_count %lld exceeds the LDS tail capacity %d", (long long)tail_count,
                  pla::max_tail_count());
  }
  return PLA_OK;
}

// Row-independent tables of the fast path, computed with the host libm exactly as NumPy does:
//   [0, M)      log1p(-(j + 0.5)/M)              psis.py:153 through log1p of psis.py:219/221
//   [M, M+64)   1 - sqrt(m_est / (j + 0.5))      psis.py:186 for m_est = 30 + isqrt(M)
int ensure_l1_table(pla_engine* e, int64_t M, hipStream_t s, const double** out) {
  for (const auto& t : e->l1_tables)
    if (t.M == M) {
      *out = t.d;
      return PLA_OK;
    }
  if (g_frozen) return fail(PLA_ERR_FROZEN, "the engine is frozen and has no quantile table for tail_count %lld", (long long)M);
  double* d = nullptr;
  hipError_t he = hipMalloc((void**)&d, (size_t)(M + 64) * sizeof(double));
  if (he != hipSuccess) return fail(PLA_ERR_NOMEM, "hipMalloc(table): %s", hipGetErrorString(he));
  std::vector<double> h((size_t)M + 64);
  for (int64_t j = 0; j < M; ++j) h[(size_t)j] = std::log1p(-(((double)j + 0.5) / (double)M));
  int64_t root = (int64_t)std::sqrt((double)M);
  while (root * root > M) --root;
  while ((root + 1) * (root + 1) <= M) ++root;
  const double mest = (double)(30 + root);
  for (int j = 0; j < 64; ++j) h[(size_t)M + j] = 1.0 - std::sqrt(mest / ((double)(j + 1) - 0.5));
  he = hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);  // h goes out of scope
  if (he != hipSuccess) {
    (void)hipFree(d);
    return fail(PLA_ERR_HIP, "table upload: %s", hipGetErrorString(he));
  }
  e->l1_tables.push_back({M, d});
  *out = d;
  return PLA_OK;
}

// every entry point: serialise on the engine and publish its frozen flag to grow().  With a stream: the call enqueues work that
// uses the engine's workspace -- it is ordered behind the previous such call when that one went to ANOTHER stream (one event
// per engine, recorded at the end of every call; nothing inside a stream capture, whose order is the caller's)
struct EngineCall {
  std::lock_guard<std::mutex> lock;
  pla_engine* e;
  hipStream_t s;
  bool ordered;
  explicit EngineCall(pla_engine* e_) : lock(e_->mu), e(e_), s(nullptr), ordered(false) { g_frozen = e->frozen; }
  EngineCall(pla_engine* e_, hipStream_t s_) : lock(e_->mu), e(e_), s(s_), ordered(false) {
    g_frozen = e->frozen;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipSetDevice(e->device) != hipSuccess || !e->order_event) return;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      return;
    }
    ordered = true;
    if (e->order_valid && e->order_stream != s) (void)hipStreamWaitEvent(s, e->order_event, 0);
  }
  ~EngineCall() {
    if (ordered && hipEventRecord(e->order_event, s) == hipSuccess) {
      e->order_stream = s;
      e->order_valid = true;
    }
    g_frozen = false;
  }
};

struct TimedLaunch {  // brackets the main kernel with events when timing is on
  pla_engine* e;
  hipStream_t s;
  TimedLaunch(pla_engine* e_, hipStream_t s_) : e(e_), s(s_) {
    if (e->timing) {
      if (e->pending == pla_engine::kTimingRing) flush(e);  // the only case in which the host waits
      e->has_mid[e->pending] = false;  // (a reused ring slot must not inherit the mid event of an earlier split pass)
      (void)hipEventRecord(e->ev0[e->pending], s);
    }
  }
  hipEvent_t mid() const { return e->timing ? e->evm[e->pending] : nullptr; }
  bool* mid_flag() const {
    if (!e->timing) return nullptr;
    e->has_mid[e->pending] = false;
    return &e->has_mid[e->pending];
  }
  ~TimedLaunch() {
    if (e->timing) {
      (void)hipEventRecord(e->ev1[e->pending], s);
      e->pending += 1;
    }
  }
  static void flush(pla_engine* e) {
    for (int i = 0; i < e->pending; ++i) {
      float ms = 0.f;
      if (hipEventSynchronize(e->ev1[i]) == hipSuccess && hipEventElapsedTime(&ms, e->ev0[i], e->ev1[i]) == hipSuccess) {
        e->acc_ms += ms;
        e->launches += 1;
        if (e->has_mid[i] && hipEventElapsedTime(&ms, e->ev0[i], e->evm[i]) == hipSuccess) {
          e->acc_first_ms += ms;
          e->first_launches += 1;
        }
      }
    }
    e->pending = 0;
    for (int i = 0; i < e->pipe_timed; ++i) {
      float ms = 0.f;
      if (hipEventSynchronize(e->pipe_t1[i]) == hipSuccess && hipEventElapsedTime(&ms, e->pipe_t0[i], e->pipe_t1[i]) == hipSuccess) {
        e->acc_first_ms += ms;
        e->first_launches += 1;
      }
    }
    e->pipe_timed = 0;
  }
};

// streams and events of the streamed pass, created on first use
int ensure_pipe(pla_engine* e) {
  if (e->pipe_first) return PLA_OK;
  if (g_frozen) return fail(PLA_ERR_FROZEN, "the engine is frozen and has no internal streams yet");
  hipError_t he = hipStreamCreateWithFlags(&e->pipe_first, hipStreamNonBlocking);
  if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->pipe_second, hipStreamNonBlocking);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&e->pipe_fork, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&e->pipe_join1, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&e->pipe_join2, hipEventDisableTiming);
  for (int i = 0; i < pla_engine::kPipeTimed && he == hipSuccess; ++i) {
    he = hipEventCreate(&e->pipe_t0[i]);
    if (he == hipSuccess) he = hipEventCreate(&e->pipe_t1[i]);
  }
  if (he != hipSuccess) return fail(PLA_ERR_HIP, "internal streams / events: %s", hipGetErrorString(he));
  return PLA_OK;
}

}  // namespace

extern "C" {

int pla_abi_version(void) { return PLA_ABI_VERSION; }

const char* pla_last_error(void) { return g_err; }

int pla_device_count(int* count) {
  if (!count) return fail(PLA_ERR_ARG, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(PLA_ERR_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return PLA_OK;
}

int pla_engine_create(int device, pla_engine** out) {
  if (!out) return fail(PLA_ERR_ARG, "out is NULL");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(PLA_ERR_NODEVICE, "no HIP device available");
  if (device < 0 || device >= n) return fail(PLA_ERR_ARG, "device %d out of range (0..%d)", device, n - 1);
  PLA_HIP(hipSetDevice(device));
  pla_engine* e = new (std::nothrow) pla_engine();
  if (!e) return fail(PLA_ERR_NOMEM, "out of host memory");
  e->device = device;
  hipError_t he = hipMalloc((void**)&e->counters, pla::kCountersTotal * sizeof(unsigned long long));
  if (he == hipSuccess) he = hipMalloc((void**)&e->d_red, (size_t)pla::reduce_workspace_doubles() * sizeof(double));
  if (he == hipSuccess) he = hipMemset(e->counters, 0, pla::kCountersTotal * sizeof(unsigned long long));
  if (he == hipSuccess) he = hipMemset(e->d_red, 0, (size_t)pla::reduce_workspace_doubles() * sizeof(double));  // (the ticket of reduce_fused)
  if (he == hipSuccess) he = hipEventCreateWithFlags(&e->order_event, hipEventDisableTiming);
  for (int i = 0; i < pla_engine::kTimingRing && he == hipSuccess; ++i) {
    he = hipEventCreate(&e->ev0[i]);
    if (he == hipSuccess) he = hipEventCreate(&e->ev1[i]);
    if (he == hipSuccess) he = hipEventCreate(&e->evm[i]);
  }
  if (he != hipSuccess) {
    pla_engine_destroy(e);
    return fail(PLA_ERR_HIP, "engine setup: %s", hipGetErrorString(he));
  }
  *out = e;
  return PLA_OK;
}

int pla_engine_destroy(pla_engine* e) {
  if (!e) return PLA_OK;
  (void)hipSetDevice(e->device);
  if (e->counters) (void)hipFree(e->counters);
  if (e->d_red) (void)hipFree(e->d_red);
  if (e->d_in) (void)hipFree(e->d_in);
  if (e->d_lw) (void)hipFree(e->d_lw);
  if (e->d_pw) (void)hipFree(e->d_pw);
  if (e->d_slow) (void)hipFree(e->d_slow);
  for (auto& t : e->l1_tables) (void)hipFree(t.d);
  if (e->d_ws) (void)hipFree(e->d_ws);
  if (e->d_rows) (void)hipFree(e->d_rows);
  if (e->d_col) (void)hipFree(e->d_col);
  if (e->d_probs) (void)hipFree(e->d_probs);
  if (e->d_slab) (void)hipFree(e->d_slab);
  if (e->d_grp) (void)hipFree(e->d_grp);
  if (e->d_gidx) (void)hipFree(e->d_gidx);
  if (e->d_cmp) (void)hipFree(e->d_cmp);
  if (e->d_cmp_out) (void)hipFree(e->d_cmp_out);
  if (e->d_nf) (void)hipFree(e->d_nf);
  if (e->d_nf_in) (void)hipFree(e->d_nf_in);
  if (e->d_nf_out) (void)hipFree(e->d_nf_out);
  if (e->d_kf) (void)hipFree(e->d_kf);
  if (e->d_mm) (void)hipFree(e->d_mm);
  if (e->d_mix) (void)hipFree(e->d_mix);
  if (e->d_pit) (void)hipFree(e->d_pit);
  if (e->d_lfo) (void)hipFree(e->d_lfo);
  if (e->d_ess) (void)hipFree(e->d_ess);
  for (int i = 0; i < 2; ++i) {
    if (e->h_kf[i]) (void)hipHostFree(e->h_kf[i]);
    if (e->kf_event[i]) (void)hipEventDestroy(e->kf_event[i]);
  }
  for (int i = 0; i < pla_engine::kTimingRing; ++i) {
    if (e->ev0[i]) (void)hipEventDestroy(e->ev0[i]);
    if (e->ev1[i]) (void)hipEventDestroy(e->ev1[i]);
    if (e->evm[i]) (void)hipEventDestroy(e->evm[i]);
  }
  if (e->order_event) (void)hipEventDestroy(e->order_event);
  if (e->pipe_first) (void)hipStreamDestroy(e->pipe_first);
  if (e->pipe_second) (void)hipStreamDestroy(e->pipe_second);
  if (e->d_sync) (void)hipFree(e->d_sync);
  for (hipEvent_t ev : {e->pipe_fork, e->pipe_join1, e->pipe_join2})
    if (ev) (void)hipEventDestroy(ev);
  for (int i = 0; i < pla_engine::kPipeTimed; ++i) {
    if (e->pipe_t0[i]) (void)hipEventDestroy(e->pipe_t0[i]);
    if (e->pipe_t1[i]) (void)hipEventDestroy(e->pipe_t1[i]);
  }
  delete e;
  return PLA_OK;
}

int pla_tail_count(int64_t n_draws, double reff, int64_t* tail_count) {
  if (!tail_count) return fail(PLA_ERR_ARG, "tail_count is NULL");
  if (n_draws < 1 || !(reff > 0.0)) return fail(PLA_ERR_ARG, "need n_draws >= 1 and reff > 0");
  const double a = (double)n_draws / 5.0;
  const double b = 3.0 * std::sqrt((double)n_draws / reff);  // base.py:139-141
  *tail_count = (int64_t)std::ceil(a < b ? a : b);
  return PLA_OK;
}

int pla_engine_set_frozen(pla_engine* e, int frozen) {
  if (!e) return fail(PLA_ERR_ARG, "engine is NULL");
  EngineCall call(e);
  e->frozen = frozen != 0;
  return PLA_OK;
}

int pla_engine_set_timing(pla_engine* e, int enable) {
  if (!e) return fail(PLA_ERR_ARG, "engine is NULL");
  EngineCall call(e);
  TimedLaunch::flush(e);
  e->timing = enable != 0;
  return PLA_OK;
}

int pla_engine_kernel_ms(pla_engine* e, double* total_ms, int64_t* launches) {
  if (!e) return fail(PLA_ERR_ARG, "engine is NULL");
  EngineCall call(e);
  TimedLaunch::flush(e);
  if (total_ms) *total_ms = e->acc_ms;
  if (launches) *launches = e->launches;
  e->acc_ms = 0.0;
  e->launches = 0;
  return PLA_OK;
}

int pla_engine_first_kernel_ms(pla_engine* e, double* total_ms, int64_t* launches) {
  if (!e) return fail(PLA_ERR_ARG, "engine is NULL");
  EngineCall call(e);
  TimedLaunch::flush(e);
  if (total_ms) *total_ms = e->acc_first_ms;
  if (launches) *launches = e->first_launches;
  e->acc_first_ms = 0.0;
  e->first_launches = 0;
  return PLA_OK;
}

int pla_engine_last_kernels(pla_engine* eng, char* buf, int cap) {
  if (!eng || !buf || cap < 1) return fail(PLA_ERR_ARG, "engine / buffer is NULL");
  EngineCall call(eng);
  snprintf(buf, (size_t)cap, "%s", eng->last_kernels.c_str());
  return PLA_OK;
}

int pla_env_overrides(char* buf, int cap) {
  if (!buf || cap < 1) return fail(PLA_ERR_ARG, "buffer is NULL");
  static const char* const kAlways[] = {"PLA_PIPE", "PLA_STREAM_PATIENCE_US", "PLA_FORCE_PATH", "PLA_INGEST_TRANSPOSE", "PLA_INGEST_BLOCK_MB"};
  static const char* const kExperiment[] = {"PLA_DEBUG_SKIP", "PLA_FUSED", "PLA_SKIP_FIT", "PLA_NO_THRESHOLD_CHECK", "PLA_NO_RETRY", "PLA_NO_TILE",
                                            "PLA_TILE_GRID", "PLA_FIT_GRID", "PLA_FIT_HELPERS", "PLA_WAVE_PRIO", "PLA_COL_BLOCK",
                                            "PLA_PRINT_REASONS", "PLA_PRINT_CLOCK"};
  std::string out = pla::kExperiment ? "EXPERIMENT-BUILD" : "";
  const auto add = [&](const char* name) {
    const char* v = getenv(name);
    if (!v) return;
    if (!out.empty()) out += " ";
    out += name;
    out += "=";
    out += v;
  };
  for (const char* n : kAlways) add(n);
  if (pla::kExperiment)
    for (const char* n : kExperiment) add(n);
  snprintf(buf, (size_t)cap, "%s", out.c_str());
  return PLA_OK;
}

int pla_engine_stream_stats(pla_engine* eng, int64_t* gave_up) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  EngineCall call(eng);
  PLA_HIP(hipSetDevice(eng->device));
  PLA_HIP(hipDeviceSynchronize());
  unsigned long long h = 0;
  PLA_HIP(hipMemcpy(&h, eng->counters + pla::kCounterGaveUp, sizeof(h), hipMemcpyDeviceToHost));
  PLA_HIP(hipMemset(eng->counters + pla::kCounterGaveUp, 0, sizeof(h)));
  if (gave_up) *gave_up = (int64_t)h;
  return PLA_OK;
}

int pla_aggregate_pack(pla_engine* eng, const double* agg, int rank, int world, double* table, void* stream) {
  if (!eng || !agg || !table) return fail(PLA_ERR_ARG, "engine / agg / table is NULL");
  if (world < 1 || rank < 0 || rank >= world) return fail(PLA_ERR_ARG, "need 0 <= rank < world");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  PLA_HIP(pla::launch_aggregate_pack(agg, rank, world, table, (hipStream_t)stream));
  return PLA_OK;
}

int pla_aggregate_merge(pla_engine* eng, const double* table, int world, double* out, void* stream) {
  if (!eng || !table || !out) return fail(PLA_ERR_ARG, "engine / table / out is NULL");
  if (world < 1) return fail(PLA_ERR_ARG, "world < 1");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  PLA_HIP(pla::launch_aggregate_merge(table, world, out, (hipStream_t)stream));
  return PLA_OK;
}

int pla_reduce_pointwise(pla_engine* eng, const double* diag, const double* loo_i, const double* lppd_i,
                         int64_t n_obs, double good_k, int mem_space, void* stream, double* agg) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (!agg) return fail(PLA_ERR_ARG, "agg is NULL");
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  if (mem_space == PLA_DEVICE) {
    pla::ReduceParams rp{diag, loo_i, lppd_i, n_obs, good_k, agg, nullptr};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
    return PLA_OK;
  }
  const size_t need = (size_t)(3 * n_obs + PLA_AGG_COUNT);
  size_t have_b = eng->d_pw_elems * sizeof(double);
  int rc = grow((void**)&eng->d_pw, &have_b, need * sizeof(double));
  eng->d_pw_elems = have_b / sizeof(double);
  if (rc) return rc;
  double* d = eng->d_pw;
  double *dd = nullptr, *dl = nullptr, *dp = nullptr;
  if (diag) { dd = d; PLA_HIP(hipMemcpyAsync(dd, diag, n_obs * sizeof(double), hipMemcpyHostToDevice, s)); }
  if (loo_i) { dl = d + n_obs; PLA_HIP(hipMemcpyAsync(dl, loo_i, n_obs * sizeof(double), hipMemcpyHostToDevice, s)); }
  if (lppd_i) { dp = d + 2 * n_obs; PLA_HIP(hipMemcpyAsync(dp, lppd_i, n_obs * sizeof(double), hipMemcpyHostToDevice, s)); }
  double* dagg = d + 3 * n_obs;
  pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, dagg, nullptr};
  PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
  PLA_HIP(hipMemcpyAsync(agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  return PLA_OK;
}

// Device matrices with the observations fastest (ArviZ's native layout behind pyloo's stacked view, loo.py:189) are brought
// to draws-fastest row blocks by a tiled transpose kernel and then take the same kernels as everything else.
static bool obs_fastest_device(int mem_space, const int64_t* row_index, int64_t n_src, int64_t n_draws, int64_t stride_obs,
                               int64_t stride_draw) {
  return mem_space == PLA_DEVICE && !row_index && n_src > 1 && n_draws > 1 && stride_obs == 1 && stride_draw >= n_src;
}
// rows per staging block: 1 GiB blocks from the host (pinned-copy granularity), 4 GiB for the device transpose
static int64_t staged_chunk_rows(int mem_space, bool ingest, int64_t n_obs, int64_t n_draws, size_t esz) {
  static const size_t ingest_bytes = [] {  // PLA_INGEST_BLOCK_MB: block size of the transposing ingestion (tuning knob)
    const char* e = getenv("PLA_INGEST_BLOCK_MB");
    const long mb = e ? atol(e) : 0;
    return mb > 0 ? (size_t)mb << 20 : (size_t)1 << 32;
  }();
  const size_t bytes = (mem_space == PLA_DEVICE && ingest) ? ingest_bytes : (size_t)1 << 30;
  int64_t r = (int64_t)(bytes / ((size_t)n_draws * esz));
  if (r < 1) r = 1;
  return r < n_obs ? r : n_obs;
}

// row selection shared by pla_psis_loo_rows / pla_waic_rows: the index list lives where the matrix lives
static int check_rows(const int64_t* row_index, int64_t n_rows, int64_t n_src, int mem_space) {
  if (n_rows < 0) return fail(PLA_ERR_ARG, "n_rows < 0");
  if (n_rows > 0 && !row_index) return fail(PLA_ERR_ARG, "row_index is NULL");
  if (n_rows > 0 && n_src <= 0) return fail(PLA_ERR_ARG, "row selection from an empty matrix");
  if (mem_space == PLA_HOST)
    for (int64_t i = 0; i < n_rows; ++i)
      if (row_index[i] < 0 || row_index[i] >= n_src) return fail(PLA_ERR_ARG, "row_index out of range");
  return PLA_OK;
}

// device path: a clamped copy of the caller's index list in engine memory (the row kernels trust it)
static int device_rows(pla_engine* eng, const int64_t* row_index, int64_t n_rows, int64_t n_src, hipStream_t s,
                       const int64_t** out) {
  int rc = grow(&eng->d_rows, &eng->d_rows_bytes, (size_t)(n_rows > 0 ? n_rows : 1) * sizeof(int64_t));
  if (rc) return rc;
  PLA_HIP(pla::launch_clamp_rows(row_index, n_rows, n_src, (int64_t*)eng->d_rows, s));
  *out = (const int64_t*)eng->d_rows;
  return PLA_OK;
}

// host path: pack rows [r0, r0 + nr) of the call (selected rows when row_index is set) into the staging buffer
static int stage_rows(pla_engine* eng, const void* ll, const int64_t* row_index, int64_t r0, int64_t nr, int64_t stride_obs,
                      size_t esz, size_t row_bytes, hipStream_t s, int64_t stride_draw = 1, int dtype = PLA_F64,
                      int64_t rows_per_chunk = 0) {
  if (stride_draw != 1) {
    // observations fastest on the host (a (chain, draw, *obs) array viewed as (obs, sample), loo.py:189): the block of
    // observations goes up as an (n_draws, nr) slab -- one pitched copy, no transpose on the host -- and is transposed
    // on the device
    const int64_t n_draws = (int64_t)(row_bytes / esz);
    int rc = grow(&eng->d_slab, &eng->d_slab_bytes, (size_t)rows_per_chunk * row_bytes);
    if (rc) return rc;
    PLA_HIP(hipMemcpy2DAsync(eng->d_slab, (size_t)nr * esz, (const char*)ll + (size_t)r0 * esz, (size_t)stride_draw * esz,
                             (size_t)nr * esz, (size_t)n_draws, hipMemcpyHostToDevice, s));
    PLA_HIP(pla::launch_transpose_rows(eng->d_slab, dtype, nr, 0, nr, (int)n_draws, eng->d_in, s));
    return PLA_OK;
  }
  if (!row_index) {
    const char* src = (const char*)ll + (size_t)r0 * stride_obs * esz;
    PLA_HIP(hipMemcpy2DAsync(eng->d_in, row_bytes, src, (size_t)stride_obs * esz, row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
  } else {
    for (int64_t i = 0; i < nr; ++i)
      PLA_HIP(hipMemcpyAsync((char*)eng->d_in + (size_t)i * row_bytes, (const char*)ll + (size_t)row_index[r0 + i] * stride_obs * esz,
                             row_bytes, hipMemcpyHostToDevice, s));
  }
  return PLA_OK;
}

static int psis_loo_run(pla_engine* eng, const void* ll, int dtype, int64_t n_src, const int64_t* row_index, int64_t n_obs,
                        int64_t n_draws, int64_t stride_obs, int64_t stride_draw, int method, int64_t tail_count,
                        double scale_value, double good_k, int mem_space, void* stream, double* diag, double* loo_i,
                        double* lppd_i, double* agg);

static int psis_loo_impl(pla_engine* eng, const void* ll, int dtype, int64_t n_src, const int64_t* row_index, int64_t n_obs,
                         int64_t n_draws, int64_t stride_obs, int64_t stride_draw, int method, int64_t tail_count,
                         double scale_value, double good_k, int mem_space, void* stream, double* diag, double* loo_i,
                         double* lppd_i, double* agg) {
  // (n_obs = observations of this call: the selected rows when row_index is set, else all n_src rows)
  int rc = check_common(eng, ll, dtype, n_src, n_draws, stride_obs, stride_draw, method, tail_count, mem_space);
  if (rc) return rc;
  if (row_index || n_obs != n_src) {
    rc = check_rows(row_index, n_obs, n_src, mem_space);
    if (rc) return rc;
  }
  EngineCall call(eng, (hipStream_t)stream);
  return psis_loo_run(eng, ll, dtype, n_src, row_index, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, scale_value,
                      good_k, mem_space, stream, diag, loo_i, lppd_i, agg);
}

// the pass itself, for a caller that has checked the arguments and holds the engine (EngineCall)
static int psis_loo_run(pla_engine* eng, const void* ll, int dtype, int64_t n_src, const int64_t* row_index, int64_t n_obs,
                        int64_t n_draws, int64_t stride_obs, int64_t stride_draw, int method, int64_t tail_count,
                        double scale_value, double good_k, int mem_space, void* stream, double* diag, double* loo_i,
                        double* lppd_i, double* agg) {
  int rc = PLA_OK;
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const bool ingest = obs_fastest_device(mem_space, row_index, n_src, n_draws, stride_obs, stride_draw);
  // observations-fastest PSIS-LOO: the lane-per-observation kernels read the matrix as it lies (pla_col.h); PLA_INGEST_TRANSPOSE=1
  // keeps round 1's transposing ingestion (A/B runs), which also serves the shapes the column kernels do not take
  static const int64_t kColBlock = [] {  // observations per launch: 8 KB of candidate lists each (PLA_COL_BLOCK: A/B runs, experiment builds only)
    const char* e = pla::exp_str("PLA_COL_BLOCK");
    const int64_t v = e ? atoll(e) : 0;
    // (at most 262 144: the lists of one launch are addressed with 32-bit byte offsets, 8 KB per observation)
    return v >= 256 ? (v <= 262144 ? v : (int64_t)262144) : (int64_t)262144;
  }();
  int col_kq = 0;
  static const bool force_transpose = getenv("PLA_INGEST_TRANSPOSE") && atoi(getenv("PLA_INGEST_TRANSPOSE")) != 0;
  constexpr int64_t kDevBlock = (int64_t)1 << 20;  // rows per launch of a device-resident matrix (bounds the hand-over buffer)
  // (the column sweep addresses the draws of a batch with 32-bit byte offsets from the batch's first draw -- sixteen draws at
  // most -- plus the lane's observation inside the block: matrices whose draws lie further apart than that allows take the
  // transposing path instead of reading zeros past a descriptor's range)
  const bool col_offsets_fit = (double)stride_draw * (double)esz * 16.0 + (double)kColBlock * (double)esz < 2147483648.0;
  const bool use_col = ingest && method == PLA_PSIS && !force_transpose && col_offsets_fit &&
                       pla::col_supported((int)n_draws, (int)tail_count, &col_kq);
  // ... a workgroup per 16 observations (pla_tile.h), streamed (the fit kernel beside it, PLA_PIPE=0: back to back) where the
  // shorter lists of the streamed pass still leave room around the expected candidate count
  const char* pipe_env0 = getenv("PLA_PIPE");
  int tile_ks = 0;
  bool tile_stream = !(pipe_env0 && atoi(pipe_env0) == 0) && use_col && mem_space == PLA_DEVICE &&
                     pla::tile_supported(dtype, (int)n_draws, (int)tail_count, stride_draw, true, &tile_ks);
  const bool use_tile = tile_stream || (use_col && pla::tile_supported(dtype, (int)n_draws, (int)tail_count, stride_draw, false, &tile_ks));
  // Streamed split pass (device-resident, draws-fastest matrices): the fit kernel runs BESIDE the wave kernel, in the registers
  // and LDS that kernel leaves free on a CU, and takes the chunks of observations as they are finished (pla_kernels.hip,
  // launch_wave).  PLA_PIPE=0: the two kernels back to back on the caller's stream (round 2's arrangement; A/B runs).
  const char* pipe_env = getenv("PLA_PIPE");  // (read per call: tests compare the two arrangements in one process)
  bool pipeline = !(pipe_env && atoi(pipe_env) == 0) && mem_space == PLA_DEVICE && !ingest && method == PLA_PSIS;

  pla::RowsParams p{};
  p.n_obs = n_obs;
  p.n_draws = (int)n_draws;
  p.method = method;
  p.tail_count = method == PLA_PSIS ? (int)tail_count : 0;
  p.tail_cap = pow2_at_least(p.tail_count);
  p.scale_value = scale_value;
  p.counters = eng->counters;
  if (n_obs > 0) {
    rc = grow(&eng->d_slow, &eng->d_slow_bytes, (size_t)n_obs * sizeof(unsigned));
    if (rc) return rc;
    p.slow_list = (unsigned*)eng->d_slow;
    if (method == PLA_PSIS) {
      rc = ensure_l1_table(eng, tail_count, s, &p.l1_table);
      if (rc) return rc;
      // hand-over buffers of the split pass (one-chunk wave kernel -> fit kernel, pla_fit.h): sized for the
      // rows one launch processes (all of them on the device path, one staging chunk on the host path)
      if ((tail_count <= 250 && n_draws >= 256 && n_draws <= 4096) || (tail_count <= 448 && n_draws >= 256)) {  // (one-chunk / chunked wave kernels)
        const int64_t col_rows = use_tile ? kDevBlock : kColBlock;
        const int64_t chunk_rows = use_col ? (n_obs < col_rows ? n_obs : col_rows) : staged_chunk_rows(mem_space, ingest, n_obs, n_draws, esz);
        // (device-resident matrices run in blocks of kDevBlock rows, so the buffer is bounded: 1.7 GB at M = 190 however
        // many observations there are)
        int64_t rows = (mem_space == PLA_DEVICE && !ingest) ? (n_obs < kDevBlock ? n_obs : kDevBlock) : chunk_rows;
        const int stride = (int)((tail_count + 63) & ~(int64_t)63);  // 16 lanes x 4 values per quad
        if (pipeline) {  // does the launcher stream these rows at all?
          pla::RowsParams q = p;
          q.in = ll;
          q.stride_obs = stride_obs;
          q.stride_draw = stride_draw;
          q.n_obs = rows;
          q.ws_y = q.ws_s = (double*)eng->counters;  // (any non-null pointer: only looked at, never dereferenced)
          q.ws_stride = stride;
          q.ws_sstride = 16;
          pipeline = pla::rows_stream_planned(q, dtype);
        }
        if (tile_stream && !(stride <= 256)) tile_stream = false;
        if (pipeline || tile_stream) {
          rc = ensure_pipe(eng);
          if (rc) return rc;
          rc = grow(&eng->d_sync, &eng->d_sync_bytes, pla::stream_sync_bytes(rows));
          if (rc) return rc;
        }
        const int sstride = (pipeline || tile_stream) ? 16 : 8;  // (streamed: one whole 128-byte line of scalars per observation)
        rc = grow(&eng->d_ws, &eng->d_ws_bytes, (size_t)rows * (size_t)(stride + sstride) * sizeof(double));
        if (rc == PLA_ERR_NOMEM && !use_col) {
          rc = 0;  // no room for the hand-over: the fused kernels need none (the split pass is the faster, not the only, path)
        } else {
          if (rc) return rc;
          p.ws_y = (double*)eng->d_ws;
          p.ws_s = (double*)eng->d_ws + (size_t)rows * stride;
          p.ws_stride = stride;
          p.ws_sstride = sstride;
        }
      }
    }
  }
  if (!p.ws_y) pipeline = tile_stream = false;
  if (!use_tile) tile_stream = false;
  if (use_tile && !tile_stream) (void)pla::tile_supported(dtype, (int)n_draws, (int)tail_count, stride_draw, false, &tile_ks);  // (the longer lists' threshold)
  // [1]: rows left to the general kernel (a streamed pass zeroes the counters together with its flags: one command less)
  if (!pipeline && !tile_stream) PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));

  if (mem_space == PLA_DEVICE) {
    // agg needs the pointwise loo_i: use the caller's vectors, or the engine scratch
    double *dd = diag, *dl = loo_i, *dp = lppd_i;
    if (agg && (!dd || !dl || !dp)) {
      size_t have_b = eng->d_pw_elems * sizeof(double);
      rc = grow((void**)&eng->d_pw, &have_b, (size_t)(3 * n_obs + PLA_AGG_COUNT) * sizeof(double));
      eng->d_pw_elems = have_b / sizeof(double);
      if (rc) return rc;
      if (!dd) dd = eng->d_pw;
      if (!dl) dl = eng->d_pw + n_obs;
      if (!dp) dp = eng->d_pw + 2 * n_obs;
    }
    if (use_tile && p.ws_y) {
      // observations-fastest input, read in place: a workgroup per 16 observations, candidate lists in LDS (pla_tile.h)
      p.stride_obs = 1;
      p.stride_draw = stride_draw;
      for (int64_t r0 = 0; r0 < n_obs; r0 += kDevBlock) {
        const int64_t nr = (n_obs - r0 < kDevBlock) ? (n_obs - r0) : kDevBlock;
        TimedLaunch t(eng, s);
        p.in = (const char*)ll + (size_t)r0 * esz;
        p.n_obs = nr;
        p.diag = dd ? dd + r0 : nullptr;
        p.loo_i = dl ? dl + r0 : nullptr;
        p.lppd_i = dp ? dp + r0 : nullptr;
        if (tile_stream) {
          pla::PipeStreams ps{eng->pipe_first, eng->pipe_second, eng->pipe_fork, eng->pipe_join1, eng->pipe_join2, (unsigned*)eng->d_sync,
                              nullptr, nullptr, r0 == 0};
          if (eng->timing && eng->pipe_timed < pla_engine::kPipeTimed) {
            ps.before_first = eng->pipe_t0[eng->pipe_timed];
            ps.after_first = eng->pipe_t1[eng->pipe_timed];
            eng->pipe_timed += 1;
          }
          PLA_HIP(pla::launch_tile(p, dtype, tile_ks, s, &ps));
          eng->last_kernels = "tile_loo_kernel<SYNC> (a workgroup per 16 observations, matrix read in place) with fit_rows_stream_kernel beside it "
                              "on a second stream + fit_rows_kernel (leftovers) + slow_rows_kernel";
        } else {
          PLA_HIP(pla::launch_tile(p, dtype, tile_ks, s));
          eng->last_kernels = "tile_loo_kernel (a workgroup per 16 observations, matrix read in place) + fit_rows_kernel + slow_rows_kernel";
        }
      }
      if (agg) {
        pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, agg, eng->counters + 1};
        PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
      }
      return PLA_OK;
    }
    if (use_col && p.ws_y) {
      // observations-fastest input, read in place: one lane per observation (pla_col.h), block by block of observations
      rc = grow(&eng->d_col, &eng->d_col_bytes, pla::col_workspace_bytes(n_obs < kColBlock ? n_obs : kColBlock));
      if (rc) return rc;
      p.stride_obs = 1;
      p.stride_draw = stride_draw;
      for (int64_t r0 = 0; r0 < n_obs; r0 += kColBlock) {
        const int64_t nr = (n_obs - r0 < kColBlock) ? (n_obs - r0) : kColBlock;
        TimedLaunch t(eng, s);
        p.in = (const char*)ll + (size_t)r0 * esz;
        p.n_obs = nr;
        p.diag = dd ? dd + r0 : nullptr;
        p.loo_i = dl ? dl + r0 : nullptr;
        p.lppd_i = dp ? dp + r0 : nullptr;
        PLA_HIP(pla::launch_col(p, dtype, col_kq, eng->d_col, s));
        eng->last_kernels = "col_sweep_kernel (one lane per observation, matrix read in place) + col_select_kernel + fit_rows_kernel + slow_rows_kernel";
      }
      if (agg) {
        pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, agg, eng->counters + 1};
        PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
      }
      return PLA_OK;
    }
    if (ingest) {
      // observations-fastest input: transpose a block of rows into the staging buffer, run the pass on it, next block
      // (all on the caller's stream: the buffer is reused in stream order, nothing synchronises)
      const int64_t rows_per_chunk = staged_chunk_rows(mem_space, true, n_obs, n_draws, esz);
      rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows_per_chunk * (size_t)n_draws * esz);
      if (rc) return rc;
      p.in = eng->d_in;
      p.stride_obs = n_draws;
      p.stride_draw = 1;
      for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
        const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
        TimedLaunch t(eng, s);
        PLA_HIP(pla::launch_transpose_rows(ll, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in, s));
        p.n_obs = nr;
        p.diag = dd ? dd + r0 : nullptr;
        p.loo_i = dl ? dl + r0 : nullptr;
        p.lppd_i = dp ? dp + r0 : nullptr;
        PLA_HIP(pla::launch_rows(p, dtype, false, s));
      eng->last_kernels = pla::last_rows_kernels();
      }
      if (agg) {
        pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, agg, eng->counters + 1};
        PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
      }
      return PLA_OK;
    }
    p.in = ll;
    p.stride_obs = stride_obs;
    p.stride_draw = stride_draw;
    if (row_index) {
      rc = device_rows(eng, row_index, n_obs, n_src, s, &p.row_index);
      if (rc) return rc;
    }
    const int64_t* all_rows = p.row_index;
    for (int64_t r0 = 0; r0 < n_obs; r0 += kDevBlock) {
      const int64_t nr = (n_obs - r0 < kDevBlock) ? (n_obs - r0) : kDevBlock;
      p.n_obs = nr;
      if (all_rows) p.row_index = all_rows + r0;
      else p.in = (const char*)ll + (size_t)r0 * (size_t)stride_obs * esz;
      p.diag = dd ? dd + r0 : nullptr;
      p.loo_i = dl ? dl + r0 : nullptr;
      p.lppd_i = dp ? dp + r0 : nullptr;
      TimedLaunch t(eng, s);
      if (pipeline) {
        pla::PipeStreams ps{eng->pipe_first, eng->pipe_second, eng->pipe_fork, eng->pipe_join1, eng->pipe_join2, (unsigned*)eng->d_sync,
                            nullptr, nullptr, r0 == 0};
        if (eng->timing && eng->pipe_timed < pla_engine::kPipeTimed) {
          ps.before_first = eng->pipe_t0[eng->pipe_timed];
          ps.after_first = eng->pipe_t1[eng->pipe_timed];
          eng->pipe_timed += 1;
        }
        PLA_HIP(pla::launch_rows(p, dtype, false, s, nullptr, nullptr, &ps));
      eng->last_kernels = pla::last_rows_kernels();
      } else {
        PLA_HIP(pla::launch_rows(p, dtype, false, s, t.mid(), t.mid_flag()));
      eng->last_kernels = pla::last_rows_kernels();
      }
    }
#if defined(PLA_WAVE_ABLATE) && PLA_WAVE_ABLATE
    if (pla::exp_str("PLA_PRINT_REASONS")) {  // profiling build only: why rows left the fast path
      unsigned long long h[16];
      PLA_HIP(hipStreamSynchronize(s));
      PLA_HIP(hipMemcpy(h, eng->counters, sizeof(h), hipMemcpyDeviceToHost));
      fprintf(stderr, "[pla] slow rows by reason: range %llu, threshold search %llu, t1>=0 %llu, pads %llu, too few candidates %llu, "
                      "too many %llu, other %llu, selection/fit %llu\n", h[8], h[9], h[10], h[11], h[12], h[13], h[14], h[15]);
    }
    if (pla::exp_str("PLA_PRINT_CLOCK")) {  // profiling build only: core clock seen by one wave of the fast kernel
      unsigned long long h[4];
      PLA_HIP(hipStreamSynchronize(s));
      PLA_HIP(hipMemcpy(h, eng->counters, sizeof(h), hipMemcpyDeviceToHost));
      if (h[3]) fprintf(stderr, "[pla] core clock %.1f MHz (%llu core ticks / %llu ticks of 100 MHz)\n",
                        100.0 * (double)h[2] / (double)h[3], h[2], h[3]);
    }
#endif
#if defined(PLA_PHASE_CLOCK)
    {  // diagnostic build: cycles per row of the wave kernel's waves, by phase (tools/phase_clock.sh)
      unsigned long long h[16];
      PLA_HIP(hipStreamSynchronize(s));
      PLA_HIP(hipMemcpy(h, eng->counters, sizeof(h), hipMemcpyDeviceToHost));
      const double rows = h[12] ? (double)h[12] : 1.0;
      fprintf(stderr, "[pla] cycles per row and wave: statistics (incl. wait for the row) %.0f, threshold %.0f, sweep %.0f, selection %.0f; rows %llu\n",
              h[8] / rows, h[9] / rows, h[10] / rows, h[11] / rows, h[12]);
    }
#endif
    if (agg) {
      pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, agg, eng->counters + 1};
      PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
    }
    return PLA_OK;
  }

  // ---- PLA_HOST: stage row blocks through the device --------------------------------------
  {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(3 * n_obs + PLA_AGG_COUNT) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
  }
  double* dd = eng->d_pw;
  double* dl = eng->d_pw + n_obs;
  double* dp = eng->d_pw + 2 * n_obs;
  double* dagg = eng->d_pw + 3 * n_obs;
  const size_t row_bytes = (size_t)n_draws * esz;
  int64_t rows_per_chunk = (int64_t)(((size_t)1 << 30) / (row_bytes ? row_bytes : 1));
  if (rows_per_chunk < 1) rows_per_chunk = 1;
  if (rows_per_chunk > n_obs) rows_per_chunk = n_obs;
  if (n_obs > 0) {
    rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows_per_chunk * row_bytes);
    if (rc) return rc;
  }
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    // pack to (nr, S) contiguous on the device; strided sources use a pitched copy
    if (stride_draw == 1 || (stride_obs == 1 && stride_draw >= n_src && !row_index)) {
      rc = stage_rows(eng, ll, row_index, r0, nr, stride_obs, esz, row_bytes, s, stride_draw, dtype, rows_per_chunk);
      if (rc) return rc;
      p.stride_obs = n_draws;
      p.stride_draw = 1;
    } else {
      return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs unit stride along the draws, or along the observations without "
                                       "a row selection");
    }
    p.in = eng->d_in;
    p.n_obs = nr;
    p.diag = dd + r0;
    p.loo_i = dl + r0;
    p.lppd_i = dp + r0;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_rows(p, dtype, false, s));
      eng->last_kernels = pla::last_rows_kernels();
    }
    PLA_HIP(hipStreamSynchronize(s));  // the staging buffer is reused by the next chunk
  }
  if (n_obs > 0) {
    if (diag) PLA_HIP(hipMemcpyAsync(diag, dd, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (loo_i) PLA_HIP(hipMemcpyAsync(loo_i, dl, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (lppd_i) PLA_HIP(hipMemcpyAsync(lppd_i, dp, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (agg) {
    pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, dagg, eng->counters + 1};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
    PLA_HIP(hipMemcpyAsync(agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  PLA_HIP(hipStreamSynchronize(s));
  return PLA_OK;
}

int pla_psis_loo(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                 int64_t stride_draw, int method, int64_t tail_count, double scale_value, double good_k,
                 int mem_space, void* stream, double* diag, double* loo_i, double* lppd_i, double* agg) {
  return psis_loo_impl(eng, ll, dtype, n_obs, nullptr, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, scale_value,
                       good_k, mem_space, stream, diag, loo_i, lppd_i, agg);
}

int pla_psis_loo_rows(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                      int64_t stride_draw, const int64_t* row_index, int64_t n_rows, int method, int64_t tail_count,
                      double scale_value, double good_k, int mem_space, void* stream, double* diag, double* loo_i,
                      double* lppd_i, double* agg) {
  if (n_rows > 0 && !row_index) return fail(PLA_ERR_ARG, "row_index is NULL");
  return psis_loo_impl(eng, ll, dtype, n_obs, row_index, n_rows, n_draws, stride_obs, stride_draw, method, tail_count,
                       scale_value, good_k, mem_space, stream, diag, loo_i, lppd_i, agg);
}

// ---- leave-one-group-out (loo_group.py:216-300) ------------------------------------------------------------------------------
// Group index: group_offsets[n_groups + 1], group_members[group_offsets[n_groups]], in the memory space of the matrix.  Host lists
// are checked here; device lists are clamped by the group-sum kernel (pla_group.h).
static int check_groups(const int64_t* offsets, const int64_t* members, int64_t n_groups, int64_t n_obs, int mem_space) {
  if (n_groups < 0) return fail(PLA_ERR_ARG, "n_groups < 0");
  if (!offsets) return fail(PLA_ERR_ARG, "group_offsets is NULL");
  if (n_groups > 0 && n_obs < 1) return fail(PLA_ERR_ARG, "groups of an empty matrix");
  if (mem_space == PLA_DEVICE) {
    if (n_groups > 0 && !members) return fail(PLA_ERR_ARG, "group_members is NULL");
    return PLA_OK;
  }
  if (offsets[0] != 0) return fail(PLA_ERR_ARG, "group_offsets[0] must be 0, got %lld", (long long)offsets[0]);
  for (int64_t g = 0; g < n_groups; ++g)
    if (offsets[g + 1] < offsets[g]) return fail(PLA_ERR_ARG, "group_offsets decrease at group %lld", (long long)g);
  if (offsets[n_groups] > 0 && !members) return fail(PLA_ERR_ARG, "group_members is NULL");
  for (int64_t g = 0; g < n_groups; ++g)
    for (int64_t m = offsets[g]; m < offsets[g + 1]; ++m) {
      if (members[m] < 0 || members[m] >= n_obs)
        return fail(PLA_ERR_ARG, "group_members[%lld] = %lld is outside [0, %lld)", (long long)m, (long long)members[m], (long long)n_obs);
      if (m > offsets[g] && members[m] < members[m - 1])
        return fail(PLA_ERR_ARG, "the members of group %lld are not in ascending order", (long long)g);
    }
  return PLA_OK;
}

// groups per block of the group-sum buffer: sized like the ingest staging (4 GiB on the device -- PLA_INGEST_BLOCK_MB, a path
// selector: the results do not depend on it -- and 1 GiB from the host)
static int64_t group_block(int mem_space, int64_t n_groups, int64_t n_draws, size_t esz) {
  const int64_t r = staged_chunk_rows(mem_space, true, n_groups, n_draws, esz);
  return r > 0 ? r : 1;
}

// Device index lists are used as they are; host lists go up to the engine buffer behind the replaced-entry counter (word 0).
static int group_index_on_device(pla_engine* eng, const int64_t* offsets, const int64_t* members, int64_t n_groups, int mem_space,
                                 hipStream_t s, const int64_t** d_off, const int64_t** d_mem, unsigned long long** d_count) {
  if (mem_space == PLA_DEVICE) {
    *d_off = offsets;
    *d_mem = members;
    *d_count = nullptr;
    return PLA_OK;
  }
  const int64_t nm = offsets[n_groups];
  int rc = grow(&eng->d_gidx, &eng->d_gidx_bytes, (size_t)(1 + n_groups + 1 + nm) * sizeof(int64_t));
  if (rc) return rc;
  int64_t* d = (int64_t*)eng->d_gidx;
  PLA_HIP(hipMemsetAsync(d, 0, sizeof(int64_t), s));
  PLA_HIP(hipMemcpyAsync(d + 1, offsets, (size_t)(n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  if (nm > 0) PLA_HIP(hipMemcpyAsync(d + 2 + n_groups, members, (size_t)nm * sizeof(int64_t), hipMemcpyHostToDevice, s));
  *d_off = d + 1;
  *d_mem = d + 2 + n_groups;
  *d_count = (unsigned long long*)d;
  return PLA_OK;
}

// Sums of groups [g0, g0 + ng) into `out` (device, (ng, n_draws) C-contiguous, dtype of ll).  Draws-contiguous device matrices are
// read in place; observations-fastest device matrices are transposed block by block into the ingest staging, host matrices are
// uploaded block by block (one pass over the matrix per call: a host matrix whose group sums exceed one block of groups is
// read once per block).  The blocks go in ascending order and the kernel continues the partial sums, so the order of the adds
// is NumPy's whatever the block sizes.
static int group_sums_run(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                          int64_t stride_draw, const int64_t* d_off, const int64_t* d_mem, int64_t n_groups, int64_t g0, int64_t ng,
                          int mem_space, hipStream_t s, void* out, unsigned long long* replaced) {
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  if (mem_space == PLA_DEVICE && stride_draw == 1) {
    PLA_HIP(pla::launch_group_sum(ll, dtype, stride_obs, 0, n_obs, n_obs, false, true, (int)n_draws, d_off, d_mem, n_groups, g0, ng,
                                  out, replaced, s));
    eng->last_kernels = "group_sum_kernel (matrix read in place)";
    return PLA_OK;
  }
  const bool obs_fastest = n_obs > 1 && n_draws > 1 && stride_obs == 1 && stride_draw >= n_obs;
  if (!obs_fastest && !(mem_space == PLA_HOST && stride_draw == 1))
    return fail(PLA_ERR_UNSUPPORTED, "group sums need unit stride along the draws, or along the observations");
  const size_t row_bytes = (size_t)n_draws * esz;
  const int64_t rows_per_chunk = mem_space == PLA_DEVICE ? staged_chunk_rows(mem_space, true, n_obs, n_draws, esz)
                                                         : staged_chunk_rows(mem_space, false, n_obs, n_draws, esz);
  int rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows_per_chunk * row_bytes);
  if (rc) return rc;
  const bool blocked = rows_per_chunk < n_obs;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    if (mem_space == PLA_DEVICE) {
      PLA_HIP(pla::launch_transpose_rows(ll, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in, s));
    } else {
      rc = stage_rows(eng, ll, nullptr, r0, nr, stride_obs, esz, row_bytes, s, stride_draw, dtype, rows_per_chunk);
      if (rc) return rc;
    }
    PLA_HIP(pla::launch_group_sum(eng->d_in, dtype, n_draws, r0, nr, n_obs, blocked, r0 == 0, (int)n_draws, d_off, d_mem, n_groups, g0,
                                  ng, out, replaced, s));
    if (mem_space == PLA_HOST) PLA_HIP(hipStreamSynchronize(s));  // the staging buffer is reused by the next block
  }
  eng->last_kernels = mem_space == PLA_DEVICE ? "transpose_rows_kernel + group_sum_kernel (blocks of observations)"
                                              : "group_sum_kernel (blocks of observations uploaded)";
  return PLA_OK;
}

int pla_group_sum(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                  const int64_t* group_offsets, const int64_t* group_members, int64_t n_groups, int mem_space, void* stream, void* out,
                  int64_t* n_replaced) {
  int rc = check_common(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, PLA_SIS, 0, mem_space);
  if (rc) return rc;
  rc = check_groups(group_offsets, group_members, n_groups, n_obs, mem_space);
  if (rc) return rc;
  if (n_groups > 0 && !out) return fail(PLA_ERR_ARG, "out is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int64_t* d_off = nullptr;
  const int64_t* d_mem = nullptr;
  unsigned long long* d_count = nullptr;
  rc = group_index_on_device(eng, group_offsets, group_members, n_groups, mem_space, s, &d_off, &d_mem, &d_count);
  if (rc) return rc;
  if (mem_space == PLA_DEVICE) {
    if (n_replaced) PLA_HIP(hipMemsetAsync(n_replaced, 0, sizeof(int64_t), s));
    TimedLaunch t(eng, s);  // (the group-sum kernel's own time: pla_engine_kernel_ms)
    return group_sums_run(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, d_off, d_mem, n_groups, 0, n_groups, mem_space, s, out,
                          (unsigned long long*)n_replaced);
  }
  const int64_t gb = group_block(mem_space, n_groups, n_draws, esz);
  if (n_groups > 0) {
    rc = grow(&eng->d_grp, &eng->d_grp_bytes, (size_t)gb * (size_t)n_draws * esz);
    if (rc) return rc;
  }
  for (int64_t g0 = 0; g0 < n_groups; g0 += gb) {
    const int64_t ng = n_groups - g0 < gb ? n_groups - g0 : gb;
    rc = group_sums_run(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, d_off, d_mem, n_groups, g0, ng, mem_space, s, eng->d_grp,
                        d_count);
    if (rc) return rc;
    PLA_HIP(hipMemcpyAsync((char*)out + (size_t)g0 * (size_t)n_draws * esz, eng->d_grp, (size_t)ng * (size_t)n_draws * esz,
                           hipMemcpyDeviceToHost, s));
  }
  unsigned long long h = 0;
  if (n_replaced) PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

int pla_psis_loo_groups(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                        int64_t stride_draw, const int64_t* group_offsets, const int64_t* group_members, int64_t n_groups, int method,
                        int64_t tail_count, double scale_value, double good_k, int mem_space, void* stream, double* diag,
                        double* logo_i, double* lppd_i, double* agg, int64_t* n_replaced) {
  int rc = check_common(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, mem_space);
  if (rc) return rc;
  if (n_groups < 1) return fail(PLA_ERR_ARG, "n_groups < 1");
  rc = check_groups(group_offsets, group_members, n_groups, n_obs, mem_space);
  if (rc) return rc;
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int64_t* d_off = nullptr;
  const int64_t* d_mem = nullptr;
  unsigned long long* d_count = nullptr;
  rc = group_index_on_device(eng, group_offsets, group_members, n_groups, mem_space, s, &d_off, &d_mem, &d_count);
  if (rc) return rc;
  if (mem_space == PLA_DEVICE) {
    d_count = (unsigned long long*)n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  }
  // pointwise outputs: the caller's device vectors, else (host calls, or agg without them) the engine scratch
  double *dd = diag, *dl = logo_i, *dp = lppd_i;
  if (mem_space == PLA_HOST || (agg && (!dd || !dl || !dp))) {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(3 * n_groups + PLA_AGG_COUNT) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
    if (mem_space == PLA_HOST || !dd) dd = eng->d_pw;
    if (mem_space == PLA_HOST || !dl) dl = eng->d_pw + n_groups;
    if (mem_space == PLA_HOST || !dp) dp = eng->d_pw + 2 * n_groups;
  }
  // one block of groups at a time: its sums in the bounded buffer, the PSIS / SIS / TIS pass over them into its slices
  const int64_t gb = group_block(mem_space, n_groups, n_draws, esz);
  rc = grow(&eng->d_grp, &eng->d_grp_bytes, (size_t)gb * (size_t)n_draws * esz);
  if (rc) return rc;
  std::string label;
  for (int64_t g0 = 0; g0 < n_groups; g0 += gb) {
    const int64_t ng = n_groups - g0 < gb ? n_groups - g0 : gb;
    rc = group_sums_run(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, d_off, d_mem, n_groups, g0, ng, mem_space, s,
                        eng->d_grp, d_count);
    if (rc) return rc;
    const std::string sum_kernels = eng->last_kernels;
    rc = psis_loo_run(eng, eng->d_grp, dtype, ng, nullptr, ng, n_draws, n_draws, 1, method, tail_count, scale_value, good_k, PLA_DEVICE,
                      stream, dd ? dd + g0 : nullptr, dl ? dl + g0 : nullptr, dp ? dp + g0 : nullptr, nullptr);
    if (rc) return rc;
    if (g0 == 0) label = sum_kernels + " per block of groups, then " + eng->last_kernels;
  }
  eng->last_kernels = label;
  // the aggregates once, over all groups
  double* dagg = mem_space == PLA_HOST ? eng->d_pw + 3 * n_groups : agg;
  if (agg) {
    pla::ReduceParams rp{dd, dl, dp, n_groups, good_k, dagg, eng->counters + 1};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
  }
  if (mem_space == PLA_DEVICE) return PLA_OK;
  if (diag) PLA_HIP(hipMemcpyAsync(diag, dd, n_groups * sizeof(double), hipMemcpyDeviceToHost, s));
  if (logo_i) PLA_HIP(hipMemcpyAsync(logo_i, dl, n_groups * sizeof(double), hipMemcpyDeviceToHost, s));
  if (lppd_i) PLA_HIP(hipMemcpyAsync(lppd_i, dp, n_groups * sizeof(double), hipMemcpyDeviceToHost, s));
  if (agg) PLA_HIP(hipMemcpyAsync(agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  unsigned long long h = 0;
  if (n_replaced) PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

// ---- approximate posteriors (loo_approximate_posterior.py:223-348) -------------------------------------------------------------
// Draw index: draw_index[n_out] in the memory space of the matrix.  Host lists are checked here; device lists are clamped by the
// gather kernel (pla_draws.h).
static int check_draws(const int64_t* draw_index, int64_t n_out, int64_t n_draws, int mem_space) {
  if (n_out < 1 || n_out > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_out out of range");
  if (!draw_index) return fail(PLA_ERR_ARG, "draw_index is NULL");
  if (mem_space == PLA_HOST)
    for (int64_t j = 0; j < n_out; ++j)
      if (draw_index[j] < 0 || draw_index[j] >= n_draws)
        return fail(PLA_ERR_ARG, "draw_index[%lld] = %lld is outside [0, %lld)", (long long)j, (long long)draw_index[j], (long long)n_draws);
  return PLA_OK;
}

static bool host_obs_fastest(int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw) {
  return n_obs > 1 && n_draws > 1 && stride_obs == 1 && stride_draw >= n_obs;
}

// Device index lists are used as they are; host lists go up to the engine buffer behind the replaced-entry counter (word 0).
static int draw_index_on_device(pla_engine* eng, const int64_t* draw_index, int64_t n_out, int mem_space, hipStream_t s,
                                const int64_t** d_idx, unsigned long long** d_count) {
  if (mem_space == PLA_DEVICE) {
    *d_idx = draw_index;
    *d_count = nullptr;
    return PLA_OK;
  }
  int rc = grow(&eng->d_gidx, &eng->d_gidx_bytes, (size_t)(1 + n_out) * sizeof(int64_t));
  if (rc) return rc;
  int64_t* d = (int64_t*)eng->d_gidx;
  PLA_HIP(hipMemsetAsync(d, 0, sizeof(int64_t), s));
  PLA_HIP(hipMemcpyAsync(d + 1, draw_index, (size_t)n_out * sizeof(int64_t), hipMemcpyHostToDevice, s));
  *d_idx = d + 1;
  *d_count = (unsigned long long*)d;
  return PLA_OK;
}

// Rows [r0, r0 + nr) of the matrix with their draws gathered into `dst` (device, (nr, n_out) C-contiguous).  Device matrices are
// read in place; a block of a host matrix goes up to the slab buffer as it lies -- (nr, n_draws) rows, or the (n_draws, nr) slab
// of an observations-fastest matrix -- and is gathered from there.
static int gather_block(pla_engine* eng, const void* ll, int dtype, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                        const int64_t* d_idx, int64_t n_out, int64_t r0, int64_t nr, int mem_space, hipStream_t s, void* dst,
                        unsigned long long* d_count, const char** route) {
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  if (mem_space == PLA_DEVICE) {
    PLA_HIP(pla::launch_gather_draws((const char*)ll + (size_t)r0 * (size_t)stride_obs * esz, dtype, stride_obs, stride_draw, nr,
                                     (int)n_draws, d_idx, (int)n_out, dst, d_count, s, route));
    return PLA_OK;
  }
  if (stride_draw == 1) {
    const size_t row_bytes = (size_t)n_draws * esz;
    PLA_HIP(hipMemcpy2DAsync(eng->d_slab, row_bytes, (const char*)ll + (size_t)r0 * (size_t)stride_obs * esz, (size_t)stride_obs * esz,
                             row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    PLA_HIP(pla::launch_gather_draws(eng->d_slab, dtype, n_draws, 1, nr, (int)n_draws, d_idx, (int)n_out, dst, d_count, s, route));
  } else {
    PLA_HIP(hipMemcpy2DAsync(eng->d_slab, (size_t)nr * esz, (const char*)ll + (size_t)r0 * esz, (size_t)stride_draw * esz,
                             (size_t)nr * esz, (size_t)n_draws, hipMemcpyHostToDevice, s));
    PLA_HIP(pla::launch_gather_draws(eng->d_slab, dtype, 1, nr, nr, (int)n_draws, d_idx, (int)n_out, dst, d_count, s, route));
  }
  return PLA_OK;
}

static int check_gather(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                        int64_t stride_draw, const int64_t* draw_index, int64_t n_out, int mem_space) {
  int rc = check_common(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, PLA_SIS, 0, mem_space);
  if (rc) return rc;
  rc = check_draws(draw_index, n_out, n_draws, mem_space);
  if (rc) return rc;
  if (mem_space == PLA_HOST && stride_draw != 1 && !host_obs_fastest(n_obs, n_draws, stride_obs, stride_draw))
    return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs unit stride along the draws, or along the observations");
  return PLA_OK;
}

// rows per block of a host call: the slab holds n_draws, the staging n_out entries per row
static int64_t host_gather_rows(int64_t n_obs, int64_t n_draws, int64_t n_out, size_t esz) {
  return staged_chunk_rows(PLA_HOST, false, n_obs, n_draws > n_out ? n_draws : n_out, esz);
}

int pla_gather_draws(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                     const int64_t* draw_index, int64_t n_out, int mem_space, void* stream, void* out, int64_t* n_replaced) {
  int rc = check_gather(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, draw_index, n_out, mem_space);
  if (rc) return rc;
  if (n_obs > 0 && !out) return fail(PLA_ERR_ARG, "out is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int64_t* d_idx = nullptr;
  unsigned long long* d_count = nullptr;
  rc = draw_index_on_device(eng, draw_index, n_out, mem_space, s, &d_idx, &d_count);
  if (rc) return rc;
  const char* route = "";
  if (mem_space == PLA_DEVICE) {
    if (n_replaced) PLA_HIP(hipMemsetAsync(n_replaced, 0, sizeof(int64_t), s));
    TimedLaunch t(eng, s);  // (the gather kernel's own time: pla_engine_kernel_ms)
    rc = gather_block(eng, ll, dtype, n_draws, stride_obs, stride_draw, d_idx, n_out, 0, n_obs, mem_space, s, out,
                      (unsigned long long*)n_replaced, &route);
    eng->last_kernels = std::string(route) + " (matrix read in place)";
    return rc;
  }
  const int64_t rows = host_gather_rows(n_obs, n_draws, n_out, esz);
  rc = grow(&eng->d_slab, &eng->d_slab_bytes, (size_t)rows * (size_t)n_draws * esz);
  if (rc) return rc;
  rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows * (size_t)n_out * esz);
  if (rc) return rc;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    rc = gather_block(eng, ll, dtype, n_draws, stride_obs, stride_draw, d_idx, n_out, r0, nr, mem_space, s, eng->d_in, d_count, &route);
    if (rc) return rc;
    PLA_HIP(hipMemcpyAsync((char*)out + (size_t)r0 * (size_t)n_out * esz, eng->d_in, (size_t)nr * (size_t)n_out * esz,
                           hipMemcpyDeviceToHost, s));
    PLA_HIP(hipStreamSynchronize(s));  // the buffers are reused by the next block
  }
  eng->last_kernels = std::string(route) + " (blocks of observations uploaded)";
  unsigned long long h = 0;
  if (n_replaced) PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

int pla_psis_loo_draws(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                       int64_t stride_draw, const int64_t* draw_index, int64_t n_out, int method, int64_t tail_count, double scale_value,
                       double good_k, int mem_space, void* stream, double* diag, double* loo_i, double* lppd_i, double* agg,
                       int64_t* n_replaced) {
  int rc = check_gather(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, draw_index, n_out, mem_space);
  if (rc) return rc;
  rc = check_common(eng, ll, dtype, n_obs, n_out, n_out, 1, method, tail_count, mem_space);  // the pass runs over n_out draws
  if (rc) return rc;
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int64_t* d_idx = nullptr;
  unsigned long long* d_count = nullptr;
  rc = draw_index_on_device(eng, draw_index, n_out, mem_space, s, &d_idx, &d_count);
  if (rc) return rc;
  if (mem_space == PLA_DEVICE) {
    d_count = (unsigned long long*)n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  }
  // pointwise outputs: the caller's device vectors, else (host calls, or agg without them) the engine scratch
  double *dd = diag, *dl = loo_i, *dp = lppd_i;
  if (mem_space == PLA_HOST || (agg && (!dd || !dl || !dp))) {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(3 * n_obs + PLA_AGG_COUNT) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
    if (mem_space == PLA_HOST || !dd) dd = eng->d_pw;
    if (mem_space == PLA_HOST || !dl) dl = eng->d_pw + n_obs;
    if (mem_space == PLA_HOST || !dp) dp = eng->d_pw + 2 * n_obs;
  }
  // one block of observations at a time: its gathered rows in the bounded staging buffer, the PSIS / SIS / TIS pass over them into
  // its slices
  const int64_t rows = mem_space == PLA_DEVICE ? staged_chunk_rows(mem_space, true, n_obs, n_out, esz) : host_gather_rows(n_obs, n_draws, n_out, esz);
  if (mem_space == PLA_HOST) {
    rc = grow(&eng->d_slab, &eng->d_slab_bytes, (size_t)rows * (size_t)n_draws * esz);
    if (rc) return rc;
  }
  rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows * (size_t)n_out * esz);
  if (rc) return rc;
  // (every block's pass zeroes the slow-row total it reports: the blocks' totals are summed beside it and put back for the reduction)
  unsigned long long* block_total = eng->counters + pla::kCounterBlockTotal;
  PLA_HIP(hipMemsetAsync(block_total, 0, sizeof(unsigned long long), s));
  std::string label;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    const char* route = "";
    rc = gather_block(eng, ll, dtype, n_draws, stride_obs, stride_draw, d_idx, n_out, r0, nr, mem_space, s, eng->d_in, d_count, &route);
    if (rc) return rc;
    rc = psis_loo_run(eng, eng->d_in, dtype, nr, nullptr, nr, n_out, n_out, 1, method, tail_count, scale_value, good_k, PLA_DEVICE, stream,
                      dd ? dd + r0 : nullptr, dl ? dl + r0 : nullptr, dp ? dp + r0 : nullptr, nullptr);
    if (rc) return rc;
    PLA_HIP(pla::launch_add_counter(eng->counters + 1, block_total, s));
    if (r0 == 0) label = std::string(route) + " per block of observations, then " + eng->last_kernels;
    if (mem_space == PLA_HOST) PLA_HIP(hipStreamSynchronize(s));  // the buffers are reused by the next block
  }
  eng->last_kernels = label;
  // the aggregates once, over all observations
  double* dagg = mem_space == PLA_HOST ? eng->d_pw + 3 * n_obs : agg;
  if (agg) {
    pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, dagg, block_total};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
  }
  if (mem_space == PLA_DEVICE) return PLA_OK;
  if (n_obs > 0) {
    if (diag) PLA_HIP(hipMemcpyAsync(diag, dd, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (loo_i) PLA_HIP(hipMemcpyAsync(loo_i, dl, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (lppd_i) PLA_HIP(hipMemcpyAsync(lppd_i, dp, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (agg) PLA_HIP(hipMemcpyAsync(agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  unsigned long long h = 0;
  if (n_replaced) PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

int pla_gather_lds_max_draws(int dtype) { return pla::gather_lds_max_draws(dtype); }

// ---- k-fold cross-validation (loo_kfold.py:250-299, 643-692) -------------------------------------------------------------------
int pla_kfold_lme(pla_engine* eng, const void* const* src_base, const int64_t* src_rows, const int64_t* src_draws,
                  const int64_t* src_stride_row, const int64_t* src_stride_draw, int64_t n_sources, int dtype, int nan_flag,
                  const int64_t* source_offsets, const int64_t* task_row, const int64_t* task_out, int64_t n_tasks, int mem_space,
                  void* stream, double* out, int64_t n_out, int64_t* n_replaced) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (mem_space == PLA_HOST) return fail(PLA_ERR_UNSUPPORTED, "pla_kfold_lme reads device memory only (upload the fold matrices first)");
  if (n_sources < 1 || n_sources > (int64_t)1 << 24) return fail(PLA_ERR_ARG, "n_sources out of range");
  if (!src_base || !src_rows || !src_draws || !src_stride_row || !src_stride_draw) return fail(PLA_ERR_ARG, "a source array is NULL");
  if (n_tasks < 0 || n_out < 0) return fail(PLA_ERR_ARG, "n_tasks < 0 or n_out < 0");
  if (n_tasks > 0 && (!source_offsets || !task_row || !task_out || !out)) return fail(PLA_ERR_ARG, "a task array or out is NULL");
  for (int64_t k = 0; k < n_sources; ++k) {
    if (src_rows[k] < 0) return fail(PLA_ERR_ARG, "source %lld: n_rows < 0", (long long)k);
    if (src_rows[k] > 0 && !src_base[k]) return fail(PLA_ERR_ARG, "source %lld: base pointer is NULL", (long long)k);
    if (src_draws[k] < 1 || src_draws[k] > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "source %lld: n_draws out of range", (long long)k);
    if (src_stride_row[k] < 0 || src_stride_draw[k] <= 0) return fail(PLA_ERR_ARG, "source %lld: bad strides", (long long)k);
  }
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  if (n_replaced) PLA_HIP(hipMemsetAsync(n_replaced, 0, sizeof(int64_t), s));
  if (n_tasks == 0) return PLA_OK;
  // the table: built in pinned host memory that outlives the call, uploaded on the caller's stream
  const size_t bytes = (size_t)n_sources * sizeof(pla::KfoldSource);
  int rc = grow(&eng->d_kf, &eng->d_kf_bytes, bytes);
  if (rc) return rc;
  const int turn = eng->kf_turn;
  eng->kf_turn ^= 1;
  if (!eng->kf_event[turn]) {
    if (g_frozen) return fail(PLA_ERR_FROZEN, "the engine is frozen and has no k-fold table yet");
    PLA_HIP(hipEventCreateWithFlags(&eng->kf_event[turn], hipEventDisableTiming));
  } else {
    PLA_HIP(hipEventSynchronize(eng->kf_event[turn]));  // (the upload of two calls ago: done, unless that call is still queued)
  }
  if (eng->h_kf_bytes[turn] < bytes) {
    if (g_frozen) return fail(PLA_ERR_FROZEN, "the engine workspace is frozen and this call needs a larger k-fold table");
    if (eng->h_kf[turn]) (void)hipHostFree(eng->h_kf[turn]);
    eng->h_kf[turn] = nullptr;
    eng->h_kf_bytes[turn] = 0;
    PLA_HIP(hipHostMalloc(&eng->h_kf[turn], bytes, hipHostMallocDefault));
    eng->h_kf_bytes[turn] = bytes;
  }
  pla::KfoldSource* tab = (pla::KfoldSource*)eng->h_kf[turn];
  unsigned routes = 0;
  for (int64_t k = 0; k < n_sources; ++k) {
    // (a source without rows has no tasks: its entry only has to be harmless)
    const int route = pla::kfold_route(src_base[k], dtype, src_stride_row[k], src_stride_draw[k], src_draws[k]);
    tab[k] = pla::KfoldSource{src_base[k], src_rows[k], src_stride_row[k], src_stride_draw[k], (int)src_draws[k],
                              route | ((k == 0 && nan_flag) ? pla::kKfoldNanFlag : 0)};
    if (src_rows[k] > 0) routes |= 1u << route;
  }
  PLA_HIP(hipMemcpyAsync(eng->d_kf, tab, bytes, hipMemcpyHostToDevice, s));
  PLA_HIP(hipEventRecord(eng->kf_event[turn], s));
  pla::KfoldParams p{(const pla::KfoldSource*)eng->d_kf, (int)n_sources, source_offsets, task_row, task_out, n_tasks, out, n_out,
                     (unsigned long long*)n_replaced};
  int launches = 0;
  {
    TimedLaunch t(eng, s);  // (the ragged pass alone: pla_engine_kernel_ms)
    PLA_HIP(pla::launch_kfold_lme(p, dtype, routes, s, &launches));
  }
  std::string label;
  for (int r = 0; r < 3; ++r)
    if (routes & (1u << r)) label += std::string(label.empty() ? "" : " + ") + pla::kfold_route_name(r) + "<" + pla::dtype_name(dtype) + ">";
  // (the count is of the launches made, not of the routes asked for)
  eng->kf_label = label + " (matrices read in place; " + std::to_string(launches) + (launches == 1 ? " launch)" : " launches)");
  eng->last_kernels = eng->kf_label;
  return PLA_OK;
}

int pla_kfold_reduce(pla_engine* eng, const double* elpd, const double* lpd_full, int64_t n_obs, double scale, const int64_t* n_replaced,
                     int mem_space, void* stream, double* p_i, double* kfold_i, double* agg) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (mem_space == PLA_HOST) return fail(PLA_ERR_UNSUPPORTED, "pla_kfold_reduce reads device memory only");
  if (n_obs < 1 || n_obs >= ((int64_t)1 << 40)) return fail(PLA_ERR_ARG, "n_obs must lie in [1, 2^40), got %lld", (long long)n_obs);
  if (!elpd || !lpd_full || !agg) return fail(PLA_ERR_ARG, "elpd, lpd_full or agg is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  int rc = grow(&eng->d_cmp, &eng->d_cmp_bytes, (size_t)pla::kfold_n_tiles(n_obs) * 4 * sizeof(double));
  if (rc) return rc;
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_kfold_reduce(elpd, lpd_full, n_obs, scale, p_i, kfold_i, (double*)eng->d_cmp,
                                     (const unsigned long long*)n_replaced, agg, eng->compare_grid, s));
  }
  // (behind pla_kfold_lme the text keeps the routes of the ragged pass)
  const std::string finish = "kfold_tiles_kernel<0> + kfold_tiles_kernel<1> + kfold_final_kernel";
  eng->last_kernels = eng->kf_label.empty() ? finish : eng->kf_label + ", then " + finish;
  eng->kf_label.clear();
  return PLA_OK;
}

// ---- Mix-IS-LOO (pla_mixis.h) -----------------------------------------------------------------------------------------------------
static int mixis_check(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                       int64_t stride_draw, int mem_space) {
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (n_obs < 1 || n_obs >= ((int64_t)1 << 40)) return fail(PLA_ERR_ARG, "n_obs must lie in [1, 2^40), got %lld", (long long)n_obs);
  if (n_draws < 1 || n_draws > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_draws must lie in [1, 2^30], got %lld", (long long)n_draws);
  if (!ll) return fail(PLA_ERR_ARG, "the matrix pointer is NULL");
  if (stride_obs < 0 || stride_draw < 0 || (n_obs > 1 && stride_obs == 0) || (n_draws > 1 && stride_draw == 0))
    return fail(PLA_ERR_ARG, "bad strides");
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (mem_space == PLA_HOST && !(stride_draw == 1 && (n_obs == 1 || stride_obs >= n_draws)) &&
      !(stride_obs == 1 && (n_draws == 1 || stride_draw >= n_obs)))
    return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs unit stride along the draws or along the observations");
  return PLA_OK;
}

// the sections of pla_engine::d_mix, in doubles
struct MixisWorkspace {
  size_t slab, c, lse, elpd, loo, agg, part, counts, total;
  MixisWorkspace(int64_t n_obs, int64_t n_draws) {
    const auto even = [](size_t n) { return (n + 1) & ~(size_t)1; };
    slab = 0;
    c = slab + 2 * (size_t)pla::mixis_n_tiles(n_obs) * (size_t)n_draws;
    lse = c + even((size_t)n_draws);
    elpd = lse + 2;
    loo = elpd + even((size_t)n_obs);  // (the scaled values of a PLA_HOST call)
    agg = loo + even((size_t)n_obs);
    part = agg + PLA_AGG_COUNT;
    counts = part + 4 * (size_t)pla::kfold_n_tiles(n_obs);
    total = counts + 2;
  }
};

// A PLA_HOST matrix goes through the staging buffer in blocks of whole tiles of pass 1, once per pass, each block in the matrix's own
// layout: rows [r0, r0 + nr) as an (nr, n_draws) block (draws fastest) or as an (n_draws, nr) slab whose pitch is nr rounded up to
// 16 bytes (observations fastest).  Block size: 1 GiB, or PLA_INGEST_BLOCK_MB (read per call).  f(ptr, r0, nr, stride_obs,
// stride_draw, vec_pitch) runs the kernels on one block; a device matrix is one block, read in place.
static int64_t mixis_block_rows(int64_t n_obs, int64_t n_draws, size_t esz) {
  const char* e = getenv("PLA_INGEST_BLOCK_MB");
  const long mb = e ? atol(e) : 0;
  const size_t bytes = mb > 0 ? (size_t)mb << 20 : (size_t)1 << 30;
  const int64_t t = pla::mixis_tile_rows_for(n_obs);
  int64_t r = (int64_t)(bytes / ((size_t)n_draws * esz)) / t * t;
  if (r < t) r = t;
  return r < n_obs ? r : n_obs;
}

using MixisBlockFn = std::function<int(const void*, int64_t, int64_t, int64_t, int64_t, int64_t)>;
static int mixis_blocks(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                        int64_t stride_draw, int mem_space, hipStream_t s, const MixisBlockFn& f) {
  if (mem_space == PLA_DEVICE) return f(ll, (int64_t)0, n_obs, stride_obs, stride_draw, stride_draw);
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const bool draws_fastest = stride_draw == 1 && (n_obs == 1 || stride_obs >= n_draws);
  const int64_t rows = mixis_block_rows(n_obs, n_draws, esz);
  const int64_t pitch = draws_fastest ? n_draws : (rows + 3) / 4 * 4;  // of the staged block, elements
  int rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)(draws_fastest ? rows : n_draws) * (size_t)pitch * esz);
  if (rc) return rc;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    if (draws_fastest) {
      PLA_HIP(hipMemcpy2DAsync(eng->d_in, (size_t)n_draws * esz, (const char*)ll + (size_t)r0 * (size_t)stride_obs * esz,
                               (size_t)(n_obs == 1 ? n_draws : stride_obs) * esz, (size_t)n_draws * esz, (size_t)nr,
                               hipMemcpyHostToDevice, s));
      rc = f(eng->d_in, r0, nr, n_draws, (int64_t)1, (int64_t)1);
    } else {
      PLA_HIP(hipMemcpy2DAsync(eng->d_in, (size_t)pitch * esz, (const char*)ll + (size_t)r0 * esz,
                               (size_t)(n_draws == 1 ? n_obs : stride_draw) * esz, (size_t)nr * esz, (size_t)n_draws,
                               hipMemcpyHostToDevice, s));
      rc = f(eng->d_in, r0, nr, (int64_t)1, pitch, n_obs);  // (16-byte loads where a device matrix of pitch n_obs takes them)
    }
    if (rc) return rc;
    PLA_HIP(hipStreamSynchronize(s));  // the staging buffer is reused by the next block
  }
  return PLA_OK;
}

static int mixis_pass1(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                       int64_t stride_draw, int mem_space, hipStream_t s, double* slab, double* c, unsigned long long* replaced,
                       char* route, int cap) {
  int rc = mixis_blocks(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, mem_space, s,
                        [&](const void* p, int64_t r0, int64_t nr, int64_t so, int64_t sd, int64_t vec_pitch) -> int {
                          PLA_HIP(pla::launch_mixis_c(p, dtype, nr, (int)n_draws, so, sd, n_obs, r0, vec_pitch, slab, replaced,
                                                      eng->mixis_grid, s, route, cap));
                          return PLA_OK;
                        });
  if (rc) return rc;
  PLA_HIP(pla::launch_mixis_c_merge(slab, n_obs, (int)n_draws, c, eng->mixis_grid, s));
  return PLA_OK;
}

int pla_mixis_tile_rows(int64_t n_obs) {
  if (n_obs < 1 || n_obs >= ((int64_t)1 << 40)) return fail(PLA_ERR_ARG, "n_obs must lie in [1, 2^40), got %lld", (long long)n_obs);
  return (int)pla::mixis_tile_rows_for(n_obs);
}

int pla_engine_set_mixis_grid(pla_engine* eng, int max_workgroups) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (max_workgroups < 0) return fail(PLA_ERR_ARG, "max_workgroups < 0");
  EngineCall call(eng);
  eng->mixis_grid = max_workgroups;
  return PLA_OK;
}

static const char* mixis_where(bool host) { return host ? "(matrix staged in blocks)" : "(matrix read in place)"; }

int pla_mixis_draw_lse(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                       int64_t stride_draw, int mem_space, void* stream, double* c, int64_t* n_replaced) {
  int rc = mixis_check(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, mem_space);
  if (rc) return rc;
  if (!c) return fail(PLA_ERR_ARG, "c is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const MixisWorkspace w(n_obs, n_draws);
  rc = grow(&eng->d_mix, &eng->d_mix_bytes, w.total * sizeof(double));
  if (rc) return rc;
  double* ws = (double*)eng->d_mix;
  const bool host = mem_space == PLA_HOST;
  PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));  // [1] NaN, [2] +-inf
  char route[96];
  double* dc = host ? ws + w.c : c;
  int64_t* dcounts = (int64_t*)(ws + w.counts);
  {
    TimedLaunch t(eng, s);
    rc = mixis_pass1(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, mem_space, s, ws + w.slab, dc, eng->counters + 1, route,
                     (int)sizeof(route));
    if (rc) return rc;
  }
  if (n_replaced) PLA_HIP(pla::launch_mixis_counts(eng->counters + 1, nullptr, host ? dcounts : n_replaced, s));
  eng->last_kernels = std::string(route) + " + mixis_c_merge_kernel " + mixis_where(host);
  if (host) {
    PLA_HIP(hipMemcpyAsync(c, dc, (size_t)n_draws * sizeof(double), hipMemcpyDeviceToHost, s));
    if (n_replaced) PLA_HIP(hipMemcpyAsync(n_replaced, dcounts, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PLA_HIP(hipStreamSynchronize(s));
  }
  return PLA_OK;
}

int pla_mixis_loo(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                  const double* c, double scale_value, int mem_space, void* stream, double* loo_i, double* agg) {
  int rc = mixis_check(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, mem_space);
  if (rc) return rc;
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const MixisWorkspace w(n_obs, n_draws);
  rc = grow(&eng->d_mix, &eng->d_mix_bytes, w.total * sizeof(double));
  if (rc) return rc;
  double* ws = (double*)eng->d_mix;
  const bool host = mem_space == PLA_HOST;
  char route1[96] = "", route2[96];
  const double* dc = c;
  TimedLaunch t(eng, s);
  if (!c) {  // pass 1 by this call (its count of replaced entries is pass 2's)
    rc = mixis_pass1(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, mem_space, s, ws + w.slab, ws + w.c, nullptr, route1,
                     (int)sizeof(route1));
    if (rc) return rc;
    dc = ws + w.c;
  } else if (host) {
    PLA_HIP(hipMemcpyAsync(ws + w.c, c, (size_t)n_draws * sizeof(double), hipMemcpyHostToDevice, s));
    dc = ws + w.c;
  }
  PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));  // [1] NaN, [2] +-inf
  PLA_HIP(pla::launch_mixis_lse_c(dc, (int)n_draws, ws + w.lse, s));
  rc = mixis_blocks(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, mem_space, s,
                    [&](const void* p, int64_t r0, int64_t nr, int64_t so, int64_t sd, int64_t) -> int {
                      PLA_HIP(pla::launch_mixis_elpd(p, dtype, nr, (int)n_draws, so, sd, dc, ws + w.lse, ws + w.elpd + r0,
                                                     eng->counters + 1, eng->mixis_grid, s, route2, (int)sizeof(route2)));
                      return PLA_OK;
                    });
  if (rc) return rc;
  // the scale and the aggregates: the k-fold finishing pass on (elpd, elpd) -- kfold_i = scale * elpd, p_i = 0
  double* dloo = host ? (loo_i ? ws + w.loo : nullptr) : loo_i;
  double* dagg = host || !agg ? ws + w.agg : agg;
  PLA_HIP(pla::launch_kfold_reduce(ws + w.elpd, ws + w.elpd, n_obs, scale_value, nullptr, dloo, ws + w.part, nullptr, dagg,
                                   eng->mixis_grid, s));
  PLA_HIP(pla::launch_mixis_counts(eng->counters + 1, dagg, nullptr, s));
  eng->last_kernels = (route1[0] ? std::string(route1) + " + mixis_c_merge_kernel, then " : std::string()) + "mixis_lse_c_kernel + " +
                      route2 + ", then kfold_tiles_kernel<0> + kfold_tiles_kernel<1> + kfold_final_kernel " + mixis_where(host);
  if (host) {
    if (loo_i) PLA_HIP(hipMemcpyAsync(loo_i, dloo, (size_t)n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (agg) PLA_HIP(hipMemcpyAsync(agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
    PLA_HIP(hipStreamSynchronize(s));
  }
  return PLA_OK;
}

// ---- moment matching (loo_moment_match.py:656-914, split_moment_match.py:132-252) -----------------------------------------------
static int mm_check(pla_engine* eng, int64_t n_batch, int64_t n_draws, int64_t n_dim, bool matrices) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (n_batch < 0 || n_batch > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_batch out of range");
  if (n_draws < 2 || n_draws > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_draws must lie in [2, 2^30], got %lld", (long long)n_draws);
  if (n_dim < 1) return fail(PLA_ERR_ARG, "n_dim < 1");
  if (matrices && n_dim > pla::kMmMaxCovDim)
    return fail(PLA_ERR_UNSUPPORTED, "moment matching with covariance matrices takes at most %d parameters, got %lld", pla::kMmMaxCovDim,
                (long long)n_dim);
  if (n_dim > pla::kMmMaxDim)
    return fail(PLA_ERR_UNSUPPORTED, "moment matching takes at most %d parameters, got %lld", pla::kMmMaxDim, (long long)n_dim);
  return PLA_OK;
}

int pla_mm_moments(pla_engine* eng, const double* upars, const double* lw, int64_t n_batch, int64_t n_draws, int64_t n_dim, int want_cov,
                   void* stream, double* stats, double* cov) {
  int rc = mm_check(eng, n_batch, n_draws, n_dim, want_cov != 0);
  if (rc) return rc;
  if (n_batch > 0 && (!upars || !lw || !stats || (want_cov && !cov))) return fail(PLA_ERR_ARG, "upars, lw, stats or cov is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  if (n_batch == 0) return PLA_OK;
  rc = grow(&eng->d_mm, &eng->d_mm_bytes, (size_t)pla::mm_moments_workspace(n_batch, n_draws, (int)n_dim, want_cov) * sizeof(double));
  if (rc) return rc;
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_mm_moments(upars, lw, n_batch, n_draws, (int)n_dim, want_cov ? 1 : 0, (double*)eng->d_mm, stats, cov,
                                   eng->compare_grid, s));
  }
  eng->last_kernels = std::string("mm_sums_kernel<0> + mm_mid_kernel + mm_sums_kernel<1> + ") + (want_cov ? "mm_cov_kernel + " : "") +
                      "mm_fin_kernel";
  return PLA_OK;
}

int pla_mm_transform(pla_engine* eng, const double* x, int64_t x_batch_stride, const double* m0, const double* pre, const double* map,
                     const double* post_div, const double* m1, int64_t n_batch, int64_t n_draws, int64_t n_dim, int64_t row_lo,
                     int64_t row_hi, void* stream, double* out) {
  int rc = mm_check(eng, n_batch, n_draws, n_dim, map != nullptr);
  if (rc) return rc;
  if (n_batch > 0 && (!x || !m0 || !m1 || !out)) return fail(PLA_ERR_ARG, "x, m0, m1 or out is NULL");
  if (x_batch_stride != 0 && x_batch_stride < n_draws * n_dim) return fail(PLA_ERR_ARG, "x_batch_stride must be 0 or at least n_draws * n_dim");
  if (row_lo < 0 || row_hi > n_draws || row_lo > row_hi) return fail(PLA_ERR_ARG, "need 0 <= row_lo <= row_hi <= n_draws");
  if (x == out) return fail(PLA_ERR_ARG, "the transform does not work in place");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  if (n_batch == 0) return PLA_OK;
  pla::MmTransformParams p{x, x_batch_stride, m0, pre, map, post_div, m1, n_batch, n_draws, (int)n_dim, row_lo, row_hi, out};
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_mm_transform(p, eng->compare_grid, s));
  }
  eng->last_kernels = map ? "mm_map_kernel" : "mm_affine_kernel";
  return PLA_OK;
}

int pla_mm_ratios(pla_engine* eng, int mode, const double* a, const double* b, const double* c, const double* jac, int64_t n_batch,
                  int64_t n_draws, void* stream, double* out) {
  int rc = mm_check(eng, n_batch, n_draws, 1, false);
  if (rc) return rc;
  if (mode < 0 || mode > 3) return fail(PLA_ERR_ARG, "mode must be 0 (update), 1 (split), 2 (sum) or 3 (finish)");
  if (n_batch > 0 && (!a || !b || !out || (mode <= 1 && !c) || (mode == 1 && !jac))) return fail(PLA_ERR_ARG, "an input or out is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  if (n_batch == 0) return PLA_OK;
  pla::MmRatiosParams p{a, b, c, jac, n_batch, n_draws, out};
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_mm_ratios(mode, p, eng->compare_grid, s));
  }
  eng->last_kernels = mode == 3 ? "mm_finish_kernel" : "mm_ratios_kernel<" + std::to_string(mode) + ">";
  return PLA_OK;
}

// ---- model comparison (compare.py:205-229, 477-577) ----------------------------------------------------------------------------
static int compare_check(pla_engine* eng, const void* x, int dtype, int64_t n_models, int64_t n_obs, int64_t pitch, int mem_space) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (!x) return fail(PLA_ERR_ARG, "input pointer is NULL");
  if (n_obs < 1 || n_obs >= ((int64_t)1 << 32)) return fail(PLA_ERR_ARG, "n_obs must lie in [1, 2^32), got %lld", (long long)n_obs);
  if (n_models < 1) return fail(PLA_ERR_ARG, "n_models < 1");
  if (n_models > PLA_COMPARE_MAX_MODELS)
    return fail(PLA_ERR_UNSUPPORTED, "n_models = %lld exceeds the device limit of %d models", (long long)n_models, PLA_COMPARE_MAX_MODELS);
  if (n_models > 1 && pitch < n_obs) return fail(PLA_ERR_ARG, "pitch %lld < n_obs %lld", (long long)pitch, (long long)n_obs);
  return PLA_OK;
}

// the (K, N) matrix on the device: device pointers as they are, host matrices uploaded once into the ingest staging (C-contiguous)
static int compare_input_on_device(pla_engine* eng, const void* x, int dtype, int64_t K, int64_t N, int64_t pitch, int mem_space,
                                   hipStream_t s, const void** dx, int64_t* dpitch) {
  if (mem_space == PLA_DEVICE) {
    *dx = x;
    *dpitch = K > 1 ? pitch : N;
    return PLA_OK;
  }
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  int rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)K * (size_t)N * esz);
  if (rc) return rc;
  PLA_HIP(hipMemcpy2DAsync(eng->d_in, (size_t)N * esz, x, (size_t)(K > 1 ? pitch : N) * esz, (size_t)N * esz, (size_t)K,
                           hipMemcpyHostToDevice, s));
  *dx = eng->d_in;
  *dpitch = N;
  return PLA_OK;
}

static const char* compare_where(int mem_space) { return mem_space == PLA_DEVICE ? "(matrix read in place)" : "(matrix uploaded)"; }

int pla_engine_set_compare_grid(pla_engine* eng, int max_workgroups) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (max_workgroups < 0) return fail(PLA_ERR_ARG, "max_workgroups < 0");
  EngineCall call(eng);
  eng->compare_grid = max_workgroups;
  return PLA_OK;
}

int pla_compare_moments(pla_engine* eng, const void* x, int dtype, int64_t n_models, int64_t n_obs, int64_t pitch, int64_t best,
                        int mem_space, void* stream, double* out) {
  int rc = compare_check(eng, x, dtype, n_models, n_obs, pitch, mem_space);
  if (rc) return rc;
  if (best < 0 || best >= n_models) return fail(PLA_ERR_ARG, "best = %lld is not a model index", (long long)best);
  if (!out) return fail(PLA_ERR_ARG, "out is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const int K = (int)n_models;
  const int64_t tiles = pla::compare_n_tiles(n_obs);
  rc = grow(&eng->d_cmp, &eng->d_cmp_bytes, (size_t)tiles * (size_t)(3 * K + 2) * sizeof(double));
  if (rc) return rc;
  double* dout = out;
  if (mem_space == PLA_HOST) {
    rc = grow(&eng->d_cmp_out, &eng->d_cmp_out_bytes, (size_t)(3 * K + 1) * sizeof(double));
    if (rc) return rc;
    dout = (double*)eng->d_cmp_out;
  }
  const void* dx = nullptr;
  int64_t dp = 0;
  rc = compare_input_on_device(eng, x, dtype, K, n_obs, pitch, mem_space, s, &dx, &dp);
  if (rc) return rc;
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_compare_moments(dx, dtype, dp, K, n_obs, (int)best, (double*)eng->d_cmp, dout, eng->compare_grid, s));
  }
  eng->last_kernels = std::string("compare_moments_kernel<") + pla::dtype_name(dtype) + "> + compare_moments_final_kernel " +
                      compare_where(mem_space);
  if (mem_space == PLA_DEVICE) return PLA_OK;
  PLA_HIP(hipMemcpyAsync(out, dout, (size_t)(3 * K + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  return PLA_OK;
}

int pla_stacking_eval(pla_engine* eng, const void* x, int dtype, int64_t n_models, int64_t n_obs, int64_t pitch, double scale_mul,
                      const double* weights, int mem_space, void* stream, double* out) {
  int rc = compare_check(eng, x, dtype, n_models, n_obs, pitch, mem_space);
  if (rc) return rc;
  if (!weights || !out) return fail(PLA_ERR_ARG, "weights / out is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const int K = (int)n_models;
  const int64_t tiles = pla::compare_n_tiles(n_obs);
  rc = grow(&eng->d_cmp, &eng->d_cmp_bytes, (size_t)tiles * (size_t)(K + 1) * sizeof(double));
  if (rc) return rc;
  rc = grow(&eng->d_cmp_out, &eng->d_cmp_out_bytes, (size_t)(2 * K + 1) * sizeof(double));  // out [K + 1], then the weights
  if (rc) return rc;
  const void* dx = nullptr;
  int64_t dp = 0;
  rc = compare_input_on_device(eng, x, dtype, K, n_obs, pitch, mem_space, s, &dx, &dp);
  if (rc) return rc;
  double* dw = (double*)eng->d_cmp_out + K + 1;
  PLA_HIP(hipMemcpyAsync(dw, weights, (size_t)K * sizeof(double), hipMemcpyHostToDevice, s));
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_stacking_eval(dx, dtype, dp, K, n_obs, scale_mul, dw, (double*)eng->d_cmp, (double*)eng->d_cmp_out,
                                      eng->compare_grid, s));
  }
  eng->last_kernels = std::string("stacking_eval_kernel<") + pla::dtype_name(dtype) + "> + compare_tiles_sum_kernel " +
                      compare_where(mem_space);
  PLA_HIP(hipMemcpyAsync(out, eng->d_cmp_out, (size_t)(K + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  return PLA_OK;
}

int pla_bb_bootstrap(pla_engine* eng, const void* x, int dtype, int64_t n_models, int64_t n_obs, int64_t pitch, double scale_mul,
                     int64_t n_boot, double alpha, uint64_t seed, int mem_space, void* stream, double* z) {
  int rc = compare_check(eng, x, dtype, n_models, n_obs, pitch, mem_space);
  if (rc) return rc;
  if (n_boot < 1 || n_boot > ((int64_t)1 << 32)) return fail(PLA_ERR_ARG, "n_boot must lie in [1, 2^32], got %lld", (long long)n_boot);
  if (!(alpha > 0.0) || !std::isfinite(alpha)) return fail(PLA_ERR_ARG, "alpha must be a positive number");
  if (!z) return fail(PLA_ERR_ARG, "z is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const int K = (int)n_models;
  const int64_t tiles = pla::compare_n_tiles(n_obs);
  // replicates per launch: their partials within 64 MiB (whole blocks of 64)
  const size_t per_rep = (size_t)tiles * (size_t)(K + 1) * sizeof(double);
  int64_t nb = (int64_t)(((size_t)64 << 20) / per_rep) / 64 * 64;
  if (nb < 64) nb = 64;
  if (nb > n_boot) nb = n_boot;
  rc = grow(&eng->d_cmp, &eng->d_cmp_bytes, (size_t)nb * per_rep);
  if (rc) return rc;
  if (mem_space == PLA_HOST) {
    rc = grow(&eng->d_cmp_out, &eng->d_cmp_out_bytes, (size_t)nb * (size_t)K * sizeof(double));
    if (rc) return rc;
  }
  const void* dx = nullptr;
  int64_t dp = 0;
  rc = compare_input_on_device(eng, x, dtype, K, n_obs, pitch, mem_space, s, &dx, &dp);
  if (rc) return rc;
  for (int64_t b0 = 0; b0 < n_boot; b0 += nb) {
    const int64_t n = n_boot - b0 < nb ? n_boot - b0 : nb;
    double* zb = mem_space == PLA_DEVICE ? z + b0 * K : (double*)eng->d_cmp_out;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_bb_bootstrap(dx, dtype, dp, K, n_obs, scale_mul, seed, alpha, b0, n, (double*)eng->d_cmp, zb, eng->compare_grid,
                                       s));
    }
    if (mem_space == PLA_HOST) {
      PLA_HIP(hipMemcpyAsync(z + b0 * K, zb, (size_t)n * (size_t)K * sizeof(double), hipMemcpyDeviceToHost, s));
      PLA_HIP(hipStreamSynchronize(s));  // the buffer is reused by the next block
    }
  }
  eng->last_kernels = std::string("bb_bootstrap_kernel<") + pla::dtype_name(dtype) + "> + bb_final_kernel " + compare_where(mem_space);
  return PLA_OK;
}

int pla_bb_gamma_draws(pla_engine* eng, uint64_t seed, double alpha, int64_t n_boot, int64_t n_obs, int mem_space, void* stream,
                       double* out) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (n_boot < 1 || n_boot > ((int64_t)1 << 32) || n_obs < 1 || n_obs >= ((int64_t)1 << 32) || n_boot * n_obs > ((int64_t)1 << 31))
    return fail(PLA_ERR_ARG, "need 1 <= n_boot <= 2^32, 1 <= n_obs < 2^32 and n_boot * n_obs <= 2^31");
  if (!(alpha > 0.0) || !std::isfinite(alpha)) return fail(PLA_ERR_ARG, "alpha must be a positive number");
  if (!out) return fail(PLA_ERR_ARG, "out is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)n_boot * (size_t)n_obs * sizeof(double);
  double* d = out;
  if (mem_space == PLA_HOST) {
    int rc = grow(&eng->d_cmp_out, &eng->d_cmp_out_bytes, bytes);
    if (rc) return rc;
    d = (double*)eng->d_cmp_out;
  }
  PLA_HIP(pla::launch_bb_gamma_draws(seed, alpha, n_boot, n_obs, d, s));
  eng->last_kernels = "bb_gamma_draws_kernel";
  if (mem_space == PLA_DEVICE) return PLA_OK;
  PLA_HIP(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  return PLA_OK;
}

int pla_importance_weights(pla_engine* eng, const void* logw, int dtype, int64_t n_obs, int64_t n_draws,
                           int64_t stride_obs, int64_t stride_draw, int method, int64_t tail_count,
                           int mem_space, void* stream, void* lw_out, double* diag) {
  int rc = check_common(eng, logw, dtype, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, mem_space);
  if (rc) return rc;
  if (n_obs > 0 && !lw_out) return fail(PLA_ERR_ARG, "lw_out is NULL");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;

  pla::RowsParams p{};
  p.n_obs = n_obs;
  p.n_draws = (int)n_draws;
  p.method = method;
  p.tail_count = method == PLA_PSIS ? (int)tail_count : 0;
  p.tail_cap = pow2_at_least(p.tail_count);
  p.scale_value = 1.0;
  p.counters = eng->counters;
  PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));
  if (n_obs > 0) {  // workspace of the fast path (rows it declines, quantile tables)
    rc = grow(&eng->d_slow, &eng->d_slow_bytes, (size_t)n_obs * sizeof(unsigned));
    if (rc) return rc;
    p.slow_list = (unsigned*)eng->d_slow;
    if (method == PLA_PSIS) {
      rc = ensure_l1_table(eng, tail_count, s, &p.l1_table);
      if (rc) return rc;
    }
  }

  if (mem_space == PLA_DEVICE) {
    if (obs_fastest_device(mem_space, nullptr, n_obs, n_draws, stride_obs, stride_draw)) {
      // observations-fastest log ratios: transposed block by block like the LOO pass; the weights come out as the
      // (n_obs, n_draws) C-contiguous matrix the header promises
      const int64_t rows_per_chunk = staged_chunk_rows(mem_space, true, n_obs, n_draws, esz);
      rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows_per_chunk * (size_t)n_draws * esz);
      if (rc) return rc;
      p.in = eng->d_in;
      p.stride_obs = n_draws;
      p.stride_draw = 1;
      TimedLaunch t(eng, s);
      for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
        const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
        PLA_HIP(pla::launch_transpose_rows(logw, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in, s));
        p.n_obs = nr;
        p.diag = diag ? diag + r0 : nullptr;
        p.lw_out = (char*)lw_out + (size_t)r0 * (size_t)n_draws * esz;
        PLA_HIP(pla::launch_rows(p, dtype, true, s));
      eng->last_kernels = pla::last_rows_kernels();
      }
      return PLA_OK;
    }
    p.in = logw;
    p.stride_obs = stride_obs;
    p.stride_draw = stride_draw;
    p.diag = diag;
    p.lw_out = lw_out;
    // Rows longer than the registers (S > 4096) with tails the fit kernel takes: the split weights pass (selection kernel -> fit
    // kernel -> output kernel, csrc/pla_lwout.h) needs the hand-over buffers -- the tail's x and eight scalars per observation -- for
    // the rows of one launch, so such calls run in blocks of 2^17 observations (0.48 GB at 448-value tails).  No room: the
    // fused weights kernel, which needs none.
    int64_t block = n_obs;
    if (method == PLA_PSIS && n_draws > 4096 && tail_count <= 448 && stride_draw == 1 && n_obs > 0) {
      const int64_t kLwBlock = (int64_t)1 << 17;
      block = n_obs < kLwBlock ? n_obs : kLwBlock;
      const int stride = (int)((tail_count + 63) & ~(int64_t)63);
      rc = grow(&eng->d_ws, &eng->d_ws_bytes, (size_t)block * (size_t)(stride + 8) * sizeof(double));
      if (rc == PLA_ERR_NOMEM) {
        block = n_obs;
      } else {
        if (rc) return rc;
        p.ws_y = (double*)eng->d_ws;
        p.ws_s = p.ws_y + (size_t)block * stride;
        p.ws_stride = stride;
        p.ws_sstride = 8;
        p.lw_split = true;
      }
    }
    TimedLaunch t(eng, s);
    for (int64_t r0 = 0; r0 < n_obs || r0 == 0; r0 += block) {
      const int64_t nr = (n_obs - r0 < block) ? (n_obs - r0) : block;
      p.in = (const char*)logw + (size_t)r0 * (size_t)stride_obs * esz;
      p.n_obs = nr;
      p.diag = diag ? diag + r0 : nullptr;
      p.lw_out = (char*)lw_out + (size_t)r0 * (size_t)n_draws * esz;
      PLA_HIP(pla::launch_rows(p, dtype, true, s));
      eng->last_kernels = pla::last_rows_kernels();
      if (n_obs == 0) break;
    }
    return PLA_OK;
  }

  if (stride_draw != 1) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs stride_draw == 1 (transpose on the host)");
  const size_t row_bytes = (size_t)n_draws * esz;
  int64_t rows_per_chunk = (int64_t)(((size_t)1 << 30) / (row_bytes ? row_bytes : 1));
  if (rows_per_chunk < 1) rows_per_chunk = 1;
  if (rows_per_chunk > n_obs) rows_per_chunk = n_obs;
  if (n_obs == 0) return PLA_OK;
  rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows_per_chunk * row_bytes);
  if (rc) return rc;
  rc = grow(&eng->d_lw, &eng->d_lw_bytes, (size_t)rows_per_chunk * row_bytes);
  if (rc) return rc;
  if (method == PLA_PSIS && n_draws > 4096 && tail_count <= 448) {  // (the split weights pass of long rows, as on the device path)
    const int stride = (int)((tail_count + 63) & ~(int64_t)63);
    rc = grow(&eng->d_ws, &eng->d_ws_bytes, (size_t)rows_per_chunk * (size_t)(stride + 8) * sizeof(double));
    if (rc && rc != PLA_ERR_NOMEM) return rc;
    if (!rc) {
      p.ws_y = (double*)eng->d_ws;
      p.ws_s = p.ws_y + (size_t)rows_per_chunk * stride;
      p.ws_stride = stride;
      p.ws_sstride = 8;
      p.lw_split = true;
    }
  }
  {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(3 * n_obs + PLA_AGG_COUNT) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
  }
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    const char* src = (const char*)logw + (size_t)r0 * stride_obs * esz;
    PLA_HIP(hipMemcpy2DAsync(eng->d_in, row_bytes, src, (size_t)stride_obs * esz, row_bytes, (size_t)nr,
                             hipMemcpyHostToDevice, s));
    p.in = eng->d_in;
    p.stride_obs = n_draws;
    p.stride_draw = 1;
    p.n_obs = nr;
    p.diag = eng->d_pw + r0;
    p.lw_out = eng->d_lw;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_rows(p, dtype, true, s));
      eng->last_kernels = pla::last_rows_kernels();
    }
    PLA_HIP(hipMemcpyAsync((char*)lw_out + (size_t)r0 * row_bytes, eng->d_lw, (size_t)nr * row_bytes,
                           hipMemcpyDeviceToHost, s));
    PLA_HIP(hipStreamSynchronize(s));
  }
  if (diag) PLA_HIP(hipMemcpyAsync(diag, eng->d_pw, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  return PLA_OK;
}

// The weights pass of one block of rows for the passes that consume a block's weights before the next block overwrites them
// (pla_loo_pit, pla_loo_diag), as pla_importance_weights sets it up: every field of `p` but in / n_obs / diag / lw_out, and the
// workspace for `*rows` rows per block -- the slow list, the quantile table, the weights buffer d_lw and, for long rows, the
// hand-over buffers of the split weights route, whose inner blocks of 2^17 rows cap *rows.
static int weights_block_setup(pla_engine* eng, int method, int64_t tail_count, int64_t n_draws, size_t esz, hipStream_t s, int64_t* rows,
                               pla::RowsParams* p) {
  p->n_draws = (int)n_draws;
  p->method = method;
  p->tail_count = method == PLA_PSIS ? (int)tail_count : 0;
  p->tail_cap = pow2_at_least(p->tail_count);
  p->scale_value = 1.0;
  p->counters = eng->counters;
  p->stride_obs = n_draws;
  p->stride_draw = 1;
  const bool split = method == PLA_PSIS && n_draws > 4096 && tail_count <= 448;
  if (split && *rows > ((int64_t)1 << 17)) *rows = (int64_t)1 << 17;
  PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));
  int rc = grow(&eng->d_slow, &eng->d_slow_bytes, (size_t)*rows * sizeof(unsigned));
  if (rc) return rc;
  p->slow_list = (unsigned*)eng->d_slow;
  if (method == PLA_PSIS) {
    rc = ensure_l1_table(eng, tail_count, s, &p->l1_table);
    if (rc) return rc;
  }
  if (split) {
    const int stride = (int)((tail_count + 63) & ~(int64_t)63);
    rc = grow(&eng->d_ws, &eng->d_ws_bytes, (size_t)*rows * (size_t)(stride + 8) * sizeof(double));
    if (rc && rc != PLA_ERR_NOMEM) return rc;
    if (!rc) {  // (no room: the fused weights kernel, which needs none)
      p->ws_y = (double*)eng->d_ws;
      p->ws_s = p->ws_y + (size_t)*rows * stride;
      p->ws_stride = stride;
      p->ws_sstride = 8;
      p->lw_split = true;
    }
  }
  return grow(&eng->d_lw, &eng->d_lw_bytes, (size_t)*rows * (size_t)n_draws * esz);
}

// ---- LOO-PIT (csrc/pla_pit.h) ---------------------------------------------------------------------------------------------------
int pla_loo_pit(pla_engine* eng, const void* in, const void* y_hat, const double* y, int dtype, int64_t n_obs, int64_t n_draws,
                int64_t stride_obs, int64_t stride_draw, int64_t yh_stride_obs, int64_t yh_stride_draw, int input_kind, int method,
                int64_t tail_count, int mem_space, void* stream, double* pit_le, double* pit_lt, double* diag, int64_t* n_replaced) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (input_kind != PLA_PIT_LOGLIK && input_kind != PLA_PIT_LOG_WEIGHTS) return fail(PLA_ERR_ARG, "bad input_kind");
  if (method != PLA_PSIS && method != PLA_SIS && method != PLA_TIS) return fail(PLA_ERR_ARG, "bad method");
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (n_draws < 2 || n_draws > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_draws out of range (at least 2)");
  if (stride_obs <= 0 || stride_draw <= 0 || yh_stride_obs <= 0 || yh_stride_draw <= 0) return fail(PLA_ERR_ARG, "strides must be positive");
  if (n_obs > 0 && (!in || !y_hat || !y || !pit_le)) return fail(PLA_ERR_ARG, "in / y_hat / y / pit_le is NULL");
  const bool loglik = input_kind == PLA_PIT_LOGLIK;
  if (loglik) {
    const int rc0 = check_common(eng, in, dtype, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, mem_space);
    if (rc0) return rc0;
  }
  const bool host = mem_space == PLA_HOST;
  const bool in_of = host_obs_fastest(n_obs, n_draws, stride_obs, stride_draw);
  const bool yh_of = host_obs_fastest(n_obs, n_draws, yh_stride_obs, yh_stride_draw);
  if (host && ((stride_draw != 1 && !in_of) || (yh_stride_draw != 1 && !yh_of)))
    return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST matrices need unit stride along the draws, or along the observations");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  if (n_obs == 0) {
    if (host && n_replaced) *n_replaced = 0;
    if (!host && n_replaced) PLA_HIP(hipMemsetAsync(n_replaced, 0, sizeof(int64_t), s));
    return PLA_OK;
  }
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int S = (int)n_draws;
  char route[160], prep_text[96] = "";
  int rc;

  // ---- log weights on the device: the PIT kernel alone, both matrices in place
  if (!loglik && !host) {
    PLA_HIP(pla::launch_pit(in, y_hat, y, dtype, n_obs, S, stride_obs, stride_draw, yh_stride_obs, yh_stride_draw, pit_le, pit_lt, s,
                            route, (int)sizeof(route)));
    if (n_replaced) PLA_HIP(hipMemsetAsync(n_replaced, 0, sizeof(int64_t), s));
    eng->last_kernels = std::string(route) + " (matrices read in place)";
    return PLA_OK;
  }

  // ---- the weights pass of a block, as pla_importance_weights sets it up; rows per block: the ingest staging's size on the device,
  // 1 GiB from the host
  pla::RowsParams p{};
  int64_t rows = staged_chunk_rows(mem_space, true, n_obs, n_draws, esz);
  if (loglik) {
    rc = weights_block_setup(eng, method, tail_count, n_draws, esz, s, &rows, &p);
    if (rc) return rc;
  }
  const size_t block_bytes = (size_t)rows * (size_t)n_draws * esz;
  if (loglik || host) {
    rc = grow(&eng->d_in, &eng->d_in_bytes, block_bytes);
    if (rc) return rc;
  }
  const bool yh_transpose = host ? yh_of : obs_fastest_device(mem_space, nullptr, n_obs, n_draws, yh_stride_obs, yh_stride_draw);
  if (host || yh_transpose) {
    rc = grow(&eng->d_pit, &eng->d_pit_bytes, block_bytes);
    if (rc) return rc;
  }
  if (host && (in_of || yh_of)) {
    rc = grow(&eng->d_slab, &eng->d_slab_bytes, block_bytes);
    if (rc) return rc;
  }
  unsigned long long* d_count = nullptr;
  const double* dy = y;
  double *d_le = pit_le, *d_lt = pit_lt, *d_diag = loglik ? diag : nullptr;
  if (host) {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(4 * n_obs + PLA_AGG_COUNT) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
    PLA_HIP(hipMemcpyAsync(eng->d_pw, y, (size_t)n_obs * sizeof(double), hipMemcpyHostToDevice, s));
    dy = eng->d_pw;
    d_le = eng->d_pw + n_obs;
    d_lt = eng->d_pw + 2 * n_obs;
    d_diag = eng->d_pw + 3 * n_obs;
    d_count = eng->counters + pla::kCounterPitReplaced;
    PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  } else {
    d_count = (unsigned long long*)n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  }

  std::string label;
  const size_t row_bytes = (size_t)n_draws * esz;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    // the weights' source as a compact draws-fastest block in d_in (log-likelihood: negated, NaN -> -1e10)
    const void* lw_block = eng->d_in;
    const char* prep = "";
    if (!host) {
      PLA_HIP(pla::launch_pit_prepare((const char*)in + (size_t)r0 * (size_t)stride_obs * esz, dtype, stride_obs, stride_draw, nr, S,
                                      eng->d_in, d_count, s, &prep));
    } else if (in_of) {  // the (n_draws, nr) slab as it lies, turned on the device
      PLA_HIP(hipMemcpy2DAsync(eng->d_slab, (size_t)nr * esz, (const char*)in + (size_t)r0 * esz, (size_t)stride_draw * esz,
                               (size_t)nr * esz, (size_t)n_draws, hipMemcpyHostToDevice, s));
      if (loglik) PLA_HIP(pla::launch_pit_prepare(eng->d_slab, dtype, 1, nr, nr, S, eng->d_in, d_count, s, &prep));
      else PLA_HIP(pla::launch_transpose_rows(eng->d_slab, dtype, nr, 0, nr, S, eng->d_in, s));
    } else {
      void* up = loglik ? eng->d_lw : eng->d_in;  // (the weights buffer is free until the weights pass writes it)
      PLA_HIP(hipMemcpy2DAsync(up, row_bytes, (const char*)in + (size_t)r0 * (size_t)stride_obs * esz, (size_t)stride_obs * esz, row_bytes,
                               (size_t)nr, hipMemcpyHostToDevice, s));
      if (loglik) PLA_HIP(pla::launch_pit_prepare(eng->d_lw, dtype, n_draws, 1, nr, S, eng->d_in, d_count, s, &prep));
    }
    if (loglik) {
      p.in = eng->d_in;
      p.n_obs = nr;
      p.diag = d_diag ? d_diag + r0 : nullptr;
      p.lw_out = eng->d_lw;
      PLA_HIP(pla::launch_rows(p, dtype, true, s));
      lw_block = eng->d_lw;
    }
    // the predictive draws of the block: in place, or draws fastest in d_pit
    const void* yh_block = (const char*)y_hat + (size_t)r0 * (size_t)yh_stride_obs * esz;
    int64_t yso = yh_stride_obs, ysd = yh_stride_draw;
    if (host && yh_of) {
      PLA_HIP(hipMemcpy2DAsync(eng->d_slab, (size_t)nr * esz, (const char*)y_hat + (size_t)r0 * esz, (size_t)yh_stride_draw * esz,
                               (size_t)nr * esz, (size_t)n_draws, hipMemcpyHostToDevice, s));
      PLA_HIP(pla::launch_transpose_rows(eng->d_slab, dtype, nr, 0, nr, S, eng->d_pit, s));
    } else if (host) {
      PLA_HIP(hipMemcpy2DAsync(eng->d_pit, row_bytes, yh_block, (size_t)yh_stride_obs * esz, row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    } else if (yh_transpose) {
      PLA_HIP(pla::launch_transpose_rows(y_hat, dtype, yh_stride_draw, r0, nr, S, eng->d_pit, s));
    }
    if (host || yh_transpose) {
      yh_block = eng->d_pit;
      yso = n_draws;
      ysd = 1;
    }
    PLA_HIP(pla::launch_pit(lw_block, yh_block, dy + r0, dtype, nr, S, n_draws, 1, yso, ysd, d_le + r0, d_lt ? d_lt + r0 : nullptr, s, route,
                            (int)sizeof(route)));
    if (r0 == 0) {
      snprintf(prep_text, sizeof(prep_text), "%s", prep);
      label = std::string(prep_text[0] ? prep_text : (in_of && host ? "transpose_rows_kernel" : "rows copied")) +
              (loglik ? " -> " + std::string(pla::last_rows_kernels()) : std::string()) +
              (yh_transpose ? " + transpose_rows_kernel (y_hat)" : "") + " -> " + route +
              (host ? " (matrices staged in blocks)" : " per block of observations");
    }
    if (host) PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  eng->last_kernels = label;
  if (!host) return PLA_OK;
  PLA_HIP(hipMemcpyAsync(pit_le, d_le, (size_t)n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
  if (pit_lt) PLA_HIP(hipMemcpyAsync(pit_lt, d_lt, (size_t)n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
  if (diag && loglik) PLA_HIP(hipMemcpyAsync(diag, d_diag, (size_t)n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
  unsigned long long h = 0;
  PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

// ---- LOO diagnostics (csrc/pla_diag.h) -------------------------------------------------------------------------------------------
// pla_loo_pit's PLA_PIT_LOGLIK pipeline with the PIT kernel replaced: per block of rows, -ll (selected rows) into the ingest staging
// d_in, the weights pass of pla_importance_weights from d_in into d_lw (it reads its input const: d_in is intact behind it), then
// diag_wave_kernel on (d_lw, d_in, sign -1) before the next block overwrites either.
int pla_loo_diag(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                 const int64_t* row_index, int64_t n_rows, int method, int64_t tail_count, int mem_space, void* stream, double* diag,
                 double* elpd_i, double* ess_w, double* var_log, int64_t* n_replaced) {
  int rc = check_common(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, mem_space);
  if (rc) return rc;
  if (n_draws < 2) return fail(PLA_ERR_ARG, "n_draws out of range (at least 2)");
  if (stride_obs <= 0 || stride_draw <= 0) return fail(PLA_ERR_ARG, "strides must be positive");
  if (row_index) {
    rc = check_rows(row_index, n_rows, n_obs, mem_space);
    if (rc) return rc;
  }
  const int64_t m = row_index ? n_rows : n_obs;  // rows of this call
  const bool host = mem_space == PLA_HOST;
  const bool in_of = host_obs_fastest(n_obs, n_draws, stride_obs, stride_draw);
  if (host && stride_draw != 1 && !in_of)
    return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST matrices need unit stride along the draws, or along the observations");
  if (host && in_of && row_index)
    return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST row selection needs unit stride along the draws");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) {
    if (host && n_replaced) *n_replaced = 0;
    if (!host && n_replaced) PLA_HIP(hipMemsetAsync(n_replaced, 0, sizeof(int64_t), s));
    return PLA_OK;
  }
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int S = (int)n_draws;
  char route[160];

  // the weights pass of a block, as pla_importance_weights sets it up
  pla::RowsParams p{};
  int64_t rows = staged_chunk_rows(mem_space, true, m, n_draws, esz);
  rc = weights_block_setup(eng, method, tail_count, n_draws, esz, s, &rows, &p);
  if (rc) return rc;
  const size_t block_bytes = (size_t)rows * (size_t)n_draws * esz;
  rc = grow(&eng->d_in, &eng->d_in_bytes, block_bytes);
  if (rc) return rc;
  if (host && in_of) {
    rc = grow(&eng->d_slab, &eng->d_slab_bytes, block_bytes);
    if (rc) return rc;
  }
  unsigned long long* d_count = nullptr;
  double *d_diag = diag, *d_elpd = elpd_i, *d_ess = ess_w, *d_var = var_log;
  if (host) {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(4 * m + PLA_AGG_COUNT) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
    d_diag = eng->d_pw;
    d_elpd = eng->d_pw + m;
    d_ess = eng->d_pw + 2 * m;
    d_var = eng->d_pw + 3 * m;
    d_count = eng->counters + pla::kCounterPitReplaced;
    PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  } else {
    d_count = (unsigned long long*)n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  }

  std::string label;
  const size_t row_bytes = (size_t)n_draws * esz;
  for (int64_t r0 = 0; r0 < m; r0 += rows) {
    const int64_t nr = m - r0 < rows ? m - r0 : rows;
    const char* prep = "";
    if (!host) {
      PLA_HIP(pla::launch_diag_prepare(ll, dtype, n_obs, stride_obs, stride_draw, row_index ? row_index + r0 : nullptr, r0, nr, S, eng->d_in,
                                       d_count, s, &prep));
    } else if (in_of) {  // the (n_draws, nr) slab as it lies, turned on the device
      PLA_HIP(hipMemcpy2DAsync(eng->d_slab, (size_t)nr * esz, (const char*)ll + (size_t)r0 * esz, (size_t)stride_draw * esz,
                               (size_t)nr * esz, (size_t)n_draws, hipMemcpyHostToDevice, s));
      PLA_HIP(pla::launch_diag_prepare(eng->d_slab, dtype, nr, 1, nr, nullptr, 0, nr, S, eng->d_in, d_count, s, &prep));
    } else {  // (the weights buffer is free until the weights pass writes it)
      if (!row_index) {
        PLA_HIP(hipMemcpy2DAsync(eng->d_lw, row_bytes, (const char*)ll + (size_t)r0 * (size_t)stride_obs * esz, (size_t)stride_obs * esz,
                                 row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
      } else {
        for (int64_t i = 0; i < nr; ++i)
          PLA_HIP(hipMemcpyAsync((char*)eng->d_lw + (size_t)i * row_bytes, (const char*)ll + (size_t)row_index[r0 + i] * (size_t)stride_obs * esz,
                                 row_bytes, hipMemcpyHostToDevice, s));
      }
      PLA_HIP(pla::launch_diag_prepare(eng->d_lw, dtype, nr, n_draws, 1, nullptr, 0, nr, S, eng->d_in, d_count, s, &prep));
    }
    p.in = eng->d_in;
    p.n_obs = nr;
    p.diag = d_diag ? d_diag + r0 : nullptr;
    p.lw_out = eng->d_lw;
    PLA_HIP(pla::launch_rows(p, dtype, true, s));
    PLA_HIP(pla::launch_diag(eng->d_lw, eng->d_in, -1.0, dtype, nr, S, n_draws, 1, n_draws, 1, d_elpd ? d_elpd + r0 : nullptr,
                             d_ess ? d_ess + r0 : nullptr, d_var ? d_var + r0 : nullptr, s, route, (int)sizeof(route)));
    if (r0 == 0)
      label = std::string(prep) + " -> " + std::string(pla::last_rows_kernels()) + " -> " + route +
              (host ? " (matrix staged in blocks)" : " per block of observations");
    if (host) PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  eng->last_kernels = label;
  if (!host) return PLA_OK;
  const size_t out_bytes = (size_t)m * sizeof(double);
  if (diag) PLA_HIP(hipMemcpyAsync(diag, d_diag, out_bytes, hipMemcpyDeviceToHost, s));
  if (elpd_i) PLA_HIP(hipMemcpyAsync(elpd_i, d_elpd, out_bytes, hipMemcpyDeviceToHost, s));
  if (ess_w) PLA_HIP(hipMemcpyAsync(ess_w, d_ess, out_bytes, hipMemcpyDeviceToHost, s));
  if (var_log) PLA_HIP(hipMemcpyAsync(var_log, d_var, out_bytes, hipMemcpyDeviceToHost, s));
  unsigned long long h = 0;
  PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

// the kernel alone on caller-supplied log weights: device matrices in place, host matrices staged in blocks (lw in d_in, ll in d_lw)
int pla_loo_diag_weights(pla_engine* eng, const void* lw, const void* ll, int dtype, int64_t n_obs, int64_t n_draws,
                         int64_t lw_stride_obs, int64_t lw_stride_draw, int64_t ll_stride_obs, int64_t ll_stride_draw, int mem_space,
                         void* stream, double* elpd_i, double* ess_w, double* var_log) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (n_draws < 2 || n_draws > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_draws out of range (at least 2)");
  if (lw_stride_obs <= 0 || lw_stride_draw <= 0 || ll_stride_obs <= 0 || ll_stride_draw <= 0)
    return fail(PLA_ERR_ARG, "strides must be positive");
  if (n_obs > 0 && (!lw || !ll)) return fail(PLA_ERR_ARG, "lw / ll is NULL");
  const bool host = mem_space == PLA_HOST;
  if (host && (lw_stride_draw != 1 || ll_stride_draw != 1))
    return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST matrices need unit stride along the draws");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  if (n_obs == 0) return PLA_OK;
  const int S = (int)n_draws;
  char route[160];
  if (!host) {
    PLA_HIP(pla::launch_diag(lw, ll, 1.0, dtype, n_obs, S, lw_stride_obs, lw_stride_draw, ll_stride_obs, ll_stride_draw, elpd_i, ess_w,
                             var_log, s, route, (int)sizeof(route)));
    eng->last_kernels = std::string(route) + " (matrices read in place)";
    return PLA_OK;
  }
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int64_t rows = staged_chunk_rows(mem_space, true, n_obs, n_draws, esz);
  const size_t row_bytes = (size_t)n_draws * esz, block_bytes = (size_t)rows * row_bytes;
  int rc = grow(&eng->d_in, &eng->d_in_bytes, block_bytes);
  if (rc) return rc;
  rc = grow(&eng->d_lw, &eng->d_lw_bytes, block_bytes);
  if (rc) return rc;
  size_t have_b = eng->d_pw_elems * sizeof(double);
  rc = grow((void**)&eng->d_pw, &have_b, (size_t)(3 * n_obs + PLA_AGG_COUNT) * sizeof(double));
  eng->d_pw_elems = have_b / sizeof(double);
  if (rc) return rc;
  double *d_elpd = eng->d_pw, *d_ess = eng->d_pw + n_obs, *d_var = eng->d_pw + 2 * n_obs;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    PLA_HIP(hipMemcpy2DAsync(eng->d_in, row_bytes, (const char*)lw + (size_t)r0 * (size_t)lw_stride_obs * esz, (size_t)lw_stride_obs * esz,
                             row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    PLA_HIP(hipMemcpy2DAsync(eng->d_lw, row_bytes, (const char*)ll + (size_t)r0 * (size_t)ll_stride_obs * esz, (size_t)ll_stride_obs * esz,
                             row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    PLA_HIP(pla::launch_diag(eng->d_in, eng->d_lw, 1.0, dtype, nr, S, n_draws, 1, n_draws, 1, d_elpd + r0, d_ess + r0, d_var + r0, s, route,
                             (int)sizeof(route)));
    PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  eng->last_kernels = std::string(route) + " (matrices staged in blocks)";
  const size_t out_bytes = (size_t)n_obs * sizeof(double);
  if (elpd_i) PLA_HIP(hipMemcpyAsync(elpd_i, d_elpd, out_bytes, hipMemcpyDeviceToHost, s));
  if (ess_w) PLA_HIP(hipMemcpyAsync(ess_w, d_ess, out_bytes, hipMemcpyDeviceToHost, s));
  if (var_log) PLA_HIP(hipMemcpyAsync(var_log, d_var, out_bytes, hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  return PLA_OK;
}

// ---- leave-future-out CV (csrc/pla_lfo.h) ----------------------------------------------------------------------------------------
// One block of steps at a time -- whole chunks of the prefix sum, sized like the other staged passes -- on the caller's stream:
//   1. the log ratios of the block (f64) into the ingest staging d_in: totals, carries (continued from block to block), ratios
//   2. the weights pass of pla_importance_weights, unchanged, from d_in into d_lw
//   3. the predict kernel: d_lw against the M future rows of every step, before the next block overwrites either buffer
// The matrix is read in place when its draws are contiguous on the device; observations-fastest device matrices and host matrices
// come as blocks of nb + M - 1 rows, draws fastest, in d_pit (transposed on the device / copied).  ratios_out: pla_lfo_ratios (step 1
// alone, straight into the caller's matrix or through d_in to the host).
static int lfo_impl(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                    int64_t first, int64_t n_steps, int64_t horizon, int64_t tail_count, double k_threshold, int mem_space, void* stream,
                    double* ratios_out, double* diag, double* elpd_i, int64_t* first_high, int64_t* n_replaced) {
  const bool ratios_only = ratios_out != nullptr;
  const bool host = mem_space == PLA_HOST;
  const bool in_of = host && host_obs_fastest(n_obs, n_draws, stride_obs, stride_draw);
  const bool dev_of = obs_fastest_device(mem_space, nullptr, n_obs, n_draws, stride_obs, stride_draw);
  if (stride_draw != 1 && !in_of && !dev_of)
    return fail(PLA_ERR_UNSUPPORTED, "the matrix needs unit stride along the draws, or along the observations (stride_draw >= n_obs)");
  if (stride_draw == 1 && n_obs > 1 && stride_obs < n_draws) return fail(PLA_ERR_ARG, "stride_obs is smaller than n_draws");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int S = (int)n_draws;
  const int64_t C = pla::lfo_chunk_rows();
  const int64_t extra = ratios_only ? 0 : horizon - 1;  // rows a block needs beyond one per step
  const bool staged = host || dev_of;

  // steps per block: the staging's size in f64 ratios, whole chunks
  int64_t rows = staged_chunk_rows(mem_space, true, n_steps, n_draws, sizeof(double));
  const bool split = !ratios_only && n_draws > 4096 && tail_count <= 448;  // (the split weights route of long rows: pla_importance_weights)
  if (split && rows > ((int64_t)1 << 17)) rows = (int64_t)1 << 17;
  if (rows < n_steps) rows = rows / C * C < C ? C : rows / C * C;
  if (rows > n_steps) rows = n_steps;
  const int64_t chunks = (rows + C - 1) / C;
  const size_t block_bytes = (size_t)rows * (size_t)n_draws * sizeof(double);
  int rc = grow(&eng->d_lfo, &eng->d_lfo_bytes, (size_t)(chunks + 1) * (size_t)n_draws * sizeof(double));
  if (rc) return rc;
  double* run = (double*)eng->d_lfo;
  double* carry = run + n_draws;
  if (!ratios_only || host) {
    rc = grow(&eng->d_in, &eng->d_in_bytes, block_bytes);
    if (rc) return rc;
  }
  if (staged) {
    const size_t stage_bytes = (size_t)(rows + extra) * (size_t)n_draws * esz;
    rc = grow(&eng->d_pit, &eng->d_pit_bytes, stage_bytes);
    if (rc) return rc;
    if (in_of) {
      rc = grow(&eng->d_slab, &eng->d_slab_bytes, stage_bytes);
      if (rc) return rc;
    }
  }
  pla::RowsParams p{};
  if (!ratios_only) {
    p.n_draws = S;
    p.method = PLA_PSIS;
    p.tail_count = (int)tail_count;
    p.tail_cap = pow2_at_least(p.tail_count);
    p.scale_value = 1.0;
    p.counters = eng->counters;
    p.stride_obs = n_draws;
    p.stride_draw = 1;
    PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));
    rc = grow(&eng->d_slow, &eng->d_slow_bytes, (size_t)rows * sizeof(unsigned));
    if (rc) return rc;
    p.slow_list = (unsigned*)eng->d_slow;
    rc = ensure_l1_table(eng, tail_count, s, &p.l1_table);
    if (rc) return rc;
    if (split) {
      const int stride = (int)((tail_count + 63) & ~(int64_t)63);
      rc = grow(&eng->d_ws, &eng->d_ws_bytes, (size_t)rows * (size_t)(stride + 8) * sizeof(double));
      if (rc && rc != PLA_ERR_NOMEM) return rc;
      if (!rc) {  // (no room: the fused weights kernel, which needs none)
        p.ws_y = (double*)eng->d_ws;
        p.ws_s = p.ws_y + (size_t)rows * stride;
        p.ws_stride = stride;
        p.ws_sstride = 8;
        p.lw_split = true;
      }
    }
    rc = grow(&eng->d_lw, &eng->d_lw_bytes, block_bytes);
    if (rc) return rc;
  }
  // outputs: the caller's device arrays, or engine memory (a host call; k when the caller wants first_high without it)
  double *d_diag = diag, *d_elpd = elpd_i;
  unsigned long long* d_count = (unsigned long long*)n_replaced;
  long long* d_high = (long long*)first_high;
  if (host) {
    d_count = eng->counters + pla::kCounterLfoReplaced;
    d_high = (long long*)(eng->counters + pla::kCounterLfoFirstHigh);
  }
  if (!ratios_only && (host || (!diag && first_high))) {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(2 * n_steps + PLA_AGG_COUNT) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
    d_diag = eng->d_pw;
    if (host) d_elpd = eng->d_pw + n_steps;
  }
  if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  PLA_HIP(hipMemsetAsync(run, 0, (size_t)n_draws * sizeof(double), s));

  std::string label;
  char route[160];
  const size_t row_bytes = (size_t)n_draws * esz;
  for (int64_t j0 = 0; j0 < n_steps; j0 += rows) {
    const int64_t nb = n_steps - j0 < rows ? n_steps - j0 : rows;
    const bool last = j0 + nb == n_steps;
    const int64_t r0 = first + j0;  // the row of the block's first step
    int64_t n_stage = nb + extra;   // rows of the matrix the block touches (the ratios of the last block stop one row short)
    if (n_stage > n_obs - r0) n_stage = n_obs - r0;
    const void* blk = (const char*)ll + (size_t)r0 * (size_t)stride_obs * esz;
    int64_t blk_so = stride_obs;
    if (staged && n_stage > 0) {
      if (dev_of) {
        PLA_HIP(pla::launch_transpose_rows(ll, dtype, stride_draw, r0, n_stage, S, eng->d_pit, s));
      } else if (in_of) {  // the (n_draws, n_stage) slab as it lies, turned on the device
        PLA_HIP(hipMemcpy2DAsync(eng->d_slab, (size_t)n_stage * esz, (const char*)ll + (size_t)r0 * esz, (size_t)stride_draw * esz,
                                 (size_t)n_stage * esz, (size_t)n_draws, hipMemcpyHostToDevice, s));
        PLA_HIP(pla::launch_transpose_rows(eng->d_slab, dtype, n_stage, 0, n_stage, S, eng->d_pit, s));
      } else {
        PLA_HIP(hipMemcpy2DAsync(eng->d_pit, row_bytes, blk, (size_t)stride_obs * esz, row_bytes, (size_t)n_stage, hipMemcpyHostToDevice, s));
      }
    }
    if (staged) {
      blk = eng->d_pit;
      blk_so = n_draws;
    }
    double* lr = (ratios_only && !host) ? ratios_out + (size_t)j0 * (size_t)n_draws : (double*)eng->d_in;
    const char* scan = "";
    PLA_HIP(pla::launch_lfo_ratios(blk, dtype, blk_so, S, nb, last ? nb - 1 : nb, last, carry, run, lr, ratios_only ? d_count : nullptr, s,
                                   &scan));
    if (ratios_only) {
      if (j0 == 0) label = std::string(scan) + " + lfo_carry_kernel";
      if (host) {
        PLA_HIP(hipMemcpyAsync(ratios_out + (size_t)j0 * (size_t)n_draws, lr, (size_t)nb * (size_t)n_draws * sizeof(double),
                               hipMemcpyDeviceToHost, s));
        PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
      }
      continue;
    }
    p.in = lr;
    p.n_obs = nb;
    p.diag = d_diag ? d_diag + j0 : nullptr;
    p.lw_out = eng->d_lw;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_rows(p, PLA_F64, true, s));
    }
    PLA_HIP(pla::launch_lfo_predict((const double*)eng->d_lw, blk, dtype, blk_so, nb, S, (int)horizon, j0 == 0, d_diag ? d_diag + j0 : nullptr,
                                    d_elpd ? d_elpd + j0 : nullptr, d_count, s, route, (int)sizeof(route)));
    if (j0 == 0)
      label = std::string(dev_of ? "transpose_rows_kernel -> " : "") + scan + " + lfo_carry_kernel -> " + pla::last_rows_kernels() + " -> " +
              route + (host ? " (matrix staged in blocks)" : " per block of steps");
    if (host) PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  eng->last_kernels = label;
  if (!ratios_only && d_high) PLA_HIP(pla::launch_lfo_first_high(d_diag, n_steps, k_threshold, d_high, s));
  if (!host) return PLA_OK;
  if (diag) PLA_HIP(hipMemcpyAsync(diag, d_diag, (size_t)n_steps * sizeof(double), hipMemcpyDeviceToHost, s));
  if (elpd_i) PLA_HIP(hipMemcpyAsync(elpd_i, d_elpd, (size_t)n_steps * sizeof(double), hipMemcpyDeviceToHost, s));
  unsigned long long h_count = 0;
  long long h_high = n_steps;
  PLA_HIP(hipMemcpyAsync(&h_count, d_count, sizeof(h_count), hipMemcpyDeviceToHost, s));
  if (!ratios_only) PLA_HIP(hipMemcpyAsync(&h_high, d_high, sizeof(h_high), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h_count;
  if (first_high) *first_high = (int64_t)h_high;
  return PLA_OK;
}

static int lfo_check(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                     int64_t first, int64_t n_steps, int64_t last_row_margin, int mem_space) {
  // (the engine last: an argument error is reported as such with or without one)
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (n_obs < 1) return fail(PLA_ERR_ARG, "n_obs < 1");
  if (n_draws < 2 || n_draws > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_draws out of range (at least 2)");
  if (stride_obs <= 0 || stride_draw <= 0) return fail(PLA_ERR_ARG, "strides must be positive");
  if (!ll) return fail(PLA_ERR_ARG, "ll is NULL");
  if (first < 0 || first > n_obs) return fail(PLA_ERR_ARG, "first out of range (0 .. n_obs)");
  if (n_steps < 1 || n_steps > n_obs - first - last_row_margin + 1)
    return fail(PLA_ERR_ARG, "n_steps out of range: 1 .. %lld for n_obs %lld, first %lld", (long long)(n_obs - first - last_row_margin + 1),
                (long long)n_obs, (long long)first);
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  return PLA_OK;
}

int pla_lfo_ratios(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                   int64_t first, int64_t n_steps, int mem_space, void* stream, double* out, int64_t* n_replaced) {
  // (step j needs rows first .. first + j - 1: n_steps <= n_obs - first + 1)
  if (!out) return fail(PLA_ERR_ARG, "out is NULL");
  const int rc = lfo_check(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, first, n_steps, 0, mem_space);
  if (rc) return rc;
  return lfo_impl(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, first, n_steps, 1, 0, 0.0, mem_space, stream, out, nullptr, nullptr,
                  nullptr, n_replaced);
}

int pla_lfo(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw, int64_t first,
            int64_t n_steps, int64_t horizon, int method, int64_t tail_count, double k_threshold, int mem_space, void* stream, double* diag,
            double* elpd_i, int64_t* first_high, int64_t* n_replaced) {
  if (method != PLA_PSIS && method != PLA_SIS && method != PLA_TIS) return fail(PLA_ERR_ARG, "bad method");
  if (method != PLA_PSIS) return fail(PLA_ERR_UNSUPPORTED, "method: leave-future-out CV takes PLA_PSIS only");
  if (horizon < 1) return fail(PLA_ERR_ARG, "horizon < 1");
  if (k_threshold != k_threshold) return fail(PLA_ERR_ARG, "k_threshold is NaN");
  int rc = lfo_check(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, first, n_steps, horizon, mem_space);
  if (rc) return rc;
  rc = check_common(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, mem_space);
  if (rc) return rc;
  return lfo_impl(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, first, n_steps, horizon, tail_count, k_threshold, mem_space, stream,
                  nullptr, diag, elpd_i, first_high, n_replaced);
}

// ---- relative MCMC efficiency (csrc/pla_ess.h) -----------------------------------------------------------------------------------
// One kernel per block of observations on the caller's stream.  Draws-fastest device matrices are read in place in one launch;
// observations-fastest ones are transposed block by block into the ingest staging d_in, host matrices are uploaded into it (and
// transposed there when their observations are fastest) -- the same kernel then runs on the staged block.
int pla_engine_set_ess_grid(pla_engine* eng, int max_workgroups) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (max_workgroups < 0) return fail(PLA_ERR_ARG, "max_workgroups < 0");
  EngineCall call(eng);
  eng->ess_grid = max_workgroups;
  return PLA_OK;
}

int pla_ess_lds_max_draws(void) { return pla::ess_lds_max_draws(); }

int pla_relative_eff(pla_engine* eng, const void* x, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                     int64_t n_chains, int flags, int mem_space, void* stream, double* r_eff, int64_t* n_invalid) {
  // (the engine last: an argument error is reported as such with or without one)
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (n_obs < 1) return fail(PLA_ERR_ARG, "n_obs < 1");
  if (n_draws < 1 || n_draws > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_draws out of range");
  if (stride_obs <= 0 || stride_draw <= 0) return fail(PLA_ERR_ARG, "strides must be positive");
  if (flags & ~(PLA_ESS_LOG | PLA_ESS_SPLIT | PLA_ESS_CAP)) return fail(PLA_ERR_ARG, "unknown bits in flags");
  if (n_chains < 1 || n_draws % n_chains != 0)
    return fail(PLA_ERR_ARG, "n_chains = %lld does not divide n_draws = %lld", (long long)n_chains, (long long)n_draws);
  const bool split = (flags & PLA_ESS_SPLIT) != 0;
  const int64_t n_src = n_draws / n_chains;
  const int64_t n = split ? n_src / 2 : n_src;
  if (n < 4) return fail(PLA_ERR_ARG, "a chain has %lld draws%s: at least 4 are needed", (long long)n, split ? " after the split" : "");
  if (!x) return fail(PLA_ERR_ARG, "x is NULL");
  if (!r_eff) return fail(PLA_ERR_ARG, "r_eff is NULL");
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  const bool host = mem_space == PLA_HOST;
  const bool in_of = host && host_obs_fastest(n_obs, n_draws, stride_obs, stride_draw);
  const bool dev_of = obs_fastest_device(mem_space, nullptr, n_obs, n_draws, stride_obs, stride_draw);
  if (stride_draw != 1 && !in_of && !dev_of)
    return fail(PLA_ERR_UNSUPPORTED, "the matrix needs unit stride along the draws, or along the observations (stride_draw >= n_obs)");
  if (stride_draw == 1 && n_obs > 1 && stride_obs < n_draws) return fail(PLA_ERR_ARG, "stride_obs is smaller than n_draws");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const size_t row_bytes = (size_t)n_draws * esz;
  const bool staged = host || dev_of;
  const int64_t rows = staged ? staged_chunk_rows(mem_space, true, n_obs, n_draws, esz) : n_obs;
  const int64_t analysed = (split ? 2 * n_chains : n_chains) * n;
  int rc;
  double* ws = nullptr;
  if (analysed > pla::ess_lds_max_draws()) {
    const int64_t slots = pla::ess_grid_for(rows, analysed, eng->ess_grid);
    rc = grow(&eng->d_ess, &eng->d_ess_bytes, (size_t)slots * (size_t)analysed * sizeof(double));
    if (rc) return rc;
    ws = (double*)eng->d_ess;
  }
  if (staged) {
    rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows * row_bytes);
    if (rc) return rc;
  }
  double* d_out = r_eff;
  unsigned long long* d_count = (unsigned long long*)n_invalid;
  if (host) {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(n_obs + PLA_AGG_COUNT) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
    d_out = eng->d_pw;
    d_count = eng->counters + pla::kCounterEssInvalid;
  }
  if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  char route[96];
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    const void* blk = x;
    int64_t blk_so = stride_obs;
    if (host) {
      rc = stage_rows(eng, x, nullptr, r0, nr, stride_obs, esz, row_bytes, s, stride_draw, dtype, rows);
      if (rc) return rc;
    } else if (dev_of) {
      PLA_HIP(pla::launch_transpose_rows(x, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in, s));
    }
    if (staged) {
      blk = eng->d_in;
      blk_so = n_draws;
    }
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_ess(blk, dtype, blk_so, nr, (int)n_chains, (int)n_src, split ? 1 : 0, (flags & PLA_ESS_LOG) ? 1 : 0,
                              (flags & PLA_ESS_CAP) ? 1 : 0, ws, eng->ess_grid, d_out + r0, d_count, s, route, (int)sizeof(route)));
    }
    if (r0 == 0)
      eng->last_kernels = std::string(dev_of || in_of ? "transpose_rows_kernel -> " : "") + route +
                          (host ? " (matrix staged in blocks)" : dev_of ? " per block of observations" : "");
    if (host) PLA_HIP(hipStreamSynchronize(s));  // the staging buffer is reused by the next block
  }
  if (!host) return PLA_OK;
  unsigned long long h_count = 0;
  PLA_HIP(hipMemcpyAsync(r_eff, d_out, (size_t)n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipMemcpyAsync(&h_count, d_count, sizeof(h_count), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_invalid) *n_invalid = (int64_t)h_count;
  return PLA_OK;
}

static int waic_impl(pla_engine* eng, const void* ll, int dtype, int64_t n_src, const int64_t* row_index, int64_t n_obs,
                     int64_t n_draws, int64_t stride_obs, int64_t stride_draw, double scale_value, int mem_space, void* stream,
                     double* lppd_i, double* var_i, double* waic_i, double* agg) {
  int rc = check_common(eng, ll, dtype, n_src, n_draws, stride_obs, stride_draw, PLA_SIS, 0, mem_space);
  if (rc) return rc;
  if (row_index || n_obs != n_src) {
    rc = check_rows(row_index, n_obs, n_src, mem_space);
    if (rc) return rc;
  }
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));  // [1]: replaced entries
  eng->last_kernels.clear();  // (no observations: nothing is launched)

  if (mem_space == PLA_DEVICE) {
    double *dl = lppd_i, *dv = var_i, *dw = waic_i;
    if (agg && (!dv || !dw)) {  // the aggregates need var_i and waic_i: engine scratch when not asked for
      size_t have_b = eng->d_pw_elems * sizeof(double);
      rc = grow((void**)&eng->d_pw, &have_b, (size_t)(3 * n_obs + PLA_AGG_COUNT) * sizeof(double));
      eng->d_pw_elems = have_b / sizeof(double);
      if (rc) return rc;
      if (!dv) dv = eng->d_pw;
      if (!dw) dw = eng->d_pw + n_obs;
    }
    static const bool force_transpose = getenv("PLA_INGEST_TRANSPOSE") && atoi(getenv("PLA_INGEST_TRANSPOSE")) != 0;
    if (obs_fastest_device(mem_space, row_index, n_src, n_draws, stride_obs, stride_draw) && !force_transpose) {
      // observations-fastest matrix, read in place: one lane per observation (pla_waic.h)
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_waic_col(ll, dtype, n_obs, (int)n_draws, stride_draw, scale_value, dl, dv, dw, eng->counters + 1, s));
      eng->last_kernels = pla::last_rows_kernels();
    } else if (obs_fastest_device(mem_space, row_index, n_src, n_draws, stride_obs, stride_draw)) {
      const int64_t rows_per_chunk = staged_chunk_rows(mem_space, true, n_obs, n_draws, esz);
      rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows_per_chunk * (size_t)n_draws * esz);
      if (rc) return rc;
      for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
        const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
        TimedLaunch t(eng, s);
        PLA_HIP(pla::launch_transpose_rows(ll, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in, s));
        PLA_HIP(pla::launch_waic(eng->d_in, nullptr, dtype, nr, (int)n_draws, n_draws, 1, scale_value, dl ? dl + r0 : nullptr,
                                 dv ? dv + r0 : nullptr, dw ? dw + r0 : nullptr, eng->counters + 1, s));
        eng->last_kernels = std::string("transpose_rows_kernel + ") + pla::last_rows_kernels();
      }
    } else {
      TimedLaunch t(eng, s);
      const int64_t* rows_d = nullptr;
      if (row_index) {
        rc = device_rows(eng, row_index, n_obs, n_src, s, &rows_d);
        if (rc) return rc;
      }
      PLA_HIP(pla::launch_waic(ll, rows_d, dtype, n_obs, (int)n_draws, stride_obs, stride_draw, scale_value, dl, dv, dw,
                               eng->counters + 1, s));
      eng->last_kernels = pla::last_rows_kernels();
    }
    if (agg) {
      pla::ReduceParams rp{dv, dw, dv, n_obs, 0.4, agg, eng->counters + 1};  // waic.py:147 threshold
      PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
    }
    return PLA_OK;
  }

  if (stride_draw != 1 && !(stride_obs == 1 && stride_draw >= n_src && !row_index))
    return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs unit stride along the draws, or along the observations without a "
                                     "row selection");
  {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(3 * n_obs + PLA_AGG_COUNT) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
  }
  double* dl = eng->d_pw;
  double* dv = eng->d_pw + n_obs;
  double* dw = eng->d_pw + 2 * n_obs;
  double* dagg = eng->d_pw + 3 * n_obs;
  const size_t row_bytes = (size_t)n_draws * esz;
  int64_t rows_per_chunk = (int64_t)(((size_t)1 << 30) / (row_bytes ? row_bytes : 1));
  if (rows_per_chunk < 1) rows_per_chunk = 1;
  if (rows_per_chunk > n_obs) rows_per_chunk = n_obs;
  if (n_obs > 0) {
    rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows_per_chunk * row_bytes);
    if (rc) return rc;
  }
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    rc = stage_rows(eng, ll, row_index, r0, nr, stride_obs, esz, row_bytes, s, stride_draw, dtype, rows_per_chunk);
    if (rc) return rc;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_waic(eng->d_in, nullptr, dtype, nr, (int)n_draws, n_draws, 1, scale_value, dl + r0, dv + r0, dw + r0,
                               eng->counters + 1, s));
      eng->last_kernels = std::string(pla::last_rows_kernels()) + " (blocks of observations uploaded)";
    }
    PLA_HIP(hipStreamSynchronize(s));  // the staging buffer is reused by the next chunk
  }
  if (n_obs > 0) {
    if (lppd_i) PLA_HIP(hipMemcpyAsync(lppd_i, dl, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (var_i) PLA_HIP(hipMemcpyAsync(var_i, dv, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (waic_i) PLA_HIP(hipMemcpyAsync(waic_i, dw, n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (agg) {
    pla::ReduceParams rp{dv, dw, dv, n_obs, 0.4, dagg, eng->counters + 1};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
    PLA_HIP(hipMemcpyAsync(agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  PLA_HIP(hipStreamSynchronize(s));
  return PLA_OK;
}

int pla_waic(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
             int64_t stride_draw, double scale_value, int mem_space, void* stream, double* lppd_i, double* var_i,
             double* waic_i, double* agg) {
  return waic_impl(eng, ll, dtype, n_obs, nullptr, n_obs, n_draws, stride_obs, stride_draw, scale_value, mem_space, stream,
                   lppd_i, var_i, waic_i, agg);
}

int pla_waic_rows(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                  int64_t stride_draw, const int64_t* row_index, int64_t n_rows, double scale_value, int mem_space,
                  void* stream, double* lppd_i, double* var_i, double* waic_i, double* agg) {
  if (n_rows > 0 && !row_index) return fail(PLA_ERR_ARG, "row_index is NULL");
  return waic_impl(eng, ll, dtype, n_obs, row_index, n_rows, n_draws, stride_obs, stride_draw, scale_value, mem_space, stream,
                   lppd_i, var_i, waic_i, agg);
}

int pla_e_loo(pla_engine* eng, const void* x, const void* log_weights, const void* log_ratios, int dtype, int64_t n_obs,
              int64_t n_draws, int64_t stride_obs, int64_t stride_draw, int64_t tail_len, int mem_space, void* stream, double* mean,
              double* variance, double* k_mean, double* k_var, double* k_ratio) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (n_obs > 0 && (!x || !log_weights)) return fail(PLA_ERR_ARG, "x / log_weights is NULL");
  if (n_draws < 1 || n_draws > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_draws out of range");
  if (stride_draw <= 0 || stride_obs < 0) return fail(PLA_ERR_ARG, "bad strides");
  if (tail_len < 5) return fail(PLA_ERR_ARG, "tail_len must be at least 5");  // e_loo.py:298-299
  if (n_obs == 0) return PLA_OK;
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  // (row list of the one-pass wave kernel: the rows it leaves to the general one)
  if (int rc0 = grow(&eng->d_slow, &eng->d_slow_bytes, (size_t)n_obs * sizeof(unsigned))) return rc0;
  if (mem_space == PLA_DEVICE) {
    PLA_HIP(pla::launch_e_loo(x, log_weights, log_ratios, dtype, n_obs, (int)n_draws, stride_obs, stride_draw, (int)tail_len, mean,
                              variance, k_mean, k_var, k_ratio, (unsigned*)eng->d_slow, eng->counters, s));
    eng->last_kernels = pla::last_rows_kernels();
    return PLA_OK;
  }
  // ---- PLA_HOST: row blocks of the two or three matrices through the staging buffers (d_in: x, d_lw: log-weights, d_slab: ratios)
  if (stride_draw != 1) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs stride_draw == 1");
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const size_t row_bytes = (size_t)n_draws * esz;
  int64_t rows_per_chunk = (int64_t)(((size_t)1 << 29) / row_bytes);
  if (rows_per_chunk < 1) rows_per_chunk = 1;
  if (rows_per_chunk > n_obs) rows_per_chunk = n_obs;
  int rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows_per_chunk * row_bytes);
  if (!rc) rc = grow(&eng->d_lw, &eng->d_lw_bytes, (size_t)rows_per_chunk * row_bytes);
  if (!rc && log_ratios) rc = grow(&eng->d_slab, &eng->d_slab_bytes, (size_t)rows_per_chunk * row_bytes);
  if (rc) return rc;
  {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(5 * rows_per_chunk) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
  }
  double* out[5] = {mean, variance, k_mean, k_var, k_ratio};
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    const size_t off = (size_t)r0 * stride_obs * esz, pitch = (size_t)stride_obs * esz;
    PLA_HIP(hipMemcpy2DAsync(eng->d_in, row_bytes, (const char*)x + off, pitch, row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    PLA_HIP(hipMemcpy2DAsync(eng->d_lw, row_bytes, (const char*)log_weights + off, pitch, row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    if (log_ratios)
      PLA_HIP(hipMemcpy2DAsync(eng->d_slab, row_bytes, (const char*)log_ratios + off, pitch, row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    double* d = eng->d_pw;
    PLA_HIP(pla::launch_e_loo(eng->d_in, eng->d_lw, log_ratios ? eng->d_slab : nullptr, dtype, nr, (int)n_draws, n_draws, 1, (int)tail_len,
                              d, d + nr, d + 2 * nr, d + 3 * nr, d + 4 * nr, (unsigned*)eng->d_slow, eng->counters, s));
    eng->last_kernels = pla::last_rows_kernels();
    for (int k = 0; k < 5; ++k)
      if (out[k]) PLA_HIP(hipMemcpyAsync(out[k] + r0, d + k * nr, (size_t)nr * sizeof(double), hipMemcpyDeviceToHost, s));
    PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  return PLA_OK;
}

int pla_e_loo_quantiles(pla_engine* eng, const void* x, const void* log_weights, int dtype, int64_t n_obs, int64_t n_draws,
                        int64_t stride_obs, int64_t stride_draw, const double* probs, int64_t n_probs, int mem_space, void* stream,
                        double* out) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (n_obs < 0 || n_probs < 0) return fail(PLA_ERR_ARG, "negative size");
  if (n_obs > 0 && (!x || !log_weights)) return fail(PLA_ERR_ARG, "x / log_weights is NULL");
  if (n_obs > 0 && n_probs > 0 && (!probs || !out)) return fail(PLA_ERR_ARG, "probs / out is NULL");
  if (n_draws < 1 || n_draws > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_draws out of range");
  if (stride_draw <= 0 || stride_obs < 0) return fail(PLA_ERR_ARG, "bad strides");
  for (int64_t i = 0; i < n_probs; ++i)
    if (!(probs[i] > 0.0 && probs[i] < 1.0)) return fail(PLA_ERR_ARG, "probs must be between 0 and 1");  // e_loo.py:158-159
  if (n_obs == 0 || n_probs == 0) return PLA_OK;
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  int rc = grow(&eng->d_probs, &eng->d_probs_bytes, (size_t)n_probs * sizeof(double));
  if (rc) return rc;
  PLA_HIP(hipMemcpyAsync(eng->d_probs, probs, (size_t)n_probs * sizeof(double), hipMemcpyHostToDevice, s));
  PLA_HIP(hipStreamSynchronize(s));  // (the caller's probs array may go away after the call)
  const double* dp = (const double*)eng->d_probs;
  if (mem_space == PLA_DEVICE) {
    rc = grow(&eng->d_slow, &eng->d_slow_bytes, (size_t)n_obs * sizeof(unsigned));
    if (rc) return rc;
    PLA_HIP(pla::launch_e_loo_quantiles(x, log_weights, dtype, n_obs, (int)n_draws, stride_obs, stride_draw, dp, (int)n_probs, out,
                                        (unsigned*)eng->d_slow, eng->counters, s));
    eng->last_kernels = pla::last_rows_kernels();
    return PLA_OK;
  }
  if (stride_draw != 1) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs stride_draw == 1");
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const size_t row_bytes = (size_t)n_draws * esz;
  int64_t rows_per_chunk = (int64_t)(((size_t)1 << 29) / row_bytes);
  if (rows_per_chunk < 1) rows_per_chunk = 1;
  if (rows_per_chunk > n_obs) rows_per_chunk = n_obs;
  rc = grow(&eng->d_in, &eng->d_in_bytes, (size_t)rows_per_chunk * row_bytes);
  if (!rc) rc = grow(&eng->d_lw, &eng->d_lw_bytes, (size_t)rows_per_chunk * row_bytes);
  if (rc) return rc;
  {
    size_t have_b = eng->d_pw_elems * sizeof(double);
    rc = grow((void**)&eng->d_pw, &have_b, (size_t)(rows_per_chunk * n_probs) * sizeof(double));
    eng->d_pw_elems = have_b / sizeof(double);
    if (rc) return rc;
  }
  rc = grow(&eng->d_slow, &eng->d_slow_bytes, (size_t)rows_per_chunk * sizeof(unsigned));
  if (rc) return rc;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    const size_t off = (size_t)r0 * stride_obs * esz, pitch = (size_t)stride_obs * esz;
    PLA_HIP(hipMemcpy2DAsync(eng->d_in, row_bytes, (const char*)x + off, pitch, row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    PLA_HIP(hipMemcpy2DAsync(eng->d_lw, row_bytes, (const char*)log_weights + off, pitch, row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    PLA_HIP(pla::launch_e_loo_quantiles(eng->d_in, eng->d_lw, dtype, nr, (int)n_draws, n_draws, 1, dp, (int)n_probs, eng->d_pw,
                                        (unsigned*)eng->d_slow, eng->counters, s));
    eng->last_kernels = pla::last_rows_kernels();
    PLA_HIP(hipMemcpyAsync(out + r0 * n_probs, eng->d_pw, (size_t)(nr * n_probs) * sizeof(double), hipMemcpyDeviceToHost, s));
    PLA_HIP(hipStreamSynchronize(s));
  }
  return PLA_OK;
}

int pla_fill_synthetic_chains(pla_engine* eng, void* ll_device, int dtype, int64_t n_obs, int64_t n_draws, int64_t row0,
                              uint64_t seed, int chains, double rho, double offset_sd, double k_lo, double k_hi, void* stream) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (n_obs < 0 || n_draws < 1) return fail(PLA_ERR_ARG, "bad shape");
  if (chains < 1 || chains > n_draws) return fail(PLA_ERR_ARG, "need 1 <= chains <= n_draws");
  if (!(rho > -1.0 && rho < 1.0) || !(offset_sd >= 0.0)) return fail(PLA_ERR_ARG, "need |rho| < 1 and offset_sd >= 0");
  if (n_obs > 0 && !ll_device) return fail(PLA_ERR_ARG, "ll_device is NULL");
  EngineCall call(eng);
  PLA_HIP(hipSetDevice(eng->device));
  PLA_HIP(pla::launch_fill_chains(ll_device, dtype, n_obs, n_draws, chains, rho, offset_sd, row0, seed, k_lo, k_hi, (hipStream_t)stream));
  return PLA_OK;
}

int pla_fill_synthetic(pla_engine* eng, void* ll_device, int dtype, int64_t n_obs, int64_t n_draws, int64_t row0,
                       uint64_t seed, double k_lo, double k_hi, double heavy_lo, double heavy_hi, void* stream) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (n_obs < 0 || n_draws < 1) return fail(PLA_ERR_ARG, "bad shape");
  if (n_obs > 0 && !ll_device) return fail(PLA_ERR_ARG, "ll_device is NULL");
  EngineCall call(eng);
  PLA_HIP(hipSetDevice(eng->device));
  PLA_HIP(pla::launch_fill_synthetic(ll_device, dtype, n_obs, n_draws, row0, seed, k_lo, k_hi, heavy_lo, heavy_hi,
                                     (hipStream_t)stream));
  return PLA_OK;
}


// ---- non-factorised LOO (loo_nonfactor.py:466-557) -------------------------------------------------------------------------------
int pla_nonfactor_lds_max_obs(void) { return pla::nonfactor_lds_max_obs(); }

int pla_engine_set_nonfactor_route(pla_engine* eng, int route) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (route < PLA_NF_ROUTE_AUTO || route > PLA_NF_ROUTE_GENERAL) return fail(PLA_ERR_ARG, "route must be 0 .. 3, got %d", route);
  EngineCall call(eng);
  eng->nonfactor_route = route;
  return PLA_OK;
}

int pla_engine_set_nonfactor_grid(pla_engine* eng, int max_workgroups) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (max_workgroups < 0) return fail(PLA_ERR_ARG, "max_workgroups < 0");
  EngineCall call(eng);
  eng->nonfactor_grid = max_workgroups;
  return PLA_OK;
}

// draws per staging block of a host call: PLA_INGEST_BLOCK_MB (default 1 GiB) of matrices
static int64_t nonfactor_block_draws(int64_t n_obs, int64_t n_draws, size_t esz) {
  static const size_t bytes = [] {
    const char* e = getenv("PLA_INGEST_BLOCK_MB");
    const long mb = e ? atol(e) : 0;
    return mb > 0 ? (size_t)mb << 20 : (size_t)1 << 30;
  }();
  int64_t r = (int64_t)(bytes / ((size_t)n_obs * (size_t)n_obs * esz));
  if (r < 1) r = 1;
  return r < n_draws ? r : n_draws;
}

// slots of the blocked and general routes: the engine's cap, else up to 512 within 1 GiB
static int nonfactor_slots(int64_t n_obs, int64_t n_draws, int grid_cap) {
  int64_t slots = (int64_t)(((size_t)1 << 30) / ((size_t)pla::nonfactor_slot_doubles((int)n_obs) * sizeof(double)));
  if (slots > 512) slots = 512;
  if (grid_cap > 0 && slots > grid_cap) slots = grid_cap;
  if (slots > n_draws) slots = n_draws;
  return (int)(slots < 1 ? 1 : slots);
}

int pla_nonfactor_loglik(pla_engine* eng, const void* y, const void* mu, const void* mat, const void* df, int dtype, int64_t n_obs,
                         int64_t n_draws, int64_t mu_pitch, int64_t mat_pitch, int model_type, int mem_space, void* stream,
                         double* out_ll, int64_t ll_stride_obs, int64_t ll_stride_draw, int32_t* flags) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (model_type != PLA_MVN_NORMAL && model_type != PLA_MVN_STUDENT_T) return fail(PLA_ERR_ARG, "bad model_type %d", model_type);
  if (!y || !mu || !mat || !out_ll || !flags) return fail(PLA_ERR_ARG, "y / mu / mat / out_ll / flags is NULL");
  if (model_type == PLA_MVN_STUDENT_T && !df) return fail(PLA_ERR_ARG, "df is NULL for a Student-t model");
  if (n_obs < 1 || n_draws < 1) return fail(PLA_ERR_ARG, "n_obs and n_draws must be at least 1");
  if (n_obs > PLA_NONFACTOR_MAX_OBS)
    return fail(PLA_ERR_UNSUPPORTED, "n_obs = %lld exceeds the device limit of %d observations", (long long)n_obs,
                PLA_NONFACTOR_MAX_OBS);
  if (n_draws >= ((int64_t)1 << 31)) return fail(PLA_ERR_ARG, "n_draws must be below 2^31");
  if ((n_draws > 1 && mu_pitch < n_obs) || (n_draws > 1 && mat_pitch < n_obs * n_obs))
    return fail(PLA_ERR_ARG, "mu_pitch / mat_pitch smaller than one draw");
  if (ll_stride_obs < 0 || ll_stride_draw < 0 || ll_stride_obs > INT32_MAX || ll_stride_draw > INT32_MAX)
    return fail(PLA_ERR_ARG, "ll_stride_obs / ll_stride_draw must lie in [0, 2^31)");
  if (mem_space == PLA_HOST && ll_stride_draw != 1 && n_draws > 1) return fail(PLA_ERR_ARG, "host calls need ll_stride_draw == 1");
  if (mem_space == PLA_HOST && n_obs > 1 && ll_stride_obs < n_draws) return fail(PLA_ERR_ARG, "ll_stride_obs < n_draws");
  EngineCall call(eng, (hipStream_t)stream);
  PLA_HIP(hipSetDevice(eng->device));
  hipStream_t s = (hipStream_t)stream;
  const int N = (int)n_obs;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int route = pla::nonfactor_route_for(N, eng->nonfactor_route);
  const int64_t nb = mem_space == PLA_DEVICE ? n_draws : nonfactor_block_draws(n_obs, n_draws, esz);
  const int slots = nonfactor_slots(n_obs, nb, eng->nonfactor_grid);
  int rc = grow(&eng->d_nf, &eng->d_nf_bytes, (size_t)slots * (size_t)pla::nonfactor_slot_doubles(N) * sizeof(double));
  if (rc) return rc;
  pla::NonfactorParams p{};
  p.N = N;
  p.model = model_type;
  p.ws = (double*)eng->d_nf;
  p.slot = (int)pla::nonfactor_slot_doubles(N);
  const char* kname = route == PLA_NF_ROUTE_LDS ? "nonfactor_lds_kernel<" : route == PLA_NF_ROUTE_WORKSPACE ? "nonfactor_blocked_kernel<" : "";
  eng->last_kernels = std::string(kname) + (*kname ? std::string(pla::dtype_name(dtype)) + "> + " : std::string()) + "nonfactor_lu_kernel<" +
                      pla::dtype_name(dtype) + ">" + (route == PLA_NF_ROUTE_GENERAL ? " (every draw)" : " (declined draws)") +
                      (mem_space == PLA_DEVICE ? " (inputs read in place)" : " (inputs staged)");
  if (mem_space == PLA_DEVICE) {
    p.y = y;
    p.mu = mu;
    p.mat = mat;
    p.df = df;
    p.n_draws = (int)n_draws;
    p.mu_pitch = n_draws > 1 ? mu_pitch : n_obs;
    p.mat_pitch = n_draws > 1 ? mat_pitch : n_obs * n_obs;
    p.out = out_ll;
    p.so = ll_stride_obs;
    p.sd = ll_stride_draw;
    p.flags = flags;
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_nonfactor(p, dtype, route, slots, eng->nonfactor_grid, s));
    return PLA_OK;
  }
  // host: blocks of nb draws through the staging buffers (C-contiguous: mu [nb][N], matrices [nb][N][N], df [nb], y [N])
  const size_t in_elems = (size_t)nb * N * N + (size_t)nb * N + (size_t)nb + (size_t)N;
  rc = grow(&eng->d_nf_in, &eng->d_nf_in_bytes, in_elems * esz);
  if (rc) return rc;
  rc = grow(&eng->d_nf_out, &eng->d_nf_out_bytes, (size_t)nb * N * sizeof(double) + (size_t)nb * sizeof(int32_t));
  if (rc) return rc;
  char* din = (char*)eng->d_nf_in;
  void* dmat = din;
  void* dmu = din + (size_t)nb * N * N * esz;
  void* ddf = din + ((size_t)nb * N * N + (size_t)nb * N) * esz;
  void* dy = din + ((size_t)nb * N * N + (size_t)nb * N + (size_t)nb) * esz;
  double* dll = (double*)eng->d_nf_out;
  int32_t* dfl = (int32_t*)(dll + (size_t)nb * N);
  PLA_HIP(hipMemcpyAsync(dy, y, (size_t)N * esz, hipMemcpyHostToDevice, s));
  for (int64_t b0 = 0; b0 < n_draws; b0 += nb) {
    const int64_t n = n_draws - b0 < nb ? n_draws - b0 : nb;
    const char* hmat = (const char*)mat + (size_t)b0 * (size_t)mat_pitch * esz;
    const char* hmu = (const char*)mu + (size_t)b0 * (size_t)mu_pitch * esz;
    const size_t row = (size_t)N * N * esz;
    PLA_HIP(hipMemcpy2DAsync(dmat, row, hmat, (size_t)(n > 1 ? mat_pitch : (int64_t)N * N) * esz, row, (size_t)n,
                             hipMemcpyHostToDevice, s));
    PLA_HIP(hipMemcpy2DAsync(dmu, (size_t)N * esz, hmu, (size_t)(n > 1 ? mu_pitch : N) * esz, (size_t)N * esz, (size_t)n,
                             hipMemcpyHostToDevice, s));
    if (model_type == PLA_MVN_STUDENT_T)
      PLA_HIP(hipMemcpyAsync(ddf, (const char*)df + (size_t)b0 * esz, (size_t)n * esz, hipMemcpyHostToDevice, s));
    p.y = dy;
    p.mu = dmu;
    p.mat = dmat;
    p.df = model_type == PLA_MVN_STUDENT_T ? ddf : nullptr;
    p.n_draws = (int)n;
    p.mu_pitch = N;
    p.mat_pitch = (int64_t)N * N;
    p.out = dll;
    p.so = n;
    p.sd = 1;
    p.flags = dfl;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_nonfactor(p, dtype, route, slots, eng->nonfactor_grid, s));
    }
    PLA_HIP(hipMemcpy2DAsync(out_ll + b0, (size_t)(N > 1 ? ll_stride_obs : n_draws) * sizeof(double), dll, (size_t)n * sizeof(double),
                             (size_t)n * sizeof(double), (size_t)N, hipMemcpyDeviceToHost, s));
    PLA_HIP(hipMemcpyAsync(flags + b0, dfl, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  return PLA_OK;
}
}  // extern "C"
