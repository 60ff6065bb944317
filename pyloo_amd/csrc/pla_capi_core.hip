// C ABI of libpyloo_amd.so (see include/pyloo_amd.h), core unit: errors, the workspace buffer, the helpers pla_capi.h declares,
// and the entry points of the engine itself -- lifecycle, timing, environment report, aggregates.  Host code only.
#include <cstdarg>
#include <new>

#include "pla_capi.h"

namespace pla::capi {

namespace {
thread_local char g_err[512] = "";
}
thread_local bool g_frozen = false;

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int Buffer::reserve(size_t want) {
  if (bytes >= want) return PLA_OK;
  if (g_frozen)
    return fail(PLA_ERR_FROZEN, "the engine workspace is frozen (pla_engine_set_frozen) and this call needs %zu more bytes of it",
                want - bytes);
  // hipFree waits for the device: launches already enqueued on any stream have finished with the old buffer
  if (p) (void)hipFree(p);
  p = nullptr;
  bytes = 0;
  hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) {
    p = nullptr;
    return fail(PLA_ERR_NOMEM, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
  }
  bytes = want;
  return PLA_OK;
}

int check_types(int dtype, int mem_space) {
  if (dtype != PLA_F64 && dtype != PLA_F32) return fail(PLA_ERR_ARG, "dtype must be PLA_F64 or PLA_F32");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  return PLA_OK;
}

int check_engine_types(const pla_engine* eng, int dtype, int mem_space) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  return check_types(dtype, mem_space);
}

int check_n_draws(int64_t n_draws, int64_t least) {
  if (n_draws < least || n_draws > (int64_t)1 << 30)
    return fail(PLA_ERR_ARG, least > 1 ? "n_draws out of range (at least %lld)" : "n_draws out of range", (long long)least);
  return PLA_OK;
}

int check_common(pla_engine* eng, const void* in, int dtype, int64_t n_obs, int64_t n_draws,
                 int64_t stride_obs, int64_t stride_draw, int method, int64_t tail_count, int mem_space) {
  if (int rc = check_engine_types(eng, dtype, mem_space)) return rc;
  if (method != PLA_PSIS && method != PLA_SIS && method != PLA_TIS) return fail(PLA_ERR_ARG, "bad method");
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (n_obs > 0 && !in) return fail(PLA_ERR_ARG, "input pointer is NULL");
  if (int rc = check_n_draws(n_draws, 1)) return rc;
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

void TimedLaunch::flush(pla_engine* e) {
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

// Device matrices with the observations fastest (ArviZ's native layout behind pyloo's stacked view, loo.py:189) are brought
// to draws-fastest row blocks by a tiled transpose kernel and then take the same kernels as everything else.
bool obs_fastest_device(int mem_space, const int64_t* row_index, int64_t n_src, int64_t n_draws, int64_t stride_obs,
                        int64_t stride_draw) {
  return mem_space == PLA_DEVICE && !row_index && n_src > 1 && n_draws > 1 && stride_obs == 1 && stride_draw >= n_src;
}
// rows per staging block: 1 GiB blocks from the host (pinned-copy granularity), 4 GiB for the device transpose
int64_t staged_chunk_rows(int mem_space, bool ingest, int64_t n_obs, int64_t n_draws, size_t esz) {
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
int check_rows(const int64_t* row_index, int64_t n_rows, int64_t n_src, int mem_space) {
  if (n_rows < 0) return fail(PLA_ERR_ARG, "n_rows < 0");
  if (n_rows > 0 && !row_index) return fail(PLA_ERR_ARG, "row_index is NULL");
  if (n_rows > 0 && n_src <= 0) return fail(PLA_ERR_ARG, "row selection from an empty matrix");
  if (mem_space == PLA_HOST)
    for (int64_t i = 0; i < n_rows; ++i)
      if (row_index[i] < 0 || row_index[i] >= n_src) return fail(PLA_ERR_ARG, "row_index out of range");
  return PLA_OK;
}

// device path: a clamped copy of the caller's index list in engine memory (the row kernels trust it)
int device_rows(pla_engine* eng, const int64_t* row_index, int64_t n_rows, int64_t n_src, hipStream_t s,
                const int64_t** out) {
  int rc = eng->d_rows.reserve((size_t)(n_rows > 0 ? n_rows : 1) * sizeof(int64_t));
  if (rc) return rc;
  PLA_HIP(pla::launch_clamp_rows(row_index, n_rows, n_src, eng->d_rows.as<int64_t>(), s));
  *out = eng->d_rows.as<const int64_t>();
  return PLA_OK;
}

bool host_obs_fastest(int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw) {
  return n_obs > 1 && n_draws > 1 && stride_obs == 1 && stride_draw >= n_obs;
}

int upload_rows(const void* src, const int64_t* row_index, int64_t r0, int64_t nr, int64_t stride_obs, int64_t n_draws, size_t esz,
                void* dst, hipStream_t s) {
  const size_t row_bytes = (size_t)n_draws * esz, pitch = (size_t)stride_obs * esz;
  if (!row_index) {  // strided sources use a pitched copy
    PLA_HIP(hipMemcpy2DAsync(dst, row_bytes, (const char*)src + (size_t)r0 * pitch, pitch, row_bytes, (size_t)nr, hipMemcpyHostToDevice, s));
    return PLA_OK;
  }
  for (int64_t i = 0; i < nr; ++i)
    PLA_HIP(hipMemcpyAsync((char*)dst + (size_t)i * row_bytes, (const char*)src + (size_t)row_index[r0 + i] * pitch, row_bytes,
                           hipMemcpyHostToDevice, s));
  return PLA_OK;
}

int upload_slab(const void* src, int64_t r0, int64_t nr, int64_t stride_draw, int64_t n_draws, size_t esz, void* dst, hipStream_t s) {
  PLA_HIP(hipMemcpy2DAsync(dst, (size_t)nr * esz, (const char*)src + (size_t)r0 * esz, (size_t)stride_draw * esz, (size_t)nr * esz,
                           (size_t)n_draws, hipMemcpyHostToDevice, s));
  return PLA_OK;
}

int stage_rows(pla_engine* eng, const void* ll, const int64_t* row_index, int64_t r0, int64_t nr, int64_t stride_obs, int64_t stride_draw,
               int dtype, int64_t n_draws, int64_t rows_per_chunk, hipStream_t s) {
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  if (stride_draw == 1) return upload_rows(ll, row_index, r0, nr, stride_obs, n_draws, esz, eng->d_in.p, s);
  int rc = eng->d_slab.reserve((size_t)rows_per_chunk * (size_t)n_draws * esz);
  if (!rc) rc = upload_slab(ll, r0, nr, stride_draw, n_draws, esz, eng->d_slab.p, s);
  if (rc) return rc;
  PLA_HIP(pla::launch_transpose_rows(eng->d_slab.p, dtype, nr, 0, nr, (int)n_draws, eng->d_in.p, s));
  return PLA_OK;
}

bool lw_split_route(int method, int64_t n_draws, int64_t tail_count, int64_t* rows) {
  constexpr int64_t kLwBlock = (int64_t)1 << 17;
  if (method != PLA_PSIS || n_draws <= 4096 || !(tail_count <= 448)) return false;
  if (*rows > kLwBlock) *rows = kLwBlock;
  return true;
}

int lw_split_workspace(pla_engine* eng, int64_t tail_count, int64_t rows, pla::RowsParams* p) {
  const int stride = (int)((tail_count + 63) & ~(int64_t)63);  // 16 lanes x 4 values per quad
  const int rc = eng->d_ws.reserve((size_t)rows * (size_t)(stride + 8) * sizeof(double));
  if (rc == PLA_ERR_NOMEM) return PLA_OK;
  if (rc) return rc;
  p->ws_y = eng->d_ws.as<double>();
  p->ws_s = p->ws_y + (size_t)rows * stride;
  p->ws_stride = stride;
  p->ws_sstride = 8;
  p->lw_split = true;
  return PLA_OK;
}

int HostOutputs::reserve(int k, int64_t n_, unsigned long long* counter_) {
  n = n_;
  counter = counter_;
  const int rc = eng->d_pw.reserve(((size_t)k * (size_t)n + PLA_AGG_COUNT) * sizeof(double));
  if (rc) return rc;
  if (counter) PLA_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), s));
  return PLA_OK;
}

int HostOutputs::copy_back(std::initializer_list<double*> host) {
  int i = 0;
  for (double* h : host) {
    if (h && n > 0) PLA_HIP(hipMemcpyAsync(h, col(i), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    ++i;
  }
  return PLA_OK;
}

int HostOutputs::finish(std::initializer_list<double*> host, int64_t* count) {
  if (int rc = copy_back(host)) return rc;
  unsigned long long h = 0;
  if (counter) PLA_HIP(hipMemcpyAsync(&h, counter, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (counter && count) *count = (int64_t)h;
  return PLA_OK;
}

}  // namespace pla::capi

using namespace pla::capi;

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
  for (auto& t : e->l1_tables) (void)hipFree(t.d);
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
  for (hipEvent_t ev : {e->pipe_fork, e->pipe_join1, e->pipe_join2})
    if (ev) (void)hipEventDestroy(ev);
  for (int i = 0; i < pla_engine::kPipeTimed; ++i) {
    if (e->pipe_t0[i]) (void)hipEventDestroy(e->pipe_t0[i]);
    if (e->pipe_t1[i]) (void)hipEventDestroy(e->pipe_t1[i]);
  }
  delete e;  // (the workspace buffers go with it: pla::capi::Buffer)
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
  PLA_ENGINE_CALL(eng, stream);
  if (mem_space == PLA_DEVICE) {
    pla::ReduceParams rp{diag, loo_i, lppd_i, n_obs, good_k, agg, nullptr};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
    return PLA_OK;
  }
  const size_t need = (size_t)(3 * n_obs + PLA_AGG_COUNT);
  int rc = eng->d_pw.reserve(need * sizeof(double));
  if (rc) return rc;
  double* d = eng->d_pw.as<double>();
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

}  // extern "C"
