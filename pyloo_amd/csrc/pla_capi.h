// Host side of the C ABI of libpyloo_amd.so (internal; the interface is include/pyloo_amd.h): the engine, and what the units
// pla_capi_<family>.hip share -- errors, the workspace buffers, the per-call guards, argument checks and host<->device staging.
//   pla_capi_core.hip    engine lifecycle, errors, timing, environment report, quantile table, aggregates; every helper declared here
//   pla_capi_loo.hip     PSIS-LOO pass, importance weights, WAIC, e_loo, synthetic fills
//   pla_capi_views.hip   groups, draw gather, k-fold
//   pla_capi_passes.hip  LOO-PIT, diagnostics, influence, leave-future-out, relative efficiency, Mix-IS
//   pla_capi_models.hip  comparison / stacking / bootstrap, moment matching, non-factorised LOO
//   pla_capi_glm.hip     GLM log-likelihood generator and its fused PSIS-LOO pass; the cluster-marginal likelihood on top of it; the
//                        leave-one-out predictive moments and PIT of the model
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pyloo_amd.h"
#include "pla_launch.h"

struct pla_engine;

namespace pla::capi {

// pla_last_error: the message of this thread's last failure; returns `code`
int fail(int code, const char* fmt, ...);

#define PLA_HIP(call)                                                                                \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      return ::pla::capi::fail(e_ == hipErrorOutOfMemory ? PLA_ERR_NOMEM : PLA_ERR_HIP, "%s: %s", #call, \
                               hipGetErrorString(e_));                                               \
  } while (0)

inline int pow2_at_least(int64_t n) {
  int p = 8;
  while (p < n) p <<= 1;
  return p;
}

// set from the engine at the start of every entry point (EngineCall); defined in pla_capi_core.hip
extern thread_local bool g_frozen;

// One buffer of the engine's workspace: device memory that grows on demand and goes with the engine.
struct Buffer {
  void* p = nullptr;
  size_t bytes = 0;
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() {
    if (p) (void)hipFree(p);
  }
  // At least `want` bytes (contents are not kept).  A frozen engine refuses to reallocate (PLA_ERR_FROZEN); when the allocation
  // fails the buffer is left empty (PLA_ERR_NOMEM: the split weights route carries on without it).
  int reserve(size_t want);
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

}  // namespace pla::capi

struct pla_engine {
  using Buffer = pla::capi::Buffer;
  int device = 0;
  // One engine = one workspace: every entry point that takes an engine holds this lock for the whole call, so
  // concurrent callers (ctypes releases the GIL) are serialised instead of racing on the buffers below.
  std::mutex mu;
  // frozen: the workspace may be referenced by a captured HIP graph; a call that would have to reallocate any of
  // it returns PLA_ERR_FROZEN instead (pla_engine_set_frozen)
  bool frozen = false;
  unsigned long long* counters = nullptr;  // [pla::kCountersTotal] device (layout: pla_launch.h): [0..15] per call, [16..] engine statistics
  double* d_red = nullptr;                 // reduction partials
  // quantile tables log1p(-(j+0.5)/M), one immutable device buffer per tail count M seen so far (never rewritten
  // or freed before the engine is destroyed: enqueued launches and captured graphs keep valid pointers)
  struct L1Table { int64_t M; double* d; };
  std::vector<L1Table> l1_tables;

  // ---- the workspace (grown on demand; freed with the engine) ----
  Buffer d_in;    // staging for PLA_HOST callers and for the transposing ingestion: one block of rows, draws fastest
  Buffer d_lw;    // the weights of one block of rows (host calls, and the passes that consume a block's weights)
  Buffer d_pw;    // pointwise outputs of a host call / scratch for the aggregates: k * n doubles + agg
  Buffer d_slow;  // [n] row list of the fast path
  Buffer d_ws;    // hand-over buffers of the split LOO pass: [n][stride] tail values + [n][8] scalars
  Buffer d_sync;  // flags between the two kernels of the streamed split pass
  Buffer d_col;   // observations-fastest LOO (pla_col.h): candidate lists + scalars of one block of observations
  Buffer d_probs; // quantile levels of pla_e_loo_quantiles
  Buffer d_rows;  // clamped copy of a caller's device row-index list
  Buffer d_slab;  // host path, observations-fastest input: (n_draws, block of observations) slab before the transpose
  Buffer d_grp;   // group sums of one block of groups (pla_psis_loo_groups; pla_group_sum from the host)
  Buffer d_gidx;  // host path of the group calls: [0] replaced-entry counter, then the uploaded offsets and members
  Buffer d_cmp;      // model comparison: per-tile partials (pla_compare.h)
  Buffer d_cmp_out;  // ... and the outputs of host calls / of the stacking evaluation
  Buffer d_nf;      // non-factorised LOO: slots of the blocked / general routes (pla_nonfactor.h)
  Buffer d_nf_in;   // ... staging of a host call: one block of draws (mu, matrices, df) and y
  Buffer d_nf_out;  // ... and its outputs (ll block, flags)
  Buffer d_kf;   // k-fold: the source table of the last pla_kfold_lme call ...
  Buffer d_mm;   // moment matching: per-tile partials of pla_mm_moments (pla_mm.h)
  Buffer d_mix;  // Mix-IS-LOO (pla_mixis.h): the slab of pass 1, c, the unscaled pointwise values, the finishing pass's partials
  Buffer d_pit;  // LOO-PIT (pla_pit.h): one block of predictive draws, draws fastest (transposed or staged from the host)
  Buffer d_lfo;  // leave-future-out CV (pla_lfo.h): the carry into a block of steps [n_draws], then the carries of its chunks
  Buffer d_ess;  // relative efficiency (pla_ess.h): a slot of centred draws per workgroup of the long-row route
  Buffer d_inf;  // LOO influence (pla_influence.h): Z^T of the call, zero padded; behind it theta, center and scale of a host call
  Buffer d_glm;     // GLM generator (pla_glm.h): the image of beta, zero padded; behind it X, beta, the vectors and rows of a host call
  Buffer d_glm_ll;  // ... one block of rows of the log-likelihood (the fused LOO pass; the matrix mode of a host call)
  Buffer d_glm_u;   // ... pla_glm_grouped alone (pla_glm_terms.h): the image of the group effects; behind it the group indices, z and u of a host call
  Buffer d_glm_marg;  // ... pla_glm_marginal alone (pla_glm_marginal.h): segment and join tables, the carry, the partial sums; behind them z, tau, nodes and log_weights of a host call
  Buffer d_glm_mll;   // ... and its block of finished clusters (the fused LOO pass; the matrix mode of a host call)
  Buffer d_glm_pred;  // ... pla_glm_predict alone (pla_glm_predict.h): the row maxima of a block's weights and its per-(row, segment) partial sums

  // ... the k-fold table's pinned host copy (the upload reads it after the call has returned), two of them used in turn, and the
  // event behind each upload: a call waits for the upload of the call before the previous one before it rewrites that copy
  void* h_kf[2] = {nullptr, nullptr};
  size_t h_kf_bytes[2] = {0, 0};
  hipEvent_t kf_event[2] = {nullptr, nullptr};
  int kf_turn = 0;
  std::string kf_label;  // the routes of the last pla_kfold_lme, for the text pla_kfold_reduce leaves in last_kernels

  int compare_grid = 0;     // pla_engine_set_compare_grid: workgroup cap of the comparison passes (0: the library's choice)
  int mixis_grid = 0;       // pla_engine_set_mixis_grid (0: the library's choice)
  int ess_grid = 0;         // pla_engine_set_ess_grid (0: the library's choice)
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
  // streamed split pass (psis_loo_run, pla_kernels.hip launch_wave): two internal streams forked from / joined to the
  // caller's stream -- the wave kernel on one, the fit kernel beside it on the other -- and the flags between them (d_sync)
  hipStream_t pipe_first = nullptr, pipe_second = nullptr;
  hipEvent_t pipe_fork = nullptr, pipe_join1 = nullptr, pipe_join2 = nullptr;
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

namespace pla::capi {

// every entry point: serialise on the engine and publish its frozen flag to Buffer::reserve.  With a stream: the call enqueues work
// that uses the engine's workspace -- it is ordered behind the previous such call when that one went to ANOTHER stream (one event
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

// opens an entry point that enqueues work: the guard above as `call`, the engine's device, the caller's stream as `s`
#define PLA_ENGINE_CALL(eng, stream)                        \
  ::pla::capi::EngineCall call(eng, (hipStream_t)stream);   \
  PLA_HIP(hipSetDevice(eng->device));                       \
  hipStream_t s = (hipStream_t)stream

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
  static void flush(pla_engine* e);  // reads back the recorded event pairs (waits for them)
};

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_common(pla_engine* eng, const void* in, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                 int method, int64_t tail_count, int mem_space);
// the opening checks of the entry points check_common does not fit, in the order they make them: dtype, then mem_space -- behind
// the engine for most (check_engine_types), ahead of it for the calls that report an argument error with or without an engine
int check_types(int dtype, int mem_space);
int check_engine_types(const pla_engine* eng, int dtype, int mem_space);
int check_n_draws(int64_t n_draws, int64_t least);  // least <= n_draws <= 2^30
// row selection shared by pla_psis_loo_rows / pla_waic_rows / pla_loo_diag: the index list lives where the matrix lives
int check_rows(const int64_t* row_index, int64_t n_rows, int64_t n_src, int mem_space);
// device path: a clamped copy of the caller's index list in engine memory (the row kernels trust it)
int device_rows(pla_engine* eng, const int64_t* row_index, int64_t n_rows, int64_t n_src, hipStream_t s, const int64_t** out);

// ---- layouts and block sizes ---------------------------------------------------------------------------------------------------
// Device matrices with the observations fastest (ArviZ's native layout behind pyloo's stacked view, loo.py:189) are brought
// to draws-fastest row blocks by a tiled transpose kernel and then take the same kernels as everything else.
bool obs_fastest_device(int mem_space, const int64_t* row_index, int64_t n_src, int64_t n_draws, int64_t stride_obs, int64_t stride_draw);
bool host_obs_fastest(int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw);
// rows per staging block: 1 GiB blocks from the host (pinned-copy granularity), 4 GiB for the device transpose
int64_t staged_chunk_rows(int mem_space, bool ingest, int64_t n_obs, int64_t n_draws, size_t esz);

// ---- block uploads of a PLA_HOST matrix (enqueued on s; the caller synchronises before it reuses dst) --------------------------
// rows [r0, r0 + nr) -- the selected rows row_index[r0 ..] when row_index is set -- as an (nr, n_draws) block, draws fastest
int upload_rows(const void* src, const int64_t* row_index, int64_t r0, int64_t nr, int64_t stride_obs, int64_t n_draws, size_t esz,
                void* dst, hipStream_t s);
// observations fastest on the host (a (chain, draw, *obs) array viewed as (obs, sample), loo.py:189): observations [r0, r0 + nr)
// as the (n_draws, nr) slab they are -- one pitched copy, no transpose on the host; a device kernel turns or reads it
int upload_slab(const void* src, int64_t r0, int64_t nr, int64_t stride_draw, int64_t n_draws, size_t esz, void* dst, hipStream_t s);
// either of the two into the ingest staging d_in, draws fastest: upload_rows, or upload_slab into d_slab (grown for rows_per_chunk
// rows) and the transpose kernel
int stage_rows(pla_engine* eng, const void* ll, const int64_t* row_index, int64_t r0, int64_t nr, int64_t stride_obs, int64_t stride_draw,
               int dtype, int64_t n_draws, int64_t rows_per_chunk, hipStream_t s);

// ---- the split weights route ---------------------------------------------------------------------------------------------------
// Rows longer than the registers (S > 4096) with tails the fit kernel takes: the split weights pass (selection kernel -> fit
// kernel -> output kernel, csrc/pla_lwout.h) needs the hand-over buffers -- the tail's x and eight scalars per observation -- for
// the rows of one launch, so such calls run in blocks of at most 2^17 observations (0.48 GB at 448-value tails).
// Does a weights pass of this shape take the route?  If so *rows, the rows of one launch, is capped.
bool lw_split_route(int method, int64_t n_draws, int64_t tail_count, int64_t* rows);
// The route's fields of p (ws_*, lw_split) for `rows` rows per launch.  No room for the buffers: p is left as it is -- the fused
// weights kernel, which needs none -- and the call carries on (PLA_OK).
int lw_split_workspace(pla_engine* eng, int64_t tail_count, int64_t rows, pla::RowsParams* p);

// ---- outputs of a PLA_HOST call ------------------------------------------------------------------------------------------------
// k columns of n doubles, and room for the aggregates behind them, in d_pw; one of the engine's counters beside them when the
// call counts something.
struct HostOutputs {
  pla_engine* eng;
  hipStream_t s;
  int64_t n = 0;
  unsigned long long* counter = nullptr;
  HostOutputs(pla_engine* e, hipStream_t s_) : eng(e), s(s_) {}
  int reserve(int k, int64_t n_, unsigned long long* counter_ = nullptr);  // (zeroes the counter)
  double* col(int i) const { return eng->d_pw.as<double>() + (size_t)i * (size_t)n; }
  // the columns back to the caller's arrays, in order (NULL: the caller does not want that one); nothing is waited for
  int copy_back(std::initializer_list<double*> host);
  // copy_back, the counter into *count (when there is one), and the synchronise that ends the call
  int finish(std::initializer_list<double*> host, int64_t* count = nullptr);
};

// ---- engine resources created on first use -------------------------------------------------------------------------------------
// Row-independent tables of the fast path, computed with the host libm exactly as NumPy does
int ensure_l1_table(pla_engine* e, int64_t M, hipStream_t s, const double** out);
// streams and events of the streamed pass
int ensure_pipe(pla_engine* e);

// the PSIS / SIS / TIS pass itself, for a caller that has checked the arguments and holds the engine (pla_capi_loo.hip)
int psis_loo_run(pla_engine* eng, const void* ll, int dtype, int64_t n_src, const int64_t* row_index, int64_t n_obs, int64_t n_draws,
                 int64_t stride_obs, int64_t stride_draw, int method, int64_t tail_count, double scale_value, double good_k,
                 int mem_space, void* stream, double* diag, double* loo_i, double* lppd_i, double* agg);
// The weights pass of one block of rows for the passes that consume a block's weights before the next block overwrites them
// (pla_loo_pit, pla_loo_diag), as pla_importance_weights sets it up (pla_capi_loo.hip)
int weights_block_setup(pla_engine* eng, int method, int64_t tail_count, int64_t n_draws, size_t esz, hipStream_t s, int64_t* rows,
                        pla::RowsParams* p);

}  // namespace pla::capi
