// Host-visible launch interface of the HIP kernels (internal to libpyloo_amd.so).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pla {

struct RowsParams {
  const void* in;       // (n_obs, n_draws) log-likelihood (LOO mode) or log ratios (LW mode)
  int64_t n_obs;
  int n_draws;
  int64_t stride_obs;   // elements
  int64_t stride_draw;  // elements
  int method;           // PLA_PSIS / PLA_SIS / PLA_TIS
  int tail_count;       // M (PSIS)
  int tail_cap;         // power of two >= M: LDS tail capacity
  double scale_value;   // LOO mode
  double* diag;         // [n_obs] or null
  double* loo_i;        // [n_obs] or null (LOO mode)
  double* lppd_i;       // [n_obs] or null (LOO mode)
  void* lw_out;         // (n_obs, n_draws) contiguous, input dtype (LW mode)
  unsigned long long* counters;  // [4] device counters: [0] rows left to the general kernel
  unsigned* slow_list;           // [n_obs] workspace for the fast path (may be null: general kernel only)
  const double* l1_table;        // [tail_count] log1p(-(j+0.5)/M), then [64] 1 - sqrt(m_est/(j+0.5)) (host-computed)
  // hand-over buffers of the split LOO pass (wave kernel -> fit kernel, pla_fit.h); null: fused pass
  double* ws_y = nullptr;        // [n_obs][ws_stride]
  double* ws_s = nullptr;        // [n_obs][8]
  int ws_stride = 0;
  // optional row selection (loo_subsample, loo_subsample.py:316-330): observation r of this call is row row_index[r] of `in`;
  // outputs stay compact ([n_obs] = number of selected rows)
  const int64_t* row_index = nullptr;  // (already clamped into the matrix: launch_clamp_rows)
  int ws_sstride = 8;            // doubles per observation in ws_s (16 in the streamed pass: one 128-byte line each)
  // weights mode of the split pass (rows longer than the registers: selection kernel -> fit kernel -> lw_output_kernel,
  // pla_lwout.h): the hand-over buffers above are there for it; false: the fused weights kernels
  bool lw_split = false;
};

// Streamed split pass: the first kernel (statistics, sweep, selection; HBM stream) on `first` and, BESIDE it on `second`, the
// fit kernel, which takes the chunks of observations as the first kernel finishes them (FastParams::done, pla_fit.h).  Both
// streams are forked from and joined to the caller's inside launch_rows(); `sync` is device memory for the flags and queues of
// one launch (stream_sync_bytes(n_obs)), zeroed by the launcher.
struct PipeStreams {
  hipStream_t first;
  hipStream_t second;
  hipEvent_t fork, join_first, join_second;  // (timing disabled)
  unsigned* sync;
  hipEvent_t before_first;  // optional (timing): recorded on `first` right before the first kernel ...
  hipEvent_t after_first;   // ... and right behind it
  bool zero_all_counters;   // first launch of a call: RowsParams::counters[0..15] are zeroed with the flags (else [0] only)
};
size_t stream_sync_bytes(int64_t n_obs);

// element offset of observation r's row in the input matrix
#define PLA_ROW_OFFSET(P, r) (((P).row_index ? (P).row_index[(r)] : (int64_t)(r)) * (P).stride_obs)

struct ReduceParams {
  const double* diag;
  const double* loo_i;
  const double* lppd_i;
  int64_t n_obs;
  double good_k;
  double* agg;  // [PLA_AGG_COUNT]
  const unsigned long long* counters;  // [0] -> PLA_AGG_N_SLOW (may be null)
};

// returns hipSuccess or the launch error; never synchronises
// `after_first`: optional event recorded right after the first kernel of a split LOO pass (timing of the dominant kernel alone);
// *recorded is set when it was
hipError_t launch_rows(const RowsParams& p, int dtype, bool lw_mode, hipStream_t stream, hipEvent_t after_first = nullptr,
                       bool* recorded = nullptr, const PipeStreams* pipe = nullptr);
// true when launch_rows() would run these rows as a split pass (first kernel + fit kernel): the shapes the pipeline serves
// true when launch_rows() given a PipeStreams would run these rows as a streamed split pass
bool rows_stream_planned(const RowsParams& p, int dtype);
hipError_t launch_reduce(const ReduceParams& p, double* workspace, hipStream_t stream);
// out[i] = min(max(in[i], 0), n_src - 1): a caller's device index list can never make a row kernel read outside the matrix
hipError_t launch_clamp_rows(const int64_t* in, int64_t n_rows, int64_t n_src, int64_t* out, hipStream_t stream);
int reduce_workspace_doubles();  // size of `workspace` (device memory)
// observation-sharded runs: a rank's row of the world x 8 table (the other rows zero) / the Chan merge of the summed table
hipError_t launch_aggregate_pack(const double* agg, int rank, int world, double* table, hipStream_t stream);
hipError_t launch_aggregate_merge(const double* table, int world, double* out, hipStream_t stream);
// text for pla_engine_last_kernels: what the last launch_rows() on this thread launched
const char* last_rows_kernels();
// Observations-fastest ingestion: ArviZ keeps log-likelihoods as (chain, draw, *obs), so the
// (obs, sample) view pyloo stacks (loo.py:189) has unit stride along the observations.  Rows [obs0, obs0 + n_rows) of
// such a matrix (element (i, s) at in[s * stride_draw + i]) are written as a contiguous (n_rows, n_draws) block.
hipError_t launch_transpose_rows(const void* in, int dtype, int64_t stride_draw, int64_t obs0, int64_t n_rows, int n_draws,
                                 void* out, hipStream_t stream);
hipError_t launch_fill_chains(void* ll, int dtype, int64_t n_obs, int64_t n_draws, int chains, double rho, double off_sd, int64_t row0,
                              uint64_t seed, double k_lo, double k_hi, hipStream_t stream);
hipError_t launch_fill_synthetic(void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t row0,
                                 uint64_t seed, double k_lo, double k_hi, double heavy_lo,
                                 double heavy_hi, hipStream_t stream);
// WAIC pass (waic.py:109-160): lppd_i, var_i, waic_i per observation; `replaced` counts NaN/inf entries
hipError_t launch_waic(const void* in, const int64_t* row_index, int dtype, int64_t n_obs, int n_draws, int64_t stride_obs, int64_t stride_draw,
                       double scale_value, double* lppd_i, double* var_i, double* waic_i,
                       unsigned long long* replaced, hipStream_t stream);
// weighted expectations + function-specific Pareto k (e_loo.py:56-264): x, lw, lr share dtype, shape and strides; lr may equal lw
hipError_t launch_e_loo(const void* x, const void* lw, const void* lr, int dtype, int64_t n_obs, int n_draws, int64_t stride_obs,
                        int64_t stride_draw, int tail_len, double* mean, double* var, double* k_mean, double* k_var, double* k_none,
                        unsigned* slow_list, unsigned long long* slow_count,
                        hipStream_t stream);
// weighted quantiles of e_loo (e_loo.py:468-515, 534-554): out[n_obs][n_probs]; probs is a DEVICE pointer
hipError_t launch_e_loo_quantiles(const void* x, const void* lw, int dtype, int64_t n_obs, int n_draws, int64_t stride_obs,
                                  int64_t stride_draw, const double* probs, int n_probs, double* out, unsigned* slow_list,
                                  unsigned long long* slow_count, hipStream_t stream);  // slow_list: [n_obs] scratch (may be null)
// Observations-fastest PSIS-LOO without a transposing pass (pla_col.h): lane-per-observation sweep + per-observation
// selection + the fit kernel of the split pass.  `p`: in = first observation of the block, stride_obs = 1, stride_draw = ld,
// ws_y / ws_s / slow_list / counters / l1_table set as for the split pass.  col_ws: col_workspace_bytes(n_obs) of device memory.
bool col_supported(int n_draws, int tail_count, int* kq);
size_t col_workspace_bytes(int64_t n_obs);
hipError_t launch_col(const RowsParams& p, int dtype, int kq, void* col_ws, hipStream_t stream);
// ... a workgroup per 16 observations, candidate lists in LDS (pla_tile.h): f64 matrices, 512 <= n_draws, tail counts <= 250 and a
// list capacity that leaves room on both sides of the expected candidate count.  No workspace beyond the split pass's hand-over.
// streamed (pipe with its flags, ws_sstride 16): the fit kernel runs beside the tile kernel, as in the streamed pass of the row kernels;
// the lists are shorter then (the fit kernel's workgroup needs its share of the CU's LDS), so `streamed` goes into the shape test.
bool tile_supported(int dtype, int n_draws, int tail_count, int64_t ld, bool streamed, int* ks);
hipError_t launch_tile(const RowsParams& p, int dtype, int ks, hipStream_t stream, const PipeStreams* pipe = nullptr);
// WAIC on an observations-fastest matrix read in place, one lane per observation (element (i, s) at in[s * ld + i])
hipError_t launch_waic_col(const void* in, int dtype, int64_t n_obs, int n_draws, int64_t ld, double scale_value, double* lppd_i,
                           double* var_i, double* waic_i, unsigned long long* replaced, hipStream_t stream);
// group sums of the leave-one-group-out pass (pla_group.h): out[g - g0, s] = sum of ll[m, s] over the members of group g in
// ascending order (NumPy's order), groups [g0, g0 + n_groups); the rows come from `in` = observations [row0, row0 + n_rows) of the
// matrix, draws contiguous (blocked: one of several blocks, partial sums continued in `out`).  replaced: NaN entries (may be null).
// *route (may be null): the vector leg taken, "16-byte loads" or "element loads", for pla_engine_last_kernels.
hipError_t launch_group_sum(const void* in, int dtype, int64_t stride_obs, int64_t row0, int64_t n_rows, int64_t n_src, bool blocked,
                            bool first_block, int n_draws, const int64_t* offsets, const int64_t* members, int64_t n_groups_total,
                            int64_t g0, int64_t n_groups, void* out, unsigned long long* replaced, hipStream_t stream,
                            const char** route);
// draw gather of the approximate-posterior pass (pla_draws.h): out[i, j] = in[i * stride_obs + clamp(draw_index[j]) * stride_draw] for
// the n_rows rows at `in`, out a contiguous (n_rows, n_out) block; NaN -> -1e10, counted in `replaced` (may be null).  *route (may be
// null): text for pla_engine_last_kernels.  Rows of at most gather_lds_max_draws(dtype) draws are staged in LDS.
int gather_lds_max_draws(int dtype);
hipError_t launch_gather_draws(const void* in, int dtype, int64_t stride_obs, int64_t stride_draw, int64_t n_rows, int n_draws,
                               const int64_t* draw_index, int n_out, void* out, unsigned long long* replaced, hipStream_t stream,
                               const char** route);
// *total += *value (one lane; the slow-row total of one block of a pla_psis_loo_draws call into the call's total)
hipError_t launch_add_counter(const unsigned long long* value, unsigned long long* total, hipStream_t stream);
// model comparison (pla_compare.h): x is a (K, N) matrix of pointwise values, row k at x + k * pitch.  `part` is engine workspace:
// compare_n_tiles(N) * (3K + 2) doubles (moments), * (K + 1) (stacking), nb * compare_n_tiles(N) * (K + 1) (bootstrap).  grid_cap > 0
// caps the workgroups per launch (the results do not depend on it).
int64_t compare_n_tiles(int64_t n_obs);
hipError_t launch_compare_moments(const void* x, int dtype, int64_t pitch, int K, int64_t N, int best, double* part, double* out,
                                  int grid_cap, hipStream_t stream);  // out [3K + 1]
hipError_t launch_stacking_eval(const void* x, int dtype, int64_t pitch, int K, int64_t N, double scale_mul, const double* w,
                                double* part, double* out, int grid_cap, hipStream_t stream);  // w [K] device; out [K + 1]: F, G
// replicates [b0, b0 + nb): z rows 0 .. nb-1 of the launch (z points at replicate b0's row)
hipError_t launch_bb_bootstrap(const void* x, int dtype, int64_t pitch, int K, int64_t N, double scale_mul, uint64_t seed, double alpha,
                               int64_t b0, int64_t nb, double* part, double* z, int grid_cap, hipStream_t stream);
hipError_t launch_bb_gamma_draws(uint64_t seed, double alpha, int64_t B, int64_t N, double* out, hipStream_t stream);
// non-factorised LOO (pla_nonfactor.h): the (N, S) conditional log-likelihood of one block of draws.  `route` is
// nonfactor_route_for(N, engine setting); p.ws holds ws_slots slots of p.slot = nonfactor_slot_doubles(N) doubles (the blocked
// and general kernels take one slot per workgroup); grid_cap > 0 caps the LDS kernel's workgroups (the results do not depend on
// either).
struct NonfactorParams;
int nonfactor_lds_max_obs();
int64_t nonfactor_slot_doubles(int n_obs);
int nonfactor_route_for(int n_obs, int forced);
hipError_t launch_nonfactor(const NonfactorParams& p, int dtype, int route, int ws_slots, int grid_cap, hipStream_t stream);
// k-fold cross-validation (pla_kfold.h).  The ragged log-mean-exp: a device table of sources and a task list grouped by source.
enum KfoldRoute { kKfoldWave = 0, kKfoldLane = 1, kKfoldBlock = 2 };
constexpr int kKfoldRouteMask = 3, kKfoldNanFlag = 4;

struct KfoldSource {  // one entry of the device table
  const void* base;
  int64_t n_rows;
  int64_t stride_row, stride_draw;  // elements
  int n_draws;
  int flags;  // route | kKfoldNanFlag
};

struct KfoldParams {
  const KfoldSource* src;  // [n_sources] device
  int n_sources;
  const int64_t* source_offsets;  // [n_sources + 1] device
  const int64_t* task_row;        // [n_tasks]
  const int64_t* task_out;        // [n_tasks]
  int64_t n_tasks;
  double* out;
  int64_t n_out;
  unsigned long long* replaced;  // [1] device counter (may be null)
};

// the route of a source (its strides, length and alignment decide), the ragged pass (one launch per route in `routes`, a bit mask of
// 1 << route) and the finishing pass (part: kfold_n_tiles(N) * 4 doubles of engine workspace; grid_cap > 0 caps the workgroups)
int kfold_route(const void* base, int dtype, int64_t stride_row, int64_t stride_draw, int64_t n_draws);
hipError_t launch_kfold_lme(const KfoldParams& p, int dtype, unsigned routes, hipStream_t stream, int* launches);  // *launches: kernels launched
const char* kfold_route_name(int route);
int64_t kfold_n_tiles(int64_t n_obs);
hipError_t launch_kfold_reduce(const double* elpd, const double* lpd_full, int64_t n_obs, double scale, double* p_i, double* kfold_i,
                               double* part, const unsigned long long* replaced, double* agg, int grid_cap, hipStream_t stream);
// Mix-IS-LOO (pla_mixis.h).  Pass 1: c[n_draws] = log sum_i exp(-ll[i, s]).  launch_mixis_c reduces rows [row0, row0 + n_rows) of a
// matrix of n_obs rows (`in` points at row row0; row0 a multiple of mixis_tile_rows_for(n_obs): a host matrix comes in blocks of
// whole tiles) into the tiles' slots of part -- 2 * mixis_n_tiles(n_obs) * n_draws doubles of engine workspace -- and
// launch_mixis_c_merge combines the slots of every draw in tile order.  vec_pitch: the pitch that decides whether the line kernel
// takes 16-byte loads beside the alignment of `in` and stride_draw (a staged block passes the whole matrix's, so that it sums in
// the order a device matrix of that layout gets).  Pass 2: *lse_c = log sum_s exp(-c[s]) (launch_mixis_lse_c, once) and
// elpd[i] = *lse_c - log sum_s exp(-ll[i, s] - c[s]), unscaled, for the rows at `in`.
// replaced [2]: NaN and +-inf entries met (may be null); grid_cap > 0 caps the workgroups of every launch (the results do not
// depend on it); route: text for pla_engine_last_kernels.
int64_t mixis_tile_rows_for(int64_t n_obs);
int64_t mixis_n_tiles(int64_t n_obs);
hipError_t launch_mixis_c(const void* in, int dtype, int64_t n_rows, int n_draws, int64_t stride_obs, int64_t stride_draw,
                          int64_t n_obs, int64_t row0, int64_t vec_pitch, double* part, unsigned long long* replaced, int grid_cap,
                          hipStream_t stream, char* route, int cap);
hipError_t launch_mixis_c_merge(const double* part, int64_t n_obs, int n_draws, double* c, int grid_cap, hipStream_t stream);
hipError_t launch_mixis_lse_c(const double* c, int n_draws, double* lse_c, hipStream_t stream);
hipError_t launch_mixis_elpd(const void* in, int dtype, int64_t n_obs, int n_draws, int64_t stride_obs, int64_t stride_draw,
                             const double* c, const double* lse_c, double* elpd, unsigned long long* replaced, int grid_cap,
                             hipStream_t stream, char* route, int cap);
// agg[PLA_AGG_N_SLOW] = replaced[0] + replaced[1], agg[PLA_AGG_N_NONFINITE] = 0 (agg may be null); counts[2] = replaced (may be null)
hipError_t launch_mixis_counts(const unsigned long long* replaced, double* agg, int64_t* counts, hipStream_t stream);
// LOO-PIT (pla_pit.h).  launch_pit_prepare: out (n_rows, n_draws) contiguous = -in with NaN -> -1e10 (counted in `replaced`, may be
// null), `in` read with its own strides.  launch_pit: pit_le[r] / pit_lt[r] (pit_lt may be null) from the log weights, the draws
// yh (the dtype of lw) and y, each matrix with its own strides; route: text for pla_engine_last_kernels.
hipError_t launch_pit_prepare(const void* in, int dtype, int64_t stride_obs, int64_t stride_draw, int64_t n_rows, int n_draws, void* out,
                              unsigned long long* replaced, hipStream_t stream, const char** route);
hipError_t launch_pit(const void* lw, const void* yh, const double* y, int dtype, int64_t n_obs, int n_draws, int64_t lw_stride_obs,
                      int64_t lw_stride_draw, int64_t yh_stride_obs, int64_t yh_stride_draw, double* pit_le, double* pit_lt,
                      hipStream_t stream, char* route, int cap);
// LOO diagnostics (pla_diag.h).  launch_diag_prepare: launch_pit_prepare with a row gather -- out row r = -in[row_index[r]] (row_index
// null: row row0 + r; a device list, clamped into [0, n_src) by the kernel).  launch_diag: elpd / ess_w / var_log (each may be null)
// from the log weights and x with ll = sign * x, each matrix with its own strides; route: text for pla_engine_last_kernels.
hipError_t launch_diag_prepare(const void* in, int dtype, int64_t n_src, int64_t stride_obs, int64_t stride_draw, const int64_t* row_index,
                               int64_t row0, int64_t n_rows, int n_draws, void* out, unsigned long long* replaced, hipStream_t stream,
                               const char** route);
hipError_t launch_diag(const void* lw, const void* x, double sign, int dtype, int64_t n_obs, int n_draws, int64_t lw_stride_obs,
                       int64_t lw_stride_draw, int64_t x_stride_obs, int64_t x_stride_draw, double* elpd, double* ess_w, double* var_log,
                       hipStream_t stream, char* route, int cap);
// LOO influence (pla_influence.h).  influence_pads: the padded extents of Z^T for n_draws x n_quant.  launch_influence_prepare:
// zt[p_pad][s_pad] = ((theta - center) / scale)^T, zero padded; theta with any positive strides.  launch_influence: shift / m2
// (n_obs, n_quant) and kl / ess_w [n_obs] (each may be null) from the log weights with their own strides and zt; route: text for
// pla_engine_last_kernels.
constexpr int kInfMaxQuant = 1024;
void influence_pads(int n_draws, int n_quant, int* s_pad, int* p_pad);
hipError_t launch_influence_prepare(const double* theta, int64_t stride_draw, int64_t stride_quant, const double* center, const double* scale,
                                    int n_draws, int n_quant, double* zt, hipStream_t stream);
hipError_t launch_influence(const void* lw, int dtype, int64_t n_obs, int n_draws, int64_t lw_stride_obs, int64_t lw_stride_draw,
                            const double* zt, int n_quant, double* shift, double* m2, double* kl, double* ess_w,
                            hipStream_t stream, char* route, int cap);
// GLM log-likelihood generator (pla_glm.h).  glm_pads: the padded extents of the image of beta for n_draws x n_pred.
// launch_glm_prepare: bimg[s_pad][p_pad] = beta, zero padded, and kGlmImagePad zeros behind it; beta with any positive strides.  launch_glm: the linear predictor or
// the log-likelihood of n_rows rows -- row_index[0 .. n_rows) of X, or rows r_first .. -- times all draws into out (row pitch in
// elements, draws fastest); replaced non-null: NaN -> -1e10, counted; route: text for pla_engine_last_kernels.
constexpr int kGlmMaxPred = 256;
constexpr int kGlmImagePad = 2;  // doubles behind the image, zero
struct GlmLaunch {
  int family;
  const double* x;
  int64_t x_stride_obs, x_stride_pred, n_src;
  const int64_t* row_index;
  int64_t r_first, n_rows;
  const double* bimg;
  int n_pred, n_draws;
  const double *y, *offset, *trials, *obs_const, *sigma, *draw_const;  // sigma: the family's scale per draw (sigma, phi, alpha)
  double* out;
  int64_t pitch;
  unsigned long long* replaced;
};
void glm_pads(int n_draws, int n_pred, int* s_pad, int* p_pad);
hipError_t launch_glm_prepare(const double* beta, int64_t stride_draw, int64_t stride_pred, int n_draws, int n_pred, double* bimg,
                              hipStream_t stream);
hipError_t launch_glm(const GlmLaunch& g, hipStream_t stream, char* route, int cap);
// ... with group-level terms (pla_glm_terms.h): eta += z_t[i] u_t[s, g_t[i]], t = 0 .. n_terms - 1, in that order.
// launch_glm_terms_prepare: uimg[sum G_t][s_pad], group-major, draws fastest, zero for s >= n_draws; term t starts at row first[t]
// (filled in here, first[n_terms] the number of rows); u_t with any positive strides.  launch_glm_terms: launch_glm with the terms
// added to the accumulator registers; group / z are [n_src] (z[t] null: 1), a group index is clamped into [0, n_groups) on load.
constexpr int kGlmMaxTerms = 8;
struct GlmTerms {
  int n_terms;
  const double* u[kGlmMaxTerms];
  int64_t u_stride_draw[kGlmMaxTerms], u_stride_group[kGlmMaxTerms];
  int n_groups[kGlmMaxTerms];
  const int32_t* group[kGlmMaxTerms];
  const double* z[kGlmMaxTerms];
  int64_t first[kGlmMaxTerms + 1];
  const double* uimg;
};
int64_t glm_terms_image_size(const GlmTerms& t, int n_draws);  // doubles
hipError_t launch_glm_terms_prepare(GlmTerms* t, int n_draws, double* uimg, hipStream_t stream);
hipError_t launch_glm_terms(const GlmLaunch& g, const GlmTerms& t, hipStream_t stream, char* route, int cap);
// ... the leave-one-out predictive moments and PIT of the model (pla_glm_predict.h): the generator's launch g (out, pitch and
// replaced unused) contracted against the log weights of its rows -- (n_rows, n_draws), row pitch lw_pitch, unit draw stride.
// work: glm_predict_workspace(n_rows, n_draws) doubles of this pass alone; mean / m2 / pit_le / pit_lt [n_rows], each may be null;
// skipped: the rows whose count lies outside [0, kGlmPredictMaxCount], added to (never zeroed here; may be null).
constexpr int kGlmPredictSeg = 16;          // tiles of 16 draws per segment of the summation rule
constexpr int kGlmPredictMaxCount = 4096;   // the largest count whose distribution function is walked
struct GlmPredictLaunch {
  const double* lw;
  int64_t lw_pitch;
  double* work;
  double *mean, *m2, *pit_le, *pit_lt;
  unsigned long long* skipped;
};
int64_t glm_predict_workspace(int64_t n_rows, int n_draws);
hipError_t launch_glm_predict(const GlmLaunch& g, const GlmPredictLaunch& q, hipStream_t stream, char* route, int cap);
// leave-future-out CV (pla_lfo.h).  launch_lfo_ratios: the log ratios of one block of n_rows steps -- whole chunks of
// lfo_chunk_rows() steps unless it is the last block -- as a contiguous (n_rows, n_draws) f64 matrix; `in` is the row of the block's
// first step (draws contiguous), rows j < n_load of the block are read (NaN -> -1e10, counted in `replaced`, may be null); carry:
// ceil(n_rows / chunk) * n_draws doubles of workspace; run [n_draws]: the carry into the block (zero before the first), left as the
// carry into the next.  launch_lfo_predict: elpd and (step 0 of a pass) k = 0 of a block of steps from its log weights and the
// matrix read in place (draws contiguous, any row stride).  launch_lfo_first_high: *out = the smallest j >= 1 with diag[j] > threshold, else n_steps.
int lfo_chunk_rows();
hipError_t launch_lfo_ratios(const void* in, int dtype, int64_t stride_obs, int n_draws, int64_t n_rows, int64_t n_load, bool last_block,
                             double* carry, double* run, double* out, unsigned long long* replaced, hipStream_t stream,
                             const char** route);
hipError_t launch_lfo_predict(const double* lw, const void* ll, int dtype, int64_t ll_stride_obs, int64_t n_steps,
                              int n_draws, int horizon, bool pass_start, double* diag, double* elpd, unsigned long long* replaced,
                              hipStream_t stream, char* route, int cap);
hipError_t launch_lfo_first_high(const double* diag, int64_t n_steps, double threshold, long long* out, hipStream_t stream);
// totals -> carries of a block's chunks in place, continued through run (lfo_carry_kernel alone: backward mode launches it between its scans)
hipError_t launch_lfo_carry(double* carry, double* run, int64_t n_chunks, int64_t n_totals, int n_draws, hipStream_t stream);
// ... backward mode (pla_lfo_bw.h): a block is n_rows values of q = last - t, whole chunks unless it is the last; `in` is the row
// last - 1 - q of its first q and the rows are walked DOWNWARD (row of local q: in - q stride_obs, read for q < n_load); out holds
// -(carry + local) of its q, compact (not launched without `write`: a block before the first step only passes its carry on).  launch_lfo_bw_predict: `ll` is row t of the block's first step, step
// j lies j rows below it and its window goes upward; pass_start: step 0 counts its whole window, exact0: and is the fit's own step.
// launch_lfo_bw_first_high: the smallest j >= j_min above the threshold, else n_steps.
hipError_t launch_lfo_bw_ratios(const void* in, int dtype, int64_t stride_obs, int n_draws, int64_t n_rows, int64_t n_load, bool last_block,
                                bool write, double* carry, double* run, double* out, hipStream_t stream, const char** route);
hipError_t launch_lfo_bw_predict(const double* lw, const void* ll, int dtype, int64_t ll_stride_obs, int64_t n_steps, int n_draws,
                                 int horizon, bool pass_start, bool exact0, double* diag, double* elpd, unsigned long long* replaced,
                                 hipStream_t stream, char* route, int cap);
hipError_t launch_lfo_bw_first_high(const double* diag, int64_t n_steps, int64_t j_min, double threshold, long long* out,
                                    hipStream_t stream);
// relative MCMC efficiency (pla_ess.h): r_eff of n_rows rows (draws contiguous, any row stride) of n_src_chains chains of n_src draws,
// chain major.  ws: ess_grid_for(...) slots of the analysed draws in doubles when they exceed ess_lds_max_draws(), else unused;
// grid_cap: 0 or a cap on the workgroups; invalid: device counter of the NaN results (may be null, never zeroed here).
int ess_lds_max_draws();
int64_t ess_grid_for(int64_t n_rows, int64_t analysed, int cap);
hipError_t launch_ess(const void* in, int dtype, int64_t stride_obs, int64_t n_rows, int n_src_chains, int n_src, int split, int log_mode,
                      int cap_one, double* ws, int grid_cap, double* out, unsigned long long* invalid, hipStream_t stream, char* route,
                      int cap);
// moment matching (pla_mm.h): batched moments, affine transform and ratio assembly, f64, device memory
constexpr int kMmMaxCovDim = 64;  // D with matrices (moments with cov, transform with a matrix)
constexpr int kMmMaxDim = 1024;   // D without

struct MmTransformParams {
  const double* x;  // batch b at x + b * x_batch_stride (0: one matrix for every b), (S, D)
  int64_t x_batch_stride;
  const double* m0;    // [B][D]
  const double* pre;   // [B][D] or null
  const double* map;   // [B][D][D] or null
  const double* post;  // [B][D] or null: a divisor
  const double* m1;    // [B][D]
  int64_t B, S;
  int D;
  int64_t row_lo, row_hi;
  double* out;  // (B, S, D)
};

struct MmRatiosParams {
  const double *a, *b, *c;  // see launch_mm_ratios
  const double* jac;        // [B][2] (mode 1)
  int64_t B, S;
  double* out;
};

// work: mm_moments_workspace(...) doubles of engine workspace; grid_cap > 0 caps the workgroups of every launch (the results do
// not depend on it).  mode of launch_mm_ratios: 0 update ratios, 1 split weights, 2 lw + ll, 3 the two logsumexp per row.
int64_t mm_moments_workspace(int64_t B, int64_t S, int D, int want_cov);
hipError_t launch_mm_moments(const double* x, const double* lw, int64_t B, int64_t S, int D, int want_cov, double* work, double* stats,
                             double* cov, int grid_cap, hipStream_t stream);
hipError_t launch_mm_transform(const MmTransformParams& p, int grid_cap, hipStream_t stream);
hipError_t launch_mm_ratios(int mode, const MmRatiosParams& p, int grid_cap, hipStream_t stream);
// largest tail count the kernels accept
int max_tail_count();

}  // namespace pla
