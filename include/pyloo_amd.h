/*
 * pyloo_amd.h -- C ABI of the MI355X-native PSIS-LOO engine (libpyloo_amd.so).
 *
 * This is the drop-in boundary for the ONE hot path of jordandeklerk/pyloo that this
 * project accelerates.  The reference has no FFI of its own: the seam
 * is the Python call `wrap_xarray_ufunc(_psislw, ...)` that loops a 1-D NumPy routine over
 * observations.  Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns an int status (0 = PLA_OK,
 *     negative = error) and never throws or aborts; pla_last_error() gives the text.
 *   - the caller owns every buffer; inputs are const and never modified (the reference
 *     deep-copies its input: psis.py:78, base.py:112); nothing is retained after return.
 *   - numeric trouble is in-band exactly as in the reference: k = +inf when the tail has
 *     <= 4 draws (psis.py:142-144), NaN weights for NaN rows, etc.  No status code for it.
 *   - `mem_space` says where ALL data pointers of that call live: PLA_HOST (the library
 *     stages through its own device buffers) or PLA_DEVICE (pointers are HIP device
 *     pointers on the engine's device, work is enqueued on `stream`, no host sync).
 *   - matrices are (n_obs, n_draws) with element strides (stride_obs, stride_draw) in
 *     ELEMENTS.  Two layouts are fast: stride_draw == 1 (draws contiguous), and stride_obs == 1 with
 *     stride_draw >= n_obs (observations contiguous: pyloo's stacked `(*obs, __sample__)` view of an ArviZ
 *     (chain, draw, *obs) array, loo.py:189) -- pla_psis_loo, pla_waic and (device pointers) pla_importance_weights
 *     transpose the latter block by block on the device.  Anything else runs on the strided general kernel (device pointers) or is refused (host pointers).
 *   - threads and streams: an engine is bound to one device and owns ONE workspace.  Every entry point that takes an
 *     engine holds the engine's mutex for the whole call, so concurrent calls from several threads are safe (they run one
 *     after the other); different engines are independent (no hidden global state).  PLA_DEVICE calls only ENQUEUE work
 *     that uses the workspace; the engine orders that work ACROSS STREAMS itself: every call records an event behind what
 *     it enqueued, and a call on another stream first makes its stream wait for the previous call's event -- two streams
 *     never run passes of one engine side by side, whatever the caller does (calls on one stream are ordered anyway).
 *     For passes that should overlap use one engine per stream.  Inside a stream capture no event is waited for or
 *     recorded: order captured work yourself.  Growing the workspace frees the old buffers with hipFree, which waits for
 *     the device, so launches already enqueued are never left with dangling pointers.
 *   - HIP graphs: a captured PLA_DEVICE call holds raw workspace pointers.  Size the workspace first (one eager call
 *     of the largest shape and tail count to be replayed), then pla_engine_set_frozen(eng, 1): from then on a call that
 *     would have to reallocate returns PLA_ERR_FROZEN instead of invalidating the graph.  The per-tail-count quantile
 *     tables are immutable once created, so eager calls with other tail counts do not disturb a captured graph.
 */
#ifndef PYLOO_AMD_H
#define PYLOO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLA_ABI_VERSION 7

/* status codes */
#define PLA_OK 0
#define PLA_ERR_ARG (-1)         /* bad argument (null pointer, n_draws < 2, bad enum ...) */
#define PLA_ERR_HIP (-2)         /* a HIP runtime call failed (text in pla_last_error) */
#define PLA_ERR_NOMEM (-3)       /* device or host allocation failed */
#define PLA_ERR_UNSUPPORTED (-4) /* shape outside what the kernels support */
#define PLA_ERR_NODEVICE (-5)    /* no usable AMD GPU */
#define PLA_ERR_FROZEN (-6)      /* the call needs to (re)allocate engine workspace while the engine is frozen */

/* element type of the log-likelihood / log-weight matrix */
#define PLA_F64 0
#define PLA_F32 1 /* read as f32, all arithmetic in f64 (hard part 5) */

#define PLA_HOST 0
#define PLA_DEVICE 1

/* importance-sampling method: ISMethod of base.py:18-23 */
#define PLA_PSIS 0
#define PLA_SIS 1
#define PLA_TIS 2

/* slots of the aggregate vector written by pla_psis_loo (all double) */
#define PLA_AGG_N 0           /* number of observations reduced                          */
#define PLA_AGG_SUM_LOO 1     /* sum_i loo_i                  (elpd_loo,  loo.py:326)      */
#define PLA_AGG_M2_LOO 2      /* sum_i (loo_i - mean)^2       (se, p_loo_se: loo.py:327,340) */
#define PLA_AGG_SUM_LPPD 3    /* sum_i lppd_i                 (loo.py:329-337)            */
#define PLA_AGG_N_HIGH 4      /* #(khat > good_k)             (loo.py:292-293)            */
#define PLA_AGG_N_NONFINITE 5 /* #(diagnostic not finite)                                 */
#define PLA_AGG_MIN_DIAG 6    /* min_i diagnostic             (min ESS, loo.py:306)       */
#define PLA_AGG_N_SLOW 7      /* rows that left the fast selection path (perf diagnostics) */
#define PLA_AGG_COUNT 8

typedef struct pla_engine pla_engine;

/* library / device ------------------------------------------------------------------- */
int pla_abi_version(void);
const char *pla_last_error(void); /* thread-local, valid until the next failing call */
int pla_device_count(int *count);

/* One engine per (process, GPU): owns the small device workspace (no per-call hipMalloc on
 * the PLA_DEVICE path, so calls can be captured in a hipGraph). */
int pla_engine_create(int device, pla_engine **out);
int pla_engine_destroy(pla_engine *eng);

/* frozen != 0: the workspace may no longer be reallocated (see "HIP graphs" above); 0 lifts it.  The reference has no
 * counterpart (it allocates per call: psis.py:92, base.py:125). */
int pla_engine_set_frozen(pla_engine *eng, int frozen);

/* M of base.py:139-141 / psis.py:89:  ceil(min(S/5, 3*sqrt(S/reff)));  cutoff_ind = -M-1 */
int pla_tail_count(int64_t n_draws, double reff, int64_t *tail_count);

/*
 * pla_psis_loo -- the fused per-observation LOO pass.
 * Replaces loo.py:286-342: compute_importance_weights(-ll) -> `log_weights += ll` ->
 * loo_i = scale * LSE_s(lw + ll) -> lppd_i = LSE_s(ll) - log S -> sums / variance / k counts,
 * i.e. the three Python loops of utils.py:137-142,171-175 over psis.py:114-160 and
 * utils.py:305-359, without ever materialising the (n_obs, n_draws) weight matrix.
 *
 *   ll          (n_obs, n_draws) log-likelihood, dtype PLA_F64 / PLA_F32, const
 *   method      PLA_PSIS / PLA_SIS / PLA_TIS
 *   tail_count  M from pla_tail_count (PSIS only; ignored otherwise)
 *   scale_value 1, -1 or -2 (loo.py:195-200); loo_i and the aggregates carry it
 *   good_k      threshold for PLA_AGG_N_HIGH (loo.py:249)
 *   diag        [n_obs] khat (PSIS) or ESS (SIS/TIS), always double (base.py:125); may be NULL
 *   loo_i       [n_obs] may be NULL          lppd_i [n_obs] may be NULL
 *   agg         [PLA_AGG_COUNT] may be NULL
 */
int pla_psis_loo(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws,
                 int64_t stride_obs, int64_t stride_draw, int method, int64_t tail_count,
                 double scale_value, double good_k, int mem_space, void *stream, double *diag,
                 double *loo_i, double *lppd_i, double *agg);

/*
 * pla_importance_weights -- smoothed, truncated, normalised log weights AND the diagnostic.
 * Replaces the batched dispatch of base.py:160-166 / psis.py:100-106 (the `_multi_ufunc`
 * loop over `_psislw` / `_sislw` / `_tislw`).
 *
 *   logw   (n_obs, n_draws) log importance ratios (for LOO: -log_likelihood), const
 *   lw_out (n_obs, n_draws) C-contiguous, same dtype as logw (base.py:125 empty_like)
 *   diag   [n_obs] double
 */
int pla_importance_weights(pla_engine *eng, const void *logw, int dtype, int64_t n_obs,
                           int64_t n_draws, int64_t stride_obs, int64_t stride_draw, int method,
                           int64_t tail_count, int mem_space, void *stream, void *lw_out,
                           double *diag);

/*
 * pla_reduce_pointwise -- only the reductions of loo.py:326-342,292-293 over pointwise
 * vectors already on the device/host (used after sharded runs and by tests).
 */
int pla_reduce_pointwise(pla_engine *eng, const double *diag, const double *loo_i,
                         const double *lppd_i, int64_t n_obs, double good_k, int mem_space,
                         void *stream, double *agg);

/*
 * pla_waic -- the WAIC pass: one read of the matrix.
 * Replaces waic.py:109-160: NaN -> -1e10 and +-inf -> +-1e10 on load (112-135),
 * lppd_i = LSE_s(ll) - log S (137-143, utils.py:305-359), var_i = population variance over draws (145),
 * waic_i = scale * (lppd_i - var_i) (158) and the sums of 159-161.
 *
 *   lppd_i, var_i, waic_i   [n_obs] double, each may be NULL
 *   agg  [PLA_AGG_COUNT] may be NULL, slots reused as
 *        PLA_AGG_N          n
 *        PLA_AGG_SUM_LOO    sum_i waic_i            (elpd_waic, waic.py:160)
 *        PLA_AGG_M2_LOO     sum_i (waic_i - mean)^2 (se = sqrt(M2), waic.py:159)
 *        PLA_AGG_SUM_LPPD   sum_i var_i             (p_waic, waic.py:161)
 *        PLA_AGG_N_HIGH     #(var_i > 0.4)          (warning, waic.py:147)
 *        PLA_AGG_MIN_DIAG   min_i var_i
 *        PLA_AGG_N_SLOW     entries replaced on load (NaN or +-inf: the front's two warnings)
 */
int pla_waic(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws,
             int64_t stride_obs, int64_t stride_draw, double scale_value, int mem_space, void *stream,
             double *lppd_i, double *var_i, double *waic_i, double *agg);

/*
 * pla_psis_loo_rows / pla_waic_rows -- the same two passes over a SELECTION of the rows of a resident matrix:
 * the subsampled LOO of loo_subsample.py:316-330 (`log_likelihood.isel(...)` on the sampled observations, then
 * compute_importance_weights + logsumexp, 373-386, and the variance over draws of the sampled rows, 389) without
 * materialising the gathered copy.
 *
 *   ll, n_obs, n_draws, strides   the full matrix, as in pla_psis_loo
 *   row_index  [n_rows] int64 observation indices into the matrix (repeats allowed), in the memory space of `ll`
 *              (device pointer for PLA_DEVICE).  Host lists are range-checked (PLA_ERR_ARG); device lists are
 *              clamped into [0, n_obs) on the device before use -- validate them before uploading.
 *   outputs    compact: entry r belongs to observation row_index[r]; [n_rows] each; agg as in the full-matrix call
 */
int pla_psis_loo_rows(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws,
                      int64_t stride_obs, int64_t stride_draw, const int64_t *row_index, int64_t n_rows,
                      int method, int64_t tail_count, double scale_value, double good_k, int mem_space,
                      void *stream, double *diag, double *loo_i, double *lppd_i, double *agg);
int pla_waic_rows(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws,
                  int64_t stride_obs, int64_t stride_draw, const int64_t *row_index, int64_t n_rows,
                  double scale_value, int mem_space, void *stream, double *lppd_i, double *var_i,
                  double *waic_i, double *agg);

/*
 * pla_group_sum / pla_psis_loo_groups -- leave-one-group-out (loo_group.py:216-300): the (n_obs, n_draws) matrix is reduced to
 * one row per group, the sums of its members' rows, and the PSIS / SIS / TIS pass of pla_psis_loo runs over those G rows.
 *
 *   ll, n_obs, n_draws, strides   the matrix, as in pla_psis_loo (draws contiguous is read in place; observations contiguous is
 *                 transposed block by block on the device; other strides: PLA_ERR_UNSUPPORTED)
 *   group_offsets [n_groups + 1], group_members [group_offsets[n_groups]]  int64, in the memory space of `ll`: the members of
 *                 group g are group_members[group_offsets[g] .. group_offsets[g+1]), observation indices in ascending order.  The
 *                 groups need not cover every observation.  Host lists are checked (offsets start at 0 and never decrease,
 *                 members in [0, n_obs) and ascending within a group: PLA_ERR_ARG); device lists are clamped into range on the
 *                 device, as pla_psis_loo_rows does -- validate them before uploading.
 *   group sums    out[g, s] = ll[m0, s] + ll[m1, s] + ... over the members in ascending order, one rounding per add, in the dtype of
 *                 ll (f32 sums stay f32): bitwise NumPy's `ll[members].sum(axis=0)` (loo_group.py:221).  NaN entries count as -1e10
 *                 (loo_group.py:188-197) and are counted in *n_replaced (memory space of ll; may be NULL); +-inf are not replaced.
 *   pla_group_sum        out (n_groups, n_draws) C-contiguous, dtype of ll, in the memory space of ll
 *   pla_psis_loo_groups  diag / logo_i / lppd_i [n_groups] double (each may be NULL), agg [PLA_AGG_COUNT] as pla_psis_loo's, reduced
 *                 over the groups (n_groups >= 1).  The sums are built one block of groups at a time in a bounded engine buffer
 *                 (sized like the ingest staging: PLA_INGEST_BLOCK_MB on the device), each block's pass writes its slices,
 *                 the aggregates are reduced once at the end: the results do not depend on the block size.  A host matrix, or an
 *                 observations-fastest one, whose group sums fill more than one block is read once per block.
 */
/* sums of the rows of each group (loo_group.py:216-224); out (n_groups, n_draws) C-contiguous, dtype of ll */
int pla_group_sum(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws,
                  int64_t stride_obs, int64_t stride_draw, const int64_t *group_offsets,
                  const int64_t *group_members, int64_t n_groups, int mem_space, void *stream,
                  void *out, int64_t *n_replaced /* may be NULL */);

/* the LOGO pass (loo_group.py:216-300): group sums -> PSIS/SIS/TIS pass over the G rows; outputs per group,
   agg as pla_psis_loo's over the groups */
int pla_psis_loo_groups(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws,
                        int64_t stride_obs, int64_t stride_draw, const int64_t *group_offsets,
                        const int64_t *group_members, int64_t n_groups, int method, int64_t tail_count,
                        double scale_value, double good_k, int mem_space, void *stream, double *diag,
                        double *logo_i, double *lppd_i, double *agg, int64_t *n_replaced);

/*
 * pla_gather_draws / pla_psis_loo_draws -- PSIS-LOO for draws of an approximate posterior (loo_approximate_posterior.py:223-348):
 * the matrix with its draws taken in the order and multiplicity of an index (the importance-resampled draws, line 263), and the
 * PSIS / SIS / TIS pass of pla_psis_loo over that matrix, without the matrix ever being materialised whole.
 *
 *   ll, n_obs, n_draws, strides   the matrix, as in pla_psis_loo.  Device matrices: any positive strides (draws contiguous with rows
 *                 of at most pla_gather_lds_max_draws(dtype) draws are staged row by row in LDS and read once; observations
 *                 contiguous goes through an LDS tile; everything else is gathered straight from global memory).  Host matrices:
 *                 draws contiguous or observations contiguous, uploaded block by block and gathered on the device.
 *   draw_index [n_out]  int64, in the memory space of `ll`; repeats allowed, 1 <= n_out <= 2^30, n_out need not equal n_draws.  Host
 *                 lists are checked (entries in [0, n_draws): PLA_ERR_ARG); device lists are clamped into range on the device.
 *   NaN entries   count as -1e10 in the dtype of ll (loo_approximate_posterior.py:223-232) and are counted in *n_replaced (memory
 *                 space of ll; may be NULL): the number of NaN entries of ll[:, draw_index].  +-inf are not replaced.
 *   pla_gather_draws     out (n_obs, n_out) C-contiguous, dtype of ll, in the memory space of ll
 *   pla_psis_loo_draws   diag / loo_i / lppd_i [n_obs] double (each may be NULL), agg [PLA_AGG_COUNT] as pla_psis_loo's; tail_count
 *                 refers to n_out.  Blocks of observations (sized like the ingest staging: PLA_INGEST_BLOCK_MB on the device) are
 *                 gathered into the engine's staging buffer, each block's pass writes its slices, the aggregates are reduced once
 *                 at the end.  Everything is enqueued on the caller's stream; once the workspace is sized nothing is allocated, so
 *                 the device call can be captured after pla_engine_set_frozen.
 *   contract      pla_gather_draws is bitwise ll[:, draw_index] (NaN replaced); the pointwise outputs of pla_psis_loo_draws are
 *                 bitwise those of pla_psis_loo on that matrix uploaded draws-fastest, the aggregates agree to 1e-12 relative
 *                 (another reduction order).  The results do not depend on the block size, on host or device input, or on the
 *                 layout of ll.
 *   pla_gather_lds_max_draws   the longest row (n_draws) the LDS route takes for a dtype (PLA_F64 / PLA_F32)
 */
int pla_gather_draws(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws,
                     int64_t stride_obs, int64_t stride_draw, const int64_t *draw_index, int64_t n_out,
                     int mem_space, void *stream, void *out, int64_t *n_replaced /* may be NULL */);

int pla_psis_loo_draws(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws,
                       int64_t stride_obs, int64_t stride_draw, const int64_t *draw_index, int64_t n_out,
                       int method, int64_t tail_count, double scale_value, double good_k, int mem_space,
                       void *stream, double *diag, double *loo_i, double *lppd_i, double *agg,
                       int64_t *n_replaced);

int pla_gather_lds_max_draws(int dtype);

/*
 * pla_kfold_lme / pla_kfold_reduce -- K-fold cross-validation from per-fold log-likelihoods (loo_kfold.py:250-299, 643-692): the
 * log mean exp of every held-out observation under its own fold's draws and of every observation under the full fit in ONE
 * ragged pass over the resident matrices, and the pointwise values, sums and standard-error moments behind it.  The refits are
 * the caller's.
 *
 * pla_kfold_lme
 *   sources       n_sources matrices of one dtype in DEVICE memory, described by parallel HOST arrays (uploaded by the call, 40
 *                 bytes a source): src_base[k], src_rows[k], src_draws[k] (1 .. 2^30), src_stride_row[k] >= 0 and
 *                 src_stride_draw[k] > 0 in elements.  Source 0 is the full fit by convention: with nan_flag != 0 its NaN entries
 *                 count as -1e10 (loo_kfold.py:250-259) and are counted in *n_replaced (device, zeroed by the call; may be NULL).
 *                 Nothing else is replaced anywhere: a NaN, a +inf or a row of -inf give NaN, as utils.py:344-357 does.
 *   tasks         source_offsets [n_sources + 1], task_row [n_tasks], task_out [n_tasks]: int64 in DEVICE memory.  Tasks
 *                 [source_offsets[k], source_offsets[k + 1]) belong to source k; task t writes
 *                     out[task_out[t]] = logsumexp_s(ll_k[task_row[t], :]) - log(src_draws[k])          (f32 reduced in f64)
 *                 task_row is clamped into the source, a task_out outside [0, n_out) is dropped.
 *   routes        per source: unit draw stride, 16-byte aligned rows, at most 4096 draws -> a wavefront per task, the row in
 *                 registers; unit row stride (observations fastest) -> a lane per task; anything else -> a workgroup per task.
 *                 One launch per route present, whatever n_sources is; pla_engine_last_kernels names them.
 *   mem_space     PLA_DEVICE.  PLA_HOST returns PLA_ERR_UNSUPPORTED (the Python engine uploads).
 * pla_kfold_reduce   elpd [n_obs] (held-out), lpd_full [n_obs], n_replaced (may be NULL): device.  Writes p_i = lpd_full - elpd and
 *                 kfold_i = scale * elpd ([n_obs] each, may be NULL) and agg [PLA_AGG_COUNT], the slots of pla_psis_loo reused:
 *                     [PLA_AGG_N] n_obs, [PLA_AGG_SUM_LOO] sum kfold_i, [PLA_AGG_M2_LOO] sum (kfold_i - mean)^2,
 *                     [PLA_AGG_SUM_LPPD] sum p_i, [PLA_AGG_N_HIGH] sum (p_i - mean)^2, [PLA_AGG_N_NONFINITE] *n_replaced, others 0
 *                 (both M2 two-pass about the mean, as np.var: se = sqrt(M2)).  The observations are cut into tiles whose width
 *                 depends on n_obs alone and the partials are combined in a fixed order: the same input gives the same bits
 *                 whatever the grid (pla_engine_set_compare_grid caps it).
 * Everything is enqueued on the caller's stream.  pla_kfold_lme keeps the table in two pinned host buffers used in turn: a call
 * waits on the host for the table upload of the call BEFORE THE PREVIOUS ONE (done long ago unless two calls are still queued), and
 * the first two calls, or a larger table, allocate pinned memory (not allowed once the engine is frozen).  pla_engine_last_kernels
 * also states how many kernels the ragged pass launched.
 */
int pla_kfold_lme(pla_engine *eng, const void *const *src_base, const int64_t *src_rows, const int64_t *src_draws,
                  const int64_t *src_stride_row, const int64_t *src_stride_draw, int64_t n_sources, int dtype,
                  int nan_flag, const int64_t *source_offsets, const int64_t *task_row, const int64_t *task_out,
                  int64_t n_tasks, int mem_space, void *stream, double *out, int64_t n_out,
                  int64_t *n_replaced /* may be NULL */);

int pla_kfold_reduce(pla_engine *eng, const double *elpd, const double *lpd_full, int64_t n_obs, double scale,
                     const int64_t *n_replaced /* may be NULL */, int mem_space, void *stream, double *p_i,
                     double *kfold_i, double *agg);

/*
 * pla_mm_moments / pla_mm_transform / pla_mm_ratios -- the batched arithmetic of moment matching (loo_moment_match.py:656-914,
 * split_moment_match.py:132-252) for B observations at once.  f64, DEVICE pointers only, contiguous arrays, everything enqueued on
 * the caller's stream; the model evaluations between the calls and the D x D factorisations are the caller's.  n_draws >= 2.
 *
 * pla_mm_moments   upars (B, S, D), lw (B, S) log weights -> stats (B, 4, D): the plain mean, the weighted mean sum exp(lw) x,
 *                  np.var (ddof 0) and the raw weighted second moment (sum w x^2 - wmean^2) * S / (S - 1) of shift_and_scale(), kept
 *                  in that one-pass form; with want_cov != 0 also cov (B, 2, D, D): np.cov(rowvar=False) and np.cov(aweights=w),
 *                  centred on the plain mean and on the weighted average (two passes), divisors S - 1 and W - W2 / W.  Several
 *                  workgroups per b over tiles of S, the per-tile partials added in tile order by a second launch, no
 *                  floating-point atomics: the bits depend neither on the grid (pla_engine_set_compare_grid caps it) nor on B.
 *                  D <= 64 with want_cov, D <= 1024 without (PLA_ERR_UNSUPPORTED beyond).
 * pla_mm_transform out[b, s, :] = (((x[b, s, :] - m0[b]) * pre[b]) . map[b]^T) / post_div[b] + m1[b] for rows s in [row_lo, row_hi),
 *                  out[b, s, :] = x[b, s, :] for the others.  pre, map (B, D, D) and post_div may be NULL; x is (S, D) at
 *                  x + b * x_batch_stride (0: one matrix for every b).  Without a matrix every operation is rounded as written
 *                  (NumPy's bits).  D <= 64 with a matrix.  Not in place.
 * pla_mm_ratios    mode 0: a = ll_new, b = lp_new (B, S), c = lp_orig (S) -> out (2B, S): rows [0, B) -ll + lp - lp_orig, rows
 *                  [B, 2B) lp - lp_orig, NaN -> -inf.  mode 1: a = ll_half, b = lp_half, c = lp_half_inv (B, S), jac (B, 2) = (sum
 *                  log total_scaling, log |det total_mapping|) -> out (B, S): the multiple-importance-sampling log weights of the
 *                  split step, log1p(exp(.)) on the stable side, NaN / +inf -> -inf.  mode 2: out = a + b, NaN / +inf -> -inf.
 *                  mode 3: a = ll, b = lw (B, S) -> out (B, 2): logsumexp(ll + lw) and logsumexp(ll) - log S, one wave per row.
 */
int pla_mm_moments(pla_engine *eng, const double *upars, const double *lw, int64_t n_batch, int64_t n_draws,
                   int64_t n_dim, int want_cov, void *stream, double *stats, double *cov /* NULL without want_cov */);
int pla_mm_transform(pla_engine *eng, const double *x, int64_t x_batch_stride, const double *m0,
                     const double *pre /* may be NULL */, const double *map /* may be NULL */,
                     const double *post_div /* may be NULL */, const double *m1, int64_t n_batch, int64_t n_draws,
                     int64_t n_dim, int64_t row_lo, int64_t row_hi, void *stream, double *out);
int pla_mm_ratios(pla_engine *eng, int mode, const double *a, const double *b, const double *c, const double *jac,
                  int64_t n_batch, int64_t n_draws, void *stream, double *out);

/*
 * pla_mixis_draw_lse / pla_mixis_loo -- Mix-IS-LOO (Silva & Zanella 2022; the estimator loo.py:252-284 and elpd.py:364-374
 * document) in two passes over the (n_obs, n_draws) matrix, one log-sum-exp along each axis:
 *     c[s]     = log sum_i exp(-ll[i, s])                                  pla_mixis_draw_lse: one value per DRAW
 *     loo_i[i] = scale_value * (LSE_s(-c) - LSE_s(-ll[i, s] - c[s]))       pla_mixis_loo
 * (The reference's code reduces the first sum over the draws, which makes every pointwise value the same constant; DESIGN.md
 * section 10 has the finding and a 2 x 2 case.)  No Pareto fit, no refit.  All arithmetic is f64, f32 is widened on load.  On load
 * NaN counts as -1e10, +inf as +1e10 and -inf as -1e10, in both passes alike; everything behind the load is plain IEEE.
 *
 *   ll, dtype, n_obs, n_draws, strides   as pla_psis_loo; 1 <= n_obs < 2^40, 1 <= n_draws <= 2^30.  PLA_DEVICE: any strides, read
 *                in place.  PLA_HOST: unit stride along the draws or along the observations (other strides:
 *                PLA_ERR_UNSUPPORTED); the matrix goes through the staging buffer in blocks of whole tiles of pass 1 (1 GiB, or
 *                PLA_INGEST_BLOCK_MB), each in the matrix's own layout, ONCE PER PASS: pla_mixis_draw_lse followed by
 *                pla_mixis_loo, or pla_mixis_loo without a c, move it to the device twice.  The staged kernels are those a compact
 *                (pitch = line length), 16-byte aligned device matrix of that layout gets: such a device matrix and the host
 *                matrix give the same bits, whatever the block size.  (A device matrix with a padded pitch or an unaligned base
 *                may take the other vector width of the line / register-row kernels and differ in the last bits.)
 *   c            [n_draws] double in the memory space of ll.  pla_mixis_draw_lse writes it; pla_mixis_loo reads it, or computes it
 *                itself when it is NULL (one call, two passes).  It is an argument so that the front reports the replaced
 *                entries once and a sharded caller can merge c across ranks between the passes.
 *   n_replaced   [2] int64 in the memory space of ll (may be NULL): NaN entries, +-inf entries met by pass 1
 *   loo_i        [n_obs] double (may be NULL)
 *   agg          [PLA_AGG_COUNT] (may be NULL), the slots of pla_psis_loo reused: [PLA_AGG_N] n_obs, [PLA_AGG_SUM_LOO] sum loo_i,
 *                [PLA_AGG_M2_LOO] sum (loo_i - mean)^2 (two-pass about the mean, as np.var: se = sqrt(M2)), [PLA_AGG_N_SLOW] the
 *                entries pass 2 replaced on load (NaN and +-inf together, as pla_waic), the others 0
 *   routes       pass 1 cuts the observations into tiles of pla_mixis_tile_rows(n_obs) rows -- max(256, ceil(n_obs / 128) rounded
 *                up to 256), a rule of n_obs alone, so at most 128 tiles -- keeps one (maximum, rescaled sum) per tile and draw in
 *                a slab of engine workspace (2 * tiles * n_draws doubles: at most 2048 * n_draws bytes) and merges a draw's
 *                partials in tile order.  Unit draw stride: lanes own adjacent draws and walk down a tile's rows; unit
 *                observation stride: a wavefront per (draw, tile) reads its piece of the draw's line with 16-byte loads (element
 *                loads when the lines are not 16-byte aligned); other strides: the first kernel with both strides.  Pass 2, unit
 *                draw stride: a wavefront per observation -- rows of at most 4096 draws in its registers with c staged in LDS
 *                (exact maximum, then the sum), longer rows streamed with c read through L2; unit observation stride: a lane per
 *                observation, c[s] wave-uniform in a scalar register (scalar loads); other strides: a workgroup per observation.  The scale and the aggregates are
 *                the tile-ordered finishing pass of pla_kfold_reduce.  No floating-point atomics anywhere: the same input gives
 *                the same bits whatever the grid (pla_engine_set_mixis_grid caps the workgroups of every launch; 0: the
 *                library's choice).  pla_engine_last_kernels names the kernels taken.
 * pla_mixis_tile_rows needs no engine and no GPU; it returns the tile height (> 0) or a negative status.
 * Everything is enqueued on the caller's stream; PLA_HOST calls return when the results are in the caller's arrays.
 */
int pla_mixis_draw_lse(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                       int64_t stride_draw, int mem_space, void *stream, double *c,
                       int64_t *n_replaced /* [2], may be NULL */);
int pla_mixis_loo(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                  int64_t stride_draw, const double *c /* NULL: computed by the call */, double scale_value, int mem_space,
                  void *stream, double *loo_i /* may be NULL */, double *agg /* may be NULL */);
int pla_engine_set_mixis_grid(pla_engine *eng, int max_workgroups);
int pla_mixis_tile_rows(int64_t n_obs);

/*
 * pla_e_loo -- PSIS-weighted expectations of a same-shape matrix and their function-specific Pareto k.
 * Replaces, per observation, e_loo.py:214-236: `_normalize_log_weights` + `_compute_weighted_mean` (430-437, 557-559),
 * `_compute_weighted_variance` / `_wvar_func` (440-459, 518-531; sd = sqrt(variance), 462-465) and `compute_pareto_k` ->
 * `k_hat` (266-390) for h = x (mean), h = x^2 (variance / sd) and h = None (quantiles), i.e. the `wrap_xarray_ufunc` loops of
 * e_loo.py:315-324, 448-457 and the callers on top of psislw: loo_score.py:227,312, loo_predictive_metric.py:208.
 *
 *   x            (n_obs, n_draws) draws to average (posterior-predictive or posterior values), const
 *   log_weights  (n_obs, n_draws) log importance weights, any normalisation (the smoothed weights of
 *                pla_importance_weights; `weights=` callers pass log(weights), e_loo.py:202-203)
 *   log_ratios   (n_obs, n_draws) raw log ratios for the diagnostics, or NULL = log_weights (e_loo.py:223-224)
 *                -- all three share dtype, shape and strides
 *   tail_len     draws per tail in k_hat (20: e_loo.py:269); >= 5
 *   mean, variance, k_mean, k_var, k_ratio   [n_obs] double, each may be NULL
 *                k_mean = k_hat(x, lr), k_var = k_hat(x^2, lr), k_ratio = k_hat(None, lr)
 * In-band semantics as in the reference: NaN / inf in x flow into mean and variance by IEEE rules and switch k to the
 * ratio-only value (e_loo.py:359-366); constant x gives variance 0 (520-521).  k_hat is reproduced AS THE REFERENCE EVALUATES
 * IT, including the descending tails it hands to `_gpdfit` (see csrc/pla_eloo.h for what that implies).
 */
int pla_e_loo(pla_engine *eng, const void *x, const void *log_weights, const void *log_ratios, int dtype,
              int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw, int64_t tail_len,
              int mem_space, void *stream, double *mean, double *variance, double *k_mean, double *k_var,
              double *k_ratio);

/*
 * pla_e_loo_quantiles -- PSIS-weighted quantiles of the draws (e_loo(type="quantile")).
 * Replaces `_compute_weighted_quantiles` (e_loo.py:468-515: the `np.ndindex` loop over observations and probabilities) and
 * `_weighted_quantile` (534-554): argsort + cumulative normalised weights + linear interpolation between the two draws that
 * bracket `prob`; np.quantile(x, prob) when the weights are all close (536-537).  No sort on the device: a weighted radix
 * selection per (observation, prob) -- see csrc/pla_eloo.h.
 *
 *   x, log_weights  (n_obs, n_draws), same dtype and strides, as in pla_e_loo
 *   probs           [n_probs] HOST array (whatever mem_space says), each strictly between 0 and 1 (e_loo.py:158-159)
 *   out             [n_obs][n_probs] double, in the memory space of the matrices
 * The Pareto k of this type is pla_e_loo's k_ratio (e_loo.py:229-230).
 */
int pla_e_loo_quantiles(pla_engine *eng, const void *x, const void *log_weights, int dtype, int64_t n_obs,
                        int64_t n_draws, int64_t stride_obs, int64_t stride_draw, const double *probs,
                        int64_t n_probs, int mem_space, void *stream, double *out);

/*
 * Model comparison -- loo_compare's weights and standard errors (compare.py:205-229, 477-577).
 * The pointwise values of K models (loo_i / waic_i) as a (n_models, n_obs) matrix `x`: row k at x + k * pitch (ELEMENTS), dtype
 * PLA_F64 or PLA_F32 (promoted on load), in `mem_space` (a host matrix is uploaded once per call).  1 <= n_models <=
 * PLA_COMPARE_MAX_MODELS (more: PLA_ERR_UNSUPPORTED); 1 <= n_obs < 2^32.  `scale_mul` multiplies every value on load: 1 ("log"), -1
 * ("negative_log") or -0.5 ("deviance") bring a table to the log scale as compare.py:489-492 / 556-559 do.  Every reduction goes
 * through fixed per-tile partials in engine workspace, combined in tile order (csrc/pla_compare.h): two calls on the same input give
 * the same bits, whatever the grid or the device.
 *
 * pla_compare_moments  the diff / dse arithmetic of compare.py:214-229.  out [3 * n_models + 1] double, memory space of x:
 *                      out[3k] = sum_i x_ik, out[3k+1] = mean_i d_ik, out[3k+2] = sum_i (d_ik - mean)^2 with d_ik = x_ik - x_{best,i}
 *                      (dse_k = sqrt(N * var(d_k)) = sqrt(out[3k+2]): compare.py:226-227), out[3K] = sum_i max_k x_ik.  The values are
 *                      taken as they are (the dse is on the table's own scale).
 * pla_stacking_eval    one evaluation of the stacking objective and its gradient (compare.py:494-514) at the weights w [n_models]
 *                      (HOST array): with m_i = max_k x'_ik, e_ik = exp(x'_ik - m_i), d_i = sum_k w_k e_ik:  out[0] = sum_i log d_i,
 *                      out[1 + k] = sum_i e_ik / d_i.  out [n_models + 1] is a HOST array; the call synchronises `stream`.
 * pla_bb_bootstrap     the Bayesian bootstrap of compare.py:551-571 without its (n_boot, n_obs) Dirichlet matrix: z [n_boot][n_models],
 *                      memory space of x, z_bk = n_obs * scale_mul * sum_i G_bi x_ik / sum_i G_bi with G_bi ~ Gamma(alpha, 1) drawn in
 *                      the kernel from the Philox4x32-10 stream specified in csrc/pla_compare.h (key = seed, counter = (i, b, attempt,
 *                      sub-block): a pure function of (seed, alpha, b, i)).  alpha > 0, 1 <= n_boot <= 2^32.  The partials of up to
 *                      64 MiB of replicates live in engine workspace; more replicates run in several launches.
 * pla_bb_gamma_draws   the same stream on its own, for tests: out [n_boot][n_obs] double (memory space mem_space) = G_bi,
 *                      n_boot * n_obs <= 2^31.
 * pla_engine_set_compare_grid  caps the workgroups per launch of the three passes above (0: the library's choice); the results do not
 *                      depend on it.
 */
#define PLA_COMPARE_MAX_MODELS 64
int pla_compare_moments(pla_engine *eng, const void *x, int dtype, int64_t n_models, int64_t n_obs, int64_t pitch,
                        int64_t best, int mem_space, void *stream, double *out);
int pla_stacking_eval(pla_engine *eng, const void *x, int dtype, int64_t n_models, int64_t n_obs, int64_t pitch,
                      double scale_mul, const double *weights, int mem_space, void *stream, double *out);
int pla_bb_bootstrap(pla_engine *eng, const void *x, int dtype, int64_t n_models, int64_t n_obs, int64_t pitch,
                     double scale_mul, int64_t n_boot, double alpha, uint64_t seed, int mem_space, void *stream,
                     double *z);
int pla_bb_gamma_draws(pla_engine *eng, uint64_t seed, double alpha, int64_t n_boot, int64_t n_obs, int mem_space,
                       void *stream, double *out);
int pla_engine_set_compare_grid(pla_engine *eng, int max_workgroups);

/*
 * Non-factorised LOO -- loo_nonfactor's conditional log-likelihood for one joint multivariate normal or Student-t model
 * (loo_nonfactor.py:466-557, and compute_beta_minus_i 686-733 in closed form).  For draw s, with C_s the given matrix, r = y - mu_s,
 * P = C_s^-1, c_i = P_ii and g = P r:
 *   PLA_MVN_NORMAL     ll_is = -log(2 pi)/2 + log(c_i)/2 - g_i^2 / (2 c_i)                                         (490-497)
 *   PLA_MVN_STUDENT_T  with nu = df_s + N - 1 and beta_i = r'g - g_i^2 / c_i, sigma_i = (df_s + beta_i) / nu / c_i:
 *                      ll_is = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi sigma_i)/2 - (nu+1)/2 log(1 + (g_i/c_i)^2 / (nu sigma_i))
 *                                                                                                                 (498-557)
 * The matrix is inverted whether it is a covariance or a precision matrix: the reference does so (478), and so does this call.
 * Inputs: y [n_obs], mu (draw s at mu + s * mu_pitch), mat (draw s at mat + s * mat_pitch, each C-contiguous n_obs x n_obs), df
 * [n_draws] (PLA_MVN_STUDENT_T only; may be NULL otherwise), all of `dtype` (PLA_F32 is promoted on load; all arithmetic is f64),
 * all in `mem_space`.  Host inputs are staged to the device in blocks of draws of PLA_INGEST_BLOCK_MB (default 1 GiB).
 * Outputs in `mem_space`: out_ll (ll of (i, s) at out_ll[i * ll_stride_obs + s * ll_stride_draw], f64; host calls need
 * ll_stride_draw == 1; the LOO pass reads (n_obs, n_draws) with the draws fastest) and flags [n_draws] int32, the status of each draw:
 *   PLA_NF_GENERAL          the general route (LU with partial pivoting) computed it
 *   PLA_NF_SINGULAR         an exact zero pivot (numpy.linalg.inv's LinAlgError, 479-481): an all -inf row, no df check
 *   PLA_NF_NONFINITE        a non-finite entry in the matrix, mu_s or y: an all -inf row (the reference's NaN inverse, 559-571)
 *   PLA_NF_DF_NONPOS        df_s <= 0 (509-516): an all -inf row
 *   PLA_NF_BETA_NONFINITE   some beta_i not finite (525-533): those entries -inf
 *   PLA_NF_CLAMPED          some c_i <= 0, clamped to DBL_EPSILON (what 486-488 intends; the reference raises there instead)
 * NaN log-likelihoods are returned as they are (the front replaces them with -inf, 559-571).
 * Routes (pla_engine_set_nonfactor_route; csrc/pla_nonfactor.h): PLA_NF_ROUTE_AUTO (0): LDS for n_obs <= the LDS bound
 * (pla_nonfactor_lds_max_obs), the blocked route above it (16-column panels, trailing updates on the f64 matrix cores);
 * PLA_NF_ROUTE_LDS: the LDS route where n_obs allows it; PLA_NF_ROUTE_WORKSPACE: the blocked route; PLA_NF_ROUTE_GENERAL: every
 * draw through LU.  The Cholesky routes leave draws that are not symmetric
 * within 1e-12 relative or not numerically positive definite to the general route.  Every draw is computed by one workgroup in a
 * fixed order: the output bits do not depend on the route grid (pla_engine_set_nonfactor_grid), the staging block, host vs device
 * input, or f32 vs the same values as f64.  n_obs > PLA_NONFACTOR_MAX_OBS: PLA_ERR_UNSUPPORTED.
 */
#define PLA_NONFACTOR_MAX_OBS 1024
#define PLA_MVN_NORMAL 0
#define PLA_MVN_STUDENT_T 1
#define PLA_NF_GENERAL 1
#define PLA_NF_SINGULAR 2
#define PLA_NF_NONFINITE 4
#define PLA_NF_DF_NONPOS 8
#define PLA_NF_BETA_NONFINITE 16
#define PLA_NF_CLAMPED 32
#define PLA_NF_ROUTE_AUTO 0
#define PLA_NF_ROUTE_LDS 1
#define PLA_NF_ROUTE_WORKSPACE 2
#define PLA_NF_ROUTE_GENERAL 3
int pla_nonfactor_loglik(pla_engine *eng, const void *y, const void *mu, const void *mat, const void *df, int dtype, int64_t n_obs,
                         int64_t n_draws, int64_t mu_pitch, int64_t mat_pitch, int model_type, int mem_space, void *stream,
                         double *out_ll, int64_t ll_stride_obs, int64_t ll_stride_draw, int32_t *flags);
int pla_engine_set_nonfactor_route(pla_engine *eng, int route);
int pla_engine_set_nonfactor_grid(pla_engine *eng, int max_workgroups);
int pla_nonfactor_lds_max_obs(void);

/*
 * LOO-PIT, the leave-one-out probability integral transform (ArviZ's loo_pit; csrc/pla_pit.h), per observation i:
 *     pit_le[i] = sum_{y_hat[i,s] <= y[i]} w[i,s]        pit_lt[i] = sum_{y_hat[i,s] < y[i]} w[i,s]
 * with w[i,.] the normalised leave-one-out weights of observation i and y_hat[i,.] its posterior-predictive draws.  `in` and y_hat
 * are (n_obs, n_draws) matrices of one dtype, each with its own strides (elements); y is [n_obs] doubles.
 *   PLA_PIT_LOGLIK       in = pointwise log-likelihood.  One block of observations at a time (PLA_INGEST_BLOCK_MB, as
 *                        pla_psis_loo_draws sizes its blocks): -in with NaN -> -1e10 (counted in *n_replaced) into the ingest
 *                        staging, the weights pass of pla_importance_weights (method, tail_count) into a second bounded buffer,
 *                        the PIT kernel against y_hat -- read in place, or, observations fastest, transposed block by block
 *                        into a third.  diag[n_obs] (may be NULL) receives the Pareto k of PLA_PSIS.  The results do not depend
 *                        on the block size, bitwise.
 *   PLA_PIT_LOG_WEIGHTS  in = log weights of any normalisation (psislw's output): used as they are, w = softmax over the draws;
 *                        method, tail_count and diag are ignored, *n_replaced = 0.  Device pointers: the PIT kernel alone, both
 *                        matrices read in place.
 * All arithmetic is f64; comparisons are IEEE (a NaN draw or a NaN y[i] is never counted), a weight of log -inf is 0, a row whose
 * weights are all NaN or all -inf gives NaN.  The three sums behind the two values take one term per draw in one fixed order:
 * pit_lt[i] == pit_le[i] bit for bit when no draw equals y[i], exactly 1 when every draw is <= y[i], exactly 0 when none is; the
 * same input gives the same bits on every call.
 * PLA_DEVICE: everything is enqueued on `stream`, the outputs and n_replaced (one int64) are device pointers, and nothing is
 * allocated once the workspace fits (pla_engine_set_frozen).  PLA_HOST: each matrix draws-fastest (unit draw stride) or
 * observations-fastest (unit observation stride, draw stride >= n_obs), staged in 1 GiB blocks; other strides return
 * PLA_ERR_UNSUPPORTED.  pit_lt, diag and n_replaced may be NULL.  PLA_ERR_ARG: a NULL matrix, y or pit_le, n_draws < 2, a bad
 * kind or method, a stride that is not positive.
 */
#define PLA_PIT_LOGLIK 0       /* in = pointwise log-likelihood: weights = PSIS/SIS/TIS of -in (NaN -> -1e10) */
#define PLA_PIT_LOG_WEIGHTS 1  /* in = log weights of any normalisation (e.g. psislw's output): used as they are */
int pla_loo_pit(pla_engine *eng, const void *in, const void *y_hat, const double *y, int dtype, int64_t n_obs, int64_t n_draws,
                int64_t stride_obs, int64_t stride_draw, int64_t yh_stride_obs, int64_t yh_stride_draw, int input_kind, int method,
                int64_t tail_count, int mem_space, void *stream, double *pit_le, double *pit_lt /* may be NULL */,
                double *diag /* may be NULL; written only for PLA_PIT_LOGLIK */, int64_t *n_replaced /* may be NULL */);

/*
 * LOO diagnostics per observation (csrc/pla_diag.h): how many effective draws stand behind loo_i and what its Monte Carlo error
 * is.  With ll row i of the log-likelihood (NaN counted as -1e10, +-inf kept), lw its log weights, m = max_s lw_s,
 * e_s = exp(lw_s - m) and w_s = e_s / sum e (a weight of log -inf is 0 and the draw contributes to nothing):
 *     elpd_i[i]  = LSE_s(lw_s + ll_s) - LSE_s(lw_s)
 *     ess_w[i]   = (sum e_s)^2 / sum e_s^2                                       (= 1 / sum w_s^2, in [1, n_draws])
 *     var_log[i] = log1p( sum_s w_s^2 (exp(ll_s - elpd_i) - 1)^2 )
 * var_log is the variance of the self-normalised importance-sampling estimator on the linear scale (Vehtari et al. 2024, eq. 6)
 * over its square, moved to the log scale by log-normal moment matching.  With the relative efficiency r_eff of observation i
 * (pla_relative_eff): n_eff = r_eff ess_w, mcse_elpd_i = sqrt(var_log / r_eff), mcse_elpd_loo = sqrt(sum mcse_elpd_i^2).
 * All arithmetic is f64 (f32 input is widened on load).  A row whose weights are all NaN or all -inf, a row with a NaN weight or a
 * NaN ll, and a row whose elpd_i is -inf (every ll -inf) give NaN in the three values.  Rows with k = +inf are computed on their
 * unsmoothed weights.  No floating-point atomics; the order of each sum is a rule of n_draws and the dtype alone, so the bits do
 * not depend on the grid, the block size (PLA_INGEST_BLOCK_MB), the memory space, the layout or the load mode.
 *
 * pla_loo_diag          ll (n_obs, n_draws) -> the weights of -ll by `method` and tail_count exactly as pla_importance_weights
 *                       computes them, then the three values; diag receives Pareto k (PLA_PSIS) or the ESS (PLA_SIS / PLA_TIS).
 *                       One block of rows at a time, as pla_loo_pit: -ll into the ingest staging, the weights pass into a second
 *                       bounded buffer, the diagnostics kernel on both before the next block overwrites either.  row_index (NULL:
 *                       every row, n_rows is ignored) selects n_rows rows, repeats allowed; the list lives where the matrix lives:
 *                       a device list is clamped into [0, n_obs), a host list out of range is PLA_ERR_ARG.  The outputs are
 *                       compact, one entry per selected row, and each may be NULL; *n_replaced (may be NULL) counts the NaN
 *                       entries of the selected rows.  Layouts: draws fastest or observations fastest in either memory space (an
 *                       observations-fastest matrix with a row_index: on the device through a gather that is correct, not fast;
 *                       on the host PLA_ERR_UNSUPPORTED), other host strides PLA_ERR_UNSUPPORTED.
 * pla_loo_diag_weights  the kernel alone on caller-supplied log weights of any normalisation (psislw's output, the weights of a
 *                       moment-matching result) and ll (NaN is not replaced here), two matrices of one dtype with their own
 *                       strides.  Device pointers are read in place, any positive strides; host matrices need unit draw strides
 *                       (PLA_ERR_UNSUPPORTED otherwise) and are staged in blocks.
 * PLA_DEVICE: everything is enqueued on `stream`, the outputs and n_replaced (one int64) are device pointers, and nothing is
 * allocated once the workspace fits (pla_engine_set_frozen).  PLA_HOST: the call returns when the results are there.
 */
int pla_loo_diag(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                 const int64_t *row_index /* NULL: every row */, int64_t n_rows, int method, int64_t tail_count, int mem_space,
                 void *stream, double *diag, double *elpd_i, double *ess_w, double *var_log, int64_t *n_replaced);
int pla_loo_diag_weights(pla_engine *eng, const void *lw, const void *ll, int dtype, int64_t n_obs, int64_t n_draws,
                         int64_t lw_stride_obs, int64_t lw_stride_draw, int64_t ll_stride_obs, int64_t ll_stride_draw,
                         int mem_space, void *stream, double *elpd_i, double *ess_w, double *var_log);

/*
 * LOO influence (csrc/pla_influence.h): what leaving observation i out does to the posterior of n_quant draw-wise quantities
 * theta[s, j] -- the Bayesian counterpart of DFBETAS and Cook's distance.  With lw row i of the log weights (of any normalisation),
 * m = max_s lw_s, e_s = exp(lw_s - m) (a weight of log -inf is 0 and the draw contributes to nothing) and
 * z_sj = (theta_sj - center_j) / scale_j:
 *     shift[i, j] = sum_s e_s z_sj / sum_s e_s             the standardised leave-one-out mean shift of quantity j
 *     m2[i, j]    = sum_s e_s z_sj^2 / sum_s e_s           its second moment (sd ratio = sqrt(max(m2 - shift^2, 0)))
 *     kl[i]       = sum_s e_s (lw_s - m) / sum e - log(sum e) + log(n_draws)     KL(p(. | y_-i) || p(. | y)) of the weighted draws
 *     ess_w[i]    = (sum e)^2 / sum e^2
 * A row whose weights are all NaN or all -inf, or hold a NaN or +inf, gives NaN in all four.  A scale_j that is zero or not finite
 * is the caller's to reject: the NaN or inf of the division is passed through.  All arithmetic is f64 (an f32 matrix is widened
 * on load); theta, center and scale are always f64.  The contraction W (n x S) . Z (S x P) runs on the f64 matrix cores; there are
 * no floating-point atomics and an observation's outputs depend on its own row, theta and n_draws alone -- not on the grid, the
 * block size (PLA_INGEST_BLOCK_MB), the position of the row, the position of the column or the load mode.
 *
 * The argument block carries its own size: set struct_size = sizeof(pla_influence_args); a call with another size is PLA_ERR_ARG.
 *   engine              the engine (NULL: PLA_ERR_ARG)
 *   mat, dtype, n_obs, n_draws, stride_obs, stride_draw      the matrix, strides in elements
 *   kind                PLA_PIT_LOGLIK: mat is the log-likelihood; the pipeline of pla_loo_diag (weights of -ll by method and
 *                       tail_count, one block of rows at a time), diag receives Pareto k / the ESS and *n_replaced the NaN count.
 *                       PLA_PIT_LOG_WEIGHTS: mat holds log weights; the kernel alone, device matrices read in place with any
 *                       positive strides, host matrices (unit stride along the draws) staged in blocks; row_index must be NULL,
 *                       diag is not written and *n_replaced is 0.
 *   row_index, n_rows   as pla_loo_diag (PLA_PIT_LOGLIK)
 *   method, tail_count  as pla_importance_weights (PLA_PIT_LOGLIK)
 *   theta, n_quant, theta_stride_draw, theta_stride_quant    n_draws x n_quant, 1 <= n_quant <= 1024; device: any positive strides;
 *                       host: dense, (n_draws, n_quant) or (n_quant, n_draws)
 *   center, scale       [n_quant]
 *   mem_space, stream   where EVERY pointer of the block lives; PLA_DEVICE: everything is enqueued on stream
 *   shift, m2           (m, n_quant) C-contiguous, m = n_rows with a row_index, else n_obs;  kl, ess_w, diag: [m];  n_replaced: one
 *                       int64.  Each output may be NULL.
 */
typedef struct pla_influence_args {
  int64_t struct_size;
  pla_engine *engine;
  const void *mat;
  int32_t dtype, kind, method, mem_space;
  int64_t n_obs, n_draws, stride_obs, stride_draw;
  const int64_t *row_index;
  int64_t n_rows, tail_count;
  const double *theta;
  int64_t n_quant, theta_stride_draw, theta_stride_quant;
  const double *center, *scale;
  void *stream;
  double *shift, *m2, *kl, *ess_w, *diag;
  int64_t *n_replaced;
} pla_influence_args;
int pla_loo_influence(const pla_influence_args *args);

/*
 * GLM log-likelihood generator and PSIS-LOO without the matrix (csrc/pla_glm.h).  For a generalised linear model the
 * (n_obs, n_draws) log-likelihood is a function of the design matrix x (n_obs x n_pred), the coefficient draws beta (n_draws x
 * n_pred) and at most one auxiliary parameter per draw; this entry writes it block by block, or consumes each block at once.  f64:
 *     eta[i, s] = sum_p x[i, p] beta[s, p] + offset_i          the sum on the f64 matrix cores, started from zero
 *     PLA_GLM_LINPRED          eta itself (PLA_GLM_MODE_MATRIX only)
 *     PLA_GLM_GAUSSIAN         draw_const_s - 0.5 ((y_i - eta) / draw_scale_s)^2      draw_const_s = -0.5 log(2 pi) - log(sigma_s)
 *     PLA_GLM_BINOMIAL_LOGIT   obs_const_i + y_i eta - trials_i softplus(eta)          softplus(e) = max(e, 0) + log1p(exp(-|e|));
 *                              obs_const_i = lgamma(n+1) - lgamma(y+1) - lgamma(n-y+1); trials NULL: 1 (Bernoulli), obs_const NULL: 0
 *     PLA_GLM_POISSON_LOG      obs_const_i + y_i eta - exp(eta)                        obs_const_i = -lgamma(y_i + 1)
 *     PLA_GLM_NEGBINOMIAL_LOG  (((obs_const_i + draw_const_s) + lgamma(y_i + phi_s)) + y_i eta) - (y_i + phi_s) L,
 *                              L = max(eta, lp_s) + log1p(exp(-|eta - lp_s|)), lp_s = log(phi_s) taken once per tile of draws;
 *                              phi_s = draw_scale_s (NB2: mean exp(eta), variance mu + mu^2 / phi), draw_const_s = phi log(phi) -
 *                              lgamma(phi), obs_const_i = -lgamma(y_i + 1)
 *     PLA_GLM_GAMMA_LOG        (draw_const_s + (alpha_s - 1) obs_const_i) - alpha_s (eta + y_i exp(-eta))
 *                              alpha_s = draw_scale_s (the shape; mean exp(eta)), draw_const_s = alpha log(alpha) - lgamma(alpha),
 *                              obs_const_i = log(y_i)
 *     PLA_GLM_BINOMIAL_PROBIT  (obs_const_i + y_i logPhi(eta)) + (trials_i - y_i) logPhi(-eta); a product whose factor y_i or
 *                              trials_i - y_i is 0 is not formed (it is 0, not 0 * -inf); trials, obs_const as for
 *                              PLA_GLM_BINOMIAL_LOGIT.  With h = 0.5 erfcx(|x| / sqrt 2), w = 0.5 fl(x^2) and r = x^2 - fl(x^2) (exact,
 *                              one fused multiply-add), logPhi(x) = log(h) - w for x < 0 and log1p(-(h exp(-w)) (1 - 0.5 r))
 *                              otherwise: finite in both tails, and the upper tail keeps its relative accuracy
 * Every sum and product is rounded once, in the order written (no contraction).  The constants are the caller's.  Values that are not finite propagate by IEEE rules; in PLA_GLM_MODE_LOO a NaN log-likelihood is
 * replaced by -1e10 and counted (the rule of pla_psis_loo's callers).  eta[i, s] and ll[i, s] depend on row i of x, row s of beta,
 * n_pred and the vectors' entries alone -- not on the grid, the block size (PLA_INGEST_BLOCK_MB), the position of the row or the
 * draw, a row list, or the layout and strides of x and beta; there are no floating-point atomics.
 *
 * The argument block carries its own size: set struct_size = sizeof(pla_glm_args); a call with another size is PLA_ERR_ARG.
 *   engine              the engine (NULL: PLA_ERR_ARG)
 *   family, mode        PLA_GLM_*; PLA_GLM_MODE_MATRIX writes the (m, n_draws) values to out (row pitch out_pitch elements, draws
 *                       fastest; n_draws >= 1), a device buffer in place, a host buffer block by block through engine memory.
 *                       PLA_GLM_MODE_LOO (not with PLA_GLM_LINPRED; n_draws >= 2): per block of rows the kernel writes into engine
 *                       memory and the pass of pla_psis_loo runs on the block; diag / loo_i / lppd_i [m] (each may be NULL), agg
 *                       [PLA_AGG_COUNT] (may be NULL) over all rows from the pointwise vectors, *n_replaced the NaN count.
 *   method, tail_count, scale_value, good_k      as pla_psis_loo (PLA_GLM_MODE_LOO)
 *   x, n_obs, n_pred, x_stride_obs, x_stride_pred            1 <= n_pred <= 256; device: any positive strides; host: dense, either
 *                       orientation
 *   beta, n_draws, beta_stride_draw, beta_stride_pred        the same
 *   y, offset, trials, obs_const     [n_obs]; y is needed by every family but PLA_GLM_LINPRED, the other three may be NULL
 *   draw_scale, draw_const           [n_draws]; PLA_GLM_GAUSSIAN, PLA_GLM_NEGBINOMIAL_LOG and PLA_GLM_GAMMA_LOG need both (NULL:
 *                       PLA_ERR_ARG, with a message of its own for each of the two under the last two families); unused otherwise
 *   row_index, n_rows   optional rows of x (m = n_rows; repeats and any order allowed), else m = n_obs; a device list is clamped
 *                       into [0, n_obs), a host list out of range is PLA_ERR_ARG
 *   mem_space, stream   where EVERY pointer of the block lives; PLA_DEVICE: everything is enqueued on stream
 */
#define PLA_GLM_LINPRED 0
#define PLA_GLM_GAUSSIAN 1
#define PLA_GLM_BINOMIAL_LOGIT 2
#define PLA_GLM_POISSON_LOG 3
#define PLA_GLM_NEGBINOMIAL_LOG 4
#define PLA_GLM_GAMMA_LOG 5
#define PLA_GLM_BINOMIAL_PROBIT 6
#define PLA_GLM_MODE_MATRIX 0
#define PLA_GLM_MODE_LOO 1
typedef struct pla_glm_args {
  int64_t struct_size;
  pla_engine *engine;
  int32_t family, mode, method, mem_space;
  void *stream;
  const double *x;
  int64_t n_obs, n_pred, x_stride_obs, x_stride_pred;
  const double *beta;
  int64_t n_draws, beta_stride_draw, beta_stride_pred;
  const double *y, *offset, *trials, *obs_const;
  const double *draw_scale, *draw_const;
  const int64_t *row_index;
  int64_t n_rows, tail_count;
  double scale_value, good_k;
  double *out;
  int64_t out_pitch;
  double *diag, *loo_i, *lppd_i, *agg;
  int64_t *n_replaced;
} pla_glm_args;
int pla_glm(const pla_glm_args *args);

/*
 * pla_glm with group-level terms -- multilevel models: varying intercepts and slopes over grouping factors (csrc/pla_glm_terms.h).
 *     eta[i, s] = ((( acc[i, s] + offset_i ) + z_0[i] u_0[s, g_0[i]] ) + z_1[i] u_1[s, g_1[i]] ) + ...
 * acc is pla_glm's sum on the matrix cores; every product and every sum is rounded once, in the order of the terms; with z_t NULL
 * (a varying intercept) the product is not formed.  Reordering the terms reorders the additions and may change the last bit.
 * Everything else -- families, modes, the NaN rule, row_index, blocks -- is pla_glm's, and so is its rule of order, extended:
 * eta[i, s] depends on row i of x, row s of beta, the entries i of the vectors and of g_t and z_t, and on u_t[s, g_t[i]], in the
 * order of the terms; not on the grid, the block size, positions, a row list, strides, the labels of the groups or the memory
 * space.  n_terms = 0 gives the bits of pla_glm.
 *
 * Set struct_size = sizeof(pla_glm_grouped_args) and glm.struct_size = sizeof(pla_glm_args); another size is PLA_ERR_ARG.
 *   glm                 the argument block of pla_glm, every field as there
 *   n_terms             0 .. PLA_GLM_MAX_TERMS
 *   terms[t]            group_index [n_obs] int32 in [0, n_groups): a device index is clamped into the range on load, a host index
 *                       out of range is PLA_ERR_ARG; z [n_obs] or NULL (1); u (n_draws x n_groups) with strides u_stride_draw /
 *                       u_stride_group in elements (device: any positive strides; host: dense, either orientation);
 *                       1 <= n_groups < 2^31.  All of them live where glm.mem_space says.
 * Engine memory: the image of the group effects, sum_t n_groups_t x n_draws (padded to 16) doubles.
 */
#define PLA_GLM_MAX_TERMS 8
typedef struct pla_glm_term {
  const int32_t *group_index;
  const double *z;
  const double *u;
  int64_t u_stride_draw, u_stride_group, n_groups;
} pla_glm_term;
typedef struct pla_glm_grouped_args {
  int64_t struct_size;
  pla_glm_args glm;
  int64_t n_terms;
  pla_glm_term terms[PLA_GLM_MAX_TERMS];
} pla_glm_grouped_args;
int pla_glm_grouped(const pla_glm_grouped_args *args);

/*
 * Cluster-marginal log-likelihood of a multilevel GLM, and PSIS-LOO over it: leave-one-cluster-out with the left-out cluster's own
 * effect integrated out of the likelihood (csrc/pla_glm_marginal.h; Merkle, Furr & Rabe-Hesketh 2019).  Every observation belongs
 * to one cluster c in [0, n_clusters); its linear predictor is eta[i, s] = rest[i, s] + z_i u with rest what pla_glm_grouped
 * computes (x beta + offset and the conditional terms) and u | draw s ~ N(0, tau_s^2).  By quadrature on nodes of the cluster:
 *     e[q]      = ( log_weights[c, q] + ( (-0.5 log 2 pi - log tau_s) - 0.5 (nodes[c, q] / tau_s)^2 ) )
 *                 + sum_{i in c, in member order} ll(y_i | rest[i, s] + z_i nodes[c, q])
 *     mll[c, s] = max_q e[q] + log sum_q exp(e[q] - max_q e[q])                 (-inf if every e[q] is -inf)
 * ll is the density of pla_glm.  The product z_i node and every sum are rounded once; with z NULL the product is not formed.
 * THE SUMMATION RULE.  With L = pla_glm_marginal_segment(), segment k of a cluster is its members [k L, (k + 1) L); a segment sum
 * starts from zero and runs in member order; the segment sums are added in order of k, starting from the sum of segment 0.
 * mll[c, s] depends on the rest values of the cluster's members in member order, on their entries of the vectors, on row c of nodes
 * and log_weights, on tau_s and on L -- not on the grid, the block size (PLA_INGEST_BLOCK_MB), the place of the cluster in the list,
 * its label, the position of the draw or the memory space.  There are no floating-point atomics.
 *
 * Set struct_size = sizeof(pla_glm_marginal_args), grouped.struct_size and grouped.glm.struct_size as pla_glm_grouped wants them.
 *   grouped             the argument block of pla_glm_grouped: family (PLA_GLM_GAUSSIAN, PLA_GLM_BINOMIAL_LOGIT or
 *                       PLA_GLM_POISSON_LOG; any other: PLA_ERR_ARG), mode, x, beta, the vectors, the terms;
 *                       grouped.glm.row_index must be NULL.  Its output fields describe one row per CLUSTER: PLA_GLM_MODE_MATRIX
 *                       writes the (n_clusters, n_draws) matrix mll to out; PLA_GLM_MODE_LOO runs the pass of pla_psis_loo on
 *                       blocks of finished clusters, diag / loo_i / lppd_i are [n_clusters]; a NaN mll is replaced by -1e10 and
 *                       counted in *n_replaced.
 *   n_clusters, cluster_offsets [n_clusters + 1], members [n_members], n_members
 *                       cluster c holds the observations members[cluster_offsets[c] .. cluster_offsets[c + 1]) -- the image of a
 *                       grouping in compressed rows, the rows sorted by cluster.  Host lists are checked (offsets start at 0, do
 *                       not decrease and end at n_members; members lie in [0, n_obs): else PLA_ERR_ARG).  A device pair of offsets
 *                       that decreases or leaves [0, n_members] is an empty cluster, a device member is clamped into [0, n_obs).
 *                       An empty cluster is legal: its mll is the log-sum-exp of prior plus log-weight alone.
 *   z                   [n_obs] or NULL (1): the covariate of the integrated effect
 *   tau                 [n_draws], positive and finite (checked on the host)
 *   n_nodes, nodes, log_weights      1 <= n_nodes <= 32; [n_clusters][n_nodes] each
 * A PLA_DEVICE call waits once, at its start, for the n_clusters + 1 offsets to reach the host -- the member list is cut into blocks
 * where clusters and segments end -- and for its tables to reach the device; inside a stream capture it is PLA_ERR_UNSUPPORTED.
 * Engine memory: one block of the linear predictor, one block of finished clusters (unless the matrix goes into a device buffer in
 * place), 24 bytes per segment, and n_nodes (padded to 8, 16 or 32) x n_draws doubles per segment of the clusters of a block that
 * are longer than L.
 */
typedef struct pla_glm_marginal_args {
  int64_t struct_size;
  pla_glm_grouped_args grouped;
  int64_t n_clusters, n_members;
  const int64_t *cluster_offsets, *members;
  const double *z, *tau;
  int64_t n_nodes;
  const double *nodes, *log_weights;
} pla_glm_marginal_args;
int pla_glm_marginal(const pla_glm_marginal_args *args);
int pla_glm_marginal_segment(void); /* L of the summation rule */

/*
 * Leave-one-out predictive moments and LOO-PIT of a GLM without predictive draws and without the matrix (csrc/pla_glm_predict.h).
 * Given eta[i, s] (pla_glm's, bit for bit) and the per-draw value, the conditional mean mu, variance v and distribution function F
 * of y_i are closed forms, so with lw row i of the log weights, m = max_s lw_s and e_s = exp(lw_s - m) (a weight of log -inf is 0
 * and its draw contributes to nothing):
 *     mean[i]   = sum_s e_s mu_is / sum e                  E_loo[y_i]
 *     m2[i]     = sum_s e_s (v_is + mu_is^2) / sum e       the raw second moment (variance = max(m2 - mean^2, 0))
 *     pit_le[i] = sum_s e_s P(Y <= y_i | draw s) / sum e   pit_lt[i] = sum_s e_s P(Y < y_i | draw s) / sum e
 *     family                   mu        v                    F
 *     PLA_GLM_GAUSSIAN         eta       sigma^2              Phi((y - eta) / sigma) from erfcx, pit_lt == pit_le bit for bit
 *     PLA_GLM_BINOMIAL_LOGIT   n p       n p (1 - p)          p = logistic(eta)        } the downward product recurrence from
 *     PLA_GLM_BINOMIAL_PROBIT  n p       n p (1 - p)          p = Phi(eta)             } pmf(y) = exp(ll): F_lt = pmf(y) T,
 *     PLA_GLM_POISSON_LOG      exp(eta)  mu                                            } F_le = min(F_lt + pmf(y), 1),
 *     PLA_GLM_NEGBINOMIAL_LOG  exp(eta)  mu + mu^2 / phi                               } T = sum_j prod_{k > y - j} pmf(k-1)/pmf(k)
 *     PLA_GLM_GAMMA_LOG        exp(eta)  mu^2 / alpha         none: a non-NULL pit_le or pit_lt is PLA_ERR_UNSUPPORTED
 * (F_le = 1 exactly for a binomial count y = n.)  The rounding order of every formula is stated in csrc/pla_glm_predict.h.  A count y outside [0, 4096] is not walked: the row's
 * two PIT values are NaN and the row is counted in *n_pit_skipped; its moments are computed.  A row whose weights are all -inf
 * gives NaN.
 * THE SUMMATION RULE.  With L = pla_glm_predict_segment(), segment k holds the draws [16 L k, 16 L (k + 1)); inside a segment
 * column c = s mod 16 adds its draws in ascending order from zero, the 16 columns combine by the butterfly c ^ 1, c ^ 2, c ^ 4,
 * c ^ 8, and the segment sums are added in order of k from segment 0's.  No floating-point atomics: a row's outputs depend on its
 * row of x, its entries of the vectors, its row of weights and n_draws alone -- not on the grid, the block size
 * (PLA_INGEST_BLOCK_MB), the memory space, the position of the row or the row list.
 *
 * Set struct_size = sizeof(pla_glm_predict_args) and glm.struct_size = sizeof(pla_glm_args); another size is PLA_ERR_ARG.
 *   glm                 the argument block of pla_glm: engine, family (PLA_GLM_LINPRED: PLA_ERR_ARG), x, beta, the vectors, row_index
 *                       / n_rows, mem_space and stream as there (n_draws >= 2); method and tail_count as pla_importance_weights takes
 *                       them (PLA_PIT_LOGLIK).  mode, scale_value, good_k and the block's own outputs are not read.
 *   kind                PLA_PIT_LOGLIK: per block of rows the generator writes the log-likelihood into engine memory, the pipeline of
 *                       pla_loo_diag runs on it (-ll with NaN -> -1e10 counted in *n_replaced, the weights pass, Pareto k or the ESS
 *                       into diag, elpd_i) and the predictive kernel consumes the block's weights before the next block.
 *                       PLA_PIT_LOG_WEIGHTS: log_weights is (m, n_draws), m the rows of the call, of any normalisation, row stride
 *                       lw_stride_obs and unit draw stride (another lw_stride_draw: PLA_ERR_UNSUPPORTED); the predictive kernel
 *                       alone, device weights read in place, host weights staged in blocks; diag and elpd_i are not written,
 *                       *n_replaced is 0.
 *   mean, m2, pit_le, pit_lt, diag, elpd_i      [m], each may be NULL;  n_replaced, n_pit_skipped: one int64 each, may be NULL
 * PLA_DEVICE: everything is enqueued on glm.stream and nothing is allocated once the workspace fits.  PLA_HOST: the call returns
 * when the results are there.  Engine memory beyond pla_glm's: 8 (1 + 5 ceil(n_draws / (16 L))) bytes per row of a block.
 */
typedef struct pla_glm_predict_args {
  int64_t struct_size;
  pla_glm_args glm;
  int64_t kind;
  const double *log_weights;
  int64_t lw_stride_obs, lw_stride_draw;
  double *mean, *m2, *pit_le, *pit_lt, *diag, *elpd_i;
  int64_t *n_replaced, *n_pit_skipped;
} pla_glm_predict_args;
int pla_glm_predict(const pla_glm_predict_args *args);
int pla_glm_predict_segment(void); /* L of the summation rule */

/*
 * PSIS leave-future-out cross-validation (Buerkner, Gabry & Vehtari 2020; forward mode, `horizon` steps ahead; csrc/pla_lfo.h).
 * The observations (rows of ll) are in time order and ll is the log-likelihood of ALL n_obs of them under the draws of one fit to
 * the first `first`.  Step j = 0 .. n_steps - 1 conditions on rows [0, first + j) and predicts rows [first + j, first + j + horizon):
 *     lr_j[s] = sum_{r = first}^{first + j - 1} ll[r, s]            f_j[s] = ll[first + j, s] + ... + ll[first + j + horizon - 1, s]
 *     j = 0:  elpd_i[0] = logsumexp_s(f_0) - log n_draws, diag[0] = 0  (the fit's own step: exact, no importance sampling)
 *     j > 0:  (lw_j, diag[j]) = PSIS(lr_j) with tail_count, as pla_importance_weights;
 *             elpd_i[j] = logsumexp_s(lw_j + f_j) - logsumexp_s(lw_j)
 * All arithmetic is f64 (f32 input is widened on load); NaN entries of ll count as -1e10 and are counted in *n_replaced (pla_lfo:
 * every entry of rows [first, first + n_steps + horizon - 1) once; pla_lfo_ratios: of rows [first, first + n_steps - 1)); +-inf are
 * kept.  A weight of log -inf is 0; a step whose weights are all NaN gives NaN, and so does a step for which lw_j + f_j is -inf at
 * every draw (an observation of likelihood 0 under every draw: logsumexp of nothing), whatever n_draws -- never -inf.
 *
 * THE SUMMATION RULE of lr.  With the chunk length C = 64, per draw, every sum taken in the order written:
 *     total[c] = ll[first + cC] + ll[first + cC + 1] + ... + ll[first + cC + C - 1]        carry[0] = 0, carry[c + 1] = carry[c] + total[c]
 *     local[j] = 0 when j is a multiple of C, else ll[first + cC] + ... + ll[first + j - 1] with c = j / C       lr_j = carry[j / C] + local[j]
 * It depends on j and C alone: the results have the same bits whatever the grid, the block size (PLA_INGEST_BLOCK_MB: the call works
 * one block of whole chunks at a time -- ratios into the ingest staging, the weights pass into a second bounded buffer, the predict
 * kernel before the next block overwrites either), the layout and the memory space.  No floating-point atomics.
 *
 * pla_lfo_ratios  out (n_steps, n_draws) C-contiguous, ALWAYS f64: out[j, s] = lr_j[s] (row 0 is all zeros).
 *                 1 <= n_steps <= n_obs - first + 1.
 * pla_lfo         diag, elpd_i [n_steps] (each may be NULL).  *first_high (may be NULL) = the smallest j >= 1 with
 *                 diag[j] > k_threshold, or n_steps when there is none (a NaN k is not above).  Needs first >= 0, horizon >= 1,
 *                 1 <= n_steps <= n_obs - first - horizon + 1, n_draws >= 2 and a tail_count pla_importance_weights accepts
 *                 (PLA_ERR_ARG otherwise); method PLA_PSIS only (PLA_SIS / PLA_TIS: PLA_ERR_UNSUPPORTED).
 * Layouts, in either memory space: draws fastest (stride_draw == 1, any stride_obs >= n_draws: read in place on the device), or
 * observations fastest (stride_obs == 1, stride_draw >= n_obs: transposed block by block, with the horizon - 1 extra rows the last
 * step of a block needs); other strides return PLA_ERR_UNSUPPORTED.  PLA_DEVICE: everything is enqueued on `stream`, the outputs,
 * first_high and n_replaced (one int64 each) are device pointers, and nothing is allocated once the workspace fits
 * (pla_engine_set_frozen).  PLA_HOST: the matrix is staged in 1 GiB blocks and the call returns when the results are there.
 *
 * BACKWARD MODE of pla_lfo (the algorithm as the paper states it; csrc/pla_lfo_bw.h): method = PLA_PSIS | PLA_LFO_BACKWARD.  The low
 * byte of `method` stays the IS method (PLA_SIS / PLA_TIS with the flag: PLA_ERR_UNSUPPORTED).  `first` then carries `last`, the
 * number of observations the fit SAW (1 .. n_obs; a walk begins with the fit to all of them, last = n_obs), and ll holds all n_obs
 * rows under its draws -- rows r >= last are the conditional terms log p(y_r | y_<r, theta_s), which the caller supplies.  The
 * steps go DOWN from t_0 = min(last, n_obs - horizon):  t_j = t_0 - j, j = 0 .. n_steps - 1, 1 <= n_steps <= t_0 + 1, and
 *     f_j[s]  = ll[t_j, s] + ... + ll[t_j + horizon - 1, s]  (in that order)      lr_j[s] = - sum_{r = t_j}^{last - 1} ll[r, s]
 *     t_j = last:  elpd_i[j] = logsumexp_s(f_j) - log n_draws, diag[j] = 0        (exact; only j = 0 can be, when last <= n_obs - horizon)
 *     t_j < last:  (lw_j, diag[j]) = PSIS(lr_j), elpd_i[j] = logsumexp_s(lw_j + f_j) - logsumexp_s(lw_j)
 * *first_high = the smallest j >= j_min with diag[j] > k_threshold, else n_steps; j_min = 1 when step 0 is exact, else 0 (with
 * last = n_obs step 0 has already removed `horizon` rows and may itself be above the threshold).  NaN entries are counted once each
 * over rows [t_{n_steps - 1}, t_0 + horizon).  The summation rule is the one above ANCHORED AT THE FIT: with a_q = ll[last - 1 - q]
 * (the same rows, walked downward), P[q] built from a as lr is built from ll[first + .] above (P[0] = 0, P[q] = carry[q / C] +
 * local[q]), lr_j = -P[last - t_j]; it depends on last - t_j and C alone.  Bad geometry returns PLA_ERR_ARG with a text in
 * pla_last_error.  Layouts, memory spaces, the block pipeline and the frozen-engine rule are those of forward mode; the horizon - 1
 * extra rows of a staged block lie above its highest row.  pla_lfo_ratios has no backward mode.
 */
#define PLA_LFO_BACKWARD 0x100
int pla_lfo_ratios(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                   int64_t first, int64_t n_steps, int mem_space, void *stream, double *out, int64_t *n_replaced /* may be NULL */);
int pla_lfo(pla_engine *eng, const void *ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
            int64_t first, int64_t n_steps, int64_t horizon, int method, int64_t tail_count, double k_threshold, int mem_space,
            void *stream, double *diag /* may be NULL */, double *elpd_i /* may be NULL */, int64_t *first_high /* may be NULL */,
            int64_t *n_replaced /* may be NULL */);

/*
 * Relative MCMC efficiency of every row of a matrix (csrc/pla_ess.h): r_eff[i] = ESS / n_draws' of the mean of row i, Stan's
 * estimator for the mean (Vehtari et al. 2021; Geyer's initial positive and monotone sequences) without rank normalisation --
 * relative_eff() of R-loo, the `reff` every PSIS entry point here takes (pass its mean).  The reference has no counterpart: its
 * loo.py:204-216 asks ArviZ for the ESS of the posterior.
 *   x        (n_obs, n_draws), PLA_F64 / PLA_F32, const.  A row is n_chains chains of n_draws / n_chains draws, chain major.
 *   flags    PLA_ESS_LOG    the rows are log-likelihoods: exp(x - row maximum) is analysed (the estimate is scale-invariant); else x.
 *            PLA_ESS_SPLIT  every chain of n0 draws becomes two, its first and its last n0 / 2 draws (the middle one of an odd chain
 *                           is dropped): ArviZ / posterior.  Without it: R-loo.
 *            PLA_ESS_CAP    results above 1 (antithetic chains) are returned as 1, as R-loo does.
 * With C chains of n draws after the split, d[c][i] the draws minus their chain mean m_c, all in f64:
 *     A(t) = sum_c sum_{i < n - t} d[c][i] d[c][i + t] / (C n)     W = A(0) n / (n - 1)     V = A(0) + var(m_c, ddof 1) (0 for C = 1)
 *     rho(t) = 1 - (W - A(t)) / V;  pairs (rho(t), rho(t + 1)), t = 2, 4, ..., are taken while t < n - 1 and the previous pair's sum is
 *     positive; a pair with a negative sum counts as zero; a pair above its predecessor counts as its predecessor;
 *     tau = -1 + 2 sum of the pairs (the first is 1 + rho(1)) + max(last rho(even), 0), at least 1 / log10(C n);  r_eff = 1 / tau.
 * The order of every sum is fixed (csrc/pla_ess.h), so the bits do not depend on the grid, the layout or the memory space.
 * Invalid rows -- a NaN or +inf entry (-inf too without PLA_ESS_LOG), a constant row (every entry -inf included), a variance that is
 * not positive and finite -- give NaN and are counted in *n_invalid (may be NULL).  Single -inf entries of a log row are likelihood 0.
 * Needs n_chains >= 1 dividing n_draws and at least 4 draws per chain after the split (PLA_ERR_ARG otherwise).  Rows of up to
 * pla_ess_lds_max_draws() analysed draws are read once and kept on chip; longer ones go through engine workspace.
 * Layouts, in either memory space: draws fastest (stride_draw == 1, any stride_obs >= n_draws: read in place on the device), or
 * observations fastest (stride_obs == 1, stride_draw >= n_obs: transposed block by block into staging); other strides return
 * PLA_ERR_UNSUPPORTED.  PLA_DEVICE: everything is enqueued on `stream`, r_eff [n_obs] and n_invalid (one int64) are device pointers
 * and nothing is allocated once the workspace fits.  PLA_HOST: the matrix is staged in 1 GiB blocks.
 * pla_engine_set_ess_grid caps the workgroups of the pass (0: the library's choice) -- a test hook: the results do not depend on it.
 */
#define PLA_ESS_LOG 1
#define PLA_ESS_SPLIT 2
#define PLA_ESS_CAP 4
int pla_relative_eff(pla_engine *eng, const void *x, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                     int64_t n_chains, int flags, int mem_space, void *stream, double *r_eff, int64_t *n_invalid /* may be NULL */);
int pla_engine_set_ess_grid(pla_engine *eng, int max_workgroups);
int pla_ess_lds_max_draws(void);

/* Timing of the dominant kernel, measured with hipEvents on the launch stream.
 * enable != 0 brackets every main-kernel launch with events; pla_engine_kernel_ms returns the
 * accumulated milliseconds and launch count since the last call (it synchronises the events). */
int pla_engine_set_timing(pla_engine *eng, int enable);
int pla_engine_kernel_ms(pla_engine *eng, double *total_ms, int64_t *launches);
/* Same, for the first (dominant) kernel alone of the passes that ran as two kernels (the split PSIS-LOO pass: the
 * wave kernel up to the tail selection); device-pointer calls only.  Read it before or after pla_engine_kernel_ms. */
int pla_engine_first_kernel_ms(pla_engine *eng, double *total_ms, int64_t *launches);

/* Which kernels the engine's last PSIS-LOO / weights / group / e_loo call launched, as text ("wave_loo_kernel<double> (streamed) +
 * fit_rows_stream_kernel beside it + ..."): for benchmark records, so that what a roofline line names is what ran.
 * Copies at most cap - 1 characters and a terminating 0 into buf. */
int pla_engine_last_kernels(pla_engine *eng, char *buf, int cap);

/* Run-time switches of the library that are SET in this process's environment, as "NAME=value NAME=value" ("" when none is):
 * for benchmark records.  The shipped library reads PLA_PIPE, PLA_STREAM_PATIENCE_US, PLA_FORCE_PATH, PLA_INGEST_TRANSPOSE and
 * PLA_INGEST_BLOCK_MB -- path selectors, every setting of which computes the same results (csrc/pla_launch.h); builds with
 * -DPLA_EXPERIMENT read more (ablation, grids, priorities), and the text then starts with "EXPERIMENT-BUILD".
 * Copies at most cap - 1 characters and a terminating 0 into buf. */
int pla_env_overrides(char *buf, int cap);

/* Streamed PSIS-LOO passes (the fit kernel running beside the sweep): *gave_up = how many passes since the last call the fit
 * kernel stopped waiting for the sweep (the two were not run side by side: a serialising profiler, a co-tenant holding the
 * CUs) and left the rest to the plain fit kernel behind it -- correct, but the pass then costs up to 20 ms more, which a
 * benchmark record should show.  Synchronises the device. */
int pla_engine_stream_stats(pla_engine *eng, int64_t *gave_up);

/*
 * Observation-sharded runs (loo.py:326-342 across devices): every device reduces its own block of
 * observations to one aggregate vector; the vectors are exchanged with ONE all-reduce (sum) of a world x PLA_AGG_COUNT
 * table in which every rank has filled its own row -- the host's collective library does that (torch.distributed / RCCL
 * in pyloo_amd.sharded; any all-reduce of doubles will do) -- and merged with the pairwise update of Chan, Golub & LeVeque.
 * Device pointers, the caller's stream, one small kernel each:
 *   pla_aggregate_pack   table[world][PLA_AGG_COUNT] = 0 except row `rank` = agg   (before the all-reduce)
 *   pla_aggregate_merge  out[PLA_AGG_COUNT] = the merged aggregates of the table   (after it; identical on every rank)
 */
int pla_aggregate_pack(pla_engine *eng, const double *agg, int rank, int world, double *table, void *stream);
int pla_aggregate_merge(pla_engine *eng, const double *table, int world, double *out, void *stream);

/* Synthetic benchmark input, generated on the device:
 *   u = splitmix64(seed ^ (i*S + s)) -> 53-bit uniform in (0,1) -> E = -log1p(-u)
 *   ll[i,s] = -k_i*E + c_i,  c_i = -1 - (i mod 7)/4,  k_i = k_lo + (k_hi-k_lo)*U(splitmix64(~seed ^ i))
 *   rows with (i mod 10) in {0,3,6} draw k_i from [heavy_lo, heavy_hi) when heavy_hi > heavy_lo.
 * row0 offsets the observation index so shards of one matrix can be generated per rank. */
int pla_fill_synthetic(pla_engine *eng, void *ll_device, int dtype, int64_t n_obs, int64_t n_draws,
                       int64_t row0, uint64_t seed, double k_lo, double k_hi, double heavy_lo,
                       double heavy_hi, void *stream);

/* The same marginals as MCMC delivers them (bench.py --rows chain_ar1): `chains` chains stacked chain-major along the draws
 * (the (chain, draw) -> __sample__ stack of loo.py:189), every chain a stationary AR(1) sequence in the draw index with
 * coefficient rho (Gaussian copula, Exp(1) marginals), k_i ~ U(k_lo, k_hi) and c_i as above, plus an offset ~ N(0, offset_sd^2)
 * of each chain's log-likelihoods. */
int pla_fill_synthetic_chains(pla_engine *eng, void *ll_device, int dtype, int64_t n_obs, int64_t n_draws,
                              int64_t row0, uint64_t seed, int chains, double rho, double offset_sd,
                              double k_lo, double k_hi, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PYLOO_AMD_H */
