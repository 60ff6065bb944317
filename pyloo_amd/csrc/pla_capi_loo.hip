// C ABI of libpyloo_amd.so, PSIS-LOO family: the LOO pass and its routing, importance weights, WAIC, e_loo, synthetic fills.
// Host code only: argument checks, host<->device staging for PLA_HOST callers, kernel launches on the caller's stream.
#include "pla_capi.h"

namespace pla::capi {

// The weights pass of one block of rows for the passes that consume a block's weights before the next block overwrites them
// (pla_loo_pit, pla_loo_diag), as pla_importance_weights sets it up: every field of `p` but in / n_obs / diag / lw_out, and the
// workspace for `*rows` rows per block -- the slow list, the quantile table, the weights buffer d_lw and, for long rows, the
// hand-over buffers of the split weights route, whose inner blocks of 2^17 rows cap *rows.
int weights_block_setup(pla_engine* eng, int method, int64_t tail_count, int64_t n_draws, size_t esz, hipStream_t s, int64_t* rows,
                        pla::RowsParams* p) {
  p->n_draws = (int)n_draws;
  p->method = method;
  p->tail_count = method == PLA_PSIS ? (int)tail_count : 0;
  p->tail_cap = pow2_at_least(p->tail_count);
  p->scale_value = 1.0;
  p->counters = eng->counters;
  p->stride_obs = n_draws;
  p->stride_draw = 1;
  const bool split = lw_split_route(method, n_draws, tail_count, rows);
  PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));
  int rc = eng->d_slow.reserve((size_t)*rows * sizeof(unsigned));
  if (rc) return rc;
  p->slow_list = eng->d_slow.as<unsigned>();
  if (method == PLA_PSIS) {
    rc = ensure_l1_table(eng, tail_count, s, &p->l1_table);
    if (rc) return rc;
  }
  if (split) {
    rc = lw_split_workspace(eng, tail_count, *rows, p);
    if (rc) return rc;
  }
  return eng->d_lw.reserve((size_t)*rows * (size_t)n_draws * esz);
}

// the pass itself, for a caller that has checked the arguments and holds the engine (EngineCall)
int psis_loo_run(pla_engine* eng, const void* ll, int dtype, int64_t n_src, const int64_t* row_index, int64_t n_obs,
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
    rc = eng->d_slow.reserve((size_t)n_obs * sizeof(unsigned));
    if (rc) return rc;
    p.slow_list = eng->d_slow.as<unsigned>();
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
          rc = eng->d_sync.reserve(pla::stream_sync_bytes(rows));
          if (rc) return rc;
        }
        const int sstride = (pipeline || tile_stream) ? 16 : 8;  // (streamed: one whole 128-byte line of scalars per observation)
        rc = eng->d_ws.reserve((size_t)rows * (size_t)(stride + sstride) * sizeof(double));
        if (rc == PLA_ERR_NOMEM && !use_col) {
          rc = 0;  // no room for the hand-over: the fused kernels need none (the split pass is the faster, not the only, path)
        } else {
          if (rc) return rc;
          p.ws_y = eng->d_ws.as<double>();
          p.ws_s = eng->d_ws.as<double>() + (size_t)rows * stride;
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
      rc = eng->d_pw.reserve((size_t)(3 * n_obs + PLA_AGG_COUNT) * sizeof(double));
      if (rc) return rc;
      if (!dd) dd = eng->d_pw.as<double>();
      if (!dl) dl = eng->d_pw.as<double>() + n_obs;
      if (!dp) dp = eng->d_pw.as<double>() + 2 * n_obs;
    }
    const auto reduce = [&]() -> int {  // the aggregates behind the pass, when asked for: how every device route ends
      if (!agg) return PLA_OK;
      pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, agg, eng->counters + 1};
      PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
      return PLA_OK;
    };
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
          pla::PipeStreams ps{eng->pipe_first, eng->pipe_second, eng->pipe_fork, eng->pipe_join1, eng->pipe_join2, eng->d_sync.as<unsigned>(),
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
      return reduce();
    }
    if (use_col && p.ws_y) {
      // observations-fastest input, read in place: one lane per observation (pla_col.h), block by block of observations
      rc = eng->d_col.reserve(pla::col_workspace_bytes(n_obs < kColBlock ? n_obs : kColBlock));
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
        PLA_HIP(pla::launch_col(p, dtype, col_kq, eng->d_col.p, s));
        eng->last_kernels = "col_sweep_kernel (one lane per observation, matrix read in place) + col_select_kernel + fit_rows_kernel + slow_rows_kernel";
      }
      return reduce();
    }
    if (ingest) {
      // observations-fastest input: transpose a block of rows into the staging buffer, run the pass on it, next block
      // (all on the caller's stream: the buffer is reused in stream order, nothing synchronises)
      const int64_t rows_per_chunk = staged_chunk_rows(mem_space, true, n_obs, n_draws, esz);
      rc = eng->d_in.reserve((size_t)rows_per_chunk * (size_t)n_draws * esz);
      if (rc) return rc;
      p.in = eng->d_in.p;
      p.stride_obs = n_draws;
      p.stride_draw = 1;
      for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
        const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
        TimedLaunch t(eng, s);
        PLA_HIP(pla::launch_transpose_rows(ll, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in.p, s));
        p.n_obs = nr;
        p.diag = dd ? dd + r0 : nullptr;
        p.loo_i = dl ? dl + r0 : nullptr;
        p.lppd_i = dp ? dp + r0 : nullptr;
        PLA_HIP(pla::launch_rows(p, dtype, false, s));
        eng->last_kernels = pla::last_rows_kernels();
      }
      return reduce();
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
        pla::PipeStreams ps{eng->pipe_first, eng->pipe_second, eng->pipe_fork, eng->pipe_join1, eng->pipe_join2, eng->d_sync.as<unsigned>(),
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
    return reduce();
  }

  // ---- PLA_HOST: stage row blocks through the device --------------------------------------
  HostOutputs out(eng, s);
  rc = out.reserve(3, n_obs);
  if (rc) return rc;
  double *dd = out.col(0), *dl = out.col(1), *dp = out.col(2), *dagg = out.col(3);
  const int64_t rows_per_chunk = staged_chunk_rows(mem_space, false, n_obs, n_draws, esz);
  if (n_obs > 0) {
    rc = eng->d_in.reserve((size_t)rows_per_chunk * (size_t)n_draws * esz);
    if (rc) return rc;
  }
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    // pack to (nr, S) contiguous on the device
    if (stride_draw == 1 || (stride_obs == 1 && stride_draw >= n_src && !row_index)) {
      rc = stage_rows(eng, ll, row_index, r0, nr, stride_obs, stride_draw, dtype, n_draws, rows_per_chunk, s);
      if (rc) return rc;
      p.stride_obs = n_draws;
      p.stride_draw = 1;
    } else {
      return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs unit stride along the draws, or along the observations without "
                                       "a row selection");
    }
    p.in = eng->d_in.p;
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
  rc = out.copy_back({diag, loo_i, lppd_i});
  if (rc) return rc;
  if (agg) {
    pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, dagg, eng->counters + 1};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
    PLA_HIP(hipMemcpyAsync(agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  PLA_HIP(hipStreamSynchronize(s));
  return PLA_OK;
}

}  // namespace pla::capi

using namespace pla::capi;

extern "C" {

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

int pla_importance_weights(pla_engine* eng, const void* logw, int dtype, int64_t n_obs, int64_t n_draws,
                           int64_t stride_obs, int64_t stride_draw, int method, int64_t tail_count,
                           int mem_space, void* stream, void* lw_out, double* diag) {
  int rc = check_common(eng, logw, dtype, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, mem_space);
  if (rc) return rc;
  if (n_obs > 0 && !lw_out) return fail(PLA_ERR_ARG, "lw_out is NULL");
  PLA_ENGINE_CALL(eng, stream);
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
    rc = eng->d_slow.reserve((size_t)n_obs * sizeof(unsigned));
    if (rc) return rc;
    p.slow_list = eng->d_slow.as<unsigned>();
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
      rc = eng->d_in.reserve((size_t)rows_per_chunk * (size_t)n_draws * esz);
      if (rc) return rc;
      p.in = eng->d_in.p;
      p.stride_obs = n_draws;
      p.stride_draw = 1;
      TimedLaunch t(eng, s);
      for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
        const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
        PLA_HIP(pla::launch_transpose_rows(logw, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in.p, s));
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
    // long rows: the split weights pass in blocks of observations (lw_split_route).  No room for its buffers: the fused weights
    // kernel, which needs none, on all rows at once.
    int64_t block = n_obs;
    if (stride_draw == 1 && n_obs > 0 && lw_split_route(method, n_draws, tail_count, &block)) {
      rc = lw_split_workspace(eng, tail_count, block, &p);
      if (rc) return rc;
      if (!p.lw_split) block = n_obs;
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
  int64_t rows_per_chunk = staged_chunk_rows(mem_space, false, n_obs, n_draws, esz);
  if (n_obs == 0) return PLA_OK;
  rc = eng->d_in.reserve((size_t)rows_per_chunk * row_bytes);
  if (rc) return rc;
  rc = eng->d_lw.reserve((size_t)rows_per_chunk * row_bytes);
  if (rc) return rc;
  // (the split weights pass of long rows, as on the device path; a 1 GiB block of such rows is below the route's cap)
  if (lw_split_route(method, n_draws, tail_count, &rows_per_chunk)) {
    rc = lw_split_workspace(eng, tail_count, rows_per_chunk, &p);
    if (rc) return rc;
  }
  HostOutputs out(eng, s);
  rc = out.reserve(3, n_obs);
  if (rc) return rc;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    rc = upload_rows(logw, nullptr, r0, nr, stride_obs, n_draws, esz, eng->d_in.p, s);
    if (rc) return rc;
    p.in = eng->d_in.p;
    p.stride_obs = n_draws;
    p.stride_draw = 1;
    p.n_obs = nr;
    p.diag = out.col(0) + r0;
    p.lw_out = eng->d_lw.p;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_rows(p, dtype, true, s));
      eng->last_kernels = pla::last_rows_kernels();
    }
    PLA_HIP(hipMemcpyAsync((char*)lw_out + (size_t)r0 * row_bytes, eng->d_lw.p, (size_t)nr * row_bytes,
                           hipMemcpyDeviceToHost, s));
    PLA_HIP(hipStreamSynchronize(s));
  }
  return out.finish({diag});
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
  PLA_ENGINE_CALL(eng, stream);
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));  // [1]: replaced entries
  eng->last_kernels.clear();  // (no observations: nothing is launched)

  if (mem_space == PLA_DEVICE) {
    double *dl = lppd_i, *dv = var_i, *dw = waic_i;
    if (agg && (!dv || !dw)) {  // the aggregates need var_i and waic_i: engine scratch when not asked for
      rc = eng->d_pw.reserve((size_t)(3 * n_obs + PLA_AGG_COUNT) * sizeof(double));
      if (rc) return rc;
      if (!dv) dv = eng->d_pw.as<double>();
      if (!dw) dw = eng->d_pw.as<double>() + n_obs;
    }
    static const bool force_transpose = getenv("PLA_INGEST_TRANSPOSE") && atoi(getenv("PLA_INGEST_TRANSPOSE")) != 0;
    if (obs_fastest_device(mem_space, row_index, n_src, n_draws, stride_obs, stride_draw) && !force_transpose) {
      // observations-fastest matrix, read in place: one lane per observation (pla_waic.h)
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_waic_col(ll, dtype, n_obs, (int)n_draws, stride_draw, scale_value, dl, dv, dw, eng->counters + 1, s));
      eng->last_kernels = pla::last_rows_kernels();
    } else if (obs_fastest_device(mem_space, row_index, n_src, n_draws, stride_obs, stride_draw)) {
      const int64_t rows_per_chunk = staged_chunk_rows(mem_space, true, n_obs, n_draws, esz);
      rc = eng->d_in.reserve((size_t)rows_per_chunk * (size_t)n_draws * esz);
      if (rc) return rc;
      for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
        const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
        TimedLaunch t(eng, s);
        PLA_HIP(pla::launch_transpose_rows(ll, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in.p, s));
        PLA_HIP(pla::launch_waic(eng->d_in.p, nullptr, dtype, nr, (int)n_draws, n_draws, 1, scale_value, dl ? dl + r0 : nullptr,
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
  HostOutputs out(eng, s);
  rc = out.reserve(3, n_obs);
  if (rc) return rc;
  double *dl = out.col(0), *dv = out.col(1), *dw = out.col(2), *dagg = out.col(3);
  const int64_t rows_per_chunk = staged_chunk_rows(mem_space, false, n_obs, n_draws, esz);
  if (n_obs > 0) {
    rc = eng->d_in.reserve((size_t)rows_per_chunk * (size_t)n_draws * esz);
    if (rc) return rc;
  }
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    rc = stage_rows(eng, ll, row_index, r0, nr, stride_obs, stride_draw, dtype, n_draws, rows_per_chunk, s);
    if (rc) return rc;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_waic(eng->d_in.p, nullptr, dtype, nr, (int)n_draws, n_draws, 1, scale_value, dl + r0, dv + r0, dw + r0,
                               eng->counters + 1, s));
      eng->last_kernels = std::string(pla::last_rows_kernels()) + " (blocks of observations uploaded)";
    }
    PLA_HIP(hipStreamSynchronize(s));  // the staging buffer is reused by the next chunk
  }
  rc = out.copy_back({lppd_i, var_i, waic_i});
  if (rc) return rc;
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
  if (int rc0 = check_engine_types(eng, dtype, mem_space)) return rc0;
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (n_obs > 0 && (!x || !log_weights)) return fail(PLA_ERR_ARG, "x / log_weights is NULL");
  if (int rc0 = check_n_draws(n_draws, 1)) return rc0;
  if (stride_draw <= 0 || stride_obs < 0) return fail(PLA_ERR_ARG, "bad strides");
  if (tail_len < 5) return fail(PLA_ERR_ARG, "tail_len must be at least 5");  // e_loo.py:298-299
  if (n_obs == 0) return PLA_OK;
  PLA_ENGINE_CALL(eng, stream);
  // (row list of the one-pass wave kernel: the rows it leaves to the general one)
  if (int rc0 = eng->d_slow.reserve((size_t)n_obs * sizeof(unsigned))) return rc0;
  if (mem_space == PLA_DEVICE) {
    PLA_HIP(pla::launch_e_loo(x, log_weights, log_ratios, dtype, n_obs, (int)n_draws, stride_obs, stride_draw, (int)tail_len, mean,
                              variance, k_mean, k_var, k_ratio, eng->d_slow.as<unsigned>(), eng->counters, s));
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
  int rc = eng->d_in.reserve((size_t)rows_per_chunk * row_bytes);
  if (!rc) rc = eng->d_lw.reserve((size_t)rows_per_chunk * row_bytes);
  if (!rc && log_ratios) rc = eng->d_slab.reserve((size_t)rows_per_chunk * row_bytes);
  if (!rc) rc = eng->d_pw.reserve((size_t)(5 * rows_per_chunk) * sizeof(double));
  if (rc) return rc;
  double* out[5] = {mean, variance, k_mean, k_var, k_ratio};
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    rc = upload_rows(x, nullptr, r0, nr, stride_obs, n_draws, esz, eng->d_in.p, s);
    if (!rc) rc = upload_rows(log_weights, nullptr, r0, nr, stride_obs, n_draws, esz, eng->d_lw.p, s);
    if (!rc && log_ratios) rc = upload_rows(log_ratios, nullptr, r0, nr, stride_obs, n_draws, esz, eng->d_slab.p, s);
    if (rc) return rc;
    double* d = eng->d_pw.as<double>();
    PLA_HIP(pla::launch_e_loo(eng->d_in.p, eng->d_lw.p, log_ratios ? eng->d_slab.p : nullptr, dtype, nr, (int)n_draws, n_draws, 1, (int)tail_len,
                              d, d + nr, d + 2 * nr, d + 3 * nr, d + 4 * nr, eng->d_slow.as<unsigned>(), eng->counters, s));
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
  if (int rc0 = check_engine_types(eng, dtype, mem_space)) return rc0;
  if (n_obs < 0 || n_probs < 0) return fail(PLA_ERR_ARG, "negative size");
  if (n_obs > 0 && (!x || !log_weights)) return fail(PLA_ERR_ARG, "x / log_weights is NULL");
  if (n_obs > 0 && n_probs > 0 && (!probs || !out)) return fail(PLA_ERR_ARG, "probs / out is NULL");
  if (int rc0 = check_n_draws(n_draws, 1)) return rc0;
  if (stride_draw <= 0 || stride_obs < 0) return fail(PLA_ERR_ARG, "bad strides");
  for (int64_t i = 0; i < n_probs; ++i)
    if (!(probs[i] > 0.0 && probs[i] < 1.0)) return fail(PLA_ERR_ARG, "probs must be between 0 and 1");  // e_loo.py:158-159
  if (n_obs == 0 || n_probs == 0) return PLA_OK;
  PLA_ENGINE_CALL(eng, stream);
  int rc = eng->d_probs.reserve((size_t)n_probs * sizeof(double));
  if (rc) return rc;
  PLA_HIP(hipMemcpyAsync(eng->d_probs.p, probs, (size_t)n_probs * sizeof(double), hipMemcpyHostToDevice, s));
  PLA_HIP(hipStreamSynchronize(s));  // (the caller's probs array may go away after the call)
  const double* dp = eng->d_probs.as<const double>();
  if (mem_space == PLA_DEVICE) {
    rc = eng->d_slow.reserve((size_t)n_obs * sizeof(unsigned));
    if (rc) return rc;
    PLA_HIP(pla::launch_e_loo_quantiles(x, log_weights, dtype, n_obs, (int)n_draws, stride_obs, stride_draw, dp, (int)n_probs, out,
                                        eng->d_slow.as<unsigned>(), eng->counters, s));
    eng->last_kernels = pla::last_rows_kernels();
    return PLA_OK;
  }
  if (stride_draw != 1) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs stride_draw == 1");
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const size_t row_bytes = (size_t)n_draws * esz;
  int64_t rows_per_chunk = (int64_t)(((size_t)1 << 29) / row_bytes);
  if (rows_per_chunk < 1) rows_per_chunk = 1;
  if (rows_per_chunk > n_obs) rows_per_chunk = n_obs;
  rc = eng->d_in.reserve((size_t)rows_per_chunk * row_bytes);
  if (!rc) rc = eng->d_lw.reserve((size_t)rows_per_chunk * row_bytes);
  if (!rc) rc = eng->d_pw.reserve((size_t)(rows_per_chunk * n_probs) * sizeof(double));
  if (!rc) rc = eng->d_slow.reserve((size_t)rows_per_chunk * sizeof(unsigned));
  if (rc) return rc;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    rc = upload_rows(x, nullptr, r0, nr, stride_obs, n_draws, esz, eng->d_in.p, s);
    if (!rc) rc = upload_rows(log_weights, nullptr, r0, nr, stride_obs, n_draws, esz, eng->d_lw.p, s);
    if (rc) return rc;
    PLA_HIP(pla::launch_e_loo_quantiles(eng->d_in.p, eng->d_lw.p, dtype, nr, (int)n_draws, n_draws, 1, dp, (int)n_probs, eng->d_pw.as<double>(),
                                        eng->d_slow.as<unsigned>(), eng->counters, s));
    eng->last_kernels = pla::last_rows_kernels();
    PLA_HIP(hipMemcpyAsync(out + r0 * n_probs, eng->d_pw.as<double>(), (size_t)(nr * n_probs) * sizeof(double), hipMemcpyDeviceToHost, s));
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

}  // extern "C"
