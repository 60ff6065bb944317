// C ABI of libpyloo_amd.so, the block-wise passes beside PSIS-LOO: Mix-IS, LOO-PIT, diagnostics, influence, leave-future-out,
// relative efficiency.
#include <functional>

#include "pla_capi.h"

using namespace pla::capi;

extern "C" {

// ---- Mix-IS-LOO (pla_mixis.h) -----------------------------------------------------------------------------------------------------
static int mixis_check(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                       int64_t stride_draw, int mem_space) {
  if (int rc = check_types(dtype, mem_space)) return rc;
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
  int rc = eng->d_in.reserve((size_t)(draws_fastest ? rows : n_draws) * (size_t)pitch * esz);
  if (rc) return rc;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    if (draws_fastest) {
      PLA_HIP(hipMemcpy2DAsync(eng->d_in.p, (size_t)n_draws * esz, (const char*)ll + (size_t)r0 * (size_t)stride_obs * esz,
                               (size_t)(n_obs == 1 ? n_draws : stride_obs) * esz, (size_t)n_draws * esz, (size_t)nr,
                               hipMemcpyHostToDevice, s));
      rc = f(eng->d_in.p, r0, nr, n_draws, (int64_t)1, (int64_t)1);
    } else {
      PLA_HIP(hipMemcpy2DAsync(eng->d_in.p, (size_t)pitch * esz, (const char*)ll + (size_t)r0 * esz,
                               (size_t)(n_draws == 1 ? n_obs : stride_draw) * esz, (size_t)nr * esz, (size_t)n_draws,
                               hipMemcpyHostToDevice, s));
      rc = f(eng->d_in.p, r0, nr, (int64_t)1, pitch, n_obs);  // (16-byte loads where a device matrix of pitch n_obs takes them)
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
  PLA_ENGINE_CALL(eng, stream);
  const MixisWorkspace w(n_obs, n_draws);
  rc = eng->d_mix.reserve(w.total * sizeof(double));
  if (rc) return rc;
  double* ws = eng->d_mix.as<double>();
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
  PLA_ENGINE_CALL(eng, stream);
  const MixisWorkspace w(n_obs, n_draws);
  rc = eng->d_mix.reserve(w.total * sizeof(double));
  if (rc) return rc;
  double* ws = eng->d_mix.as<double>();
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

// ---- LOO-PIT (csrc/pla_pit.h) ---------------------------------------------------------------------------------------------------
int pla_loo_pit(pla_engine* eng, const void* in, const void* y_hat, const double* y, int dtype, int64_t n_obs, int64_t n_draws,
                int64_t stride_obs, int64_t stride_draw, int64_t yh_stride_obs, int64_t yh_stride_draw, int input_kind, int method,
                int64_t tail_count, int mem_space, void* stream, double* pit_le, double* pit_lt, double* diag, int64_t* n_replaced) {
  if (int rc0 = check_engine_types(eng, dtype, mem_space)) return rc0;
  if (input_kind != PLA_PIT_LOGLIK && input_kind != PLA_PIT_LOG_WEIGHTS) return fail(PLA_ERR_ARG, "bad input_kind");
  if (method != PLA_PSIS && method != PLA_SIS && method != PLA_TIS) return fail(PLA_ERR_ARG, "bad method");
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (int rc0 = check_n_draws(n_draws, 2)) return rc0;
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
  PLA_ENGINE_CALL(eng, stream);
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
    rc = eng->d_in.reserve(block_bytes);
    if (rc) return rc;
  }
  const bool yh_transpose = host ? yh_of : obs_fastest_device(mem_space, nullptr, n_obs, n_draws, yh_stride_obs, yh_stride_draw);
  if (host || yh_transpose) {
    rc = eng->d_pit.reserve(block_bytes);
    if (rc) return rc;
  }
  if (host && (in_of || yh_of)) {
    rc = eng->d_slab.reserve(block_bytes);
    if (rc) return rc;
  }
  unsigned long long* d_count = nullptr;
  const double* dy = y;
  double *d_le = pit_le, *d_lt = pit_lt, *d_diag = loglik ? diag : nullptr;
  HostOutputs out(eng, s);
  if (host) {  // (y goes up into the first column)
    d_count = eng->counters + pla::kCounterPitReplaced;
    rc = out.reserve(4, n_obs, d_count);
    if (rc) return rc;
    PLA_HIP(hipMemcpyAsync(out.col(0), y, (size_t)n_obs * sizeof(double), hipMemcpyHostToDevice, s));
    dy = out.col(0);
    d_le = out.col(1);
    d_lt = out.col(2);
    d_diag = out.col(3);
  } else {
    d_count = (unsigned long long*)n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  }

  std::string label;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    // the weights' source as a compact draws-fastest block in d_in (log-likelihood: negated, NaN -> -1e10)
    const void* lw_block = eng->d_in.p;
    const char* prep = "";
    if (!host) {
      PLA_HIP(pla::launch_pit_prepare((const char*)in + (size_t)r0 * (size_t)stride_obs * esz, dtype, stride_obs, stride_draw, nr, S,
                                      eng->d_in.p, d_count, s, &prep));
    } else if (in_of) {  // the (n_draws, nr) slab as it lies, turned on the device
      rc = upload_slab(in, r0, nr, stride_draw, n_draws, esz, eng->d_slab.p, s);
      if (rc) return rc;
      if (loglik) PLA_HIP(pla::launch_pit_prepare(eng->d_slab.p, dtype, 1, nr, nr, S, eng->d_in.p, d_count, s, &prep));
      else PLA_HIP(pla::launch_transpose_rows(eng->d_slab.p, dtype, nr, 0, nr, S, eng->d_in.p, s));
    } else {
      void* up = loglik ? eng->d_lw.p : eng->d_in.p;  // (the weights buffer is free until the weights pass writes it)
      rc = upload_rows(in, nullptr, r0, nr, stride_obs, n_draws, esz, up, s);
      if (rc) return rc;
      if (loglik) PLA_HIP(pla::launch_pit_prepare(eng->d_lw.p, dtype, n_draws, 1, nr, S, eng->d_in.p, d_count, s, &prep));
    }
    if (loglik) {
      p.in = eng->d_in.p;
      p.n_obs = nr;
      p.diag = d_diag ? d_diag + r0 : nullptr;
      p.lw_out = eng->d_lw.p;
      PLA_HIP(pla::launch_rows(p, dtype, true, s));
      lw_block = eng->d_lw.p;
    }
    // the predictive draws of the block: in place, or draws fastest in d_pit
    const void* yh_block = (const char*)y_hat + (size_t)r0 * (size_t)yh_stride_obs * esz;
    int64_t yso = yh_stride_obs, ysd = yh_stride_draw;
    if (host && yh_of) {
      rc = upload_slab(y_hat, r0, nr, yh_stride_draw, n_draws, esz, eng->d_slab.p, s);
      if (rc) return rc;
      PLA_HIP(pla::launch_transpose_rows(eng->d_slab.p, dtype, nr, 0, nr, S, eng->d_pit.p, s));
    } else if (host) {
      rc = upload_rows(y_hat, nullptr, r0, nr, yh_stride_obs, n_draws, esz, eng->d_pit.p, s);
      if (rc) return rc;
    } else if (yh_transpose) {
      PLA_HIP(pla::launch_transpose_rows(y_hat, dtype, yh_stride_draw, r0, nr, S, eng->d_pit.p, s));
    }
    if (host || yh_transpose) {
      yh_block = eng->d_pit.p;
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
  return out.finish({nullptr, pit_le, pit_lt, loglik ? diag : nullptr}, n_replaced);
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
  PLA_ENGINE_CALL(eng, stream);
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
  rc = eng->d_in.reserve(block_bytes);
  if (rc) return rc;
  if (host && in_of) {
    rc = eng->d_slab.reserve(block_bytes);
    if (rc) return rc;
  }
  unsigned long long* d_count = nullptr;
  double *d_diag = diag, *d_elpd = elpd_i, *d_ess = ess_w, *d_var = var_log;
  HostOutputs out(eng, s);
  if (host) {
    d_count = eng->counters + pla::kCounterPitReplaced;
    rc = out.reserve(4, m, d_count);
    if (rc) return rc;
    d_diag = out.col(0);
    d_elpd = out.col(1);
    d_ess = out.col(2);
    d_var = out.col(3);
  } else {
    d_count = (unsigned long long*)n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  }

  std::string label;
  for (int64_t r0 = 0; r0 < m; r0 += rows) {
    const int64_t nr = m - r0 < rows ? m - r0 : rows;
    const char* prep = "";
    if (!host) {
      PLA_HIP(pla::launch_diag_prepare(ll, dtype, n_obs, stride_obs, stride_draw, row_index ? row_index + r0 : nullptr, r0, nr, S, eng->d_in.p,
                                       d_count, s, &prep));
    } else if (in_of) {  // the (n_draws, nr) slab as it lies, turned on the device
      rc = upload_slab(ll, r0, nr, stride_draw, n_draws, esz, eng->d_slab.p, s);
      if (rc) return rc;
      PLA_HIP(pla::launch_diag_prepare(eng->d_slab.p, dtype, nr, 1, nr, nullptr, 0, nr, S, eng->d_in.p, d_count, s, &prep));
    } else {  // (the weights buffer is free until the weights pass writes it)
      rc = upload_rows(ll, row_index, r0, nr, stride_obs, n_draws, esz, eng->d_lw.p, s);
      if (rc) return rc;
      PLA_HIP(pla::launch_diag_prepare(eng->d_lw.p, dtype, nr, n_draws, 1, nullptr, 0, nr, S, eng->d_in.p, d_count, s, &prep));
    }
    p.in = eng->d_in.p;
    p.n_obs = nr;
    p.diag = d_diag ? d_diag + r0 : nullptr;
    p.lw_out = eng->d_lw.p;
    PLA_HIP(pla::launch_rows(p, dtype, true, s));
    PLA_HIP(pla::launch_diag(eng->d_lw.p, eng->d_in.p, -1.0, dtype, nr, S, n_draws, 1, n_draws, 1, d_elpd ? d_elpd + r0 : nullptr,
                             d_ess ? d_ess + r0 : nullptr, d_var ? d_var + r0 : nullptr, s, route, (int)sizeof(route)));
    if (r0 == 0)
      label = std::string(prep) + " -> " + std::string(pla::last_rows_kernels()) + " -> " + route +
              (host ? " (matrix staged in blocks)" : " per block of observations");
    if (host) PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  eng->last_kernels = label;
  if (!host) return PLA_OK;
  return out.finish({diag, elpd_i, ess_w, var_log}, n_replaced);
}

// the kernel alone on caller-supplied log weights: device matrices in place, host matrices staged in blocks (lw in d_in, ll in d_lw)
int pla_loo_diag_weights(pla_engine* eng, const void* lw, const void* ll, int dtype, int64_t n_obs, int64_t n_draws,
                         int64_t lw_stride_obs, int64_t lw_stride_draw, int64_t ll_stride_obs, int64_t ll_stride_draw, int mem_space,
                         void* stream, double* elpd_i, double* ess_w, double* var_log) {
  if (int rc0 = check_engine_types(eng, dtype, mem_space)) return rc0;
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (int rc0 = check_n_draws(n_draws, 2)) return rc0;
  if (lw_stride_obs <= 0 || lw_stride_draw <= 0 || ll_stride_obs <= 0 || ll_stride_draw <= 0)
    return fail(PLA_ERR_ARG, "strides must be positive");
  if (n_obs > 0 && (!lw || !ll)) return fail(PLA_ERR_ARG, "lw / ll is NULL");
  const bool host = mem_space == PLA_HOST;
  if (host && (lw_stride_draw != 1 || ll_stride_draw != 1))
    return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST matrices need unit stride along the draws");
  PLA_ENGINE_CALL(eng, stream);
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
  const size_t block_bytes = (size_t)rows * (size_t)n_draws * esz;
  HostOutputs out(eng, s);
  int rc = eng->d_in.reserve(block_bytes);
  if (!rc) rc = eng->d_lw.reserve(block_bytes);
  if (!rc) rc = out.reserve(3, n_obs);
  if (rc) return rc;
  double *d_elpd = out.col(0), *d_ess = out.col(1), *d_var = out.col(2);
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    rc = upload_rows(lw, nullptr, r0, nr, lw_stride_obs, n_draws, esz, eng->d_in.p, s);
    if (!rc) rc = upload_rows(ll, nullptr, r0, nr, ll_stride_obs, n_draws, esz, eng->d_lw.p, s);
    if (rc) return rc;
    PLA_HIP(pla::launch_diag(eng->d_in.p, eng->d_lw.p, 1.0, dtype, nr, S, n_draws, 1, n_draws, 1, d_elpd + r0, d_ess + r0, d_var + r0, s, route,
                             (int)sizeof(route)));
    PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  eng->last_kernels = std::string(route) + " (matrices staged in blocks)";
  return out.finish({elpd_i, ess_w, var_log});
}

// ---- LOO influence (csrc/pla_influence.h) ----------------------------------------------------------------------------------------
// Z^T of the call into d_inf once, then pla_loo_diag's pipeline with the influence kernel as the consumer of a block's weights in
// d_lw (PLA_PIT_LOGLIK), or the kernel alone on the caller's weights: a device matrix in place, a host matrix staged through d_in
// (PLA_PIT_LOG_WEIGHTS).  Outputs of a host call in d_pw: kl, ess_w and diag [m] each, then shift and m2 of ONE block of rows,
// (rows, n_quant) each, copied to the caller block by block -- bounded like the staging of the input.
int pla_loo_influence(const pla_influence_args* a) {
  if (!a) return fail(PLA_ERR_ARG, "args is NULL");
  if (a->struct_size != (int64_t)sizeof(pla_influence_args))
    return fail(PLA_ERR_ARG, "struct_size is %lld, pla_influence_args of this library has %lld bytes", (long long)a->struct_size,
                (long long)sizeof(pla_influence_args));
  pla_engine* eng = a->engine;
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  const bool loglik = a->kind == PLA_PIT_LOGLIK;
  if (!loglik && a->kind != PLA_PIT_LOG_WEIGHTS) return fail(PLA_ERR_ARG, "bad kind");
  const int dtype = a->dtype, mem_space = a->mem_space;
  const int64_t n_obs = a->n_obs, n_draws = a->n_draws, stride_obs = a->stride_obs, stride_draw = a->stride_draw, P = a->n_quant;
  int rc;
  if (loglik) {
    rc = check_common(eng, a->mat, dtype, n_obs, n_draws, stride_obs, stride_draw, a->method, a->tail_count, mem_space);
    if (rc) return rc;
  } else {
    rc = check_engine_types(eng, dtype, mem_space);
    if (rc) return rc;
    if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
    if (n_obs > 0 && !a->mat) return fail(PLA_ERR_ARG, "the matrix pointer is NULL");
    if (a->row_index) return fail(PLA_ERR_ARG, "row_index needs PLA_PIT_LOGLIK");
  }
  if (int rc0 = check_n_draws(n_draws, 2)) return rc0;
  if (stride_obs <= 0 || stride_draw <= 0) return fail(PLA_ERR_ARG, "strides must be positive");
  if (P < 1 || P > pla::kInfMaxQuant) return fail(PLA_ERR_ARG, "n_quant must lie in [1, %d], got %lld", pla::kInfMaxQuant, (long long)P);
  if (!a->theta || !a->center || !a->scale) return fail(PLA_ERR_ARG, "theta / center / scale is NULL");
  if (a->theta_stride_draw <= 0 || a->theta_stride_quant <= 0) return fail(PLA_ERR_ARG, "theta strides must be positive");
  if (a->row_index) {
    rc = check_rows(a->row_index, a->n_rows, n_obs, mem_space);
    if (rc) return rc;
  }
  const int64_t m = a->row_index ? a->n_rows : n_obs;  // rows of this call
  const bool host = mem_space == PLA_HOST;
  const bool in_of = loglik && host_obs_fastest(n_obs, n_draws, stride_obs, stride_draw);
  if (host && stride_draw != 1 && !in_of)
    return fail(PLA_ERR_UNSUPPORTED, loglik ? "PLA_HOST matrices need unit stride along the draws, or along the observations"
                                            : "PLA_HOST log weights need unit stride along the draws");
  if (host && in_of && a->row_index) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST row selection needs unit stride along the draws");
  const bool theta_sp = a->theta_stride_quant == 1 && a->theta_stride_draw == P;
  const bool theta_ps = a->theta_stride_draw == 1 && (P == 1 || a->theta_stride_quant == n_draws);
  if (host && !theta_sp && !theta_ps) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST theta must be dense, (n_draws, n_quant) or (n_quant, n_draws)");
  PLA_ENGINE_CALL(eng, a->stream);
  if (m == 0) {
    if (host && a->n_replaced) *a->n_replaced = 0;
    if (!host && a->n_replaced) PLA_HIP(hipMemsetAsync(a->n_replaced, 0, sizeof(int64_t), s));
    return PLA_OK;
  }
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int S = (int)n_draws, Pq = (int)P;

  // ---- Z^T, once per call
  int s_pad, p_pad;
  pla::influence_pads(S, Pq, &s_pad, &p_pad);
  const size_t zt_doubles = (size_t)s_pad * (size_t)p_pad, th_doubles = (size_t)n_draws * (size_t)P;
  rc = eng->d_inf.reserve((zt_doubles + (host ? th_doubles + 2 * (size_t)P : 0)) * sizeof(double));
  if (rc) return rc;
  double* zt = eng->d_inf.as<double>();
  const double *d_theta = a->theta, *d_center = a->center, *d_scale = a->scale;
  if (host) {
    double* up = zt + zt_doubles;
    PLA_HIP(hipMemcpyAsync(up, a->theta, th_doubles * sizeof(double), hipMemcpyHostToDevice, s));
    PLA_HIP(hipMemcpyAsync(up + th_doubles, a->center, (size_t)P * sizeof(double), hipMemcpyHostToDevice, s));
    PLA_HIP(hipMemcpyAsync(up + th_doubles + P, a->scale, (size_t)P * sizeof(double), hipMemcpyHostToDevice, s));
    d_theta = up;
    d_center = up + th_doubles;
    d_scale = up + th_doubles + P;
  }
  PLA_HIP(pla::launch_influence_prepare(d_theta, a->theta_stride_draw, a->theta_stride_quant, d_center, d_scale, S, Pq, zt, s));

  // ---- the rows of a block, and for PLA_PIT_LOGLIK its weights pass as pla_importance_weights sets it up
  pla::RowsParams p{};
  int64_t rows = staged_chunk_rows(mem_space, true, m, n_draws, esz);
  if (loglik) {
    rc = weights_block_setup(eng, a->method, a->tail_count, n_draws, esz, s, &rows, &p);
    if (rc) return rc;
  }

  // ---- outputs: the caller's device arrays, or engine memory (shift and m2 of a host call: one block at a time)
  unsigned long long* d_count = nullptr;
  double *d_shift = a->shift, *d_m2 = a->m2, *d_kl = a->kl, *d_ess = a->ess_w, *d_diag = loglik ? a->diag : nullptr;
  HostOutputs out(eng, s);
  if (host) {
    d_count = eng->counters + pla::kCounterPitReplaced;
    rc = out.reserve(1, 3 * m + 2 * rows * P, d_count);
    if (rc) return rc;
    d_kl = out.col(0);
    d_ess = d_kl + m;
    d_diag = d_ess + m;
    d_shift = d_diag + m;
    d_m2 = d_shift + (size_t)rows * (size_t)P;
  } else {
    d_count = (unsigned long long*)a->n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  }
  // the kernel on one block; a host call's shift and m2 go back to the caller behind it (the caller synchronises before the next block)
  const auto kernel = [&](const void* lw, int64_t r0, int64_t nr, int64_t so, int64_t sd, char* route, int cap) -> int {
    const size_t at = host ? 0 : (size_t)r0 * (size_t)P;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_influence(lw, dtype, nr, S, so, sd, zt, Pq, d_shift ? d_shift + at : nullptr, d_m2 ? d_m2 + at : nullptr,
                                    d_kl ? d_kl + r0 : nullptr, d_ess ? d_ess + r0 : nullptr, s, route, cap));
    }
    if (host) {
      const size_t bytes = (size_t)nr * (size_t)P * sizeof(double);
      if (a->shift) PLA_HIP(hipMemcpyAsync(a->shift + (size_t)r0 * (size_t)P, d_shift, bytes, hipMemcpyDeviceToHost, s));
      if (a->m2) PLA_HIP(hipMemcpyAsync(a->m2 + (size_t)r0 * (size_t)P, d_m2, bytes, hipMemcpyDeviceToHost, s));
    }
    return PLA_OK;
  };
  char route[160];
  std::string label;

  if (!loglik && !host) {  // the kernel alone, the weights in place
    rc = kernel(a->mat, 0, n_obs, stride_obs, stride_draw, route, (int)sizeof(route));
    if (rc) return rc;
    eng->last_kernels = std::string("influence_prepare_kernel -> ") + route + " (matrix read in place)";
    return PLA_OK;
  }
  if (!loglik) {  // ... staged in blocks
    rc = eng->d_in.reserve((size_t)rows * (size_t)n_draws * esz);
    if (rc) return rc;
    for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
      const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
      rc = upload_rows(a->mat, nullptr, r0, nr, stride_obs, n_draws, esz, eng->d_in.p, s);
      if (!rc) rc = kernel(eng->d_in.p, r0, nr, n_draws, 1, route, (int)sizeof(route));
      if (rc) return rc;
      PLA_HIP(hipStreamSynchronize(s));  // the staging buffer is reused by the next block
    }
    label = std::string("influence_prepare_kernel, rows copied -> ") + route + " (matrix staged in blocks)";
  } else {
    const size_t block_bytes = (size_t)rows * (size_t)n_draws * esz;
    rc = eng->d_in.reserve(block_bytes);
    if (rc) return rc;
    if (host && in_of) {
      rc = eng->d_slab.reserve(block_bytes);
      if (rc) return rc;
    }
    for (int64_t r0 = 0; r0 < m; r0 += rows) {
      const int64_t nr = m - r0 < rows ? m - r0 : rows;
      const char* prep = "";
      if (!host) {
        PLA_HIP(pla::launch_diag_prepare(a->mat, dtype, n_obs, stride_obs, stride_draw, a->row_index ? a->row_index + r0 : nullptr, r0, nr, S,
                                         eng->d_in.p, d_count, s, &prep));
      } else if (in_of) {  // the (n_draws, nr) slab as it lies, turned on the device
        rc = upload_slab(a->mat, r0, nr, stride_draw, n_draws, esz, eng->d_slab.p, s);
        if (rc) return rc;
        PLA_HIP(pla::launch_diag_prepare(eng->d_slab.p, dtype, nr, 1, nr, nullptr, 0, nr, S, eng->d_in.p, d_count, s, &prep));
      } else {  // (the weights buffer is free until the weights pass writes it)
        rc = upload_rows(a->mat, a->row_index, r0, nr, stride_obs, n_draws, esz, eng->d_lw.p, s);
        if (rc) return rc;
        PLA_HIP(pla::launch_diag_prepare(eng->d_lw.p, dtype, nr, n_draws, 1, nullptr, 0, nr, S, eng->d_in.p, d_count, s, &prep));
      }
      p.in = eng->d_in.p;
      p.n_obs = nr;
      p.diag = d_diag ? d_diag + r0 : nullptr;
      p.lw_out = eng->d_lw.p;
      PLA_HIP(pla::launch_rows(p, dtype, true, s));
      rc = kernel(eng->d_lw.p, r0, nr, n_draws, 1, route, (int)sizeof(route));
      if (rc) return rc;
      if (r0 == 0)
        label = std::string("influence_prepare_kernel, ") + prep + " -> " + std::string(pla::last_rows_kernels()) + " -> " + route +
                (host ? " (matrix staged in blocks)" : " per block of observations");
      if (host) PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
    }
  }
  eng->last_kernels = label;
  if (!host) return PLA_OK;
  if (a->kl) PLA_HIP(hipMemcpyAsync(a->kl, d_kl, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  if (a->ess_w) PLA_HIP(hipMemcpyAsync(a->ess_w, d_ess, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  if (a->diag && loglik) PLA_HIP(hipMemcpyAsync(a->diag, d_diag, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  unsigned long long h_count = 0;
  PLA_HIP(hipMemcpyAsync(&h_count, d_count, sizeof(h_count), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (a->n_replaced) *a->n_replaced = (int64_t)h_count;
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
  PLA_ENGINE_CALL(eng, stream);
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int S = (int)n_draws;
  const int64_t C = pla::lfo_chunk_rows();
  const int64_t extra = ratios_only ? 0 : horizon - 1;  // rows a block needs beyond one per step
  const bool staged = host || dev_of;

  // steps per block: the staging's size in f64 ratios, whole chunks
  int64_t rows = staged_chunk_rows(mem_space, true, n_steps, n_draws, sizeof(double));
  const bool split = !ratios_only && lw_split_route(PLA_PSIS, n_draws, tail_count, &rows);  // (long rows, as in pla_importance_weights)
  if (rows < n_steps) rows = rows / C * C < C ? C : rows / C * C;
  if (rows > n_steps) rows = n_steps;
  const int64_t chunks = (rows + C - 1) / C;
  const size_t block_bytes = (size_t)rows * (size_t)n_draws * sizeof(double);
  int rc = eng->d_lfo.reserve((size_t)(chunks + 1) * (size_t)n_draws * sizeof(double));
  if (rc) return rc;
  double* run = eng->d_lfo.as<double>();
  double* carry = run + n_draws;
  if (!ratios_only || host) {
    rc = eng->d_in.reserve(block_bytes);
    if (rc) return rc;
  }
  if (staged) {
    const size_t stage_bytes = (size_t)(rows + extra) * (size_t)n_draws * esz;
    rc = eng->d_pit.reserve(stage_bytes);
    if (rc) return rc;
    if (in_of) {
      rc = eng->d_slab.reserve(stage_bytes);
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
    rc = eng->d_slow.reserve((size_t)rows * sizeof(unsigned));
    if (rc) return rc;
    p.slow_list = eng->d_slow.as<unsigned>();
    rc = ensure_l1_table(eng, tail_count, s, &p.l1_table);
    if (rc) return rc;
    if (split) {
      rc = lw_split_workspace(eng, tail_count, rows, &p);
      if (rc) return rc;
    }
    rc = eng->d_lw.reserve(block_bytes);
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
  HostOutputs out(eng, s);  // (its own two counters are the call's business: zeroed and read below)
  if (!ratios_only && (host || (!diag && first_high))) {
    rc = out.reserve(2, n_steps);
    if (rc) return rc;
    d_diag = out.col(0);
    if (host) d_elpd = out.col(1);
  }
  if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  PLA_HIP(hipMemsetAsync(run, 0, (size_t)n_draws * sizeof(double), s));

  std::string label;
  char route[160];
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
        PLA_HIP(pla::launch_transpose_rows(ll, dtype, stride_draw, r0, n_stage, S, eng->d_pit.p, s));
      } else if (in_of) {  // the (n_draws, n_stage) slab as it lies, turned on the device
        rc = upload_slab(ll, r0, n_stage, stride_draw, n_draws, esz, eng->d_slab.p, s);
        if (rc) return rc;
        PLA_HIP(pla::launch_transpose_rows(eng->d_slab.p, dtype, n_stage, 0, n_stage, S, eng->d_pit.p, s));
      } else {
        rc = upload_rows(ll, nullptr, r0, n_stage, stride_obs, n_draws, esz, eng->d_pit.p, s);
        if (rc) return rc;
      }
    }
    if (staged) {
      blk = eng->d_pit.p;
      blk_so = n_draws;
    }
    double* lr = (ratios_only && !host) ? ratios_out + (size_t)j0 * (size_t)n_draws : eng->d_in.as<double>();
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
    p.lw_out = eng->d_lw.p;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_rows(p, PLA_F64, true, s));
    }
    PLA_HIP(pla::launch_lfo_predict(eng->d_lw.as<const double>(), blk, dtype, blk_so, nb, S, (int)horizon, j0 == 0, d_diag ? d_diag + j0 : nullptr,
                                    d_elpd ? d_elpd + j0 : nullptr, d_count, s, route, (int)sizeof(route)));
    if (j0 == 0)
      label = std::string(dev_of ? "transpose_rows_kernel -> " : "") + scan + " + lfo_carry_kernel -> " + pla::last_rows_kernels() + " -> " +
              route + (host ? " (matrix staged in blocks)" : " per block of steps");
    if (host) PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  eng->last_kernels = label;
  if (!ratios_only && d_high) PLA_HIP(pla::launch_lfo_first_high(d_diag, n_steps, k_threshold, d_high, s));
  if (!host) return PLA_OK;
  rc = out.copy_back({diag, elpd_i});
  if (rc) return rc;
  unsigned long long h_count = 0;
  long long h_high = n_steps;
  PLA_HIP(hipMemcpyAsync(&h_count, d_count, sizeof(h_count), hipMemcpyDeviceToHost, s));
  if (!ratios_only) PLA_HIP(hipMemcpyAsync(&h_high, d_high, sizeof(h_high), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h_count;
  if (first_high) *first_high = (int64_t)h_high;
  return PLA_OK;
}

// Backward mode (csrc/pla_lfo_bw.h): the same pipeline in descending row order.  A block is whole chunks of q = last - t (the sums
// begin at q = 0, the fit; the steps at q0 = last - t_0, so the first q0 <= M values of q are no step and only feed the sums); its
// ratios go to d_in compact in q, and the weights pass begins at the block's first step.  A staged block holds the rows [lo, hi]
// it touches in ascending order in d_pit: down to the row below its lowest step (the one that completes its last chunk's total;
// the last block stops at its lowest step), up to the end of its highest step's window -- the M - 1 extra rows lie on the side
// already visited.
static int lfo_bw_impl(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                       int64_t last, int64_t n_steps, int64_t horizon, int64_t tail_count, double k_threshold, int mem_space, void* stream,
                       double* diag, double* elpd_i, int64_t* first_high, int64_t* n_replaced) {
  const bool host = mem_space == PLA_HOST;
  const bool in_of = host && host_obs_fastest(n_obs, n_draws, stride_obs, stride_draw);
  const bool dev_of = obs_fastest_device(mem_space, nullptr, n_obs, n_draws, stride_obs, stride_draw);
  if (stride_draw != 1 && !in_of && !dev_of)
    return fail(PLA_ERR_UNSUPPORTED, "the matrix needs unit stride along the draws, or along the observations (stride_draw >= n_obs)");
  if (stride_draw == 1 && n_obs > 1 && stride_obs < n_draws) return fail(PLA_ERR_ARG, "stride_obs is smaller than n_draws");
  PLA_ENGINE_CALL(eng, stream);
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int S = (int)n_draws;
  const int64_t C = pla::lfo_chunk_rows();
  const int64_t t0 = last < n_obs - horizon ? last : n_obs - horizon;
  const int64_t q0 = last - t0;       // 0 .. horizon: the q of step 0
  const int64_t n_q = q0 + n_steps;   // the q of the pass: 0 .. n_q - 1
  const bool staged = host || dev_of;

  // q per block: the staging's size in f64 ratios, whole chunks
  int64_t rows = staged_chunk_rows(mem_space, true, n_q, n_draws, sizeof(double));
  const bool split = lw_split_route(PLA_PSIS, n_draws, tail_count, &rows);  // (long rows, as in pla_importance_weights)
  if (rows < n_q) rows = rows / C * C < C ? C : rows / C * C;
  if (rows > n_q) rows = n_q;
  const int64_t chunks = (rows + C - 1) / C;
  const size_t block_bytes = (size_t)rows * (size_t)n_draws * sizeof(double);
  int rc = eng->d_lfo.reserve((size_t)(chunks + 1) * (size_t)n_draws * sizeof(double));
  if (rc) return rc;
  double* run = eng->d_lfo.as<double>();
  double* carry = run + n_draws;
  rc = eng->d_in.reserve(block_bytes);
  if (rc) return rc;
  if (staged) {
    const size_t stage_bytes = (size_t)(rows + horizon) * (size_t)n_draws * esz;
    rc = eng->d_pit.reserve(stage_bytes);
    if (rc) return rc;
    if (in_of) {
      rc = eng->d_slab.reserve(stage_bytes);
      if (rc) return rc;
    }
  }
  pla::RowsParams p{};
  p.n_draws = S;
  p.method = PLA_PSIS;
  p.tail_count = (int)tail_count;
  p.tail_cap = pow2_at_least(p.tail_count);
  p.scale_value = 1.0;
  p.counters = eng->counters;
  p.stride_obs = n_draws;
  p.stride_draw = 1;
  PLA_HIP(hipMemsetAsync(eng->counters, 0, pla::kCountersPerCall * sizeof(unsigned long long), s));
  rc = eng->d_slow.reserve((size_t)rows * sizeof(unsigned));
  if (rc) return rc;
  p.slow_list = eng->d_slow.as<unsigned>();
  rc = ensure_l1_table(eng, tail_count, s, &p.l1_table);
  if (rc) return rc;
  if (split) {
    rc = lw_split_workspace(eng, tail_count, rows, &p);
    if (rc) return rc;
  }
  rc = eng->d_lw.reserve(block_bytes);
  if (rc) return rc;
  // outputs: the caller's device arrays, or engine memory (a host call; k when the caller wants first_high without it)
  double *d_diag = diag, *d_elpd = elpd_i;
  unsigned long long* d_count = (unsigned long long*)n_replaced;
  long long* d_high = (long long*)first_high;
  if (host) {
    d_count = eng->counters + pla::kCounterLfoReplaced;
    d_high = (long long*)(eng->counters + pla::kCounterLfoFirstHigh);
  }
  HostOutputs out(eng, s);  // (its own two counters are the call's business: zeroed and read below)
  if (host || (!diag && first_high)) {
    rc = out.reserve(2, n_steps);
    if (rc) return rc;
    d_diag = out.col(0);
    if (host) d_elpd = out.col(1);
  }
  if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  PLA_HIP(hipMemsetAsync(run, 0, (size_t)n_draws * sizeof(double), s));

  std::string label;
  char route[160];
  for (int64_t qb = 0; qb < n_q; qb += rows) {
    const int64_t nq = n_q - qb < rows ? n_q - qb : rows;
    const bool last_block = qb + nq == n_q;
    const int64_t skip = q0 > qb ? (q0 - qb < nq ? q0 - qb : nq) : 0;  // q of the block before the first step of the pass
    const int64_t nb = nq - skip;                                      // steps of the block
    const int64_t j0 = qb + skip - q0;                                 // ... the first of them
    const int64_t n_load = last_block ? nq - 1 : nq;                   // (the last step's own row enters no sum)
    const int64_t top = last - 1 - qb;                                 // the row of the block's first q (read when n_load > 0)
    const int64_t t_first = last - qb - skip;                          // the row of the block's first step
    const int64_t lo = last - qb - nq + (last_block ? 1 : 0);          // >= 0: the lowest row the block touches
    int64_t hi = nb > 0 ? t_first + horizon - 1 : top;                 // <= n_obs - 1: the highest
    if (hi < top) hi = top;
    const int64_t n_stage = hi - lo + 1;                               // <= nq + horizon
    const char* base = (const char*)ll;
    int64_t blk_so = stride_obs, row0 = 0;
    if (staged) {
      if (n_stage > 0) {
        if (dev_of) {
          PLA_HIP(pla::launch_transpose_rows(ll, dtype, stride_draw, lo, n_stage, S, eng->d_pit.p, s));
        } else if (in_of) {  // the (n_draws, n_stage) slab as it lies, turned on the device
          rc = upload_slab(ll, lo, n_stage, stride_draw, n_draws, esz, eng->d_slab.p, s);
          if (rc) return rc;
          PLA_HIP(pla::launch_transpose_rows(eng->d_slab.p, dtype, n_stage, 0, n_stage, S, eng->d_pit.p, s));
        } else {
          rc = upload_rows(ll, nullptr, lo, n_stage, stride_obs, n_draws, esz, eng->d_pit.p, s);
          if (rc) return rc;
        }
      }
      base = (const char*)eng->d_pit.p;
      blk_so = n_draws;
      row0 = lo;
    }
    // (a row no kernel reads may lie one below the matrix or the staged block: the address is formed, never followed)
    const void* scan_in = base + (top - row0) * blk_so * (int64_t)esz;
    const void* step_in = base + (t_first - row0) * blk_so * (int64_t)esz;
    const char* scan = "";
    PLA_HIP(pla::launch_lfo_bw_ratios(scan_in, dtype, blk_so, S, nq, n_load, last_block, nb > 0, carry, run, eng->d_in.as<double>(), s,
                                      &scan));
    if (nb > 0) {
      p.in = eng->d_in.as<double>() + (size_t)skip * (size_t)n_draws;  // (behind the q that are no step)
      p.n_obs = nb;
      p.diag = d_diag ? d_diag + j0 : nullptr;
      p.lw_out = eng->d_lw.p;
      {
        TimedLaunch t(eng, s);
        PLA_HIP(pla::launch_rows(p, PLA_F64, true, s));
      }
      PLA_HIP(pla::launch_lfo_bw_predict(eng->d_lw.as<const double>(), step_in, dtype, blk_so, nb, S, (int)horizon, j0 == 0, q0 == 0,
                                         d_diag ? d_diag + j0 : nullptr, d_elpd ? d_elpd + j0 : nullptr, d_count, s, route,
                                         (int)sizeof(route)));
      if (j0 == 0)
        label = std::string(dev_of ? "transpose_rows_kernel -> " : "") + scan + " + lfo_carry_kernel -> " + pla::last_rows_kernels() +
                " -> " + route + (host ? " (matrix staged in blocks)" : " per block of steps");
    }
    if (host) PLA_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next block
  }
  eng->last_kernels = label;
  if (d_high) PLA_HIP(pla::launch_lfo_bw_first_high(d_diag, n_steps, q0 == 0 ? 1 : 0, k_threshold, d_high, s));
  if (!host) return PLA_OK;
  rc = out.copy_back({diag, elpd_i});
  if (rc) return rc;
  unsigned long long h_count = 0;
  long long h_high = n_steps;
  PLA_HIP(hipMemcpyAsync(&h_count, d_count, sizeof(h_count), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipMemcpyAsync(&h_high, d_high, sizeof(h_high), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h_count;
  if (first_high) *first_high = (int64_t)h_high;
  return PLA_OK;
}

static int lfo_check(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                     int64_t first, int64_t n_steps, int64_t last_row_margin, int mem_space) {
  // (the engine last: an argument error is reported as such with or without one)
  if (int rc = check_types(dtype, mem_space)) return rc;
  if (n_obs < 1) return fail(PLA_ERR_ARG, "n_obs < 1");
  if (int rc = check_n_draws(n_draws, 2)) return rc;
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
  const bool backward = (method & ~0xFF) == PLA_LFO_BACKWARD;  // (the low byte is the IS method; any other high bit is a bad method)
  if (backward) method &= 0xFF;
  if (method != PLA_PSIS && method != PLA_SIS && method != PLA_TIS) return fail(PLA_ERR_ARG, "bad method");
  if (method != PLA_PSIS) return fail(PLA_ERR_UNSUPPORTED, "method: leave-future-out CV takes PLA_PSIS only");
  if (horizon < 1) return fail(PLA_ERR_ARG, "horizon < 1");
  if (k_threshold != k_threshold) return fail(PLA_ERR_ARG, "k_threshold is NaN");
  if (backward) {  // `first` carries `last`, the observations the fit saw; the steps go down from t_0 = min(last, n_obs - horizon)
    const int64_t last = first;
    int rc = check_types(dtype, mem_space);  // (in the order of lfo_check, the engine last)
    if (rc) return rc;
    if (n_obs < 1) return fail(PLA_ERR_ARG, "n_obs < 1");
    rc = check_n_draws(n_draws, 2);
    if (rc) return rc;
    if (stride_obs <= 0 || stride_draw <= 0) return fail(PLA_ERR_ARG, "strides must be positive");
    if (!ll) return fail(PLA_ERR_ARG, "ll is NULL");
    if (last < 1 || last > n_obs) return fail(PLA_ERR_ARG, "last (passed as first) out of range (1 .. n_obs)");
    if (horizon > n_obs) return fail(PLA_ERR_ARG, "horizon exceeds n_obs");
    const int64_t t0 = last < n_obs - horizon ? last : n_obs - horizon;
    if (n_steps < 1 || n_steps > t0 + 1)
      return fail(PLA_ERR_ARG, "n_steps out of range: 1 .. %lld for n_obs %lld, last %lld, horizon %lld", (long long)(t0 + 1),
                  (long long)n_obs, (long long)last, (long long)horizon);
    if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
    rc = check_common(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, mem_space);
    if (rc) return rc;
    return lfo_bw_impl(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, last, n_steps, horizon, tail_count, k_threshold, mem_space,
                       stream, diag, elpd_i, first_high, n_replaced);
  }
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
  if (int rc0 = check_types(dtype, mem_space)) return rc0;
  if (n_obs < 1) return fail(PLA_ERR_ARG, "n_obs < 1");
  if (int rc0 = check_n_draws(n_draws, 1)) return rc0;
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
  PLA_ENGINE_CALL(eng, stream);
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const size_t row_bytes = (size_t)n_draws * esz;
  const bool staged = host || dev_of;
  const int64_t rows = staged ? staged_chunk_rows(mem_space, true, n_obs, n_draws, esz) : n_obs;
  const int64_t analysed = (split ? 2 * n_chains : n_chains) * n;
  int rc;
  double* ws = nullptr;
  if (analysed > pla::ess_lds_max_draws()) {
    const int64_t slots = pla::ess_grid_for(rows, analysed, eng->ess_grid);
    rc = eng->d_ess.reserve((size_t)slots * (size_t)analysed * sizeof(double));
    if (rc) return rc;
    ws = eng->d_ess.as<double>();
  }
  if (staged) {
    rc = eng->d_in.reserve((size_t)rows * row_bytes);
    if (rc) return rc;
  }
  double* d_out = r_eff;
  unsigned long long* d_count = (unsigned long long*)n_invalid;
  HostOutputs out(eng, s);
  if (host) {
    d_count = eng->counters + pla::kCounterEssInvalid;
    rc = out.reserve(1, n_obs, d_count);
    if (rc) return rc;
    d_out = out.col(0);
  } else if (d_count) {
    PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  }
  char route[96];
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    const void* blk = x;
    int64_t blk_so = stride_obs;
    if (host) {
      rc = stage_rows(eng, x, nullptr, r0, nr, stride_obs, stride_draw, dtype, n_draws, rows, s);
      if (rc) return rc;
    } else if (dev_of) {
      PLA_HIP(pla::launch_transpose_rows(x, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in.p, s));
    }
    if (staged) {
      blk = eng->d_in.p;
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
  return out.finish({r_eff}, n_invalid);
}

}  // extern "C"
