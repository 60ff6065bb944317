// C ABI of libpyloo_amd.so, model-level calls: moment matching, comparison / stacking / bootstrap, non-factorised LOO.
#include "pla_capi.h"
#include "pla_nonfactor.h"

using namespace pla::capi;

extern "C" {

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
  PLA_ENGINE_CALL(eng, stream);
  if (n_batch == 0) return PLA_OK;
  rc = eng->d_mm.reserve((size_t)pla::mm_moments_workspace(n_batch, n_draws, (int)n_dim, want_cov) * sizeof(double));
  if (rc) return rc;
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_mm_moments(upars, lw, n_batch, n_draws, (int)n_dim, want_cov ? 1 : 0, eng->d_mm.as<double>(), stats, cov,
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
  PLA_ENGINE_CALL(eng, stream);
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
  PLA_ENGINE_CALL(eng, stream);
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
  if (int rc0 = check_engine_types(eng, dtype, mem_space)) return rc0;
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
  int rc = eng->d_in.reserve((size_t)K * (size_t)N * esz);
  if (rc) return rc;
  PLA_HIP(hipMemcpy2DAsync(eng->d_in.p, (size_t)N * esz, x, (size_t)(K > 1 ? pitch : N) * esz, (size_t)N * esz, (size_t)K,
                           hipMemcpyHostToDevice, s));
  *dx = eng->d_in.p;
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
  PLA_ENGINE_CALL(eng, stream);
  const int K = (int)n_models;
  const int64_t tiles = pla::compare_n_tiles(n_obs);
  rc = eng->d_cmp.reserve((size_t)tiles * (size_t)(3 * K + 2) * sizeof(double));
  if (rc) return rc;
  double* dout = out;
  if (mem_space == PLA_HOST) {
    rc = eng->d_cmp_out.reserve((size_t)(3 * K + 1) * sizeof(double));
    if (rc) return rc;
    dout = eng->d_cmp_out.as<double>();
  }
  const void* dx = nullptr;
  int64_t dp = 0;
  rc = compare_input_on_device(eng, x, dtype, K, n_obs, pitch, mem_space, s, &dx, &dp);
  if (rc) return rc;
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_compare_moments(dx, dtype, dp, K, n_obs, (int)best, eng->d_cmp.as<double>(), dout, eng->compare_grid, s));
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
  PLA_ENGINE_CALL(eng, stream);
  const int K = (int)n_models;
  const int64_t tiles = pla::compare_n_tiles(n_obs);
  rc = eng->d_cmp.reserve((size_t)tiles * (size_t)(K + 1) * sizeof(double));
  if (rc) return rc;
  rc = eng->d_cmp_out.reserve((size_t)(2 * K + 1) * sizeof(double));  // out [K + 1], then the weights
  if (rc) return rc;
  const void* dx = nullptr;
  int64_t dp = 0;
  rc = compare_input_on_device(eng, x, dtype, K, n_obs, pitch, mem_space, s, &dx, &dp);
  if (rc) return rc;
  double* dw = eng->d_cmp_out.as<double>() + K + 1;
  PLA_HIP(hipMemcpyAsync(dw, weights, (size_t)K * sizeof(double), hipMemcpyHostToDevice, s));
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_stacking_eval(dx, dtype, dp, K, n_obs, scale_mul, dw, eng->d_cmp.as<double>(), eng->d_cmp_out.as<double>(),
                                      eng->compare_grid, s));
  }
  eng->last_kernels = std::string("stacking_eval_kernel<") + pla::dtype_name(dtype) + "> + compare_tiles_sum_kernel " +
                      compare_where(mem_space);
  PLA_HIP(hipMemcpyAsync(out, eng->d_cmp_out.p, (size_t)(K + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
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
  PLA_ENGINE_CALL(eng, stream);
  const int K = (int)n_models;
  const int64_t tiles = pla::compare_n_tiles(n_obs);
  // replicates per launch: their partials within 64 MiB (whole blocks of 64)
  const size_t per_rep = (size_t)tiles * (size_t)(K + 1) * sizeof(double);
  int64_t nb = (int64_t)(((size_t)64 << 20) / per_rep) / 64 * 64;
  if (nb < 64) nb = 64;
  if (nb > n_boot) nb = n_boot;
  rc = eng->d_cmp.reserve((size_t)nb * per_rep);
  if (rc) return rc;
  if (mem_space == PLA_HOST) {
    rc = eng->d_cmp_out.reserve((size_t)nb * (size_t)K * sizeof(double));
    if (rc) return rc;
  }
  const void* dx = nullptr;
  int64_t dp = 0;
  rc = compare_input_on_device(eng, x, dtype, K, n_obs, pitch, mem_space, s, &dx, &dp);
  if (rc) return rc;
  for (int64_t b0 = 0; b0 < n_boot; b0 += nb) {
    const int64_t n = n_boot - b0 < nb ? n_boot - b0 : nb;
    double* zb = mem_space == PLA_DEVICE ? z + b0 * K : eng->d_cmp_out.as<double>();
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_bb_bootstrap(dx, dtype, dp, K, n_obs, scale_mul, seed, alpha, b0, n, eng->d_cmp.as<double>(), zb, eng->compare_grid,
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
  PLA_ENGINE_CALL(eng, stream);
  const size_t bytes = (size_t)n_boot * (size_t)n_obs * sizeof(double);
  double* d = out;
  if (mem_space == PLA_HOST) {
    int rc = eng->d_cmp_out.reserve(bytes);
    if (rc) return rc;
    d = eng->d_cmp_out.as<double>();
  }
  PLA_HIP(pla::launch_bb_gamma_draws(seed, alpha, n_boot, n_obs, d, s));
  eng->last_kernels = "bb_gamma_draws_kernel";
  if (mem_space == PLA_DEVICE) return PLA_OK;
  PLA_HIP(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
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
  if (int rc0 = check_engine_types(eng, dtype, mem_space)) return rc0;
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
  PLA_ENGINE_CALL(eng, stream);
  const int N = (int)n_obs;
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int route = pla::nonfactor_route_for(N, eng->nonfactor_route);
  const int64_t nb = mem_space == PLA_DEVICE ? n_draws : nonfactor_block_draws(n_obs, n_draws, esz);
  const int slots = nonfactor_slots(n_obs, nb, eng->nonfactor_grid);
  int rc = eng->d_nf.reserve((size_t)slots * (size_t)pla::nonfactor_slot_doubles(N) * sizeof(double));
  if (rc) return rc;
  pla::NonfactorParams p{};
  p.N = N;
  p.model = model_type;
  p.ws = eng->d_nf.as<double>();
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
  rc = eng->d_nf_in.reserve(in_elems * esz);
  if (rc) return rc;
  rc = eng->d_nf_out.reserve((size_t)nb * N * sizeof(double) + (size_t)nb * sizeof(int32_t));
  if (rc) return rc;
  char* din = eng->d_nf_in.as<char>();
  void* dmat = din;
  void* dmu = din + (size_t)nb * N * N * esz;
  void* ddf = din + ((size_t)nb * N * N + (size_t)nb * N) * esz;
  void* dy = din + ((size_t)nb * N * N + (size_t)nb * N + (size_t)nb) * esz;
  double* dll = eng->d_nf_out.as<double>();
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
