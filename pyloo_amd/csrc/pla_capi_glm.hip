// C ABI of libpyloo_amd.so, the GLM log-likelihood generator (csrc/pla_glm.h): the matrix from the design matrix, the draws and the
// family -- written out (PLA_GLM_MODE_MATRIX) or consumed block by block by the PSIS-LOO pass (PLA_GLM_MODE_LOO).
// pla_glm_grouped is the same pass with group-level terms added to the linear predictor (csrc/pla_glm_terms.h); the image of the group
// effects, d_glm_u, is its buffer alone.
// Host code only: argument checks, uploads of a PLA_HOST call, kernel launches on the caller's stream.
#include "pla_capi.h"

using namespace pla::capi;

namespace {

// the pointers of one call as the kernels see them: the caller's for PLA_DEVICE, the uploaded copies in d_glm for PLA_HOST
struct GlmInputs {
  const double *x, *beta, *y, *offset, *trials, *obs_const, *sigma, *draw_const;
  const int64_t* rows;
};

// uploads of a host call behind the image of beta in d_glm (sizes in doubles; `at` is advanced)
int glm_upload(const double* src, size_t n, double** at, const double** out, hipStream_t s) {
  *out = nullptr;
  if (!src || n == 0) return PLA_OK;
  PLA_HIP(hipMemcpyAsync(*at, src, n * sizeof(double), hipMemcpyHostToDevice, s));
  *out = *at;
  *at += n;
  return PLA_OK;
}

// pla_glm (n_terms = 0, terms null) and pla_glm_grouped behind their own checks of the block's size
int glm_run(const pla_glm_args* a, int64_t n_terms, const pla_glm_term* terms) {
  pla_engine* eng = a->engine;
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  const int family = a->family, mode = a->mode, mem_space = a->mem_space;
  if (family != PLA_GLM_LINPRED && family != PLA_GLM_GAUSSIAN && family != PLA_GLM_BINOMIAL_LOGIT && family != PLA_GLM_POISSON_LOG)
    return fail(PLA_ERR_ARG, "bad family %d", family);
  if (mode != PLA_GLM_MODE_MATRIX && mode != PLA_GLM_MODE_LOO) return fail(PLA_ERR_ARG, "bad mode %d", mode);
  const bool loo = mode == PLA_GLM_MODE_LOO;
  if (loo && family == PLA_GLM_LINPRED) return fail(PLA_ERR_ARG, "PLA_GLM_MODE_LOO needs a likelihood, not PLA_GLM_LINPRED");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  const int64_t n_obs = a->n_obs, P = a->n_pred, n_draws = a->n_draws;
  if (P < 1 || P > pla::kGlmMaxPred) return fail(PLA_ERR_ARG, "n_pred must lie in [1, %d], got %lld", pla::kGlmMaxPred, (long long)P);
  if (n_obs < 0) return fail(PLA_ERR_ARG, "n_obs < 0");
  if (int rc0 = check_n_draws(n_draws, loo ? 2 : 1)) return rc0;
  if (n_obs > 0 && !a->x) return fail(PLA_ERR_ARG, "x is NULL");
  if (!a->beta) return fail(PLA_ERR_ARG, "beta is NULL");
  if (a->x_stride_obs <= 0 || a->x_stride_pred <= 0) return fail(PLA_ERR_ARG, "x strides must be positive");
  if (a->beta_stride_draw <= 0 || a->beta_stride_pred <= 0) return fail(PLA_ERR_ARG, "beta strides must be positive");
  if (family != PLA_GLM_LINPRED && n_obs > 0 && !a->y) return fail(PLA_ERR_ARG, "y is NULL");
  if (family == PLA_GLM_GAUSSIAN && (!a->draw_scale || !a->draw_const))
    return fail(PLA_ERR_ARG, "PLA_GLM_GAUSSIAN needs draw_scale and draw_const");
  if (loo) {
    if (a->method != PLA_PSIS && a->method != PLA_SIS && a->method != PLA_TIS) return fail(PLA_ERR_ARG, "bad method");
    if (a->method == PLA_PSIS) {
      if (a->tail_count < 1 || a->tail_count + 1 > n_draws)
        return fail(PLA_ERR_ARG, "tail_count %lld needs at least %lld draws, got %lld", (long long)a->tail_count,
                    (long long)a->tail_count + 1, (long long)n_draws);
      if (a->tail_count > pla::max_tail_count())
        return fail(PLA_ERR_UNSUPPORTED, "tail_count %lld exceeds the LDS tail capacity %d", (long long)a->tail_count, pla::max_tail_count());
    }
  }
  int rc;
  if (a->row_index) {
    rc = check_rows(a->row_index, a->n_rows, n_obs, mem_space);
    if (rc) return rc;
  }
  const int64_t m = a->row_index ? a->n_rows : n_obs;  // rows of this call
  const bool host = mem_space == PLA_HOST;
  // ---- the group-level terms
  if (n_terms < 0 || n_terms > PLA_GLM_MAX_TERMS)
    return fail(PLA_ERR_ARG, "n_terms must lie in [0, %d], got %lld", PLA_GLM_MAX_TERMS, (long long)n_terms);
  for (int64_t t = 0; t < n_terms; ++t) {
    const pla_glm_term& k = terms[t];
    if (k.n_groups < 1 || k.n_groups > INT32_MAX)
      return fail(PLA_ERR_ARG, "term %lld: n_groups must lie in [1, 2^31), got %lld", (long long)t, (long long)k.n_groups);
    if (!k.u) return fail(PLA_ERR_ARG, "term %lld: u is NULL", (long long)t);
    if (n_obs > 0 && !k.group_index) return fail(PLA_ERR_ARG, "term %lld: group_index is NULL", (long long)t);
    if (k.u_stride_draw <= 0 || k.u_stride_group <= 0) return fail(PLA_ERR_ARG, "term %lld: u strides must be positive", (long long)t);
    if (!host) continue;
    const bool u_sg = k.u_stride_group == 1 && (n_draws == 1 || k.u_stride_draw == k.n_groups);
    const bool u_gs = k.u_stride_draw == 1 && (k.n_groups == 1 || k.u_stride_group == n_draws);
    if (!u_sg && !u_gs)
      return fail(PLA_ERR_UNSUPPORTED, "term %lld: PLA_HOST u must be dense, (n_draws, n_groups) or (n_groups, n_draws)", (long long)t);
    for (int64_t i = 0; i < n_obs; ++i)
      if (k.group_index[i] < 0 || k.group_index[i] >= k.n_groups)
        return fail(PLA_ERR_ARG, "term %lld: group_index[%lld] = %d is outside [0, %lld)", (long long)t, (long long)i, (int)k.group_index[i],
                    (long long)k.n_groups);
  }
  if (!loo && m > 0 && !a->out) return fail(PLA_ERR_ARG, "out is NULL");
  if (!loo && m > 1 && a->out_pitch < n_draws) return fail(PLA_ERR_ARG, "out_pitch %lld is less than n_draws", (long long)a->out_pitch);
  if (host) {
    const bool x_np = a->x_stride_pred == 1 && (n_obs <= 1 || a->x_stride_obs == P);
    const bool x_pn = a->x_stride_obs == 1 && (P == 1 || a->x_stride_pred == n_obs);
    if (!x_np && !x_pn) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST x must be dense, (n_obs, n_pred) or (n_pred, n_obs)");
    const bool b_sp = a->beta_stride_pred == 1 && (n_draws == 1 || a->beta_stride_draw == P);
    const bool b_ps = a->beta_stride_draw == 1 && (P == 1 || a->beta_stride_pred == n_draws);
    if (!b_sp && !b_ps) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST beta must be dense, (n_draws, n_pred) or (n_pred, n_draws)");
  }
  PLA_ENGINE_CALL(eng, a->stream);
  if (m == 0) {
    if (loo && host && a->n_replaced) *a->n_replaced = 0;
    if (loo && !host && a->n_replaced) PLA_HIP(hipMemsetAsync(a->n_replaced, 0, sizeof(int64_t), s));
    return PLA_OK;
  }
  const int S = (int)n_draws, Pp = (int)P;

  // ---- the image of beta once per call; behind it the inputs of a host call
  int s_pad, p_pad;
  pla::glm_pads(S, Pp, &s_pad, &p_pad);
  const size_t img = (size_t)s_pad * (size_t)p_pad + pla::kGlmImagePad, nx = (size_t)n_obs * (size_t)P, nb = (size_t)n_draws * (size_t)P;
  // (a host row list takes n_rows 8-byte slots like the doubles)
  const size_t up = host ? nx + nb + 4 * (size_t)n_obs + 2 * (size_t)n_draws + (a->row_index ? (size_t)m : 0) : 0;
  rc = eng->d_glm.reserve((img + up) * sizeof(double));
  if (rc) return rc;
  double* bimg = eng->d_glm.as<double>();
  GlmInputs in{a->x, a->beta, a->y, a->offset, a->trials, a->obs_const, a->draw_scale, a->draw_const, a->row_index};
  if (host) {
    double* at = bimg + img;
    if ((rc = glm_upload(a->x, nx, &at, &in.x, s))) return rc;
    if ((rc = glm_upload(a->beta, nb, &at, &in.beta, s))) return rc;
    if ((rc = glm_upload(a->y, (size_t)n_obs, &at, &in.y, s))) return rc;
    if ((rc = glm_upload(a->offset, (size_t)n_obs, &at, &in.offset, s))) return rc;
    if ((rc = glm_upload(a->trials, (size_t)n_obs, &at, &in.trials, s))) return rc;
    if ((rc = glm_upload(a->obs_const, (size_t)n_obs, &at, &in.obs_const, s))) return rc;
    if ((rc = glm_upload(a->draw_scale, (size_t)n_draws, &at, &in.sigma, s))) return rc;
    if ((rc = glm_upload(a->draw_const, (size_t)n_draws, &at, &in.draw_const, s))) return rc;
    if (a->row_index) {
      PLA_HIP(hipMemcpyAsync(at, a->row_index, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, s));
      in.rows = reinterpret_cast<const int64_t*>(at);
    }
  }
  PLA_HIP(pla::launch_glm_prepare(in.beta, a->beta_stride_draw, a->beta_stride_pred, S, Pp, bimg, s));

  // ---- the image of the group effects once per call (d_glm_u); behind it the indices, z and u of a host call
  pla::GlmTerms gt{};
  gt.n_terms = (int)n_terms;
  if (n_terms > 0) {
    size_t up_u = 0;  // in 8-byte slots; an int32 index list takes (n_obs + 1) / 2 of them
    const size_t idx_slots = ((size_t)n_obs + 1) / 2;
    for (int t = 0; t < gt.n_terms; ++t) {
      gt.n_groups[t] = (int)terms[t].n_groups;
      gt.u[t] = terms[t].u;
      gt.u_stride_draw[t] = terms[t].u_stride_draw;
      gt.u_stride_group[t] = terms[t].u_stride_group;
      gt.group[t] = terms[t].group_index;
      gt.z[t] = terms[t].z;
      if (host) up_u += idx_slots + (terms[t].z ? (size_t)n_obs : 0) + (size_t)terms[t].n_groups * (size_t)n_draws;
    }
    const size_t uimg_n = (size_t)pla::glm_terms_image_size(gt, S);
    rc = eng->d_glm_u.reserve((uimg_n + up_u) * sizeof(double));
    if (rc) return rc;
    double* uimg = eng->d_glm_u.as<double>();
    if (host) {
      double* at = uimg + uimg_n;
      for (int t = 0; t < gt.n_terms; ++t) {
        PLA_HIP(hipMemcpyAsync(at, terms[t].group_index, (size_t)n_obs * sizeof(int32_t), hipMemcpyHostToDevice, s));
        gt.group[t] = reinterpret_cast<const int32_t*>(at);
        at += idx_slots;
        if ((rc = glm_upload(terms[t].z, (size_t)n_obs, &at, &gt.z[t], s))) return rc;
        if ((rc = glm_upload(terms[t].u, (size_t)terms[t].n_groups * (size_t)n_draws, &at, &gt.u[t], s))) return rc;
      }
    }
    PLA_HIP(pla::launch_glm_terms_prepare(&gt, S, uimg, s));
  }
  const std::string prepared = n_terms > 0 ? "glm_prepare_kernel -> glm_terms_prepare_kernel -> " : "glm_prepare_kernel -> ";

  pla::GlmLaunch g{};
  g.family = family;
  g.x = in.x;
  g.x_stride_obs = a->x_stride_obs;
  g.x_stride_pred = a->x_stride_pred;
  g.n_src = n_obs;
  g.bimg = bimg;
  g.n_pred = Pp;
  g.n_draws = S;
  g.y = in.y;
  g.offset = in.offset;
  g.trials = family == PLA_GLM_BINOMIAL_LOGIT ? in.trials : nullptr;
  g.obs_const = in.obs_const;
  g.sigma = in.sigma;
  g.draw_const = in.draw_const;
  // rows [r0, r0 + nr) of the call into dst
  const auto block = [&](int64_t r0, int64_t nr, double* dst, int64_t pitch, unsigned long long* count, char* route, int cap) -> int {
    g.row_index = in.rows ? in.rows + r0 : nullptr;
    g.r_first = r0;
    g.n_rows = nr;
    g.out = dst;
    g.pitch = pitch;
    g.replaced = count;
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_glm_terms(g, gt, s, route, cap));
    return PLA_OK;
  };
  char route[160];

  if (!loo) {
    if (!host) {  // written in place
      rc = block(0, m, a->out, m > 1 ? a->out_pitch : n_draws, nullptr, route, (int)sizeof(route));
      if (rc) return rc;
      eng->last_kernels = prepared + route + " (matrix written in place)";
      return PLA_OK;
    }
    const int64_t rows = staged_chunk_rows(mem_space, false, m, n_draws, sizeof(double));
    rc = eng->d_glm_ll.reserve((size_t)rows * (size_t)n_draws * sizeof(double));
    if (rc) return rc;
    const size_t row_bytes = (size_t)n_draws * sizeof(double), pitch_bytes = (size_t)(m > 1 ? a->out_pitch : n_draws) * sizeof(double);
    for (int64_t r0 = 0; r0 < m; r0 += rows) {
      const int64_t nr = m - r0 < rows ? m - r0 : rows;
      rc = block(r0, nr, eng->d_glm_ll.as<double>(), n_draws, nullptr, route, (int)sizeof(route));
      if (rc) return rc;
      PLA_HIP(hipMemcpy2DAsync((char*)a->out + (size_t)r0 * pitch_bytes, pitch_bytes, eng->d_glm_ll.p, row_bytes, row_bytes, (size_t)nr,
                               hipMemcpyDeviceToHost, s));
      PLA_HIP(hipStreamSynchronize(s));  // the block buffer is reused by the next block
    }
    eng->last_kernels = prepared + route + " (matrix copied back in blocks)";
    return PLA_OK;
  }

  // ---- PLA_GLM_MODE_LOO: per block of rows the kernel into d_glm_ll, then the LOO pass on the block as on a resident
  // (rows, n_draws) f64 matrix (pitch n_draws: the route such a tensor takes)
  unsigned long long* d_count = nullptr;
  double *dd = a->diag, *dl = a->loo_i, *dp = a->lppd_i;
  HostOutputs out(eng, s);
  if (host) {
    d_count = eng->counters + pla::kCounterGlmReplaced;
    rc = out.reserve(3, m, d_count);
    if (rc) return rc;
    dd = out.col(0);
    dl = out.col(1);
    dp = out.col(2);
  } else {
    if (a->agg && (!dd || !dl || !dp)) {
      rc = out.reserve(3, m);
      if (rc) return rc;
      if (!dd) dd = out.col(0);
      if (!dl) dl = out.col(1);
      if (!dp) dp = out.col(2);
    }
    d_count = (unsigned long long*)a->n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
    else {  // (the kernel replaces NaN only with a counter to count into)
      d_count = eng->counters + pla::kCounterGlmReplaced;
      PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
    }
  }
  const int64_t rows = staged_chunk_rows(PLA_DEVICE, true, m, n_draws, sizeof(double));
  rc = eng->d_glm_ll.reserve((size_t)rows * (size_t)n_draws * sizeof(double));
  if (rc) return rc;
  std::string label;
  for (int64_t r0 = 0; r0 < m; r0 += rows) {
    const int64_t nr = m - r0 < rows ? m - r0 : rows;
    rc = block(r0, nr, eng->d_glm_ll.as<double>(), n_draws, d_count, route, (int)sizeof(route));
    if (rc) return rc;
    rc = psis_loo_run(eng, eng->d_glm_ll.p, PLA_F64, nr, nullptr, nr, n_draws, n_draws, 1, a->method, a->tail_count, a->scale_value,
                      a->good_k, PLA_DEVICE, a->stream, dd ? dd + r0 : nullptr, dl ? dl + r0 : nullptr, dp ? dp + r0 : nullptr, nullptr);
    if (rc) return rc;
    if (r0 == 0) label = prepared + route + " -> " + eng->last_kernels + " per block of observations";
  }
  eng->last_kernels = label;
  // the aggregates once, over all rows, from the pointwise vectors
  double* dagg = host ? out.col(3) : a->agg;
  if (a->agg) {
    pla::ReduceParams rp{dd, dl, dp, m, a->good_k, dagg, nullptr};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
  }
  if (!host) return PLA_OK;
  rc = out.copy_back({a->diag, a->loo_i, a->lppd_i});
  if (rc) return rc;
  if (a->agg) PLA_HIP(hipMemcpyAsync(a->agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  unsigned long long h = 0;
  PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (a->n_replaced) *a->n_replaced = (int64_t)h;
  return PLA_OK;
}

}  // namespace

extern "C" {

int pla_glm(const pla_glm_args* a) {
  if (!a) return fail(PLA_ERR_ARG, "args is NULL");
  if (a->struct_size != (int64_t)sizeof(pla_glm_args))
    return fail(PLA_ERR_ARG, "struct_size is %lld, pla_glm_args of this library has %lld bytes", (long long)a->struct_size,
                (long long)sizeof(pla_glm_args));
  return glm_run(a, 0, nullptr);
}

int pla_glm_grouped(const pla_glm_grouped_args* a) {
  if (!a) return fail(PLA_ERR_ARG, "args is NULL");
  if (a->struct_size != (int64_t)sizeof(pla_glm_grouped_args))
    return fail(PLA_ERR_ARG, "struct_size is %lld, pla_glm_grouped_args of this library has %lld bytes", (long long)a->struct_size,
                (long long)sizeof(pla_glm_grouped_args));
  if (a->glm.struct_size != (int64_t)sizeof(pla_glm_args))
    return fail(PLA_ERR_ARG, "glm.struct_size is %lld, pla_glm_args of this library has %lld bytes", (long long)a->glm.struct_size,
                (long long)sizeof(pla_glm_args));
  return glm_run(&a->glm, a->n_terms, a->terms);
}

}  // extern "C"
