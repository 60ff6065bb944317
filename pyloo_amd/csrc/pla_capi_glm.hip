// C ABI of libpyloo_amd.so, the GLM log-likelihood generator (csrc/pla_glm.h): the matrix from the design matrix, the draws and the
// family -- written out (PLA_GLM_MODE_MATRIX) or consumed block by block by the PSIS-LOO pass (PLA_GLM_MODE_LOO).
// pla_glm_grouped is the same pass with group-level terms added to the linear predictor (csrc/pla_glm_terms.h); the image of the group
// effects, d_glm_u, is its buffer alone.
// pla_glm_marginal integrates one effect per cluster out of the likelihood (csrc/pla_glm_marginal.h): the generator writes the linear
// predictor of a block of members, the marginal kernels turn it into rows of the (n_clusters, n_draws) matrix; the segment tables,
// the partial sums and the carry, d_glm_marg, and the block of finished clusters, d_glm_mll, are its buffers alone.
// pla_glm_predict contracts the generator's tile against a block of leave-one-out weights instead of storing it
// (csrc/pla_glm_predict.h): the predictive moments and PIT; the row maxima and the partial sums, d_glm_pred, are its buffer alone.
// Host code only: argument checks, uploads of a PLA_HOST call, kernel launches on the caller's stream.
#include "pla_capi.h"
#include "pla_glm_marginal.h"

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

// what glm_prepare leaves for the launches of one call
struct GlmSetup {
  GlmInputs in;
  pla::GlmLaunch g;
  pla::GlmTerms gt;
  std::string prepared;
};

// the argument checks of pla_glm, pla_glm_grouped and pla_glm_marginal; row_index / n_rows: the row list of the call (the block's
// own for the first two, the member list for the third)
// m_out: the rows of the output (one per row of the call; one per cluster for the third)
int glm_check(const pla_glm_args* a, int64_t n_terms, const pla_glm_term* terms, const int64_t* row_index, int64_t n_rows, int64_t m_out) {
  pla_engine* eng = a->engine;
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  const int family = a->family, mode = a->mode, mem_space = a->mem_space;
  if (family < PLA_GLM_LINPRED || family > PLA_GLM_BINOMIAL_PROBIT) return fail(PLA_ERR_ARG, "bad family %d", family);
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
  if (family == PLA_GLM_NEGBINOMIAL_LOG || family == PLA_GLM_GAMMA_LOG) {
    const char* name = family == PLA_GLM_GAMMA_LOG ? "PLA_GLM_GAMMA_LOG" : "PLA_GLM_NEGBINOMIAL_LOG";
    const char* what = family == PLA_GLM_GAMMA_LOG ? "the shape alpha" : "the dispersion phi";
    if (!a->draw_scale) return fail(PLA_ERR_ARG, "%s needs draw_scale, %s per draw", name, what);
    if (!a->draw_const) return fail(PLA_ERR_ARG, "%s needs draw_const, a log(a) - lgamma(a) of draw_scale per draw", name);
  }
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
  if (row_index) {
    rc = check_rows(row_index, n_rows, n_obs, mem_space);
    if (rc) return rc;
  }
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
  if (!loo && m_out > 0 && !a->out) return fail(PLA_ERR_ARG, "out is NULL");
  if (!loo && m_out > 1 && a->out_pitch < n_draws) return fail(PLA_ERR_ARG, "out_pitch %lld is less than n_draws", (long long)a->out_pitch);
  if (host) {
    const bool x_np = a->x_stride_pred == 1 && (n_obs <= 1 || a->x_stride_obs == P);
    const bool x_pn = a->x_stride_obs == 1 && (P == 1 || a->x_stride_pred == n_obs);
    if (!x_np && !x_pn) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST x must be dense, (n_obs, n_pred) or (n_pred, n_obs)");
    const bool b_sp = a->beta_stride_pred == 1 && (n_draws == 1 || a->beta_stride_draw == P);
    const bool b_ps = a->beta_stride_draw == 1 && (P == 1 || a->beta_stride_pred == n_draws);
    if (!b_sp && !b_ps) return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST beta must be dense, (n_draws, n_pred) or (n_pred, n_draws)");
  }
  return PLA_OK;
}

// a call without rows: the counter alone
int glm_nothing(const pla_glm_args* a, hipStream_t s) {
  const bool loo = a->mode == PLA_GLM_MODE_LOO, host = a->mem_space == PLA_HOST;
  if (loo && host && a->n_replaced) *a->n_replaced = 0;
  if (loo && !host && a->n_replaced) PLA_HIP(hipMemsetAsync(a->n_replaced, 0, sizeof(int64_t), s));
  return PLA_OK;
}

// the images of beta and of the group effects, once per call, and the uploads of a host call behind them: the generator's launch
// block with everything but the rows of a launch.  `family`: what the generator writes (pla_glm_marginal: the linear predictor).
int glm_prepare(const pla_glm_args* a, int family, int64_t n_terms, const pla_glm_term* terms, const int64_t* row_index, int64_t m,
                hipStream_t s, GlmSetup* out) {
  pla_engine* eng = a->engine;
  const bool host = a->mem_space == PLA_HOST;
  const int64_t n_obs = a->n_obs, P = a->n_pred, n_draws = a->n_draws;
  int rc;
  const int S = (int)n_draws, Pp = (int)P;

  // ---- the image of beta once per call; behind it the inputs of a host call
  int s_pad, p_pad;
  pla::glm_pads(S, Pp, &s_pad, &p_pad);
  const size_t img = (size_t)s_pad * (size_t)p_pad + pla::kGlmImagePad, nx = (size_t)n_obs * (size_t)P, nb = (size_t)n_draws * (size_t)P;
  // (a host row list takes n_rows 8-byte slots like the doubles)
  const size_t up = host ? nx + nb + 4 * (size_t)n_obs + 2 * (size_t)n_draws + (row_index ? (size_t)m : 0) : 0;
  rc = eng->d_glm.reserve((img + up) * sizeof(double));
  if (rc) return rc;
  double* bimg = eng->d_glm.as<double>();
  GlmInputs& in = out->in;
  in = GlmInputs{a->x, a->beta, a->y, a->offset, a->trials, a->obs_const, a->draw_scale, a->draw_const, row_index};
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
    if (row_index && m > 0) {
      PLA_HIP(hipMemcpyAsync(at, row_index, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, s));
      in.rows = reinterpret_cast<const int64_t*>(at);
    }
  }
  PLA_HIP(pla::launch_glm_prepare(in.beta, a->beta_stride_draw, a->beta_stride_pred, S, Pp, bimg, s));

  // ---- the image of the group effects once per call (d_glm_u); behind it the indices, z and u of a host call
  pla::GlmTerms& gt = out->gt;
  gt = pla::GlmTerms{};
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
  out->prepared = n_terms > 0 ? "glm_prepare_kernel -> glm_terms_prepare_kernel -> " : "glm_prepare_kernel -> ";

  pla::GlmLaunch& g = out->g;
  g = pla::GlmLaunch{};
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
  g.trials = family == PLA_GLM_BINOMIAL_LOGIT || family == PLA_GLM_BINOMIAL_PROBIT ? in.trials : nullptr;
  g.obs_const = in.obs_const;
  g.sigma = in.sigma;
  g.draw_const = in.draw_const;
  return PLA_OK;
}

// pla_glm (n_terms = 0, terms null) and pla_glm_grouped behind their own checks of the block's size
int glm_run(const pla_glm_args* a, int64_t n_terms, const pla_glm_term* terms) {
  int rc = glm_check(a, n_terms, terms, a->row_index, a->n_rows, a->row_index ? a->n_rows : a->n_obs);
  if (rc) return rc;
  pla_engine* eng = a->engine;
  const int mem_space = a->mem_space;
  const bool loo = a->mode == PLA_GLM_MODE_LOO, host = mem_space == PLA_HOST;
  const int64_t n_obs = a->n_obs, n_draws = a->n_draws;
  const int64_t m = a->row_index ? a->n_rows : n_obs;  // rows of this call
  PLA_ENGINE_CALL(eng, a->stream);
  if (m == 0) return glm_nothing(a, s);
  GlmSetup su;
  if ((rc = glm_prepare(a, a->family, n_terms, terms, a->row_index, m, s, &su))) return rc;
  const GlmInputs& in = su.in;
  pla::GlmLaunch& g = su.g;
  const pla::GlmTerms& gt = su.gt;
  const std::string& prepared = su.prepared;
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

// ---- pla_glm_marginal ------------------------------------------------------------------------------------------------------------
// One launch of the call: members [r0, r0 + nr) through the generator, its segments and joins through the marginal kernels, the
// clusters [c0, c0 + nc) finished by it.
struct MargBlock {
  int64_t r0, nr, seg0, n_segs, join0, n_joins, c0, nc;
};

// The blocks of a call, cut at segment boundaries, and their tables.  lo / hi: the member range of every cluster, clamped.  A block
// holds whole clusters -- at most max_clusters of them, spanning at most max_rows members -- or, for a cluster longer than that,
// a run of its segments alone; the sums of such a cluster travel from block to block in the carry.
void marg_plan(const std::vector<int64_t>& lo, const std::vector<int64_t>& hi, int64_t max_rows, int64_t max_clusters,
               std::vector<MargBlock>* blocks, std::vector<pla::GlmMargSeg>* segs, std::vector<pla::GlmMargJoin>* joins, int64_t* max_slots) {
  const int64_t L = pla::kGlmMargSeg, C = (int64_t)lo.size();
  *max_slots = 0;
  int64_t c = 0;
  while (c < C) {
    const int64_t len = hi[c] - lo[c];
    if (len > max_rows) {  // segments [k0, k1) of one cluster per block
      const int64_t n_seg = (len + L - 1) / L, per = max_rows / L;
      for (int64_t k0 = 0; k0 < n_seg; k0 += per) {
        const int64_t k1 = k0 + per < n_seg ? k0 + per : n_seg;
        MargBlock b{lo[c] + k0 * L, 0, (int64_t)segs->size(), k1 - k0, (int64_t)joins->size(), 1, c, k1 == n_seg ? 1 : 0};
        b.nr = (lo[c] + k1 * L < hi[c] ? lo[c] + k1 * L : hi[c]) - b.r0;
        for (int64_t k = k0; k < k1; ++k) {
          const int64_t first = (k - k0) * L;
          segs->push_back(pla::GlmMargSeg{c, first, (int32_t)(b.nr - first < L ? b.nr - first : L), (int32_t)(k - k0)});
        }
        joins->push_back(pla::GlmMargJoin{c, 0, (int32_t)(k1 - k0), k0 > 0 ? 1 : 0, k1 == n_seg ? 1 : 0});
        if (k1 - k0 > *max_slots) *max_slots = k1 - k0;
        blocks->push_back(b);
      }
      c += 1;
      continue;
    }
    int64_t n = 0, blo = 0, bhi = 0;
    bool any = false;
    while (c + n < C && n < max_clusters) {
      const int64_t l = lo[c + n], h = hi[c + n];
      if (h - l > max_rows) break;
      if (h > l) {
        const int64_t nlo = any && blo < l ? blo : l, nhi = any && bhi > h ? bhi : h;
        if (nhi - nlo > max_rows) break;
        blo = nlo;
        bhi = nhi;
        any = true;
      }
      n += 1;
    }
    MargBlock b{blo, bhi - blo, (int64_t)segs->size(), 0, (int64_t)joins->size(), 0, c, n};
    int64_t slots = 0;
    for (int64_t j = c; j < c + n; ++j) {
      const int64_t l = lo[j], ln = hi[j] - lo[j], n_seg = (ln + L - 1) / L;
      if (n_seg <= 1) {
        segs->push_back(pla::GlmMargSeg{j, ln > 0 ? l - blo : 0, (int32_t)ln, -1});
        continue;
      }
      joins->push_back(pla::GlmMargJoin{j, (int32_t)slots, (int32_t)n_seg, 0, 1});
      for (int64_t k = 0; k < n_seg; ++k)
        segs->push_back(pla::GlmMargSeg{j, l - blo + k * L, (int32_t)(ln - k * L < L ? ln - k * L : L), (int32_t)slots++});
    }
    b.n_segs = (int64_t)segs->size() - b.seg0;
    b.n_joins = (int64_t)joins->size() - b.join0;
    if (slots > *max_slots) *max_slots = slots;
    blocks->push_back(b);
    c += n;
  }
}

int marg_run(const pla_glm_marginal_args* a) {
  const pla_glm_args* ga = &a->grouped.glm;
  if (ga->family == PLA_GLM_NEGBINOMIAL_LOG || ga->family == PLA_GLM_GAMMA_LOG || ga->family == PLA_GLM_BINOMIAL_PROBIT)
    return fail(PLA_ERR_ARG, "pla_glm_marginal takes PLA_GLM_GAUSSIAN, PLA_GLM_BINOMIAL_LOGIT and PLA_GLM_POISSON_LOG, not %s",
                ga->family == PLA_GLM_NEGBINOMIAL_LOG ? "PLA_GLM_NEGBINOMIAL_LOG" : ga->family == PLA_GLM_GAMMA_LOG ? "PLA_GLM_GAMMA_LOG"
                                                                                                                  : "PLA_GLM_BINOMIAL_PROBIT");
  int rc = glm_check(ga, a->grouped.n_terms, a->grouped.terms, nullptr, 0, a->n_clusters);
  if (rc) return rc;
  pla_engine* eng = ga->engine;
  const bool loo = ga->mode == PLA_GLM_MODE_LOO, host = ga->mem_space == PLA_HOST;
  const int64_t n_obs = ga->n_obs, n_draws = ga->n_draws, C = a->n_clusters, Q = a->n_nodes, NM = a->n_members;
  if (ga->family == PLA_GLM_LINPRED) return fail(PLA_ERR_ARG, "pla_glm_marginal needs a likelihood, not PLA_GLM_LINPRED");
  if (ga->row_index) return fail(PLA_ERR_ARG, "glm.row_index must be NULL: the member list is the row list");
  if (C < 0) return fail(PLA_ERR_ARG, "n_clusters < 0");
  if (NM < 0) return fail(PLA_ERR_ARG, "n_members < 0");
  if (Q < 1 || Q > pla::kGlmMargMaxNodes)
    return fail(PLA_ERR_ARG, "n_nodes must lie in [1, %d], got %lld", pla::kGlmMargMaxNodes, (long long)Q);
  if (!a->cluster_offsets) return fail(PLA_ERR_ARG, "cluster_offsets is NULL");
  if (NM > 0 && !a->members) return fail(PLA_ERR_ARG, "members is NULL");
  if (NM > 0 && n_obs < 1) return fail(PLA_ERR_ARG, "members without observations");
  if (!a->tau) return fail(PLA_ERR_ARG, "tau is NULL");
  if (C > 0 && (!a->nodes || !a->log_weights)) return fail(PLA_ERR_ARG, "nodes or log_weights is NULL");
  if (host) {
    const int64_t* off = a->cluster_offsets;
    if (off[0] != 0) return fail(PLA_ERR_ARG, "cluster_offsets[0] must be 0, got %lld", (long long)off[0]);
    for (int64_t c = 0; c < C; ++c)
      if (off[c + 1] < off[c]) return fail(PLA_ERR_ARG, "cluster_offsets decrease at cluster %lld", (long long)c);
    if (off[C] != NM) return fail(PLA_ERR_ARG, "cluster_offsets end at %lld, n_members is %lld", (long long)off[C], (long long)NM);
    for (int64_t j = 0; j < NM; ++j)
      if (a->members[j] < 0 || a->members[j] >= n_obs)
        return fail(PLA_ERR_ARG, "members[%lld] = %lld is outside [0, %lld)", (long long)j, (long long)a->members[j], (long long)n_obs);
    for (int64_t t = 0; t < n_draws; ++t)
      if (!(a->tau[t] > 0.0) || !std::isfinite(a->tau[t]))
        return fail(PLA_ERR_ARG, "tau[%lld] = %g is not positive and finite", (long long)t, a->tau[t]);
  }
  PLA_ENGINE_CALL(eng, ga->stream);
  if (!host) {  // the call waits for the stream: not inside a capture
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &capture) != hipSuccess) (void)hipGetLastError();
    else if (capture != hipStreamCaptureStatusNone)
      return fail(PLA_ERR_UNSUPPORTED, "pla_glm_marginal waits for the cluster offsets and cannot be captured in a graph");
  }
  if (C == 0) return glm_nothing(ga, s);
  const int S = (int)n_draws, cap = pla::glm_marginal_capacity((int)Q);

  // ---- the member range of every cluster: a pair of offsets that is out of range or decreasing is an empty cluster.  A device
  // list comes to the host for this (the one wait of a PLA_DEVICE call): the blocks are cut where the clusters end
  std::vector<int64_t> lo((size_t)C), hi((size_t)C);
  {
    std::vector<int64_t> copy;
    const int64_t* off = a->cluster_offsets;
    if (!host) {
      copy.resize((size_t)C + 1);
      PLA_HIP(hipMemcpyAsync(copy.data(), a->cluster_offsets, (size_t)(C + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
      PLA_HIP(hipStreamSynchronize(s));
      off = copy.data();
    }
    for (int64_t c = 0; c < C; ++c) {
      const bool ok = off[c] >= 0 && off[c] <= off[c + 1] && off[c + 1] <= NM;
      lo[(size_t)c] = ok ? off[c] : 0;
      hi[(size_t)c] = ok ? off[c + 1] : 0;
    }
  }
  const int64_t L = pla::kGlmMargSeg;
  int64_t max_rows = staged_chunk_rows(PLA_DEVICE, true, NM > L ? NM : L, n_draws, sizeof(double));
  if (max_rows < NM) max_rows = max_rows / L * L;  // (blocks are cut at segment boundaries)
  if (max_rows < L) max_rows = L;
  const bool in_place = !loo && !host;  // the matrix into the caller's device buffer
  const int64_t max_clusters = in_place ? C : staged_chunk_rows(PLA_DEVICE, true, C, n_draws, sizeof(double));
  std::vector<MargBlock> blocks;
  std::vector<pla::GlmMargSeg> segs;
  std::vector<pla::GlmMargJoin> joins;
  struct WaitOnExit {  // (declared behind the tables: on an early return their queued copies end before they do)
    hipStream_t s;
    bool armed;
    ~WaitOnExit() {
      if (armed) (void)hipStreamSynchronize(s);
    }
  } tables_in_flight{s, false};
  int64_t max_slots = 0, block_rows = 1, block_clusters = 1;
  marg_plan(lo, hi, max_rows, max_clusters, &blocks, &segs, &joins, &max_slots);
  for (const MargBlock& b : blocks) {
    if (b.nr > block_rows) block_rows = b.nr;
    if (b.nc > block_clusters) block_clusters = b.nc;
  }

  GlmSetup su;
  if ((rc = glm_prepare(ga, PLA_GLM_LINPRED, a->grouped.n_terms, a->grouped.terms, a->members, NM, s, &su))) return rc;
  const int64_t* d_members = su.in.rows;

  // ---- d_glm_marg: the tables, the carry, the partial sums; behind them z, tau, nodes and log_weights of a host call
  const size_t seg_bytes = segs.size() * sizeof(pla::GlmMargSeg), join_bytes = joins.size() * sizeof(pla::GlmMargJoin);
  const size_t carry_n = joins.empty() ? 0 : (size_t)cap * (size_t)S, part_n = (size_t)max_slots * (size_t)cap * (size_t)S;
  const size_t up_n = host ? (a->z ? (size_t)n_obs : 0) + (size_t)n_draws + 2 * (size_t)C * (size_t)Q : 0;
  rc = eng->d_glm_marg.reserve(seg_bytes + join_bytes + (carry_n + part_n + up_n) * sizeof(double));
  if (rc) return rc;
  char* base = eng->d_glm_marg.as<char>();
  tables_in_flight.armed = true;
  PLA_HIP(hipMemcpyAsync(base, segs.data(), seg_bytes, hipMemcpyHostToDevice, s));
  if (join_bytes) PLA_HIP(hipMemcpyAsync(base + seg_bytes, joins.data(), join_bytes, hipMemcpyHostToDevice, s));
  double* carry = reinterpret_cast<double*>(base + seg_bytes + join_bytes);
  pla::GlmMargParams mp{};
  mp.z = a->z;
  mp.tau = a->tau;
  mp.nodes = a->nodes;
  mp.logw = a->log_weights;
  if (host) {
    double* at = carry + carry_n + part_n;
    if ((rc = glm_upload(a->z, (size_t)n_obs, &at, &mp.z, s))) return rc;
    if ((rc = glm_upload(a->tau, (size_t)n_draws, &at, &mp.tau, s))) return rc;
    if ((rc = glm_upload(a->nodes, (size_t)C * (size_t)Q, &at, &mp.nodes, s))) return rc;
    if ((rc = glm_upload(a->log_weights, (size_t)C * (size_t)Q, &at, &mp.logw, s))) return rc;
  }
  PLA_HIP(hipStreamSynchronize(s));  // (the tables are this call's own host memory)
  tables_in_flight.armed = false;
  mp.n_src = n_obs;
  mp.y = su.in.y;
  mp.trials = ga->family == PLA_GLM_BINOMIAL_LOGIT ? su.in.trials : nullptr;
  mp.obs_const = su.in.obs_const;
  mp.sigma = su.in.sigma;
  mp.draw_const = su.in.draw_const;
  mp.n_nodes = (int)Q;
  mp.n_draws = S;
  mp.carry = carry;
  mp.part = carry + carry_n;

  // ---- the outputs, as glm_run sets them up; one row per cluster
  unsigned long long* d_count = nullptr;
  double *dd = ga->diag, *dl = ga->loo_i, *dp = ga->lppd_i;
  HostOutputs out(eng, s);
  if (loo) {
    if (host) {
      d_count = eng->counters + pla::kCounterGlmReplaced;
      rc = out.reserve(3, C, d_count);
      if (rc) return rc;
      dd = out.col(0);
      dl = out.col(1);
      dp = out.col(2);
    } else {
      if (ga->agg && (!dd || !dl || !dp)) {
        rc = out.reserve(3, C);
        if (rc) return rc;
        if (!dd) dd = out.col(0);
        if (!dl) dl = out.col(1);
        if (!dp) dp = out.col(2);
      }
      d_count = (unsigned long long*)ga->n_replaced;
      if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
      else {
        d_count = eng->counters + pla::kCounterGlmReplaced;
        PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
      }
    }
  }
  rc = eng->d_glm_ll.reserve((size_t)block_rows * (size_t)n_draws * sizeof(double));
  if (rc) return rc;
  if (!in_place) {
    rc = eng->d_glm_mll.reserve((size_t)block_clusters * (size_t)n_draws * sizeof(double));
    if (rc) return rc;
  }
  const size_t row_bytes = (size_t)n_draws * sizeof(double), pitch_bytes = (size_t)(C > 1 ? ga->out_pitch : n_draws) * sizeof(double);
  pla::GlmLaunch& g = su.g;
  char route[160], mroute[160];
  std::string gen_label, marg_label, loo_label;  // the generator's route, the marginal kernels' (with the join kernel, if any block has one)
  for (const MargBlock& b : blocks) {
    if (b.nr > 0) {  // the linear predictor of the block's members
      g.row_index = d_members + b.r0;
      g.r_first = b.r0;
      g.n_rows = b.nr;
      g.out = eng->d_glm_ll.as<double>();
      g.pitch = n_draws;
      g.replaced = nullptr;
      PLA_HIP(pla::launch_glm_terms(g, su.gt, s, route, (int)sizeof(route)));
    }
    mp.rest = eng->d_glm_ll.as<double>();
    mp.n_rows = b.nr;
    mp.members = d_members + b.r0;
    mp.segs = reinterpret_cast<const pla::GlmMargSeg*>(base) + b.seg0;
    mp.n_segs = b.n_segs;
    mp.joins = reinterpret_cast<const pla::GlmMargJoin*>(base + seg_bytes) + b.join0;
    mp.n_joins = b.n_joins;
    mp.out = in_place ? ga->out : eng->d_glm_mll.as<double>();
    mp.out_first = in_place ? 0 : b.c0;
    mp.out_pitch = in_place ? (C > 1 ? ga->out_pitch : n_draws) : n_draws;
    mp.replaced = loo ? d_count : nullptr;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_glm_marginal(ga->family, mp, s, mroute, (int)sizeof(mroute)));
    }
    if (gen_label.empty() && b.nr > 0) gen_label = su.prepared + route + " -> ";
    if (marg_label.empty() || (b.n_joins > 0 && marg_label.find("join") == std::string::npos)) marg_label = mroute;
    if (b.nc == 0 || in_place) continue;
    if (!loo) {
      PLA_HIP(hipMemcpy2DAsync((char*)ga->out + (size_t)b.c0 * pitch_bytes, pitch_bytes, eng->d_glm_mll.p, row_bytes, row_bytes, (size_t)b.nc,
                               hipMemcpyDeviceToHost, s));
      PLA_HIP(hipStreamSynchronize(s));  // the block buffer is reused by the next block
      continue;
    }
    rc = psis_loo_run(eng, eng->d_glm_mll.p, PLA_F64, b.nc, nullptr, b.nc, n_draws, n_draws, 1, ga->method, ga->tail_count, ga->scale_value,
                      ga->good_k, PLA_DEVICE, ga->stream, dd ? dd + b.c0 : nullptr, dl ? dl + b.c0 : nullptr, dp ? dp + b.c0 : nullptr,
                      nullptr);
    if (rc) return rc;
    if (loo_label.empty()) loo_label = " -> " + eng->last_kernels + " per block of clusters";
  }
  eng->last_kernels = gen_label + marg_label + (loo ? loo_label.c_str() : in_place ? " (matrix written in place)" : " (matrix copied back in blocks)") +
                      "; blocks of members: " + std::to_string(blocks.size());
  if (!loo) return PLA_OK;
  double* dagg = host ? out.col(3) : ga->agg;
  if (ga->agg) {
    pla::ReduceParams rp{dd, dl, dp, C, ga->good_k, dagg, nullptr};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
  }
  if (!host) return PLA_OK;
  rc = out.copy_back({ga->diag, ga->loo_i, ga->lppd_i});
  if (rc) return rc;
  if (ga->agg) PLA_HIP(hipMemcpyAsync(ga->agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  unsigned long long h = 0;
  PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (ga->n_replaced) *ga->n_replaced = (int64_t)h;
  return PLA_OK;
}

// ---- pla_glm_predict -------------------------------------------------------------------------------------------------------------
// PLA_PIT_LOGLIK: per block of rows the generator into d_glm_ll, then pla_loo_diag's pipeline on the block as on a resident matrix
// (-ll into d_in, the weights pass into d_lw, diag_wave_kernel for elpd_i), then the predictive kernel on d_lw before the next block
// overwrites anything.  PLA_PIT_LOG_WEIGHTS: the predictive kernel alone, on the caller's device weights in place or on blocks of
// host weights staged in d_lw.  Outputs of a host call in d_pw.
int predict_run(const pla_glm_predict_args* a) {
  const bool loglik = a->kind == PLA_PIT_LOGLIK;
  if (!loglik && a->kind != PLA_PIT_LOG_WEIGHTS) return fail(PLA_ERR_ARG, "bad kind %lld", (long long)a->kind);
  if (a->glm.family == PLA_GLM_LINPRED) return fail(PLA_ERR_ARG, "pla_glm_predict needs a likelihood, not PLA_GLM_LINPRED");
  pla_glm_args ga = a->glm;  // as glm_check reads a fused pass: at least two draws; the weights' method and tail count for PLA_PIT_LOGLIK
  ga.mode = PLA_GLM_MODE_LOO;
  if (!loglik) ga.method = PLA_SIS;
  const int64_t m = ga.row_index ? ga.n_rows : ga.n_obs;  // rows of this call
  int rc = glm_check(&ga, 0, nullptr, ga.row_index, ga.n_rows, m);
  if (rc) return rc;
  const bool want_pit = a->pit_le || a->pit_lt;
  if (ga.family == PLA_GLM_GAMMA_LOG && want_pit)
    return fail(PLA_ERR_UNSUPPORTED, "PLA_GLM_GAMMA_LOG has no distribution function here: pit_le and pit_lt must be NULL");
  if (!loglik) {
    if (m > 0 && !a->log_weights) return fail(PLA_ERR_ARG, "log_weights is NULL");
    if (a->lw_stride_obs <= 0 || a->lw_stride_draw <= 0) return fail(PLA_ERR_ARG, "log_weights strides must be positive");
    if (a->lw_stride_draw != 1) return fail(PLA_ERR_UNSUPPORTED, "log_weights need unit stride along the draws");
    if (m > 1 && a->lw_stride_obs < ga.n_draws) return fail(PLA_ERR_ARG, "lw_stride_obs %lld is less than n_draws", (long long)a->lw_stride_obs);
  }
  pla_engine* eng = ga.engine;
  const bool host = ga.mem_space == PLA_HOST;
  const int64_t n_draws = ga.n_draws;
  const int S = (int)n_draws;
  PLA_ENGINE_CALL(eng, ga.stream);
  if (m == 0) {
    for (int64_t* c : {a->n_replaced, a->n_pit_skipped}) {
      if (host && c) *c = 0;
      if (!host && c) PLA_HIP(hipMemsetAsync(c, 0, sizeof(int64_t), s));
    }
    return PLA_OK;
  }
  GlmSetup su;
  if ((rc = glm_prepare(&ga, ga.family, 0, nullptr, ga.row_index, m, s, &su))) return rc;
  pla::GlmLaunch& g = su.g;

  // ---- the rows of a block, and for PLA_PIT_LOGLIK its weights pass as pla_importance_weights sets it up
  pla::RowsParams p{};
  int64_t rows = staged_chunk_rows(loglik ? PLA_DEVICE : ga.mem_space, true, m, n_draws, sizeof(double));
  const size_t block_bytes = (size_t)rows * (size_t)n_draws * sizeof(double);
  if (loglik) {
    rc = weights_block_setup(eng, ga.method, ga.tail_count, n_draws, sizeof(double), s, &rows, &p);
    if (!rc) rc = eng->d_glm_ll.reserve(block_bytes);
    if (!rc) rc = eng->d_in.reserve(block_bytes);
  } else if (host) {
    rc = eng->d_lw.reserve(block_bytes);
  }
  if (!rc) rc = eng->d_glm_pred.reserve((size_t)pla::glm_predict_workspace(rows, S) * sizeof(double));
  if (rc) return rc;

  // ---- outputs: the caller's device arrays, or engine memory
  unsigned long long *d_count = nullptr, *d_skipped = nullptr;
  double *d_mean = a->mean, *d_m2 = a->m2, *d_le = a->pit_le, *d_lt = a->pit_lt, *d_diag = loglik ? a->diag : nullptr,
         *d_elpd = loglik ? a->elpd_i : nullptr;
  HostOutputs out(eng, s);
  if (host) {
    d_count = eng->counters + pla::kCounterGlmReplaced;
    d_skipped = eng->counters + pla::kCounterGlmPitSkipped;
    rc = out.reserve(6, m, d_count);
    if (rc) return rc;
    PLA_HIP(hipMemsetAsync(d_skipped, 0, sizeof(unsigned long long), s));
    d_mean = a->mean ? out.col(0) : nullptr;
    d_m2 = a->m2 ? out.col(1) : nullptr;
    d_le = a->pit_le ? out.col(2) : nullptr;
    d_lt = a->pit_lt ? out.col(3) : nullptr;
    d_diag = loglik && a->diag ? out.col(4) : nullptr;
    d_elpd = loglik && a->elpd_i ? out.col(5) : nullptr;
  } else {
    d_count = a->n_replaced ? (unsigned long long*)a->n_replaced : eng->counters + pla::kCounterGlmReplaced;
    d_skipped = a->n_pit_skipped ? (unsigned long long*)a->n_pit_skipped : eng->counters + pla::kCounterGlmPitSkipped;
    PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
    PLA_HIP(hipMemsetAsync(d_skipped, 0, sizeof(unsigned long long), s));
  }

  char route[200], droute[160];
  std::string label;
  for (int64_t r0 = 0; r0 < m; r0 += rows) {
    const int64_t nr = m - r0 < rows ? m - r0 : rows;
    g.row_index = su.in.rows ? su.in.rows + r0 : nullptr;
    g.r_first = r0;
    g.n_rows = nr;
    g.out = nullptr;
    g.pitch = n_draws;
    g.replaced = nullptr;
    pla::GlmPredictLaunch q{};
    const char* prep = "";
    std::string weights;
    if (loglik) {
      char groute[160];
      g.out = eng->d_glm_ll.as<double>();
      PLA_HIP(pla::launch_glm(g, s, groute, (int)sizeof(groute)));
      PLA_HIP(pla::launch_diag_prepare(eng->d_glm_ll.p, PLA_F64, nr, n_draws, 1, nullptr, 0, nr, S, eng->d_in.p, d_count, s, &prep));
      p.in = eng->d_in.p;
      p.n_obs = nr;
      p.diag = d_diag ? d_diag + r0 : nullptr;
      p.lw_out = eng->d_lw.p;
      PLA_HIP(pla::launch_rows(p, PLA_F64, true, s));
      weights = std::string(groute) + " -> " + prep + " -> " + pla::last_rows_kernels() + " -> ";
      if (d_elpd) {
        PLA_HIP(pla::launch_diag(eng->d_lw.p, eng->d_in.p, -1.0, PLA_F64, nr, S, n_draws, 1, n_draws, 1, d_elpd + r0, nullptr, nullptr, s, droute,
                                 (int)sizeof(droute)));
        weights += std::string(droute) + " -> ";
      }
      q.lw = eng->d_lw.as<double>();
      q.lw_pitch = n_draws;
    } else if (host) {
      rc = upload_rows(a->log_weights, nullptr, r0, nr, a->lw_stride_obs, n_draws, sizeof(double), eng->d_lw.p, s);
      if (rc) return rc;
      q.lw = eng->d_lw.as<double>();
      q.lw_pitch = n_draws;
    } else {
      q.lw = a->log_weights + (size_t)r0 * (size_t)a->lw_stride_obs;
      q.lw_pitch = a->lw_stride_obs;
    }
    q.work = eng->d_glm_pred.as<double>();
    q.mean = d_mean ? d_mean + r0 : nullptr;
    q.m2 = d_m2 ? d_m2 + r0 : nullptr;
    q.pit_le = d_le ? d_le + r0 : nullptr;
    q.pit_lt = d_lt ? d_lt + r0 : nullptr;
    q.skipped = d_skipped;
    g.out = nullptr;
    {
      TimedLaunch t(eng, s);
      PLA_HIP(pla::launch_glm_predict(g, q, s, route, (int)sizeof(route)));
    }
    if (r0 == 0)
      label = su.prepared + weights + route +
              (loglik ? " per block of observations" : host ? " (weights staged in blocks)" : " (weights read in place)");
    if (host && !loglik) PLA_HIP(hipStreamSynchronize(s));  // the staging buffer is reused by the next block
  }
  eng->last_kernels = label;
  if (!host) return PLA_OK;
  rc = out.copy_back({a->mean, a->m2, a->pit_le, a->pit_lt, loglik ? a->diag : nullptr, loglik ? a->elpd_i : nullptr});
  if (rc) return rc;
  unsigned long long h[2] = {0, 0};
  PLA_HIP(hipMemcpyAsync(&h[0], d_count, sizeof(h[0]), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipMemcpyAsync(&h[1], d_skipped, sizeof(h[1]), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (a->n_replaced) *a->n_replaced = (int64_t)h[0];
  if (a->n_pit_skipped) *a->n_pit_skipped = (int64_t)h[1];
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

int pla_glm_marginal(const pla_glm_marginal_args* a) {
  if (!a) return fail(PLA_ERR_ARG, "args is NULL");
  if (a->struct_size != (int64_t)sizeof(pla_glm_marginal_args))
    return fail(PLA_ERR_ARG, "struct_size is %lld, pla_glm_marginal_args of this library has %lld bytes", (long long)a->struct_size,
                (long long)sizeof(pla_glm_marginal_args));
  if (a->grouped.struct_size != (int64_t)sizeof(pla_glm_grouped_args))
    return fail(PLA_ERR_ARG, "grouped.struct_size is %lld, pla_glm_grouped_args of this library has %lld bytes",
                (long long)a->grouped.struct_size, (long long)sizeof(pla_glm_grouped_args));
  if (a->grouped.glm.struct_size != (int64_t)sizeof(pla_glm_args))
    return fail(PLA_ERR_ARG, "grouped.glm.struct_size is %lld, pla_glm_args of this library has %lld bytes",
                (long long)a->grouped.glm.struct_size, (long long)sizeof(pla_glm_args));
  return marg_run(a);
}

int pla_glm_marginal_segment(void) { return pla::kGlmMargSeg; }

int pla_glm_predict(const pla_glm_predict_args* a) {
  if (!a) return fail(PLA_ERR_ARG, "args is NULL");
  if (a->struct_size != (int64_t)sizeof(pla_glm_predict_args))
    return fail(PLA_ERR_ARG, "struct_size is %lld, pla_glm_predict_args of this library has %lld bytes", (long long)a->struct_size,
                (long long)sizeof(pla_glm_predict_args));
  if (a->glm.struct_size != (int64_t)sizeof(pla_glm_args))
    return fail(PLA_ERR_ARG, "glm.struct_size is %lld, pla_glm_args of this library has %lld bytes", (long long)a->glm.struct_size,
                (long long)sizeof(pla_glm_args));
  return predict_run(a);
}

int pla_glm_predict_segment(void) { return pla::kGlmPredictSeg; }

}  // extern "C"
