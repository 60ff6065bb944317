// launchers of the GLM log-likelihood kernels with group-level terms (pla_glm_terms.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdio>

#define PLA_GLM_SHARED_ONLY
#include "pla_glm_terms.h"
#include "pla_launch.h"

namespace pla {

#define PLA_GLM_TERMS_LAUNCH(kernel, grid, block)                      \
  do {                                                                 \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, p); \
    const hipError_t e_ = hipGetLastError();                           \
    if (e_ != hipSuccess) return e_;                                   \
  } while (0)

static int64_t glm_terms_rows(const GlmTerms& t) {
  int64_t rows = 0;
  for (int k = 0; k < t.n_terms; ++k) rows += t.n_groups[k];
  return rows;
}

int64_t glm_terms_image_size(const GlmTerms& t, int n_draws) {
  const int64_t s_pad = ((int64_t)n_draws + kGlmTile - 1) / kGlmTile * kGlmTile;
  return glm_terms_rows(t) * s_pad;
}

hipError_t launch_glm_terms_prepare(GlmTerms* t, int n_draws, double* uimg, hipStream_t stream) {
  if (t->n_terms < 0 || t->n_terms > kGlmMaxTerms) return hipErrorInvalidValue;
  GlmTermsPrepareParams p{};
  int64_t rows = 0;
  for (int k = 0; k <= kGlmMaxTerms; ++k) {
    p.first[k] = t->first[k] = rows;
    if (k >= t->n_terms) continue;
    p.u[k] = t->u[k];
    p.st_draw[k] = t->u_stride_draw[k];
    p.st_group[k] = t->u_stride_group[k];
    rows += t->n_groups[k];
  }
  t->uimg = uimg;
  if (rows == 0 || n_draws <= 0) return hipSuccess;
  p.n_terms = t->n_terms;
  p.n_draws = n_draws;
  p.s_pad = (n_draws + kGlmTile - 1) / kGlmTile * kGlmTile;
  p.uimg = uimg;
  const int64_t units = (rows + kGlmTermsTile - 1) / kGlmTermsTile * (p.s_pad / kGlmTermsTile);
  const int64_t want = (units + 256 / kWave - 1) / (256 / kWave);
  PLA_GLM_TERMS_LAUNCH(glm_terms_prepare_kernel, (unsigned)(want < 16384 ? want : 16384), 256);
  return hipSuccess;
}

hipError_t launch_glm_terms(const GlmLaunch& g, const GlmTerms& t, hipStream_t stream, char* route, int cap) {
  if (t.n_terms == 0) return launch_glm(g, stream, route, cap);  // (no terms: the kernel of pla_glm.h itself)
  if (route && cap > 0) route[0] = 0;
  if (t.n_terms < 0 || t.n_terms > kGlmMaxTerms || !t.uimg) return hipErrorInvalidValue;
  if (g.n_rows <= 0 || g.n_draws <= 0 || g.n_pred <= 0) return hipSuccess;
  GlmTermsParams p{};
  const unsigned grid = glm_fill_params(g, &p.glm);
  p.uimg = t.uimg;
  p.n_terms = t.n_terms;
  for (int k = 0; k < t.n_terms; ++k) {
    if (t.n_groups[k] < 1 || !t.group[k]) return hipErrorInvalidValue;
    p.group[k] = t.group[k];
    p.z[k] = t.z[k];
    p.first[k] = t.first[k];
    p.last_group[k] = t.n_groups[k] - 1;
  }
  hipError_t e;
  const char* name = "";
  switch (g.family) {
    case PLA_GLM_GAUSSIAN: e = glm_terms_launch_family<PLA_GLM_GAUSSIAN>(p, grid, stream); name = "gaussian"; break;
    case PLA_GLM_BINOMIAL_LOGIT: e = glm_terms_launch_family<PLA_GLM_BINOMIAL_LOGIT>(p, grid, stream); name = "binomial logit"; break;
    case PLA_GLM_POISSON_LOG: e = glm_terms_launch_family<PLA_GLM_POISSON_LOG>(p, grid, stream); name = "poisson log"; break;
    case PLA_GLM_LINPRED: e = glm_terms_launch_family<PLA_GLM_LINPRED>(p, grid, stream); name = "linear predictor"; break;
    default: e = launch_glm_terms_more(g.family, p, grid, stream, &name);  // (pla_k_glm_terms_families.hip)
  }
  if (e == hipErrorInvalidValue) return e;  // (a family nobody has)
  if (route) {
    const bool panel = p.glm.p_pad > kGlmK * kGlmPanel;
    snprintf(route, cap, "glm_terms_kernel<%s, %d chunks of 16 predictors%s, %d group-level terms>", name, panel ? kGlmPanel : p.glm.p_pad / kGlmK,
             panel ? " per panel" : " in registers", t.n_terms);
  }
  return e;
}

}  // namespace pla
