// launchers of the GLM log-likelihood kernels (pla_glm.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdio>

#include "pla_glm.h"
#include "pla_launch.h"

namespace pla {

static unsigned glm_grid(int64_t want, int64_t cap) {
  const int64_t g = want < cap ? want : cap;
  return (unsigned)(g < 1 ? 1 : g);
}

#define PLA_GLM_LAUNCH(kernel, grid, block)                            \
  do {                                                                 \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, p); \
    const hipError_t e_ = hipGetLastError();                           \
    if (e_ != hipSuccess) return e_;                                   \
  } while (0)

// chunks of 16 predictors a wavefront keeps in registers: 1, 2, 4, 8 for P <= 16, 32, 64, 128; beyond, panels of 8
static int glm_chunks(int n_pred) { return n_pred <= 16 ? 1 : n_pred <= 32 ? 2 : n_pred <= 64 ? 4 : kGlmPanel; }

void glm_pads(int n_draws, int n_pred, int* s_pad, int* p_pad) {
  const int w = kGlmK * glm_chunks(n_pred);
  *s_pad = (n_draws + kGlmTile - 1) / kGlmTile * kGlmTile;
  *p_pad = (n_pred + w - 1) / w * w;
}

hipError_t launch_glm_prepare(const double* beta, int64_t stride_draw, int64_t stride_pred, int n_draws, int n_pred, double* bimg,
                              hipStream_t stream) {
  if (n_draws <= 0 || n_pred <= 0) return hipSuccess;
  GlmPrepareParams p{beta, stride_draw, stride_pred, n_draws, n_pred, 0, 0, bimg};
  glm_pads(n_draws, n_pred, &p.s_pad, &p.p_pad);
  PLA_GLM_LAUNCH(glm_prepare_kernel, glm_grid(((int64_t)p.s_pad * p.p_pad + kGlmImagePad + 255) / 256, 8192), 256);
  return hipSuccess;
}

unsigned glm_fill_params(const GlmLaunch& g, GlmParams* out) {
  GlmParams& p = *out;
  p = GlmParams{};
  p.x = g.x;
  p.sx_obs = g.x_stride_obs;
  p.sx_pred = g.x_stride_pred;
  p.n_src = g.n_src;
  p.row_index = g.row_index;
  p.r_first = g.r_first;
  p.n_rows = g.n_rows;
  p.bimg = g.bimg;
  p.n_pred = g.n_pred;
  p.n_draws = g.n_draws;
  glm_pads(g.n_draws, g.n_pred, &p.s_pad, &p.p_pad);
  p.zero = g.bimg + (size_t)p.s_pad * (size_t)p.p_pad;
  p.y = g.y;
  p.offset = g.offset;
  p.trials = g.trials;
  p.obs_const = g.obs_const;
  p.sigma = g.sigma;
  p.draw_const = g.draw_const;
  p.out = g.out;
  p.pitch = g.pitch;
  p.replaced = g.replaced;
  // a wavefront per tile of observations and strip of draw tiles: whole rows while there are tiles of observations enough to fill
  // the chip, shorter strips for few observations (the values do not depend on it)
  constexpr int64_t kWantWaves = 8192;
  const int64_t row_tiles = (g.n_rows + kGlmTile - 1) / kGlmTile;
  const int n_dtiles = p.s_pad / kGlmTile;
  int64_t strips = (kWantWaves + row_tiles - 1) / row_tiles;
  if (strips > n_dtiles) strips = n_dtiles;
  p.strip_tiles = (int)((n_dtiles + strips - 1) / strips);
  p.n_strips = (n_dtiles + p.strip_tiles - 1) / p.strip_tiles;
  return glm_grid((row_tiles * p.n_strips + kGlmWaves - 1) / kGlmWaves, (int64_t)1 << 20);
}

hipError_t launch_glm(const GlmLaunch& g, hipStream_t stream, char* route, int cap) {
  if (route && cap > 0) route[0] = 0;
  if (g.n_rows <= 0 || g.n_draws <= 0 || g.n_pred <= 0) return hipSuccess;
  GlmParams p;
  const unsigned grid = glm_fill_params(g, &p);
  hipError_t e;
  const char* name = "";
  switch (g.family) {
    case PLA_GLM_GAUSSIAN: e = glm_launch_family<PLA_GLM_GAUSSIAN>(p, grid, stream); name = "gaussian"; break;
    case PLA_GLM_BINOMIAL_LOGIT: e = glm_launch_family<PLA_GLM_BINOMIAL_LOGIT>(p, grid, stream); name = "binomial logit"; break;
    case PLA_GLM_POISSON_LOG: e = glm_launch_family<PLA_GLM_POISSON_LOG>(p, grid, stream); name = "poisson log"; break;
    case PLA_GLM_LINPRED: e = glm_launch_family<PLA_GLM_LINPRED>(p, grid, stream); name = "linear predictor"; break;
    default: e = launch_glm_more(g.family, p, grid, stream, &name);  // (pla_k_glm_families.hip)
  }
  if (e == hipErrorInvalidValue) return e;  // (a family nobody has)
  if (route) {
    const int nch = p.p_pad > kGlmK * kGlmPanel ? kGlmPanel : p.p_pad / kGlmK;
    snprintf(route, cap, "glm_kernel<%s, %d chunks of 16 predictors%s>", name, nch, p.p_pad > kGlmK * kGlmPanel ? " per panel" : " in registers");
  }
  return e;
}

}  // namespace pla
