// launchers of the GLM predictive kernels (pla_glm_predict.h): the row maxima of the weights, the generator's chain contracted
// against them, the combination of the segments
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdint>
#include <cstdio>

#define PLA_GLM_SHARED_ONLY
#include "pla_glm_predict.h"
#include "pla_launch.h"

namespace pla {

static unsigned glm_predict_grid(int64_t want, int64_t cap) {
  const int64_t g = want < cap ? want : cap;
  return (unsigned)(g < 1 ? 1 : g);
}

static int glm_predict_segments(int n_draws) {
  const int n_dtiles = (n_draws + kGlmTile - 1) / kGlmTile;
  return (n_dtiles + kGlmPredictSeg - 1) / kGlmPredictSeg;
}

int64_t glm_predict_workspace(int64_t n_rows, int n_draws) {
  return n_rows * (1 + (int64_t)glm_predict_segments(n_draws) * kGlmPredictSums);
}

hipError_t launch_glm_predict(const GlmLaunch& g, const GlmPredictLaunch& q, hipStream_t stream, char* route, int cap) {
  if (route && cap > 0) route[0] = 0;
  if (g.n_rows <= 0 || g.n_draws <= 0 || g.n_pred <= 0) return hipSuccess;
  GlmPredictParams p{};
  glm_fill_params(g, &p.g);
  p.g.out = nullptr;
  p.g.replaced = nullptr;
  p.lw = q.lw;
  p.lw_pitch = q.lw_pitch;
  p.row_max = q.work;
  p.part = q.work + g.n_rows;
  p.n_seg = glm_predict_segments(g.n_draws);
  p.want_pit = q.pit_le || q.pit_lt;
  p.discrete = glm_discrete(g.family);
  p.mean = q.mean;
  p.m2 = q.m2;
  p.pit_le = q.pit_le;
  p.pit_lt = q.pit_lt;
  p.skipped = q.skipped;
  // a wavefront per tile of observations and strip of whole segments: whole rows while there are tiles of observations enough to
  // fill the chip, shorter strips for few observations (the values do not depend on it: a segment is summed by one wavefront)
  constexpr int64_t kWantWaves = 8192;
  const int64_t row_tiles = (g.n_rows + kGlmTile - 1) / kGlmTile;
  int64_t strips = (kWantWaves + row_tiles - 1) / row_tiles;
  if (strips > p.n_seg) strips = p.n_seg;
  const int strip_segs = (int)((p.n_seg + strips - 1) / strips);
  p.g.strip_tiles = strip_segs * kGlmPredictSeg;
  p.g.n_strips = (p.n_seg + strip_segs - 1) / strip_segs;
  // (a wavefront per unit and no walk over the units: strips beyond one only below 8192 tiles of observations)
  const int64_t groups = (row_tiles * p.g.n_strips + kGlmWaves - 1) / kGlmWaves;
  if (groups > (int64_t)INT32_MAX) return hipErrorInvalidValue;  // (beyond 2^35 rows of one launch: the callers' blocks are far smaller)
  const unsigned grid = (unsigned)groups;

  hipLaunchKernelGGL(glm_predict_rowmax_kernel, dim3(glm_predict_grid((g.n_rows + 3) / 4, 16384)), dim3(256), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const char* name = "";
  switch (g.family) {
    case PLA_GLM_GAUSSIAN: e = glm_predict_launch_family<PLA_GLM_GAUSSIAN>(p, grid, stream); name = "gaussian"; break;
    case PLA_GLM_BINOMIAL_LOGIT: e = glm_predict_launch_family<PLA_GLM_BINOMIAL_LOGIT>(p, grid, stream); name = "binomial logit"; break;
    case PLA_GLM_POISSON_LOG: e = glm_predict_launch_family<PLA_GLM_POISSON_LOG>(p, grid, stream); name = "poisson log"; break;
    default: e = launch_glm_predict_more(g.family, p, grid, stream, &name);  // (pla_k_glm_predict_families.hip)
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(glm_predict_combine_kernel, dim3(glm_predict_grid((g.n_rows + 255) / 256, 8192)), dim3(256), 0, stream, p);
  e = hipGetLastError();
  if (route) {
    const int nch = p.g.p_pad > kGlmK * kGlmPanel ? kGlmPanel : p.g.p_pad / kGlmK;
    snprintf(route, cap, "glm_predict_rowmax_kernel -> glm_predict_kernel<%s, %d chunks of 16 predictors%s> -> glm_predict_combine_kernel", name,
             nch, p.g.p_pad > kGlmK * kGlmPanel ? " per panel" : " in registers");
  }
  return e;
}

}  // namespace pla
