// launchers of the cluster-marginal GLM kernels (pla_glm_marginal.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdio>

#define PLA_GLM_SHARED_ONLY
#define PLA_GLM_MARGINAL_KERNELS
#include "pla_glm_marginal.h"
#include "pla_launch.h"

namespace pla {

#define PLA_GLM_MARG_LAUNCH(kernel, grid, block)                       \
  do {                                                                 \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, p); \
    const hipError_t e_ = hipGetLastError();                           \
    if (e_ != hipSuccess) return e_;                                   \
  } while (0)

int glm_marginal_capacity(int n_nodes) { return n_nodes <= 8 ? 8 : n_nodes <= 16 ? 16 : 32; }

static unsigned glm_marg_grid(int64_t units) {
  const int64_t want = (units + kGlmWaves - 1) / kGlmWaves;
  return (unsigned)(want < 1 ? 1 : want < 65536 ? want : 65536);
}

template <int FAM>
static hipError_t launch_glm_marginal_family(const GlmMargParams& p, hipStream_t stream) {
  constexpr int block = kWave * kGlmWaves;
  const int cap = glm_marginal_capacity(p.n_nodes);
  if (p.n_segs > 0) {
    const unsigned grid = glm_marg_grid(p.n_segs * p.n_strips);
    if (cap == 8) PLA_GLM_MARG_LAUNCH((glm_marginal_kernel<FAM, 8>), grid, block);
    else if (cap == 16) PLA_GLM_MARG_LAUNCH((glm_marginal_kernel<FAM, 16>), grid, block);
    else PLA_GLM_MARG_LAUNCH((glm_marginal_kernel<FAM, 32>), grid, block);
  }
  if (p.n_joins > 0) {
    const unsigned grid = glm_marg_grid(p.n_joins * p.n_strips);
    if (cap == 8) PLA_GLM_MARG_LAUNCH((glm_marginal_join_kernel<8>), grid, block);
    else if (cap == 16) PLA_GLM_MARG_LAUNCH((glm_marginal_join_kernel<16>), grid, block);
    else PLA_GLM_MARG_LAUNCH((glm_marginal_join_kernel<32>), grid, block);
  }
  return hipSuccess;
}

hipError_t launch_glm_marginal(int family, const GlmMargParams& q, hipStream_t stream, char* route, int cap) {
  if (route && cap > 0) route[0] = 0;
  if (q.n_nodes < 1 || q.n_nodes > kGlmMargMaxNodes || q.n_draws < 1 || q.n_segs < 0 || q.n_joins < 0) return hipErrorInvalidValue;
  if (q.n_segs > 0 && (!q.segs || !q.out || !q.tau || !q.nodes || !q.logw)) return hipErrorInvalidValue;
  if (q.n_joins > 0 && (!q.joins || !q.part || !q.carry)) return hipErrorInvalidValue;
  GlmMargParams p = q;
  p.n_strips = (q.n_draws + kWave - 1) / kWave;
  hipError_t e;
  const char* name;
  switch (family) {
    case PLA_GLM_GAUSSIAN: e = launch_glm_marginal_family<PLA_GLM_GAUSSIAN>(p, stream); name = "gaussian"; break;
    case PLA_GLM_BINOMIAL_LOGIT: e = launch_glm_marginal_family<PLA_GLM_BINOMIAL_LOGIT>(p, stream); name = "binomial logit"; break;
    case PLA_GLM_POISSON_LOG: e = launch_glm_marginal_family<PLA_GLM_POISSON_LOG>(p, stream); name = "poisson log"; break;
    default: return hipErrorInvalidValue;
  }
  if (route)
    snprintf(route, cap, "glm_marginal_kernel<%s, %d nodes in registers>%s", name, glm_marginal_capacity(p.n_nodes),
             p.n_joins > 0 ? " -> glm_marginal_join_kernel" : "");
  return e;
}

}  // namespace pla
