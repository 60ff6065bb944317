// launchers of the GLM log-likelihood kernels (pla_glm.h) of the families with a special function or a second value per draw in the
// epilogue: PLA_GLM_NEGBINOMIAL_LOG, PLA_GLM_GAMMA_LOG, PLA_GLM_BINOMIAL_PROBIT.  pla_k_glm.hip hands them over (launch_glm_more).
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#define PLA_GLM_SHARED_ONLY
#include "pla_glm.h"
#include "pla_launch.h"

namespace pla {

hipError_t launch_glm_more(int family, const GlmParams& p, unsigned grid, hipStream_t stream, const char** name) {
  switch (family) {
    case PLA_GLM_NEGBINOMIAL_LOG: *name = "negative binomial log"; return glm_launch_family<PLA_GLM_NEGBINOMIAL_LOG>(p, grid, stream);
    case PLA_GLM_GAMMA_LOG: *name = "gamma log"; return glm_launch_family<PLA_GLM_GAMMA_LOG>(p, grid, stream);
    case PLA_GLM_BINOMIAL_PROBIT: *name = "binomial probit"; return glm_launch_family<PLA_GLM_BINOMIAL_PROBIT>(p, grid, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pla
