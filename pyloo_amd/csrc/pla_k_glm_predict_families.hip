// launchers of the GLM predictive kernels (pla_glm_predict.h) of the families with a special function or a second value per draw in
// the epilogue: PLA_GLM_NEGBINOMIAL_LOG, PLA_GLM_GAMMA_LOG, PLA_GLM_BINOMIAL_PROBIT.  pla_k_glm_predict.hip hands them over.
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#define PLA_GLM_SHARED_ONLY
#define PLA_GLM_PREDICT_SHARED_ONLY
#include "pla_glm_predict.h"
#include "pla_launch.h"

namespace pla {

hipError_t launch_glm_predict_more(int family, const GlmPredictParams& p, unsigned grid, hipStream_t stream, const char** name) {
  switch (family) {
    case PLA_GLM_NEGBINOMIAL_LOG: *name = "negative binomial log"; return glm_predict_launch_family<PLA_GLM_NEGBINOMIAL_LOG>(p, grid, stream);
    case PLA_GLM_GAMMA_LOG: *name = "gamma log"; return glm_predict_launch_family<PLA_GLM_GAMMA_LOG>(p, grid, stream);
    case PLA_GLM_BINOMIAL_PROBIT: *name = "binomial probit"; return glm_predict_launch_family<PLA_GLM_BINOMIAL_PROBIT>(p, grid, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pla
