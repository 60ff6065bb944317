// launchers of the GLM log-likelihood kernels with group-level terms (pla_glm_terms.h) of PLA_GLM_NEGBINOMIAL_LOG, PLA_GLM_GAMMA_LOG
// and PLA_GLM_BINOMIAL_PROBIT.  pla_k_glm_terms.hip hands them over (launch_glm_terms_more).
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#define PLA_GLM_SHARED_ONLY
#define PLA_GLM_TERMS_SHARED_ONLY
#include "pla_glm_terms.h"
#include "pla_launch.h"

namespace pla {

hipError_t launch_glm_terms_more(int family, const GlmTermsParams& p, unsigned grid, hipStream_t stream, const char** name) {
  switch (family) {
    case PLA_GLM_NEGBINOMIAL_LOG: *name = "negative binomial log"; return glm_terms_launch_family<PLA_GLM_NEGBINOMIAL_LOG>(p, grid, stream);
    case PLA_GLM_GAMMA_LOG: *name = "gamma log"; return glm_terms_launch_family<PLA_GLM_GAMMA_LOG>(p, grid, stream);
    case PLA_GLM_BINOMIAL_PROBIT: *name = "binomial probit"; return glm_terms_launch_family<PLA_GLM_BINOMIAL_PROBIT>(p, grid, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pla
