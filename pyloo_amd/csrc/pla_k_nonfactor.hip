// launchers of the non-factorised LOO kernels (pla_nonfactor.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include "pla_launch.h"
#include "pla_nonfactor.h"

namespace pla {

namespace {

constexpr int kNfGridAuto = 2048;  // workgroups of the LDS route unless the engine caps it (the results do not depend on it)

template <typename T>
hipError_t launch_typed(const NonfactorParams& base, int route, int ws_slots, int grid_cap, hipStream_t s) {
  NonfactorParams p = base;
  const int lds_cap = grid_cap > 0 ? grid_cap : kNfGridAuto;
  const unsigned lds_grid = (unsigned)(p.n_draws < lds_cap ? p.n_draws : lds_cap);
  const unsigned ws_grid = (unsigned)(p.n_draws < ws_slots ? p.n_draws : ws_slots);
  if (route == kNfRouteGeneral) {  // every draw to the general kernel
    const hipError_t m = hipMemsetD32Async((hipDeviceptr_t)p.flags, kNfGeneral, (size_t)p.n_draws, s);
    if (m != hipSuccess) return m;
  } else if (route == kNfRouteLds)
    hipLaunchKernelGGL((nonfactor_lds_kernel<T>), dim3(lds_grid), dim3(kNfThreads), 0, s, p);
  else if (route == kNfRouteWorkspace)
    hipLaunchKernelGGL((nonfactor_blocked_kernel<T>), dim3(ws_grid), dim3(kNfThreads), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the general route: every draw (forced), else the draws the Cholesky kernel declined (it skips the others)
  hipLaunchKernelGGL((nonfactor_lu_kernel<T>), dim3(ws_grid), dim3(kNfThreads), 0, s, p);
  return hipGetLastError();
}

}  // namespace

int nonfactor_lds_max_obs() { return kNfLdsMaxObs; }

int64_t nonfactor_slot_doubles(int n_obs) {  // the blocked route's Np x Np matrix and Np x 16 panel; the general route's N x N
  const int64_t np = (n_obs + kNfTile - 1) / kNfTile * kNfTile;
  return np * np + np * kNfTile;
}

int nonfactor_route_for(int n_obs, int forced) {
  if (forced == kNfRouteGeneral || forced == kNfRouteWorkspace) return forced;
  return n_obs <= kNfLdsMaxObs ? kNfRouteLds : kNfRouteWorkspace;  // automatic, or the LDS route where the shape allows it
}

hipError_t launch_nonfactor(const NonfactorParams& p, int dtype, int route, int ws_slots, int grid_cap, hipStream_t stream) {
  if (p.n_draws <= 0) return hipSuccess;
  return dtype == PLA_F64 ? launch_typed<double>(p, route, ws_slots, grid_cap, stream)
                          : launch_typed<float>(p, route, ws_slots, grid_cap, stream);
}

}  // namespace pla
static_assert(pla::kNfMaxObs == PLA_NONFACTOR_MAX_OBS, "the C ABI names the device limit");
static_assert(pla::kNfGeneral == PLA_NF_GENERAL && pla::kNfSingular == PLA_NF_SINGULAR && pla::kNfNonfinite == PLA_NF_NONFINITE &&
                  pla::kNfDfNonpos == PLA_NF_DF_NONPOS && pla::kNfBetaNonfinite == PLA_NF_BETA_NONFINITE &&
                  pla::kNfClamped == PLA_NF_CLAMPED,
              "the C ABI names the status bits");
static_assert(pla::kNfStudentT == PLA_MVN_STUDENT_T && pla::kNfNormal == PLA_MVN_NORMAL, "the C ABI names the model types");
static_assert(pla::kNfRouteLds == PLA_NF_ROUTE_LDS && pla::kNfRouteWorkspace == PLA_NF_ROUTE_WORKSPACE &&
                  pla::kNfRouteGeneral == PLA_NF_ROUTE_GENERAL,
              "the C ABI names the routes");
