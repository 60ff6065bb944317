// launchers of the relative-efficiency kernels (pla_ess.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdio>

#include "pla_ess.h"
#include "pla_launch.h"

namespace pla {

int ess_lds_max_draws() { return kEssLdsDraws; }

// workgroups of a launch over n_rows rows: a workgroup is one wavefront and takes rows blockIdx.x, + grid, ...
int64_t ess_grid_for(int64_t n_rows, int64_t analysed, int cap) {
  // LDS route: 4 to 5 workgroups per CU x 256 CUs resident, some 16 rounds of them so that rows of unequal cost even out;
  // long route: every workgroup owns a slot of workspace, so fewer
  int64_t g = analysed <= kEssLdsDraws ? 16 * 1280 : 512;
  if (cap > 0 && cap < g) g = cap;
  if (n_rows < g) g = n_rows;
  return g < 1 ? 1 : g;
}

template <typename T>
static hipError_t launch_ess_typed(const EssParams& p, bool lds, unsigned grid, hipStream_t stream) {
  if (lds) hipLaunchKernelGGL((ess_row_kernel<T, true>), dim3(grid), dim3(kWave), 0, stream, p);
  else hipLaunchKernelGGL((ess_row_kernel<T, false>), dim3(grid), dim3(kWave), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_ess(const void* in, int dtype, int64_t stride_obs, int64_t n_rows, int n_src_chains, int n_src, int split, int log_mode,
                      int cap_one, double* ws, int grid_cap, double* out, unsigned long long* invalid, hipStream_t stream, char* route,
                      int cap) {
  if (route && cap > 0) route[0] = 0;
  if (n_rows <= 0) return hipSuccess;
  const int n = split ? n_src / 2 : n_src;
  const int64_t analysed = (int64_t)(split ? 2 * n_src_chains : n_src_chains) * n;
  const bool lds = analysed <= kEssLdsDraws;
  if (!lds && !ws) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)ess_grid_for(n_rows, analysed, grid_cap);
  EssParams p{in, stride_obs, n_rows, n_src_chains, n_src, n, split, log_mode, cap_one, ws, out, invalid};
  if (route) snprintf(route, cap, "ess_row_kernel<%s, %s>", dtype_name(dtype), lds ? "LDS" : "global workspace");
  return dtype == PLA_F64 ? launch_ess_typed<double>(p, lds, grid, stream) : launch_ess_typed<float>(p, lds, grid, stream);
}

}  // namespace pla
