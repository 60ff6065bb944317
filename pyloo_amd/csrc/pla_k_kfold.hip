// launchers of the k-fold cross-validation kernels (pla_kfold.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include "pla_kfold.h"
#include "pla_launch.h"

namespace pla {

int kfold_route(const void* base, int dtype, int64_t stride_row, int64_t stride_draw, int64_t n_draws) {
  const int64_t vec = dtype == PLA_F64 ? 2 : 4;
  if (stride_draw == 1 && (uintptr_t)base % 16 == 0 && stride_row % vec == 0 && n_draws <= kWave * kWaveSlots) return kKfoldWave;
  if (stride_row == 1 && stride_draw != 1) return kKfoldLane;
  return kKfoldBlock;
}

const char* kfold_route_name(int route) {
  return route == kKfoldWave ? "kfold_wave_kernel" : route == kKfoldLane ? "kfold_lane_kernel" : "kfold_block_kernel";
}

template <typename T>
static hipError_t launch_kfold_typed(const KfoldParams& p, unsigned routes, hipStream_t stream, int* launches) {
  constexpr int kVec = 16 / (int)sizeof(T);
  if (routes & (1u << kKfoldWave)) {
    int64_t grid = (p.n_tasks + kWavesPerBlock - 1) / kWavesPerBlock;
    if (grid > 2048 * 8 / kWavesPerBlock) grid = 2048 * 8 / kWavesPerBlock;
    hipLaunchKernelGGL((kfold_wave_kernel<T, kVec>), dim3((unsigned)grid), dim3(kWave * kWavesPerBlock), 0, stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++*launches;
  }
  if (routes & (1u << kKfoldLane)) {
    int64_t grid = (p.n_tasks + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL((kfold_lane_kernel<T>), dim3((unsigned)grid), dim3(256), 0, stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++*launches;
  }
  if (routes & (1u << kKfoldBlock)) {
    const int64_t grid = p.n_tasks < 8192 ? p.n_tasks : 8192;
    hipLaunchKernelGGL((kfold_block_kernel<T, 256>), dim3((unsigned)grid), dim3(256), 0, stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++*launches;
  }
  return hipSuccess;
}

hipError_t launch_kfold_lme(const KfoldParams& p, int dtype, unsigned routes, hipStream_t stream, int* launches) {
  *launches = 0;  // kernels launched by this call
  if (p.n_tasks <= 0 || p.n_sources <= 0) return hipSuccess;
  return dtype == PLA_F64 ? launch_kfold_typed<double>(p, routes, stream, launches) : launch_kfold_typed<float>(p, routes, stream, launches);
}

int64_t kfold_n_tiles(int64_t n_obs) {
  const int64_t tc = kfold_tile_cols(n_obs);
  return (n_obs + tc - 1) / tc;
}

hipError_t launch_kfold_reduce(const double* elpd, const double* lpd_full, int64_t n_obs, double scale, double* p_i, double* kfold_i,
                               double* part, const unsigned long long* replaced, double* agg, int grid_cap, hipStream_t stream) {
  const int64_t tc = kfold_tile_cols(n_obs);
  KfoldReduceParams p{elpd, lpd_full, n_obs, scale, p_i, kfold_i, part, tc, (n_obs + tc - 1) / tc, replaced, agg};
  int64_t grid = p.n_tiles;
  if (grid_cap > 0 && grid > grid_cap) grid = grid_cap;
  hipLaunchKernelGGL(kfold_tiles_kernel<0>, dim3((unsigned)grid), dim3(kKfoldThreads), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kfold_tiles_kernel<1>, dim3((unsigned)grid), dim3(kKfoldThreads), 0, stream, p);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kfold_final_kernel, dim3(1), dim3(kKfoldThreads), 0, stream, p);
  return hipGetLastError();
}

}  // namespace pla
