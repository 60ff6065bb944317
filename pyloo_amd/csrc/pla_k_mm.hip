// launchers of the moment-matching kernels (pla_mm.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include "pla_mm.h"
#include "pla_launch.h"

namespace pla {

static unsigned mm_grid(int64_t want, int grid_cap) {
  int64_t g = want < 1 ? 1 : want > 16384 ? 16384 : want;
  if (grid_cap > 0 && g > grid_cap) g = grid_cap;
  return (unsigned)g;
}

#define PLA_MM_LAUNCH(kernel, grid, p)                                          \
  do {                                                                          \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kMmThreads), 0, stream, p);     \
    const hipError_t e_ = hipGetLastError();                                    \
    if (e_ != hipSuccess) return e_;                                            \
  } while (0)

int64_t mm_moments_workspace(int64_t B, int64_t S, int D, int want_cov) { return mm_workspace_doubles(B, S, D, want_cov); }

hipError_t launch_mm_moments(const double* x, const double* lw, int64_t B, int64_t S, int D, int want_cov, double* work, double* stats,
                             double* cov, int grid_cap, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int64_t nT = mm_tiles(S), nTc = mm_cov_tiles(S);
  MmMomentsParams p{x, lw, B, S, D, want_cov, nullptr, nullptr, nullptr, nullptr, stats, cov};
  p.part0 = work;
  p.mid = p.part0 + B * nT * (3 * (int64_t)D + 2);
  p.part1 = p.mid + B * (D + 2);
  p.partc = p.part1 + B * nT * D;
  const int per_b = D + (want_cov ? mm_pairs(D) : 0);
  PLA_MM_LAUNCH(mm_sums_kernel<0>, mm_grid(B * nT, grid_cap), p);
  PLA_MM_LAUNCH(mm_mid_kernel, mm_grid((B * D + kMmThreads - 1) / kMmThreads, grid_cap), p);
  PLA_MM_LAUNCH(mm_sums_kernel<1>, mm_grid(B * nT, grid_cap), p);
  if (want_cov) PLA_MM_LAUNCH(mm_cov_kernel, mm_grid(B * nTc, grid_cap), p);
  PLA_MM_LAUNCH(mm_fin_kernel, mm_grid((B * per_b + kMmThreads - 1) / kMmThreads, grid_cap), p);
  return hipSuccess;
}

hipError_t launch_mm_transform(const MmTransformParams& p, int grid_cap, hipStream_t stream) {
  if (p.B <= 0) return hipSuccess;
  if (p.map) {
    PLA_MM_LAUNCH(mm_map_kernel, mm_grid(p.B * ((p.S + kMmMapRows - 1) / kMmMapRows), grid_cap), p);
  } else {
    PLA_MM_LAUNCH(mm_affine_kernel, mm_grid((p.B * p.S * p.D + kMmThreads - 1) / kMmThreads, grid_cap), p);
  }
  return hipSuccess;
}

hipError_t launch_mm_ratios(int mode, const MmRatiosParams& p, int grid_cap, hipStream_t stream) {
  if (p.B <= 0) return hipSuccess;
  const unsigned grid = mm_grid((p.B * p.S + kMmThreads - 1) / kMmThreads, grid_cap);
  if (mode == 0) {
    PLA_MM_LAUNCH(mm_ratios_kernel<0>, grid, p);
  } else if (mode == 1) {
    PLA_MM_LAUNCH(mm_ratios_kernel<1>, grid, p);
  } else if (mode == 2) {
    PLA_MM_LAUNCH(mm_ratios_kernel<2>, grid, p);
  } else {
    PLA_MM_LAUNCH(mm_finish_kernel, mm_grid((p.B + kMmThreads / 64 - 1) / (kMmThreads / 64), grid_cap), p);
  }
  return hipSuccess;
}

}  // namespace pla
