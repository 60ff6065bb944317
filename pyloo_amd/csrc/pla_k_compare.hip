// launchers of the model-comparison kernels (pla_compare.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include "pla_compare.h"
#include "pla_launch.h"

namespace pla {

namespace {

constexpr int64_t kCompareGridAuto = 16384;  // workgroups per launch unless the engine caps it (the results do not depend on it)

CompareInput compare_input(const void* x, int64_t pitch, int K, int64_t N, double scale_mul) {
  const int64_t tc = compare_tile_cols(N);
  return CompareInput{x, pitch, K, N, scale_mul, tc, (N + tc - 1) / tc};
}

unsigned grid_of(int64_t items, int grid_cap) {
  int64_t g = items < kCompareGridAuto ? items : kCompareGridAuto;
  if (grid_cap > 0 && g > grid_cap) g = grid_cap;
  return (unsigned)(g > 0 ? g : 1);
}

unsigned model_groups(int K, int chunk = kCompareChunk) { return (unsigned)((K + chunk - 1) / chunk); }

}  // namespace

int64_t compare_n_tiles(int64_t n_obs) {
  const int64_t tc = compare_tile_cols(n_obs);
  return (n_obs + tc - 1) / tc;
}

hipError_t launch_compare_moments(const void* x, int dtype, int64_t pitch, int K, int64_t N, int best, double* part, double* out,
                                  int grid_cap, hipStream_t stream) {
  MomentsParams p{compare_input(x, pitch, K, N, 1.0), best, part};
  const dim3 grid(grid_of(p.in.n_tiles, grid_cap), model_groups(K, kMomentsChunk));
  if (dtype == PLA_F64)
    hipLaunchKernelGGL((compare_moments_kernel<double>), grid, dim3(kCompareThreads), 0, stream, p);
  else
    hipLaunchKernelGGL((compare_moments_kernel<float>), grid, dim3(kCompareThreads), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(compare_moments_final_kernel, dim3(1), dim3(128), 0, stream, (const double*)part, K, p.in.n_tiles, out);
  return hipGetLastError();
}

hipError_t launch_stacking_eval(const void* x, int dtype, int64_t pitch, int K, int64_t N, double scale_mul, const double* w,
                                double* part, double* out, int grid_cap, hipStream_t stream) {
  StackingParams p{compare_input(x, pitch, K, N, scale_mul), w, part};
  const dim3 grid(grid_of(p.in.n_tiles, grid_cap), model_groups(K));
  if (dtype == PLA_F64)
    hipLaunchKernelGGL((stacking_eval_kernel<double>), grid, dim3(kCompareThreads), 0, stream, p);
  else
    hipLaunchKernelGGL((stacking_eval_kernel<float>), grid, dim3(kCompareThreads), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(compare_tiles_sum_kernel, dim3(1), dim3(128), 0, stream, (const double*)part, K + 1, p.in.n_tiles, out);
  return hipGetLastError();
}

hipError_t launch_bb_bootstrap(const void* x, int dtype, int64_t pitch, int K, int64_t N, double scale_mul, uint64_t seed, double alpha,
                               int64_t b0, int64_t nb, double* part, double* z, int grid_cap, hipStream_t stream) {
  BBParams p{compare_input(x, pitch, K, N, scale_mul), seed, alpha, b0, nb, part};
  // (tiles x blocks of 64 replicates within kCompareGridAuto workgroups, or the engine's cap, per group of models)
  const int64_t nbb = (nb + 63) / 64;
  int64_t cap = grid_cap > 0 ? grid_cap : kCompareGridAuto;
  const int64_t gx = p.in.n_tiles < cap ? p.in.n_tiles : cap;
  int64_t gy = cap / gx;
  gy = gy < 1 ? 1 : (gy > nbb ? nbb : (gy > 65535 ? 65535 : gy));
  const dim3 grid((unsigned)gx, (unsigned)gy, model_groups(K));
  if (dtype == PLA_F64)
    hipLaunchKernelGGL((bb_bootstrap_kernel<double>), grid, dim3(kCompareThreads), 0, stream, p);
  else
    hipLaunchKernelGGL((bb_bootstrap_kernel<float>), grid, dim3(kCompareThreads), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t threads = nb * K;
  hipLaunchKernelGGL(bb_final_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, (const double*)part, K,
                     p.in.n_tiles, nb, (double)N * scale_mul, z);
  return hipGetLastError();
}

hipError_t launch_bb_gamma_draws(uint64_t seed, double alpha, int64_t B, int64_t N, double* out, hipStream_t stream) {
  const int64_t n = B * N;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(bb_gamma_draws_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed, alpha, B, N, out);
  return hipGetLastError();
}

}  // namespace pla
static_assert(pla::kCompareMaxModels == PLA_COMPARE_MAX_MODELS, "the C ABI names the device limit");
