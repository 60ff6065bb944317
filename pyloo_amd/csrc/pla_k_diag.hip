// launchers of the LOO diagnostics kernels (pla_diag.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdio>

#include "pla_diag.h"
#include "pla_launch.h"

namespace pla {

static unsigned diag_grid(int64_t want, int64_t cap) {
  const int64_t g = want < cap ? want : cap;
  return (unsigned)(g < 1 ? 1 : g);
}

#define PLA_DIAG_LAUNCH(kernel, grid, block)                           \
  do {                                                                 \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, p); \
    const hipError_t e_ = hipGetLastError();                           \
    if (e_ != hipSuccess) return e_;                                   \
  } while (0)

template <typename T>
static hipError_t launch_diag_prepare_typed(const DiagPrepareParams& p, hipStream_t stream, const char** route) {
  const bool f64 = sizeof(T) == 8;
  if (p.stride_obs == 1 && p.stride_draw != 1 && p.n_src > 1) {
    const int64_t units = ((p.n_rows + 63) / 64) * ((p.n_draws + 63) / 64);
    PLA_DIAG_LAUNCH((diag_prepare_tile_kernel<T>), diag_grid(units, 8192), 256);
    if (route) *route = f64 ? "diag_prepare_tile_kernel<double>" : "diag_prepare_tile_kernel<float>";
  } else {
    const int64_t units = p.n_rows * ((p.n_draws + 1023) / 1024);
    PLA_DIAG_LAUNCH((diag_prepare_row_kernel<T>), diag_grid(units, 8192), 256);
    if (route) *route = f64 ? "diag_prepare_row_kernel<double>" : "diag_prepare_row_kernel<float>";
  }
  return hipSuccess;
}

hipError_t launch_diag_prepare(const void* in, int dtype, int64_t n_src, int64_t stride_obs, int64_t stride_draw, const int64_t* row_index,
                               int64_t row0, int64_t n_rows, int n_draws, void* out, unsigned long long* replaced, hipStream_t stream,
                               const char** route) {
  if (n_rows <= 0 || n_draws <= 0 || n_src <= 0) return hipSuccess;
  DiagPrepareParams p{in, out, row_index, row0, n_src, n_rows, n_draws, stride_obs, stride_draw, replaced};
  return dtype == PLA_F64 ? launch_diag_prepare_typed<double>(p, stream, route) : launch_diag_prepare_typed<float>(p, stream, route);
}

template <typename T, int MODE>
static hipError_t launch_diag_wave(const DiagParams& p, hipStream_t stream) {
  const unsigned grid = diag_grid((p.n_obs + kPitWaves - 1) / kPitWaves, 4096);
  if constexpr (MODE == kPitStrided) {  // (always streamed: the same terms in the same order, see pla_diag.h)
    PLA_DIAG_LAUNCH((diag_wave_kernel<T, MODE, false>), grid, kWave * kPitWaves);
  } else {
    if (p.n_draws <= kPitRegDraws) PLA_DIAG_LAUNCH((diag_wave_kernel<T, MODE, true>), grid, kWave * kPitWaves);
    else PLA_DIAG_LAUNCH((diag_wave_kernel<T, MODE, false>), grid, kWave * kPitWaves);
  }
  return hipSuccess;
}

template <typename T>
static hipError_t launch_diag_typed(const DiagParams& p, hipStream_t stream, char* route, int cap) {
  constexpr int kVec = 16 / (int)sizeof(T);
  const char* tn = sizeof(T) == 8 ? "double" : "float";
  const char* how = p.n_draws <= kPitRegDraws ? "registers" : "streamed";
  hipError_t e;
  if (p.lw_sd == 1 && p.x_sd == 1) {
    const bool aligned = (uintptr_t)p.lw % 16 == 0 && (uintptr_t)p.x % 16 == 0 && p.lw_so % kVec == 0 && p.x_so % kVec == 0 &&
                         p.n_draws % kVec == 0;
    e = aligned ? launch_diag_wave<T, kPitVec>(p, stream) : launch_diag_wave<T, kPitElem>(p, stream);
    if (route) snprintf(route, cap, "diag_wave_kernel<%s, %s, %s>", tn, aligned ? "16-byte loads" : "element loads", how);
  } else {
    e = launch_diag_wave<T, kPitStrided>(p, stream);
    if (route) snprintf(route, cap, "diag_wave_kernel<%s, strided, streamed>", tn);
  }
  return e;
}

hipError_t launch_diag(const void* lw, const void* x, double sign, int dtype, int64_t n_obs, int n_draws, int64_t lw_stride_obs,
                       int64_t lw_stride_draw, int64_t x_stride_obs, int64_t x_stride_draw, double* elpd, double* ess_w, double* var_log,
                       hipStream_t stream, char* route, int cap) {
  if (route && cap > 0) route[0] = 0;
  if (n_obs <= 0 || n_draws <= 0) return hipSuccess;
  DiagParams p{lw, x, sign, n_obs, n_draws, lw_stride_obs, lw_stride_draw, x_stride_obs, x_stride_draw, elpd, ess_w, var_log};
  return dtype == PLA_F64 ? launch_diag_typed<double>(p, stream, route, cap) : launch_diag_typed<float>(p, stream, route, cap);
}

}  // namespace pla
