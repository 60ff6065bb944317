// launchers of the LOO-PIT kernels (pla_pit.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdio>

#include "pla_pit.h"
#include "pla_launch.h"

namespace pla {

static unsigned pit_grid(int64_t want, int64_t cap) {
  const int64_t g = want < cap ? want : cap;
  return (unsigned)(g < 1 ? 1 : g);
}

#define PLA_PIT_LAUNCH(kernel, grid, block)                            \
  do {                                                                 \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, p); \
    const hipError_t e_ = hipGetLastError();                           \
    if (e_ != hipSuccess) return e_;                                   \
  } while (0)

template <typename T>
static hipError_t launch_pit_prepare_typed(const PitPrepareParams& p, hipStream_t stream, const char** route) {
  const bool f64 = sizeof(T) == 8;
  if (p.stride_obs == 1 && p.stride_draw != 1 && p.n_rows > 1) {
    const int64_t units = ((p.n_rows + 63) / 64) * ((p.n_draws + 63) / 64);
    PLA_PIT_LAUNCH((pit_prepare_tile_kernel<T>), pit_grid(units, 8192), 256);
    if (route) *route = f64 ? "pit_prepare_tile_kernel<double>" : "pit_prepare_tile_kernel<float>";
  } else {
    const int64_t units = p.n_rows * ((p.n_draws + 1023) / 1024);
    PLA_PIT_LAUNCH((pit_prepare_row_kernel<T>), pit_grid(units, 8192), 256);
    if (route) *route = f64 ? "pit_prepare_row_kernel<double>" : "pit_prepare_row_kernel<float>";
  }
  return hipSuccess;
}

hipError_t launch_pit_prepare(const void* in, int dtype, int64_t stride_obs, int64_t stride_draw, int64_t n_rows, int n_draws, void* out,
                              unsigned long long* replaced, hipStream_t stream, const char** route) {
  if (n_rows <= 0 || n_draws <= 0) return hipSuccess;
  PitPrepareParams p{in, out, n_rows, n_draws, stride_obs, stride_draw, replaced};
  return dtype == PLA_F64 ? launch_pit_prepare_typed<double>(p, stream, route) : launch_pit_prepare_typed<float>(p, stream, route);
}

template <typename T, int MODE>
static hipError_t launch_pit_wave(const PitParams& p, hipStream_t stream) {
  const unsigned grid = pit_grid((p.n_obs + kPitWaves - 1) / kPitWaves, 4096);
  if (p.n_draws <= kPitRegDraws) PLA_PIT_LAUNCH((pit_wave_kernel<T, MODE, true>), grid, kWave * kPitWaves);
  else PLA_PIT_LAUNCH((pit_wave_kernel<T, MODE, false>), grid, kWave * kPitWaves);
  return hipSuccess;
}

template <typename T>
static hipError_t launch_pit_typed(const PitParams& p, hipStream_t stream, char* route, int cap) {
  constexpr int kVec = 16 / (int)sizeof(T);
  const char* tn = sizeof(T) == 8 ? "double" : "float";
  const char* how = p.n_draws <= kPitRegDraws ? "registers" : "streamed";
  hipError_t e;
  if (p.lw_sd == 1 && p.yh_sd == 1) {
    const bool aligned = (uintptr_t)p.lw % 16 == 0 && (uintptr_t)p.yh % 16 == 0 && p.lw_so % kVec == 0 && p.yh_so % kVec == 0 &&
                         p.n_draws % kVec == 0;
    e = aligned ? launch_pit_wave<T, kPitVec>(p, stream) : launch_pit_wave<T, kPitElem>(p, stream);
    if (route) snprintf(route, cap, "pit_wave_kernel<%s, %s, %s>", tn, aligned ? "16-byte loads" : "element loads", how);
  } else if (p.lw_so == 1 && p.yh_so == 1) {
    PLA_PIT_LAUNCH((pit_lane_kernel<T>), pit_grid((p.n_obs + 255) / 256, 8192), 256);
    e = hipSuccess;
    if (route) snprintf(route, cap, "pit_lane_kernel<%s>", tn);
  } else {
    e = launch_pit_wave<T, kPitStrided>(p, stream);
    if (route) snprintf(route, cap, "pit_wave_kernel<%s, strided, %s>", tn, how);
  }
  return e;
}

hipError_t launch_pit(const void* lw, const void* yh, const double* y, int dtype, int64_t n_obs, int n_draws, int64_t lw_stride_obs,
                      int64_t lw_stride_draw, int64_t yh_stride_obs, int64_t yh_stride_draw, double* pit_le, double* pit_lt,
                      hipStream_t stream, char* route, int cap) {
  if (route && cap > 0) route[0] = 0;
  if (n_obs <= 0 || n_draws <= 0) return hipSuccess;
  PitParams p{lw, yh, y, n_obs, n_draws, lw_stride_obs, lw_stride_draw, yh_stride_obs, yh_stride_draw, pit_le, pit_lt};
  return dtype == PLA_F64 ? launch_pit_typed<double>(p, stream, route, cap) : launch_pit_typed<float>(p, stream, route, cap);
}

}  // namespace pla
