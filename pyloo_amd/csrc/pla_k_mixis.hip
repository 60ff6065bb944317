// launchers of the Mix-IS-LOO kernels (pla_mixis.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdio>

#include "pla_mixis.h"
#include "pla_launch.h"

namespace pla {

int64_t mixis_tile_rows_for(int64_t n_obs) { return mixis_tile_rows(n_obs); }
int64_t mixis_n_tiles(int64_t n_obs) {
  const int64_t t = mixis_tile_rows(n_obs);
  return (n_obs + t - 1) / t;
}

static unsigned capped(int64_t want, int64_t dflt, int grid_cap) {
  int64_t g = want < dflt ? want : dflt;
  if (grid_cap > 0 && g > grid_cap) g = grid_cap;
  return (unsigned)(g < 1 ? 1 : g);
}

#define PLA_MIXIS_LAUNCH(kernel, grid, block)                                   \
  do {                                                                          \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, p);          \
    const hipError_t e_ = hipGetLastError();                                    \
    if (e_ != hipSuccess) return e_;                                            \
  } while (0)

template <typename T>
static hipError_t launch_mixis_c_typed(const MixisParams& p, int64_t vec_pitch, int grid_cap, hipStream_t stream, char* route, int cap) {
  constexpr int kVec = 16 / (int)sizeof(T);
  const int64_t n_db = (p.n_draws + 255) / 256;
  const char* tn = sizeof(T) == 8 ? "double" : "float";
  if (p.stride_draw == 1) {
    PLA_MIXIS_LAUNCH((mixis_c_tile_kernel<T, true>), capped(n_db * p.n_tiles, 4096, grid_cap), 256);
    snprintf(route, cap, "mixis_c_tile_kernel<%s, unit>", tn);
  } else if (p.stride_obs == 1) {
    const unsigned grid = capped(((int64_t)p.n_draws * p.n_tiles + 3) / 4, 8192, grid_cap);
    const bool aligned = (uintptr_t)p.in % 16 == 0 && p.stride_draw % kVec == 0 && vec_pitch % kVec == 0;
    if (aligned) PLA_MIXIS_LAUNCH((mixis_c_line_kernel<T, kVec>), grid, 256);
    else PLA_MIXIS_LAUNCH((mixis_c_line_kernel<T, 1>), grid, 256);
    snprintf(route, cap, "mixis_c_line_kernel<%s, %d>", tn, aligned ? kVec : 1);
  } else {
    PLA_MIXIS_LAUNCH((mixis_c_tile_kernel<T, false>), capped(n_db * p.n_tiles, 4096, grid_cap), 256);
    snprintf(route, cap, "mixis_c_tile_kernel<%s, strided>", tn);
  }
  return hipSuccess;
}

hipError_t launch_mixis_c(const void* in, int dtype, int64_t n_rows, int n_draws, int64_t stride_obs, int64_t stride_draw,
                          int64_t n_obs, int64_t row0, int64_t vec_pitch, double* part, unsigned long long* replaced, int grid_cap,
                          hipStream_t stream, char* route, int cap) {
  const int64_t t = mixis_tile_rows(n_obs);
  MixisParams p{in, n_rows, n_draws, stride_obs, stride_draw, t, (n_rows + t - 1) / t, row0 / t, mixis_n_tiles(n_obs), part, nullptr,
                nullptr, nullptr, nullptr, replaced};
  return dtype == PLA_F64 ? launch_mixis_c_typed<double>(p, vec_pitch, grid_cap, stream, route, cap)
                          : launch_mixis_c_typed<float>(p, vec_pitch, grid_cap, stream, route, cap);
}

hipError_t launch_mixis_c_merge(const double* part, int64_t n_obs, int n_draws, double* c, int grid_cap, hipStream_t stream) {
  MixisParams p{nullptr, n_obs, n_draws, 0, 0, mixis_tile_rows(n_obs), 0, 0, mixis_n_tiles(n_obs), const_cast<double*>(part), c, nullptr,
                nullptr, nullptr, nullptr};
  PLA_MIXIS_LAUNCH(mixis_c_merge_kernel, capped((n_draws + 255) / 256, 1024, grid_cap), 256);
  return hipSuccess;
}

hipError_t launch_mixis_lse_c(const double* c, int n_draws, double* lse_c, hipStream_t stream) {
  MixisParams p{nullptr, 0, n_draws, 0, 0, 0, 0, 0, 0, nullptr, nullptr, c, lse_c, nullptr, nullptr};
  PLA_MIXIS_LAUNCH(mixis_lse_c_kernel, 1, 256);
  return hipSuccess;
}

template <typename T>
static hipError_t launch_mixis_elpd_typed(const MixisParams& p, int grid_cap, hipStream_t stream, char* route, int cap) {
  constexpr int kVec = 16 / (int)sizeof(T);
  const char* tn = sizeof(T) == 8 ? "double" : "float";
  if (p.stride_draw == 1) {
    const bool aligned = (uintptr_t)p.in % 16 == 0 && p.stride_obs % kVec == 0 && p.n_draws % kVec == 0;
    if (p.n_draws <= kMixisRegDraws) {
      const unsigned grid = capped((p.n_obs + kWavesPerBlock - 1) / kWavesPerBlock, 1024, grid_cap);
      if (aligned) PLA_MIXIS_LAUNCH((mixis_row_wave_kernel<T, kVec>), grid, kWave * kWavesPerBlock);
      else PLA_MIXIS_LAUNCH((mixis_row_wave_kernel<T, 1>), grid, kWave * kWavesPerBlock);
      snprintf(route, cap, "mixis_row_wave_kernel<%s, %d>", tn, aligned ? kVec : 1);
    } else {
      const unsigned grid = capped((p.n_obs + 3) / 4, 8192, grid_cap);
      const bool al = (uintptr_t)p.in % 16 == 0 && p.stride_obs % kVec == 0;  // (the draws behind the last whole vector: single loads)
      if (al) PLA_MIXIS_LAUNCH((mixis_row_stream_kernel<T, kVec>), grid, 256);
      else PLA_MIXIS_LAUNCH((mixis_row_stream_kernel<T, 1>), grid, 256);
      snprintf(route, cap, "mixis_row_stream_kernel<%s, %d>", tn, al ? kVec : 1);
    }
  } else if (p.stride_obs == 1) {
    PLA_MIXIS_LAUNCH((mixis_col_kernel<T>), capped((p.n_obs + 255) / 256, 8192, grid_cap), 256);
    snprintf(route, cap, "mixis_col_kernel<%s>", tn);
  } else {
    PLA_MIXIS_LAUNCH((mixis_row_block_kernel<T>), capped(p.n_obs, 8192, grid_cap), 256);
    snprintf(route, cap, "mixis_row_block_kernel<%s>", tn);
  }
  return hipSuccess;
}

hipError_t launch_mixis_elpd(const void* in, int dtype, int64_t n_obs, int n_draws, int64_t stride_obs, int64_t stride_draw,
                             const double* c, const double* lse_c, double* elpd, unsigned long long* replaced, int grid_cap,
                             hipStream_t stream, char* route, int cap) {
  MixisParams p{in, n_obs, n_draws, stride_obs, stride_draw, 0, 0, 0, 0, nullptr, nullptr, c, const_cast<double*>(lse_c), elpd, replaced};
  return dtype == PLA_F64 ? launch_mixis_elpd_typed<double>(p, grid_cap, stream, route, cap)
                          : launch_mixis_elpd_typed<float>(p, grid_cap, stream, route, cap);
}

// agg[PLA_AGG_N_SLOW] = the entries pass 2 replaced (behind the k-fold finishing pass, which leaves the slot 0); counts[2] = them
__global__ void mixis_counts_kernel(const unsigned long long* replaced, double* agg, int64_t* counts) {
  if (agg) {
    agg[PLA_AGG_N_NONFINITE] = 0.0;
    agg[PLA_AGG_N_SLOW] = (double)(replaced[0] + replaced[1]);
  }
  if (counts) {
    counts[0] = (int64_t)replaced[0];
    counts[1] = (int64_t)replaced[1];
  }
}

hipError_t launch_mixis_counts(const unsigned long long* replaced, double* agg, int64_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL(mixis_counts_kernel, dim3(1), dim3(1), 0, stream, replaced, agg, counts);
  return hipGetLastError();
}

}  // namespace pla
