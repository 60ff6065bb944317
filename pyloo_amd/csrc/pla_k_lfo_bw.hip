// launchers of the backward leave-future-out kernels (pla_lfo_bw.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdio>

#include "pla_lfo_bw.h"
#include "pla_launch.h"

namespace pla {

static unsigned lfo_bw_grid(int64_t want, int64_t cap) {
  const int64_t g = want < cap ? want : cap;
  return (unsigned)(g < 1 ? 1 : g);
}

#define PLA_LFO_BW_LAUNCH(kernel, grid, block, ...)                              \
  do {                                                                           \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                                     \
    if (e_ != hipSuccess) return e_;                                             \
  } while (0)

template <typename T, bool VEC>
static hipError_t launch_lfo_bw_scan_typed(LfoBwScanParams p, int64_t n_totals, bool write, double* run, hipStream_t stream) {
  constexpr int W = VEC ? 16 / (int)sizeof(T) : 1;
  const int S = p.n_draws;
  const int64_t n_db = (S + W * 256 - 1) / (W * 256);
  const int64_t n_chunks = p.n_chunks;
  if (n_totals > 0) {  // totals of the chunks that have a successor (here or in the next block): all their rows exist
    LfoBwScanParams t = p;
    t.n_chunks = n_totals;
    t.n_load = n_totals * kLfoChunk;
    PLA_LFO_BW_LAUNCH((lfo_bw_scan_kernel<T, VEC, false>), lfo_bw_grid(n_totals * n_db, (int64_t)1 << 22), 256, t);
  }
  const hipError_t e = launch_lfo_carry(p.carry, run, n_chunks, n_totals, S, stream);  // (forward mode's kernel: the same rule in q)
  if (e != hipSuccess) return e;
  if (write)  // (a block that lies before the first step of the pass only passes its carry on)
    PLA_LFO_BW_LAUNCH((lfo_bw_scan_kernel<T, VEC, true>), lfo_bw_grid(n_chunks * n_db, (int64_t)1 << 22), 256, p);
  return hipSuccess;
}

hipError_t launch_lfo_bw_ratios(const void* in, int dtype, int64_t stride_obs, int n_draws, int64_t n_rows, int64_t n_load, bool last_block,
                                bool write, double* carry, double* run, double* out, hipStream_t stream, const char** route) {
  if (n_rows <= 0 || n_draws <= 0) return hipSuccess;
  const int64_t n_chunks = (n_rows + kLfoChunk - 1) / kLfoChunk;
  const int64_t n_totals = last_block ? n_chunks - 1 : n_chunks;
  LfoBwScanParams p{in, stride_obs, n_draws, n_chunks, n_rows, n_load, carry, out};
  const int vec = dtype == PLA_F64 ? 2 : 4;
  const bool aligned = (uintptr_t)in % 16 == 0 && stride_obs % vec == 0 && n_draws % vec == 0 && (uintptr_t)out % 16 == 0 &&
                       (uintptr_t)carry % 16 == 0;
  if (route)
    *route = dtype == PLA_F64 ? (aligned ? "lfo_bw_scan_kernel<double, 16-byte loads>" : "lfo_bw_scan_kernel<double, element loads>")
                              : (aligned ? "lfo_bw_scan_kernel<float, 16-byte loads>" : "lfo_bw_scan_kernel<float, element loads>");
  if (dtype == PLA_F64)
    return aligned ? launch_lfo_bw_scan_typed<double, true>(p, n_totals, write, run, stream)
                   : launch_lfo_bw_scan_typed<double, false>(p, n_totals, write, run, stream);
  return aligned ? launch_lfo_bw_scan_typed<float, true>(p, n_totals, write, run, stream)
                 : launch_lfo_bw_scan_typed<float, false>(p, n_totals, write, run, stream);
}

template <typename T, bool VEC>
static hipError_t launch_lfo_bw_predict_typed(const LfoBwPredictParams& p, hipStream_t stream) {
  const unsigned grid = lfo_bw_grid((p.n_steps + kLfoWaves - 1) / kLfoWaves, 8192);
  if (p.n_draws <= kLfoRegDraws) PLA_LFO_BW_LAUNCH((lfo_bw_predict_kernel<T, VEC, true>), grid, kWave * kLfoWaves, p);
  else PLA_LFO_BW_LAUNCH((lfo_bw_predict_kernel<T, VEC, false>), grid, kWave * kLfoWaves, p);
  return hipSuccess;
}

hipError_t launch_lfo_bw_predict(const double* lw, const void* ll, int dtype, int64_t ll_stride_obs, int64_t n_steps, int n_draws,
                                 int horizon, bool pass_start, bool exact0, double* diag, double* elpd, unsigned long long* replaced,
                                 hipStream_t stream, char* route, int cap) {
  if (route && cap > 0) route[0] = 0;
  if (n_steps <= 0 || n_draws <= 0) return hipSuccess;
  LfoBwPredictParams p{lw, ll, ll_stride_obs, n_steps, n_draws, horizon, pass_start ? 1 : 0, exact0 ? 1 : 0, diag, elpd, replaced};
  const int vec = dtype == PLA_F64 ? 2 : 4;
  const bool aligned = (uintptr_t)ll % 16 == 0 && ll_stride_obs % vec == 0 && n_draws % vec == 0 && (uintptr_t)lw % 16 == 0;
  if (route)
    snprintf(route, cap, "lfo_bw_predict_kernel<%s, %s, %s>", dtype_name(dtype), aligned ? "16-byte loads" : "element loads",
             n_draws <= kLfoRegDraws ? "registers" : "streamed");
  if (dtype == PLA_F64)
    return aligned ? launch_lfo_bw_predict_typed<double, true>(p, stream) : launch_lfo_bw_predict_typed<double, false>(p, stream);
  return aligned ? launch_lfo_bw_predict_typed<float, true>(p, stream) : launch_lfo_bw_predict_typed<float, false>(p, stream);
}

hipError_t launch_lfo_bw_first_high(const double* diag, int64_t n_steps, int64_t j_min, double threshold, long long* out,
                                    hipStream_t stream) {
  PLA_LFO_BW_LAUNCH(lfo_bw_first_high_kernel, 1, 256, diag, n_steps, j_min, threshold, out);
  return hipSuccess;
}

}  // namespace pla
