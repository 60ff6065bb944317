// launchers of the LOO influence kernels (pla_influence.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include <cstdio>

#include "pla_influence.h"
#include "pla_launch.h"

namespace pla {

static unsigned influence_grid(int64_t want, int64_t cap) {
  const int64_t g = want < cap ? want : cap;
  return (unsigned)(g < 1 ? 1 : g);
}

#define PLA_INF_LAUNCH(kernel, grid, block)                            \
  do {                                                                 \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, p); \
    const hipError_t e_ = hipGetLastError();                           \
    if (e_ != hipSuccess) return e_;                                   \
  } while (0)

// column tiles of a panel: one for up to 16 quantities, two up to 32, four (64 quantities) beyond
static int influence_panel_tiles(int n_quant) { return n_quant <= kInfTile ? 1 : n_quant <= 2 * kInfTile ? 2 : 4; }

void influence_pads(int n_draws, int n_quant, int* s_pad, int* p_pad) {
  const int w = kInfTile * influence_panel_tiles(n_quant);
  *s_pad = (n_draws + kInfK - 1) / kInfK * kInfK;
  *p_pad = (n_quant + w - 1) / w * w;
}

hipError_t launch_influence_prepare(const double* theta, int64_t stride_draw, int64_t stride_quant, const double* center, const double* scale,
                                    int n_draws, int n_quant, double* zt, hipStream_t stream) {
  if (n_draws <= 0 || n_quant <= 0) return hipSuccess;
  InfPrepareParams p{theta, stride_draw, stride_quant, center, scale, n_draws, n_quant, 0, 0, zt};
  influence_pads(n_draws, n_quant, &p.s_pad, &p.p_pad);
  PLA_INF_LAUNCH(influence_prepare_kernel, influence_grid(((int64_t)p.s_pad * p.p_pad + 255) / 256, 8192), 256);
  return hipSuccess;
}

template <typename T, int MODE>
static hipError_t launch_influence_mode(const InfParams& p, int nct, hipStream_t stream) {
  const unsigned grid = influence_grid(((p.n_obs + kInfTile - 1) / kInfTile + kInfWaves - 1) / kInfWaves, 4096);
  if (nct == 1) PLA_INF_LAUNCH((influence_kernel<T, MODE, 1>), grid, kWave * kInfWaves);
  else if (nct == 2) PLA_INF_LAUNCH((influence_kernel<T, MODE, 2>), grid, kWave * kInfWaves);
  else PLA_INF_LAUNCH((influence_kernel<T, MODE, 4>), grid, kWave * kInfWaves);
  return hipSuccess;
}

template <typename T>
static hipError_t launch_influence_typed(const InfParams& p, hipStream_t stream, char* route, int cap) {
  constexpr int kVec = 16 / (int)sizeof(T);
  const bool vec = p.lw_sd == 1 && (uintptr_t)p.lw % 16 == 0 && (p.n_obs == 1 || p.lw_so % kVec == 0) && p.n_draws % kVec == 0;
  const int nct = influence_panel_tiles(p.n_quant);
  const hipError_t e = vec ? launch_influence_mode<T, kInfVec>(p, nct, stream) : launch_influence_mode<T, kInfElem>(p, nct, stream);
  if (route)
    snprintf(route, cap, "influence_kernel<%s, %s, %d column tiles>", sizeof(T) == 8 ? "double" : "float",
             vec ? "16-byte loads" : "element loads", nct);
  return e;
}

hipError_t launch_influence(const void* lw, int dtype, int64_t n_obs, int n_draws, int64_t lw_stride_obs, int64_t lw_stride_draw,
                            const double* zt, int n_quant, double* shift, double* m2, double* kl, double* ess_w,
                            hipStream_t stream, char* route, int cap) {
  if (route && cap > 0) route[0] = 0;
  if (n_obs <= 0 || n_draws <= 0 || n_quant <= 0) return hipSuccess;
  InfParams p{lw, n_obs, n_draws, lw_stride_obs, lw_stride_draw, zt, 0, 0, n_quant, shift, m2, kl, ess_w};
  influence_pads(n_draws, n_quant, &p.s_pad, &p.p_pad);
  return dtype == PLA_F64 ? launch_influence_typed<double>(p, stream, route, cap) : launch_influence_typed<float>(p, stream, route, cap);
}

}  // namespace pla
