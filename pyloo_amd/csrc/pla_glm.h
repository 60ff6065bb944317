// GLM log-likelihood generator: a block of the (n_obs, n_draws) matrix from the design matrix X (N x P), the coefficient draws
// beta (S x P) and the family, never the matrix as a whole.  All arithmetic is f64.
//     eta[i, s] = acc[i, s] + offset_i,   acc = the MFMA chain sum_p x[i, p] beta[s, p] started from zero
//     PLA_GLM_LINPRED          eta
//     PLA_GLM_GAUSSIAN         draw_const_s - 0.5 ((y_i - eta) / sigma_s)^2            (a division)
//     PLA_GLM_BINOMIAL_LOGIT   obs_const_i + y_i eta - trials_i softplus(eta),  softplus(e) = max(e, 0) + log1p(exp(-|e|))
//     PLA_GLM_POISSON_LOG      obs_const_i + y_i eta - exp(eta)
// offset, trials and obs_const may be null (0, 1, 0).  Values that are not finite propagate by IEEE rules; with a counter given
// (the LOO route) a NaN result is stored as -1e10 and counted (loo.py:218-227).
//
// PREPARE.  glm_prepare_kernel writes the image of beta, bimg[s_pad][p_pad], zero for s >= n_draws and p >= n_pred, once per call,
// and kGlmImagePad zeros behind it (what a predictor past P is read from);
// beta is read with any positive strides, (S, P) or a .T view.
//
// GLM.  glm_kernel<FAM, NCH, PANEL>: one wavefront per tile of 16 observations x 16 draws on v_mfma_f64_16x16x4f64.
//   operands     lane l = (i = l & 15, q = l >> 4) gives A[i][k] = x of observation i and B[k][i] = beta of draw i, both of the
//                k-quarter q (pla_nonfactor.h:329-337).  A K chunk is kGlmK = 16 consecutive predictors; quarter q owns predictors
//                4q .. 4q + 3 of it and MFMA step t multiplies predictor 4q + t of every quarter: a permutation of the predictors
//                that A and B share (pla_influence.h), in which a lane's operands of a chunk are 32 consecutive bytes of bimg.
//   A            X rows read in place with their own strides, gathered through row_index, clamped on load (rows past the block,
//                predictors past P enter as 0 against bimg's zero padding).  NCH chunks of a row stay in registers across the
//                wavefront's strip of draw tiles (P <= 16 NCH, NCH = 1, 2, 4, 8); PANEL (P > 128) walks K in panels of 8 chunks,
//                reloading the panel per draw tile, the accumulator carried through: the same chain in the same order.
//   C / D        col = lane & 15 is the draw, row = (lane >> 4) + 4 reg the observation: one accumulator register stores 16
//                consecutive draws of a row, 128 bytes, draws fastest.
//   epilogue     on the accumulator registers, fp contract(off); the per-observation values of the lane's four rows are loaded once
//                per tile of observations, the per-draw values once per tile of draws.
// eta[i, s] and ll[i, s] are functions of row i of X, row s of beta, P and the vectors' entries alone: a row of the MFMA result is a
// function of that row of A, a column of that column of B, the chain runs over p_pad(P) predictors in one order, K is never split
// across wavefronts and there are no floating-point atomics -- nothing depends on the grid, the strip, the block, the position of
// a row or a draw in its tile, the row list or the strides.
#pragma once

#include "../../include/pyloo_amd.h"
#include "pla_device.h"
#include "pla_kernels.h"

namespace pla {

constexpr int kGlmK = 16;      // predictors per K chunk: four MFMA steps, four consecutive predictors per lane
constexpr int kGlmTile = 16;   // observations / draws per MFMA tile
constexpr int kGlmWaves = 4;   // wavefronts per workgroup
constexpr int kGlmPanel = 8;   // chunks per panel of the PANEL route

typedef double glm_v4d __attribute__((ext_vector_type(4)));

struct GlmPrepareParams {
  const double* beta;  // n_draws x n_pred with strides (st_draw, st_pred), elements
  int64_t st_draw, st_pred;
  int n_draws, n_pred;
  int s_pad, p_pad;
  double* bimg;  // [s_pad][p_pad], and kGlmImagePad zeros behind it
};

struct GlmParams {
  const double* x;  // n_src x n_pred with strides (sx_obs, sx_pred), elements
  int64_t sx_obs, sx_pred;
  int64_t n_src;             // rows of X (and entries of the per-observation vectors)
  const int64_t* row_index;  // [n_rows] source rows of this launch, or null: rows r_first .. r_first + n_rows - 1
  int64_t r_first;
  int64_t n_rows;
  const double* bimg;  // [s_pad][p_pad]
  const double* zero;  // a 0.0 (the slot behind bimg)
  int s_pad, p_pad, n_pred, n_draws;
  const double *y, *offset, *trials, *obs_const;  // [n_src]; the last three may be null
  const double *sigma, *draw_const;               // [n_draws], PLA_GLM_GAUSSIAN
  double* out;                                    // (n_rows, n_draws) with row pitch `pitch`, draws fastest
  int64_t pitch;
  unsigned long long* replaced;  // non-null: NaN -> -1e10, counted here
  int n_strips, strip_tiles;     // a wavefront's strip: strip_tiles tiles of draws; n_strips strips cover s_pad
};

// the kernel's parameters of a launch and its grid (pla_k_glm.hip; shared with the flavour with group-level terms, pla_glm_terms.h)
unsigned glm_fill_params(const GlmLaunch& g, GlmParams* out);

#ifndef PLA_GLM_SHARED_ONLY  // (pla_k_glm_terms.hip takes the shared parts; this kernel is pla_k_glm.hip's)
__global__ __launch_bounds__(256) void glm_prepare_kernel(GlmPrepareParams P) {
  const int64_t total = (int64_t)P.s_pad * P.p_pad + kGlmImagePad;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int s = (int)(e / P.p_pad);
    const int p = (int)(e - (int64_t)s * P.p_pad);
    double b = 0.0;  // (the pad behind the image: s >= s_pad)
    if (s < P.n_draws && p < P.n_pred) b = P.beta[(int64_t)s * P.st_draw + (int64_t)p * P.st_pred];
    P.bimg[e] = b;
  }
}
#endif

// the source row of row r of the launch, clamped to the block and to X
__device__ __forceinline__ int64_t glm_source_row(const GlmParams& P, int64_t r) {
  r = r < P.n_rows ? r : P.n_rows - 1;
  if (!P.row_index) return P.r_first + r;
  const int64_t v = P.row_index[r];
  return v < 0 ? 0 : v < P.n_src ? v : P.n_src - 1;
}

// a lane's A operands of NCH chunks from predictor p0 on: 0 past P -- read from the zero behind bimg, the address chosen by
// arithmetic inside the loop.  (A compare per operand is loop-invariant: hoisted out of the loop over the tiles, 32 lane masks --
// or as many scalar element offsets -- spill the SGPR file into vector lanes; hence the opaque p and the walking pointer.)
template <int NCH>
__device__ __forceinline__ void glm_load_x(const double* xr, const double* zero, int64_t sp, int p0, int q, int n_pred, double (&a)[NCH * 4]) {
  const double* at = xr + (int64_t)(p0 + 4 * q) * sp;
  const int64_t skip = (kGlmK - 4) * sp;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int p = p0 + c * kGlmK + 4 * q + k;
      asm volatile("" : "+v"(p));  // (not hoisted out of the loop over the tiles as a lane mask per operand)
      const intptr_t past = (intptr_t)((n_pred - 1 - p) >> 31);  // all ones for p >= n_pred
      a[c * 4 + k] = *reinterpret_cast<const double*>((intptr_t)at + (((intptr_t)zero - (intptr_t)at) & past));
      at += sp;
      asm volatile("" : "+v"(at));
    }
    at += skip;
  }
}

template <int FAM>
__device__ __forceinline__ double glm_density(double eta, double y, double trials, double obs_const, double sigma, double draw_const) {
#pragma clang fp contract(off)
  if constexpr (FAM == PLA_GLM_GAUSSIAN) {
    const double t = (y - eta) / sigma;
    return draw_const - 0.5 * (t * t);
  } else if constexpr (FAM == PLA_GLM_BINOMIAL_LOGIT) {
    const double sp = fmax(eta, 0.0) + log1p(exp(-fabs(eta)));
    return (obs_const + y * eta) - trials * sp;
  } else if constexpr (FAM == PLA_GLM_POISSON_LOG) {
    return (obs_const + y * eta) - exp(eta);
  } else {
    return eta;
  }
}

template <int FAM, int NCH, bool PANEL>
__global__ __launch_bounds__(kWave * kGlmWaves) void glm_kernel(GlmParams P) {
  const int S = P.n_draws;
  const int lane = threadIdx.x & (kWave - 1), i = lane & 15, q = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int n_dtiles = P.s_pad / kGlmTile;
  const int n_panels = PANEL ? P.p_pad / (kGlmK * NCH) : 1;
  const int64_t n_units = (P.n_rows + kGlmTile - 1) / kGlmTile * P.n_strips;
  const int64_t nw = (int64_t)gridDim.x * kGlmWaves;
  unsigned long long n_nan = 0;
  for (int64_t u = (int64_t)blockIdx.x * kGlmWaves + wv; u < n_units; u += nw) {
    const int64_t rt = u / P.n_strips;
    const int st = (int)(u - rt * P.n_strips);
    const int64_t r0 = rt * kGlmTile;
    // ---- A: this lane's row of X
    const double* xr = P.x + glm_source_row(P, r0 + i) * P.sx_obs;
    double a[NCH * 4];
    if constexpr (!PANEL) glm_load_x<NCH>(xr, P.zero, P.sx_pred, 0, q, P.n_pred, a);
    // ---- the per-observation values of this lane's four rows of C / D
    double yv[4], ov[4], tv[4], cv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t src = glm_source_row(P, r0 + q + 4 * g);
      ov[g] = P.offset ? P.offset[src] : 0.0;
      yv[g] = FAM != PLA_GLM_LINPRED ? P.y[src] : 0.0;
      tv[g] = FAM == PLA_GLM_BINOMIAL_LOGIT && P.trials ? P.trials[src] : 1.0;
      cv[g] = (FAM == PLA_GLM_BINOMIAL_LOGIT || FAM == PLA_GLM_POISSON_LOG) && P.obs_const ? P.obs_const[src] : 0.0;
    }
    const int t_end = (st + 1) * P.strip_tiles < n_dtiles ? (st + 1) * P.strip_tiles : n_dtiles;
#pragma unroll 1
    for (int dt = st * P.strip_tiles; dt < t_end; ++dt) {
      const int s = dt * kGlmTile + i;  // this lane's draw: B column and C / D column (s < s_pad)
      glm_v4d acc = glm_v4d{0.0, 0.0, 0.0, 0.0};
      const double* bp = P.bimg + (int64_t)s * P.p_pad + 4 * q;
#pragma unroll 1
      for (int pn = 0; pn < n_panels; ++pn) {
        if constexpr (PANEL) glm_load_x<NCH>(xr, P.zero, P.sx_pred, pn * NCH * kGlmK, q, P.n_pred, a);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const double* bc = bp + (pn * NCH + c) * kGlmK;
          const double2 ba = *reinterpret_cast<const double2*>(bc), bb = *reinterpret_cast<const double2*>(bc + 2);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[c * 4 + 0], ba.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[c * 4 + 1], ba.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[c * 4 + 2], bb.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[c * 4 + 3], bb.y, acc, 0, 0, 0);
        }
      }
      // ---- epilogue: C / D col = lane & 15 (the draw), row = (lane >> 4) + 4 reg
      const bool s_ok = s < S;
      double sig = 1.0, dc = 0.0;
      if constexpr (FAM == PLA_GLM_GAUSSIAN) {
        sig = P.sigma[s_ok ? s : S - 1];
        dc = P.draw_const[s_ok ? s : S - 1];
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma clang fp contract(off)
        const double eta = acc[g] + ov[g];
        double ll = glm_density<FAM>(eta, yv[g], tv[g], cv[g], sig, dc);
        const int64_t r = r0 + q + 4 * g;
        if (s_ok && r < P.n_rows) {
          if (P.replaced && ll != ll) {
            ll = -1e10;
            n_nan += 1;
          }
          P.out[r * P.pitch + s] = ll;
        }
      }
    }
  }
  if (P.replaced) {  // (an integer count: the order of the additions does not matter)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_nan += __shfl_xor(n_nan, d);
    if (lane == 0 && n_nan) atomicAdd(P.replaced, n_nan);
  }
}

}  // namespace pla
