// GLM log-likelihood generator: a block of the (n_obs, n_draws) matrix from the design matrix X (N x P), the coefficient draws
// beta (S x P) and the family, never the matrix as a whole.  All arithmetic is f64.
//     eta[i, s] = acc[i, s] + offset_i,   acc = the MFMA chain sum_p x[i, p] beta[s, p] started from zero
//     PLA_GLM_LINPRED          eta
//     PLA_GLM_GAUSSIAN         draw_const_s - 0.5 ((y_i - eta) / sigma_s)^2            (a division)
//     PLA_GLM_BINOMIAL_LOGIT   obs_const_i + y_i eta - trials_i softplus(eta),  softplus(e) = max(e, 0) + log1p(exp(-|e|))
//     PLA_GLM_POISSON_LOG      obs_const_i + y_i eta - exp(eta)
//     PLA_GLM_NEGBINOMIAL_LOG  (((obs_const_i + draw_const_s) + lgamma(y_i + phi_s)) + y_i eta) - (y_i + phi_s) L,
//                              L = max(eta, lp_s) + log1p(exp(-|eta - lp_s|)), phi_s = sigma_s, lp_s = log(phi_s) once per tile of draws
//     PLA_GLM_GAMMA_LOG        (draw_const_s + (alpha_s - 1) obs_const_i) - alpha_s (eta + y_i exp(-eta)),  alpha_s = sigma_s
//     PLA_GLM_BINOMIAL_PROBIT  (obs_const_i + y_i logPhi(eta)) + (trials_i - y_i) logPhi(-eta), a product with a zero factor not formed;
//                              glm_log_ndtr_pair: with h = 0.5 erfcx(|e| / sqrt 2), w = 0.5 fl(e^2), r = e^2 - fl(e^2): logPhi(-|e|) = log(h) - w, logPhi(|e|) = log1p(-(h exp(-w)) (1 - 0.5 r))
// (the last three are instantiated in pla_k_glm_families.hip and pla_k_glm_terms_families.hip; lgamma and erfcx are the device library's)
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
  const double *sigma, *draw_const;               // [n_draws], the families of glm_draw_values
  double* out;                                    // (n_rows, n_draws) with row pitch `pitch`, draws fastest
  int64_t pitch;
  unsigned long long* replaced;  // non-null: NaN -> -1e10, counted here
  int n_strips, strip_tiles;     // a wavefront's strip: strip_tiles tiles of draws; n_strips strips cover s_pad
};

// the kernel's parameters of a launch and its grid (pla_k_glm.hip; shared with the flavour with group-level terms, pla_glm_terms.h)
unsigned glm_fill_params(const GlmLaunch& g, GlmParams* out);
// the families pla_k_glm.hip does not instantiate (pla_k_glm_families.hip); *name: the family as the route text names it
hipError_t launch_glm_more(int family, const GlmParams& p, unsigned grid, hipStream_t stream, const char** name);

// what a family reads: a scale and a constant per draw; trials per observation; a constant per observation
constexpr bool glm_draw_values(int fam) { return fam == PLA_GLM_GAUSSIAN || fam == PLA_GLM_NEGBINOMIAL_LOG || fam == PLA_GLM_GAMMA_LOG; }
constexpr bool glm_has_trials(int fam) { return fam == PLA_GLM_BINOMIAL_LOGIT || fam == PLA_GLM_BINOMIAL_PROBIT; }
constexpr bool glm_has_obs_const(int fam) { return fam != PLA_GLM_LINPRED && fam != PLA_GLM_GAUSSIAN; }

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

// logPhi(-|e|) and logPhi(|e|), Phi the standard normal distribution function, from one scaled complementary error function:
// Phi(-|e|) = h exp(-w) with h = 0.5 erfcx(|e| / sqrt 2) and w = 0.5 e^2.  The lower tail is log(h) - w, finite and accurate where
// log(0.5 erfc) underflows (below -38); the upper is log1p(-h exp(-w)).  erfcx varies slowly, so the rounding of |e| / sqrt 2 costs
// an ulp.  The rounding of e^2 would enter exp(-w) as a relative error of w ulp -- erfc(|e| / sqrt 2) takes twice that from its
// rounded argument -- and with y = trials the upper tail is all there is of ll: the square's remainder r = e^2 - fl(e^2), exact from
// one fused multiply-add, is put back as the factor 1 - r / 2 (its own square is below 1e-26).
__device__ __forceinline__ void glm_log_ndtr_pair(double eta, double* lower, double* upper) {
#pragma clang fp contract(off)
  const double h = 0.5 * erfcx(fabs(eta) * 0.70710678118654752440);
  const double sq = eta * eta;
  const double r = sq < HUGE_VAL ? fma(eta, eta, -sq) : 0.0;
  const double w = 0.5 * sq;
  *lower = log(h) - w;
  *upper = log1p(-((h * exp(-w)) * (1.0 - 0.5 * r)));
}

// log_scale: log(sigma), PLA_GLM_NEGBINOMIAL_LOG alone
template <int FAM>
__device__ __forceinline__ double glm_density(double eta, double y, double trials, double obs_const, double sigma, double draw_const,
                                              double log_scale = 0.0) {
#pragma clang fp contract(off)
  if constexpr (FAM == PLA_GLM_GAUSSIAN) {
    const double t = (y - eta) / sigma;
    return draw_const - 0.5 * (t * t);
  } else if constexpr (FAM == PLA_GLM_BINOMIAL_LOGIT) {
    const double sp = fmax(eta, 0.0) + log1p(exp(-fabs(eta)));
    return (obs_const + y * eta) - trials * sp;
  } else if constexpr (FAM == PLA_GLM_POISSON_LOG) {
    return (obs_const + y * eta) - exp(eta);
  } else if constexpr (FAM == PLA_GLM_NEGBINOMIAL_LOG) {
    const double yp = y + sigma;
    const double L = fmax(eta, log_scale) + log1p(exp(-fabs(eta - log_scale)));
    return (((obs_const + draw_const) + lgamma(yp)) + y * eta) - yp * L;
  } else if constexpr (FAM == PLA_GLM_GAMMA_LOG) {
    return (draw_const + (sigma - 1.0) * obs_const) - sigma * (eta + y * exp(-eta));
  } else if constexpr (FAM == PLA_GLM_BINOMIAL_PROBIT) {
    double lower, upper;
    glm_log_ndtr_pair(eta, &lower, &upper);
    const bool neg = eta < 0.0;
    const double m = trials - y;
    const double a = y != 0.0 ? y * (neg ? lower : upper) : 0.0;
    const double b = m != 0.0 ? m * (neg ? upper : lower) : 0.0;
    return (obs_const + a) + b;
  } else {
    return eta;
  }
}

// The families whose density holds a special function (lgamma; erfc and erfcx) take the lane's four rows one after the other, in a
// loop that is not unrolled: four inlined copies of such a function hold more polynomial coefficients in scalar registers than the
// file has (they spill into vector lanes, and under the terms kernel's register cap into scratch) and quadruple the code.  The
// loop works on entry 0 of the rows' values and rotates them by one entry per turn -- moves between registers, no indexed register
// and no lane mask per entry; after the four turns every array stands as it stood.
constexpr bool glm_rolled(int fam) { return fam == PLA_GLM_NEGBINOMIAL_LOG || fam == PLA_GLM_BINOMIAL_PROBIT; }

__device__ __forceinline__ void glm_rotate(double (&v)[4]) {
  const double first = v[0];
  v[0] = v[1];
  v[1] = v[2];
  v[2] = v[3];
  v[3] = first;
}

// the density of the lane's four rows, the NaN rule and the stores of a tile; returns the NaN entries replaced
template <int FAM>
__device__ __forceinline__ unsigned glm_rolled_epilogue(const GlmParams& P, double (&eta)[4], double (&yv)[4], double (&tv)[4], double (&cv)[4],
                                                        double sig, double dc, double lsc, int64_t r0, int q, int s, bool s_ok) {
  unsigned n_nan = 0;
  // (the lane's address, its step and its rows left in vector registers: the loop holds no scalar of the launch but the counter's flag)
  double* at = P.out + ((r0 + q) * P.pitch + s);
  int64_t step = 4 * P.pitch, left = s_ok ? P.n_rows - (r0 + q) : 0;
  asm volatile("" : "+v"(step), "+v"(left));
  const bool count = P.replaced != nullptr;
#pragma unroll 1
  for (int g = 0; g < 4; ++g) {
    double ll = glm_density<FAM>(eta[0], yv[0], tv[0], cv[0], sig, dc, lsc);
    glm_rotate(eta);
    glm_rotate(yv);
    if constexpr (glm_has_trials(FAM)) glm_rotate(tv);
    glm_rotate(cv);
    if (left > 0) {
      if (count && ll != ll) {
        ll = -1e10;
        n_nan += 1;
      }
      *at = ll;
    }
    at += step;
    left -= 4;
  }
  return n_nan;
}

// the MFMA chain of one tile: observations of the lane's row of X (a: its operands, reloaded per panel on the PANEL route) times
// the 16 draws from s - (s & 15) on, all p_pad predictors in one order, started from zero
// (shared with the predictive kernel, pla_glm_predict.h: the same chain gives the same bits)
template <int NCH, bool PANEL>
__device__ __forceinline__ glm_v4d glm_tile_chain(const GlmParams& P, const double* xr, double (&a)[NCH * 4], int q, int s, int n_panels) {
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
  return acc;
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
      tv[g] = glm_has_trials(FAM) && P.trials ? P.trials[src] : 1.0;
      cv[g] = glm_has_obs_const(FAM) && P.obs_const ? P.obs_const[src] : 0.0;
    }
    const int t_end = (st + 1) * P.strip_tiles < n_dtiles ? (st + 1) * P.strip_tiles : n_dtiles;
#pragma unroll 1
    for (int dt = st * P.strip_tiles; dt < t_end; ++dt) {
      const int s = dt * kGlmTile + i;  // this lane's draw: B column and C / D column (s < s_pad)
      glm_v4d acc = glm_tile_chain<NCH, PANEL>(P, xr, a, q, s, n_panels);
      // ---- epilogue: C / D col = lane & 15 (the draw), row = (lane >> 4) + 4 reg
      const bool s_ok = s < S;
      double sig = 1.0, dc = 0.0, lsc = 0.0;
      if constexpr (glm_draw_values(FAM)) {
        sig = P.sigma[s_ok ? s : S - 1];
        dc = P.draw_const[s_ok ? s : S - 1];
      }
      if constexpr (FAM == PLA_GLM_NEGBINOMIAL_LOG) lsc = log(sig);
      if constexpr (glm_rolled(FAM)) {
        double eta[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) eta[g] = acc[g] + ov[g];
        n_nan += glm_rolled_epilogue<FAM>(P, eta, yv, tv, cv, sig, dc, lsc, r0, q, s, s_ok);
        continue;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma clang fp contract(off)
        const double eta = acc[g] + ov[g];
        double ll = glm_density<FAM>(eta, yv[g], tv[g], cv[g], sig, dc, lsc);
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

// the instantiation of a family for the padded predictor count of a launch
template <int FAM>
inline hipError_t glm_launch_family(const GlmParams& p, unsigned grid, hipStream_t stream) {
  const dim3 block(kWave * kGlmWaves);
  if (p.p_pad > kGlmK * kGlmPanel) hipLaunchKernelGGL((glm_kernel<FAM, kGlmPanel, true>), dim3(grid), block, 0, stream, p);
  else if (p.p_pad == kGlmK * 8) hipLaunchKernelGGL((glm_kernel<FAM, 8, false>), dim3(grid), block, 0, stream, p);
  else if (p.p_pad == kGlmK * 4) hipLaunchKernelGGL((glm_kernel<FAM, 4, false>), dim3(grid), block, 0, stream, p);
  else if (p.p_pad == kGlmK * 2) hipLaunchKernelGGL((glm_kernel<FAM, 2, false>), dim3(grid), block, 0, stream, p);
  else hipLaunchKernelGGL((glm_kernel<FAM, 1, false>), dim3(grid), block, 0, stream, p);
  return hipGetLastError();
}

}  // namespace pla
