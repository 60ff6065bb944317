// GLM log-likelihood generator with group-level terms (multilevel models): the tile kernel of pla_glm.h with
//     eta[i, s] = ((( acc[i, s] + offset_i ) + z_0[i] u_0[s, g_0[i]] ) + z_1[i] u_1[s, g_1[i]] ) + ...
// added to the accumulator registers before glm_density.  acc is the MFMA chain of pla_glm.h, unchanged; every product and every
// sum is rounded once (fp contract(off)), in the order of the terms; with z_t null the product is not formed.
//
// PREPARE.  glm_terms_prepare_kernel writes the image of the group effects, uimg[sum G_t][s_pad], once per call: group-major, draws
// fastest, zero for s >= n_draws; term t starts at row first[t].  u_t is read with any positive strides -- (S, G), a .T view, a
// padded pitch.  A wavefront moves a tile of 8 groups x 8 draws: 64 consecutive bytes on the side that is contiguous, either way.
// Indexing is 64-bit (sum G_t * s_pad passes 2^31 at a few hundred thousand groups).
//
// GLM.  glm_terms_kernel<FAM, NCH, PANEL>: lane (col = lane & 15, q) reads, for each of its four rows and each term,
// uimg[first_t + g][dt * 16 + col] -- the 16 lanes of a quarter read 128 consecutive bytes, rows of a tile that share a group hit
// the same lines.  The source rows of a lane's four rows stay in registers across the strip (8 registers); the group index and z of
// a row and a term are re-read from cache per tile of draws: with up to 8 terms they would be 96 registers, more than the
// instantiations with 8 chunks of predictors have left, and a term count known only at run time cannot index registers.  The
// indices of term t + 1 are loaded under the lines of term t (4 registers), so a term exposes one memory latency, not two.
//   clamping     rows past the block go through glm_source_row, their group index comes from the clamped source row; a group index
//                is clamped into [0, G_t) on load; draws s >= n_draws read the zero padding of the image (s < s_pad always).
// The order rule of pla_glm.h, extended: eta[i, s] depends on row i of X, row s of beta, the entries i of the vectors and of g_t,
// z_t, and on u_t[s, g_t[i]], in the order of the terms -- not on the grid, the strip, the block, the position in a tile, the row
// list, the strides, the labels of the groups or the memory space.  Reordering the terms reorders the additions.
// No LDS, no scratch, no floating-point atomics.
#pragma once

#include "pla_glm.h"

namespace pla {

struct GlmTermsPrepareParams {
  const double* u[kGlmMaxTerms];  // n_draws x G_t with strides (st_draw, st_group), elements
  int64_t st_draw[kGlmMaxTerms], st_group[kGlmMaxTerms];
  int64_t first[kGlmMaxTerms + 1];  // first image row of term t; [n_terms .. kGlmMaxTerms]: the number of rows
  int n_terms, n_draws, s_pad;
  double* uimg;  // [first[n_terms]][s_pad]
};

struct GlmTermsParams {
  GlmParams glm;
  const double* uimg;
  const int32_t* group[kGlmMaxTerms];  // [n_src]
  const double* z[kGlmMaxTerms];       // [n_src] or null (1)
  int64_t first[kGlmMaxTerms];
  int last_group[kGlmMaxTerms];  // G_t - 1
  int n_terms;
};

constexpr int kGlmTermsTile = 8;  // groups / draws per wavefront tile of the prepare pass

// the families pla_k_glm_terms.hip does not instantiate (pla_k_glm_terms_families.hip); *name: the family as the route text names it
hipError_t launch_glm_terms_more(int family, const GlmTermsParams& p, unsigned grid, hipStream_t stream, const char** name);

#ifndef PLA_GLM_TERMS_SHARED_ONLY  // (pla_k_glm_terms_families.hip takes the shared parts; this kernel is pla_k_glm_terms.hip's)
__global__ __launch_bounds__(256) void glm_terms_prepare_kernel(GlmTermsPrepareParams P) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t total = P.first[kGlmMaxTerms];
  const int64_t s_tiles = P.s_pad / kGlmTermsTile;
  const int64_t n_units = (total + kGlmTermsTile - 1) / kGlmTermsTile * s_tiles;
  const int64_t nw = (int64_t)gridDim.x * (256 / kWave);
  for (int64_t w = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave; w < n_units; w += nw) {
    const int64_t rt = w / s_tiles;
    const int64_t row = rt * kGlmTermsTile + (lane & 7);
    const int s = (int)(w - rt * s_tiles) * kGlmTermsTile + (lane >> 3);  // (s < s_pad: s_pad is a multiple of 16)
    if (row >= total) continue;
    double v = 0.0;
    for (int t = 0; t < P.n_terms; ++t) {  // (t is uniform: the arrays of the argument block are indexed by a scalar)
      const int64_t j = row - P.first[t];
      if (j >= 0 && row < P.first[t + 1] && s < P.n_draws) v = P.u[t][(int64_t)s * P.st_draw[t] + j * P.st_group[t]];
    }
    P.uimg[row * (int64_t)P.s_pad + s] = v;
  }
}
#endif

// (one or two chunks in registers: held to the 128 registers of four wavefronts per SIMD, which the epilogue's `exp` / `log1p` want;
// not the families of glm_rolled: lgamma, erfc and erfcx under that cap go to scratch)
template <int FAM, int NCH, bool PANEL>
__global__ __launch_bounds__(kWave * kGlmWaves) __attribute__((amdgpu_waves_per_eu(NCH <= 2 && !glm_rolled(FAM) ? 4 : 1))) void glm_terms_kernel(GlmTermsParams T) {
  const GlmParams& P = T.glm;
  const int S = P.n_draws;
  const int lane = threadIdx.x & (kWave - 1), i = lane & 15, q = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int n_dtiles = P.s_pad / kGlmTile;
  const int n_panels = PANEL ? P.p_pad / (kGlmK * NCH) : 1;
  const int64_t n_units = (P.n_rows + kGlmTile - 1) / kGlmTile * P.n_strips;
  const int64_t nw = (int64_t)gridDim.x * kGlmWaves;
  int64_t img_pitch = P.s_pad;
  if constexpr (glm_rolled(FAM)) asm volatile("" : "+v"(img_pitch));  // (a lane's multiplier: these kernels have no scalar register to spare)
  unsigned long long n_nan = 0;
  for (int64_t u = (int64_t)blockIdx.x * kGlmWaves + wv; u < n_units; u += nw) {
    const int64_t rt = u / P.n_strips;
    const int st = (int)(u - rt * P.n_strips);
    const int64_t r0 = rt * kGlmTile;
    // ---- A: this lane's row of X
    const double* xr = P.x + glm_source_row(P, r0 + i) * P.sx_obs;
    double a[NCH * 4];
    if constexpr (!PANEL) glm_load_x<NCH>(xr, P.zero, P.sx_pred, 0, q, P.n_pred, a);
    // ---- the per-observation values of this lane's four rows of C / D, and their source rows for the terms
    double yv[4], ov[4], tv[4], cv[4];
    int64_t src[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      src[g] = glm_source_row(P, r0 + q + 4 * g);
      ov[g] = P.offset ? P.offset[src[g]] : 0.0;
      yv[g] = FAM != PLA_GLM_LINPRED ? P.y[src[g]] : 0.0;
      tv[g] = glm_has_trials(FAM) && P.trials ? P.trials[src[g]] : 1.0;
      cv[g] = glm_has_obs_const(FAM) && P.obs_const ? P.obs_const[src[g]] : 0.0;
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
      double sig = 1.0, dc = 0.0, lsc = 0.0;
      if constexpr (glm_draw_values(FAM)) {
        sig = P.sigma[s_ok ? s : S - 1];
        dc = P.draw_const[s_ok ? s : S - 1];
      }
      if constexpr (FAM == PLA_GLM_NEGBINOMIAL_LOG) lsc = log(sig);
      double eta[4];
      {
#pragma clang fp contract(off)
#pragma unroll
        for (int g = 0; g < 4; ++g) eta[g] = acc[g] + ov[g];
        // ---- the terms, in order: column s of the image row of the group (s < s_pad: zero padding past the draws)
        // (the indices of term t + 1 are loaded under the lines of term t: one exposed latency per term, not two)
        const double* uc = T.uimg + s;
        int jn[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) jn[g] = T.group[0][src[g]];
#pragma unroll 1
        for (int t = 0; t < T.n_terms; ++t) {
          const double* zt = T.z[t];
          const int64_t first = T.first[t];
          const int last = T.last_group[t];
          double uv[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int j = jn[g] < 0 ? 0 : jn[g] < last ? jn[g] : last;
            uv[g] = uc[(first + j) * img_pitch];
          }
          if (t + 1 < T.n_terms) {
            const int32_t* gn = T.group[t + 1];
#pragma unroll
            for (int g = 0; g < 4; ++g) jn[g] = gn[src[g]];
          }
          if (zt) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const double zu = zt[src[g]] * uv[g];
              eta[g] = eta[g] + zu;
            }
          } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) eta[g] = eta[g] + uv[g];
          }
        }
      }
      if constexpr (glm_rolled(FAM)) {
        n_nan += glm_rolled_epilogue<FAM>(P, eta, yv, tv, cv, sig, dc, lsc, r0, q, s, s_ok);
        continue;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        double ll = glm_density<FAM>(eta[g], yv[g], tv[g], cv[g], sig, dc, lsc);
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
inline hipError_t glm_terms_launch_family(const GlmTermsParams& p, unsigned grid, hipStream_t stream) {
  const dim3 block(kWave * kGlmWaves);
  const int p_pad = p.glm.p_pad;
  if (p_pad > kGlmK * kGlmPanel) hipLaunchKernelGGL((glm_terms_kernel<FAM, kGlmPanel, true>), dim3(grid), block, 0, stream, p);
  else if (p_pad == kGlmK * 8) hipLaunchKernelGGL((glm_terms_kernel<FAM, 8, false>), dim3(grid), block, 0, stream, p);
  else if (p_pad == kGlmK * 4) hipLaunchKernelGGL((glm_terms_kernel<FAM, 4, false>), dim3(grid), block, 0, stream, p);
  else if (p_pad == kGlmK * 2) hipLaunchKernelGGL((glm_terms_kernel<FAM, 2, false>), dim3(grid), block, 0, stream, p);
  else hipLaunchKernelGGL((glm_terms_kernel<FAM, 1, false>), dim3(grid), block, 0, stream, p);
  return hipGetLastError();
}

}  // namespace pla
