// GLM leave-one-out predictive moments and PIT: the generator's tile of eta (pla_glm.h), contracted against a block of log weights
// in the epilogue instead of stored.  Per observation i, with lw row i of the weights (any normalisation), m = max_s lw_s,
// e_s = exp(lw_s - m) (a weight of log -inf is 0; a draw whose e_s is 0 contributes to nothing):
//     mean[i]   = sum e mu / sum e          m2[i]     = sum e (v + mu^2) / sum e
//     pit_le[i] = sum e F_le / sum e        pit_lt[i] = sum e F_lt / sum e
// mu, v and F the conditional mean, variance and distribution function of y_i under draw s: Rao-Blackwellised, no predictive draws.
// All arithmetic is f64, fp contract(off), every sum and product rounded once in the order written:
//     eta = acc + offset_i                                               the generator's bits (pla_glm.h: the same chain)
//     tail(t) = (h exp(-w)) (1 - 0.5 r), h = 0.5 erfcx(|t| / sqrt 2), w = 0.5 fl(t^2), r = t^2 - fl(t^2)     = Phi(-|t|),
//                                                                        the arithmetic of glm_log_ndtr_pair
//   PLA_GLM_GAUSSIAN         mu = eta, v = sigma sigma, second = v + mu mu; t = (y - eta) / sigma,
//                            F_le = F_lt = t < 0 ? tail(t) : 1 - tail(t)
//   PLA_GLM_GAMMA_LOG        mu = exp(eta), second = (mu mu) / alpha + mu mu; no distribution function
//   PLA_GLM_POISSON_LOG      mu = exp(eta), v = mu;                                   c = exp(-eta),        r_k = k c
//   PLA_GLM_NEGBINOMIAL_LOG  mu = exp(eta), v = mu + (mu mu) / phi;                   c = (mu + phi) / mu,  r_k = (k / ((k - 1) + phi)) c
//   PLA_GLM_BINOMIAL_LOGIT   x = exp(-|eta|), d = 1 + x, big = 1 / d, small = x / d, (p, 1 - p) = eta >= 0 ? (big, small) : (small, big),
//                            mu = n p, v = mu (1 - p);                                c = exp(-eta),        r_k = (k / ((n - k) + 1)) c
//   PLA_GLM_BINOMIAL_PROBIT  lo = tail(eta), hi = 1 - lo, (p, 1 - p) = eta < 0 ? (lo, hi) : (hi, lo),
//                            mu = n p, v = mu (1 - p);                                c = (1 - p) / p,      r_k = (k / ((n - k) + 1)) c
//   the four discrete families: second = v + mu mu; pmf = exp(ll), ll = glm_density<FAM> on the same registers; r_k = pmf(k - 1) / pmf(k);
//                            t = 1, T = 0; for k = y, y - 1, ..., 1: t = t r_k, T = T + t;      (downward from the pmf at y)
//                            F_lt = pmf T, F_le = F_lt + pmf (the unclipped F_lt), each 1 where it exceeds 1;
//                            T = +inf, or pmf = 0 with r_y > 1 (y far above the mode): F_lt = F_le = 1; pmf = 0 with r_y <= 1: both 0, by
//                            the products themselves.  All terms are positive: no cancellation.  The two binomial families:
//                            F_le = 1 for y >= n, the end of the support (a sum of the whole pmf would round beside it).
// A count outside [0, kGlmPredictMaxCount] is not walked: the combine kernel writes NaN into the row's two PIT values and counts the
// row; its moments are computed as any other's.
//
// THE SUMMATION RULE.  A segment is kGlmPredictSeg tiles of 16 draws.  Inside a segment the lane of column c adds the terms of the
// draws 16 t + c in order of t, each of the five sums started from zero; the 16 columns are combined by the butterfly
// v += v(lane ^ 1), ^ 2, ^ 4, ^ 8 (both partners form the same sum); the per-(row, segment) partials go to a workspace of this pass
// alone, and glm_predict_combine_kernel adds them in order of the segments, starting from segment 0's, and divides by sum e.
// m is the row maximum of a pre-pass (glm_predict_rowmax_kernel; NaN entries ignored by fmax: they reach the sums as NaN).
// A row's outputs depend on its row of X, its entries of the vectors, its row of lw and n_draws alone -- not on the grid, the strip
// (whole segments), the block, the row's position or the row list.  There are no floating-point atomics; the skipped rows are
// counted by an integer atomic.  No LDS allocation and no scratch.
#pragma once

#include "pla_glm.h"

namespace pla {

constexpr int kGlmPredictSums = 5;  // sum e, sum e mu, sum e (v + mu^2), sum e F_le, sum e F_lt

struct GlmPredictParams {
  GlmParams g;            // the generator's launch (out, pitch and replaced unused); strips are whole segments
  const double* lw;       // (n_rows, n_draws) log weights of the launch's rows, row pitch lw_pitch, draws fastest
  int64_t lw_pitch;
  double* row_max;        // [n_rows]
  double* part;           // [n_rows][n_seg][kGlmPredictSums]
  int n_seg;
  int want_pit;           // 0: the discrete recurrence is not walked (nobody reads the PIT sums)
  int discrete;           // the family has counts: the cap applies
  double *mean, *m2, *pit_le, *pit_lt;  // [n_rows], each may be null
  unsigned long long* skipped;
};

// the families pla_k_glm_predict.hip does not instantiate (pla_k_glm_predict_families.hip); *name: the family as the route text names it
hipError_t launch_glm_predict_more(int family, const GlmPredictParams& p, unsigned grid, hipStream_t stream, const char** name);

constexpr bool glm_discrete(int fam) {
  return fam == PLA_GLM_BINOMIAL_LOGIT || fam == PLA_GLM_POISSON_LOG || fam == PLA_GLM_NEGBINOMIAL_LOG || fam == PLA_GLM_BINOMIAL_PROBIT;
}

#ifndef PLA_GLM_PREDICT_SHARED_ONLY  // (the two small kernels are pla_k_glm_predict.hip's)
__global__ __launch_bounds__(256) void glm_predict_rowmax_kernel(GlmPredictParams Q) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave; r < Q.g.n_rows; r += nw) {
    const double* row = Q.lw + r * Q.lw_pitch;
    double m = -HUGE_VAL;
    for (int s = lane; s < Q.g.n_draws; s += kWave) m = fmax(m, row[s]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d));
    if (lane == 0) Q.row_max[r] = m;
  }
}

__global__ __launch_bounds__(256) void glm_predict_combine_kernel(GlmPredictParams Q) {
#pragma clang fp contract(off)
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < Q.g.n_rows; r += (int64_t)gridDim.x * 256) {
    const double* p = Q.part + r * Q.n_seg * kGlmPredictSums;
    double a[kGlmPredictSums];
#pragma unroll
    for (int k = 0; k < kGlmPredictSums; ++k) a[k] = p[k];
    for (int sg = 1; sg < Q.n_seg; ++sg) {
#pragma unroll
      for (int k = 0; k < kGlmPredictSums; ++k) a[k] = a[k] + p[sg * kGlmPredictSums + k];
    }
    double le = a[3] / a[0], lt = a[4] / a[0];
    if (Q.discrete && Q.want_pit) {
      const double y = Q.g.y[glm_source_row(Q.g, r)];
      if (!(y >= 0.0 && y <= (double)kGlmPredictMaxCount)) {
        le = lt = __builtin_nan("");
        if (Q.skipped) atomicAdd(Q.skipped, 1ull);
      }
    }
    if (Q.mean) Q.mean[r] = a[1] / a[0];
    if (Q.m2) Q.m2[r] = a[2] / a[0];
    if (Q.pit_le) Q.pit_le[r] = le;
    if (Q.pit_lt) Q.pit_lt[r] = lt;
  }
}

#endif

// Phi(-|t|): glm_log_ndtr_pair's h exp(-w) (1 - r / 2)
__device__ __forceinline__ double glm_ndtr_tail(double t) {
#pragma clang fp contract(off)
  const double h = 0.5 * erfcx(fabs(t) * 0.70710678118654752440);
  const double sq = t * t;
  const double r = sq < HUGE_VAL ? fma(t, t, -sq) : 0.0;
  const double w = 0.5 * sq;
  return (h * exp(-w)) * (1.0 - 0.5 * r);
}

// r_k of a discrete family (the header's table); a: trials or phi, c: the draw's constant factor
template <int FAM>
__device__ __forceinline__ double glm_pmf_ratio(double k, double a, double c) {
#pragma clang fp contract(off)
  if constexpr (FAM == PLA_GLM_POISSON_LOG) return k * c;
  else if constexpr (FAM == PLA_GLM_NEGBINOMIAL_LOG) return (k / ((k - 1.0) + a)) * c;
  else return (k / ((a - k) + 1.0)) * c;
}

// mu, the second moment and the two distribution function values of one (observation, draw); walk: the count is inside the cap
template <int FAM>
__device__ __forceinline__ void glm_predict_point(double eta, double y, double trials, double obs_const, double sigma, double draw_const,
                                                  double log_scale, bool walk, double* mu, double* second, double* f_le, double* f_lt) {
#pragma clang fp contract(off)
  if constexpr (FAM == PLA_GLM_GAUSSIAN) {
    const double v = sigma * sigma;
    *mu = eta;
    *second = v + eta * eta;
    const double t = (y - eta) / sigma;
    const double lo = glm_ndtr_tail(t);
    *f_le = *f_lt = t < 0.0 ? lo : 1.0 - lo;
  } else if constexpr (FAM == PLA_GLM_GAMMA_LOG) {
    const double m = exp(eta);
    *mu = m;
    *second = (m * m) / sigma + m * m;
    *f_le = *f_lt = 0.0;
  } else {
    double m, v, c, a;
    if constexpr (FAM == PLA_GLM_POISSON_LOG) {
      m = exp(eta);
      v = m;
      c = exp(-eta);
      a = 0.0;
    } else if constexpr (FAM == PLA_GLM_NEGBINOMIAL_LOG) {
      m = exp(eta);
      v = m + (m * m) / sigma;
      c = (m + sigma) / m;
      a = sigma;
    } else if constexpr (FAM == PLA_GLM_BINOMIAL_LOGIT) {
      const double x = exp(-fabs(eta)), d = 1.0 + x;
      const double big = 1.0 / d, small = x / d;
      const bool pos = eta >= 0.0;
      m = trials * (pos ? big : small);
      v = m * (pos ? small : big);
      c = exp(-eta);
      a = trials;
    } else {
      const double lo = glm_ndtr_tail(eta), hi = 1.0 - lo;
      const bool neg = eta < 0.0;
      const double p = neg ? lo : hi, q = neg ? hi : lo;
      m = trials * p;
      v = m * q;
      c = q / p;
      a = trials;
    }
    *mu = m;
    *second = v + m * m;
    const double pmf = exp(glm_density<FAM>(eta, y, trials, obs_const, sigma, draw_const, log_scale));
    double t = 1.0, T = 0.0, ry = 0.0;
    if (walk) {  // (at most kGlmPredictMaxCount turns; lanes past their own count are masked off)
      if (y >= 1.0) ry = glm_pmf_ratio<FAM>(y, a, c);
      for (double k = y; k >= 1.0; k -= 1.0) {
        t = t * glm_pmf_ratio<FAM>(k, a, c);
        T = T + t;
      }
    }
    double lt = pmf * T, le = lt + pmf;
    le = le > 1.0 ? 1.0 : le;
    lt = lt > 1.0 ? 1.0 : lt;
    if (T == HUGE_VAL || (pmf == 0.0 && ry > 1.0)) lt = le = 1.0;
    if constexpr (glm_has_trials(FAM)) le = y >= trials ? 1.0 : le;  // (the end of the support)
    *f_le = le;
    *f_lt = lt;
  }
}

template <int FAM, int NCH, bool PANEL>
__global__ __launch_bounds__(kWave * kGlmWaves) void glm_predict_kernel(GlmPredictParams Q) {
  const GlmParams& P = Q.g;
  const int S = P.n_draws;
  const int lane = threadIdx.x & (kWave - 1), i = lane & 15, q = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int n_dtiles = P.s_pad / kGlmTile;
  const int n_panels = PANEL ? P.p_pad / (kGlmK * NCH) : 1;
  // One unit per wavefront, no walk over the units: the scalars of a launch that the loop over the tiles does not read end with the
  // preamble (held across an outer loop, beside the constants of exp and of the special functions, they spill into vector lanes).
  const int64_t n_units = (P.n_rows + kGlmTile - 1) / kGlmTile * P.n_strips;
  const int64_t u = (int64_t)blockIdx.x * kGlmWaves + wv;
  if (u >= n_units) return;
  {
    const int64_t rt = u / P.n_strips;
    const int st = (int)(u - rt * P.n_strips);
    const int64_t r0 = rt * kGlmTile;
    // ---- A: this lane's row of X
    const double* xr = P.x + glm_source_row(P, r0 + i) * P.sx_obs;
    double a[NCH * 4];
    if constexpr (!PANEL) glm_load_x<NCH>(xr, P.zero, P.sx_pred, 0, q, P.n_pred, a);
    // ---- the per-observation values of this lane's four rows of C / D, and their maxima of lw
    double yv[4], ov[4], tv[4], cv[4], mv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t r = r0 + q + 4 * g;
      const int64_t src = glm_source_row(P, r);
      ov[g] = P.offset ? P.offset[src] : 0.0;
      yv[g] = P.y[src];
      tv[g] = glm_has_trials(FAM) && P.trials ? P.trials[src] : 1.0;
      cv[g] = glm_has_obs_const(FAM) && P.obs_const ? P.obs_const[src] : 0.0;
      mv[g] = Q.row_max[r < P.n_rows ? r : P.n_rows - 1];
    }
    const int t_end = (st + 1) * P.strip_tiles < n_dtiles ? (st + 1) * P.strip_tiles : n_dtiles;
#pragma unroll 1
    for (int t0 = st * P.strip_tiles; t0 < t_end; t0 += kGlmPredictSeg) {  // one segment
      double sum[kGlmPredictSums][4];
#pragma unroll
      for (int k = 0; k < kGlmPredictSums; ++k)
#pragma unroll
        for (int g = 0; g < 4; ++g) sum[k][g] = 0.0;
      const int t1 = t0 + kGlmPredictSeg < t_end ? t0 + kGlmPredictSeg : t_end;
#pragma unroll 1
      for (int dt = t0; dt < t1; ++dt) {
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
        double eta[4], ev[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma clang fp contract(off)
          eta[g] = acc[g] + ov[g];
          const int64_t r = r0 + q + 4 * g;
          const double lw = s_ok && r < P.n_rows ? Q.lw[r * Q.lw_pitch + s] : -HUGE_VAL;
          ev[g] = lw == -HUGE_VAL ? 0.0 : exp(lw - mv[g]);
        }
        // (the lane's four rows one after the other, rotated as in glm_rolled_epilogue: one copy of the special functions)
        const bool want = Q.want_pit != 0;
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {
#pragma clang fp contract(off)
          double mu, second, f_le, f_lt;
          const bool walk = want && yv[0] >= 0.0 && yv[0] <= (double)kGlmPredictMaxCount;
          glm_predict_point<FAM>(eta[0], yv[0], tv[0], cv[0], sig, dc, lsc, walk, &mu, &second, &f_le, &f_lt);
          const double e = ev[0];
          const bool in = !(e == 0.0);  // (a NaN weight stays in)
          sum[0][0] = sum[0][0] + e;
          sum[1][0] = sum[1][0] + (in ? e * mu : 0.0);
          sum[2][0] = sum[2][0] + (in ? e * second : 0.0);
          if constexpr (FAM != PLA_GLM_GAMMA_LOG) {
            sum[3][0] = sum[3][0] + (in ? e * f_le : 0.0);
            sum[4][0] = sum[4][0] + (in ? e * f_lt : 0.0);
          }
          glm_rotate(eta);
          glm_rotate(ev);
          glm_rotate(yv);
          if constexpr (glm_has_trials(FAM)) glm_rotate(tv);
          glm_rotate(cv);
#pragma unroll
          for (int k = 0; k < kGlmPredictSums; ++k) glm_rotate(sum[k]);
        }
      }
      // ---- the 16 columns of a row, then one partial per (row, segment)
#pragma unroll
      for (int d = 1; d <= 8; d <<= 1)
#pragma unroll
        for (int k = 0; k < kGlmPredictSums; ++k)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
#pragma clang fp contract(off)
            sum[k][g] = sum[k][g] + __shfl_xor(sum[k][g], d);
          }
      if (i == 0) {
        const int sg = t0 / kGlmPredictSeg;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int64_t r = r0 + q + 4 * g;
          if (r < P.n_rows) {
            double* p = Q.part + (r * Q.n_seg + sg) * kGlmPredictSums;
#pragma unroll
            for (int k = 0; k < kGlmPredictSums; ++k) p[k] = sum[k][g];
          }
        }
      }
    }
  }
}

// the instantiation of a family for the padded predictor count of a launch (glm_launch_family's choice)
template <int FAM>
inline hipError_t glm_predict_launch_family(const GlmPredictParams& p, unsigned grid, hipStream_t stream) {
  const dim3 block(kWave * kGlmWaves);
  const int pp = p.g.p_pad;
  if (pp > kGlmK * kGlmPanel) hipLaunchKernelGGL((glm_predict_kernel<FAM, kGlmPanel, true>), dim3(grid), block, 0, stream, p);
  else if (pp == kGlmK * 8) hipLaunchKernelGGL((glm_predict_kernel<FAM, 8, false>), dim3(grid), block, 0, stream, p);
  else if (pp == kGlmK * 4) hipLaunchKernelGGL((glm_predict_kernel<FAM, 4, false>), dim3(grid), block, 0, stream, p);
  else if (pp == kGlmK * 2) hipLaunchKernelGGL((glm_predict_kernel<FAM, 2, false>), dim3(grid), block, 0, stream, p);
  else hipLaunchKernelGGL((glm_predict_kernel<FAM, 1, false>), dim3(grid), block, 0, stream, p);
  return hipGetLastError();
}

}  // namespace pla
