// LOO diagnostics kernels: per observation r, from its log weights lw (of any normalisation) and its log-likelihood ll,
//     m = max_s lw_s,  e_s = exp(lw_s - m)  (lw_s = -inf: weight 0, the draw contributes to nothing)
//     elpd[r]    = LSE_s(lw_s + ll_s) - LSE_s(lw_s)
//     ess_w[r]   = (sum e_s)^2 / sum e_s^2                                     (= 1 / sum w_s^2, in [1, n_draws])
//     var_log[r] = log1p( sum_s (e_s (exp(ll_s - elpd) - 1))^2 / (sum e_s)^2 )  (= log1p(sum w_s^2 (exp(ll_s - elpd) - 1)^2))
// var_log is the variance of the self-normalised estimator on the linear scale (Vehtari et al. 2024, eq. 6) divided by its
// square and moved to the log scale by log-normal moment matching.  The front multiplies ess_w by r_eff and divides var_log by it.
// exp(x) - 1, not expm1(x): expm1 of the device library is exp's range reduction and polynomial plus a correction sequence on
// top, exp(x) - 1 is one v_add_f64 behind exp.  Its absolute error of one ulp of 1 matters only where ll_s - elpd is below 1e-8
// for every draw that carries weight, and var_log is then below 1e-16 (a constant row gives rounding noise below 1e-24).
//
// PREPARE.  diag_prepare_row_kernel / diag_prepare_tile_kernel are the prepare kernels of pla_pit.h with a row gather: they write
// -ll[row_index[r], :] (row_index null: row r) as a compact draws-fastest block in the dtype of ll, NaN -> -1e10 before the negation
// (loo.py:218-227) and counted, +-inf kept.  Every index is clamped into [0, n_src) here (a device list is the caller's; a host
// list has been range-checked before).  The row kernel reads any strides; the tile kernel takes observations-fastest input through
// a 64 x 64 tile of LDS -- with a row index its reads along the observations are a gather: correct, not fast.
//
// DIAG.  diag_wave_kernel<T, MODE, REG>: a wavefront per observation; draw <-> (lane, vector, element) and the three load modes are
// pit_wave_kernel's (pla_pit.h), so the order of every sum -- per lane by vector and element, then xor butterflies -- is a rule of
// n_draws and the dtype alone.  All arithmetic is f64.  Two matrices of one dtype, each with its own strides: lw, and x with
// ll_s = sign * x_s (sign = -1 reads the staged -ll block that fed the weights pass).  Three sweeps, exact maxima first (no
// online rescale):
//     A  m1 = max lw, m2 = max (lw + ll)
//     B  s1 = sum e, s2 = sum e^2, s3 = sum exp(lw + ll - m2)      -> elpd = (m2 - m1) + log(s3 / s1), ess_w = s1^2 / s2
//     C  s4 = sum (e (exp(ll - elpd) - 1))^2                       -> var_log = log1p(s4 / s1^2)
// REG (n_draws <= kPitRegDraws): the row of lw is read once into registers in sweep A and replaced by e in sweep B (three exp
// per draw); x is re-read in every sweep -- it was written or read a moment ago and comes from L2 / MALL.  Longer rows stream
// both matrices in each sweep (four exp per draw), and so does the strided mode at every length: e is the same exp of the same
// difference whether it is kept or taken again, and the sums below are never contracted into fused multiply-adds, so the register
// and the streamed form of a row give the same bits.  Holding lw alone keeps the register form at two waves per SIMD.
// A row whose weights are all NaN or all -inf, a row with a NaN weight or NaN ll, and a row whose elpd is NaN or -inf (every ll
// -inf) give NaN in the three values.  No floating-point atomics: a row's results depend on that row alone.
#pragma once

#include "pla_pit.h"

namespace pla {

struct DiagParams {
  const void* lw;  // (n_obs, n_draws) log weights
  const void* x;   // (n_obs, n_draws), the dtype of lw: ll = sign * x
  double sign;     // +1 or -1
  int64_t n_obs;
  int n_draws;
  int64_t lw_so, lw_sd, x_so, x_sd;  // elements
  double* elpd;     // [n_obs], each may be null
  double* ess_w;
  double* var_log;
};

struct DiagPrepareParams {
  const void* in;            // the matrix (row 0)
  void* out;                 // (n_rows, n_draws) contiguous
  const int64_t* row_index;  // [n_rows] device, or null: rows row0 .. row0 + n_rows - 1
  int64_t row0;
  int64_t n_src;             // rows of the matrix
  int64_t n_rows;
  int n_draws;
  int64_t stride_obs, stride_draw;  // elements
  unsigned long long* replaced;     // device counter (may be null)
};

__device__ __forceinline__ int64_t diag_source_row(const DiagPrepareParams& P, int64_t r) {
  const int64_t v = P.row_index ? P.row_index[r] : P.row0 + r;
  return v < 0 ? 0 : (v >= P.n_src ? P.n_src - 1 : v);
}

// ---- prepare --------------------------------------------------------------------------------------------------------------------
// a workgroup per (row, 1024 draws): thread t takes draws t, t + 256, ...
template <typename T>
__global__ __launch_bounds__(256) void diag_prepare_row_kernel(DiagPrepareParams P) {
  const int S = P.n_draws;
  const int64_t n_db = (S + 1023) / 1024, n_units = n_db * P.n_rows;
  unsigned n_nan = 0;
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int64_t r = u / n_db;
    const int d0 = (int)(u - r * n_db) * 1024 + (int)threadIdx.x;
    const T* ip = reinterpret_cast<const T*>(P.in) + diag_source_row(P, r) * P.stride_obs;
    T* op = reinterpret_cast<T*>(P.out) + r * S;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int d = d0 + j * 256;
      if (d < S) op[d] = pit_neg_ll(ip[(int64_t)d * P.stride_draw], n_nan);
    }
  }
  pit_count(P.replaced, n_nan);
}

// observations fastest (stride_obs == 1): a 64 x 64 tile through LDS, read along the observations, written along the draws
template <typename T>
__global__ __launch_bounds__(256) void diag_prepare_tile_kernel(DiagPrepareParams P) {
  __shared__ T tile[64][65];
  const int S = P.n_draws;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t n_tr = (P.n_rows + 63) / 64, n_td = (S + 63) / 64, n_units = n_tr * n_td;
  unsigned n_nan = 0;
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int64_t tr = u % n_tr, td = u / n_tr;
    const int64_t r0 = tr * 64;
    const int d0 = (int)td * 64;
    const int64_t r = r0 + tx;
    const int64_t src = r < P.n_rows ? diag_source_row(P, r) : 0;
#pragma unroll 4
    for (int j = ty; j < 64; j += 4) {  // tile[draw][observation]
      const int d = d0 + j;
      if (r < P.n_rows && d < S) tile[j][tx] = pit_neg_ll(reinterpret_cast<const T*>(P.in)[(int64_t)d * P.stride_draw + src], n_nan);
    }
    __syncthreads();
#pragma unroll 4
    for (int j = ty; j < 64; j += 4) {
      const int64_t ro = r0 + j;
      const int d = d0 + tx;
      if (ro < P.n_rows && d < S) reinterpret_cast<T*>(P.out)[ro * S + d] = tile[tx][j];
    }
    __syncthreads();
  }
  pit_count(P.replaced, n_nan);
}

// ---- diagnostics: a wavefront per observation ------------------------------------------------------------------------------------
// lw + ll of a draw that carries weight (a weight of log -inf carries none, whatever its ll)
__device__ __forceinline__ double diag_joint(double lw, double ll) { return lw == -pinf() ? -pinf() : lw + ll; }

// sweep B: one draw into the three sums; returns e
__device__ __forceinline__ double diag_sums(double lw, double ll, double m1, double m2, double& s1, double& s2, double& s3) {
#pragma clang fp contract(off)
  const double e = exp(lw - m1);
  s1 += e;
  s2 += e * e;
  s3 += exp(diag_joint(lw, ll) - m2);
  return e;
}

// sweep C: one draw into the last sum (e == 0: nothing, whatever exp(ll - elpd) is)
__device__ __forceinline__ void diag_dev(double e, double ll, double elpd, double& s4) {
#pragma clang fp contract(off)
  const double t = e == 0.0 ? 0.0 : e * (exp(ll - elpd) - 1.0);
  s4 += t * t;
}

__device__ __forceinline__ void diag_store(const DiagParams& P, int64_t r, double elpd, double s1, double s2, double s4) {
#pragma clang fp contract(off)
  s4 = wave_reduce<OpSum>(s4);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    const bool ok = elpd == elpd && elpd != -pinf();
    if (P.elpd) P.elpd[r] = ok ? elpd : qnan();
    if (P.ess_w) P.ess_w[r] = ok ? s1 * s1 / s2 : qnan();
    if (P.var_log) P.var_log[r] = ok ? log1p(s4 / (s1 * s1)) : qnan();
  }
}

template <typename T, int MODE, bool REG>
__global__ __launch_bounds__(kWave * kPitWaves) void diag_wave_kernel(DiagParams P) {
  constexpr int VEC = 16 / (int)sizeof(T), NQ = kPitSlots / VEC;
  const int S = P.n_draws;
  const double sign = P.sign;
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int nq = (S + kWave * VEC - 1) / (kWave * VEC);  // vectors per lane (wave-uniform)
  const int64_t nw = (int64_t)gridDim.x * kPitWaves;
  for (int64_t r = (int64_t)blockIdx.x * kPitWaves + wv; r < P.n_obs; r += nw) {
    const T* lp = reinterpret_cast<const T*>(P.lw) + r * P.lw_so;
    const T* xp = reinterpret_cast<const T*>(P.x) + r * P.x_so;
    double mx1 = -pinf(), mx2 = -pinf(), s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, elpd;
    if constexpr (REG) {
      // every lane's vectors q < nq - 1 lie inside the row as a whole: plain loads; only the last one is clamped and masked
      // (past the row: lw = -inf, weight 0)
      int nfull = nq - 1;
      asm volatile("" : "+s"(nfull));  // (opaque inside the row loop, as in pit_wave_kernel: the conditions q < nfull stay scalar compares)
      double x[NQ - 1][VEC], xl[VEC], v[VEC];
#pragma unroll
      for (int q = 0; q < NQ - 1; ++q) {
        if (q < nfull) {
          pit_load_whole<T, MODE, VEC>(lp, P.lw_sd, (q * kWave + lane) * VEC, x[q]);
          pit_load_whole<T, MODE, VEC>(xp, P.x_sd, (q * kWave + lane) * VEC, v);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            mx1 = fmax(mx1, x[q][e]);
            mx2 = fmax(mx2, diag_joint(x[q][e], sign * v[e]));
          }
        }
      }
      pit_load<T, MODE, VEC>(lp, P.lw_sd, (nfull * kWave + lane) * VEC, S, -pinf(), xl);
      pit_load<T, MODE, VEC>(xp, P.x_sd, (nfull * kWave + lane) * VEC, S, 0.0, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        mx1 = fmax(mx1, xl[e]);
        mx2 = fmax(mx2, diag_joint(xl[e], sign * v[e]));
      }
      const double m1 = wave_reduce<OpMax>(mx1), m2 = wave_reduce<OpMax>(mx2);
      int nb = nfull;
      asm volatile("" : "+s"(nb));
#pragma unroll
      for (int q = 0; q < NQ - 1; ++q) {
        if (q < nb) {
          pit_load_whole<T, MODE, VEC>(xp, P.x_sd, (q * kWave + lane) * VEC, v);
#pragma unroll
          for (int e = 0; e < VEC; ++e) x[q][e] = diag_sums(x[q][e], sign * v[e], m1, m2, s1, s2, s3);
        }
      }
      pit_load<T, MODE, VEC>(xp, P.x_sd, (nfull * kWave + lane) * VEC, S, 0.0, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) xl[e] = diag_sums(xl[e], sign * v[e], m1, m2, s1, s2, s3);
      s1 = wave_reduce<OpSum>(s1);
      s2 = wave_reduce<OpSum>(s2);
      s3 = wave_reduce<OpSum>(s3);
      elpd = (m2 - m1) + log(s3 / s1);
      int nc = nfull;
      asm volatile("" : "+s"(nc));
#pragma unroll
      for (int q = 0; q < NQ - 1; ++q) {
        if (q < nc) {
          pit_load_whole<T, MODE, VEC>(xp, P.x_sd, (q * kWave + lane) * VEC, v);
#pragma unroll
          for (int e = 0; e < VEC; ++e) diag_dev(x[q][e], sign * v[e], elpd, s4);
        }
      }
      pit_load<T, MODE, VEC>(xp, P.x_sd, (nfull * kWave + lane) * VEC, S, 0.0, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) diag_dev(xl[e], sign * v[e], elpd, s4);
    } else {
      constexpr int U = 8 / VEC;  // vectors of a batch: eight elements of each matrix in flight per lane
#pragma unroll 1
      for (int q0 = 0; q0 < nq; q0 += U) {
        double x[U][VEC], v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          pit_load<T, MODE, VEC>(lp, P.lw_sd, ((q0 + u) * kWave + lane) * VEC, S, -pinf(), x[u]);
          pit_load<T, MODE, VEC>(xp, P.x_sd, ((q0 + u) * kWave + lane) * VEC, S, 0.0, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            mx1 = fmax(mx1, x[u][e]);
            mx2 = fmax(mx2, diag_joint(x[u][e], sign * v[u][e]));
          }
      }
      const double m1 = wave_reduce<OpMax>(mx1), m2 = wave_reduce<OpMax>(mx2);
#pragma unroll 1
      for (int q0 = 0; q0 < nq; q0 += U) {
        double x[U][VEC], v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          pit_load<T, MODE, VEC>(lp, P.lw_sd, ((q0 + u) * kWave + lane) * VEC, S, -pinf(), x[u]);
          pit_load<T, MODE, VEC>(xp, P.x_sd, ((q0 + u) * kWave + lane) * VEC, S, 0.0, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int e = 0; e < VEC; ++e) (void)diag_sums(x[u][e], sign * v[u][e], m1, m2, s1, s2, s3);
      }
      s1 = wave_reduce<OpSum>(s1);
      s2 = wave_reduce<OpSum>(s2);
      s3 = wave_reduce<OpSum>(s3);
      elpd = (m2 - m1) + log(s3 / s1);
#pragma unroll 1
      for (int q0 = 0; q0 < nq; q0 += U) {
        double x[U][VEC], v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          pit_load<T, MODE, VEC>(lp, P.lw_sd, ((q0 + u) * kWave + lane) * VEC, S, -pinf(), x[u]);
          pit_load<T, MODE, VEC>(xp, P.x_sd, ((q0 + u) * kWave + lane) * VEC, S, 0.0, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int e = 0; e < VEC; ++e) diag_dev(exp(x[u][e] - m1), sign * v[u][e], elpd, s4);
      }
    }
    diag_store(P, r, elpd, s1, s2, s4);
  }
}

}  // namespace pla
