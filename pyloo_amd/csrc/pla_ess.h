// Relative MCMC efficiency of every row of a matrix: r_eff = ESS / (C n) of the row mean, Stan's estimator for the mean (Vehtari et al.
// 2021, Geyer 1992) WITHOUT rank normalisation -- relative_eff of R-loo on exp(log_lik).  A row holds C0 chains of n0 draws, chain
// major.  split: every chain is replaced by its first n = n0 / 2 and its last n draws as two chains (C = 2 C0; the middle draw of an
// odd chain is never read); otherwise C = C0, n = n0.  log: the values analysed are x = exp(row - max of the row's used draws); otherwise
// the row as it is.  All arithmetic is f64 (f32 input is widened on load).  With d[c][i] = x[c][i] - m_c:
//     S(t)   = sum_c sum_{i < n - t} d[c][i] d[c][i + t]          A(t) = S(t) / (C n)        (the divisor-n autocovariance, mean over chains)
//     W = A(0) n / (n - 1)      V = A(0) + var_ddof1(m_c) (0 when C = 1)      rho(t) = 1 - (W - A(t)) / V
//     Geyer:  e = 1, o = rho(1), P = S_ = e + o, t = 2;  while t < n - 1 and e + o > 0:  e = rho(t), o = rho(t + 1), q = e + o;
//             if q >= 0: P = min(q, P) (the initial monotone sequence: a pair above its predecessor takes the predecessor's sum), S_ += P;
//             t += 2.      tau = -1 + 2 S_ + max(e, 0), tau = max(tau, 1 / log10(C n)),  r_eff = 1 / tau  (cap: at most 1)
// (S_ is the sum of the corrected rho-hat below the stopping lag T = t, accumulated pair by pair; max(e, 0) is rho-hat(T).)
// INVALID ROWS give NaN and are counted: a NaN or +inf entry (-inf too when log is off), a constant row (max == min: every entry -inf
// included), V not positive and finite.  Single -inf entries of a log row are likelihood 0.
//
// THE SUMMATION RULE.  Lane l of the row's wavefront owns, in chain c, the draws i = l, l + 64, l + 128, ...  Every sum over the draws
// of a chain (the chain sum behind m_c = sum / n) and every S(t) (over all chains: c ascending, then i ascending, each term added with
// one fma, acc = fma(d[c][i], d[c][i + t], acc)) is accumulated per lane in that order from +0.0 and the 64 lane values are then merged by
// xor butterflies at distances 32, 16, 8, 4, 2, 1.  The mean of the m_c and the sum of (m_c - mean)^2 are taken in chain order.
// That rule depends on (C, n) alone: not on the grid, on which workgroup takes a row, on the layout (observations-fastest input is
// transposed into staging and takes the same kernel), on the memory space or on where d lives.  No floating-point atomics (the
// invalid-row counter is an integer).
//
// ess_row_kernel<T, true>   C n <= kEssLdsDraws (4096): the row is read from memory ONCE, into registers (64 slots a lane) a row ahead
//                           of its turn and from there into the wavefront's 32 KiB of LDS -- a workgroup is one wavefront; a CU's
//                           160 KiB admit five, the registers of the row in flight (256 VGPRs + ~100 AGPRs) one per SIMD, so four
//                           are resident -- where it is transformed and centred in place; the lags read LDS only, a pair
//                           (t, t + 1) per sweep with d[c][i] shared, until Geyer's rule stops.
// ess_row_kernel<T, false>  longer rows: the same code with d in a slot of global workspace per workgroup (L2-resident at 20 000 f64).
// The stop test is wave-uniform (a butterfly sum has the same bits in every lane).  A row that never stops costs O(C n^2).
#pragma once

#include "../../include/pyloo_amd.h"
#include "pla_device.h"
#include "pla_kernels.h"

namespace pla {

constexpr int kEssLdsDraws = 4096;  // analysed draws of a row that fit the wavefront's LDS (32 KiB of f64)
constexpr int kEssLoadBatch = 16;   // loads in flight per lane while a row comes in
constexpr int kEssBatch = 8;        // LDS reads in flight per lane and operand in the sweeps over a chain

struct EssParams {
  const void* in;      // row 0, draws contiguous
  int64_t stride_obs;  // elements
  int64_t n_obs;
  int n_src_chains;  // C0
  int n_src;         // n0: draws per chain in memory
  int n;             // draws per analysed chain (n0, or n0 / 2 when split)
  int split, log, cap;
  double* ws;        // long route: gridDim.x slots of C n doubles
  double* out;       // [n_obs]
  unsigned long long* invalid;  // device counter (may be null)
};

// `len` consecutive draws into dst, widened; the lane's maximum / minimum and whether it met a NaN
template <typename T>
__device__ __forceinline__ void ess_load(const T* src, double* dst, int len, int lane, double& mx, double& mn, bool& nan) {
  for (int i0 = 0; i0 < len; i0 += kWave * kEssLoadBatch) {
    double v[kEssLoadBatch];
#pragma unroll
    for (int u = 0; u < kEssLoadBatch; ++u) {
      const int i = i0 + u * kWave + lane;
      v[u] = i < len ? (double)src[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kEssLoadBatch; ++u) {
      const int i = i0 + u * kWave + lane;
      if (i < len) {
        dst[i] = v[u];
        nan = nan || v[u] != v[u];
        mx = fmax(mx, v[u]);
        mn = fmin(mn, v[u]);
      }
    }
  }
}

// S(t) (and S(t + 1) when PAIR) of the centred row d.  The reads of kEssBatch terms are issued together -- a wavefront has a SIMD
// almost to itself, so nothing else hides their latency; a slot past the end contributes fma(0, 0, acc) = acc, which leaves the bits
// of the rule's sum unchanged.
template <bool PAIR>
__device__ __forceinline__ void ess_lag(const double* d, int C, int n, int t, int lane, double& s0, double& s1) {
  double a0 = 0.0, a1 = 0.0;
  const int m = n - t;  // terms of lag t per chain; lag t + 1 has m - 1
  for (int c = 0; c < C; ++c) {
    const double* dc = d + (size_t)c * n;
    for (int i0 = lane; i0 < m; i0 += kWave * kEssBatch) {
      double x[kEssBatch], y[kEssBatch], z[kEssBatch];
#pragma unroll
      for (int u = 0; u < kEssBatch; ++u) {
        const int i = i0 + u * kWave;
        x[u] = i < m ? dc[i] : 0.0;
        y[u] = i < m ? dc[i + t] : 0.0;
        z[u] = (PAIR && i + 1 < m) ? dc[i + t + 1] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kEssBatch; ++u) {
        a0 = fma(x[u], y[u], a0);
        if (PAIR) a1 = fma(x[u], z[u], a1);
      }
    }
  }
  s0 = wave_reduce<OpSum>(a0);
  if (PAIR) s1 = wave_reduce<OpSum>(a1);
}

// A whole unsplit row of the on-chip route into registers: slot u of a lane is draw j = 64 u + lane.  Issued a row ahead (the
// wavefront's next row is in flight while it works on the current one in LDS), committed to LDS by ess_commit.  Split rows are
// read straight into LDS by ess_read, like the long route's.
constexpr int kEssSlots = kEssLdsDraws / kWave;

template <typename T>
__device__ __forceinline__ void ess_fetch(const T* x, int total, int lane, double (&v)[kEssSlots]) {
#pragma unroll
  for (int u = 0; u < kEssSlots; ++u) {
    const int j = u * kWave + lane;
    v[u] = (double)x[j < total ? j : total - 1];  // (no predicate to keep: a slot past the end re-reads the last draw and is dropped)
  }
}

// (every slot is stored: j < kEssLdsDraws always, the LDS behind the row is unused, and a slot past the end holds the last draw
// again, which changes neither the maximum, the minimum nor the NaN flag -- no per-slot predicates to keep in scalar registers)
__device__ __forceinline__ void ess_commit(const double (&v)[kEssSlots], double* d, int lane, double& mx, double& mn, bool& nan) {
#pragma unroll
  for (int u = 0; u < kEssSlots; ++u) {
    d[u * kWave + lane] = v[u];
    nan = nan || v[u] != v[u];
    mx = fmax(mx, v[u]);
    mn = fmin(mn, v[u]);
  }
}

// the row straight into d (the long route)
template <typename T>
__device__ __forceinline__ void ess_read(const EssParams& P, const T* x, double* d, int lane, double& mx, double& mn, bool& nan) {
  const int n = P.n, n0 = P.n_src;
  const int C = P.split ? 2 * P.n_src_chains : P.n_src_chains;
  if (P.split) {
    for (int c = 0; c < C; ++c) ess_load(x + (size_t)(c >> 1) * n0 + ((c & 1) ? n0 - n : 0), d + (size_t)c * n, n, lane, mx, mn, nan);
  } else {
    ess_load(x, d, C * n, lane, mx, mn, nan);
  }
}

// everything after the row is in d: (mx, mn, nan) are the lane's maximum, minimum and NaN flag of the draws it stored
__device__ __forceinline__ double ess_finish(const EssParams& P, double* d, int lane, double mx, double mn, bool nan) {
  const int n = P.n;
  const int C = P.split ? 2 * P.n_src_chains : P.n_src_chains;
  const int total = C * n;
  mx = wave_reduce<OpMax>(mx);
  mn = wave_reduce<OpMin>(mn);
  const bool bad = __ballot(nan) != 0ull || mx == pinf() || mx == mn || (!P.log && mn == -pinf());
  __syncthreads();  // (the lanes own other draws from here on)
  if (bad) return qnan();

  // 2. transform in place, chain sums; then centre, S(0) and the variance of the chain means
  double sum_m = 0.0;
  for (int c = 0; c < C; ++c) {
    double* dc = d + (size_t)c * n;
    double acc = 0.0;
    for (int i0 = lane; i0 < n; i0 += kWave * kEssBatch) {
      double v[kEssBatch];
#pragma unroll
      for (int u = 0; u < kEssBatch; ++u) {
        const int i = i0 + u * kWave;
        v[u] = i < n ? dc[i] : 0.0;
      }
      if (P.log) {
#pragma unroll
        for (int u = 0; u < kEssBatch; ++u) {
          const int i = i0 + u * kWave;
          if (i < n) {
            v[u] = exp(v[u] - mx);
            dc[i] = v[u];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kEssBatch; ++u) acc += v[u];  // (a slot past the end adds +0.0)
    }
    sum_m += wave_reduce<OpSum>(acc) / (double)n;
  }
  const double mean_m = sum_m / (double)C;
  double ss_m = 0.0, a0 = 0.0;
  for (int c = 0; c < C; ++c) {
    double* dc = d + (size_t)c * n;
    double acc = 0.0;
    for (int i0 = lane; i0 < n; i0 += kWave * kEssBatch) {
      double v[kEssBatch];
#pragma unroll
      for (int u = 0; u < kEssBatch; ++u) {
        const int i = i0 + u * kWave;
        v[u] = i < n ? dc[i] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kEssBatch; ++u) acc += v[u];
    }
    const double m_c = wave_reduce<OpSum>(acc) / (double)n;  // (the bits of the first sweep)
    ss_m += (m_c - mean_m) * (m_c - mean_m);
    for (int i0 = lane; i0 < n; i0 += kWave * kEssBatch) {
      double v[kEssBatch];
#pragma unroll
      for (int u = 0; u < kEssBatch; ++u) {
        const int i = i0 + u * kWave;
        v[u] = i < n ? dc[i] - m_c : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kEssBatch; ++u) {
        const int i = i0 + u * kWave;
        if (i < n) dc[i] = v[u];
        a0 = fma(v[u], v[u], a0);
      }
    }
  }
  __syncthreads();
  const double cn = (double)total;
  const double A0 = wave_reduce<OpSum>(a0) / cn;
  const double W = A0 * (double)n / (double)(n - 1);
  const double V = A0 + (C > 1 ? ss_m / (double)(C - 1) : 0.0);
  if (!(V > 0.0) || V == pinf()) return qnan();

  // 3. Geyer's initial positive and monotone sequences, a pair of lags per sweep
  double s0, s1 = 0.0;
  ess_lag<false>(d, C, n, 1, lane, s0, s1);
  double e = 1.0, o = 1.0 - (W - s0 / cn) / V;
  double prev = e + o, acc = prev;
  for (int t = 2; t < n - 1 && e + o > 0.0; t += 2) {
    ess_lag<true>(d, C, n, t, lane, s0, s1);
    e = 1.0 - (W - s0 / cn) / V;
    o = 1.0 - (W - s1 / cn) / V;
    const double q = e + o;
    if (q >= 0.0) {
      prev = q > prev ? prev : q;
      acc += prev;
    }
  }
  double tau = -1.0 + 2.0 * acc + (e > 0.0 ? e : 0.0);
  tau = fmax(tau, 1.0 / log10(cn));
  const double r = 1.0 / tau;
  return (P.cap && r > 1.0) ? 1.0 : r;
}

template <typename T, bool LDS>
__global__ __launch_bounds__(kWave) void ess_row_kernel(EssParams P) {
  __shared__ double lds[LDS ? kEssLdsDraws : 1];
  const int lane = threadIdx.x;
  const int total = (P.split ? 2 * P.n_src_chains : P.n_src_chains) * P.n;
  const T* in = static_cast<const T*>(P.in);
  unsigned n_bad = 0;
  if constexpr (LDS) {
    double v[kEssSlots];
    const bool ahead = !P.split;
    int64_t row = blockIdx.x;
    if (ahead && row < P.n_obs) ess_fetch<T>(in + row * P.stride_obs, total, lane, v);
    for (; row < P.n_obs; row += gridDim.x) {
      double mx = -pinf(), mn = pinf();
      bool nan = false;
      if (ahead) ess_commit(v, lds, lane, mx, mn, nan);
      else ess_read<T>(P, in + row * P.stride_obs, lds, lane, mx, mn, nan);
      const int64_t next = row + gridDim.x;
      if (ahead && next < P.n_obs) ess_fetch<T>(in + next * P.stride_obs, total, lane, v);  // (in flight while this row is worked on)
      const double r = ess_finish(P, lds, lane, mx, mn, nan);
      n_bad += r != r ? 1u : 0u;
      if (lane == 0) P.out[row] = r;
      __syncthreads();  // (the next row overwrites the LDS)
    }
  } else {
    double* d = P.ws + (size_t)blockIdx.x * (size_t)total;
    for (int64_t row = blockIdx.x; row < P.n_obs; row += gridDim.x) {
      double mx = -pinf(), mn = pinf();
      bool nan = false;
      ess_read<T>(P, in + row * P.stride_obs, d, lane, mx, mn, nan);
      const double r = ess_finish(P, d, lane, mx, mn, nan);
      n_bad += r != r ? 1u : 0u;
      if (lane == 0) P.out[row] = r;
      __syncthreads();  // (the next row overwrites d)
    }
  }
  if (P.invalid && lane == 0 && n_bad) atomicAdd(P.invalid, (unsigned long long)n_bad);
}

}  // namespace pla
