// PSIS leave-future-out cross-validation, BACKWARD mode (Buerkner, Gabry & Vehtari 2020, as the paper states its algorithm): the
// pass serves ONE fit that saw the first `last` observations (the first pass of a walk: all of them) and walks the steps downward,
//     t_0 = min(last, n_obs - M),   t_j = t_0 - j,   j = 0 .. n_steps - 1
//     f_j[s]   = ll[t_j, s] + ... + ll[t_j + M - 1, s]                          the future term, added in that order (as forward)
//     lr_j[s]  = - sum_{r = t_j}^{last - 1} ll[r, s]                            the rows the fit saw and the step must not
//     t_j = last:  elpd_j = logsumexp_s(f_j) - log S, k_j = 0                   (exact; only j = 0 can be)
//     t_j < last:  (lw_j, k_j) = PSIS(lr_j);  elpd_j = logsumexp_s(lw_j + f_j) - logsumexp_s(lw_j)
// All arithmetic is f64, NaN entries count as -1e10, +-inf are kept (pla_lfo.h, whose __device__ helpers these kernels use).
//
// THE SUMMATION RULE is forward mode's, anchored AT THE FIT: with a_q = ll[last - 1 - q] (the same rows, walked downward) and
// C = kLfoChunk,
//     total[c] = (..(a_{cC} + a_{cC + 1}) + ..) + a_{cC + C - 1},   carry[0] = 0,   carry[c + 1] = carry[c] + total[c]
//     local[q] = 0 at q = c(q) C, else (..(a_{cC} + a_{cC + 1}) + ..) + a_{q - 1},     P[q] = carry[c(q)] + local[q],     c(q) = q / C
//     lr_j     = -P[last - t_j]                                                         (the negation is exact)
// a function of last - t_j and C alone.  The steps of a pass begin at q = last - t_0 (0 .. M); the sums begin at q = 0.
//   lfo_bw_scan_kernel<T, VEC, false>  total[c] of the chunks of a block of q: a thread per (chunk, 16 bytes of draws) walks C rows down
//   lfo_carry_kernel (pla_lfo.h)       totals -> carries in place, continued from block to block through `run`: forward mode's
//                                      kernel as it is (launch_lfo_carry), the rule being the same in q
//   lfo_bw_scan_kernel<T, VEC, true>   -(carry + local) of the q of the block, a compact (n_rows, n_draws) f64 matrix (the q below the
//                                      first step of the pass, M at the most, are written too: the weights pass begins behind them)
//
// lfo_bw_predict_kernel<T, VEC, REG>: forward mode's predict kernel (a wavefront per step, the same draw-to-lane mapping, the same
// two routes) with the step stride negative and the window stride positive; the exact step is step 0 of a pass whose t_0 = last;
// every step counts the NaN entries of the FIRST row of its window, step 0 of the pass those of the whole of it.
//
// lfo_bw_first_high_kernel: the smallest j >= j_min with k_j > k_threshold, else n_steps (j_min = 1 when step 0 is exact).
#pragma once

#define PLA_LFO_HELPERS_ONLY
#include "pla_lfo.h"

namespace pla {

struct LfoBwScanParams {
  const void* in;       // row last - 1 - q of the block's first q, draws contiguous; the row of local q is `in - q stride_obs`
  int64_t stride_obs;   // elements, positive
  int n_draws;
  int64_t n_chunks;     // chunks of this launch
  int64_t n_rows;       // q of the block (ratios exist for q < n_rows)
  int64_t n_load;       // rows of the block that may be read (and enter a sum): q < n_load
  double* carry;        // (n_chunks, n_draws): the totals (written) / the carries (read)
  double* out;          // (n_rows, n_draws) contiguous (ratio launch)
};

struct LfoBwPredictParams {
  const double* lw;     // (n_steps, n_draws) contiguous log weights of the block (not read for an exact step)
  const void* ll;       // row t of the block's first step; step j of the block is `ll - j ll_so`, its window goes upward
  int64_t ll_so;        // elements between rows, positive (the draws are contiguous)
  int64_t n_steps;
  int n_draws;
  int horizon;
  int pass_start;       // 1: step 0 of this block is step 0 of the pass (it counts the NaN entries of its whole window)
  int exact0;           // 1: ... and it is the fit's own step, t_0 = last (exact, k = 0)
  double* diag;         // [n_steps] (only k = 0 of an exact step is written; may be null)
  double* elpd;         // [n_steps] or null
  unsigned long long* replaced;  // device counter (may be null)
};

// ---- prefix sums down the rows -----------------------------------------------------------------------------------------------------
// eight rows of a chunk: loads first, then (ratio launch) the stores of -(carry + local), each before its row enters `local`.
// ip, op: the chunk's first row of the matrix (walked downward) and of out at this thread's draws; i: the row within the chunk; rows
// i < n_ld are read, rows i < n_wr written (32-bit bounds of the chunk, so that the conditions are scalar compares)
template <typename T, int W, bool WRITE, bool WHOLE>
__device__ __forceinline__ void lfo_bw_scan_rows(const T* ip, int64_t so, double* op, int S, int i, int n_ld, int n_wr,
                                                 const double (&cr)[W], double (&acc)[W]) {
  constexpr int U = 8;
  double x[U][W];
  unsigned unused = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (WHOLE || i + u < n_ld) {  // (uniform over the workgroup)
      lfo_load<T, W>(ip - (int64_t)(i + u) * so, x[u]);
#pragma unroll
      for (int e = 0; e < W; ++e) x[u][e] = lfo_clean(x[u][e], unused, false);
    } else {
#pragma unroll
      for (int e = 0; e < W; ++e) x[u][e] = 0.0;
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if constexpr (WRITE) {
      if (WHOLE || i + u < n_wr) {
        double o[W];
#pragma unroll
        for (int e = 0; e < W; ++e) o[e] = -(cr[e] + acc[e]);
        lfo_store<W>(op + (int64_t)(i + u) * S, o);
      }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] += x[u][e];
  }
}

__device__ __forceinline__ int lfo_bw_clamp_chunk(int64_t v) { return v < 0 ? 0 : v > kLfoChunk ? kLfoChunk : (int)v; }

template <typename T, bool VEC, bool WRITE>
__global__ __launch_bounds__(256) void lfo_bw_scan_kernel(LfoBwScanParams P) {
  constexpr int W = VEC ? 16 / (int)sizeof(T) : 1;
  const int S = P.n_draws;
  const int64_t n_db = (S + W * 256 - 1) / (W * 256), n_units = P.n_chunks * n_db;
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int64_t c = u / n_db;
    const int d = ((int)(u - c * n_db) * 256 + (int)threadIdx.x) * W;
    if (d >= S) continue;
    const int64_t q0 = c * kLfoChunk;
    const T* ip = reinterpret_cast<const T*>(P.in) + d - q0 * P.stride_obs;
    double* op = WRITE ? P.out + q0 * (int64_t)S + d : nullptr;
    const int n_ld = lfo_bw_clamp_chunk(P.n_load - q0), n_wr = lfo_bw_clamp_chunk(P.n_rows - q0);
    double acc[W], cr[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = cr[e] = 0.0;
    if constexpr (WRITE) {
#pragma unroll
      for (int e = 0; e < W; ++e) cr[e] = P.carry[c * (int64_t)S + d + e];
    }
    // a chunk every row of which is read (and, in the ratio launch, written) takes the loads without a condition
    const bool whole = n_ld == kLfoChunk && (!WRITE || n_wr == kLfoChunk);
    if (whole) {
#pragma unroll 1
      for (int i = 0; i < kLfoChunk; i += 8) lfo_bw_scan_rows<T, W, WRITE, true>(ip, P.stride_obs, op, S, i, n_ld, n_wr, cr, acc);
    } else {
#pragma unroll 1
      for (int i = 0; i < kLfoChunk; i += 8) lfo_bw_scan_rows<T, W, WRITE, false>(ip, P.stride_obs, op, S, i, n_ld, n_wr, cr, acc);
    }
    if constexpr (!WRITE) lfo_store<W>(P.carry + c * (int64_t)S + d, acc);
  }
}

// ---- predict: a wavefront per step ------------------------------------------------------------------------------------------------
// f = the M rows of the window at lane's vector, added in order (four rows in flight); the first row is counted, the others when
// count_all
template <typename T, int V, bool VEC, bool CLAMP>
__device__ __forceinline__ void lfo_bw_future(const T* fp, int64_t so, int M, int base, int S, bool count_all, unsigned& n_nan,
                                              double (&f)[V]) {
  lfo_load_ll<T, V, VEC, CLAMP>(fp, base, S, true, n_nan, f);
#pragma unroll 1
  for (int m0 = 1; m0 < M; m0 += 4) {
    double v[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + u < M ? m0 + u : M - 1;  // (a row past the window: the last one again, neither counted nor added)
      lfo_load_ll<T, V, VEC, CLAMP>(fp + (int64_t)m * so, base, S, m0 + u < M && count_all, n_nan, v[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (m0 + u < M) {
#pragma unroll
        for (int e = 0; e < V; ++e) f[e] += v[u][e];
      }
  }
}

template <typename T, bool VEC, bool REG>
__global__ __launch_bounds__(kWave * kLfoWaves) __attribute__((amdgpu_waves_per_eu(2))) void lfo_bw_predict_kernel(LfoBwPredictParams P) {
  constexpr int V = 16 / (int)sizeof(T), NQ = kLfoSlots / V;
  constexpr int kLfoBatch = 16 / V;  // vectors of a future row in flight per lane (the register budget decides)
  const int S = P.n_draws, M = P.horizon;
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int nq = (S + kWave * V - 1) / (kWave * V);  // vectors per lane (wave-uniform)
  const int64_t nw = (int64_t)gridDim.x * kLfoWaves;
  unsigned n_nan = 0;
  for (int64_t j = (int64_t)blockIdx.x * kLfoWaves + wv; j < P.n_steps; j += nw) {
    const bool all = P.pass_start != 0 && j == 0;  // (step 0 of the pass: the whole window is counted)
    const bool exact = all && P.exact0 != 0;
    const double* lp = P.lw + j * (int64_t)S;
    const T* fp = reinterpret_cast<const T*>(P.ll) - j * P.ll_so;
    double m_lw, den, m_a, num;
    if constexpr (REG) {
      // as lfo_predict_kernel: plain loads for a lane's vectors q < nq - 1, the last one clamped and masked, an opaque copy of the
      // count per sweep
      int n1 = nq - 1;
      asm volatile("" : "+s"(n1));
      double x[NQ - 1][V], xl[V];
      double mx = -pinf();
#pragma unroll
      for (int q = 0; q < NQ - 1; ++q)
        if (q < n1) {
          lfo_load_lw<V, VEC, false>(lp, (q * kWave + lane) * V, S, exact, x[q]);
#pragma unroll
          for (int e = 0; e < V; ++e) mx = fmax(mx, x[q][e]);
        }
      lfo_load_lw<V, VEC, true>(lp, (n1 * kWave + lane) * V, S, exact, xl);
#pragma unroll
      for (int e = 0; e < V; ++e) mx = fmax(mx, xl[e]);
      m_lw = wave_reduce<OpMax>(mx);
      int n2 = n1;
      asm volatile("" : "+s"(n2));
      den = 0.0;
#pragma unroll
      for (int q = 0; q < NQ - 1; ++q)
        if (q < n2) {
#pragma unroll
          for (int e = 0; e < V; ++e) den += exp(x[q][e] - m_lw);
        }
#pragma unroll
      for (int e = 0; e < V; ++e) den += exp(xl[e] - m_lw);  // (past the row: exp(-inf) = 0)
      int n3 = n2;
      asm volatile("" : "+s"(n3));
      mx = -pinf();
#pragma unroll
      for (int q0 = 0; q0 < NQ - 1; q0 += kLfoBatch) {
        if (q0 < n3) {
          double f[kLfoBatch][V];
#pragma unroll
          for (int u = 0; u < kLfoBatch; ++u)
#pragma unroll
            for (int e = 0; e < V; ++e) f[u][e] = 0.0;
#pragma unroll 1
          for (int m = 0; m < M; ++m) {
            const T* rp = fp + (int64_t)m * P.ll_so;
            const bool cnt = all || m == 0;
            double v[kLfoBatch][V];
#pragma unroll
            for (int u = 0; u < kLfoBatch; ++u) {
              const int qq = q0 + u < n3 ? q0 + u : n3 - 1;
              lfo_load_ll<T, V, VEC, false>(rp, (qq * kWave + lane) * V, S, cnt && q0 + u < n3, n_nan, v[u]);
            }
#pragma unroll
            for (int u = 0; u < kLfoBatch; ++u)
#pragma unroll
              for (int e = 0; e < V; ++e) f[u][e] += v[u][e];
          }
#pragma unroll
          for (int u = 0; u < kLfoBatch; ++u)
            if (q0 + u < NQ - 1 && q0 + u < n3) {
#pragma unroll
              for (int e = 0; e < V; ++e) {
                x[q0 + u][e] += f[u][e];
                mx = fmax(mx, x[q0 + u][e]);
              }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      {
        double f[V];
        lfo_bw_future<T, V, VEC, true>(fp, P.ll_so, M, (n3 * kWave + lane) * V, S, all, n_nan, f);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          xl[e] += f[e];  // (past the row: -inf + 0)
          mx = fmax(mx, xl[e]);
        }
      }
      m_a = wave_reduce<OpMax>(mx);
      int n4 = n3;
      asm volatile("" : "+s"(n4));
      num = 0.0;
#pragma unroll
      for (int q = 0; q < NQ - 1; ++q)
        if (q < n4) {
#pragma unroll
          for (int e = 0; e < V; ++e) num += exp(x[q][e] - m_a);
        }
#pragma unroll
      for (int e = 0; e < V; ++e) num += exp(xl[e] - m_a);
    } else {
      // streamed: per lane a running maximum of lw and of a, the sums rescaled when a maximum moves (they are 0 while it is -inf)
      double ml = -pinf(), ma = -pinf();
      den = 0.0;
      num = 0.0;
#pragma unroll 1
      for (int q = 0; q < nq; ++q) {
        double x[V], f[V];
        const int base = (q * kWave + lane) * V;
        lfo_load_lw<V, VEC, true>(lp, base, S, exact, x);
        lfo_bw_future<T, V, VEC, true>(fp, P.ll_so, M, base, S, all, n_nan, f);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const double w = x[e], a = x[e] + f[e];
          if (w > ml) {
            den *= exp(ml - w);
            ml = w;
          }
          den += w == -pinf() ? 0.0 : exp(w - ml);
          if (a > ma) {
            num *= exp(ma - a);
            ma = a;
          }
          num += a == -pinf() ? 0.0 : exp(a - ma);
        }
      }
      m_lw = wave_reduce<OpMax>(ml);
      m_a = wave_reduce<OpMax>(ma);
      den = ml == -pinf() ? den : den * exp(ml - m_lw);  // (a lane without a finite weight holds 0, or NaN from a NaN weight)
      num = ma == -pinf() ? num : num * exp(ma - m_a);
      num = m_a == -pinf() ? m_a - m_a : num;  // (no draw has a finite a: NaN, the register route's exp(-inf - -inf); wave-uniform)
    }
    den = wave_reduce<OpSum>(den);
    num = wave_reduce<OpSum>(num);
    if (lane == 0) {
      if (P.elpd) P.elpd[j] = (m_a + log(num)) - (m_lw + log(den));
      if (exact && P.diag) P.diag[j] = 0.0;
    }
  }
  lfo_count(P.replaced, n_nan);
}

// ---- the first step above the threshold -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lfo_bw_first_high_kernel(const double* diag, int64_t n_steps, int64_t j_min, double threshold,
                                                                long long* out) {
  __shared__ unsigned long long best;
  if (threadIdx.x == 0) best = (unsigned long long)n_steps;
  __syncthreads();
  unsigned long long mine = (unsigned long long)n_steps;
  for (int64_t j = j_min + threadIdx.x; j < n_steps; j += 256)
    if (diag[j] > threshold) {  // (false for NaN)
      mine = (unsigned long long)j;
      break;
    }
  if (mine < (unsigned long long)n_steps) atomicMin(&best, mine);
  __syncthreads();
  if (threadIdx.x == 0) *out = (long long)best;
}

}  // namespace pla
