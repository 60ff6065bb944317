// PSIS leave-future-out cross-validation (Buerkner, Gabry & Vehtari 2020), forward mode, M steps ahead.  Observations are in time
// order; step j of a pass predicts rows [first + j, first + j + M) of the log-likelihood matrix ll of ONE fit (to the first `first`
// observations) given rows [0, first + j):
//     lr_j[s]  = sum_{r = first}^{first + j - 1} ll[r, s]                   the log ratios (empty sum at j = 0)
//     f_j[s]   = ll[first + j, s] + ... + ll[first + j + M - 1, s]          the future term, added in that order
//     j = 0:   elpd_j = logsumexp_s(f_j) - log S, k_j = 0                   (the fit's own step: exact)
//     j > 0:   (lw_j, k_j) = PSIS(lr_j);  elpd_j = logsumexp_s(lw_j + f_j) - logsumexp_s(lw_j)
// All arithmetic is f64 (f32 input is widened on load); NaN entries of ll count as -1e10 and are counted, +-inf are kept.
//
// THE SUMMATION RULE OF THE LOG RATIOS.  With the compile-time chunk length C = kLfoChunk = 64 and c(j) = j / C:
//     total[c]  = (..((ll[first + cC] + ll[first + cC + 1]) + ll[first + cC + 2]) + ..) + ll[first + cC + C - 1]     (C rows, in order)
//     carry[0]  = 0,   carry[c + 1] = carry[c] + total[c]                                                            (in order)
//     local[j]  = 0 at j = c(j) C, else (..(ll[first + cC] + ll[first + cC + 1]) + ..) + ll[first + j - 1]           (in order)
//     lr_j      = carry[c(j)] + local[j]
// per draw.  It is a function of j and C alone: not of the grid, of the staging block (blocks are whole chunks and the carry is
// continued from one block to the next), of the layout, of the load width or of where the matrix lives.  No floating-point atomics.
//   lfo_scan_kernel<T, VEC, false>   total[c] of the chunks of a block: a thread per (chunk, 16 bytes of draws) walks the C rows
//   lfo_carry_kernel                 totals -> carries in place, a thread per draw walks the chunks; `run` (the carry into the
//                                    block) is read at the start and left as the carry into the next block
//   lfo_scan_kernel<T, VEC, true>    lr_j = carry + local of the block, written as a compact (steps, n_draws) f64 matrix
//   VEC: 16-byte loads and stores (rows 16-byte aligned, n_draws % (16 / sizeof(T)) == 0); else a thread per draw, element loads.
//
// PREDICT.  lfo_predict_kernel<T, VEC, REG>: a wavefront per step.  Draw V (lane + 64 q) + e (V = 16 bytes / sizeof(T)) is element e
// of lane's q-th vector IN EVERY MODE, so the summation order -- per lane by q and e, then xor butterflies -- is a rule of n_draws
// and the dtype alone.  REG (n_draws <= kLfoRegDraws = 4096): the row of lw is read once into registers: its maximum and
// den = sum exp(lw - max lw), then a = lw + f in place with the M future rows read in place through the matrix's row stride, max a, and
// num = sum exp(a - max a).  Longer rows are streamed once with a running maximum per lane (the sums are rescaled when it moves;
// the lanes are merged at the end).  elpd = (max a + log num) - (max lw + log den).  lw = -inf carries weight 0; a step whose
// weights are all NaN gives NaN, and so does a step no draw of which has a finite a (every a = -inf: an observation of likelihood
// 0 under every draw) -- ON BOTH ROUTES: in registers exp(-inf - -inf) is NaN by itself, the streamed route skips a = -inf terms
// and says so at the end.  NaN entries of ll are counted once each over a pass: every step counts the last row of its window,
// step 0 of the pass the whole of it.
//
// lfo_first_high_kernel: the smallest j >= 1 with k_j > k_threshold (n_steps when there is none; NaN is not above), one workgroup,
// an integer atomic min in LDS.
#pragma once

#include "../../include/pyloo_amd.h"
#include "pla_device.h"
#include "pla_kernels.h"

namespace pla {

constexpr int kLfoChunk = 64;                    // rows per chunk of the two-level prefix sum (THE constant of the summation rule)
constexpr int kLfoWaves = 4;                     // wavefronts per workgroup of the predict kernel
constexpr int kLfoSlots = 64;                    // register slots per lane
constexpr int kLfoRegDraws = kWave * kLfoSlots;  // rows up to this length sit in a wavefront's registers (4096)

struct LfoScanParams {
  const void* in;       // the row of the block's first step (row first + j0 of the matrix), draws contiguous
  int64_t stride_obs;   // elements
  int n_draws;
  int64_t n_chunks;     // chunks of this launch
  int64_t n_rows;       // steps of the block (ratios are written for j < n_rows)
  int64_t n_load;       // rows of the block that may be read (and enter a sum): j < n_load
  double* carry;        // (n_chunks, n_draws): the totals (written) / the carries (read)
  double* out;          // (n_rows, n_draws) contiguous (ratio launch)
  unsigned long long* replaced;  // device counter (may be null)
};

struct LfoPredictParams {
  const double* lw;     // (n_steps, n_draws) contiguous log weights of the block (not read for step 0 of a pass)
  const void* ll;       // the row of the block's first step
  int64_t ll_so;        // elements between its rows (the draws are contiguous)
  int64_t n_steps;
  int n_draws;
  int horizon;
  int pass_start;       // 1: step 0 of this block is step 0 of the pass (exact, k = 0)
  double* diag;         // [n_steps] (k of step 0 of the pass is written 0; may be null)
  double* elpd;         // [n_steps] or null
  unsigned long long* replaced;  // device counter (may be null)
};

__device__ __forceinline__ double lfo_clean(double x, unsigned& n_nan, bool count) {
  const bool nan = x != x;
  n_nan += (nan && count) ? 1u : 0u;
  return nan ? -1e10 : x;
}

__device__ __forceinline__ void lfo_count(unsigned long long* replaced, unsigned n_nan) {
  if (!replaced) return;
  if (__ballot(n_nan != 0u) == 0ull) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_nan += (unsigned)__shfl_xor((int)n_nan, o);
  if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(replaced, (unsigned long long)n_nan);
}

// W consecutive draws of one row, widened
template <typename T, int W>
__device__ __forceinline__ void lfo_load(const T* p, double (&x)[W]) {
  if constexpr (W == 1) {
    x[0] = (double)p[0];
  } else if constexpr (sizeof(T) == 8) {
    const double2 t = *reinterpret_cast<const double2*>(p);
    x[0] = t.x;
    x[1] = t.y;
  } else {
    const float4 t = *reinterpret_cast<const float4*>(p);
    x[0] = (double)t.x;
    x[1] = (double)t.y;
    x[2] = (double)t.z;
    x[3] = (double)t.w;
  }
}

template <int W>
__device__ __forceinline__ void lfo_store(double* p, const double (&x)[W]) {
  if constexpr (W == 1) {
    p[0] = x[0];
  } else {
#pragma unroll
    for (int e = 0; e < W; e += 2) *reinterpret_cast<double2*>(p + e) = make_double2(x[e], x[e + 1]);
  }
}

// ---- prefix sums -----------------------------------------------------------------------------------------------------------------
// eight rows of a chunk: loads first, then (ratio launch) the stores of carry + local, each before its row enters `local`
template <typename T, int W, bool WRITE, bool WHOLE>
__device__ __forceinline__ void lfo_scan_rows(const LfoScanParams& P, const T* ip, int64_t j, int d, const double (&cr)[W], double (&acc)[W],
                                              unsigned& n_nan) {
  constexpr int U = 8;
  double x[U][W];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (WHOLE || j + u < P.n_load) {  // (uniform over the workgroup)
      lfo_load<T, W>(ip + (j + u) * P.stride_obs, x[u]);
#pragma unroll
      for (int e = 0; e < W; ++e) x[u][e] = lfo_clean(x[u][e], n_nan, true);
    } else {
#pragma unroll
      for (int e = 0; e < W; ++e) x[u][e] = 0.0;
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if constexpr (WRITE) {
      if (WHOLE || j + u < P.n_rows) {
        double o[W];
#pragma unroll
        for (int e = 0; e < W; ++e) o[e] = cr[e] + acc[e];
        lfo_store<W>(P.out + (j + u) * (int64_t)P.n_draws + d, o);
      }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] += x[u][e];
  }
}

template <typename T, bool VEC, bool WRITE>
__global__ __launch_bounds__(256) void lfo_scan_kernel(LfoScanParams P) {
  constexpr int W = VEC ? 16 / (int)sizeof(T) : 1;
  const int S = P.n_draws;
  const int64_t n_db = (S + W * 256 - 1) / (W * 256), n_units = P.n_chunks * n_db;
  unsigned n_nan = 0;
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int64_t c = u / n_db;
    const int d = ((int)(u - c * n_db) * 256 + (int)threadIdx.x) * W;
    if (d >= S) continue;
    const T* ip = reinterpret_cast<const T*>(P.in) + d;
    const int64_t j0 = c * kLfoChunk;
    double acc[W], cr[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = cr[e] = 0.0;
    if constexpr (WRITE) {
#pragma unroll
      for (int e = 0; e < W; ++e) cr[e] = P.carry[c * (int64_t)S + d + e];
    }
    // a chunk every row of which is read (and, in the ratio launch, written) takes the loads without a condition
    const bool whole = j0 + kLfoChunk <= P.n_load && (!WRITE || j0 + kLfoChunk <= P.n_rows);
    if (whole) {
#pragma unroll 1
      for (int i = 0; i < kLfoChunk; i += 8) lfo_scan_rows<T, W, WRITE, true>(P, ip, j0 + i, d, cr, acc, n_nan);
    } else {
#pragma unroll 1
      for (int i = 0; i < kLfoChunk; i += 8) lfo_scan_rows<T, W, WRITE, false>(P, ip, j0 + i, d, cr, acc, n_nan);
    }
    if constexpr (!WRITE) lfo_store<W>(P.carry + c * (int64_t)S + d, acc);
  }
  if constexpr (WRITE) lfo_count(P.replaced, n_nan);
}

#ifndef PLA_LFO_HELPERS_ONLY  // (pla_lfo_bw.h takes the __device__ helpers and the templates; a second unit must not define these)
// carry[c] = run + total[0] + ... + total[c - 1] in place of total[c]; run += the n_totals totals there are (the last chunk of the
// last block has none)
__global__ __launch_bounds__(256) void lfo_carry_kernel(double* carry, double* run, int64_t n_chunks, int64_t n_totals, int n_draws) {
  const int d = (int)(blockIdx.x * 256 + threadIdx.x);
  if (d >= n_draws) return;
  double r = run[d];
  double* p = carry + d;
#pragma unroll 4
  for (int64_t c = 0; c < n_chunks; ++c) {
    const double t = c < n_totals ? p[c * (int64_t)n_draws] : 0.0;
    p[c * (int64_t)n_draws] = r;
    r += t;
  }
  run[d] = r;
}
#endif

// ---- predict: a wavefront per step ------------------------------------------------------------------------------------------------
// lane's vector at draw `base` of a row of lw (f64, unit stride); CLAMP: -inf past the row (such a lane reads the row's last vector
// or element instead: clamped addresses and selects, no branch around a load)
template <int V, bool VEC, bool CLAMP>
__device__ __forceinline__ void lfo_load_lw(const double* p, int base, int S, bool zero, double (&x)[V]) {
#pragma unroll
  for (int e = 0; e < V; e += (VEC ? 2 : 1)) {
    const bool ok = !CLAMP || base + e < S;
    if (zero) {  // (step 0 of a pass: every weight is 1; wave-uniform)
      x[e] = ok ? 0.0 : -pinf();
      if constexpr (VEC) x[e + 1] = x[e];
    } else if constexpr (VEC) {  // (n_draws is even: a pair is inside the row or past it as a whole)
      const double2 t = *reinterpret_cast<const double2*>(p + (ok ? base + e : S - 2));
      x[e] = ok ? t.x : -pinf();
      x[e + 1] = ok ? t.y : -pinf();
    } else {
      const double t = p[ok ? base + e : S - 1];
      x[e] = ok ? t : -pinf();
    }
  }
}

// ... of a row of ll: NaN -> -1e10, 0 past the row
template <typename T, int V, bool VEC, bool CLAMP>
__device__ __forceinline__ void lfo_load_ll(const T* p, int base, int S, bool count, unsigned& n_nan, double (&x)[V]) {
  if constexpr (VEC) {
    const bool ok = !CLAMP || base < S;
    double t[V];
    lfo_load<T, V>(p + (ok ? base : S - V), t);
#pragma unroll
    for (int e = 0; e < V; ++e) x[e] = ok ? lfo_clean(t[e], n_nan, count) : 0.0;
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const bool ok = !CLAMP || base + e < S;
      const double t = (double)p[ok ? base + e : S - 1];
      x[e] = ok ? lfo_clean(t, n_nan, count) : 0.0;
    }
  }
}

// f = the M rows of the window at lane's vector, added in order (four rows in flight)
template <typename T, int V, bool VEC, bool CLAMP>
__device__ __forceinline__ void lfo_future(const T* fp, int64_t so, int M, int base, int S, bool count_all, unsigned& n_nan,
                                           double (&f)[V]) {
  lfo_load_ll<T, V, VEC, CLAMP>(fp, base, S, count_all || M == 1, n_nan, f);
#pragma unroll 1
  for (int m0 = 1; m0 < M; m0 += 4) {
    double v[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + u < M ? m0 + u : M - 1;  // (a row past the window: the last one again, neither counted nor added)
      lfo_load_ll<T, V, VEC, CLAMP>(fp + (int64_t)m * so, base, S, m0 + u < M && (count_all || m == M - 1), n_nan, v[u]);
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
__global__ __launch_bounds__(kWave * kLfoWaves) __attribute__((amdgpu_waves_per_eu(2))) void lfo_predict_kernel(LfoPredictParams P) {
  constexpr int V = 16 / (int)sizeof(T), NQ = kLfoSlots / V;
  constexpr int kLfoBatch = 16 / V;  // vectors of a future row in flight per lane (the register budget decides)
  const int S = P.n_draws, M = P.horizon;
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int nq = (S + kWave * V - 1) / (kWave * V);  // vectors per lane (wave-uniform)
  const int64_t nw = (int64_t)gridDim.x * kLfoWaves;
  unsigned n_nan = 0;
  for (int64_t j = (int64_t)blockIdx.x * kLfoWaves + wv; j < P.n_steps; j += nw) {
    const bool exact = P.pass_start != 0 && j == 0;
    const double* lp = P.lw + j * (int64_t)S;
    const T* fp = reinterpret_cast<const T*>(P.ll) + j * P.ll_so;
    double m_lw, den, m_a, num;
    if constexpr (REG) {
      // every lane's vectors q < nq - 1 lie inside the row as a whole: plain loads; only the last one is clamped and masked.  Each
      // sweep has its own opaque copy of that count, so that the conditions q < nq - 1 are scalar compares inside the sweep and not
      // masks computed once and kept in scalar registers across the row
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
      // the whole vectors in batches of kLfoBatch: the window's rows one after the other, a batch's loads of a row in flight at once
      // (a vector past the count repeats the last whole one, neither counted nor added: no branch around a load)
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
            const bool cnt = exact || m == M - 1;
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
        lfo_future<T, V, VEC, true>(fp, P.ll_so, M, (n3 * kWave + lane) * V, S, exact, n_nan, f);
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
        lfo_future<T, V, VEC, true>(fp, P.ll_so, M, base, S, exact, n_nan, f);
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

#ifndef PLA_LFO_HELPERS_ONLY
// ---- the first step above the threshold -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lfo_first_high_kernel(const double* diag, int64_t n_steps, double threshold, long long* out) {
  __shared__ unsigned long long best;
  if (threadIdx.x == 0) best = (unsigned long long)n_steps;
  __syncthreads();
  unsigned long long mine = (unsigned long long)n_steps;
  for (int64_t j = 1 + threadIdx.x; j < n_steps; j += 256)
    if (diag[j] > threshold) {  // (false for NaN)
      mine = (unsigned long long)j;
      break;
    }
  if (mine < (unsigned long long)n_steps) atomicMin(&best, mine);
  __syncthreads();
  if (threadIdx.x == 0) *out = (long long)best;
}
#endif

}  // namespace pla
