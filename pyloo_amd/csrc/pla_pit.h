// LOO-PIT kernels: the leave-one-out probability integral transform (ArviZ's loo_pit, the ppc_loo_pit_* input of bayesplot)
//     pit_le[r] = sum_{yh[r,s] <= y[r]} w[r,s]        pit_lt[r] = sum_{yh[r,s] < y[r]} w[r,s]
// from the log weights lw of observation r (of any normalisation: w = exp(lw - max) / sum exp(lw - max)), its posterior-predictive
// draws yh and its observed value y.
//
// PREPARE.  pit_prepare_row_kernel / pit_prepare_tile_kernel write -ll of a block of observations as a compact draws-fastest block
// (row pitch = n_draws) in the dtype of ll: NaN becomes -1e10 before the negation (loo.py:218-227) and is counted, +-inf are kept.
// The row kernel reads any strides (coalesced when the draws are contiguous); the tile kernel takes observations-fastest input
// through a 64 x 64 tile of LDS, reads and writes coalesced.
//
// PIT.  All arithmetic is f64 (f32 input is widened on load).  With m = max_s lw[r,s] and e_s = exp(lw[r,s] - m) there are three
// accumulators, den += e_s, le += (yh <= y ? e_s : 0), lt += (yh < y ? e_s : 0): the same term in the same order in all three, so
// that a row without yh == y has pit_lt == pit_le bit for bit, a row with every draw <= y gives exactly 1 and a row with none
// exactly 0.  Comparisons are IEEE (a NaN draw or a NaN y is never counted), lw = -inf carries weight 0 and a row whose weights
// are all NaN or all -inf gives NaN.  No floating-point atomics: an observation's result depends on its own row alone, whatever
// the grid or the block of observations it comes in.
//   pit_wave_kernel<T, MODE, REG>  a wavefront per observation.  Draw VEC * (lane + 64 q) + e (VEC = 16 bytes / sizeof(T)) is
//                                  element e of lane's q-th vector IN EVERY MODE, so the summation order -- per lane by q and e,
//                                  then xor butterflies -- is a rule of n_draws and the dtype alone:
//                                    MODE kPitVec      16-byte loads (both rows 16-byte aligned, n_draws % VEC == 0)
//                                    MODE kPitElem     element loads, unit draw strides
//                                    MODE kPitStrided  element loads with the matrices' draw strides (correct, not fast)
//                                  REG (n_draws <= kPitRegDraws): the row of lw is read once into registers (maximum, then sums);
//                                  else it is streamed in two sweeps.  yh is read once in both.
//   pit_lane_kernel<T>             both matrices observations-fastest: a lane per observation walks the draws in order with a
//                                  running maximum and three sums rescaled alike when the maximum moves.
#pragma once

#include "../../include/pyloo_amd.h"
#include "pla_device.h"
#include "pla_kernels.h"

namespace pla {

constexpr int kPitWaves = 4;                        // wavefronts per workgroup of the wave kernel
constexpr int kPitSlots = 64;                       // register slots per lane
constexpr int kPitRegDraws = kWave * kPitSlots;     // rows up to this length sit in a wavefront's registers (4096)
enum PitMode { kPitVec = 0, kPitElem = 1, kPitStrided = 2 };

struct PitParams {
  const void* lw;   // (n_obs, n_draws) log weights
  const void* yh;   // (n_obs, n_draws) posterior-predictive draws, the dtype of lw
  const double* y;  // [n_obs]
  int64_t n_obs;
  int n_draws;
  int64_t lw_so, lw_sd, yh_so, yh_sd;  // elements
  double* pit_le;   // [n_obs]
  double* pit_lt;   // [n_obs] or null
};

struct PitPrepareParams {
  const void* in;  // first observation of the block
  void* out;       // (n_rows, n_draws) contiguous
  int64_t n_rows;
  int n_draws;
  int64_t stride_obs, stride_draw;  // elements
  unsigned long long* replaced;     // device counter (may be null)
};

// ---- prepare --------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T pit_neg_ll(T x, unsigned& n_nan) {
  const bool nan = x != x;
  n_nan += nan ? 1u : 0u;
  return -(nan ? (T)-1e10 : x);
}

__device__ __forceinline__ void pit_count(unsigned long long* replaced, unsigned n_nan) {
  if (!replaced) return;
  if (__ballot(n_nan != 0u) == 0ull) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_nan += (unsigned)__shfl_xor((int)n_nan, o);
  if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(replaced, (unsigned long long)n_nan);
}

// a workgroup per (row, 1024 draws): thread t takes draws t, t + 256, ...
template <typename T>
__global__ __launch_bounds__(256) void pit_prepare_row_kernel(PitPrepareParams P) {
  const int S = P.n_draws;
  const int64_t n_db = (S + 1023) / 1024, n_units = n_db * P.n_rows;
  unsigned n_nan = 0;
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int64_t r = u / n_db;
    const int d0 = (int)(u - r * n_db) * 1024 + (int)threadIdx.x;
    const T* ip = reinterpret_cast<const T*>(P.in) + r * P.stride_obs;
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
__global__ __launch_bounds__(256) void pit_prepare_tile_kernel(PitPrepareParams P) {
  __shared__ T tile[64][65];
  const int S = P.n_draws;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t n_tr = (P.n_rows + 63) / 64, n_td = (S + 63) / 64, n_units = n_tr * n_td;
  unsigned n_nan = 0;
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int64_t tr = u % n_tr, td = u / n_tr;  // neighbouring workgroups: neighbouring observations of the same draws
    const int64_t r0 = tr * 64;
    const int d0 = (int)td * 64;
#pragma unroll 4
    for (int j = ty; j < 64; j += 4) {  // tile[draw][observation]
      const int64_t r = r0 + tx;
      const int d = d0 + j;
      if (r < P.n_rows && d < S) tile[j][tx] = pit_neg_ll(reinterpret_cast<const T*>(P.in)[(int64_t)d * P.stride_draw + r], n_nan);
    }
    __syncthreads();
#pragma unroll 4
    for (int j = ty; j < 64; j += 4) {
      const int64_t r = r0 + j;
      const int d = d0 + tx;
      if (r < P.n_rows && d < S) reinterpret_cast<T*>(P.out)[r * S + d] = tile[tx][j];
    }
    __syncthreads();
  }
  pit_count(P.replaced, n_nan);
}

// ---- PIT: a wavefront per observation --------------------------------------------------------------------------------------------
// lane's q-th vector of a row: x[e] = p[(VEC * (lane + 64 q) + e) * sd], `fill` where that is past the row (such a lane reads the
// row's last vector or element instead: clamped addresses and selects, no branch around a load)
template <typename T, int MODE, int VEC>
__device__ __forceinline__ void pit_load(const T* p, int64_t sd, int base, int S, double fill, double (&x)[VEC]) {
  if constexpr (MODE == kPitVec) {  // (n_draws % VEC == 0: a vector is inside the row or past it as a whole)
    const bool ok = base < S;
    const int b = ok ? base : S - VEC;
    if constexpr (VEC == 2) {
      const double2 t = *reinterpret_cast<const double2*>(p + b);
      x[0] = ok ? t.x : fill;
      x[1] = ok ? t.y : fill;
    } else {
      const float4 t = *reinterpret_cast<const float4*>(p + b);
      x[0] = ok ? (double)t.x : fill;
      x[1] = ok ? (double)t.y : fill;
      x[2] = ok ? (double)t.z : fill;
      x[3] = ok ? (double)t.w : fill;
    }
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int d = base + e;
      const bool ok = d < S;
      const int dd = ok ? d : S - 1;
      const double t = (double)p[MODE == kPitStrided ? (int64_t)dd * sd : (int64_t)dd];
      x[e] = ok ? t : fill;
    }
  }
}

// ... a vector that lies inside the row in every lane
template <typename T, int MODE, int VEC>
__device__ __forceinline__ void pit_load_whole(const T* p, int64_t sd, int base, double (&x)[VEC]) {
  if constexpr (MODE == kPitVec) {
    if constexpr (VEC == 2) {
      const double2 t = *reinterpret_cast<const double2*>(p + base);
      x[0] = t.x;
      x[1] = t.y;
    } else {
      const float4 t = *reinterpret_cast<const float4*>(p + base);
      x[0] = (double)t.x;
      x[1] = (double)t.y;
      x[2] = (double)t.z;
      x[3] = (double)t.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) x[e] = (double)p[MODE == kPitStrided ? (int64_t)(base + e) * sd : (int64_t)(base + e)];
  }
}

// one term into the three accumulators
__device__ __forceinline__ void pit_term(double e, double v, double yr, double& den, double& le, double& lt) {
  den += e;
  le += v <= yr ? e : 0.0;
  lt += v < yr ? e : 0.0;
}

__device__ __forceinline__ void pit_store(const PitParams& P, int64_t r, double den, double le, double lt) {
  den = wave_reduce<OpSum>(den);
  le = wave_reduce<OpSum>(le);
  lt = wave_reduce<OpSum>(lt);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    P.pit_le[r] = le / den;
    if (P.pit_lt) P.pit_lt[r] = lt / den;
  }
}

template <typename T, int MODE, bool REG>
__global__ __launch_bounds__(kWave * kPitWaves) void pit_wave_kernel(PitParams P) {
  constexpr int VEC = 16 / (int)sizeof(T), NQ = kPitSlots / VEC;
  const int S = P.n_draws;
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int nq = (S + kWave * VEC - 1) / (kWave * VEC);  // vectors per lane (wave-uniform)
  const int64_t nw = (int64_t)gridDim.x * kPitWaves;
  for (int64_t r = (int64_t)blockIdx.x * kPitWaves + wv; r < P.n_obs; r += nw) {
    const T* lp = reinterpret_cast<const T*>(P.lw) + r * P.lw_so;
    const T* yp = reinterpret_cast<const T*>(P.yh) + r * P.yh_so;
    const double yr = P.y[r];
    double den = 0.0, le = 0.0, lt = 0.0;
    if constexpr (REG) {
      // every lane's vectors q < nq - 1 lie inside the row as a whole: plain loads; only the last one is clamped and masked
      int nfull = nq - 1;
      asm volatile("" : "+s"(nfull));  // (opaque inside the row loop: the 31 conditions q < nfull are not to be hoisted out of it as masks ...)
      double x[NQ - 1][VEC], xl[VEC];
      double mx = -pinf();
#pragma unroll
      for (int q = 0; q < NQ - 1; ++q) {
        if (q < nfull) {
          pit_load_whole<T, MODE, VEC>(lp, P.lw_sd, (q * kWave + lane) * VEC, x[q]);
#pragma unroll
          for (int e = 0; e < VEC; ++e) mx = fmax(mx, x[q][e]);
        }
      }
      pit_load<T, MODE, VEC>(lp, P.lw_sd, (nfull * kWave + lane) * VEC, S, -pinf(), xl);
#pragma unroll
      for (int e = 0; e < VEC; ++e) mx = fmax(mx, xl[e]);
      const double m = wave_reduce<OpMax>(mx);
      int nsum = nfull;
      asm volatile("" : "+s"(nsum));  // (... nor kept from the sweep above for the one below)
#pragma unroll
      for (int q = 0; q < NQ - 1; ++q) {
        if (q < nsum) {
          double v[VEC];
          pit_load_whole<T, MODE, VEC>(yp, P.yh_sd, (q * kWave + lane) * VEC, v);
#pragma unroll
          for (int e = 0; e < VEC; ++e) pit_term(exp(x[q][e] - m), v[e], yr, den, le, lt);
        }
      }
      double vl[VEC];
      pit_load<T, MODE, VEC>(yp, P.yh_sd, (nfull * kWave + lane) * VEC, S, qnan(), vl);
#pragma unroll
      for (int e = 0; e < VEC; ++e) pit_term(exp(xl[e] - m), vl[e], yr, den, le, lt);  // (past the row: exp(-inf - m) = 0)
    } else {
      constexpr int U = 8 / VEC;  // vectors of a batch: eight elements of each matrix in flight per lane
      double mx = -pinf();
#pragma unroll 1
      for (int q0 = 0; q0 < nq; q0 += U) {
        double x[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) pit_load<T, MODE, VEC>(lp, P.lw_sd, ((q0 + u) * kWave + lane) * VEC, S, -pinf(), x[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int e = 0; e < VEC; ++e) mx = fmax(mx, x[u][e]);
      }
      const double m = wave_reduce<OpMax>(mx);
#pragma unroll 1
      for (int q0 = 0; q0 < nq; q0 += U) {
        double x[U][VEC], v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          pit_load<T, MODE, VEC>(lp, P.lw_sd, ((q0 + u) * kWave + lane) * VEC, S, -pinf(), x[u]);
          pit_load<T, MODE, VEC>(yp, P.yh_sd, ((q0 + u) * kWave + lane) * VEC, S, qnan(), v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int e = 0; e < VEC; ++e) pit_term(exp(x[u][e] - m), v[u][e], yr, den, le, lt);
      }
    }
    pit_store(P, r, den, le, lt);
  }
}

// ---- PIT: a lane per observation (both matrices observations-fastest) -----------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pit_lane_kernel(PitParams P) {
  constexpr int U = 8;
  const int S = P.n_draws;
  const int64_t n_blk = (P.n_obs + 255) / 256;
  for (int64_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
    const int64_t i = b * 256 + threadIdx.x;
    const bool live = i < P.n_obs;
    const int64_t ii = live ? i : P.n_obs - 1;  // (dead lanes walk a live lane's column and store nothing)
    const T* lp = reinterpret_cast<const T*>(P.lw) + ii;
    const T* yp = reinterpret_cast<const T*>(P.yh) + ii;
    const double yr = P.y[ii];
    double m = -pinf(), den = 0.0, le = 0.0, lt = 0.0;
#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += U) {
      double x[U], v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int s = s0 + u < S ? s0 + u : S - 1;
        x[u] = (double)__builtin_nontemporal_load(lp + (int64_t)s * P.lw_sd);
        v[u] = (double)__builtin_nontemporal_load(yp + (int64_t)s * P.yh_sd);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (s0 + u < S) {  // (wave-uniform)
          if (x[u] > m) {  // a new maximum: the three sums are rescaled by one factor (they are 0 while m is -inf)
            const double f = exp(m - x[u]);
            den *= f;
            le *= f;
            lt *= f;
            m = x[u];
          }
          const double e = x[u] == -pinf() ? 0.0 : exp(x[u] - m);
          pit_term(e, v[u], yr, den, le, lt);
        }
      }
    }
    if (live) {
      P.pit_le[i] = le / den;
      if (P.pit_lt) P.pit_lt[i] = lt / den;
    }
  }
}

}  // namespace pla
