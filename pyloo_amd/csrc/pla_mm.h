// Kernels of moment matching (reference: pyloo loo_moment_match.py:656-914, split_moment_match.py:132-252).
//
// One call works on a batch of B observations at once: upars (B, S, D) draws-major, D fastest, f64; log weights (B, S).
//
// a. moments.  Per b, in the reference's own formulas (loo_moment_match.py:831-833, 857-864, 891-896):
//        mean_d   = sum_s x_sd / S                                   np.mean
//        wmean_d  = sum_s w_s x_sd,  w_s = exp(lw_s)                 the weighted mean of shift()
//        var_d    = sum_s (x_sd - mean_d)^2 / S                      np.var, ddof 0 (two passes)
//        mii_d    = (sum_s w_s x_sd^2 - wmean_d^2) * S / (S - 1)     ONE pass, as shift_and_scale() has it: its cancellation is kept
//        cov_jk   = sum_s (x_sj - mean_j)(x_sk - mean_k) / (S - 1)   np.cov(rowvar=False)
//        wcov_jk  = sum_s w_s (x_sj - a_j)(x_sk - a_k) / (W - W2 / W), a = sum w x / W, W = sum w, W2 = sum w^2   np.cov(aweights=w)
//    Determinism.  The S draws are cut into tiles whose length is a constant (kMmTile draws for the vectors, kMmCovTile for the
//    matrices).  A workgroup reduces one (b, tile) at a time in a grid-stride loop, so the grid size does not matter; inside a
//    tile every lane walks its draws in ascending order and the lanes are combined in a fixed order through LDS.  Every tile's
//    partial goes to its own slot of engine workspace and a small second launch adds the slots in tile order.  No floating-point
//    atomics: the same input gives the same bits whatever the grid, the batch size or the position of b in the batch.
//    Launches: mm_sums_kernel<0> (sum x, sum w x, sum w x^2, W, W2) -> mm_mid_kernel (mean, wmean, mii, a, W, W2) ->
//    mm_sums_kernel<1> (sum (x - mean)^2) [-> mm_cov_kernel] -> mm_fin_kernel.
//    mm_cov_kernel stages kMmCovBlock draws of one b in LDS; every lane owns a fixed set of (j, k) pairs of the upper triangle
//    (pair p = lane, lane + 256, ...: at D = 64 that is 2080 pairs, at most kMmPairsPerThread = 9 a lane) and keeps their two
//    accumulators in registers over the whole tile.  Plain f64 FMA.
// b. transform.  out[b, s, :] = (((x[b, s, :] - m0[b]) * pre[b]) . map[b]^T) / post[b] + m1[b] for the rows s in [row_lo, row_hi),
//    out = x for the others; pre, map and post are optional.  Without a matrix (mm_affine_kernel) every operation is written as it
//    stands (no contraction into fma), so shift() and shift_and_scale() give NumPy's bits.  With one (mm_map_kernel, D <= 64) the
//    matrix sits transposed in LDS and a workgroup walks a chunk of rows of one b.  The split step is two calls on the original
//    draws (x_batch_stride = 0): rows [0, S/2) forward, rows [S/2, S) with the inverse matrix and post = the total scaling.
// c. ratios.  mode 0: lr = -ll + lp - lp_orig and full_lr = lp - lp_orig, NaN -> -inf, as a (2B, S) stack for one PSIS call
//    (loo_moment_match.py:784-799).  mode 1: the multiple-importance-sampling weights of the split step
//    (split_moment_match.py:219-245).  mode 2: lw + ll with NaN / +inf -> -inf (250-251).  mode 3: per b logsumexp(ll + lw) and
//    logsumexp(ll) - log S, one wave per row (loo_moment_match.py:621, 991).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pla_kernels.h"

namespace pla {

constexpr int kMmThreads = 256;
constexpr int kMmTile = 256;         // draws per tile of the vector passes
constexpr int kMmCovTile = 512;      // draws per tile of the matrix pass
constexpr int kMmCovBlock = 32;      // ... staged in LDS at a time
constexpr int kMmPairsPerThread = 9;  // ceil(64 * 65 / 2 / 256)
constexpr int kMmMapRows = 256;      // rows per chunk of mm_map_kernel

__host__ __device__ inline int64_t mm_tiles(int64_t S) { return (S + kMmTile - 1) / kMmTile; }
__host__ __device__ inline int64_t mm_cov_tiles(int64_t S) { return (S + kMmCovTile - 1) / kMmCovTile; }
__host__ __device__ inline int mm_pairs(int D) { return D * (D + 1) / 2; }
__host__ __device__ inline int mm_pow2(int D) {
  int p = 1;
  while (p < D && p < kMmThreads) p <<= 1;
  return p;
}

struct MmMomentsParams {
  const double* x;   // (B, S, D)
  const double* lw;  // (B, S)
  int64_t B, S;
  int D, want_cov;
  double* part0;  // [B][nT][3D + 2]
  double* mid;    // [B][D + 2]: a, W, W2
  double* part1;  // [B][nT][D]
  double* partc;  // [B][nTc][2][pairs]
  double* stats;  // [B][4][D]: mean, wmean, var, mii
  double* cov;    // [B][2][D][D]: cov, wcov
};

// workspace doubles of one moments call
inline int64_t mm_workspace_doubles(int64_t B, int64_t S, int D, int want_cov) {
  const int64_t nT = mm_tiles(S), nTc = mm_cov_tiles(S);
  return B * (nT * (3 * (int64_t)D + 2) + (D + 2) + nT * D + (want_cov ? nTc * 2 * mm_pairs(D) : 0));
}

// PASS 0: sum x, sum w x, sum w x^2 per (b, tile, d), W and W2 per (b, tile).  PASS 1: sum (x - mean)^2.
template <int PASS>
__global__ __launch_bounds__(kMmThreads) void mm_sums_kernel(MmMomentsParams P) {
#pragma clang fp contract(off)
  __shared__ double wl[kMmTile];
  __shared__ double red[3][kMmThreads];
  const int tid = threadIdx.x;
  const int D = P.D, Dp = mm_pow2(D), G = kMmThreads / Dp;
  const int dl = tid & (Dp - 1), g = tid / Dp;
  const int64_t nT = mm_tiles(P.S), n_work = P.B * nT;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int64_t b = w / nT, tile = w - b * nT;
    const int64_t s0 = tile * kMmTile;
    const int nr = (int)(P.S - s0 < kMmTile ? P.S - s0 : kMmTile);
    const double* xb = P.x + (b * P.S + s0) * D;
    if (PASS == 0) {
      wl[tid] = tid < nr ? exp(P.lw[b * P.S + s0 + tid]) : 0.0;
      __syncthreads();
    }
    for (int d0 = 0; d0 < D; d0 += Dp) {
      const int d = d0 + dl;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
      if (d < D) {
        if (PASS == 0) {
          for (int i = g; i < nr; i += G) {
            const double x = xb[(int64_t)i * D + d], wt = wl[i];
            a0 += x;
            a1 += wt * x;
            a2 += wt * (x * x);
          }
        } else {
          const double m = P.stats[b * 4 * D + d];
          for (int i = g; i < nr; i += G) {
            const double c = xb[(int64_t)i * D + d] - m;
            a0 += c * c;
          }
        }
      }
      red[0][tid] = a0;
      if (PASS == 0) {
        red[1][tid] = a1;
        red[2][tid] = a2;
      }
      __syncthreads();
      if (g == 0 && d < D) {
        for (int q = 0; q < (PASS == 0 ? 3 : 1); ++q) {
          double s = red[q][dl];
          for (int gg = 1; gg < G; ++gg) s += red[q][gg * Dp + dl];
          if (PASS == 0)
            P.part0[w * (3 * (int64_t)D + 2) + (int64_t)q * D + d] = s;
          else
            P.part1[w * D + d] = s;
        }
      }
      __syncthreads();
    }
    if (PASS == 0) {
      red[0][tid] = wl[tid];
      red[1][tid] = wl[tid] * wl[tid];
      __syncthreads();
      for (int off = kMmThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
          red[0][tid] += red[0][tid + off];
          red[1][tid] += red[1][tid + off];
        }
        __syncthreads();
      }
      if (tid == 0) {
        P.part0[w * (3 * (int64_t)D + 2) + 3 * (int64_t)D] = red[0][0];
        P.part0[w * (3 * (int64_t)D + 2) + 3 * (int64_t)D + 1] = red[1][0];
      }
      __syncthreads();
    }
  }
}

// the tiles of pass 0 in tile order: mean, wmean, mii -> stats; a, W, W2 -> mid.  One lane per (b, d).
__global__ __launch_bounds__(kMmThreads) void mm_mid_kernel(MmMomentsParams P) {
#pragma clang fp contract(off)
  const int D = P.D;
  const int64_t nT = mm_tiles(P.S), n = P.B * D, st = 3 * (int64_t)D + 2;
  for (int64_t e = (int64_t)blockIdx.x * kMmThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kMmThreads) {
    const int64_t b = e / D;
    const int d = (int)(e - b * D);
    const double* p = P.part0 + b * nT * st;
    double sx = 0.0, swx = 0.0, swxx = 0.0, W = 0.0, W2 = 0.0;
    for (int64_t t = 0; t < nT; ++t) {
      sx += p[t * st + d];
      swx += p[t * st + D + d];
      swxx += p[t * st + 2 * D + d];
      W += p[t * st + 3 * D];
      W2 += p[t * st + 3 * D + 1];
    }
    const double Sd = (double)P.S;
    double* s = P.stats + b * 4 * D;
    s[d] = sx / Sd;
    s[D + d] = swx;
    s[3 * D + d] = (swxx - swx * swx) * Sd / (Sd - 1.0);
    double* m = P.mid + b * (D + 2);
    m[d] = swx / W;
    if (d == 0) {
      m[D] = W;
      m[D + 1] = W2;
    }
  }
}

// the centred second moments of one (b, tile of kMmCovTile draws): both matrices, upper triangle, a fixed set of pairs per lane
__global__ __launch_bounds__(kMmThreads) void mm_cov_kernel(MmMomentsParams P) {
  __shared__ double xs[kMmCovBlock][kMmMaxCovDim + 1];
  __shared__ double ws[kMmCovBlock];
  __shared__ double mu[2][kMmMaxCovDim];
  const int tid = threadIdx.x;
  const int D = P.D, np = mm_pairs(D);
  int jk[kMmPairsPerThread];  // (j << 8) | k of pair tid + 256 i; pair 0 beyond the triangle (never written)
#pragma unroll
  for (int i = 0; i < kMmPairsPerThread; ++i) {
    int p = tid + i * kMmThreads, j = 0;
    if (p >= np) p = 0;
    while (p >= D - j) {
      p -= D - j;
      ++j;
    }
    jk[i] = (j << 8) | (j + p);
  }
  const int64_t nTc = mm_cov_tiles(P.S), n_work = P.B * nTc;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int64_t b = w / nTc, tile = w - b * nTc;
    const int64_t s0 = tile * kMmCovTile;
    const int nr = (int)(P.S - s0 < kMmCovTile ? P.S - s0 : kMmCovTile);
    double acc0[kMmPairsPerThread], acc1[kMmPairsPerThread];
#pragma unroll
    for (int i = 0; i < kMmPairsPerThread; ++i) acc0[i] = acc1[i] = 0.0;
    if (tid < D) {
      mu[0][tid] = P.stats[b * 4 * D + tid];
      mu[1][tid] = P.mid[b * (D + 2) + tid];
    }
    for (int r0 = 0; r0 < nr; r0 += kMmCovBlock) {
      const int nb = nr - r0 < kMmCovBlock ? nr - r0 : kMmCovBlock;
      __syncthreads();  // (the block before has been read; mu is written)
      const double* xb = P.x + (b * P.S + s0 + r0) * D;
      for (int idx = tid; idx < nb * D; idx += kMmThreads) {
        const int r = idx / D;
        xs[r][idx - r * D] = xb[idx];
      }
      if (tid < nb) ws[tid] = exp(P.lw[b * P.S + s0 + r0 + tid]);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kMmPairsPerThread; ++i) {
        const int j = jk[i] >> 8, k = jk[i] & 255;
        const double mj = mu[0][j], mk = mu[0][k], aj = mu[1][j], ak = mu[1][k];
        double c0 = acc0[i], c1 = acc1[i];
        for (int r = 0; r < nb; ++r) {
          const double xj = xs[r][j], xk = xs[r][k];
          c0 += (xj - mj) * (xk - mk);
          c1 += (xj - aj) * ((xk - ak) * ws[r]);
        }
        acc0[i] = c0;
        acc1[i] = c1;
      }
    }
    __syncthreads();  // (mu is rewritten for the next work item)
    double* out = P.partc + w * 2 * np;
#pragma unroll
    for (int i = 0; i < kMmPairsPerThread; ++i) {
      const int p = tid + i * kMmThreads;
      if (p < np) {
        out[p] = acc0[i];
        out[np + p] = acc1[i];
      }
    }
  }
}

// the tiles of pass 1 and of the matrix pass in tile order: var -> stats, cov / wcov -> cov.  One lane per (b, d) or (b, pair).
__global__ __launch_bounds__(kMmThreads) void mm_fin_kernel(MmMomentsParams P) {
#pragma clang fp contract(off)
  const int D = P.D, np = P.want_cov ? mm_pairs(D) : 0, per_b = D + np;
  const int64_t nT = mm_tiles(P.S), nTc = mm_cov_tiles(P.S), n = P.B * per_b;
  for (int64_t e = (int64_t)blockIdx.x * kMmThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kMmThreads) {
    const int64_t b = e / per_b;
    const int q = (int)(e - b * per_b);
    if (q < D) {
      const double* p = P.part1 + b * nT * D;
      double s = 0.0;
      for (int64_t t = 0; t < nT; ++t) s += p[t * D + q];
      P.stats[b * 4 * D + 2 * D + q] = s / (double)P.S;
    } else {
      int p = q - D, j = 0;
      const int pair = p;
      while (p >= D - j) {
        p -= D - j;
        ++j;
      }
      const int k = j + p;
      const double* pc = P.partc + b * nTc * 2 * np;
      double c0 = 0.0, c1 = 0.0;
      for (int64_t t = 0; t < nTc; ++t) {
        c0 += pc[t * 2 * np + pair];
        c1 += pc[t * 2 * np + np + pair];
      }
      const double W = P.mid[b * (D + 2) + D], W2 = P.mid[b * (D + 2) + D + 1];
      c0 *= 1.0 / ((double)P.S - 1.0);
      c1 *= 1.0 / (W - W2 / W);
      double* o = P.cov + b * 2 * D * D;
      o[j * D + k] = c0;
      o[k * D + j] = c0;
      o[D * D + j * D + k] = c1;
      o[D * D + k * D + j] = c1;
    }
  }
}

// ---- b. transform ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kMmThreads) void mm_affine_kernel(MmTransformParams P) {
#pragma clang fp contract(off)
  const int D = P.D;
  const int64_t n = P.B * P.S * D;
  for (int64_t e = (int64_t)blockIdx.x * kMmThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kMmThreads) {
    const int64_t bs = e / D, b = bs / P.S, s = bs - b * P.S;
    const int d = (int)(e - bs * D);
    double v = P.x[b * P.x_batch_stride + s * D + d];
    if (s >= P.row_lo && s < P.row_hi) {
      v = v - P.m0[b * D + d];
      if (P.pre) v = v * P.pre[b * D + d];
      if (P.post) v = v / P.post[b * D + d];
      v = v + P.m1[b * D + d];
    }
    P.out[e] = v;
  }
}

__global__ __launch_bounds__(kMmThreads) void mm_map_kernel(MmTransformParams P) {
  __shared__ double mt[kMmMaxCovDim][kMmMaxCovDim + 1];  // mt[e][d] = map[d][e]
  __shared__ double xc[kMmThreads];                      // [rows of one step][Dp]
  const int tid = threadIdx.x;
  const int D = P.D, Dp = mm_pow2(D), R = kMmThreads / Dp;
  const int d = tid & (Dp - 1), r = tid / Dp;
  const int64_t n_chunks = (P.S + kMmMapRows - 1) / kMmMapRows, n_work = P.B * n_chunks;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int64_t b = w / n_chunks, s0 = (w - b * n_chunks) * kMmMapRows;
    const int nr = (int)(P.S - s0 < kMmMapRows ? P.S - s0 : kMmMapRows);
    __syncthreads();  // (the work item before has finished with mt)
    for (int idx = tid; idx < D * D; idx += kMmThreads) {
      const int dd = idx / D;
      mt[idx - dd * D][dd] = P.map[b * D * D + idx];
    }
    double m0 = 0.0, pre = 1.0, post = 1.0, m1 = 0.0;
    if (d < D) {
      m0 = P.m0[b * D + d];
      m1 = P.m1[b * D + d];
      if (P.pre) pre = P.pre[b * D + d];
      if (P.post) post = P.post[b * D + d];
    }
    const double* xb = P.x + b * P.x_batch_stride + s0 * D;
    double* ob = P.out + (b * P.S + s0) * D;
    for (int r0 = 0; r0 < nr; r0 += R) {
      const int row = r0 + r;
      const bool live = row < nr && d < D;
      const double x = live ? xb[(int64_t)row * D + d] : 0.0;
      __syncthreads();  // (the step before has been read; mt is written)
      xc[tid] = (x - m0) * pre;
      __syncthreads();
      if (live) {
        double v = x;
        if (s0 + row >= P.row_lo && s0 + row < P.row_hi) {
          double acc = 0.0;
          for (int e = 0; e < D; ++e) acc += xc[r * Dp + e] * mt[e][d];
          v = (P.post ? acc / post : acc) + m1;
        }
        ob[(int64_t)row * D + d] = v;
      }
    }
  }
}

// ---- c. ratios ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double mm_neg_inf() { return -__builtin_huge_val(); }

template <int MODE>
__global__ __launch_bounds__(kMmThreads) void mm_ratios_kernel(MmRatiosParams P) {
#pragma clang fp contract(off)
  const int64_t n = P.B * P.S;
  for (int64_t e = (int64_t)blockIdx.x * kMmThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kMmThreads) {
    const int64_t b = e / P.S, s = e - b * P.S;
    if (MODE == 0) {  // a = ll_new (B, S), b = lp_new (B, S), c = lp_orig (S)
      const double lp = P.b[e], lo = P.c[s];
      double lr = -P.a[e] + lp - lo, full = lp - lo;
      if (lr != lr) lr = mm_neg_inf();
      if (full != full) full = mm_neg_inf();
      P.out[e] = lr;
      P.out[n + e] = full;
    } else if (MODE == 1) {  // a = ll_half, b = lp_half, c = lp_half_inv (B, S); jac = (sum log scaling, log |det mapping|)
      const double lp = P.b[e];
      const double li = (P.c[e] - P.jac[2 * b]) - P.jac[2 * b + 1];
      double l = -P.a[e] + lp;
      if (lp > li)
        l = l - (lp + log1p(exp(li - lp)));
      else
        l = l - (li + log1p(exp(lp - li)));
      if (l != l || l == __builtin_huge_val()) l = mm_neg_inf();
      P.out[e] = l;
    } else {  // a = lw, b = ll
      double l = P.a[e] + P.b[e];
      if (l != l || l == __builtin_huge_val()) l = mm_neg_inf();
      P.out[e] = l;
    }
  }
}

// NaN wins, as in np.max
__device__ __forceinline__ double mm_max(double m, double v) { return (v > m || v != v) ? v : m; }

// mode 3: a = ll (B, S), b = lw (B, S); out[2b] = logsumexp(ll + lw), out[2b + 1] = logsumexp(ll) - log S.  One wave per row.
__global__ __launch_bounds__(kMmThreads) void mm_finish_kernel(MmRatiosParams P) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * kMmThreads + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * kMmThreads) >> 6;
  for (int64_t b = wave; b < P.B; b += n_waves) {
    const double* ll = P.a + b * P.S;
    const double* lw = P.b + b * P.S;
    double m0 = mm_neg_inf(), m1 = mm_neg_inf();
    for (int64_t s = lane; s < P.S; s += 64) {
      m0 = mm_max(m0, ll[s] + lw[s]);
      m1 = mm_max(m1, ll[s]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      m0 = mm_max(m0, __shfl_xor(m0, off, 64));
      m1 = mm_max(m1, __shfl_xor(m1, off, 64));
    }
    double s0 = 0.0, s1 = 0.0;
    for (int64_t s = lane; s < P.S; s += 64) {
      s0 += exp((ll[s] + lw[s]) - m0);
      s1 += exp(ll[s] - m1);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s0 += __shfl_xor(s0, off, 64);
      s1 += __shfl_xor(s1, off, 64);
    }
    if (lane == 0) {
      P.out[2 * b] = log(s0) + m0;
      P.out[2 * b + 1] = (log(s1) + m1) - log((double)P.S);
    }
  }
}

}  // namespace pla
