// Kernels of the model comparison (reference: pyloo compare.py:205-229, 477-577).
//
// Input of all three passes: a (K, N) matrix of pointwise values (loo_i / waic_i of K models over N observations), row k at
// x + k * pitch, f64 or f32 (promoted on load), multiplied on load by `scale_mul`: 1, -1 or -1/2 bring a "log", "negative_log" or
// "deviance" table to the log scale (compare.py:489-492, 556-559); the moments pass takes 1 (dse is on the table's own scale).
// K <= kCompareMaxModels.
//
// Determinism.  The N observations are cut into tiles whose width depends on N alone (compare_tile_cols: at least
// kCompareMinTile columns, at most kCompareMaxTiles tiles).  A workgroup reduces one tile (a grid-stride loop over the tiles, so
// the grid size does not matter), in a fixed order: every lane walks its columns in ascending order, the lanes of a wave are
// combined by an xor butterfly, the waves in wave order through LDS.  Each tile's partial goes to its own slot of engine
// workspace, and a one-pass final kernel combines the slots in tile order.  Two calls with the same input give the same bits,
// whatever the grid or the device.
//
// a. compare_moments_kernel: per model k, sum_i x'_ik, and the mean and M2 (Chan, Golub & LeVeque) of d_ik = x'_ik - x'_{best,i}
//    (dse = sqrt(N * var(d)) = sqrt(M2): compare.py:226-227); plus sum_i max_k x'_ik (the log score of picking the best model at
//    every point: an upper bound of the stacking score).
// b. stacking_eval_kernel: for weights w (host, in the kernel arguments), with m_i = max_k x'_ik and e_ik = exp(x'_ik - m_i):
//        d_i = sum_k w_k e_ik,   F = sum_i log d_i,   G_k = sum_i e_ik / d_i
//    The objective of compare.py:497-503 is -(F + sum_i m_i) up to the constant, its gradient (505-514) -(G_k - G_{K-1}).
//    e_ik is recomputed from x on every call (no (K, N) buffer): one read of the matrix per evaluation.
// c. bb_bootstrap_kernel: z_bk = N * scale_mul * (sum_i G_bi x_ik) / (sum_i G_bi), G_bi ~ Gamma(alpha, 1) generated in the kernel
//    (a Dirichlet draw is a vector of normalised gammas: compare.py:561-571, `b_weighting @ (N * x)`, without the B x N matrix).
//    Work layout: a workgroup of four waves takes 64 replicates (one per lane: gridDim.y) and one tile (gridDim.x); wave w walks the tile's columns
//    w, w + 4, ... and every lane adds G_bi and G_bi * x_ik for its replicate; the column values are the same for all lanes (one
//    broadcast load).  The waves' sums are added in wave order through LDS and written as the (replicate, tile) partial.  The
//    matrix is read once per block of 64 replicates (ceil(B / 64) times in all, from L2 for the most part), and once more per
//    extra group of kCompareChunk models when K > kCompareChunk (the gammas are then generated again for every group).
//
// The gamma stream (bb_gamma): a pure function of (seed, alpha, b, i), independent of the launch geometry.
//   block(i, b, t, j) = Philox4x32-10 (Random123: multipliers 0xD2511F53, 0xCD9E8D57, Weyl key increments 0x9E3779B9,
//                       0xBB67AE85) of counter (c0, c1, c2, c3) = (i, b, t, j) with key (k0, k1) = (seed mod 2^32, seed >> 32)
//                       -> four 32-bit words (r0, r1, r2, r3)
//   U53(hi, lo)       = (((hi << 32 | lo) >> 11) + 1) * 2^-53, in (0, 1]
//   alpha == 1        G = -log(U53(r0, r1)) of block(i, b, 0, 0)
//   a >= 1            Marsaglia & Tsang (2000), with a = alpha (alpha > 1) or a = alpha + 1 (alpha < 1):
//                       d = a - 1/3, c = 1 / sqrt(9 d); for attempt t = 0, 1, ..., kGammaAttempts - 1:
//                         (r0..r3) = block(i, b, t, 0); x = sqrt(-2 log U53(r0, r1)) * cos(2 pi * U53(r2, r3))   (Box-Muller)
//                         v = 1 + c x; if v <= 0 the attempt is rejected
//                         v3 = v * v * v; (s0..s3) = block(i, b, t, 1)
//                         accept when log(U53(s0, s1)) < 0.5 x x + d - d v3 + d log(v3): G = d v3
//                       (no attempt accepted -- probability below 0.05^64 -- gives G = d)
//   alpha < 1         G = G_{alpha+1} * U53(s2, s3)^(1 / alpha) with (s0..s3) = block(i, b, 0, 1)
//   Every operation is written as it stands (no contraction into fma), so tests/test_compare_host.py restates it in NumPy.
// pla_bb_gamma_draws writes G for a (B, N) grid through the same device function.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pla {

constexpr int kCompareMaxModels = 64;
constexpr int kCompareChunk = 16;          // models per group of accumulators of the stacking and bootstrap passes (gridDim.y / .z)
constexpr int kMomentsChunk = 8;           // ... of the moments pass (three accumulators per model)
constexpr int64_t kCompareMinTile = 1024;  // columns
constexpr int64_t kCompareMaxTiles = 2048;
constexpr int kCompareThreads = 256;
constexpr int kGammaAttempts = 64;

// tile width for N observations: max(kCompareMinTile, ceil(N / kCompareMaxTiles) rounded up to 256)
__host__ __device__ inline int64_t compare_tile_cols(int64_t n) {
  int64_t t = (n + kCompareMaxTiles - 1) / kCompareMaxTiles;
  t = (t + 255) / 256 * 256;
  return t < kCompareMinTile ? kCompareMinTile : t;
}

struct CompareInput {
  const void* x;     // (K, N), row k at x + k * pitch (elements)
  int64_t pitch;
  int K;
  int64_t N;
  double scale_mul;
  int64_t tile_cols, n_tiles;
};

template <typename T>
__device__ __forceinline__ double cmp_load(const CompareInput& in, int k, int64_t i) {
  return in.scale_mul * (double)reinterpret_cast<const T*>(in.x)[(int64_t)k * in.pitch + i];
}

// ---- Philox4x32-10 and the gamma sampler --------------------------------------------------------------------------------------
struct Philox4 {
  uint32_t r[4];
};

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  return (double)((v >> 11) + 1) * 0x1.0p-53;
}

__device__ inline double bb_gamma(uint64_t seed, double alpha, uint32_t b, uint32_t i) {
#pragma clang fp contract(off)
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  if (alpha == 1.0) {
    const Philox4 r = philox4x32_10(i, b, 0, 0, k0, k1);
    return -log(u53(r.r[0], r.r[1]));
  }
  const double a = alpha < 1.0 ? alpha + 1.0 : alpha;
  const double d = a - 1.0 / 3.0;
  const double c = 1.0 / sqrt(9.0 * d);
  double g = d;
  for (uint32_t t = 0; t < (uint32_t)kGammaAttempts; ++t) {
    const Philox4 r = philox4x32_10(i, b, t, 0, k0, k1);
    const double x = sqrt(-2.0 * log(u53(r.r[0], r.r[1]))) * cos(6.283185307179586 * u53(r.r[2], r.r[3]));
    const double v = 1.0 + c * x;
    if (v <= 0.0) continue;
    const double v3 = v * v * v;
    const Philox4 s = philox4x32_10(i, b, t, 1, k0, k1);
    if (log(u53(s.r[0], s.r[1])) < 0.5 * x * x + d - d * v3 + d * log(v3)) {
      g = d * v3;
      break;
    }
  }
  if (alpha < 1.0) {
    const Philox4 s = philox4x32_10(i, b, 0, 1, k0, k1);
    g = g * pow(u53(s.r[2], s.r[3]), 1.0 / alpha);
  }
  return g;
}

// ---- wave / workgroup helpers (fixed order) ----------------------------------------------------------------------------------
__device__ __forceinline__ double cmp_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double cmp_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// Chan, Golub & LeVeque: (na, ma, Ma) += (nb, mb, Mb)
__device__ __forceinline__ void chan_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
  const double n = na + nb;
  if (nb == 0.0) return;
  if (na == 0.0) {
    na = nb;
    ma = mb;
    Ma = Mb;
    return;
  }
  const double delta = mb - ma;
  ma = ma + delta * (nb / n);
  Ma = Ma + Mb + delta * delta * (na * nb / n);
  na = n;
}

// ---- a. moments --------------------------------------------------------------------------------------------------------------
// partials per tile: [0] count, then per model k of the group [1 + 3k] sum, [2 + 3k] mean of d, [3 + 3k] M2 of d, [1 + 3K] sum of max
struct MomentsParams {
  CompareInput in;
  int best;
  double* part;  // [n_tiles][3K + 2]
};

template <typename T>
__global__ __launch_bounds__(kCompareThreads) void compare_moments_kernel(MomentsParams P) {
  __shared__ double lds[kCompareThreads / 64][3 * kMomentsChunk + 2];
  const CompareInput& in = P.in;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = blockIdx.y * kMomentsChunk;
  const int kn = in.K - k0 < kMomentsChunk ? in.K - k0 : kMomentsChunk;
  const int stride = 3 * in.K + 2;
  for (int64_t tile = blockIdx.x; tile < in.n_tiles; tile += gridDim.x) {
    const int64_t c0 = tile * in.tile_cols;
    const int64_t c1 = c0 + in.tile_cols < in.N ? c0 + in.tile_cols : in.N;
    double n = 0.0, smax = 0.0;
    double sum[kMomentsChunk], mean[kMomentsChunk], m2[kMomentsChunk];
#pragma unroll
    for (int k = 0; k < kMomentsChunk; ++k) sum[k] = mean[k] = m2[k] = 0.0;
    for (int64_t i = c0 + threadIdx.x; i < c1; i += kCompareThreads) {
      const double xb = cmp_load<T>(in, P.best, i);
      n += 1.0;
      if (blockIdx.y == 0) {
        double mx = xb;
        for (int k = 0; k < in.K; ++k) mx = fmax(mx, cmp_load<T>(in, k, i));
        smax += mx;
      }
#pragma unroll
      for (int k = 0; k < kMomentsChunk; ++k) {
        if (k < kn) {
          const double v = cmp_load<T>(in, k0 + k, i);
          sum[k] += v;
          const double dv = v - xb;
          const double delta = dv - mean[k];
          mean[k] += delta / n;
          m2[k] += delta * (dv - mean[k]);
        }
      }
    }
    // lanes of a wave (butterfly), then waves in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double nb = __shfl_xor(n, off, 64);
#pragma unroll
      for (int k = 0; k < kMomentsChunk; ++k) {
        const double mb = __shfl_xor(mean[k], off, 64), Mb = __shfl_xor(m2[k], off, 64);
        double na = n;
        chan_merge(na, mean[k], m2[k], nb, mb, Mb);
        sum[k] += __shfl_xor(sum[k], off, 64);
      }
      n += nb;
      smax += __shfl_xor(smax, off, 64);
    }
    if (lane == 0) {
      lds[wave][0] = n;
#pragma unroll
      for (int k = 0; k < kMomentsChunk; ++k) {
        lds[wave][1 + 3 * k] = sum[k];
        lds[wave][2 + 3 * k] = mean[k];
        lds[wave][3 + 3 * k] = m2[k];
      }
      lds[wave][1 + 3 * kMomentsChunk] = smax;
    }
    __syncthreads();
    if (threadIdx.x < kn || (threadIdx.x == kMomentsChunk && blockIdx.y == 0)) {
      double* out = P.part + tile * stride;
      if (threadIdx.x == kMomentsChunk) {
        double s = lds[0][1 + 3 * kMomentsChunk], cnt = lds[0][0];
        for (int w = 1; w < kCompareThreads / 64; ++w) {
          s += lds[w][1 + 3 * kMomentsChunk];
          cnt += lds[w][0];
        }
        out[0] = cnt;
        out[1 + 3 * in.K] = s;
      } else {
        const int k = threadIdx.x;
        double na = lds[0][0], ma = lds[0][2 + 3 * k], Ma = lds[0][3 + 3 * k], s = lds[0][1 + 3 * k];
        for (int w = 1; w < kCompareThreads / 64; ++w) {
          chan_merge(na, ma, Ma, lds[w][0], lds[w][2 + 3 * k], lds[w][3 + 3 * k]);
          s += lds[w][1 + 3 * k];
        }
        out[1 + 3 * (k0 + k)] = s;
        out[2 + 3 * (k0 + k)] = ma;
        out[3 + 3 * (k0 + k)] = Ma;
      }
    }
    __syncthreads();
  }
}

// out[3k] = sum_k, out[3k + 1] = mean of d_k, out[3k + 2] = M2 of d_k, out[3K] = sum of the row maxima: tiles in order
__global__ __launch_bounds__(128) void compare_moments_final_kernel(const double* part, int K, int64_t n_tiles, double* out) {
  const int k = threadIdx.x;
  if (k > K) return;
  const int stride = 3 * K + 2;
  if (k == K) {
    double s = 0.0;
    for (int64_t t = 0; t < n_tiles; ++t) s += part[t * stride + 1 + 3 * K];
    out[3 * K] = s;
    return;
  }
  double n = 0.0, m = 0.0, M = 0.0, s = 0.0;
  for (int64_t t = 0; t < n_tiles; ++t) {
    const double* p = part + t * stride;
    chan_merge(n, m, M, p[0], p[2 + 3 * k], p[3 + 3 * k]);
    s += p[1 + 3 * k];
  }
  out[3 * k] = s;
  out[3 * k + 1] = m;
  out[3 * k + 2] = M;
}

// ---- b. stacking objective and gradient --------------------------------------------------------------------------------------
struct StackingParams {
  CompareInput in;
  const double* w;  // [K] device
  double* part;  // [n_tiles][K + 1]: F, then G_k
};

template <typename T>
__global__ __launch_bounds__(kCompareThreads) void stacking_eval_kernel(StackingParams P) {
  __shared__ double lds[kCompareThreads / 64][kCompareChunk + 1];
  const CompareInput& in = P.in;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = blockIdx.y * kCompareChunk;
  const int kn = in.K - k0 < kCompareChunk ? in.K - k0 : kCompareChunk;
  for (int64_t tile = blockIdx.x; tile < in.n_tiles; tile += gridDim.x) {
    const int64_t c0 = tile * in.tile_cols;
    const int64_t c1 = c0 + in.tile_cols < in.N ? c0 + in.tile_cols : in.N;
    double F = 0.0, G[kCompareChunk];
#pragma unroll
    for (int k = 0; k < kCompareChunk; ++k) G[k] = 0.0;
    // (a loop with the same trip count for every lane, the last columns masked by selects: no exec-masked region around the
    // body, where the compiler would have to keep spilled scalars)
    for (int64_t base = c0; base < c1; base += kCompareThreads) {
      const int64_t i0 = base + threadIdx.x;
      const bool live = i0 < c1;
      const int64_t i = live ? i0 : c0;
      double m = cmp_load<T>(in, 0, i);
      for (int k = 1; k < in.K; ++k) m = fmax(m, cmp_load<T>(in, k, i));
      double d = 0.0;
      for (int k = 0; k < in.K; ++k) d += P.w[k] * exp(cmp_load<T>(in, k, i) - m);
      F += live ? log(d) : 0.0;
      const double r = live ? 1.0 / d : 0.0;
#pragma unroll
      for (int k = 0; k < kCompareChunk; ++k)
        if (k < kn) G[k] += exp(cmp_load<T>(in, k0 + k, i) - m) * r;
    }
    F = cmp_wave_sum(F);
#pragma unroll
    for (int k = 0; k < kCompareChunk; ++k) G[k] = cmp_wave_sum(G[k]);
    if (lane == 0) {
      lds[wave][0] = F;
#pragma unroll
      for (int k = 0; k < kCompareChunk; ++k) lds[wave][1 + k] = G[k];
    }
    __syncthreads();
    if (threadIdx.x <= kCompareChunk) {
      const int j = threadIdx.x;  // 0: F, 1 + k: G_k
      if ((j == 0 && blockIdx.y == 0) || (j >= 1 && j - 1 < kn)) {
        double s = lds[0][j];
        for (int w = 1; w < kCompareThreads / 64; ++w) s += lds[w][j];
        P.part[tile * (in.K + 1) + (j == 0 ? 0 : 1 + k0 + j - 1)] = s;
      }
    }
    __syncthreads();
  }
}

// out[j] = sum over the tiles, in order, of part[t][j], j <= K
__global__ __launch_bounds__(128) void compare_tiles_sum_kernel(const double* part, int width, int64_t n_tiles, double* out) {
  const int j = threadIdx.x;
  if (j >= width) return;
  double s = 0.0;
  for (int64_t t = 0; t < n_tiles; ++t) s += part[t * width + j];
  out[j] = s;
}

// ---- c. Bayesian bootstrap ---------------------------------------------------------------------------------------------------
struct BBParams {
  CompareInput in;
  uint64_t seed;
  double alpha;
  int64_t b0, nb;  // replicates [b0, b0 + nb) of this launch
  double* part;    // [nb][n_tiles][K + 1]: sum of G, then sum of G * x_k
};

template <typename T>
__global__ __launch_bounds__(kCompareThreads) void bb_bootstrap_kernel(BBParams P) {
  __shared__ double lds[kCompareThreads / 64][kCompareChunk + 1][64];
  const CompareInput& in = P.in;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int k0 = blockIdx.z * kCompareChunk;
  const int kn = in.K - k0 < kCompareChunk ? in.K - k0 : kCompareChunk;
  const int64_t nbb = (P.nb + 63) / 64;
  for (int64_t bb = blockIdx.y; bb < nbb; bb += gridDim.y)
  for (int64_t tile = blockIdx.x; tile < in.n_tiles; tile += gridDim.x) {
    const int64_t bl = bb * 64 + lane;  // replicate of this lane, relative to b0
    const bool live = bl < P.nb;
    const uint32_t b = (uint32_t)(P.b0 + (live ? bl : 0));
    const int64_t c0 = tile * in.tile_cols;
    const int64_t c1 = c0 + in.tile_cols < in.N ? c0 + in.tile_cols : in.N;
    double S = 0.0, Tk[kCompareChunk];
#pragma unroll
    for (int k = 0; k < kCompareChunk; ++k) Tk[k] = 0.0;
    for (int64_t i = c0 + wave; i < c1; i += kCompareThreads / 64) {
      const double g = bb_gamma(P.seed, P.alpha, b, (uint32_t)i);
      S += g;
#pragma unroll
      for (int k = 0; k < kCompareChunk; ++k)
        if (k < kn) Tk[k] += g * (double)reinterpret_cast<const T*>(in.x)[(int64_t)(k0 + k) * in.pitch + i];
    }
    lds[wave][0][lane] = S;
#pragma unroll
    for (int k = 0; k < kCompareChunk; ++k) lds[wave][1 + k][lane] = Tk[k];
    __syncthreads();
    if (wave == 0 && live) {
      double* out = P.part + (bl * in.n_tiles + tile) * (in.K + 1);
      if (blockIdx.z == 0) out[0] = ((lds[0][0][lane] + lds[1][0][lane]) + lds[2][0][lane]) + lds[3][0][lane];
      for (int k = 0; k < kn; ++k)
        out[1 + k0 + k] = ((lds[0][1 + k][lane] + lds[1][1 + k][lane]) + lds[2][1 + k][lane]) + lds[3][1 + k][lane];
    }
    __syncthreads();
  }
}

// z[r][k] = N * scale_mul * (sum_t T) / (sum_t S) for the replicates r < nb of one launch, tiles in order; one thread per
// (replicate, model)
__global__ __launch_bounds__(256) void bb_final_kernel(const double* part, int K, int64_t n_tiles, int64_t nb, double n_scale, double* z) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= nb * K) return;
  const int64_t r = id / K;
  const int k = (int)(id % K);
  const double* p = part + r * n_tiles * (K + 1);
  double S = 0.0, T = 0.0;
  for (int64_t t = 0; t < n_tiles; ++t) {
    S += p[t * (K + 1)];
    T += p[t * (K + 1) + 1 + k];
  }
  z[r * K + k] = n_scale * (T / S);
}

// G[b][i] for b < B, i < N (the stream of bb_bootstrap_kernel on its own)
__global__ __launch_bounds__(256) void bb_gamma_draws_kernel(uint64_t seed, double alpha, int64_t B, int64_t N, double* out) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * N) return;
  out[id] = bb_gamma(seed, alpha, (uint32_t)(id / N), (uint32_t)(id % N));
}

}  // namespace pla
