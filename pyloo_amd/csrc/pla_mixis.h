// Mix-IS-LOO kernels (Silva & Zanella 2022; the estimator the reference documents at loo.py:252-284 and elpd.py:364-374).
//
// Two passes over the (n_obs, n_draws) log-likelihood matrix, one log-sum-exp along each axis:
//     c[s]    = log sum_i exp(-ll[i, s])                    PASS 1: one value per DRAW, over the observations
//     a[i]    = log sum_s exp(-ll[i, s] - c[s])             PASS 2: one value per observation, over the draws
//     elpd[i] = log sum_s exp(-c[s]) - a[i]
// (The reference's own code takes the first log-sum-exp over the draws, which makes every elpd[i] the same constant: DESIGN.md.)
// All arithmetic is f64, f32 input is widened on load.  NaN counts as -1e10, +inf as +1e10 and -inf as -1e10 (loo.py:218-227 and
// pla_waic's rule), in both passes alike, and the two kinds are counted separately; everything behind the load is plain IEEE.
// The kernels form y = -x - c from the raw entry and repair y where it is not finite (mixis_fix): y is NaN exactly where x is,
// -inf where x is +inf and +inf where x is -inf, because c is finite.
//
// PASS 1.  The observations are cut into tiles of mixis_tile_rows(n_obs) rows -- a rule of n_obs alone -- and every (tile, draw)
// has a slot of its own for its (maximum, rescaled sum) in a slab of engine workspace; mixis_c_merge_kernel combines the slots of
// a draw in tile order.  No floating-point atomics: c does not change bits with the grid or from run to run.
//   mixis_c_tile_kernel   draws fastest (or any other strides: UNIT = false): adjacent lanes own adjacent draws and walk down
//                         the rows of a tile with a running maximum and a rescaled sum each.
//   mixis_c_line_kernel   observations fastest: a draw is one contiguous line of n_obs elements; a wavefront per (draw, tile)
//                         reads its piece of the line with 16-byte loads (VEC = 1: element loads, for lines that are not 16-byte
//                         aligned), every lane with a running maximum and a rescaled sum, merged across the wave in a fixed order.
//   slab size: 2 * n_tiles * n_draws doubles with n_tiles <= kMixisMaxTiles, that is at most 2048 * n_draws bytes.
// PASS 2.  mixis_lse_c_kernel computes log sum_s exp(-c[s]) once (one workgroup, fixed order).
//   mixis_row_wave_kernel    draws fastest, n_draws <= kMixisRegDraws: one wavefront per observation, the row's y in its registers,
//                            c staged in LDS once per workgroup; the exact maximum first, then the sum.
//   mixis_row_stream_kernel  draws fastest, longer rows: one wavefront per observation, c read chunk by chunk through L2, every
//                            lane with a running maximum and a rescaled sum.
//   mixis_col_kernel         observations fastest: one lane per observation streams down its column; c[s] is wave-uniform and
//                            sits in a scalar register pair (scalar loads through the constant address space).
//   mixis_row_block_kernel   any other strides: one workgroup per observation, two strided passes over the row.
// An observation's result depends on its row and on c alone.  The pointwise values are handed to the tile-ordered reduction of
// the k-fold finishing pass (pla_kfold.h) for the scale and the aggregates.
#pragma once

#include "../../include/pyloo_amd.h"
#include "pla_kernels.h"
#include "pla_wave.h"

namespace pla {

constexpr int64_t kMixisMinTile = 256, kMixisMaxTiles = 128;
constexpr int kMixisRegDraws = kWave * kWaveSlots;  // rows up to this length sit in a wavefront's registers (4096)

// rows per partial of pass 1: max(kMixisMinTile, ceil(n_obs / kMixisMaxTiles) rounded up to 256) -- at most kMixisMaxTiles tiles
__host__ __device__ inline int64_t mixis_tile_rows(int64_t n) {
  int64_t t = (n + kMixisMaxTiles - 1) / kMixisMaxTiles;
  t = (t + 255) / 256 * 256;
  return t < kMixisMinTile ? kMixisMinTile : t;
}

struct MixisParams {
  const void* in;
  int64_t n_obs;
  int n_draws;
  int64_t stride_obs, stride_draw;  // elements
  int64_t tile_rows, n_tiles;  // pass 1: rows per tile (a rule of the WHOLE matrix) and the tiles of the rows at `in`
  int64_t tile0, tiles_total;  // ... which are tiles [tile0, tile0 + n_tiles) of tiles_total (a host matrix comes in blocks of whole tiles)
  double* part;      // pass 1: [2][tiles_total][n_draws] -- the maxima, then the sums
  double* c_out;     // pass 1: [n_draws]
  const double* c;   // pass 2: [n_draws]
  double* lse_c;     // [1] log sum_s exp(-c[s]): written by mixis_lse_c_kernel, read by pass 2
  double* elpd;      // pass 2: [n_obs], unscaled
  unsigned long long* replaced;  // [2] device counters: NaN, +-inf (may be null)
};

// y = -x - c of a raw entry x that is NaN or infinite, as the clamped entry gives it
__device__ __forceinline__ double mixis_fix(double y, double c, bool count, unsigned& n_nan, unsigned& n_inf) {
  const bool nan = y != y;
  const bool inf = !nan && (y - y != 0.0);
  n_nan += (count && nan) ? 1u : 0u;
  n_inf += (count && inf) ? 1u : 0u;
  const double r = (nan || y > 0.0) ? 1e10 : -1e10;
  return (nan || inf) ? r - c : y;
}

__device__ __forceinline__ void mixis_count(const MixisParams& P, unsigned n_nan, unsigned n_inf) {
  if (!P.replaced) return;
  if (__ballot((n_nan | n_inf) != 0u) == 0ull) return;
  const unsigned a = (unsigned)wave_reduce<OpSum>((double)n_nan), b = (unsigned)wave_reduce<OpSum>((double)n_inf);
  if (wave_lane() == 0) {
    if (a) atomicAdd(P.replaced, (unsigned long long)a);
    if (b) atomicAdd(P.replaced + 1, (unsigned long long)b);
  }
}

// one batch of U values of y into a lane's running (maximum m, sum se of exp(y - m)); the first nb count
template <int U>
__device__ __forceinline__ void mixis_take(const double (&y)[U], int nb, double& m, double& se, const double* tab) {
  double bm = -pinf();
#pragma unroll
  for (int u = 0; u < U; ++u) bm = (u < nb && y[u] > bm) ? y[u] : bm;
  if (bm > m) {  // this lane has a new maximum: rescale what it has summed so far (se is 0 while m is -inf)
    se *= exp_tab(fmax(m - bm, -700.0), tab);
    m = bm;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const double e = exp_tab(fmax(y[u] - m, -700.0), tab);  // (a NaN from -inf - -inf: fmax drops it, the select below the value)
    se += u < nb ? e : 0.0;
  }
}

// A lane streams down n elements p[0], p[step], ...: y[j] = -p[j * step] - (SUBC ? cs[j] : 0), cs indexed wave-uniformly.
// live: the lane's elements are real ones (dead lanes read a live lane's and count nothing).
template <typename T, bool SUBC>
__device__ __forceinline__ void mixis_lane_stream(const T* p, int64_t step, int64_t n, const double* cs, const double* tab, bool live,
                                                  double& m, double& se, unsigned& n_nan, unsigned& n_inf) {
  constexpr int U = 8;
  // c through the constant address space (nothing writes it while a kernel of pass 2 runs): with a wave-uniform index these are
  // scalar loads, c[j] in a scalar register pair -- left generic, the stores of the results keep them vector loads, one per lane
  const auto csc = (const __attribute__((address_space(4))) double*)cs;
  m = -pinf();
  se = 0.0;
#pragma unroll 1
  for (int64_t j0 = 0; j0 < n; j0 += U) {
    const int nb = n - j0 < U ? (int)(n - j0) : U;  // (wave-uniform)
    double y[U], cc[U];
    double z = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + u < n ? j0 + u : n - 1;
      cc[u] = SUBC ? csc[j] : 0.0;
      y[u] = -(double)__builtin_nontemporal_load(p + j * step) - cc[u];
      z = fma(y[u], 0.0, z);
    }
    if (__ballot(z != z) != 0ull) {  // rare: some entry of the wave's batch is NaN or infinite
#pragma unroll
      for (int u = 0; u < U; ++u) y[u] = mixis_fix(y[u], cc[u], live && u < nb, n_nan, n_inf);
    }
    mixis_take<U>(y, nb, m, se, tab);
  }
}

template <typename T, int VEC>
__device__ __forceinline__ void mixis_load_vec(const T* p, T (&x)[VEC]) {
  if constexpr (VEC == 1) {
    x[0] = __builtin_nontemporal_load(p);
  } else if constexpr (VEC == 2) {
    const double2 t = *reinterpret_cast<const double2*>(p);
    x[0] = (T)t.x;
    x[1] = (T)t.y;
  } else {
    const float4 t = *reinterpret_cast<const float4*>(p);
    x[0] = (T)t.x;
    x[1] = (T)t.y;
    x[2] = (T)t.z;
    x[3] = (T)t.w;
  }
}

// A wavefront reduces the n >= 1 elements of one contiguous line: y[d] = -p[d] - (SUBC ? cs[d] : 0).  Lane l takes the vectors
// l, l + 64, ... of VEC elements (p is 16-byte aligned when VEC > 1), 8 elements a batch, with a running maximum and a rescaled
// sum; the n % VEC elements behind the last whole vector go to lanes 0 ...; the lanes are merged by xor butterflies.  M and tot
// come back wave-uniform: the line's maximum and its sum of exp(y - M).
template <typename T, int VEC, bool SUBC>
__device__ __forceinline__ void mixis_wave_line(const T* p, int64_t n, const double* cs, const double* tab, double& M, double& tot,
                                                unsigned& n_nan, unsigned& n_inf) {
  constexpr int UV = 8 / VEC;
  const int lane = wave_lane();
  const int64_t nvec = n / VEC;
  double m = -pinf(), se = 0.0;
#pragma unroll 1
  for (int64_t v0 = 0; v0 < nvec; v0 += UV * kWave) {
    double y[8], cc[8];
    int nb = 0;  // this lane's elements of the batch: whole vectors, the valid ones first
    double z = 0.0;
#pragma unroll
    for (int j = 0; j < UV; ++j) {
      const int64_t vi = v0 + j * kWave + lane;
      const bool ok = vi < nvec;
      const int64_t d = (ok ? vi : nvec - 1) * VEC;
      nb += ok ? VEC : 0;
      T x[VEC];
      mixis_load_vec<T, VEC>(p + d, x);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        cc[j * VEC + e] = SUBC ? cs[d + e] : 0.0;
        y[j * VEC + e] = -(double)x[e] - cc[j * VEC + e];
        z = fma(y[j * VEC + e], 0.0, z);
      }
    }
    if (__ballot(z != z) != 0ull) {
#pragma unroll
      for (int u = 0; u < 8; ++u) y[u] = mixis_fix(y[u], cc[u], u < nb, n_nan, n_inf);
    }
    mixis_take<8>(y, nb, m, se, tab);
  }
  const int rem = (int)(n - nvec * VEC);
  if (rem > 0) {  // (wave-uniform)
    const bool ok = lane < rem;
    const int64_t d = nvec * VEC + (ok ? lane : 0);
    double y[1], cc = SUBC ? cs[d] : 0.0;
    y[0] = -(double)p[d] - cc;
    y[0] = mixis_fix(y[0], cc, ok, n_nan, n_inf);
    mixis_take<1>(y, ok ? 1 : 0, m, se, tab);
  }
  M = wave_reduce<OpMax>(m);
  se = m == -pinf() ? 0.0 : se * exp_tab(fmax(m - M, -700.0), tab);
  tot = wave_reduce<OpSum>(se);
}

// ---- pass 1 -------------------------------------------------------------------------------------------------------------------
template <typename T, bool UNIT>
__global__ __launch_bounds__(256) void mixis_c_tile_kernel(MixisParams P) {
  __shared__ __attribute__((aligned(16))) double tab[2 * kTabN];
  for (int j = threadIdx.x; j < kTabN; j += 256) exp_table_entry(tab, j);
  __syncthreads();
  const int S = P.n_draws;
  const int64_t sd = UNIT ? 1 : P.stride_draw;
  const int64_t n_db = (S + 255) / 256, n_units = n_db * P.n_tiles;
  unsigned n_nan = 0, n_inf = 0;
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {  // neighbouring workgroups: neighbouring draws of the same rows
    const int64_t tile = u / n_db, s = (u - tile * n_db) * 256 + threadIdx.x;
    const bool live = s < S;
    const int64_t r0 = tile * P.tile_rows;
    const int64_t r1 = r0 + P.tile_rows < P.n_obs ? r0 + P.tile_rows : P.n_obs;
    const T* p = reinterpret_cast<const T*>(P.in) + r0 * P.stride_obs + (live ? s : S - 1) * sd;
    double m, se;
    mixis_lane_stream<T, false>(p, P.stride_obs, r1 - r0, nullptr, tab, live, m, se, n_nan, n_inf);
    if (live) {
      P.part[(P.tile0 + tile) * S + s] = m;
      P.part[(P.tiles_total + P.tile0 + tile) * S + s] = se;
    }
  }
  mixis_count(P, n_nan, n_inf);
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void mixis_c_line_kernel(MixisParams P) {
  __shared__ __attribute__((aligned(16))) double tab[2 * kTabN];
  for (int j = threadIdx.x; j < kTabN; j += 256) exp_table_entry(tab, j);
  __syncthreads();
  const int S = P.n_draws;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int64_t n_units = (int64_t)S * P.n_tiles, nw = (int64_t)gridDim.x * 4;
  unsigned n_nan = 0, n_inf = 0;
  for (int64_t u = (int64_t)blockIdx.x * 4 + wv; u < n_units; u += nw) {  // neighbouring waves: neighbouring pieces of one line
    const int64_t s = u / P.n_tiles, tile = u - s * P.n_tiles;
    const int64_t r0 = tile * P.tile_rows;
    const int64_t r1 = r0 + P.tile_rows < P.n_obs ? r0 + P.tile_rows : P.n_obs;
    double M, tot;
    mixis_wave_line<T, VEC, false>(reinterpret_cast<const T*>(P.in) + s * P.stride_draw + r0, r1 - r0, nullptr, tab, M, tot, n_nan,
                                   n_inf);
    if (wave_lane() == 0) {
      P.part[(P.tile0 + tile) * S + s] = M;
      P.part[(P.tiles_total + P.tile0 + tile) * S + s] = tot;
    }
  }
  mixis_count(P, n_nan, n_inf);
}

// c[s] from the tiles' partials of draw s, in tile order
__global__ __launch_bounds__(256) void mixis_c_merge_kernel(MixisParams P) {
  const int S = P.n_draws;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < S; s += (int64_t)gridDim.x * 256) {
    double m = P.part[s], acc = P.part[P.tiles_total * S + s];
    for (int64_t t = 1; t < P.tiles_total; ++t) {
      const double pm = P.part[t * S + s], ps = P.part[(P.tiles_total + t) * S + s];
      if (pm > m) {
        acc *= exp(m - pm);
        m = pm;
      }
      acc += ps * exp(pm - m);
    }
    P.c_out[s] = log(acc) + m;
  }
}

// ---- pass 2 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mixis_lse_c_kernel(MixisParams P) {
  __shared__ double red[4];
  const int S = P.n_draws;
  double mx = -pinf();
  for (int s = threadIdx.x; s < S; s += 256) mx = fmax(mx, -P.c[s]);
  const double m = block_reduce<OpMax, 256>(mx, red);
  double se = 0.0;
  for (int s = threadIdx.x; s < S; s += 256) se += exp(-P.c[s] - m);
  se = block_reduce<OpSum, 256>(se, red);
  if (threadIdx.x == 0) *P.lse_c = log(se) + m;
}

// rows of at most kMixisRegDraws draws, n_draws % VEC == 0, 16-byte aligned when VEC > 1
template <typename T, int VEC>
__global__ __launch_bounds__(kWave * kWavesPerBlock, 2) void mixis_row_wave_kernel(MixisParams P) {
  __shared__ __attribute__((aligned(16))) double tab[2 * kTabN];
  __shared__ __attribute__((aligned(16))) double lt[2 * kLogTabN];
  __shared__ __attribute__((aligned(16))) double cs[kMixisRegDraws];
  constexpr int EPT = kWaveSlots, NQ = EPT / VEC, kThreads = kWave * kWavesPerBlock;
  const int tid = threadIdx.x;
  const int S = P.n_draws;
  for (int j = tid; j < kTabN; j += kThreads) exp_table_entry(tab, j);
  for (int j = tid; j < kLogTabN; j += kThreads) log_table_entry(lt, j);
  for (int j = tid; j < kMixisRegDraws; j += kThreads) cs[j] = j < S ? P.c[j] : pinf();  // (past the row: y = -inf by itself)
  __syncthreads();
  const int lane = wave_lane();
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const double lse_c = *P.lse_c;
  const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
  unsigned n_nan = 0, n_inf = 0;
  for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wv; r < P.n_obs; r += nw) {
    const T* rp = reinterpret_cast<const T*>(P.in) + r * P.stride_obs;
    double y[EPT];
    double z = 0.0, mx = -pinf();
    int last = S - VEC;  // (opaque inside the row loop: otherwise the 64 clamped offsets are hoisted out of it and spill)
    asm volatile("" : "+s"(last));
    // slot q * VEC + e holds draw VEC * (lane + 64 q) + e; vectors past the row read its last one (finite like the row: z) and
    // meet c = +inf.  A group of vectors at a time, so that the loads in flight and the y they become fit the registers.
    constexpr int G = 4;
#pragma unroll
    for (int g = 0; g < NQ; g += G) {
      T x[G][VEC];
#pragma unroll
      for (int q = g; q < g + G; ++q) {
        const int d = (q * kWave + lane) * VEC;
        mixis_load_vec<T, VEC>(rp + min(d, last), x[q - g]);
      }
#pragma unroll
      for (int q = g; q < g + G; ++q) {
        const int d = (q * kWave + lane) * VEC;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          z = fma((double)x[q - g][e], 0.0, z);
          y[q * VEC + e] = -(double)x[q - g][e] - cs[d + e];
          mx = fmax(mx, y[q * VEC + e]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (__ballot(z != z) != 0ull) {  // rare: a NaN or an infinity in the row
      mx = -pinf();  // (a slot past the row: c = +inf makes it -inf again, whatever it read)
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int d = (q * kWave + lane) * VEC;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const double cc = cs[d + e];
          y[q * VEC + e] = mixis_fix(y[q * VEC + e], cc, cc < pinf(), n_nan, n_inf);
          mx = fmax(mx, y[q * VEC + e]);
        }
      }
    }
    const double m = wave_all<R_MAX>(mx);
    double se = 0.0;  // (the slots past the row: e^-700 each, nothing)
#pragma unroll
    for (int i = 0; i < EPT; ++i) se += exp_tab(fmax(y[i] - m, -700.0), tab);
    se = wave_all<R_SUM>(se);
    if (lane == 0) P.elpd[r] = lse_c - (log_tab(se, lt) + m);
  }
  mixis_count(P, n_nan, n_inf);
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void mixis_row_stream_kernel(MixisParams P) {
  __shared__ __attribute__((aligned(16))) double tab[2 * kTabN];
  __shared__ __attribute__((aligned(16))) double lt[2 * kLogTabN];
  for (int j = threadIdx.x; j < kTabN; j += 256) exp_table_entry(tab, j);
  for (int j = threadIdx.x; j < kLogTabN; j += 256) log_table_entry(lt, j);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const double lse_c = *P.lse_c;
  const int64_t nw = (int64_t)gridDim.x * 4;
  unsigned n_nan = 0, n_inf = 0;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < P.n_obs; r += nw) {
    double M, tot;
    mixis_wave_line<T, VEC, true>(reinterpret_cast<const T*>(P.in) + r * P.stride_obs, P.n_draws, P.c, tab, M, tot, n_nan, n_inf);
    if (wave_lane() == 0) P.elpd[r] = lse_c - (log_tab(tot, lt) + M);
  }
  mixis_count(P, n_nan, n_inf);
}

template <typename T>
__global__ __launch_bounds__(256) void mixis_col_kernel(MixisParams P) {
  __shared__ __attribute__((aligned(16))) double tab[2 * kTabN];
  __shared__ __attribute__((aligned(16))) double lt[2 * kLogTabN];
  for (int j = threadIdx.x; j < kTabN; j += 256) exp_table_entry(tab, j);
  for (int j = threadIdx.x; j < kLogTabN; j += 256) log_table_entry(lt, j);
  __syncthreads();
  const double lse_c = *P.lse_c;
  const int64_t n_blk = (P.n_obs + 255) / 256;
  unsigned n_nan = 0, n_inf = 0;
  for (int64_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
    const int64_t i = b * 256 + threadIdx.x;
    const bool live = i < P.n_obs;
    const T* col = reinterpret_cast<const T*>(P.in) + (live ? i : P.n_obs - 1);
    double m, se;
    mixis_lane_stream<T, true>(col, P.stride_draw, P.n_draws, P.c, tab, live, m, se, n_nan, n_inf);
    if (live) P.elpd[i] = lse_c - (log_tab(se, lt) + m);
  }
  mixis_count(P, n_nan, n_inf);
}

template <typename T>
__global__ __launch_bounds__(256) void mixis_row_block_kernel(MixisParams P) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int S = P.n_draws;
  const double lse_c = *P.lse_c;
  unsigned n_nan = 0, n_inf = 0;
  for (int64_t r = blockIdx.x; r < P.n_obs; r += gridDim.x) {
    const T* rp = reinterpret_cast<const T*>(P.in) + r * P.stride_obs;
    double mx = -pinf();
    for (int d = tid; d < S; d += 256) {
      const double cc = P.c[d];
      mx = fmax(mx, mixis_fix(-(double)rp[(int64_t)d * P.stride_draw] - cc, cc, true, n_nan, n_inf));
    }
    const double m = block_reduce<OpMax, 256>(mx, red);
    double se = 0.0;
    unsigned dummy = 0;
    for (int d = tid; d < S; d += 256) {
      const double cc = P.c[d];
      se += exp(mixis_fix(-(double)rp[(int64_t)d * P.stride_draw] - cc, cc, false, dummy, dummy) - m);
    }
    se = block_reduce<OpSum, 256>(se, red);
    if (tid == 0) P.elpd[r] = lse_c - (log(se) + m);
  }
  mixis_count(P, n_nan, n_inf);
}

}  // namespace pla
