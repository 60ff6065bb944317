// Draw-gather kernel of the approximate-posterior LOO pass (reference: pyloo loo_approximate_posterior.py:223-232, 263).
//
//   out[i, j] = ll[i * stride_obs + clamp(draw_index[j]) * stride_draw]      i in [0, n_rows),  j in [0, n_out)
//
// `out` is a draws-fastest (n_rows, n_out) block in the dtype of `ll`; the values are copied, never computed with.  NaN entries
// become -1e10 in the input dtype as they are written and are counted (one count per entry of `out`: the count is that of
// ll[:, draw_index], whatever the route); +-inf pass through.  The index may repeat draws and need not have n_draws entries; it is
// clamped into [0, n_draws) here (device lists are not validated on the host).
//
// Routes (template parameter ROUTE):
//   kGatherLds / kGatherLdsIdx   draws fastest (stride_draw == 1), rows of at most gather_lds_max_draws() draws: a workgroup walks over
//       rows; a row is staged in LDS with coalesced 16-byte non-temporal loads, then out[j] = lds[idx[j]] is written coalesced.  The
//       matrix is read once.  kGatherLdsIdx also keeps the clamped index in LDS (32-bit, loaded once per workgroup, shared by all
//       its rows) when row + index fit the budget; kGatherLds reads the index from global memory (L2) for every row.
//   kGatherGlobal   any strides, any row length: a lane per output draw holds its index in a register and walks over the rows,
//       gathering straight from global memory.
//   kGatherTile   observations fastest (stride_obs == 1): transpose_rows_kernel (pla_k_general.hip) with the source draw row looked
//       up through the index; 64 observations x 16 draws through an LDS tile, reads and writes both coalesced.
//
// LDS budget: 80 KB per workgroup, i.e. two workgroups of eight waves on a CU's 160 KB at the longest rows, more at shorter ones
// (the allocation is the row (+ the index), not the budget).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pla {

enum GatherRoute { kGatherLds = 0, kGatherLdsIdx = 1, kGatherGlobal = 2, kGatherTile = 3 };

constexpr int kGatherThreads = 512;
constexpr int kGatherLdsBytes = 80 * 1024;
constexpr int kGatherTileDraws = 16, kGatherTileObs = 64;

struct GatherParams {
  const void* in;
  int64_t stride_obs, stride_draw;  // elements
  int64_t n_rows;
  int n_draws;
  const int64_t* draw_index;  // [n_out]
  int n_out;
  void* out;                     // (n_rows, n_out) C-contiguous
  unsigned long long* replaced;  // [1] NaN entries replaced (may be null)
  int idx_off;                   // kGatherLdsIdx: byte offset of the index behind the row in LDS
  int64_t n_obs_tiles;           // kGatherTile: tiles of 64 observations (blockIdx.x = draw chunk * n_obs_tiles + observation tile)
};

__device__ __forceinline__ int gather_clamp(int64_t v, int n_draws) { return v < 0 ? 0 : (v >= n_draws ? n_draws - 1 : (int)v); }

template <typename T>
__device__ __forceinline__ T gather_fix(T x, unsigned& nrep) {
  const bool nan = x != x;
  nrep += nan ? 1u : 0u;
  return nan ? (T)-1e10 : x;  // loo_approximate_posterior.py:232, in the input dtype
}

template <typename T, int ROUTE, int VEC>
__global__ __launch_bounds__(ROUTE == kGatherTile ? 256 : kGatherThreads) void gather_draws_kernel(GatherParams P) {
  const int tid = threadIdx.x;
  const T* in = reinterpret_cast<const T*>(P.in);
  T* out = reinterpret_cast<T*>(P.out);
  unsigned nrep = 0;
  if constexpr (ROUTE == kGatherLds || ROUTE == kGatherLdsIdx) {
    typedef T vt __attribute__((ext_vector_type(VEC)));
    extern __shared__ __attribute__((aligned(16))) unsigned char gather_lds[];
    T* row = reinterpret_cast<T*>(gather_lds);
    int* lidx = reinterpret_cast<int*>(gather_lds + P.idx_off);
    if constexpr (ROUTE == kGatherLdsIdx) {
      for (int j = tid; j < P.n_out; j += kGatherThreads) lidx[j] = gather_clamp(P.draw_index[j], P.n_draws);
      // (visible to the other waves behind the barrier that follows the first row's staging)
    }
    const int nvec = P.n_draws / VEC, nvec_out = P.n_out / VEC;  // (VEC > 1: n_out is a multiple of VEC)
    for (int64_t r = blockIdx.x; r < P.n_rows; r += gridDim.x) {
      const T* src = in + r * P.stride_obs;
      if constexpr (VEC == 1) {
#pragma unroll 4
        for (int e = tid; e < P.n_draws; e += kGatherThreads) row[e] = __builtin_nontemporal_load(src + e);
      } else {
#pragma unroll 4
        for (int v = tid; v < nvec; v += kGatherThreads)
          reinterpret_cast<vt*>(row)[v] = __builtin_nontemporal_load(reinterpret_cast<const vt*>(src) + v);
        for (int e = nvec * VEC + tid; e < P.n_draws; e += kGatherThreads) row[e] = __builtin_nontemporal_load(src + e);
      }
      __syncthreads();
      T* dst = out + r * (int64_t)P.n_out;
#pragma unroll 2
      for (int v = tid; v < nvec_out; v += kGatherThreads) {
        int s[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if constexpr (ROUTE == kGatherLdsIdx) s[e] = lidx[v * VEC + e];
          else s[e] = gather_clamp(P.draw_index[v * VEC + e], P.n_draws);
        }
        if constexpr (VEC == 1) {
          dst[v] = gather_fix(row[s[0]], nrep);
        } else {
          vt y;
#pragma unroll
          for (int e = 0; e < VEC; ++e) y[e] = gather_fix(row[s[e]], nrep);
          reinterpret_cast<vt*>(dst)[v] = y;
        }
      }
      __syncthreads();  // the next row overwrites the staged one
    }
  } else if constexpr (ROUTE == kGatherGlobal) {
    const int64_t j = (int64_t)blockIdx.x * kGatherThreads + tid;
    if (j < P.n_out) {
      const T* col = in + (int64_t)gather_clamp(P.draw_index[j], P.n_draws) * P.stride_draw;
      for (int64_t r = blockIdx.y; r < P.n_rows; r += gridDim.y) out[r * (int64_t)P.n_out + j] = gather_fix(col[r * P.stride_obs], nrep);
    }
  } else {
    // the +1 pitch keeps the column reads at two lanes per bank for f64 and conflict-free for f32 (as transpose_rows_kernel)
    constexpr int TD = kGatherTileDraws, TO = kGatherTileObs;
    __shared__ T tile[TD][TO + 1];
    const int64_t o0 = ((int64_t)blockIdx.x % P.n_obs_tiles) * TO;
    const int64_t d0 = ((int64_t)blockIdx.x / P.n_obs_tiles) * TD;
    {
      const int tx = tid & (TO - 1), ty = tid >> 6;
      const int64_t oi = o0 + tx;
#pragma unroll 4
      for (int d = ty; d < TD; d += 4) {
        const int64_t dd = d0 + d;
        if (dd < P.n_out && oi < P.n_rows) {
          const int64_t s = gather_clamp(P.draw_index[dd], P.n_draws);  // (one address per wave: a scalar load)
          tile[d][tx] = gather_fix(__builtin_nontemporal_load(in + s * P.stride_draw + oi), nrep);
        }
      }
    }
    __syncthreads();
    {
      const int tx = tid & (TD - 1), ty = tid / TD;
      const int64_t dw = d0 + tx;
#pragma unroll 4
      for (int o = ty; o < TO; o += 256 / TD) {
        const int64_t oo = o0 + o;
        if (oo < P.n_rows && dw < P.n_out) out[oo * (int64_t)P.n_out + dw] = tile[tx][o];
      }
    }
  }
  if (P.replaced) {
    unsigned tot = nrep;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
    if ((threadIdx.x & 63) == 0 && tot) atomicAdd(P.replaced, (unsigned long long)tot);
  }
}

}  // namespace pla
