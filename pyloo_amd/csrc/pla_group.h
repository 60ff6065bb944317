// Group-sum kernel of the leave-one-group-out pass (reference: pyloo loo_group.py:188-197, 216-224).
//
//   out[g, s] = sum over the members m of group g, in ascending order, of ll[m, s]
//
// Numerical contract: bitwise NumPy's `ll[members].sum(axis=0)` -- a plain sequential sum over the member rows that starts
// from the first member's row (not from 0.0), one rounding per add, in the INPUT dtype (f32 sums stay f32).  Every lane owns
// VEC consecutive draws of one group and adds its members strictly in order; only the loads run ahead (two batches of
// kGroupBatch member rows in flight per lane).  NaN entries become -1e10 on load, before they are added (loo_group.py:188-197),
// and are counted; +-inf flow through IEEE addition as in the reference.
//
// One workgroup of four waves per (group, 256 vectors of draws: blockIdx.x, blockIdx.y); a wave per 64 vectors.  The matrix is read once
// (non-temporal loads).  Rows come either from the matrix in place (draws contiguous) or from a staging block of
// observations [row0, row0 + n_rows) (observations-fastest and host inputs, transposed / uploaded block by block): a group's
// members inside a block are a contiguous stretch of its ascending list (binary search), and the partial sums of the
// earlier blocks are read back from `out`, so the order of the adds is the same whatever the block size.
//
// Index lists are clamped into range here (device lists are not validated on the host): offsets into [0, offsets[G]],
// members into [0, n_src) and into the block.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pla {

struct GroupSumParams {
  const void* in;          // row (member - row0) of the block at in + (member - row0) * stride_obs, draws contiguous
  int64_t stride_obs;      // elements
  int64_t row0, n_rows;    // the block of observations held by `in`
  int64_t n_src;           // observations of the whole matrix (member clamp)
  bool blocked;            // several blocks: find each group's members inside the block, continue the partial sums
  bool first_block;        // (blocked) the first block: empty groups are written as 0 here
  int n_draws;
  const int64_t* offsets;  // [n_groups_total + 1]
  const int64_t* members;  // [offsets[n_groups_total]]
  int64_t n_groups_total;
  int64_t g0;              // first group of this launch (blockIdx.x = g - g0)
  int64_t vec0;            // first vector of draws of this launch (blockIdx.y: 256 vectors each)
  void* out;               // (groups, n_draws) C-contiguous: row g - g0
  unsigned long long* replaced;  // [1] NaN entries replaced (may be null)
};

constexpr int kGroupWaves = 4, kGroupBatch = 8;

template <typename T, int VEC>
struct GroupVec {
  T v[VEC];
};

template <typename T, int VEC>
__device__ __forceinline__ GroupVec<T, VEC> group_load(const T* p, unsigned& nrep) {
  GroupVec<T, VEC> r;
  if constexpr (VEC == 1) {
    r.v[0] = __builtin_nontemporal_load(p);
  } else {
    typedef T vt __attribute__((ext_vector_type(VEC)));
    const vt x = __builtin_nontemporal_load(reinterpret_cast<const vt*>(p));
#pragma unroll
    for (int e = 0; e < VEC; ++e) r.v[e] = x[e];
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const bool nan = r.v[e] != r.v[e];
    nrep += nan ? 1u : 0u;
    r.v[e] = nan ? (T)-1e10 : r.v[e];  // loo_group.py:197, in the input dtype
  }
  return r;
}

__device__ __forceinline__ int64_t group_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// first position in members[lo, hi) whose (clamped) value is >= key
__device__ __forceinline__ int64_t group_lower_bound(const int64_t* members, int64_t lo, int64_t hi, int64_t key, int64_t n_src) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (group_clamp(members[mid], 0, n_src - 1) < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <typename T, int VEC>
__global__ __launch_bounds__(64 * kGroupWaves) void group_sum_kernel(GroupSumParams P) {
  const int64_t g = P.g0 + (int64_t)blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t vec = P.vec0 + ((int64_t)blockIdx.y * kGroupWaves + wave) * 64 + (threadIdx.x & 63);
  const int nvec = P.n_draws / VEC;
  unsigned nrep = 0;
  if (vec < nvec) {
    const int64_t nm = group_clamp(P.offsets[P.n_groups_total], 0, INT64_MAX);
    int64_t lo = group_clamp(P.offsets[g], 0, nm);
    int64_t hi = group_clamp(P.offsets[g + 1], lo, nm);
    T* out = reinterpret_cast<T*>(P.out) + (g - P.g0) * (int64_t)P.n_draws + vec * VEC;
    const T* base = reinterpret_cast<const T*>(P.in) + vec * VEC;
    const int64_t last = P.n_src - 1;
    // (the row inside the block is clamped too: a device list that is not ascending cannot send a lane outside the staging block)
    const auto row = [&](int64_t m) {
      return base + group_clamp(group_clamp(P.members[m], 0, last) - P.row0, 0, P.n_rows - 1) * P.stride_obs;
    };
    bool empty = lo == hi, cont = false;
    if (P.blocked && !empty) {
      const int64_t a = group_lower_bound(P.members, lo, hi, P.row0, P.n_src);
      const int64_t b = group_lower_bound(P.members, a, hi, P.row0 + P.n_rows, P.n_src);
      cont = a != lo;  // members before this block: continue their partial sums
      lo = a;
      hi = b;
    }
    if (lo == hi) {
      if (empty && (!P.blocked || P.first_block)) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) out[e] = (T)0;
      }
    } else {
      GroupVec<T, VEC> acc;
      int64_t m = lo;
      if (cont) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[e] = out[e];
      } else {
        acc = group_load<T, VEC>(row(m), nrep);  // NumPy starts from the first member's row
        ++m;
      }
      // two batches of member rows in flight: the loads of batch k + 1 are issued before the adds of batch k
      GroupVec<T, VEC> x[kGroupBatch], y[kGroupBatch];
      if (m + kGroupBatch <= hi) {
#pragma unroll
        for (int k = 0; k < kGroupBatch; ++k) x[k] = group_load<T, VEC>(row(m + k), nrep);
        for (; m + 2 * kGroupBatch <= hi; m += kGroupBatch) {
#pragma unroll
          for (int k = 0; k < kGroupBatch; ++k) y[k] = group_load<T, VEC>(row(m + kGroupBatch + k), nrep);
#pragma unroll
          for (int k = 0; k < kGroupBatch; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc.v[e] += x[k].v[e];
#pragma unroll
          for (int k = 0; k < kGroupBatch; ++k) x[k] = y[k];
        }
#pragma unroll
        for (int k = 0; k < kGroupBatch; ++k)
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc.v[e] += x[k].v[e];
        m += kGroupBatch;
      }
      for (; m < hi; ++m) {
        const GroupVec<T, VEC> z = group_load<T, VEC>(row(m), nrep);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[e] += z.v[e];
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) out[e] = acc.v[e];
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
