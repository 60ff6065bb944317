// launcher of the draw-gather kernel of the approximate-posterior LOO pass (pla_draws.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include "pla_draws.h"
#include "pla_launch.h"

namespace pla {

int gather_lds_max_draws(int dtype) { return kGatherLdsBytes / (dtype == PLA_F64 ? 8 : 4); }

template <typename T, int ROUTE, int VEC>
static hipError_t launch_gather_lds(const GatherParams& p, size_t lds, hipStream_t stream) {
  auto kern = gather_draws_kernel<T, ROUTE, VEC>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kGatherLdsBytes);
    if (e != hipSuccess) return e;
  }
  constexpr int64_t kMaxGrid = 2048;  // eight workgroups per CU at most; the rows are strided over the grid
  const int64_t grid = p.n_rows < kMaxGrid ? p.n_rows : kMaxGrid;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kGatherThreads), lds, stream, p);
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_gather_typed(GatherParams p, hipStream_t stream, const char** route) {
  constexpr int kVec = 16 / (int)sizeof(T);
  if (p.stride_obs == 1 && p.stride_draw != 1 && p.n_rows > 1) {
    p.n_obs_tiles = (p.n_rows + kGatherTileObs - 1) / kGatherTileObs;
    const int64_t tiles = p.n_obs_tiles * (((int64_t)p.n_out + kGatherTileDraws - 1) / kGatherTileDraws);
    if (tiles > 0x7fffffff) return hipErrorInvalidValue;
    if (route) *route = "gather_draws_kernel<tile> (observations fastest: 64 x 16 tiles through LDS)";
    hipLaunchKernelGGL((gather_draws_kernel<T, kGatherTile, 1>), dim3((unsigned)tiles), dim3(256), 0, stream, p);
    return hipGetLastError();
  }
  const size_t row_bytes = ((size_t)p.n_draws * sizeof(T) + 15) & ~(size_t)15;
  if (p.stride_draw == 1 && row_bytes <= (size_t)kGatherLdsBytes) {
    // 16-byte loads and stores where every row and every output row starts on a 16-byte boundary
    const bool wide = (uintptr_t)p.in % 16 == 0 && (uintptr_t)p.out % 16 == 0 && p.stride_obs % kVec == 0 && p.n_out % kVec == 0;
    const size_t with_idx = row_bytes + (size_t)p.n_out * sizeof(int);
    if (with_idx <= (size_t)kGatherLdsBytes) {
      p.idx_off = (int)row_bytes;
      if (route)
        *route = wide ? "gather_draws_kernel<lds+index> (draws fastest: row and index staged in LDS; 16-byte loads)"
                      : "gather_draws_kernel<lds+index> (draws fastest: row and index staged in LDS; element loads)";
      return wide ? launch_gather_lds<T, kGatherLdsIdx, kVec>(p, with_idx, stream) : launch_gather_lds<T, kGatherLdsIdx, 1>(p, with_idx, stream);
    }
    if (route)
      *route = wide ? "gather_draws_kernel<lds> (draws fastest: row staged in LDS, index from global memory; 16-byte loads)"
                    : "gather_draws_kernel<lds> (draws fastest: row staged in LDS, index from global memory; element loads)";
    return wide ? launch_gather_lds<T, kGatherLds, kVec>(p, row_bytes, stream) : launch_gather_lds<T, kGatherLds, 1>(p, row_bytes, stream);
  }
  if (route) *route = "gather_draws_kernel<global> (gathered straight from global memory)";
  const int64_t chunks = ((int64_t)p.n_out + kGatherThreads - 1) / kGatherThreads;
  const int64_t gy = p.n_rows < 65535 ? p.n_rows : 65535;
  hipLaunchKernelGGL((gather_draws_kernel<T, kGatherGlobal, 1>), dim3((unsigned)chunks, (unsigned)gy), dim3(kGatherThreads), 0, stream, p);
  return hipGetLastError();
}

__global__ __launch_bounds__(64) void add_counter_kernel(const unsigned long long* value, unsigned long long* total) {
  if (threadIdx.x == 0) *total += *value;
}

hipError_t launch_add_counter(const unsigned long long* value, unsigned long long* total, hipStream_t stream) {
  hipLaunchKernelGGL(add_counter_kernel, dim3(1), dim3(64), 0, stream, value, total);
  return hipGetLastError();
}

hipError_t launch_gather_draws(const void* in, int dtype, int64_t stride_obs, int64_t stride_draw, int64_t n_rows, int n_draws,
                               const int64_t* draw_index, int n_out, void* out, unsigned long long* replaced, hipStream_t stream,
                               const char** route) {
  if (n_rows <= 0 || n_draws <= 0 || n_out <= 0) return hipSuccess;
  GatherParams p{in, stride_obs, stride_draw, n_rows, n_draws, draw_index, n_out, out, replaced, 0, 1};
  return dtype == PLA_F64 ? launch_gather_typed<double>(p, stream, route) : launch_gather_typed<float>(p, stream, route);
}

}  // namespace pla
