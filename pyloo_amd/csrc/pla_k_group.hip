// launcher of the group-sum kernel of the leave-one-group-out pass (pla_group.h)
// (one translation unit of libpyloo_amd.so: the kernels are compiled in parallel, pyloo_amd/build.py)
#include "pla_group.h"
#include "pla_launch.h"

namespace pla {

template <typename T, int VEC>
static hipError_t launch_group_sum_typed(GroupSumParams p, int64_t n_groups, hipStream_t stream) {
  constexpr int64_t kVecPerBlock = 64 * kGroupWaves;
  constexpr int64_t kMaxX = (int64_t)1 << 20, kMaxY = 32768;  // workgroups per launch along the groups / the draws
  const int64_t nvec = p.n_draws / VEC;
  const int64_t chunks = (nvec + kVecPerBlock - 1) / kVecPerBlock;
  void* out0 = p.out;
  const int64_t g0 = p.g0;
  for (int64_t gs = 0; gs < n_groups; gs += kMaxX) {
    const int64_t ng = n_groups - gs < kMaxX ? n_groups - gs : kMaxX;
    for (int64_t c0 = 0; c0 < chunks; c0 += kMaxY) {
      const int64_t nc = chunks - c0 < kMaxY ? chunks - c0 : kMaxY;
      p.g0 = g0 + gs;
      p.out = reinterpret_cast<T*>(out0) + gs * (int64_t)p.n_draws;
      p.vec0 = c0 * kVecPerBlock;
      hipLaunchKernelGGL((group_sum_kernel<T, VEC>), dim3((unsigned)ng, (unsigned)nc), dim3(64 * kGroupWaves), 0, stream, p);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

hipError_t launch_group_sum(const void* in, int dtype, int64_t stride_obs, int64_t row0, int64_t n_rows, int64_t n_src, bool blocked,
                            bool first_block, int n_draws, const int64_t* offsets, const int64_t* members, int64_t n_groups_total,
                            int64_t g0, int64_t n_groups, void* out, unsigned long long* replaced, hipStream_t stream,
                            const char** route) {
  // 16-byte loads and stores where every row and every output row starts on a 16-byte boundary
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int vec = (int)(16 / esz);
  const bool wide = (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0 && stride_obs % vec == 0 && n_draws % vec == 0;
  if (route) *route = wide ? "16-byte loads" : "element loads";
  if (n_groups <= 0 || n_draws <= 0) return hipSuccess;
  GroupSumParams p{in, stride_obs, row0, n_rows, n_src, blocked, first_block, n_draws, offsets, members, n_groups_total, g0, 0, out,
                   replaced};
  if (dtype == PLA_F64)
    return wide ? launch_group_sum_typed<double, 2>(p, n_groups, stream) : launch_group_sum_typed<double, 1>(p, n_groups, stream);
  return wide ? launch_group_sum_typed<float, 4>(p, n_groups, stream) : launch_group_sum_typed<float, 1>(p, n_groups, stream);
}

}  // namespace pla
