// C ABI of libpyloo_amd.so, views of the matrix that end in the PSIS-LOO pass: groups of observations, gathered draws, k-fold.
#include <string>

#include "pla_capi.h"

using namespace pla::capi;

extern "C" {

// ---- leave-one-group-out (loo_group.py:216-300) ------------------------------------------------------------------------------
// Group index: group_offsets[n_groups + 1], group_members[group_offsets[n_groups]], in the memory space of the matrix.  Host lists
// are checked here; device lists are clamped by the group-sum kernel (pla_group.h).
static int check_groups(const int64_t* offsets, const int64_t* members, int64_t n_groups, int64_t n_obs, int mem_space) {
  if (n_groups < 0) return fail(PLA_ERR_ARG, "n_groups < 0");
  if (!offsets) return fail(PLA_ERR_ARG, "group_offsets is NULL");
  if (n_groups > 0 && n_obs < 1) return fail(PLA_ERR_ARG, "groups of an empty matrix");
  if (mem_space == PLA_DEVICE) {
    if (n_groups > 0 && !members) return fail(PLA_ERR_ARG, "group_members is NULL");
    return PLA_OK;
  }
  if (offsets[0] != 0) return fail(PLA_ERR_ARG, "group_offsets[0] must be 0, got %lld", (long long)offsets[0]);
  for (int64_t g = 0; g < n_groups; ++g)
    if (offsets[g + 1] < offsets[g]) return fail(PLA_ERR_ARG, "group_offsets decrease at group %lld", (long long)g);
  if (offsets[n_groups] > 0 && !members) return fail(PLA_ERR_ARG, "group_members is NULL");
  for (int64_t g = 0; g < n_groups; ++g)
    for (int64_t m = offsets[g]; m < offsets[g + 1]; ++m) {
      if (members[m] < 0 || members[m] >= n_obs)
        return fail(PLA_ERR_ARG, "group_members[%lld] = %lld is outside [0, %lld)", (long long)m, (long long)members[m], (long long)n_obs);
      if (m > offsets[g] && members[m] < members[m - 1])
        return fail(PLA_ERR_ARG, "the members of group %lld are not in ascending order", (long long)g);
    }
  return PLA_OK;
}

// groups per block of the group-sum buffer: sized like the ingest staging (4 GiB on the device -- PLA_INGEST_BLOCK_MB, a path
// selector: the results do not depend on it -- and 1 GiB from the host)
static int64_t group_block(int mem_space, int64_t n_groups, int64_t n_draws, size_t esz) {
  const int64_t r = staged_chunk_rows(mem_space, true, n_groups, n_draws, esz);
  return r > 0 ? r : 1;
}

// Device index lists are used as they are; host lists go up to the engine buffer behind the replaced-entry counter (word 0).
static int group_index_on_device(pla_engine* eng, const int64_t* offsets, const int64_t* members, int64_t n_groups, int mem_space,
                                 hipStream_t s, const int64_t** d_off, const int64_t** d_mem, unsigned long long** d_count) {
  if (mem_space == PLA_DEVICE) {
    *d_off = offsets;
    *d_mem = members;
    *d_count = nullptr;
    return PLA_OK;
  }
  const int64_t nm = offsets[n_groups];
  int rc = eng->d_gidx.reserve((size_t)(1 + n_groups + 1 + nm) * sizeof(int64_t));
  if (rc) return rc;
  int64_t* d = eng->d_gidx.as<int64_t>();
  PLA_HIP(hipMemsetAsync(d, 0, sizeof(int64_t), s));
  PLA_HIP(hipMemcpyAsync(d + 1, offsets, (size_t)(n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  if (nm > 0) PLA_HIP(hipMemcpyAsync(d + 2 + n_groups, members, (size_t)nm * sizeof(int64_t), hipMemcpyHostToDevice, s));
  *d_off = d + 1;
  *d_mem = d + 2 + n_groups;
  *d_count = (unsigned long long*)d;
  return PLA_OK;
}

// Sums of groups [g0, g0 + ng) into `out` (device, (ng, n_draws) C-contiguous, dtype of ll).  Draws-contiguous device matrices are
// read in place; observations-fastest device matrices are transposed block by block into the ingest staging, host matrices are
// uploaded block by block (one pass over the matrix per call: a host matrix whose group sums exceed one block of groups is
// read once per block).  The blocks go in ascending order and the kernel continues the partial sums, so the order of the adds
// is NumPy's whatever the block sizes.
static int group_sums_run(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                          int64_t stride_draw, const int64_t* d_off, const int64_t* d_mem, int64_t n_groups, int64_t g0, int64_t ng,
                          int mem_space, hipStream_t s, void* out, unsigned long long* replaced) {
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const char* leg = "";  // the vector leg of the (last) launch: "16-byte loads" / "element loads"
  if (mem_space == PLA_DEVICE && stride_draw == 1) {
    PLA_HIP(pla::launch_group_sum(ll, dtype, stride_obs, 0, n_obs, n_obs, false, true, (int)n_draws, d_off, d_mem, n_groups, g0, ng,
                                  out, replaced, s, &leg));
    eng->last_kernels = std::string("group_sum_kernel (matrix read in place; ") + leg + ")";
    return PLA_OK;
  }
  const bool obs_fastest = n_obs > 1 && n_draws > 1 && stride_obs == 1 && stride_draw >= n_obs;
  if (!obs_fastest && !(mem_space == PLA_HOST && stride_draw == 1))
    return fail(PLA_ERR_UNSUPPORTED, "group sums need unit stride along the draws, or along the observations");
  const size_t row_bytes = (size_t)n_draws * esz;
  const int64_t rows_per_chunk = staged_chunk_rows(mem_space, mem_space == PLA_DEVICE, n_obs, n_draws, esz);
  int rc = eng->d_in.reserve((size_t)rows_per_chunk * row_bytes);
  if (rc) return rc;
  const bool blocked = rows_per_chunk < n_obs;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows_per_chunk) {
    const int64_t nr = (n_obs - r0 < rows_per_chunk) ? (n_obs - r0) : rows_per_chunk;
    if (mem_space == PLA_DEVICE) {
      PLA_HIP(pla::launch_transpose_rows(ll, dtype, stride_draw, r0, nr, (int)n_draws, eng->d_in.p, s));
    } else {
      rc = stage_rows(eng, ll, nullptr, r0, nr, stride_obs, stride_draw, dtype, n_draws, rows_per_chunk, s);
      if (rc) return rc;
    }
    PLA_HIP(pla::launch_group_sum(eng->d_in.p, dtype, n_draws, r0, nr, n_obs, blocked, r0 == 0, (int)n_draws, d_off, d_mem, n_groups, g0,
                                  ng, out, replaced, s, &leg));
    if (mem_space == PLA_HOST) PLA_HIP(hipStreamSynchronize(s));  // the staging buffer is reused by the next block
  }
  // (every block has the staging buffer's base and pitch: one leg for all of them)
  eng->last_kernels = std::string(mem_space == PLA_DEVICE ? "transpose_rows_kernel + group_sum_kernel (blocks of observations; "
                                                          : "group_sum_kernel (blocks of observations uploaded; ") + leg + ")";
  return PLA_OK;
}

int pla_group_sum(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                  const int64_t* group_offsets, const int64_t* group_members, int64_t n_groups, int mem_space, void* stream, void* out,
                  int64_t* n_replaced) {
  int rc = check_common(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, PLA_SIS, 0, mem_space);
  if (rc) return rc;
  rc = check_groups(group_offsets, group_members, n_groups, n_obs, mem_space);
  if (rc) return rc;
  if (n_groups > 0 && !out) return fail(PLA_ERR_ARG, "out is NULL");
  PLA_ENGINE_CALL(eng, stream);
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int64_t* d_off = nullptr;
  const int64_t* d_mem = nullptr;
  unsigned long long* d_count = nullptr;
  rc = group_index_on_device(eng, group_offsets, group_members, n_groups, mem_space, s, &d_off, &d_mem, &d_count);
  if (rc) return rc;
  if (mem_space == PLA_DEVICE) {
    if (n_replaced) PLA_HIP(hipMemsetAsync(n_replaced, 0, sizeof(int64_t), s));
    TimedLaunch t(eng, s);  // (the group-sum kernel's own time: pla_engine_kernel_ms)
    return group_sums_run(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, d_off, d_mem, n_groups, 0, n_groups, mem_space, s, out,
                          (unsigned long long*)n_replaced);
  }
  const int64_t gb = group_block(mem_space, n_groups, n_draws, esz);
  if (n_groups > 0) {
    rc = eng->d_grp.reserve((size_t)gb * (size_t)n_draws * esz);
    if (rc) return rc;
  }
  for (int64_t g0 = 0; g0 < n_groups; g0 += gb) {
    const int64_t ng = n_groups - g0 < gb ? n_groups - g0 : gb;
    rc = group_sums_run(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, d_off, d_mem, n_groups, g0, ng, mem_space, s, eng->d_grp.p,
                        d_count);
    if (rc) return rc;
    PLA_HIP(hipMemcpyAsync((char*)out + (size_t)g0 * (size_t)n_draws * esz, eng->d_grp.p, (size_t)ng * (size_t)n_draws * esz,
                           hipMemcpyDeviceToHost, s));
  }
  unsigned long long h = 0;
  if (n_replaced) PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

int pla_psis_loo_groups(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                        int64_t stride_draw, const int64_t* group_offsets, const int64_t* group_members, int64_t n_groups, int method,
                        int64_t tail_count, double scale_value, double good_k, int mem_space, void* stream, double* diag,
                        double* logo_i, double* lppd_i, double* agg, int64_t* n_replaced) {
  int rc = check_common(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, method, tail_count, mem_space);
  if (rc) return rc;
  if (n_groups < 1) return fail(PLA_ERR_ARG, "n_groups < 1");
  rc = check_groups(group_offsets, group_members, n_groups, n_obs, mem_space);
  if (rc) return rc;
  PLA_ENGINE_CALL(eng, stream);
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int64_t* d_off = nullptr;
  const int64_t* d_mem = nullptr;
  unsigned long long* d_count = nullptr;
  rc = group_index_on_device(eng, group_offsets, group_members, n_groups, mem_space, s, &d_off, &d_mem, &d_count);
  if (rc) return rc;
  if (mem_space == PLA_DEVICE) {
    d_count = (unsigned long long*)n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  }
  // pointwise outputs: the caller's device vectors, else (host calls, or agg without them) the engine scratch
  double *dd = diag, *dl = logo_i, *dp = lppd_i;
  HostOutputs out(eng, s);
  if (mem_space == PLA_HOST || (agg && (!dd || !dl || !dp))) {
    rc = out.reserve(3, n_groups);
    if (rc) return rc;
    if (mem_space == PLA_HOST || !dd) dd = out.col(0);
    if (mem_space == PLA_HOST || !dl) dl = out.col(1);
    if (mem_space == PLA_HOST || !dp) dp = out.col(2);
  }
  // one block of groups at a time: its sums in the bounded buffer, the PSIS / SIS / TIS pass over them into its slices
  const int64_t gb = group_block(mem_space, n_groups, n_draws, esz);
  rc = eng->d_grp.reserve((size_t)gb * (size_t)n_draws * esz);
  if (rc) return rc;
  std::string label;
  for (int64_t g0 = 0; g0 < n_groups; g0 += gb) {
    const int64_t ng = n_groups - g0 < gb ? n_groups - g0 : gb;
    rc = group_sums_run(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, d_off, d_mem, n_groups, g0, ng, mem_space, s,
                        eng->d_grp.p, d_count);
    if (rc) return rc;
    const std::string sum_kernels = eng->last_kernels;
    rc = psis_loo_run(eng, eng->d_grp.p, dtype, ng, nullptr, ng, n_draws, n_draws, 1, method, tail_count, scale_value, good_k, PLA_DEVICE,
                      stream, dd ? dd + g0 : nullptr, dl ? dl + g0 : nullptr, dp ? dp + g0 : nullptr, nullptr);
    if (rc) return rc;
    if (g0 == 0) label = sum_kernels + " per block of groups, then " + eng->last_kernels;
  }
  eng->last_kernels = label;
  // the aggregates once, over all groups
  double* dagg = mem_space == PLA_HOST ? out.col(3) : agg;
  if (agg) {
    pla::ReduceParams rp{dd, dl, dp, n_groups, good_k, dagg, eng->counters + 1};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
  }
  if (mem_space == PLA_DEVICE) return PLA_OK;
  rc = out.copy_back({diag, logo_i, lppd_i});
  if (rc) return rc;
  if (agg) PLA_HIP(hipMemcpyAsync(agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  unsigned long long h = 0;
  if (n_replaced) PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

// ---- approximate posteriors (loo_approximate_posterior.py:223-348) -------------------------------------------------------------
// Draw index: draw_index[n_out] in the memory space of the matrix.  Host lists are checked here; device lists are clamped by the
// gather kernel (pla_draws.h).
static int check_draws(const int64_t* draw_index, int64_t n_out, int64_t n_draws, int mem_space) {
  if (n_out < 1 || n_out > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "n_out out of range");
  if (!draw_index) return fail(PLA_ERR_ARG, "draw_index is NULL");
  if (mem_space == PLA_HOST)
    for (int64_t j = 0; j < n_out; ++j)
      if (draw_index[j] < 0 || draw_index[j] >= n_draws)
        return fail(PLA_ERR_ARG, "draw_index[%lld] = %lld is outside [0, %lld)", (long long)j, (long long)draw_index[j], (long long)n_draws);
  return PLA_OK;
}

// Device index lists are used as they are; host lists go up to the engine buffer behind the replaced-entry counter (word 0).
static int draw_index_on_device(pla_engine* eng, const int64_t* draw_index, int64_t n_out, int mem_space, hipStream_t s,
                                const int64_t** d_idx, unsigned long long** d_count) {
  if (mem_space == PLA_DEVICE) {
    *d_idx = draw_index;
    *d_count = nullptr;
    return PLA_OK;
  }
  int rc = eng->d_gidx.reserve((size_t)(1 + n_out) * sizeof(int64_t));
  if (rc) return rc;
  int64_t* d = eng->d_gidx.as<int64_t>();
  PLA_HIP(hipMemsetAsync(d, 0, sizeof(int64_t), s));
  PLA_HIP(hipMemcpyAsync(d + 1, draw_index, (size_t)n_out * sizeof(int64_t), hipMemcpyHostToDevice, s));
  *d_idx = d + 1;
  *d_count = (unsigned long long*)d;
  return PLA_OK;
}

// Rows [r0, r0 + nr) of the matrix with their draws gathered into `dst` (device, (nr, n_out) C-contiguous).  Device matrices are
// read in place; a block of a host matrix goes up to the slab buffer as it lies -- (nr, n_draws) rows, or the (n_draws, nr) slab
// of an observations-fastest matrix -- and is gathered from there.
static int gather_block(pla_engine* eng, const void* ll, int dtype, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                        const int64_t* d_idx, int64_t n_out, int64_t r0, int64_t nr, int mem_space, hipStream_t s, void* dst,
                        unsigned long long* d_count, const char** route) {
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  if (mem_space == PLA_DEVICE) {
    PLA_HIP(pla::launch_gather_draws((const char*)ll + (size_t)r0 * (size_t)stride_obs * esz, dtype, stride_obs, stride_draw, nr,
                                     (int)n_draws, d_idx, (int)n_out, dst, d_count, s, route));
    return PLA_OK;
  }
  if (stride_draw == 1) {
    if (int rc = upload_rows(ll, nullptr, r0, nr, stride_obs, n_draws, esz, eng->d_slab.p, s)) return rc;
    PLA_HIP(pla::launch_gather_draws(eng->d_slab.p, dtype, n_draws, 1, nr, (int)n_draws, d_idx, (int)n_out, dst, d_count, s, route));
  } else {
    if (int rc = upload_slab(ll, r0, nr, stride_draw, n_draws, esz, eng->d_slab.p, s)) return rc;
    PLA_HIP(pla::launch_gather_draws(eng->d_slab.p, dtype, 1, nr, nr, (int)n_draws, d_idx, (int)n_out, dst, d_count, s, route));
  }
  return PLA_OK;
}

static int check_gather(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                        int64_t stride_draw, const int64_t* draw_index, int64_t n_out, int mem_space) {
  int rc = check_common(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, PLA_SIS, 0, mem_space);
  if (rc) return rc;
  rc = check_draws(draw_index, n_out, n_draws, mem_space);
  if (rc) return rc;
  if (mem_space == PLA_HOST && stride_draw != 1 && !host_obs_fastest(n_obs, n_draws, stride_obs, stride_draw))
    return fail(PLA_ERR_UNSUPPORTED, "PLA_HOST input needs unit stride along the draws, or along the observations");
  return PLA_OK;
}

// rows per block of a host call: the slab holds n_draws, the staging n_out entries per row
static int64_t host_gather_rows(int64_t n_obs, int64_t n_draws, int64_t n_out, size_t esz) {
  return staged_chunk_rows(PLA_HOST, false, n_obs, n_draws > n_out ? n_draws : n_out, esz);
}

int pla_gather_draws(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs, int64_t stride_draw,
                     const int64_t* draw_index, int64_t n_out, int mem_space, void* stream, void* out, int64_t* n_replaced) {
  int rc = check_gather(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, draw_index, n_out, mem_space);
  if (rc) return rc;
  if (n_obs > 0 && !out) return fail(PLA_ERR_ARG, "out is NULL");
  PLA_ENGINE_CALL(eng, stream);
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int64_t* d_idx = nullptr;
  unsigned long long* d_count = nullptr;
  rc = draw_index_on_device(eng, draw_index, n_out, mem_space, s, &d_idx, &d_count);
  if (rc) return rc;
  const char* route = "";
  if (mem_space == PLA_DEVICE) {
    if (n_replaced) PLA_HIP(hipMemsetAsync(n_replaced, 0, sizeof(int64_t), s));
    TimedLaunch t(eng, s);  // (the gather kernel's own time: pla_engine_kernel_ms)
    rc = gather_block(eng, ll, dtype, n_draws, stride_obs, stride_draw, d_idx, n_out, 0, n_obs, mem_space, s, out,
                      (unsigned long long*)n_replaced, &route);
    eng->last_kernels = std::string(route) + " (matrix read in place)";
    return rc;
  }
  const int64_t rows = host_gather_rows(n_obs, n_draws, n_out, esz);
  rc = eng->d_slab.reserve((size_t)rows * (size_t)n_draws * esz);
  if (rc) return rc;
  rc = eng->d_in.reserve((size_t)rows * (size_t)n_out * esz);
  if (rc) return rc;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    rc = gather_block(eng, ll, dtype, n_draws, stride_obs, stride_draw, d_idx, n_out, r0, nr, mem_space, s, eng->d_in.p, d_count, &route);
    if (rc) return rc;
    PLA_HIP(hipMemcpyAsync((char*)out + (size_t)r0 * (size_t)n_out * esz, eng->d_in.p, (size_t)nr * (size_t)n_out * esz,
                           hipMemcpyDeviceToHost, s));
    PLA_HIP(hipStreamSynchronize(s));  // the buffers are reused by the next block
  }
  eng->last_kernels = std::string(route) + " (blocks of observations uploaded)";
  unsigned long long h = 0;
  if (n_replaced) PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

int pla_psis_loo_draws(pla_engine* eng, const void* ll, int dtype, int64_t n_obs, int64_t n_draws, int64_t stride_obs,
                       int64_t stride_draw, const int64_t* draw_index, int64_t n_out, int method, int64_t tail_count, double scale_value,
                       double good_k, int mem_space, void* stream, double* diag, double* loo_i, double* lppd_i, double* agg,
                       int64_t* n_replaced) {
  int rc = check_gather(eng, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, draw_index, n_out, mem_space);
  if (rc) return rc;
  rc = check_common(eng, ll, dtype, n_obs, n_out, n_out, 1, method, tail_count, mem_space);  // the pass runs over n_out draws
  if (rc) return rc;
  PLA_ENGINE_CALL(eng, stream);
  const size_t esz = dtype == PLA_F64 ? 8 : 4;
  const int64_t* d_idx = nullptr;
  unsigned long long* d_count = nullptr;
  rc = draw_index_on_device(eng, draw_index, n_out, mem_space, s, &d_idx, &d_count);
  if (rc) return rc;
  if (mem_space == PLA_DEVICE) {
    d_count = (unsigned long long*)n_replaced;
    if (d_count) PLA_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  }
  // pointwise outputs: the caller's device vectors, else (host calls, or agg without them) the engine scratch
  double *dd = diag, *dl = loo_i, *dp = lppd_i;
  HostOutputs out(eng, s);
  if (mem_space == PLA_HOST || (agg && (!dd || !dl || !dp))) {
    rc = out.reserve(3, n_obs);
    if (rc) return rc;
    if (mem_space == PLA_HOST || !dd) dd = out.col(0);
    if (mem_space == PLA_HOST || !dl) dl = out.col(1);
    if (mem_space == PLA_HOST || !dp) dp = out.col(2);
  }
  // one block of observations at a time: its gathered rows in the bounded staging buffer, the PSIS / SIS / TIS pass over them into
  // its slices
  const int64_t rows = mem_space == PLA_DEVICE ? staged_chunk_rows(mem_space, true, n_obs, n_out, esz) : host_gather_rows(n_obs, n_draws, n_out, esz);
  if (mem_space == PLA_HOST) {
    rc = eng->d_slab.reserve((size_t)rows * (size_t)n_draws * esz);
    if (rc) return rc;
  }
  rc = eng->d_in.reserve((size_t)rows * (size_t)n_out * esz);
  if (rc) return rc;
  // (every block's pass zeroes the slow-row total it reports: the blocks' totals are summed beside it and put back for the reduction)
  unsigned long long* block_total = eng->counters + pla::kCounterBlockTotal;
  PLA_HIP(hipMemsetAsync(block_total, 0, sizeof(unsigned long long), s));
  std::string label;
  for (int64_t r0 = 0; r0 < n_obs; r0 += rows) {
    const int64_t nr = n_obs - r0 < rows ? n_obs - r0 : rows;
    const char* route = "";
    rc = gather_block(eng, ll, dtype, n_draws, stride_obs, stride_draw, d_idx, n_out, r0, nr, mem_space, s, eng->d_in.p, d_count, &route);
    if (rc) return rc;
    rc = psis_loo_run(eng, eng->d_in.p, dtype, nr, nullptr, nr, n_out, n_out, 1, method, tail_count, scale_value, good_k, PLA_DEVICE, stream,
                      dd ? dd + r0 : nullptr, dl ? dl + r0 : nullptr, dp ? dp + r0 : nullptr, nullptr);
    if (rc) return rc;
    PLA_HIP(pla::launch_add_counter(eng->counters + 1, block_total, s));
    if (r0 == 0) label = std::string(route) + " per block of observations, then " + eng->last_kernels;
    if (mem_space == PLA_HOST) PLA_HIP(hipStreamSynchronize(s));  // the buffers are reused by the next block
  }
  eng->last_kernels = label;
  // the aggregates once, over all observations
  double* dagg = mem_space == PLA_HOST ? out.col(3) : agg;
  if (agg) {
    pla::ReduceParams rp{dd, dl, dp, n_obs, good_k, dagg, block_total};
    PLA_HIP(pla::launch_reduce(rp, eng->d_red, s));
  }
  if (mem_space == PLA_DEVICE) return PLA_OK;
  rc = out.copy_back({diag, loo_i, lppd_i});
  if (rc) return rc;
  if (agg) PLA_HIP(hipMemcpyAsync(agg, dagg, PLA_AGG_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  unsigned long long h = 0;
  if (n_replaced) PLA_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
  PLA_HIP(hipStreamSynchronize(s));
  if (n_replaced) *n_replaced = (int64_t)h;
  return PLA_OK;
}

int pla_gather_lds_max_draws(int dtype) { return pla::gather_lds_max_draws(dtype); }

// ---- k-fold cross-validation (loo_kfold.py:250-299, 643-692) -------------------------------------------------------------------
int pla_kfold_lme(pla_engine* eng, const void* const* src_base, const int64_t* src_rows, const int64_t* src_draws,
                  const int64_t* src_stride_row, const int64_t* src_stride_draw, int64_t n_sources, int dtype, int nan_flag,
                  const int64_t* source_offsets, const int64_t* task_row, const int64_t* task_out, int64_t n_tasks, int mem_space,
                  void* stream, double* out, int64_t n_out, int64_t* n_replaced) {
  if (int rc0 = check_engine_types(eng, dtype, mem_space)) return rc0;
  if (mem_space == PLA_HOST) return fail(PLA_ERR_UNSUPPORTED, "pla_kfold_lme reads device memory only (upload the fold matrices first)");
  if (n_sources < 1 || n_sources > (int64_t)1 << 24) return fail(PLA_ERR_ARG, "n_sources out of range");
  if (!src_base || !src_rows || !src_draws || !src_stride_row || !src_stride_draw) return fail(PLA_ERR_ARG, "a source array is NULL");
  if (n_tasks < 0 || n_out < 0) return fail(PLA_ERR_ARG, "n_tasks < 0 or n_out < 0");
  if (n_tasks > 0 && (!source_offsets || !task_row || !task_out || !out)) return fail(PLA_ERR_ARG, "a task array or out is NULL");
  for (int64_t k = 0; k < n_sources; ++k) {
    if (src_rows[k] < 0) return fail(PLA_ERR_ARG, "source %lld: n_rows < 0", (long long)k);
    if (src_rows[k] > 0 && !src_base[k]) return fail(PLA_ERR_ARG, "source %lld: base pointer is NULL", (long long)k);
    if (src_draws[k] < 1 || src_draws[k] > (int64_t)1 << 30) return fail(PLA_ERR_ARG, "source %lld: n_draws out of range", (long long)k);
    if (src_stride_row[k] < 0 || src_stride_draw[k] <= 0) return fail(PLA_ERR_ARG, "source %lld: bad strides", (long long)k);
  }
  PLA_ENGINE_CALL(eng, stream);
  if (n_replaced) PLA_HIP(hipMemsetAsync(n_replaced, 0, sizeof(int64_t), s));
  if (n_tasks == 0) return PLA_OK;
  // the table: built in pinned host memory that outlives the call, uploaded on the caller's stream
  const size_t bytes = (size_t)n_sources * sizeof(pla::KfoldSource);
  int rc = eng->d_kf.reserve(bytes);
  if (rc) return rc;
  const int turn = eng->kf_turn;
  eng->kf_turn ^= 1;
  if (!eng->kf_event[turn]) {
    if (g_frozen) return fail(PLA_ERR_FROZEN, "the engine is frozen and has no k-fold table yet");
    PLA_HIP(hipEventCreateWithFlags(&eng->kf_event[turn], hipEventDisableTiming));
  } else {
    PLA_HIP(hipEventSynchronize(eng->kf_event[turn]));  // (the upload of two calls ago: done, unless that call is still queued)
  }
  if (eng->h_kf_bytes[turn] < bytes) {
    if (g_frozen) return fail(PLA_ERR_FROZEN, "the engine workspace is frozen and this call needs a larger k-fold table");
    if (eng->h_kf[turn]) (void)hipHostFree(eng->h_kf[turn]);
    eng->h_kf[turn] = nullptr;
    eng->h_kf_bytes[turn] = 0;
    PLA_HIP(hipHostMalloc(&eng->h_kf[turn], bytes, hipHostMallocDefault));
    eng->h_kf_bytes[turn] = bytes;
  }
  pla::KfoldSource* tab = (pla::KfoldSource*)eng->h_kf[turn];
  unsigned routes = 0;
  for (int64_t k = 0; k < n_sources; ++k) {
    // (a source without rows has no tasks: its entry only has to be harmless)
    const int route = pla::kfold_route(src_base[k], dtype, src_stride_row[k], src_stride_draw[k], src_draws[k]);
    tab[k] = pla::KfoldSource{src_base[k], src_rows[k], src_stride_row[k], src_stride_draw[k], (int)src_draws[k],
                              route | ((k == 0 && nan_flag) ? pla::kKfoldNanFlag : 0)};
    if (src_rows[k] > 0) routes |= 1u << route;
  }
  PLA_HIP(hipMemcpyAsync(eng->d_kf.p, tab, bytes, hipMemcpyHostToDevice, s));
  PLA_HIP(hipEventRecord(eng->kf_event[turn], s));
  pla::KfoldParams p{eng->d_kf.as<const pla::KfoldSource>(), (int)n_sources, source_offsets, task_row, task_out, n_tasks, out, n_out,
                     (unsigned long long*)n_replaced};
  int launches = 0;
  {
    TimedLaunch t(eng, s);  // (the ragged pass alone: pla_engine_kernel_ms)
    PLA_HIP(pla::launch_kfold_lme(p, dtype, routes, s, &launches));
  }
  std::string label;
  for (int r = 0; r < 3; ++r)
    if (routes & (1u << r)) label += std::string(label.empty() ? "" : " + ") + pla::kfold_route_name(r) + "<" + pla::dtype_name(dtype) + ">";
  // (the count is of the launches made, not of the routes asked for)
  eng->kf_label = label + " (matrices read in place; " + std::to_string(launches) + (launches == 1 ? " launch)" : " launches)");
  eng->last_kernels = eng->kf_label;
  return PLA_OK;
}

int pla_kfold_reduce(pla_engine* eng, const double* elpd, const double* lpd_full, int64_t n_obs, double scale, const int64_t* n_replaced,
                     int mem_space, void* stream, double* p_i, double* kfold_i, double* agg) {
  if (!eng) return fail(PLA_ERR_ARG, "engine is NULL");
  if (mem_space != PLA_HOST && mem_space != PLA_DEVICE) return fail(PLA_ERR_ARG, "bad mem_space");
  if (mem_space == PLA_HOST) return fail(PLA_ERR_UNSUPPORTED, "pla_kfold_reduce reads device memory only");
  if (n_obs < 1 || n_obs >= ((int64_t)1 << 40)) return fail(PLA_ERR_ARG, "n_obs must lie in [1, 2^40), got %lld", (long long)n_obs);
  if (!elpd || !lpd_full || !agg) return fail(PLA_ERR_ARG, "elpd, lpd_full or agg is NULL");
  PLA_ENGINE_CALL(eng, stream);
  int rc = eng->d_cmp.reserve((size_t)pla::kfold_n_tiles(n_obs) * 4 * sizeof(double));
  if (rc) return rc;
  {
    TimedLaunch t(eng, s);
    PLA_HIP(pla::launch_kfold_reduce(elpd, lpd_full, n_obs, scale, p_i, kfold_i, eng->d_cmp.as<double>(),
                                     (const unsigned long long*)n_replaced, agg, eng->compare_grid, s));
  }
  // (behind pla_kfold_lme the text keeps the routes of the ragged pass)
  const std::string finish = "kfold_tiles_kernel<0> + kfold_tiles_kernel<1> + kfold_final_kernel";
  eng->last_kernels = eng->kf_label.empty() ? finish : eng->kf_label + ", then " + finish;
  eng->kf_label.clear();
  return PLA_OK;
}

}  // extern "C"
