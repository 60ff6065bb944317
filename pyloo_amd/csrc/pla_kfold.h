// K-fold cross-validation kernels (reference: pyloo loo_kfold.py:250-299, 643-692).
//
// 1. The ragged log-mean-exp.  Several resident matrices ("sources": source 0 the full fit, sources 1..K the fold fits, each with
//    its own number of draws, strides and base pointer, one dtype for all) and ONE task list grouped by source in CSR form:
//    tasks [source_offsets[k], source_offsets[k + 1]) belong to source k.  Task t of source k writes
//        out[task_out[t]] = logsumexp_s(ll_k[task_row[t], :]) - log(S_k)
//    computed as utils.py:344-357 does (max, sum exp(x - max), log, + max - log S), f32 widened on load and reduced in f64.
//    Nothing is replaced -- a NaN anywhere in a row, a row of -inf, a +inf give NaN, as that expression does in NumPy -- except
//    in a source that carries kKfoldNanFlag (the full fit, loo_kfold.py:250-259): its NaN entries count as -1e10 and are
//    counted in `replaced` (one atomicAdd per wave after a wave reduction).
//
//    Three kernels, one per ROUTE; the launcher (pla_k_kfold.hip) gives every source its route and launches a kernel only when
//    some source takes it, so the number of launches does not depend on K.  Every kernel walks the whole task list and leaves
//    the tasks of the other routes alone; the route is uniform within a wave (lane route: within each step of a wave).
//      kfold_wave_kernel   unit draw stride, 16-byte aligned rows, S_k <= 4096: one wavefront per task, the row in its registers
//                          (pla_wave.h's row loads and padding) -- one HBM read, max, then sum; the next task's row streams into
//                          the registers the second pass has consumed, as in waic_wave_kernel.  The S_k % (16 / sizeof T)
//                          draws behind the last whole 16-byte vector travel in one more register of lanes 0 ...
//      kfold_lane_kernel   unit ROW stride (observations fastest: an (S, n) buffer seen as .T): a wave takes 64 consecutive
//                          tasks, one per lane, and every lane streams down its own column with a running maximum and a
//                          rescaled sum.  Consecutive rows (compact form, contiguous folds) are neighbouring elements; with
//                          scattered folds in the full form every lane touches a line of its own.  A wave
//                          whose 64 tasks straddle sources takes them source by source.
//      kfold_block_kernel  any other stride or length: one workgroup per task, two strided passes over the (L2-resident) row.
//    A lane's / wave's / workgroup's result depends on the row's values alone: the same row gives the same bits wherever it lies.
//    Rows and outputs are bounds-checked on the device (task_row clamped into the source, stores outside [0, n_out) dropped).
//
// 2. The finishing pass over elpd[N] (held-out) and lpd_full[N]: p_i = lpd_full_i - elpd_i, kfold_i = scale * elpd_i, and into
//    agg (slots of pla_psis_loo reused, see include/pyloo_amd.h): N, sum kfold_i, M2 of kfold_i, sum p_i, M2 of p_i -- the M2
//    two-pass about the mean, as np.var -- and the replaced-NaN count.  N is cut into tiles whose width depends on N alone
//    (kfold_tile_cols, the comparison kernels' rule); a workgroup reduces a tile in a fixed order, every tile's partial has a
//    slot of its own, and the slots are combined in a fixed order (kfold_combine): the aggregates do not change bits with the grid.
#pragma once

#include "../../include/pyloo_amd.h"
#include "pla_kernels.h"
#include "pla_wave.h"

namespace pla {

// the source of task t (t < n_tasks): the last k with source_offsets[k] <= t.  (k, end) is the caller's cursor: the source of its
// previous task and where that source ends.  Offsets that do not ascend cannot send the search outside the table.
__device__ __forceinline__ void kfold_seek(const KfoldParams& P, int64_t t, int& k, int64_t& end) {
  if (t < end) return;
  int lo = k, hi = P.n_sources - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (P.source_offsets[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  k = lo;
  end = k + 1 < P.n_sources ? P.source_offsets[k + 1] : P.n_tasks;
  if (end <= t) end = t + 1;
}

// a source's tasks are this kernel's (a source without rows has none to read)
__device__ __forceinline__ bool kfold_takes(const KfoldSource& s, int route) {
  return (s.flags & kKfoldRouteMask) == route && s.n_rows > 0;
}
__device__ __forceinline__ int64_t kfold_row(const KfoldParams& P, const KfoldSource& s, int64_t t) {
  int64_t r = P.task_row[t];
  r = r < 0 ? 0 : r;
  return r < s.n_rows ? r : s.n_rows - 1;
}
__device__ __forceinline__ void kfold_store(const KfoldParams& P, int64_t t, double v) {
  const int64_t o = P.task_out[t];
  if (o >= 0 && o < P.n_out) P.out[o] = v;
}
__device__ __forceinline__ void kfold_count(const KfoldParams& P, unsigned nrep) {
  if (!P.replaced) return;
  const unsigned tot = (unsigned)wave_reduce<OpSum>((double)nrep);
  if (wave_lane() == 0 && tot) atomicAdd(P.replaced, (unsigned long long)tot);
}

template <typename T>
__device__ __forceinline__ T kfold_lane_bcast(T v, int lane);
template <>
__device__ __forceinline__ double kfold_lane_bcast<double>(double v, int lane) { return lane_value(v, lane); }
template <>
__device__ __forceinline__ float kfold_lane_bcast<float>(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// every slot past the row's whole vectors := padv (pad_tail leaves vector 0 alone: rows shorter than 64 vectors pad it here)
template <typename T, int VEC>
__device__ __forceinline__ void kfold_pad(T (&v)[kWaveSlots], int qfull, int qrem, T padv) {
  constexpr int NQ = kWaveSlots / VEC;
  // (every call works its lane masks out afresh: shared between the calls of one row they stay live across its passes -- 31 of
  // them for an f64 row -- and spill)
  asm volatile("" : "+s"(qfull), "+s"(qrem));
  pad_tail<T, VEC, NQ - 1, true>(v, qfull, qrem, padv);
  if (qfull == 0) {
    const bool ok = wave_lane() < qrem;
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = ok ? v[e] : padv;
  }
}

// ---- wave route ---------------------------------------------------------------------------------------------------------------
template <typename T>
struct KfoldWaveTask {  // wave-uniform description of one task
  const T* rp;   // its row; null: not a task of this route
  int S;
  int flags;
  T extra;       // lane l < S % VEC: draw (S / VEC) * VEC + l (loaded with the description)
};

template <typename T, int VEC>
__device__ __forceinline__ KfoldWaveTask<T> kfold_wave_task(const KfoldParams& P, int64_t t, int& k, int64_t& end) {
  KfoldWaveTask<T> w{nullptr, 0, 0, (T)0};
  if (t >= P.n_tasks) return w;
  kfold_seek(P, t, k, end);
  const KfoldSource s = P.src[k];
  if (!kfold_takes(s, kKfoldWave)) return w;
  w.rp = reinterpret_cast<const T*>(s.base) + kfold_row(P, s, t) * s.stride_row;
  w.S = s.n_draws;
  w.flags = s.flags;
  const int whole = w.S / VEC * VEC, rem = w.S - whole;
  if (rem > 0) w.extra = w.rp[whole + (wave_lane() < rem ? wave_lane() : 0)];
  return w;
}

template <typename T, int VEC>
__global__ __launch_bounds__(kWave * kWavesPerBlock, 2) void kfold_wave_kernel(KfoldParams P) {
  __shared__ __attribute__((aligned(16))) double tab[2 * kTabN];
  __shared__ __attribute__((aligned(16))) double lt[2 * kLogTabN];
  constexpr int EPT = kWaveSlots, NQ = EPT / VEC;
  const int tid = threadIdx.x;
  for (int j = tid; j < kTabN; j += kWave * kWavesPerBlock) exp_table_entry(tab, j);
  for (int j = tid; j < kLogTabN; j += kWave * kWavesPerBlock) log_table_entry(lt, j);
  __syncthreads();
  const int lane = wave_lane();
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t w0 = (int64_t)blockIdx.x * kWavesPerBlock + wv, nw = (int64_t)gridDim.x * kWavesPerBlock;
  const T ninf = (T)(-pinf());
  int k = 0;
  int64_t end = 0;
  T v[kWaveSlots];
  // the wave's tasks of this route, w0, w0 + nw, ... (the others are stepped over): the first row is loaded here, every later
  // one streams in behind the second pass of the row before it
  const auto next_task = [&](int64_t& t) {
    KfoldWaveTask<T> w = kfold_wave_task<T, VEC>(P, t, k, end);
    while (!w.rp && t < P.n_tasks) {
      t += nw;
      w = kfold_wave_task<T, VEC>(P, t, k, end);
    }
    return w;
  };
  int64_t t = w0;
  KfoldWaveTask<T> cur = next_task(t);
  if (cur.rp) issue_row_loads<T, VEC>(v, cur.rp, cur.S / VEC * VEC);
  unsigned nrep = 0;
  while (cur.rp) {
    int64_t tn = t + nw;
    const KfoldWaveTask<T> next = next_task(tn);
    const __amdgpu_buffer_rsrc_t rs_next = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(next.rp ? next.rp : cur.rp), 0, next.rp ? next.S / VEC * VEC * (int)sizeof(T) : 0, 0x00020000);
    const int S = __builtin_amdgcn_readfirstlane(cur.S);
    const int nvec = S / VEC, rem = S - nvec * VEC;
    const int qfull = nvec / kWave, qrem = nvec - qfull * kWave;
    // ---- pass 1: the maximum, and whether every draw is finite.  Slots past the row hold draw 0 for it (harmless for both).
    T extra = cur.extra;
    const T x0 = nvec > 0 ? kfold_lane_bcast<T>(v[0], 0) : kfold_lane_bcast<T>(extra, 0);
    kfold_pad<T, VEC>(v, qfull, qrem, x0);
    extra = lane < rem ? extra : x0;
    T mx[2] = {extra, extra}, z[2] = {extra * (T)0, (T)0};  // z: 0 * x summed -- NaN as soon as one draw is NaN or infinite
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      mx[i & 1] = vmax_nc<false>(v[i], mx[i & 1]);
      z[i & 1] = fma_t(v[i], (T)0, z[i & 1]);
    }
    double m = wave_all<R_MAX>((double)vmax_nc<false>(mx[0], mx[1]));
    const double zz = wave_all<R_SUM>((double)(z[0] + z[1]));
    bool bad = false;
    int n_fixed = 0;  // NaN draws of the row that count as -1e10 (wave-uniform)
    if (zz != zz) {
      // rare: classify.  NaN entries of a flagged source become -1e10 and are counted (real draws only); a NaN that stays, a
      // +inf or a row of -inf make the result NaN (utils.py:346-357 on such a row)
      // (count_if: compare and add as one statement -- left to the compiler, the 65 masks are collected in scalar registers
      // first and spill)
      const bool fix = (cur.flags & kKfoldNanFlag) != 0;
      kfold_pad<T, VEC>(v, qfull, qrem, ninf);  // (the slots past the row: no NaN to count there)
      extra = lane < rem ? extra : ninf;
      int ok = 0;  // draws of this lane that are not NaN
#pragma unroll
      for (int i = 0; i < EPT; ++i) count_if<true>(ok, v[i], v[i]);
      count_if<true>(ok, extra, extra);
      int nn = EPT + 1 - ok;
      if (fix) {
        // the NaN draws leave the registers as -inf (v_max drops a quiet NaN and quiets a signalling one: twice) and come back
        // as n_fixed draws of -1e10 below
        nrep += (unsigned)nn;
        n_fixed = wave_sum_int(nn);
        nn = 0;
#pragma unroll
        for (int i = 0; i < EPT; ++i) v[i] = vmax_nc<false>(vmax_nc<false>(v[i], ninf), ninf);
        extra = vmax_nc<false>(vmax_nc<false>(extra, ninf), ninf);
      }
      T mq[2] = {extra, ninf};  // (v_max drops a NaN)
#pragma unroll
      for (int i = 0; i < EPT; ++i) mq[i & 1] = vmax_nc<false>(v[i], mq[i & 1]);
      m = wave_all<R_MAX>((double)vmax_nc<false>(mq[0], mq[1]));
      if (n_fixed > 0) m = fmax(m, -1e10);
      bad = __ballot(nn > 0) != 0ull || m == pinf() || m == -pinf();
    }
    // ---- pass 2: sum exp(x - m); the slots past the row hold -inf now (e^-700 each: nothing).  The next row streams in behind it.
    kfold_pad<T, VEC>(v, qfull, qrem, ninf);
    extra = lane < rem ? extra : ninf;
    double se = exp_tab(fmax((double)extra - m, -700.0), tab);
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      se += exp_tab(fmax((double)v[i] - m, -700.0), tab);
      if ((i % VEC) == VEC - 1) issue_row_vector<T, VEC>(v, rs_next, i / VEC);
    }
    se = wave_all<R_SUM>(se);
    if (n_fixed > 0) se += (double)n_fixed * exp_tab(fmax(-1e10 - m, -700.0), tab);
    const double res = bad ? qnan() : (log_tab(se, lt) + m) - log((double)S);  // utils.py:352-357
    if (lane == 0) kfold_store(P, t, res);
    cur = next;
    t = tn;
  }
  kfold_count(P, nrep);
}

// ---- lane route ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void kfold_lane_kernel(KfoldParams P) {
  __shared__ __attribute__((aligned(16))) double tab[2 * kTabN];
  __shared__ __attribute__((aligned(16))) double lt[2 * kLogTabN];
  for (int j = threadIdx.x; j < kTabN; j += 256) exp_table_entry(tab, j);
  for (int j = threadIdx.x; j < kLogTabN; j += 256) log_table_entry(lt, j);
  __syncthreads();
  constexpr int U = 8;
  const int lane = wave_lane();
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int64_t nw = (int64_t)gridDim.x * 4;
  unsigned nrep = 0;
  int k = 0;
  int64_t end = 0;
  for (int64_t t0 = ((int64_t)blockIdx.x * 4 + wv) * kWave; t0 < P.n_tasks; t0 += nw * kWave) {
    const int64_t t1 = t0 + kWave < P.n_tasks ? t0 + kWave : P.n_tasks;
    const int64_t t = t0 + lane;
    for (int64_t tt = t0; tt < t1;) {  // the sources this wave's 64 tasks belong to, one after the other
      kfold_seek(P, tt, k, end);
      const int64_t te = end < t1 ? end : t1;
      const KfoldSource s = P.src[k];
      if (kfold_takes(s, kKfoldLane)) {
        const bool live = t >= tt && t < te;
        const bool fix = (s.flags & kKfoldNanFlag) != 0;
        const int S = s.n_draws;
        const int64_t ld = s.stride_draw;
        const T* col = reinterpret_cast<const T*>(s.base) + kfold_row(P, s, live ? t : tt) * s.stride_row;
        double m = -pinf(), se = 0.0;  // running maximum, sum of exp(x - m)
        unsigned nnan = 0;  // NaN entries of this lane's column
        T ring[2][U];
        const auto fetch = [&](T (&dst)[U], const int s0) {  // (draws past the row: its last draw again, never looked at)
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int d = s0 + u < S ? s0 + u : S - 1;
            dst[u] = __builtin_nontemporal_load(col + (int64_t)d * ld);
          }
        };
        const auto take = [&](const T (&src)[U], const int nb) {
          double x[U];
          double bm = -pinf();
#pragma unroll
          for (int u = 0; u < U; ++u) {
            x[u] = (double)src[u];
            if (u < nb) {
              const bool isn = x[u] != x[u];
              nnan += isn ? 1u : 0u;
              x[u] = (isn && fix) ? -1e10 : x[u];
              bm = x[u] > bm ? x[u] : bm;  // (a NaN never compares above)
            }
          }
          if (bm > m) {  // this lane has a new maximum: rescale what it has summed so far
            se *= exp_tab(fmax(m - bm, -700.0), tab);
            m = bm;
          }
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (u < nb) se += exp_tab(fmax(x[u] - m, -700.0), tab);  // (NaN - m: fmax drops it, the result is NaN below)
        };
        fetch(ring[0], 0);
        int s0 = 0;
#pragma unroll 1
        for (; s0 + 2 * U <= S; s0 += 2 * U) {  // two batches in flight: the loads of the batch after next behind each conversion
          fetch(ring[1], s0 + U);
          take(ring[0], U);
          fetch(ring[0], s0 + 2 * U);
          take(ring[1], U);
        }
        if (s0 < S) {
          const int nb = S - s0 < U ? S - s0 : U;
          if (S - s0 > U) fetch(ring[1], s0 + U);
          take(ring[0], nb);
          if (S - s0 > U) take(ring[1], S - s0 - U);
        }
        nrep += (fix && live) ? nnan : 0u;
        const bool bad = (!fix && nnan > 0) || m == pinf() || m == -pinf();
        const double res = bad ? qnan() : (log_tab(se, lt) + m) - log((double)S);  // utils.py:352-357
        if (live) kfold_store(P, t, res);
      }
      tt = te;
    }
  }
  kfold_count(P, nrep);
}

// ---- block route --------------------------------------------------------------------------------------------------------------
template <typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void kfold_block_kernel(KfoldParams P) {
  __shared__ double red[16];
  const int tid = threadIdx.x;
  unsigned nrep = 0;
  int k = 0;
  int64_t end = 0;
  for (int64_t t = blockIdx.x; t < P.n_tasks; t += gridDim.x) {
    kfold_seek(P, t, k, end);
    const KfoldSource s = P.src[k];
    if (!kfold_takes(s, kKfoldBlock)) continue;
    const bool fix = (s.flags & kKfoldNanFlag) != 0;
    const int S = s.n_draws;
    const T* rp = reinterpret_cast<const T*>(s.base) + kfold_row(P, s, t) * s.stride_row;
    // (plain max / exp / log: a NaN, a +inf or a row of -inf come out as NaN by the arithmetic itself, as in NumPy)
    double mx = -pinf();
    for (int d = tid; d < S; d += BLOCK) {
      double x = (double)rp[(int64_t)d * s.stride_draw];
      if (fix && x != x) {
        x = -1e10;
        ++nrep;
      }
      mx = fmax(mx, x);
    }
    const double m = block_reduce<OpMax, BLOCK>(mx, red);
    double se = 0.0;
    for (int d = tid; d < S; d += BLOCK) {
      double x = (double)rp[(int64_t)d * s.stride_draw];
      if (fix && x != x) x = -1e10;
      se += exp(x - m);
    }
    se = block_reduce<OpSum, BLOCK>(se, red);
    if (tid == 0) kfold_store(P, t, (log(se) + m) - log((double)S));
  }
  kfold_count(P, nrep);
}

// ---- finishing pass -----------------------------------------------------------------------------------------------------------
constexpr int64_t kKfoldMinTile = 1024, kKfoldMaxTiles = 2048;
constexpr int kKfoldThreads = 256;

// tile width for N observations: max(kKfoldMinTile, ceil(N / kKfoldMaxTiles) rounded up to 256) -- pla_compare.h's rule
__host__ __device__ inline int64_t kfold_tile_cols(int64_t n) {
  int64_t t = (n + kKfoldMaxTiles - 1) / kKfoldMaxTiles;
  t = (t + 255) / 256 * 256;
  return t < kKfoldMinTile ? kKfoldMinTile : t;
}

struct KfoldReduceParams {
  const double* elpd;      // [N] held-out log predictive densities
  const double* lpd_full;  // [N] the same under the full fit
  int64_t N;
  double scale;
  double* p_i;      // [N] or null
  double* kfold_i;  // [N] or null
  double* part;     // [n_tiles][4]: sum kfold, sum p, M2 kfold, M2 p
  int64_t tile_cols, n_tiles;
  const unsigned long long* replaced;  // may be null
  double* agg;  // [PLA_AGG_COUNT]
};

// a workgroup's sum in a fixed order: the lanes of a wave by an xor butterfly, the waves in wave order
__device__ __forceinline__ double kfold_block_sum(double v, double* lds) {
  v = wave_reduce<OpSum>(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = lds[0];
  for (int w = 1; w < kKfoldThreads / 64; ++w) r += lds[w];
  return r;
}
// the tiles' partials of one column of `part` in a fixed order: thread j adds tiles j, j + 256, ... ascending, then the workgroup
__device__ __forceinline__ double kfold_combine(const double* part, int64_t n_tiles, int col, double* lds) {
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n_tiles; i += kKfoldThreads) a += part[4 * i + col];
  return kfold_block_sum(a, lds);
}

// PASS 0: pointwise outputs and the tiles' sums; PASS 1: the tiles' sums of squared deviations about the means of pass 0
template <int PASS>
__global__ __launch_bounds__(kKfoldThreads) void kfold_tiles_kernel(KfoldReduceParams P) {
  __shared__ double lds[kKfoldThreads / 64];
  double mean_k = 0.0, mean_p = 0.0;
  if constexpr (PASS == 1) {
    mean_k = kfold_combine(P.part, P.n_tiles, 0, lds) / (double)P.N;
    mean_p = kfold_combine(P.part, P.n_tiles, 1, lds) / (double)P.N;
  }
  for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
    const int64_t c0 = tile * P.tile_cols;
    const int64_t c1 = c0 + P.tile_cols < P.N ? c0 + P.tile_cols : P.N;
    double a = 0.0, b = 0.0;
    for (int64_t i = c0 + threadIdx.x; i < c1; i += kKfoldThreads) {
      const double e = P.elpd[i];
      const double p = P.lpd_full[i] - e, kf = P.scale * e;
      if constexpr (PASS == 0) {
        if (P.p_i) P.p_i[i] = p;
        if (P.kfold_i) P.kfold_i[i] = kf;
        a += kf;
        b += p;
      } else {
        a += (kf - mean_k) * (kf - mean_k);
        b += (p - mean_p) * (p - mean_p);
      }
    }
    a = kfold_block_sum(a, lds);
    b = kfold_block_sum(b, lds);
    if (threadIdx.x == 0) {
      P.part[4 * tile + 2 * PASS] = a;
      P.part[4 * tile + 2 * PASS + 1] = b;
    }
  }
}

__global__ __launch_bounds__(kKfoldThreads) void kfold_final_kernel(KfoldReduceParams P) {
  __shared__ double lds[kKfoldThreads / 64];
  double r[4];
  for (int c = 0; c < 4; ++c) r[c] = kfold_combine(P.part, P.n_tiles, c, lds);
  if (threadIdx.x == 0) {
    P.agg[PLA_AGG_N] = (double)P.N;
    P.agg[PLA_AGG_SUM_LOO] = r[0];    // sum kfold_i
    P.agg[PLA_AGG_M2_LOO] = r[2];     // M2 of kfold_i
    P.agg[PLA_AGG_SUM_LPPD] = r[1];   // sum p_i
    P.agg[PLA_AGG_N_HIGH] = r[3];     // M2 of p_i (the slot is reused: include/pyloo_amd.h)
    P.agg[PLA_AGG_N_NONFINITE] = P.replaced ? (double)*P.replaced : 0.0;  // NaN entries of the full fit taken as -1e10
    P.agg[PLA_AGG_MIN_DIAG] = 0.0;
    P.agg[PLA_AGG_N_SLOW] = 0.0;
  }
}

}  // namespace pla
