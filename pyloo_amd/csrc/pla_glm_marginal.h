// Cluster-marginal log-likelihood of a multilevel GLM: the effect u of the left-out cluster integrated out by quadrature.
//     eta[i, s] = rest[i, s] + z_i u,   u | draw s ~ N(0, tau_s^2)
//     e[q]      = ( logw[c, q] + ( (-0.5 log 2 pi - log tau_s) - 0.5 (node[c, q] / tau_s)^2 ) )
//                 + sum_{i in c, in member order} ll(y_i | rest[i, s] + z_i node[c, q])
//     mll[c, s] = max_q e[q] + log sum_q exp(e[q] - max_q e[q])            (-inf if every e[q] is -inf)
// rest is a block of the linear predictor as the generator of pla_glm.h / pla_glm_terms.h wrote it (PLA_GLM_LINPRED with the member
// list as its row list); ll is glm_density of pla_glm.h.  The product z_i node and every sum are rounded once (fp contract(off));
// with z null the product is not formed.  All arithmetic is f64.
//
// SEGMENTS.  Segment k of a cluster is its members [k L, (k + 1) L), L = kGlmMargSeg.  A segment sum starts from zero and runs in
// member order; the sums of a cluster's segments are added in order of k, starting from the sum of segment 0.  The host cuts the
// member list into blocks at segment boundaries and hands each block a table of its segments (GlmMargSeg) and of the clusters of
// more than one segment that it continues or closes (GlmMargJoin); the kernels trust the tables (the host builds them from offsets
// it has clamped) and clamp every member into [0, n_src) on load.
//
// SEGMENT KERNEL.  glm_marginal_kernel<FAM, CAP>: one lane per draw, a wavefront takes 64 consecutive draws of one segment -- a row
// of rest is a 512-byte coalesced read; y, z, trials, obs_const of the row and the cluster's nodes are wave-uniform.  The running
// sums of up to CAP nodes live in registers (CAP = 8, 16, 32, fully unrolled; a node past n_nodes repeats the last one with the log-weight -inf).
// A cluster of one segment (or none: an empty cluster) is finished in place -- prior, log-weight and the log-sum-exp over q in the
// lane; a segment of a longer cluster stores its (n_nodes, S) sums into its slot of the workspace.
// JOIN KERNEL.  glm_marginal_join_kernel<CAP>: per cluster of several segments, the slots added in order of k (onto the carry when
// the cluster began in an earlier block), then the finish above, or the carry for the next block.  At most one cluster is open
// across a block boundary, so there is one carry.
//
// mll[c, s] depends on the rest values of the cluster's members in member order, those members' entries of the vectors, row c of
// nodes and log_weights, tau_s and L -- not on the grid, the block size, the place of the cluster in the list, its label, the
// position of the draw or the memory space.  No LDS, no scratch, no floating-point atomics.
#pragma once

#include "pla_kernels.h"

namespace pla {

constexpr int kGlmMargSeg = 128;    // L: members per segment
constexpr int kGlmMargMaxNodes = 32;

struct GlmMargSeg {  // one segment of a block
  int64_t cluster;
  int64_t first;  // its first member, as a row of the block (0 <= first, first + len <= n_rows)
  int32_t len;    // 0 .. kGlmMargSeg
  int32_t slot;   // < 0: the cluster's only segment, finished by the segment kernel; else the workspace slot of its sums
};

struct GlmMargJoin {  // one cluster of several segments, as far as a block holds it
  int64_t cluster;
  int32_t slot0, n_slots;  // its segments of this block, in order of k
  int32_t carry_in;        // it began in an earlier block: the sums so far are in the carry
  int32_t finish;          // its last segment is here: mll is written; else the carry
};

struct GlmMargParams {
  const double* rest;  // (n_rows, n_draws), pitch n_draws: the block of the linear predictor
  int64_t n_rows;
  const int64_t* members;  // [n_rows] source rows of the block's rows
  int64_t n_src;
  const double *y, *z, *trials, *obs_const;  // [n_src]; the last three may be null
  const double *sigma, *draw_const;          // [n_draws], PLA_GLM_GAUSSIAN
  const double* tau;                         // [n_draws]
  const double *nodes, *logw;                // [n_clusters][n_nodes]
  int n_nodes, n_draws, n_strips;
  const GlmMargSeg* segs;
  int64_t n_segs;
  const GlmMargJoin* joins;
  int64_t n_joins;
  double* part;   // [slot][CAP][n_draws]
  double* carry;  // [CAP][n_draws]
  double* out;    // row (cluster - out_first) with pitch out_pitch
  int64_t out_first, out_pitch;
  unsigned long long* replaced;  // non-null: NaN -> -1e10, counted here
};

// node capacity of the kernels for n_nodes (8, 16 or 32), the segment kernel on one block, then the join kernel when the block has
// clusters of several segments (pla_k_glm_marginal.hip); route: text for pla_engine_last_kernels
int glm_marginal_capacity(int n_nodes);
hipError_t launch_glm_marginal(int family, const GlmMargParams& p, hipStream_t stream, char* route, int cap);

}  // namespace pla

#ifdef PLA_GLM_MARGINAL_KERNELS  // (pla_k_glm_marginal.hip; the host unit takes the structures above)
#include "pla_glm.h"

namespace pla {

// The arguments that a unit needs once, before or behind its loop over the rows, are read from the kernel-argument segment where they
// are needed -- held in scalar registers across that loop, beside its lane masks, they spill into vector lanes.  The pointer is
// opaque, so the loads stay where they are written; a pointer read this way is cast to the global address space by hand.
typedef const __attribute__((address_space(4))) GlmMargParams* GlmMargArgs;
__device__ __forceinline__ GlmMargArgs glm_marg_args() {
  GlmMargArgs a = (GlmMargArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return a;
}
typedef const __attribute__((address_space(1))) double* GlmMargIn;
typedef __attribute__((address_space(1))) double* GlmMargOut;

// node q of a cluster's row, q >= n_nodes read as the last node: the index is formed inside the loop from an opaque q (a compare
// per node is loop-invariant: hoisted out of the loop over the rows, 32 of them spill the scalar registers into vector lanes)
__device__ __forceinline__ double glm_marg_node(const double* row, int q, int n_nodes) {
  // (the chains of the nodes are scheduled four at a time: 32 side by side hold more lane masks than there are scalar registers)
  if ((q & 3) == 0) __builtin_amdgcn_sched_barrier(0);
  asm volatile("" : "+s"(q));
  return row[q < n_nodes ? q : n_nodes - 1];
}

// prior, log-weight and log-sum-exp over the nodes of one lane; a node past n_nodes has the log-weight -inf: its term is exp(-inf) = 0
template <int CAP>
__device__ __forceinline__ double glm_marg_finish(const double (&sum)[CAP], int n_nodes, const double* nodes, GlmMargIn logw, double tau) {
#pragma clang fp contract(off)
  const double lt = -0.91893853320467274178 - log(tau);
  double e[CAP];
  double m = -INFINITY;
  bool any_nan = false;
#pragma unroll
  for (int q = 0; q < CAP; ++q) {
    const double t = glm_marg_node(nodes, q, n_nodes) / tau;
    const double prior = lt - 0.5 * (t * t);
    int qq = q;
    asm volatile("" : "+s"(qq));  // (as in glm_marg_node: the compare stays here)
    const double lw = qq < n_nodes ? logw[qq] : -INFINITY;
    e[q] = (lw + prior) + sum[q];
    m = fmax(m, e[q]);
    any_nan |= e[q] != e[q];
  }
  if (m == -INFINITY) return any_nan ? (double)NAN : m;  // (fmax passes over a NaN: with nothing else above -inf it is the answer)
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < CAP; ++q) {
    if ((q & 3) == 0) __builtin_amdgcn_sched_barrier(0);
    acc = acc + exp(e[q] - m);
  }
  return m + log(acc);
}

__device__ __forceinline__ void glm_marg_count(unsigned long long n_nan, int lane) {
  unsigned long long* replaced = glm_marg_args()->replaced;
  if (replaced) {  // (an integer count: the order of the additions does not matter)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_nan += __shfl_xor(n_nan, d);
    if (lane == 0 && n_nan) atomicAdd(replaced, n_nan);
  }
}

// the end of a cluster: prior, log-weight, log-sum-exp, the NaN rule, the store
template <int CAP>
__device__ __forceinline__ void glm_marg_store(const double (&sum)[CAP], int n_nodes, const double* nodes, int64_t cluster, int s, bool s_ok,
                                               int sc, unsigned long long* n_nan) {
  const GlmMargArgs A = glm_marg_args();
  double v = glm_marg_finish<CAP>(sum, n_nodes, nodes, (GlmMargIn)A->logw + cluster * (int64_t)n_nodes, ((GlmMargIn)A->tau)[sc]);
  if (s_ok) {
    if (A->replaced && v != v) {
      v = -1e10;
      *n_nan += 1;
    }
    ((GlmMargOut)A->out)[(cluster - A->out_first) * A->out_pitch + s] = v;
  }
}

template <int FAM, int CAP>
__global__ __launch_bounds__(kWave * kGlmWaves) void glm_marginal_kernel(GlmMargParams P) {
  const int S = P.n_draws, Q = P.n_nodes;
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int64_t n_units = P.n_segs * P.n_strips;
  const int64_t nw = (int64_t)gridDim.x * kGlmWaves;
  unsigned long long n_nan = 0;
  for (int64_t u = (int64_t)blockIdx.x * kGlmWaves + wv; u < n_units; u += nw) {
    const int64_t sg = u / P.n_strips;
    const int st = (int)(u - sg * P.n_strips);
    const GlmMargSeg seg = P.segs[sg];
    const int s = st * kWave + lane;
    const bool s_ok = s < S;
    const int sc = s_ok ? s : S - 1;
    double sig = 1.0, dc = 0.0;
    if constexpr (FAM == PLA_GLM_GAUSSIAN) {
      const GlmMargArgs A = glm_marg_args();
      sig = ((GlmMargIn)A->sigma)[sc];
      dc = ((GlmMargIn)A->draw_const)[sc];
    }
    const double* nd = P.nodes + seg.cluster * (int64_t)Q;
    double sum[CAP];
#pragma unroll
    for (int q = 0; q < CAP; ++q) sum[q] = 0.0;
    const double* rp = P.rest + seg.first * (int64_t)S + sc;
#pragma unroll 1
    for (int j = 0; j < seg.len; ++j) {
      // (the row's pointers come from the argument segment row by row: what the loop holds in scalar registers besides its lane
      // masks and the coefficients of exp and log1p spills)
      const GlmMargArgs R = glm_marg_args();
      typedef const __attribute__((address_space(1))) int64_t* Members;
      const GlmMargIn zp = (GlmMargIn)R->z, tp = (GlmMargIn)R->trials, cp = (GlmMargIn)R->obs_const;
      const int64_t v = ((Members)R->members)[seg.first + j], n_src = R->n_src;
      const int64_t src = v < 0 ? 0 : v < n_src ? v : n_src - 1;
      const double yv = ((GlmMargIn)R->y)[src];
      const double tv = FAM == PLA_GLM_BINOMIAL_LOGIT && tp ? tp[src] : 1.0;
      const double cv = (FAM == PLA_GLM_BINOMIAL_LOGIT || FAM == PLA_GLM_POISSON_LOG) && cp ? cp[src] : 0.0;
      const double r = rp[(int64_t)j * S];
      // (the nodes are re-read per row, from cache: held across the loop, 32 of them leave no scalar registers for anything else)
      const double zv = zp ? zp[src] : 1.0;
#pragma unroll
      for (int q = 0; q < CAP; ++q) {
#pragma clang fp contract(off)
        const double nq = glm_marg_node(nd, q, Q);
        const double zn = zp ? zv * nq : nq;  // (z null: the product is not formed)
        const double eta = r + zn;
        sum[q] = sum[q] + glm_density<FAM>(eta, yv, tv, cv, sig, dc);
      }
    }
    if (seg.slot < 0) {
      glm_marg_store<CAP>(sum, Q, nd, seg.cluster, s, s_ok, sc, &n_nan);
    } else if (s_ok) {
      GlmMargOut pp = (GlmMargOut)glm_marg_args()->part + (int64_t)seg.slot * CAP * S + s;
#pragma unroll
      for (int q = 0; q < CAP; ++q) pp[(int64_t)q * S] = sum[q];
    }
  }
  glm_marg_count(n_nan, lane);
}

template <int CAP>
__global__ __launch_bounds__(kWave * kGlmWaves) void glm_marginal_join_kernel(GlmMargParams P) {
  const int S = P.n_draws, Q = P.n_nodes;
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int64_t n_units = P.n_joins * P.n_strips;
  const int64_t nw = (int64_t)gridDim.x * kGlmWaves;
  unsigned long long n_nan = 0;
  for (int64_t u = (int64_t)blockIdx.x * kGlmWaves + wv; u < n_units; u += nw) {
    const int64_t jn = u / P.n_strips;
    const int st = (int)(u - jn * P.n_strips);
    const GlmMargJoin J = P.joins[jn];
    const int s = st * kWave + lane;
    const bool s_ok = s < S;
    const int sc = s_ok ? s : S - 1;
    double sum[CAP];
    const double* first = J.carry_in ? P.carry + sc : P.part + (int64_t)J.slot0 * CAP * S + sc;
#pragma unroll
    for (int q = 0; q < CAP; ++q) sum[q] = first[(int64_t)q * S];
#pragma unroll 1
    for (int k = J.carry_in ? 0 : 1; k < J.n_slots; ++k) {
      const double* pp = P.part + (int64_t)(J.slot0 + k) * CAP * S + sc;
#pragma unroll
      for (int q = 0; q < CAP; ++q) {
#pragma clang fp contract(off)
        sum[q] = sum[q] + pp[(int64_t)q * S];
      }
    }
    if (J.finish) {
      glm_marg_store<CAP>(sum, Q, P.nodes + J.cluster * (int64_t)Q, J.cluster, s, s_ok, sc, &n_nan);
    } else if (s_ok) {
#pragma unroll
      for (int q = 0; q < CAP; ++q) P.carry[(int64_t)q * S + s] = sum[q];
    }
  }
  glm_marg_count(n_nan, lane);
}

}  // namespace pla

#endif  // PLA_GLM_MARGINAL_KERNELS
