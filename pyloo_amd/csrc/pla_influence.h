// LOO influence kernels: what leaving observation r out does to the posterior of P draw-wise quantities theta[s, j].  With lw the
// log weights of observation r (of any normalisation), m = max_s lw_s, e_s = exp(lw_s - m) (lw_s = -inf: weight 0, the draw
// contributes to nothing) and z_sj = (theta_sj - center_j) / scale_j (a division):
//     s1 = sum e_s,  s2 = sum e_s^2
//     shift[r, j] = (sum_s e_s z_sj) / s1                        standardised LOO mean shift of quantity j
//     m2[r, j]    = (sum_s e_s z_sj^2) / s1                      its second moment
//     kl[r]       = (sum_s e_s (lw_s - m)) / s1 - log(s1) + log(S)     KL of the weighted draws from the unweighted ones
//     ess_w[r]    = s1^2 / s2
// A row whose weights are all NaN or all -inf, a row with a NaN weight and a row with a +inf weight give NaN in all outputs (the
// rule of pla_diag.h).  All arithmetic is f64 (f32 weights are widened on load).
//
// PREPARE.  influence_prepare_kernel writes Z^T, draws fastest, once per call: zt[j * s_pad + s] = z_sj, zero for s >= n_draws
// (s_pad = n_draws rounded up to the K chunk kInfK) and for j >= n_quant (p_pad = n_quant rounded up to whole panels of NCT
// 16-column tiles).  theta is read with any positive strides, (S, P) or (P, S).
//
// INFLUENCE.  influence_kernel<T, MODE, NCT>: W (N x S) . Z (S x P) and W . Z^2 on v_mfma_f64_16x16x4f64, one wavefront per tile
// of 16 observations and a panel of NCT tiles of 16 quantities at a time (NCT = 1, 2, 4: up to 16, 32, and more quantities).
//   operands     lane l = (i = l & 15, q = l >> 4) gives A[i][k] and B[k][i] of the k-quarter q (pla_nonfactor.h:329-337).  A K chunk
//                is kInfK = 16 consecutive draws; quarter q owns draws 4q .. 4q + 3 of it and MFMA step t of the chunk multiplies
//                draw 4q + t of every quarter: a permutation of the draws that A and B share, in which a lane's operands of the four
//                steps are 32 consecutive bytes -- two 16-byte loads of lw (one for f32) and two of Z^T, and the four quarters of a
//                row together read one whole 128-byte line per chunk.
//   A            e = exp(lw - m): two sweeps per tile, the exact row maxima first (no online rescale), then the products.  Rows
//                past the block are clamped on load and masked on store; draws past S enter as lw = -inf, e = 0, against Z^T's
//                zero padding.
//   B            z from Z^T for the first accumulator, z * z formed in registers for the second.
//   VALU sums    s1, s2 and sum e (lw - m) accumulate in the lanes that hold e (per lane by chunk and draw), then two xor
//                butterflies over the four k-quarters; never contracted into fused multiply-adds.
//   panels       more than 16 NCT quantities run as panels with exp taken again per panel (the same exp of the same difference).
//   MODE         kInfVec: 16-byte loads (rows 16-byte aligned, n_draws a multiple of the vector); kInfElem: element loads with
//                the matrix's draw stride -- unaligned bases, odd pitches and observations-fastest views: correct, not fast.
// An observation's outputs depend on its own row, Z^T and S alone: not on the grid, the block of observations the row arrives in,
// its position inside a tile (a row's sums live in its own lanes; row i of the MFMA result is a function of row i of A), the
// position of a column inside a panel, or the load mode.  No floating-point atomics.
#pragma once

#include "pla_pit.h"

namespace pla {

constexpr int kInfK = 16;      // draws per K chunk: four MFMA steps, four consecutive draws per lane
constexpr int kInfTile = 16;   // observations / quantities per MFMA tile
constexpr int kInfWaves = 4;   // wavefronts per workgroup
enum InfMode { kInfVec = 0, kInfElem = 1 };

typedef double inf_v4d __attribute__((ext_vector_type(4)));

struct InfPrepareParams {
  const double* theta;  // n_draws x n_quant with strides (st_draw, st_quant), elements
  int64_t st_draw, st_quant;
  const double* center;  // [n_quant]
  const double* scale;   // [n_quant]
  int n_draws, n_quant;
  int s_pad, p_pad;
  double* zt;  // [p_pad][s_pad]
};

struct InfParams {
  const void* lw;  // (n_obs, n_draws) log weights
  int64_t n_obs;
  int n_draws;
  int64_t lw_so, lw_sd;  // elements
  const double* zt;      // [p_pad][s_pad]
  int s_pad, p_pad, n_quant;
  double* shift;  // (n_obs, n_quant), each may be null
  double* m2;
  double* kl;     // [n_obs]
  double* ess_w;
};

__global__ __launch_bounds__(256) void influence_prepare_kernel(InfPrepareParams P) {
  const int64_t total = (int64_t)P.p_pad * P.s_pad;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e / P.s_pad);
    const int s = (int)(e - (int64_t)j * P.s_pad);
    double z = 0.0;
    if (j < P.n_quant && s < P.n_draws) z = (P.theta[(int64_t)s * P.st_draw + (int64_t)j * P.st_quant] - P.center[j]) / P.scale[j];
    P.zt[e] = z;
  }
}

// a lane's four consecutive draws d0 .. d0 + 3 of a row, -inf past the row (clamped addresses and selects, no branch around a load)
template <typename T, int MODE>
__device__ __forceinline__ void inf_load(const T* row, int64_t sd, int d0, int S, double (&x)[4]) {
  if constexpr (MODE == kInfVec && sizeof(T) == 8) {  // (n_draws % 2 == 0: a pair is inside the row or past it as a whole)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = d0 + 2 * h;
      const bool ok = d < S;
      const double2 t = *reinterpret_cast<const double2*>(row + (ok ? d : S - 2));
      x[2 * h] = ok ? t.x : -pinf();
      x[2 * h + 1] = ok ? t.y : -pinf();
    }
  } else if constexpr (MODE == kInfVec) {  // (n_draws % 4 == 0)
    const bool ok = d0 < S;
    const float4 t = *reinterpret_cast<const float4*>(row + (ok ? d0 : S - 4));
    x[0] = ok ? (double)t.x : -pinf();
    x[1] = ok ? (double)t.y : -pinf();
    x[2] = ok ? (double)t.z : -pinf();
    x[3] = ok ? (double)t.w : -pinf();
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = d0 + k;
      const bool ok = d < S;
      const double v = (double)row[(int64_t)(ok ? d : S - 1) * sd];
      x[k] = ok ? v : -pinf();
    }
  }
}

// one draw into the three sums of its row; returns e
__device__ __forceinline__ double inf_sums(double lw, double m, double& s1, double& s2, double& sk) {
#pragma clang fp contract(off)
  const double d = lw - m;
  const double e = exp(d);
  s1 += e;
  s2 += e * e;
  sk += e == 0.0 ? 0.0 : e * d;
  return e;
}

// the sum over the four k-quarters of a row (lanes i, i + 16, i + 32, i + 48): the same bits in all four
__device__ __forceinline__ double inf_quarters(double v) {
#pragma clang fp contract(off)
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

template <typename T, int MODE, int NCT>
__global__ __launch_bounds__(kWave * kInfWaves) void influence_kernel(InfParams P) {
  const int S = P.n_draws;
  const int lane = threadIdx.x & (kWave - 1), i = lane & 15, q = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int n_chunks = P.s_pad / kInfK;
  const int n_panels = P.p_pad / (kInfTile * NCT);
  const int64_t n_tiles = (P.n_obs + kInfTile - 1) / kInfTile;
  const int64_t nw = (int64_t)gridDim.x * kInfWaves;
  const double log_s = log((double)S);
  for (int64_t u = (int64_t)blockIdx.x * kInfWaves + wv; u < n_tiles; u += nw) {
    const int64_t r0 = u * kInfTile;
    const T* row = reinterpret_cast<const T*>(P.lw) + (r0 + i < P.n_obs ? r0 + i : P.n_obs - 1) * P.lw_so;
    // ---- sweep 1: the exact maximum of the row, and whether it holds a NaN
    double m = -pinf();
    int bad = 0;
#pragma unroll 2
    for (int c = 0; c < n_chunks; ++c) {
      double x[4];
      inf_load<T, MODE>(row, P.lw_sd, c * kInfK + 4 * q, S, x);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        m = fmax(m, x[k]);
        bad |= x[k] != x[k] ? 1 : 0;
      }
    }
    m = fmax(m, __shfl_xor(m, 16));
    m = fmax(m, __shfl_xor(m, 32));
    bad |= __shfl_xor(bad, 16);
    bad |= __shfl_xor(bad, 32);
    bad |= (m == -pinf() || m == pinf()) ? 1 : 0;
    // ---- sweep 2, per panel of NCT column tiles: e on the VALU, the two products on the matrix cores
    for (int pn = 0; pn < n_panels; ++pn) {
      inf_v4d a1[NCT], a2[NCT];
      double s1 = 0.0, s2 = 0.0, sk = 0.0;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        a1[ct] = inf_v4d{0.0, 0.0, 0.0, 0.0};
        a2[ct] = inf_v4d{0.0, 0.0, 0.0, 0.0};
      }
      const double* zp = P.zt + ((int64_t)(pn * NCT) * kInfTile + i) * P.s_pad + 4 * q;
#pragma unroll 1
      for (int c = 0; c < n_chunks; ++c) {
        double x[4], e[4];
        inf_load<T, MODE>(row, P.lw_sd, c * kInfK + 4 * q, S, x);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = inf_sums(x[k], m, s1, s2, sk);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const double* zc = zp + (int64_t)ct * kInfTile * P.s_pad + c * kInfK;
          const double2 za = *reinterpret_cast<const double2*>(zc), zb = *reinterpret_cast<const double2*>(zc + 2);
          const double z[4] = {za.x, za.y, zb.x, zb.y};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            a1[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(e[k], z[k], a1[ct], 0, 0, 0);
            a2[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(e[k], z[k] * z[k], a2[ct], 0, 0, 0);
          }
        }
      }
      // ---- the row sums over the four k-quarters, then the stores: C / D col = lane & 15, row = (lane >> 4) + 4 reg
      {
#pragma clang fp contract(off)
        const double t1 = inf_quarters(s1), t2 = inf_quarters(s2), tk = inf_quarters(sk);
        if (pn == 0 && q == 0 && r0 + i < P.n_obs) {
          if (P.kl) P.kl[r0 + i] = bad ? qnan() : tk / t1 - log(t1) + log_s;
          if (P.ess_w) P.ess_w[r0 + i] = bad ? qnan() : t1 * t1 / t2;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int rr = q + 4 * g;  // this lane's row of the tile in register g; its sums sit in lane rr
          const double den = __shfl(t1, rr);
          const int nan = __shfl(bad, rr);
          const int64_t r = r0 + rr;
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
            const int j = (pn * NCT + ct) * kInfTile + i;
            if (r < P.n_obs && j < P.n_quant) {
              if (P.shift) P.shift[r * P.n_quant + j] = nan ? qnan() : a1[ct][g] / den;
              if (P.m2) P.m2[r * P.n_quant + j] = nan ? qnan() : a2[ct][g] / den;
            }
          }
        }
      }
    }
  }
}

}  // namespace pla
