// Kernels of the non-factorised LOO log-likelihood (reference: pyloo loo_nonfactor.py:466-557, compute_beta_minus_i 686-733).
//
// For one draw s: C = the given N x N matrix (cov, or prec: the reference inverts either, loo_nonfactor.py:478), r = y - mu_s,
// P = C^-1, c_i = P_ii, g = P r.  The conditional log-likelihood of observation i given the others is
//   normal     ll_i = -1/2 log 2pi + 1/2 log c_i - 1/2 g_i^2 / c_i                                   (490-497)
//   Student-t  nu' = df_s + N - 1, beta_i = r'g - g_i^2 / c_i (the closed form of 686-733),
//              sigma_i = (df_s + beta_i) / nu' / c_i,
//              ll_i = lgamma((nu'+1)/2) - lgamma(nu'/2) - 1/2 log(nu' pi sigma_i) - (nu'+1)/2 log(1 + (g_i/c_i)^2 / (nu' sigma_i))
//                                                                                                      (498-557)
// The formulas are evaluated in the reference's operation order.  All arithmetic is f64; f32 inputs are promoted on load.
//
// Routes.  Every draw is computed by ONE workgroup of kNfThreads threads, start to end, in a fixed order of operations: no
// partial result of a draw depends on the grid, on which workgroup takes the draw, or on the other draws.  The output bits
// are therefore independent of the grid size, of the host staging block and of the input dtype (f32 values promote exactly).
//   lds        N <= kNfLdsMaxObs: the lower triangle, packed, and four vectors of the draw live in LDS (80 KiB: two
//              workgroups per CU).  Column Cholesky C = L L' (right-looking), in-place triangular inverse L^-1 (LAPACK dtrti2
//              order), c_i = sum_k (L^-1)_ki^2, z = L^-1 r, g = L^-T z, r'g = |z|^2.
//   blocked    kNfLdsMaxObs < N <= kNfMaxObs: blocked right-looking Cholesky and blocked triangular inverse (LAPACK dpotrf /
//              dtrtri lower, 16-column panels) on an Np x Np slot of engine memory owned by the workgroup (Np = N rounded up to
//              16; the pad is the identity, so the factor and the inverse are [L, 0; 0, I]).  Each panel: the 16 x 16 diagonal
//              block is staged in LDS and factored (inverted) there; the panel below it is solved row by row against it; every
//              16 x 16 product of the trailing update (and of the inverse's X_IK L_Kj, X_Ij = -T_I X_jj) runs on
//              v_mfma_f64_16x16x4f64, one tile per wave.  f64 MFMA rounds every product and sum as the VALU does, in a fixed
//              order per tile, so the bits do not depend on the grid either.
//   general    LU with partial pivoting (LAPACK getf2 order: the first largest |a_ik| is the pivot) on an N x N slot, then the
//              in-place inverses of U and of the unit L (dtrti2); c_i = (U^-1 L^-1)_{i,q(i)} with q the inverse row
//              permutation, g = U^-1 L^-1 (P' r), r'g = sum_i r_i g_i.  It serves the draws the Cholesky routes decline (flag
//              kNfGeneral): a matrix that is not symmetric within kNfSymTol, or a Cholesky pivot that is not finite or not
//              above N * eps * C_jj (indefinite or numerically singular).  An exact zero LU pivot is the reference's
//              LinAlgError: an all -inf row, no df check (kNfSingular).
// Every route: non-finite input (matrix, mu_s or y) gives an all -inf row (kNfNonfinite; for Student-t draws also the df or
// beta flag the reference's NaN inverse would raise); c_i <= 0 is clamped to DBL_EPSILON (kNfClamped: the reference's line 488
// meant this and raises instead).  Student-t: df_s <= 0 gives an all -inf row (kNfDfNonpos), a non-finite beta_i an -inf entry
// (kNfBetaNonfinite).  NaN log-likelihoods are written as they come; the front turns them into -inf (559-571).
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace pla {

constexpr int kNfThreads = 256;
constexpr int kNfWaves = kNfThreads / 64;
constexpr int kNfMaxObs = 1024;                  // PLA_NONFACTOR_MAX_OBS
// LDS route: packed triangle N(N+1)/2 + 4 vectors of N doubles within 80 KiB (two workgroups per CU of 160 KiB)
constexpr int kNfLdsBytes = 80 * 1024;
constexpr int nf_lds_doubles(int n) { return n * (n + 1) / 2 + 4 * n; }
constexpr int kNfLdsMaxObs = 138;
static_assert(nf_lds_doubles(kNfLdsMaxObs) * 8 <= kNfLdsBytes && nf_lds_doubles(kNfLdsMaxObs + 1) * 8 > kNfLdsBytes,
              "kNfLdsMaxObs is the largest N whose draw fits the LDS budget");
constexpr double kNfSymTol = 1e-12;  // |a_ij - a_ji| <= kNfSymTol * max(|a_ij|, |a_ji|), else the general route

// status word of a draw (PLA_NF_* in include/pyloo_amd.h)
constexpr int kNfGeneral = 1, kNfSingular = 2, kNfNonfinite = 4, kNfDfNonpos = 8, kNfBetaNonfinite = 16, kNfClamped = 32;
constexpr int kNfNormal = 0, kNfStudentT = 1;
constexpr int kNfRouteAuto = 0, kNfRouteLds = 1, kNfRouteWorkspace = 2, kNfRouteGeneral = 3;  // pla_engine_set_nonfactor_route

struct NonfactorParams {
  const void* y;        // [N]
  const void* mu;       // draw s at mu + s * mu_pitch
  const void* mat;      // draw s at mat + s * mat_pitch, C-contiguous N x N
  const void* df;       // [n_draws] (Student-t)
  int N;
  int n_draws;           // < 2^31 (checked by the C API)
  int64_t mu_pitch, mat_pitch;  // elements
  int model;
  int slot;             // doubles per slot of `ws` (< 2^31)
  double* out;          // ll of (i, s) at out[i * so + s * sd]
  int so, sd;           // < 2^31 (checked by the C API)
  int* flags;           // [n_draws]
  double* ws;           // workspace: gridDim.x slots of `slot` doubles (blocked and general routes)
};

template <typename T>
__device__ __forceinline__ double nf_ld(const void* base, int64_t idx) {
  return (double)reinterpret_cast<const T*>(base)[idx];
}

struct NfPacked {  // lower triangle, packed by rows, in LDS
  double* a;
  __device__ __forceinline__ double& operator()(int i, int j) const { return a[i * (i + 1) / 2 + j]; }
};
struct NfSquare {  // N x N row-major slot of engine memory
  double* a;
  int n;
  __device__ __forceinline__ double& operator()(int i, int j) const { return a[(int64_t)i * n + j]; }
};

__device__ __forceinline__ void nf_row_value(const NonfactorParams& p, int s, double v) {
  for (int i = threadIdx.x; i < p.N; i += kNfThreads) p.out[(int64_t)i * p.so + (int64_t)s * p.sd] = v;
}

// y - mu_s into r (the reference's y_vals - mu_s); returns nonzero when some entry is not finite (block-uniform)
template <typename T>
__device__ int nf_load_residual(const NonfactorParams& p, int s, double* r) {
  int bad = 0;
  for (int i = threadIdx.x; i < p.N; i += kNfThreads) {
    const double v = nf_ld<T>(p.y, i) - nf_ld<T>(p.mu, (int64_t)s * p.mu_pitch + i);
    bad |= !isfinite(v);
    r[i] = v;
  }
  return bad;
}

// The status of a draw whose input is not finite: the reference's inverse is NaN, so a Student-t draw raises the df warning
// (df <= 0) or the beta warning.
template <typename T>
__device__ int nf_nonfinite_status(const NonfactorParams& p, int s) {
  if (p.model != kNfStudentT) return kNfNonfinite;
  const double df = nf_ld<T>(p.df, s);
  return kNfNonfinite | (df <= 0.0 ? kNfDfNonpos : kNfBetaNonfinite);
}

// The lower triangle (and its diagonal into dg) while checking finiteness and symmetry.  Returns kNfNonfinite / kNfGeneral bits
// (block-uniform).
template <typename T, class M>
__device__ int nf_load_lower(const NonfactorParams& p, int s, M A, double* dg) {
  const int N = p.N, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)s * p.mat_pitch;
  int nonfinite = 0, asym = 0;
  for (int i = wave; i < N; i += kNfWaves)
    for (int j = lane; j <= i; j += 64) {
      const double a = nf_ld<T>(p.mat, base + (int64_t)i * N + j);
      const double b = nf_ld<T>(p.mat, base + (int64_t)j * N + i);
      if (!isfinite(a) || !isfinite(b))
        nonfinite = 1;
      else if (fabs(a - b) > kNfSymTol * fmax(fabs(a), fabs(b)))
        asym = 1;
      A(i, j) = a;
      if (i == j) dg[i] = a;
    }
  const int nf = __syncthreads_or(nonfinite);
  const int as = __syncthreads_or(asym);
  return (nf ? kNfNonfinite : 0) | (as ? kNfGeneral : 0);
}

// Right-looking column Cholesky of the lower triangle in place.  colbuf (LDS, N) holds column j of L during step j.
// false: a pivot is not finite or not above tol_n * eps * C_jj (tol_n: the draw's N; the draw goes to the general route).
template <class M>
__device__ bool nf_cholesky(M A, int N, double tol_n, const double* dg, double* colbuf) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = 0; j < N; ++j) {
    const double d = A(j, j);
    if (!(d > 0.0) || !(d > tol_n * DBL_EPSILON * dg[j]) || !(d < INFINITY)) return false;
    const double l = sqrt(d);
    __syncthreads();  // every thread has read A(j, j)
    for (int i = j + 1 + tid; i < N; i += kNfThreads) {
      const double v = A(i, j) / l;
      A(i, j) = v;
      colbuf[i] = v;
    }
    if (tid == 0) A(j, j) = l;
    __syncthreads();
    for (int i = j + 1 + wave; i < N; i += kNfWaves) {
      const double lij = colbuf[i];
      for (int k = j + 1 + lane; k <= i; k += 64) A(i, k) = A(i, k) - lij * colbuf[k];
    }
    __syncthreads();
  }
  return true;
}

// In-place inverse of the lower triangle (LAPACK dtrti2, lower: columns from the right).  unit: the diagonal is 1 and is not
// read or written.  Step j reads column j from its copy in colbuf only, so each new entry is written as soon as it is known.
template <class M>
__device__ void nf_invert_lower(M A, int N, bool unit, double* colbuf) {
  const int tid = threadIdx.x;
  for (int j = N - 1; j >= 0; --j) {
    for (int k = j + 1 + tid; k < N; k += kNfThreads) colbuf[k] = A(k, j);
    const double inv = unit ? 1.0 : 1.0 / A(j, j);
    __syncthreads();
    for (int i = j + 1 + tid; i < N; i += kNfThreads) {
      double sum = 0.0;
      for (int k = j + 1; k < i; ++k) sum += A(i, k) * colbuf[k];
      sum += (unit ? 1.0 : A(i, i)) * colbuf[i];
      A(i, j) = -inv * sum;
    }
    if (tid == 0 && !unit) A(j, j) = inv;
    __syncthreads();
  }
}

// In-place inverse of the upper triangle (LAPACK dtrti2, upper: columns from the left), diagonal included.
template <class M>
__device__ void nf_invert_upper(M A, int N, double* colbuf) {
  const int tid = threadIdx.x;
  for (int j = 0; j < N; ++j) {
    for (int k = tid; k < j; k += kNfThreads) colbuf[k] = A(k, j);
    const double inv = 1.0 / A(j, j);
    __syncthreads();
    for (int i = tid; i < j; i += kNfThreads) {
      double sum = 0.0;
      for (int k = i; k < j; ++k) sum += A(i, k) * colbuf[k];
      A(i, j) = -inv * sum;
    }
    if (tid == 0) A(j, j) = inv;
    __syncthreads();
  }
}

// From X = L^-1 (lower, in place): c_i = sum_{k>=i} X_ki^2, z = X r, g = X' z, returns r'g = |z|^2 (thread 0's sum, in order).
template <class M>
__device__ double nf_cholesky_solve(M X, int N, const double* r, double* c, double* z, double* g, double* red) {
  for (int i = threadIdx.x; i < N; i += kNfThreads) {
    double cs = 0.0, zs = 0.0;
    for (int k = i; k < N; ++k) cs += X(k, i) * X(k, i);
    for (int m = 0; m <= i; ++m) zs += X(i, m) * r[m];
    c[i] = cs;
    z[i] = zs;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < N; i += kNfThreads) {
    double gs = 0.0;
    for (int k = i; k < N; ++k) gs += X(k, i) * z[k];
    g[i] = gs;
  }
  if (threadIdx.x == 0) {
    double q = 0.0;
    for (int k = 0; k < N; ++k) q += z[k] * z[k];
    red[0] = q;
  }
  __syncthreads();
  return red[0];
}

// The conditional log-likelihood row of draw s from c, g and r'g; returns the status bits it adds.
template <typename T>
__device__ int nf_finish(const NonfactorParams& p, int s, const double* c, const double* g, double rtg) {
  const int N = p.N;
  constexpr double kLogConst = -0x1.d67f1c864beb4p-1;  // -0.5 * log(2 pi) as NumPy rounds it
  constexpr double kPi = 0x1.921fb54442d18p+1;
  double df = 0.0, nu = 0.0, lg = 0.0;
  if (p.model == kNfStudentT) {
    df = nf_ld<T>(p.df, s);
    if (df <= 0.0) {
      nf_row_value(p, s, -INFINITY);
      return kNfDfNonpos;
    }
    nu = df + (double)N - 1.0;
    lg = lgamma((nu + 1.0) / 2.0) - lgamma(nu / 2.0);
  }
  int clamped = 0, badbeta = 0;
  for (int i = threadIdx.x; i < N; i += kNfThreads) {
    double ci = c[i];
    if (ci <= 0.0) {  // (a NaN stays NaN, as in the reference's bad_idx)
      ci = DBL_EPSILON;
      clamped = 1;
    }
    const double gi = g[i];
    double ll;
    if (p.model != kNfStudentT) {
      ll = kLogConst + 0.5 * log(ci) - 0.5 * (gi * gi / ci);
    } else {
      const double beta = rtg - gi * gi / ci;
      if (!isfinite(beta)) {
        ll = -INFINITY;
        badbeta = 1;
      } else {
        const double yi = nf_ld<T>(p.y, i);
        const double loc = yi - gi / ci;
        const double sigma = ((df + beta) / nu) * (1.0 / ci);
        const double d = yi - loc;
        ll = lg - 0.5 * log(nu * kPi * sigma) - ((nu + 1.0) / 2.0) * log(1.0 + (1.0 / nu) * (d * d / sigma));
      }
    }
    p.out[(int64_t)i * p.so + (int64_t)s * p.sd] = ll;
  }
  const int cl = __syncthreads_or(clamped);
  const int bb = __syncthreads_or(badbeta);
  return (cl ? kNfClamped : 0) | (bb ? kNfBetaNonfinite : 0);
}

// Cholesky routes (LDS or workspace slot): one draw.  Writes flags[s] (kNfGeneral: left to the general kernel).
template <typename T, class M, class Factor>
__device__ void nf_cholesky_draw(const NonfactorParams& p, int s, M A, double* r, double* dg, double* z, double* g,
                                 double* red, Factor factor_and_invert) {
  const int N = p.N;
  const int rbad = __syncthreads_or(nf_load_residual<T>(p, s, r));
  const int st = nf_load_lower<T>(p, s, A, dg);
  if (rbad || (st & kNfNonfinite)) {
    nf_row_value(p, s, -INFINITY);
    if (threadIdx.x == 0) p.flags[s] = nf_nonfinite_status<T>(p, s);
    __syncthreads();
    return;
  }
  if ((st & kNfGeneral) || !factor_and_invert()) {
    if (threadIdx.x == 0) p.flags[s] = kNfGeneral;
    __syncthreads();
    return;
  }
  double* c = dg;  // the diagonal of C is no longer needed
  const double rtg = nf_cholesky_solve(A, N, r, c, z, g, red);
  const int fl = nf_finish<T>(p, s, c, g, rtg);
  if (threadIdx.x == 0) p.flags[s] = fl;
  __syncthreads();
}

template <typename T>
__global__ void __launch_bounds__(kNfThreads) nonfactor_lds_kernel(NonfactorParams p) {
  __shared__ double sm[nf_lds_doubles(kNfLdsMaxObs)];
  __shared__ double red[1];
  const int N = p.N;
  double* tri = sm;
  double* r = tri + N * (N + 1) / 2;
  double* dg = r + N;
  double* z = dg + N;
  double* g = z + N;
  for (int s = blockIdx.x; s < p.n_draws; s += gridDim.x)
    nf_cholesky_draw<T>(p, s, NfPacked{tri}, r, dg, z, g, red, [&] {
      // (g is free until the solve: it holds the working column)
      if (!nf_cholesky(NfPacked{tri}, N, (double)N, dg, g)) return false;
      nf_invert_lower(NfPacked{tri}, N, false, g);
      return true;
    });
}

typedef double nf_v4d __attribute__((ext_vector_type(4)));
constexpr int kNfTile = 16;
constexpr int kNfTilePitch = 17;  // LDS tiles: one pad double per row against bank conflicts

struct NfTileLds {  // 16 x 16 tile in LDS
  double* a;
  __device__ __forceinline__ double& operator()(int i, int j) const { return a[i * kNfTilePitch + j]; }
};

// C + A B over one 16 x 16 x 16 product on v_mfma_f64_16x16x4f64 (one wave).  a(i, k) / b(k, j) return this lane's operand:
// lane l gives A[l & 15][k] and B[k][l & 15] with k = 4 step + (l >> 4); C / D: col = l & 15, row = (l >> 4) + 4 reg.
template <class FA, class FB>
__device__ __forceinline__ nf_v4d nf_mfma16(FA a, FB b, nf_v4d c) {
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
#pragma unroll
  for (int st = 0; st < 4; ++st) c = __builtin_amdgcn_mfma_f64_16x16x4f64(a(i, 4 * st + q), b(4 * st + q, i), c, 0, 0, 0);
  return c;
}

// X = L^-1 of the lower 16 x 16 tile L (LDS), zeros above the diagonal: column tid by forward substitution (threads 0..15).
__device__ __forceinline__ void nf_tile_invert(NfTileLds L, NfTileLds X) {
  if (threadIdx.x < kNfTile) {
    const int c = threadIdx.x;
    for (int i = 0; i < c; ++i) X(i, c) = 0.0;
    X(c, c) = 1.0 / L(c, c);
    for (int i = c + 1; i < kNfTile; ++i) {
      double v = 0.0;
      for (int k = c; k < i; ++k) v += L(i, k) * X(k, c);
      X(i, c) = -v / L(i, i);
    }
  }
}

// Blocked right-looking Cholesky of the Np x Np slot (lower; dpotrf order over 16-column panels).  false: a pivot declined.
__device__ bool nf_blocked_cholesky(NfSquare A, int Np, int N, const double* dg, double* tile, double* colbuf) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = Np / kNfTile;
  const NfTileLds T{tile}, Xk{tile + kNfTile * kNfTilePitch};
  for (int kb = 0; kb < nb; ++kb) {
    const int k0 = kb * kNfTile;
    {  // the diagonal block, staged in LDS and factored there
      const int i = tid >> 4, j = tid & 15;
      T(i, j) = j <= i ? A(k0 + i, k0 + j) : 0.0;
    }
    __syncthreads();
    if (!nf_cholesky(T, kNfTile, (double)N, dg + k0, colbuf)) return false;
    {
      const int i = tid >> 4, j = tid & 15;
      if (j <= i) A(k0 + i, k0 + j) = T(i, j);
    }
    // the panel below: L_Ik = A_Ik L_kk^-T, one 16-row tile per wave on the matrix cores
    nf_tile_invert(T, Xk);
    __syncthreads();
    for (int I = kb + 1 + wave; I < nb; I += kNfWaves) {
      const int I0 = I * kNfTile;
      nf_v4d c = {0.0, 0.0, 0.0, 0.0};
      c = nf_mfma16([&](int i, int k) { return A(I0 + i, k0 + k); }, [&](int k, int j) { return Xk(j, k); }, c);
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) A(I0 + (lane >> 4) + 4 * r4, k0 + (lane & 15)) = c[r4];
    }
    __syncthreads();
    // trailing update A_IJ -= L_Ik L_Jk' for kb < J <= I, one 16 x 16 tile per wave
    int t = 0;
    for (int I = kb + 1; I < nb; ++I)
      for (int J = kb + 1; J <= I; ++J, ++t) {
        if ((t & (kNfWaves - 1)) != wave) continue;
        const int I0 = I * kNfTile, J0 = J * kNfTile, col = lane & 15, row = lane >> 4;
        nf_v4d c;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) c[r4] = A(I0 + row + 4 * r4, J0 + col);
        c = nf_mfma16([&](int i, int k) { return -A(I0 + i, k0 + k); }, [&](int k, int j) { return A(J0 + j, k0 + k); }, c);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) A(I0 + row + 4 * r4, J0 + col) = c[r4];
      }
    __syncthreads();
  }
  return true;
}

// Blocked in-place inverse of the lower factor (dtrtri lower: block columns from the right).  For block column jb:
// X_jj = L_jj^-1 (in LDS), P = L_{>jb, jb} copied to pbuf, then for every block row I > jb: T_I = sum_{K=jb+1..I} X_IK P_K and
// X_Ij = -T_I X_jj, one block row per wave (T_I passes through the wave's LDS tile to become an A operand).
__device__ void nf_blocked_invert(NfSquare A, int Np, double* tile, double* wtiles, double* pbuf) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = Np / kNfTile;
  const NfTileLds L{tile}, X{tile + kNfTile * kNfTilePitch}, W{wtiles + wave * kNfTile * kNfTilePitch};
  for (int jb = nb - 1; jb >= 0; --jb) {
    const int j0 = jb * kNfTile;
    {
      const int i = tid >> 4, j = tid & 15;
      L(i, j) = j <= i ? A(j0 + i, j0 + j) : 0.0;
    }
    for (int e = tid; e < (Np - j0 - kNfTile) * kNfTile; e += kNfThreads) {
      const int i = j0 + kNfTile + e / kNfTile, c = e % kNfTile;
      pbuf[(int64_t)i * kNfTile + c] = A(i, j0 + c);
    }
    __syncthreads();
    nf_tile_invert(L, X);
    __syncthreads();
    {
      const int i = tid >> 4, j = tid & 15;
      A(j0 + i, j0 + j) = X(i, j);
    }
    for (int I = jb + 1 + wave; I < nb; I += kNfWaves) {
      const int I0 = I * kNfTile, col = lane & 15, row = lane >> 4;
      nf_v4d t = {0.0, 0.0, 0.0, 0.0};
      for (int K = jb + 1; K <= I; ++K) {
        const int K0 = K * kNfTile;
        t = nf_mfma16([&](int i, int k) { return A(I0 + i, K0 + k); }, [&](int k, int j) { return pbuf[(int64_t)(K0 + k) * kNfTile + j]; },
                      t);
      }
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) W(row + 4 * r4, col) = t[r4];
      __builtin_amdgcn_wave_barrier();
      nf_v4d x = {0.0, 0.0, 0.0, 0.0};
      x = nf_mfma16([&](int i, int k) { return -W(i, k); }, [&](int k, int j) { return X(k, j); }, x);
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) A(I0 + row + 4 * r4, j0 + col) = x[r4];
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
}

template <typename T>
__global__ void __launch_bounds__(kNfThreads) nonfactor_blocked_kernel(NonfactorParams p) {
  __shared__ double vec[5 * kNfMaxObs];
  __shared__ double tiles[2 * kNfTile * kNfTilePitch];
  __shared__ double wtiles[kNfWaves * kNfTile * kNfTilePitch];
  __shared__ double red[1];
  double* r = vec;
  double* dg = r + kNfMaxObs;
  double* z = dg + kNfMaxObs;
  double* g = z + kNfMaxObs;
  double* colbuf = g + kNfMaxObs;
  const int N = p.N, Np = (N + kNfTile - 1) / kNfTile * kNfTile;
  const NfSquare A{p.ws + (int64_t)blockIdx.x * p.slot, Np};
  double* pbuf = A.a + (int64_t)Np * Np;  // [Np][16]: the panel the inverse works with
  for (int s = blockIdx.x; s < p.n_draws; s += gridDim.x)
    nf_cholesky_draw<T>(p, s, A, r, dg, z, g, red, [&] {
      for (int e = threadIdx.x; e < (Np - N) * Np; e += kNfThreads) {  // the pad: identity rows
        const int i = N + e / Np, j = e % Np;
        A(i, j) = i == j ? 1.0 : 0.0;
        if (i == j) dg[i] = 1.0;
      }
      __syncthreads();
      if (!nf_blocked_cholesky(A, Np, N, dg, tiles, colbuf)) return false;
      nf_blocked_invert(A, Np, tiles, wtiles, pbuf);
      return true;
    });
}

// General route: LU with partial pivoting on the workgroup's slot, for the draws flagged kNfGeneral (by the Cholesky kernel, or
// all of them by the launcher when the route is forced).
template <typename T>
__global__ void __launch_bounds__(kNfThreads) nonfactor_lu_kernel(NonfactorParams p) {
  __shared__ double vec[5 * kNfMaxObs];
  __shared__ int perm[kNfMaxObs];
  __shared__ int qinv[kNfMaxObs];
  __shared__ double rv[kNfThreads];
  __shared__ int ri[kNfThreads];
  __shared__ double red[1];
  __shared__ int piv_sh;
  __shared__ double piv_val;
  const int N = p.N, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* r = vec;
  double* w = r + kNfMaxObs;
  double* c = w + kNfMaxObs;
  double* g = c + kNfMaxObs;
  double* colbuf = g + kNfMaxObs;
  double* rowbuf = w;  // the permuted residual is formed after the factorisation
  const NfSquare A{p.ws + (int64_t)blockIdx.x * p.slot, N};
  for (int s = blockIdx.x; s < p.n_draws; s += gridDim.x) {
    if (!(p.flags[s] & kNfGeneral)) continue;  // (flags[s] is read by every thread: uniform)
    const int rbad = __syncthreads_or(nf_load_residual<T>(p, s, r));
    int mbad = 0;
    const int64_t base = (int64_t)s * p.mat_pitch;
    for (int i = wave; i < N; i += kNfWaves)
      for (int j = lane; j < N; j += 64) {
        const double a = nf_ld<T>(p.mat, base + (int64_t)i * N + j);
        mbad |= !isfinite(a);
        A(i, j) = a;
      }
    for (int i = tid; i < N; i += kNfThreads) perm[i] = i;
    if (__syncthreads_or(mbad) || rbad) {
      nf_row_value(p, s, -INFINITY);
      if (tid == 0) p.flags[s] = kNfGeneral | nf_nonfinite_status<T>(p, s);
      __syncthreads();
      continue;
    }
    bool singular = false;
    for (int k = 0; k < N; ++k) {
      // pivot: the first row of largest |a_ik|, i >= k (each thread scans its rows in order, thread 0 the threads in order)
      double best = -1.0;
      int bi = N;
      for (int i = k + tid; i < N; i += kNfThreads) {
        const double v = fabs(A(i, k));
        if (v > best) {
          best = v;
          bi = i;
        }
      }
      rv[tid] = best;
      ri[tid] = bi;
      __syncthreads();
      if (tid == 0) {
        double b = -1.0;
        int bidx = N;
        for (int t = 0; t < kNfThreads; ++t)
          if (rv[t] > b || (rv[t] == b && ri[t] < bidx)) {
            b = rv[t];
            bidx = ri[t];
          }
        if (bidx >= N) bidx = k;  // no entry compared greater (a NaN column): row k, as idamax, and the NaN propagates
        piv_sh = bidx;
        piv_val = A(bidx, k);
      }
      __syncthreads();
      const int pr = piv_sh;
      if (piv_val == 0.0) {
        singular = true;
        break;
      }
      if (pr != k) {
        for (int j = tid; j < N; j += kNfThreads) {
          const double t = A(k, j);
          A(k, j) = A(pr, j);
          A(pr, j) = t;
        }
        if (tid == 0) {
          const int t = perm[k];
          perm[k] = perm[pr];
          perm[pr] = t;
        }
      }
      __syncthreads();
      const double d = A(k, k);
      for (int i = k + 1 + tid; i < N; i += kNfThreads) {
        const double v = A(i, k) / d;
        A(i, k) = v;
        colbuf[i] = v;
      }
      for (int j = k + 1 + tid; j < N; j += kNfThreads) rowbuf[j] = A(k, j);
      __syncthreads();
      for (int i = k + 1 + wave; i < N; i += kNfWaves) {
        const double lik = colbuf[i];
        for (int j = k + 1 + lane; j < N; j += 64) A(i, j) = A(i, j) - lik * rowbuf[j];
      }
      __syncthreads();
    }
    __syncthreads();
    if (singular) {
      nf_row_value(p, s, -INFINITY);
      if (tid == 0) p.flags[s] = kNfGeneral | kNfSingular;
      __syncthreads();
      continue;
    }
    nf_invert_upper(A, N, colbuf);
    nf_invert_lower(A, N, true, colbuf);
    for (int k = tid; k < N; k += kNfThreads) {
      qinv[perm[k]] = k;
      w[k] = r[perm[k]];
    }
    __syncthreads();
    // c_i = sum_{m >= max(i, q)} U^-1_im L^-1_mq (L^-1_qq = 1), q = qinv[i]; v = L^-1 w into colbuf
    for (int i = tid; i < N; i += kNfThreads) {
      const int q = qinv[i];
      double cs = 0.0;
      for (int m = i > q ? i : q; m < N; ++m) cs += A(i, m) * (m == q ? 1.0 : A(m, q));
      c[i] = cs;
      double vs = w[i];
      for (int k = 0; k < i; ++k) vs += A(i, k) * w[k];
      colbuf[i] = vs;
    }
    __syncthreads();
    for (int i = tid; i < N; i += kNfThreads) {
      double gs = 0.0;
      for (int m = i; m < N; ++m) gs += A(i, m) * colbuf[m];
      g[i] = gs;
    }
    __syncthreads();
    if (tid == 0) {
      double q = 0.0;
      for (int i = 0; i < N; ++i) q += r[i] * g[i];
      red[0] = q;
    }
    __syncthreads();
    const int fl = nf_finish<T>(p, s, c, g, red[0]);
    if (tid == 0) p.flags[s] = kNfGeneral | fl;
    __syncthreads();
  }
}

}  // namespace pla
