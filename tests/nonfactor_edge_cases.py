"""TEST INFRASTRUCTURE ONLY: the inputs of the loo_nonfactor edge suites (csrc/pla_nonfactor.h).

``tests/test_nonfactor_edges_host.py`` proves, on the CPU alone, the properties that make a comparison on these inputs
meaningful (rows that really swap, a Cholesky that declines at the column named, condition numbers under which the project's
tolerances were set, a restatement that a long-double evaluation confirms); ``tests/test_gpu_nonfactor_edges.py`` runs the same
inputs through the kernels.  The inputs are defined here, once, in pure NumPy.

Every generator starts from ``spd_draws`` of tests/test_gpu_nonfactor.py: an exponential kernel over N random points plus
0.1 I, one length scale per draw.

    pivoting_draws   SPD + skew (R - R'): positive definite and not symmetric, so the inverse has a positive diagonal (nothing is
                     clamped), the Cholesky routes decline every draw, and partial pivoting swaps rows at most steps.
    decline_batch    three SPD draws, C[m, m] of the middle one negated: the leading m x m block is untouched, so a Cholesky in
                     any order -- column, or blocked over 16-column panels -- declines exactly at column m.
    mixed_batch      twelve draws, one of each kind the status word knows, among plain SPD ones.
    scaled           cov c, y sqrt(c), mu sqrt(c): every ll_i moves by -1/2 log c and no route decision may move at all.
"""

import functools

import numpy as np
import scipy.linalg
import scipy.special

import nonfactor_ref
from test_gpu_nonfactor import spd_draws

EPS = np.finfo(np.float64).eps
MODELS = ("normal", "student_t")
LDS_MAX_OBS = 138          # kNfLdsMaxObs
TILE = 16                  # kNfTile
SYM_TOL = 1e-12            # kNfSymTol
LDS_GRID, WS_SLOTS = 2048, 512  # kNfGridAuto, the cap of nonfactor_slots()
COND_BOUND = 1e3           # the condition number under which 1e-9 (N < 500) and 1e-8 were set (tests/test_gpu_nonfactor.py)

# ------------------------------------------------------------------------------------------------------------ the case tables
PIVOT_N = (1, 2, 3, 16, 17, 63, 64, 65, 255, 256, 257, 300, 513, 1023, 1024)
PIVOT_F32_N = (17, 257)
PIVOT_AUTO_N = (17, 150)
# seed = N, except: seed 2 swaps no row in any of its four 2 x 2 draws; seed 64 gives a Student-t row with df + beta_i < 0 (a NaN
# the restatement would have to share bit for bit).  The host file holds every seed to the same conditions.
PIVOT_RESEEDED = {2: 1005, 64: 1064}
PIVOT_SEED = {N: PIVOT_RESEEDED.get(N, N) for N in PIVOT_N + PIVOT_AUTO_N}
PANEL_N = (15, 16, 31, 32, 33, 48, 80, 143, 144, 145, 1008, 1009, 1023)
DECLINE_M = {24: (0, 1, 15, 16, 17, 23), 150: (0, 1, 15, 16, 17, 100, 143, 144, 149)}
DECLINE_SEED = {24: 24, 150: 150}
MIXED_N = (24, 150)
MIXED_SEED = {24: 24, 150: 150}
MIXED_DECLINE_M = {24: 17, 150: 100}
MIXED_NAN, MIXED_ASYM, MIXED_DECLINE, MIXED_SINGULAR, MIXED_DF, MIXED_INF_MU, MIXED_NEAR_SYM = 1, 3, 4, 6, 8, 9, 10
SCALES = (1e-100, 1e100)
SCALE_N = (24, 150)
LAUNCH_N, LAUNCH_S, LAUNCH_SEED = 3, 4100, 3
BLOCK_CASES = ((400, 3, "f8"), (400, 3, "f4"), (150, 1, "f8"))  # (N, S, dtype) of the one-draw-per-block calls
DTYPES = {"f8": np.float64, "f4": np.float32}


def tol(N):
    return 1e-9 if N < 500 else 1e-8


def pivot_s(N):
    return 2 if N >= 1000 else 4


def panel_s(N):
    return (1, 5) if N < 200 else (2,)


def nan_as_ninf(a):
    """NaN log-likelihoods are -inf after the front (loo_nonfactor.py:559-571): both sides are compared that way."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), -np.inf, a)


# ----------------------------------------------------------------------------------------------------------------- generators
def pivoting_draws(N, S, seed, skew=0.5):
    y, mu, cov, df = spd_draws(N, S, seed)
    R = np.random.default_rng(seed + 77).normal(size=(S, N, N))
    return y, mu, cov + skew * (R - R.transpose(0, 2, 1)), df


def decline_batch(N, m, seed):
    """Three SPD draws; the middle one has C[m, m] negated."""
    y, mu, cov, df = spd_draws(N, 3, seed)
    cov[1, m, m] = -cov[1, m, m]
    return y, mu, cov, df


def declining_at(N, m, seed):
    """The planted draw of ``decline_batch`` alone."""
    y, mu, cov, df = decline_batch(N, m, seed)
    return y, mu[1:2], cov[1:2], df[1:2]


def mixed_batch(N, seed):
    y, mu, mat, df = spd_draws(N, 12, seed)
    mat[MIXED_NAN, 3, N - 2] = np.nan                                # upper triangle only
    mat[MIXED_ASYM, 0, N - 1] *= 1 + 1e-10                           # asymmetric beyond kNfSymTol
    m = MIXED_DECLINE_M[N]
    mat[MIXED_DECLINE, m, m] = -mat[MIXED_DECLINE, m, m]             # a Cholesky declines at column m
    mat[MIXED_SINGULAR, 4, :] = mat[MIXED_SINGULAR, :, 4] = 0.0      # exactly singular: a zero pivot in any order
    df[MIXED_DF] = -1.0
    mu[MIXED_INF_MU, N - 1] = np.inf
    mat[MIXED_NEAR_SYM, 0, N - 1] *= 1 + 1e-14                       # asymmetric within kNfSymTol: stays a Cholesky draw
    return y, mu, mat, df


def nan_y_batch(N, seed):
    y, mu, cov, df = spd_draws(N, 3, seed)
    y[N // 2] = np.nan
    return y, mu, cov, df


def scaled(inputs, c):
    y, mu, cov, df = inputs
    return y * np.sqrt(c), mu * np.sqrt(c), cov * c, df


def f32_ulp_batch(N, seed):
    """Four f32 SPD draws; draw 2 has one entry above the diagonal raised by one f32 ulp (relative 6e-8 > kNfSymTol)."""
    y, mu, cov, df = (a.astype(np.float32) for a in spd_draws(N, 4, seed))
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    cov[2, 1, N - 2] = np.nextafter(cov[2, 1, N - 2], np.float32(np.inf))
    return y, mu, cov, df


def stride_batch(N, seed):
    """Five draws: draw 1 holds a NaN, draw 3 is asymmetric."""
    y, mu, cov, df = spd_draws(N, 5, seed)
    cov[1, N - 1, 0] = np.nan
    cov[3, 0, 1] += 0.25
    return y, mu, cov, df


def block_batch(N, S, dtype):
    """SPD draws for the one-draw-per-block calls; draw 1 (when there is one) is asymmetric."""
    y, mu, cov, df = (a.astype(DTYPES[dtype]) for a in spd_draws(N, S, seed=N + S))
    if S > 1:
        cov[1, 2, N - 3] *= 1.5
    return y, mu, cov, df


@functools.lru_cache(maxsize=None)
def pivot_case(N, dtype="f8"):
    """(inputs, {model: (ll, flags)}) of the pivoting-LU test at N: the restatement on the values as the kernel widens them."""
    inp = tuple(a.astype(DTYPES[dtype]) for a in pivoting_draws(N, pivot_s(N), PIVOT_SEED[N]))
    return inp, references(inp)


@functools.lru_cache(maxsize=None)
def panel_case(N, S):
    inp = spd_draws(N, S, seed=N)
    return inp, references(inp)


def references(inp):
    wide = [np.asarray(a, dtype=np.float64) for a in inp]
    out = {model: nonfactor_ref.loglik(*wide, model) for model in MODELS}
    for ll, fl in out.values():
        ll.setflags(write=False)
        fl.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ properties (host test only)
def swap_count(a):
    """Rows LAPACK's partial pivoting (dgetrf) swaps while it factors ``a``."""
    _, piv = scipy.linalg.lu_factor(a)
    return int(np.count_nonzero(piv != np.arange(a.shape[0])))


def lu_gather(a, inverse_permutation=True):
    """diag(a^-1) the way the LU kernel gathers it: P a = L U, c_i = (U^-1 L^-1)[i, q(i)] with q the inverse of the row
    permutation.  inverse_permutation=False takes the permutation itself: the slip the pivoting inputs have to expose."""
    lu, piv = scipy.linalg.lu_factor(a)
    n = a.shape[0]
    perm = np.arange(n)
    for k, p in enumerate(piv):
        perm[[k, p]] = perm[[p, k]]
    qinv = np.empty(n, dtype=np.int64)
    qinv[perm] = np.arange(n)
    x = np.linalg.inv(np.triu(lu)) @ np.linalg.inv(np.tril(lu, -1) + np.eye(n))
    return x[np.arange(n), qinv if inverse_permutation else perm]


def cond(a):
    return float(np.linalg.cond(np.asarray(a, dtype=np.float64)))


def cholesky_decline_column(c):
    """The column at which a right-looking column Cholesky with the kernel's pivot rule (finite and above N eps C_jj) declines
    ``c``, or None."""
    a = np.array(c, dtype=np.float64)
    n = a.shape[0]
    dg = np.diag(a).copy()
    for j in range(n):
        d = a[j, j]
        if not (d > 0.0) or not (d > n * EPS * dg[j]) or not (d < np.inf):
            return j
        col = a[j + 1:, j] / np.sqrt(d)
        a[j + 1:, j + 1:] -= np.outer(col, col)
    return None


def inverse_longdouble(a):
    """Gauss-Jordan with partial pivoting in ``numpy.longdouble`` (80-bit where the host test runs; it asserts that)."""
    n = a.shape[0]
    w = np.array(a, dtype=np.longdouble)
    swaps = []
    for k in range(n):  # in place: column k of the identity side replaces column k of the matrix as it is eliminated
        p = k + int(np.argmax(np.abs(w[k:, k])))
        if p != k:
            w[[k, p]] = w[[p, k]]
        swaps.append(p)
        piv = w[k, k]
        w[k, k] = 1
        w[k] /= piv
        f = w[:, k].copy()
        f[k] = 0
        w[:, k] -= f
        w -= f[:, None] * w[k][None]
    for k in reversed(range(n)):  # (P A)^-1 = A^-1 P': undo the row swaps on the columns
        if swaps[k] != k:
            w[:, [k, swaps[k]]] = w[:, [swaps[k], k]]
    return w


def loglik_longdouble(y, mu_s, P, df_s, model):
    """One finite, non-singular draw through the formulas of nonfactor_ref.loglik, in long double from the inverse ``P`` on (the
    two lgamma values are f64: they are the same numbers on both sides)."""
    ld = np.longdouble
    N = y.shape[0]
    r = (np.asarray(y, dtype=np.float64) - np.asarray(mu_s, dtype=np.float64)).astype(ld)
    g = P @ r
    c = np.diag(P).copy()
    c[c <= 0] = ld(EPS)
    pi = ld(np.pi)
    with np.errstate(all="ignore"):
        if model == "normal":
            return -ld(0.5) * np.log(2 * pi) + ld(0.5) * np.log(c) - ld(0.5) * (g**2 / c)
        beta = r @ g - g**2 / c
        nu = ld(df_s) + N - 1
        sigma = ((ld(df_s) + beta) / nu) * (1 / c)
        d = g / c
        lg = ld(scipy.special.gammaln(float((nu + 1) / 2))) - ld(scipy.special.gammaln(float(nu / 2)))
        return lg - ld(0.5) * np.log(nu * pi * sigma) - ((nu + 1) / 2) * np.log(1 + (1 / nu) * (d**2 / sigma))
