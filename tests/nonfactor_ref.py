"""NumPy restatement of the non-factorised conditional log-likelihood (test-only; csrc/pla_nonfactor.h states the math).

It follows loo_nonfactor.py:466-557 with beta in closed form, the clamp of c_i <= 0 to eps that line 488 intends, and the
all -inf row of a draw with non-finite input.  ``tests/test_nonfactor_host.py`` anchors it to the reference goldens, so the
large-N GPU tests can use it where the reference is too slow.  Returns (ll (N, S), flags (S,)) without the PLA_NF_GENERAL bit.
"""

import numpy as np
import scipy.special

GENERAL, SINGULAR, NONFINITE, DF_NONPOS, BETA_NONFINITE, CLAMPED = 1, 2, 4, 8, 16, 32


def loglik(y, mu, mat, df=None, model="normal"):
    y = np.asarray(y, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    mat = np.asarray(mat, dtype=np.float64)
    df = None if df is None else np.asarray(df, dtype=np.float64)
    S, N = mu.shape
    ll = np.empty((N, S))
    flags = np.zeros(S, dtype=np.int32)
    for s in range(S):
        r = y - mu[s]
        if not (np.all(np.isfinite(mat[s])) and np.all(np.isfinite(r))):
            ll[:, s] = -np.inf
            flags[s] = NONFINITE
            if model == "student_t":
                flags[s] |= DF_NONPOS if df[s] <= 0 else BETA_NONFINITE
            continue
        try:
            P = np.linalg.inv(mat[s])
        except np.linalg.LinAlgError:
            ll[:, s] = -np.inf
            flags[s] = SINGULAR
            continue
        g = P @ r
        c = np.diag(P).copy()
        if np.any(c <= 0):
            flags[s] |= CLAMPED
            c[c <= 0] = np.finfo(float).eps
        with np.errstate(all="ignore"):
            if model == "normal":
                ll[:, s] = -0.5 * np.log(2 * np.pi) + 0.5 * np.log(c) - 0.5 * (g**2 / c)
                continue
            if df[s] <= 0:
                ll[:, s] = -np.inf
                flags[s] = DF_NONPOS
                continue
            beta = r @ g - g**2 / c
            nu = df[s] + N - 1
            sigma = ((df[s] + beta) / nu) * (1 / c)
            d = y - (y - g / c)
            row = (scipy.special.gammaln((nu + 1) / 2) - scipy.special.gammaln(nu / 2) - 0.5 * np.log(nu * np.pi * sigma)
                   - ((nu + 1) / 2) * np.log(1 + (1 / nu) * (d**2 / sigma)))
            bad = ~np.isfinite(beta)
            if bad.any():
                flags[s] |= BETA_NONFINITE
                row[bad] = -np.inf
            ll[:, s] = row
    return ll, flags


def beta_by_deletion(y, mu_s, P, i):
    """compute_beta_minus_i (loo_nonfactor.py:686-733) as the reference writes it."""
    r = np.delete(y - mu_s, i)
    p = np.delete(P[:, i], i)
    sub = np.delete(np.delete(P, i, axis=0), i, axis=1)
    return r @ (sub - np.outer(p, p) / P[i, i]) @ r
