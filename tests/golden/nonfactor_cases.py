"""Inputs of the non-factorised LOO goldens (``nonfactor.npz``), regenerated from their seeds.

Spatial exponential-kernel models as in the reference docstring's example: N points in a 10 x 10 square, per draw a mean
``2 + b_x x - b_y y`` and a covariance ``sigma^2 exp(-d / ls) + 0.01 I`` (κ <= 1e4 is asserted by the generator for the SPD
cases).  Special draws are planted into some cases (see ``special``).  Every case: (S = chains * draws) draws.
"""

import numpy as np

# name: (N, chains, draws, model, matrix kind, dtype, method, scale, reff, special, seed)
CASES = {
    "sp25_normal": (25, 2, 100, "normal", "cov", "f64", "psis", "log", 1.0, None, 1),
    "sp25_student": (25, 2, 100, "student_t", "cov", "f64", "psis", "log", 1.0, None, 2),
    "sp25_prec": (25, 1, 120, "normal", "prec", "f64", "psis", "deviance", 0.7, None, 3),
    "sp25_f32": (25, 1, 120, "student_t", "cov", "f32", "psis", "negative_log", 1.0, None, 4),
    "sp25_sis": (25, 1, 120, "normal", "cov", "f64", "sis", "log", 1.0, None, 5),
    "sp25_tis": (25, 1, 120, "student_t", "cov", "f64", "tis", "deviance", 0.7, None, 6),
    "n1": (1, 1, 80, "normal", "cov", "f64", "psis", "log", 1.0, None, 7),
    "n2": (2, 1, 80, "student_t", "cov", "f64", "psis", "log", 1.0, None, 8),
    "n100_normal": (100, 1, 60, "normal", "cov", "f64", "psis", "log", 1.0, None, 9),
    "n100_student": (100, 1, 60, "student_t", "cov", "f64", "psis", "log", 1.0, None, 10),
    "n138": (138, 1, 40, "normal", "cov", "f64", "psis", "log", 1.0, None, 11),
    "n139": (139, 1, 40, "student_t", "cov", "f64", "psis", "log", 1.0, None, 12),
    "highk": (25, 1, 40, "normal", "cov", "f64", "psis", "log", 1.0, "wide", 13),
    "singular": (25, 1, 60, "student_t", "cov", "f64", "psis", "log", 1.0, "singular", 14),
    "nan_entry": (25, 1, 60, "normal", "cov", "f64", "psis", "log", 1.0, "nan", 15),
    "inf_entry": (25, 1, 60, "student_t", "cov", "f64", "psis", "log", 1.0, "inf", 16),
    "df_nonpos": (25, 1, 60, "student_t", "cov", "f64", "psis", "log", 1.0, "df", 17),
    "asym": (25, 1, 60, "normal", "cov", "f64", "psis", "log", 1.0, "asym", 18),
    "indefinite": (25, 1, 60, "normal", "cov", "f64", "psis", "log", 1.0, "indefinite", 19),
}


def spatial_draws(N, S, seed, wide=False):
    """(y, mu (S, N), cov (S, N, N), df (S,)) of one spatial model."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 10, size=(N, 2))
    d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
    true_cov = np.exp(-d / 2.0) + 0.01 * np.eye(N)
    y = rng.multivariate_normal(2 + 0.5 * xy[:, 0] - 0.3 * xy[:, 1], true_cov)
    sig = np.abs(rng.normal(1.0, 0.1, size=S))
    ls = rng.gamma(20.0, 0.1, size=S)
    bx = rng.normal(0.5, 0.5 if wide else 0.05, size=S)
    by = rng.normal(0.3, 0.5 if wide else 0.05, size=S)
    mu = 2 + bx[:, None] * xy[None, :, 0] - by[:, None] * xy[None, :, 1]
    cov = sig[:, None, None] ** 2 * np.exp(-d[None] / ls[:, None, None]) + 0.05 * np.eye(N)[None]
    df = rng.uniform(3.0, 12.0, size=S)
    return y, mu, cov, df


def case_inputs(name):
    """(y, mu, mat, df) with the draws leading, in the case's dtype."""
    N, C, D, model, kind, dt, method, scale, reff, special, seed = CASES[name]
    S = C * D
    y, mu, cov, df = spatial_draws(N, S, seed, wide=special == "wide")
    rng = np.random.default_rng(seed + 1000)
    if special == "singular":
        s = 7
        cov[s, 3, :] = 0.0  # a zero row and column: an exact zero pivot, numpy.linalg.inv raises LinAlgError
        cov[s, :, 3] = 0.0
    elif special == "nan":
        cov[4, 6, 2] = np.nan
    elif special == "inf":
        cov[9, 2, 7] = np.inf  # (an inf where numpy.linalg.inv returns all NaN: elsewhere the reference raises at line 488)
    elif special == "df":
        df[3] = 0.0
        df[11] = -2.0
    elif special == "asym":
        for s in (2, 5):
            cov[s, 1, 4] += 0.01
    elif special == "indefinite":
        for s in (1, 8):
            q, _ = np.linalg.qr(rng.normal(size=(N, N)))
            lam = rng.uniform(1.0, 3.0, size=N)
            lam[:3] = -rng.uniform(0.2, 0.4, size=3)
            while True:
                p = (q * lam) @ q.T
                if np.all(np.diag(p) > 0):
                    break
                lam[:3] *= 0.5
            cov[s] = np.linalg.inv(p)
            cov[s] = 0.5 * (cov[s] + cov[s].T)
    # (kind "prec" passes the same matrices under that name: the reference inverts them too)
    cast = np.float32 if dt == "f32" else np.float64
    return y.astype(cast), mu.astype(cast), cov.astype(cast), df.astype(cast)
