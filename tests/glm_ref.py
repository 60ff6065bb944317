"""NumPy restatement of the GLM log-likelihood generator (include/pyloo_amd.h, ``pla_glm``): the formulas of the kernel's epilogue
in the kernel's order of operations, the constants the fronts hand over, and generators of test models.  TEST INFRASTRUCTURE ONLY."""

import numpy as np
from scipy.special import gammaln

U = 2.0 ** -53
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
ENGINE_FAMILY = {"gaussian": "gaussian", "bernoulli": "binomial", "binomial": "binomial", "poisson": "poisson"}


def gamma_n(n):
    """The constant of the standard dot-product bound: n u / (1 - n u)."""
    return n * U / (1.0 - n * U)


def linpred(X, beta, offset=None, dtype=np.float64):
    X, beta = np.asarray(X, dtype=dtype), np.asarray(beta, dtype=dtype)
    with np.errstate(all="ignore"):
        eta = X @ beta.T
        if offset is not None:
            eta = eta + np.asarray(offset, dtype=dtype)[:, None]
    return eta


def linpred_bound(X, beta, offset=None):
    """gamma_{P+1} (sum_p |x_ip beta_sp| + |offset_i|): holds for any order of summation and for fused multiply-adds."""
    X, beta = np.asarray(X, dtype=np.longdouble), np.asarray(beta, dtype=np.longdouble)
    mag = np.abs(X) @ np.abs(beta).T
    if offset is not None:
        mag = mag + np.abs(np.asarray(offset, dtype=np.longdouble))[:, None]
    return (gamma_n(X.shape[1] + 1) * mag).astype(np.float64)


def obs_const(family, y, trials=None):
    y = np.asarray(y, dtype=np.float64)
    if family == "binomial":
        n = np.asarray(trials, dtype=np.float64)
        return (gammaln(n + 1.0) - gammaln(y + 1.0)) - gammaln(n - y + 1.0)
    if family == "poisson":
        return -gammaln(y + 1.0)
    return None


def draw_const(sigma):
    return -HALF_LOG_2PI - np.log(np.asarray(sigma, dtype=np.float64))


def density(family, eta, y, sigma=None, trials=None, oc=None, dc=None):
    """``ll`` (n, S) from ``eta`` (n, S) by the kernel's formulas; ``family`` is the engine's ("gaussian", "binomial", "poisson"),
    ``oc`` / ``dc`` the constants handed to the kernel (None: 0 / computed from sigma)."""
    eta = np.asarray(eta, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        if family == "gaussian":
            sigma = np.asarray(sigma, dtype=np.float64)
            dc = draw_const(sigma) if dc is None else np.asarray(dc, dtype=np.float64)
            t = (y - eta) / sigma[None, :]
            return dc[None, :] - 0.5 * (t * t)
        c = 0.0 if oc is None else np.asarray(oc, dtype=np.float64)[:, None]
        if family == "binomial":
            n = 1.0 if trials is None else np.asarray(trials, dtype=np.float64)[:, None]
            sp = np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta)))
            return (c + y * eta) - n * sp
        if family == "poisson":
            return (c + y * eta) - np.exp(eta)
    raise ValueError(family)


def log_lik(X, y, beta, family, sigma=None, offset=None, trials=None):
    """The (N, S) matrix of the user-facing family ("bernoulli" included) with NumPy's own ``X @ beta.T``."""
    fam = ENGINE_FAMILY[family]
    oc = None if family == "bernoulli" else obs_const(fam, y, trials)
    return density(fam, linpred(X, beta, offset), y, sigma=sigma, trials=trials, oc=oc)


def make_model(rng, n, s, p, family, with_offset=False):
    """beta = b0 + 0.15 N(0,1)/sqrt(P), b0 = 0.5 N(0,1)/sqrt(P), X ~ N(0,1) with an intercept column, y drawn from the model at b0."""
    X = rng.normal(size=(n, p))
    X[:, 0] = 1.0
    b0 = 0.5 * rng.normal(size=p) / np.sqrt(p)
    beta = b0 + 0.15 * rng.normal(size=(s, p)) / np.sqrt(p)
    offset = 0.3 * rng.normal(size=n) if with_offset else None
    eta0 = X @ b0 + (0.0 if offset is None else offset)
    out = dict(X=X, beta=beta, family=family, sigma=None, trials=None, offset=offset)
    if family == "gaussian":
        out["sigma"] = np.exp(0.1 * rng.normal(size=s))
        out["y"] = eta0 + rng.normal(size=n)
    elif family == "bernoulli":
        out["y"] = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta0))).astype(np.float64)
    elif family == "binomial":
        out["trials"] = rng.integers(1, 12, size=n).astype(np.float64)
        out["y"] = rng.binomial(out["trials"].astype(int), 1.0 / (1.0 + np.exp(-eta0))).astype(np.float64)
    elif family == "poisson":
        out["y"] = rng.poisson(np.exp(eta0)).astype(np.float64)
    else:
        raise ValueError(family)
    return out


def matrix_of(model):
    return log_lik(model["X"], model["y"], model["beta"], model["family"], model["sigma"], model["offset"], model["trials"])
