"""Inputs of ``compare.npz`` (``make_golden_compare.py``) and of the tests that read it: every case's (K, N) matrix of pointwise
values is regenerated from its seed with NumPy's PCG64 generator, so the fixture holds only the reference's results."""

import numpy as np

# name: (seed, K, N, scale, kind); kind "plain": K models of different quality, "identical": models 0 and 1 equal (a flat stacking
# optimum), "dominated": the last model far below the others, "close": models within a bootstrap standard error of one another
CASES = {
    "k2_n1_log": (11, 2, 1, "log", "plain"),
    "k2_n8_log": (12, 2, 8, "log", "plain"),
    "k3_n2000_neg": (13, 3, 2000, "negative_log", "plain"),
    "k4_n2000_dev": (14, 4, 2000, "deviance", "plain"),
    "k4_n100000_log": (15, 4, 100000, "log", "plain"),
    "k8_n100000_log": (16, 8, 100000, "log", "plain"),
    "k3_n2000_identical": (17, 3, 2000, "log", "identical"),
    "k3_n2000_dominated": (18, 3, 2000, "log", "dominated"),
    "k8_n8_dev": (19, 8, 8, "deviance", "plain"),
}

# Bayesian bootstrap: (seed of the input, K, N, scale), alpha, B, seed of the reference's RandomState
BB_INPUT = (21, 3, 2000, "log", "close")
BB_ALPHAS = (1.0, 0.5, 2.0)
BB_SAMPLES = 1000
BB_SEED = 1234

_SCALE = {"log": 1.0, "negative_log": -1.0, "deviance": -2.0}


def pointwise(seed, K, N, scale, kind="plain"):
    """(K, N) pointwise values on ``scale``: log-scale values -1.2 - step * k (step = 0.08 / K) + 0.6 * (an effect shared by the models, so they are
    correlated as real ones are) + 0.5 * (a model's own noise, large enough that every model is best somewhere and the stacking
    optimum is interior and well conditioned), then multiplied by the scale's factor."""
    rng = np.random.default_rng(seed)
    common = rng.normal(size=N)
    x = np.empty((K, N))
    step = 0.0025 if kind == "close" else 0.08 / K
    noise = 0.25 if kind == "close" else 0.5
    for k in range(K):
        x[k] = -1.2 - step * k + 0.6 * common + noise * rng.normal(size=N)
    if kind == "identical":
        x[1] = x[0]
    elif kind == "dominated":
        x[K - 1] = x[0] - 3.0 - 0.5 * np.abs(rng.normal(size=N))
    return _SCALE[scale] * x
