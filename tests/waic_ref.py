"""Plain restatement of the WAIC arithmetic (waic.py:109-161), the yardstick of tests/test_gpu_waic_routes.py.

It shares nothing with the kernels, with ``pyloo_amd`` or with ``oracle``: NumPy and ``math`` only.

    x      = ll with NaN -> -1e10, +inf -> +1e10, -inf -> -1e10, in the input dtype (the kernels replace on load, before
             they widen), then widened
    lppd_i = m + log sum_s exp(x - m) - log S        with m = max_s x
    var_i  = sum_s (x - mean)^2 / S                  two passes, ddof 0
    waic_i = scale_value * (lppd_i - var_i)

``wide=True``: ``np.longdouble`` arithmetic, totals with ``math.fsum``.  ``wide=False``: vectorised float64, for matrices too
large for that.
"""

import math

import numpy as np


def sanitise(ll):
    """(matrix with the replacements applied, in the dtype of ``ll``; number of NaN entries; number of infinite entries)"""
    ll = np.asarray(ll)
    nan, inf = np.isnan(ll), np.isinf(ll)
    big = ll.dtype.type(1e10)
    x = np.where(nan, -big, ll)
    x = np.where(inf, np.where(ll > 0, big, -big), x).astype(ll.dtype)
    return x, int(nan.sum()), int(inf.sum())


def waic_ref(ll, scale_value, wide=True):
    """dict(lppd_i, var_i, waic_i, elpd_waic, se, p_waic, n_high, n_nan, n_inf) of an (n_obs, n_draws) float32 / float64 matrix"""
    x, n_nan, n_inf = sanitise(ll)
    n, s = x.shape
    x = x.astype(np.longdouble if wide else np.float64)
    m = x.max(axis=1)
    lppd = m + np.log(np.exp(x - m[:, None]).sum(axis=1)) - np.log(x.dtype.type(s))
    mean = x.sum(axis=1) / s
    var = ((x - mean[:, None]) ** 2).sum(axis=1) / s
    waic = x.dtype.type(scale_value) * (lppd - var)
    lppd_i, var_i, waic_i = (np.asarray(v, dtype=np.float64) for v in (lppd, var, waic))
    if wide:
        elpd = math.fsum(waic_i)
        dev = waic - np.longdouble(elpd) / n
        m2 = math.fsum(np.asarray(dev * dev, dtype=np.float64))
        p_waic = math.fsum(var_i)
    else:
        elpd = float(waic_i.sum())
        m2 = float(((waic_i - waic_i.mean()) ** 2).sum())
        p_waic = float(var_i.sum())
    return {
        "lppd_i": lppd_i,
        "var_i": var_i,
        "waic_i": waic_i,
        "elpd_waic": elpd,
        "se": math.sqrt(m2),  # (n * var(waic_i)) ** 0.5
        "p_waic": p_waic,
        "n_high": int(np.sum(var_i > 0.4)),
        "n_nan": n_nan,
        "n_inf": n_inf,
    }
