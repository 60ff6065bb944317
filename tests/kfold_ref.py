"""Plain restatement of the k-fold log-mean-exp (loo_kfold.py:250-261, 643-667; utils.py:344-357), the yardstick of
tests/test_gpu_kfold_tasks.py.

It shares nothing with the kernels, with ``pyloo_amd`` or with ``oracle``: NumPy only.

    x     = the row widened to ``np.longdouble`` (with ``nan_fix``: NaN -> -1e10 first, and counted)
    lme_i = m + log sum_s exp(x - m) - log S        with m = max_s x

Nothing else is replaced: a NaN that stays, a +inf (inf - inf) and a row of nothing but -inf (-inf + inf) come out as NaN by the
arithmetic itself.  The values come back rounded to float64.
"""

import numpy as np


def lme_ref(rows, nan_fix=False):
    """(lme [n] float64, replaced [n] int64) of an (n, S) float32 / float64 matrix, or of a list of rows of any lengths"""
    if not (isinstance(rows, np.ndarray) and rows.ndim == 2):
        parts = [lme_ref(np.asarray(r).reshape(1, -1), nan_fix) for r in rows]
        return np.array([p[0][0] for p in parts], dtype=np.float64), np.array([p[1][0] for p in parts], dtype=np.int64)
    x = rows.astype(np.longdouble)
    replaced = np.zeros(x.shape[0], dtype=np.int64)
    with np.errstate(all="ignore"):
        if nan_fix:
            nan = np.isnan(x)
            replaced = nan.sum(axis=1).astype(np.int64)
            x = np.where(nan, np.longdouble(-1e10), x)
        m = x.max(axis=1)  # (np.max hands a NaN on)
        lme = m + np.log(np.exp(x - m[:, None]).sum(axis=1)) - np.log(np.longdouble(x.shape[1]))
    return np.asarray(lme, dtype=np.float64), replaced
