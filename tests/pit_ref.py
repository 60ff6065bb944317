"""NumPy restatement of the LOO-PIT values on the CPU oracle's weights (TEST INFRASTRUCTURE ONLY).

    pit_le[i] = sum_{y_hat[i,s] <= y[i]} w[i,s]        pit_lt[i] = sum_{y_hat[i,s] < y[i]} w[i,s]

with ``w = softmax(lw)`` over the draws and ``lw`` from ``oracle.psis_oracle.psislw(-ll, reff)`` (NaN log-likelihoods count as
-1e10, loo.py:218-227) or ``importance_weights(-ll, method)``.  Sums are plain float64 sums of ``exp(lw - max)``; the sum over
no draws is 0 (the reference's ``exp(logsumexp(...))`` of an empty set is NaN, -inf - -inf: ``golden_expected`` puts the 0 there)."""

import os

import numpy as np

from oracle import psis_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_pit.npz")


def pit_from_log_weights(lw, y_hat, y):
    """(pit_le, pit_lt) in float64 from log weights of any normalisation."""
    lw = np.asarray(lw, dtype=np.float64)
    yh = np.asarray(y_hat, dtype=np.float64)
    yv = np.asarray(y, dtype=np.float64).reshape(-1, 1)
    with np.errstate(all="ignore"):
        e = np.exp(lw - np.max(lw, axis=-1, keepdims=True))
        den = e.sum(axis=-1)
        le = np.where(yh <= yv, e, 0.0).sum(axis=-1) / den
        lt = np.where(yh < yv, e, 0.0).sum(axis=-1) / den
    return le, lt


def log_weights(ll, reff=1.0, method="psis"):
    """(lw, diag, n_replaced): the oracle's weights of -ll in ll's dtype."""
    ll = np.asarray(ll)
    nan = np.isnan(ll)
    clean = np.where(nan, ll.dtype.type(-1e10), ll)
    with np.errstate(all="ignore"):
        if method == "psis":
            lw, diag = orc.psislw(-clean, reff)
        else:
            lw, diag = orc.importance_weights(-clean, method)
    return lw, np.asarray(diag, dtype=np.float64), int(nan.sum())


def loo_pit(ll, y_hat, y, reff=1.0, method="psis"):
    """dict(pit_le, pit_lt, diag, n_replaced, lw)."""
    lw, diag, nrep = log_weights(ll, reff, method)
    le, lt = pit_from_log_weights(lw, y_hat, y)
    return {"pit_le": le, "pit_lt": lt, "diag": diag, "n_replaced": nrep, "lw": lw}


def load_golden():
    """{case: dict(ll, yh, y, reff, lw, k, pit_le, pit_lt)} of tests/golden/loo_pit.npz."""
    z = np.load(GOLDEN)
    out = {}
    for name in z["names"]:
        name = str(name)
        out[name] = {key: z[f"{name}_{key}"] for key in ("ll", "yh", "y", "reff", "lw", "k", "pit_le", "pit_lt")}
        out[name]["reff"] = float(out[name]["reff"])
    return out


def golden_expected(case):
    """The fixture's (pit_le, pit_lt) with 0 where no draw is counted (the reference's logsumexp of an empty set is NaN)."""
    yh, y = case["yh"], case["y"].reshape(-1, 1)
    le = np.where((yh <= y).any(axis=1), case["pit_le"], 0.0)
    lt = np.where((yh < y).any(axis=1), case["pit_lt"], 0.0)
    return le, lt
