"""NumPy restatement of the LOO diagnostics on the CPU oracle's weights (TEST INFRASTRUCTURE ONLY).

Per observation, with ``m = max lw``, ``e = exp(lw - m)`` and ``w = e / sum e`` (a weight of log -inf is 0 and its draw contributes
to nothing, whatever its ll):

    elpd    = LSE(lw + ll) - LSE(lw)
    ess_w   = (sum e)^2 / sum e^2
    var_log = log1p( sum w^2 (exp(ll - elpd) - 1)^2 )

A row whose elpd is NaN or -inf gives NaN in the three values.  ``loo_diag`` takes the weights from
``oracle.psis_oracle.psis_row(-ll, M)`` per row (its own tail count per row when ``M`` is a vector) or from ``importance_weights``
for SIS / TIS, NaN log-likelihoods counting as -1e10 (loo.py:218-227).  Sums are plain float64 sums over the row."""

import numpy as np

from oracle import psis_oracle as orc


def from_log_weights(lw, ll):
    """dict(elpd_i, ess_w, var_log), float64 [n_obs], from log weights of any normalisation and the log-likelihood."""
    lw = np.atleast_2d(np.asarray(lw, dtype=np.float64))
    ll = np.atleast_2d(np.asarray(ll, dtype=np.float64))
    with np.errstate(all="ignore"):
        live = lw != -np.inf
        m1 = np.max(lw, axis=1, keepdims=True)
        e = np.where(live, np.exp(lw - m1), 0.0)
        s1 = e.sum(axis=1)
        s2 = (e * e).sum(axis=1)
        joint = np.where(live, lw + ll, -np.inf)
        m2 = np.max(joint, axis=1, keepdims=True)
        s3 = np.where(live, np.exp(joint - m2), 0.0).sum(axis=1)
        elpd = (m2 - m1).reshape(-1) + np.log(s3 / s1)
        t = np.where(e == 0.0, 0.0, e * (np.exp(ll - elpd[:, None]) - 1.0))
        s4 = (t * t).sum(axis=1)
        ess = s1 * s1 / s2
        var = np.log1p(s4 / (s1 * s1))
        bad = ~np.isfinite(m1.reshape(-1)) | np.isnan(elpd) | (elpd == -np.inf) | np.isnan(s1)
    nan = np.full(lw.shape[0], np.nan)
    return {"elpd_i": np.where(bad, nan, elpd), "ess_w": np.where(bad, nan, ess), "var_log": np.where(bad, nan, var)}


def tail_counts(n_draws, reff, n_obs):
    """One tail count per observation from a scalar or per-observation reff."""
    r = np.broadcast_to(np.asarray(reff, dtype=np.float64).reshape(-1) if np.ndim(reff) else np.float64(reff), (n_obs,))
    return np.array([orc.tail_count(n_draws, float(v)) for v in r], dtype=np.int64)


def loo_diag(ll, reff=1.0, method="psis", M=None):
    """dict(diag, elpd_i, ess_w, var_log, n_replaced, lw, M).  ``reff``: a float or one value per observation; ``M``: the tail
    count(s) directly instead (a scalar or one per observation)."""
    ll = np.asarray(ll)
    n, s = ll.shape
    nan = np.isnan(ll)
    clean = np.where(nan, ll.dtype.type(-1e10), ll)
    lw = np.empty_like(clean)
    diag = np.empty(n)
    with np.errstate(all="ignore"):
        if method == "psis":
            Ms = tail_counts(s, reff, n) if M is None else np.broadcast_to(np.asarray(M, dtype=np.int64), (n,))
            for i in range(n):
                lw[i], diag[i] = orc.psis_row(-clean[i], int(Ms[i]))
        else:
            Ms = np.zeros(n, dtype=np.int64)
            lw, diag = orc.importance_weights(-clean, method)
    out = from_log_weights(lw, clean)
    out.update(diag=np.asarray(diag, dtype=np.float64), n_replaced=int(nan.sum()), lw=lw, M=Ms)
    return out


def front_values(ref, reff):
    """dict(n_eff, mcse_elpd_i, mcse_elpd_loo) from ``loo_diag``'s output and the relative efficiencies."""
    r = np.broadcast_to(np.asarray(reff, dtype=np.float64), ref["ess_w"].shape)
    with np.errstate(all="ignore"):
        mcse = np.sqrt(ref["var_log"] / r)
    return {"n_eff": r * ref["ess_w"], "mcse_elpd_i": mcse, "mcse_elpd_loo": float(np.sqrt(np.sum(mcse * mcse)))}
