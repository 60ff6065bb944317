"""NumPy restatement of the LOO influence values on the CPU oracle's weights (TEST INFRASTRUCTURE ONLY).

Per observation, with ``m = max lw``, ``e = exp(lw - m)`` (a weight of log -inf is 0 and its draw contributes to nothing) and
``z = (theta - center) / scale`` (a division):

    s1 = sum e, s2 = sum e^2
    shift[i, j] = sum_s e_s z_sj / s1
    m2[i, j]    = sum_s e_s z_sj^2 / s1
    kl[i]       = sum_s e_s (lw_s - m) / s1 - log(s1) + log(S)          (terms with e_s = 0 are 0)
    ess_w[i]    = s1^2 / s2

A row whose weights are all NaN or all -inf, or hold a NaN (or a +inf), gives NaN in all of its outputs.  ``loo_influence`` takes
the weights from the oracle exactly as ``diag_ref.loo_diag`` does.  Sums are plain float64 sums over the row."""

import numpy as np

import diag_ref


def center_scale(theta):
    """(center, scale): the mean and the sd (ddof 1) of the draws, per column."""
    th = np.asarray(theta, dtype=np.float64)
    th = th.reshape(-1, 1) if th.ndim == 1 else th
    return th.mean(axis=0), th.std(axis=0, ddof=1)


def from_log_weights(lw, theta, center, scale):
    """dict(shift, m2 (n_obs, P); kl, ess_w [n_obs]) in float64 from log weights of any normalisation."""
    lw = np.atleast_2d(np.asarray(lw, dtype=np.float64))
    th = np.asarray(theta, dtype=np.float64)
    th = th.reshape(-1, 1) if th.ndim == 1 else th
    n, s = lw.shape
    assert th.shape[0] == s
    with np.errstate(all="ignore"):
        z = (th - np.asarray(center, dtype=np.float64)) / np.asarray(scale, dtype=np.float64)
        m = np.max(np.where(np.isnan(lw), -np.inf, lw), axis=1, keepdims=True)
        bad = np.isnan(lw).any(axis=1) | ~np.isfinite(m.reshape(-1))
        d = lw - m
        e = np.where(lw == -np.inf, 0.0, np.exp(d))
        e = np.where(bad[:, None], 0.0, e)  # (keeps the NaN of a bad row out of the products of the others)
        s1 = e.sum(axis=1)
        s2 = (e * e).sum(axis=1)
        shift = np.stack([(e * z[:, j]).sum(axis=1) for j in range(z.shape[1])], axis=1) / s1[:, None]
        m2 = np.stack([(e * (z[:, j] * z[:, j])).sum(axis=1) for j in range(z.shape[1])], axis=1) / s1[:, None]
        kl = np.where(e == 0.0, 0.0, e * d).sum(axis=1) / s1 - np.log(s1) + np.log(float(s))
        ess = s1 * s1 / s2
    nan = np.full(n, np.nan)
    return {"shift": np.where(bad[:, None], np.nan, shift), "m2": np.where(bad[:, None], np.nan, m2),
            "kl": np.where(bad, nan, kl), "ess_w": np.where(bad, nan, ess)}


def loo_influence(ll, theta, reff=1.0, method="psis", M=None, center=None, scale=None):
    """dict(shift, m2, kl, ess_w, diag, n_replaced, lw, M, center, scale): the oracle's weights of -ll (NaN counted as -1e10), each
    row with its own tail count when ``reff`` or ``M`` is a vector; center / scale default to ``center_scale(theta)``."""
    w = diag_ref.loo_diag(ll, reff, method=method, M=M)
    if center is None:
        center, scale = center_scale(theta)
    out = from_log_weights(w["lw"], theta, center, scale)
    out.update(diag=w["diag"], n_replaced=w["n_replaced"], lw=w["lw"], M=w["M"], center=center, scale=scale)
    return out


def front_values(ref, theta):
    """dict(mean_loo, sd_ratio, distance) from ``loo_influence``'s output, as the specification writes them."""
    th = np.asarray(theta, dtype=np.float64)
    th = th.reshape(-1, 1) if th.ndim == 1 else th
    shift = ref["shift"]
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.maximum(ref["m2"] - shift ** 2, 0.0))
        sd = np.where(np.isnan(ref["m2"]), np.nan, sd)
        if th.shape[1] == 1:
            dist = shift[:, 0] ** 2
        else:
            rinv = np.linalg.pinv(np.corrcoef(th, rowvar=False))
            dist = np.array([row @ rinv @ row for row in shift])
    return {"mean_loo": ref["center"] + ref["scale"] * shift, "sd_ratio": sd, "distance": dist}


def make_theta(rng, s, p=5):
    """(n_draws, p) test quantities: standard normal columns, then from the third on a log-normal one, an offset one
    (1e6 + 1e-3 N(0, 1): a column mean far from zero next to a tiny scale) and a pair correlated at 0.8."""
    base = rng.normal(size=(s, p))
    if p > 2:
        base[:, 2] = np.exp(base[:, 2])
    if p > 3:
        base[:, 3] = 1e6 + 1e-3 * base[:, 3]
    if p > 4:
        base[:, 4] = 0.8 * base[:, 0] + 0.6 * base[:, 4]
    return base
