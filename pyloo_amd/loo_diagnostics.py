"""``loo_diagnostics()`` -- how many effective draws stand behind every ``loo_i`` and what its Monte Carlo error is, on the HIP
engine: the ``n_eff`` column ("Min. ESS") of R-loo's Pareto-k table and its ``mcse_elpd_loo`` line.  The reference has neither.

Per observation i, with ``w`` the normalised leave-one-out weights (``pla_loo_diag``, csrc/pla_diag.h):

    ess_w_i   = 1 / sum_s w_is^2
    var_log_i = log1p( sum_s w_is^2 (exp(ll_is - elpd_i) - 1)^2 )        (Vehtari et al. 2024, eq. 6, on the log scale)
    n_eff_i       = r_eff_i ess_w_i
    mcse_elpd_i   = sqrt(var_log_i / r_eff_i)
    mcse_elpd_loo = sqrt(sum_i mcse_elpd_i^2)

``reff`` is a float, a vector with one relative efficiency per observation (NumPy or a torch CUDA tensor, e.g. the output of
``relative_eff``), or None: ``relative_eff`` of the same matrix.  A vector also sets every observation's own PSIS tail length:
the observations are bucketed by tail count (``base.tail_buckets``) and every bucket runs through the row-selection route of the
unchanged kernels.

    r = pl.relative_eff_from_matrix(ll, n_chains=4)
    d = pl.loo_diagnostics_from_matrix(ll, reff=r)
    print(pl.pareto_k_table(d), d.mcse_elpd_loo)

Out of scope: R-loo's older simulation-based ``mcse_elpd``, rank-normalised / bulk / tail ESS.
"""

import warnings
from dataclasses import dataclass
from typing import Any

import numpy as np

from .base import ISMethod, check_reff_vector, is_reff_vector, parse_method, tail_count_for
from .e_loo import _pareto_khat_threshold
from .engine import _host, _is_torch_tensor, get_engine
from .loo import bucketed_matrix, scatter_buckets
from .relative_eff import relative_eff_from_matrix
from .utils import get_log_likelihood, stack_samples, to_inference_data, wrap_obs

__all__ = ["loo_diagnostics", "loo_diagnostics_from_matrix", "pareto_k_table", "LooDiagnostics"]

_KEYS = ("diag", "elpd_i", "ess_w", "var_log")


@dataclass
class LooDiagnostics:
    """Pointwise (observation-shaped): ``pareto_k`` (None unless PSIS; then ``ess`` is None), ``n_eff``, ``r_eff``, ``mcse_elpd_i``,
    ``elpd_i`` and ``min_ss``, the sample size ``k`` asks for (Vehtari et al. 2024, eq. 9).  Scalars: ``mcse_elpd_loo``,
    ``khat_threshold``, ``good_k``, ``n_samples``, ``n_replaced``."""

    pareto_k: Any
    n_eff: Any
    r_eff: Any
    mcse_elpd_i: Any
    elpd_i: Any
    mcse_elpd_loo: float
    min_ss: Any
    khat_threshold: Any
    good_k: Any
    n_samples: int
    n_replaced: int
    ess: Any = None
    method: str = "psis"


def _min_ss(k):
    """:func:`e_loo._pareto_min_ss` of every entry (``10^(1 / (1 - max(0, k)))`` below 1, inf from 1 on; NaN stays NaN)."""
    k = np.asarray(k, dtype=np.float64)
    with np.errstate(all="ignore"):
        out = np.where(k < 1, np.power(10.0, 1.0 / (1.0 - np.maximum(k, 0.0))), np.inf)
    return np.where(np.isnan(k), np.nan, out)


def _arrays(ll, reff, method, n_chains):
    """Flat NumPy arrays ``dict(diag, elpd_i, ess_w, var_log, r_eff)`` and the NaN count; every check before the first engine call."""
    if len(ll.shape) != 2:
        raise ValueError("ll must be a 2-D (n_obs, n_draws) matrix")
    n_obs, n_samples = ll.shape
    if reff is None:
        if n_chains is None:
            raise ValueError("reff=None asks for relative_eff of the matrix and needs its chains: pass n_chains, or reff")
        reff = relative_eff_from_matrix(ll, n_chains=n_chains)
    eng_of = lambda m: get_engine(m.device.index if _is_torch_tensor(m) else None)  # noqa: E731
    if is_reff_vector(reff) and method == ISMethod.PSIS:
        matrix, r, buckets = bucketed_matrix(ll, reff)
        eng = eng_of(matrix)
        if len(buckets) <= 1:
            res = eng.loo_diag(matrix, buckets[0][0] if buckets else 0, method.value)
            n_replaced = int(_host(res["n_replaced"]).reshape(-1)[0])
        else:
            counts = []

            def run(m, index):
                out = eng.loo_diag(matrix, m, method.value, rows=index)
                counts.append(out["n_replaced"])
                return out

            res = scatter_buckets(matrix, buckets, _KEYS, run)
            n_replaced = int(sum(int(_host(c).reshape(-1)[0]) for c in counts))
        r = _host(r)
    else:
        if is_reff_vector(reff):  # (no tail to set: the multiplier of n_eff and the divisor of the variance alone)
            r = _host(check_reff_vector(reff, n_obs))
            M = 0
        else:
            M = tail_count_for(n_samples, reff) if method == ISMethod.PSIS else 0
            if method == ISMethod.PSIS and M + 1 > n_samples:
                raise IndexError(f"index {-M - 1} is out of bounds for axis 0 with size {n_samples}")
            r = np.full(n_obs, float(reff))
        res = eng_of(ll).loo_diag(ll, M, method.value)
        n_replaced = int(_host(res["n_replaced"]).reshape(-1)[0])
    if _is_torch_tensor(res["diag"]):  # one copy to the host for the four vectors
        import torch

        stacked = torch.stack([res[k] for k in _KEYS]).cpu().numpy()
        out = {k: stacked[i] for i, k in enumerate(_KEYS)}
    else:
        out = {k: np.asarray(res[k], dtype=np.float64) for k in _KEYS}
    out["r_eff"] = np.asarray(r, dtype=np.float64)
    return out, n_replaced


def _result(a, n_replaced, method, n_samples, wrap):
    if n_replaced > 0:  # loo.py:218-227
        warnings.warn("NaN values detected in log-likelihood. These will be ignored in the LOO calculation.", UserWarning, stacklevel=3)
    r = a["r_eff"]
    n_eff = r * a["ess_w"]
    with np.errstate(invalid="ignore"):
        mcse = np.sqrt(a["var_log"] / r)
    total = float(np.sqrt(np.sum(mcse * mcse)))
    psis = method == ISMethod.PSIS
    return LooDiagnostics(
        pareto_k=wrap(a["diag"], "pareto_shape") if psis else None,
        n_eff=wrap(n_eff, "n_eff"), r_eff=wrap(r, "r_eff"), mcse_elpd_i=wrap(mcse, "mcse_elpd_i"), elpd_i=wrap(a["elpd_i"], "elpd_i"),
        mcse_elpd_loo=total,
        min_ss=wrap(_min_ss(a["diag"]), "min_ss") if psis else None,
        khat_threshold=_pareto_khat_threshold(n_samples) if psis else None,
        good_k=min(_pareto_khat_threshold(n_samples), 0.7) if psis else None,
        n_samples=int(n_samples), n_replaced=int(n_replaced),
        ess=None if psis else wrap(a["diag"], "ess"), method=method.value)


def loo_diagnostics_from_matrix(ll, reff=1.0, method="psis", n_chains=None):
    """Diagnostics from an ``(n_obs, n_draws)`` log-likelihood matrix, a NumPy array or a torch CUDA tensor (read in place with the
    draws or the observations contiguous).  ``reff``: a float, a vector of length ``n_obs`` of either kind (``ValueError`` for a
    wrong length or an entry that is not positive and finite, before anything runs), or None: ``relative_eff_from_matrix`` of
    ``ll`` with ``n_chains`` chains (``ValueError`` without ``n_chains``).  With ``method`` "sis" or "tis" a vector sets no tail
    length and only scales ``n_eff`` and the error.  Returns :class:`LooDiagnostics` with flat NumPy arrays."""
    method = parse_method(method)
    a, n_replaced = _arrays(ll, reff, method, n_chains)
    return _result(a, n_replaced, method, ll.shape[1], lambda v, name: v)


def loo_diagnostics(data, var_name=None, reff=None, method="psis"):
    """Diagnostics of the observations of ``data`` (InferenceData with ArviZ, a dict of groups or a ``(chain, draw, *obs)`` array,
    as ``loo()`` takes them).  ``reff=None``: ``relative_eff`` of the log-likelihood with the chains of ``data`` -- this function's
    own default; a float or an observation-shaped array otherwise.  The pointwise fields are shaped like the observations."""
    method = parse_method(method)
    log_likelihood = get_log_likelihood(to_inference_data(data), var_name=var_name)
    sizes = getattr(log_likelihood, "sizes", None)
    n_chains = int(sizes["chain"]) if sizes is not None and "chain" in sizes else int(np.shape(getattr(log_likelihood, "values", log_likelihood))[0])
    matrix, obs_shape, obs_dims, coords = stack_samples(log_likelihood)
    a, n_replaced = _arrays(matrix, reff, method, n_chains)
    return _result(a, n_replaced, method, matrix.shape[1], lambda v, name: wrap_obs(v, obs_shape, obs_dims, coords, name))


def pareto_k_table(d):
    """R-loo's Pareto-k table of a :class:`LooDiagnostics`: a DataFrame over the bins ``(-inf, good_k]``, ``(good_k, 1]`` and
    ``(1, inf)`` with ``Count``, ``Pct.`` and ``Min. n_eff``.  A k that is not finite counts in the last bin; an empty bin has
    ``Min. n_eff`` NaN."""
    import pandas as pd

    if d.pareto_k is None:
        raise ValueError("the Pareto-k table needs method='psis'")
    k = np.asarray(getattr(d.pareto_k, "values", d.pareto_k), dtype=np.float64).reshape(-1)
    n_eff = np.asarray(getattr(d.n_eff, "values", d.n_eff), dtype=np.float64).reshape(-1)
    good = float(d.good_k)
    first = k <= good
    second = (k > good) & (k <= 1.0)
    masks = [first, second, ~(first | second)]
    labels = [f"(-Inf, {good:.2f}]", f"({good:.2f}, 1]", "(1, Inf)"]
    words = ["(good)", "(bad)", "(very bad)"]
    rows = []
    for mask in masks:
        vals = n_eff[mask]
        vals = vals[~np.isnan(vals)]
        count = int(mask.sum())
        rows.append((count, 100.0 * count / k.size if k.size else 0.0, float(vals.min()) if vals.size else float("nan")))
    frame = pd.DataFrame(rows, columns=["Count", "Pct.", "Min. n_eff"], index=[f"{a} {b}" for a, b in zip(labels, words)])
    frame.index.name = "Pareto k"
    return frame
