"""Leave-one-out predictions of a generalised linear model from the design matrix and the draws: the LOO predictive mean and
variance, the residuals, LOO-RMSE, LOO-R2 and LOO-PIT -- the numbers that sit next to ``elpd_loo`` -- without the ``(n_obs,
n_draws)`` log-likelihood matrix and without a matrix of posterior-predictive draws.

For a GLM the conditional mean ``mu``, variance ``v`` and distribution function ``F`` of ``y_i`` given draw ``s`` are closed forms
of the linear predictor and the per-draw auxiliary value, so the leave-one-out quantities are weighted sums over the draws,

    E_loo[y_i] = sum_s w_is mu_is        PIT_i = sum_s w_is F(y_i | draw s),

Rao-Blackwellised: no sampling noise from ``y_hat``, and for counts ``P(Y < y)`` and ``P(Y <= y)`` exactly.  ``pla_glm_predict``
(csrc/pla_glm_predict.h) forms them in the epilogue of the generator's matrix-core tile, against the block of PSIS weights the fused
pass of ``loo_glm`` has just computed.

* ``loo_glm_predict_from_design``   from ``X``, ``y`` and ``beta``
* ``loo_glm_predict``               the same with the draws taken from the ``posterior`` group of ``idata``

Families and links are those of ``loo_glm``; the gamma family has moments and no PIT here.  A count above 4096 has no PIT (NaN,
counted in ``n_pit_skipped``); its moments are computed.  NumPy or torch CUDA inputs; the per-observation results are small and come
back as NumPy arrays, as ``loo_pit``'s do.
"""

import warnings
from dataclasses import dataclass
from typing import Any

import numpy as np

from .base import ISMethod, parse_method, tail_count_for
from .engine import _host
from .loo_glm import _check_reff, _engine_family, _engine_of, _prepare
from .loo_influence import _posterior_columns
from .loo_pit import _randomize
from .utils import to_inference_data

__all__ = ["LooGlmPredict", "loo_glm_predict_from_design", "loo_glm_predict"]

MAX_COUNT = 4096


@dataclass
class LooGlmPredict:
    """Per observation: the LOO predictive ``mean``, ``var`` and ``sd``; ``resid = y - mean`` and ``std_resid = resid / sd``; ``pit``
    (randomised between ``pit_lt`` and ``pit_le`` where asked for; None for the gamma family); ``pareto_k`` and ``elpd_i`` of the
    weights (None when ``log_weights`` were given; ``pareto_k`` also for a method other than PSIS).  Scalars: ``rmse``, ``mae``,
    ``r2 = 1 - var(resid) / var(y)`` (the LOO-R2 of Gelman et al. 2019), ``good_k``, ``n_pit_skipped``, ``warning``."""

    mean: Any
    var: Any
    sd: Any
    resid: Any
    std_resid: Any
    pit: Any
    pit_le: Any
    pit_lt: Any
    pareto_k: Any
    good_k: Any
    elpd_i: Any
    rmse: float
    mae: float
    r2: float
    n_pit_skipped: int
    warning: bool = False


def _np(x):
    return np.asarray(_host(x), dtype=np.float64).reshape(-1)


def loo_glm_predict_from_design(X, y, beta, family, sigma=None, offset=None, trials=None, *, phi=None, shape=None, link=None, reff=1.0,
                                method="psis", log_weights=None, rows=None, randomized="auto", seed=None, groups=None):
    """The LOO predictive moments, residual summaries and LOO-PIT of a GLM from its design matrix ``X`` (N, P), the outcomes ``y`` [N]
    and the draws ``beta`` (S, P), in one fused pass (the module's text).  ``sigma`` / ``phi`` / ``shape``, ``offset``, ``trials``,
    ``link``, ``reff``, ``method`` and ``rows`` as ``loo_glm_from_design`` takes them.  ``log_weights`` (rows of the call, S): log
    weights of any normalisation to use instead of the model's own PSIS weights -- moment-matched ones, say; ``pareto_k`` and
    ``elpd_i`` are then None.  ``randomized``, ``seed``: as ``loo_pit`` (``"auto"`` randomises when any ``pit_lt != pit_le``)."""
    if groups is not None:
        raise NotImplementedError("loo_glm_predict has no group-level terms yet: groups= is outside this pass (use glm_log_lik and loo_pit "
                                  "on a subset of rows)")
    method = parse_method(method)
    reff = _check_reff(reff)
    if randomized not in (True, False, "auto"):
        raise ValueError(f"randomized must be True, False or 'auto', got {randomized!r}")
    if family == "gamma" and randomized is True:
        raise ValueError("the gamma family has no PIT here: randomized=True cannot be honoured")
    Xc, bc, v = _prepare(X, y, beta, family, sigma, offset, trials, phi, shape, link)
    s = bc.shape[0]
    if s < 2:
        raise ValueError("leave-one-out weights need at least two draws")
    M = 0
    if log_weights is None and method == ISMethod.PSIS:
        M = tail_count_for(s, reff)
        if M + 1 > s:
            raise IndexError(f"index {-M - 1} is out of bounds for axis 0 with size {s}")
    res = _engine_of(Xc).glm_predict(Xc, bc, _engine_family(family, link), rows=rows, tail_count=M, method=method.value,
                                     log_weights=log_weights, **v)
    if int(_host(res["n_replaced"]).reshape(-1)[0]) > 0:
        warnings.warn("NaN values detected in log-likelihood. These will be ignored in the LOO calculation.", UserWarning, stacklevel=2)
    yv = _np(v["y"])
    if rows is not None:
        yv = yv[np.asarray(_host(rows), dtype=np.int64).reshape(-1)]
    mean, m2 = _np(res["mean"]), _np(res["m2"])
    var = np.maximum(m2 - mean * mean, 0.0)
    sd = np.sqrt(var)
    resid = yv - mean
    with np.errstate(divide="ignore", invalid="ignore"):
        std_resid = resid / sd
        r2 = float(1.0 - np.var(resid) / np.var(yv)) if yv.size else float("nan")
    k = good_k = None
    warn = False
    if log_weights is None and method == ISMethod.PSIS:
        k = _np(res["diag"])
        good_k = min(1 - 1 / np.log10(s), 0.7)
        if np.any(k > good_k):
            warnings.warn(
                f"Estimated shape parameter of Pareto distribution is greater than {good_k:.2f} for {np.sum(k > good_k)} "
                "observations. This indicates that importance sampling may be unreliable because the marginal posterior and "
                "LOO posterior are very different.", UserWarning, stacklevel=2)
            warn = True
    pit = le = lt = None
    skipped = 0
    if family != "gamma":
        le, lt = _np(res["pit_le"]), _np(res["pit_lt"])
        pit = _randomize(le, lt, randomized, seed)
        skipped = int(_host(res["n_pit_skipped"]).reshape(-1)[0])
        if skipped:
            warnings.warn(f"{skipped} observations have counts above {MAX_COUNT}: their PIT values are NaN", UserWarning, stacklevel=2)
    return LooGlmPredict(mean=mean, var=var, sd=sd, resid=resid, std_resid=std_resid, pit=pit, pit_le=le, pit_lt=lt, pareto_k=k,
                         good_k=good_k, elpd_i=None if log_weights is not None else _np(res["elpd_i"]),
                         rmse=float(np.sqrt(np.mean(resid * resid))) if resid.size else float("nan"),
                         mae=float(np.mean(np.abs(resid))) if resid.size else float("nan"), r2=r2, n_pit_skipped=skipped, warning=warn)


def loo_glm_predict(idata, X, y, family, var_names, sigma_name=None, var_name=None, offset=None, trials=None, reff=1.0, method="psis",
                    rows=None, group_terms=None, *, phi_name=None, shape_name=None, link=None, log_weights=None, randomized="auto",
                    seed=None):
    """``loo_glm_predict_from_design`` with the draws taken from ``idata``, every argument as ``loo_glm`` takes it: the columns of
    ``beta`` are the variables ``var_names`` of the ``posterior`` group; ``sigma_name`` / ``phi_name`` / ``shape_name`` name the
    per-draw scale; ``y=None`` reads ``observed_data[var_name]``.  ``group_terms`` is not supported here (NotImplementedError)."""
    if group_terms is not None:
        raise NotImplementedError("loo_glm_predict has no group-level terms yet: group_terms= is outside this pass")
    data = to_inference_data(idata)
    beta, names, _ = _posterior_columns(data, var_names)
    if beta.shape[1] != X.shape[1]:
        raise ValueError(f"var_names give {beta.shape[1]} columns ({', '.join(names)}) for the {X.shape[1]} columns of X")
    per_draw = {}
    for what, name in (("sigma_name", sigma_name), ("phi_name", phi_name), ("shape_name", shape_name)):
        per_draw[what] = None
        if name is not None:
            col, _, _ = _posterior_columns(data, [name])
            if col.shape[1] != 1:
                raise ValueError(f"{what} must name a scalar variable, '{name}' has {col.shape[1]} entries per draw")
            per_draw[what] = col[:, 0]
    if y is None:
        if var_name is None or not hasattr(data, "observed_data"):
            raise ValueError("y=None needs var_name and an observed_data group")
        obs = data.observed_data[var_name]
        y = np.asarray(getattr(obs, "values", obs), dtype=np.float64).reshape(-1)
    return loo_glm_predict_from_design(X, y, beta, family, sigma=per_draw["sigma_name"], offset=offset, trials=trials,
                                       phi=per_draw["phi_name"], shape=per_draw["shape_name"], link=link, reff=reff, method=method,
                                       log_weights=log_weights, rows=rows, randomized=randomized, seed=seed)
