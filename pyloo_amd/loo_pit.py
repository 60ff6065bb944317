"""``loo_pit()`` -- the leave-one-out probability integral transform (ArviZ's ``loo_pit``; the ``ppc_loo_pit_*`` input of
bayesplot and R-loo), on the HIP engine.

    pit_i = P(y~_i <= y_i | y_-i)  ~  sum_s w_is 1[y^_is <= y_i]

with ``w_i`` the Pareto-smoothed leave-one-out weights of observation i and ``y^_i`` its posterior-predictive draws.  The whole
of it is ``pla_loo_pit``: blocks of observations go through the weights pass and are consumed against the predictive draws before
the next block overwrites them, so no ``(n_obs, n_draws)`` weight or indicator matrix is ever written.  The pass returns the
``<=`` and the strict ``<`` value at once; for count data (ties between draws and observation) the PIT is randomised between
the two, ``pit = pit_lt + u (pit_le - pit_lt)`` with ``u`` uniform.  ``loo_pit_from_matrix`` takes the matrices directly
(NumPy or torch CUDA tensors)."""

import warnings
from dataclasses import dataclass
from typing import Any

import numpy as np

from .base import ISMethod, parse_method, tail_count_for
from .engine import _host, _is_torch_tensor, get_engine
from .utils import get_log_likelihood, group_variable, stack_samples, to_inference_data, wrap_obs

__all__ = ["loo_pit", "loo_pit_from_matrix", "LooPitResult"]


@dataclass
class LooPitResult:
    """``pit`` (randomised where asked for), the two one-sided values it lies between, and the Pareto k of the weights (None
    when the weights were given or the method is not PSIS)."""

    pit: Any
    pit_le: Any
    pit_lt: Any
    pareto_k: Any = None
    good_k: Any = None
    warning: Any = None


def _randomize(pit_le, pit_lt, randomized, seed):
    """pit = pit_lt + u (pit_le - pit_lt), clipped to at most 1; rows with pit_lt == pit_le keep their value bit for bit."""
    if randomized not in (True, False, "auto"):
        raise ValueError(f"randomized must be True, False or 'auto', got {randomized!r}")
    ties = pit_lt != pit_le
    if randomized is True or (randomized == "auto" and bool(np.any(ties))):
        u = np.random.default_rng(seed).uniform(size=pit_le.shape[0])
        pit = np.where(ties, pit_lt + u * (pit_le - pit_lt), pit_le)
    else:
        pit = pit_le.copy()
    return np.minimum(pit, 1.0)


def _pit_arrays(log_lik, y_hat, y, log_weights, reff, method, randomized, seed):
    """(pit, pit_le, pit_lt, k or None, good_k or None, warning flag) as flat NumPy arrays."""
    mat = log_weights if log_weights is not None else log_lik
    if mat is None:
        raise ValueError("either a log-likelihood or log_weights is needed")
    if len(mat.shape) != 2 or tuple(y_hat.shape) != tuple(mat.shape):
        raise ValueError(f"y_hat dimensions {tuple(y_hat.shape)} are not compatible with the {tuple(mat.shape)} "
                         f"{'log_weights' if log_weights is not None else 'log-likelihood'} matrix")
    n, s = mat.shape
    y_shape = tuple(y.shape) if hasattr(y, "shape") else np.shape(y)
    if int(np.prod(y_shape)) != n:
        raise ValueError(f"y dimensions {y_shape} are not compatible with {n} observations")
    if _is_torch_tensor(mat) != _is_torch_tensor(y_hat):
        raise ValueError("the matrices must be of one kind: NumPy arrays, or torch CUDA tensors")
    dev = mat.device.index if _is_torch_tensor(mat) else None
    eng = get_engine(dev)
    if log_weights is not None:
        res = eng.loo_pit(mat, y_hat, y, 0, "psis", kind="log_weights")
        k = good_k = None
        warn = False
    else:
        M = tail_count_for(s, reff) if method == ISMethod.PSIS else 0
        if method == ISMethod.PSIS and M + 1 > s:
            raise IndexError(f"index {-M - 1} is out of bounds for axis 0 with size {s}")
        res = eng.loo_pit(mat, y_hat, y, M, method.value, kind="loglik")
        if int(_host(res["n_replaced"]).reshape(-1)[0]) > 0:  # loo.py:218-227
            warnings.warn("NaN values detected in log-likelihood. These will be ignored in the LOO calculation.", UserWarning,
                          stacklevel=3)
        k = good_k = None
        warn = False
        if method == ISMethod.PSIS:
            k = np.asarray(_host(res["diag"]), dtype=np.float64)
            good_k = min(1 - 1 / np.log10(s), 0.7)
            if np.any(k > good_k):
                warnings.warn(
                    f"Estimated shape parameter of Pareto distribution is greater than {good_k:.2f} for {np.sum(k > good_k)} "
                    "observations. This indicates that importance sampling may be unreliable because the marginal posterior and "
                    "LOO posterior are very different.", UserWarning, stacklevel=3)
                warn = True
    pit_le = np.asarray(_host(res["pit_le"]), dtype=np.float64)
    pit_lt = np.asarray(_host(res["pit_lt"]), dtype=np.float64)
    return _randomize(pit_le, pit_lt, randomized, seed), pit_le, pit_lt, k, good_k, warn


def loo_pit_from_matrix(log_lik, y_hat, y, log_weights=None, reff=1.0, method="psis", randomized="auto", seed=None):
    """LOO-PIT from ``(n_obs, n_draws)`` matrices -- NumPy arrays or torch CUDA tensors -- and ``y`` of length n_obs.
    ``log_lik`` may be None when ``log_weights`` (of any normalisation, e.g. ``psislw``'s output) are given: no smoothing then,
    and ``pareto_k`` is None."""
    method = parse_method(method)
    pit, le, lt, k, good_k, warn = _pit_arrays(log_lik, y_hat, y, log_weights, reff, method, randomized, seed)
    return LooPitResult(pit=pit, pit_le=le, pit_lt=lt, pareto_k=k, good_k=good_k, warning=warn)


def _sample_matrix(idata, group, value, arg):
    """A name in ``group`` or an array ``(chain, draw, *obs)`` -> (matrix (n_obs, n_draws), obs_shape, obs_dims, coords)."""
    if value is None or isinstance(value, str):
        da, _ = group_variable(idata, group, value, arg)
        return stack_samples(da)
    arr = np.asarray(getattr(value, "values", value))
    if arr.ndim < 2:
        raise ValueError(f"{arg} must have (chain, draw, *obs) dimensions, got shape {arr.shape}")
    return stack_samples(value if hasattr(value, "dims") else arr)


def loo_pit(data=None, y=None, y_hat=None, log_weights=None, var_name=None, reff=None, method="psis", randomized="auto",
            seed=None):
    """LOO-PIT values of the observations of ``data``.

    ``data``: InferenceData (with ArviZ), or without it the dict of groups ``loo_score`` accepts.  ``y`` / ``y_hat``: names in
    ``observed_data`` / ``posterior_predictive`` (None: the only variable of the group), or arrays ``(*obs)`` /
    ``(chain, draw, *obs)``.  ``log_weights``: ``(chain, draw, *obs)`` log weights used as they are instead of smoothing the
    log-likelihood ``var_name``.  ``randomized``: True, False, or "auto" (randomise iff some draw ties with its observation)."""
    method = parse_method(method)
    idata = to_inference_data(data) if data is not None else None
    if idata is None and (y is None or isinstance(y, str) or y_hat is None or isinstance(y_hat, str)):
        raise ValueError("without data, y and y_hat must be arrays")
    yh, obs_shape, obs_dims, coords = _sample_matrix(idata, "posterior_predictive", y_hat, "y_hat")
    if y is None or isinstance(y, str):
        y_da, _ = group_variable(idata, "observed_data", y, "y")
        yv = np.asarray(getattr(y_da, "values", y_da), dtype=np.float64)
    else:
        yv = np.asarray(getattr(y, "values", y), dtype=np.float64)
    if tuple(yv.shape) != tuple(obs_shape):
        raise ValueError(f"y dimensions {tuple(yv.shape)} are not compatible with y_hat dimensions {tuple(obs_shape)}")
    ll = lw = None
    if log_weights is not None:
        lw, w_shape, _, _ = _sample_matrix(idata, "log_weights", log_weights, "log_weights")
        if tuple(w_shape) != tuple(obs_shape) or lw.shape != yh.shape:
            raise ValueError(f"log_weights dimensions {tuple(w_shape)} are not compatible with y_hat dimensions {tuple(obs_shape)}")
    else:
        if idata is None:
            raise ValueError("without log_weights, data with a log_likelihood group is needed")
        ll, ll_shape, _, _ = stack_samples(get_log_likelihood(idata, var_name=var_name))
        if tuple(ll_shape) != tuple(obs_shape) or ll.shape != yh.shape:
            raise ValueError(f"log_lik dimensions {tuple(ll_shape)} are not compatible with y_hat dimensions {tuple(obs_shape)}")
        if reff is None:
            from .loo import _relative_efficiency

            reff = _relative_efficiency(idata, yh.shape[-1])
    pit, le, lt, k, good_k, warn = _pit_arrays(ll, yh, yv.reshape(-1), lw, reff, method, randomized, seed)
    wrap = lambda v, name: wrap_obs(v, obs_shape, obs_dims, coords, name)  # noqa: E731
    return LooPitResult(pit=wrap(pit, "loo_pit"), pit_le=wrap(le, "loo_pit_le"), pit_lt=wrap(lt, "loo_pit_lt"),
                        pareto_k=None if k is None else wrap(k, "pareto_shape"), good_k=good_k, warning=warn)
