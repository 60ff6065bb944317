"""``loo_lfo()`` -- approximate leave-future-out cross-validation for time series (PSIS-LFO-CV: Buerkner, Gabry & Vehtari 2020,
*J. Stat. Comput. Simul.* 90(14); the "LFO-CV" vignette of R-loo), forward or backward mode, M steps ahead, on the HIP engine.  The
reference has no such function.

The observations 0 .. N-1 are in time order.  ``L`` of them come before the first prediction and ``M`` is the horizon: step
``t = L .. N-M`` conditions on observations ``[0, t)`` and predicts ``[t, t+M)``,

    elpd_lfo = sum_t log p(y_t .. y_{t+M-1} | y_0 .. y_{t-1}).

A model fitted to the first ``i*`` observations serves the steps ``t >= i*`` by importance sampling: the log ratios of step t are
the sum of the log-likelihood rows ``i* .. t-1`` under that fit's draws, Pareto-smoothed; at ``t = i*`` the step is exact.  When
the Pareto k of a step exceeds ``k_threshold`` the model is refitted to the first t observations -- by the caller: ``refit(t)``
returns the log-likelihood of ALL N observations under the new fit -- and the walk goes on from there.

One device pass per fit (``pla_lfo``) computes k and the predictive density of every remaining step at once -- prefix sums down
the observation axis, the weights pass, the predict kernel, block by block, so that no N x S matrix is ever written -- and the
host reads one scalar, the first step above the threshold.  The steps beyond it are discarded: a pass costs milliseconds, a refit
minutes.

``mode="backward"`` is the algorithm as the paper states it.  ``data`` is then the fit to ALL N observations -- the one every user
already has -- and the walk goes DOWN from ``t = N-M`` to ``L``: a fit that saw the first ``last`` observations serves the steps
``t <= last`` with the log ratios ``-sum_{r=t}^{last-1} ll[r]``, which remove from the posterior what the step must not have seen.
Rows ``r >= last`` of a fit's log-likelihood are the conditional terms ``log p(y_r | y_<r, theta)``, which the caller supplies.
With the full fit step ``N-M`` has already removed M observations, so it may itself ask for a refit.  When k exceeds the threshold at
step t the model is refitted to the first t observations (``refit(t)``, the same contract), that step is exact, and the walk goes on
below it.  ``refits`` is in call order, hence descending.  A posterior built on more data moves less per removed observation, so
this mode usually refits less often, and it needs no extra fit to get started.

Out of scope: a combined mode (the paper defines forward and backward PSIS-LFO-CV and no algorithm that mixes them), SIS / TIS,
sharding across GPUs, ``loo_compare`` on LFO results, running the refits, per-step r_eff estimation (``reff`` is one number per fit).
"""

import warnings

import numpy as np

from .base import ISMethod, parse_method, tail_count_for
from .elpd import ELPDData
from .engine import _host, _is_torch_tensor, get_engine
from .loo import _scale_value
from .rcparams import rcParams
from .utils import get_log_likelihood, stack_samples, to_inference_data, wrap_obs

__all__ = ["loo_lfo", "loo_lfo_from_matrix"]


def _time_matrix(obj, var_name):
    """A log-likelihood as an (N, S) matrix with time along the rows: a 2-D CUDA tensor or ndarray is that matrix already,
    anything else goes through the path of ``loo()`` (``(chain, draw, N)`` arrays, dicts, InferenceData)."""
    if _is_torch_tensor(obj):
        if obj.dim() != 2:
            raise ValueError("a tensor log-likelihood must be a 2-D (n_obs, n_draws) matrix")
        return obj if obj.is_cuda else obj.numpy()
    if isinstance(obj, np.ndarray) and obj.ndim == 2:
        return obj
    matrix, obs_shape, _, _ = stack_samples(get_log_likelihood(to_inference_data(obj), var_name=var_name))
    if len(obs_shape) != 1:
        raise ValueError(f"leave-future-out CV needs one observation dimension (time), got observation shape {tuple(obs_shape)}")
    return matrix


def _check(N, L, M, method):
    if parse_method(method) != ISMethod.PSIS:
        raise ValueError("leave-future-out CV supports method='psis' only")
    if int(L) != L or int(M) != M:
        raise ValueError("L and M must be integers")
    if L < 1:
        raise ValueError(f"L must be at least 1, got {L}")
    if M < 1:
        raise ValueError(f"M must be at least 1, got {M}")
    if L + M > N:
        raise ValueError(f"L + M = {L + M} exceeds the {N} observations")


def _walk(mat, reff, L, M, refit, k_threshold, var_name):
    """The host loop: (elpd_t, k_t) for t = L .. N-M as NumPy arrays, the refit steps, the NaN count and the draws of the first fit."""
    N, n_first = int(mat.shape[0]), int(mat.shape[1])
    n_total = N - M - L + 1
    elpd, k = np.empty(n_total), np.empty(n_total)
    refits, n_replaced = [], 0
    t = L
    while True:
        S = int(mat.shape[1])
        tail = tail_count_for(S, reff)
        if tail + 1 > S:
            raise IndexError(f"index {-tail - 1} is out of bounds for axis 0 with size {S}")
        n_steps = N - M - t + 1
        dev = mat.device.index if _is_torch_tensor(mat) else None
        res = get_engine(dev).lfo(mat, t, n_steps, M, tail, k_threshold)
        # without a refit every step is taken; with one, the only value the walk waits for is the first step above the threshold
        take = n_steps if refit is None else int(_host(res["first_high"]).reshape(-1)[0])
        trigger = k[t - L] if refits else 0.0  # (the k that asked for this fit, recorded for its first step)
        elpd[t - L:t - L + take] = _host(res["elpd_i"][:take])
        k[t - L:t - L + take] = _host(res["diag"][:take])
        if refits:
            k[t - L] = trigger
        n_replaced += int(_host(res["n_replaced"]).reshape(-1)[0])
        if take == n_steps:
            break
        k[t - L + take] = float(_host(res["diag"][take:take + 1])[0])
        t += take
        out = refit(t)
        new_reff = reff
        if isinstance(out, tuple):
            out, new_reff = out
        mat = _time_matrix(out, var_name)
        reff = float(new_reff)
        if int(mat.shape[0]) != N:
            raise ValueError(f"refit({t}) returned a log-likelihood of {int(mat.shape[0])} observations, expected all {N}")
        refits.append(t)
    return elpd, k, refits, n_replaced, n_first


def _walk_backward(mat, reff, L, M, refit, k_threshold, var_name):
    """The host loop of backward mode, downward from t = N-M: the same five values as ``_walk`` (``refits`` in call order)."""
    N, n_first = int(mat.shape[0]), int(mat.shape[1])
    n_total = N - M - L + 1
    elpd, k = np.empty(n_total), np.empty(n_total)
    refits, n_replaced = [], 0
    last, t0 = N, N - M  # the observations the current fit saw; the step its pass begins at
    while True:
        S = int(mat.shape[1])
        tail = tail_count_for(S, reff)
        if tail + 1 > S:
            raise IndexError(f"index {-tail - 1} is out of bounds for axis 0 with size {S}")
        n_steps = t0 - L + 1
        dev = mat.device.index if _is_torch_tensor(mat) else None
        res = get_engine(dev).lfo(mat, last, n_steps, M, tail, k_threshold, mode="backward")
        take = n_steps if refit is None else int(_host(res["first_high"]).reshape(-1)[0])
        trigger = k[t0 - L] if refits else 0.0  # (the k that asked for this fit, recorded for its first step)
        lo = t0 - L - take + 1  # step j of the pass is t0 - j: the taken ones fill [lo, t0 - L], reversed
        elpd[lo:t0 - L + 1] = _host(res["elpd_i"][:take])[::-1]
        k[lo:t0 - L + 1] = _host(res["diag"][:take])[::-1]
        if refits:
            k[t0 - L] = trigger
        n_replaced += int(_host(res["n_replaced"]).reshape(-1)[0])
        if take == n_steps:
            break
        t0 -= take
        k[t0 - L] = float(_host(res["diag"][take:take + 1])[0])
        out = refit(t0)
        new_reff = reff
        if isinstance(out, tuple):
            out, new_reff = out
        mat = _time_matrix(out, var_name)
        reff = float(new_reff)
        if int(mat.shape[0]) != N:
            raise ValueError(f"refit({t0}) returned a log-likelihood of {int(mat.shape[0])} observations, expected all {N}")
        refits.append(t0)
        last = t0
    return elpd, k, refits, n_replaced, n_first


def _result(mat, reff, L, M, refit, k_threshold, scale, pointwise, method, var_name, wrap=None, mode="forward"):
    if mode not in ("forward", "backward"):
        raise ValueError(f"mode must be 'forward' or 'backward', got {mode!r}")
    N = int(mat.shape[0])
    _check(N, L, M, method)
    L, M = int(L), int(M)
    if refit is not None and not callable(refit):
        raise TypeError("refit must be None or a callable refit(n_train)")
    k_threshold = float(k_threshold)
    if np.isnan(k_threshold):
        raise ValueError("k_threshold is NaN")
    scale, scale_value = _scale_value(scale)
    pointwise = rcParams["stats.ic_pointwise"] if pointwise is None else pointwise
    walk = _walk if mode == "forward" else _walk_backward
    elpd, k, refits, n_replaced, n_samples = walk(mat, float(reff), L, M, refit, k_threshold, var_name)
    warn = False
    if n_replaced > 0:  # loo.py:218-227
        warnings.warn("NaN values detected in log-likelihood. These will be ignored in the LOO calculation.", UserWarning, stacklevel=3)
    n_high = int(np.sum(k > k_threshold))
    if refit is None and n_high > 0:  # loo.py:291-304, per step
        warnings.warn(
            f"Estimated shape parameter of Pareto distribution is greater than {k_threshold:.2f} for {n_high} steps. This indicates "
            "that importance sampling may be unreliable because the marginal posterior and LOO posterior are very different.",
            UserWarning, stacklevel=3)
        warn = True
    lfo_t = scale_value * elpd
    n_steps = lfo_t.size
    data = [float(lfo_t.sum()), float((n_steps * np.var(lfo_t)) ** 0.5), n_samples, n_steps, warn]
    index = ["elpd_lfo", "se", "n_samples", "n_data_points", "warning"]

    def by_t(v, name):  # indexed by t = 0 .. N-1: NaN where there is no step
        full = np.full(N, np.nan)
        full[L:N - M + 1] = v
        return full if wrap is None else wrap(full, name)

    if pointwise:
        data.append(by_t(lfo_t, "lfo_i"))
        index.append("lfo_i")
    data += [scale, L, M, k_threshold, len(refits), list(refits)]
    index += ["scale", "L", "M", "k_threshold", "n_refits", "refits"]
    if pointwise:
        data.append(by_t(k, "pareto_shape"))
        index.append("pareto_k")
    data.append(min(1 - 1 / np.log10(n_samples), 0.7))
    index.append("good_k")
    out = ELPDData(data=data, index=index)
    out.method = "psis"
    object.__setattr__(out, "lfo_mode", mode)  # (a plain attribute: not a key of the result, whose index is the same in both modes)
    return out


def loo_lfo_from_matrix(log_likelihood, L, M=1, refit=None, k_threshold=0.7, reff=1.0, scale=None, pointwise=False, method="psis",
                        mode="forward"):
    """PSIS leave-future-out CV from an ``(N, S)`` log-likelihood matrix with time along the rows: a NumPy array or a torch CUDA
    tensor (read in place with the draws or the observations contiguous, so a ``.T`` view of an ``(S, N)`` buffer is not copied).

    ``log_likelihood[r, s] = log p(y_r | theta_s)`` for ALL N observations under the draws of a fit to the first ``L``.
    ``refit(n_train)`` returns the same under a fit to the first ``n_train`` observations -- an ``(N, S')`` matrix, or a tuple
    ``(matrix, reff)``; the draw count may differ from fit to fit (the tail count is recomputed).  It is called at the first step
    whose Pareto k exceeds ``k_threshold``; every fit gets one device pass over all the steps that remain, and what that pass
    computed beyond the next refit is discarded (a pass costs milliseconds, a refit minutes).  With ``refit=None`` every step uses
    the first fit and the steps above the threshold are counted in a warning.

    Returns an ``ELPDData``: ``elpd_lfo``, ``se`` (``sqrt(n_steps var)``), ``n_samples`` (of the first fit), ``n_data_points`` (the
    number of steps), ``warning``, ``scale``, ``L``, ``M``, ``k_threshold``, ``n_refits``, ``refits`` (the steps t at which a refit
    happened; the k recorded there is the one that asked for it), ``good_k``; with ``pointwise=True`` also ``lfo_i`` and
    ``pareto_k``, length N and indexed by t (NaN where there is no step).  The attribute ``lfo_mode`` is the mode.

    ``mode="backward"``: ``log_likelihood`` is that of the fit to ALL N observations; the walk goes down from ``t = N-M`` to ``L``,
    ``refit(t)`` is called at the first step (from above) whose k exceeds the threshold, and ``refits`` is descending (see the
    module's text)."""
    if len(log_likelihood.shape) != 2:
        raise ValueError("log_likelihood must be a 2-D (n_obs, n_draws) matrix")
    return _result(_time_matrix(log_likelihood, None), reff, L, M, refit, k_threshold, scale, pointwise, method, None, mode=mode)


def loo_lfo(data, L, M=1, refit=None, var_name=None, k_threshold=0.7, reff=None, scale=None, pointwise=None, method="psis",
            mode="forward"):
    """PSIS leave-future-out CV of a time series model (see :func:`loo_lfo_from_matrix`).

    ``data``: the fit to the first ``L`` observations with the log-likelihood of all N -- InferenceData (with ArviZ), a dict of
    groups, or a ``(chain, draw, N)`` array; more than one observation dimension raises ``ValueError`` (time is one axis).
    ``refit(n_train)`` returns the same kind of object for a fit to the first ``n_train`` observations (or an ``(N, S)`` matrix),
    alone or as ``(log_likelihood, reff)``; without a ``reff`` of its own a refit keeps the current one.  ``reff=None`` estimates
    the relative efficiency of the first fit as ``loo()`` does.  ``mode="backward"``: ``data`` is the fit to ALL N observations."""
    idata = to_inference_data(data)
    log_likelihood = get_log_likelihood(idata, var_name=var_name)
    matrix, obs_shape, obs_dims, coords = stack_samples(log_likelihood)
    if len(obs_shape) != 1:
        raise ValueError(f"leave-future-out CV needs one observation dimension (time), got observation shape {tuple(obs_shape)}")
    if reff is None:
        from .loo import _relative_efficiency

        reff = _relative_efficiency(idata, matrix.shape[-1])
    return _result(matrix, reff, L, M, refit, k_threshold, scale, pointwise, method, var_name,
                   wrap=lambda v, name: wrap_obs(v, obs_shape, obs_dims, coords, name), mode=mode)
