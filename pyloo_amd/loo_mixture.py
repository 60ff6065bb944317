"""``loo_mixture()`` -- Mix-IS-LOO (Silva & Zanella 2022), the estimator behind ``pyloo.loo(..., mixture=True)``
(pyloo/loo.py:252-284 with 360-365 / 400-410 and 536-597), executed by the HIP engine.

For draws from the mixture of leave-one-out posteriors, with ``ll`` the ``(n_obs, n_draws)`` log-likelihood:

    c_s    = log sum_i exp(-ll[i, s])              one value per DRAW, over the observations
    a_i    = log sum_s exp(-ll[i, s] - c_s)        one value per observation, over the draws
    elpd_i = log sum_s exp(-c_s)  -  a_i

No Pareto fit, no refit: two log-sum-exp reductions over the matrix, one along each axis (``pla_mixis_draw_lse`` and
``pla_mixis_loo``).  Host Python: argument handling, the warnings and the ``ELPDData`` packing.

Deliberate departures from the reference:

* The axis of ``c``.  The reference's code takes the first log-sum-exp over the DRAWS (loo.py:261-266), subtracts it per
  observation (271) and reduces over the draws again (274): ``l_i - l_i = 0``, so every pointwise value equals the constant
  ``log_norm_const``.  With ``exp(ll) = [[1/2, 1/4], [1/8, 1/2]]`` it returns ``log(4/15)`` twice; the estimator its warning text,
  its report, the paper and the ArviZ case study it was taken from describe -- the formulas above -- gives
  ``[log(4/13), log(4/17)]``.  This module computes the documented estimator.
* ``mixture=True`` stays a ``NotImplementedError`` in ``loo()``; this is the entry point.
* On load NaN counts as -1e10 (loo.py:218-227, with the reference's warning) and +inf / -inf as +1e10 / -1e10 (``waic``'s rule):
  without it one -inf makes ``c_s = +inf`` and turns a whole draw into NaN for every observation.
* float32 input is widened on load and reduced in float64.
* ``loo_compare`` does not take these results: they carry no ``p_loo``, which the reference's table needs.
"""

import warnings

import numpy as np

from ._capi import AGG_M2_LOO, AGG_SUM_LOO
from .elpd import ELPDData
from .engine import _is_torch_tensor, get_engine
from .loo import _scale_value
from .rcparams import rcParams
from .utils import get_log_likelihood, stack_samples, to_inference_data, wrap_obs

__all__ = ["loo_mixture", "loo_mixture_from_matrix"]

_MIXTURE_WARNING = (
    "Mix-IS-LOO requires a model that is sampled from a mixture of"
    " leave-one-out posteriors. Ensure the inference data passed to the `loo`"
    " function comes from a model that is sampled from such a distribution."
)


def _to_host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _engine_passes(matrix, scale_value, pointwise, stacklevel):
    """Both passes; the NaN warning of loo.py:218-227 from the count of pass 1.  Returns (engine result, agg ndarray).  A host
    matrix goes to the device once per pass."""
    dev = matrix.device.index if _is_torch_tensor(matrix) else None
    eng = get_engine(dev)
    first = eng.mixis_draw_lse(matrix)
    if int(_to_host(first["n_replaced"])[0]) > 0:
        warnings.warn(
            "NaN values detected in log-likelihood. These will be ignored in the LOO calculation.",
            UserWarning,
            stacklevel=stacklevel,
        )
    res = eng.mixis_loo(matrix, c=first["c"], scale_value=scale_value, pointwise=pointwise)
    return res, _to_host(res["agg"])


def _pack(agg, n_samples, n_data_points, scale, good_k, pointwise, loo_i=None, pareto_k=None):
    """Index order of loo.py:536-597 + 360-365 / 400-410 for a mixture result: no p_loo, no looic."""
    elpd, se = float(agg[AGG_SUM_LOO]), float(agg[AGG_M2_LOO]) ** 0.5  # (n * var)^0.5 with var = M2 / n
    data = [elpd, se, n_samples, n_data_points, False]
    index = ["elpd_loo", "se", "n_samples", "n_data_points", "warning"]
    if pointwise:
        data.append(loo_i)
        index.append("loo_i")
    data.append(scale)
    index.append("scale")
    if pointwise:
        data.append(pareto_k)
        index.append("pareto_k")
    data += [good_k, n_data_points]
    index += ["good_k", "subsample_size"]
    return ELPDData(data=data, index=index)


def _same_pointwise_warning(loo_i, stacklevel):
    if loo_i.size and np.allclose(loo_i, loo_i.flat[0]):  # loo.py:377-382
        warnings.warn(
            "The point-wise LOO is the same with the sum LOO, please double check "
            "the Observed RV in your model to make sure it returns element-wise logp.",
            stacklevel=stacklevel,
        )


def loo_mixture_from_matrix(log_likelihood, scale=None, pointwise=False):
    """Mix-IS-LOO from an ``(n_obs, n_draws)`` log-likelihood matrix -- the engine-level entry point.

    ``log_likelihood`` may be a NumPy array (host) or a torch CUDA tensor (device-resident: read in place, twice, whatever its
    strides).  With ``pointwise=True`` on a tensor ``loo_i`` and ``pareto_k`` are returned as device tensors; the check behind the
    reference's "point-wise LOO is the same" warning still copies ``loo_i`` to the host once, and the two replaced-entry counts
    and the aggregates always come back to the host, so the call synchronises."""
    if len(log_likelihood.shape) != 2:
        raise ValueError("log_likelihood must be a 2-D (n_obs, n_draws) matrix")
    scale, scale_value = _scale_value(scale)
    n_data_points, n_samples = int(log_likelihood.shape[0]), int(log_likelihood.shape[1])
    good_k = min(1 - 1 / np.log10(n_samples), 0.7) if n_samples > 1 else 0.7
    warnings.warn(_MIXTURE_WARNING, UserWarning, stacklevel=2)
    res, agg = _engine_passes(log_likelihood, scale_value, pointwise, 3)
    if not pointwise:
        return _pack(agg, n_samples, n_data_points, scale, good_k, False)
    loo_i = res["loo_i"]
    _same_pointwise_warning(_to_host(loo_i), 3)
    pareto_k = loo_i.new_zeros(loo_i.shape) if _is_torch_tensor(loo_i) else np.zeros(n_data_points)
    return _pack(agg, n_samples, n_data_points, scale, good_k, True, loo_i, pareto_k)


def loo_mixture(data, pointwise=None, var_name=None, scale=None):
    """Mix-IS-LOO for draws from a mixture of leave-one-out posteriors (``pyloo.loo(..., mixture=True)``).

    ``data``, ``pointwise``, ``var_name`` and ``scale`` as in ``loo()``.  Returns an ``ELPDData`` with the reference's mixture
    layout: ``elpd_loo, se, n_samples, n_data_points, warning, [loo_i,] scale, [pareto_k,] good_k, subsample_size`` --
    ``warning`` is ``False`` and ``pareto_k`` all zeros (there is no Pareto fit), and there is no ``p_loo`` and no ``looic``."""
    idata = to_inference_data(data)
    log_likelihood = get_log_likelihood(idata, var_name=var_name)
    pointwise = rcParams["stats.ic_pointwise"] if pointwise is None else pointwise
    matrix, obs_shape, obs_dims, coords = stack_samples(log_likelihood)  # loo.py:189
    n_samples = matrix.shape[-1]
    n_data_points = int(np.prod(obs_shape))  # loo.py:192
    scale, scale_value = _scale_value(scale)
    good_k = min(1 - 1 / np.log10(n_samples), 0.7) if n_samples > 1 else 0.7  # loo.py:249
    warnings.warn(_MIXTURE_WARNING, UserWarning, stacklevel=2)  # loo.py:253-259
    res, agg = _engine_passes(matrix, scale_value, pointwise, 3)
    if not pointwise:
        return _pack(agg, n_samples, n_data_points, scale, good_k, False)
    loo_i = np.asarray(res["loo_i"])
    _same_pointwise_warning(loo_i, 3)
    loo_da = wrap_obs(loo_i, obs_shape, obs_dims, coords, "loo_i")
    k_da = wrap_obs(np.zeros(n_data_points), obs_shape, obs_dims, coords, "pareto_shape")  # loo.py:277
    return _pack(agg, n_samples, n_data_points, scale, good_k, True, loo_da, k_da)
