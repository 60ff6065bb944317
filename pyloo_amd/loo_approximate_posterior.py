"""``loo_approximate_posterior()`` -- PSIS-LOO for draws that come from an approximation ``q`` of the posterior (ADVI, Laplace),
corrected with ``log_p`` / ``log_q``, with the reference's signature and result object (pyloo/loo_approximate_posterior.py:20-434),
executed by the HIP engine.

What runs where: argument handling, warnings and ``ELPDData`` packing are host Python (loo_approximate_posterior.py:184-249,
295-320, 350-432); the importance resampling of the draws is :func:`pyloo_amd.loo_subsample.importance_resample` (smoothing on the
device, NumPy's generator); the gather of the whole matrix along the draw axis (line 263), the shift by the column maximum
(266-268: the pass subtracts the row maximum itself), the importance weights and the sums (284-343) are one ``pla_psis_loo_draws``
call: blocks of observations are gathered through the index into the bounded staging buffer by ``gather_draws_kernel`` and passed on,
so the resampled matrix is never materialised whole.  ``p_loo`` uses the lppd of the RESAMPLED matrix, as the reference does
(335-343).

Two places where the reference cannot be followed literally:

* when the resampling raises (non-finite ratios), the reference warns "Importance resampling failed ... Falling back to original
  samples." and then fails on an unbound ``log_ratios_matrix`` (line 279).  Here the warning is the same and the fall-back it
  announces is taken: the identity index, i.e. the plain ``pla_psis_loo`` pass.
* an index whose length is not ``n_samples``, or with entries outside the draws, is treated as ``loo_subsample`` treats it
  (loo_subsample.py:348-370): raised inside the guarded block, so it ends in the same warning and fall-back.

:func:`loo_approximate_posterior_from_matrix` takes the NaN warning from the engine's count of replaced entries, i.e. from the NaN
entries of the draws the index selects (with the reference's permutations: all of them); the matrix is not scanned separately.
"""

import warnings

import numpy as np

from .base import ISMethod, parse_method, tail_count_for
from .elpd import ELPDData
from .engine import _is_torch_tensor, get_engine
from .loo import _checked_method, _diagnostic_warning, _relative_efficiency, _replace_nan, _scale_value, _summaries
from .loo_subsample import importance_resample
from .rcparams import rcParams
from .utils import get_log_likelihood, stack_samples, to_inference_data, wrap_obs

__all__ = ["loo_approximate_posterior", "loo_approximate_posterior_from_matrix"]


def _pack(summ, n_samples, n_data_points, warn, scale, method, good_k, pointwise, loo_i=None, diag=None):
    """Index order of loo_approximate_posterior.py:353-432."""
    data = [summ["elpd_loo"], summ["se"], summ["p_loo"], summ["p_loo_se"], n_samples, n_data_points, warn]
    index = ["elpd_loo", "se", "p_loo", "p_loo_se", "n_samples", "n_data_points", "warning"]
    if pointwise:
        data.append(loo_i)
        index.append("loo_i")
    data += [scale, summ["looic"], summ["looic_se"]]
    index += ["scale", "looic", "looic_se"]
    if pointwise:
        data.append(diag)
        index.append("pareto_k" if method == ISMethod.PSIS else "ess")
    if method == ISMethod.PSIS:
        data.append(good_k)
        index.append("good_k")
    return ELPDData(data=data, index=index)


def _run(matrix, draw_index, method, reff, scale_value, good_k, pointwise):
    """The pass over ``matrix[:, draw_index]`` (the plain pass for ``draw_index=None``).  Returns (pointwise dict, agg, n_replaced)."""
    n_out = matrix.shape[-1] if draw_index is None else int(draw_index.shape[0])
    M = tail_count_for(n_out, reff) if method == ISMethod.PSIS else 0
    if method == ISMethod.PSIS and M + 1 > n_out:
        raise IndexError(f"index {-M - 1} is out of bounds for axis 0 with size {n_out}")
    eng = get_engine(matrix.device.index if _is_torch_tensor(matrix) else None)
    if draw_index is None:
        res = eng.psis_loo(matrix, M, method.value, scale_value, good_k, pointwise, True)
        nrep = 0
    else:
        res = eng.psis_loo_draws(matrix, draw_index, M, method.value, scale_value, good_k, pointwise, True)
        nrep = res["n_replaced"]
    a = res["agg"]
    agg = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)  # (the one host read of a device call)
    return res, agg, int(nrep.item()) if hasattr(nrep, "item") else int(nrep)


def loo_approximate_posterior_from_matrix(log_likelihood, draw_index, reff=1.0, scale=None, method="psis", pointwise=False):
    """Approximate-posterior LOO from an ``(n_obs, n_draws)`` log-likelihood matrix and the index of the resampled draws -- the
    engine-level entry point, like ``loo_from_matrix``.

    ``log_likelihood``: NumPy array or CUDA tensor, draws contiguous or observations contiguous (ArviZ's layout).
    ``draw_index``: the draws in the order and multiplicity the pass should see them (:func:`importance_resample`); an integer
    array, or a CUDA tensor (used as it is: entries outside the draws are clamped on the device); its length need not be the
    matrix's number of draws, and ``n_samples``, ``good_k`` and the low-ESS threshold are those of ``len(draw_index)`` draws.  One
    ``psis_loo_draws`` call and one host read of the aggregates; the pointwise outputs stay where the matrix is."""
    method = parse_method(method)
    scale, scale_value = _scale_value(scale)
    n_obs = log_likelihood.shape[0]
    if not _is_torch_tensor(draw_index):
        draw_index = np.asarray(draw_index).reshape(-1)
    n_samples = int(draw_index.shape[0])  # the draws the pass sees: good_k, the low-ESS threshold and the n_samples row refer to them
    good_k = min(1 - 1 / np.log10(n_samples), 0.7)
    res, agg, nrep = _run(log_likelihood, draw_index, method, reff, scale_value, good_k, pointwise)
    if nrep > 0:
        warnings.warn("NaN values detected in log-likelihood. These will be ignored in the LOO calculation.", UserWarning, stacklevel=2)
    if method != ISMethod.PSIS:
        warnings.warn(
            f"Using {method.value.upper()} for LOO computation. Note that PSIS is the"
            " recommended method as it is typically more efficient and reliable.",
            UserWarning,
            stacklevel=2,
        )
    warn = _diagnostic_warning(method, agg, good_k, n_samples)
    summ = _summaries(agg, n_obs, scale_value)
    out = _pack(summ, n_samples, n_obs, warn, scale, method, good_k, pointwise, res["loo_i"], res["diag"])
    out.method = method.value
    return out


def loo_approximate_posterior(data, log_p, log_q, pointwise=None, var_name=None, reff=None, scale=None, method="psis",
                              resample_method="psis", seed=None):
    """PSIS-LOO-CV for approximate posteriors (e.g. variational inference), from the log densities of the target (``log_p``) and of
    the proposal (``log_q``) at the draws.

    Same parameters, warnings, exceptions and ``ELPDData`` layout as ``pyloo.loo_approximate_posterior``
    (loo_approximate_posterior.py:20-434); the result carries ``approximate_posterior = {"log_p", "log_q"}``.
    """
    idata = to_inference_data(data)
    log_likelihood = get_log_likelihood(idata, var_name=var_name)
    pointwise = rcParams["stats.ic_pointwise"] if pointwise is None else pointwise
    matrix, obs_shape, obs_dims, coords = stack_samples(log_likelihood)  # loo_approximate_posterior.py:188
    n_samples = matrix.shape[-1]
    n_data_points = int(np.prod(obs_shape))
    scale, scale_value = _scale_value(scale)
    if len(log_p) != len(log_q):
        raise ValueError(f"log_p and log_q must have the same length, got {len(log_p)} and {len(log_q)}")
    if reff is None:
        reff = _relative_efficiency(idata, n_samples)
    matrix = _replace_nan(matrix)  # loo_approximate_posterior.py:223-232
    method = _checked_method(method)  # 234-249
    try:
        draw_index = importance_resample(log_p=log_p, log_q=log_q, method=resample_method, seed=seed)
        if len(draw_index) != n_samples:
            # the reference reshapes the resampled draws to the stacked shape (279-282): any other length raises there
            raise ValueError(f"cannot reshape array of size {len(draw_index)} into shape ({n_samples},)")
        if len(draw_index) and (np.min(draw_index) < 0 or np.max(draw_index) >= n_samples):
            raise IndexError(f"index {int(np.max(draw_index))} is out of bounds for axis 0 with size {n_samples}")
    except Exception as e:  # noqa: BLE001  (the reference's catch-all: loo_approximate_posterior.py:270-276)
        warnings.warn(f"Importance resampling failed: {str(e)}. Falling back to original samples.", UserWarning, stacklevel=2)
        draw_index = None
    good_k = min(1 - 1 / np.log10(n_samples), 0.7)  # loo_approximate_posterior.py:296
    res, agg, _ = _run(matrix, draw_index, method, reff, scale_value, good_k, pointwise)
    warn = _diagnostic_warning(method, agg, good_k, n_samples)
    summ = _summaries(agg, n_data_points, scale_value)
    if not pointwise:
        out = _pack(summ, n_samples, n_data_points, warn, scale, method, good_k, False)
    else:
        loo_i = np.asarray(res["loo_i"])
        if loo_i.size and np.allclose(loo_i, loo_i.flat[0]):  # loo_approximate_posterior.py:388-393
            warnings.warn(
                "The point-wise LOO is the same with the sum LOO, please double check "
                "the Observed RV in your model to make sure it returns element-wise logp.",
                stacklevel=2,
            )
        loo_da = wrap_obs(loo_i, obs_shape, obs_dims, coords, "loo_i")
        diag_da = wrap_obs(res["diag"], obs_shape, obs_dims, coords, "pareto_shape" if method == ISMethod.PSIS else "ess")
        out = _pack(summ, n_samples, n_data_points, warn, scale, method, good_k, True, loo_da, diag_da)
    out.method = method.value
    object.__setattr__(out, "approximate_posterior", {"log_p": log_p, "log_q": log_q})
    return out
