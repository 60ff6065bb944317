"""``loo_nonfactor()`` -- LOO for one joint multivariate normal or Student-t likelihood (pyloo/loo_nonfactor.py), with the
reference's signature, checks, warnings and ``ELPDData`` layout.

What runs where: argument handling, warnings and packing are host Python (loo_nonfactor.py:289-464, 559-682).  The per-draw
loop of 466-557 -- a dense inverse per draw and, for Student-t models, an (N-1) x (N-1) quadratic form per observation -- is one
``pla_nonfactor_loglik`` call (csrc/pla_nonfactor.h: Cholesky or LU per draw on the GPU, beta in closed form), and its (N, S)
result goes to the existing ``pla_psis_loo`` pass as a device tensor when the inputs are CUDA tensors.

Decided deviations ("Non-factorised LOO"):
- ``prec`` is inverted like ``cov`` (loo_nonfactor.py:478): ``prec=P`` gives the numbers of ``cov=P``, as in the reference.
- ``c_i <= 0`` is clamped to ``np.finfo(float).eps`` as line 488 intends (the reference raises there: ``np.diag`` is read-only).
- A draw with a non-finite entry in its matrix, its mean or ``y`` gives an all ``-inf`` row.
"""

import warnings

import numpy as np

from ._capi import NF_BETA_NONFINITE, NF_DF_NONPOS, PLA_NONFACTOR_MAX_OBS
from .base import ISMethod, parse_method
from .elpd import ELPDData
from .engine import _is_torch_tensor, get_engine
from .loo import _engine_pass, _relative_efficiency, _scale_value, _summaries
from .rcparams import rcParams
from .utils import to_inference_data, wrap_obs

__all__ = ["loo_nonfactor", "loo_nonfactor_from_arrays", "nonfactor_log_lik"]

_MODEL_TYPES = ("normal", "student_t")


def _names(group):
    return list(group.data_vars) if hasattr(group, "data_vars") else list(group.keys())


def _values(v):
    return v.values if hasattr(v, "values") and not isinstance(v, np.ndarray) and not _is_torch_tensor(v) else v


def _validate_model_structure(idata, mu_var_name, cov_var_name, prec_var_name, model_type="normal", df_var_name="df"):
    """loo_nonfactor.py:736-786."""
    if not hasattr(idata, "posterior"):
        return False
    names = _names(idata.posterior)
    if mu_var_name not in names:
        warnings.warn(
            f"Mean vector '{mu_var_name}' not found in posterior. "
            "This function requires a multivariate normal model with a mean vector.",
            UserWarning,
            stacklevel=3,
        )
        return False
    has_cov = (cov_var_name is not None and cov_var_name in names) or "cov" in names
    has_prec = (prec_var_name is not None and prec_var_name in names) or "prec" in names
    if not (has_cov or has_prec):
        warnings.warn(
            "Neither covariance nor precision matrix found in posterior. "
            "loo_nonfactor() requires a multivariate normal model with either "
            "a covariance or precision matrix.",
            UserWarning,
            stacklevel=3,
        )
        return False
    if model_type == "student_t" and df_var_name not in names:
        warnings.warn(
            f"Degrees of freedom variable '{df_var_name}' not found in posterior. "
            "Student-t models require a degrees of freedom parameter. "
            "Verify the variable name using the 'df_var_name' parameter.",
            UserWarning,
            stacklevel=3,
        )
        return False
    return True


def _check_obs(n_obs):
    if n_obs > PLA_NONFACTOR_MAX_OBS:
        raise NotImplementedError(
            f"loo_nonfactor supports at most {PLA_NONFACTOR_MAX_OBS} observations on the GPU (got {n_obs})"
        )


def nonfactor_log_lik(y, mu, cov=None, prec=None, df=None, model_type="normal"):
    """The (N, S) conditional log-likelihood ``log p(y_i | y_-i, theta_s)`` of loo_nonfactor.py:466-557 and the (S,) int32
    status word of every draw (``PLA_NF_*`` bits, include/pyloo_amd.h), without the NaN -> -inf replacement of 559-571.

    ``y`` (N,), ``mu`` (S, N), ``cov`` or ``prec`` (S, N, N) -- either is inverted, as in the reference --, ``df`` (S,) for
    ``model_type="student_t"``.  NumPy or CUDA tensors; CUDA in, CUDA out.  Feed the result to ``e_loo``,
    ``loo_predictive_metric`` or ``waic_from_matrix``."""
    if model_type not in _MODEL_TYPES:
        raise ValueError(f"Unsupported model_type: {model_type}. Must be 'normal' or 'student_t'.")
    mat = cov if cov is not None else prec
    if mat is None:
        raise ValueError("pass cov or prec")
    if model_type == "student_t" and df is None:
        raise ValueError("Must provide degrees of freedom variable when model_type='student_t'.")
    S, N = tuple(mu.shape)
    if tuple(y.shape) != (N,) or tuple(mat.shape) != (S, N, N) or (df is not None and model_type == "student_t" and tuple(df.shape) != (S,)):
        raise ValueError(f"expected y (N,), mu (S, N), matrices (S, N, N) and df (S,); got {tuple(y.shape)}, {(S, N)}, "
                         f"{tuple(mat.shape)}" + (f", {tuple(df.shape)}" if df is not None else ""))
    _check_obs(N)
    tensors = [a for a in (y, mu, mat, df) if _is_torch_tensor(a) and a.is_cuda]
    eng = get_engine(tensors[0].device.index if tensors else None)
    return eng.nonfactor_log_lik(y, mu, mat, df if model_type == "student_t" else None, model_type)


def _draw_warnings(flags):
    """The per-draw warnings of loo_nonfactor.py:509-533, in draw order."""
    fl = flags.detach().cpu().numpy() if _is_torch_tensor(flags) else np.asarray(flags)
    for s in np.flatnonzero(fl & (NF_DF_NONPOS | NF_BETA_NONFINITE)):
        if fl[s] & NF_DF_NONPOS:
            yield "df", int(s)
        else:
            yield "beta", int(s)


def _warn_draws(flags, df):
    for kind, s in _draw_warnings(flags):
        if kind == "df":
            df_s = float(df[s])
            warnings.warn(
                f"Sample {s}: Non-positive degrees of freedom ({df_s}). Setting log-likelihood to -inf.",
                UserWarning,
                stacklevel=3,
            )
        else:
            warnings.warn(
                f"Sample {s}: Numerical issues in beta computation. Setting problematic points to -inf.",
                UserWarning,
                stacklevel=3,
            )


def _replace_invalid(ll):
    """loo_nonfactor.py:559-571: NaN -> -inf, one warning when there is a NaN or a -inf."""
    if _is_torch_tensor(ll):
        import torch

        nan = torch.isnan(ll)
        bad = bool((nan | torch.isneginf(ll)).any())
        if bad:
            ll = torch.where(nan, torch.full_like(ll, -np.inf), ll)
    else:
        nan = np.isnan(ll)
        bad = bool(nan.any() or np.isneginf(ll).any())
        if bad:
            ll = np.where(nan, -np.inf, ll)
    if bad:
        warnings.warn(
            "Invalid values detected in log-likelihood calculation. "
            "NaN values have been replaced with -inf. "
            "Points with -inf values will have zero weight in the final calculation.",
            UserWarning,
            stacklevel=3,
        )
    return ll


def _diagnostic_warning(method, agg, good_k, n_samples):
    """loo_nonfactor.py:580-606."""
    from ._capi import AGG_MIN_DIAG, AGG_N_HIGH

    if method == ISMethod.PSIS:
        n_high = int(agg[AGG_N_HIGH])
        if n_high > 0:
            warnings.warn(
                "Estimated shape parameter of Pareto distribution is greater than"
                f" {good_k:.2f} for {n_high} observations. This indicates that"
                " importance sampling may be unreliable. Consider running moment"
                " matching or exact LOO-CV.",
                UserWarning,
                stacklevel=3,
            )
            return True
        return False
    min_ess = float(agg[AGG_MIN_DIAG])
    if min_ess < n_samples * 0.1:
        warnings.warn(
            f"Low effective sample size detected (minimum ESS: {min_ess:.1f})."
            " Importance sampling approximation may be unreliable. Consider using"
            " PSIS.",
            UserWarning,
            stacklevel=3,
        )
        return True
    return False


def _loo_pass(ll, method, reff, scale, scale_value, model_type, pointwise, obs_dim=None, coords=None):
    """loo_nonfactor.py:573-682 on an (N, S) conditional log-likelihood (host array or CUDA tensor)."""
    n_data_points, n_samples = tuple(ll.shape)
    good_k = min(1 - 1 / np.log10(n_samples), 0.7) if n_samples > 1 else 0.7
    res, agg = _engine_pass(ll, method, reff, scale_value, good_k)
    warn = _diagnostic_warning(method, agg, good_k, n_samples)
    summ = _summaries(agg, n_data_points, scale_value)
    data = [summ["elpd_loo"], summ["se"], summ["p_loo"], summ["p_loo_se"], n_samples, n_data_points, warn,
            scale, summ["looic"], summ["looic_se"]]
    index = ["elpd_loo", "se", "p_loo", "p_loo_se", "n_samples", "n_data_points", "warning", "scale", "looic", "looic_se"]
    if pointwise:
        loo_i, diag = res["loo_i"], res["diag"]
        if _is_torch_tensor(loo_i):
            loo_i, diag = loo_i.detach().cpu().numpy(), diag.detach().cpu().numpy()
        dims = (obs_dim,) if obs_dim is not None else ()
        diag_name = "pareto_k" if method == ISMethod.PSIS else "ess"
        data.insert(index.index("scale"), wrap_obs(loo_i, (n_data_points,), dims, coords, "loo_i"))
        index.insert(index.index("scale"), "loo_i")
        data.append(wrap_obs(diag, (n_data_points,), dims, coords, diag_name))
        index.append(diag_name)
        if method == ISMethod.PSIS:
            data.append(good_k)
            index.append("good_k")
    out = ELPDData(data=data, index=index)
    out.attrs = {"is_mvn": True, "model_type": model_type}
    return out


def loo_nonfactor_from_arrays(y, mu, cov=None, prec=None, df=None, model_type="normal", reff=1.0, scale=None, method="psis",
                              pointwise=False):
    """``loo_nonfactor`` on arrays with the draws leading: ``y`` (N,), ``mu`` (S, N), ``cov`` or ``prec`` (S, N, N), ``df`` (S,).
    NumPy or CUDA tensors (the log-likelihood then stays on the device).  Parallels ``loo_from_matrix``."""
    if model_type not in _MODEL_TYPES:
        raise ValueError(f"Unsupported model_type: {model_type}. Must be 'normal' or 'student_t'.")
    scale, scale_value = _scale_value(scale)
    method = parse_method(method)
    ll, flags = nonfactor_log_lik(y, mu, cov, prec, df, model_type)
    if model_type == "student_t":
        _warn_draws(flags, df)
    ll = _replace_invalid(ll)
    return _loo_pass(ll, method, reff, scale, scale_value, model_type, pointwise)


def loo_nonfactor(data, pointwise=None, var_name=None, reff=None, scale=None, method="psis", mu_var_name="mu",
                  cov_var_name=None, prec_var_name=None, model_type="normal", df_var_name="df"):
    """LOO-CV for multivariate normal and Student-t models by importance sampling (loo_nonfactor.py:21-684).

    Same parameters, checks, warnings and ``ELPDData`` rows as ``pyloo.loo_nonfactor``.  ``data`` is anything ArviZ converts,
    or without ArviZ a dict / ``SimpleInferenceData`` with ``posterior = {mu: (chain, draw, N), cov: (chain, draw, N, N),
    df: (chain, draw)}`` and ``observed_data = {y: (N,)}``.  N above 1024 raises ``NotImplementedError``.
    """
    if model_type not in _MODEL_TYPES:
        raise ValueError(f"Unsupported model_type: {model_type}. Must be 'normal' or 'student_t'.")
    warnings.warn(
        f"loo_nonfactor() with model_type='{model_type}' requires the correct model"
        " specification. Using this function with mismatched models will produce"
        " incorrect results.",
        UserWarning,
        stacklevel=2,
    )
    idata = to_inference_data(data)
    _validate_model_structure(idata, mu_var_name, cov_var_name, prec_var_name, model_type, df_var_name)
    if not hasattr(idata, "observed_data"):
        raise TypeError("Must be able to extract an observed_data group from data.")
    if not hasattr(idata, "posterior"):
        raise TypeError("Must be able to extract a posterior group from data.")

    pointwise = rcParams["stats.ic_pointwise"] if pointwise is None else pointwise
    scale, scale_value = _scale_value(scale)

    obs_group = idata.observed_data
    if var_name is None:
        obs_vars = _names(obs_group)
        if len(obs_vars) == 1:
            var_name = obs_vars[0]
        elif not obs_vars:
            raise ValueError("No variables found in observed_data group.")
        else:
            raise ValueError(
                f"Multiple variables found in observed_data: {obs_vars}. "
                "Please specify the response variable using `var_name`."
            )
    try:
        y = obs_group[var_name]
    except KeyError:
        raise ValueError(f"Variable '{var_name}' not found in observed_data group.") from None
    y_name = var_name
    if y.ndim != 1:
        raise ValueError(f"Observed data '{y_name}' must be 1-dimensional (N,). Found shape {y.shape}.")
    n_data_points = y.shape[0]

    post = idata.posterior
    try:
        mu = post[mu_var_name]
    except KeyError:
        raise ValueError(f"Posterior variable '{mu_var_name}' not found.") from None
    cov_matrix = prec_matrix = None
    if cov_var_name:
        try:
            cov_matrix = post[cov_var_name]
        except KeyError:
            raise ValueError(f"Posterior variable '{cov_var_name}' not found.") from None
    elif prec_var_name:
        try:
            prec_matrix = post[prec_var_name]
        except KeyError:
            raise ValueError(f"Posterior variable '{prec_var_name}' not found.") from None
    else:
        try:
            cov_matrix = post["cov"]
            cov_var_name = "cov"
        except KeyError:
            try:
                prec_matrix = post["prec"]
                prec_var_name = "prec"
            except KeyError:
                pass
    if cov_matrix is None and prec_matrix is None:
        raise ValueError(
            "Could not find posterior samples for covariance ('cov') or precision"
            " ('prec') matrix. Specify the variable name using `cov_var_name` or"
            " `prec_var_name`."
        )
    if cov_matrix is not None and prec_matrix is not None:  # (unreachable, as in the reference)
        warnings.warn(
            f"Found both covariance ('{cov_var_name}') and precision"
            f" ('{prec_var_name}') matrices. Using covariance matrix '{cov_var_name}'.",
            UserWarning,
            stacklevel=2,
        )
        prec_matrix = None

    mu_v = np.asarray(_values(mu))
    n_samples = int(np.prod(mu_v.shape[:2])) if mu_v.ndim >= 2 else 0
    mu_stacked_shape = tuple(mu_v.shape[2:]) + (n_samples,)  # the reference's (..., __sample__) view
    for name, mat in ((cov_var_name, cov_matrix), (prec_var_name, prec_matrix)):
        if mat is None:
            continue
        m = np.asarray(_values(mat))
        stacked = tuple(m.shape[2:]) + (int(np.prod(m.shape[:2])),)
        if stacked[-3:] != (n_data_points, n_data_points, mu_stacked_shape[-1]):
            kind = "Covariance" if mat is cov_matrix else "Precision"
            raise ValueError(
                f"{kind} matrix '{name}' shape {stacked[:-1]} "
                f"is incompatible with observed data size {n_data_points} "
                f"and number of samples {mu_stacked_shape[-1]}."
            )
    if len(mu_stacked_shape) < 2 or mu_stacked_shape[-2] != n_data_points:
        raise ValueError(
            f"Mean vector '{mu_var_name}' shape {mu_stacked_shape[:-1]} is incompatible with "
            f"observed data size {n_data_points}."
        )

    if reff is None:
        reff = _relative_efficiency(idata, n_samples)
    method = parse_method(method)
    if method != ISMethod.PSIS:
        warnings.warn(
            f"Using {method.value.upper()} for LOO computation. Note that PSIS is the"
            " recommended method as it is typically more efficient and reliable.",
            UserWarning,
            stacklevel=2,
        )

    obs_dim, coords = _observation_dim(mu, y_name, n_data_points, n_samples, mu_var_name)

    df = None
    if model_type == "student_t":
        try:
            df = post[df_var_name]
        except KeyError:
            raise ValueError(
                f"Degrees of freedom variable '{df_var_name}' not found in posterior. "
                "Please specify the correct variable name using 'df_var_name'."
            ) from None
        df = np.asarray(_values(df)).reshape(n_samples)

    mat = np.asarray(_values(cov_matrix if cov_matrix is not None else prec_matrix))
    mu_v = mu_v.reshape(n_samples, n_data_points)
    mat = mat.reshape(n_samples, n_data_points, n_data_points)
    _check_obs(n_data_points)
    ll, flags = nonfactor_log_lik(np.asarray(_values(y)), mu_v, mat, None, df, model_type)
    if model_type == "student_t":
        _warn_draws(flags, df)
    ll = _replace_invalid(ll)
    return _loo_pass(ll, method, reff, scale, scale_value, model_type, pointwise, obs_dim, coords)


def _observation_dim(mu, y_name, n_data_points, n_samples, mu_var_name):
    """loo_nonfactor.py:445-461: the name of the observation dimension of the stacked mean, with the reference's warning when the
    coordinates do not tell it.  Without xarray the stacked coordinates are those ArviZ gives a bare array: ``{mu}_dim_0`` (N),
    and ``__sample__``, ``chain`` and ``draw`` (all S).  So one coordinate matches N, or four when S == N (then the warning)."""
    if hasattr(mu, "stack") and hasattr(mu, "coords"):
        st = mu.stack(__sample__=("chain", "draw"))
        dims, coords = st.dims, st.coords
        if y_name in coords:
            return y_name, {y_name: coords[y_name].values}
        matching = [d for d, c in coords.items() if c.size == n_data_points]
        if len(matching) == 1:
            return matching[0], {matching[0]: coords[matching[0]].values}
        obs_dim = dims[-2] if len(dims) > 1 else dims[0]
    else:
        obs_dim = f"{mu_var_name}_dim_0"
        if n_samples != n_data_points:
            return obs_dim, {obs_dim: np.arange(n_data_points)}
    warnings.warn(
        f"Could not reliably determine the observation dimension name. Assuming '{obs_dim}'.",
        UserWarning,
        stacklevel=3,
    )
    return obs_dim, None
