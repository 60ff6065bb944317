"""PSIS-LOO for generalised linear models from the design matrix and the draws -- the ``(n_obs, n_draws)`` log-likelihood matrix is
never held (R-loo's ``loo.function``; the reference's ``approximations/plpd.py:76-88`` takes a ``log_likelihood_fn`` for the same
reason).  For a GLM the matrix is a function of three small objects: ``X`` (N, P), the coefficient draws ``beta`` (S, P) and at most
one auxiliary parameter per draw.  ``pla_glm`` (csrc/pla_glm.h) writes it one block of rows at a time on the f64 matrix cores and
the unchanged PSIS-LOO pass consumes each block before the next overwrites it.

* ``glm_log_lik``            the ``(m, S)`` matrix of all rows or of ``rows=`` -- for ``waic_from_matrix``, ``loo_pit``, ... of a subset
* ``glm_plpd``               ``[N]``, the log-likelihood at the posterior mean: a real point log predictive density
* ``loo_glm_from_design``    ``ELPDData`` as ``loo_from_matrix`` packs it
* ``loo_glm``                the same with ``beta`` taken from the ``posterior`` group of ``idata``
* ``loo_subsample_glm``      subsampled LOO at an N for which no matrix can exist

Families: ``"gaussian"`` (identity link, ``sigma`` per draw), ``"bernoulli"`` and ``"binomial"`` (logit link, or
``link="probit"``), ``"poisson"`` (log link), ``"negbinomial"`` (log link, ``phi`` per draw: NB2 with mean ``mu = exp(eta)`` and
variance ``mu + mu^2 / phi``) and ``"gamma"`` (log link, ``shape`` per draw: mean ``exp(eta)``, rate ``shape / mean``).  ``link=None``
is the canonical link named above.  NumPy ``X`` -> NumPy results; a torch CUDA ``X`` -> everything is moved to its device and stays there.  The fronts compute
the per-observation and per-draw constants the kernel is handed (``obs_const``, ``draw_const``): ``scipy.special.gammaln`` /
``np.log`` on the host, ``torch.lgamma`` / ``torch.log`` on the device.

Multilevel models: ``groups=`` is a sequence of at most eight group-level terms, ``(index, draws)`` -- a varying intercept -- or
``(index, draws, z)`` -- a varying slope on the covariate ``z`` [N] --, with ``index`` [N] integers in ``[0, G)`` and ``draws``
(S, G).  The linear predictor becomes ``((X beta + offset) + z_0 u_0[:, index_0]) + z_1 u_1[:, index_1] + ...``, every product and
sum rounded once in the order given (``pla_glm_grouped``, csrc/pla_glm_terms.h): another order of the terms is another order of
additions and may differ in the last bit.  A term over a product of factors takes the joint index, formed by the caller.
"""

import warnings

import numpy as np

from .base import ISMethod, parse_method, tail_count_for
from .engine import _is_torch_tensor, get_engine
from .loo import _diagnostic_warning, _pack, _scale_value, _summaries
from .loo_influence import _posterior_columns
from .loo_subsample import (APPROXIMATIONS, ESTIMATORS, SubsampleIndices, _estimate_and_pack, _to_host, subsample_indices)
from .utils import to_inference_data

__all__ = ["glm_log_lik", "glm_plpd", "loo_glm_from_design", "loo_glm", "loo_subsample_glm"]

FAMILIES = ("gaussian", "bernoulli", "binomial", "poisson", "negbinomial", "gamma")
MAX_PREDICTORS = 256
MAX_TERMS = 8
_ENGINE_FAMILY = {"gaussian": "gaussian", "bernoulli": "binomial", "binomial": "binomial", "poisson": "poisson",
                  "negbinomial": "negbinomial", "gamma": "gamma"}
_CANONICAL_LINK = {"gaussian": "identity", "bernoulli": "logit", "binomial": "logit", "poisson": "log", "negbinomial": "log", "gamma": "log"}
_SCALE_ARGUMENT = {"gaussian": "sigma", "negbinomial": "phi", "gamma": "shape"}  # what travels as the engine's draw_scale
_HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def _all(flag):
    return bool(flag.all().item()) if hasattr(flag, "item") else bool(np.all(flag))


def _engine_family(family, link=None):
    """The engine's name of a family of FAMILIES under ``link``: None and the canonical link are one path, ``"probit"`` goes on the
    two binomial families."""
    probit_too = family in ("bernoulli", "binomial")
    if link is None or link == _CANONICAL_LINK[family]:
        return _ENGINE_FAMILY[family]
    if link == "probit" and probit_too:
        return "binomial_probit"
    takes = f"None, {_CANONICAL_LINK[family]!r}" + (" or 'probit'" if probit_too else "")
    raise ValueError(f"link of the {family} family must be {takes}, got {link!r}")


def _draw_const(family, scale):
    """The per-draw constant of a family with a scale per draw, NumPy or torch: ``-0.5 log(2 pi) - log(sigma)`` for the Gaussian,
    ``a log(a) - lgamma(a)`` for ``a`` = ``phi`` of the negative binomial or the gamma family's ``shape``."""
    if _is_torch_tensor(scale):
        import torch

        lgamma, log = torch.lgamma, torch.log
    else:
        from scipy.special import gammaln as lgamma

        log = np.log
    if family == "gaussian":
        return -_HALF_LOG_2PI - log(scale)
    return scale * log(scale) - lgamma(scale)


def _prepare(X, y, beta, family, sigma, offset, trials, phi=None, shape=None, link=None):
    """Every check of the fronts, before any engine call, and the vectors the engine is handed -- in the memory space of ``X``.
    Returns ``(X, beta, dict(y, offset, trials, obs_const, draw_scale, draw_const))``."""
    if family not in FAMILIES:
        raise ValueError(f"family must be one of {', '.join(FAMILIES)}, got {family!r}")
    _engine_family(family, link)
    tensor = _is_torch_tensor(X)
    if tensor:
        import torch

        dev = X.device
        vec = lambda v: torch.as_tensor(v, device=dev).to(torch.float64)  # noqa: E731
        X, beta = X.to(torch.float64), vec(beta)
        finite, floor, lgamma, log = torch.isfinite, torch.floor, torch.lgamma, torch.log
        ndim = lambda a: a.dim()  # noqa: E731
    else:
        from scipy.special import gammaln as lgamma

        vec = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
        X, beta = vec(X), vec(beta)
        finite, floor, log = np.isfinite, np.floor, np.log
        ndim = lambda a: a.ndim  # noqa: E731
    if ndim(X) != 2:
        raise ValueError(f"X must be a 2-D (n_obs, P) array, got shape {tuple(X.shape)}")
    n, p = X.shape
    if ndim(beta) != 2 or beta.shape[1] != p:
        raise ValueError(f"beta must be (n_draws, P) with P = {p} columns as X has, got shape {tuple(beta.shape)}")
    s = beta.shape[0]
    if p < 1 or p > MAX_PREDICTORS:
        raise ValueError(f"X has {p} columns; between 1 and {MAX_PREDICTORS} predictors are supported")
    if s < 1:
        raise ValueError("beta has no draws")
    y = vec(y).reshape(-1)
    if y.shape[0] != n:
        raise ValueError(f"y needs {n} values, one per row of X, got {y.shape[0]}")
    if offset is not None:
        offset = vec(offset).reshape(-1)
        if offset.shape[0] != n:
            raise ValueError(f"offset needs {n} values, got {offset.shape[0]}")
    if family == "gaussian":
        if sigma is None:
            raise ValueError("the gaussian family needs sigma, one value per draw")
        sigma = vec(sigma).reshape(-1)
        if sigma.shape[0] != s:
            raise ValueError(f"sigma needs {s} values, one per draw, got {sigma.shape[0]}")
        if not _all(finite(sigma) & (sigma > 0)):
            raise ValueError("sigma must be finite and positive")
    elif sigma is not None:
        raise ValueError(f"sigma belongs to the gaussian family, not to {family!r}")
    for name, owner, value in (("phi", "negbinomial", phi), ("shape", "gamma", shape)):
        if family != owner:
            if value is not None:
                raise ValueError(f"{name} belongs to the {owner} family, not to {family!r}")
            continue
        if value is None:
            raise ValueError(f"the {owner} family needs {name}, one value per draw")
        value = vec(value).reshape(-1)
        if value.shape[0] != s:
            raise ValueError(f"{name} needs {s} values, one per draw, got {value.shape[0]}")
        if not _all(finite(value) & (value > 0)):
            raise ValueError(f"{name} must be finite and positive")
        sigma = value  # (the engine's draw_scale)
    if family == "binomial":
        if trials is None:
            raise ValueError("the binomial family needs trials (family='bernoulli' is one trial each)")
        trials = vec(trials).reshape(-1)
        if trials.shape[0] != n:
            raise ValueError(f"trials needs {n} values, got {trials.shape[0]}")
        if not _all(finite(trials) & (trials >= 0) & (floor(trials) == trials)):
            raise ValueError("trials must be non-negative integers")
    elif trials is not None:
        raise ValueError(f"trials belongs to the binomial family, not to {family!r}")
    if family == "gamma":
        if not _all(finite(y) & (y > 0)):
            raise ValueError("y of the gamma family must be finite and positive")
    elif family != "gaussian":
        if not _all(finite(y) & (y >= 0) & (floor(y) == y)):
            raise ValueError(f"y of the {family} family must be non-negative integers")
        if family == "bernoulli" and not _all(y <= 1):
            raise ValueError("y exceeds trials: the bernoulli family takes 0 or 1")
        if family == "binomial" and not _all(y <= trials):
            raise ValueError("y exceeds trials")
    for name, a in (("X", X), ("beta", beta), ("offset", offset)):
        if a is not None and not _all(finite(a)):
            raise ValueError(f"{name} holds values that are not finite")
    obs_const = draw_const = None
    if family == "binomial":
        obs_const = (lgamma(trials + 1.0) - lgamma(y + 1.0)) - lgamma(trials - y + 1.0)
    elif family in ("poisson", "negbinomial"):
        obs_const = -lgamma(y + 1.0)
    elif family == "gamma":
        obs_const = log(y)
    if family in _SCALE_ARGUMENT:
        draw_const = _draw_const(family, sigma)
    return X, beta, {"y": y, "offset": offset, "trials": trials, "obs_const": obs_const, "draw_scale": sigma, "draw_const": draw_const}


def _prepare_groups(groups, X, n_draws):
    """Every check of the group-level terms, before any engine call: ``[(index, draws, z), ...]`` in the memory space of ``X``, or
    None when there is no term (``groups`` None or empty: the call without terms)."""
    if groups is None:
        return None
    groups = list(groups)
    if not groups:
        return None
    if len(groups) > MAX_TERMS:
        raise ValueError(f"at most {MAX_TERMS} group-level terms are supported, got {len(groups)}")
    n = X.shape[0]
    tensor = _is_torch_tensor(X)
    if tensor:
        import torch
    out = []
    for t, term in enumerate(groups):
        if not isinstance(term, (tuple, list)) or len(term) not in (2, 3):
            raise ValueError(f"groups[{t}] must be (index, draws) or (index, draws, z)")
        index, draws, z = (*term, None)[:3]
        if tensor:
            index = torch.as_tensor(index, device=X.device).reshape(-1)
            integer = not (index.is_floating_point() or index.is_complex() or index.dtype == torch.bool)
            draws = torch.as_tensor(draws, device=X.device).to(torch.float64)
            z = None if z is None else torch.as_tensor(z, device=X.device).to(torch.float64).reshape(-1)
            finite, ndim = torch.isfinite, draws.dim()
        else:
            index = np.asarray(index).reshape(-1)
            integer = np.issubdtype(index.dtype, np.integer)
            draws = np.asarray(draws, dtype=np.float64)
            z = None if z is None else np.asarray(z, dtype=np.float64).reshape(-1)
            finite, ndim = np.isfinite, draws.ndim
        if not integer:
            raise TypeError(f"groups[{t}]: index must hold integers, got dtype {index.dtype}")
        if index.shape[0] != n:
            raise ValueError(f"groups[{t}]: index needs {n} values, one per row of X, got {index.shape[0]}")
        if ndim != 2 or draws.shape[0] != n_draws:
            raise ValueError(f"groups[{t}]: draws must be a 2-D (n_draws, G) array with n_draws = {n_draws} rows as beta has, "
                             f"got shape {tuple(draws.shape)}")
        g = draws.shape[1]
        if g == 0:
            raise ValueError(f"groups[{t}]: draws has no groups (G = 0)")
        if n > 0:
            lo, hi = int(index.min()), int(index.max())
            if lo < 0 or hi >= g:
                raise ValueError(f"groups[{t}]: index must lie in [0, {g}), got range [{lo}, {hi}]")
        if z is not None and z.shape[0] != n:
            raise ValueError(f"groups[{t}]: z needs {n} values, got {z.shape[0]}")
        for name, a in (("draws", draws), ("z", z)):
            if a is not None and not _all(finite(a)):
                raise ValueError(f"groups[{t}]: {name} holds values that are not finite")
        out.append((index, draws, z))
    return out


def _with_groups(terms):
    """The keyword the engine is handed: none at all without terms -- the existing call with the existing arguments."""
    return {} if terms is None else {"groups": terms}


def _groups_at(terms, pick):
    """The terms with ``pick`` applied to the draws of each: the posterior mean, a thinned set of draws."""
    return None if terms is None else [(index, pick(draws), z) for index, draws, z in terms]


def _engine_of(X):
    return get_engine(X.device.index if _is_torch_tensor(X) else None)


def _check_reff(reff):
    if isinstance(reff, bool) or not isinstance(reff, (int, float, np.integer, np.floating)) or not np.isfinite(reff) or reff <= 0:
        raise ValueError(f"reff must be a positive float here (a vector and None are not supported), got {reff!r}")
    return float(reff)


def glm_log_lik(X, y, beta, family, sigma=None, offset=None, trials=None, rows=None, linpred=False, groups=None, *, phi=None,
                shape=None, link=None):
    """The ``(m, S)`` log-likelihood matrix of a GLM -- of all N rows of ``X``, or of ``rows`` (any order, repeats allowed) -- or,
    with ``linpred=True``, the posterior linear predictor ``X @ beta.T + offset`` (plus the terms of ``groups``, see the module's
    text).  ``phi`` [S]: the dispersion of ``family="negbinomial"``; ``shape`` [S]: the shape of ``family="gamma"``; ``link``: None
    (canonical) or ``"probit"`` on the binomial families.  torch on the device for a CUDA ``X``, NumPy otherwise."""
    Xc, bc, v = _prepare(X, y, beta, family, sigma, offset, trials, phi, shape, link)
    terms = _prepare_groups(groups, Xc, bc.shape[0])
    eng = _engine_of(Xc)
    if linpred:
        return eng.glm(Xc, bc, "linpred", offset=v["offset"], rows=rows, **_with_groups(terms))
    return eng.glm(Xc, bc, _engine_family(family, link), rows=rows, **v, **_with_groups(terms))


def _posterior_mean(beta, v, family="gaussian"):
    """``beta`` and the per-draw vectors of ``v`` at the posterior mean: one draw.  The constant of the draw is evaluated again at
    the mean of ``sigma`` / ``phi`` / ``shape``."""
    b1 = beta.mean(0).reshape(1, -1)
    v1 = dict(v)
    if v["draw_scale"] is not None:
        s1 = v["draw_scale"].mean().reshape(1)
        v1["draw_scale"] = s1
        v1["draw_const"] = _draw_const(family, s1)
    return b1, v1


def _mean_draw(draws):
    return draws.mean(0).reshape(1, -1)


def glm_plpd(X, y, beta, family, sigma=None, offset=None, trials=None, groups=None, *, phi=None, shape=None, link=None):
    """``[N]``: the log-likelihood of every observation at the posterior mean of ``beta`` (of ``sigma`` / ``phi`` / ``shape``, and of
    the draws of every term of ``groups``) -- the point log predictive density of Magnusson et al. (2019), the matrix mode with one
    draw."""
    Xc, bc, v = _prepare(X, y, beta, family, sigma, offset, trials, phi, shape, link)
    terms = _prepare_groups(groups, Xc, bc.shape[0])
    b1, v1 = _posterior_mean(bc, v, family)
    return _engine_of(Xc).glm(Xc, b1, _engine_family(family, link), **v1, **_with_groups(_groups_at(terms, _mean_draw))).reshape(-1)


def loo_glm_from_design(X, y, beta, family, sigma=None, offset=None, trials=None, reff=1.0, scale=None, method="psis", pointwise=False,
                        rows=None, groups=None, *, phi=None, shape=None, link=None):
    """PSIS-LOO of a GLM from its design matrix ``X`` (N, P), the outcomes ``y`` [N] and the draws ``beta`` (S, P), in one fused
    pass: per block of observations the log-likelihood is generated into a bounded buffer and consumed by the LOO kernels.
    Returns the ``ELPDData`` of ``loo_from_matrix`` on the materialised matrix -- the same keys, warnings and texts.  ``rows``:
    the pass over these observations only.  ``groups``: the group-level terms of a multilevel model (the module's text).  ``phi``,
    ``shape``, ``link``: as ``glm_log_lik`` takes them."""
    method = parse_method(method)
    scale, scale_value = _scale_value(scale)
    reff = _check_reff(reff)
    Xc, bc, v = _prepare(X, y, beta, family, sigma, offset, trials, phi, shape, link)
    terms = _prepare_groups(groups, Xc, bc.shape[0])
    n_samples = bc.shape[0]
    if n_samples < 2:
        raise ValueError("PSIS-LOO needs at least two draws")
    good_k = min(1 - 1 / np.log10(n_samples), 0.7)
    M = tail_count_for(n_samples, reff) if method == ISMethod.PSIS else 0
    if method == ISMethod.PSIS and M + 1 > n_samples:
        raise IndexError(f"index {-M - 1} is out of bounds for axis 0 with size {n_samples}")
    res = _engine_of(Xc).glm(Xc, bc, _engine_family(family, link), rows=rows, mode="loo", tail_count=M, method=method.value,
                             scale_value=scale_value, good_k=good_k, **v, **_with_groups(terms))
    if int(res["n_replaced"]) > 0:
        warnings.warn("NaN values detected in log-likelihood. These will be ignored in the LOO calculation.", UserWarning, stacklevel=2)
    agg = _to_host(res["agg"])
    n_data_points = int(agg[0])
    warn = _diagnostic_warning(method, agg, good_k, n_samples)
    summ = _summaries(agg, n_data_points, scale_value)
    out = _pack(summ, n_samples, n_data_points, warn, scale, method, good_k, pointwise, res["loo_i"], res["diag"])
    out.method = method.value
    return out


def loo_glm(idata, X, y, family, var_names, sigma_name=None, var_name=None, offset=None, trials=None, reff=1.0, scale=None,
            method="psis", pointwise=False, rows=None, group_terms=None, *, phi_name=None, shape_name=None, link=None):
    """``loo_glm_from_design`` with the draws taken from ``idata``: the columns of ``beta`` are the variables ``var_names`` of the
    ``posterior`` group, each flattened over its own dimensions, in the order given; their count must equal ``X.shape[1]``.
    ``sigma_name``: the posterior variable that holds the Gaussian scale; ``phi_name`` / ``shape_name``: the one that holds the
    dispersion of the negative binomial / the shape of the gamma family; ``link``: as ``glm_log_lik`` takes it.  ``y=None`` reads ``observed_data[var_name]``.
    ``group_terms``: a sequence of ``(name, index)`` or ``(name, index, z)`` -- the posterior variable ``name`` of shape
    ``(chain, draw, G)`` holds the group effects of the term --, handed on as ``groups`` in the order given."""
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
    groups = None
    if group_terms is not None:
        groups = []
        for t, term in enumerate(group_terms):
            if not isinstance(term, (tuple, list)) or len(term) not in (2, 3) or not isinstance(term[0], str):
                raise ValueError(f"group_terms[{t}] must be (name, index) or (name, index, z)")
            draws, _, _ = _posterior_columns(data, [term[0]])
            groups.append((term[1], draws, *term[2:]))
    return loo_glm_from_design(X, y, beta, family, sigma=per_draw["sigma_name"], offset=offset, trials=trials, reff=reff, scale=scale,
                               method=method, pointwise=pointwise, rows=rows, groups=groups, phi=per_draw["phi_name"],
                               shape=per_draw["shape_name"], link=link)


def loo_subsample_glm(X, y, beta, family, observations=100, loo_approximation="plpd", estimator="diff_srs",
                      loo_approximation_draws=None, sigma=None, offset=None, trials=None, reff=1.0, scale=None, pointwise=False,
                      groups=None, *, phi=None, shape=None, link=None):
    """Subsampled PSIS-LOO (Magnusson et al. 2019, 2020) of a GLM without its matrix.  The approximation for ALL observations is
    ``"plpd"`` -- ``glm_plpd``, the log-likelihood at the posterior mean -- or ``"lpd"``, the ``lppd_i`` of a fused pass over
    (thinned) draws; the subsample is drawn by ``subsample_indices``; only the ``m`` sampled rows of the matrix are generated
    (``glm_log_lik(rows=idx)``) and go through PSIS-LOO and the variance over draws.  Estimators, warnings and result layout are
    those of ``loo_subsample_from_matrix``.  ``groups``: the group-level terms of a multilevel model (the module's text).  ``phi``,
    ``shape``, ``link``: as ``glm_log_lik`` takes them.  Returns ``(ELPDData, SubsampleIndices, Estimate)``."""
    kind = str(loo_approximation).lower()
    if kind not in ("plpd", "lpd"):
        raise ValueError(f"Invalid loo_approximation '{loo_approximation}'. Must be one of: plpd, lpd (of {', '.join(APPROXIMATIONS)})")
    est = str(estimator).lower()
    if est not in ESTIMATORS:
        raise ValueError(f"Invalid estimator '{estimator}'. Must be one of: {', '.join(ESTIMATORS)}")
    scale, scale_value = _scale_value(scale)
    reff = _check_reff(reff)
    Xc, bc, v = _prepare(X, y, beta, family, sigma, offset, trials, phi, shape, link)
    terms = _prepare_groups(groups, Xc, bc.shape[0])
    n_data_points, n_samples = Xc.shape[0], bc.shape[0]
    if isinstance(observations, (int, np.integer)) and not isinstance(observations, bool):
        if observations <= 0 or observations > n_data_points:
            raise ValueError(f"Number of observations must be between 1 and {n_data_points}, got {observations}")
    elif isinstance(observations, np.ndarray):
        if not np.issubdtype(observations.dtype, np.integer):
            raise TypeError("observations array must contain integers")
        if observations.min() < 0 or observations.max() >= n_data_points:
            raise ValueError(f"Observation indices must be between 0 and {n_data_points - 1}, "
                             f"got range [{observations.min()}, {observations.max()}]")
    else:
        raise TypeError("observations must be an integer or an array of integers")
    if n_samples < 2:
        raise ValueError("PSIS-LOO needs at least two draws")
    good_k = min(1 - 1 / np.log10(n_samples), 0.7)
    M = tail_count_for(n_samples, reff)
    if M + 1 > n_samples:
        raise IndexError(f"index {-M - 1} is out of bounds for axis 0 with size {n_samples}")
    if loo_approximation_draws is not None and loo_approximation_draws > n_samples:
        raise ValueError(f"Requested {loo_approximation_draws} draws but only {n_samples} are available")

    eng = _engine_of(Xc)
    fam = _engine_family(family, link)
    if kind == "plpd":
        b1, v1 = _posterior_mean(bc, v, family)
        approx = _to_host(eng.glm(Xc, b1, fam, **v1, **_with_groups(_groups_at(terms, _mean_draw)))).reshape(-1).astype(np.float64)
    else:
        bt, vt, tt = bc, v, terms
        if loo_approximation_draws is not None:  # approximations/base.py:60-102: evenly spaced draws
            cols = np.linspace(0, n_samples - 1, loo_approximation_draws, dtype=int)
            if _is_torch_tensor(bc):
                import torch

                cols = torch.as_tensor(cols, device=bc.device)
            bt = bc[cols]
            vt = dict(v)
            for k in ("draw_scale", "draw_const"):
                vt[k] = None if v[k] is None else v[k][cols]
            tt = _groups_at(terms, lambda draws: draws[cols])
        approx = _to_host(eng.glm(Xc, bt, fam, mode="loo", method="sis", aggregate=False, **vt, **_with_groups(tt))["lppd_i"]).astype(np.float64)
    if isinstance(observations, np.ndarray):
        indices = SubsampleIndices(idx=observations, m_i=np.ones_like(observations))
    else:
        indices = subsample_indices(est, approx, int(observations))

    sub = eng.glm(Xc, bc, fam, rows=indices.idx, **v, **_with_groups(terms))  # the m sampled rows, draws fastest
    res = eng.psis_loo(sub, M, ISMethod.PSIS.value, scale_value, good_k, aggregate=False)
    var_m = eng.waic(sub, 1.0, aggregate=False)["var_i"]
    loo_m = _to_host(res["loo_i"]).astype(np.float64)
    khat = _to_host(res["diag"]).astype(np.float64)
    p_loo_m = _to_host(var_m).astype(np.float64)
    return _estimate_and_pack(est, approx, indices, loo_m, khat, p_loo_m, n_data_points, n_samples, good_k, scale, pointwise)
