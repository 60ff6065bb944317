"""Cluster-marginal LOO for multilevel GLMs: leave-one-cluster-out with the left-out cluster's own effect integrated out of the
likelihood (Merkle, Furr & Rabe-Hesketh 2019; the integrated LOO of the roaches case study).  The conditional fronts of
``loo_glm`` leave out one observation with every group effect held at its draws -- with a few observations per group, or one effect
per observation, those importance weights have Pareto k far above 0.7.  Here every observation ``i`` belongs to one cluster
``c(i)``, its linear predictor is ``rest[i, s] + z_i u`` with ``rest`` what ``loo_glm`` computes (``X beta + offset`` and the
conditional terms of ``groups=``) and ``u | draw s ~ N(0, tau_s^2)``, and

    mll[c, s] = log  integral  prod_{i in c} p(y_i | rest[i, s] + z_i u) N(u; 0, tau_s^2) du

is evaluated by adaptive Gauss-Hermite quadrature on ``n_nodes`` nodes of the cluster (``pla_glm_marginal``,
csrc/pla_glm_marginal.h): with ``x_q, w_q`` the physicists' rule, ``node[c, q] = loc_c + sqrt(2) scale_c x_q`` and
``logw[c, q] = log w_q + x_q^2 + log(sqrt(2) scale_c)``.  With the draws ``u`` (S, C) of the effect, ``loc_c`` and ``scale_c`` are the
posterior mean and standard deviation of ``u[:, c]``; without, ``loc_c = 0`` and ``scale_c = mean(tau)``.  The (C, S) result is an
ordinary log-likelihood matrix with one row per cluster, in the order of ``group_index(cluster).labels``: PSIS-LOO over it is
leave-one-cluster-out on the marginal likelihood, and with one cluster per observation it is integrated LOO.

* ``glm_marginal_log_lik``            the ``(C, S)`` matrix
* ``loo_glm_marginal_from_design``    ``ELPDData`` as ``loo_group_from_matrix`` packs it, from one fused pass
* ``loo_glm_marginal``                the same with ``beta``, ``u`` and ``tau`` taken from the ``posterior`` group of ``idata``

One integrated effect per cluster, a zero-mean normal prior, f64, a scalar ``reff``.  NumPy ``X`` -> NumPy results; a torch CUDA
``X`` -> everything is moved to its device and stays there.
"""

import warnings

import numpy as np

from .base import ISMethod, parse_method, tail_count_for
from .engine import _is_torch_tensor
from .loo import _scale_value
from .loo_glm import _ENGINE_FAMILY, _all, _engine_family, _check_reff, _engine_of, _prepare, _prepare_groups, _with_groups
from .loo_group import _diagnostic_warning, _logo_array, _method_warning, _nan_warning, _pack, _summaries, group_index
from .loo_influence import _posterior_columns
from .loo_subsample import _to_host
from .utils import to_inference_data

__all__ = ["glm_marginal_log_lik", "loo_glm_marginal_from_design", "loo_glm_marginal"]

MAX_NODES = 32


def gauss_hermite_nodes(loc, scale, n_nodes):
    """``(nodes, log_weights)``, each (C, n_nodes), of the adaptive rule centred at ``loc`` [C] with spread ``scale`` [C] (NumPy)."""
    x, w = np.polynomial.hermite.hermgauss(int(n_nodes))
    loc, scale = np.asarray(loc, dtype=np.float64).reshape(-1, 1), np.asarray(scale, dtype=np.float64).reshape(-1, 1)
    root2_scale = np.sqrt(2.0) * scale
    return loc + root2_scale * x[None, :], (np.log(w) + x * x)[None, :] + np.log(root2_scale)


def _prepare_marginal(X, n_draws, cluster, tau, z, u, loc, scale, n_nodes, groups):
    """Every check of the marginal fronts, before any engine call, in the memory space of ``X`` (as ``_prepare`` left it).
    Returns ``(index, tau, z, nodes, log_weights)``."""
    n = X.shape[0]
    tensor = _is_torch_tensor(X)
    if tensor:
        import torch

        vec = lambda v: torch.as_tensor(v, device=X.device).to(torch.float64)  # noqa: E731
        finite = torch.isfinite
        cl = torch.as_tensor(cluster, device=X.device).reshape(-1)
        integer = not (cl.is_floating_point() or cl.is_complex() or cl.dtype == torch.bool)
    else:
        vec = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
        finite = np.isfinite
        cl = np.asarray(cluster).reshape(-1)
        integer = np.issubdtype(cl.dtype, np.integer)
    if not integer:
        raise TypeError(f"cluster must hold integers, got dtype {cl.dtype}")
    if cl.shape[0] != n:
        raise ValueError(f"cluster needs {n} values, one per row of X, got {cl.shape[0]}")
    if isinstance(n_nodes, bool) or not isinstance(n_nodes, (int, np.integer)) or not 1 <= n_nodes <= MAX_NODES:
        raise ValueError(f"n_nodes must be an integer between 1 and {MAX_NODES}, got {n_nodes!r}")
    tau = vec(tau).reshape(-1)
    if tau.shape[0] != n_draws:
        raise ValueError(f"tau needs {n_draws} values, one per draw, got {tau.shape[0]}")
    if not _all(finite(tau) & (tau > 0)):
        raise ValueError("tau must be finite and positive")
    if z is not None:
        z = vec(z).reshape(-1)
        if z.shape[0] != n:
            raise ValueError(f"z needs {n} values, got {z.shape[0]}")
        if not _all(finite(z)):
            raise ValueError("z holds values that are not finite")
    if u is not None and (loc is not None or scale is not None):
        raise ValueError("loc and scale are computed from u: give u, or loc and scale, not both")
    index = group_index(cl)
    n_clusters = index.n_groups
    if u is not None:
        u = vec(u)
        if len(u.shape) != 2 or u.shape[0] != n_draws or u.shape[1] != n_clusters:
            raise ValueError(f"u must be (n_draws, C) = ({n_draws}, {n_clusters}), one column per cluster in the order of its sorted "
                             f"labels, got shape {tuple(u.shape)}")
        if n_draws < 2:
            raise ValueError("u needs at least two draws for its standard deviation")
        if not _all(finite(u)):
            raise ValueError("u holds values that are not finite")
        loc = _to_host(u.mean(0)).astype(np.float64)
        scale = _to_host(u.std(0, unbiased=True) if tensor else u.std(0, ddof=1)).astype(np.float64)
        if not np.all(scale > 0):
            raise ValueError("u does not vary within a cluster: its standard deviation must be positive")
    else:
        loc = np.zeros(n_clusters) if loc is None else np.asarray(_to_host(loc), dtype=np.float64).reshape(-1)
        if loc.shape[0] != n_clusters:
            raise ValueError(f"loc needs {n_clusters} values, one per cluster, got {loc.shape[0]}")
        if not np.all(np.isfinite(loc)):
            raise ValueError("loc holds values that are not finite")
        if scale is None:
            scale = np.full(n_clusters, float(tau.mean()))
        else:
            scale = np.asarray(_to_host(scale), dtype=np.float64).reshape(-1)
            if scale.shape[0] != n_clusters:
                raise ValueError(f"scale needs {n_clusters} values, one per cluster, got {scale.shape[0]}")
            if not np.all(np.isfinite(scale) & (scale > 0)):
                raise ValueError("scale must be finite and positive")
    for t, term in enumerate(groups or ()):
        same = term[0].shape == cl.shape and _all(term[0] == cl)
        if same:
            warnings.warn(f"cluster is also the index of groups[{t}]: that effect is held at its draws and integrated out as well -- "
                          "it is counted twice", UserWarning, stacklevel=3)
    nodes, logw = gauss_hermite_nodes(loc, scale, n_nodes)
    if tensor:
        nodes, logw = vec(nodes), vec(logw)
    return index, tau, z, nodes, logw


MARGINAL_FAMILIES = ("gaussian", "bernoulli", "binomial", "poisson")


def _setup(X, y, beta, family, cluster, tau, z, u, loc, scale, n_nodes, sigma, offset, trials, groups, link=None):
    if family in ("negbinomial", "gamma") or link == "probit":
        what = f"the {family} family" if link != "probit" else "the probit link"
        raise ValueError(f"the cluster-marginal pass takes the families {', '.join(MARGINAL_FAMILIES)} with their canonical links, "
                         f"not {what}")
    Xc, bc, v = _prepare(X, y, beta, family, sigma, offset, trials)
    terms = _prepare_groups(groups, Xc, bc.shape[0])
    _engine_family(family, link)
    index, tau, z, nodes, logw = _prepare_marginal(Xc, bc.shape[0], cluster, tau, z, u, loc, scale, n_nodes, terms)
    return Xc, bc, v, terms, index, dict(tau=tau, z=z, nodes=nodes, log_weights=logw)


def glm_marginal_log_lik(X, y, beta, family, cluster, tau, z=None, u=None, loc=None, scale=None, n_nodes=15, sigma=None, offset=None,
                         trials=None, groups=None, *, link=None):
    """The ``(C, S)`` marginal log-likelihood of the clusters of ``cluster`` [N] (integer labels), rows in the order of
    ``group_index(cluster).labels``.  ``tau`` [S]: the scale of the integrated effect per draw; ``z`` [N]: its covariate (None: an
    intercept); ``u`` (S, C): its draws, which centre the nodes -- or ``loc`` / ``scale`` [C] (the module's text); ``groups``: the
    conditional terms of ``loo_glm``, held at their draws; ``link``: None or the canonical link of the family (the probit link,
    like the negative binomial and gamma families, is not integrated here).  torch on the device for a CUDA ``X``, NumPy otherwise."""
    Xc, bc, v, terms, index, q = _setup(X, y, beta, family, cluster, tau, z, u, loc, scale, n_nodes, sigma, offset, trials, groups, link)
    return _engine_of(Xc).glm_marginal(Xc, bc, _ENGINE_FAMILY[family], index, **q, **v, **_with_groups(terms))


def loo_glm_marginal_from_design(X, y, beta, family, cluster, tau, z=None, u=None, loc=None, node_scale=None, n_nodes=15, sigma=None,
                                 offset=None, trials=None, groups=None, reff=1.0, scale=None, method="psis", pointwise=False, *, link=None):
    """Leave-one-cluster-out PSIS-LOO on the marginal likelihood in one fused pass: per block of members the linear predictor is
    generated into a bounded buffer, turned into rows of ``mll`` and consumed by the LOO kernels.  Returns the ``ELPDData`` of
    ``loo_group_from_matrix`` on ``glm_marginal_log_lik(...)`` with one group per row -- the same keys, warnings and texts.
    ``node_scale`` is ``glm_marginal_log_lik``'s ``scale`` (``scale`` here is the scale of the ELPD)."""
    method = parse_method(method)
    scale, scale_value = _scale_value(scale)
    reff = _check_reff(reff)
    Xc, bc, v, terms, index, q = _setup(X, y, beta, family, cluster, tau, z, u, loc, node_scale, n_nodes, sigma, offset, trials, groups,
                                        link)
    n_samples = bc.shape[0]
    if n_samples < 2:
        raise ValueError("PSIS-LOO needs at least two draws")
    good_k = min(1 - 1 / np.log10(n_samples), 0.7)
    M = tail_count_for(n_samples, reff) if method == ISMethod.PSIS else 0
    if method == ISMethod.PSIS and M + 1 > n_samples:
        raise IndexError(f"index {-M - 1} is out of bounds for axis 0 with size {n_samples}")
    res = _engine_of(Xc).glm_marginal(Xc, bc, _ENGINE_FAMILY[family], index, **q, mode="loo", tail_count=M, method=method.value,
                                      scale_value=scale_value, good_k=good_k, **v, **_with_groups(terms))
    _nan_warning(res["n_replaced"])
    _method_warning(method)
    agg = _to_host(res["agg"])
    warn = _diagnostic_warning(method, agg, good_k, n_samples)
    summ = _summaries(agg, scale_value)
    logo_i = _logo_array(_to_host(res["loo_i"]), index.labels) if pointwise else None
    out = _pack(summ, n_samples, index.n_groups, warn, scale, method, good_k, pointwise, logo_i, res["diag"])
    out.method = method.value
    return out


def loo_glm_marginal(idata, X, y, family, var_names, cluster, u_name, tau_name, z=None, n_nodes=15, sigma_name=None, var_name=None,
                     offset=None, trials=None, group_terms=None, reff=1.0, scale=None, method="psis", pointwise=False, *, link=None):
    """``loo_glm_marginal_from_design`` with the draws taken from ``idata``: ``beta`` from ``var_names`` as ``loo_glm`` takes it,
    the draws of the integrated effect from ``u_name`` (shape ``(chain, draw, C)``, one entry per cluster in the order of its sorted
    labels; None: nodes from ``mean(tau)``) and its scale from the scalar ``tau_name``.  ``group_terms``, ``sigma_name`` and
    ``y=None`` are ``loo_glm``'s."""
    data = to_inference_data(idata)
    beta, names, _ = _posterior_columns(data, var_names)
    if beta.shape[1] != X.shape[1]:
        raise ValueError(f"var_names give {beta.shape[1]} columns ({', '.join(names)}) for the {X.shape[1]} columns of X")

    def scalar(name, what):
        col, _, _ = _posterior_columns(data, [name])
        if col.shape[1] != 1:
            raise ValueError(f"{what} must name a scalar variable, '{name}' has {col.shape[1]} entries per draw")
        return col[:, 0]

    tau = scalar(tau_name, "tau_name")
    sigma = None if sigma_name is None else scalar(sigma_name, "sigma_name")
    u = None if u_name is None else _posterior_columns(data, [u_name])[0]
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
    return loo_glm_marginal_from_design(X, y, beta, family, cluster, tau, z=z, u=u, n_nodes=n_nodes, sigma=sigma, offset=offset,
                                        trials=trials, groups=groups, reff=reff, scale=scale, method=method, pointwise=pointwise,
                                        link=link)
