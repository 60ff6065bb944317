"""``loo_influence()`` -- what leaving observation i out does to the posterior itself, on the HIP engine: the Bayesian counterpart
of DFBETAS and Cook's distance.  Every other per-observation number of the package (``elpd_i``, Pareto k, PIT, ``n_eff``)
describes the fit to the held-out point; this one says which parameters the point pulls on, and by how much.  The reference has
only a bar plot of ``-elpd_i`` (plots/influence_plot.py).

Per observation i and draw-wise quantity j (a parameter, or any function of the parameters, one value per posterior draw), with
``w`` the normalised leave-one-out weights and ``z = (theta - center) / scale`` (``pla_loo_influence``, csrc/pla_influence.h):

    shift_ij    = sum_s w_is z_sj                       standardised LOO mean shift: (E[theta_j | y_-i] - E[theta_j | y]) / sd_j
    mean_loo_ij = center_j + scale_j shift_ij           the LOO posterior mean
    sd_ratio_ij = sqrt(max(sum_s w_is z_sj^2 - shift_ij^2, 0))       sd[theta_j | y_-i] / sd[theta_j | y]
    kl_i        = sum_s w_is log(S w_is)                KL( p(. | y_-i) || p(. | y) ) of the weighted draws
    ess_w_i     = 1 / sum_s w_is^2
    distance_i  = shift_i' R^+ shift_i                  R the P x P correlation of the draws (Cook's-distance-like)

``center`` and ``scale`` are the mean and the standard deviation (ddof 1) of the draws, computed here -- NumPy for host input,
torch for CUDA input -- and handed to the kernel.  The weights are never materialised: the kernel consumes one block of them at a
time, ``exp`` once per (observation, draw) for all P columns, and the contraction runs on the f64 matrix cores.

    res = pl.loo_influence_from_matrix(ll, theta, reff=r, names=["alpha", "beta"])
    print(pl.influence_table(res))

The shifts of an observation whose Pareto k is above the threshold are as unreliable as its ``elpd_i`` (a warning counts them).
Out of scope: moment-matched weights for those observations, plots, more than 1024 columns, multi-GPU sharding.
"""

import warnings
from dataclasses import dataclass
from typing import Any

import numpy as np

from .base import ISMethod, check_reff_vector, is_reff_vector, parse_method, tail_buckets, tail_count_for
from .e_loo import _pareto_khat_threshold
from .engine import _host, _is_torch_tensor, get_engine
from .loo import bucketed_matrix
from .relative_eff import relative_eff_from_matrix
from .utils import get_log_likelihood, stack_samples, to_inference_data

__all__ = ["loo_influence", "loo_influence_from_matrix", "influence_table", "LooInfluence"]

MAX_QUANTITIES = 1024  # PLA n_quant limit of pla_loo_influence
_VECTORS = ("kl", "ess_w", "diag")
_MATRICES = ("shift", "m2")
_NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."


@dataclass
class LooInfluence:
    """``shift``, ``mean_loo`` and ``sd_ratio`` are ``(*obs, P)``; ``kl``, ``ess_w``, ``pareto_k`` (None unless PSIS; then ``ess``
    holds the method's diagnostic) and ``distance`` are shaped like the observations.  ``names``: the P column names; ``center``
    and ``scale`` [P]: the posterior mean and sd the shifts are standardised with."""

    shift: Any
    mean_loo: Any
    sd_ratio: Any
    kl: Any
    ess_w: Any
    pareto_k: Any
    distance: Any
    names: list
    n_replaced: int
    khat_threshold: Any
    center: Any = None
    scale: Any = None
    n_samples: int = 0
    ess: Any = None
    method: str = "psis"


def _check_theta(theta, n_samples, names, on_device):
    """(theta (S, P) f64 of the kind of the matrix, center, scale, names); every rejection of theta and names."""
    if _is_torch_tensor(theta) or on_device is not None:
        import torch

        th = torch.as_tensor(theta, device=on_device).to(torch.float64)
        th = th.reshape(-1, 1) if th.dim() == 1 else th
        shape = tuple(th.shape)
    else:
        th = np.asarray(getattr(theta, "values", theta), dtype=np.float64)
        th = th.reshape(-1, 1) if th.ndim == 1 else th
        shape = th.shape
    if len(shape) != 2 or shape[0] != n_samples:
        raise ValueError(f"theta must be (n_draws, P) or (n_draws,) with n_draws = {n_samples}, got shape {tuple(shape)}")
    n_quant = shape[1]
    if n_quant < 1:
        raise ValueError("theta has no columns")
    if n_quant > MAX_QUANTITIES:
        raise ValueError(f"theta has {n_quant} columns; at most {MAX_QUANTITIES} are supported in one call")
    if names is None:
        names = [f"theta[{j}]" for j in range(n_quant)] if n_quant > 1 else ["theta"]
    names = [str(v) for v in names]
    if len(names) != n_quant:
        raise ValueError(f"names has {len(names)} entries for {n_quant} columns")
    finite = (torch.isfinite(th).all(dim=0).cpu().numpy() if _is_torch_tensor(th) else np.isfinite(th).all(axis=0))
    if not finite.all():
        j = int(np.nonzero(~finite)[0][0])
        raise ValueError(f"theta column {j} ('{names[j]}') holds values that are not finite")
    if _is_torch_tensor(th):
        center = th.mean(dim=0)
        scale = th.std(dim=0, unbiased=True) if n_samples > 1 else torch.zeros_like(center)
        scale_h = scale.cpu().numpy()
    else:
        center = th.mean(axis=0)
        scale = th.std(axis=0, ddof=1) if n_samples > 1 else np.zeros_like(center)
        scale_h = scale
    flat = ~(np.isfinite(scale_h) & (scale_h > 0))
    if flat.any():
        j = int(np.nonzero(flat)[0][0])
        raise ValueError(f"theta column {j} ('{names[j]}') is constant over the draws: it has no scale to standardise a shift with")
    return th, center, scale, names


def _check_rows(rows, n_obs):
    if rows is None:
        return None
    idx = np.ascontiguousarray(_host(rows).reshape(-1), dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n_obs):
        raise IndexError(f"row indices must lie in [0, {n_obs}), got range [{idx.min()}, {idx.max()}]")
    return idx


def _scatter(m_out, parts):
    """``parts``: (positions, engine output) per bucket -> the vectors [m_out] and matrices (m_out, P) of the kind of the outputs."""
    full = {}
    for k in _MATRICES + _VECTORS:
        first = parts[0][1][k]
        shape = (m_out,) + tuple(first.shape[1:])
        full[k] = first.new_empty(shape) if _is_torch_tensor(first) else np.empty(shape)
        for pos, out in parts:
            if _is_torch_tensor(first) and not _is_torch_tensor(pos):
                import torch

                pos = torch.as_tensor(np.asarray(pos), device=first.device)
            full[k][pos] = out[k]
    return full


def _arrays(ll, theta, reff, method, names, rows, n_chains):
    """Flat host arrays ``dict(shift, m2, kl, ess_w, diag)``, the NaN count, (center, scale) on the host, the names; every check
    before the first engine call."""
    if len(ll.shape) != 2:
        raise ValueError("ll must be a 2-D (n_obs, n_draws) matrix")
    n_obs, n_samples = ll.shape
    tensor = _is_torch_tensor(ll)
    th, center, scale, names = _check_theta(theta, n_samples, names, ll.device if tensor else None)
    idx = _check_rows(rows, n_obs)
    if reff is None and n_chains is None:
        raise ValueError("reff=None asks for relative_eff of the matrix and needs its chains: pass n_chains, or reff")
    if reff is not None and is_reff_vector(reff):
        check_reff_vector(reff, n_obs)
    elif reff is not None and method == ISMethod.PSIS and tail_count_for(n_samples, reff) + 1 > n_samples:
        raise IndexError(f"index {-tail_count_for(n_samples, reff) - 1} is out of bounds for axis 0 with size {n_samples}")
    if reff is None:
        reff = relative_eff_from_matrix(ll, n_chains=n_chains)
    eng_of = lambda m: get_engine(m.device.index if _is_torch_tensor(m) else None)  # noqa: E731
    counts = []

    def call(eng, matrix, M, index=None):
        out = eng.loo_influence(matrix, th, center, scale, M, method.value, "loglik", rows=index)
        counts.append(out["n_replaced"])
        return out

    if is_reff_vector(reff) and method == ISMethod.PSIS:
        # one pass per distinct tail count through the rows= route: (tail count, positions in the output, rows of the matrix)
        if idx is None:
            matrix, _, buckets = bucketed_matrix(ll, reff)
            jobs = [(m, pos, pos) for m, pos in buckets]
        else:
            r_sel = _host(check_reff_vector(reff, n_obs))[idx]
            _, buckets = tail_buckets(r_sel, n_samples)
            if buckets and buckets[-1][0] + 1 > n_samples:
                raise IndexError(f"index {-buckets[-1][0] - 1} is out of bounds for axis 0 with size {n_samples}")
            matrix = ll
            if n_samples > 1 and (ll.stride(1) != 1 if tensor else np.asarray(ll).strides[1] != np.asarray(ll).itemsize):
                matrix = ll.contiguous() if tensor else np.ascontiguousarray(ll)
            jobs = [(m, pos, idx[pos]) for m, pos in buckets]
        eng = eng_of(matrix)
        if idx is None and len(jobs) <= 1:
            res = call(eng, matrix, jobs[0][0] if jobs else 0)
        else:
            res = _scatter(n_obs if idx is None else idx.size, [(pos, call(eng, matrix, m, sel)) for m, pos, sel in jobs])
    else:
        M = tail_count_for(n_samples, reff) if method == ISMethod.PSIS and not is_reff_vector(reff) else 0
        res = call(eng_of(ll), ll, M, idx)
    n_replaced = int(sum(int(_host(c).reshape(-1)[0]) for c in counts))
    out = {k: np.asarray(_host(res[k]), dtype=np.float64) for k in _MATRICES + _VECTORS}
    return out, n_replaced, (np.asarray(_host(center), dtype=np.float64), np.asarray(_host(scale), dtype=np.float64)), names, _host(th)


def _distance(shift, theta_host):
    """shift_i' R^+ shift_i with R the correlation matrix of the columns of theta (pinv: collinear columns count once)."""
    if theta_host.shape[1] == 1:
        return shift[:, 0] ** 2
    corr = np.atleast_2d(np.corrcoef(theta_host, rowvar=False))
    rinv = np.linalg.pinv(corr, hermitian=True)
    return np.einsum("ij,jk,ik->i", shift, rinv, shift)


def _result(a, n_replaced, center_scale, names, theta_host, method, n_samples, obs_shape):
    if n_replaced > 0:  # loo.py:218-227
        warnings.warn(_NAN_TEXT, UserWarning, stacklevel=3)
    center, scale = center_scale
    psis = method == ISMethod.PSIS
    threshold = _pareto_khat_threshold(n_samples) if psis else None
    if psis:
        high = int(np.sum(a["diag"] > threshold))
        if high:
            warnings.warn(
                f"Estimated shape parameter of Pareto distribution is greater than {threshold:.2f} for {high} observations. "
                "Their shifts are as unreliable as their elpd_i: the leave-one-out posterior is too far from the full posterior "
                "for importance sampling.", UserWarning, stacklevel=3)
    shift = a["shift"]
    with np.errstate(invalid="ignore"):
        sd_ratio = np.sqrt(np.maximum(a["m2"] - shift * shift, 0.0))
        sd_ratio = np.where(np.isnan(a["m2"]), np.nan, sd_ratio)
        distance = _distance(shift, theta_host)
    vec = lambda v: np.asarray(v).reshape(obs_shape)  # noqa: E731
    mat = lambda v: np.asarray(v).reshape(tuple(obs_shape) + (len(names),))  # noqa: E731
    return LooInfluence(
        shift=mat(shift), mean_loo=mat(center + scale * shift), sd_ratio=mat(sd_ratio), kl=vec(a["kl"]), ess_w=vec(a["ess_w"]),
        pareto_k=vec(a["diag"]) if psis else None, distance=vec(distance), names=list(names), n_replaced=int(n_replaced),
        khat_threshold=threshold, center=center, scale=scale, n_samples=int(n_samples),
        ess=None if psis else vec(a["diag"]), method=method.value)


def loo_influence_from_matrix(ll, theta, reff=1.0, method="psis", names=None, rows=None, n_chains=None):
    """Case-deletion shifts from an ``(n_obs, n_draws)`` log-likelihood matrix and ``theta``, ``(n_draws, P)`` or ``(n_draws,)``,
    the draw-wise quantities -- both NumPy arrays, or both torch CUDA tensors (``theta`` is moved to the matrix's device).
    ``reff``: a float, a vector with one relative efficiency per observation (each observation then takes its own PSIS tail
    length), or None: ``relative_eff_from_matrix`` of ``ll`` with ``n_chains`` chains.  ``names``: P column names.  ``rows``:
    observation indices; the result then has one entry per index.  ``ValueError`` before anything runs for a ``theta`` of the
    wrong shape, with values that are not finite, with a constant column or with more than 1024 columns, and for a ``reff``
    vector of the wrong length.  Returns :class:`LooInfluence` with flat NumPy arrays."""
    method = parse_method(method)
    a, n_replaced, cs, names, th = _arrays(ll, theta, reff, method, names, rows, n_chains)
    return _result(a, n_replaced, cs, names, th, method, ll.shape[1], (a["kl"].shape[0],))


def _posterior_columns(idata, var_names):
    """(theta (n_draws, P), names, n_chains) of the ``posterior`` group: every variable flattened over its own dimensions."""
    if not hasattr(idata, "posterior"):
        raise ValueError("InferenceData object does not have a posterior group")
    group = idata.posterior
    available = list(group.data_vars) if hasattr(group, "data_vars") else list(group.keys())
    if var_names is None:
        var_names = available
    elif isinstance(var_names, str):
        var_names = [var_names]
    columns, names, n_chains = [], [], None
    for name in var_names:
        if name not in available:
            raise ValueError(f"Variable '{name}' not found in posterior group. Available variables: {available}")
        v = group[name]
        if hasattr(v, "dims") and hasattr(v, "transpose") and "chain" in v.dims and "draw" in v.dims:
            v = v.transpose("chain", "draw", ...)
        arr = np.asarray(getattr(v, "values", v), dtype=np.float64)
        if arr.ndim < 2:
            raise ValueError(f"posterior variable '{name}' must have (chain, draw, ...) dimensions, got shape {arr.shape}")
        n_chains = arr.shape[0] if n_chains is None else n_chains
        own = arr.shape[2:]
        flat = arr.reshape((arr.shape[0] * arr.shape[1], -1))
        columns.append(flat)
        if not own:
            names.append(str(name))
        else:
            names.extend(f"{name}[{','.join(str(i) for i in index)}]" for index in np.ndindex(*own))
    if not columns:
        raise ValueError("no posterior variable selected")
    return np.concatenate(columns, axis=1), names, int(n_chains)


def loo_influence(data, var_names=None, var_name=None, reff=None, method="psis"):
    """Case-deletion shifts of the posterior variables ``var_names`` (None: all of them) of ``data`` -- InferenceData with ArviZ,
    or the dict of groups ``loo()`` takes, with a ``posterior`` group of ``(chain, draw, ...)`` arrays.  Every variable is
    flattened over its own dimensions into named columns (``"beta[2]"``).  ``var_name``: the log-likelihood variable.
    ``reff=None``: ``relative_eff`` of the log-likelihood with the chains of ``data``; a float or an observation-shaped array
    otherwise.  ``shift``, ``mean_loo`` and ``sd_ratio`` are ``(*obs, P)``, the other pointwise fields are observation-shaped."""
    method = parse_method(method)
    idata = to_inference_data(data)
    theta, names, n_chains = _posterior_columns(idata, var_names)
    matrix, obs_shape, _, _ = stack_samples(get_log_likelihood(idata, var_name=var_name))
    if reff is not None and is_reff_vector(reff):
        reff = np.asarray(getattr(reff, "values", reff), dtype=np.float64).reshape(-1)
    a, n_replaced, cs, names, th = _arrays(matrix, theta, reff, method, names, None, n_chains)
    return _result(a, n_replaced, cs, names, th, method, matrix.shape[1], tuple(obs_shape))


def influence_table(res, n=10):
    """A DataFrame of the ``n`` observations of largest ``distance`` (flat observation index), with their Pareto k, ``kl``, and
    the largest ``|shift|`` with the name of its column.  Observations whose distance is NaN come last."""
    import pandas as pd

    n_quant = len(res.names)
    shift = np.asarray(getattr(res.shift, "values", res.shift), dtype=np.float64).reshape(-1, n_quant)
    flat = lambda v: None if v is None else np.asarray(getattr(v, "values", v), dtype=np.float64).reshape(-1)  # noqa: E731
    distance, kl, k = flat(res.distance), flat(res.kl), flat(res.pareto_k)
    order = np.argsort(-np.where(np.isnan(distance), -np.inf, distance), kind="stable")[: max(int(n), 0)]
    with np.errstate(invalid="ignore"):
        mag = np.where(np.isnan(shift), -1.0, np.abs(shift))
    col = mag.argmax(axis=1)
    frame = pd.DataFrame({
        "distance": distance[order],
        "pareto_k": k[order] if k is not None else np.full(order.size, np.nan),
        "kl": kl[order],
        "max_abs_shift": np.abs(shift[order, col[order]]),
        "shift": shift[order, col[order]],
        "column": [res.names[j] for j in col[order]],
    }, index=order)
    frame.index.name = "observation"
    return frame
