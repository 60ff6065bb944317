"""``loo_group()`` -- leave-one-group-out cross-validation (LOGO-CV) with the reference's signature and result object
(pyloo/loo_group.py:19-380), executed by the HIP engine.

What runs where: argument handling, warnings and ``ELPDData`` packing are host Python (loo_group.py:147-214, 239-281, 300-380);
the group sums (216-224: a Python loop over the groups, each building a mask over all observations) and the PSIS / SIS / TIS pass
over them (226-299) are one ``pla_psis_loo_groups`` call: one read of the log-likelihood matrix.

Deviation: NaN group labels are rejected with a ``ValueError`` (``np.unique`` gives every NaN a group of its own, while the
reference's ``group_ids == group`` mask never matches a NaN, so those groups would be empty sums).
"""

import warnings

import numpy as np

from ._capi import AGG_M2_LOO, AGG_MIN_DIAG, AGG_N, AGG_N_HIGH, AGG_SUM_LOO, AGG_SUM_LPPD
from .base import ISMethod, parse_method, tail_count_for
from .elpd import ELPDData
from .engine import _is_torch_tensor, get_engine
from .loo import _relative_efficiency, _scale_value
from .rcparams import rcParams
from .utils import get_log_likelihood, stack_samples, to_inference_data

try:  # optional: logo_i becomes a DataArray over the groups when xarray is there
    import xarray as xr
except Exception:  # pragma: no cover - absent in the build container
    xr = None

__all__ = ["GroupIndex", "group_index", "loo_group", "loo_group_from_matrix"]


class GroupIndex:
    """Groups of observations in compressed form: group ``g`` (label ``labels[g]``, in ``np.unique`` order) holds the observations
    ``members[offsets[g]:offsets[g + 1]]``, ascending.  ``offsets`` / ``members`` are int64 NumPy arrays or CUDA tensors (built where
    the labels were, or moved by :func:`group_index`'s ``device``); ``labels`` are always on the host.  Reusable across calls and
    models, and what a captured graph needs (no host work left in the call)."""

    def __init__(self, labels, offsets, members):
        self.labels = labels
        self.offsets = offsets
        self.members = members

    @property
    def n_groups(self):
        return len(self.labels)

    @property
    def n_obs(self):
        return int(self.members.shape[0])

    @property
    def on_device(self):
        return _is_torch_tensor(self.members)

    def to(self, device):
        """The same index with ``offsets`` / ``members`` on ``device`` (a torch device), or on the host for ``device=None``."""
        if device is None:
            conv = lambda a: a.detach().cpu().numpy() if _is_torch_tensor(a) else a  # noqa: E731
        else:
            import torch

            conv = lambda a: (a if _is_torch_tensor(a) else torch.from_numpy(np.asarray(a))).to(device=device, dtype=torch.int64)  # noqa: E731
        return GroupIndex(self.labels, conv(self.offsets), conv(self.members))


def _nan_labels():
    return ValueError("group_ids must not contain NaN (a NaN label matches no observation in the reference)")


def group_index(group_ids, device=None):
    """:class:`GroupIndex` of a label array (ints, floats or strings; any shape, flattened in C order).

    Host labels: ``np.unique(..., return_inverse=True)`` and a stable argsort.  A CUDA tensor of numeric labels is indexed on its
    device with ``torch.unique(sorted=True, return_inverse=True)`` and a stable ``torch.sort``.  ``device``: where ``offsets`` and
    ``members`` should live (default: where the labels are)."""
    if _is_torch_tensor(group_ids):
        import torch

        ids = group_ids.reshape(-1)
        if ids.is_floating_point() and bool(torch.isnan(ids).any()):
            raise _nan_labels()
        labels, inverse = torch.unique(ids, sorted=True, return_inverse=True)
        members = torch.sort(inverse, stable=True).indices.to(torch.int64)
        counts = torch.bincount(inverse, minlength=labels.numel())
        offsets = torch.zeros(labels.numel() + 1, dtype=torch.int64, device=ids.device)
        offsets[1:] = torch.cumsum(counts, 0)
        out = GroupIndex(labels.cpu().numpy(), offsets, members)
        return out if device is None else out.to(device)
    ids = np.asarray(group_ids).reshape(-1)
    if ids.dtype.kind in "fc" and np.isnan(ids).any():
        raise _nan_labels()
    labels, inverse = np.unique(ids, return_inverse=True)
    inverse = inverse.reshape(-1)
    members = np.argsort(inverse, kind="stable").astype(np.int64)
    offsets = np.zeros(labels.size + 1, dtype=np.int64)
    np.cumsum(np.bincount(inverse, minlength=labels.size), out=offsets[1:])
    out = GroupIndex(labels, offsets, members)
    return out if device is None else out.to(device)


def _flat_ids(group_ids, obs_shape, n_data_points):
    """loo_group.py:156-160: one label per observation (or an array of the observations' shape, flattened in C order)."""
    if isinstance(group_ids, GroupIndex):
        if group_ids.n_obs != n_data_points:
            raise ValueError(
                f"Length of group_ids ({group_ids.n_obs}) must match the number of observations in log_likelihood ({n_data_points})."
            )
        return group_ids
    shape = tuple(group_ids.shape) if hasattr(group_ids, "shape") else None
    if shape is not None and len(shape) > 1 and shape == tuple(obs_shape):
        return group_ids.reshape(-1)
    if len(group_ids) != n_data_points:
        raise ValueError(
            f"Length of group_ids ({len(group_ids)}) must match the number of observations in log_likelihood ({n_data_points})."
        )
    return group_ids


def _nan_warning(n_replaced):
    """loo_group.py:188-197."""
    if int(n_replaced) > 0:
        warnings.warn(
            "NaN values detected in log-likelihood. These will be ignored in the LOGO calculation.",
            UserWarning,
            stacklevel=3,
        )


def _method_warning(method):
    """loo_group.py:205-214."""
    if method != ISMethod.PSIS:
        warnings.warn(
            f"Using {method.value.upper()} for LOGO computation. Note that PSIS is the recommended method as it is typically more"
            " efficient and reliable.",
            UserWarning,
            stacklevel=3,
        )


def _diagnostic_warning(method, agg, good_k, n_samples):
    """loo_group.py:240-281.  Returns the ``warning`` flag."""
    if method == ISMethod.PSIS:
        n_high = int(agg[AGG_N_HIGH])
        if n_high > 0:
            warnings.warn(
                "Estimated shape parameter of Pareto distribution is greater than "
                f"{good_k:.2f} for {n_high} groups. This indicates that "
                "importance sampling may be unreliable because the marginal posterior "
                "and LOGO posterior are very different.",
                UserWarning,
                stacklevel=3,
            )
            return True
        return False
    min_ess = float(agg[AGG_MIN_DIAG])
    if min_ess < n_samples * 0.1:
        warnings.warn(
            f"Low effective sample size detected (minimum ESS: {min_ess:.1f}). This"
            " indicates that the importance sampling approximation may be"
            " unreliable. Consider using PSIS which is more robust to such cases.",
            UserWarning,
            stacklevel=3,
        )
        return True
    return False


def _summaries(agg, scale_value):
    """loo_group.py:283-306 from the reduced moments (the arithmetic of loo's summaries)."""
    n_groups = float(agg[AGG_N])
    elpd = float(agg[AGG_SUM_LOO])
    m2 = float(agg[AGG_M2_LOO])
    se = m2**0.5  # (G * var)^0.5 with var = M2 / G
    lppd = float(agg[AGG_SUM_LPPD])
    return {
        "elpd_logo": elpd,
        "se": se,
        "p_logo": lppd - elpd / scale_value,
        "p_logo_se": (m2 / n_groups) ** 0.5 if n_groups else float("nan"),
        "logoic": -2 * elpd,
        "logoic_se": 2 * se,
    }


def _pack(summ, n_samples, n_groups, warn, scale, method, good_k, pointwise, logo_i=None, diag=None):
    """Index order of loo_group.py:308-378."""
    data = [summ["elpd_logo"], summ["se"], summ["p_logo"], summ["p_logo_se"], n_samples, n_groups, warn]
    index = ["elpd_logo", "se", "p_logo", "p_logo_se", "n_samples", "n_groups", "warning"]
    if pointwise:
        data.append(logo_i)
        index.append("logo_i")
    data += [scale, summ["logoic"], summ["logoic_se"]]
    index += ["scale", "logoic", "logoic_se"]
    if pointwise:
        data.append(diag)
        index.append("pareto_k" if method == ISMethod.PSIS else "ess")
    if method == ISMethod.PSIS:
        data.append(good_k)
        index.append("good_k")
    return ELPDData(data=data, index=index)


def _run(matrix, index, method, reff, scale_value, good_k, pointwise):
    n_samples = matrix.shape[-1]
    M = tail_count_for(n_samples, reff) if method == ISMethod.PSIS else 0
    if method == ISMethod.PSIS and M + 1 > n_samples:
        raise IndexError(f"index {-M - 1} is out of bounds for axis 0 with size {n_samples}")
    dev = matrix.device.index if _is_torch_tensor(matrix) else None
    if dev is not None and not index.on_device:
        index = index.to(matrix.device)
    res = get_engine(dev).psis_loo_groups(matrix, index, M, method.value, scale_value, good_k, pointwise, True)
    a = res["agg"]
    agg = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    nrep = res["n_replaced"]
    return res, agg, int(nrep.item()) if hasattr(nrep, "item") else int(nrep)


def _logo_array(values, labels):
    values = np.asarray(values)
    if xr is not None:
        return xr.DataArray(values, dims=["group"], coords={"group": labels}, name="logo_i")
    return values


def loo_group_from_matrix(log_likelihood, group_ids, reff=1.0, scale=None, method="psis", pointwise=False):
    """LOGO from an ``(n_obs, n_draws)`` log-likelihood matrix -- the engine-level entry point, like ``loo_from_matrix``.

    ``log_likelihood``: NumPy array or CUDA tensor, draws contiguous or observations contiguous (ArviZ's layout).
    ``group_ids``: one label per observation (ndarray, or a CUDA tensor of numeric labels), or a prebuilt :class:`GroupIndex`.
    Pointwise outputs (``logo_i``, ``pareto_k`` / ``ess``) are indexed by the sorted unique labels and stay where the matrix is.
    """
    method = parse_method(method)
    scale, scale_value = _scale_value(scale)
    n_obs, n_samples = log_likelihood.shape
    index = _flat_ids(group_ids, (n_obs,), n_obs)
    if not isinstance(index, GroupIndex):
        index = group_index(index)
    good_k = min(1 - 1 / np.log10(n_samples), 0.7)
    res, agg, nrep = _run(log_likelihood, index, method, reff, scale_value, good_k, pointwise)
    _nan_warning(nrep)
    _method_warning(method)
    warn = _diagnostic_warning(method, agg, good_k, n_samples)
    summ = _summaries(agg, scale_value)
    out = _pack(summ, n_samples, index.n_groups, warn, scale, method, good_k, pointwise, res["logo_i"], res["diag"])
    out.method = method.value
    return out


def loo_group(data, group_ids, pointwise=None, var_name=None, reff=None, scale=None, method="psis"):
    """Leave-one-group-out cross-validation by importance sampling (PSIS by default).

    Same parameters, warnings, exceptions and ``ELPDData`` layout as ``pyloo.loo_group`` (loo_group.py:19-380).  ``group_ids`` holds
    one label per observation (ints, floats or strings; or an array of the observations' shape), or is a :class:`GroupIndex`.
    """
    idata = to_inference_data(data)
    log_likelihood = get_log_likelihood(idata, var_name=var_name)
    pointwise = rcParams["stats.ic_pointwise"] if pointwise is None else pointwise
    matrix, obs_shape, _, _ = stack_samples(log_likelihood)  # loo_group.py:150
    n_samples = matrix.shape[-1]
    n_data_points = int(np.prod(obs_shape))
    ids = _flat_ids(group_ids, obs_shape, n_data_points)  # loo_group.py:156-160
    scale, scale_value = _scale_value(scale)  # loo_group.py:163-172
    index = ids if isinstance(ids, GroupIndex) else group_index(ids)
    if reff is None:
        reff = _relative_efficiency(idata, n_samples)  # loo_group.py:174-186
    method = parse_method(method)  # loo_group.py:199-203
    good_k = min(1 - 1 / np.log10(n_samples), 0.7)  # loo_group.py:240
    res, agg, nrep = _run(matrix, index, method, reff, scale_value, good_k, pointwise)
    _nan_warning(nrep)
    _method_warning(method)
    warn = _diagnostic_warning(method, agg, good_k, n_samples)
    summ = _summaries(agg, scale_value)
    if not pointwise:
        out = _pack(summ, n_samples, index.n_groups, warn, scale, method, good_k, False)
    else:
        logo = _logo_array(res["logo_i"], index.labels)
        out = _pack(summ, n_samples, index.n_groups, warn, scale, method, good_k, True, logo, np.asarray(res["diag"]))
    out.method = method.value
    return out
