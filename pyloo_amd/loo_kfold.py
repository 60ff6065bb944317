"""``loo_kfold()`` -- exact K-fold cross-validation with the reference's signature and result object
(pyloo/loo_kfold.py:22-394), the arithmetic around the refits executed by the HIP engine.

Host Python: the fold assignment (``kfold_split_random`` / ``kfold_split_stratified`` / ``kfold_split_grouped`` make the
``np.random`` calls of loo_kfold.py:479-604 in the same order, so a seed gives the reference's folds), ``_prepare_folds``'
checks and messages (412-476), the NaN warning and the ``ELPDData`` packing (250-259, 301-394).  Engine (``pla_kfold_lme`` +
``pla_kfold_reduce``, one read of every matrix): ``log mean_s exp(ll)`` of every held-out observation under its own fold's draws
(643-667), the same under the full fit (675-692), ``p_kfold``, the sums and the standard errors (291-299).

Deliberate departures from the reference:

* The refits are the caller's.  The reference re-samples a PyMC model per fold; here ``fit_fold(train_idx, val_idx, **kwargs)``
  returns the held-out log-likelihood of fold k under whatever sampler the caller has (or ``fold_log_likelihoods`` holds them
  precomputed).
* Fold labels must be exactly the integers 1..K, otherwise ``ValueError("Fold indices must be the integers 1..K")``.  The
  reference loops ``k = 1..len(unique)`` and silently leaves ``elpd = 0`` for observations with any other label.
* An exception in ``fit_fold`` propagates.  The reference logs it and leaves zeros for the fold.
* float32 inputs are widened on load and reduced in float64 (the reference reduces them in float32).
* With fewer groups than K the result's ``K`` is the number of groups (the reference lowers K inside its splitter only and
  then skips the empty folds).
* What the reference logs (K > N, ``folds`` overriding ``stratify``, fewer groups than K, a single stratum) is a
  ``warnings.warn`` here.
"""

import warnings

import numpy as np

from ._capi import AGG_M2_LOO, AGG_N_HIGH, AGG_N_NONFINITE, AGG_SUM_LOO, AGG_SUM_LPPD
from .elpd import ELPDData
from .engine import _is_torch_tensor, get_engine
from .loo import _scale_value
from .rcparams import rcParams
from .utils import get_log_likelihood, stack_samples, to_inference_data, wrap_obs

__all__ = ["loo_kfold", "loo_kfold_from_matrix", "kfold_split_random", "kfold_split_stratified", "kfold_split_grouped"]


# ---------------------------------------------------------------------------------------------------------------- fold assignment
# The three splitters draw from NumPy's global generator exactly what the reference's draw (loo_kfold.py:479-604: one
# ``permutation`` per splitter call, or per stratum in ascending stratum order), so a seed gives the reference's folds.
def _deal(labels, members, K):
    """Label ``members`` (an index array in the order it is to be dealt) 1..K in consecutive runs whose lengths differ by at
    most one, the longer runs first."""
    share, extra = divmod(len(members), K)
    labels[members] = np.repeat(np.arange(1, K + 1), share + (np.arange(K) < extra))


def _reseed(seed):
    if seed is not None:
        np.random.seed(seed)


def kfold_split_random(K, N, seed=None):
    """Random folds of (nearly) equal size: labels 1..K for N observations."""
    _reseed(seed)
    labels = np.zeros(N, dtype=int)
    _deal(labels, np.random.permutation(N), K)
    return labels


def kfold_split_stratified(K, x, seed=None):
    """Folds that keep the distribution of ``x``: every stratum is shuffled and dealt over the K folds.  A numeric ``x`` with more
    than K distinct values is cut at its K-quantiles first; a single stratum falls back to random folds (with a warning)."""
    _reseed(seed)
    x = np.asarray(x)
    if K <= 1:
        raise ValueError(f"K must be > 1 for stratified folds, got {K}")
    numeric = np.issubdtype(x.dtype, np.number)
    if numeric and np.isnan(x).any():
        raise ValueError("Stratification variable contains NaN values")
    strata = x
    if numeric and np.unique(x).size > K:
        edges = np.unique(np.percentile(x, np.linspace(0, 100, K + 1)))
        strata = np.digitize(x, edges[:-1])
    levels = np.unique(strata)
    if levels.size == 1:
        warnings.warn("Only 1 unique value in stratification variable, using random folds instead", UserWarning, stacklevel=2)
        return kfold_split_random(K, len(x), seed)
    labels = np.zeros(len(x), dtype=int)
    for level in levels:
        _deal(labels, np.random.permutation(np.flatnonzero(strata == level)), K)
    return labels


def kfold_split_grouped(K, groups, seed=None):
    """Folds that keep every group together: the groups, shuffled, go to the folds in turn.  With fewer groups than K, K becomes
    the number of groups (with a warning)."""
    _reseed(seed)
    names, member_of = np.unique(np.asarray(groups), return_inverse=True)
    if names.size < K:
        warnings.warn(f"Number of groups ({names.size}) is less than K ({K}). Setting K={names.size}", UserWarning, stacklevel=2)
        K = names.size
    if K <= 1:
        raise ValueError(f"K must be > 1 for group-based folds, got {K}")
    fold_of_group = np.empty(names.size, dtype=int)
    fold_of_group[np.random.permutation(names.size)] = np.arange(names.size) % K + 1
    return fold_of_group[member_of.reshape(-1)]


def _as_long_as(what, values, n_obs):
    values = np.asarray(values)
    if len(values) != n_obs:
        raise ValueError(f"Length of {what} ({len(values)}) must match observations ({n_obs})")
    return values


def _prepare_folds(folds, K, n_obs, stratify, groups, random_seed):
    """``(folds, K)`` from what the caller gave, in the reference's order of precedence (loo_kfold.py:412-476) and with its
    messages: the caller's ``folds``, else ``groups``, else ``stratify``, else random folds."""
    if K <= 0:
        raise ValueError(f"K must be positive, got {K}")
    if K > n_obs:
        warnings.warn(f"K ({K}) is greater than N ({n_obs}), setting K=N", UserWarning, stacklevel=3)
        K = n_obs
    if folds is not None:
        if stratify is not None:
            warnings.warn("Both folds and stratify were provided. Using the provided folds and ignoring stratify.", UserWarning,
                          stacklevel=3)
        folds = _as_long_as("folds", folds, n_obs)
        distinct = np.unique(folds)
        if distinct.size < 2:
            raise ValueError(f"Need at least 2 unique fold values, got {distinct.size}")
        if (distinct == 0).any():
            raise ValueError("Fold indices must be >= 1")
        return folds, int(distinct.size)
    for what, values, split in (("groups", groups, kfold_split_grouped), ("stratify", stratify, kfold_split_stratified)):
        if values is None:
            continue
        values = _as_long_as(what, values, n_obs)
        kind = "group-based" if what == "groups" else "stratified"
        try:
            made = split(K, values, seed=random_seed)
        except Exception as err:
            raise ValueError(f"Failed to create {kind} folds: {err}") from err
        return made, int(made.max())  # (fewer groups than K: the splitter lowered K)
    return kfold_split_random(K, n_obs, random_seed), K


def _kfold_scale(scale):
    """``(scale, factor)``; ``None`` is the log scale, as in the reference's ``loo_kfold`` (loo_kfold.py:232-241)."""
    scale = "log" if scale is None else scale.lower()
    if scale not in ("log", "negative_log", "deviance"):
        raise ValueError("Scale must be 'log', 'negative_log', or 'deviance'")
    return _scale_value(scale)


def _check_labels(folds, K):
    """Labels exactly the integers 1..K, as a host int64 array."""
    f = np.asarray(folds)
    if f.ndim != 1 or f.size == 0 or f.dtype.kind not in "iuf" or (f.dtype.kind == "f" and not np.all(f == np.floor(f))):
        raise ValueError("Fold indices must be the integers 1..K")
    f = f.astype(np.int64)
    if not np.array_equal(np.unique(f), np.arange(1, K + 1)):
        raise ValueError("Fold indices must be the integers 1..K")
    return f


# -------------------------------------------------------------------------------------------------------------------- the result
def _kfold_result(ll_full, fold_log_liks, folds, K, scale, scale_value, pointwise, n_samples, stratified, grouped, wrap=None,
                  fits=None):
    N = int(ll_full.shape[0])
    mats = list(fold_log_liks)
    if len(mats) != K:
        raise ValueError(f"Expected {K} fold log-likelihood matrices, got {len(mats)}")
    dtypes = {str(m.dtype).split(".")[-1] for m in [ll_full] + mats}
    if len(dtypes) != 1:
        raise TypeError(f"The full and the fold log-likelihoods must share one dtype, got {sorted(dtypes)}")
    counts = np.bincount(folds - 1, minlength=K)
    for k, m in enumerate(mats):
        if len(m.shape) != 2 or int(m.shape[0]) not in (int(counts[k]), N):
            raise ValueError(f"Fold {k + 1}: expected a ({counts[k]}, S) or ({N}, S) log-likelihood matrix, got {tuple(m.shape)}")
    dev = ll_full.device.index if _is_torch_tensor(ll_full) and ll_full.is_cuda else None
    res = get_engine(dev).kfold(ll_full, mats, folds, scale_value)
    a = res["agg"]
    agg = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    if agg[AGG_N_NONFINITE] > 0:  # loo_kfold.py:250-259 (the engine counted what it replaced while reading the matrix)
        warnings.warn("NaN values detected in log-likelihood. These will be ignored in the LOGO calculation.", UserWarning, stacklevel=3)
    scale_factor = {"log": 1, "negative_log": -1, "deviance": -2}[scale]
    elpd_kfold = float(agg[AGG_SUM_LOO])             # loo_kfold.py:295
    se = float(agg[AGG_M2_LOO]) ** 0.5               # 296: sqrt(n * var) with var = M2 / n
    p_kfold = float(agg[AGG_SUM_LPPD])               # 297
    p_kfold_se = float(agg[AGG_N_HIGH]) ** 0.5       # 292 (the slot holds M2 of p_i: include/pyloo_amd.h)
    kfoldic = -2 * elpd_kfold / scale_factor         # 298
    kfoldic_se = 2 * se
    data = [elpd_kfold, se, p_kfold, p_kfold_se, n_samples, N, False]
    index = ["elpd_kfold", "se", "p_kfold", "p_kfold_se", "n_samples", "n_data_points", "warning"]
    if pointwise:
        ki = res["kfold_i"]
        if wrap is not None:
            ki = wrap(ki.detach().cpu().numpy() if hasattr(ki, "detach") else np.asarray(ki))
        data.append(ki)
        index.append("kfold_i")
    data += [scale, K, kfoldic, kfoldic_se, stratified, grouped]
    index += ["scale", "K", "kfoldic", "kfoldic_se", "stratified", "grouped"]
    if fits is not None:
        data.append(fits)
        index.append("fits")
    out = ELPDData(data=data, index=index)
    out.method = "kfold"
    out.K = K
    out.stratified = stratified
    out.grouped = grouped
    return out


def loo_kfold_from_matrix(ll_full, fold_log_liks, folds, *, pointwise=None, scale=None):
    """K-fold cross-validation from matrices in this package's observations x draws convention.

    ``ll_full`` (N, S): the full fit.  ``fold_log_liks``: K matrices; matrix k (fold label k + 1) is compact
    ``(n_val_k, S_k)`` with its rows in ascending observation order, or full ``(N, S_k)`` -- told apart by ``shape[0]``, the
    forms may be mixed, the dtypes may not (``TypeError``).  ``folds`` (N,): exactly the integers 1..K.  ``scale=None`` is the log
    scale, as in ``loo_kfold``.  NumPy arrays or torch
    CUDA tensors (read in place through their strides; ``kfold_i`` then stays on the device)."""
    pointwise = rcParams["stats.ic_pointwise"] if pointwise is None else pointwise
    scale, scale_value = _kfold_scale(scale)
    if len(ll_full.shape) != 2:
        raise ValueError("ll_full must be a 2-D (n_obs, n_draws) matrix")
    mats = list(fold_log_liks)
    K = len(mats)
    if K < 2:
        raise ValueError(f"Need at least 2 folds, got {K}")
    f = folds.detach().cpu().numpy() if _is_torch_tensor(folds) else np.asarray(folds)
    if f.ndim == 1 and len(f) != int(ll_full.shape[0]):
        raise ValueError(f"Length of folds ({len(f)}) must match observations ({int(ll_full.shape[0])})")
    f = _check_labels(f, K)
    return _kfold_result(ll_full, mats, f, K, scale, scale_value, pointwise, int(ll_full.shape[1]), False, False)


def _held_out_matrix(obj, var_name):
    """What ``fit_fold`` returned, as an (n_val, S_k) matrix: a 2-D CUDA tensor or ndarray is that matrix already, anything else
    goes through the path of ``loo()`` (``to_inference_data`` -> ``get_log_likelihood`` -> the stacked (obs, sample) view)."""
    if _is_torch_tensor(obj):
        if obj.dim() != 2:
            raise ValueError("a tensor returned by fit_fold must be a 2-D (n_val, n_draws) matrix")
        return obj if obj.is_cuda else obj.numpy()
    if isinstance(obj, np.ndarray) and obj.ndim == 2:
        return obj
    return stack_samples(get_log_likelihood(to_inference_data(obj), var_name=var_name))[0]


def loo_kfold(data, fit_fold=None, *, fold_log_likelihoods=None, K=10, pointwise=None, folds=None, var_name=None, scale=None,
              save_fits=False, stratify=None, groups=None, random_seed=None, **kwargs):
    """Exact K-fold cross-validation (pyloo.loo_kfold with the PyMC wrapper replaced by the caller's refit).

    ``data``: the full fit, whatever ``loo()`` accepts.  ``fit_fold(train_idx, val_idx, **kwargs)`` is called once per fold,
    k = 1..K, and returns the held-out log-likelihood of the ``len(val_idx)`` observations under that fold's draws -- anything
    ``loo()`` accepts, or an ``(n_val, S_k)`` matrix (CUDA tensor or 2-D ndarray); ``fold_log_likelihoods`` is the same thing precomputed (a sequence of
    K).  Exactly one of the two is given.  ``K``, ``folds`` (labels 1..K), ``stratify``, ``groups``, ``random_seed``, ``scale``,
    ``pointwise`` and ``save_fits`` as in the reference; ``save_fits=True`` appends ``"fits"``: a list of
    ``(fit_fold's return value, val_idx)``.  Returns an ``ELPDData`` with the reference's index."""
    if (fit_fold is None) == (fold_log_likelihoods is None):
        raise ValueError("Give exactly one of fit_fold and fold_log_likelihoods")
    idata = to_inference_data(data)
    log_likelihood = get_log_likelihood(idata, var_name=var_name)
    pointwise = rcParams["stats.ic_pointwise"] if pointwise is None else pointwise
    matrix, obs_shape, obs_dims, coords = stack_samples(log_likelihood)
    n_obs, n_samples = int(matrix.shape[0]), int(matrix.shape[1])
    scale, scale_value = _kfold_scale(scale)
    user_folds = folds is not None
    fold_arr, K = _prepare_folds(folds, K, n_obs, stratify, groups, random_seed)
    fold_arr = _check_labels(fold_arr, K)
    fits = [] if save_fits else None
    if fit_fold is not None:
        sources = []
        for k in range(1, K + 1):
            val_idx = np.where(fold_arr == k)[0]
            fit = fit_fold(np.where(fold_arr != k)[0], val_idx, **kwargs)
            sources.append(fit)
            if save_fits:
                fits.append((fit, val_idx))
    else:
        sources = list(fold_log_likelihoods)
        if len(sources) != K:
            raise ValueError(f"Expected {K} fold log-likelihoods, got {len(sources)}")
        if save_fits:
            fits = [(src, np.where(fold_arr == k + 1)[0]) for k, src in enumerate(sources)]
    mats = [_held_out_matrix(src, var_name) for src in sources]
    return _kfold_result(matrix, mats, fold_arr, K, scale, scale_value, pointwise, n_samples,
                         stratify is not None and not user_folds, groups is not None and not user_folds,
                         wrap=lambda w: wrap_obs(w, obs_shape, obs_dims, coords, "kfold_i"), fits=fits)
