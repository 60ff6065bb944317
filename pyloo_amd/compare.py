"""``loo_compare()`` -- model comparison with the reference's signature, warnings and table (pyloo/compare.py:23-596), its
weights computed by the HIP engine.

What runs where: argument handling, ``_calculate_ics`` and the table are host Python (compare.py:170-264, 285-456).  The
pointwise values of the K models are stacked into one (K, N) matrix -- on the device when they are CUDA tensors, as
``loo_from_matrix`` returns them for a device matrix -- and every pass over it is a kernel (csrc/pla_compare.h):

- ``dse`` (compare.py:226-227): one ``pla_compare_moments`` pass, the mean and M2 of every model's difference to the best;
- stacking (477-536): scipy's SLSQP with the reference's setup, every objective / gradient point one ``pla_stacking_eval`` pass
  (``fun`` and ``jac`` at the same point share it);
- Bayesian-bootstrap pseudo-BMA (539-577): one ``pla_bb_bootstrap`` pass draws the B x N gamma weights inside the kernel (no
  Dirichlet matrix) and writes the B x K replicates ``z``; their softmax, mean and std over B are NumPy.
- pseudo-BMA (580-596) works on K numbers and stays NumPy.

Deviations: the Bayesian bootstrap draws from a specified Philox4x32-10 stream (csrc/pla_compare.h), not from NumPy's
``RandomState`` Dirichlet stream, so its weights agree with the reference statistically, not bit for bit.  As in the reference,
an ``int`` seed also seeds NumPy's global generator (``np.random.seed(seed)``, compare.py:548-549).  ``ic="kfold"`` on anything
but precomputed ``ELPDData`` (of ``loo_kfold``) needs the refits and raises ``NotImplementedError``.  The input dictionary is copied shallowly (the reference deep-copies it; nothing
here modifies it).
"""

import warnings

import numpy as np
import pandas as pd

from .elpd import ELPDData
from .engine import _is_torch_tensor, get_engine
from .loo import loo
from .loo_subsample import loo_subsample
from .waic import waic

__all__ = ["compare_weights", "loo_compare"]

def _validate_scale(value):
    """rcparams.py:14-19 of the reference."""
    valid_scales = {"deviance", "log", "negative_log"}
    if isinstance(value, str) and value.lower() in valid_scales:
        return value.lower()
    raise ValueError(f"Scale must be one of {valid_scales}, not {value}")


_SCALE_MUL = {"log": 1.0, "negative_log": -1.0, "deviance": -0.5}  # x / -2 and x * -1 of compare.py:489-492, 556-559


def loo_compare(compare_dict, ic="loo", method="stacking", b_samples=1000, alpha=1, seed=None, scale=None, var_name=None,
                observations=None, estimator=None, K=None, folds=None, stratify=None, random_seed=None):
    """Compare models by their expected log pointwise predictive density (ELPD).

    Same parameters, checks, warnings and result as ``pyloo.loo_compare`` (compare.py:23-264): a ``pandas.DataFrame`` ordered
    from the best model to the worst with the columns ``rank``, ``elpd_{ic}``, ``p_{ic}``, ``elpd_diff``, ``weight``, ``se``,
    ``dse``, ``warning`` and ``scale``.  ``compare_dict`` maps model names to data that :func:`pyloo_amd.loo` /
    :func:`~pyloo_amd.waic` / :func:`~pyloo_amd.loo_subsample` accept, or to ``ELPDData`` computed with ``pointwise=True``.
    """
    if not isinstance(compare_dict, dict):
        raise TypeError("compare_dict must be a dictionary")
    if len(compare_dict) < 2:
        raise ValueError("You must specify at least two models for comparison")
    if scale is None:
        scale = "log"
    scale = scale.lower()
    if scale not in ["log", "negative_log", "deviance"]:
        raise ValueError("Scale must be 'log', 'negative_log' or 'deviance'")
    method = method.lower()
    if method not in ["stacking", "bb-pseudo-bma", "pseudo-bma"]:
        raise ValueError("Method must be 'stacking', 'BB-pseudo-BMA' or 'pseudo-BMA'")
    if ic not in ["loo", "waic", "kfold"]:
        raise ValueError("ic must be 'loo', 'waic', or 'kfold'")

    elpds, scale, ic = _calculate_ics(compare_dict, scale=scale, ic=ic, var_name=var_name, observations=observations,
                                      estimator=estimator, K=K, folds=folds, stratify=stratify, random_seed=random_seed)
    ascending = scale != "log"
    model_names = list(elpds.keys())
    elpd_values = np.array([elpds[name][f"elpd_{ic}"] for name in model_names])
    order = np.argsort(elpd_values) if ascending else np.argsort(-elpd_values)
    ordered_names = [model_names[i] for i in order]
    best_model = ordered_names[0]

    pointwise = _pointwise_matrix(elpds, f"{ic}_i", model_names, best_model)
    eng = _engine_for(pointwise)
    n_obs = int(pointwise.shape[1])
    mom = eng.compare_moments(pointwise, model_names.index(best_model))
    mom = mom.detach().cpu().numpy() if _is_torch_tensor(mom) else np.asarray(mom)

    diffs, ses, dses = [], [], []
    for name in ordered_names:
        if name == best_model:
            diff = 0
            dse = 0
        else:
            diff = elpds[name][f"elpd_{ic}"] - elpds[best_model][f"elpd_{ic}"]
            if scale == "negative_log":
                diff *= -1
            elif scale == "deviance":
                diff *= -2
            m2 = float(mom[3 * model_names.index(name) + 2])
            dse = np.sqrt(n_obs * (m2 / n_obs))  # sqrt(len(pointwise_diff) * np.var(pointwise_diff))
        diffs.append(diff)
        ses.append(elpds[name]["se"])
        dses.append(dse)

    if method == "pseudo-bma":
        weights = dict(zip(model_names, _pseudo_bma(elpd_values.copy(), scale)))
    else:
        w, computed_ses = compare_weights(pointwise, method=method, b_samples=b_samples, alpha=alpha, seed=seed, scale=scale)
        weights = dict(zip(model_names, w))
        if method == "bb-pseudo-bma":
            computed_ses = pd.Series(computed_ses, index=elpds.keys())
            ses = [computed_ses[name] for name in ordered_names]

    return pd.DataFrame(
        {
            "rank": range(len(ordered_names)),
            f"elpd_{ic}": [elpds[name][f"elpd_{ic}"] for name in ordered_names],
            f"p_{ic}": [elpds[name][f"p_{ic}"] for name in ordered_names],
            "elpd_diff": diffs,
            "weight": [weights[name] for name in ordered_names],
            "se": ses,
            "dse": dses,
            "warning": [elpds[name]["warning"] for name in ordered_names],
            "scale": scale,
        },
        index=ordered_names,
    )


def compare_weights(pointwise, method="stacking", b_samples=1000, alpha=1.0, seed=None, scale="log"):
    """Model weights from a ``(n_models, n_obs)`` matrix of pointwise values (NumPy array or CUDA tensor) on ``scale``.

    Returns ``(weights, ses)``: ``weights`` an ndarray of n_models entries summing to one; ``ses`` the bootstrap standard errors
    ``z_bs.std(axis=0)`` for ``method="bb-pseudo-bma"`` (compare.py:576), else ``None``.  ``seed`` (bootstrap only): ``None`` draws
    a 64-bit key from ``np.random.SeedSequence()``, an ``int`` is the key (and also seeds NumPy's global generator, as the
    reference does), a ``np.random.RandomState`` supplies the key with one ``randint`` call."""
    method = method.lower()
    if method not in ["stacking", "bb-pseudo-bma", "pseudo-bma"]:
        raise ValueError("Method must be 'stacking', 'BB-pseudo-BMA' or 'pseudo-BMA'")
    scale = _validate_scale(scale)
    if not _is_torch_tensor(pointwise):
        pointwise = np.asarray(pointwise, dtype=np.float64)
    if pointwise.ndim != 2 or pointwise.shape[0] < 1 or pointwise.shape[1] < 1:
        raise ValueError("pointwise must be a non-empty 2-D (n_models, n_obs) array")
    n_models = int(pointwise.shape[0])
    if n_models > 64:
        raise ValueError(f"compare_weights supports at most 64 models on the device, got {n_models}")
    eng = _engine_for(pointwise)
    if method == "pseudo-bma":
        mom = eng.compare_moments(pointwise, 0)
        mom = mom.detach().cpu().numpy() if _is_torch_tensor(mom) else np.asarray(mom)
        return _pseudo_bma(np.array([mom[3 * k] for k in range(n_models)]), scale), None
    if method == "stacking":
        return _stacking(eng, pointwise, n_models, _SCALE_MUL[scale]), None
    key = _seed_key(seed)
    z = eng.bb_bootstrap(pointwise, int(b_samples), float(alpha), key, _SCALE_MUL[scale])
    z = z.detach().cpu().numpy() if _is_torch_tensor(z) else np.asarray(z)
    rel = z - np.max(z, axis=1, keepdims=True)  # compare.py:568-573, every replicate at once
    w = np.exp(rel)
    w = w / np.sum(w, axis=1, keepdims=True)
    return w.mean(axis=0), z.std(axis=0)


# ---------------------------------------------------------------------------------------------------------------------------
def _calculate_ics(compare_dict, scale=None, ic=None, var_name=None, observations=None, estimator=None, K=None, folds=None,
                   stratify=None, random_seed=None):
    """compare.py:285-456: precomputed ``ELPDData`` are checked for one ic, one scale and pointwise values; everything else
    goes through this package's ``loo`` / ``waic`` / ``loo_subsample`` with ``pointwise=True``."""
    precomputed_elpds = {name: elpd_data for name, elpd_data in compare_dict.items() if isinstance(elpd_data, ELPDData)}
    precomputed_ic = None
    precomputed_scale = None
    if precomputed_elpds:
        _, arbitrary_elpd = precomputed_elpds.popitem()
        precomputed_ic = arbitrary_elpd.index[0].split("_")[1]
        precomputed_scale = arbitrary_elpd["scale"]
        raise_non_pointwise = f"{precomputed_ic}_i" not in arbitrary_elpd
        if any(elpd_data.index[0].split("_")[1] != precomputed_ic for elpd_data in precomputed_elpds.values()):
            raise ValueError("All information criteria to be compared must be the same")
        if any(elpd_data["scale"] != precomputed_scale for elpd_data in precomputed_elpds.values()):
            raise ValueError("All information criteria to be compared must use the same scale")
        if any(f"{precomputed_ic}_i" not in elpd_data for elpd_data in precomputed_elpds.values()) or raise_non_pointwise:
            raise ValueError("Not all provided ELPDData have been calculated with pointwise=True")
        if ic is not None and ic.lower() != precomputed_ic.lower():
            warnings.warn(
                "Provided ic argument is incompatible with precomputed elpd data. "
                f"Using ic from precomputed elpddata: {precomputed_ic}",
                stacklevel=3,
            )
            ic = precomputed_ic
        if scale is not None and scale.lower() != precomputed_scale:
            warnings.warn(
                "Provided scale argument is incompatible with precomputed elpd data. "
                f"Using scale from precomputed elpddata: {precomputed_scale}",
                stacklevel=3,
            )
            scale = precomputed_scale

    if ic is None and precomputed_ic is None:
        ic = "loo"
    elif ic is None:
        ic = precomputed_ic
    else:
        ic = ic.lower()
    if scale is None and precomputed_scale is None:
        scale = "log"
    elif scale is None:
        scale = precomputed_scale
    else:
        scale = _validate_scale(scale)

    compare_dict = dict(compare_dict)
    for name, dataset in compare_dict.items():
        if isinstance(dataset, ELPDData):
            continue
        if ic == "kfold":
            raise NotImplementedError("ic='kfold' needs the refits of every model: compute them with loo_kfold(..., pointwise=True) and pass the ELPDData")
        try:
            if ic == "waic":
                compare_dict[name] = waic(dataset, pointwise=True, var_name=var_name, scale=scale)
            elif observations is not None:
                compare_dict[name] = loo_subsample(dataset, observations=observations, estimator=estimator, pointwise=True,
                                                   var_name=var_name, scale=scale)
            else:
                compare_dict[name] = loo(dataset, pointwise=True, var_name=var_name, scale=scale)
        except Exception as e:
            raise e.__class__(f"Encountered error trying to compute {ic} from model {name}.") from e
    if scale is None:
        scale = "log"
    return compare_dict, scale, ic


def _values(v):
    """A pointwise entry of an ``ELPDData`` as a 1-D NumPy array or CUDA tensor (DataArrays give their ``.values``)."""
    if _is_torch_tensor(v):
        return v.reshape(-1)
    return np.asarray(getattr(v, "values", v), dtype=np.float64).reshape(-1)


def _pointwise_matrix(elpds, ic_i, model_names, best_model):
    """The (K, N) matrix of the models' pointwise values, stacked on the device when every one of them is a CUDA tensor."""
    cols = [_values(elpds[name][ic_i]) for name in model_names]
    best = cols[model_names.index(best_model)]
    for name, c in zip(model_names, cols):
        if tuple(c.shape) != tuple(best.shape):
            raise ValueError(
                "The number of observations should be the same across all models: "
                f"{name} has shape {tuple(c.shape)}, {best_model} has shape {tuple(best.shape)}"
            )
    if all(_is_torch_tensor(c) for c in cols):
        import torch

        dev = cols[0].device
        return torch.stack([c.to(device=dev, dtype=torch.float64) for c in cols])
    return np.stack([c.detach().cpu().numpy().astype(np.float64) if _is_torch_tensor(c) else c for c in cols])


def _engine_for(pointwise):
    return get_engine(pointwise.device.index if _is_torch_tensor(pointwise) else None)


def _pseudo_bma(elpd_values, scale):
    """compare.py:580-596 on the K totals (host)."""
    if scale == "deviance":
        elpd_values /= -2
    elif scale == "negative_log":
        elpd_values *= -1
    rel_elpds = elpd_values - np.max(elpd_values)
    weights = np.exp(rel_elpds)
    return weights / np.sum(weights)


def _stacking(eng, pointwise, n_models, scale_mul, stats=None):
    """compare.py:494-536: scipy's SLSQP with the reference's x0, bounds, constraints and options; the objective and its
    gradient at a point come from one ``stacking_eval`` pass (a one-entry cache serves ``fun`` and ``jac`` at the same x).
    ``stats``: optional dict that receives the number of passes (``"evaluations"``)."""
    from scipy import optimize

    if n_models == 1:
        return np.ones(1)
    cache = {}

    def full(weights):
        weights = np.concatenate((weights, [max(1.0 - np.sum(weights), 0.0)]))
        weights = np.maximum(weights, 0)
        return weights / np.sum(weights)

    def evaluate(x):
        key = np.asarray(x, dtype=np.float64).tobytes()
        if key not in cache:
            cache.clear()
            cache[key] = eng.stacking_eval(pointwise, full(x), scale_mul)
            if stats is not None:
                stats["evaluations"] = stats.get("evaluations", 0) + 1
        return cache[key]

    def objective(x):
        return -evaluate(x)[0]

    def gradient(x):
        G = evaluate(x)[1]
        return -(G[:-1] - G[-1])

    x0 = np.full(n_models - 1, 1.0 / n_models)
    bounds = [(0.0, 1.0)] * (n_models - 1)
    constraints = [
        {"type": "ineq", "fun": lambda x: 1.0 - np.sum(x)},
        {"type": "ineq", "fun": np.sum},
    ]
    result = optimize.minimize(objective, x0, jac=gradient, bounds=bounds, constraints=constraints, method="SLSQP",
                               options={"ftol": 1e-12, "maxiter": 2000})
    return full(result.x)


def _seed_key(seed):
    """64-bit key of the bootstrap stream; an int seed also seeds NumPy's global generator (compare.py:548-549)."""
    if seed is None:
        return int(np.random.SeedSequence().generate_state(1, np.uint64)[0])
    if isinstance(seed, np.random.RandomState):
        return int(seed.randint(0, 2**64, dtype=np.uint64))
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
        np.random.seed(seed)
        return int(seed) & (2**64 - 1)
    raise TypeError(f"seed must be None, an int or a np.random.RandomState, not {type(seed).__name__}")
