#!/usr/bin/env python3
"""Generate ``kfold.npz`` (loo_kfold) from the REAL reference.

Run only in the build container (the reference checkout does not exist on the GPU box):
``python tests/golden/make_golden_kfold.py``

The reference's ``loo_kfold.py`` is loaded in place as ``pyloo.loo_kfold`` once the modules it imports and never reaches here are
placeholders (``pymc``, ``xarray``, ``pyloo.rcparams``, ``pyloo.wrapper.pymc.pymc``); ``pyloo.utils`` (``_logsumexp``,
``wrap_xarray_ufunc``) and ``pyloo.elpd`` (the printed report; it needs pandas only) are the real ones.  The refits are the part
of the reference that is not run: the per-fold log-likelihoods are seeded arrays, and the reference's own lines are chained
around them -- loo_kfold.py:250-261 (NaN of the full fit, ``_compute_lpds_full``), 643-657 per fold (``wrap_xarray_ufunc`` of
``_logsumexp`` with ``b_inv`` = the fold's draws), 285-299 (scatter, ``p_kfold``, sums and standard errors), 388-392 (the
``ELPDData`` of the report).  Only inputs and what the reference computed are written.
"""

import importlib.util
import os
import sys
import types
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, load_reference  # noqa: E402


def load_kfold():
    utils = load_reference()["utils"]

    def placeholder(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    placeholder("pymc")
    placeholder("pyloo.rcparams", rcParams={"stats.ic_pointwise": False})
    placeholder("pyloo.wrapper").__path__ = []
    placeholder("pyloo.wrapper.pymc").__path__ = []
    placeholder("pyloo.wrapper.pymc.pymc", PyMCWrapper=type("PyMCWrapper", (), {}))
    mods = {}
    for name in ("elpd", "loo_kfold"):
        spec = importlib.util.spec_from_file_location(f"pyloo.{name}", f"{REF}/{name}.py")
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"pyloo.{name}"] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return utils, mods["elpd"], mods["loo_kfold"]


def lme_rows(utils, ll):
    """loo_kfold.py:648-657 / 682-691 on an (n, S) array: ``_logsumexp`` of every row with ``b_inv = S``."""
    with np.errstate(all="ignore"):
        return np.asarray(utils.wrap_xarray_ufunc(utils._logsumexp, ll, func_kwargs={"b_inv": ll.shape[-1]},
                                                  ufunc_kwargs={"n_dims": 1, "ravel": False}, input_core_dims=[["__sample__"]]))


def run_reference(utils, ll_full, fold_lls, folds, scale):
    """The reference's arithmetic around the refits; ``fold_lls[k - 1]`` is the compact (n_val_k, S_k) matrix of fold k."""
    n_obs = ll_full.shape[0]
    scale_factor = {"log": 1, "negative_log": -1, "deviance": -2}[scale]
    K = len(np.unique(folds))
    full = ll_full.astype(np.float64)
    n_nan = int(np.isnan(full).sum())
    if n_nan:  # 250-259
        full = np.where(~np.isnan(full), full, -1e10)
    lpds_full = lme_rows(utils, full)  # 261
    elpds = np.zeros(n_obs)
    for k in range(1, K + 1):  # 265-286
        val_indices = np.where(folds == k)[0]
        fold_elpds = lme_rows(utils, fold_lls[k - 1].astype(np.float64))
        for idx, val in zip(val_indices, fold_elpds):
            elpds[idx] = val
    held_out = elpds.copy()
    with np.errstate(all="ignore"):
        p_kfold = lpds_full - elpds  # 291-299
        p_kfold_se = np.sqrt(n_obs * np.var(p_kfold))
        elpds = scale_factor * elpds
        elpd_kfold = np.sum(elpds)
        se = np.sqrt(n_obs * np.var(elpds))
        p_kfold_sum = np.sum(p_kfold)
    kfoldic = -2 * elpd_kfold / scale_factor
    return {"lpd_full": lpds_full, "elpd": held_out, "p_i": p_kfold, "kfold_i": elpds, "n_nan": n_nan, "K": K,
            "stats": np.array([elpd_kfold, se, p_kfold_sum, p_kfold_se, kfoldic, 2 * se])}


def report(elpd_mod, r, n_samples, n_obs, scale, stratified):
    """str() of the ELPDData of loo_kfold.py:320-392 (pointwise=False)."""
    e, se, p, pse, ic, icse = r["stats"]
    data = [e, se, p, pse, n_samples, n_obs, False, scale, r["K"], ic, icse, stratified, False]
    index = ["elpd_kfold", "se", "p_kfold", "p_kfold_se", "n_samples", "n_data_points", "warning", "scale", "K", "kfoldic",
             "kfoldic_se", "stratified", "grouped"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = elpd_mod.ELPDData(data=data, index=index)
        out.method = "kfold"
        out.K = r["K"]
        out.stratified = stratified
        out.grouped = False
    return str(out)


def draws(rng, n, s, dtype=np.float64):
    """Pointwise log-likelihoods as a model gives them: a per-observation level, per-draw noise, a few heavy rows."""
    level = rng.normal(-1.4, 0.8, size=(n, 1))
    spread = rng.uniform(0.2, 1.5, size=(n, 1))
    return (level - spread * rng.gamma(1.2, 1.0, size=(n, s))).astype(dtype)


def compact(rng, folds, sizes, dtype=np.float64):
    return [draws(rng, int(np.sum(folds == k + 1)), s, dtype) for k, s in enumerate(sizes)]


def main():
    utils, elpd_mod, kf = load_kfold()
    out = {}

    def store(case, ll_full, fold_lls, folds, scale, **extra):
        r = run_reference(utils, ll_full, fold_lls, folds, scale)
        out[f"{case}/ll_full"] = ll_full
        out[f"{case}/folds"] = folds
        out[f"{case}/scale"] = np.array(scale)
        for k, m in enumerate(fold_lls):
            out[f"{case}/fold_{k + 1}"] = m
        for key in ("lpd_full", "elpd", "p_i", "kfold_i", "stats"):
            out[f"{case}/{key}"] = r[key]
        out[f"{case}/K"] = np.array(r["K"])
        out[f"{case}/n_nan"] = np.array(r["n_nan"])
        for key, v in extra.items():
            out[f"{case}/{key}"] = v
        print(case, r["K"], r["stats"])
        return r

    rng = np.random.default_rng(20261017)
    # random: the reference's splitter, every S 256, log scale
    folds = kf._kfold_split_random(5, 60, seed=11)
    full = draws(rng, 60, 256)
    r = store("random", full, compact(rng, folds, [256] * 5), folds, "log")
    out["report/random"] = np.array(report(elpd_mod, r, 256, 60, "log", False))
    # ragged: S_k = 7, 64, 257, 1000 against a full fit of 400 draws, deviance; the same values as float32
    folds = kf._kfold_split_random(4, 47, seed=3)
    full, fl = draws(rng, 47, 400), compact(rng, folds, [7, 64, 257, 1000])
    store("ragged", full, fl, folds, "deviance")
    store("ragged_f32", full.astype(np.float32), [m.astype(np.float32) for m in fl], folds, "deviance")
    # stratified: a continuous x, and a 0/1 x
    x = rng.normal(size=40)
    folds = kf._kfold_split_stratified(3, x, seed=5)
    r = store("stratified", draws(rng, 40, 64), compact(rng, folds, [64, 48, 80]), folds, "log", x=x)
    out["report/stratified"] = np.array(report(elpd_mod, r, 64, 40, "log", True))
    x = (rng.uniform(size=40) < 0.3).astype(int)
    folds = kf._kfold_split_stratified(3, x, seed=6)
    store("stratified_binary", draws(rng, 40, 64), compact(rng, folds, [64, 64, 64]), folds, "log", x=x)
    # grouped: 9 groups over K 4; 3 groups under K 5 (the splitter lowers K to 3)
    g = rng.integers(0, 9, size=36)
    g[:9] = np.arange(9)
    folds = kf._kfold_split_grouped(4, g, seed=8)
    store("grouped", draws(rng, 36, 32), compact(rng, folds, [32, 40, 24, 32]), folds, "log", groups=g)
    g = np.repeat(np.array([10, 20, 30]), 4)
    folds = kf._kfold_split_grouped(5, g, seed=9)
    store("grouped_few", draws(rng, 12, 32), compact(rng, folds, [32] * 3), folds, "log", groups=g)
    # exact LOO: K = N
    folds = kf._kfold_split_random(12, 12, seed=2)
    store("loo_exact", draws(rng, 12, 100), compact(rng, folds, [100] * 12), folds, "log")
    # the user's folds: sizes 1, 4, 20, negative_log
    folds = rng.permutation(np.repeat(np.array([1, 2, 3]), [1, 4, 20]))
    store("user_folds", draws(rng, 25, 50), compact(rng, folds, [50, 30, 70]), folds, "negative_log")
    # NaN in the full matrix only
    folds = kf._kfold_split_random(3, 30, seed=4)
    full = draws(rng, 30, 64)
    full[rng.integers(0, 30, size=12), rng.integers(0, 64, size=12)] = np.nan
    store("nan_full", full, compact(rng, folds, [64] * 3), folds, "log")
    # extreme values: -1e10 entries, -inf entries, a held-out row of -inf, a row with +inf
    folds = kf._kfold_split_random(2, 20, seed=1)
    full, fl = draws(rng, 20, 32), compact(rng, folds, [32, 45])
    full[2, 5] = -1e10
    full[3, :] = -1e10
    full[4, 7] = -np.inf
    full[6, 1] = np.inf
    fl[0][0, 3] = -1e10
    fl[0][1, :] = -np.inf
    fl[0][2, 9] = -np.inf
    fl[1][0, 2] = np.inf
    fl[1][3, 40] = -np.inf
    store("extreme", full, fl, folds, "log")
    # fold arrays of the three splitters
    for K, N, seed in ((5, 23, 7), (10, 100, 0), (3, 3, 1)):
        out[f"split/random_{K}_{N}_{seed}"] = kf._kfold_split_random(K, N, seed=seed)
    xs = {"continuous": rng.normal(size=31), "discrete": rng.integers(0, 3, size=29), "string": np.array(list("abcabbcaacbbabc")),
          "single": np.ones(10)}
    for name, x in xs.items():
        out[f"split/stratified_{name}_x"] = x
        out[f"split/stratified_{name}"] = kf._kfold_split_stratified(4, x, seed=13)
    g = rng.integers(0, 7, size=40)
    out["split/grouped_groups"] = g
    out["split/grouped"] = kf._kfold_split_grouped(3, g, seed=21)
    np.savez_compressed(os.path.join(HERE, "kfold.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "kfold.npz")), "bytes")


if __name__ == "__main__":
    main()
