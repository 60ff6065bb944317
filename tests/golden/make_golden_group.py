#!/usr/bin/env python3
"""Generate ``loo_group.npz`` (leave-one-group-out) from the REAL reference.

Run only in the build container (``/root/reference`` does not exist on the GPU box):
``python tests/golden/make_golden_group.py``

``loo_group()`` itself (``loo_group.py``) needs real xarray, so its lines 188-300 are chained here with the reference's own
primitives, loaded in place the way ``make_golden.py`` loads them (``base.py`` behind the same two placeholder modules):
NaN -> -1e10 (188-197), the group sums ``log_likelihood.values[group_ids == group].sum(axis=0)`` (216-224),
``compute_importance_weights(-group_log_lik, method, reff)`` per group (226-236), ``_logsumexp`` of the weighted rows and of
the group sums with ``b_inv = n_samples`` (262-298) and the sums / variances of 283-306.  f32 inputs are summed in f32 as the
reference does; the pass over the sums takes them in f64 (the parity target of every f32 golden).

Only inputs and the numbers the reference computes are written.
"""

import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, load_reference  # noqa: E402

SCALES = {"log": 1, "negative_log": -1, "deviance": -2}


def load_base(mods):
    spec = importlib.util.spec_from_file_location("pyloo.base", f"{REF}/base.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules["pyloo.base"] = m
    spec.loader.exec_module(m)
    mods["base"] = m
    return mods


def run_reference(mods, ll, group_ids, reff, method, scale):
    base, utils = mods["base"], mods["utils"]
    scale_value = SCALES[scale]
    n_samples = ll.shape[-1]
    has_nan = bool(np.any(np.isnan(ll)))
    if has_nan:
        ll = np.where(np.isnan(ll), ll.dtype.type(-1e10), ll)
    unique_groups = np.unique(group_ids)
    sums = np.array([ll[group_ids == g].sum(axis=0) for g in unique_groups])
    rows = sums.astype(np.float64)
    logo_i, lppd_i, diag = [], [], []
    for r in rows:
        lw, d = base.compute_importance_weights(-r, method=method, reff=reff)
        logo_i.append(scale_value * utils._logsumexp(lw + r))
        lppd_i.append(utils._logsumexp(r, b_inv=n_samples))
        diag.append(d)
    logo_i, lppd_i, diag = np.array(logo_i), np.array(lppd_i), np.array(diag, dtype=np.float64)
    G = len(unique_groups)
    good_k = min(1 - 1 / np.log10(n_samples), 0.7)
    elpd = logo_i.sum()
    se = (G * np.var(logo_i)) ** 0.5
    lppd = lppd_i.sum()
    if method == "psis":
        warn = bool(np.any(diag > good_k))
    else:
        warn = bool(np.min(diag) < n_samples * 0.1)
    return {
        "sums": sums, "logo_i": logo_i, "lppd_i": lppd_i, "diag": diag, "elpd_logo": elpd, "se": se,
        "p_logo": lppd - elpd / scale_value, "p_logo_se": np.sqrt(np.sum(np.var(logo_i))), "logoic": -2 * elpd,
        "logoic_se": 2 * se, "good_k": good_k, "warning": warn, "has_nan": has_nan, "n_high": int(np.sum(diag > good_k)),
        "min_diag": float(np.min(diag)), "labels": unique_groups,
    }


def make_cases():
    rng = np.random.default_rng(20261016)

    def smooth(n, s, k_lo=0.05, k_hi=0.5):
        k = rng.uniform(k_lo, k_hi, size=n)
        return -k[:, None] * rng.exponential(size=(n, s)) + rng.normal(-1.0, 0.3, size=(n, 1))

    cases = {}
    ll = smooth(60, 256)
    ids = rng.integers(0, 12, size=60)  # scattered integer labels
    cases["int_f64"] = (ll, ids, 0.8, "psis", "log")
    cases["int_f32"] = (ll.astype(np.float32), ids, 0.8, "psis", "log")
    ll = smooth(40, 250)
    ids = rng.choice(np.array(["county_b", "county_a", "site 3", "zz", "Åland"]), size=40)
    cases["str"] = (ll, ids, 1.0, "psis", "deviance")
    ll = smooth(30, 200)
    cases["singleton"] = (ll, np.arange(30), 1.0, "psis", "log")
    ll = smooth(36, 400)
    ll[5] = -1.6 * rng.standard_cauchy(size=400) ** 2 - 1.0  # one heavy-tailed observation: its group's k-hat > good_k
    ids = np.repeat(np.arange(6), 6)
    rng.shuffle(ids)
    cases["heavy"] = (ll, ids, 1.0, "psis", "log")
    ll = smooth(30, 200)
    ll[rng.integers(0, 30, size=12), rng.integers(0, 200, size=12)] = np.nan
    cases["nan"] = (ll, rng.integers(0, 5, size=30), 1.0, "psis", "log")
    ll = smooth(30, 200)
    ids = rng.integers(0, 6, size=30)
    cases["sis"] = (ll, ids, 1.0, "sis", "log")
    cases["tis"] = (ll, ids, 1.0, "tis", "negative_log")
    ll = smooth(20, 200)
    ll[3, ::7] = -1e10  # a group whose sum reaches -1e10 in those draws
    ll[11, 1::9] = 2.5e9
    cases["big"] = (ll, np.arange(20) % 4, 1.0, "psis", "log")
    return cases


def main():
    mods = load_base(load_reference())
    out = {}
    for name, (ll, ids, reff, method, scale) in make_cases().items():
        ref = run_reference(mods, ll, ids, reff, method, scale)
        out[f"{name}__ll"] = ll
        out[f"{name}__ids"] = ids
        out[f"{name}__meta"] = np.array([reff, {"psis": 0, "sis": 1, "tis": 2}[method], SCALES[scale]], dtype=np.float64)
        for k, v in ref.items():
            out[f"{name}__{k}"] = np.asarray(v)
    np.savez_compressed(os.path.join(HERE, "loo_group.npz"), **out)


if __name__ == "__main__":
    main()
