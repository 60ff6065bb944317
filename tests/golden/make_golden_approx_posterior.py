#!/usr/bin/env python3
"""Generate ``approx_posterior.npz`` (PSIS-LOO for approximate posteriors) from the REAL reference.

Run only in the build container (the reference does not exist on the GPU box):
``python tests/golden/make_golden_approx_posterior.py``

``loo_approximate_posterior()`` itself (``loo_approximate_posterior.py``) needs arviz and real xarray, so its lines 223-348 are
chained here with the reference's own primitives, loaded in place the way ``make_golden.py`` / ``make_golden_group.py`` load them,
and with the ``importance_resample`` FUNCTION taken out of the reference's file at run time (``make_golden_resample.py``):
NaN -> -1e10 (223-232), ``indices = importance_resample(log_p, log_q, resample_method, seed)`` (256-261), the gather of the matrix
along the draw axis (263), the ratios ``-ll`` shifted by each observation's maximum (264-268),
``compute_importance_weights(ratios, method, reff)`` per observation (284-286), ``_logsumexp`` of the weighted resampled rows
(325-330) and of the resampled rows with ``b_inv = n_samples`` (335-343), and the sums / variances of 332-348.  f32 inputs are
gathered in f32; the pass takes the gathered rows in f64 (the parity target of every f32 golden).

The ``nonfinite`` case (log_p / log_q of resample.npz's case of that name) is the one in which the reference's resampling raises
and its announced fall-back "to original samples" then fails on an unbound name (line 279): the numbers recorded for it are the
same chain over the ORIGINAL draws (the identity index), i.e. what the announced fall-back computes.

Only inputs, the index arrays and the numbers the reference computes are written.
"""

import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402
from make_golden_group import SCALES, load_base  # noqa: E402
from make_golden_resample import load_function  # noqa: E402

METHODS = {"psis": 0, "sis": 1, "tis": 2}


def run_reference(mods, ll, idx, reff, method, scale):
    base, utils = mods["base"], mods["utils"]
    scale_value = SCALES[scale]
    n_obs, n_samples = ll.shape
    has_nan = bool(np.any(np.isnan(ll)))
    if has_nan:
        ll = np.where(np.isnan(ll), ll.dtype.type(-1e10), ll)
    gathered = ll[:, idx]  # (the reference gathers the (sample, obs) transpose along axis 0: line 263)
    rows = gathered.astype(np.float64)
    loo_i, lppd_i, diag = [], [], []
    for r in rows:
        ratios = -r
        ratios = ratios - np.max(ratios)
        lw, d = base.compute_importance_weights(ratios, method=method, reff=reff)
        loo_i.append(scale_value * utils._logsumexp(lw + r))
        lppd_i.append(utils._logsumexp(r, b_inv=n_samples))
        diag.append(d)
    loo_i, lppd_i, diag = np.array(loo_i), np.array(lppd_i), np.array(diag, dtype=np.float64)
    good_k = min(1 - 1 / np.log10(n_samples), 0.7)
    elpd = loo_i.sum()
    se = (n_obs * np.var(loo_i)) ** 0.5
    lppd = lppd_i.sum()
    warn = bool(np.any(diag > good_k)) if method == "psis" else bool(np.min(diag) < n_samples * 0.1)
    return {
        "loo_i": loo_i, "lppd_i": lppd_i, "diag": diag, "elpd_loo": elpd, "se": se,
        "p_loo": lppd - elpd / scale_value, "p_loo_se": np.sqrt(np.sum(np.var(loo_i))), "looic": -2 * elpd, "looic_se": 2 * se,
        "good_k": good_k, "warning": warn, "has_nan": has_nan, "n_high": int(np.sum(diag > good_k)), "min_diag": float(np.min(diag)),
    }


def make_cases():
    """name -> (ll, log_p, log_q, resample_method, seed, reff, method, scale)"""
    rng = np.random.default_rng(20261017)
    with np.load(os.path.join(HERE, "resample.npz")) as z:
        resample = {k: z[k] for k in z.files}

    def grid(x):  # multiples of 2^-12: exact in f32 and f64, and the file stays small
        return np.round(x * 4096.0) / 4096.0

    def smooth(n, s, k_lo=0.05, k_hi=0.5):
        k = rng.uniform(k_lo, k_hi, size=n)
        return grid(-k[:, None] * rng.exponential(size=(n, s)) + rng.normal(-1.0, 0.3, size=(n, 1)))

    def densities(s, spread):
        log_q = grid(rng.normal(size=s) - 3.0)
        return grid(log_q + spread * rng.standard_t(df=5, size=s)), log_q

    cases = {}
    # log_p / log_q / seed of resample.npz's cases 1 ("psis", seed 12) and 2 ("psir", seed 13), and of its non-finite case
    cases["psis_psis"] = (smooth(8, 2000), resample["c1_log_p"], resample["c1_log_q"], "psis", 12, 0.9, "psis", "log")
    cases["psir_psis"] = (smooth(8, 2000), resample["c2_log_p"], resample["c2_log_q"], "psir", 13, 1.0, "psis", "deviance")
    cases["nonfinite"] = (smooth(4, 2000), resample["nonfinite_log_p"], resample["nonfinite_log_q"], "psis", 17, 1.0, "psis", "log")
    cases["sis_sis"] = (smooth(10, 1000),) + densities(1000, 1.0) + ("sis", 21, 1.0, "sis", "negative_log")
    cases["psis_tis"] = (smooth(20, 500),) + densities(500, 0.5) + ("psis", 22, 1.0, "tis", "log")
    cases["psir_tis"] = (smooth(40, 100),) + densities(100, 1.0) + ("psir", 23, 1.0, "tis", "deviance")
    cases["sis_psis"] = (smooth(4, 4000),) + densities(4000, 1.5) + ("sis", 24, 0.7, "psis", "log")
    cases["psir_sis"] = (smooth(25, 400),) + densities(400, 2.0) + ("psir", 25, 1.0, "sis", "log")
    cases["f32"] = (smooth(20, 1000).astype(np.float32),) + densities(1000, 1.0) + ("psir", 26, 1.0, "psis", "log")
    ll = smooth(30, 300)
    ll[rng.integers(0, 30, size=12), rng.integers(0, 300, size=12)] = np.nan
    cases["nan"] = (ll,) + densities(300, 1.0) + ("psis", 27, 1.0, "psis", "log")
    ll = smooth(150, 200)
    for i in (5, 77, 120):  # heavy-tailed observations: k-hat > good_k
        ll[i] = grid(-1.6 * rng.standard_cauchy(size=200) ** 2 - 1.0)
    cases["heavy"] = (ll,) + densities(200, 1.0) + ("psir", 28, 1.0, "psis", "log")
    # (appended later; the cases above keep their draws from the generator) the two remaining resampler x method pairs ...
    cases["psis_sis"] = (smooth(12, 600),) + densities(600, 1.0) + ("psis", 29, 1.0, "sis", "deviance")
    cases["sis_tis"] = (smooth(12, 600),) + densities(600, 1.0) + ("sis", 30, 1.0, "tis", "negative_log")
    # ... and heavy-tailed observations under SIS / TIS: the minimum ESS falls below a tenth of the draws (the low-ESS warning)
    ll = smooth(20, 400)
    for i in (3, 11):
        ll[i] = grid(-1.6 * rng.standard_cauchy(size=400) ** 2 - 1.0)
    dens = densities(400, 1.0)
    cases["heavy_sis"] = (ll,) + dens + ("psis", 31, 1.0, "sis", "log")
    cases["heavy_tis"] = (ll,) + dens + ("psir", 32, 1.0, "tis", "log")
    return cases


def main():
    mods = load_base(load_reference())
    resample = load_function()
    out = {}
    for name, (ll, log_p, log_q, rmethod, seed, reff, method, scale) in make_cases().items():
        n_samples = ll.shape[1]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                idx = np.asarray(resample(log_p, log_q, method=rmethod, seed=seed), dtype=np.int64)
                fallback = False
            except Exception as e:  # noqa: BLE001  (loo_approximate_posterior.py:270-276)
                print(name, "resampling raised", type(e).__name__, e)
                idx = np.arange(n_samples, dtype=np.int64)
                fallback = True
        assert idx.shape == (n_samples,) and idx.min() >= 0 and idx.max() < n_samples
        ref = run_reference(mods, ll, idx, reff, method, scale)
        out[f"{name}__ll"] = ll
        out[f"{name}__log_p"] = log_p
        out[f"{name}__log_q"] = log_q
        out[f"{name}__idx"] = idx
        out[f"{name}__fallback"] = np.array(fallback)
        out[f"{name}__resample"] = np.array(rmethod)
        out[f"{name}__seed"] = np.array(seed)
        out[f"{name}__meta"] = np.array([reff, METHODS[method], SCALES[scale]], dtype=np.float64)
        for k, v in ref.items():
            out[f"{name}__{k}"] = np.asarray(v)
        print(name, ll.shape, ll.dtype, rmethod, method, scale, "distinct draws", len(np.unique(idx)), "elpd", ref["elpd_loo"],
              "warning", ref["warning"], "n_high", ref["n_high"])
    np.savez_compressed(os.path.join(HERE, "approx_posterior.npz"), **out)


if __name__ == "__main__":
    main()
