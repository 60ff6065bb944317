#!/usr/bin/env python3
"""Generate ``moment_match.npz`` (loo_moment_match) from the REAL reference.

Run only in the build container (the reference checkout does not exist on the GPU box):
``python tests/golden/make_golden_moment_match.py``

The reference's ``loo_moment_match.py`` and ``split_moment_match.py`` are loaded in place as ``pyloo.loo_moment_match`` /
``pyloo.split_moment_match`` and RUN -- the callback path, with the analytic model of ``tests/mm_models.py`` -- once the modules
they import and never reach here are placeholders (``pymc``, ``arviz``, ``pyloo.wrapper.pymc.pymc``) and
``tests/fake_xarray.py`` stands in for ``xarray``.  ``pyloo.base`` (``compute_importance_weights``), ``pyloo.psis``, ``pyloo.utils``,
``pyloo.helpers`` and ``pyloo.elpd`` are the real ones.  The reference's ``shift`` / ``shift_and_scale`` / ``shift_and_cov`` / ``update_quantities_i`` /
``loo_moment_match_split`` are wrapped by recorders, so that every stage's new k is known.

Only inputs and what the reference computed are written.  The generator asserts the conditions the tests rely on and moves to the
next seed when one fails: every accept / reject decision and every loop-exit test is at least 1e-3 away from its threshold.
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
sys.path.insert(0, os.path.dirname(HERE))
import fake_xarray  # noqa: E402

fake_xarray.apply_ufunc = None
sys.modules["xarray"] = fake_xarray
from make_golden import REF, load_reference  # noqa: E402
import mm_models  # noqa: E402

MARGIN = 1e-3
# dataset -> (S, D, correlated)
DATASETS = {"a": (400, 2, False), "a_mix": (400, 2, True), "b": (400, 1, False), "c": (1000, 5, True), "d": (1000, 17, True),
            "e": (400, 64, True)}
# run -> (dataset, k_threshold (None: the default), split, cov, max_iters)
RUNS = {
    "a_default": ("a", None, True, True, 30),
    "a_low": ("a", -0.05, True, True, 30),
    "a_low_nosplit": ("a", -0.05, False, True, 30),
    "a_low_nocov": ("a", -0.05, True, False, 30),
    "a_low_nosplit_nocov": ("a", -0.05, False, False, 30),
    "a_one_iter": ("a", None, True, True, 1),
    "a_mix_default": ("a_mix", None, True, True, 30),
    "a_mix_low": ("a_mix", -0.05, True, True, 30),
    "a_mix_low_nosplit": ("a_mix", -0.05, False, True, 30),
    "b_default": ("b", None, True, True, 30),
    "b_low": ("b", -0.05, True, True, 30),
    "c_default": ("c", None, True, True, 30),
    "c_low": ("c", -0.05, True, True, 30),
    "c_low_nosplit": ("c", -0.05, False, True, 30),
    "c_low_nocov": ("c", -0.05, True, False, 30),
    "d_default": ("d", None, True, True, 30),
    "d_low": ("d", -0.05, True, True, 30),
    "e_default": ("e", None, True, True, 30),
    "e_default_nocov": ("e", None, False, False, 30),
}


def load_moment_match():
    mods = load_reference()

    def placeholder(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    placeholder("pymc")
    az = sys.modules["arviz"]
    az.stats = placeholder("arviz.stats")
    az.stats.__path__ = []
    az.stats.diagnostics = placeholder("arviz.stats.diagnostics", ess=None)
    placeholder("pyloo.wrapper").__path__ = []
    placeholder("pyloo.wrapper.pymc").__path__ = []
    placeholder("pyloo.wrapper.pymc.pymc", PyMCWrapper=type("PyMCWrapper", (), {}))
    for name in ("helpers", "base", "elpd", "split_moment_match", "loo_moment_match"):
        spec = importlib.util.spec_from_file_location(f"pyloo.{name}", f"{REF}/{name}.py")
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"pyloo.{name}"] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods


class Recorder:
    """Wraps the reference's stage functions: ``calls`` = (observation, stage, k_new, kf_new) in call order, ``split`` = the
    observations that reached the split step, ``first`` = the first call of every stage function with what it returned."""

    def __init__(self, mm):
        self.mm, self.calls, self.split, self.first, self.stage = mm, [], [], {}, None
        self.real = {n: getattr(mm, n) for n in ("shift", "shift_and_scale", "shift_and_cov", "update_quantities_i", "loo_moment_match_split")}
        for tag, name in (("sh", "shift"), ("sc", "shift_and_scale"), ("co", "shift_and_cov")):
            setattr(mm, name, self._transform(tag, name))
        mm.update_quantities_i = self._update
        mm.loo_moment_match_split = self._split

    def restore(self):
        for n, f in self.real.items():
            setattr(self.mm, n, f)

    def _transform(self, tag, name):
        def wrapped(upars, lwi):
            self.stage = tag
            return self.real[name](upars, lwi)

        return wrapped

    def _update(self, model, upars, i, *a, **kw):
        out = self.real["update_quantities_i"](model, upars, i, *a, **kw)
        self.calls.append((int(i), self.stage, float(out["ki"]), float(out["kfi"])))
        return out

    def _split(self, model, upars, cov, ts, tsc, tm, i, r_eff_i, **kw):
        out = self.real["loo_moment_match_split"](model, upars, cov, ts, tsc, tm, i, r_eff_i, **kw)
        self.split.append(int(i))
        return out


def initial_loo(mods, model):
    """The pointwise LOO the reference would start from (loo.py:286-342 with its own primitives), as its ELPDData."""
    base, utils, elpd = mods["base"], mods["utils"], mods["elpd"]
    n, S = model.n, model.upars.shape[0]
    loo_i, lppd_i, ks = np.empty(n), np.empty(n), np.empty(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            ll = mm_models.log_lik_i(model, i)
            lw, k = base.compute_importance_weights(-ll)
            loo_i[i], lppd_i[i], ks[i] = utils._logsumexp(lw + ll), utils._logsumexp(ll, b_inv=S), k
    e = loo_i.sum()
    se = (n * np.var(loo_i)) ** 0.5
    good_k = min(1 - 1 / np.log10(S), 0.7)
    data = [e, se, lppd_i.sum() - e, np.sqrt(np.sum(np.var(loo_i))), S, n, bool(np.any(ks > good_k)),
            fake_xarray.DataArray(loo_i, dims=["obs"]), "log", -2 * e, 2 * se, fake_xarray.DataArray(ks, dims=["obs"]), good_k]
    index = ["elpd_loo", "se", "p_loo", "p_loo_se", "n_samples", "n_data_points", "warning", "loo_i", "scale", "looic", "looic_se",
             "pareto_k", "good_k"]
    return elpd.ELPDData(data=data, index=index)


def run_reference(mods, model, loo0, k_threshold, split, cov, max_iters):
    mm = mods["loo_moment_match"]
    rec = Recorder(mm)
    try:
        with warnings.catch_warnings(record=True) as caught, np.errstate(all="ignore"):
            warnings.simplefilter("always")
            out = mm.loo_moment_match(model, loo0, max_iters=max_iters, k_threshold=k_threshold, split=split, cov=cov,
                                      **mm_models.CALLBACKS)
    finally:
        rec.restore()
    S = model.upars.shape[0]
    thr = min(1 - 1 / np.log10(S), 0.7) if k_threshold is None else k_threshold
    ks0 = loo0.pareto_k.values
    kinds = ("sh", "sc", "co") if cov else ("sh", "sc")
    obs = [int(i) for i in np.where(ks0 > thr)[0]]
    decisions, traces, margin = [], [], np.inf
    for i in obs:
        k_cur, text, trace = ks0[i], "", []
        for (j, stage, k_new, _) in rec.calls:
            if j != i:
                continue
            margin = min(margin, abs(k_new - k_cur))
            text += stage + ("+" if k_new < k_cur else "-")
            trace.append(k_new)
            if k_new < k_cur:
                k_cur = k_new
            if stage == kinds[-1]:  # the end of a pass: the loop tests k against the threshold
                margin = min(margin, abs(k_cur - thr))
        decisions.append(text)
        traces.append(trace)
    return {
        "out": out, "obs": obs, "decisions": decisions, "traces": traces, "margin": margin, "split_obs": sorted(rec.split),
        "warnings": sorted({w.category.__name__ + ":" + str(w.message)[:40] for w in caught}),
        "n_warnings": len(caught),
    }


def first_stage(mods, model, obs):
    """The reference's three transforms and ``update_quantities_i`` on observation ``obs`` at the original draws."""
    mm, base = mods["loo_moment_match"], mods["base"]
    ll = mm_models.log_lik_i(model, obs)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lwi, _ = base.compute_importance_weights(-ll)
        lp0 = mm_models.log_prob_upars(model, model.upars)
        out = {"lwi": lwi, "obs": np.array(obs)}
        for tag, f in (("sh", mm.shift), ("sc", mm.shift_and_scale), ("co", mm.shift_and_cov)):
            res = f(model.upars, lwi)
            for k, v in res.items():
                out[f"{tag}_{k}"] = v
            q = mm.update_quantities_i(model, res["upars"], obs, lp0, 1.0, None, mm_models.log_prob_upars, mm_models.log_lik_i_upars)
            for k, v in q.items():
                out[f"{tag}_q_{k}"] = np.asarray(v)
    return out


def main():
    mods = load_moment_match()
    out = {}
    chosen = {}
    results = {}
    for ds, (S, D, mixed) in DATASETS.items():
        for seed in range(1, 400):
            model = mm_models.make_model(S, D, seed, mixed)
            loo0 = initial_loo(mods, model)
            runs = {name: run_reference(mods, model, loo0, thr, split, cov, iters)
                    for name, (d, thr, split, cov, iters) in RUNS.items() if d == ds}
            worst = min(r["margin"] for r in runs.values())
            empty = any(not r["obs"] for r in runs.values())
            if worst >= MARGIN and not empty:
                break
            print(f"  {ds}: seed {seed} rejected (margin {worst:.2e}, empty {empty})")
        else:
            raise SystemExit(f"no seed for {ds}")
        chosen[ds] = seed
        results.update(runs)
        out[f"data/{ds}/y"], out[f"data/{ds}/upars"] = model.y, model.upars
        out[f"data/{ds}/mix"] = np.zeros((0, 0)) if model.mix is None else model.mix
        out[f"data/{ds}/sigma"] = np.array(model.sigma)
        out[f"data/{ds}/seed"] = np.array(seed)
        out[f"data/{ds}/loo_i"], out[f"data/{ds}/pareto_k"] = loo0.loo_i.values, loo0.pareto_k.values
        out[f"data/{ds}/scalars"] = np.array([loo0[k] for k in ("elpd_loo", "se", "p_loo", "p_loo_se", "looic", "looic_se", "good_k")], dtype=float)
        if ds in ("a_mix", "b"):
            for k, v in first_stage(mods, model, int(np.argmax(loo0.pareto_k.values))).items():
                out[f"first/{ds}/{k}"] = v
        for name, r in runs.items():
            _, thr, split, cov, iters = RUNS[name]
            res = r["out"]
            out[f"run/{name}/settings"] = np.array([np.nan if thr is None else thr, float(split), float(cov), float(iters)])
            out[f"run/{name}/obs"] = np.array(r["obs"], dtype=np.int64)
            out[f"run/{name}/decisions"] = np.array(r["decisions"])
            out[f"run/{name}/trace"] = np.array([k for t in r["traces"] for k in t])
            out[f"run/{name}/trace_len"] = np.array([len(t) for t in r["traces"]], dtype=np.int64)
            out[f"run/{name}/split_obs"] = np.array(r["split_obs"], dtype=np.int64)
            out[f"run/{name}/warnings"] = np.array(r["warnings"])
            out[f"run/{name}/margin"] = np.array(r["margin"])
            out[f"run/{name}/loo_i"], out[f"run/{name}/pareto_k"] = res.loo_i.values, res.pareto_k.values
            out[f"run/{name}/p_loo_i"] = res.p_loo_i.values
            out[f"run/{name}/scalars"] = np.array([res[k] for k in ("elpd_loo", "se", "p_loo", "p_loo_se", "looic", "looic_se")], dtype=float)
            print(name, "seed", seed, "margin %.2e" % r["margin"], r["decisions"], "split", r["split_obs"], r["warnings"])
    # ---- the conditions across the file
    every = "".join(d for r in results.values() for d in r["decisions"])
    for tag in ("sh", "sc", "co"):
        assert tag + "+" in every and tag + "-" in every, f"stage {tag} is not both accepted and rejected somewhere"
    assert any(r["split_obs"] for r in results.values()), "no observation reaches the split step"
    assert any("Cholesky" in w for w in results["b_low"]["warnings"] + results["b_default"]["warnings"]), "D = 1 does not fall back"
    # ---- a row of -inf through the reference's PSIS
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lw, k = mods["base"].compute_importance_weights(np.full(400, -np.inf))
    out["neg_inf_row/lw"], out["neg_inf_row/k"] = lw, np.asarray(k, dtype=np.float64)
    path = os.path.join(HERE, "moment_match.npz")
    np.savez_compressed(path, **out)
    print("seeds", chosen, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
