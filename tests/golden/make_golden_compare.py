#!/usr/bin/env python3
"""Generate ``compare.npz`` (loo_compare) from the REAL reference.

Run only in the build container (the reference checkout does not exist on the GPU box):
``python tests/golden/make_golden_compare.py``

The reference's ``compare.py`` is loaded in place as ``pyloo.compare`` once its imports are placeholder modules (``arviz.data``,
``.elpd``, ``.loo``, ``.loo_kfold``, ``.loo_subsample``, ``.rcparams``, ``.waic``); its ``_stacking_weights``,
``_pseudo_bma_weights`` and ``_bb_pseudo_bma_weights`` then run on dictionaries that hold what they read.  ``elpd_diff`` and ``dse``
follow the arithmetic of ``loo_compare`` (compare.py:205-229).  Inputs come from ``compare_cases.py``; only the numbers the
reference computes are written.
"""

import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from compare_cases import BB_ALPHAS, BB_INPUT, BB_SAMPLES, BB_SEED, CASES, pointwise  # noqa: E402
from make_golden import REF  # noqa: E402


def load_compare():
    def placeholder(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    arviz = placeholder("arviz")
    arviz.data = placeholder("arviz.data", InferenceData=type("InferenceData", (), {}))
    pkg = placeholder("pyloo")
    pkg.__path__ = []
    placeholder("pyloo.elpd", ELPDData=type("ELPDData", (dict,), {}))
    placeholder("pyloo.loo", loo=None)
    placeholder("pyloo.loo_kfold", loo_kfold=None)
    placeholder("pyloo.loo_subsample", loo_subsample=None)
    placeholder("pyloo.rcparams", _validate_scale=lambda s: s)
    placeholder("pyloo.waic", waic=None)
    spec = importlib.util.spec_from_file_location("pyloo.compare", f"{REF}/compare.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules["pyloo.compare"] = m
    spec.loader.exec_module(m)
    return m


def elpds_of(x, scale):
    names = [f"m{k}" for k in range(x.shape[0])]
    return {n: {"loo_i": types.SimpleNamespace(values=x[k].copy()), "elpd_loo": float(x[k].sum()), "scale": scale}
            for k, n in enumerate(names)}, names


def main():
    cmp = load_compare()
    out = {}
    for case, (seed, K, N, scale, kind) in CASES.items():
        x = pointwise(seed, K, N, scale, kind)
        elpds, names = elpds_of(x, scale)
        elpd_values = np.array([elpds[n]["elpd_loo"] for n in names])
        order = np.argsort(elpd_values) if scale != "log" else np.argsort(-elpd_values)
        best = names[order[0]]
        diff, dse = np.zeros(K), np.zeros(K)
        for k, n in enumerate(names):  # compare.py:214-227, in model order
            if n == best:
                continue
            d = elpds[n]["elpd_loo"] - elpds[best]["elpd_loo"]
            diff[k] = d * (-1 if scale == "negative_log" else -2 if scale == "deviance" else 1)
            pw = elpds[n]["loo_i"].values - elpds[best]["loo_i"].values
            dse[k] = np.sqrt(len(pw) * np.var(pw))
        w_st = cmp._stacking_weights(elpds, "loo", scale)
        w_pb = cmp._pseudo_bma_weights(elpds, "loo", scale)
        out[f"{case}/elpd"] = elpd_values
        out[f"{case}/order"] = order
        out[f"{case}/elpd_diff"] = diff
        out[f"{case}/dse"] = dse
        out[f"{case}/stacking"] = np.array([w_st[n] for n in names])
        out[f"{case}/pseudo_bma"] = np.array([w_pb[n] for n in names])
        print(case, out[f"{case}/stacking"])
    seed, K, N, scale, kind = BB_INPUT
    x = pointwise(seed, K, N, scale, kind)
    elpds, names = elpds_of(x, scale)
    for alpha in BB_ALPHAS:
        w, ses = cmp._bb_pseudo_bma_weights(elpds, "loo", BB_SAMPLES, alpha, BB_SEED, scale)
        out[f"bb_a{alpha:g}/weights"] = np.array([w[n] for n in names])
        out[f"bb_a{alpha:g}/ses"] = np.array([ses[n] for n in names])
        print("bb", alpha, out[f"bb_a{alpha:g}/weights"], out[f"bb_a{alpha:g}/ses"])
    np.savez_compressed(os.path.join(HERE, "compare.npz"), **out)


if __name__ == "__main__":
    main()
