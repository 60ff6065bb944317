#!/usr/bin/env python3
"""Secondary benchmark: K-fold cross-validation from per-fold log-likelihoods (Engine.kfold) on device-resident matrices.

    python tools/bench_kfold.py [--obs N] [--folds K] [--draws S] [--layout draws|obs] [--dtype f64|f32] [--form compact|full]
                                [--ragged] [--scattered] [--steps K] [--warmup W]

One step = Engine.kfold: the task index (torch: stable sort by fold), pla_kfold_lme (one ragged pass over the full fit and the K
fold matrices) and pla_kfold_reduce.  Reported, each as the MEDIAN wall time of --steps synchronised repetitions: the call, the
index build alone, the ragged kernels alone (the engine's event timing around pla_kfold_lme), and two yardsticks -- the way
available before this pass existed (per fold: index_select of the held-out rows where the matrix is in the full form,
Engine.waic(...)["lppd_i"], a torch scatter; plus Engine.waic of the full fit) and torch.logsumexp per fold.  Algorithmic bytes =
every held-out row and every row of the full fit once; their fraction of 8 TB/s over the kernel time.  --ragged: S_k runs from
S / 2 to 3 S / 2 over the folds; --scattered: random folds (default: contiguous blocks of observations).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=200_000)
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--layout", choices=["draws", "obs"], default="draws")
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--form", choices=["compact", "full"], default="compact")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--scattered", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import math

    import numpy as np
    import torch

    from pyloo_amd._capi import env_overrides
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, K, S = args.obs, args.folds, args.draws
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    esz = 8 if args.dtype == "f64" else 4
    folds = np.repeat(np.arange(1, K + 1), [len(c) for c in np.array_split(np.arange(N), K)])
    if args.scattered:
        folds = np.random.default_rng(3).permutation(folds)
    counts = np.bincount(folds - 1, minlength=K)
    draws = [max(8, int(S * (0.5 + k / max(K - 1, 1))) // 8 * 8) if args.ragged else S for k in range(K)]

    def matrix(n, s, seed):
        if args.layout == "draws":
            t = torch.empty((n, s), dtype=dt, device="cuda")
            eng.fill_synthetic(t, seed=seed, k_lo=0.01, k_hi=0.05)
            return t
        t = torch.empty((s, n), dtype=dt, device="cuda")  # (sample, obs) buffer viewed as (obs, sample): observations fastest
        eng.fill_synthetic(t, seed=seed, k_lo=0.01, k_hi=0.05)
        return t.T

    full = matrix(N, S, 0x5EED0100)
    mats = [matrix(N if args.form == "full" else int(counts[k]), draws[k], 0x5EED0101 + k) for k in range(K)]
    fdev = torch.from_numpy(folds).cuda()
    idx = [torch.nonzero(fdev == k + 1).reshape(-1) for k in range(K)]
    torch.cuda.synchronize()

    def median_ms(fn):
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return out, statistics.median(ts)

    res, call_ms = median_ms(lambda: eng.kfold(full, mats, fdev))
    kernels = eng.last_kernels()
    plan, index_ms = median_ms(lambda: eng._kfold_plan(full, mats, fdev))
    # the ragged kernels alone: the engine's events around pla_kfold_lme, one bracket per call
    per_call = []
    eng.set_timing(True)
    eng.kernel_ms()
    for _ in range(args.steps):
        eng._kfold_lme(plan)
        per_call.append(eng.kernel_ms()[0])
    eng.set_timing(False)
    kernel_ms = statistics.median(per_call)

    def earlier_way():
        elpd = torch.empty(N, dtype=torch.float64, device="cuda")
        lpd = eng.waic(full, 1.0)["lppd_i"]
        for k in range(K):
            m = mats[k].index_select(0, idx[k]) if args.form == "full" else mats[k]
            elpd[idx[k]] = eng.waic(m, 1.0)["lppd_i"]
        return lpd, elpd

    def torch_way():
        elpd = torch.empty(N, dtype=torch.float64, device="cuda")
        lpd = torch.logsumexp(full.double(), dim=1) - math.log(S)
        for k in range(K):
            m = mats[k].index_select(0, idx[k]) if args.form == "full" else mats[k]
            elpd[idx[k]] = torch.logsumexp(m.double(), dim=1) - math.log(draws[k])
        return lpd, elpd

    (lpd_w, elpd_w), waic_ms = median_ms(earlier_way)
    (lpd_t, elpd_t), torch_ms = median_ms(torch_way)
    alg = (float(N) * S + float(sum(int(c) * s for c, s in zip(counts, draws)))) * esz
    err = lambda a, b: float((a - b).abs().max())  # noqa: E731
    print(json.dumps({
        "metric": "kfold_ms_per_call", "value": call_ms, "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
        "config": {"workload": f"Engine.kfold, synthetic {args.dtype} N={N}, K={K}, S={S} ({'S_k ' + str(draws) if args.ragged else 'every S_k = S'}), "
                               f"{args.form} form, {args.layout} contiguous, {'scattered' if args.scattered else 'contiguous'} folds, device-resident"},
        "median_wall_ms": {"call": call_ms, "index_build": index_ms, "ragged_kernels": kernel_ms,
                           "per_fold_index_select_waic_scatter": waic_ms, "per_fold_torch_logsumexp": torch_ms},
        "algorithmic_bytes": alg, "kernel_fraction_of_8tbps": alg / (kernel_ms * 1e-3) / 8e12,
        "call_over_waic_way": call_ms / waic_ms, "call_over_torch_way": call_ms / torch_ms,
        "max_abs_difference": {"elpd_vs_waic_way": err(res["elpd_i"], elpd_w), "lpd_full_vs_waic_way": err(res["lpd_full_i"], lpd_w),
                               "elpd_vs_torch_way": err(res["elpd_i"], elpd_t)},
        "elpd_kfold": float(res["agg"][1]), "kernels": kernels, "env": env_overrides(),
    }))


if __name__ == "__main__":
    main()
