#!/usr/bin/env python3
"""Side bench of loo_compare's kernels (csrc/pla_compare.h) on a device-resident (K, N) pointwise matrix.

    python tools/bench_compare.py [--n 1000000] [--k 4 16] [--b 1000] [--reps 20] [--full]

One line per measurement: the moments pass, one stacking evaluation, the whole stacking call (SLSQP: evaluations and total ms)
and the Bayesian bootstrap at alpha 1 and 0.5.  Times are wall clock around the call with the device synchronised, median of
--reps.  --full adds the reference's arithmetic on the CPU (NumPy + SLSQP, the Dirichlet matrix of the bootstrap) at a smaller N
for scale.  bench.py is not involved.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, sync):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def matrix(K, N, device):
    import torch

    g = torch.Generator(device=device).manual_seed(K * 7919 + N)
    common = torch.randn(N, device=device, dtype=torch.float64, generator=g)
    rows = [-1.2 - 0.08 / K * k + 0.6 * common + 0.5 * torch.randn(N, device=device, dtype=torch.float64, generator=g) for k in range(K)]
    return torch.stack(rows)


def cpu_reference(x, b_samples, alpha):
    """The reference's arithmetic (compare.py:494-536, 551-577) on the host."""
    import scipy.stats as st
    from scipy import optimize

    K, N = x.shape
    t0 = time.perf_counter()
    pe = x.T.copy()
    ee = np.exp(pe - pe.max(axis=1, keepdims=True))

    def full(w):
        w = np.maximum(np.concatenate((w, [max(1.0 - np.sum(w), 0.0)])), 0)
        return w / np.sum(w)

    def obj(w):
        return -np.sum(np.log(ee @ full(w)))

    def grad(w):
        d = ee @ full(w)
        return -np.array([np.sum((ee[:, k] - ee[:, -1]) / d) for k in range(K - 1)])

    optimize.minimize(obj, np.full(K - 1, 1.0 / K), jac=grad, bounds=[(0.0, 1.0)] * (K - 1), method="SLSQP",
                      constraints=[{"type": "ineq", "fun": lambda v: 1.0 - np.sum(v)}, {"type": "ineq", "fun": np.sum}],
                      options={"ftol": 1e-12, "maxiter": 2000})
    t_stack = time.perf_counter() - t0
    t0 = time.perf_counter()
    bw = st.dirichlet.rvs(alpha=[alpha] * N, size=b_samples, random_state=np.random.RandomState(0))
    _ = bw @ (x.T * N)
    return t_stack * 1e3, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--b", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--cpu-n", type=int, default=20_000)
    args = ap.parse_args()

    import torch

    from pyloo_amd import compare
    from pyloo_amd.engine import get_engine

    dev = torch.device("cuda", torch.cuda.current_device())
    eng = get_engine(dev.index)
    sync = torch.cuda.synchronize
    for K in args.k:
        x = matrix(K, args.n, dev)
        w = np.full(K, 1.0 / K)
        eng.compare_moments(x, 0)
        eng.stacking_eval(x, w)
        base = {"K": K, "N": args.n}
        print(json.dumps({**base, "what": "compare_moments", "ms": timed(lambda: eng.compare_moments(x, 0), args.reps, sync),
                          "kernels": eng.last_kernels()}), flush=True)
        print(json.dumps({**base, "what": "stacking_eval", "ms": timed(lambda: eng.stacking_eval(x, w), args.reps, sync),
                          "bytes": x.numel() * 8}), flush=True)
        stats = {}
        compare._stacking(eng, x, K, 1.0, stats)
        n_eval = stats["evaluations"]
        ms = timed(lambda: compare._stacking(eng, x, K, 1.0), max(3, args.reps // 4), sync)
        print(json.dumps({**base, "what": "stacking (SLSQP)", "evaluations": n_eval, "ms": ms}), flush=True)
        for alpha in (1.0, 0.5):
            eng.bb_bootstrap(x, args.b, alpha, 1)
            ms = timed(lambda: eng.bb_bootstrap(x, args.b, alpha, 1), max(3, args.reps // 4), sync)
            gammas = args.b * args.n
            print(json.dumps({**base, "what": f"bb_bootstrap alpha={alpha:g}", "B": args.b, "ms": ms,
                              "gammas_per_s": gammas / (ms * 1e-3)}), flush=True)
        del x
        if args.full:
            xc = matrix(K, args.cpu_n, dev).cpu().numpy()
            t_st, t_bb = cpu_reference(xc, args.b, 1.0)
            print(json.dumps({"K": K, "N": args.cpu_n, "what": "reference arithmetic on the CPU", "stacking_ms": t_st,
                              "bb_ms": t_bb, "B": args.b}), flush=True)


if __name__ == "__main__":
    main()
