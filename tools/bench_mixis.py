#!/usr/bin/env python3
"""Secondary benchmark: Mix-IS-LOO (Engine.mixis_loo) on a device-resident matrix.

    python tools/bench_mixis.py [--obs N] [--draws S] [--layout draws|obs] [--dtype f64|f32] [--steps K] [--warmup W]

One step = Engine.mixis_loo without a c: pla_mixis_draw_lse (pass 1, c[s] over the observations) and pla_mixis_loo (pass 2, the
pointwise values over the draws, the scale and the aggregates).  Reported, each as the MEDIAN wall time of --steps synchronised
repetitions after --warmup unrecorded ones, with the minimum, the quartiles and the maximum beside it (the variants are timed in
rounds, one call of each per round): the call, each pass alone, and two yardsticks on the same device and matrix --
(a) the torch formulation, c = logsumexp(-ll, 0); logsumexp(-c, 0) - logsumexp(-ll - c, 1) in f64, and (b) twice one pla_waic
pass, which also reads the matrix once and takes one exponential per element: the floor this design can approach.  Algorithmic
bytes = the matrix twice; their fraction of 8 TB/s over the call.  One JSON line."""
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
    ap.add_argument("--obs", type=int, default=50_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--layout", choices=["draws", "obs"], default="draws")
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    from pyloo_amd._capi import env_overrides
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S = args.obs, args.draws
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    esz = 8 if args.dtype == "f64" else 4
    if args.layout == "draws":
        ll = torch.empty((N, S), dtype=dt, device="cuda")
        eng.fill_synthetic(ll, seed=0x5EED0200, k_lo=0.01, k_hi=0.05)
    else:
        buf = torch.empty((S, N), dtype=dt, device="cuda")  # (sample, obs) buffer viewed as (obs, sample): observations fastest
        eng.fill_synthetic(buf, seed=0x5EED0200, k_lo=0.01, k_hi=0.05)
        ll = buf.T
    torch.cuda.synchronize()

    def torch_way():
        x = -ll.double()
        c = torch.logsumexp(x, dim=0)
        return c, torch.logsumexp(-c, dim=0) - torch.logsumexp(x - c, dim=1)

    first = eng.mixis_draw_lse(ll)
    variants = {
        "call": lambda: eng.mixis_loo(ll),
        "pass1_draw_lse": lambda: eng.mixis_draw_lse(ll),
        "pass2_loo": lambda: eng.mixis_loo(ll, c=first["c"]),
        "torch_formulation": torch_way,
        "one_waic_pass": lambda: eng.waic(ll, 1.0),
    }
    # every variant warmed up, then timed in ROUNDS: one synchronised call of each per round, so that drift of the machine
    # falls on all of them alike
    out = {}
    for name, fn in variants.items():
        for _ in range(args.warmup):
            out[name] = fn()
        if name == "pass1_draw_lse":
            kernels = eng.last_kernels()
        if name == "pass2_loo":
            kernels += " | " + eng.last_kernels()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.steps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)

    def spread(ts):
        q = statistics.quantiles(ts, n=4)
        return {"median": statistics.median(ts), "min": min(ts), "q1": q[0], "q3": q[2], "max": max(ts)}

    stats = {name: spread(ts) for name, ts in times.items()}
    med = {name: st["median"] for name, st in stats.items()}
    med["two_waic_passes"] = 2 * med["one_waic_pass"]
    res, (c_t, elpd_t) = out["call"], out["torch_formulation"]
    call_ms = med["call"]
    alg = 2.0 * N * S * esz
    err = lambda a, b: float((a - b).abs().max())  # noqa: E731
    print(json.dumps({
        "metric": "mixis_ms_per_call", "value": call_ms, "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
        "config": {"workload": f"Engine.mixis_loo, synthetic {args.dtype} N={N}, S={S}, {args.layout} contiguous, device-resident"},
        "median_wall_ms": med, "spread_wall_ms": stats,
        "algorithmic_bytes": alg, "call_fraction_of_8tbps": alg / (call_ms * 1e-3) / 8e12,
        "exponentials_per_second": 2.0 * N * S / (call_ms * 1e-3),
        "call_over_torch_formulation": call_ms / med["torch_formulation"], "call_over_two_waic_passes": call_ms / med["two_waic_passes"],
        "max_abs_difference": {"c_vs_torch": err(res["c"], c_t), "loo_i_vs_torch": err(res["loo_i"], elpd_t)},
        "elpd_loo": float(res["agg"][1]), "kernels": kernels, "env": env_overrides(),
    }))


if __name__ == "__main__":
    main()
