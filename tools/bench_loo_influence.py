#!/usr/bin/env python3
"""Secondary benchmark: LOO influence (Engine.loo_influence) on a device-resident log-likelihood matrix.

    python tools/bench_loo_influence.py [--obs N] [--draws S] [--quantities 1,16,32,64] [--f32-quantities 64] [--steps K] [--warmup W]
                                        [--out profiles/loo_influence_bench]

One step = Engine.loo_influence on the log-likelihood and P draw-wise quantities: Z^T once, then per block of observations the
prepare kernel, the weights pass and the influence kernel (pla_loo_influence).  Reported per (dtype, P), each as the MEDIAN wall
time of --steps synchronised repetitions after --warmup unrecorded ones, with the minimum, the quartiles and the maximum beside it
(the variants are timed in rounds, one call of each per round):
  call                  the whole call
  weights_pass          pla_importance_weights alone on the already negated matrix (what the call runs between its kernels)
  kernel                influence_kernel alone (and Z^T's prepare kernel): kind="log_weights" on the weights, read in place
  user_route            the yardstick: importance_weights(-ll), then torch.softmax(lw, 1) @ z and @ z^2 -- rocBLAS on a materialised
                        N x S weight matrix
  call_block_64mb       the call in a fresh process with PLA_INGEST_BLOCK_MB=64 (the variable is read once per process)
With the kernel's time: the achieved rate of its 4 N S P matrix flops (two products), and that rate over the 78.6 TFLOP/s of the
data sheet's f64 matrix peak.  One JSON line; with --out also one file per dtype, <out>_<dtype>.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MATRIX_PEAK = 78.6e12  # MI355X data sheet, FP64 matrix


def spread(ts):
    q = statistics.quantiles(ts, n=4) if len(ts) > 1 else [ts[0]] * 3
    return {"median": statistics.median(ts), "min": min(ts), "q1": q[0], "q3": q[2], "max": max(ts)}


def timed(variants, steps, warmup, sync, last_kernels):
    out, kernels = {}, {}
    for name, fn in variants.items():
        for _ in range(warmup):
            out[name] = fn()
        kernels[name] = last_kernels()
    sync()
    times = {name: [] for name in variants}
    for _ in range(steps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            sync()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return out, kernels, {name: spread(ts) for name, ts in times.items()}


def run(eng, torch, N, S, dtype, quantities, steps, warmup, call_only):
    from pyloo_amd.base import tail_count_for

    dt = torch.float64 if dtype == "f64" else torch.float32
    M = tail_count_for(S, 1.0)
    ll = torch.empty((N, S), dtype=dt, device="cuda")
    eng.fill_synthetic(ll, seed=0x5EED0500, k_lo=0.05, k_hi=0.6)
    gen = torch.Generator(device="cuda").manual_seed(7)
    records = []
    neg = lw0 = None
    if not call_only:
        neg = -ll
        lw0, _ = eng.importance_weights(neg, M, "psis")
    for P in quantities:
        theta = torch.randn((S, P), dtype=torch.float64, device="cuda", generator=gen)
        cen, sc = theta.mean(dim=0), theta.std(dim=0, unbiased=True)
        z = ((theta - cen) / sc).to(dt)

        def user_route():
            lw, k = eng.importance_weights(neg, M, "psis")
            w = torch.softmax(lw, dim=1)
            return w @ z, w @ (z * z), k

        variants = {"call": lambda: eng.loo_influence(ll, theta, cen, sc, M, "psis", "loglik")}
        if not call_only:
            variants.update({
                "weights_pass": lambda: eng.importance_weights(neg, M, "psis"),
                "kernel": lambda: eng.loo_influence(lw0, theta, cen, sc, kind="log_weights"),
                "user_route": user_route,
            })
        out, kernels, stats = timed(variants, steps, warmup, torch.cuda.synchronize, eng.last_kernels)
        med = {name: st["median"] for name, st in stats.items()}
        rec = {"dtype": dtype, "n_quant": P, "median_wall_ms": med, "spread_wall_ms": stats, "kernels": kernels}
        if not call_only:
            res = out["call"]
            shift_u, m2_u, k_u = out["user_route"]
            flops = 4.0 * N * S * P
            best = med["kernel"]
            rec.update({
                "matrix_flops": flops, "kernel_flops_per_second": flops / (best * 1e-3),
                "kernel_fraction_of_f64_matrix_peak": flops / (best * 1e-3) / F64_MATRIX_PEAK,
                "kernel_weight_bytes_per_second": 2.0 * N * S * (8 if dtype == "f64" else 4) / (best * 1e-3),
                "call_over_user_route": med["call"] / med["user_route"],
                "max_difference_vs_user_route": {
                    "shift_abs": float((res["shift"] - shift_u).abs().max()), "m2_abs": float((res["m2"] - m2_u).abs().max()),
                    "pareto_k_abs": float((res["diag"] - k_u).abs().max())},
            })
            del res, shift_u, m2_u, k_u
        del out
        torch.cuda.empty_cache()
        records.append(rec)
    return records, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=200_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--quantities", default="1,16,32,64")
    ap.add_argument("--f32-quantities", default="64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="path prefix of the per-dtype JSON files")
    ap.add_argument("--call-only", action="store_true", help="time the call alone (the child run at another block size)")
    args = ap.parse_args()

    import torch

    from pyloo_amd._capi import env_overrides
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S = args.obs, args.draws
    parse = lambda text: [int(v) for v in text.split(",") if v]  # noqa: E731
    result = {}
    for dtype, quantities in (("f64", parse(args.quantities)), ("f32", parse(args.f32_quantities))):
        if not quantities:
            continue
        records, M = run(eng, torch, N, S, dtype, quantities, args.steps, args.warmup, args.call_only)
        torch.cuda.empty_cache()
        result[dtype] = records
    record = {
        "metric": "loo_influence_ms_per_call", "value": result[next(iter(result))][-1]["median_wall_ms"]["call"], "unit": "ms",
        "higher_is_better": False, "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "config": {"workload": f"Engine.loo_influence, synthetic N={N}, S={S}, log-likelihood draws contiguous, device-resident, "
                               f"tail count {M}, theta standard normal"},
        "results": result, "env": env_overrides(),
    }
    if args.call_only:
        print(json.dumps(record))
        return
    env = dict(os.environ, PLA_INGEST_BLOCK_MB="64")
    cmd = [sys.executable, os.path.abspath(__file__), "--call-only", "--obs", str(N), "--draws", str(S), "--quantities", args.quantities,
           "--f32-quantities", args.f32_quantities, "--steps", str(args.steps), "--warmup", str(args.warmup)]
    child = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if child.returncode != 0:
        raise RuntimeError("the run at PLA_INGEST_BLOCK_MB=64 failed:\n" + child.stderr[-2000:])
    small = json.loads(child.stdout.strip().split("\n")[-1])
    record["env_call_block_64mb"] = small["env"]
    for dtype, records in result.items():
        for rec, other in zip(records, small["results"][dtype]):
            rec["median_wall_ms"]["call_block_64mb"] = other["median_wall_ms"]["call"]
            rec["spread_wall_ms"]["call_block_64mb"] = other["spread_wall_ms"]["call"]
    if args.out:
        for dtype, records in result.items():
            with open(f"{args.out}_{dtype}.json", "w") as f:  # (the metric of a file: that dtype's last record)
                json.dump(dict(record, value=records[-1]["median_wall_ms"]["call"], results={dtype: records}), f, indent=1)
                f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
