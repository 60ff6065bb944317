#!/usr/bin/env python3
"""Secondary benchmark: LOO-PIT (Engine.loo_pit) on device-resident matrices.

    python tools/bench_loo_pit.py [--obs N] [--draws S] [--dtype f64|f32] [--ll-layout draws|obs] [--yhat-layout draws|obs]
                                  [--steps K] [--warmup W]

One step = Engine.loo_pit on the log-likelihood: per block of observations the prepare kernel, the weights pass and the PIT kernel
(pla_loo_pit).  Reported, each as the MEDIAN wall time of --steps synchronised repetitions after --warmup unrecorded ones, with the
minimum, the quartiles and the maximum beside it (the variants are timed in rounds, one call of each per round):
  call                  the whole call at the default block size
  weights_pass          pla_importance_weights alone on the already negated matrix (what the call runs between its two kernels)
  pit_kernel            the PIT kernel alone: the call on log weights, both matrices read in place
  prepare_by_difference call - weights_pass - pit_kernel: the prepare kernel (and the launches between), not a measurement of its own
  user_route            the yardstick, what a user does today: importance_weights(-ll), an indicator matrix, e_loo
  call_block_64mb       the same call in a fresh process with PLA_INGEST_BLOCK_MB=64 (the variable is read once per process)
Bytes the call moves per observation: prepare reads and writes a row, the weights pass reads and writes it, the PIT kernel reads
two rows -- six rows of n_draws elements; the two reads the problem needs are the floor.  One JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median": statistics.median(ts), "min": min(ts), "q1": q[0], "q3": q[2], "max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=200_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--ll-layout", choices=["draws", "obs"], default="draws")
    ap.add_argument("--yhat-layout", choices=["draws", "obs"], default="draws")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--call-only", action="store_true", help="time the call alone (the child run at another block size)")
    args = ap.parse_args()

    import torch

    from pyloo_amd._capi import env_overrides
    from pyloo_amd.base import tail_count_for
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S = args.obs, args.draws
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    esz = 8 if args.dtype == "f64" else 4
    M = tail_count_for(S, 1.0)
    ll = torch.empty((N, S), dtype=dt, device="cuda")
    eng.fill_synthetic(ll, seed=0x5EED0300, k_lo=0.05, k_hi=0.6)
    if args.ll_layout == "obs":
        ll = ll.T.contiguous().T  # the same values, observations fastest: the prepare kernel's tile route
    gen = torch.Generator(device="cuda").manual_seed(7)
    if args.yhat_layout == "draws":
        yh = torch.randn((N, S), dtype=dt, device="cuda", generator=gen)
    else:
        yh = torch.randn((S, N), dtype=dt, device="cuda", generator=gen).T  # observations fastest, as ArviZ keeps it
    y = torch.randn(N, dtype=torch.float64, device="cuda", generator=gen)
    torch.cuda.synchronize()

    def user_route():
        lw, k = eng.importance_weights(-ll, M, "psis")
        ind = (yh <= y.unsqueeze(1).to(dt)).to(dt)
        return eng.e_loo(ind, lw)["mean"], k

    variants = {"call": lambda: eng.loo_pit(ll, yh, y, M, "psis")}
    if not args.call_only:
        neg = -ll
        lw0, _ = eng.importance_weights(neg, M, "psis")
        if args.ll_layout == "obs" and args.yhat_layout == "obs":
            lw0 = lw0.T.contiguous().T  # an observations-fastest pair: the lane kernel
        variants.update({
            "weights_pass": lambda: eng.importance_weights(neg, M, "psis"),
            "pit_kernel": lambda: eng.loo_pit(lw0, yh, y, 0, "psis", kind="log_weights"),
            "user_route": user_route,
        })
    out, kernels = {}, {}
    for name, fn in variants.items():
        for _ in range(args.warmup):
            out[name] = fn()
        kernels[name] = eng.last_kernels()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.steps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    stats = {name: spread(ts) for name, ts in times.items()}
    med = {name: st["median"] for name, st in stats.items()}
    call_ms = med["call"]
    record = {
        "metric": "loo_pit_ms_per_call", "value": call_ms, "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
        "config": {"workload": f"Engine.loo_pit, synthetic {args.dtype} N={N}, S={S}, log-likelihood {args.ll_layout} contiguous, y_hat "
                               f"{args.yhat_layout} contiguous, device-resident, tail count {M}"},
        "median_wall_ms": med, "spread_wall_ms": stats, "kernels": kernels, "env": env_overrides(),
    }
    if not args.call_only:
        res = out["call"]
        mean_u, k_u = out["user_route"]
        moved = 6.0 * N * S * esz + (2.0 * N * S * esz if args.yhat_layout == "obs" else 0.0)
        med["prepare_by_difference"] = call_ms - med["weights_pass"] - med["pit_kernel"]
        record.update({
            "bytes_moved_per_observation": moved / N, "bytes_needed_per_observation": 2.0 * S * esz,
            "call_bytes_per_second": moved / (call_ms * 1e-3),
            "pit_kernel_bytes_per_second": 2.0 * N * S * esz / (med["pit_kernel"] * 1e-3),
            "call_over_user_route": call_ms / med["user_route"],
            "max_abs_difference": {"pit_le_vs_user_route": float((res["pit_le"] - mean_u).abs().max()),
                                   "pareto_k_vs_user_route": float((res["diag"] - k_u).abs().max())},
            "n_replaced": int(res["n_replaced"].item()),
        })
        env = dict(os.environ, PLA_INGEST_BLOCK_MB="64")
        cmd = [sys.executable, os.path.abspath(__file__), "--call-only", "--obs", str(N), "--draws", str(S), "--dtype", args.dtype,
               "--ll-layout", args.ll_layout, "--yhat-layout", args.yhat_layout, "--steps", str(args.steps), "--warmup", str(args.warmup)]
        child = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if child.returncode != 0:
            raise RuntimeError("the run at PLA_INGEST_BLOCK_MB=64 failed:\n" + child.stderr[-2000:])
        small = json.loads(child.stdout.strip().split("\n")[-1])
        med["call_block_64mb"] = small["median_wall_ms"]["call"]
        stats["call_block_64mb"] = small["spread_wall_ms"]["call"]
        record["env_call_block_64mb"] = small["env"]
    print(json.dumps(record))


if __name__ == "__main__":
    main()
