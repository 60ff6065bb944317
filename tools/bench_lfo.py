#!/usr/bin/env python3
"""Secondary benchmark: one pass of PSIS leave-future-out CV (Engine.lfo) on a device-resident matrix.

    python tools/bench_lfo.py [--obs N] [--draws S] [--dtype f64|f32] [--layout draws|obs] [--horizon M] [--first L]
                              [--steps K] [--warmup W] [--mode forward|backward]

One step = Engine.lfo over all the steps first .. N - M of one fit: per block of steps the prefix-sum kernels, the weights pass and
the predict kernel, then the first-above-threshold reduction (pla_lfo).  Reported, each as the MEDIAN wall time of --steps
synchronised repetitions after --warmup unrecorded ones, with the minimum, the quartiles and the maximum beside it (the variants
are timed in rounds, one call of each per round):
  call                  the whole call at the default block size
  ratios                pla_lfo_ratios alone: the three prefix-sum launches, the ratios written to a matrix of the caller's
  weights_pass          pla_importance_weights alone on those ratios (what the call runs between its kernels)
  predict_by_difference call - ratios - weights_pass: the predict kernel (and, observations fastest, the transposition, which the
                        ratios call runs too and is therefore counted once), not a measurement of its own
  torch_route           the yardstick, what a user can do with the entry points of the release before this one: torch.cumsum of the
                        rows, importance_weights, a window sum of the next M rows, torch.logsumexp twice, the first k above the
                        threshold
  call_block_64mb       the same call in a fresh process with PLA_INGEST_BLOCK_MB=64 (the variable is read once per process)
--mode backward times the backward pass (Engine.lfo(mode="backward") from the fit to all N observations, the same N - M - first + 1
steps walked downward) IN THE SAME RUN as the forward call at the same shape, which moves the same bytes, and as its own yardstick:
  call_backward         the whole backward call at the default block size
  call_forward          the forward call over the same steps
  torch_route_backward  the same torch route on the flipped rows: flip, cumsum, negate, importance_weights, a window sum,
                        torch.logsumexp twice, the first k above the threshold
One JSON line."""
import argparse
import json
import math
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
    ap.add_argument("--obs", type=int, default=20_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--layout", choices=["draws", "obs"], default="draws")
    ap.add_argument("--horizon", type=int, default=1)
    ap.add_argument("--first", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--call-only", action="store_true", help="time the call alone (the child run at another block size)")
    ap.add_argument("--mode", choices=["forward", "backward"], default="forward")
    args = ap.parse_args()

    import torch

    from pyloo_amd._capi import env_overrides
    from pyloo_amd.base import tail_count_for
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S, M, first = args.obs, args.draws, args.horizon, args.first
    n_steps = N - first - M + 1
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    esz = 8 if args.dtype == "f64" else 4
    tail = tail_count_for(S, 1.0)
    thr = 0.7
    ll = torch.empty((N, S), dtype=dt, device="cuda")
    eng.fill_synthetic(ll, seed=0x5EED0400, k_lo=0.05, k_hi=0.6)
    ll /= 40.0  # (sums of thousands of rows: ratios a PSIS fit can still work on for the first few hundred steps)
    if args.layout == "obs":
        ll = ll.T.contiguous().T  # the same values, observations fastest
    torch.cuda.synchronize()

    def torch_route():
        lr = torch.cumsum(ll[first:first + n_steps - 1].double(), 0)
        lw, k = eng.importance_weights(lr, tail, "psis")
        f = ll[first:first + n_steps].double()
        for m in range(1, M):
            f = f + ll[first + m:first + m + n_steps]
        elpd = torch.empty(n_steps, dtype=torch.float64, device="cuda")
        elpd[0] = torch.logsumexp(f[0], 0) - math.log(S)
        elpd[1:] = torch.logsumexp(lw + f[1:], 1) - torch.logsumexp(lw, 1)
        above = torch.nonzero(k > thr)
        high = int(above[0]) + 1 if above.numel() else n_steps
        return elpd, k, high

    if args.mode == "backward":
        return backward(args, eng, ll, tail, thr)

    variants = {"call": lambda: eng.lfo(ll, first, n_steps, M, tail, thr)}
    if not args.call_only:
        lr0 = eng.lfo_ratios(ll, first, n_steps)["ratios"]
        variants.update({
            "ratios": lambda: eng.lfo_ratios(ll, first, n_steps),
            "weights_pass": lambda: eng.importance_weights(lr0, tail, "psis"),
            "torch_route": torch_route,
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
        "metric": "lfo_ms_per_pass", "value": call_ms, "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
        "config": {"workload": f"Engine.lfo, synthetic {args.dtype} N={N}, S={S}, {args.layout} contiguous, first={first}, horizon={M}, "
                               f"{n_steps} steps, device-resident, tail count {tail}"},
        "median_wall_ms": med, "spread_wall_ms": stats, "kernels": kernels, "env": env_overrides(),
    }
    if not args.call_only:
        res = out["call"]
        elpd_t, k_t, high_t = out["torch_route"]
        k_call = res["diag"][1:]
        both = torch.isfinite(k_call) & torch.isfinite(k_t)
        # the call reads the matrix for totals, ratios and the M future rows, writes and reads the ratios and the weights
        moved = (2.0 + M) * n_steps * S * esz + 4.0 * n_steps * S * 8 + (2.0 * n_steps * S * esz if args.layout == "obs" else 0.0)
        med["predict_by_difference"] = call_ms - med["ratios"] - med["weights_pass"]
        record.update({
            "bytes_moved": moved, "bytes_of_the_matrix": float(n_steps) * S * esz, "call_bytes_per_second": moved / (call_ms * 1e-3),
            "ratios_bytes_per_second": (2.0 * n_steps * S * esz + n_steps * S * 8.0) / (med["ratios"] * 1e-3),
            "call_over_torch_route": call_ms / med["torch_route"],
            "max_abs_difference": {"elpd_vs_torch_route": float((res["elpd_i"] - elpd_t).abs().nan_to_num(0.0, 0.0, 0.0).max()),
                                   "pareto_k_vs_torch_route": float((k_call - k_t)[both].abs().max()) if bool(both.any()) else 0.0},
            "first_high": int(res["first_high"].item()), "first_high_torch_route": high_t, "n_replaced": int(res["n_replaced"].item()),
        })
        env = dict(os.environ, PLA_INGEST_BLOCK_MB="64")
        cmd = [sys.executable, os.path.abspath(__file__), "--call-only", "--obs", str(N), "--draws", str(S), "--dtype", args.dtype,
               "--layout", args.layout, "--horizon", str(M), "--first", str(first), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        child = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if child.returncode != 0:
            raise RuntimeError("the run at PLA_INGEST_BLOCK_MB=64 failed:\n" + child.stderr[-2000:])
        small = json.loads(child.stdout.strip().split("\n")[-1])
        med["call_block_64mb"] = small["median_wall_ms"]["call"]
        stats["call_block_64mb"] = small["spread_wall_ms"]["call"]
        record["env_call_block_64mb"] = small["env"]
    print(json.dumps(record))


def backward(args, eng, ll, tail, thr):
    import torch

    from pyloo_amd._capi import env_overrides

    N, S, M, first = args.obs, args.draws, args.horizon, args.first
    n_steps = N - first - M + 1  # t = N - M down to first
    esz = 8 if args.dtype == "f64" else 4

    def torch_route():
        cs = torch.cumsum(torch.flip(ll[first:], (0,)).double(), 0)  # cs[i] = ll[N - 1] + ... + ll[N - 1 - i]
        lr = -cs[M - 1:M - 1 + n_steps]                                  # step j = N - M - j removes rows N - M - j .. N - 1
        lw, k = eng.importance_weights(lr, tail, "psis")
        f = ll[first:first + n_steps].double()
        for m in range(1, M):
            f = f + ll[first + m:first + m + n_steps]
        f = torch.flip(f, (0,))
        elpd = torch.logsumexp(lw + f, 1) - torch.logsumexp(lw, 1)
        above = torch.nonzero(k > thr)
        high = int(above[0]) if above.numel() else n_steps
        return elpd, k, high

    variants = {
        "call_backward": lambda: eng.lfo(ll, N, n_steps, M, tail, thr, mode="backward"),
        "call_forward": lambda: eng.lfo(ll, first, n_steps, M, tail, thr),
        "torch_route_backward": torch_route,
    }
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
    res = out["call_backward"]
    elpd_t, k_t, high_t = out["torch_route_backward"]
    both = torch.isfinite(res["diag"]) & torch.isfinite(k_t)
    moved = (2.0 + M) * n_steps * S * esz + 4.0 * n_steps * S * 8 + (2.0 * n_steps * S * esz if args.layout == "obs" else 0.0)
    print(json.dumps({
        "metric": "lfo_backward_ms_per_pass", "value": med["call_backward"], "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
        "config": {"workload": f"Engine.lfo(mode='backward'), synthetic {args.dtype} N={N}, S={S}, {args.layout} contiguous, last={N}, "
                               f"horizon={M}, {n_steps} steps down to t={first}, device-resident, tail count {tail}"},
        "median_wall_ms": med, "spread_wall_ms": stats, "kernels": kernels, "env": env_overrides(),
        "bytes_moved": moved, "call_bytes_per_second": moved / (med["call_backward"] * 1e-3),
        "backward_over_forward": med["call_backward"] / med["call_forward"],
        "backward_over_torch_route": med["call_backward"] / med["torch_route_backward"],
        "max_abs_difference": {"elpd_vs_torch_route": float((res["elpd_i"] - elpd_t).abs().nan_to_num(0.0, 0.0, 0.0).max()),
                               "pareto_k_vs_torch_route": float((res["diag"] - k_t)[both].abs().max()) if bool(both.any()) else 0.0},
        "first_high": int(res["first_high"].item()), "first_high_torch_route": high_t, "n_replaced": int(res["n_replaced"].item()),
    }))


if __name__ == "__main__":
    main()
