#!/usr/bin/env python3
"""Secondary benchmark: the relative efficiency of every row (Engine.relative_eff) of a device-resident log-likelihood matrix.

    python tools/bench_relative_eff.py [--obs N] [--draws S] [--chains C] [--rho R] [--offset-sd O] [--dtype f64|f32] [--layout draws|obs]
                                       [--steps K] [--warmup W] [--torch-steps T] [--torch-block B]

The rows are Engine.fill_synthetic_chains rows: C AR(1) chains with coefficient --rho, chain major, as MCMC delivers them (--offset-sd 0.3
adds the generator's per-chain offsets: chains that have not mixed, rows that Geyer's rule never stops).  One step = Engine.relative_eff(ll, C) (pla_relative_eff, log mode, no split).  Reported, each as the MEDIAN wall
time of --steps synchronised repetitions after --warmup unrecorded ones, with the minimum, the quartiles and the maximum beside it
(the variants are timed in rounds, one call of each per round):
  call          the whole call
  loo           the first yardstick: pl.loo_from_matrix on the same matrix with reff = the mean of the call's result
  torch_route   the second yardstick (--torch-steps repetitions, in blocks of --torch-block rows so that its temporaries fit): exp of
                the max-shifted rows, the autocovariances of all lags by torch.fft, Geyer's rule vectorised over the observations
and, from hipEvents around the launches (a run of the call of its own): ess_kernel, the device time of the row kernel per call;
observations fastest, transpose_by_difference = call - ess_kernel.  One JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ts):
    if len(ts) < 2:
        return {"median": ts[0], "min": ts[0], "q1": ts[0], "q3": ts[0], "max": ts[0]}
    q = statistics.quantiles(ts, n=4)
    return {"median": statistics.median(ts), "min": min(ts), "q1": q[0], "q3": q[2], "max": max(ts)}


def torch_relative_eff(ll, C, block):
    """exp, FFT autocovariances, Geyer's initial positive and monotone sequences, all observations of a block at once."""
    import torch

    N, S = ll.shape
    n = S // C
    out = torch.empty(N, dtype=torch.float64, device=ll.device)
    for r0 in range(0, N, block):
        x = ll[r0:r0 + block].double()
        x = torch.exp(x - x.max(dim=1, keepdim=True).values).reshape(-1, C, n)
        m = x.mean(dim=2)
        d = x - m[:, :, None]
        f = torch.fft.rfft(d, 2 * n, dim=2)
        A = (torch.fft.irfft(f * f.conj(), 2 * n, dim=2)[:, :, :n] / n).mean(dim=1)
        W = A[:, 0] * n / (n - 1)
        V = A[:, 0] + (m.var(dim=1, unbiased=True) if C > 1 else 0.0)
        rho = 1.0 - (W[:, None] - A) / V[:, None]
        rho[:, 0] = 1.0
        if n % 2:
            rho = torch.cat([rho, torch.zeros_like(rho[:, :1])], dim=1)
        even, pair = rho[:, 0::2], rho[:, 0::2] + rho[:, 1::2]
        k = torch.arange(pair.shape[1], device=ll.device)
        in_range = (2 * k < n - 1) | (k == 0)
        ahead = torch.cumprod(((pair > 0) & in_range).to(torch.int8), dim=1)  # every pair up to k is positive
        taken = torch.ones_like(ahead)
        taken[:, 1:] = ahead[:, :-1]
        taken = taken.bool() & in_range  # pair k was evaluated
        kept = torch.where(taken & (pair >= 0), pair, torch.zeros_like(pair))
        mono = torch.cummin(torch.where(taken & (pair >= 0), pair, torch.full_like(pair, math.inf)), dim=1).values
        total = torch.where(taken & (pair >= 0), torch.minimum(mono, kept), torch.zeros_like(pair)).sum(dim=1)
        last = taken.to(torch.int64).sum(dim=1) - 1
        e = even.gather(1, last[:, None])[:, 0]
        tau = torch.clamp(-1.0 + 2.0 * total + torch.clamp(e, min=0.0), min=1.0 / math.log10(S))
        out[r0:r0 + block] = torch.clamp(1.0 / tau, max=1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--rho", type=float, default=0.5)
    ap.add_argument("--offset-sd", type=float, default=0.0,
                    help="sd of the per-chain offsets (0: mixed chains; 0.3, the generator's default: chains that have not mixed)")
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--layout", choices=["draws", "obs"], default="draws")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=2)
    ap.add_argument("--torch-block", type=int, default=32768)
    args = ap.parse_args()

    import torch

    import pyloo_amd as pl
    from pyloo_amd._capi import env_overrides
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S, C = args.obs, args.draws, args.chains
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    esz = 8 if args.dtype == "f64" else 4
    ll = torch.empty((N, S), dtype=dt, device="cuda")
    eng.fill_synthetic_chains(ll, seed=0x5EED0500, chains=C, rho=args.rho, offset_sd=args.offset_sd)
    if args.layout == "obs":
        ll = ll.T.contiguous().T  # the same values, observations fastest
    torch.cuda.synchronize()

    r = eng.relative_eff(ll, C)
    reff = float(r["r_eff"].nanmean())
    variants = {"call": lambda: eng.relative_eff(ll, C), "loo": lambda: pl.loo_from_matrix(ll, reff=reff)}
    kernels = {}
    for name, fn in variants.items():
        for _ in range(args.warmup):
            fn()
        kernels[name] = eng.last_kernels()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.steps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    # the row kernel alone, from events around its launches
    eng.set_timing(True)
    eng.kernel_ms()
    for _ in range(args.steps):
        eng.relative_eff(ll, C)
    torch.cuda.synchronize()
    k_ms, k_launches = eng.kernel_ms()
    eng.set_timing(False)
    kernel_ms = k_ms / args.steps
    # the torch formulation
    times["torch_route"] = []
    r_torch = None
    for i in range(args.torch_steps + 1 if args.torch_steps > 0 else 0):
        t0 = time.perf_counter()
        r_torch = torch_relative_eff(ll, C, args.torch_block)
        torch.cuda.synchronize()
        if i > 0:
            times["torch_route"].append((time.perf_counter() - t0) * 1e3)

    stats = {name: spread(ts) for name, ts in times.items() if ts}
    med = {name: st["median"] for name, st in stats.items()}
    med["ess_kernel"] = kernel_ms
    if args.layout == "obs":
        med["transpose_by_difference"] = med["call"] - kernel_ms
    got = r["r_eff"]
    differ = (got - r_torch).abs() if r_torch is not None else torch.zeros_like(got)
    matrix_bytes = float(N) * S * esz
    record = {
        "metric": "relative_eff_ms_per_call", "value": med["call"], "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
        "config": {"workload": f"Engine.relative_eff, fill_synthetic_chains {args.dtype} N={N}, S={S} ({C} chains x {S // C}), rho={args.rho}, offset_sd={args.offset_sd}, "
                               f"{args.layout} contiguous, device-resident, log mode, no split"},
        "median_wall_ms": med, "spread_wall_ms": stats, "kernels": kernels, "kernel_launches_per_call": k_launches / args.steps,
        "env": env_overrides(), "bytes_of_the_matrix": matrix_bytes,
        "call_fraction_of_8tbps": matrix_bytes / (med["call"] * 1e-3) / 8e12,
        "ess_kernel_fraction_of_8tbps": matrix_bytes / (kernel_ms * 1e-3) / 8e12,
        "loo_fraction_of_8tbps": matrix_bytes / (med["loo"] * 1e-3) / 8e12,
        "call_over_loo": med["call"] / med["loo"],
        "call_over_torch_route": med["call"] / med["torch_route"] if "torch_route" in med else None,
        "mean_r_eff": reff, "min_r_eff": float(got.nan_to_num(1.0).min()), "n_invalid": int(r["n_invalid"].item()),
        "torch_route_block_rows": args.torch_block,
        "max_abs_difference_vs_torch_route": float(differ.nan_to_num(0.0).max()),
        "rows_differing_by_more_than_1e-6": int((differ > 1e-6).sum().item()),
    }
    print(json.dumps(record))


if __name__ == "__main__":
    main()
