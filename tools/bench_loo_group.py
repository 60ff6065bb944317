#!/usr/bin/env python3
"""Secondary benchmark: leave-one-group-out (pl.loo_group_from_matrix) on a device-resident matrix.

    python tools/bench_loo_group.py [--obs N] [--draws S] [--groups G] [--scatter] [--skew] [--layout draws|obs] [--dtype f64|f32]
                                    [--host] [--steps K] [--warmup W]

One step = pla_psis_loo_groups (the group sums, then the PSIS pass over the G rows) + the host packing of the result, with a
prebuilt device GroupIndex.  Reported next to it: the group-sum kernel's own event time (pla_group_sum, timed by the engine), the
time to build the GroupIndex on the device, algorithmic bytes N*S*sizeof(T) + 2*G*S*sizeof(T) (the matrix once, the sums written
and read back) and their fraction of 8 TB/s, and pl.loo_from_matrix of the same matrix as the yardstick.  Labels: contiguous
blocks by default, random with --scatter, one group holding half the observations with --skew.  --host: the matrix as a host
ndarray (step = pl.loo_group_from_matrix from host memory).  One JSON line."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--groups", type=int, default=10_000)
    ap.add_argument("--scatter", action="store_true")
    ap.add_argument("--skew", action="store_true")
    ap.add_argument("--layout", choices=["draws", "obs"], default="draws")
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch

    import pyloo_amd as pl
    from pyloo_amd._capi import env_overrides
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S, G = args.obs, args.draws, min(args.groups, args.obs)
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    esz = 8 if args.dtype == "f64" else 4
    if args.layout == "draws":
        ll = torch.empty((N, S), dtype=dt, device="cuda")
        eng.fill_synthetic(ll, seed=0x5EED0004, k_lo=0.01, k_hi=0.05)
    else:
        ll = torch.empty((S, N), dtype=dt, device="cuda")  # (sample, obs) buffer viewed as (obs, sample): observations fastest
        eng.fill_synthetic(ll, seed=0x5EED0004, k_lo=0.01, k_hi=0.05)
        ll = ll.T
    rng = np.random.default_rng(1)
    if args.skew:
        ids = rng.integers(1, G, size=N) if G > 1 else np.zeros(N, dtype=np.int64)
        ids[rng.random(N) < 0.5] = 0
    elif args.scatter:
        ids = rng.integers(0, G, size=N)
    else:
        ids = np.arange(N) * G // N
    labels = torch.as_tensor(ids).cuda()
    torch.cuda.synchronize()
    c0 = time.perf_counter()
    index = pl.group_index(labels)
    torch.cuda.synchronize()
    t_index = time.perf_counter() - c0
    G = index.n_groups
    src = ll.cpu().numpy() if args.host else ll
    warnings.simplefilter("ignore")
    for _ in range(args.warmup):
        out = pl.loo_group_from_matrix(src, index)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = pl.loo_group_from_matrix(src, index)
    torch.cuda.synchronize()
    dt_call = (time.perf_counter() - t0) / args.steps
    kernels = eng.last_kernels()
    # the group-sum kernel alone (device matrices: pla_group_sum with the engine's event timing)
    sum_ms = None
    if not args.host:
        eng.group_sum(ll, index)
        torch.cuda.synchronize()
        eng.set_timing(True)
        for _ in range(args.steps):
            eng.group_sum(ll, index)
        ms, launches = eng.kernel_ms()
        eng.set_timing(False)
        sum_ms = ms / max(launches, 1)
    for _ in range(args.warmup):
        full = pl.loo_from_matrix(ll)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        full = pl.loo_from_matrix(ll)
    torch.cuda.synchronize()
    dt_loo = (time.perf_counter() - t0) / args.steps
    alg = (float(N) * S + 2.0 * G * S) * esz
    kind = "skewed" if args.skew else ("scattered" if args.scatter else "contiguous")
    print(json.dumps({
        "metric": "loo_group_ms_per_call", "value": dt_call * 1e3, "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
        "config": {"workload": f"loo_group_from_matrix, synthetic {args.dtype} S={S} x N={N}, G={G} {kind} groups, "
                               f"{args.layout} contiguous, {'host ndarray' if args.host else 'device-resident'}"},
        "algorithmic_bytes": alg, "algorithmic_tb_per_s": alg / dt_call / 1e12,
        "group_sum_kernel_ms": sum_ms,
        "group_sum_fraction_of_8tbps": None if sum_ms is None else (float(N) * S + G * S) * esz / (sum_ms * 1e-3) / 8e12,
        "group_index_build_ms": t_index * 1e3,
        "loo_from_matrix_ms": dt_loo * 1e3,
        "elpd_logo": float(out["elpd_logo"]), "elpd_loo": float(full["elpd_loo"]),
        "kernels": kernels, "env": env_overrides(),
    }))


if __name__ == "__main__":
    main()
