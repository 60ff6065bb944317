#!/usr/bin/env python3
"""Secondary benchmark: LOO diagnostics (Engine.loo_diag) and the per-observation reff on device-resident matrices.

    python tools/bench_loo_diagnostics.py [--obs N] [--draws S] [--dtype f64|f32] [--layout draws|obs] [--vector-obs N2]
                                          [--steps K] [--warmup W] [--vector-steps V] [--rho R] [--offset-sd D]

One step = Engine.loo_diag on the log-likelihood: per block of observations the prepare kernel, the weights pass and the
diagnostics kernel (pla_loo_diag).  Reported, each as the MEDIAN wall time of --steps synchronised repetitions after --warmup
unrecorded ones, with the minimum, the quartiles and the maximum beside it (the variants are timed in rounds, one call of each per
round):
  call                  the whole call at the default block size
  weights_pass          pla_importance_weights alone on the already negated matrix (what the call runs between its two kernels)
  diag_kernel           diag_wave_kernel alone: pla_loo_diag_weights on (log weights, ll), both matrices read in place
  prepare_by_difference call - weights_pass - diag_kernel: the prepare kernel (and the launches between), not a measurement of its own
  user_route            the yardstick: importance_weights(-ll), then the three sums written with torch operations
  call_block_64mb       the same call in a fresh process with PLA_INGEST_BLOCK_MB=64 (the variable is read once per process)
Bytes the call moves per observation: prepare reads and writes a row, the weights pass reads and writes it, the diagnostics kernel
reads the weights once and -ll three times -- eight rows of n_draws elements, six of them from HBM at most if the re-reads of -ll
hit L2 / MALL; the one read the problem needs is the floor.

The vector reff (--vector-obs N2 > 0): N2 rows of pla_fill_synthetic_chains (4 chains, AR(1)), r = relative_eff_from_matrix, then
  loo_vector_reff       pl.loo_from_matrix(ll, reff=r): one pla_psis_loo_rows pass per distinct tail count and a reduction
  loo_scalar_reff       pl.loo_from_matrix(ll, reff=float(r.mean())): the existing single pass, the yardstick
  diagnostics_vector_reff / diagnostics_scalar_reff   pl.loo_diagnostics_from_matrix likewise
with the number of buckets and their sizes beside them.  One JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=200_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--layout", choices=["draws", "obs"], default="draws")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vector-obs", type=int, default=200_000)
    ap.add_argument("--vector-steps", type=int, default=5)
    ap.add_argument("--rho", type=float, default=0.5, help="AR(1) coefficient of the chains of the vector-reff part")
    ap.add_argument("--offset-sd", type=float, default=0.0, help="spread of the chain offsets there (0: chains that have mixed)")
    ap.add_argument("--call-only", action="store_true", help="time the call alone (the child run at another block size)")
    args = ap.parse_args()

    import torch

    import pyloo_amd as pl
    from pyloo_amd._capi import env_overrides
    from pyloo_amd.base import tail_buckets, tail_count_for
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S = args.obs, args.draws
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    esz = 8 if args.dtype == "f64" else 4
    M = tail_count_for(S, 1.0)
    ll = torch.empty((N, S), dtype=dt, device="cuda")
    eng.fill_synthetic(ll, seed=0x5EED0400, k_lo=0.05, k_hi=0.6)
    if args.layout == "obs":
        ll = ll.T.contiguous().T  # the same values, observations fastest: the prepare kernel's tile route
    torch.cuda.synchronize()

    def user_route():
        lw, k = eng.importance_weights(-ll, M, "psis")
        lw, x = lw.to(torch.float64), ll.to(torch.float64)
        e = torch.exp(lw - lw.max(dim=1, keepdim=True).values)
        s1 = e.sum(dim=1)
        ess = s1 * s1 / (e * e).sum(dim=1)
        elpd = torch.logsumexp(lw + x, dim=1) - torch.logsumexp(lw, dim=1)
        t = e * (torch.exp(x - elpd.unsqueeze(1)) - 1.0)
        return elpd, ess, torch.log1p((t * t).sum(dim=1) / (s1 * s1)), k

    variants = {"call": lambda: eng.loo_diag(ll, M, "psis")}
    if not args.call_only:
        neg = -ll
        lw0, _ = eng.importance_weights(neg, M, "psis")
        llc = ll.contiguous()
        variants.update({
            "weights_pass": lambda: eng.importance_weights(neg, M, "psis"),
            "diag_kernel": lambda: eng.loo_diag_weights(lw0, llc),
            "user_route": user_route,
        })
    out, kernels, stats = timed(variants, args.steps, args.warmup, torch.cuda.synchronize, eng.last_kernels)
    med = {name: st["median"] for name, st in stats.items()}
    call_ms = med["call"]
    record = {
        "metric": "loo_diag_ms_per_call", "value": call_ms, "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
        "config": {"workload": f"Engine.loo_diag, synthetic {args.dtype} N={N}, S={S}, log-likelihood {args.layout} contiguous, "
                               f"device-resident, tail count {M}"},
        "median_wall_ms": med, "spread_wall_ms": stats, "kernels": kernels, "env": env_overrides(),
    }
    if args.call_only:
        print(json.dumps(record))
        return
    res = out["call"]
    elpd_u, ess_u, var_u, k_u = out["user_route"]
    moved = 8.0 * N * S * esz
    med["prepare_by_difference"] = call_ms - med["weights_pass"] - med["diag_kernel"]
    record.update({
        "bytes_moved_per_observation": moved / N, "bytes_needed_per_observation": 1.0 * S * esz,
        "call_bytes_per_second": moved / (call_ms * 1e-3),
        "diag_kernel_bytes_per_second_if_every_read_were_hbm": 4.0 * N * S * esz / (med["diag_kernel"] * 1e-3),
        "diag_kernel_bytes_per_second_of_the_two_rows": 2.0 * N * S * esz / (med["diag_kernel"] * 1e-3),
        "call_over_user_route": call_ms / med["user_route"],
        "max_difference_vs_user_route": {
            "elpd_i_abs": float((res["elpd_i"] - elpd_u).abs().max()), "ess_w_rel": float(((res["ess_w"] - ess_u) / ess_u).abs().max()),
            "var_log_rel": float(((res["var_log"] - var_u) / var_u).abs().max()), "pareto_k_abs": float((res["diag"] - k_u).abs().max())},
        "n_replaced": int(res["n_replaced"].item()),
    })
    env = dict(os.environ, PLA_INGEST_BLOCK_MB="64")
    cmd = [sys.executable, os.path.abspath(__file__), "--call-only", "--obs", str(N), "--draws", str(S), "--dtype", args.dtype,
           "--layout", args.layout, "--steps", str(args.steps), "--warmup", str(args.warmup)]
    del out, res, elpd_u, ess_u, var_u, k_u, lw0, neg, llc
    torch.cuda.empty_cache()
    child = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if child.returncode != 0:
        raise RuntimeError("the run at PLA_INGEST_BLOCK_MB=64 failed:\n" + child.stderr[-2000:])
    small = json.loads(child.stdout.strip().split("\n")[-1])
    med["call_block_64mb"] = small["median_wall_ms"]["call"]
    stats["call_block_64mb"] = small["spread_wall_ms"]["call"]
    record["env_call_block_64mb"] = small["env"]

    if args.vector_obs > 0:
        N2 = args.vector_obs
        del ll
        torch.cuda.empty_cache()
        chains = torch.empty((N2, S), dtype=dt, device="cuda")
        eng.fill_synthetic_chains(chains, seed=0x5EED0401, chains=4, rho=args.rho, offset_sd=args.offset_sd)
        if args.layout == "obs":
            chains = chains.T.contiguous().T  # the same values, observations fastest (the bucketed fronts copy such a matrix once per call)
        r = pl.relative_eff_from_matrix(chains, n_chains=4)
        valid = torch.isfinite(r) & (r > 0)
        r = torch.where(valid, r, torch.ones_like(r))
        r_mean = float(r.mean())
        _, buckets = tail_buckets(r, S)
        sizes = sorted(int(idx.numel()) for _, idx in buckets)

        def quiet(fn):
            def run():
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    return fn()
            return run

        vec = {
            "loo_vector_reff": quiet(lambda: pl.loo_from_matrix(chains, reff=r)),
            "loo_scalar_reff": quiet(lambda: pl.loo_from_matrix(chains, reff=r_mean)),
            "diagnostics_vector_reff": quiet(lambda: pl.loo_diagnostics_from_matrix(chains, reff=r)),
            "diagnostics_scalar_reff": quiet(lambda: pl.loo_diagnostics_from_matrix(chains, reff=r_mean)),
        }
        vout, vkernels, vstats = timed(vec, args.vector_steps, 1, torch.cuda.synchronize, eng.last_kernels)
        vmed = {name: st["median"] for name, st in vstats.items()}
        record["vector_reff"] = {
            "workload": f"pla_fill_synthetic_chains {args.dtype} N={N2}, S={S}, 4 chains, rho {args.rho}, offset_sd {args.offset_sd}; "
                        f"r = relative_eff_from_matrix; matrix {args.layout} contiguous",
            "steps": args.vector_steps, "warmup": 1, "n_buckets": len(buckets), "bucket_rows_min_median_max": [sizes[0], sizes[len(sizes) // 2], sizes[-1]],
            "tail_count_min_max": [buckets[0][0], buckets[-1][0]], "r_eff_mean": r_mean, "r_eff_min": float(r.min()), "r_eff_max": float(r.max()),
            "rows_with_invalid_r_eff_set_to_1": int((~valid).sum()),
            "median_wall_ms": vmed, "spread_wall_ms": vstats, "kernels": vkernels,
            "loo_vector_over_scalar": vmed["loo_vector_reff"] / vmed["loo_scalar_reff"],
            "diagnostics_vector_over_scalar": vmed["diagnostics_vector_reff"] / vmed["diagnostics_scalar_reff"],
            "ms_per_bucket_loo": (vmed["loo_vector_reff"] - vmed["loo_scalar_reff"]) / max(len(buckets), 1),
            "elpd_loo": {"vector": float(vout["loo_vector_reff"]["elpd_loo"]), "scalar": float(vout["loo_scalar_reff"]["elpd_loo"])},
            "mcse_elpd_loo": {"vector": vout["diagnostics_vector_reff"].mcse_elpd_loo, "scalar": vout["diagnostics_scalar_reff"].mcse_elpd_loo},
        }
    print(json.dumps(record))


if __name__ == "__main__":
    main()
