#!/usr/bin/env python3
"""Secondary benchmark: PSIS-LOO of a GLM from its design matrix and draws (Engine.glm) against the materialised route.

    python tools/bench_loo_glm.py [--obs N] [--draws S] [--predictors 4,16,64] [--families gaussian,binomial,poisson] [--steps K]
                                  [--warmup W] [--big-obs 4000000] [--big-predictors 16] [--out profiles/loo_glm_bench]
(--families takes the engine's names: also negbinomial, gamma, binomial_probit)

One step = Engine.glm(mode="loo"): the image of beta once, then per block of observations the GLM kernel into the engine's block
buffer and the PSIS-LOO pass on the block (pla_glm).  Reported per (family, P), each as the MEDIAN wall time of --steps synchronised
repetitions after --warmup unrecorded ones, with the minimum, the quartiles and the maximum beside it (the variants are timed in
rounds, one call of each per round):
  call              the fused call
  kernel            the GLM kernel alone: mode="matrix" into a resident (N, S) buffer
  yard_matmul       the yardstick's first half: torch X @ beta.T + offset into a resident matrix (rocBLAS)
  yard_formula      its second half: the elementwise density in torch on that matrix
  loo_from_matrix   Engine.psis_loo on the materialised log-likelihood
  user_route        the three in a row: what a user writes today, same process, same visit
With --big-obs one more run, the fused call alone at a shape whose matrix is not held (N x S f64 beside its torch formulation):
its time and the device memory the process holds outside torch's allocator (the engine's workspace).  One JSON line; with --out
also one file per family, <out>_<family>.json, and <out>_big.json."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MATRIX_PEAK = 78.6e12  # MI355X data sheet, FP64 matrix


def spread(ts):
    q = statistics.quantiles(ts, n=4) if len(ts) > 1 else [ts[0]] * 3
    return {"median": statistics.median(ts), "min": min(ts), "q1": q[0], "q3": q[2], "max": max(ts)}


def timed(variants, steps, warmup, sync, last_kernels):
    kernels = {}
    for name, fn in variants.items():
        for _ in range(warmup):
            fn()
        kernels[name] = last_kernels()
    sync()
    times = {name: [] for name in variants}
    for _ in range(steps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            sync()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return kernels, {name: spread(ts) for name, ts in times.items()}


def make_model(torch, N, S, P, family, seed):
    """X ~ N(0, 1) with an intercept column, beta = b0 + 0.15 N(0, 1) / sqrt(P), y from the model at b0: Pareto k well below 0.7."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    X = rn(N, P)
    X[:, 0] = 1.0
    b0 = 0.5 * rn(P) / math.sqrt(P)
    beta = b0 + 0.15 * rn(S, P) / math.sqrt(P)
    offset = 0.3 * rn(N)
    eta0 = X @ b0 + offset
    v = dict(y=None, offset=offset, trials=None, obs_const=None, draw_scale=None, draw_const=None)
    if family == "gaussian":
        v["draw_scale"] = torch.exp(0.1 * rn(S))
        v["draw_const"] = -0.5 * math.log(2.0 * math.pi) - torch.log(v["draw_scale"])
        v["y"] = eta0 + rn(N)
    elif family == "binomial":
        v["trials"] = torch.full((N,), 10.0, dtype=torch.float64, device="cuda")
        v["y"] = torch.binomial(v["trials"], torch.sigmoid(eta0), generator=gen)
        v["obs_const"] = torch.lgamma(v["trials"] + 1.0) - torch.lgamma(v["y"] + 1.0) - torch.lgamma(v["trials"] - v["y"] + 1.0)
    elif family == "binomial_probit":
        v["trials"] = torch.full((N,), 10.0, dtype=torch.float64, device="cuda")
        v["y"] = torch.binomial(v["trials"], torch.special.ndtr(eta0), generator=gen)
        v["obs_const"] = torch.lgamma(v["trials"] + 1.0) - torch.lgamma(v["y"] + 1.0) - torch.lgamma(v["trials"] - v["y"] + 1.0)
    elif family == "negbinomial":  # NB2 with phi near 2: a gamma mixture of Poissons
        a = v["draw_scale"] = 2.0 * torch.exp(0.2 * rn(S))
        v["draw_const"] = a * torch.log(a) - torch.lgamma(a)
        rate = torch.distributions.Gamma(torch.full((N,), 2.0, dtype=torch.float64, device="cuda"), 2.0 / torch.exp(eta0)).sample()
        v["y"] = torch.poisson(rate, generator=gen)
        v["obs_const"] = -torch.lgamma(v["y"] + 1.0)
    elif family == "gamma":  # shape near 3, mean exp(eta)
        a = v["draw_scale"] = 3.0 * torch.exp(0.2 * rn(S))
        v["draw_const"] = a * torch.log(a) - torch.lgamma(a)
        v["y"] = torch.distributions.Gamma(torch.full((N,), 3.0, dtype=torch.float64, device="cuda"), 3.0 / torch.exp(eta0)).sample()
        v["obs_const"] = torch.log(v["y"])
    else:
        v["y"] = torch.poisson(torch.exp(eta0), generator=gen)
        v["obs_const"] = -torch.lgamma(v["y"] + 1.0)
    return X, beta, v


def formula(torch, family, eta, v):
    y = v["y"][:, None]
    if family == "gaussian":
        return v["draw_const"][None, :] - 0.5 * ((y - eta) / v["draw_scale"][None, :]) ** 2
    if family == "binomial":
        sp = torch.clamp(eta, min=0.0) + torch.log1p(torch.exp(-eta.abs()))
        return v["obs_const"][:, None] + y * eta - v["trials"][:, None] * sp
    if family == "binomial_probit":
        return v["obs_const"][:, None] + y * torch.special.log_ndtr(eta) + (v["trials"][:, None] - y) * torch.special.log_ndtr(-eta)
    if family == "negbinomial":
        a = v["draw_scale"][None, :]
        L = torch.logaddexp(eta, torch.log(a))
        return v["obs_const"][:, None] + v["draw_const"][None, :] + torch.lgamma(y + a) + y * eta - (y + a) * L
    if family == "gamma":
        a = v["draw_scale"][None, :]
        return v["draw_const"][None, :] + (a - 1.0) * v["obs_const"][:, None] - a * (eta + y * torch.exp(-eta))
    return v["obs_const"][:, None] + y * eta - torch.exp(eta)


def run(eng, torch, N, S, family, predictors, steps, warmup):
    from pyloo_amd.base import tail_count_for

    M = tail_count_for(S, 1.0)
    good_k = min(1 - 1 / math.log10(S), 0.7)
    records = []
    for P in predictors:
        X, beta, v = make_model(torch, N, S, P, family, 1000 + P)
        matmul = lambda: torch.addmm(v["offset"][:, None].expand(N, S), X, beta.T)  # noqa: E731
        eta = matmul()
        ll = formula(torch, family, eta, v)

        def user_route():
            return eng.psis_loo(formula(torch, family, matmul(), v), M, "psis", 1.0, good_k)

        variants = {
            "call": lambda: eng.glm(X, beta, family, mode="loo", tail_count=M, good_k=good_k, **v),
            "kernel": lambda: eng.glm(X, beta, family, **v),
            "yard_matmul": matmul,
            "yard_formula": lambda: formula(torch, family, eta, v),
            "loo_from_matrix": lambda: eng.psis_loo(ll, M, "psis", 1.0, good_k),
            "user_route": user_route,
        }
        kernels, stats = timed(variants, steps, warmup, torch.cuda.synchronize, eng.last_kernels)
        med = {name: st["median"] for name, st in stats.items()}
        fused, plain = variants["call"](), variants["loo_from_matrix"]()
        flops = 2.0 * N * S * P
        records.append({
            "family": family, "n_pred": P, "median_wall_ms": med, "spread_wall_ms": stats, "kernels": kernels,
            "call_over_user_route": med["call"] / med["user_route"],
            "kernel_over_yard_matmul_plus_formula": med["kernel"] / (med["yard_matmul"] + med["yard_formula"]),
            "kernel_matrix_flops_per_second": flops / (med["kernel"] * 1e-3),
            "kernel_store_bytes_per_second": 8.0 * N * S / (med["kernel"] * 1e-3),
            "max_difference_vs_user_route": {
                "loo_i_abs": float((fused["loo_i"] - plain["loo_i"]).abs().max()), "pareto_k_abs": float((fused["diag"] - plain["diag"]).abs().max()),
                "ll_abs_over_max_1_ll": float(((variants["kernel"]() - ll).abs() / ll.abs().clamp(min=1.0)).max())},
            "pareto_k_max": float(plain["diag"].max()),
        })
        del eta, ll, fused, plain, X, beta, v
        torch.cuda.empty_cache()
    return records, M


def big_run(eng, torch, N, S, P, steps, warmup):
    from pyloo_amd.base import tail_count_for

    M = tail_count_for(S, 1.0)
    X, beta, v = make_model(torch, N, S, P, "poisson", 77)
    call = lambda: eng.glm(X, beta, "poisson", mode="loo", tail_count=M, good_k=0.7, pointwise=True, **v)  # noqa: E731
    kernels, stats = timed({"call": call}, steps, warmup, torch.cuda.synchronize, eng.last_kernels)
    res = call()
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return {"n_obs": N, "n_draws": S, "n_pred": P, "family": "poisson", "spread_wall_ms": stats, "kernels": kernels,
            "matrix_bytes_never_held": 8.0 * N * S, "inputs_bytes": 8.0 * (N * P + S * P + 3 * N),
            "device_bytes_outside_torch_allocator": int(total - free - torch.cuda.memory_reserved()),
            "elpd_loo": float(res["agg"][1]), "n_high_k": float(res["agg"][4]), "n_replaced": int(res["n_replaced"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=200_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--predictors", default="4,16,64")
    ap.add_argument("--families", default="gaussian,binomial,poisson")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-obs", type=int, default=0, help="one more run of the fused call alone at this N (0: none)")
    ap.add_argument("--big-predictors", type=int, default=16)
    ap.add_argument("--out", default="", help="path prefix of the JSON files")
    args = ap.parse_args()

    import torch

    from pyloo_amd._capi import env_overrides
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S = args.obs, args.draws
    predictors = [int(t) for t in args.predictors.split(",") if t]
    result = {}
    M = 0
    for family in [f for f in args.families.split(",") if f]:
        result[family], M = run(eng, torch, N, S, family, predictors, args.steps, args.warmup)
    record = {
        "metric": "loo_glm_ms_per_call", "unit": "ms", "higher_is_better": False, "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "value": result[next(iter(result))][-1]["median_wall_ms"]["call"] if result else None,
        "config": {"workload": f"Engine.glm(mode='loo'), synthetic GLM N={N}, S={S}, device-resident X and beta, tail count {M}"},
        "results": result, "env": env_overrides(),
    }
    if args.big_obs:
        torch.cuda.empty_cache()
        record["big"] = big_run(eng, torch, args.big_obs, S, args.big_predictors, max(3, args.steps // 3), 1)
    if args.out:
        for family, records in result.items():
            with open(f"{args.out}_{family}.json", "w") as f:
                json.dump(dict(record, value=records[-1]["median_wall_ms"]["call"], results={family: records}, big=None), f, indent=1)
                f.write("\n")
        if args.big_obs:
            with open(f"{args.out}_big.json", "w") as f:
                json.dump({k: record[k] for k in ("metric", "unit", "n_gpus", "env", "big")}, f, indent=1)
                f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
