#!/usr/bin/env python3
"""Secondary benchmark: PSIS-LOO of a multilevel GLM from its design matrix, draws and group-level terms (Engine.glm(groups=...))
against the materialised route and against the same call without terms.

    python tools/bench_loo_glm_terms.py [--obs N] [--draws S] [--predictors 4,64] [--families gaussian,binomial] [--terms 0,1,2,4]
                                        [--groups 100,10000] [--steps K] [--warmup W] [--big-obs 4000000] [--out profiles/loo_glm_terms_bench]

One step = Engine.glm(mode="loo", groups=terms): the images of beta and of the group effects once, then per block of observations
the tile kernel with the terms in its epilogue and the PSIS-LOO pass on the block (pla_glm_grouped).  Term t is a varying intercept
for even t and a varying slope (z ~ N(0, 1)) for odd t, G groups each; "shuffled": every index vector is uniform random, "sorted":
each is sorted, so a tile of 16 observations meets one or two groups per term.  Reported per (family, P, T, G, order), each the
MEDIAN wall time of --steps synchronised repetitions after --warmup unrecorded ones with the quartiles beside it (timed in rounds,
one call of each variant per round):
  call          the fused call
  kernel        the generator alone: mode="matrix" into a resident (N, S) buffer
  user_route    what a user writes today, same process, same visit: torch.addmm for X @ beta.T + offset into a resident matrix,
                u[:, g].T * z[:, None] added per term, the elementwise density in torch, Engine.psis_loo on the result
Two ratios per record: call / user_route, and call (and kernel) over the same shape with T = 0, also per term; with the bytes the
terms gather (T * N * S * 8, one 128-byte line per row, term and tile of draws) over the kernel's extra time.  With --big-obs one
more run, the fused call alone at a shape whose matrix is not held (Poisson, T = 2), with the device memory the process holds outside
torch's allocator.  One JSON line; with --out also <out>_<family>.json and <out>_big.json."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_loo_glm import formula, timed  # noqa: E402


def make_model(torch, N, S, P, family, n_terms, G, order, seed):
    """bench_loo_glm.make_model with group-level terms: u_t = u0_t + 0.1 N(0, 1), u0_t = 0.3 N(0, 1); y from the model at the centres."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    X = rn(N, P)
    X[:, 0] = 1.0
    b0 = 0.5 * rn(P) / math.sqrt(P)
    beta = b0 + 0.15 * rn(S, P) / math.sqrt(P)
    offset = 0.3 * rn(N)
    eta0 = X @ b0 + offset
    terms = []
    for t in range(n_terms):
        index = torch.randint(0, G, (N,), device="cuda", generator=gen)
        if order == "sorted":
            index = index.sort().values
        u0 = 0.3 * rn(G)
        u = u0 + 0.1 * rn(S, G)
        z = rn(N) if t % 2 == 1 else None
        eta0 = eta0 + (u0[index] if z is None else z * u0[index])
        terms.append((index.to(torch.int32), u, z))
    v = dict(y=None, offset=offset, trials=None, obs_const=None, draw_scale=None, draw_const=None)
    if family == "gaussian":
        v["draw_scale"] = torch.exp(0.1 * rn(S))
        v["draw_const"] = -0.5 * math.log(2.0 * math.pi) - torch.log(v["draw_scale"])
        v["y"] = eta0 + rn(N)
    elif family == "binomial":
        v["trials"] = torch.full((N,), 10.0, dtype=torch.float64, device="cuda")
        v["y"] = torch.binomial(v["trials"], torch.sigmoid(eta0), generator=gen)
        v["obs_const"] = torch.lgamma(v["trials"] + 1.0) - torch.lgamma(v["y"] + 1.0) - torch.lgamma(v["trials"] - v["y"] + 1.0)
    else:
        v["y"] = torch.poisson(torch.exp(eta0), generator=gen)
        v["obs_const"] = -torch.lgamma(v["y"] + 1.0)
    return X, beta, v, terms


def configs(term_counts, group_counts):
    for n_terms in term_counts:
        if n_terms == 0:
            yield 0, 0, "none"
            continue
        for G in group_counts:
            for order in ("sorted", "shuffled"):
                yield n_terms, G, order


def run(eng, torch, N, S, family, predictors, term_counts, group_counts, steps, warmup):
    from pyloo_amd.base import tail_count_for

    M = tail_count_for(S, 1.0)
    good_k = min(1 - 1 / math.log10(S), 0.7)
    s_pad = (S + 15) // 16 * 16
    records = []
    for P in predictors:
        plain = None
        for n_terms, G, order in configs(term_counts, group_counts):
            X, beta, v, terms = make_model(torch, N, S, P, family, n_terms, G, order, 1000 + P)
            index64 = [g.long() for g, _, _ in terms]

            def linpred():
                eta = torch.addmm(v["offset"][:, None].expand(N, S), X, beta.T)
                for g, (_, u, z) in zip(index64, terms):
                    eta += u[:, g].T if z is None else u[:, g].T * z[:, None]
                return eta

            def user_route():
                return eng.psis_loo(formula(torch, family, linpred(), v), M, "psis", 1.0, good_k)

            groups = dict(groups=terms) if terms else {}
            variants = {
                "call": lambda: eng.glm(X, beta, family, mode="loo", tail_count=M, good_k=good_k, **v, **groups),
                "kernel": lambda: eng.glm(X, beta, family, **v, **groups),
                "user_route": user_route,
            }
            kernels, stats = timed(variants, steps, warmup, torch.cuda.synchronize, eng.last_kernels)
            med = {name: st["median"] for name, st in stats.items()}
            fused, ref = variants["call"](), user_route()
            rec = {
                "family": family, "n_pred": P, "n_terms": n_terms, "n_groups": G, "rows": order, "median_wall_ms": med, "spread_wall_ms": stats,
                "kernels": kernels, "call_over_user_route": med["call"] / med["user_route"], "image_bytes": 8.0 * n_terms * G * s_pad,
                "max_difference_vs_user_route": {"loo_i_abs": float((fused["loo_i"] - ref["loo_i"]).abs().max()),
                                                 "pareto_k_abs": float((fused["diag"] - ref["diag"]).abs().max())},
                "pareto_k_max": float(ref["diag"].max()),
            }
            if n_terms == 0:
                plain = med
            elif plain is not None:
                extra = (med["kernel"] - plain["kernel"]) * 1e-3
                rec.update({
                    "call_over_no_terms": med["call"] / plain["call"], "kernel_over_no_terms": med["kernel"] / plain["kernel"],
                    "call_extra_ms_per_term": (med["call"] - plain["call"]) / n_terms,
                    "kernel_extra_ms_per_term": (med["kernel"] - plain["kernel"]) / n_terms,
                    "gather_bytes_per_second_of_kernel_extra": 8.0 * n_terms * N * S / extra if extra > 0 else None,
                })
            records.append(rec)
            del X, beta, v, terms, index64, fused, ref
            torch.cuda.empty_cache()
    return records, M


def big_run(eng, torch, N, S, P, G, steps, warmup):
    from pyloo_amd.base import tail_count_for

    M = tail_count_for(S, 1.0)
    X, beta, v, terms = make_model(torch, N, S, P, "poisson", 2, G, "shuffled", 77)
    call = lambda: eng.glm(X, beta, "poisson", mode="loo", tail_count=M, good_k=0.7, pointwise=True, groups=terms, **v)  # noqa: E731
    kernels, stats = timed({"call": call}, steps, warmup, torch.cuda.synchronize, eng.last_kernels)
    res = call()
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return {"n_obs": N, "n_draws": S, "n_pred": P, "family": "poisson", "n_terms": 2, "n_groups": G, "rows": "shuffled", "spread_wall_ms": stats,
            "kernels": kernels, "matrix_bytes_never_held": 8.0 * N * S, "inputs_bytes": 8.0 * (N * P + S * P + 3 * N + 2 * S * G + N) + 8.0 * N,
            "device_bytes_outside_torch_allocator": int(total - free - torch.cuda.memory_reserved()),
            "elpd_loo": float(res["agg"][1]), "n_high_k": float(res["agg"][4]), "n_replaced": int(res["n_replaced"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=200_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--predictors", default="4,64")
    ap.add_argument("--families", default="gaussian,binomial")
    ap.add_argument("--terms", default="0,1,2,4")
    ap.add_argument("--groups", default="100,10000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-obs", type=int, default=0, help="one more run of the fused call alone at this N (0: none)")
    ap.add_argument("--big-predictors", type=int, default=16)
    ap.add_argument("--big-groups", type=int, default=10000)
    ap.add_argument("--out", default="", help="path prefix of the JSON files")
    args = ap.parse_args()

    import torch

    from pyloo_amd._capi import env_overrides
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S = args.obs, args.draws
    ints = lambda text: [int(t) for t in text.split(",") if t]  # noqa: E731
    result = {}
    M = 0
    for family in [f for f in args.families.split(",") if f]:
        result[family], M = run(eng, torch, N, S, family, ints(args.predictors), ints(args.terms), ints(args.groups), args.steps, args.warmup)
    record = {
        "metric": "loo_glm_terms_ms_per_call", "unit": "ms", "higher_is_better": False, "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "value": result[next(iter(result))][-1]["median_wall_ms"]["call"] if result else None,
        "config": {"workload": f"Engine.glm(mode='loo', groups=...), synthetic multilevel GLM N={N}, S={S}, device-resident inputs, tail count {M}"},
        "results": result, "env": env_overrides(),
    }
    if args.big_obs:
        torch.cuda.empty_cache()
        record["big"] = big_run(eng, torch, args.big_obs, S, args.big_predictors, args.big_groups, max(3, args.steps // 3), 1)
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
