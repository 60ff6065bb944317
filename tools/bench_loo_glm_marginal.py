#!/usr/bin/env python3
"""Secondary benchmark: cluster-marginal PSIS-LOO of a multilevel GLM (Engine.glm_marginal) against what a user writes today.

    python tools/bench_loo_glm_marginal.py [--obs N] [--draws S] [--predictors P] [--families gaussian,binomial,poisson]
                                           [--sizes 1,5,2000] [--nodes 7,15,32] [--steps K] [--warmup W] [--big-obs 4000000]
                                           [--big-size 4] [--out profiles/loo_glm_marginal_bench]

One step = Engine.glm_marginal(mode="loo"): the image of beta once, then per block of members the generator's linear predictor,
the segment kernel (and the join kernel for clusters longer than a segment) and the PSIS-LOO pass on the finished clusters
(pla_glm_marginal).  Clusters are runs of --sizes consecutive observations; the nodes are the fronts' without u: loc = 0, scale =
mean(tau).  Reported per (family, cluster size, nodes), each the MEDIAN wall time of --steps synchronised repetitions after --warmup
unrecorded ones with the quartiles beside it (timed in rounds, one call of each variant per round):
  call          the fused call
  matrix        the marginal matrix alone: mode="matrix" into a resident (C, S) buffer
  user_route    what a user writes today, same process, same visit: Engine.glm("linpred") into a resident (N, S) matrix, per node
                the density in torch and index_add_ over the clusters, the prior and log-weight, torch.logsumexp over the nodes
                (a running logaddexp where the (Q, C, S) stack would pass 32 GB), Engine.psis_loo on the result
and the kernel alone (pla_engine_kernel_ms over matrix-mode calls: the marginal kernels, summed over the blocks), its share of the call and its
density evaluations per second.  With --big-obs one more run, the fused call alone at a shape whose matrix is not held.
One JSON line; with --out also <out>_<family>.json and <out>_big.json."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_loo_glm import formula, make_model, timed  # noqa: E402

STACK_LIMIT = 32e9


def clustered(torch, N, S, P, family, size, n_nodes, seed):
    import numpy as np

    from pyloo_amd.loo_glm_marginal import gauss_hermite_nodes
    from pyloo_amd.loo_group import GroupIndex

    X, beta, v = make_model(torch, N, S, P, family, seed)
    gen = torch.Generator(device="cuda").manual_seed(seed + 1)
    tau = 0.5 * torch.exp(0.1 * torch.randn(S, dtype=torch.float64, device="cuda", generator=gen))
    C = (N + size - 1) // size
    cluster = torch.arange(N, device="cuda") // size
    offsets = torch.clamp(torch.arange(C + 1, device="cuda") * size, max=N)
    index = GroupIndex(np.arange(C), offsets, torch.arange(N, device="cuda"))
    nodes, logw = gauss_hermite_nodes(np.zeros(C), np.full(C, float(tau.mean())), n_nodes)
    return X, beta, v, tau, cluster, index, torch.as_tensor(nodes).cuda(), torch.as_tensor(logw).cuda()


def user_matrix(eng, torch, family, X, beta, v, tau, cluster, C, nodes, logw):
    """The (C, S) marginal matrix by the parts a user has today."""
    rest = eng.glm(X, beta, "linpred", offset=v["offset"])
    S, Q = rest.shape[1], nodes.shape[1]
    lt = -0.5 * math.log(2.0 * math.pi) - torch.log(tau)
    stack = Q * C * S * 8.0 <= STACK_LIMIT
    terms, acc = [], None
    for q in range(Q):
        ll = formula(torch, family, rest + nodes[cluster, q][:, None], v)
        e = torch.zeros((C, S), dtype=torch.float64, device=rest.device).index_add_(0, cluster, ll)
        e += (logw[:, q][:, None] + (lt[None, :] - 0.5 * (nodes[:, q][:, None] / tau[None, :]) ** 2))
        if stack:
            terms.append(e)
        else:
            acc = e if acc is None else torch.logaddexp(acc, e)
    return torch.logsumexp(torch.stack(terms), 0) if stack else acc


def run(eng, torch, N, S, P, family, sizes, node_counts, steps, warmup):
    from pyloo_amd.base import tail_count_for

    M = tail_count_for(S, 1.0)
    good_k = min(1 - 1 / math.log10(S), 0.7)
    records = []
    for size in sizes:
        for Q in node_counts:
            X, beta, v, tau, cluster, index, nodes, logw = clustered(torch, N, S, P, family, size, Q, 1000 + size)
            C = index.n_groups
            args = (X, beta, family, index, tau, nodes, logw)

            def user_route():
                return eng.psis_loo(user_matrix(eng, torch, family, X, beta, v, tau, cluster, C, nodes, logw), M, "psis", 1.0, good_k)

            variants = {
                "call": lambda: eng.glm_marginal(*args, mode="loo", tail_count=M, good_k=good_k, **v),
                "matrix": lambda: eng.glm_marginal(*args, **v),
                "user_route": user_route,
            }
            kernels, stats = timed(variants, steps, warmup, torch.cuda.synchronize, eng.last_kernels)
            med = {name: st["median"] for name, st in stats.items()}
            eng.set_timing(True)
            eng.kernel_ms()
            for _ in range(3):
                variants["matrix"]()  # (matrix mode: the marginal kernels are the only timed launches)
            torch.cuda.synchronize()
            k_ms, launches = eng.kernel_ms()
            eng.set_timing(False)
            kernel_ms = k_ms / 3.0
            fused, ref = variants["call"](), user_route()
            cap = 8 if Q <= 8 else 16 if Q <= 16 else 32
            records.append({
                "family": family, "cluster_size": size, "n_clusters": C, "n_nodes": Q, "node_capacity": cap, "n_pred": P,
                "median_wall_ms": med, "spread_wall_ms": stats, "kernels": kernels, "call_over_user_route": med["call"] / med["user_route"],
                "marginal_kernels_ms_per_call": kernel_ms, "marginal_kernel_launches_per_call": launches / 3.0,
                "marginal_kernels_share_of_call": kernel_ms / med["call"],
                "density_evaluations_per_second": float(N) * S * Q / (kernel_ms * 1e-3) if kernel_ms > 0 else None,
                "density_evaluations_per_second_with_padding": float(N) * S * cap / (kernel_ms * 1e-3) if kernel_ms > 0 else None,
                "max_difference_vs_user_route": {"loo_i_abs": float((fused["loo_i"] - ref["loo_i"]).abs().max()),
                                                 "pareto_k_abs": float((fused["diag"] - ref["diag"]).abs().max())},
                "pareto_k_max": float(ref["diag"].max()),
            })
            print(f"{family} size {size} nodes {Q}: call {med['call']:.1f} ms, user route {med['user_route']:.1f} ms, kernels {kernel_ms:.1f} ms",
                  file=sys.stderr, flush=True)
            del X, beta, v, tau, cluster, index, nodes, logw, fused, ref, args
            torch.cuda.empty_cache()
    return records, M


def big_run(eng, torch, N, S, P, size, Q, steps, warmup):
    from pyloo_amd.base import tail_count_for

    M = tail_count_for(S, 1.0)
    X, beta, v, tau, cluster, index, nodes, logw = clustered(torch, N, S, P, "poisson", size, Q, 77)
    call = lambda: eng.glm_marginal(X, beta, "poisson", index, tau, nodes, logw, mode="loo", tail_count=M, good_k=0.7, **v)  # noqa: E731
    kernels, stats = timed({"call": call}, steps, warmup, torch.cuda.synchronize, eng.last_kernels)
    res = call()
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return {"n_obs": N, "n_draws": S, "n_pred": P, "family": "poisson", "cluster_size": size, "n_clusters": index.n_groups, "n_nodes": Q,
            "spread_wall_ms": stats, "kernels": kernels, "matrix_bytes_never_held": 8.0 * N * S, "marginal_matrix_bytes_never_held": 8.0 * index.n_groups * S,
            "device_bytes_outside_torch_allocator": int(total - free - torch.cuda.memory_reserved()),
            "elpd_logo": float(res["agg"][1]), "n_high_k": float(res["agg"][4]), "n_replaced": int(res["n_replaced"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=200_000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--predictors", type=int, default=16)
    ap.add_argument("--families", default="gaussian,binomial,poisson")
    ap.add_argument("--sizes", default="1,5,2000")
    ap.add_argument("--nodes", default="7,15,32")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-obs", type=int, default=0, help="one more run of the fused call alone at this N (0: none)")
    ap.add_argument("--big-size", type=int, default=4)
    ap.add_argument("--big-nodes", type=int, default=15)
    ap.add_argument("--out", default="", help="path prefix of the JSON files")
    args = ap.parse_args()

    import torch

    from pyloo_amd._capi import env_overrides
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    N, S, P = args.obs, args.draws, args.predictors
    ints = lambda text: [int(t) for t in text.split(",") if t]  # noqa: E731
    result = {}
    M = 0
    for family in [f for f in args.families.split(",") if f]:
        result[family], M = run(eng, torch, N, S, P, family, ints(args.sizes), ints(args.nodes), args.steps, args.warmup)
    record = {
        "metric": "loo_glm_marginal_ms_per_call", "unit": "ms", "higher_is_better": False, "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "value": result[next(iter(result))][-1]["median_wall_ms"]["call"] if result else None,
        "config": {"workload": f"Engine.glm_marginal(mode='loo'), synthetic clustered GLM N={N}, S={S}, P={P}, device-resident inputs, "
                               f"tail count {M}, segment length {eng.glm_marginal_segment()}"},
        "results": result, "env": env_overrides(),
    }
    if args.big_obs:
        torch.cuda.empty_cache()
        record["big"] = big_run(eng, torch, args.big_obs, S, P, args.big_size, args.big_nodes, max(3, args.steps // 3), 1)
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
