#!/usr/bin/env python3
"""Secondary benchmark: moment matching (pl.loo_moment_match) for B high-k observations x S draws x D parameters.

    python tools/bench_moment_match.py [--obs B] [--draws S] [--dim D] [--no-cov] [--steps K] [--warmup W] [--numpy-obs M]

The model is synthetic and lives on the device: y_i ~ N(mu, sigma) with theta = (mu, log sigma, D - 2 nuisance dimensions with a
N(0, 1) prior), the draws a seeded normal approximation mixed by a fixed matrix, B of the observations planted far from the rest.
Only those of them whose Pareto k exceeds 0 are processed by the call (``observations_processed``); the three kernel times are for
the full (B, S, D) batch.  Its callbacks are batched torch functions (``batched=True``).

One step = one pl.loo_moment_match call (wall time, callbacks included).  Reported next to it: the engine's event time of each of
the three new entry points on the (B, S, D) batch -- pla_mm_moments (with the covariance matrices unless --no-cov),
pla_mm_transform (with a matrix unless --no-cov) and pla_mm_ratios (the update ratios) -- and, as the yardstick, the same
arithmetic (moments, transform, ratios; no PSIS, no model) in a NumPy loop over M observations on the host, per observation and
scaled to B.  One JSON line."""
import argparse
import json
import math
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=256)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--no-cov", action="store_true")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--numpy-obs", type=int, default=16)
    args = ap.parse_args()
    import numpy as np
    import torch

    import pyloo_amd as pl
    from pyloo_amd._capi import env_overrides
    from pyloo_amd.engine import get_engine

    eng = get_engine(0)
    B, S, D, cov = args.obs, args.draws, max(args.dim, 2), not args.no_cov
    rng = np.random.default_rng(0x5EED)
    y = np.concatenate([rng.normal(size=64), rng.choice([-1.0, 1.0], size=B) * rng.uniform(3.0, 5.0, size=B)])
    n, sd = len(y), y.std(ddof=1)
    theta = rng.normal(size=(S, D))
    theta[:, 0] = y.mean() + theta[:, 0] * sd / math.sqrt(n)
    theta[:, 1] = math.log(sd) + theta[:, 1] / math.sqrt(2 * n)
    mix = np.eye(D) + 0.6 * rng.uniform(-1, 1, size=(D, D)) / math.sqrt(D)
    upars = torch.from_numpy(theta @ np.linalg.inv(mix)).cuda()
    mix_d, y_d = torch.from_numpy(mix).cuda(), torch.from_numpy(y).cuda()
    sum_y, sum_yy = float(y.sum()), float((y**2).sum())
    c = 0.5 * math.log(2 * math.pi)

    def log_prob(model, upars, **kw):
        th = upars @ mix_d
        mu, ls = th[..., 0], th[..., 1]
        lp = -n * ls - 0.5 * (sum_yy - 2 * mu * sum_y + n * mu * mu) * torch.exp(-2 * ls) - 0.5 * (mu / 10) ** 2 - 0.5 * (ls / 2) ** 2
        return lp - 0.5 * (th[..., 2:] ** 2).sum(-1)

    def log_lik_upars(model, upars, i, **kw):
        th = upars @ mix_d
        yi = y_d[i]
        yi = yi[:, None] if yi.dim() == 1 else yi
        return -c - th[..., 1] - 0.5 * (yi - th[..., 0]) ** 2 * torch.exp(-2 * th[..., 1])

    def log_lik(model, i, **kw):
        return log_lik_upars(model, upars[None] if getattr(i, "dim", lambda: 0)() == 1 else upars, i)

    cbs = dict(post_draws=lambda model, **kw: upars, unconstrain_pars=lambda model, pars, **kw: pars, log_lik_i=log_lik,
               log_prob_upars_fn=log_prob, log_lik_i_upars_fn=log_lik_upars)
    obs = torch.arange(64, n, device="cuda")
    ll = log_lik(None, obs)
    ll_all = torch.cat([log_lik(None, torch.arange(0, 64, device="cuda")), ll])
    loo0 = pl.loo_from_matrix(ll_all, pointwise=True)
    ks0 = loo0["pareto_k"].cpu().numpy()
    ks0[:64] = -1.0  # only the B outliers are processed
    data = {k: loo0[k] for k in loo0.index}
    data["pareto_k"], data["loo_i"] = ks0, loo0["loo_i"].cpu().numpy()
    loo0 = pl.ELPDData(data=list(data.values()), index=list(data.keys()))
    warnings.simplefilter("ignore")
    mm = sys.modules["pyloo_amd.loo_moment_match"]
    for _ in range(args.warmup):
        out = pl.loo_moment_match(None, loo0, k_threshold=0.0, cov=cov, batched=True, **cbs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = pl.loo_moment_match(None, loo0, k_threshold=0.0, cov=cov, batched=True, **cbs)
    torch.cuda.synchronize()
    dt_call = (time.perf_counter() - t0) / args.steps
    stages = sum(len(t["ks"]) for t in mm.last_trace.values())
    # ---- the three entry points alone, on the (B, S, D) batch
    U = upars[None].expand(B, S, D).contiguous()
    lw, _ = eng.importance_weights(-ll, pl.base.tail_count_for(S, 1.0), "psis")
    stats, covs = eng.mm_moments(U, lw, cov=cov)
    mapping = torch.eye(D, dtype=torch.float64, device="cuda")[None].expand(B, D, D).contiguous() if cov else None
    lp0 = log_prob(None, upars)

    def timed(f):
        f()
        torch.cuda.synchronize()
        eng.kernel_ms()
        eng.set_timing(True)
        for _ in range(args.steps):
            f()
        ms, launches = eng.kernel_ms()
        eng.set_timing(False)
        return ms / max(launches, 1)

    ms_moments = timed(lambda: eng.mm_moments(U, lw, cov=cov))
    ms_transform = timed(lambda: eng.mm_transform(U, stats[:, 0], stats[:, 1], mapping=mapping))
    ms_ratios = timed(lambda: eng.mm_ratios("update", ll, ll, lp0))
    # ---- the yardstick: the same arithmetic per observation in NumPy
    M = min(args.numpy_obs, B)
    Uh, lwh, llh, lph = upars.cpu().numpy(), lw[:M].cpu().numpy(), ll[:M].cpu().numpy(), lp0.cpu().numpy()
    t0 = time.perf_counter()
    for b in range(M):
        w = np.exp(lwh[b])
        mean, wmean = Uh.mean(axis=0), (w[:, None] * Uh).sum(axis=0)
        mii = ((w[:, None] * Uh**2).sum(axis=0) - wmean**2) * S / (S - 1)
        np.sqrt(mii / Uh.var(axis=0))
        if cov:
            np.cov(Uh, rowvar=False), np.cov(Uh, rowvar=False, aweights=w)
            new = (Uh - mean) @ np.eye(D).T + wmean
        else:
            new = (Uh - mean) + wmean
        lr = -llh[b] + lph - lph
        lr[np.isnan(lr)] = -np.inf
    dt_numpy = (time.perf_counter() - t0) / M
    del new
    print(json.dumps({
        "metric": "loo_moment_match_ms_per_call", "value": dt_call * 1e3, "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": "f64",
        "config": {"workload": f"loo_moment_match, synthetic batched torch model, B={B} observations x S={S} x D={D}, cov={cov}, "
                               "k_threshold=0, split=True, device-resident"},
        "observations_processed": len(mm.last_trace), "stages_evaluated": stages, "ms_per_stage_and_observation": dt_call * 1e3 / max(stages, 1),
        "mm_moments_kernel_ms": ms_moments, "mm_transform_kernel_ms": ms_transform, "mm_ratios_kernel_ms": ms_ratios,
        "numpy_arithmetic_ms_per_observation": dt_numpy * 1e3, "numpy_arithmetic_ms_for_batch": dt_numpy * 1e3 * B,
        "device_arithmetic_ms_for_batch": ms_moments + ms_transform + ms_ratios,
        "n_improved": int((out["pareto_k"] < ks0).sum()), "elpd_loo": float(out["elpd_loo"]),
        "kernels": eng.last_kernels(), "env": env_overrides(),
    }))


if __name__ == "__main__":
    main()
