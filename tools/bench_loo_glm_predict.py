"""Times ``loo_glm_predict_from_design`` against what a user writes today in the same process.

    python tools/bench_loo_glm_predict.py [--n 200000] [--s 4000] [--reps 5] [--out profiles/loo_glm_predict_bench_<tag>.json]

Per family (Gaussian, binomial, Poisson at two scales of y) and P in {4, 64}, device-resident inputs, medians and quartiles of:
  fused       loo_glm_predict_from_design (generator -> weights pass -> predictive kernel, block by block)
  predict     the predictive kernel alone on resident log weights (log_weights=)
  loo_glm     loo_glm_from_design on the same inputs (the parent's fused pass: what the new pass adds to)
  yardstick   glm_log_lik(linpred=True) into a resident matrix, mu / v / the distribution function in torch, psislw of the
              log-likelihood, the weighted sums -- on a row block that fits next to its temporaries, scaled to N rows
Every timed region ends with a device synchronise; the first call of each kind is a warm-up and is not recorded.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quartiles(ts):
    q = np.percentile(np.asarray(ts), [25, 50, 75])
    return {"q25_ms": float(q[0]) * 1e3, "median_ms": float(q[1]) * 1e3, "q75_ms": float(q[2]) * 1e3, "n": len(ts)}


def timed(fn, reps, torch):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return quartiles(ts)


def model(torch, n, s, p, family, y_mean, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(n, p, device="cuda", dtype=torch.float64, generator=g)
    X[:, 0] = 1.0
    b0 = 0.5 * torch.randn(p, device="cuda", dtype=torch.float64, generator=g) / p ** 0.5
    b0[0] = float(np.log(y_mean)) if family == "poisson" else 0.0
    beta = b0 + 0.15 * torch.randn(s, p, device="cuda", dtype=torch.float64, generator=g) / p ** 0.5
    eta0 = X @ b0
    kw = {}
    if family == "gaussian":
        kw["sigma"] = torch.exp(0.1 * torch.randn(s, device="cuda", dtype=torch.float64, generator=g))
        y = eta0 + torch.randn(n, device="cuda", dtype=torch.float64, generator=g)
    elif family == "binomial":
        trials = torch.full((n,), 20.0, device="cuda", dtype=torch.float64)
        y = torch.binomial(trials, torch.sigmoid(eta0), generator=g)
        kw["trials"] = trials
    else:
        y = torch.poisson(torch.exp(eta0), generator=g).clamp(max=4096.0)
    return X, y, beta, kw


def yardstick(pl, torch, X, y, beta, family, kw):
    """What a user writes today: the resident eta and ll matrices, torch for mu and F, psislw, the weighted sums."""
    eta = pl.glm_log_lik(X, y, beta, family, linpred=True, **kw)
    ll = pl.glm_log_lik(X, y, beta, family, **kw)
    lw = pl.psislw(-ll)[0]
    w = torch.softmax(lw, dim=1)
    if family == "gaussian":
        mu = eta
        F = torch.special.ndtr((y[:, None] - eta) / kw["sigma"][None, :])
        F_lt = F
    elif family == "binomial":
        p = torch.sigmoid(eta)
        mu = kw["trials"][:, None] * p
        n = kw["trials"][:, None]
        # P(Y <= y) = I_{1-p}(n - y, y + 1): torch has no incomplete beta; the sum over the support is what runs today
        ks = torch.arange(0, int(kw["trials"].max().item()) + 1, device=X.device, dtype=torch.float64)[None, None, :]
        logpmf = (torch.lgamma(n + 1)[..., None] - torch.lgamma(ks + 1) - torch.lgamma((n[..., None] - ks).clamp(min=0) + 1)
                  + ks * torch.log(p)[..., None] + (n[..., None] - ks) * torch.log1p(-p)[..., None])
        pmf = torch.exp(logpmf) * (ks <= n[..., None])
        F = (pmf * (ks <= y[:, None, None])).sum(-1)
        F_lt = (pmf * (ks < y[:, None, None])).sum(-1)
    else:
        mu = torch.exp(eta)
        F = torch.special.gammaincc(y[:, None] + 1.0, mu)
        F_lt = torch.where(y[:, None] >= 1.0, torch.special.gammaincc(y[:, None].clamp(min=1.0), mu), torch.zeros_like(mu))
    return (w * mu).sum(1), (w * F).sum(1), (w * F_lt).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--s", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--yard-rows", type=int, default=20000, help="rows of the yardstick's block (scaled to --n)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import pyloo_amd as pl

    records = []
    cases = [("gaussian", None), ("binomial", None), ("poisson", 3.0), ("poisson", 300.0)]
    for family, y_mean in cases:
        for p in (4, 64):
            X, y, beta, kw = model(torch, a.n, a.s, p, family, y_mean or 1.0)
            rec = {"family": family, "y_mean": float(y.mean().item()), "n": a.n, "s": a.s, "p": p}
            rec["fused"] = timed(lambda: pl.loo_glm_predict_from_design(X, y, beta, family, **kw), a.reps, torch)
            rec["loo_glm"] = timed(lambda: pl.loo_glm_from_design(X, y, beta, family, **kw), a.reps, torch)
            nb = min(a.yard_rows, a.n)
            Xb, yb = X[:nb], y[:nb]
            kb = {k: (v[:nb] if k == "trials" else v) for k, v in kw.items()}
            lwb = pl.psislw(-pl.glm_log_lik(Xb, yb, beta, family, **kb))[0]
            rec["predict_alone_block"] = dict(timed(lambda: pl.loo_glm_predict_from_design(Xb, yb, beta, family, log_weights=lwb, **kb),
                                                    a.reps, torch), rows=nb)
            if family == "binomial":  # (the support sum holds (rows, S, 21) temporaries)
                nb = min(nb, 2000)
                Xb, yb, kb = X[:nb], y[:nb], {k: (v[:nb] if k == "trials" else v) for k, v in kw.items()}
            yd = timed(lambda: yardstick(pl, torch, Xb, yb, beta, family, kb), a.reps, torch)
            rec["yardstick_block"] = dict(yd, rows=nb)
            rec["yardstick_scaled_median_ms"] = yd["median_ms"] * a.n / nb
            rec["fused_over_yardstick"] = rec["fused"]["median_ms"] / rec["yardstick_scaled_median_ms"]
            rec["fused_over_loo_glm"] = rec["fused"]["median_ms"] / rec["loo_glm"]["median_ms"]
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del X, y, beta, lwb
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_loo_glm_predict.py", "device": torch.cuda.get_device_name(0), "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
