#!/usr/bin/env python3
"""Side bench of loo_nonfactor's log-likelihood kernels (csrc/pla_nonfactor.h).

    python tools/bench_nonfactor.py [--obs 100] [--draws 4000] [--model normal|student_t] [--dtype f64|f32] [--host]
                                    [--route 0..3] [--steps 5]

Spatial exponential-kernel covariances (SPD, nugget 0.05).  Prints one JSON line: the median wall time of the whole
``Engine.nonfactor_log_lik`` call (device synchronised), the kernels' event time (engine timing), GFLOP/s on a stated count of
2 N^3 / 3 per draw (Cholesky N^3/3 plus triangular inverse N^3/3), the matrix bytes S N^2 sizeof(dtype) and GB/s, and a
yardstick: a NumPy per-draw ``numpy.linalg.inv`` loop (the reference's method, plus its closed-form follow-up) timed on a few
draws on the host and extrapolated to S -- labelled as such.  bench.py is not involved.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(N, S, dtype, seed=0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 10, size=(N, 2))
    d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1))
    ls = rng.uniform(1.0, 3.0, size=S)
    cov = np.empty((S, N, N), dtype=dtype)
    for s0 in range(0, S, 256):
        cov[s0:s0 + 256] = np.exp(-d[None] / ls[s0:s0 + 256, None, None]) + 0.05 * np.eye(N)[None]
    mu = rng.normal(size=(S, N)).astype(dtype)
    y = rng.normal(size=N).astype(dtype)
    df = rng.uniform(3, 10, size=S).astype(dtype)
    return y, mu, cov, df


def numpy_loop_ms_per_draw(y, mu, cov, model, draws=8):
    """The per-draw inverse of loo_nonfactor.py:466-557 with beta in closed form, in NumPy on the host: ms per draw."""
    n = min(draws, mu.shape[0])
    t0 = time.perf_counter()
    for s in range(n):
        P = np.linalg.inv(cov[s].astype(np.float64))
        r = y - mu[s]
        g = P @ r
        c = np.diag(P)
        if model == "student_t":
            _ = r @ g - g**2 / c
        _ = 0.5 * np.log(c) - 0.5 * g**2 / c
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=100)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--model", default="normal", choices=["normal", "student_t"])
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--host", action="store_true", help="NumPy inputs (staged by the library) instead of device tensors")
    ap.add_argument("--route", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()

    import torch

    from pyloo_amd.engine import get_engine

    N, S = a.obs, a.draws
    dt = np.float64 if a.dtype == "f64" else np.float32
    y, mu, cov, df = inputs(N, S, dt)
    eng = get_engine(0)
    eng.set_nonfactor_route(a.route)
    args = (y, mu, cov, df) if a.host else tuple(torch.as_tensor(v).cuda() for v in (y, mu, cov, df))
    eng.nonfactor_log_lik(*args, model=a.model)  # warm-up: workspace, code objects
    torch.cuda.synchronize()
    eng.set_timing(True)
    eng.kernel_ms()
    ts = []
    for _ in range(a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ll, flags = eng.nonfactor_log_lik(*args, model=a.model)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    kms, launches = eng.kernel_ms()
    eng.set_timing(False)
    call_ms = float(np.median(ts))
    kernel_ms = kms / a.steps
    fl = flags.cpu().numpy() if hasattr(flags, "cpu") else flags
    flop = 2.0 * N**3 / 3.0 * S
    nbytes = float(S) * N * N * np.dtype(dt).itemsize
    np_ms = numpy_loop_ms_per_draw(y, mu, cov, a.model) * S
    print(json.dumps({
        "bench": "nonfactor_loglik", "obs": N, "draws": S, "model": a.model, "dtype": a.dtype, "host": a.host, "route": a.route,
        "kernels": eng.last_kernels(), "general_draws": int(np.sum(fl & 1)) if a.route != 3 else S,
        "call_ms": round(call_ms, 3), "kernel_event_ms": round(kernel_ms, 3),
        "gflops_2n3_over_3": round(flop / (call_ms * 1e6), 2), "bytes": nbytes, "gbps": round(nbytes / (call_ms * 1e6), 2),
        "numpy_inv_loop_ms_extrapolated": round(np_ms, 1), "speedup_vs_numpy_loop": round(np_ms / call_ms, 1),
    }))


if __name__ == "__main__":
    main()
