#!/usr/bin/env python3
"""Secondary benchmark: approximate-posterior LOO (pl.loo_approximate_posterior_from_matrix) on a device-resident matrix.

    python tools/bench_approx_posterior.py [--obs N] [--draws S] [--layout draws|obs] [--dtype f64|f32] [--resample psis|psir]
                                           [--spread X] [--host] [--steps K] [--warmup W]

One step = pla_psis_loo_draws (blocks of observations gathered through the draw index into the staging buffer, the PSIS pass over
each) + the host packing of the result.  The index comes from pl.importance_resample on synthetic log_p / log_q ("psis": a weighted
permutation; "psir": with replacement).  Reported next to it: the gather kernel's own event time (pla_gather_draws block by block
into one reused block buffer, timed by the engine), algorithmic bytes N*S*e + 2*N*S'*e (the matrix once, the gathered block written
and read back) and their fraction of 8 TB/s, and two yardsticks: pl.loo_from_matrix(ll) (the pass alone) and
pl.loo_from_matrix(ll.index_select(1, idx).contiguous()) (the gather as a second full-size matrix through torch), each with
torch.cuda.max_memory_allocated above the resident matrix; for the step also the device memory in use outside torch's allocator
(the engine's workspace, which torch does not see).  --host: the matrix as a host ndarray.  One JSON line."""
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
    ap.add_argument("--layout", choices=["draws", "obs"], default="draws")
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--resample", choices=["psis", "psir"], default="psir")
    ap.add_argument("--spread", type=float, default=0.3, help="scale of log_p - log_q (Student-t, 5 df): the larger, the fewer distinct draws a psir index keeps")
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
    N, S = args.obs, args.draws
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    esz = 8 if args.dtype == "f64" else 4
    if args.layout == "draws":
        ll = torch.empty((N, S), dtype=dt, device="cuda")
        eng.fill_synthetic(ll, seed=0x5EED0005, k_lo=0.01, k_hi=0.05)
    else:
        ll = torch.empty((S, N), dtype=dt, device="cuda")  # (sample, obs) buffer viewed as (obs, sample): observations fastest
        eng.fill_synthetic(ll, seed=0x5EED0005, k_lo=0.01, k_hi=0.05)
        ll = ll.T
    rng = np.random.default_rng(1)
    log_q = rng.normal(size=S) - 3.0
    log_p = log_q + args.spread * rng.standard_t(df=5, size=S)
    warnings.simplefilter("ignore")
    index = np.asarray(pl.importance_resample(log_p, log_q, method=args.resample, seed=7), dtype=np.int64)
    n_out = len(index)
    idx = torch.as_tensor(index).cuda()
    src, src_idx = (ll.cpu().numpy(), index) if args.host else (ll, idx)
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()

    def timed(fn):
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) / args.steps, torch.cuda.max_memory_allocated() - resident

    out, dt_call, peak_call = timed(lambda: pl.loo_approximate_posterior_from_matrix(src, src_idx))
    kernels = eng.last_kernels()
    free, total = torch.cuda.mem_get_info()
    outside_torch = (total - free) - torch.cuda.memory_reserved()
    # the gather kernel alone (device matrices: pla_gather_draws block by block with the engine's event timing)
    gather_ms = None
    if not args.host:
        rows = max(1, min(N, (4 << 30) // (n_out * esz)))
        buf = torch.empty((rows, n_out), dtype=dt, device="cuda")
        blocks = [(r0, min(rows, N - r0)) for r0 in range(0, N, rows)]
        for r0, nr in blocks:
            eng.gather_draws(ll[r0:r0 + nr], idx, out=buf[:nr])
        torch.cuda.synchronize()
        eng.set_timing(True)
        for _ in range(args.steps):
            for r0, nr in blocks:
                eng.gather_draws(ll[r0:r0 + nr], idx, out=buf[:nr])
        ms, _ = eng.kernel_ms()
        eng.set_timing(False)
        gather_ms = ms / args.steps
        gather_kernel = eng.last_kernels()
        del buf
    plain, dt_loo, peak_loo = timed(lambda: pl.loo_from_matrix(ll))
    today, dt_today, peak_today = timed(lambda: pl.loo_from_matrix(ll.index_select(1, idx).contiguous()))
    alg = (float(N) * S + 2.0 * N * n_out) * esz
    print(json.dumps({
        "metric": "loo_approximate_posterior_ms_per_call", "value": dt_call * 1e3, "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
        "config": {"workload": f"loo_approximate_posterior_from_matrix, synthetic {args.dtype} S={S} x N={N}, {args.resample} index of "
                               f"{n_out} draws ({len(np.unique(index))} distinct, log_p - log_q spread {args.spread}), {args.layout} contiguous, "
                               f"{'host ndarray' if args.host else 'device-resident'}"},
        "algorithmic_bytes": alg, "algorithmic_tb_per_s": alg / dt_call / 1e12, "fraction_of_8tbps": alg / dt_call / 8e12,
        "gather_kernel_ms": gather_ms,
        "gather_fraction_of_8tbps": None if gather_ms is None else (float(N) * S + float(N) * n_out) * esz / (gather_ms * 1e-3) / 8e12,
        "gather_kernel": None if gather_ms is None else gather_kernel,
        "loo_from_matrix_ms": dt_loo * 1e3,
        "index_select_contiguous_then_loo_from_matrix_ms": dt_today * 1e3,
        "step_over_index_select_way": dt_call / dt_today,
        "peak_torch_bytes_above_matrix": {"step": peak_call, "loo_from_matrix": peak_loo, "index_select_way": peak_today},
        "device_bytes_outside_torch_after_step": outside_torch,
        "elpd_loo": float(out["elpd_loo"]), "elpd_loo_index_select_way": float(today["elpd_loo"]), "elpd_loo_plain": float(plain["elpd_loo"]),
        "kernels": kernels, "env": env_overrides(),
    }))


if __name__ == "__main__":
    main()
