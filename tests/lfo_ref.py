"""NumPy restatement of PSIS leave-future-out CV on the CPU oracle (TEST INFRASTRUCTURE ONLY).

Forward mode, M steps ahead, for the log-likelihood ``ll`` (N, S) of one fit to the first ``first`` observations:

    lr_j[s] = sum_{r = first}^{first + j - 1} ll[r, s]        f_j[s] = ll[first + j, s] + ... + ll[first + j + M - 1, s]
    j = 0:  elpd_0 = lse(f_0) - log S, k_0 = 0                j > 0:  (lw, k_j) = psis_row(lr_j, tail_count);  elpd_j = lse(lw + f_j) - lse(lw)

``ratios`` restates the summation rule include/pyloo_amd.h documents (chunks of ``CHUNK`` rows: ``lr_j = carry[j // CHUNK] +
local[j]``, every sum sequential), so that the library's log ratios can be compared bit for bit.  NaN entries count as -1e10."""

import numpy as np

from oracle import psis_oracle as orc

CHUNK = 64


def clean(ll):
    """float64 copy with NaN -> -1e10, and the NaN mask."""
    a = np.asarray(ll).astype(np.float64)
    nan = np.isnan(a)
    return np.where(nan, -1e10, a), nan


def ratios(ll, first, n_steps):
    """(n_steps, S) float64 log ratios in the documented order."""
    a, _ = clean(ll)
    S = a.shape[1]
    out = np.zeros((n_steps, S))
    carry = np.zeros(S)
    with np.errstate(all="ignore"):
        for c0 in range(0, n_steps, CHUNK):
            local = np.zeros(S)
            for j in range(c0, min(c0 + CHUNK, n_steps)):
                out[j] = carry + local
                if j + 1 < n_steps:  # (the last step's own row enters no sum)
                    local = local + a[first + j]
            carry = carry + local  # (of a whole chunk: its total)
    return out


def future(a, t, M):
    f = np.zeros(a.shape[1])
    with np.errstate(all="ignore"):
        for m in range(M):
            f = f + a[t + m]
    return f


def first_high(k, threshold):
    above = np.flatnonzero(np.asarray(k)[1:] > threshold)
    return int(above[0]) + 1 if above.size else len(k)


def lfo_pass(ll, first, n_steps, M, reff=1.0, k_threshold=0.7, tail_count=None):
    """dict(diag, elpd_i, first_high, n_replaced, ratios) of one pass over the steps first .. first + n_steps - 1."""
    a, nan = clean(ll)
    S = a.shape[1]
    tail = orc.tail_count(S, reff) if tail_count is None else tail_count
    lr = ratios(ll, first, n_steps)
    k, elpd = np.zeros(n_steps), np.zeros(n_steps)
    with np.errstate(all="ignore"):
        for j in range(n_steps):
            f = future(a, first + j, M)
            if j == 0:
                elpd[j] = orc.lse(f) - np.log(S)
                continue
            lw, k[j] = orc.psis_row(lr[j], tail)
            elpd[j] = orc.lse(lw + f) - orc.lse(lw)
    return {"diag": k, "elpd_i": elpd, "first_high": first_high(k, k_threshold), "n_replaced": int(nan[first:first + n_steps + M - 1].sum()),
            "ratios": lr}


def lfo_walk(ll0, L, M, refit=None, k_threshold=0.7, reff=1.0):
    """The host loop: dict(elpd, k (both for t = L .. N-M), refits, n_replaced).  ``refit(t)`` -> matrix or (matrix, reff)."""
    mat = np.asarray(ll0)
    N = mat.shape[0]
    n_total = N - M - L + 1
    elpd, k = np.empty(n_total), np.empty(n_total)
    refits, n_replaced, t, trigger = [], 0, L, None
    while True:
        n_steps = N - M - t + 1
        res = lfo_pass(mat, t, n_steps, M, reff, k_threshold)
        take = n_steps if refit is None else res["first_high"]
        elpd[t - L:t - L + take] = res["elpd_i"][:take]
        k[t - L:t - L + take] = res["diag"][:take]
        if trigger is not None:
            k[t - L] = trigger
        n_replaced += res["n_replaced"]
        if take == n_steps:
            break
        trigger = res["diag"][take]
        t += take
        out = refit(t)
        if isinstance(out, tuple):
            out, reff = out
        mat = np.asarray(out)
        refits.append(t)
    return {"elpd": elpd, "k": k, "refits": refits, "n_replaced": n_replaced}


class OracleLfoEngine:
    """Stand-in for ``Engine.lfo`` / ``Engine.lfo_ratios`` on the restatement (the product has no CPU path)."""

    device = "cpu-oracle"

    def __init__(self):
        self.calls = []

    def lfo_ratios(self, ll, first, n_steps):
        return {"ratios": ratios(ll, first, n_steps), "n_replaced": int(np.isnan(np.asarray(ll)[first:first + n_steps - 1]).sum())}

    def lfo(self, ll, first, n_steps, horizon=1, tail_count=0, k_threshold=0.7, method="psis"):
        ll = np.asarray(ll)
        self.calls.append({"first": first, "n_steps": n_steps, "horizon": horizon, "tail_count": tail_count, "shape": ll.shape,
                           "k_threshold": k_threshold})
        r = lfo_pass(ll, first, n_steps, horizon, k_threshold=k_threshold, tail_count=tail_count)
        return {key: r[key] for key in ("diag", "elpd_i", "first_high", "n_replaced")}


def draw_ll(rng, n, s, dtype=np.float64, k_lo=0.05, k_hi=0.6):
    """Seeded rows ll = -k_r Exp(1) + c_r, as the other suites draw them."""
    kr = rng.uniform(k_lo, k_hi, size=(n, 1))
    cr = -1.0 - (np.arange(n) % 7)[:, None] / 4.0
    return (-kr * rng.exponential(size=(n, s)) + cr).astype(dtype)
