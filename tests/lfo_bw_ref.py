"""NumPy restatement of BACKWARD PSIS leave-future-out CV on the CPU oracle (TEST INFRASTRUCTURE ONLY), built on tests/lfo_ref.py.

A pass serves one fit that saw the first ``last`` rows of ``ll`` (N, S); rows r >= last are the conditional terms the caller supplies:

    t_0 = min(last, N - M),  t_j = t_0 - j          f_j[s] = ll[t_j, s] + ... + ll[t_j + M - 1, s]
    lr_j[s] = - sum_{r = t_j}^{last - 1} ll[r, s]   = -P[last - t_j], P = lfo_ref.ratios of the rows last-1, last-2, ... (the rule is
                                                      anchored at the fit: chunks of lfo_ref.CHUNK rows counted from row last - 1 down)
    t_j = last:  elpd_j = lse(f_j) - log S, k_j = 0         t_j < last:  (lw, k_j) = psis_row(lr_j, tail);  elpd_j = lse(lw + f_j) - lse(lw)
    first_high = the smallest j >= j_min with k_j > threshold, else n_steps;  j_min = 1 when step 0 is exact, else 0

NaN entries count as -1e10 and are counted once each over rows [t_{n_steps - 1}, t_0 + M)."""

import numpy as np

import lfo_ref
from oracle import psis_oracle as orc


def ratios(ll, last, n_q):
    """(n_q, S): row q is lr of the step t = last - q, i.e. -P[q]; P[q] needs the rows last - 1 .. last - q."""
    rev = np.asarray(ll)[:last][::-1]  # a_q = ll[last - 1 - q]
    return -lfo_ref.ratios(rev, 0, n_q)


def first_high(k, threshold, j_min):
    above = np.flatnonzero(np.asarray(k)[j_min:] > threshold)
    return int(above[0]) + j_min if above.size else len(k)


def lfo_pass(ll, last, n_steps, M, reff=1.0, k_threshold=0.7, tail_count=None):
    """dict(diag, elpd_i, first_high, n_replaced, ratios, t) of one backward pass; ratios[j] = lr_j, t[j] = t_j."""
    a, nan = lfo_ref.clean(ll)
    N, S = a.shape
    assert 0 < last <= N and M <= N
    t0 = min(last, N - M)
    assert 1 <= n_steps <= t0 + 1
    q0 = last - t0
    tail = orc.tail_count(S, reff) if tail_count is None else tail_count
    lr = ratios(ll, last, q0 + n_steps)[q0:]
    k, elpd = np.zeros(n_steps), np.zeros(n_steps)
    with np.errstate(all="ignore"):
        for j in range(n_steps):
            t = t0 - j
            f = lfo_ref.future(a, t, M)
            if t == last:
                elpd[j] = orc.lse(f) - np.log(S)
                continue
            lw, k[j] = orc.psis_row(lr[j], tail)
            elpd[j] = orc.lse(lw + f) - orc.lse(lw)
    return {"diag": k, "elpd_i": elpd, "first_high": first_high(k, k_threshold, 1 if q0 == 0 else 0),
            "n_replaced": int(nan[t0 - n_steps + 1:t0 + M].sum()), "ratios": lr, "t": t0 - np.arange(n_steps)}


def lfo_walk(ll_full, L, M, refit=None, k_threshold=0.7, reff=1.0):
    """The host loop, downward from t = N - M to L: dict(elpd, k (both indexed t - L), refits (call order), n_replaced).
    ``refit(t)`` -> matrix or (matrix, reff)."""
    mat = np.asarray(ll_full)
    N = mat.shape[0]
    n_total = N - M - L + 1
    elpd, k = np.empty(n_total), np.empty(n_total)
    refits, n_replaced, trigger = [], 0, None
    last, t0 = N, N - M
    while True:
        n_steps = t0 - L + 1
        res = lfo_pass(mat, last, n_steps, M, reff, k_threshold)
        take = n_steps if refit is None else res["first_high"]
        for j in range(take):
            elpd[t0 - j - L] = res["elpd_i"][j]
            k[t0 - j - L] = res["diag"][j]
        if trigger is not None:
            k[t0 - L] = trigger
        n_replaced += res["n_replaced"]
        if take == n_steps:
            break
        trigger = res["diag"][take]
        t0 -= take
        k[t0 - L] = trigger
        out = refit(t0)
        if isinstance(out, tuple):
            out, reff = out
        mat = np.asarray(out)
        refits.append(t0)
        last = t0
    return {"elpd": elpd, "k": k, "refits": refits, "n_replaced": n_replaced}


class OracleLfoEngine(lfo_ref.OracleLfoEngine):
    """The stand-in engine of tests/lfo_ref.py with the ``mode`` keyword of ``Engine.lfo``."""

    def lfo(self, ll, first, n_steps, horizon=1, tail_count=0, k_threshold=0.7, method="psis", mode="forward"):
        if mode == "forward":
            return super().lfo(ll, first, n_steps, horizon, tail_count, k_threshold, method)
        if mode != "backward":
            raise ValueError(mode)
        ll = np.asarray(ll)
        self.calls.append({"first": first, "n_steps": n_steps, "horizon": horizon, "tail_count": tail_count, "shape": ll.shape,
                           "k_threshold": k_threshold, "mode": mode})
        r = lfo_pass(ll, first, n_steps, horizon, k_threshold=k_threshold, tail_count=tail_count)
        return {key: r[key] for key in ("diag", "elpd_i", "first_high", "n_replaced")}
