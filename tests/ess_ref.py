"""NumPy restatement of the relative-efficiency rule of include/pyloo_amd.h (``pla_relative_eff``), written from the rule with a
rho-hat array and the two sequences applied one after the other -- not from the kernel, which accumulates them online.

TEST INFRASTRUCTURE ONLY (like tests/lfo_ref.py): the product never imports it.

``ess_row`` returns ``(r_eff, margin, stop)``: ``margin`` is the DECIDING MARGIN of the row, the smallest ``|rho_e + rho_o|`` and
``|rho_e|`` on which a branch of Geyer's rule was taken -- a rounding-level change of the autocovariances can flip a branch only
when it is of that size -- and ``stop`` the stopping lag T.  Autocovariances by direct lag sums (lag by lag, as far as the rule
goes) or, ``fft=True``, all at once by FFT.
"""

import numpy as np


def chains_of(row, n_chains, log=True, split=False):
    """The (C, n) array analysed, or None for an invalid row (NaN / +inf entries, -inf without log, constant)."""
    x = np.asarray(row, dtype=np.float64).reshape(n_chains, -1)
    if split:
        n = x.shape[1] // 2
        x = np.stack([x[:, :n], x[:, x.shape[1] - n:]], axis=1).reshape(2 * n_chains, n)
    if np.isnan(x).any() or (x == np.inf).any() or (not log and (x == -np.inf).any()) or x.max() == x.min():
        return None
    if log:
        x = np.exp(x - x.max())
    return x


def acov_fft(d):
    """A(t), t = 0 .. n - 1, of the centred chains d (C, n): the divisor-n autocovariance, mean over chains."""
    n = d.shape[1]
    f = np.fft.rfft(d, 2 * n, axis=1)
    return (np.fft.irfft(f * np.conj(f), 2 * n, axis=1)[:, :n] / n).mean(axis=0)


class _Direct:
    def __init__(self, d):
        self.d, self.n = d, d.shape[1]

    def __getitem__(self, t):
        d, n = self.d, self.n
        return np.mean(np.sum(d[:, : n - t] * d[:, t:], axis=1) / n)


def ess_row(row, n_chains, log=True, split=False, cap=True, fft=False):
    x = chains_of(row, n_chains, log, split)
    if x is None:
        return np.nan, np.inf, 0
    C, n = x.shape
    m = x.mean(axis=1)
    d = x - m[:, None]
    A = acov_fft(d) if fft else _Direct(d)
    A0 = A[0]
    W = A0 * n / (n - 1)
    V = A0 + (np.var(m, ddof=1) if C > 1 else 0.0)
    if not (V > 0 and np.isfinite(V)):
        return np.nan, np.inf, 0

    def rho(t):
        return 1.0 - (W - A[t]) / V

    # initial positive sequence
    hat = np.zeros(n + 3)
    hat[0] = 1.0
    hat[1] = rho(1)
    re, ro, t = 1.0, hat[1], 2
    margin = np.inf
    while True:
        if t < n - 1:
            margin = min(margin, abs(re + ro))
        if not (t < n - 1 and not np.isnan(re + ro) and re + ro > 0):
            break
        re, ro = rho(t), rho(t + 1)
        margin = min(margin, abs(re + ro))
        if re + ro >= 0:
            hat[t], hat[t + 1] = re, ro
        t += 2
    T = t
    margin = min(margin, abs(re))
    if re > 0:
        hat[T] = re
    # initial monotone sequence
    for t in range(2, T - 1, 2):
        if hat[t] + hat[t + 1] > hat[t - 2] + hat[t - 1]:
            hat[t] = hat[t + 1] = (hat[t - 2] + hat[t - 1]) / 2
    tau = -1.0 + 2.0 * np.sum(hat[:T]) + hat[T]
    tau = max(tau, 1.0 / np.log10(C * n))
    r = 1.0 / tau
    return (min(r, 1.0) if cap else r), margin, T


def relative_eff(mat, n_chains, log=True, split=False, cap=True, fft=False):
    """(r_eff, margin, stop) arrays over the rows of mat."""
    out = [ess_row(r, n_chains, log, split, cap, fft) for r in np.asarray(mat)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


# ---- seeded row families ---------------------------------------------------------------------------------------------------------
FAMILIES = {"iid": 0.0, "ar0.5": 0.5, "ar0.9": 0.9, "ar0.99": 0.99, "anti": -0.5}


def ar1_rows(rng, n_rows, n_chains, n, phi, log=True):
    """(n_rows, n_chains * n) f64: stationary AR(1) chains with unit marginal variance, chain major.  log=True: a log-likelihood
    (the values scaled to sd 0.7 around -3, so the likelihood exp(.) is a smooth positive function of the chain); log=False: the
    values themselves, negative ones included."""
    e = rng.standard_normal((n_rows, n_chains, n))
    z = np.empty_like(e)
    z[..., 0] = e[..., 0]
    s = np.sqrt(1.0 - phi * phi)
    for i in range(1, n):
        z[..., i] = phi * z[..., i - 1] + s * e[..., i]
    z = z.reshape(n_rows, n_chains * n)
    return -3.0 + 0.7 * z if log else z


# chains x draws of the parity cases of tests/test_gpu_relative_eff.py: the smallest chains, odd lengths, the standard shape, the
# on-chip limit of the kernels (4096 analysed draws) and one beyond it, and a row of the long route
PARITY_SHAPES = ((1, 4), (3, 4), (2, 33), (4, 250), (4, 1000), (1, 4096), (1, 4097), (2, 10000))
MARGIN_FLOOR = 1e-8  # rows whose deciding margin is below it may flip a branch at rounding level


def parity_matrix(n_chains, n, log, dtype=np.float64):
    """The rows of one parity case: every family of FAMILIES in turn, three rows each (one for the long shapes)."""
    per = 3 if n_chains * n <= 4000 else 1
    rng = np.random.default_rng(77000 + 100 * n_chains + n + (5 if log else 0))
    return np.concatenate([ar1_rows(rng, per, n_chains, n, phi, log) for phi in FAMILIES.values()]).astype(dtype)


# ---- rows at the two ends of Geyer's loop (tests/test_gpu_relative_eff_edges.py) ------------------------------------------------------
def unmixed_rows(rng, n_rows, n_chains, n, log):
    """Chains that have not mixed: AR(1) at phi = 0.5 with chain c shifted by 10 c -- z + 10 c, or -3 + 0.07 (z + 10 c) for a log row.
    V >> W keeps rho-hat near 1, so Geyer's rule never stops: the loop walks every lag the rule allows (stop = n for even n, n - 1
    for odd n) with margins near 1.  Needs n_chains >= 2.  Chain major like ar1_rows."""
    assert n_chains >= 2
    z = ar1_rows(rng, n_rows, n_chains, n, 0.5, log=False).reshape(n_rows, n_chains, n)
    v = (z + 10.0 * np.arange(n_chains)[None, :, None]).reshape(n_rows, n_chains * n)
    return -3.0 + 0.07 * v if log else v


def alternating_rows(rng, n_rows, n_chains, n, log):
    """Chains that flip sign at every draw: (+1, -1, +1, ...) times 1 + 0.01 N(0, 1) per chain, plus 1e-3 N(0, 1) per draw; a log row
    is -3 + 0.7 times that.  rho-hat(1) <= -1, so the loop ends at once or after one pair and tau lands on its floor:
    r_eff = log10(C n) of the analysed shape.  Chain major like ar1_rows."""
    e = ar1_rows(rng, n_rows, n_chains, n, 0.0, log=False).reshape(n_rows, n_chains, n)
    amp = 1.0 + 0.01 * rng.standard_normal((n_rows, n_chains, 1))
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    v = (sign * amp + 1e-3 * e).reshape(n_rows, n_chains * n)
    return -3.0 + 0.7 * v if log else v


# chains x draws at the strides of csrc/pla_ess.h, by the structure each group steps over (tests/test_gpu_relative_eff_edges.py runs
# them with parity_matrix's rows, split as well wherever a half chain keeps four draws)
EDGE_SHAPES = {
    # lane l owns draws l, l + 64, ... of a chain (kWave)
    "wave": ((1, 63), (1, 64), (1, 65), (3, 63), (3, 64), (3, 65)),
    # the sweeps issue kEssBatch x 64 = 512 draws per step; the last three split into halves of 511 / 512 / 513
    "sweep": ((1, 511), (1, 512), (1, 513), (2, 511), (2, 513), (1, 1023), (1, 1025), (2, 1027)),
    # ess_load takes kEssLoadBatch x 64 = 1024 draws per step (split rows and the long route): split halves of 1025 and of 1024
    # (the middle draw skipped), and an unsplit row of the long route
    "load": ((1, 2050), (2, 2049), (3, 1366)),
    # the 64 register slots of ess_fetch / ess_commit with several chains: 4096 analysed draws, 4095, and just above the limit
    "limit": ((8, 512), (64, 64), (1024, 4), (3, 1365), (7, 585), (3, 1366), (17, 241), (1025, 4)),
    # the route follows the analysed draws: long unsplit and on chip split; long both ways; long with split chains of 4096
    "route": ((2, 2049), (1, 4098), (1, 8192)),
    # the Geyer loop's bound t < n - 1 at tiny n; the last five split into halves of four or five draws
    "tiny": ((1, 5), (1, 6), (1, 7), (2, 5), (1, 8), (1, 9), (2, 8), (3, 9), (1, 11)),
}
UNMIXED_SHAPES = ((2, 4), (2, 5), (2, 6), (2, 7), (3, 64), (3, 65), (2, 513), (8, 512), (3, 1366), (2, 1027))
ALTERNATING_SHAPES = ((1, 4), (1, 5), (1, 10), (1, 64), (1, 65), (4, 250), (1, 513), (1, 4096), (1, 4097), (3, 1366))


def loop_end_matrix(family, n_chains, n, log, dtype=np.float64):
    """Three rows of unmixed_rows or alternating_rows for one shape, seeded like parity_matrix."""
    make = {"unmixed": unmixed_rows, "alternating": alternating_rows}[family]
    rng = np.random.default_rng({"unmixed": 78000, "alternating": 79000}[family] + 100 * n_chains + n + (5 if log else 0))
    return make(rng, 3, n_chains, n, log).astype(dtype)


class OracleEssEngine:
    """Stand-in for ``Engine.relative_eff`` on this restatement; records what the front passed."""

    def __init__(self):
        self.calls = []

    def relative_eff(self, x, n_chains=1, log=True, split=False, cap=True):
        x = np.asarray(x)
        self.calls.append({"x": x.copy(), "n_chains": n_chains, "log": log, "split": split, "cap": cap})
        r = relative_eff(x, n_chains, log, split, cap)[0]
        return {"r_eff": r, "n_invalid": int(np.isnan(r).sum())}
