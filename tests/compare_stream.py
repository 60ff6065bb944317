"""NumPy restatement of the model-comparison kernels (csrc/pla_compare.h), for the tests.

``philox4x32_10`` and ``gamma_draws`` restate the bootstrap's gamma stream operation by operation; ``bb_z`` its replicates
(all of them, or the ones named by ``replicates=``).  ``moments_reference`` and ``stacking_reference`` are the moments and the
stacking pass in wider arithmetic (``math.fsum`` and ``np.longdouble``), to judge the kernels' f64 results against.
``NumpyCompareEngine`` answers the Engine methods that ``pyloo_amd.compare`` calls, so the CPU suite can run the front without
a GPU.  TEST INFRASTRUCTURE ONLY."""

import math

import numpy as np

M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 of counters ``ctr`` (4 arrays of uint32 values) under ``key`` (2 values): 4 arrays of uint32 words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def u53(hi, lo):
    v = (np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)
    return ((v >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0**-53


def _replicate_numbers(B, replicates):
    if replicates is None:
        return np.arange(B, dtype=np.uint64)
    reps = np.asarray(replicates, dtype=np.int64).reshape(-1)
    if reps.size and (reps.min() < 0 or reps.max() >= B):
        raise ValueError(f"replicates must lie in [0, {B})")
    return reps.astype(np.uint64)


def gamma_draws(seed, alpha, B, N, replicates=None):
    """G[b, i] of the stream specified in csrc/pla_compare.h, for b < B; with ``replicates`` (an array of replicate numbers
    below B) only those rows, in the order given: the stream is a function of (seed, alpha, b, i), so they are the bits of the
    same rows of the full call."""
    b, i = np.meshgrid(_replicate_numbers(B, replicates), np.arange(N, dtype=np.uint64), indexing="ij")
    key = (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    zero, one = np.zeros_like(b), np.ones_like(b)
    if alpha == 1.0:
        r = philox4x32_10((i, b, zero, zero), key)
        return -np.log(u53(r[0], r[1]))
    a = alpha + 1.0 if alpha < 1.0 else alpha
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    g = np.full(b.shape, d)
    done = np.zeros(b.shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(64):
            tt = np.full_like(b, t)
            r = philox4x32_10((i, b, tt, zero), key)
            x = np.sqrt(-2.0 * np.log(u53(r[0], r[1]))) * np.cos(6.283185307179586 * u53(r[2], r[3]))
            v = 1.0 + c * x
            v3 = v * v * v
            s = philox4x32_10((i, b, tt, one), key)
            acc = (~done) & (v > 0.0) & (np.log(u53(s[0], s[1])) < 0.5 * x * x + d - d * v3 + d * np.log(v3))
            g = np.where(acc, d * v3, g)
            done |= acc
            if done.all():
                break
    if alpha < 1.0:
        s = philox4x32_10((i, b, zero, one), key)
        g = g * u53(s[2], s[3]) ** (1.0 / alpha)
    return g


def bb_z(x, B, alpha, seed, scale_mul=1.0, replicates=None):
    """z[b, k] = N * scale_mul * (sum_i G_bi x_ki / sum_i G_bi), for b < B or for the rows ``replicates`` alone."""
    x = np.asarray(x, dtype=np.float64)
    return bb_z_from_gammas(gamma_draws(seed, alpha, B, x.shape[1], replicates), x, scale_mul)


def bb_z_from_gammas(G, x, scale_mul=1.0):
    """``bb_z`` for gamma draws ``G`` (rows of ``gamma_draws``) that the caller holds: they depend on (seed, alpha, b, i) alone,
    so tests of several matrices of one width generate them once."""
    x = np.asarray(x, dtype=np.float64)
    return (x.shape[1] * scale_mul) * ((G @ x.T) / G.sum(axis=1, keepdims=True))


def stacking_objective(x, w, scale_mul=1.0):
    """-sum_i log(exp(x' - max) @ w): the reference's objective (compare.py:494-503) at full weights w."""
    xs = scale_mul * np.asarray(x, dtype=np.float64).T
    e = np.exp(xs - xs.max(axis=1, keepdims=True))
    return -np.sum(np.log(e @ np.asarray(w)))


def moments_reference(x, best):
    """``out[3K + 1]`` of ``compare_moments`` in wider arithmetic, as ``np.longdouble``: the row sums and the sum of the column
    maxima by ``math.fsum`` (exactly rounded), the mean and the two-pass M2 of ``d = x[k] - x[best]`` in ``np.longdouble``.
    f32 input is widened first (exactly): the kernels promote on load, so this is the arithmetic on the f32 values."""
    x = np.asarray(x).astype(np.float64)
    K, N = x.shape
    xl = x.astype(np.longdouble)
    out = np.zeros(3 * K + 1, dtype=np.longdouble)
    for k in range(K):
        d = xl[k] - xl[best]
        mean = d.sum() / np.longdouble(N)
        out[3 * k], out[3 * k + 1], out[3 * k + 2] = math.fsum(x[k]), mean, np.sum((d - mean) ** 2)
    out[3 * K] = math.fsum(x.max(axis=0))
    return out


def stacking_reference(x, w, scale_mul=1.0):
    """``(F, G)`` of ``stacking_eval`` in ``np.longdouble``: F = sum_i log d_i, G[k] = sum_i e_ik / d_i with
    e_ik = exp(s x_ik - max_k s x_ik), d_i = sum_k w_k e_ik.  f32 input is widened first (exactly)."""
    xs = np.longdouble(scale_mul) * np.asarray(x).astype(np.float64).astype(np.longdouble).T
    e = np.exp(xs - xs.max(axis=1, keepdims=True))
    d = e @ np.asarray(w, dtype=np.float64).astype(np.longdouble)
    return np.sum(np.log(d)), (e / d[:, None]).sum(axis=0)


class NumpyCompareEngine:
    device = "cpu-numpy"

    def compare_moments(self, x, best):
        x = np.asarray(x, dtype=np.float64)
        K = x.shape[0]
        out = np.empty(3 * K + 1)
        for k in range(K):
            d = x[k] - x[best]
            out[3 * k], out[3 * k + 1], out[3 * k + 2] = x[k].sum(), d.mean(), np.sum((d - d.mean()) ** 2)
        out[3 * K] = x.max(axis=0).sum()
        return out

    def stacking_eval(self, x, weights, scale_mul=1.0):
        xs = scale_mul * np.asarray(x, dtype=np.float64).T
        e = np.exp(xs - xs.max(axis=1, keepdims=True))
        d = e @ np.asarray(weights)
        return float(np.sum(np.log(d))), (e / d[:, None]).sum(axis=0)

    def bb_bootstrap(self, x, n_boot, alpha=1.0, seed=0, scale_mul=1.0):
        return bb_z(x, n_boot, alpha, seed, scale_mul)
