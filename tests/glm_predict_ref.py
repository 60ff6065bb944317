"""NumPy restatement of the GLM predictive kernel (csrc/pla_glm_predict.h): the per-(observation, draw) mean, second moment and
distribution function values in the header's rounding order, the weighted sums in long double, and scipy's distribution functions
as the independent check.  TEST INFRASTRUCTURE ONLY."""

import numpy as np
from scipy import special as sp

import glm_families_ref as fam_ref
import glm_ref

SEG = 16          # tiles of 16 draws per segment (pla_glm_predict_segment)
MAX_COUNT = 4096  # the largest count whose distribution function is walked
ENGINE_FAMILIES = ("gaussian", "binomial", "poisson", "negbinomial", "gamma", "binomial_probit")
DISCRETE = ("binomial", "poisson", "negbinomial", "binomial_probit")


def ndtr_tail(t):
    """Phi(-|t|) = (h exp(-w)) (1 - 0.5 r): the arithmetic of ``glm_log_ndtr_pair`` (the remainder of t^2 from Veltkamp's split)."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        h = 0.5 * sp.erfcx(np.abs(t) * 0.70710678118654752440)
        sq = t * t
        c = 134217729.0 * t
        hi = c - (c - t)
        lo = t - hi
        r = np.where(sq < np.inf, ((hi * hi - sq) + 2.0 * (hi * lo)) + lo * lo, 0.0)
        r = np.where(np.isfinite(r), r, 0.0)
        w = 0.5 * sq
        return (h * np.exp(-w)) * (1.0 - 0.5 * r)


def _density(family, eta, y, scale, trials, oc, dc):
    if family in ("gaussian", "binomial", "poisson"):
        return glm_ref.density(family, eta, y, sigma=scale, trials=trials, oc=oc, dc=dc)
    return fam_ref.density(family, eta, y, scale=scale, trials=trials, oc=oc, dc=dc)


def constants(family, y, trials=None, scale=None):
    """(obs_const, draw_const) as the fronts hand them to the kernel."""
    if family == "gaussian":
        return None, glm_ref.draw_const(scale)
    if family in ("binomial", "poisson"):
        return (glm_ref.obs_const(family, y, trials) if family == "poisson" or trials is not None else None), None
    oc = fam_ref.obs_const(family, y, trials)
    return oc, (None if family == "binomial_probit" else fam_ref.draw_const(scale))


def ratio(family, k, a, c):
    """r_k = pmf(k - 1) / pmf(k) in the kernel's order; ``a``: trials or phi, ``c``: the draw's constant factor."""
    if family == "poisson":
        return k * c
    if family == "negbinomial":
        return (k / ((k - 1.0) + a)) * c
    return (k / ((a - k) + 1.0)) * c


def point(family, eta, y, scale=None, trials=None):
    """``(mu, second, f_le, f_lt)``, each (n, S), from ``eta`` (n, S), ``y`` [n], ``scale`` [S] (sigma / phi / alpha) and ``trials``
    [n] (None: 1) -- the header's formulas in the header's order.  The PIT values of the gamma family are zeros; a count outside
    [0, MAX_COUNT] is not walked (its values are whatever T = 0 gives: the kernel's combine step overwrites them with NaN)."""
    eta = np.asarray(eta, dtype=np.float64)
    n, S = eta.shape
    yc = np.asarray(y, dtype=np.float64)[:, None] + np.zeros((1, S))
    sc = None if scale is None else np.asarray(scale, dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        if family == "gaussian":
            v = sc * sc
            t = (yc - eta) / sc
            lo = ndtr_tail(t)
            F = np.where(t < 0.0, lo, 1.0 - lo)
            return eta + 0.0 * v, v + eta * eta, F, F.copy()
        if family == "gamma":
            m = np.exp(eta)
            return m, (m * m) / sc + m * m, np.zeros_like(m), np.zeros_like(m)
        nt = np.ones((n, 1)) if trials is None else np.asarray(trials, dtype=np.float64)[:, None]
        if family == "poisson":
            m = np.exp(eta)
            v, c, a = m, np.exp(-eta), np.zeros_like(eta)
        elif family == "negbinomial":
            m = np.exp(eta)
            v, c, a = m + (m * m) / sc, (m + sc) / m, sc + np.zeros_like(eta)
        elif family == "binomial":
            x = np.exp(-np.abs(eta))
            d = 1.0 + x
            big, small = 1.0 / d, x / d
            pos = eta >= 0.0
            m = nt * np.where(pos, big, small)
            v, c, a = m * np.where(pos, small, big), np.exp(-eta), nt + np.zeros_like(eta)
        elif family == "binomial_probit":
            lo = ndtr_tail(eta)
            hi = 1.0 - lo
            neg = eta < 0.0
            p, q = np.where(neg, lo, hi), np.where(neg, hi, lo)
            m = nt * p
            v, c, a = m * q, q / p, nt + np.zeros_like(eta)
        else:
            raise ValueError(family)
        oc, dc = constants(family, y, None if trials is None else trials, scale)
        pmf = np.exp(_density(family, eta, y, scale, trials, oc, dc))
        walk = (yc >= 0.0) & (yc <= MAX_COUNT)
        t, T = np.ones_like(eta), np.zeros_like(eta)
        ry = np.where(walk & (yc >= 1.0), ratio(family, yc, a, c), 0.0)
        k = yc.copy()
        for _ in range(int(np.max(np.where(walk, yc, 0.0), initial=0.0))):
            on = walk & (k >= 1.0)
            t = np.where(on, t * ratio(family, k, a, c), t)
            T = np.where(on, T + t, T)
            k = k - 1.0
        lt = pmf * T
        le = lt + pmf
        le = np.where(le > 1.0, 1.0, le)
        lt = np.where(lt > 1.0, 1.0, lt)
        one = (T == np.inf) | ((pmf == 0.0) & (ry > 1.0))
        le, lt = np.where(one, 1.0, le), np.where(one, 1.0, lt)
        if family in ("binomial", "binomial_probit"):
            le = np.where(yc >= nt, 1.0, le)  # the end of the support
        return m, v + m * m, le, lt


def scipy_cdf(family, eta, y, scale=None, trials=None):
    """``(P(Y <= y), P(Y < y))`` from scipy's own distribution functions: the independent check."""
    eta = np.asarray(eta, dtype=np.float64)
    yc = np.asarray(y, dtype=np.float64)[:, None] + np.zeros((1, eta.shape[1]))
    sc = None if scale is None else np.asarray(scale, dtype=np.float64)[None, :]
    nt = np.ones((eta.shape[0], 1)) if trials is None else np.asarray(trials, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        if family == "gaussian":
            F = sp.ndtr((yc - eta) / sc)
            return F, F
        if family == "poisson":
            f = lambda k: sp.pdtr(k, np.exp(eta))  # noqa: E731
        elif family == "negbinomial":  # nbdtr(k, phi, p) = I_p(phi, k + 1), p = phi / (phi + mu); nbdtr itself truncates phi to an integer
            f = lambda k: sp.betainc(sc + 0.0 * eta, k + 1.0, sc / (sc + np.exp(eta)))  # noqa: E731
        elif family == "binomial":
            f = lambda k: sp.bdtr(k, (nt + 0.0 * eta).astype(np.int64), sp.expit(eta))  # noqa: E731
        elif family == "binomial_probit":
            f = lambda k: sp.bdtr(k, (nt + 0.0 * eta).astype(np.int64), sp.ndtr(eta))  # noqa: E731
        else:
            raise ValueError(family)
        return f(yc), np.where(yc >= 1.0, f(np.maximum(yc - 1.0, 0.0)), 0.0)


def weighted(lw, terms):
    """``sum_s e_s term_s / sum_s e_s`` per row in long double, ``e = exp(lw - max lw)``, a weight of log -inf contributing nothing;
    ``terms``: a sequence of (n, S) arrays.  A row whose weights are all -inf gives NaN."""
    lw = np.asarray(lw, dtype=np.longdouble)
    with np.errstate(all="ignore"):
        m = np.max(lw, axis=1, keepdims=True)
        e = np.where(np.isneginf(lw), 0.0, np.exp(lw - m))
        se = e.sum(axis=1)
        return [(np.where(e == 0.0, 0.0, e * np.asarray(t, dtype=np.longdouble)).sum(axis=1) / se).astype(np.float64) for t in terms]


def weighted_bound(lw, term):
    """The bound on a weighted sum of ``term`` (n, S) whose entries are good to ``1e-10 max(1, |term|)`` each (device lgamma / erfcx
    against scipy's): ``W(1e-10 max(1, |term|)) + (S + 4) 2^-53 W(|term|)`` with ``W`` the weighted mean of ``weighted`` in long
    double -- a convex combination of the per-element bound, plus the standard bound of a sum of S products and one division."""
    t = np.abs(np.asarray(term, dtype=np.float64))
    per_element, magnitude = weighted(lw, [1e-10 * np.maximum(1.0, t), t])
    return per_element + (t.shape[1] + 4) * 2.0 ** -53 * magnitude


def one_hot(n, S, s0):
    lw = np.full((n, S), -np.inf)
    lw[:, s0] = 0.0
    return lw
