"""NumPy restatement of the negative-binomial, gamma and probit densities of the GLM log-likelihood generator (include/pyloo_amd.h,
``pla_glm``, family codes 4, 5, 6) in the kernel's order of operations, the constants the fronts hand over, an mpmath reference that
takes those constants and ``eta`` as exact inputs, the error measure of DESIGN.md section 19 and generators of test models.
TEST INFRASTRUCTURE ONLY."""

import functools

import numpy as np
from scipy.special import erfcx, gammaln

import glm_ref

U = 2.0 ** -53
ENGINE_FAMILIES = ("negbinomial", "gamma", "binomial_probit")
# the front's (family, link) of an engine family, and the keyword its per-draw scale travels under
FRONT = {"negbinomial": ("negbinomial", None, "phi"), "gamma": ("gamma", None, "shape"), "binomial_probit": ("binomial", "probit", None)}

# The worst value of `measure` of this restatement against the mpmath reference on `accuracy_grid`, rounded up: 1.93, 8.98 and 10.13
# with scipy's gammaln / erfcx and NumPy's exp / log1p (test_glm_families_host.py measures them again and holds them within twice
# the record).  The gamma figure is the cancellation inside eta + y exp(-eta), which the measure counts as one term; the probit
# figure is scipy's erfcx, good to 1e-15, not to the ulp.  The device functions differ from these by a few units in the last place each: the GPU tests allow GPU_FACTOR times
# these figures, DESIGN.md section 19.
RESTATEMENT_FIGURE = {"negbinomial": 2.0, "gamma": 9.0, "binomial_probit": 10.2}
GPU_FACTOR = 4.0


def obs_const(family, y, trials=None):
    y = np.asarray(y, dtype=np.float64)
    if family == "negbinomial":
        return -gammaln(y + 1.0)
    if family == "gamma":
        return np.log(y)
    if family == "binomial_probit":
        return None if trials is None else glm_ref.obs_const("binomial", y, trials)
    raise ValueError(family)


def draw_const(scale):
    """``a log(a) - lgamma(a)`` of the negative binomial's ``phi`` / the gamma family's ``shape``."""
    a = np.asarray(scale, dtype=np.float64)
    return a * np.log(a) - gammaln(a)


def log_ndtr_pair(eta):
    """``(logPhi(-|eta|), logPhi(|eta|))`` as the kernel forms them (csrc/pla_glm.h, glm_log_ndtr_pair): one ``erfcx``, and the
    remainder of ``eta^2`` -- here from Veltkamp's split, there from a fused multiply-add; both are exact -- put back into the upper
    tail.  (``scipy.special.log_ndtr`` is ``log1p(-erfc(fl(x / sqrt 2)) / 2)`` there and loses ``x^2`` ulp to the rounded argument.)"""
    eta = np.asarray(eta, dtype=np.float64)
    with np.errstate(all="ignore"):
        h = 0.5 * erfcx(np.abs(eta) * 0.70710678118654752440)
        sq = eta * eta
        c = 134217729.0 * eta
        hi = c - (c - eta)
        lo = eta - hi
        r = np.where(sq < np.inf, ((hi * hi - sq) + 2.0 * (hi * lo)) + lo * lo, 0.0)
        r = np.where(np.isfinite(r), r, 0.0)  # (the split itself overflows above 1e300)
        w = 0.5 * sq
        return np.log(h) - w, np.log1p(-((h * np.exp(-w)) * (1.0 - 0.5 * r)))


def density(family, eta, y, scale=None, trials=None, oc=None, dc=None):
    """``ll`` (n, S) from ``eta`` (n, S) by the kernel's formulas; ``family`` is the engine's, ``scale`` [S] phi / alpha, ``oc`` [n] /
    ``dc`` [S] the constants handed to the kernel (None: 0 / computed from ``scale``)."""
    eta = np.asarray(eta, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)[:, None]
    c = 0.0 if oc is None else np.asarray(oc, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        if family == "binomial_probit":
            n = 1.0 if trials is None else np.asarray(trials, dtype=np.float64)[:, None]
            m = n - y
            lower, upper = log_ndtr_pair(eta)
            neg = eta < 0.0
            a = np.where(y != 0.0, y * np.where(neg, lower, upper), 0.0)
            b = np.where(m != 0.0, m * np.where(neg, upper, lower), 0.0)
            return (c + a) + b
        a = np.asarray(scale, dtype=np.float64)[None, :]
        d = (draw_const(scale) if dc is None else np.asarray(dc, dtype=np.float64))[None, :]
        if family == "negbinomial":
            lp = np.log(a)
            yp = y + a
            L = np.maximum(eta, lp) + np.log1p(np.exp(-np.abs(eta - lp)))
            return (((c + d) + gammaln(yp)) + y * eta) - yp * L
        if family == "gamma":
            return (d + (a - 1.0) * c) - a * (eta + y * np.exp(-eta))
    raise ValueError(family)


def magnitude(family, eta, y, scale=None, trials=None, oc=None, dc=None):
    """``T`` of the error measure in f64: the sum of the magnitudes of the formula's terms (good to a few ulp, which is all a
    denominator needs)."""
    eta = np.asarray(eta, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)[:, None]
    c = 0.0 if oc is None else np.asarray(oc, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        if family == "binomial_probit":
            n = 1.0 if trials is None else np.asarray(trials, dtype=np.float64)[:, None]
            lower, upper = log_ndtr_pair(eta)
            neg = eta < 0.0
            a = np.where(y != 0.0, y * np.where(neg, lower, upper), 0.0)
            b = np.where(n - y != 0.0, (n - y) * np.where(neg, upper, lower), 0.0)
            return np.abs(c) + np.abs(a) + np.abs(b)
        a = np.asarray(scale, dtype=np.float64)[None, :]
        d = np.asarray(dc, dtype=np.float64)[None, :]
        if family == "negbinomial":
            lp = np.log(a)
            L = np.maximum(eta, lp) + np.log1p(np.exp(-np.abs(eta - lp)))
            return np.abs(c) + np.abs(d) + np.abs(gammaln(y + a)) + np.abs(y * eta) + np.abs((y + a) * L)
        if family == "gamma":
            return np.abs(d) + np.abs((a - 1.0) * c) + np.abs(a * (eta + y * np.exp(-eta)))
    raise ValueError(family)


def log_lik(X, y, beta, family, scale=None, offset=None, trials=None):
    """The (N, S) matrix of an engine family with NumPy's own ``X @ beta.T`` and the fronts' constants."""
    return density(family, glm_ref.linpred(X, beta, offset), y, scale=scale, trials=trials, oc=obs_const(family, y, trials))


def reference(family, eta, y, scale=None, trials=None, oc=None, dc=None, digits=60):
    """``(ll, T)``: the formula at ``digits`` decimal digits with ``eta`` and the handed constants exact, rounded to f64, and the sum
    of the magnitudes of its terms (the error measure's denominator)."""
    import mpmath as mp

    eta = np.asarray(eta, dtype=np.float64)
    n, s = eta.shape
    ll, T = np.empty((n, s)), np.empty((n, s))
    with mp.workdps(digits):
        root2 = mp.sqrt(2)
        # (log1p on the upper side: 1 - Phi(-x) rounds to 1 at any working precision once x is large enough)
        log_phi = lambda x: mp.log(mp.erfc(-x / root2) / 2) if x < 0 else mp.log1p(-mp.erfc(x / root2) / 2)  # noqa: E731
        for i in range(n):
            yi = mp.mpf(float(y[i]))
            ci = mp.mpf(0.0 if oc is None else float(oc[i]))
            ni = mp.mpf(1.0 if trials is None else float(trials[i]))
            for j in range(s):
                e = mp.mpf(float(eta[i, j]))
                if family == "binomial_probit":
                    terms = [ci, yi * log_phi(e) if yi != 0 else mp.mpf(0), (ni - yi) * log_phi(-e) if ni != yi else mp.mpf(0)]
                else:
                    a, d = mp.mpf(float(scale[j])), mp.mpf(float(dc[j]))
                    if family == "negbinomial":
                        terms = [ci, d, mp.loggamma(yi + a), yi * e, -(yi + a) * mp.log(mp.exp(e) + a)]
                    else:
                        terms = [d, (a - 1) * ci, -a * (e + yi * mp.exp(-e))]
                ll[i, j] = float(mp.fsum(terms))
                T[i, j] = float(mp.fsum(abs(t) for t in terms))
    return ll, T


def measure(ll, ref, T):
    """``|ll - ref| / (u T + 1e-300)``: the error in units of the rounding of the formula's largest term."""
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(ll, dtype=np.float64) - ref) / (U * T + 1e-300)


def eta_values():
    rng = np.random.default_rng(1906)
    return np.concatenate([rng.uniform(-40.0, 40.0, 40), rng.uniform(-3.0, 3.0, 21), [0.0, 37.5, -37.5]])


@functools.lru_cache(maxsize=None)
def accuracy_grid(family):
    """A model with one predictor whose ``eta[i, s]`` is ``beta[s, 0]`` exactly (``X`` is a column of ones): rows carry the grid of
    ``y`` (and trials), draws the product of the grid of phi / alpha with ``eta_values()``.  Returns the model as a dict with the
    handed constants ``oc`` / ``dc`` and the engine family."""
    e = eta_values()
    trials = None
    if family == "negbinomial":
        y, scales = np.array([0.0, 1.0, 2.0, 7.0, 50.0, 1e4]), np.array([0.05, 0.5, 1.0, 3.7, 40.0, 1e3, 1e5])
    elif family == "gamma":
        y, scales = np.array([1e-8, 0.3, 1.0, 17.5, 1e6]), np.array([0.05, 0.5, 1.0, 3.7, 40.0, 1e3])
    elif family == "binomial_probit":
        y, trials, scales = np.array([0.0, 1.0, 3.0, 12.0]), np.full(4, 12.0), None
    elif family == "bernoulli_probit":
        y, scales = np.array([0.0, 1.0]), None
    else:
        raise ValueError(family)
    eng = "binomial_probit" if family == "bernoulli_probit" else family
    scale = None if scales is None else np.repeat(scales, e.size)
    beta = (e if scales is None else np.tile(e, scales.size)).reshape(-1, 1)
    return dict(X=np.ones((y.size, 1)), y=y, beta=beta, scale=scale, trials=trials, family=eng, oc=obs_const(eng, y, trials),
                dc=None if scale is None else draw_const(scale))


@functools.lru_cache(maxsize=None)
def _grid_reference(family, eta_bytes):
    g = accuracy_grid(family)
    eta = np.frombuffer(eta_bytes, dtype=np.float64).reshape(g["y"].size, -1)
    return reference(g["family"], eta, g["y"], g["scale"], g["trials"], g["oc"], g["dc"])


def grid_reference(family, eta):
    """``reference`` of ``accuracy_grid(family)`` on ``eta`` (the engine's own, or the restatement's): computed once per ``eta``."""
    return _grid_reference(family, np.ascontiguousarray(eta, dtype=np.float64).tobytes())


def make_model(rng, n, s, p, family, with_offset=False):
    """``glm_ref.make_model`` for an engine family of ENGINE_FAMILIES (``y`` drawn from the model at b0): a dict with ``scale`` [S]
    (phi / alpha or None) and ``trials``."""
    X = rng.normal(size=(n, p))
    X[:, 0] = 1.0
    b0 = 0.5 * rng.normal(size=p) / np.sqrt(p)
    beta = b0 + 0.15 * rng.normal(size=(s, p)) / np.sqrt(p)
    offset = 0.3 * rng.normal(size=n) if with_offset else None
    eta0 = X @ b0 + (0.0 if offset is None else offset)
    out = dict(X=X, beta=beta, family=family, scale=None, trials=None, offset=offset)
    if family == "negbinomial":
        out["scale"] = 2.0 * np.exp(0.2 * rng.normal(size=s))
        out["y"] = rng.negative_binomial(2.0, 2.0 / (2.0 + np.exp(eta0))).astype(np.float64)
    elif family == "gamma":
        out["scale"] = 3.0 * np.exp(0.2 * rng.normal(size=s))
        out["y"] = rng.gamma(3.0, np.exp(eta0) / 3.0)
    elif family == "binomial_probit":
        from scipy.special import ndtr

        out["trials"] = rng.integers(1, 12, size=n).astype(np.float64)
        out["y"] = rng.binomial(out["trials"].astype(int), ndtr(eta0)).astype(np.float64)
    else:
        raise ValueError(family)
    return out


def front_call(model, **more):
    """``(args, kwargs)`` of a front of ``pyloo_amd.loo_glm`` for a model of ``make_model``."""
    family, link, scale_kw = FRONT[model["family"]]
    kw = dict(offset=model["offset"], trials=model["trials"], **more)
    if link is not None:
        kw["link"] = link
    if scale_kw is not None:
        kw[scale_kw] = model["scale"]
    return (model["X"], model["y"], model["beta"], family), kw


def matrix_of(model):
    return log_lik(model["X"], model["y"], model["beta"], model["family"], model["scale"], model["offset"], model["trials"])
