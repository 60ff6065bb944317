"""NumPy restatement of the GLM generator with group-level terms (include/pyloo_amd.h, ``pla_glm_grouped``): the terms added to the
linear predictor of tests/glm_ref.py in the kernel's order of operations, generators of multilevel test models and a stand-in
engine whose grouped call is this restatement.  TEST INFRASTRUCTURE ONLY."""

import numpy as np

import glm_ref
from fake_engine import OracleEngine


def split(term):
    """``(index, draws, z)`` of a term given as ``(index, draws)`` or ``(index, draws, z)``."""
    return (*term, None)[:3]


def add_terms(eta, terms, rows=None):
    """``((eta + z_0 u_0[:, g_0].T) + z_1 u_1[:, g_1].T) + ...``: every product and every sum rounded once, in the order of the
    terms; with ``z`` None the product is not formed.  ``rows``: the observations the rows of ``eta`` stand for."""
    eta = np.asarray(eta, dtype=np.float64)
    sel = slice(None) if rows is None else np.asarray(rows)
    with np.errstate(all="ignore"):
        for term in terms or ():
            index, draws, z = split(term)
            u = np.asarray(draws, dtype=np.float64)[:, np.asarray(index)[sel]].T
            eta = eta + u if z is None else eta + np.asarray(z, dtype=np.float64)[sel][:, None] * u
    return eta


def linpred(X, beta, offset=None, terms=None):
    return add_terms(glm_ref.linpred(X, beta, offset), terms)


def log_lik(X, y, beta, family, sigma=None, offset=None, trials=None, terms=None):
    """The (N, S) matrix of the user-facing family with NumPy's own ``X @ beta.T`` and the terms added."""
    fam = glm_ref.ENGINE_FAMILY[family]
    oc = None if family == "bernoulli" else glm_ref.obs_const(fam, y, trials)
    return glm_ref.density(fam, linpred(X, beta, offset, terms), y, sigma=sigma, trials=trials, oc=oc)


def make_terms(rng, n, s, sizes, slopes):
    """One term per entry of ``sizes``: group indices in no order, the last group held by the last row only when there is room;
    draws u = u0 + 0.15 N(0,1), u0 = 0.4 N(0,1); a covariate z ~ N(0,1) where ``slopes`` says so.  Returns (terms, u0 per term)."""
    terms, centres = [], []
    for g, slope in zip(sizes, slopes):
        index = rng.integers(0, max(g - 1, 1), size=n).astype(np.int64)
        index[-1] = g - 1
        u0 = 0.4 * rng.normal(size=g)
        draws = u0 + 0.15 * rng.normal(size=(s, g))
        terms.append((index, draws, rng.normal(size=n)) if slope else (index, draws))
        centres.append(u0)
    return terms, centres


def make_model(rng, n, s, p, family, sizes=(5, 3), slopes=(False, True), with_offset=True):
    """glm_ref.make_model with group-level terms: ``y`` is drawn from the model at b0 and the centres of the group effects."""
    X = rng.normal(size=(n, p))
    X[:, 0] = 1.0
    b0 = 0.5 * rng.normal(size=p) / np.sqrt(p)
    beta = b0 + 0.15 * rng.normal(size=(s, p)) / np.sqrt(p)
    offset = 0.3 * rng.normal(size=n) if with_offset else None
    terms, centres = make_terms(rng, n, s, sizes, slopes)
    eta0 = X @ b0 + (0.0 if offset is None else offset)
    for term, u0 in zip(terms, centres):
        index, _, z = split(term)
        eta0 = eta0 + (1.0 if z is None else z) * u0[index]
    out = dict(X=X, beta=beta, family=family, sigma=None, trials=None, offset=offset, terms=terms)
    if family == "gaussian":
        out["sigma"] = np.exp(0.1 * rng.normal(size=s))
        out["y"] = eta0 + rng.normal(size=n)
    elif family == "bernoulli":
        out["y"] = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta0))).astype(np.float64)
    elif family == "binomial":
        out["trials"] = rng.integers(1, 12, size=n).astype(np.float64)
        out["y"] = rng.binomial(out["trials"].astype(int), 1.0 / (1.0 + np.exp(-eta0))).astype(np.float64)
    elif family == "poisson":
        out["y"] = rng.poisson(np.exp(eta0)).astype(np.float64)
    else:
        raise ValueError(family)
    return out


def matrix_of(model):
    return log_lik(model["X"], model["y"], model["beta"], model["family"], model["sigma"], model["offset"], model["trials"], model["terms"])


def front_args(model):
    return ((model["X"], model["y"], model["beta"], model["family"]),
            dict(sigma=model["sigma"], offset=model["offset"], trials=model["trials"], groups=model["terms"]))


class GroupedEngine(OracleEngine):
    """The oracle-backed stand-in with ``Engine.glm``: the restatement on the vectors and the terms it is handed; records calls
    (``groups`` as it arrived: absent, None or the list)."""

    def __init__(self):
        self.calls = []

    def glm(self, X, beta, family, y=None, offset=None, trials=None, obs_const=None, draw_scale=None, draw_const=None, rows=None,
            mode="matrix", tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True, **extra):
        assert set(extra) <= {"groups"}, extra
        self.calls.append(dict(op="glm", family=family, mode=mode, tail_count=tail_count, method=method, y=y, offset=offset, trials=trials,
                               obs_const=obs_const, draw_scale=draw_scale, draw_const=draw_const, n_draws=np.asarray(beta).shape[0],
                               rows=None if rows is None else np.asarray(rows).copy(), has_groups="groups" in extra,
                               groups=extra.get("groups"), good_k=good_k, scale_value=scale_value))
        X = np.asarray(X)
        sel = slice(None) if rows is None else np.asarray(rows)
        pick = lambda v: None if v is None else np.asarray(v)[sel]  # noqa: E731
        eta = add_terms(glm_ref.linpred(X[sel], beta, pick(offset)), extra.get("groups"), rows=rows)
        ll = eta if family == "linpred" else glm_ref.density(family, eta, pick(y), sigma=draw_scale, trials=pick(trials), oc=pick(obs_const),
                                                               dc=draw_const)
        if mode == "matrix":
            return ll
        bad = np.isnan(ll)
        res = self.psis_loo(np.where(bad, -1e10, ll), tail_count, method, scale_value, good_k)
        res["n_replaced"] = int(bad.sum())
        return res
