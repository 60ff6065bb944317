"""Host side of the GLM fronts (``pyloo_amd/loo_glm.py``) without a GPU.  The yardstick first: the NumPy restatement
(tests/glm_ref.py) against closed forms and scipy's densities.  Then the feature: the fronts through an oracle-backed stand-in
engine (every rejection before the first engine call, the constants handed over, ``ELPDData`` keys and warnings against
``loo_from_matrix`` on the restatement's matrix, column order of ``loo_glm``, ``rows=``, ``loo_subsample_glm`` against
``loo_subsample_from_matrix``), the C export and the generated code of the new kernels.

The tests of the first section hold the restatement itself and pass with or without the feature.  Every test from the front on
fails without it (the module, the symbol and the kernel unit are missing)."""

import ctypes as C
import importlib
import os
import re
import shutil
import sys
import warnings

import numpy as np
import pytest
from scipy import stats

import glm_ref
from fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."
FAMILIES = ("gaussian", "bernoulli", "binomial", "poisson")


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def test_closed_forms():
    n, s = 7, 5
    eta = np.zeros((n, s))
    y = np.array([0.0, 1, 1, 0, 1, 0, 0])
    assert np.array_equal(glm_ref.density("binomial", eta, y), np.full((n, s), -np.log(2.0)))
    rng = np.random.default_rng(1)
    eta = rng.normal(size=(n, s)) * 3.0
    assert np.array_equal(glm_ref.density("poisson", eta, np.zeros(n), oc=glm_ref.obs_const("poisson", np.zeros(n))), -np.exp(eta))
    # softplus at the far ends neither overflows nor loses the linear part: y eta - softplus(eta) is -4e-18 and -40 - 4e-18, here
    # to the rounding of numbers of size 40 (half an ulp, 2^-48)
    far = glm_ref.density("binomial", np.array([[40.0, -40.0]]), np.array([1.0]))
    assert abs(far[0, 0]) <= 2.0 ** -48 and far[0, 1] == -40.0


def test_densities_match_scipy():
    rng = np.random.default_rng(2)
    n, s = 40, 30
    eta = rng.normal(size=(n, s)) * 1.5
    worst = {}
    y = rng.normal(size=n) * 2.0
    sigma = np.exp(0.3 * rng.normal(size=s))
    got = glm_ref.density("gaussian", eta, y, sigma=sigma)
    worst["gaussian"] = np.abs(got - stats.norm.logpdf(y[:, None], eta, sigma[None, :])).max()
    trials = rng.integers(1, 15, size=n).astype(np.float64)
    yb = rng.binomial(trials.astype(int), 0.4).astype(np.float64)
    got = glm_ref.density("binomial", eta, yb, trials=trials, oc=glm_ref.obs_const("binomial", yb, trials))
    worst["binomial"] = np.abs(got - stats.binom.logpmf(yb[:, None], trials[:, None], 1.0 / (1.0 + np.exp(-eta)))).max()
    yp = rng.poisson(2.0, size=n).astype(np.float64)
    got = glm_ref.density("poisson", eta, yp, oc=glm_ref.obs_const("poisson", yp))
    worst["poisson"] = np.abs(got - stats.poisson.logpmf(yp[:, None], np.exp(eta))).max()
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v <= 1e-12 for v in worst.values()), worst


def test_the_dot_product_bound_holds_for_numpy_itself():
    rng = np.random.default_rng(3)
    for p in (1, 5, 64, 256):
        X, beta, off = rng.normal(size=(33, p)), rng.normal(size=(17, p)), rng.normal(size=33)
        exact = glm_ref.linpred(X, beta, off, dtype=np.longdouble)
        err = np.abs(glm_ref.linpred(X, beta, off).astype(np.longdouble) - exact).astype(np.float64)
        assert np.all(err <= glm_ref.linpred_bound(X, beta, off)), p


# -------------------------------------------------------------------------------------------------------------------- the front
class GlmEngine(OracleEngine):
    """The oracle-backed stand-in with the pass this feature calls: the restatement on the vectors it is handed; records calls."""

    def __init__(self):
        self.calls = []

    def glm(self, X, beta, family, y=None, offset=None, trials=None, obs_const=None, draw_scale=None, draw_const=None, rows=None,
            mode="matrix", tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True):
        self.calls.append(dict(op="glm", family=family, mode=mode, tail_count=tail_count, method=method, y=y, offset=offset, trials=trials,
                               obs_const=obs_const, draw_scale=draw_scale, draw_const=draw_const, n_draws=np.asarray(beta).shape[0],
                               rows=None if rows is None else np.asarray(rows).copy()))
        X = np.asarray(X)
        sel = slice(None) if rows is None else np.asarray(rows)
        pick = lambda v: None if v is None else np.asarray(v)[sel]  # noqa: E731
        eta = glm_ref.linpred(X[sel], beta, pick(offset))
        ll = eta if family == "linpred" else glm_ref.density(family, eta, pick(y), sigma=draw_scale, trials=pick(trials), oc=pick(obs_const),
                                                               dc=draw_const)
        if mode == "matrix":
            return ll
        bad = np.isnan(ll)
        res = self.psis_loo(np.where(bad, -1e10, ll), tail_count, method, scale_value, good_k)
        res["n_replaced"] = int(bad.sum())
        return res


@pytest.fixture()
def fake(monkeypatch):
    eng = GlmEngine()
    for name in ("pyloo_amd.loo", "pyloo_amd.loo_glm", "pyloo_amd.loo_subsample", "pyloo_amd.base"):
        monkeypatch.setattr(importlib.import_module(name), "get_engine", lambda device=None: eng)
    return eng


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


def front_args(model):
    return (model["X"], model["y"], model["beta"], model["family"]), dict(sigma=model["sigma"], offset=model["offset"], trials=model["trials"])


@pytest.fixture(scope="module")
def models():
    rng = np.random.default_rng(11)
    return {f: glm_ref.make_model(rng, 14, 400, 5, f, with_offset=f != "bernoulli") for f in FAMILIES}


def test_every_rejection_comes_before_any_engine_call(fake, models):
    import pyloo_amd as pl

    g, b, po = models["gaussian"], models["binomial"], models["poisson"]

    def variant(model, **changes):
        m = dict(model)
        m.update(changes)
        a, k = front_args(m)
        extra = {key: m[key] for key in ("reff",) if key in m}
        return a, {**k, **extra}

    X, beta = g["X"], g["beta"]
    bad_x = X.copy()
    bad_x[3, 2] = np.inf
    bad_b = beta.copy()
    bad_b[7, 1] = np.nan
    frac = po["y"].copy()
    frac[2] = 1.5
    neg = po["y"].copy()
    neg[4] = -1.0
    cases = [
        (variant(g, beta=beta[:, :4]), "P = 5"),
        (variant(g, y=g["y"][:-1]), "y needs 14 values"),
        (variant(g, X=np.ones((14, 257)), beta=np.ones((400, 257))), "257 columns"),
        (variant(g, sigma=None), "needs sigma"),
        (variant(po, sigma=g["sigma"]), "sigma belongs to the gaussian family"),
        (variant(g, sigma=np.where(np.arange(400) == 9, 0.0, g["sigma"])), "finite and positive"),
        (variant(g, sigma=np.where(np.arange(400) == 9, np.inf, g["sigma"])), "finite and positive"),
        (variant(g, sigma=g["sigma"][:-1]), "sigma needs 400 values"),
        (variant(po, trials=b["trials"]), "trials belongs to the binomial family"),
        (variant(b, trials=None), "needs trials"),
        (variant(po, y=frac), "non-negative integers"),
        (variant(po, y=neg), "non-negative integers"),
        (variant(b, y=b["trials"] + 1.0), "y exceeds trials"),
        (variant(models["bernoulli"], y=np.full(14, 2.0)), "y exceeds trials"),
        (variant(g, X=bad_x), "X holds values that are not finite"),
        (variant(g, beta=bad_b), "beta holds values that are not finite"),
        (variant(g, offset=np.where(np.arange(14) == 1, np.nan, g["offset"])), "offset holds values that are not finite"),
        (variant(g, offset=g["offset"][:3]), "offset needs 14 values"),
        (variant(g, reff=None), "reff must be a positive float"),
        (variant(g, reff=np.full(14, 0.8)), "reff must be a positive float"),
        (variant(g, reff=0.0), "reff must be a positive float"),
        (variant(g, reff=-1.0), "reff must be a positive float"),
    ]
    for (a, k), word in cases:
        with pytest.raises(ValueError) as err:
            pl.loo_glm_from_design(*a, **k)
        assert word in str(err.value), (word, str(err.value))
        k.pop("reff", None)
        for fn in (pl.glm_log_lik, pl.glm_plpd):
            if "reff" in word:
                continue
            with pytest.raises(ValueError) as err:
                fn(*a, **k)
            assert word in str(err.value), (fn.__name__, word, str(err.value))
    with pytest.raises(ValueError, match="family must be one of"):
        pl.loo_glm_from_design(X, g["y"], beta, "probit")
    with pytest.raises(ValueError, match="2-D"):
        pl.glm_log_lik(X[0], g["y"], beta, "gaussian", sigma=g["sigma"])
    with pytest.raises(ValueError, match="loo_approximation"):
        pl.loo_subsample_glm(X, g["y"], beta, "gaussian", sigma=g["sigma"], loo_approximation="tis")
    with pytest.raises(ValueError, match="between 1 and 14"):
        pl.loo_subsample_glm(X, g["y"], beta, "gaussian", sigma=g["sigma"], observations=15)
    assert fake.calls == []


def test_the_constants_handed_over_are_the_restatements(fake, models):
    import pyloo_amd as pl

    for f in FAMILIES:
        m = models[f]
        a, k = front_args(m)
        fake.calls.clear()
        ll = pl.glm_log_lik(*a, **k)
        c = fake.calls[0]
        assert c["family"] == glm_ref.ENGINE_FAMILY[f] and c["mode"] == "matrix" and c["rows"] is None
        want_oc = None if f in ("gaussian", "bernoulli") else glm_ref.obs_const(glm_ref.ENGINE_FAMILY[f], m["y"], m["trials"])
        assert (c["obs_const"] is None) == (want_oc is None) and (want_oc is None or np.array_equal(c["obs_const"], want_oc)), f
        if f == "gaussian":
            assert np.array_equal(c["draw_const"], glm_ref.draw_const(m["sigma"])) and np.array_equal(c["draw_scale"], m["sigma"])
        else:
            assert c["draw_const"] is None and c["draw_scale"] is None
        assert (c["trials"] is None) == (f != "binomial")
        assert np.array_equal(ll, glm_ref.matrix_of(m)), f
        # the linear predictor: no family vectors travel
        fake.calls.clear()
        eta = pl.glm_log_lik(*a, **k, linpred=True)
        assert fake.calls[0]["family"] == "linpred" and fake.calls[0]["y"] is None and fake.calls[0]["obs_const"] is None
        assert np.array_equal(eta, glm_ref.linpred(m["X"], m["beta"], m["offset"]))


def test_plpd_is_the_log_likelihood_at_the_posterior_mean(fake, models):
    import pyloo_amd as pl

    for f in FAMILIES:
        m = models[f]
        a, k = front_args(m)
        fake.calls.clear()
        got, msgs = quiet(pl.glm_plpd, *a, **k)
        assert not msgs and len(fake.calls) == 1 and fake.calls[0]["n_draws"] == 1 and fake.calls[0]["mode"] == "matrix"
        sig = None if m["sigma"] is None else m["sigma"].mean().reshape(1)
        want = glm_ref.log_lik(m["X"], m["y"], m["beta"].mean(0).reshape(1, -1), f, sig, m["offset"], m["trials"])[:, 0]
        assert got.shape == (14,) and np.array_equal(got, want), f


@pytest.mark.parametrize("family", FAMILIES)
def test_elpd_data_equals_loo_from_matrix_on_the_restatements_matrix(fake, models, family):
    import pyloo_amd as pl

    m = models[family]
    a, k = front_args(m)
    ll = glm_ref.matrix_of(m)
    for kwargs in (dict(), dict(pointwise=True, reff=0.7), dict(method="sis", pointwise=True), dict(method="tis", scale="deviance")):
        fake.calls.clear()
        got, msgs = quiet(pl.loo_glm_from_design, *a, **k, **kwargs)
        want, want_msgs = quiet(pl.loo_from_matrix, ll, **kwargs)
        assert len(fake.calls) == 1 and fake.calls[0]["mode"] == "loo"
        assert list(got.index) == list(want.index) and msgs == want_msgs, (kwargs, msgs, want_msgs)
        assert got.method == want.method
        for key in want.index:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), (kwargs, key)


def test_high_k_and_nan_warnings_have_loo_from_matrix_texts(fake, models, monkeypatch):
    import pyloo_amd as pl

    m = dict(models["poisson"])
    m["y"] = m["y"].copy()
    m["y"][3] = 60.0  # an outlier: its Pareto k is high
    a, k = front_args(m)
    got, msgs = quiet(pl.loo_glm_from_design, *a, **k, pointwise=True)
    want, want_msgs = quiet(pl.loo_from_matrix, glm_ref.matrix_of(m), pointwise=True)
    assert any("Pareto" in t for t in msgs) and msgs == want_msgs and got["warning"] is True

    class NanEngine(GlmEngine):  # a NaN can only come out of the generator (the fronts reject what is not finite): through the engine
        def glm(self, *args, **kw):
            kw["offset"] = np.where(np.arange(14) == 5, np.nan, 0.0)
            return GlmEngine.glm(self, *args, **kw)

    eng = NanEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_glm"), "get_engine", lambda device=None: eng)
    res, msgs = quiet(pl.loo_glm_from_design, *front_args(models["poisson"])[0], pointwise=True)
    assert msgs.count(NAN_TEXT) == 1 and np.isfinite(res["elpd_loo"])


def test_rows(fake, models):
    import pyloo_amd as pl

    m = models["binomial"]
    a, k = front_args(m)
    rows = [9, 2, 2, 13, 0]
    full = glm_ref.matrix_of(m)
    sub = pl.glm_log_lik(*a, **k, rows=rows)
    assert fake.calls[-1]["rows"].tolist() == rows and np.array_equal(sub, full[rows])
    got, _ = quiet(pl.loo_glm_from_design, *a, **k, rows=rows, pointwise=True)
    want, _ = quiet(pl.loo_from_matrix, full[rows], pointwise=True)
    assert fake.calls[-1]["rows"].tolist() == rows and got["n_data_points"] == 5
    assert np.array_equal(got["loo_i"], want["loo_i"]) and np.array_equal(got["pareto_k"], want["pareto_k"])


def test_loo_glm_takes_the_columns_in_the_order_given(fake, models):
    import pyloo_amd as pl

    m = models["gaussian"]
    chains = 4
    beta, sigma = m["beta"], m["sigma"]
    post = {"slopes": beta[:, 1:4].reshape(chains, 100, 3), "last": beta[:, 4].reshape(chains, 100),
            "intercept": beta[:, 0].reshape(chains, 100), "sigma": sigma.reshape(chains, 100)}
    data = {"posterior": post}
    got, _ = quiet(pl.loo_glm, data, m["X"], m["y"], "gaussian", ["intercept", "slopes", "last"], sigma_name="sigma", offset=m["offset"],
                   pointwise=True)
    want, _ = quiet(pl.loo_glm_from_design, m["X"], m["y"], beta, "gaussian", sigma=sigma, offset=m["offset"], pointwise=True)
    assert np.array_equal(got["loo_i"], want["loo_i"]) and got["elpd_loo"] == want["elpd_loo"]
    # another order is another model
    other, _ = quiet(pl.loo_glm, data, m["X"], m["y"], "gaussian", ["slopes", "intercept", "last"], sigma_name="sigma", offset=m["offset"])
    assert other["elpd_loo"] != want["elpd_loo"]
    with pytest.raises(ValueError) as err:
        pl.loo_glm(data, m["X"], m["y"], "gaussian", ["intercept", "slopes"], sigma_name="sigma")
    assert "4 columns (intercept, slopes[0], slopes[1], slopes[2]) for the 5 columns of X" in str(err.value)
    with pytest.raises(ValueError, match="not found in posterior"):
        pl.loo_glm(data, m["X"], m["y"], "gaussian", ["intercept", "gamma"])
    with pytest.raises(ValueError, match="scalar variable"):
        pl.loo_glm(data, m["X"], m["y"], "gaussian", ["intercept", "slopes", "last"], sigma_name="slopes")
    # y from observed_data
    data["observed_data"] = {"obs": m["y"]}
    named, _ = quiet(pl.loo_glm, data, m["X"], None, "gaussian", ["intercept", "slopes", "last"], sigma_name="sigma", var_name="obs",
                     offset=m["offset"])
    assert named["elpd_loo"] == want["elpd_loo"]


# ---------------------------------------------------------------------------------------------------------------- subsampled LOO
@pytest.mark.parametrize("estimator", ["diff_srs", "hh_pps", "srs"])
@pytest.mark.parametrize("family", ["gaussian", "poisson"])
def test_subsample_lpd_equals_loo_subsample_from_matrix(fake, family, estimator):
    import pyloo_amd as pl

    m = glm_ref.make_model(np.random.default_rng(21), 60, 300, 4, family)
    a, k = front_args(m)
    ll = glm_ref.matrix_of(m)
    for obs, draws in ((12, None), (np.array([3, 50, 7, 8, 21, 22]), 64)):
        if isinstance(obs, np.ndarray) and estimator == "hh_pps":
            continue
        np.random.seed(5)
        (got, idx, est), msgs = quiet(pl.loo_subsample_glm, *a, **k, observations=obs, loo_approximation="lpd", estimator=estimator,
                                      loo_approximation_draws=draws, pointwise=True)
        np.random.seed(5)
        (want, widx, west), wmsgs = quiet(pl.loo_subsample_from_matrix, ll, observations=obs, loo_approximation="lpd", estimator=estimator,
                                          loo_approximation_draws=draws, pointwise=True)
        assert np.array_equal(idx.idx, widx.idx) and np.array_equal(idx.m_i, widx.m_i) and msgs == wmsgs
        assert list(got.index) == list(want.index)
        np.testing.assert_allclose(np.array(est[:4], dtype=float), np.array(west[:4], dtype=float), rtol=1e-12)
        for key in ("elpd_loo", "se", "p_loo", "p_loo_se", "subsampling_SE", "looic"):
            np.testing.assert_allclose(got[key], want[key], rtol=1e-12, err_msg=key)
        np.testing.assert_allclose(got["loo_i"], want["loo_i"], rtol=1e-12, equal_nan=True)
        rows_call = [c for c in fake.calls if c["rows"] is not None][-1]
        assert rows_call["rows"].tolist() == list(idx.idx) and rows_call["mode"] == "matrix"


def test_subsample_plpd_uses_the_posterior_mean_without_a_warning(fake):
    import pyloo_amd as pl

    m = glm_ref.make_model(np.random.default_rng(22), 50, 300, 3, "binomial", with_offset=True)
    a, k = front_args(m)
    np.random.seed(9)
    (got, idx, est), msgs = quiet(pl.loo_subsample_glm, *a, **k, observations=10, loo_approximation="plpd")
    assert not msgs, msgs
    first = fake.calls[0]
    assert first["n_draws"] == 1 and first["mode"] == "matrix" and first["rows"] is None
    approx = glm_ref.log_lik(m["X"], m["y"], m["beta"].mean(0).reshape(1, -1), "binomial", None, m["offset"], m["trials"])[:, 0]
    # the difference estimator with the restatement's approximation and the oracle's loo_i of the sampled rows
    from pyloo_amd.loo_subsample import diff_srs_estimate

    eng = OracleEngine()
    from oracle import psis_oracle as orc

    loo_m = eng.psis_loo(glm_ref.matrix_of(m)[idx.idx], orc.tail_count(300, 1.0))["loo_i"]
    want = diff_srs_estimate(approx, loo_m, idx.idx)
    np.testing.assert_allclose(est.y_hat, want.y_hat, rtol=1e-12)
    assert got["elpd_loo"] == est.y_hat and got["subsample_size"] == 10 and got.method == "loo_subsample"


# ------------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (as tests/test_capi_abi.py: a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


def test_new_symbol_in_header_binding_and_library(lib):
    from pyloo_amd import _capi
    from pyloo_amd import build as b

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pla_glm" in _capi.SYMBOLS and hasattr(lib, "pla_glm")
    assert re.search(r"\bint pla_glm\(const pla_glm_args \*", header) and re.search(r"\bpla_glm\b", guide)
    assert len(lib.pla_glm.argtypes) == 1
    assert lib.pla_abi_version() == 7 and _capi.ABI_VERSION == 7 and "#define PLA_ABI_VERSION 7" in header
    assert "pla_k_glm.hip" in b.SOURCES and "pla_capi_glm.hip" in b.SOURCES
    # the binding's struct is the header's, field for field
    body = re.search(r"typedef struct pla_glm_args \{(.*?)\} pla_glm_args;", header, flags=re.S).group(1)
    declared = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert declared == [name for name, _ in _capi.GlmArgs._fields_], declared
    assert C.sizeof(_capi.GlmArgs) == 8 * (len(declared) - 2)  # (every field 8 bytes but the four int32)
    for name in ("PLA_GLM_LINPRED", "PLA_GLM_GAUSSIAN", "PLA_GLM_BINOMIAL_LOGIT", "PLA_GLM_POISSON_LOG", "PLA_GLM_MODE_MATRIX",
                 "PLA_GLM_MODE_LOO"):
        assert f"#define {name} {getattr(_capi, name)}\n" in header, name


def test_argument_errors_each_have_their_own_message(lib):
    from pyloo_amd import _capi

    seen = set()

    def message(args):
        assert lib.pla_glm(C.byref(args)) == -1
        msg = lib.pla_last_error()
        assert msg not in seen, msg
        seen.add(msg)
        return msg

    assert lib.pla_glm(None) == -1 and lib.pla_last_error() == b"args is NULL"
    seen.add(b"args is NULL")
    args = _capi.GlmArgs(n_obs=2, n_pred=3, n_draws=16, x_stride_obs=3, x_stride_pred=1, beta_stride_draw=3, beta_stride_pred=1)
    assert b"engine is NULL" in message(args)
    args.struct_size -= 8
    args.engine = 1  # (never followed: nothing below gets past the argument checks)
    msg = message(args)
    assert b"struct_size" in msg and str(C.sizeof(_capi.GlmArgs)).encode() in msg
    args.struct_size += 8
    args.family = 7
    assert b"family" in message(args)
    args.family, args.mode = _capi.PLA_GLM_POISSON_LOG, 5
    assert b"mode" in message(args)
    args.family, args.mode = _capi.PLA_GLM_LINPRED, _capi.PLA_GLM_MODE_LOO
    assert b"LINPRED" in message(args)
    args.family, args.mode = _capi.PLA_GLM_POISSON_LOG, _capi.PLA_GLM_MODE_MATRIX
    args.n_pred = 0
    assert b"n_pred must lie in [1, 256], got 0" in message(args)
    args.n_pred = 257
    assert b"n_pred must lie in [1, 256], got 257" in message(args)
    args.n_pred = 3
    assert b"x is NULL" in message(args)
    buf = (C.c_double * 64)()
    args.x = C.addressof(buf)
    assert b"beta is NULL" in message(args)
    args.beta = C.addressof(buf)
    args.x_stride_pred = 0
    assert b"x strides" in message(args)
    args.x_stride_pred, args.beta_stride_draw = 1, -3
    assert b"beta strides" in message(args)
    args.beta_stride_draw = 3
    assert b"y is NULL" in message(args)
    args.y = C.addressof(buf)
    args.family = _capi.PLA_GLM_GAUSSIAN
    assert b"draw_scale" in message(args)


# ------------------------------------------------------------------------------------------------------------- the generated code
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_new_kernels_use_no_scratch_and_keep_the_stated_occupancy(tmp_path):
    """no scratch, no LDS and no scalar register in a vector lane in any kernel of the unit; one MFMA chain of four
    steps per chunk in every GLM kernel; four wavefronts per SIMD with one or two chunks of predictors in registers (P <= 32),
    three with four (P <= 64), two with eight (P <= 128 and the panels beyond); the prepare kernel within 64 registers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    lines = isa_stats.compile_isa(out=str(tmp_path / "glm.s"), units=["pla_k_glm.hip"])
    names = [k for k in isa_stats.all_kernels(lines) if "glm_" in k]
    # prepare; four families x (1, 2, 4, 8 chunks in registers + panels of 8)
    assert len(names) == 1 + 20, names
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert not isa_stats.masked_spills(lines, k[2:]) and total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert res.get("LDSByteSize", 0) == 0, (name, res)
        regs = res["NumVgprs"] + res.get("NumAgprs", 0)
        if "prepare" in k:
            assert regs <= 64, (name, res)
            continue
        nch, panel = re.search(r"Li\dELi(\d)ELb([01])E", k).groups()
        start = next(i for i, l in enumerate(lines) if l.startswith(k + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[i]))
        mfma = sum(l.strip().startswith("v_mfma_f64_16x16x4_f64") for l in lines[start:end])
        assert mfma == 4 * int(nch), (name, mfma)  # one chain: four steps per chunk, the tile loop not duplicated
        waves = {1: 4, 2: 4, 4: 3, 8: 2}[int(nch)]
        assert regs <= 512 // waves // 8 * 8 and res.get("Occupancy", 0) >= waves, (name, res)
