"""Host side of the negative-binomial and gamma families and the probit link of the GLM fronts (``pyloo_amd/loo_glm.py``) without a
GPU.  The yardstick first: the NumPy restatement (tests/glm_families_ref.py) against scipy's distributions and against the mpmath
reference on the accuracy grid -- the figures the GPU tests' bound is made of.  Then the feature: the fronts through an
oracle-backed stand-in engine (every rejection before the first engine call, the constants handed over, ``loo_glm``'s
``phi_name`` / ``shape_name``, ``glm_plpd`` at the mean), the marginal fronts' refusal, the C export and the generated code of the
new kernel units.

The tests of the first section hold the restatement itself and pass with or without the feature.  Every test from the front on
fails without it (the fronts do not know the arguments, the library not the codes, the units are missing)."""

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

import glm_families_ref as fref
import glm_ref
from fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def test_densities_match_scipy():
    rng = np.random.default_rng(2)
    n, s = 40, 30
    eta = rng.normal(size=(n, s)) * 1.5
    worst = {}
    phi = np.exp(rng.normal(size=s))
    y = rng.poisson(3.0, size=n).astype(np.float64)
    got = fref.density("negbinomial", eta, y, scale=phi, oc=fref.obs_const("negbinomial", y))
    worst["negbinomial"] = np.abs(got - stats.nbinom.logpmf(y[:, None], phi[None, :], phi[None, :] / (phi[None, :] + np.exp(eta)))).max()
    alpha = np.exp(rng.normal(size=s))
    yg = rng.gamma(2.0, 1.0, size=n)
    got = fref.density("gamma", eta, yg, scale=alpha, oc=fref.obs_const("gamma", yg))
    worst["gamma"] = np.abs(got - stats.gamma.logpdf(yg[:, None], alpha[None, :], scale=np.exp(eta) / alpha[None, :])).max()
    trials = rng.integers(1, 15, size=n).astype(np.float64)
    yb = rng.binomial(trials.astype(int), 0.4).astype(np.float64)
    got = fref.density("binomial_probit", eta, yb, trials=trials, oc=fref.obs_const("binomial_probit", yb, trials))
    # (not binom.logpmf at p = norm.cdf(eta): its log1p(-p) has lost the upper tail to the rounding of p)
    want = stats.binom.logpmf(yb, trials, 0.5)[:, None] + trials[:, None] * np.log(2.0)
    want = want + yb[:, None] * stats.norm.logcdf(eta) + (trials - yb)[:, None] * stats.norm.logcdf(-eta)
    worst["probit"] = np.abs(got - want).max()
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v <= 1e-11 for v in worst.values()), worst


def test_probit_tails_are_finite_and_a_zero_factor_forms_no_product():
    eta = np.array([[37.5, -37.5, 0.0, np.inf, -np.inf]])
    one, zero = fref.density("binomial_probit", eta, np.array([1.0])), fref.density("binomial_probit", eta, np.array([0.0]))
    assert np.all(np.isfinite(one[0, :3])) and np.all(np.isfinite(zero[0, :3]))
    assert one[0, 0] < 0.0 and abs(one[0, 0]) < 1e-300 and abs(one[0, 1] + 707.669) < 0.001 and one[0, 1] == zero[0, 0]
    assert one[0, 2] == zero[0, 2] and abs(one[0, 2] + np.log(2.0)) <= 2.0 ** -52
    # y = 1 at eta = +inf: 1 * logPhi(inf) + 0 * logPhi(-inf) is 0, not 0 * -inf
    assert one[0, 3] == 0.0 and one[0, 4] == -np.inf and zero[0, 3] == -np.inf and zero[0, 4] == 0.0


@pytest.mark.parametrize("grid", fref.ENGINE_FAMILIES + ("bernoulli_probit",))
def test_the_restatements_own_error_on_the_accuracy_grid(grid):
    """The figure the GPU tests' bound is four times of: the restatement against the mpmath reference, eta and the handed constants
    exact.  It is measured here, not assumed; no value on the grid is non-finite.  The GPU bound is made of the recorded figures
    (RESTATEMENT_FIGURE), not of this run's: this test holds the run within twice the record, since another build of NumPy's exp /
    log1p may differ by an ulp per call and the cancellation inside the gamma term (0.467 - 0.443 at the worst point) turns one ulp
    into 4.8 units of the measure."""
    g = fref.accuracy_grid(grid)
    eta = glm_ref.linpred(g["X"], g["beta"])
    assert np.array_equal(eta, np.broadcast_to(g["beta"][:, 0], eta.shape))  # (X is a column of ones: eta is beta, exactly)
    ref, T = fref.grid_reference(grid, eta)
    ll = fref.density(g["family"], eta, g["y"], g["scale"], g["trials"], g["oc"], g["dc"])
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(ref)) and np.all(T >= 0)
    worst = float(fref.measure(ll, ref, T).max())
    print(f"{grid}: the restatement's largest |ll - mpmath| / (u T) = {worst:.2f}")
    assert worst <= 2.0 * fref.RESTATEMENT_FIGURE[g["family"]], worst
    np.testing.assert_allclose(fref.magnitude(g["family"], eta, g["y"], g["scale"], g["trials"], g["oc"], g["dc"]), T, rtol=1e-13, atol=1e-300)


# -------------------------------------------------------------------------------------------------------------------- the front
class GlmEngine(OracleEngine):
    """The oracle-backed stand-in with the pass the fronts call: the restatements on the vectors it is handed; records calls."""

    def __init__(self):
        self.calls = []

    def glm(self, X, beta, family, y=None, offset=None, trials=None, obs_const=None, draw_scale=None, draw_const=None, rows=None,
            mode="matrix", tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True):
        self.calls.append(dict(op="glm", family=family, mode=mode, y=y, offset=offset, trials=trials, obs_const=obs_const,
                               draw_scale=draw_scale, draw_const=draw_const, n_draws=np.asarray(beta).shape[0],
                               rows=None if rows is None else np.asarray(rows).copy()))
        X = np.asarray(X)
        sel = slice(None) if rows is None else np.asarray(rows)
        pick = lambda v: None if v is None else np.asarray(v)[sel]  # noqa: E731
        eta = glm_ref.linpred(X[sel], beta, pick(offset))
        if family == "linpred":
            ll = eta
        elif family in fref.ENGINE_FAMILIES:
            ll = fref.density(family, eta, pick(y), scale=draw_scale, trials=pick(trials), oc=pick(obs_const), dc=draw_const)
        else:
            ll = glm_ref.density(family, eta, pick(y), sigma=draw_scale, trials=pick(trials), oc=pick(obs_const), dc=draw_const)
        if mode == "matrix":
            return ll
        bad = np.isnan(ll)
        res = self.psis_loo(np.where(bad, -1e10, ll), tail_count, method, scale_value, good_k)
        res["n_replaced"] = int(bad.sum())
        return res

    def glm_marginal(self, *args, **kwargs):
        self.calls.append(dict(op="glm_marginal"))
        raise AssertionError("the marginal pass must not be reached")


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


@pytest.fixture(scope="module")
def models():
    rng = np.random.default_rng(11)
    return {f: fref.make_model(rng, 14, 400, 5, f, with_offset=True) for f in fref.ENGINE_FAMILIES}


def test_every_rejection_comes_before_any_engine_call(fake, models):
    import pyloo_amd as pl

    nb, ga, pr = models["negbinomial"], models["gamma"], models["binomial_probit"]
    gauss = glm_ref.make_model(np.random.default_rng(12), 14, 400, 5, "gaussian")
    pois = glm_ref.make_model(np.random.default_rng(13), 14, 400, 5, "poisson")
    at9 = np.arange(400) == 9

    def call(model, **changes):
        a, k = fref.front_call(model)
        k.update(changes)
        y = k.pop("y", a[1])
        family = k.pop("family", a[3])
        return (a[0], y, a[2], family), k

    old = lambda m, **k: ((m["X"], m["y"], m["beta"], m["family"]), dict(sigma=m["sigma"], **k))  # noqa: E731
    frac, neg, zero = nb["y"].copy(), nb["y"].copy(), ga["y"].copy()
    frac[2], neg[4], zero[3] = 1.5, -1.0, 0.0
    cases = [
        (call(nb, phi=None), "the negbinomial family needs phi, one value per draw"),
        (call(nb, phi=nb["scale"][:-1]), "phi needs 400 values, one per draw, got 399"),
        (call(nb, phi=np.where(at9, 0.0, nb["scale"])), "phi must be finite and positive"),
        (call(nb, phi=np.where(at9, np.inf, nb["scale"])), "phi must be finite and positive"),
        (call(nb, phi=np.where(at9, np.nan, nb["scale"])), "phi must be finite and positive"),
        (call(ga, shape=None), "the gamma family needs shape, one value per draw"),
        (call(ga, shape=ga["scale"][:3]), "shape needs 400 values, one per draw, got 3"),
        (call(ga, shape=np.where(at9, -1.0, ga["scale"])), "shape must be finite and positive"),
        (call(ga, phi=ga["scale"]), "phi belongs to the negbinomial family, not to 'gamma'"),
        (call(nb, shape=nb["scale"]), "shape belongs to the gamma family, not to 'negbinomial'"),
        (old(pois, phi=nb["scale"]), "phi belongs to the negbinomial family, not to 'poisson'"),
        (old(gauss, shape=ga["scale"]), "shape belongs to the gamma family, not to 'gaussian'"),
        (call(nb, sigma=gauss["sigma"]), "sigma belongs to the gaussian family, not to 'negbinomial'"),
        (call(ga, sigma=gauss["sigma"]), "sigma belongs to the gaussian family, not to 'gamma'"),
        (call(nb, trials=pr["trials"]), "trials belongs to the binomial family, not to 'negbinomial'"),
        (call(ga, trials=pr["trials"]), "trials belongs to the binomial family, not to 'gamma'"),
        (call(ga, y=zero), "y of the gamma family must be finite and positive"),
        (call(ga, y=-ga["y"]), "y of the gamma family must be finite and positive"),
        (call(ga, y=np.where(np.arange(14) == 1, np.inf, ga["y"])), "y of the gamma family must be finite and positive"),
        (call(nb, y=frac), "y of the negbinomial family must be non-negative integers"),
        (call(nb, y=neg), "y of the negbinomial family must be non-negative integers"),
        (call(pr, trials=None), "needs trials"),
        (call(pr, y=pr["trials"] + 1.0), "y exceeds trials"),
        (call(pr, link="cloglog"), "link of the binomial family must be None, 'logit' or 'probit', got 'cloglog'"),
        (call(pr, link="log"), "link of the binomial family must be None, 'logit' or 'probit', got 'log'"),
        (call(nb, link="probit"), "link of the negbinomial family must be None, 'log', got 'probit'"),
        (call(ga, link="identity"), "link of the gamma family must be None, 'log', got 'identity'"),
        (old(gauss, link="probit"), "link of the gaussian family must be None, 'identity', got 'probit'"),
        (old(pois, link="logit"), "link of the poisson family must be None, 'log', got 'logit'"),
    ]
    texts = set()
    for (a, k), text in cases:
        for fn in (pl.loo_glm_from_design, pl.glm_log_lik, pl.glm_plpd, pl.loo_subsample_glm):
            with pytest.raises(ValueError) as err:
                fn(*a, **k)
            assert text in str(err.value), (fn.__name__, text, str(err.value))
        texts.add(text)
    assert len(texts) >= 22  # (each with its own text)
    with pytest.raises(ValueError, match="family must be one of"):  # the link is a keyword, not a family name
        pl.loo_glm_from_design(nb["X"], nb["y"], nb["beta"], "probit")
    with pytest.raises(TypeError):  # keyword-only: no existing positional call changes meaning
        pl.glm_log_lik(nb["X"], nb["y"], nb["beta"], "negbinomial", None, None, None, None, False, None, nb["scale"])
    assert fake.calls == []


def test_the_constants_handed_over_are_the_restatements(fake, models):
    import pyloo_amd as pl

    for f in fref.ENGINE_FAMILIES:
        m = models[f]
        a, k = fref.front_call(m)
        fake.calls.clear()
        ll = pl.glm_log_lik(*a, **k)
        c = fake.calls[0]
        assert c["family"] == f and c["mode"] == "matrix" and c["rows"] is None
        assert np.array_equal(c["obs_const"], fref.obs_const(f, m["y"], m["trials"])), f
        if m["scale"] is None:
            assert c["draw_scale"] is None and c["draw_const"] is None and np.array_equal(c["trials"], m["trials"])
        else:
            assert np.array_equal(c["draw_scale"], m["scale"]) and np.array_equal(c["draw_const"], fref.draw_const(m["scale"])), f
            assert c["trials"] is None
        assert np.array_equal(ll, fref.matrix_of(m)) and np.all(np.isfinite(ll)), f
        rows = [9, 2, 2, 13, 0]
        assert np.array_equal(pl.glm_log_lik(*a, **k, rows=rows), fref.matrix_of(m)[rows]) and fake.calls[-1]["rows"].tolist() == rows
        fake.calls.clear()
        eta = pl.glm_log_lik(*a, **k, linpred=True)
        assert fake.calls[0]["family"] == "linpred" and fake.calls[0]["y"] is None and fake.calls[0]["draw_scale"] is None
        assert np.array_equal(eta, glm_ref.linpred(m["X"], m["beta"], m["offset"]))
    # the Bernoulli probit: no trials, no constant
    m = dict(models["binomial_probit"])
    m["y"] = (m["y"] > 0).astype(np.float64)
    fake.calls.clear()
    ll = pl.glm_log_lik(m["X"], m["y"], m["beta"], "bernoulli", offset=m["offset"], link="probit")
    c = fake.calls[0]
    assert c["family"] == "binomial_probit" and c["trials"] is None and c["obs_const"] is None
    assert np.array_equal(ll, fref.density("binomial_probit", glm_ref.linpred(m["X"], m["beta"], m["offset"]), m["y"]))
    # the canonical link by name is the path of link=None
    for name, model in (("logit", m), ("log", models["negbinomial"])):
        a, k = fref.front_call(model) if name == "log" else ((m["X"], m["y"], m["beta"], "bernoulli"), dict(offset=m["offset"]))
        k.pop("link", None)
        fake.calls.clear()
        assert np.array_equal(pl.glm_log_lik(*a, **k, link=name), pl.glm_log_lik(*a, **k))
        assert fake.calls[0]["family"] == fake.calls[1]["family"] == ("binomial" if name == "logit" else "negbinomial")


def test_plpd_uses_the_mean_of_phi_and_shape(fake, models):
    import pyloo_amd as pl

    for f in fref.ENGINE_FAMILIES:
        m = models[f]
        a, k = fref.front_call(m)
        fake.calls.clear()
        got, msgs = quiet(pl.glm_plpd, *a, **k)
        c = fake.calls[0]
        assert not msgs and len(fake.calls) == 1 and c["n_draws"] == 1 and c["mode"] == "matrix"
        mean = dict(m, beta=m["beta"].mean(0).reshape(1, -1), scale=None if m["scale"] is None else m["scale"].mean().reshape(1))
        if m["scale"] is not None:  # the constant of the draw is evaluated again at the mean, not averaged
            assert np.array_equal(c["draw_scale"], mean["scale"]) and np.array_equal(c["draw_const"], fref.draw_const(mean["scale"]))
            assert c["draw_const"][0] != fref.draw_const(m["scale"]).mean()
        assert got.shape == (14,) and np.array_equal(got, fref.matrix_of(mean)[:, 0]), f


@pytest.mark.parametrize("family", fref.ENGINE_FAMILIES)
def test_elpd_data_equals_loo_from_matrix_on_the_restatements_matrix(fake, models, family):
    import pyloo_amd as pl

    m = models[family]
    a, k = fref.front_call(m)
    ll = fref.matrix_of(m)
    for kwargs in (dict(), dict(pointwise=True, reff=0.7), dict(method="sis", pointwise=True)):
        fake.calls.clear()
        got, msgs = quiet(pl.loo_glm_from_design, *a, **k, **kwargs)
        want, want_msgs = quiet(pl.loo_from_matrix, ll, **kwargs)
        assert len(fake.calls) == 1 and fake.calls[0]["mode"] == "loo" and fake.calls[0]["family"] == family
        assert list(got.index) == list(want.index) and msgs == want_msgs
        for key in want.index:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), (kwargs, key)


def test_subsample_takes_the_new_families(fake, models):
    import pyloo_amd as pl

    m = fref.make_model(np.random.default_rng(21), 60, 300, 4, "negbinomial")
    a, k = fref.front_call(m)
    ll = fref.matrix_of(m)
    np.random.seed(5)
    (got, idx, est), msgs = quiet(pl.loo_subsample_glm, *a, **k, observations=12, loo_approximation="lpd", loo_approximation_draws=64)
    np.random.seed(5)
    (want, widx, west), wmsgs = quiet(pl.loo_subsample_from_matrix, ll, observations=12, loo_approximation="lpd", loo_approximation_draws=64)
    assert np.array_equal(idx.idx, widx.idx) and msgs == wmsgs
    np.testing.assert_allclose(got["elpd_loo"], want["elpd_loo"], rtol=1e-12)
    thinned = [c for c in fake.calls if c["n_draws"] == 64][0]  # phi and its constant are thinned with the draws
    cols = np.linspace(0, 299, 64, dtype=int)
    assert np.array_equal(thinned["draw_scale"], m["scale"][cols]) and np.array_equal(thinned["draw_const"], fref.draw_const(m["scale"])[cols])
    fake.calls.clear()
    quiet(pl.loo_subsample_glm, *a, **k, observations=12, loo_approximation="plpd")
    assert fake.calls[0]["n_draws"] == 1 and np.array_equal(fake.calls[0]["draw_scale"], m["scale"].mean().reshape(1))


def test_loo_glm_picks_phi_and_shape_from_the_posterior(fake, models):
    import pyloo_amd as pl

    for f, name_kw in (("negbinomial", "phi_name"), ("gamma", "shape_name")):
        m = models[f]
        beta = m["beta"]
        post = {"b": beta.reshape(4, 100, 5), "aux": m["scale"].reshape(4, 100), "wide": beta[:, :2].reshape(4, 100, 2)}
        got, _ = quiet(pl.loo_glm, {"posterior": post}, m["X"], m["y"], f, ["b"], offset=m["offset"], pointwise=True, **{name_kw: "aux"})
        a, k = fref.front_call(m)
        want, _ = quiet(pl.loo_glm_from_design, *a, **k, pointwise=True)
        assert np.array_equal(got["loo_i"], want["loo_i"]) and got["elpd_loo"] == want["elpd_loo"]
        with pytest.raises(ValueError, match=f"{name_kw} must name a scalar variable, 'wide' has 2 entries per draw"):
            pl.loo_glm({"posterior": post}, m["X"], m["y"], f, ["b"], **{name_kw: "wide"})
        with pytest.raises(ValueError, match="needs"):  # the family's parameter is not guessed
            pl.loo_glm({"posterior": post}, m["X"], m["y"], f, ["b"])
    m = models["binomial_probit"]
    post = {"b": m["beta"].reshape(4, 100, 5)}
    got, _ = quiet(pl.loo_glm, {"posterior": post}, m["X"], m["y"], "binomial", ["b"], offset=m["offset"], trials=m["trials"], link="probit")
    a, k = fref.front_call(m)
    assert got["elpd_loo"] == quiet(pl.loo_glm_from_design, *a, **k)[0]["elpd_loo"]
    logit, _ = quiet(pl.loo_glm, {"posterior": post}, m["X"], m["y"], "binomial", ["b"], offset=m["offset"], trials=m["trials"])
    assert logit["elpd_loo"] != got["elpd_loo"]


def test_the_marginal_fronts_reject_the_new_families_and_the_probit_link(fake, models):
    import pyloo_amd as pl

    monkey = importlib.import_module("pyloo_amd.loo_glm_marginal")
    assert monkey._engine_of is importlib.import_module("pyloo_amd.loo_glm")._engine_of
    cluster = np.arange(14) % 3
    tau = np.ones(400)
    takes = "takes the families gaussian, bernoulli, binomial, poisson with their canonical links"
    for f, what in (("negbinomial", "not the negbinomial family"), ("gamma", "not the gamma family"), ("binomial_probit", "not the probit link")):
        a, k = fref.front_call(models[f])
        k.pop("phi", None), k.pop("shape", None)
        for fn in (pl.glm_marginal_log_lik, pl.loo_glm_marginal_from_design):
            with pytest.raises(ValueError) as err:
                fn(*a, cluster, tau, **k)
            assert takes in str(err.value) and what in str(err.value), str(err.value)
    m = models["negbinomial"]
    post = {"b": m["beta"].reshape(4, 100, 5), "tau": tau.reshape(4, 100)}
    with pytest.raises(ValueError, match="not the negbinomial family"):
        pl.loo_glm_marginal({"posterior": post}, m["X"], m["y"], "negbinomial", ["b"], cluster, None, "tau")
    assert fake.calls == []


# ------------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (as tests/test_capi_abi.py: a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


def test_codes_in_header_binding_and_build(lib):
    from pyloo_amd import _capi
    from pyloo_amd import build as b

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, code in (("PLA_GLM_NEGBINOMIAL_LOG", 4), ("PLA_GLM_GAMMA_LOG", 5), ("PLA_GLM_BINOMIAL_PROBIT", 6)):
        assert getattr(_capi, name) == code and f"#define {name} {code}\n" in header and name in guide, name
    assert lib.pla_abi_version() == 7 and _capi.ABI_VERSION == 7 and C.sizeof(_capi.GlmArgs) == 256  # (no new field, no new entry)
    assert "pla_k_glm_families.hip" in b.SOURCES and "pla_k_glm_terms_families.hip" in b.SOURCES


def test_argument_errors_of_the_new_codes(lib):
    from pyloo_amd import _capi

    buf = (C.c_double * 64)(*([1.0] * 64))
    out = (C.c_double * 64)()
    p = C.addressof(buf)

    def args(family, **more):
        return _capi.GlmArgs(engine=1,  # (never followed: nothing below gets past the argument checks)
                             family=family, mode=_capi.PLA_GLM_MODE_MATRIX, mem_space=_capi.PLA_HOST, n_obs=2, n_pred=3, n_draws=16, x=p,
                             x_stride_obs=3, x_stride_pred=1, beta=p, beta_stride_draw=3, beta_stride_pred=1, y=p, out=C.addressof(out),
                             out_pitch=16, **more)

    seen = set()
    for family, name in ((_capi.PLA_GLM_NEGBINOMIAL_LOG, b"PLA_GLM_NEGBINOMIAL_LOG"), (_capi.PLA_GLM_GAMMA_LOG, b"PLA_GLM_GAMMA_LOG")):
        for more, word in ((dict(), b"needs draw_scale"), (dict(draw_const=p), b"needs draw_scale"), (dict(draw_scale=p), b"needs draw_const")):
            assert lib.pla_glm(C.byref(args(family, **more))) == -1
            msg = lib.pla_last_error()
            assert name in msg and word in msg, msg
            seen.add(msg)
        grouped = _capi.GlmGroupedArgs(n_terms=0)
        grouped.glm = args(family, draw_scale=p)
        assert lib.pla_glm_grouped(C.byref(grouped)) == -1 and name + b" needs draw_const" in lib.pla_last_error()
    assert len(seen) == 4  # (each family and each vector with its own message)
    a7 = args(7, draw_scale=p, draw_const=p)
    assert lib.pla_glm(C.byref(a7)) == -1 and b"bad family 7" in lib.pla_last_error()
    # the cluster-marginal pass does not take them
    offsets, members = (C.c_int64 * 3)(0, 1, 2), (C.c_int64 * 2)(0, 1)
    for family, name in ((4, b"PLA_GLM_NEGBINOMIAL_LOG"), (5, b"PLA_GLM_GAMMA_LOG"), (6, b"PLA_GLM_BINOMIAL_PROBIT")):
        marg = _capi.GlmMarginalArgs(n_clusters=2, n_members=2, cluster_offsets=C.addressof(offsets), members=C.addressof(members), tau=p,
                                     n_nodes=3, nodes=p, log_weights=p)
        marg.grouped.glm = args(family, draw_scale=p, draw_const=p)
        assert lib.pla_glm_marginal(C.byref(marg)) == -1  # PLA_ERR_ARG
        msg = lib.pla_last_error()
        assert b"pla_glm_marginal takes PLA_GLM_GAUSSIAN, PLA_GLM_BINOMIAL_LOGIT and PLA_GLM_POISSON_LOG, not " + name in msg, msg


# ------------------------------------------------------------------------------------------------------------- the generated code
# registers (vector + accumulation) of glm_kernel / glm_terms_kernel per (family code, chunks, panel), measured with
# tools/isa_stats.py: the budget is the next multiple of 8 of the 512-register file divided by the waves
WAVES = {
    "pla_k_glm_families.hip": {(4, 1, 0): 4, (4, 2, 0): 3, (4, 4, 0): 3, (4, 8, 0): 2, (4, 8, 1): 3,
                               (5, 1, 0): 5, (5, 2, 0): 4, (5, 4, 0): 4, (5, 8, 0): 3, (5, 8, 1): 3,
                               (6, 1, 0): 4, (6, 2, 0): 3, (6, 4, 0): 3, (6, 8, 0): 2, (6, 8, 1): 3},
    "pla_k_glm_terms_families.hip": {(4, 1, 0): 3, (4, 2, 0): 3, (4, 4, 0): 2, (4, 8, 0): 2, (4, 8, 1): 3,
                                     (5, 1, 0): 4, (5, 2, 0): 4, (5, 4, 0): 3, (5, 8, 0): 2, (5, 8, 1): 3,
                                     (6, 1, 0): 3, (6, 2, 0): 3, (6, 4, 0): 2, (6, 8, 0): 2, (6, 8, 1): 3},
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
@pytest.mark.parametrize("unit", sorted(WAVES))
def test_new_units_use_no_scratch_and_keep_the_measured_occupancy(tmp_path, unit):
    """three families x (1, 2, 4, 8 chunks in registers + panels of 8) kernels per unit and nothing else (the
    prepare kernels stay in the units that had them); no scratch, no LDS and no scalar register in a vector lane; one MFMA chain of
    four steps per chunk; the waves per SIMD the section's table states."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    lines = isa_stats.compile_isa(out=str(tmp_path / "glm.s"), units=[unit])
    names = isa_stats.all_kernels(lines)
    assert len(names) == 15 and all("glm_" in k and "prepare" not in k for k in names), names
    seen = set()
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert not isa_stats.masked_spills(lines, k[2:]) and total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert res.get("LDSByteSize", 0) == 0, (name, res)
        fam, nch, panel = map(int, re.search(r"Li(\d)ELi(\d)ELb([01])E", k).groups())
        seen.add((fam, nch, panel))
        start = next(i for i, l in enumerate(lines) if l.startswith(k + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[i]))
        mfma = sum(l.strip().startswith("v_mfma_f64_16x16x4_f64") for l in lines[start:end])
        assert mfma == 4 * nch, (name, mfma)  # one chain: four steps per chunk, the tile loop not duplicated
        waves = WAVES[unit][(fam, nch, panel)]
        regs = res["NumVgprs"] + res.get("NumAgprs", 0)
        assert regs <= 512 // waves // 8 * 8 and res.get("Occupancy", 0) >= waves, (name, res, waves)
    assert seen == set(WAVES[unit])
