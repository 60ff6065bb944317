"""GPU tests of ``loo_glm_predict`` (csrc/pla_glm_predict.h): the generator's bits of eta, the per-element functions against the NumPy
restatement and scipy, the weighted sums against long double, the same bits under every re-arrangement, the fused pass end to end,
the count cap, and the gamma family's moments."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import glm_predict_ref as ref
import glm_ref
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = ref.SEG
# the engine's family -> the front's family, link and the name of its per-draw scale
FRONT = {"gaussian": ("gaussian", None, "sigma"), "binomial": ("binomial", None, None), "poisson": ("poisson", None, None),
         "negbinomial": ("negbinomial", None, "phi"), "gamma": ("gamma", None, "shape"), "binomial_probit": ("binomial", "probit", None)}


@pytest.fixture(scope="module")
def pl():
    import pyloo_amd

    return pyloo_amd


def cuda(a):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def front_args(fam, X, y, beta, scale=None, trials=None, offset=None, put=lambda a: a):
    family, link, scale_name = FRONT[fam]
    if family == "binomial" and trials is None:
        family = "bernoulli"
    kw = dict(offset=put(offset), trials=put(trials), link=link)
    if scale_name is not None:
        kw[scale_name] = put(scale)
    return (put(X), put(y), put(beta), family), kw


def predict(pl, fam, X, y, beta, scale=None, trials=None, offset=None, put=lambda a: a, **more):
    args, kw = front_args(fam, X, y, beta, scale, trials, offset, put)
    if more.get("log_weights") is not None:
        more["log_weights"] = put(more["log_weights"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return pl.loo_glm_predict_from_design(*args, **kw, **more)


def linpred(pl, fam, X, y, beta, scale=None, trials=None, offset=None):
    args, kw = front_args(fam, X, y, beta, scale, trials, offset)
    return pl.glm_log_lik(*args, linpred=True, **kw)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------ 1. the bits of eta
@pytest.mark.parametrize("p", [1, 5, 17, 64, 129])
def test_one_hot_gaussian_mean_is_the_generators_eta_bit_for_bit(pl, p):
    """log_weights one-hot on draw s0: sum e = 1 and every other term is an exact zero, so the Gaussian mean is eta[:, s0] as
    ``glm_log_lik(linpred=True)`` writes it, bit for bit -- for every chunk count and the panel route, s0 in the first and the
    last tile."""
    rng = np.random.default_rng(p)
    for n in (1, 15, 16, 17, 33):
        for s in (2, 16, 17, 250):
            X, beta = rng.normal(size=(n, p)), rng.normal(size=(s, p))
            y, offset, sigma = rng.normal(size=n), rng.normal(size=n), np.exp(0.1 * rng.normal(size=s))
            eta = linpred(pl, "gaussian", X, y, beta, sigma, offset=offset)
            for s0 in sorted({0, min(3, s - 1), s - 1}):
                res = predict(pl, "gaussian", X, y, beta, sigma, offset=offset, log_weights=ref.one_hot(n, s, s0))
                assert same_bits(res.mean, eta[:, s0]), (n, s, p, s0)
                assert res.n_pit_skipped == 0 and res.pareto_k is None and res.elpd_i is None


# -------------------------------------------------------------------------------------------------------- 2. the per-element functions
ETAS = np.array([-8.0, -3.3, -0.7, 0.0, 0.4, 2.1, 6.9, 8.0])
COUNTS = (0.0, 1.0, 2.0, 17.0, 1000.0)
TRIALS = (1.0, 7.0, 1000.0)


def element_grid(fam):
    """Rows: every (y, trials, eta) of the grid -- X holds eta, beta is ones, so eta[i, s] = eta_i for every draw."""
    if fam in ("binomial", "binomial_probit"):
        pairs = [(y, n) for n in TRIALS for y in COUNTS if y <= n]
    elif fam in ("gaussian", "gamma"):
        pairs = [(y, 1.0) for y in (0.3, 1.0, 2.5, 17.0, 1000.0)] if fam == "gamma" else [(y, 1.0) for y in (-9.0, -0.2, 0.0, 1.5, 11.0)]
    else:
        pairs = [(y, 1.0) for y in COUNTS]
    y = np.array([yy for yy, _ in pairs for _ in ETAS])
    trials = np.array([nn for _, nn in pairs for _ in ETAS])
    X = np.tile(ETAS, len(pairs))[:, None]
    return X, y, (trials if fam in ("binomial", "binomial_probit") else None)


@pytest.mark.parametrize("fam", ["gaussian", "binomial", "binomial_probit", "poisson", "negbinomial"])
def test_per_element_functions_match_the_restatement_and_scipy(pl, fam):
    X, y, trials = element_grid(fam)
    S, s0 = 17, 16
    beta = np.ones((S, 1))
    scale = np.linspace(0.7, 2.3, S) if FRONT[fam][2] else None
    eta = linpred(pl, fam, X, y, beta, scale, trials)
    assert np.array_equal(eta[:, s0], X[:, 0])
    res = predict(pl, fam, X, y, beta, scale, trials, log_weights=ref.one_hot(len(y), S, s0))
    assert res.n_pit_skipped == 0
    mu, second, f_le, f_lt = (a[:, s0] for a in ref.point(fam, eta, y, scale, trials))
    m2 = res.var + res.mean * res.mean
    for name, got, want in (("mean", res.mean, mu), ("pit_le", res.pit_le, f_le), ("pit_lt", res.pit_lt, f_lt)):
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print(fam, name, "against the restatement:", err.max())
        assert err.max() <= 1e-10, (fam, name, err.max())
    err = np.abs(m2 - second) / np.maximum(1.0, np.abs(second))  # (var = m2 - mean^2 was formed and undone in f64: 4 u of m2 more)
    print(fam, "m2 against the restatement:", err.max())
    assert err.max() <= 1e-10
    s_le, s_lt = (a[:, s0] for a in ref.scipy_cdf(fam, eta, y, scale, trials))
    for name, got, want in (("pit_le", res.pit_le, s_le), ("pit_lt", res.pit_lt, s_lt)):
        print(fam, name, "against scipy:", np.abs(got - want).max())
        assert np.abs(got - want).max() <= 1e-10, (fam, name)
    if fam == "gaussian":
        assert same_bits(res.pit_le, res.pit_lt)


def test_m2_itself_matches_the_restatement(pl):
    """The raw second moment as the engine returns it (the front only reports the variance)."""
    from pyloo_amd.engine import get_engine

    for fam in ("poisson", "negbinomial", "gamma"):
        X, y, trials = element_grid(fam)
        S, s0 = 17, 16
        beta, scale = np.ones((S, 1)), (np.linspace(0.7, 2.3, S) if FRONT[fam][2] else None)
        oc, dc = ref.constants(fam, y, trials, scale)
        out = get_engine(None).glm_predict(X, beta, fam, y=y, obs_const=oc, draw_scale=scale, draw_const=dc,
                                           log_weights=ref.one_hot(len(y), S, s0))
        _, second, _, _ = ref.point(fam, X @ beta.T, y, scale, trials)
        assert np.all(np.abs(out["m2"] - second[:, s0]) <= 1e-10 * np.maximum(1.0, np.abs(second[:, s0])))


def test_bernoulli_ends_are_exact(pl):
    X = np.tile(ETAS, 2)[:, None]
    y = np.repeat([0.0, 1.0], len(ETAS))
    for link in ("binomial", "binomial_probit"):
        res = predict(pl, link, X, y, np.ones((16, 1)), log_weights=ref.one_hot(len(y), 16, 5))
        assert np.all(res.pit_lt[y == 0.0] == 0.0) and np.all(res.pit_le[y == 1.0] == 1.0)


def test_poisson_rescue_cases_are_exactly_zero_or_one(pl):
    X = np.array([[40.0], [40.0], [-40.0], [-40.0]])
    y = np.array([0.0, 1000.0, 0.0, 1000.0])
    res = predict(pl, "poisson", X, y, np.ones((16, 1)), log_weights=ref.one_hot(4, 16, 0))
    assert np.array_equal(res.pit_le, [0.0, 0.0, 1.0, 1.0]) and np.array_equal(res.pit_lt, [0.0, 0.0, 0.0, 1.0])
    assert res.n_pit_skipped == 0 and np.all(np.isfinite(res.mean))


# ------------------------------------------------------------------------------------------------------------------ 3. the weighted sums
@pytest.mark.parametrize("s", [15, 16 * SEG - 1, 16 * SEG, 16 * SEG + 1, 4100])
def test_weighted_sums_match_long_double(pl, s):
    """Random weights shifted by +700 and -700 per row, some of log -inf; a row of -inf alone gives NaN."""
    n, p = 17, 5
    for fam in ("gaussian", "poisson"):
        m = glm_ref.make_model(np.random.default_rng(s), n, s, p, fam, with_offset=True)
        rng = np.random.default_rng(s + 1)
        lw = 3.0 * rng.normal(size=(n, s)) + np.where(np.arange(n) % 2 == 0, 700.0, -700.0)[:, None]
        lw[rng.uniform(size=(n, s)) < 0.1] = -np.inf
        lw[11] = -np.inf
        res = predict(pl, fam, m["X"], m["y"], m["beta"], m["sigma"], offset=m["offset"], log_weights=lw)
        eta = linpred(pl, fam, m["X"], m["y"], m["beta"], m["sigma"], offset=m["offset"])
        mu, _, f_le, f_lt = ref.point(fam, eta, m["y"], m["sigma"])
        want = ref.weighted(lw, [mu, f_le, f_lt])
        assert res.n_pit_skipped == 0
        ok = np.arange(n) != 11
        for name, got, w in zip(("mean", "pit_le", "pit_lt"), (res.mean, res.pit_le, res.pit_lt), want):
            assert np.isnan(got[11]), name
            zero = w[ok] == 0.0  # (P(Y < 0) under every draw: an exact zero on both sides, relative error 0)
            assert np.all(got[ok][zero] == 0.0), name
            err = np.abs(got[ok][~zero] - w[ok][~zero]) / np.abs(w[ok][~zero])
            print(fam, s, name, err.max())
            assert err.max() <= 1e-12, (fam, s, name, err.max())


# ------------------------------------------------------------------------------------------------------- 4. the same bits, re-arranged
FIELDS = ("mean", "var", "pit_le", "pit_lt")


def rearrangement_model():
    m = glm_ref.make_model(np.random.default_rng(5), 33, 300, 5, "poisson", with_offset=True)
    lw = 2.0 * np.random.default_rng(6).normal(size=(33, 300))
    return m, lw


def test_same_bits_for_permuted_rows_row_lists_single_rows_and_memory_spaces(pl):
    m, lw = rearrangement_model()
    call = lambda idx, **kw: predict(pl, "poisson", m["X"][idx], m["y"][idx], m["beta"], offset=m["offset"][idx], log_weights=lw[idx], **kw)  # noqa: E731
    base = call(np.arange(33))
    perm = np.random.default_rng(7).permutation(33)
    got = call(perm)
    for f in FIELDS:
        assert same_bits(getattr(got, f), getattr(base, f)[perm]), f
    rows = np.array([31, 2, 2, 17, 0, 32, 2])
    listed = predict(pl, "poisson", m["X"], m["y"], m["beta"], offset=m["offset"], log_weights=lw[rows], rows=rows)
    alone = call(np.array([17]))
    dev = call(np.arange(33), put=cuda)
    for f in FIELDS:
        assert same_bits(getattr(listed, f), getattr(base, f)[rows]), f
        assert same_bits(getattr(alone, f), getattr(base, f)[[17]]), f
        assert same_bits(getattr(dev, f), getattr(base, f)), f
    assert np.array_equal(listed.resid, m["y"][rows] - listed.mean)


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import glm_ref
import pyloo_amd as pl
from pyloo_amd.engine import get_engine
m = glm_ref.make_model(np.random.default_rng(11), 300, 1000, 5, "poisson", with_offset=True)
out = {}
for where, put in (("host", lambda a: a), ("device", lambda a: torch.as_tensor(a, device="cuda"))):
    r = pl.loo_glm_predict_from_design(put(m["X"]), put(m["y"]), put(m["beta"]), "poisson", offset=put(m["offset"]))
    for f in ("mean", "var", "pit_le", "pit_lt", "pareto_k", "elpd_i"):
        out[where + "_" + f] = getattr(r, f)
    out[where + "_route"] = np.array(get_engine(0 if where == "device" else None).last_kernels())
np.savez(sys.argv[2], **out)
"""


def test_same_bits_with_one_megabyte_blocks(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 cuts the 300 x 1000 fused pass into blocks of 131 rows: every output is the one-block run's, bit for
    bit, host and device."""
    runs = []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        env.update(env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            runs.append({k: z[k] for k in z.files})
    assert "glm_predict_kernel" in str(runs[0]["device_route"]) and "per block of observations" in str(runs[1]["device_route"])
    for k in runs[0]:
        if not k.endswith("route"):
            assert same_bits(runs[0][k], runs[1][k]), k
            assert same_bits(runs[0][k], runs[0]["host_" + k.split("_", 1)[1]]), k


# ------------------------------------------------------------------------------------------------------------------- 5. end to end
E2E = {}


def e2e_model(n, s, family):
    key = (n, s, family)
    if key not in E2E:
        m = glm_ref.make_model(np.random.default_rng(n * 7 + 5), n, s, 5, family, with_offset=True)
        E2E[key] = (m, orc.loo_pointwise(glm_ref.matrix_of(m), 1.0, "psis"))
    return E2E[key]


@pytest.mark.parametrize("family", ["gaussian", "binomial", "poisson"])
@pytest.mark.parametrize("n,s", [(37, 1000), (5, 4100)])
def test_fused_pass_end_to_end(pl, family, n, s):
    """PLA_PIT_LOGLIK: k and elpd_i are loo_glm_from_design's and the oracle's to 1e-9; the predictive outputs are those of the
    log_weights kind fed with psislw(-glm_log_lik(...)) to 1e-12 (the weights come from the same weights pass, yet through another
    entry point: their bits are not asserted equal); the Gaussian mean is e_loo's on the materialised eta to 1e-10."""
    m, oracle = e2e_model(n, s, family)
    args, kw = front_args(family, m["X"], m["y"], m["beta"], m["sigma"], m["trials"], m["offset"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = pl.loo_glm_predict_from_design(*args, **kw)
        loo = pl.loo_glm_from_design(*args, **{k: v for k, v in kw.items()}, pointwise=True)
    assert res.n_pit_skipped == 0
    np.testing.assert_allclose(res.pareto_k, np.asarray(loo["pareto_k"]).reshape(-1), rtol=0, atol=1e-9)
    np.testing.assert_allclose(res.elpd_i, np.asarray(loo["loo_i"]).reshape(-1), rtol=0, atol=1e-9)
    np.testing.assert_allclose(res.pareto_k, oracle["diag"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(res.elpd_i, oracle["loo_i"], rtol=0, atol=1e-9)
    ll = pl.glm_log_lik(*args, **kw)
    lw = pl.psislw(-ll)[0]
    lw = np.asarray(getattr(lw, "values", lw), dtype=np.float64).reshape(n, s)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        given = pl.loo_glm_predict_from_design(*args, **kw, log_weights=lw)
    for f in FIELDS:
        a, b = getattr(res, f), getattr(given, f)
        print(family, n, s, f, "bitwise" if same_bits(a, b) else np.abs(a - b).max())
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)
    if family == "gaussian":
        eta = pl.glm_log_lik(*args, linpred=True, **kw)
        want = np.asarray(pl.e_loo(eta, log_weights=lw, type="mean").value).reshape(-1)
        np.testing.assert_allclose(res.mean, want, rtol=0, atol=1e-10)
    yv = m["y"]
    assert np.array_equal(res.resid, yv - res.mean) and res.rmse == float(np.sqrt(np.mean(res.resid ** 2)))
    assert res.r2 == float(1.0 - np.var(res.resid) / np.var(yv)) and res.good_k == min(1 - 1 / np.log10(s), 0.7)


# -------------------------------------------------------------------------------------------------------------------- 6. the cap
def test_count_above_the_cap_has_no_pit_and_leaves_the_other_rows_alone(pl):
    m = glm_ref.make_model(np.random.default_rng(3), 16, 250, 5, "poisson")
    lw = np.random.default_rng(4).normal(size=(16, 250))
    y = m["y"].copy()
    y[9] = 4097.0
    res = predict(pl, "poisson", m["X"], y, m["beta"], log_weights=lw)
    assert res.n_pit_skipped == 1 and np.isnan(res.pit_le[9]) and np.isnan(res.pit_lt[9]) and np.isfinite(res.mean[9])
    keep = np.arange(16) != 9
    rest = predict(pl, "poisson", m["X"][keep], y[keep], m["beta"], log_weights=lw[keep])
    assert rest.n_pit_skipped == 0
    for f in FIELDS:
        assert same_bits(getattr(res, f)[keep], getattr(rest, f)), f
    at = predict(pl, "poisson", m["X"][[9]], np.array([4096.0]), m["beta"], log_weights=lw[[9]])
    assert at.n_pit_skipped == 0 and np.isfinite(at.pit_le[0])


# ------------------------------------------------------------------------------------------------------------------- 7. gamma
def test_gamma_has_moments_and_no_pit(pl):
    import ctypes as C

    from pyloo_amd import _capi
    from pyloo_amd.engine import get_engine

    X, y, _ = element_grid("gamma")
    S, s0 = 17, 16
    beta, shape = np.ones((S, 1)), np.linspace(0.7, 2.3, S)
    res = predict(pl, "gamma", X, y, beta, shape, log_weights=ref.one_hot(len(y), S, s0))
    assert res.pit is None and res.pit_le is None and res.pit_lt is None and res.n_pit_skipped == 0
    mu, second, _, _ = ref.point("gamma", X @ beta.T, y, shape)
    assert np.all(np.abs(res.mean - mu[:, s0]) <= 1e-10 * np.maximum(1.0, np.abs(mu[:, s0])))
    m2 = res.var + res.mean ** 2
    assert np.all(np.abs(m2 - second[:, s0]) <= 1e-10 * np.maximum(1.0, second[:, s0]))
    with pytest.raises(ValueError, match="gamma"):
        predict(pl, "gamma", X, y, beta, shape, randomized=True)
    # at the ABI a PIT request is PLA_ERR_UNSUPPORTED
    eng = get_engine(None)
    lib = _capi.load_library()
    dc = ref.constants("gamma", y, None, shape)[1]
    oc = np.log(y)
    lw = np.ascontiguousarray(ref.one_hot(len(y), S, s0))
    out = np.empty(len(y))
    a = _capi.GlmPredictArgs(kind=_capi.PLA_PIT_LOG_WEIGHTS, lw_stride_obs=S, lw_stride_draw=1)
    a.glm = _capi.GlmArgs(engine=eng._h.value, family=_capi.PLA_GLM_GAMMA_LOG, mem_space=_capi.PLA_HOST, n_obs=len(y), n_pred=1,
                          x_stride_obs=1, x_stride_pred=1, n_draws=S, beta_stride_draw=1, beta_stride_pred=1)
    keep = [np.ascontiguousarray(v, dtype=np.float64) for v in (X, beta, y, oc, shape, dc)]
    a.glm.x, a.glm.beta, a.glm.y, a.glm.obs_const, a.glm.draw_scale, a.glm.draw_const = (v.ctypes.data for v in keep)
    a.log_weights, a.pit_le = lw.ctypes.data, out.ctypes.data
    assert lib.pla_glm_predict(C.byref(a)) == -4  # PLA_ERR_UNSUPPORTED
    assert b"PLA_GLM_GAMMA_LOG" in lib.pla_last_error()
    a.pit_le, a.mean = None, out.ctypes.data
    assert lib.pla_glm_predict(C.byref(a)) == 0
    assert same_bits(out, res.mean)
