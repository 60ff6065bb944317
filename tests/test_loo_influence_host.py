"""Host side of ``loo_influence`` without a GPU.  The yardstick first: the NumPy restatement (tests/influence_ref.py) against
properties that hold whatever the implementation, a model with a closed form, and its sensitivity to the precision the project
holds the log weights to.  Then the feature: the fronts through an oracle-backed stand-in engine (bucket scatter order, ``rows=``,
column names, the arithmetic, every check before the first engine call, both warnings, the table), the C export and the generated
code of the new kernels.

The tests of the first section hold the restatement itself and import nothing of the feature: they pass with or without it.
Every test from the front on fails without the feature (the functions, the symbol and the kernel unit are missing)."""

import ctypes as C
import importlib
import os
import re
import shutil
import sys
import warnings

import numpy as np
import pytest

import influence_ref
import pit_ref
from fake_engine import OracleEngine
from oracle import psis_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."
KEYS = ("shift", "m2", "kl", "ess_w")


def draw_ll(rng, n, s, k_lo=0.05, k_hi=0.9):
    k = rng.uniform(k_lo, k_hi, size=(n, 1))
    return -k * rng.exponential(size=(n, s)) - 1.0 - rng.uniform(size=(n, 1))


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def test_one_hot_weights_pick_that_draw():
    rng = np.random.default_rng(1)
    for s in (5, 64, 257):
        theta = influence_ref.make_theta(rng, s)
        c, sc = influence_ref.center_scale(theta)
        hot = rng.integers(0, s, size=6)
        lw = np.full((6, s), -np.inf)
        lw[np.arange(6), hot] = rng.normal(size=6) * 50.0
        r = influence_ref.from_log_weights(lw, theta, c, sc)
        z = (theta - c) / sc
        assert np.array_equal(r["shift"], z[hot]) and np.array_equal(r["m2"], z[hot] * z[hot])
        assert np.array_equal(r["kl"], np.full(6, np.log(float(s)))) and np.array_equal(r["ess_w"], np.ones(6))


def test_uniform_weights_leave_the_posterior_where_it_is():
    """(Columns of unit order: with the offset column 1e6 + 1e-3 N(0, 1) the rounding of the column mean itself, 1e-10 against a
    scale of 1e-3, shows as a shift of 1e-7 -- the reason kernel and restatement are handed the same center and scale.)"""
    rng = np.random.default_rng(2)
    for s in (8, 100, 4000):
        theta = influence_ref.make_theta(rng, s, p=3)
        c, sc = influence_ref.center_scale(theta)
        r = influence_ref.from_log_weights(np.full((3, s), -7.25), theta, c, sc)
        assert np.abs(r["shift"]).max() <= 1e-12, np.abs(r["shift"]).max()
        np.testing.assert_allclose(r["m2"], (s - 1.0) / s, rtol=0, atol=1e-12)
        assert np.abs(r["kl"]).max() <= 1e-12 and np.array_equal(r["ess_w"], np.full(3, float(s)))


def test_a_shift_of_the_log_weights_changes_nothing():
    rng = np.random.default_rng(3)
    ll = draw_ll(rng, 20, 700)
    theta = influence_ref.make_theta(rng, 700)
    ref = influence_ref.loo_influence(ll, theta, 0.8)
    for off in (37.5, -812.0):
        r = influence_ref.from_log_weights(ref["lw"] + off, theta, ref["center"], ref["scale"])
        for key in KEYS:
            scale = max(1.0, np.abs(ref[key]).max()) if key == "ess_w" else 1.0
            np.testing.assert_allclose(r[key], ref[key], rtol=0, atol=1e-12 * scale, err_msg=key)


def test_rows_of_nan_or_no_weight_give_nan_and_minus_inf_draws_drop_out():
    rng = np.random.default_rng(4)
    theta = influence_ref.make_theta(rng, 60)
    c, sc = influence_ref.center_scale(theta)
    lw = rng.normal(size=(5, 60))
    lw[0, ::2] = -np.inf
    lw[1] = -np.inf
    lw[2] = np.nan
    lw[3, 9] = np.nan
    r = influence_ref.from_log_weights(lw, theta, c, sc)
    for key in KEYS:
        assert np.isnan(r[key]).reshape(5, -1).all(axis=1).tolist() == [False, True, True, True, False], key
    z = (theta - c) / sc
    half = influence_ref.from_log_weights(lw[:1, 1::2], z[1::2], np.zeros(5), np.ones(5))
    np.testing.assert_allclose(r["shift"][0], half["shift"][0], rtol=0, atol=1e-14)
    assert r["ess_w"][0] == half["ess_w"][0] and abs(r["kl"][0] - (half["kl"][0] + np.log(2.0))) <= 1e-13


def test_normal_mean_model_matches_the_closed_form():
    """y_i ~ N(mu, 1) with a flat prior, n = 20, S = 4000 exact posterior draws, y_0 = 3: the LOO posterior mean of mu is the mean
    of the other observations, so shift_i = ((sum y - y_i) / (n - 1) - center) / scale, here within five Monte Carlo standard
    errors sd_loo / sqrt(ess_w) of the weighted mean (observed: the largest ratio over seeds 1-3 is printed)."""
    worst = 0.0
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        n, s = 20, 4000
        y = rng.normal(size=n)
        y[0] = 3.0
        mu = y.mean() + rng.normal(size=s) / np.sqrt(n)
        ll = -0.5 * (y[:, None] - mu[None, :]) ** 2 - 0.5 * np.log(2.0 * np.pi)
        ref = influence_ref.loo_influence(ll, mu, 1.0)
        assert np.all(ref["diag"] < 0.7)
        closed = ((y.sum() - y) / (n - 1) - ref["center"][0]) / ref["scale"][0]
        sd_loo = influence_ref.front_values(ref, mu)["sd_ratio"][:, 0]
        ratio = np.abs(ref["shift"][:, 0] - closed) / (sd_loo / np.sqrt(ref["ess_w"]))
        worst = max(worst, ratio.max())
        assert np.all(ratio <= 5.0), (seed, ratio.max())
        assert ref["shift"][0, 0] < -0.5 and np.all(ref["kl"] >= 0.0)  # (the outlier pulls mu up: leaving it out, down)
    print(f"normal-mean model: largest |shift - closed form| / (sd_loo / sqrt(ess_w)) = {worst:.2f}")


PERTURBED = ("s4000_r1", "edges_s500_r1", "s100_r1")


def test_sensitivity_to_the_precision_of_the_log_weights():
    """The project holds lw to 1e-10.  A perturbation of that size of the reference's own weights (tests/golden/loo_pit.npz) moves
    shift, m2 and kl by less than 1e-10 in standardised units: the derivation of the 1e-8 bound of tests/test_gpu_loo_influence.py."""
    gold = pit_ref.load_golden()
    rng = np.random.default_rng(5)
    worst = 0.0
    for name in PERTURBED:
        lw = gold[name]["lw"].astype(np.float64)
        theta = influence_ref.make_theta(rng, lw.shape[1])
        c, sc = influence_ref.center_scale(theta)
        base = influence_ref.from_log_weights(lw, theta, c, sc)
        for _ in range(3):
            moved = influence_ref.from_log_weights(lw + rng.uniform(-1e-10, 1e-10, size=lw.shape), theta, c, sc)
            for key in ("shift", "m2", "kl"):
                assert np.array_equal(np.isnan(moved[key]), np.isnan(base[key]))
                worst = max(worst, float(np.nanmax(np.abs(moved[key] - base[key]))))
    print(f"a 1e-10 perturbation of lw moves shift / m2 / kl by at most {worst:.2e}")
    assert worst <= 1e-10, worst


# -------------------------------------------------------------------------------------------------------------------- the front
class InfluenceEngine(OracleEngine):
    """The oracle-backed stand-in with the two passes this feature calls; records calls."""

    def __init__(self):
        self.calls = []

    def loo_influence(self, mat, theta, center, scale, tail_count=0, method="psis", kind="loglik", rows=None):
        mat = np.asarray(mat)
        self.calls.append(dict(op="loo_influence", tail_count=tail_count, kind=kind, rows=None if rows is None else np.asarray(rows).copy(),
                               draws_fastest=mat.shape[1] <= 1 or mat.strides[1] == mat.itemsize))
        sub = mat if rows is None else mat[np.asarray(rows)]
        ref = influence_ref.loo_influence(sub, theta, method=method, M=tail_count, center=center, scale=scale)
        return {k: ref[k] for k in KEYS + ("diag", "n_replaced")}

    def relative_eff(self, x, n_chains=1, log=True, split=False, cap=True):
        self.calls.append(dict(op="relative_eff", n_chains=n_chains))
        return {"r_eff": np.linspace(0.3, 1.0, np.asarray(x).shape[0]), "n_invalid": 0}


@pytest.fixture()
def fake(monkeypatch):
    eng = InfluenceEngine()
    for name in ("pyloo_amd.loo", "pyloo_amd.loo_influence", "pyloo_amd.relative_eff", "pyloo_amd.base"):
        monkeypatch.setattr(importlib.import_module(name), "get_engine", lambda device=None: eng)
    return eng


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


R2 = np.array([0.8, 0.25, 0.8, 0.25, 0.25, 0.8, 0.8, 0.25, 0.8, 0.8, 0.25, 0.8])  # two buckets, interleaved


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(8)
    ll = draw_ll(rng, 12, 1000, 0.05, 0.5)
    theta = influence_ref.make_theta(rng, 1000)
    return ll, theta


def test_vector_reff_runs_one_pass_per_bucket_and_scatters_in_order(fake, case):
    import pyloo_amd as pl

    ll, theta = case
    res, msgs = quiet(pl.loo_influence_from_matrix, ll, theta, reff=R2)
    assert not msgs
    want_M = [orc.tail_count(1000, v) for v in R2]
    assert [c["tail_count"] for c in fake.calls] == sorted(set(want_M)) and len(fake.calls) == 2
    for c in fake.calls:
        assert c["rows"].tolist() == [i for i in range(12) if want_M[i] == c["tail_count"]] and c["kind"] == "loglik"
    ref = influence_ref.loo_influence(ll, theta, R2)
    assert np.array_equal(res.shift, ref["shift"]) and np.array_equal(res.kl, ref["kl"]) and np.array_equal(res.ess_w, ref["ess_w"])
    assert np.array_equal(res.pareto_k, ref["diag"]) and res.shift.shape == (12, 5) and res.kl.shape == (12,)
    # a vector with one distinct tail count: the full-matrix call, the matrix as it came
    fake.calls.clear()
    flipped = np.ascontiguousarray(ll.T).T
    one, _ = quiet(pl.loo_influence_from_matrix, flipped, theta, reff=np.full(12, 0.8))
    assert len(fake.calls) == 1 and fake.calls[0]["rows"] is None and not fake.calls[0]["draws_fastest"]
    flt, _ = quiet(pl.loo_influence_from_matrix, ll, theta, reff=0.8)
    np.testing.assert_allclose(one.shift, flt.shift, rtol=0, atol=1e-13)  # (the stand-in's sums run over another layout)
    assert np.array_equal(one.pareto_k, flt.pareto_k)
    # two buckets of an observations-fastest matrix: one copy, then the rows route
    fake.calls.clear()
    two, _ = quiet(pl.loo_influence_from_matrix, flipped, theta, reff=R2)
    assert all(c["draws_fastest"] for c in fake.calls) and np.array_equal(two.shift, res.shift)


def test_rows_selects_observations_with_a_float_and_with_a_vector(fake, case):
    import pyloo_amd as pl

    ll, theta = case
    rows = [7, 1, 1, 11, 0]
    sub, _ = quiet(pl.loo_influence_from_matrix, ll, theta, reff=0.8, rows=rows)
    assert len(fake.calls) == 1 and fake.calls[0]["rows"].tolist() == rows
    full, _ = quiet(pl.loo_influence_from_matrix, ll, theta, reff=0.8)
    for key in ("shift", "mean_loo", "sd_ratio", "kl", "ess_w", "pareto_k", "distance"):
        assert np.array_equal(getattr(sub, key), getattr(full, key)[rows]), key
    fake.calls.clear()
    vec, _ = quiet(pl.loo_influence_from_matrix, ll, theta, reff=R2, rows=rows)
    assert sorted(c["tail_count"] for c in fake.calls) == sorted({orc.tail_count(1000, R2[i]) for i in rows})
    assert sorted(sum((c["rows"].tolist() for c in fake.calls), [])) == sorted(rows)
    ref = influence_ref.loo_influence(ll, theta, R2)
    assert np.array_equal(vec.shift, ref["shift"][rows]) and np.array_equal(vec.pareto_k, ref["diag"][rows])


def test_column_names(fake, case):
    import pyloo_amd as pl

    ll, theta = case
    res, _ = quiet(pl.loo_influence_from_matrix, ll, theta)
    assert res.names == [f"theta[{j}]" for j in range(5)]
    one, _ = quiet(pl.loo_influence_from_matrix, ll, theta[:, 1])
    assert one.names == ["theta"] and one.shift.shape == (12, 1)
    np.testing.assert_allclose(one.shift[:, 0], res.shift[:, 1], rtol=0, atol=1e-13)  # (NumPy's column mean of a vector and of a matrix)
    named, _ = quiet(pl.loo_influence_from_matrix, ll, theta, names=list("abcde"))
    assert named.names == list("abcde")
    # the data front: every posterior variable flattened over its own dimensions, the chains from the data
    chains = 4
    post = {"mu": theta[:, 0].reshape(chains, 250), "beta": theta[:, 1:4].reshape(chains, 250, 3),
            "L": np.stack([theta[:, 4], theta[:, 0] + theta[:, 1], theta[:, 1] * 2.0 + theta[:, 4], theta[:, 2]], axis=1).reshape(chains, 250, 2, 2)}
    data = {"log_likelihood": {"obs": np.moveaxis(ll.reshape(3, 4, chains, 250), (2, 3), (0, 1))}, "posterior": post}
    fake.calls.clear()
    d, _ = quiet(pl.loo_influence, data)
    assert d.names == ["mu", "beta[0]", "beta[1]", "beta[2]", "L[0,0]", "L[0,1]", "L[1,0]", "L[1,1]"]
    assert fake.calls[0] == dict(op="relative_eff", n_chains=4)
    assert d.shift.shape == (3, 4, 8) and d.kl.shape == (3, 4) and d.distance.shape == (3, 4)
    assert np.array_equal(d.center[:4], influence_ref.center_scale(theta[:, :4])[0])
    some, _ = quiet(pl.loo_influence, data, var_names=["beta"], reff=1.0)
    assert some.names == ["beta[0]", "beta[1]", "beta[2]"]
    full, _ = quiet(pl.loo_influence_from_matrix, ll, theta[:, 1:4], reff=1.0)
    assert np.array_equal(some.shift.reshape(12, 3), full.shift)
    with pytest.raises(ValueError, match="not found in posterior"):
        pl.loo_influence(data, var_names=["gamma"])
    with pytest.raises(ValueError, match="posterior group"):
        pl.loo_influence({"log_likelihood": data["log_likelihood"]})


def test_result_arithmetic(fake, case):
    import pyloo_amd as pl

    ll, theta = case
    res, _ = quiet(pl.loo_influence_from_matrix, ll, theta, reff=0.5)
    assert fake.calls[0]["tail_count"] == orc.tail_count(1000, 0.5) and fake.calls[0]["rows"] is None
    ref = influence_ref.loo_influence(ll, theta, 0.5)
    want = influence_ref.front_values(ref, theta)
    assert np.array_equal(res.center, ref["center"]) and np.array_equal(res.scale, ref["scale"])
    assert np.array_equal(res.shift, ref["shift"]) and np.array_equal(res.mean_loo, want["mean_loo"])
    assert np.array_equal(res.sd_ratio, want["sd_ratio"])
    np.testing.assert_allclose(res.distance, want["distance"], rtol=1e-12)
    assert np.all(res.distance >= 0) and res.khat_threshold == orc.pareto_khat_threshold(1000)
    assert res.n_replaced == 0 and res.n_samples == 1000 and res.method == "psis" and res.ess is None
    # collinear columns count once in the distance (pinv)
    twice, _ = quiet(pl.loo_influence_from_matrix, ll, np.column_stack([theta[:, 0], theta[:, 0]]), reff=0.5)
    alone, _ = quiet(pl.loo_influence_from_matrix, ll, theta[:, 0], reff=0.5)
    np.testing.assert_allclose(twice.distance, alone.distance, rtol=1e-10)
    assert np.array_equal(alone.distance, alone.shift[:, 0] ** 2)
    # SIS / TIS: no Pareto k
    for method in ("sis", "tis"):
        fake.calls.clear()
        s, msgs = quiet(pl.loo_influence_from_matrix, ll, theta, reff=R2, method=method)
        assert len(fake.calls) == 1 and fake.calls[0]["tail_count"] == 0 and fake.calls[0]["rows"] is None and not msgs
        m = influence_ref.loo_influence(ll, theta, method=method)
        assert s.pareto_k is None and s.khat_threshold is None and np.array_equal(s.ess, m["diag"]) and np.array_equal(s.shift, m["shift"])


def test_every_rejection_comes_before_any_engine_call(fake, case):
    import pyloo_amd as pl

    ll, theta = case
    bad = theta.copy()
    bad[17, 2] = np.nan
    flat = theta.copy()
    flat[:, 3] = 1e6
    cases = [
        (dict(theta=theta[:999]), ValueError, "n_draws = 1000"),
        (dict(theta=theta.reshape(1000, 5, 1)), ValueError, "n_draws = 1000"),
        (dict(theta=bad), ValueError, "column 2 ('theta[2]') holds values that are not finite"),
        (dict(theta=np.where(np.isnan(bad), np.inf, bad)), ValueError, "not finite"),
        (dict(theta=flat, names=list("abcde")), ValueError, "column 3 ('d') is constant"),
        (dict(theta=np.zeros((1000, 1025))), ValueError, "1025 columns"),
        (dict(theta=theta, names=["a", "b"]), ValueError, "names has 2 entries for 5 columns"),
        (dict(theta=theta, reff=R2[:11]), ValueError, "11 values for 12 observations"),
        (dict(theta=theta, reff=np.where(np.arange(12) == 3, np.nan, R2)), ValueError, "reff[3] = nan"),
        (dict(theta=theta, reff=None), ValueError, "n_chains"),
        (dict(theta=theta, rows=[0, 12]), IndexError, "[0, 12)"),
        (dict(theta=theta, rows=[-1]), IndexError, "[0, 12)"),
        (dict(theta=theta, method="nope"), ValueError, ""),
    ]
    for kwargs, kind, word in cases:
        with pytest.raises(kind) as err:
            pl.loo_influence_from_matrix(ll, **kwargs)
        assert word in str(err.value), (word, str(err.value))
    with pytest.raises(ValueError, match="2-D"):
        pl.loo_influence_from_matrix(ll[0], theta)
    assert fake.calls == []


def test_both_warnings(fake, case):
    import pyloo_amd as pl

    ll, theta = case
    rng = np.random.default_rng(9)
    heavy = ll.copy()
    heavy[2] = -3.0 * rng.exponential(size=1000)
    heavy[9] = -2.5 * rng.exponential(size=1000)
    heavy[4, 5] = np.nan
    heavy[4, 6] = np.nan
    res, msgs = quiet(pl.loo_influence_from_matrix, heavy, theta, reff=R2)
    assert res.n_replaced == 2 and msgs.count(NAN_TEXT) == 1
    high = int(np.sum(res.pareto_k > res.khat_threshold))
    assert high >= 2 and res.pareto_k[2] > res.khat_threshold
    text = [m for m in msgs if "Pareto" in m]
    assert len(text) == 1 and f"for {high} observations" in text[0] and "unreliable" in text[0]
    clean, msgs = quiet(pl.loo_influence_from_matrix, ll, theta, reff=R2)
    assert not msgs and np.all(clean.pareto_k <= clean.khat_threshold)


def test_influence_table():
    import pyloo_amd as pl
    from pyloo_amd.loo_influence import LooInfluence

    shift = np.array([[0.1, -0.5, 0.2], [2.0, 0.3, -2.5], [np.nan, np.nan, np.nan], [-0.7, 0.0, 0.1], [0.0, 0.05, 0.0]])
    dist = np.array([0.3, 9.0, np.nan, 0.5, 0.0025])
    res = LooInfluence(shift=shift, mean_loo=shift, sd_ratio=np.ones_like(shift), kl=np.array([0.01, 0.9, np.nan, 0.02, 0.0]),
                       ess_w=np.ones(5), pareto_k=np.array([0.1, 0.8, np.nan, 0.2, 0.0]), distance=dist, names=["a", "b", "c"], n_replaced=0,
                       khat_threshold=0.7)
    t = pl.influence_table(res, n=3)
    assert list(t.index) == [1, 3, 0] and t.index.name == "observation"
    assert t["column"].tolist() == ["c", "a", "b"] and t["max_abs_shift"].tolist() == [2.5, 0.7, 0.5] and t["shift"].tolist() == [-2.5, -0.7, -0.5]
    assert t["distance"].tolist() == [9.0, 0.5, 0.3] and t["pareto_k"].tolist() == [0.8, 0.2, 0.1] and t["kl"].tolist() == [0.9, 0.02, 0.01]
    every = pl.influence_table(res, n=10)
    assert list(every.index) == [1, 3, 0, 4, 2]  # (the NaN row last)
    # observation-shaped fields are read flat
    res.shift, res.distance, res.kl, res.pareto_k = shift[:4].reshape(2, 2, 3), dist[:4].reshape(2, 2), res.kl[:4].reshape(2, 2), None
    t = pl.influence_table(res, n=1)
    assert list(t.index) == [1] and np.isnan(t["pareto_k"].iloc[0])


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
    assert "pla_loo_influence" in _capi.SYMBOLS and hasattr(lib, "pla_loo_influence")
    assert re.search(r"\bint pla_loo_influence\(const pla_influence_args \*", header) and re.search(r"\bpla_loo_influence\b", guide)
    assert len(lib.pla_loo_influence.argtypes) == 1
    assert f"#define PLA_ABI_VERSION {lib.pla_abi_version()}" in header and lib.pla_abi_version() == _capi.ABI_VERSION
    assert "pla_k_influence.hip" in b.SOURCES
    # the binding's struct is the header's, field for field
    body = re.search(r"typedef struct pla_influence_args \{(.*?)\} pla_influence_args;", header, flags=re.S).group(1)
    declared = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert declared == [name for name, _ in _capi.InfluenceArgs._fields_], declared
    assert C.sizeof(_capi.InfluenceArgs) == 8 * (len(declared) - 2)  # (every field 8 bytes but the four int32)


def test_argument_errors_each_have_their_own_message(lib):
    from pyloo_amd import _capi

    assert lib.pla_loo_influence(None) == -1 and lib.pla_last_error() == b"args is NULL"
    args = _capi.InfluenceArgs(n_obs=2, n_draws=16, stride_obs=16, stride_draw=1, n_quant=1)
    assert lib.pla_loo_influence(C.byref(args)) == -1 and b"engine" in lib.pla_last_error()
    args.struct_size -= 8
    args.engine = 1  # (never followed: the size is checked first)
    assert lib.pla_loo_influence(C.byref(args)) == -1
    msg = lib.pla_last_error()
    assert b"struct_size" in msg and str(C.sizeof(_capi.InfluenceArgs)).encode() in msg


# ------------------------------------------------------------------------------------------------------------- the generated code
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_new_kernels_use_no_scratch_and_keep_the_stated_occupancy(tmp_path):
    """DESIGN.md (LOO influence): four wavefronts per SIMD with one column tile, three with two, two with the 64-quantity panel; no
    scalar register in a vector lane."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    lines = isa_stats.compile_isa(out=str(tmp_path / "influence.s"), units=["pla_k_influence.hip"])
    names = [k for k in isa_stats.all_kernels(lines) if "influence_" in k]
    # prepare; influence: two dtypes x 16-byte / element loads x one / two / four column tiles
    assert len(names) == 1 + 12, names
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert not isa_stats.masked_spills(lines, k[2:]) and total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        regs = res["NumVgprs"] + res.get("NumAgprs", 0)
        if "prepare" in k:
            assert regs <= 64, (name, res)
            continue
        nct = int(re.search(r"Li[01]ELi(\d)E", k).group(1))
        waves = {1: 4, 2: 3, 4: 2}[nct]
        assert regs <= 512 // waves // 8 * 8 and res.get("Occupancy", 0) >= waves, (name, res)
