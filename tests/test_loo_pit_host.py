"""Host side of ``loo_pit`` without a GPU.  The yardstick first: the NumPy restatement (tests/pit_ref.py) on the CPU oracle's
weights against the fixtures of the real reference (tests/golden/loo_pit.npz).  Then the feature: the new C export and its
argument checks, the front through an oracle-backed stand-in engine (validation, dict-of-groups ingestion, obs-shape reshaping,
the three ``randomized`` settings, the seed, clipping, the two warnings, the ``log_weights=`` path) and the generated code of
the new kernels."""

import importlib
import os
import re
import shutil
import sys
import warnings

import numpy as np
import pytest

import pit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."
K_TEXT = "Estimated shape parameter of Pareto distribution is greater than"


# ------------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.fixture(scope="module")
def cases():
    return pit_ref.load_golden()


def test_fixture_has_the_cases(cases):
    assert sorted(cases) == ["edges_s500_r1", "poisson_s500_r1", "s1000_r0p7", "s1000_r1_f32", "s100_r1", "s4000_r1"]
    assert cases["s1000_r1_f32"]["ll"].dtype == np.float32 and cases["s1000_r1_f32"]["yh"].dtype == np.float32
    assert cases["s1000_r0p7"]["reff"] == 0.7
    p = cases["poisson_s500_r1"]
    assert np.all((p["yh"] == p["y"][:, None]).any(axis=1))  # ties in every row
    e = cases["edges_s500_r1"]
    assert np.isnan(e["ll"]).sum() == 1 and np.isnan(e["yh"]).sum() == 2 and np.isinf(e["yh"]).sum() == 2 and np.isnan(e["y"]).sum() == 1


def test_restatement_equals_the_reference_fixtures(cases):
    """1e-12: the bound test_oracle_golden.py holds the oracle's weights to."""
    for name, c in cases.items():
        r = pit_ref.loo_pit(c["ll"].astype(np.float64), c["yh"], c["y"], c["reff"])  # (f32 inputs: the numbers of their upcast)
        le, lt = pit_ref.golden_expected(c)
        np.testing.assert_allclose(r["pit_le"], le, rtol=0, atol=1e-12, err_msg=name)
        np.testing.assert_allclose(r["pit_lt"], lt, rtol=0, atol=1e-12, err_msg=name)
        np.testing.assert_allclose(r["diag"], c["k"], rtol=1e-12, err_msg=name)
        assert r["n_replaced"] == int(np.isnan(c["ll"]).sum())


def test_restatement_on_the_edge_rows(cases):
    e = cases["edges_s500_r1"]
    r = pit_ref.loo_pit(e["ll"], e["yh"], e["y"], 1.0)
    assert r["pit_le"][0] == 0.0 and r["pit_lt"][0] == 0.0 and r["pit_le"][1] == 1.0 and r["pit_lt"][1] == 1.0
    count = (e["yh"][2] <= e["y"][2]).sum() / 500.0
    assert abs(r["pit_le"][2] - count) < 1e-12 and np.isinf(r["diag"][2])
    assert r["pit_le"][6] == 0.0  # a NaN observation: nothing is counted
    p = cases["poisson_s500_r1"]
    rp = pit_ref.loo_pit(p["ll"], p["yh"], p["y"], 1.0)
    assert np.all(rp["pit_lt"] < rp["pit_le"])


def test_the_weights_normalisation_does_not_matter(cases):
    c = cases["s100_r1"]
    a = pit_ref.pit_from_log_weights(c["lw"], c["yh"], c["y"])
    b = pit_ref.pit_from_log_weights(c["lw"] + 123.0, c["yh"], c["y"])
    np.testing.assert_allclose(a[0], b[0], rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (as tests/test_capi_abi.py: a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


def test_new_symbol_in_header_binding_and_library(lib):
    from pyloo_amd import _capi

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    assert "pla_loo_pit" in _capi.SYMBOLS and hasattr(lib, "pla_loo_pit")
    assert re.search(r"\bint pla_loo_pit\(", header)
    assert "#define PLA_PIT_LOGLIK 0" in header and "#define PLA_PIT_LOG_WEIGHTS 1" in header
    assert (_capi.PLA_PIT_LOGLIK, _capi.PLA_PIT_LOG_WEIGHTS) == (0, 1)
    assert len(lib.pla_loo_pit.argtypes) == 20
    assert f"#define PLA_ABI_VERSION {lib.pla_abi_version()}" in header and lib.pla_abi_version() == _capi.ABI_VERSION
    assert "pla_loo_pit" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    from pyloo_amd import build as b

    assert "pla_k_pit.hip" in b.SOURCES


def test_null_engine_is_an_argument_error(lib):
    rc = lib.pla_loo_pit(None, None, None, None, 0, 1, 10, 10, 1, 10, 1, 0, 0, 2, 0, None, None, None, None, None)
    assert rc == -1 and b"engine" in lib.pla_last_error()


# -------------------------------------------------------------------------------------------------------------------- the front
class OraclePitEngine:
    """Stand-in for ``Engine.loo_pit`` on the restatement (test infrastructure: the product has no CPU path)."""

    device = "cpu-oracle"

    def __init__(self):
        self.calls = []

    def loo_pit(self, mat, y_hat, y, tail_count=0, method="psis", kind="loglik"):
        from oracle import psis_oracle as orc

        mat, y_hat = np.asarray(mat), np.asarray(y_hat)
        self.calls.append({"kind": kind, "method": method, "tail_count": tail_count, "shape": mat.shape})
        if kind == "log_weights":
            le, lt = pit_ref.pit_from_log_weights(mat, y_hat, y)
            return {"pit_le": le, "pit_lt": lt, "diag": None, "n_replaced": 0}
        nan = np.isnan(mat)
        clean = np.where(nan, -1e10, mat)
        with np.errstate(all="ignore"):
            if method == "psis":
                rows = [orc.psis_row(-r, tail_count) for r in clean]
                lw, diag = np.array([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=np.float64)
            else:
                lw, diag = orc.importance_weights(-clean, method)
        le, lt = pit_ref.pit_from_log_weights(lw, y_hat, y)
        return {"pit_le": le, "pit_lt": lt, "diag": diag, "n_replaced": int(nan.sum())}


@pytest.fixture()
def fake(monkeypatch):
    eng = OraclePitEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_pit"), "get_engine", lambda device=None: eng)
    return eng


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


def groups(rng, chains=2, draws=150, obs=(7,), poisson=False, tail=0.4):
    shape = (chains, draws) + obs
    ll = -tail * rng.exponential(size=shape) - 1.0
    if poisson:
        yh = rng.poisson(3.0, size=shape).astype(np.float64)
        y = rng.poisson(3.0, size=obs).astype(np.float64)
    else:
        yh = rng.normal(size=shape)
        y = rng.normal(size=obs)
    return {"log_likelihood": {"obs": ll}, "posterior_predictive": {"obs": yh}, "observed_data": {"obs": y},
            "posterior": {"mu": rng.normal(size=(chains, draws))}}


def stacked(a):
    """(chain, draw, *obs) -> (n_obs, n_draws), chain-major along the draws (loo.py:189)."""
    a = np.asarray(a)
    return np.moveaxis(a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:]), 0, -1).reshape(-1, a.shape[0] * a.shape[1])


def test_front_is_exported():
    import pyloo_amd as pl

    for name in ("loo_pit", "loo_pit_from_matrix", "LooPitResult"):
        assert name in pl.__all__ and hasattr(pl, name)


def test_dict_of_groups_equals_the_stacked_matrices(fake):
    import pyloo_amd as pl

    g = groups(np.random.default_rng(1))
    res, _ = quiet(pl.loo_pit, g, reff=1.0)
    ll, yh = stacked(g["log_likelihood"]["obs"]), stacked(g["posterior_predictive"]["obs"])
    ref = pit_ref.loo_pit(ll, yh, g["observed_data"]["obs"], 1.0)
    np.testing.assert_allclose(np.asarray(res.pit_le), ref["pit_le"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.asarray(res.pareto_k), ref["diag"], rtol=1e-12)
    mres, _ = quiet(pl.loo_pit_from_matrix, ll, yh, g["observed_data"]["obs"], reff=1.0)
    assert np.array_equal(mres.pit, np.asarray(res.pit)) and np.array_equal(mres.pit_lt, np.asarray(res.pit_lt))
    assert np.array_equal(np.asarray(res.pit), np.asarray(res.pit_le))  # continuous data: nothing to randomise
    assert res.good_k == min(1 - 1 / np.log10(300), 0.7)
    assert fake.calls[0] == {"kind": "loglik", "method": "psis", "tail_count": 52, "shape": (7, 300)}
    # names and arrays
    named, _ = quiet(pl.loo_pit, g, y="obs", y_hat="obs", var_name="obs", reff=1.0)
    arrays, _ = quiet(pl.loo_pit, g, y=g["observed_data"]["obs"], y_hat=g["posterior_predictive"]["obs"], reff=1.0)
    assert np.array_equal(np.asarray(named.pit), np.asarray(res.pit)) and np.array_equal(np.asarray(arrays.pit), np.asarray(res.pit))


def test_multi_dimensional_observations_come_back_in_shape(fake):
    import pyloo_amd as pl

    g = groups(np.random.default_rng(2), obs=(3, 4))
    res, _ = quiet(pl.loo_pit, g, reff=1.0)
    for v in (res.pit, res.pit_le, res.pit_lt, res.pareto_k):
        assert np.asarray(v).shape == (3, 4)
    ref = pit_ref.loo_pit(stacked(g["log_likelihood"]["obs"]), stacked(g["posterior_predictive"]["obs"]),
                          g["observed_data"]["obs"].reshape(-1), 1.0)
    np.testing.assert_allclose(np.asarray(res.pit_le).reshape(-1), ref["pit_le"], rtol=0, atol=1e-12)


def test_reff_none_goes_through_the_relative_efficiency(fake):
    import pyloo_amd as pl

    g = groups(np.random.default_rng(3), chains=1, draws=200)
    res, _ = quiet(pl.loo_pit, g)  # one chain: reff = 1
    assert fake.calls[0]["tail_count"] == 40
    g.pop("posterior")
    with pytest.raises(TypeError, match="posterior"):
        pl.loo_pit(g)


def test_randomized_settings_seed_and_ties(fake):
    import pyloo_amd as pl

    g = groups(np.random.default_rng(4), poisson=True)
    ll, yh, y = stacked(g["log_likelihood"]["obs"]), stacked(g["posterior_predictive"]["obs"]), g["observed_data"]["obs"]
    yh[0] = np.random.default_rng(5).normal(size=yh.shape[1]) + 0.5  # one row without ties
    off, _ = quiet(pl.loo_pit_from_matrix, ll, yh, y, randomized=False)
    auto, _ = quiet(pl.loo_pit_from_matrix, ll, yh, y, randomized="auto", seed=11)
    on, _ = quiet(pl.loo_pit_from_matrix, ll, yh, y, randomized=True, seed=11)
    again, _ = quiet(pl.loo_pit_from_matrix, ll, yh, y, randomized=True, seed=11)
    other, _ = quiet(pl.loo_pit_from_matrix, ll, yh, y, randomized=True, seed=12)
    assert np.array_equal(off.pit, off.pit_le)
    ties = off.pit_lt != off.pit_le
    assert ties[1:].all() and not ties[0]
    u = np.random.default_rng(11).uniform(size=7)
    want = np.minimum(off.pit_lt + u * (off.pit_le - off.pit_lt), 1.0)
    assert np.array_equal(on.pit, want) and np.array_equal(auto.pit, want) and np.array_equal(again.pit, on.pit)
    assert not np.array_equal(other.pit, on.pit)
    assert on.pit[0] == off.pit_le[0] and other.pit[0] == off.pit_le[0]  # a row without ties is unchanged, bit for bit
    assert np.all(on.pit[1:] >= off.pit_lt[1:]) and np.all(on.pit[1:] <= off.pit_le[1:])
    # "auto" without any tie: no randomisation, whatever the seed
    cont = groups(np.random.default_rng(6))
    a, _ = quiet(pl.loo_pit, cont, reff=1.0, randomized="auto", seed=3)
    assert np.array_equal(np.asarray(a.pit), np.asarray(a.pit_le))
    t, _ = quiet(pl.loo_pit, cont, reff=1.0, randomized=True, seed=3)
    assert np.array_equal(np.asarray(t.pit), np.asarray(a.pit_le))
    with pytest.raises(ValueError, match="randomized"):
        pl.loo_pit_from_matrix(ll, yh, y, randomized="yes")


def test_values_are_clipped_to_one(monkeypatch):
    import pyloo_amd as pl

    class Above:
        def loo_pit(self, mat, y_hat, y, tail_count=0, method="psis", kind="loglik"):
            n = np.asarray(mat).shape[0]
            return {"pit_le": np.full(n, 1.0 + 4e-16), "pit_lt": np.full(n, 0.25), "diag": np.zeros(n), "n_replaced": 0}

    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_pit"), "get_engine", lambda device=None: Above())
    r = pl.loo_pit_from_matrix(np.zeros((3, 50)), np.zeros((3, 50)), np.zeros(3), randomized=False)
    assert np.all(r.pit == 1.0) and np.all(r.pit_le > 1.0)
    r = pl.loo_pit_from_matrix(np.zeros((3, 50)), np.zeros((3, 50)), np.zeros(3), randomized=True, seed=1)
    assert np.all(r.pit <= 1.0)


def test_the_two_warnings(fake):
    import pyloo_amd as pl

    g = groups(np.random.default_rng(7))
    g["log_likelihood"]["obs"][0, 3, 2] = np.nan
    res, msgs = quiet(pl.loo_pit, g, reff=1.0)
    assert NAN_TEXT in msgs
    assert np.all(np.isfinite(np.asarray(res.pit_le)))
    rng = np.random.default_rng(8)
    g = groups(rng)
    g["log_likelihood"]["obs"] = -3.0 * rng.pareto(0.6, size=g["log_likelihood"]["obs"].shape)  # very heavy tails of the ratios
    res, msgs = quiet(pl.loo_pit, g, reff=1.0)
    k = np.asarray(res.pareto_k)
    assert np.any(k > res.good_k) and res.warning is True
    text = [m for m in msgs if m.startswith(K_TEXT)]
    assert text and f"for {np.sum(k > res.good_k)} observations" in text[0] and f"{res.good_k:.2f}" in text[0]
    calm, msgs = quiet(pl.loo_pit, groups(np.random.default_rng(9), tail=0.05), reff=1.0)  # light tails: every k is small
    assert calm.warning is False and not [m for m in msgs if m.startswith(K_TEXT)]


def test_log_weights_path(fake):
    import pyloo_amd as pl

    g = groups(np.random.default_rng(10))
    ll, yh, y = stacked(g["log_likelihood"]["obs"]), stacked(g["posterior_predictive"]["obs"]), g["observed_data"]["obs"]
    lw = pit_ref.log_weights(ll, 1.0)[0]
    res, msgs = quiet(pl.loo_pit_from_matrix, None, yh, y, log_weights=lw)
    assert res.pareto_k is None and res.good_k is None and res.warning is False and not msgs
    assert fake.calls[-1]["kind"] == "log_weights"
    full, _ = quiet(pl.loo_pit_from_matrix, ll, yh, y)
    np.testing.assert_allclose(res.pit_le, full.pit_le, rtol=0, atol=1e-12)
    # (chain, draw, *obs) weights through the front; no log-likelihood group, no posterior needed
    lw3 = np.moveaxis(lw, -1, 0).reshape(g["log_likelihood"]["obs"].shape)
    front, _ = quiet(pl.loo_pit, {"posterior_predictive": g["posterior_predictive"], "observed_data": g["observed_data"]},
                     log_weights=lw3)
    assert np.array_equal(np.asarray(front.pit_le), res.pit_le) and front.pareto_k is None
    bare, _ = quiet(pl.loo_pit, None, y=y, y_hat=g["posterior_predictive"]["obs"], log_weights=lw3)
    assert np.array_equal(np.asarray(bare.pit_le), res.pit_le)


def test_validation_errors(fake):
    import pyloo_amd as pl

    g = groups(np.random.default_rng(12))
    ll, yh, y = stacked(g["log_likelihood"]["obs"]), stacked(g["posterior_predictive"]["obs"]), g["observed_data"]["obs"]
    with pytest.raises(ValueError, match="Invalid method"):
        pl.loo_pit(g, reff=1.0, method="foo")
    with pytest.raises(ValueError, match="Invalid method"):
        pl.loo_pit_from_matrix(ll, yh, y, method="foo")
    with pytest.raises(ValueError, match="y_hat dimensions"):
        pl.loo_pit_from_matrix(ll, yh[:, :-1], y)
    with pytest.raises(ValueError, match="y dimensions"):
        pl.loo_pit_from_matrix(ll, yh, y[:-1])
    with pytest.raises(ValueError, match="y dimensions"):
        pl.loo_pit(g, y=np.zeros(6), reff=1.0)
    with pytest.raises(ValueError, match="y dimensions"):
        pl.loo_pit(g, y=np.zeros((7, 1)), reff=1.0)
    bad = dict(g, log_likelihood={"obs": g["log_likelihood"]["obs"][:, :, :-1]})
    with pytest.raises(ValueError, match="log_lik dimensions"):
        pl.loo_pit(bad, reff=1.0)
    with pytest.raises(ValueError, match="log_weights dimensions"):
        pl.loo_pit(g, log_weights=np.zeros((2, 150, 6)))
    with pytest.raises(ValueError, match="not found in posterior_predictive"):
        pl.loo_pit(g, y_hat="nope", reff=1.0)
    two = dict(g, posterior_predictive={"a": g["posterior_predictive"]["obs"], "b": g["posterior_predictive"]["obs"]})
    with pytest.raises(ValueError, match="Multiple variables"):
        pl.loo_pit(two, reff=1.0)
    with pytest.raises(ValueError, match="either a log-likelihood or log_weights"):
        pl.loo_pit_from_matrix(None, yh, y)
    with pytest.raises(ValueError, match="without data"):
        pl.loo_pit(None, y="obs", y_hat=yh)
    sis, msgs = quiet(pl.loo_pit, g, reff=1.0, method="sis")
    assert sis.pareto_k is None and sis.good_k is None and fake.calls[-1]["method"] == "sis"


# ------------------------------------------------------------------------------------------------------------- the generated code
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_new_kernels_use_no_scratch_and_spill_no_scalars(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    lines = isa_stats.compile_isa(out=str(tmp_path / "pit.s"), units=["pla_k_pit.hip"])
    names = [k for k in isa_stats.all_kernels(lines) if "pit_" in k]
    # prepare: row and tile, f64 and f32; wave: three load modes x registers / streamed x two dtypes; lane: two dtypes
    assert len(names) == 4 + 12 + 2, names
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert not isa_stats.masked_spills(lines, k[2:]), name
        assert res.get("Occupancy", 0) >= 1 and res.get("LDSByteSize", 0) <= 40 * 1024, (name, res)
        if "pit_wave_kernel" in k and "Li2E" not in k:  # the unit-stride routes: two waves per SIMD at least
            assert res["NumVgprs"] + res.get("NumAgprs", 0) <= 256, (name, res)
