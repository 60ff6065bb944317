"""Host side of ``loo_lfo`` without a GPU.  The yardstick first: the NumPy restatement of PSIS leave-future-out CV
(tests/lfo_ref.py) against properties that hold whatever the implementation.  Then the feature: the two C exports and their
argument checks, the front through an oracle-backed stand-in engine (validation, ingestion, the refit protocol, the result's keys,
the report, the warnings, indexing by t) and the generated code of the new kernels."""

import importlib
import math
import os
import re
import shutil
import sys
import warnings

import numpy as np
import pytest

import lfo_ref
from oracle import psis_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."
K_TEXT = "Estimated shape parameter of Pareto distribution is greater than"
C = lfo_ref.CHUNK


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def test_prefix_sums_within_the_classical_bound_of_exact_sums():
    """|lr_j - fsum| <= (j - 1) 2^-53 sum |ll|: the first-order bound of any order of j - 1 additions."""
    rng = np.random.default_rng(11)
    ll = lfo_ref.draw_ll(rng, 3 * C + 9, 6)
    for first in (0, 5):
        n_steps = ll.shape[0] - first + 1
        lr = lfo_ref.ratios(ll, first, n_steps)
        assert lr.shape == (n_steps, 6) and np.all(lr[0] == 0.0)
        for s in range(6):
            col = ll[first:, s]
            for j in range(1, n_steps):
                exact = math.fsum(col[:j])
                bound = (j - 1) * 2.0 ** -53 * math.fsum(np.abs(col[:j]))
                assert abs(lr[j, s] - exact) <= bound, (first, s, j, lr[j, s], exact, bound)


def test_prefix_sums_are_cumsum_when_the_sums_are_exact():
    rng = np.random.default_rng(12)
    ll = rng.integers(-4096, 4096, size=(2 * C + 17, 5)).astype(np.float64) / 64.0
    lr = lfo_ref.ratios(ll, 3, ll.shape[0] - 2)
    want = np.vstack([np.zeros((1, 5)), np.cumsum(ll[3:], axis=0)])
    assert np.array_equal(lr, want)
    ll32 = ll.astype(np.float32)  # (f32 input is widened: the same numbers)
    assert np.array_equal(lfo_ref.ratios(ll32, 3, ll.shape[0] - 2), want)


def test_nan_counts_as_minus_1e10_and_inf_propagates():
    ll = lfo_ref.draw_ll(np.random.default_rng(13), 20, 8)
    ll[4, 2] = np.nan
    ll[6, 3] = -np.inf
    lr = lfo_ref.ratios(ll, 2, 10)
    assert lr[2, 2] == ll[2, 2] + ll[3, 2] and lr[3, 2] == (ll[2, 2] + ll[3, 2]) + -1e10
    assert np.isfinite(lr[4, 3]) and np.all(lr[5:, 3] == -np.inf)
    r = lfo_ref.lfo_pass(ll, 2, 10, 2)
    assert r["n_replaced"] == 1 and lfo_ref.lfo_pass(ll, 5, 10, 2)["n_replaced"] == 0


def test_the_first_importance_step_weights_are_psislw_of_one_row():
    rng = np.random.default_rng(14)
    ll = lfo_ref.draw_ll(rng, 12, 400)
    first = 3
    r = lfo_ref.lfo_pass(ll, first, 4, 1)
    assert np.array_equal(r["ratios"][1], ll[first])
    lw, k = orc.psislw(+ll[first])
    assert r["diag"][1] == k and r["diag"][0] == 0.0
    assert r["elpd_i"][1] == orc.lse(lw + ll[first + 1]) - orc.lse(lw)
    assert r["elpd_i"][0] == orc.lse(ll[first]) - np.log(400)


def test_a_matrix_constant_over_the_draws():
    """Every draw agrees: the weights are uniform (k = inf, no tail) and the predictive density is the window's sum, exactly.
    The rows are multiples of 1/4, the window sums c stay in [-3.75, 0] and S = 64: log 64 (in [4, 8), a multiple of 2^-50) enters
    and leaves each value as (c - log S) + log S, and c - log S is a multiple of 2^-50 below 8, so both steps are exact."""
    rows = np.array([-0.25, -0.5, -0.75, -1.0, -0.25, -0.5, -1.25, -0.75, -0.5, -0.25, -1.0, -0.5])
    ll = np.repeat(rows[:, None], 64, axis=1)
    for M in (1, 2, 4):
        r = lfo_ref.lfo_pass(ll, 2, 7, M)
        want = np.array([rows[2 + j:2 + j + M].sum() for j in range(7)])
        assert np.array_equal(r["elpd_i"], want), (M, r["elpd_i"] - want)
        assert r["diag"][0] == 0.0 and np.all(np.isinf(r["diag"][1:])) and np.all(r["diag"][1:] > 0)


def test_minus_inf_threshold_refits_at_every_step_and_is_exact():
    N, L, M = 14, 4, 2
    mats = {t: lfo_ref.draw_ll(np.random.default_rng(100 + t), N, 50 + t) for t in range(L, N)}
    called = []

    def refit(t):
        called.append(t)
        return mats[t]

    w = lfo_ref.lfo_walk(mats[L], L, M, refit, k_threshold=-np.inf)
    steps = list(range(L, N - M + 1))
    assert w["refits"] == steps[1:] == called
    for i, t in enumerate(steps):
        f = mats[t][t] + mats[t][t + 1]
        assert w["elpd"][i] == orc.lse(f) - np.log(mats[t].shape[1]), t


def test_plus_inf_threshold_never_refits():
    ll = lfo_ref.draw_ll(np.random.default_rng(16), 30, 200, k_lo=0.8, k_hi=1.5)

    def refit(t):
        raise AssertionError("refit called")

    w = lfo_ref.lfo_walk(ll, 5, 1, refit, k_threshold=np.inf)
    p = lfo_ref.lfo_pass(ll, 5, 25, 1)
    assert w["refits"] == [] and np.array_equal(w["elpd"], p["elpd_i"]) and np.array_equal(w["k"], p["diag"])
    assert lfo_ref.first_high([0.0, 9.0, np.nan, 0.8], 0.7) == 1 and lfo_ref.first_high([9.0, 0.1, np.nan, 0.2], 0.7) == 4


# ------------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (as tests/test_capi_abi.py: a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


def test_new_symbols_in_header_binding_and_library(lib):
    from pyloo_amd import _capi
    from pyloo_amd import build as b

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    for sym, n_args in (("pla_lfo_ratios", 13), ("pla_lfo", 19)):
        assert sym in _capi.SYMBOLS and hasattr(lib, sym)
        assert re.search(r"\bint " + sym + r"\(", header)
        assert len(getattr(lib, sym).argtypes) == n_args
        assert sym in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"#define PLA_ABI_VERSION {lib.pla_abi_version()}" in header and lib.pla_abi_version() == _capi.ABI_VERSION == 7
    assert "pla_k_lfo.hip" in b.SOURCES


def _lfo(lib, eng=None, ll=1, dtype=0, n_obs=100, n_draws=50, so=50, sd=1, first=10, n_steps=20, horizon=2, method=0, tail=15, thr=0.7,
         space=1):
    """(status, text); ll = 1: a pointer that is never followed (every call here fails its argument checks first)."""
    rc = lib.pla_lfo(eng, ll, dtype, n_obs, n_draws, so, sd, first, n_steps, horizon, method, tail, thr, space, None, None, None, None, None)
    return rc, lib.pla_last_error().decode()


def test_null_engine_and_argument_errors(lib):
    assert _lfo(lib) == (-1, "engine is NULL")
    rc = lib.pla_lfo_ratios(None, 1, 0, 100, 50, 50, 1, 10, 20, 1, None, 1, None)
    assert rc == -1 and lib.pla_last_error() == b"engine is NULL"
    for kwargs, code, word in (
        (dict(first=-1), -1, "first"),
        (dict(horizon=0), -1, "horizon"),
        (dict(n_steps=0), -1, "n_steps"),
        (dict(n_steps=90), -1, "n_steps"),       # 100 - 10 - 2 + 1 = 89 steps at most
        (dict(n_draws=1, so=1), -1, "n_draws"),
        (dict(method=1), -4, "method"),
        (dict(method=2), -4, "method"),
        (dict(method=7), -1, "method"),
        (dict(dtype=5), -1, "dtype"),
        (dict(space=3), -1, "mem_space"),
        (dict(ll=None), -1, "ll"),
        (dict(thr=float("nan")), -1, "k_threshold"),
        (dict(so=0), -1, "strides"),
    ):
        rc, text = _lfo(lib, **kwargs)
        assert rc == code and word in text, (kwargs, rc, text)
    assert _lfo(lib, n_steps=89)[1] == "engine is NULL"  # (the largest n_steps passes the checks)
    rc = lib.pla_lfo_ratios(None, 1, 0, 100, 50, 50, 1, 10, 92, 1, None, 1, None)  # 100 - 10 + 1 = 91 at most
    assert rc == -1 and b"n_steps" in lib.pla_last_error()
    rc = lib.pla_lfo_ratios(None, 1, 0, 100, 50, 50, 1, 10, 91, 1, None, None, None)
    assert rc == -1 and b"out" in lib.pla_last_error()


# -------------------------------------------------------------------------------------------------------------------- the front
@pytest.fixture()
def fake(monkeypatch):
    eng = lfo_ref.OracleLfoEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_lfo"), "get_engine", lambda device=None: eng)
    return eng


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


def _chains(mat, chains=2):
    """(N, S) -> (chain, draw, N) with the stacked (obs, sample) view equal to mat."""
    n, s = mat.shape
    return np.ascontiguousarray(mat.T.reshape(chains, s // chains, n))


def test_validation_errors(fake):
    import pyloo_amd as pl

    ll = lfo_ref.draw_ll(np.random.default_rng(20), 12, 40)
    for kwargs, text in ((dict(L=0), "L must be at least 1"), (dict(L=3, M=0), "M must be at least 1"), (dict(L=10, M=3), "exceeds"),
                         (dict(L=3, method="sis"), "psis"), (dict(L=3, method="tis"), "psis")):
        with pytest.raises(ValueError, match=text):
            pl.loo_lfo_from_matrix(ll, **kwargs)
    with pytest.raises(ValueError, match="expected all 12"):
        pl.loo_lfo_from_matrix(ll, 3, refit=lambda t: ll[:11], k_threshold=-np.inf)
    with pytest.raises(ValueError, match="one observation dimension"):
        pl.loo_lfo(np.zeros((2, 20, 4, 3)), 1, reff=1.0)
    with pytest.raises(ValueError, match="2-D"):
        pl.loo_lfo_from_matrix(np.zeros(5), 1)
    assert len(fake.calls) == 1  # (the pass before the refit that returned another N; no other case reaches the engine)


def test_ingestion_of_dicts_and_chain_draw_arrays(fake):
    import pyloo_amd as pl

    ll = lfo_ref.draw_ll(np.random.default_rng(21), 15, 60)
    want = lfo_ref.lfo_walk(ll, 4, 2)
    a, _ = quiet(pl.loo_lfo_from_matrix, ll, 4, 2, pointwise=True)
    b, _ = quiet(pl.loo_lfo, _chains(ll), 4, 2, reff=1.0, pointwise=True)
    c, _ = quiet(pl.loo_lfo, {"log_likelihood": {"y": _chains(ll)}, "posterior": {"mu": np.zeros((2, 30))}}, 4, 2, reff=1.0, pointwise=True)
    for r in (a, b, c):
        assert r["elpd_lfo"] == want["elpd"].sum() and r["n_data_points"] == 10 and r["n_samples"] == 60
        assert np.array_equal(np.asarray(r["lfo_i"])[4:14], want["elpd"])
    assert fake.calls[0]["tail_count"] == orc.tail_count(60, 1.0) and fake.calls[0]["first"] == 4 and fake.calls[0]["n_steps"] == 10


def test_refit_protocol_tuple_and_another_draw_count(fake):
    import pyloo_amd as pl

    N, L, M = 40, 6, 1
    gen = lambda t, s: lfo_ref.draw_ll(np.random.default_rng(300 + t), N, s, k_lo=0.3, k_hi=1.2)  # noqa: E731
    ll0 = gen(L, 100)
    def make(containers):
        seen = []

        def refit(t):  # in turn: a (matrix, reff) tuple; a log-likelihood alone, with another draw count
            seen.append(t)
            if len(seen) % 2:
                return gen(t, 80 + t), 0.8
            m = gen(t, 80 + 2 * t)
            return _chains(m) if containers else m

        return refit, seen

    want = lfo_ref.lfo_walk(ll0, L, M, make(False)[0], 0.5)
    refit, seen = make(True)
    res, msgs = quiet(pl.loo_lfo_from_matrix, ll0, L, M, refit=refit, k_threshold=0.5, pointwise=True)
    assert len(want["refits"]) >= 2, want["refits"]  # (the inputs are chosen so that the walk refits more than once)
    assert res["refits"] == want["refits"] == seen and res["n_refits"] == len(seen)
    np.testing.assert_array_equal(np.asarray(res["lfo_i"])[L:N - M + 1], want["elpd"])
    np.testing.assert_array_equal(np.asarray(res["pareto_k"])[L:N - M + 1], want["k"])
    for t in res["refits"]:  # the k recorded at a refit step is the one that asked for it
        assert res["pareto_k"][t] > 0.5
    # every pass starts at its fit's own step, takes all the steps that remain and recomputes the tail count from its draw count
    assert [c["first"] for c in fake.calls] == [L] + seen
    assert all(c["n_steps"] == N - M - c["first"] + 1 for c in fake.calls)
    assert fake.calls[1]["shape"][1] == 80 + seen[0] and fake.calls[1]["tail_count"] == orc.tail_count(80 + seen[0], 0.8)
    assert fake.calls[2]["tail_count"] == orc.tail_count(80 + 2 * seen[1], 0.8)  # (no reff of its own: the current one)
    assert not any(K_TEXT in m for m in msgs)


def test_result_keys_order_scale_and_report(fake):
    import pyloo_amd as pl

    ll = lfo_ref.draw_ll(np.random.default_rng(23), 20, 100)
    want = lfo_ref.lfo_walk(ll, 5, 2)
    res, _ = quiet(pl.loo_lfo_from_matrix, ll, 5, 2)
    assert list(res.index) == ["elpd_lfo", "se", "n_samples", "n_data_points", "warning", "scale", "L", "M", "k_threshold", "n_refits",
                               "refits", "good_k"]
    assert res["se"] == (14 * np.var(want["elpd"])) ** 0.5 and res["scale"] == "log" and res["good_k"] == min(1 - 1 / np.log10(100), 0.7)
    assert (res["L"], res["M"], res["k_threshold"], res["n_refits"], res["refits"]) == (5, 2, 0.7, 0, [])
    pw, _ = quiet(pl.loo_lfo_from_matrix, ll, 5, 2, pointwise=True, scale="deviance")
    assert list(pw.index) == ["elpd_lfo", "se", "n_samples", "n_data_points", "warning", "lfo_i", "scale", "L", "M", "k_threshold",
                              "n_refits", "refits", "pareto_k", "good_k"]
    assert pw["elpd_lfo"] == (-2 * want["elpd"]).sum() and pw["scale"] == "deviance"
    text = str(res)
    assert "100 posterior samples using 2-step-ahead leave-future-out cross-validation" in text
    assert "with 14 steps (L = 5), 0 refits at k > 0.70." in text
    assert re.search(r"elpd_lfo\s+-?\d+\.\d\d\s+\d+\.\d\d", text)
    assert "Pareto k" not in text and ("All Pareto k" in str(pw) or "Pareto k diagnostic values" in str(pw))


def test_pointwise_is_indexed_by_t(fake):
    import pyloo_amd as pl

    ll = lfo_ref.draw_ll(np.random.default_rng(24), 16, 64)
    res, _ = quiet(pl.loo_lfo_from_matrix, ll, 3, 4, pointwise=True)
    lfo_i, k = np.asarray(res["lfo_i"]), np.asarray(res["pareto_k"])
    assert lfo_i.shape == k.shape == (16,)
    assert np.all(np.isnan(lfo_i[:3])) and np.all(np.isnan(lfo_i[13:])) and np.all(np.isfinite(lfo_i[3:13]))
    assert np.all(np.isnan(k[:3])) and k[3] == 0.0 and np.all(np.isnan(k[13:]))
    assert lfo_i[3] == orc.lse(ll[3] + ll[4] + ll[5] + ll[6]) - np.log(64)


def test_the_two_warnings(fake):
    import pyloo_amd as pl

    ll = lfo_ref.draw_ll(np.random.default_rng(25), 30, 200, k_lo=0.9, k_hi=1.6)
    want = lfo_ref.lfo_walk(ll, 4, 1)
    n_high = int(np.sum(want["k"] > 0.7))
    assert n_high > 0
    res, msgs = quiet(pl.loo_lfo_from_matrix, ll, 4, 1, pointwise=True)
    hit = [m for m in msgs if K_TEXT in m]
    assert len(hit) == 1 and f"0.70 for {n_high} steps." in hit[0] and "observations" not in hit[0] and res["warning"]
    assert "There has been a warning" in str(res) and "(bad)" in str(res)
    calm, msgs = quiet(pl.loo_lfo_from_matrix, ll, 4, 1, k_threshold=np.inf)
    assert not msgs and not calm["warning"]
    bad = ll.copy()
    bad[7, 3] = np.nan
    bad[1, 0] = np.nan  # (before the first step: never read)
    res, msgs = quiet(pl.loo_lfo_from_matrix, bad, 4, 1, k_threshold=np.inf)
    assert msgs.count(NAN_TEXT) == 1


# ------------------------------------------------------------------------------------------------------------- the generated code
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_new_kernels_use_no_scratch_and_spill_no_scalars(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    lines = isa_stats.compile_isa(out=str(tmp_path / "lfo.s"), units=["pla_k_lfo.hip"])
    names = [k for k in isa_stats.all_kernels(lines) if "lfo_" in k]
    # scan: totals / ratios x 16-byte / element loads x two dtypes; carry; predict: two load modes x registers / streamed x two
    # dtypes; first-high
    assert len(names) == 8 + 1 + 8 + 1, names
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert not isa_stats.masked_spills(lines, k[2:]), name
        regs = res["NumVgprs"] + res.get("NumAgprs", 0)
        assert regs <= (256 if "lfo_predict" in k else 128), (name, res)
