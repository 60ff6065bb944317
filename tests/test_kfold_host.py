"""Host side of ``loo_kfold`` without a GPU: the yardstick of the GPU task tests (tests/kfold_ref.py) against the goldens and the
oracle, the splitters against the reference's fold arrays, the front against the reference's
numbers through an oracle-backed stand-in engine, its errors and warnings, the ``ELPDData`` it builds and prints, ``loo_compare`` on
k-fold results, the two C entry points and the generated code of the new kernels."""

import ctypes as C
import importlib
import os
import re
import sys
import warnings

import numpy as np
import pytest

import pyloo_amd as pl
from oracle import psis_oracle as orc
from pyloo_amd._capi import AGG_COUNT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kfold.npz")
CASES = ("random", "ragged", "ragged_f32", "stratified", "stratified_binary", "grouped", "grouped_few", "loo_exact", "user_folds",
         "nan_full", "extreme")
INDEX = ["elpd_kfold", "se", "p_kfold", "p_kfold_se", "n_samples", "n_data_points", "warning", "kfold_i", "scale", "K", "kfoldic",
         "kfoldic_se", "stratified", "grouped"]


class OracleKfoldEngine:
    """Stand-in for ``Engine.kfold`` on the CPU oracle (test infrastructure: the product has no CPU path)."""

    device = "cpu-oracle"

    def kfold(self, ll_full, fold_log_liks, folds, scale_value=1.0, nan_flag=True):
        full = np.asarray(ll_full, dtype=np.float64)
        n = full.shape[0]
        folds = np.asarray(folds)
        nan = np.isnan(full)
        full = np.where(nan, -1e10, full) if nan_flag else full
        with np.errstate(all="ignore"):
            lpd = np.array([orc.lse(r, b_inv=full.shape[1]) for r in full], dtype=np.float64)
            elpd = np.zeros(n)
            for k, m in enumerate(fold_log_liks):
                idx = np.where(folds == k + 1)[0]
                m = np.asarray(m, dtype=np.float64)
                m = m[idx] if m.shape[0] == n else m
                elpd[idx] = [orc.lse(r, b_inv=m.shape[1]) for r in m]
            p_i, kfold_i = lpd - elpd, scale_value * elpd
            agg = np.zeros(AGG_COUNT)
            agg[:6] = [n, kfold_i.sum(), np.sum((kfold_i - kfold_i.mean()) ** 2), p_i.sum(), np.sum((p_i - p_i.mean()) ** 2),
                       nan.sum() if nan_flag else 0]
        return {"elpd_i": elpd, "lpd_full_i": lpd, "p_i": p_i, "kfold_i": kfold_i, "agg": agg}


@pytest.fixture()
def fake(monkeypatch):
    eng = OracleKfoldEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_kfold"), "get_engine", lambda device=None: eng)
    return eng


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def case_inputs(gold, case):
    K = int(gold[f"{case}/K"])
    return gold[f"{case}/ll_full"], [gold[f"{case}/fold_{k + 1}"] for k in range(K)], gold[f"{case}/folds"], str(gold[f"{case}/scale"])


# ------------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("case", CASES)
def test_lme_ref_against_goldens_and_oracle(gold, case):
    """tests/kfold_ref.py (the yardstick of tests/test_gpu_kfold_tasks.py) on every golden case: against the reference's stored
    vectors and against the oracle on the f64 widening, at the project's log-mean-exp tolerances, NaN in the same places."""
    from kfold_ref import lme_ref

    full, mats, folds, _ = case_inputs(gold, case)
    n = full.shape[0]
    lpd, n_rep = lme_ref(full, nan_fix=True)
    assert n_rep.sum() == int(gold[f"{case}/n_nan"]) == np.isnan(full).sum()
    elpd = np.zeros(n)
    held = [None] * n  # observation i's row under the fit that left it out
    for k, m in enumerate(mats):
        idx = np.where(folds == k + 1)[0]
        rows = m[idx] if m.shape[0] == n else m
        elpd[idx], n_rep = lme_ref(rows, nan_fix=False)
        assert n_rep.sum() == 0
        for i, r in zip(idx, rows):
            held[i] = r
    with np.errstate(all="ignore"):
        o_lpd = np.array([orc.lse(np.where(np.isnan(r), -1e10, r).astype(np.float64), b_inv=r.size) for r in full])
        o_elpd = np.array([orc.lse(r.astype(np.float64), b_inv=r.size) for r in held])
    for got, stored, oracle in ((lpd, gold[f"{case}/lpd_full"], o_lpd), (elpd, gold[f"{case}/elpd"], o_elpd)):
        for want in (stored, oracle):
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
            np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12, equal_nan=True)
    # without the flag a NaN of the full fit stays
    raw, n_rep = lme_ref(full, nan_fix=False)
    assert n_rep.sum() == 0
    np.testing.assert_array_equal(np.isnan(raw), np.isnan(full).any(axis=1) | np.isnan(lpd))


# ------------------------------------------------------------------------------------------------------------------ the splitters
def test_splitters_give_the_reference_folds(gold):
    for K, N, seed in ((5, 23, 7), (10, 100, 0), (3, 3, 1)):
        np.testing.assert_array_equal(pl.kfold_split_random(K, N, seed=seed), gold[f"split/random_{K}_{N}_{seed}"])
    for name in ("continuous", "discrete", "string"):
        got = pl.kfold_split_stratified(4, gold[f"split/stratified_{name}_x"], seed=13)
        np.testing.assert_array_equal(got, gold[f"split/stratified_{name}"])
    with pytest.warns(UserWarning, match="Only 1 unique value in stratification variable, using random folds instead"):
        got = pl.kfold_split_stratified(4, gold["split/stratified_single_x"], seed=13)
    np.testing.assert_array_equal(got, gold["split/stratified_single"])
    np.testing.assert_array_equal(pl.kfold_split_grouped(3, gold["split/grouped_groups"], seed=21), gold["split/grouped"])
    # the folds of the golden cases come from the reference's splitters too
    np.testing.assert_array_equal(pl.kfold_split_random(5, 60, seed=11), gold["random/folds"])
    np.testing.assert_array_equal(pl.kfold_split_stratified(3, gold["stratified/x"], seed=5), gold["stratified/folds"])
    np.testing.assert_array_equal(pl.kfold_split_stratified(3, gold["stratified_binary/x"], seed=6), gold["stratified_binary/folds"])
    np.testing.assert_array_equal(pl.kfold_split_grouped(4, gold["grouped/groups"], seed=8), gold["grouped/folds"])
    with pytest.warns(UserWarning, match=r"Number of groups \(3\) is less than K \(5\). Setting K=3"):
        got = pl.kfold_split_grouped(5, gold["grouped_few/groups"], seed=9)
    np.testing.assert_array_equal(got, gold["grouped_few/folds"])
    assert set(got) == {1, 2, 3}


def test_splitter_errors():
    with pytest.raises(ValueError, match="K must be > 1 for stratified folds, got 1"):
        pl.kfold_split_stratified(1, np.arange(5.0))
    with pytest.raises(ValueError, match="Stratification variable contains NaN values"):
        pl.kfold_split_stratified(2, np.array([0.0, np.nan, 1.0]))
    with pytest.warns(UserWarning, match="Setting K=1"), pytest.raises(ValueError, match="K must be > 1 for group-based folds, got 1"):
        pl.kfold_split_grouped(3, np.zeros(6, dtype=int))


# --------------------------------------------------------------------------------------------------- the front against the goldens
@pytest.mark.parametrize("case", CASES)
def test_from_matrix_against_reference(fake, gold, case):
    full, mats, folds, scale = case_inputs(gold, case)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_kfold_from_matrix(full, mats, folds, pointwise=True, scale=scale)
    nan_warned = [w for w in rec if "NaN values detected in log-likelihood" in str(w.message)]
    assert len(nan_warned) == (1 if int(gold[f"{case}/n_nan"]) else 0)
    assert list(res.index) == INDEX
    np.testing.assert_allclose(np.asarray(res["kfold_i"]), gold[f"{case}/kfold_i"], rtol=1e-10, atol=1e-12, equal_nan=True)
    want = gold[f"{case}/stats"]
    got = [res["elpd_kfold"], res["se"], res["p_kfold"], res["p_kfold_se"], res["kfoldic"], res["kfoldic_se"]]
    np.testing.assert_allclose(got[0::2], want[0::2], rtol=1e-10, equal_nan=True)
    np.testing.assert_allclose(got[1::2], want[1::2], rtol=1e-8, atol=1e-9, equal_nan=True)
    assert res["n_samples"] == full.shape[1] and res["n_data_points"] == full.shape[0] and res["warning"] is False
    assert res["scale"] == scale and res["K"] == res.K == int(gold[f"{case}/K"]) and res.method == "kfold"
    assert res["stratified"] is False and res["grouped"] is False


def test_full_form_and_mixed_forms_equal_compact(fake, gold):
    full, mats, folds, scale = case_inputs(gold, "ragged")
    want = pl.loo_kfold_from_matrix(full, mats, folds, pointwise=True, scale=scale)
    rng = np.random.default_rng(1)
    wide = []
    for k, m in enumerate(mats):
        w = rng.normal(size=(full.shape[0], m.shape[1]))  # the other rows hold anything: they are not held out
        w[folds == k + 1] = m
        wide.append(w)
    for forms in (wide, [wide[0], mats[1], wide[2], mats[3]]):
        got = pl.loo_kfold_from_matrix(full, forms, folds, pointwise=True, scale=scale)
        np.testing.assert_array_equal(np.asarray(got["kfold_i"]), np.asarray(want["kfold_i"]))
        assert got["elpd_kfold"] == want["elpd_kfold"]


def test_index_without_pointwise_and_with_fits(fake, gold):
    full, mats, folds, scale = case_inputs(gold, "random")
    res = pl.loo_kfold_from_matrix(full, mats, folds, pointwise=False)
    assert list(res.index) == [k for k in INDEX if k != "kfold_i"]
    data = {"log_likelihood": {"y": full.T.reshape(2, 128, 60)}}  # (chain, draw, obs)
    res = pl.loo_kfold(data, fold_log_likelihoods=mats, folds=folds, pointwise=True, save_fits=True)
    assert list(res.index) == INDEX + ["fits"]
    assert len(res["fits"]) == 5 and all(np.array_equal(v, np.where(folds == k + 1)[0]) for k, (_, v) in enumerate(res["fits"]))
    np.testing.assert_allclose(res["elpd_kfold"], gold["random/stats"][0], rtol=1e-10)
    assert res["n_samples"] == 256


# ------------------------------------------------------------------------------------------------------------------------ loo_kfold
def prepared(gold, case="random"):
    full, mats, folds, scale = case_inputs(gold, case)
    n, s = full.shape
    return {"log_likelihood": {"y": np.ascontiguousarray(full.T).reshape(2, s // 2, n)}}, full, mats, folds, scale


def test_fit_fold_is_called_per_fold_in_order(fake, gold):
    data, full, mats, _, _ = prepared(gold)
    calls = []

    def fit_fold(train_idx, val_idx, tag=None):
        k = len(calls)
        calls.append((train_idx.copy(), val_idx.copy(), tag))
        # a dict as loo() accepts it: (chain, draw, obs) of the held-out observations
        return {"log_likelihood": {"y": np.ascontiguousarray(mats[k].T).reshape(1, mats[k].shape[1], mats[k].shape[0])}}

    res = pl.loo_kfold(data, fit_fold, K=5, random_seed=11, pointwise=True, save_fits=True, tag="kw")
    folds = gold["random/folds"]  # K = 5, seed 11: the reference's folds
    assert len(calls) == 5
    for k, (tr, va, tag) in enumerate(calls):
        np.testing.assert_array_equal(va, np.where(folds == k + 1)[0])
        np.testing.assert_array_equal(tr, np.where(folds != k + 1)[0])
        assert tag == "kw"
    np.testing.assert_allclose(np.asarray(res["kfold_i"]).ravel(), gold["random/kfold_i"], rtol=1e-10, atol=1e-12)
    assert [f[0] is not None for f in res["fits"]] == [True] * 5 and res["stratified"] is False and res["grouped"] is False
    direct = pl.loo_kfold_from_matrix(full, mats, folds, pointwise=True)
    np.testing.assert_array_equal(np.asarray(res["kfold_i"]).ravel(), np.asarray(direct["kfold_i"]))


def test_fit_fold_exception_propagates(fake, gold):
    data = prepared(gold)[0]

    def broken(train_idx, val_idx):
        raise RuntimeError("sampler diverged")

    with pytest.raises(RuntimeError, match="sampler diverged"):
        pl.loo_kfold(data, broken, K=3, random_seed=1)


def test_stratify_groups_and_flags(fake, gold):
    data, full, mats, folds, _ = prepared(gold, "stratified")
    res = pl.loo_kfold(data, fold_log_likelihoods=mats, K=3, stratify=gold["stratified/x"], random_seed=5, pointwise=True)
    assert res["stratified"] is True and res.stratified is True and res["grouped"] is False
    np.testing.assert_allclose(res["elpd_kfold"], gold["stratified/stats"][0], rtol=1e-10)
    data, full, mats, folds, _ = prepared(gold, "grouped")
    # groups come before stratify (loo_kfold.py:443-472): the folds are the grouped ones
    res = pl.loo_kfold(data, fold_log_likelihoods=mats, K=4, groups=gold["grouped/groups"], stratify=np.arange(36) % 2, random_seed=8)
    assert res["grouped"] is True and res.grouped is True
    np.testing.assert_allclose(res["elpd_kfold"], gold["grouped/stats"][0], rtol=1e-10)
    data, full, mats, folds, _ = prepared(gold, "grouped_few")
    with pytest.warns(UserWarning, match="Setting K=3"):
        res = pl.loo_kfold(data, fold_log_likelihoods=mats, K=5, groups=gold["grouped_few/groups"], random_seed=9)
    assert res["K"] == 3
    np.testing.assert_allclose(res["elpd_kfold"], gold["grouped_few/stats"][0], rtol=1e-10)
    # folds override stratify, with a warning; the result is not "stratified" then
    data, full, mats, folds, _ = prepared(gold, "stratified")
    with pytest.warns(UserWarning, match="Both folds and stratify were provided. Using the provided folds and ignoring stratify."):
        res = pl.loo_kfold(data, fold_log_likelihoods=mats, folds=folds, stratify=gold["stratified/x"])
    assert res["stratified"] is False


def test_errors_with_their_messages(fake, gold):
    data, full, mats, folds, _ = prepared(gold)
    fit = lambda tr, va: None  # noqa: E731
    with pytest.raises(ValueError, match="exactly one of fit_fold and fold_log_likelihoods"):
        pl.loo_kfold(data)
    with pytest.raises(ValueError, match="exactly one of fit_fold and fold_log_likelihoods"):
        pl.loo_kfold(data, fit, fold_log_likelihoods=mats)
    with pytest.raises(ValueError, match="K must be positive, got 0"):
        pl.loo_kfold(data, fit, K=0)
    with pytest.raises(ValueError, match=r"Length of folds \(59\) must match observations \(60\)"):
        pl.loo_kfold(data, fit, folds=folds[:-1])
    with pytest.raises(ValueError, match="Need at least 2 unique fold values, got 1"):
        pl.loo_kfold(data, fit, folds=np.ones(60, dtype=int))
    with pytest.raises(ValueError, match="Fold indices must be >= 1"):
        pl.loo_kfold(data, fit, folds=folds - 1)
    with pytest.raises(ValueError, match=r"Fold indices must be the integers 1\.\.K"):
        pl.loo_kfold(data, fit, folds=np.where(folds == 5, 7, folds))
    with pytest.raises(ValueError, match=r"Length of groups \(3\) must match observations \(60\)"):
        pl.loo_kfold(data, fit, groups=[1, 2, 3])
    with pytest.raises(ValueError, match=r"Length of stratify \(3\) must match observations \(60\)"):
        pl.loo_kfold(data, fit, stratify=[1, 2, 3])
    with pytest.raises(ValueError, match="Scale must be 'log', 'negative_log', or 'deviance'"):
        pl.loo_kfold(data, fit, scale="bits")
    with pytest.raises(ValueError, match="Expected 5 fold log-likelihoods, got 4"):
        pl.loo_kfold(data, fold_log_likelihoods=mats[:4], folds=folds)
    # the matrix front
    with pytest.raises(ValueError, match=r"Fold indices must be the integers 1\.\.K"):
        pl.loo_kfold_from_matrix(full, mats, np.where(folds == 2, 9, folds))
    with pytest.raises(ValueError, match=r"Fold indices must be the integers 1\.\.K"):
        pl.loo_kfold_from_matrix(full, mats, folds + 0.5)
    with pytest.raises(ValueError, match=r"Length of folds \(59\) must match observations \(60\)"):
        pl.loo_kfold_from_matrix(full, mats, folds[:-1])
    with pytest.raises(ValueError, match="Need at least 2 folds, got 1"):
        pl.loo_kfold_from_matrix(full, mats[:1], np.ones(60, dtype=int))
    with pytest.raises(TypeError, match="must share one dtype"):
        pl.loo_kfold_from_matrix(full, [mats[0].astype(np.float32)] + mats[1:], folds)
    with pytest.raises(ValueError, match=r"Fold 1: expected a \(12, S\) or \(60, S\) log-likelihood matrix, got \(11, 256\)"):
        pl.loo_kfold_from_matrix(full, [mats[0][:-1]] + mats[1:], folds)


def test_k_larger_than_n_warns_and_becomes_n(fake, gold):
    data, full, mats, folds, _ = prepared(gold, "loo_exact")
    with pytest.warns(UserWarning, match=r"K \(40\) is greater than N \(12\), setting K=N"):
        res = pl.loo_kfold(data, fold_log_likelihoods=mats, K=40, random_seed=2)
    assert res["K"] == 12
    np.testing.assert_allclose(res["elpd_kfold"], gold["loo_exact/stats"][0], rtol=1e-10)


# ------------------------------------------------------------------------------------------------------------- report and compare
def test_printed_report_is_the_references(fake, gold):
    full, mats, folds, scale = case_inputs(gold, "random")
    assert str(pl.loo_kfold_from_matrix(full, mats, folds, pointwise=True)) == str(gold["report/random"])
    data, full, mats, folds, _ = prepared(gold, "stratified")
    res = pl.loo_kfold(data, fold_log_likelihoods=mats, K=3, stratify=gold["stratified/x"], random_seed=5)
    assert str(res) == str(gold["report/stratified"]) and "Using stratified k-fold cross-validation" in repr(res)
    assert "5-fold cross-validation\nwith 60 observations." in str(gold["report/random"])


def test_loo_compare_ranks_kfold_results(fake, gold, monkeypatch):
    full, mats, folds, _ = case_inputs(gold, "random")
    a = pl.loo_kfold_from_matrix(full, mats, folds, pointwise=True)
    worse = [m - 0.25 - 0.01 * np.arange(m.shape[0])[:, None] for m in mats]
    b = pl.loo_kfold_from_matrix(full, worse, folds, pointwise=True)

    class Moments:  # loo_compare's engine call (pla_compare_moments) in NumPy
        def compare_moments(self, x, best):
            x = np.asarray(x)
            d = x - x[best]
            return np.concatenate([np.stack([x.sum(1), d.mean(1), ((d - d.mean(1, keepdims=True)) ** 2).sum(1)], 1).ravel(), [x.max(0).sum()]])

    monkeypatch.setattr(importlib.import_module("pyloo_amd.compare"), "get_engine", lambda device=None: Moments())
    table = pl.loo_compare({"worse": b, "better": a}, ic="kfold", method="pseudo-BMA")
    assert list(table.index) == ["better", "worse"] and list(table["rank"]) == [0, 1]
    assert "elpd_kfold" in table.columns and "p_kfold" in table.columns
    ka, kb = np.asarray(a["kfold_i"]), np.asarray(b["kfold_i"])
    np.testing.assert_allclose(table.loc["worse", "elpd_diff"], b["elpd_kfold"] - a["elpd_kfold"], rtol=1e-10)  # compare.py:214-216
    np.testing.assert_allclose(table.loc["worse", "dse"], np.sqrt(60 * np.var(kb - ka)), rtol=1e-8)
    np.testing.assert_allclose(table.loc["better", "elpd_kfold"], gold["random/stats"][0], rtol=1e-10)
    np.testing.assert_allclose(table.loc["worse", "p_kfold"], b["p_kfold"], rtol=1e-12)
    with pytest.raises(NotImplementedError, match="kfold"):
        pl.loo_compare({"m": {"log_likelihood": {"y": np.zeros((1, 4, 3))}}, "n": {"log_likelihood": {"y": np.zeros((1, 4, 3))}}}, ic="kfold")


# ---------------------------------------------------------------------------------------------------------------- C entry points
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (as tests/test_capi_abi.py: a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


def test_new_symbols_and_null_engine(lib):
    from pyloo_amd import _capi

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    for sym in ("pla_kfold_lme", "pla_kfold_reduce"):
        assert sym in _capi.SYMBOLS and hasattr(lib, sym)
        assert re.search(r"\bint " + sym + r"\(", header), sym
    assert lib.pla_abi_version() == 7
    a = np.zeros(4, dtype=np.int64)
    P = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.pla_kfold_lme(None, P(a), P(a), P(a), P(a), P(a), 1, 0, 1, P(a), P(a), P(a), 1, _capi.PLA_DEVICE, None, P(a), 1, None) == -1
    assert b"engine is NULL" in lib.pla_last_error()
    assert lib.pla_kfold_reduce(None, P(a), P(a), 4, 1.0, None, _capi.PLA_DEVICE, None, None, None, P(a)) == -1
    assert b"engine is NULL" in lib.pla_last_error()


def test_kfold_kernel_resources(lib):
    """Every kernel of pla_k_kfold.hip from the gfx950 code object's metadata and listing: no scratch, no vector or scalar
    register spilled, nothing written to a vector lane under an execution mask; the wave kernels keep two waves per SIMD and
    their 8 KB of tables leave room for eight workgroups per CU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    assert "pla_k_kfold.hip" in isa_stats.KERNEL_UNITS and isa_stats.unit_of("kfold_wave_kernelId") == ["pla_k_kfold.hip"]
    lines = isa_stats.compile_isa(units=["pla_k_kfold.hip"], out="/tmp/pla_isa_kfold.s")
    text = "\n".join(lines)
    blocks = re.split(r"\n\s+- \.", text[text.index("amdhsa.kernels"):])
    meta = {}
    for b in blocks:
        m = re.search(r"\.name:\s+(_ZN3pla\d+kfold_\S+)", b)
        if not m:
            continue
        vals = dict(re.findall(r"\.(vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", b))
        meta[m.group(1)] = {k: int(v) for k, v in vals.items()}
    # f64 and f32 x (wave, lane, block), the two tile passes and the final kernel
    assert len(meta) == 9, sorted(meta)
    for name, r in meta.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        _, total, _, res = isa_stats.kernel_stats(lines, name[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(k.startswith("scratch_") for k in total), (name, res)
        assert total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert isa_stats.masked_spills(lines, name[2:]) == []
        if "kfold_wave_kernel" in name:
            assert r["vgpr_count"] <= 256 and res["Occupancy"] >= 2 and r["group_segment_fixed_size"] == 8192, (name, r, res)
