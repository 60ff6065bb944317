"""Host side of ``loo_mixture`` without a GPU.  The first five tests check the YARDSTICK, not the product: the NumPy restatement of
the estimator (tests/mixis_ref.py) against hand-checkable cases and its own invariants -- they need none of the feature.  The rest
needs it: the front through an oracle-backed stand-in engine (index orders, warnings, errors, shapes, scales, the printed report
against the reference's text), ``loo(mixture=True)`` still refusing, the new C entry points' argument checks and the generated
code of the new kernels."""

import ctypes as C
import importlib
import os
import re
import sys
import warnings

import numpy as np
import pytest

import pyloo_amd as pl
from conftest import load_golden
from mixis_ref import clamp, draw_lse, mixis, reference_axis
from oracle import psis_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_BY_TWO = np.log(np.array([[1 / 2, 1 / 4], [1 / 8, 1 / 2]]))
INDEX = ["elpd_loo", "se", "n_samples", "n_data_points", "warning", "scale", "good_k", "subsample_size"]
INDEX_PW = ["elpd_loo", "se", "n_samples", "n_data_points", "warning", "loo_i", "scale", "pareto_k", "good_k", "subsample_size"]
MIX_TEXT = ("Mix-IS-LOO requires a model that is sampled from a mixture of leave-one-out posteriors. Ensure the inference data "
            "passed to the `loo` function comes from a model that is sampled from such a distribution.")
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."
SAME_TEXT = "The point-wise LOO is the same with the sum LOO"


class OracleMixisEngine:
    """Stand-in for ``Engine.mixis_draw_lse`` / ``Engine.mixis_loo`` on the restatement (test infrastructure: the product has no
    CPU path)."""

    device = "cpu-oracle"

    def mixis_draw_lse(self, ll):
        return {"c": draw_lse(ll), "n_replaced": clamp(ll)[1]}

    def mixis_loo(self, ll, c=None, scale_value=1.0, pointwise=True, aggregate=True):
        r = mixis(ll, scale_value, c)
        return {"loo_i": r["loo_i"], "c": r["c"], "agg": r["agg"]}


@pytest.fixture()
def fake(monkeypatch):
    eng = OracleMixisEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_mixture"), "get_engine", lambda device=None: eng)
    return eng


@pytest.fixture(scope="module")
def seeded():
    return np.random.default_rng(20221).normal(-1.5, 1.2, size=(37, 200))


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_two_by_two_case_and_the_reference_axis():
    got = mixis(TWO_BY_TWO)["elpd_i"]
    np.testing.assert_allclose(got, [np.log(4 / 13), np.log(4 / 17)], rtol=1e-14)
    assert got[0] != got[1]
    np.testing.assert_allclose(draw_lse(TWO_BY_TWO), [np.log(10), np.log(6)], rtol=1e-14)
    # the reference's lines reduce over the draws first: one constant for every observation
    np.testing.assert_allclose(reference_axis(TWO_BY_TWO), [np.log(4 / 15)] * 2, rtol=1e-14)


def test_single_observation_is_the_log_mean(seeded):
    row = seeded[:1]
    np.testing.assert_allclose(mixis(row)["elpd_i"][0], orc.lse(row[0], b_inv=row.shape[1]), rtol=1e-13)


def test_weights_sum_to_the_number_of_draws(seeded):
    r = mixis(seeded)
    np.testing.assert_allclose(np.sum(np.exp(-r["elpd_i"])) * np.sum(np.exp(-r["c"])), seeded.shape[1], rtol=1e-12)
    assert np.ptp(reference_axis(seeded)) < 1e-13 < np.ptp(r["elpd_i"])


def test_permutations(seeded):
    rng = np.random.default_rng(5)
    base = mixis(seeded)["elpd_i"]
    po, pd_ = rng.permutation(seeded.shape[0]), rng.permutation(seeded.shape[1])
    np.testing.assert_allclose(mixis(seeded[po])["elpd_i"], base[po], rtol=0, atol=1e-12)
    np.testing.assert_allclose(mixis(seeded[:, pd_])["elpd_i"], base, rtol=0, atol=1e-12)


def test_clamp_rule():
    x = np.array([[np.nan, 1.0, np.inf], [0.5, -np.inf, 2.0]], dtype=np.float32)
    got, counts = clamp(x)
    assert got.dtype == np.float64 and counts.tolist() == [1, 2]
    np.testing.assert_array_equal(got, [[-1e10, 1.0, 1e10], [0.5, -1e10, 2.0]])
    assert np.all(np.isfinite(mixis(x)["elpd_i"]))


# -------------------------------------------------------------------------------------------------------------------- the front
def test_from_matrix_index_orders_and_values(fake, seeded):
    res, msgs = quiet(pl.loo_mixture_from_matrix, seeded)
    assert list(res.index) == INDEX and msgs == [MIX_TEXT]
    pw, _ = quiet(pl.loo_mixture_from_matrix, seeded, pointwise=True)
    assert list(pw.index) == INDEX_PW
    want = mixis(seeded)
    np.testing.assert_allclose(np.asarray(pw["loo_i"]), want["loo_i"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(pw["elpd_loo"], want["loo_i"].sum(), rtol=1e-10)
    np.testing.assert_allclose(pw["se"], (37 * np.var(want["loo_i"])) ** 0.5, rtol=1e-8, atol=1e-9)
    assert res["elpd_loo"] == pw["elpd_loo"] and res["se"] == pw["se"]
    assert pw["warning"] is False and res["warning"] is False
    assert pw["n_samples"] == 200 and pw["n_data_points"] == 37 and pw["subsample_size"] == 37 and pw["scale"] == "log"
    assert pw["good_k"] == min(1 - 1 / np.log10(200), 0.7)
    np.testing.assert_array_equal(np.asarray(pw["pareto_k"]), np.zeros(37))
    assert "p_loo" not in pw and "looic" not in pw
    with pytest.raises(ValueError, match="2-D"):
        pl.loo_mixture_from_matrix(seeded[0])


def test_front_on_a_chain_draw_obs_grid(fake):
    rng = np.random.default_rng(9)
    ll = rng.normal(-1.0, 0.8, size=(2, 50, 3, 4))
    res, msgs = quiet(pl.loo_mixture, {"log_likelihood": {"y": ll}}, pointwise=True)
    assert list(res.index) == INDEX_PW and msgs == [MIX_TEXT] and res["warning"] is False
    matrix = np.moveaxis(ll.reshape(100, 3, 4), 0, -1).reshape(12, 100)
    want = mixis(matrix)
    assert np.asarray(res["loo_i"]).shape == (3, 4) and np.asarray(res["pareto_k"]).shape == (3, 4)
    np.testing.assert_allclose(np.asarray(res["loo_i"]).reshape(-1), want["loo_i"], rtol=1e-10, atol=1e-12)
    np.testing.assert_array_equal(np.asarray(res["pareto_k"]), np.zeros((3, 4)))
    if hasattr(res["loo_i"], "dims"):
        assert tuple(res["loo_i"].dims) == tuple(res["pareto_k"].dims) and len(res["loo_i"].dims) == 2
    assert res["n_samples"] == 100 and res["n_data_points"] == 12
    plain, _ = quiet(pl.loo_mixture, {"log_likelihood": {"y": ll}})
    assert list(plain.index) == INDEX and plain["elpd_loo"] == res["elpd_loo"]


@pytest.mark.parametrize("scale,value", [("log", 1.0), ("negative_log", -1.0), ("deviance", -2.0)])
def test_scales(fake, seeded, scale, value):
    res, _ = quiet(pl.loo_mixture_from_matrix, seeded, scale=scale, pointwise=True)
    want = value * mixis(seeded)["elpd_i"]
    assert res["scale"] == scale
    np.testing.assert_allclose(np.asarray(res["loo_i"]), want, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(res["elpd_loo"], want.sum(), rtol=1e-10)
    np.testing.assert_allclose(res["se"], (37 * np.var(want)) ** 0.5, rtol=1e-8, atol=1e-9)


def test_scale_type_error(fake, seeded):
    with pytest.raises(TypeError, match='Valid scale values are "deviance", "log", "negative_log"'):
        quiet(pl.loo_mixture_from_matrix, seeded, scale="bits")
    with pytest.raises(TypeError, match='Valid scale values are "deviance", "log", "negative_log"'):
        quiet(pl.loo_mixture, {"log_likelihood": {"y": seeded.T.reshape(2, 100, 37)}}, scale="bits")


def test_mixture_warning_is_issued_on_every_call(fake, seeded):
    for _ in range(2):
        with pytest.warns(UserWarning, match=re.escape(MIX_TEXT)):
            pl.loo_mixture_from_matrix(seeded)
    with pytest.warns(UserWarning, match=re.escape(MIX_TEXT)):
        pl.loo_mixture({"log_likelihood": {"y": np.ascontiguousarray(seeded.T).reshape(2, 100, 37)}})


def test_nan_warning_and_its_effect(fake, seeded):
    ll = seeded.copy()
    ll[3, 7] = np.nan
    res, msgs = quiet(pl.loo_mixture_from_matrix, ll, pointwise=True)
    assert msgs.count(NAN_TEXT) == 1 and MIX_TEXT in msgs
    filled = ll.copy()
    filled[3, 7] = -1e10
    np.testing.assert_allclose(np.asarray(res["loo_i"]), mixis(filled)["loo_i"], rtol=1e-10, atol=1e-12)
    assert np.all(np.isfinite(np.asarray(res["loo_i"])))
    data = {"log_likelihood": {"y": np.ascontiguousarray(ll.T).reshape(2, 100, 37)}}
    res2, msgs2 = quiet(pl.loo_mixture, data, pointwise=True)
    assert msgs2.count(NAN_TEXT) == 1
    np.testing.assert_allclose(np.asarray(res2["loo_i"]), np.asarray(res["loo_i"]), rtol=1e-12)
    _, clean = quiet(pl.loo_mixture_from_matrix, seeded)
    assert NAN_TEXT not in clean


def test_var_name_errors(fake, seeded):
    y = np.ascontiguousarray(seeded.T).reshape(2, 100, 37)
    with pytest.raises(TypeError, match="var_name cannot be None"):
        quiet(pl.loo_mixture, {"log_likelihood": {"y": y, "z": y}})
    with pytest.raises(TypeError, match="No log likelihood data named w found"):
        quiet(pl.loo_mixture, {"log_likelihood": {"y": y}}, var_name="w")
    res, _ = quiet(pl.loo_mixture, {"log_likelihood": {"y": y, "z": y + 1.0}}, var_name="y")
    np.testing.assert_allclose(res["elpd_loo"], mixis(seeded)["loo_i"].sum(), rtol=1e-10)


def test_identical_pointwise_warning(fake):
    ll = np.full((5, 40), -0.75)
    res, msgs = quiet(pl.loo_mixture_from_matrix, ll, pointwise=True)
    assert sum(SAME_TEXT in m for m in msgs) == 1
    np.testing.assert_allclose(np.asarray(res["loo_i"]), np.full(5, -0.75), rtol=1e-12)
    _, msgs = quiet(pl.loo_mixture_from_matrix, ll)
    assert not any(SAME_TEXT in m for m in msgs)


def test_rcparams_pointwise_default(fake, seeded):
    data = {"log_likelihood": {"y": np.ascontiguousarray(seeded.T).reshape(2, 100, 37)}}
    old = pl.rcParams["stats.ic_pointwise"]
    try:
        pl.rcParams["stats.ic_pointwise"] = True
        res, _ = quiet(pl.loo_mixture, data)
        assert list(res.index) == INDEX_PW
    finally:
        pl.rcParams["stats.ic_pointwise"] = old
    res, _ = quiet(pl.loo_mixture, data, pointwise=False)
    assert list(res.index) == INDEX


def test_report_text_is_the_reference_s():
    gold = load_golden("mixture_report")
    from pyloo_amd.elpd import ELPDData

    for name in ("plain", "pointwise", "deviance"):
        elpd, se, n_samples, n, _, good_k, pointwise = gold[f"args/{name}"]
        n_samples, n, pointwise = int(n_samples), int(n), bool(pointwise)
        data, index = [elpd, se, n_samples, n, False], ["elpd_loo", "se", "n_samples", "n_data_points", "warning"]
        if pointwise:
            data.append(np.full(n, elpd / n))
            index.append("loo_i")
        data.append(str(gold[f"scale/{name}"]))
        index.append("scale")
        if pointwise:
            data.append(np.zeros(n))
            index.append("pareto_k")
        res = ELPDData(data=data + [good_k, n], index=index + ["good_k", "subsample_size"])
        assert str(res) == str(gold[f"report/{name}"]) and repr(res) == str(res)
    assert "mixture posterior" in str(gold["report/plain"]) and "p_loo" not in str(gold["report/plain"])


def test_report_of_a_front_result(fake, seeded):
    res, _ = quiet(pl.loo_mixture_from_matrix, seeded, pointwise=True)
    text = str(res)
    assert text.startswith("\nComputed from 200 posterior samples and 37 observations log-likelihood matrix with\nmixture posterior.\n")
    assert f"elpd_loo   {res['elpd_loo']:<8.2f}    -" in text and "All Pareto k estimates are good (k < 0.6)" in text


def test_loo_with_mixture_true_still_refuses():
    ll = np.random.default_rng(0).normal(size=(2, 20, 4))
    with pytest.raises(NotImplementedError, match="loo_mixture"):
        pl.loo({"log_likelihood": {"y": ll}}, reff=1.0, mixture=True)


# ---------------------------------------------------------------------------------------------------------------- the C entry points
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd import _capi

    return _capi.load_library()


def test_new_symbols_and_argument_errors(lib):
    from pyloo_amd import _capi

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    for sym in ("pla_mixis_draw_lse", "pla_mixis_loo", "pla_engine_set_mixis_grid", "pla_mixis_tile_rows"):
        assert sym in _capi.SYMBOLS and hasattr(lib, sym)
        assert re.search(r"\bint " + sym + r"\(", header), sym
    assert lib.pla_abi_version() == 7
    a = np.zeros(8)
    P = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    HOST = _capi.PLA_HOST
    # (engine, ll, dtype, n_obs, n_draws, stride_obs, stride_draw, ...): every bad argument is a status, whatever the engine
    bad = [
        ((P(a), 0, 0, 2, 2, 1), b"n_obs"), ((P(a), 0, 2, 0, 2, 1), b"n_draws"), ((None, 0, 2, 2, 2, 1), b"NULL"),
        ((P(a), 7, 2, 2, 2, 1), b"dtype"), ((P(a), 0, 2, 2, -2, 1), b"strides"), ((P(a), 0, 2, 2, 2, 1), b"engine is NULL"),
    ]
    for args, text in bad:
        assert lib.pla_mixis_draw_lse(None, *args, HOST, None, P(a), None) == -1
        assert text in lib.pla_last_error(), (args, lib.pla_last_error())
        assert lib.pla_mixis_loo(None, *args, None, 1.0, HOST, None, P(a), P(a)) == -1
        assert text in lib.pla_last_error(), (args, lib.pla_last_error())
    assert lib.pla_mixis_loo(None, P(a), 0, 2, 2, 2, 1, None, 1.0, 5, None, P(a), P(a)) == -1
    assert b"mem_space" in lib.pla_last_error()
    assert lib.pla_engine_set_mixis_grid(None, 3) == -1 and b"engine is NULL" in lib.pla_last_error()


def test_tile_rows_rule(lib):
    assert lib.pla_mixis_tile_rows(0) == -1 and lib.pla_mixis_tile_rows(-5) == -1
    for n, want in ((1, 256), (256, 256), (257, 256), (128 * 256, 256), (128 * 256 + 1, 512), (100_000, 1024), (1 << 30, 1 << 23)):
        assert lib.pla_mixis_tile_rows(n) == want, n
        assert -(-n // want) <= 128  # the slab holds at most 128 partials per draw
    from pyloo_amd.engine import Engine

    assert Engine.mixis_tile_rows(5000) == 256
    with pytest.raises(Exception, match="n_obs"):
        Engine.mixis_tile_rows(0)


def test_mixis_kernel_resources():
    """Every kernel of pla_k_mixis.hip from the gfx950 code object's metadata and listing: no scratch, no register spilled, and an
    LDS size that lets two workgroups share a CU (the register-row kernel holds 32 KB of c and 8 KB of tables)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    assert "pla_k_mixis.hip" in isa_stats.KERNEL_UNITS and isa_stats.unit_of("mixis_col_kernelId") == ["pla_k_mixis.hip"]
    lines = isa_stats.compile_isa(units=["pla_k_mixis.hip"], out="/tmp/pla_isa_mixis.s")
    text = "\n".join(lines)
    blocks = re.split(r"\n\s+- \.", text[text.index("amdhsa.kernels"):])
    meta = {}
    for b in blocks:
        m = re.search(r"\.name:\s+(_ZN3pla\d+mixis_\S+)", b)
        if not m:
            continue
        vals = dict(re.findall(r"\.(vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", b))
        meta[m.group(1)] = {k: int(v) for k, v in vals.items()}
    # f64 and f32 x (tile unit, tile strided, line 16-byte, line element, row-wave 16-byte, row-wave element, stream 16-byte,
    # stream element, col, block) + merge, lse_c, counts
    assert len(meta) == 23, sorted(meta)
    for name, r in meta.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        _, total, _, res = isa_stats.kernel_stats(lines, name[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(k.startswith("scratch_") for k in total), (name, res)
        assert r["group_segment_fixed_size"] <= 81920, (name, r)
        if "mixis_row_wave_kernel" in name:
            assert r["group_segment_fixed_size"] == 40960 and r["vgpr_count"] <= 256 and res["Occupancy"] >= 2, (name, r, res)
