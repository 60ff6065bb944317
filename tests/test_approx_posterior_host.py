"""``loo_approximate_posterior`` without a GPU: the front against the reference's numbers (tests/golden/approx_posterior.npz) with
the recorded draw index through a stand-in engine, warning texts and their order, the ELPDData layout, the two documented
fall-backs, argument errors, the three new C symbols and the gather kernel's resources from the gfx950 ISA."""

import ctypes as C
import importlib
import os
import re
import sys
import warnings

import numpy as np
import pytest

from fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = {0: "psis", 1: "sis", 2: "tis"}
SCALES = {1: "log", -1: "negative_log", -2: "deviance"}
CASES = ["psis_psis", "psir_psis", "nonfinite", "sis_sis", "psis_tis", "psir_tis", "sis_psis", "psir_sis", "f32", "nan", "heavy",
         "psis_sis", "sis_tis", "heavy_sis", "heavy_tis"]


class DrawsOracleEngine(OracleEngine):
    """Stand-in for the engine's draw calls: NumPy's gather (NaN -> -1e10 in the input dtype, counted), then the oracle pass."""

    def gather_draws(self, ll, draw_index):
        g = np.asarray(ll)[:, np.asarray(draw_index)]
        nan = np.isnan(g)
        return np.where(nan, g.dtype.type(-1e10), g), int(nan.sum())

    def psis_loo_draws(self, ll, draw_index, tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True):
        g, nrep = self.gather_draws(ll, draw_index)
        res = self.psis_loo(g.astype(np.float64), tail_count, method, scale_value, good_k)
        return dict(res, n_replaced=nrep)


@pytest.fixture
def fake(monkeypatch):
    eng = DrawsOracleEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_approximate_posterior"), "get_engine", lambda device=None: eng)
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_subsample"), "get_engine", lambda device=None: eng)
    return eng


@pytest.fixture(scope="module")
def gold(golden):
    return golden("approx_posterior")


def case(z, name):
    reff, m, sv = z[f"{name}__meta"]
    return z[f"{name}__ll"], z[f"{name}__idx"], float(reff), METHODS[int(m)], SCALES[int(sv)]


def as_data(ll):
    from pyloo_amd.utils import SimpleInferenceData

    arr = np.ascontiguousarray(ll.T).reshape(1, ll.shape[1], ll.shape[0])  # one chain: (chain, draw, obs)
    return SimpleInferenceData(log_likelihood={"obs": arr}, posterior={"mu": np.zeros((1, ll.shape[1]))})


def recorded_index(monkeypatch, idx):
    """The front resamples with the index the reference's own importance_resample returned for this case."""
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_approximate_posterior"), "importance_resample",
                        lambda log_p, log_q, method="psis", seed=None: idx)


def texts(rec):
    return [str(w.message) for w in rec]


NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."


def expected_warnings(z, name):
    method = case(z, name)[3]
    p = f"{name}__"
    out = []
    if bool(z[p + "has_nan"]):
        out.append(NAN_TEXT)
    if method != "psis":
        out.append(f"Using {method.upper()} for LOO computation. Note that PSIS is the recommended method as it is typically more "
                   "efficient and reliable.")
    if method == "psis" and bool(z[p + "warning"]):
        gk = float(z[p + "good_k"])
        out.append(f"Estimated shape parameter of Pareto distribution is greater than {gk:.2f} for {int(z[p + 'n_high'])} observations. "
                   "This indicates that importance sampling may be unreliable because the marginal posterior and LOO posterior are "
                   "very different.")
    if method != "psis" and bool(z[p + "warning"]):
        out.append(f"Low effective sample size detected (minimum ESS: {float(z[p + 'min_diag']):.1f}). This indicates that the "
                   "importance sampling approximation may be unreliable. Consider using PSIS which is more robust to such cases.")
    return out


def check_result(res, z, name, pointwise):
    p = f"{name}__"
    ll, _, _, method, scale = case(z, name)
    for key in ("elpd_loo", "looic"):
        np.testing.assert_allclose(res[key], z[p + key], rtol=1e-9, err_msg=key)
    np.testing.assert_allclose(res["p_loo"], z[p + "p_loo"], rtol=1e-8, atol=1e-6, err_msg="p_loo")  # (a difference near zero)
    for key in ("se", "p_loo_se", "looic_se"):
        np.testing.assert_allclose(res[key], z[p + key], rtol=1e-8, err_msg=key)
    assert res["n_samples"] == ll.shape[1] and res["n_data_points"] == ll.shape[0] and res["scale"] == scale
    assert bool(res["warning"]) == bool(z[p + "warning"])
    head = ["elpd_loo", "se", "p_loo", "p_loo_se", "n_samples", "n_data_points", "warning"]
    if pointwise:
        tail = ["pareto_k", "good_k"] if method == "psis" else ["ess"]
        assert list(res.index) == head + ["loo_i", "scale", "looic", "looic_se"] + tail
        np.testing.assert_allclose(np.asarray(getattr(res["loo_i"], "values", res["loo_i"])), z[p + "loo_i"], rtol=1e-9, atol=1e-10)
        diag = res["pareto_k" if method == "psis" else "ess"]
        np.testing.assert_allclose(np.asarray(getattr(diag, "values", diag)), z[p + "diag"], rtol=1e-9, atol=1e-10)
    else:
        assert list(res.index) == head + ["scale", "looic", "looic_se"] + (["good_k"] if method == "psis" else [])
    if method == "psis":
        assert res["good_k"] == pytest.approx(float(z[p + "good_k"]), rel=1e-15)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("pointwise", [True, False])
def test_front_against_reference(fake, gold, monkeypatch, name, pointwise):
    import pyloo_amd as pl

    ll, idx, reff, method, scale = case(gold, name)
    recorded_index(monkeypatch, idx)
    log_p, log_q = gold[f"{name}__log_p"], gold[f"{name}__log_q"]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_approximate_posterior(as_data(ll), log_p, log_q, pointwise=pointwise, reff=reff, scale=scale, method=method,
                                           resample_method=str(gold[f"{name}__resample"]), seed=int(gold[f"{name}__seed"]))
    assert texts(rec) == expected_warnings(gold, name)
    check_result(res, gold, name, pointwise)
    assert set(res.approximate_posterior) == {"log_p", "log_q"}
    assert res.approximate_posterior["log_p"] is log_p and res.approximate_posterior["log_q"] is log_q


@pytest.mark.parametrize("name", CASES)
def test_from_matrix_against_reference(fake, gold, name):
    import pyloo_amd as pl

    ll, idx, reff, method, scale = case(gold, name)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_approximate_posterior_from_matrix(ll, idx, reff=reff, scale=scale, method=method, pointwise=True)
    assert texts(rec) == expected_warnings(gold, name)
    check_result(res, gold, name, True)


def test_resampling_failure_falls_back_to_the_original_draws(fake, gold):
    """Non-finite ratios (resample.npz's case): the reference's warning, then the fall-back it announces -- the plain pass."""
    import pyloo_amd as pl

    name = "nonfinite"
    assert bool(gold[f"{name}__fallback"])
    ll, idx, reff, method, scale = case(gold, name)
    assert np.array_equal(idx, np.arange(ll.shape[1]))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_approximate_posterior(as_data(ll), gold[f"{name}__log_p"], gold[f"{name}__log_q"], pointwise=True, reff=reff,
                                           scale=scale, method=method, resample_method="psis", seed=int(gold[f"{name}__seed"]))
    t = texts(rec)
    assert t[0] == "Found 3 non-finite importance weights. These will be excluded."
    assert t[-1].startswith("Importance resampling failed: ") and t[-1].endswith(". Falling back to original samples.")
    check_result(res, gold, name, True)


@pytest.mark.parametrize("bad,message", [
    (np.arange(1999), "Importance resampling failed: cannot reshape array of size 1999 into shape (2000,). Falling back to original samples."),
    (np.r_[np.arange(1999), 2000], "Importance resampling failed: index 2000 is out of bounds for axis 0 with size 2000. Falling back to "
                                   "original samples."),
])
def test_bad_index_falls_back_like_loo_subsample(fake, gold, monkeypatch, bad, message):
    import pyloo_amd as pl

    ll, idx, reff, method, scale = case(gold, "psis_psis")
    recorded_index(monkeypatch, bad)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_approximate_posterior(as_data(ll), gold["psis_psis__log_p"], gold["psis_psis__log_q"], pointwise=True, reff=reff)
    assert texts(rec) == [message]
    M = pl.loo_approximate_posterior.__globals__["tail_count_for"](ll.shape[1], reff)
    plain = fake.psis_loo(ll, M, "psis", 1.0, float(res["good_k"]))
    assert np.array_equal(np.asarray(getattr(res["loo_i"], "values", res["loo_i"])), plain["loo_i"])


def test_argument_errors(fake, gold):
    import pyloo_amd as pl

    ll, idx, *_ = case(gold, "psir_tis")
    log_p, log_q = gold["psir_tis__log_p"], gold["psir_tis__log_q"]
    with pytest.raises(ValueError, match=r"^log_p and log_q must have the same length, got 100 and 99$"):
        pl.loo_approximate_posterior(as_data(ll), log_p, log_q[:-1], reff=1.0)
    with pytest.raises(TypeError, match='Valid scale values are "deviance", "log", "negative_log"'):
        pl.loo_approximate_posterior(as_data(ll), log_p, log_q, reff=1.0, scale="bits")
    with pytest.raises(ValueError, match=r"Invalid method 'mix'\. Must be one of: psis, sis, tis"):
        pl.loo_approximate_posterior(as_data(ll), log_p, log_q, reff=1.0, method="mix")
    with pytest.raises(TypeError, match="Must be able to extract a posterior group from data."):
        pl.loo_approximate_posterior({"log_likelihood": {"obs": np.ascontiguousarray(ll.T).reshape(1, 100, 40)}}, log_p, log_q)
    # one chain: reff=None is 1.0 without ArviZ
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = pl.loo_approximate_posterior(as_data(ll), log_p, log_q, seed=3)
        b = pl.loo_approximate_posterior(as_data(ll), log_p, log_q, seed=3, reff=1.0)
    assert a["elpd_loo"] == b["elpd_loo"]


def test_pointwise_same_warning_comes_last(fake, monkeypatch):
    import pyloo_amd as pl

    rng = np.random.default_rng(1)
    ll = np.tile(-rng.exponential(size=(1, 200)), (5, 1))  # every observation the same row
    recorded_index(monkeypatch, rng.permutation(200))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        pl.loo_approximate_posterior(as_data(ll), np.zeros(200), np.zeros(200), pointwise=True, reff=1.0, method="sis")
    t = texts(rec)
    assert t[0].startswith("Using SIS for LOO computation.")
    assert t[-1] == ("The point-wise LOO is the same with the sum LOO, please double check the Observed RV in your model to make sure "
                     "it returns element-wise logp.")


def test_host_index_is_range_checked():
    from pyloo_amd.engine import Engine

    assert Engine._host_draws([3, 0, 3], 4).dtype == np.int64
    for bad in ([0, 4], [-1, 2]):
        with pytest.raises(IndexError, match=r"draw indices must lie in \[0, 4\)"):
            Engine._host_draws(bad, 4)
    with pytest.raises(ValueError, match="empty"):
        Engine._host_draws([], 4)


# ---------------------------------------------------------------------------------------------------- C entry points
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (as tests/test_capi_abi.py: a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


def test_new_symbols_and_null_engine(lib):
    from pyloo_amd import _capi

    for sym in ("pla_gather_draws", "pla_psis_loo_draws", "pla_gather_lds_max_draws"):
        assert sym in _capi.SYMBOLS and hasattr(lib, sym)
    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    for sym in ("pla_gather_draws", "pla_psis_loo_draws", "pla_gather_lds_max_draws"):
        assert re.search(r"\bint " + sym + r"\(", header), sym
    assert lib.pla_abi_version() == 7
    f64, f32 = lib.pla_gather_lds_max_draws(_capi.PLA_F64), lib.pla_gather_lds_max_draws(_capi.PLA_F32)
    assert f32 == 2 * f64 and 4096 < f64 and 2 * 8 * f64 <= 160 * 1024  # two workgroups' rows in a CU's 160 KB of LDS
    ll = np.zeros((4, 16))
    idx = np.array([0, 5, 5, 15], dtype=np.int64)
    out = np.zeros((4, 4))
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.pla_gather_draws(None, P(ll), 0, 4, 16, 16, 1, P(idx), 4, _capi.PLA_HOST, None, P(out), None) == -1
    assert b"engine is NULL" in lib.pla_last_error()
    assert lib.pla_psis_loo_draws(None, P(ll), 0, 4, 16, 16, 1, P(idx), 4, 0, 1, 1.0, 0.7, _capi.PLA_HOST, None, None, None, None, None,
                                  None) == -1
    assert b"engine is NULL" in lib.pla_last_error()


def test_gather_kernel_resources(lib):
    """Every instantiation of gather_draws_kernel from the gfx950 ISA: no scratch, no spills; the bound pla_gather_lds_max_draws
    exports is 80 KB of row per workgroup (two workgroups in a CU's 160 KB).  The LDS routes allocate their row (+ index)
    dynamically, which no listing shows: the routes the launcher picks around that bound are pinned on the GPU
    (tests/test_gpu_approx_posterior.py::test_routes_by_shape); the static LDS seen here is the tile route's tile alone."""
    from pyloo_amd import _capi

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    assert "pla_k_draws.hip" in isa_stats.KERNEL_UNITS
    lines = isa_stats.compile_isa(units=["pla_k_draws.hip"], out="/tmp/pla_isa_draws.s")
    text = "\n".join(lines)
    blocks = re.split(r"\n\s+- \.", text[text.index("amdhsa.kernels"):])
    meta = {}
    for b in blocks:
        m = re.search(r"\.name:\s+(_ZN3pla19gather_draws_kernel\S+)", b)
        if not m:
            continue
        vals = dict(re.findall(r"\.(vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", b))
        meta[m.group(1)] = {k: int(v) for k, v in vals.items()}
    # f64 and f32 x (lds, lds + index: 16-byte and scalar accesses; global; tile)
    assert len(meta) == 12, sorted(meta)
    budget = 8 * lib.pla_gather_lds_max_draws(_capi.PLA_F64)
    assert budget == 4 * lib.pla_gather_lds_max_draws(_capi.PLA_F32) and budget == 80 * 1024
    for name, r in meta.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)  # eight waves per SIMD: the 512-thread workgroups are limited by LDS, not registers
        # static LDS: the tile route's kGatherTileDraws x (kGatherTileObs + 1) elements (16 x 65: pla_draws.h), nothing else
        m = re.match(r"_ZN3pla19gather_draws_kernelI([df])Li(\d)ELi(\d)EEE", name)
        esz, route = {"d": 8, "f": 4}[m.group(1)], int(m.group(2))
        assert r["group_segment_fixed_size"] == (16 * 65 * esz if route == 3 else 0), (name, r)
        _, total, _, res = isa_stats.kernel_stats(lines, name[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(k.startswith("scratch_") for k in total), (name, res)
        assert total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert isa_stats.masked_spills(lines, name[2:]) == []
