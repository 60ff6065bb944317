"""Host-side tests of loo_moment_match: validation and its messages, refusals, limits, the ABI additions and the invariants of the
golden file the GPU tests rely on.  No GPU work here (tests/test_gpu_moment_match.py has it)."""

import importlib
import os
import re

import numpy as np
import pytest

import mm_models
import pyloo_amd as pl
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pla_mm_moments", "pla_mm_transform", "pla_mm_ratios")


def mm_module():
    return importlib.import_module("pyloo_amd.loo_moment_match")


@pytest.fixture(scope="module")
def gold():
    return load_golden("moment_match")


@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()
    from pyloo_amd import _capi

    return _capi.load_library()


def small_case(S=50, D=2):
    model = mm_models.make_model(S, D, seed=1)
    n = model.n
    loo = pl.ELPDData(data=[-30.0, 1.0, 2.0, 0.5, S, n, True, np.full(n, -2.0), "log", 60.0, 2.0, np.linspace(0.0, 1.0, n), 0.7],
                      index=["elpd_loo", "se", "p_loo", "p_loo_se", "n_samples", "n_data_points", "warning", "loo_i", "scale", "looic",
                             "looic_se", "pareto_k", "good_k"])
    return model, loo


def has_gpu():
    from pyloo_amd import _capi

    return _capi.device_count() > 0


# ------------------------------------------------------------------------------------------------------------------- the front
def test_exported_with_the_reference_signature():
    import inspect

    assert "loo_moment_match" in pl.__all__ and "loo_moment_match_split" in pl.__all__
    names = list(inspect.signature(pl.loo_moment_match).parameters)
    assert names == ["model", "loo_data", "post_draws", "log_lik_i", "unconstrain_pars", "log_prob_upars_fn", "log_lik_i_upars_fn",
                     "max_iters", "k_threshold", "split", "cov", "method", "verbose", "r_eff", "batched", "batch_size", "kwargs"]
    names = list(inspect.signature(pl.loo_moment_match_split).parameters)
    assert names[:11] == ["model", "upars", "cov", "total_shift", "total_scaling", "total_mapping", "i", "r_eff_i", "log_prob_upars_fn",
                          "log_lik_i_upars_fn", "method"]
    mod = mm_module()
    for name in ("shift", "shift_and_scale", "shift_and_cov", "update_quantities_i"):
        assert callable(getattr(mod, name))


def test_missing_callbacks_are_named():
    model, loo = small_case()
    cbs = dict(mm_models.CALLBACKS)
    cbs["log_lik_i"] = None
    cbs["post_draws"] = None
    with pytest.raises(ValueError, match=r"you must provide all the following functions: post_draws, log_lik_i, unconstrain_pars, "
                                         r"log_prob_upars_fn, log_lik_i_upars_fn\. Missing: post_draws, log_lik_i"):
        pl.loo_moment_match(model, loo, **cbs)


def test_callback_signatures_are_checked():
    model, loo = small_case()
    cbs = dict(mm_models.CALLBACKS)
    cbs["log_lik_i_upars_fn"] = lambda model, upars: None
    with pytest.raises(ValueError, match=r"Custom function 'log_lik_i_upars_fn' is missing required parameters: \['i'\]. "
                                         r"Expected signature should include: \['model', 'upars', 'i'\]"):
        pl.loo_moment_match(model, loo, **cbs)
    cbs["log_lik_i_upars_fn"] = lambda **kw: None  # **kwargs covers every expected argument
    cbs["unconstrain_pars"] = lambda model, p: None
    with pytest.raises(ValueError, match="Custom function 'unconstrain_pars' is missing required parameters"):
        pl.loo_moment_match(model, loo, **cbs)


@pytest.mark.parametrize("bad, text", [
    (lambda model, pars, **kw: None, "Function returned None for upars"),
    (lambda model, pars, **kw: pars[:, 0], "Expected 2 dimensions for upars, got 1"),
    (lambda model, pars, **kw: np.where(pars > 1e9, pars, np.nan), "NaN values detected in upars"),
    (lambda model, pars, **kw: [["a", "b"]], "Could not convert upars to numpy array"),
    (lambda model, pars, **kw: 1 / 0, "division by zero"),
])
def test_unconstrained_parameter_errors(bad, text):
    model, loo = small_case()
    cbs = dict(mm_models.CALLBACKS, unconstrain_pars=bad)
    with pytest.raises(ValueError, match="Error getting unconstrained parameters: .*" + re.escape(text)) as err:
        pl.loo_moment_match(model, loo, **cbs)
    assert "Make sure your post_draws and unconstrain_pars functions are implemented correctly." in str(err.value)


def test_original_log_prob_errors():
    model, loo = small_case()
    cbs = dict(mm_models.CALLBACKS, log_prob_upars_fn=lambda model, upars, **kw: np.zeros((len(upars), 2)))
    with pytest.raises(ValueError, match="Error computing log probabilities: Expected 1 dimensions for orig_log_prob, got 2"):
        pl.loo_moment_match(model, loo, **cbs)


def test_needs_pareto_k():
    model, loo = small_case()
    with pytest.raises(ValueError, match="Moment matching requires pointwise LOO results with Pareto k values"):
        pl.loo_moment_match(model, loo.drop("pareto_k"), **mm_models.CALLBACKS)


def test_pymc_wrapper_is_refused():
    PyMCWrapper = type("PyMCWrapper", (), {})
    _, loo = small_case()
    with pytest.raises(NotImplementedError, match="PyMCWrapper"):
        pl.loo_moment_match(PyMCWrapper(), loo)
    with pytest.raises(NotImplementedError, match="PyMCWrapper"):
        pl.loo_moment_match_split(PyMCWrapper(), np.zeros((10, 2)), True, None, None, None, 0, 1.0)
    with pytest.raises(NotImplementedError, match="PyMCWrapper"):
        mm_module().update_quantities_i(PyMCWrapper(), np.zeros((10, 2)), 0, np.zeros(10), 1.0)


def test_dimension_limits():
    for D, cov, text in ((65, True, "with cov=True takes at most 64 parameters, got 65"), (1025, False, "at most 1024 parameters, got 1025")):
        model, loo = small_case(S=20, D=D)
        with pytest.raises(ValueError, match=text):
            pl.loo_moment_match(model, loo, cov=cov, **mm_models.CALLBACKS)
    from pyloo_amd.engine import Engine

    Engine.mm_check_dim(64, True)
    Engine.mm_check_dim(1024, False)


def test_callbacks_are_needed_by_the_stage_functions():
    mod = mm_module()
    with pytest.raises(ValueError, match="log_prob_upars_fn and log_lik_i_upars_fn must be provided when not using PyMCWrapper"):
        mod.update_quantities_i(object(), np.zeros((10, 2)), 0, np.zeros(10), 1.0)
    with pytest.raises(ValueError, match="you must provide the following functions: log_prob_upars_fn and log_lik_i_upars_fn"):
        pl.loo_moment_match_split(object(), np.zeros((10, 2)), True, None, None, None, 0, 1.0)


def test_no_cpu_fallback_and_input_untouched():
    if has_gpu():
        pytest.skip("a GPU is present")
    model, loo = small_case()
    before = loo.copy(deep=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pl.loo_moment_match(model, loo, **mm_models.CALLBACKS)
    assert np.array_equal(loo["pareto_k"], before["pareto_k"]) and np.array_equal(loo["loo_i"], before["loo_i"])
    assert loo["elpd_loo"] == before["elpd_loo"] and "p_loo_i" not in loo
    mod = mm_module()
    for f in (mod.shift, mod.shift_and_scale, mod.shift_and_cov):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(model.upars, np.full(len(model.upars), -np.log(len(model.upars))))


def test_two_dimensional_log_lik_points_to_r_eff():
    """The reference would take the second axis for chains and ask ArviZ for the ESS; here the caller passes r_eff."""
    cb = mm_module()._Callbacks(object(), None, None, lambda model, i, **kw: np.zeros((10, 4)), False, False, None, {})
    with pytest.raises(TypeError, match="r_eff"):
        cb.log_lik_original([3], 10)


# --------------------------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_in_header_and_binding(lib):
    from pyloo_amd import _capi

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and re.search(r"\bint " + name + r"\(", header) and hasattr(lib, name)
    assert lib.pla_abi_version() == 7 and "#define PLA_ABI_VERSION 7" in header
    assert "pla_k_mm.hip" in __import__("pyloo_amd.build", fromlist=["SOURCES"]).SOURCES


def test_null_engine_and_bad_arguments_are_status_codes(lib):
    assert lib.pla_mm_moments(None, None, None, 1, 10, 2, 1, None, None, None) == -1
    assert lib.pla_mm_transform(None, None, 0, None, None, None, None, None, 1, 10, 2, 0, 10, None, None) == -1
    assert lib.pla_mm_ratios(None, 0, None, None, None, None, 1, 10, None, None) == -1
    assert b"engine is NULL" in lib.pla_last_error()


# -------------------------------------------------------------------------------------------------------------- the golden file
def runs_of(gold):
    return sorted({k.split("/")[1] for k in gold if k.startswith("run/")})


def test_golden_decisions_keep_their_margins(gold):
    assert len(runs_of(gold)) >= 15
    for name in runs_of(gold):
        ds = max((d for d in ("a_mix", "a", "b", "c", "d", "e") if name.startswith(d + "_")), key=len)
        thr, split, cov, iters = gold[f"run/{name}/settings"]
        S = gold[f"data/{ds}/upars"].shape[0]
        thr = min(1 - 1 / np.log10(S), 0.7) if np.isnan(thr) else thr
        ks0 = gold[f"data/{ds}/pareto_k"]
        obs = gold[f"run/{name}/obs"]
        assert np.array_equal(obs, np.where(ks0 > thr)[0]) and len(obs) > 0
        trace, lens = gold[f"run/{name}/trace"], gold[f"run/{name}/trace_len"]
        pos = np.concatenate([[0], np.cumsum(lens)])
        kinds = ("sh", "sc", "co") if cov else ("sh", "sc")
        for n, i in enumerate(obs):
            text = str(gold[f"run/{name}/decisions"][n])
            stages = re.findall(r"(sh|sc|co)([+-])", text)
            assert len(stages) == lens[n] and "".join(a + b for a, b in stages) == text
            k = ks0[i]
            for (tag, sign), k_new in zip(stages, trace[pos[n]:pos[n + 1]]):
                assert abs(k_new - k) >= 1e-3 and (k_new < k) == (sign == "+"), (name, i, tag)
                k = min(k, k_new)
                if tag == kinds[-1]:
                    assert abs(k - thr) >= 1e-3, (name, i)
            assert gold[f"run/{name}/pareto_k"][i] == k
        assert float(gold[f"run/{name}/margin"]) >= 1e-3


def test_golden_covers_every_branch(gold):
    every = "".join(str(d) for name in runs_of(gold) for d in gold[f"run/{name}/decisions"])
    for tag in ("sh", "sc", "co"):
        assert tag + "+" in every and tag + "-" in every
    assert any(len(gold[f"run/{name}/split_obs"]) for name in runs_of(gold))
    assert any("Cholesky" in str(w) for w in gold["run/b_low/warnings"])  # D = 1: the identity-mapping fallback
    assert gold["run/a_one_iter/settings"][3] == 1
    shapes = {gold[f"data/{d}/upars"].shape for d in ("a", "a_mix", "b", "c", "d", "e")}
    assert shapes == {(400, 2), (400, 1), (1000, 5), (1000, 17), (400, 64)}
    assert np.array_equal(gold["data/a/y"][-4:], [6.0, -5.0, 4.5, 3.5])
    # the model of the tests reproduces the generator's inputs
    model = mm_models.make_model(400, 2, int(gold["data/a_mix/seed"]), mixed=True)
    assert np.array_equal(model.upars, gold["data/a_mix/upars"]) and np.array_equal(model.y, gold["data/a_mix/y"])
