"""Leave-one-group-out front without a GPU: GroupIndex construction, argument errors and warning texts, the ELPDData layout and
report, the packing of the front against the reference's numbers (tests/golden/loo_group.npz) through a stand-in engine, and the
status codes of the two C entry points for bad arguments (library built, no GPU needed)."""

import ctypes as C
import importlib
import warnings

import numpy as np
import pytest

from fake_engine import OracleEngine

METHODS = {0: "psis", 1: "sis", 2: "tis"}
SCALES = {1: "log", -1: "negative_log", -2: "deviance"}
CASES = ["int_f64", "int_f32", "str", "singleton", "heavy", "nan", "sis", "tis", "big"]


class GroupOracleEngine(OracleEngine):
    """Stand-in for the engine's group calls: NumPy's group sums (NaN -> -1e10 first, in the input dtype), then the oracle pass."""

    def group_sum(self, ll, index):
        ll = np.asarray(ll)
        nan = np.isnan(ll)
        clean = np.where(nan, ll.dtype.type(-1e10), ll)
        off, mem = np.asarray(index.offsets), np.asarray(index.members)
        sums = np.stack([clean[mem[off[g]:off[g + 1]]].sum(axis=0) for g in range(index.n_groups)])
        return sums, int(nan.sum())

    def psis_loo_groups(self, ll, index, tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True):
        sums, nrep = self.group_sum(ll, index)
        res = self.psis_loo(sums.astype(np.float64), tail_count, method, scale_value, good_k)
        return {"diag": res["diag"], "logo_i": res["loo_i"], "lppd_i": res["lppd_i"], "agg": res["agg"], "n_replaced": nrep}


@pytest.fixture
def fake(monkeypatch):
    eng = GroupOracleEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_group"), "get_engine", lambda device=None: eng)
    return eng


@pytest.fixture(scope="module")
def gold(golden):
    return golden("loo_group")


def case(z, name):
    reff, m, sv = z[f"{name}__meta"]
    return z[f"{name}__ll"], z[f"{name}__ids"], float(reff), METHODS[int(m)], SCALES[int(sv)]


def as_data(ll):
    from pyloo_amd.utils import SimpleInferenceData

    arr = np.ascontiguousarray(ll.T).reshape(1, ll.shape[1], ll.shape[0])
    return SimpleInferenceData(log_likelihood={"obs": arr}, posterior={"mu": np.zeros((1, ll.shape[1]))})


# ---------------------------------------------------------------------------------------------------- GroupIndex
@pytest.mark.parametrize("ids,labels,offsets,members", [
    (np.array([3, 1, 3, 2, 1, 3]), [1, 2, 3], [0, 2, 3, 6], [1, 4, 3, 0, 2, 5]),
    (np.array([0.5, -2.0, 0.5, 7.25, -2.0, 0.5]), [-2.0, 0.5, 7.25], [0, 2, 5, 6], [1, 4, 0, 2, 5, 3]),
    (np.array(["b", "a", "b", "c", "a", "b"]), ["a", "b", "c"], [0, 2, 5, 6], [1, 4, 0, 2, 5, 3]),
    ([3, 1, 3, 2, 1, 3], [1, 2, 3], [0, 2, 3, 6], [1, 4, 3, 0, 2, 5]),
])
def test_group_index_order_offsets_members(ids, labels, offsets, members):
    import pyloo_amd as pl

    idx = pl.group_index(ids)
    assert list(idx.labels) == labels and idx.n_groups == 3 and idx.n_obs == 6
    assert idx.offsets.dtype == np.int64 and idx.members.dtype == np.int64
    assert list(idx.offsets) == offsets
    assert list(idx.members) == members  # ascending inside every group
    flat = np.asarray(ids).reshape(-1)
    for g in range(3):
        mem = idx.members[idx.offsets[g]:idx.offsets[g + 1]]
        assert np.all(np.diff(mem) > 0) and np.all(flat[mem] == idx.labels[g])


def test_group_index_multidimensional_ids_flatten_in_c_order():
    import pyloo_amd as pl

    ids = np.array([[2, 0, 2], [1, 0, 2]])
    idx = pl.group_index(ids)
    assert list(idx.labels) == [0, 1, 2] and list(idx.offsets) == [0, 2, 3, 6] and list(idx.members) == [1, 4, 3, 0, 2, 5]


def test_group_index_rejects_nan_labels():
    import pyloo_amd as pl

    with pytest.raises(ValueError, match="NaN"):
        pl.group_index(np.array([1.0, np.nan, 2.0]))


# ---------------------------------------------------------------------------------------------------- errors and warnings
def test_length_mismatch_raises_reference_error(fake, gold):
    import pyloo_amd as pl

    ll, ids, *_ = case(gold, "int_f64")
    with pytest.raises(ValueError, match=r"^Length of group_ids \(59\) must match the number of observations in log_likelihood \(60\)\.$"):
        pl.loo_group(as_data(ll), ids[:-1], reff=1.0)


def test_bad_scale_and_method(fake, gold):
    import pyloo_amd as pl

    ll, ids, *_ = case(gold, "int_f64")
    with pytest.raises(TypeError, match='Valid scale values are "deviance", "log", "negative_log"'):
        pl.loo_group(as_data(ll), ids, reff=1.0, scale="bits")
    with pytest.raises(ValueError, match=r"Invalid method 'mix'\. Must be one of: psis, sis, tis"):
        pl.loo_group(as_data(ll), ids, reff=1.0, method="mix")


def test_ids_of_the_observations_shape(fake, gold):
    import pyloo_amd as pl

    ll, ids, reff, method, scale = case(gold, "int_f64")
    arr = np.ascontiguousarray(ll.T).reshape(1, ll.shape[1], 6, 10)  # observations (6, 10)
    a = pl.loo_group({"log_likelihood": {"obs": arr}, "posterior": {"mu": np.zeros((1, ll.shape[1]))}}, ids.reshape(6, 10),
                     reff=reff, scale=scale, pointwise=True)
    b = pl.loo_group(as_data(ll), ids, reff=reff, scale=scale, pointwise=True)
    assert a["elpd_logo"] == b["elpd_logo"]
    assert np.array_equal(np.asarray(getattr(a["logo_i"], "values", a["logo_i"])), np.asarray(getattr(b["logo_i"], "values", b["logo_i"])))


def texts(rec):
    return [str(w.message) for w in rec]


def test_warning_texts_are_the_references(fake, gold):
    import pyloo_amd as pl

    ll, ids, reff, method, scale = case(gold, "nan")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        pl.loo_group(as_data(ll), ids, reff=reff, scale=scale)
    gk = float(gold["nan__good_k"])
    assert texts(rec) == [
        "NaN values detected in log-likelihood. These will be ignored in the LOGO calculation.",
        f"Estimated shape parameter of Pareto distribution is greater than {gk:.2f} for {int(gold['nan__n_high'])} groups. This "
        "indicates that importance sampling may be unreliable because the marginal posterior and LOGO posterior are very different.",
    ]
    ll, ids, reff, method, scale = case(gold, "heavy")  # (its heavy-tailed group has a small ESS)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        pl.loo_group(as_data(ll), ids, reff=reff, scale=scale, method="SIS")
    t = texts(rec)
    assert t[0] == ("Using SIS for LOGO computation. Note that PSIS is the recommended method as it is typically more efficient and "
                    "reliable.")
    assert len(t) == 2 and t[1].startswith("Low effective sample size detected (minimum ESS: ") and t[1].endswith(
        "). This indicates that the importance sampling approximation may be unreliable. Consider using PSIS which is more robust "
        "to such cases.")


# ---------------------------------------------------------------------------------------------------- ELPDData
KEYS = ["elpd_logo", "se", "p_logo", "p_logo_se", "n_samples", "n_groups", "warning"]


@pytest.mark.parametrize("method,tail", [("psis", ["pareto_k", "good_k"]), ("sis", ["ess"]), ("tis", ["ess"])])
def test_elpddata_keys_in_reference_order(fake, gold, method, tail):
    import pyloo_amd as pl

    ll, ids, *_ = case(gold, "sis")
    res = pl.loo_group(as_data(ll), ids, reff=1.0, method=method, pointwise=True)
    assert list(res.index) == KEYS + ["logo_i", "scale", "logoic", "logoic_se"] + tail
    res = pl.loo_group(as_data(ll), ids, reff=1.0, method=method, pointwise=False)
    assert list(res.index) == KEYS + ["scale", "logoic", "logoic_se"] + (["good_k"] if method == "psis" else [])


def test_logo_report(fake, gold):
    import pyloo_amd as pl

    ll, ids, reff, method, scale = case(gold, "heavy")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = pl.loo_group(as_data(ll), ids, reff=reff, pointwise=True)
    gk = res["good_k"]
    k = np.asarray(res["pareto_k"])
    c = np.histogram(k, bins=[-np.inf, gk, 1, np.inf])[0]
    p = c / c.sum() * 100
    want = (f"\nComputed from {ll.shape[1]} posterior samples and 6 groups log-likelihood matrix.\n\n"
            "         Estimate       SE\n"
            f"elpd_logo   {res['elpd_logo']:<8.2f}    {res['se']:<.2f}\n"
            f"p_logo       {res['p_logo']:<8.2f}    {res['p_logo_se']:<.2f}\n"
            f"logoic      {res['logoic']:<8.2f}    {res['logoic_se']:<.2f}"
            "\n\nThere has been a warning during the calculation. Please check the results."
            "\n------\n\nPareto k diagnostic values:\n                         Count   Pct.\n"
            f"(-Inf, {gk:.2f}]   (good)      {c[0]:d}   {p[0]:.1f}%\n"
            f"   ({gk:.2f}, 1]   (bad)         {c[1]:d}    {p[1]:.1f}%\n"
            f"   (1, Inf)   (very bad)    {c[2]:d}    {p[2]:.1f}%")
    assert str(res) == want
    quiet = pl.loo_group(as_data(case(gold, "sis")[0]), case(gold, "sis")[1], reff=1.0, pointwise=False)
    text = str(quiet)
    assert text.startswith("\nComputed from 200 posterior samples and 6 groups log-likelihood matrix.") and "Pareto k" not in text


# ---------------------------------------------------------------------------------------------------- packing vs the reference
@pytest.mark.parametrize("name", CASES)
def test_front_packing_against_reference(fake, gold, name):
    import pyloo_amd as pl

    ll, ids, reff, method, scale = case(gold, name)
    p = f"{name}__"
    sums, nrep = fake.group_sum(ll, pl.group_index(ids))
    assert np.array_equal(sums, gold[p + "sums"]) and (nrep > 0) == bool(gold[p + "has_nan"])
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        res = pl.loo_group(as_data(ll), ids, reff=reff, scale=scale, method=method, pointwise=True)
    for key in ("elpd_logo", "p_logo", "logoic"):
        np.testing.assert_allclose(res[key], gold[p + key], rtol=1e-9, atol=1e-6, err_msg=key)
    for key in ("se", "p_logo_se", "logoic_se"):
        np.testing.assert_allclose(res[key], gold[p + key], rtol=1e-8, err_msg=key)
    np.testing.assert_allclose(np.asarray(getattr(res["logo_i"], "values", res["logo_i"])), gold[p + "logo_i"], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(res["pareto_k" if method == "psis" else "ess"], gold[p + "diag"], rtol=1e-9, atol=1e-10)
    assert res["n_groups"] == len(gold[p + "labels"]) and bool(res["warning"]) == bool(gold[p + "warning"])
    assert res["scale"] == scale


def test_from_matrix_takes_a_prebuilt_index(fake, gold):
    import pyloo_amd as pl

    ll, ids, reff, method, scale = case(gold, "int_f64")
    idx = pl.group_index(ids)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = pl.loo_group_from_matrix(ll, idx, reff=reff, pointwise=True)
        b = pl.loo_group_from_matrix(ll, ids, reff=reff, pointwise=True)
    assert a["elpd_logo"] == b["elpd_logo"] and np.array_equal(a["logo_i"], b["logo_i"])
    np.testing.assert_allclose(a["elpd_logo"], gold["int_f64__elpd_logo"], rtol=1e-9)


# ---------------------------------------------------------------------------------------------------- C entry points
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd import _capi

    try:
        return _capi.load_library()
    except Exception as err:  # pragma: no cover - library not built
        pytest.skip(f"library not built: {err}")


def test_group_entry_points_reject_bad_arguments(lib):
    from pyloo_amd import _capi

    ll = np.zeros((4, 16))
    p = ll.ctypes.data_as(C.c_void_p)
    off = np.array([0, 2, 4], dtype=np.int64)
    mem = np.array([0, 1, 2, 3], dtype=np.int64)
    out = np.zeros((2, 16))
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    # no engine
    assert lib.pla_group_sum(None, p, 0, 4, 16, 16, 1, P(off), P(mem), 2, _capi.PLA_HOST, None, P(out), None) == -1
    assert b"engine is NULL" in lib.pla_last_error()
    assert lib.pla_psis_loo_groups(None, p, 0, 4, 16, 16, 1, P(off), P(mem), 2, 0, 3, 1.0, 0.7, _capi.PLA_HOST, None, None, None, None,
                                   None, None) == -1
    assert b"engine is NULL" in lib.pla_last_error()


@pytest.mark.gpu
def test_group_index_checks_with_an_engine():
    """Host index lists are checked before anything reaches the device (an engine needs a GPU)."""
    from pyloo_amd._capi import EngineError
    from pyloo_amd.engine import get_engine
    from pyloo_amd.loo_group import GroupIndex

    eng = get_engine(0)
    ll = np.zeros((4, 16))
    for off, mem, msg in (([1, 2, 4], [0, 1, 2, 3], "group_offsets\\[0\\]"), ([0, 3, 2], [0, 1, 2, 3], "decrease"),
                          ([0, 2, 4], [0, 1, 2, 9], "outside"), ([0, 2, 4], [1, 0, 2, 3], "ascending")):
        idx = GroupIndex(np.arange(2), np.array(off, dtype=np.int64), np.array(mem, dtype=np.int64))
        with pytest.raises(EngineError, match=msg) as err:
            eng.group_sum(ll, idx)
        assert err.value.code == -1
