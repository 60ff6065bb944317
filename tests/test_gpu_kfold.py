"""GPU tests of k-fold cross-validation (pla_kfold_lme / pla_kfold_reduce through the engine and the front); run with ``-m gpu``.

Tolerances are the project's own for log-mean-exp values (tests/test_gpu_waic.py): pointwise rtol 1e-10 / atol 1e-12, sums rtol
1e-10, standard errors rtol 1e-8 / atol 1e-9 -- against the reference's goldens or, for seeded inputs, against
``oracle.psis_oracle.lse(row, b_inv=S)``."""

import warnings

import numpy as np
import pytest

import pyloo_amd as pl
from conftest import load_golden
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu
CASES = ("random", "ragged", "ragged_f32", "stratified", "stratified_binary", "grouped", "grouped_few", "loo_exact", "user_folds",
         "nan_full", "extreme")
SCALE = {"log": 1.0, "negative_log": -1.0, "deviance": -2.0}


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


@pytest.fixture(scope="module")
def gold():
    return load_golden("kfold")


def case_inputs(gold, case):
    K = int(gold[f"{case}/K"])
    return gold[f"{case}/ll_full"], [gold[f"{case}/fold_{k + 1}"] for k in range(K)], gold[f"{case}/folds"], str(gold[f"{case}/scale"])


def lme(a):
    """log mean exp of every row as the reference computes it, on the f64 widening."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.array([orc.lse(r, b_inv=a.shape[1]) for r in a], dtype=np.float64)


def expected(full, mats, folds, nan_fix=True):
    """(lpd_full, elpd) by the oracle; ``mats`` compact or full form."""
    full = np.asarray(full, dtype=np.float64)
    n = full.shape[0]
    lpd = lme(np.where(np.isnan(full), -1e10, full) if nan_fix else full)
    elpd = np.zeros(n)
    for k, m in enumerate(mats):
        idx = np.where(folds == k + 1)[0]
        elpd[idx] = lme(m[idx] if m.shape[0] == n else m)
    return lpd, elpd


def layout(a, kind):
    """A host matrix on the device: draws fastest, observations fastest (an (S, n) buffer seen as .T), every second draw of a
    wider buffer, or every second row of a taller one."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if kind == "draws":
        return t
    if kind == "obs":
        return t.T.contiguous().T
    if kind == "draw2":
        buf = torch.full((t.shape[0], 2 * t.shape[1]), float("nan"), dtype=t.dtype, device="cuda")
        buf[:, ::2] = t
        return buf[:, ::2]
    buf = torch.full((2 * t.shape[0], t.shape[1]), float("nan"), dtype=t.dtype, device="cuda")
    buf[::2] = t
    return buf[::2]


def check_pointwise(res, lpd, elpd, scale_value=1.0):
    g = {k: v.cpu().numpy() if hasattr(v, "cpu") else v for k, v in res.items()}
    np.testing.assert_allclose(g["lpd_full_i"], lpd, rtol=1e-10, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(g["elpd_i"], elpd, rtol=1e-10, atol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(g["p_i"], g["lpd_full_i"] - g["elpd_i"])
    np.testing.assert_array_equal(g["kfold_i"], scale_value * g["elpd_i"])
    return g


def check_agg(g, n_nan=0):
    agg, n = g["agg"], g["kfold_i"].size
    assert agg[0] == n and agg[5] == n_nan and agg[6] == 0 and agg[7] == 0
    with np.errstate(all="ignore"):
        np.testing.assert_allclose(agg[1], g["kfold_i"].sum(), rtol=1e-10, equal_nan=True)
        np.testing.assert_allclose(agg[3], g["p_i"].sum(), rtol=1e-10, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(np.sqrt(agg[2]), np.sqrt(n * np.var(g["kfold_i"])), rtol=1e-8, atol=1e-9, equal_nan=True)
        np.testing.assert_allclose(np.sqrt(agg[4]), np.sqrt(n * np.var(g["p_i"])), rtol=1e-8, atol=1e-9, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ the goldens
@pytest.mark.parametrize("case", CASES)
def test_golden_cases_through_the_front(eng, gold, case):
    import torch

    full, mats, folds, scale = case_inputs(gold, case)
    n_nan = int(gold[f"{case}/n_nan"])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_kfold_from_matrix(torch.from_numpy(full).cuda(), [torch.from_numpy(m).cuda() for m in mats], folds,
                                       pointwise=True, scale=scale)
    assert len([w for w in rec if "NaN values detected in log-likelihood" in str(w.message)]) == (1 if n_nan else 0)
    assert res["kfold_i"].is_cuda
    np.testing.assert_allclose(res["kfold_i"].cpu().numpy(), gold[f"{case}/kfold_i"], rtol=1e-10, atol=1e-12, equal_nan=True)
    want = gold[f"{case}/stats"]
    got = [res["elpd_kfold"], res["se"], res["p_kfold"], res["p_kfold_se"], res["kfoldic"], res["kfoldic_se"]]
    np.testing.assert_allclose(got[0::2], want[0::2], rtol=1e-10, equal_nan=True)
    np.testing.assert_allclose(got[1::2], want[1::2], rtol=1e-8, atol=1e-9, equal_nan=True)
    assert res["K"] == int(gold[f"{case}/K"]) and res["n_samples"] == full.shape[1] and res["n_data_points"] == full.shape[0]
    # the engine's pointwise vectors, NumPy in -> NumPy out
    r = eng.kfold(full, mats, folds, SCALE[scale])
    assert isinstance(r["elpd_i"], np.ndarray)
    np.testing.assert_allclose(r["lpd_full_i"], gold[f"{case}/lpd_full"], rtol=1e-10, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(r["elpd_i"], gold[f"{case}/elpd"], rtol=1e-10, atol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(r["p_i"], r["lpd_full_i"] - r["elpd_i"])  # (the difference of the two vectors held above)
    assert r["agg"][5] == n_nan


@pytest.mark.parametrize("case", ("nan_full", "extreme"))
@pytest.mark.parametrize("kind,route", [("obs", "kfold_lane_kernel"), ("draw2", "kfold_block_kernel"), ("row2", "kfold_wave_kernel")])
def test_nan_and_infinities_on_every_route(eng, gold, case, kind, route):
    """NaN of the full fit counted and taken as -1e10, -inf entries, a row of -inf, a +inf: what the reference's expression gives."""
    full, mats, folds, scale = case_inputs(gold, case)
    res = eng.kfold(layout(full, kind), [layout(m, kind) for m in mats], folds)
    assert route in eng.last_kernels() and eng.last_kernels().count("kfold_") == 4, eng.last_kernels()  # one route + the finish
    g = check_pointwise(res, gold[f"{case}/lpd_full"], gold[f"{case}/elpd"])
    assert g["agg"][5] == int(gold[f"{case}/n_nan"])
    # without the flag a NaN stays a NaN
    res = eng.kfold(layout(full, kind), [layout(m, kind) for m in mats], folds, nan_flag=False)
    lpd, _ = expected(full, mats, folds, nan_fix=False)
    np.testing.assert_allclose(res["lpd_full_i"].cpu().numpy(), lpd, rtol=1e-10, atol=1e-12, equal_nan=True)
    assert res["agg"][5].item() == 0


# ---------------------------------------------------------------------------------------------------------------- the wave route
def padded(a):
    """(n, S) on the device as a view of a buffer whose rows start on 16-byte boundaries."""
    import torch

    n, s = a.shape
    vec = 16 // a.itemsize
    buf = torch.full((n, (s + vec - 1) // vec * vec), float("nan"), dtype=torch.from_numpy(a).dtype, device="cuda")
    buf[:, :s] = torch.from_numpy(a).cuda()
    return buf[:, :s]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_wave_route_edges(eng, dt):
    """One launch whose folds have S_k = 7, 63, 64, 65, 257, 4096 with one to five rows each.  Padded to 16-byte rows they all
    take the wave route (lengths that are no multiple of the 16-byte vector included); one more fold of 65 draws lies
    contiguous -- a row pitch that is no multiple of 16 bytes -- and is right on whichever route takes it."""
    rng = np.random.default_rng(7)
    sizes = [(7, 1), (63, 2), (64, 3), (65, 4), (257, 5), (4096, 2), (65, 3)]
    folds = rng.permutation(np.repeat(np.arange(1, len(sizes) + 1), [r for _, r in sizes]))
    n = folds.size
    full = rng.normal(-2, 1.5, size=(n, 100)).astype(dt)
    mats = [(rng.normal(-1, 2, size=(r, s)) - 3 * rng.exponential(size=(r, 1))).astype(dt) for s, r in sizes]
    dev = [padded(m) for m in mats[:-1]] + [layout(mats[-1], "draws")]
    res = eng.kfold(layout(full, "draws"), dev, folds)
    kern = eng.last_kernels()
    assert "kfold_wave_kernel" in kern and "kfold_block_kernel" in kern and "kfold_lane_kernel" not in kern, kern
    g = check_pointwise(res, *expected(full, mats, folds))
    check_agg(g)
    # all of them padded: the wave route alone
    res2 = eng.kfold(layout(full, "draws"), [padded(m) for m in mats], folds)
    assert "kfold_block_kernel" not in eng.last_kernels()
    check_pointwise(res2, *expected(full, mats, folds))


def test_rows_beyond_the_registers(eng):
    """S_k = 4097 and 20 000 (f32, 6 rows) beside a short fold: the block route beside the wave route in one call."""
    rng = np.random.default_rng(11)
    sizes = [(4097, 6), (20000, 6), (64, 5)]
    folds = np.repeat(np.arange(1, 4), [r for _, r in sizes])
    full = rng.normal(-2, 1, size=(17, 128)).astype(np.float32)
    mats = [(rng.normal(-1, 2, size=(r, s))).astype(np.float32) for s, r in sizes]
    res = eng.kfold(layout(full, "draws"), [padded(m) for m in mats], folds)
    kern = eng.last_kernels()
    assert "kfold_wave_kernel<float>" in kern and "kfold_block_kernel<float>" in kern, kern
    check_agg(check_pointwise(res, *expected(full, mats, folds)))


# ---------------------------------------------------------------------------------------------------------------- the lane route
def lane_case(rng, dt=np.float64):
    counts = [1, 63, 64, 65, 130]
    draws = [7, 257, 1000, 7, 257]
    n = sum(counts)
    full = rng.normal(-2, 1.5, size=(n, 257)).astype(dt)
    return counts, draws, n, full


@pytest.mark.parametrize("form", ["compact", "full_contiguous", "full_scattered"])
def test_lane_route(eng, form):
    """.T views of (S_k, n) buffers with 1, 63, 64, 65 and 130 tasks per source and S = 7, 257, 1000."""
    rng = np.random.default_rng(13)
    counts, draws, n, full = lane_case(rng)
    folds = np.repeat(np.arange(1, 6), counts)
    if form == "full_scattered":
        folds = rng.permutation(folds)
    mats = [rng.normal(-1, 2, size=(n if form != "compact" else c, s)) for c, s in zip(counts, draws)]
    res = eng.kfold(layout(full, "obs"), [layout(m, "obs") for m in mats], folds)
    kern = eng.last_kernels()
    if form == "compact":  # (one row of S draws has no row stride to speak of: it goes to the wave route)
        assert "kfold_lane_kernel" in kern and "kfold_block_kernel" not in kern, kern
    else:
        assert "kfold_lane_kernel" in kern and "kfold_wave_kernel" not in kern and "kfold_block_kernel" not in kern, kern
    check_agg(check_pointwise(res, *expected(full, mats, folds)))


def test_strided_inputs(eng):
    rng = np.random.default_rng(17)
    folds = rng.permutation(np.repeat(np.arange(1, 4), [20, 31, 9]))
    full = rng.normal(-2, 1, size=(60, 300))
    mats = [rng.normal(-1, 2, size=(c, s)) for c, s in zip([20, 31, 9], [129, 300, 64])]
    want = expected(full, mats, folds)
    res = eng.kfold(layout(full, "draw2"), [layout(m, "draw2") for m in mats], folds)
    assert "kfold_block_kernel" in eng.last_kernels() and "kfold_wave" not in eng.last_kernels()
    a = check_pointwise(res, *want)
    res = eng.kfold(layout(full, "row2"), [layout(m, "row2") for m in mats], folds)
    assert "kfold_wave_kernel" in eng.last_kernels()
    b = check_pointwise(res, *want)
    np.testing.assert_allclose(a["elpd_i"], b["elpd_i"], rtol=1e-10, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ forms and spaces
@pytest.mark.parametrize("kind", ["draws", "obs"])
def test_forms_and_memory_spaces_agree_bitwise(eng, kind):
    rng = np.random.default_rng(19)
    counts, draws = [70, 5, 129], [256, 1000, 64]
    folds = rng.permutation(np.repeat(np.arange(1, 4), counts))
    n = folds.size
    full = rng.normal(-2, 1.5, size=(n, 400))
    wide = [rng.normal(-1, 2, size=(n, s)) for s in draws]
    compact = [w[folds == k + 1] for k, w in enumerate(wide)]
    host = lambda a: a if kind == "draws" else np.ascontiguousarray(a.T).T  # noqa: E731
    a = eng.kfold(layout(full, kind), [layout(m, kind) for m in compact], folds)
    b = eng.kfold(layout(full, kind), [layout(m, kind) for m in wide], folds)
    c = eng.kfold(layout(full, kind), [layout(wide[0], kind), layout(compact[1], kind), layout(wide[2], kind)], folds)
    d = eng.kfold(host(full), [host(m) for m in compact], folds)
    e = eng.kfold(host(full), [host(m) for m in wide], folds)  # (cut to the held-out rows on the host)
    assert isinstance(d["elpd_i"], np.ndarray) and a["elpd_i"].is_cuda
    for key in ("elpd_i", "lpd_full_i", "p_i", "kfold_i", "agg"):
        ref = a[key].cpu().numpy()
        for other in (b, c):
            np.testing.assert_array_equal(other[key].cpu().numpy(), ref)
        for other in (d, e):
            np.testing.assert_array_equal(other[key], ref)
    check_pointwise(a, *expected(full, compact, folds))


def test_layouts_agree(eng):
    rng = np.random.default_rng(23)
    folds = rng.permutation(np.repeat(np.arange(1, 4), [40, 41, 42]))
    full = rng.normal(-2, 1.5, size=(123, 500))
    mats = [rng.normal(-1, 2, size=(c, s)) for c, s in zip([40, 41, 42], [500, 333, 64])]
    a = eng.kfold(layout(full, "draws"), [layout(m, "draws") for m in mats], folds)
    b = eng.kfold(layout(full, "obs"), [layout(m, "obs") for m in mats], folds)
    for key in ("elpd_i", "lpd_full_i"):
        np.testing.assert_allclose(a[key].cpu().numpy(), b[key].cpu().numpy(), rtol=1e-10, atol=1e-12)
    # device folds are used as they are
    import torch

    c = eng.kfold(layout(full, "draws"), [layout(m, "draws") for m in mats], torch.from_numpy(folds).cuda())
    np.testing.assert_array_equal(c["elpd_i"].cpu().numpy(), a["elpd_i"].cpu().numpy())


def test_dtypes_may_not_be_mixed(eng):
    full = np.zeros((6, 8))
    with pytest.raises(TypeError, match="must share one dtype"):
        eng.kfold(full, [np.zeros((3, 8), dtype=np.float32), np.zeros((3, 8))], np.repeat([1, 2], 3))
    with pytest.raises(ValueError, match="Fold indices must be the integers"):
        eng.kfold(full, [np.zeros((3, 8)), np.zeros((3, 8))], np.repeat([1, 3], 3))


# ------------------------------------------------------------------------------------------------------ launches and aggregates
def launches_of(text):
    """The number of kernels the ragged pass launched, as the library counted them where it launches (pla_k_kfold.hip)."""
    import re

    return int(re.search(r"; (\d+) launch(?:es)?\)", text).group(1))


def test_launch_count_does_not_depend_on_k(eng):
    """One launch per route present, whatever K is: the count the launcher keeps of the launches it made, and the timed brackets."""
    rng = np.random.default_rng(29)
    n = 600
    full = layout(rng.normal(-2, 1, size=(n, 128)), "draws")
    counts, brackets = {}, {}
    eng.set_timing(True)
    try:
        for K in (2, 10):
            folds = np.arange(n) % K + 1
            mats = [layout(rng.normal(-1, 2, size=(int(np.sum(folds == k + 1)), 64 + 8 * k)), "draws") for k in range(K)]
            eng.kernel_ms()
            eng.kfold(full, mats, folds)
            assert eng.last_kernels().startswith("kfold_wave_kernel<double> (matrices read in place; 1 launch), then kfold_tiles_kernel")
            counts[K] = launches_of(eng.last_kernels())
            brackets[K] = eng.kernel_ms()[1]
            # two routes -> two launches, again whatever K is
            eng.kfold(full, [layout(m.cpu().numpy(), "draw2") for m in mats], folds)
            assert launches_of(eng.last_kernels()) == 2 and "kfold_block_kernel" in eng.last_kernels(), eng.last_kernels()
            eng.kernel_ms()
    finally:
        eng.set_timing(False)
    assert counts[2] == counts[10] == 1, counts
    assert brackets[2] == brackets[10] == 2, brackets  # the ragged pass and the finishing pass, one bracket each


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 5000])
def test_aggregates_against_numpy(eng, n):
    rng = np.random.default_rng(n)
    K = 1 if n == 1 else 2
    folds = np.arange(n) % K + 1
    full = rng.normal(-2, 1.5, size=(n, 64))
    mats = [rng.normal(-1, 2, size=(int(np.sum(folds == k + 1)), 32)) - 5 * (k + 1) for k in range(K)]
    res = eng.kfold(layout(full, "draws"), [layout(m, "draws") for m in mats], folds, -2.0)
    g = check_pointwise(res, *expected(full, mats, folds), scale_value=-2.0)
    check_agg(g)
    # the grid does not change a bit of them
    eng.set_compare_grid(1)
    try:
        one = eng.kfold(layout(full, "draws"), [layout(m, "draws") for m in mats], folds, -2.0)
    finally:
        eng.set_compare_grid(0)
    np.testing.assert_array_equal(one["agg"].cpu().numpy(), g["agg"])


# ------------------------------------------------------------------------------------------------------------------ the front
def test_front_with_a_refit_closure(eng, gold):
    import torch

    full, mats, _, _ = case_inputs(gold, "random")
    n, s = full.shape
    rng = np.random.default_rng(31)
    held = torch.from_numpy(rng.normal(-1.5, 1.0, size=(n, 96))).cuda()  # row i: observation i under the fit that left it out
    data = {"log_likelihood": {"y": np.ascontiguousarray(full.T).reshape(4, s // 4, n)}}
    calls = []

    def fit_fold(train_idx, val_idx, thin=1):
        calls.append((train_idx.copy(), val_idx.copy(), thin))
        return held[torch.from_numpy(val_idx).cuda()][:, ::thin]

    with pytest.raises(TypeError, match="must share one dtype"):  # a float32 refit beside a float64 full fit
        pl.loo_kfold(data, lambda tr, va: held[torch.from_numpy(va).cuda()].float(), K=5, random_seed=11)
    res = pl.loo_kfold(data, fit_fold, K=5, random_seed=11, pointwise=True, save_fits=True, thin=2)
    folds = gold["random/folds"]  # (K = 5, N = 60, seed 11: the reference's folds)
    assert [c[2] for c in calls] == [2] * 5
    for k, (tr, va, _) in enumerate(calls):
        np.testing.assert_array_equal(va, np.where(folds == k + 1)[0])
        np.testing.assert_array_equal(tr, np.where(folds != k + 1)[0])
    assert list(res.index)[-1] == "fits" and len(res["fits"]) == 5
    for k, (fit, va) in enumerate(res["fits"]):
        assert fit.is_cuda and tuple(fit.shape) == (int(np.sum(folds == k + 1)), 48)
        np.testing.assert_array_equal(va, np.where(folds == k + 1)[0])
    direct = pl.loo_kfold_from_matrix(layout(full, "obs"), [held[torch.from_numpy(np.where(folds == k + 1)[0]).cuda()][:, ::2] for k in range(5)],
                                      folds, pointwise=True)
    np.testing.assert_array_equal(np.asarray(res["kfold_i"]).ravel(), direct["kfold_i"].cpu().numpy())
    assert res["elpd_kfold"] == direct["elpd_kfold"] and res["se"] == direct["se"] and res["p_kfold"] == direct["p_kfold"]
    np.testing.assert_allclose(np.asarray(res["kfold_i"]).ravel(), expected(full, [held.cpu().numpy()[:, ::2]] * 5, folds)[1],
                               rtol=1e-10, atol=1e-12)
    assert "5-fold cross-validation" in str(res)
