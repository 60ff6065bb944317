"""loo_compare's host side without a GPU: the front against a NumPy engine (tests/compare_stream.py), the Philox4x32-10
restatement against known answers, and the static resource limits of the comparison kernels (csrc/pla_compare.h)."""

import os
import shutil
import sys

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from compare_cases import CASES, pointwise  # noqa: E402
from compare_stream import (NumpyCompareEngine, bb_z, gamma_draws, moments_reference, philox4x32_10, stacking_objective,  # noqa: E402
                            stacking_reference)

GOLD = np.load(os.path.join(HERE, "golden", "compare.npz"))


@pytest.fixture
def fake(monkeypatch):
    import pyloo_amd.compare as cmp

    eng = NumpyCompareEngine()
    monkeypatch.setattr(cmp, "get_engine", lambda device=None: eng)
    return eng


def elpd(x_k, scale="log", ic="loo", pointwise_=True, total=None):
    from pyloo_amd import ELPDData

    data = [float(np.sum(x_k)) if total is None else total, 1.5, 2.5, False, scale]
    index = [f"elpd_{ic}", "se", f"p_{ic}", "warning", "scale"]
    if pointwise_:
        data.append(np.asarray(x_k))
        index.append(f"{ic}_i")
    return ELPDData(data=data, index=index)


def models(case):
    seed, K, N, scale, kind = CASES[case]
    x = pointwise(seed, K, N, scale, kind)
    return {f"m{k}": elpd(x[k], scale, total=float(GOLD[f"{case}/elpd"][k])) for k in range(K)}, x


# ---- Philox4x32-10 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, want):
    got = philox4x32_10([np.uint64(c) for c in ctr], [np.uint64(k) for k in key])
    assert tuple(int(v) for v in got) == want


@pytest.mark.parametrize("alpha", [1.0, 0.5, 2.0, 7.5])
def test_gamma_stream_moments(alpha):
    """The restated stream is Gamma(alpha, 1): mean alpha, variance alpha (4 000 x 50 draws, 6 standard errors)."""
    g = gamma_draws(77, alpha, 4000, 50).ravel()
    n = g.size
    assert abs(g.mean() - alpha) < 6 * np.sqrt(alpha / n)
    assert abs(g.var() / alpha - 1) < 0.05
    assert np.all(g > 0)


def test_gamma_stream_is_a_function_of_its_coordinates():
    a = gamma_draws(5, 0.5, 6, 9)
    b = gamma_draws(5, 0.5, 10, 20)
    assert np.array_equal(a, b[:6, :9])
    assert not np.array_equal(a, gamma_draws(6, 0.5, 6, 9))


@pytest.mark.parametrize("alpha", [1.0, 0.5, 2.0])
def test_replicate_subset_is_the_same_rows_of_the_full_call(alpha):
    """``replicates=`` restates a few replicates of a long vector: bitwise the rows of the full call, in the order asked for."""
    reps = np.array([0, 63, 64, 7, 129])
    full = gamma_draws(91, alpha, 130, 301)
    assert np.array_equal(gamma_draws(91, alpha, 130, 301, replicates=reps), full[reps])
    x = pointwise(2, 3, 301, "log")
    assert np.array_equal(bb_z(x, 130, alpha, 91, -0.5, replicates=reps), bb_z(x, 130, alpha, 91, -0.5)[reps])
    assert gamma_draws(91, alpha, 130, 301, replicates=[]).shape == (0, 301)
    with pytest.raises(ValueError, match="replicates"):
        gamma_draws(91, alpha, 130, 301, replicates=[130])


def test_wider_references_agree_with_the_f64_restatement():
    """``moments_reference`` / ``stacking_reference`` (fsum, longdouble) against the plain f64 NumPy engine, on well-conditioned
    input; f32 input is the arithmetic on the widened f32 values."""
    eng = NumpyCompareEngine()
    x = pointwise(4, 5, 777, "deviance")
    w = np.array([0.1, 0.3, 0.2, 0.15, 0.25])
    for xx in (x, x.astype(np.float32)):
        ref = moments_reference(xx, 3)
        assert ref.dtype == np.longdouble and ref[3 * 3 + 1] == 0 and ref[3 * 3 + 2] == 0
        np.testing.assert_allclose(ref.astype(float), eng.compare_moments(xx.astype(np.float64), 3), rtol=1e-12, atol=1e-13)
        F, G = stacking_reference(xx, w, -0.5)
        F64, G64 = eng.stacking_eval(xx.astype(np.float64), w, -0.5)
        assert abs(float(F) - F64) <= 1e-12 * abs(F64)
        np.testing.assert_allclose(G.astype(float), G64, rtol=1e-12)
    # two-pass in longdouble holds where a one-pass sum of squares in f64 has lost everything
    rng = np.random.default_rng(0)
    noise = rng.normal(size=5000)
    y = np.stack([np.zeros(5000), 1e6 + 1e-3 * noise])
    m2 = float(moments_reference(y, 0)[3 + 2])
    assert abs(m2 / (1e-6 * np.sum((noise - noise.mean()) ** 2)) - 1) < 1e-6


# ---- the front ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(fake):
    import pyloo_amd as pl

    d, _ = models("k3_n2000_neg")
    with pytest.raises(TypeError, match="compare_dict must be a dictionary"):
        pl.loo_compare(list(d.values()))
    with pytest.raises(ValueError, match="at least two models"):
        pl.loo_compare({"a": d["m0"]})
    with pytest.raises(ValueError, match="Scale must be"):
        pl.loo_compare(d, scale="bits")
    with pytest.raises(ValueError, match="Method must be"):
        pl.loo_compare(d, method="bma")
    with pytest.raises(ValueError, match="ic must be"):
        pl.loo_compare(d, ic="aic")
    with pytest.raises(NotImplementedError, match="kfold"):
        pl.loo_compare({"a": object(), "b": object()}, ic="kfold")


def test_precomputed_checks_and_warnings(fake):
    import pyloo_amd as pl

    x = pointwise(1, 3, 50, "log")
    a, b = elpd(x[0]), elpd(x[1])
    with pytest.raises(ValueError, match="All information criteria to be compared must be the same"):
        pl.loo_compare({"a": a, "b": elpd(x[1], ic="waic")})
    with pytest.raises(ValueError, match="must use the same scale"):
        pl.loo_compare({"a": a, "b": elpd(x[1], scale="deviance")})
    with pytest.raises(ValueError, match="pointwise=True"):
        pl.loo_compare({"a": a, "b": elpd(x[1], pointwise_=False)})
    with pytest.warns(UserWarning, match="Using ic from precomputed elpddata: loo"):
        df = pl.loo_compare({"a": a, "b": b}, ic="waic")
    assert "elpd_loo" in df.columns
    with pytest.warns(UserWarning, match="Using scale from precomputed elpddata: log"):
        df = pl.loo_compare({"a": a, "b": b}, scale="deviance")
    assert (df["scale"] == "log").all()


def test_mixed_n_names_both_shapes(fake):
    import pyloo_amd as pl

    with pytest.raises(ValueError) as err:
        pl.loo_compare({"small": elpd(np.zeros(8) - 1), "large": elpd(np.zeros(10000) - 2)})
    assert "(10000,)" in str(err.value) and "(8,)" in str(err.value)


def test_errors_of_the_ic_function_are_re_raised_with_the_model(fake):
    import pyloo_amd as pl

    with pytest.raises(Exception, match="Encountered error trying to compute loo from model a"):
        pl.loo_compare({"a": "not data", "b": "nor this"})


@pytest.mark.parametrize("case", sorted(CASES))
def test_table_against_reference(fake, case):
    import pyloo_amd as pl

    _, K, _, scale, _ = CASES[case]
    d, x = models(case)
    names = list(d)
    for method in ("stacking", "pseudo-bma"):
        df = pl.loo_compare(d, method=method)
        assert list(df.columns) == ["rank", "elpd_loo", "p_loo", "elpd_diff", "weight", "se", "dse", "warning", "scale"]
        assert list(df.index) == [names[i] for i in GOLD[f"{case}/order"]]
        assert df["rank"].tolist() == list(range(K))
        col = lambda c: np.array([df.loc[n, c] for n in names], dtype=float)  # noqa: E731
        np.testing.assert_allclose(col("elpd_diff"), GOLD[f"{case}/elpd_diff"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(col("dse"), GOLD[f"{case}/dse"], rtol=1e-12, atol=0)
        if method == "pseudo-bma":
            np.testing.assert_allclose(col("weight"), GOLD[f"{case}/pseudo_bma"], rtol=1e-12, atol=1e-300)
        else:
            w, want = col("weight"), GOLD[f"{case}/stacking"]
            s = {"log": 1.0, "negative_log": -1.0, "deviance": -0.5}[scale]
            f_w, f_ref = stacking_objective(x, w, s), stacking_objective(x, want, s)
            assert f_w <= f_ref + 1e-6 * abs(f_ref) + 1e-12
            assert np.max(np.abs(w - want)) <= 1e-4
        if scale != "log":
            assert np.all(np.diff(df["elpd_loo"].to_numpy()) >= 0)  # ascending
        else:
            assert np.all(np.diff(df["elpd_loo"].to_numpy()) <= 0)


def test_bootstrap_ses_and_seeds(fake):
    import pyloo_amd as pl

    d, x = models("k3_n2000_neg")
    a = pl.loo_compare(d, method="bb-pseudo-bma", b_samples=50, seed=7)
    b = pl.loo_compare(d, method="BB-pseudo-BMA", b_samples=50, seed=7)
    pd.testing.assert_frame_equal(a, b)
    z = NumpyCompareEngine().bb_bootstrap(x, 50, 1.0, 7, -1.0)
    ses = pd.Series(z.std(axis=0), index=list(d))
    assert [a.loc[n, "se"] for n in a.index] == [ses[n] for n in a.index]
    # an int seed also seeds NumPy's global generator (compare.py:548-549)
    pl.loo_compare(d, method="bb-pseudo-bma", b_samples=5, seed=99)
    first = np.random.random()
    np.random.seed(99)
    assert first == np.random.random()
    # a RandomState supplies the key with one randint call
    from pyloo_amd.compare import _seed_key

    assert _seed_key(np.random.RandomState(3)) == int(np.random.RandomState(3).randint(0, 2**64, dtype=np.uint64))
    assert 0 <= _seed_key(None) < 2**64
    with pytest.raises(TypeError):
        _seed_key(1.5)


def test_compare_weights_shapes(fake):
    import pyloo_amd as pl

    x = pointwise(3, 4, 100, "log")
    w, ses = pl.compare_weights(x)
    assert w.shape == (4,) and ses is None and abs(w.sum() - 1) < 1e-12
    w, ses = pl.compare_weights(x, method="bb-pseudo-bma", b_samples=20, seed=1)
    assert ses.shape == (4,)
    with pytest.raises(ValueError, match="64"):
        pl.compare_weights(np.zeros((65, 3)))
    with pytest.raises(ValueError, match="2-D"):
        pl.compare_weights(np.zeros(3))


# ---- static resources of the comparison kernels -------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_compare_kernel_resources(tmp_path):
    """No scratch, at most 192 vector registers (moments: three accumulators per model of an eight-model group), 128 elsewhere,
    and LDS for at least four workgroups per CU (160 KB)."""
    import isa_stats

    lines = isa_stats.compile_isa(out=str(tmp_path / "cmp.s"), units=["pla_k_compare.hip"])
    limits = {"compare_moments_kernelId": 192, "compare_moments_kernelIf": 192, "stacking_eval_kernelId": 128,
              "stacking_eval_kernelIf": 128, "bb_bootstrap_kernelId": 128, "bb_bootstrap_kernelIf": 128,
              "compare_moments_final_kernel": 64, "compare_tiles_sum_kernel": 64, "bb_final_kernel": 64, "bb_gamma_draws_kernel": 96}
    for pat, vgprs in limits.items():
        name, total, _, res = isa_stats.kernel_stats(lines, pat)
        assert res.get("ScratchSize", 0) == 0 and not any(k.startswith("scratch_") for k in total), (name, res)
        assert res["NumVgprs"] + res.get("NumAgprs", 0) <= vgprs, (name, res)
        assert 4 * res.get("LDSByteSize", 0) <= 160 * 1024, (name, res)
    for k in isa_stats.all_kernels(lines):
        assert not isa_stats.masked_spills(lines, k[2:]), k
