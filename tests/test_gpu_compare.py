"""loo_compare on the MI355X: the moments, stacking and Bayesian-bootstrap kernels (csrc/pla_compare.h) against the reference's
goldens (tests/golden/compare.npz) and against the NumPy restatement of the gamma stream (tests/compare_stream.py)."""

import os
import sys

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

from compare_cases import BB_ALPHAS, BB_INPUT, BB_SAMPLES, CASES, pointwise  # noqa: E402
from compare_stream import bb_z, gamma_draws, stacking_objective  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, "golden", "compare.npz"))
SCALE_MUL = {"log": 1.0, "negative_log": -1.0, "deviance": -0.5}


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    e = get_engine()
    e.set_compare_grid(0)
    return e


def elpd_data(x_k, scale, elpd):
    from pyloo_amd import ELPDData

    return ELPDData(data=[elpd, 1.0, 2.0, False, x_k, scale], index=["elpd_loo", "se", "p_loo", "warning", "loo_i", "scale"])


def table(case, method="stacking", device=False, **kw):
    import torch

    import pyloo_amd as pl

    seed, K, N, scale, kind = CASES[case]
    x = pointwise(seed, K, N, scale, kind)
    elpd = GOLD[f"{case}/elpd"]
    rows = [torch.from_numpy(x[k].copy()).cuda() if device else x[k] for k in range(K)]
    d = {f"m{k}": elpd_data(rows[k], scale, float(elpd[k])) for k in range(K)}
    return pl.loo_compare(d, method=method, **kw), x


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) if a.size else 0.0


@pytest.mark.parametrize("case", sorted(CASES))
def test_table_against_reference(case):
    _, K, _, scale, _ = CASES[case]
    df, x = table(case, method="pseudo-bma")
    names = [f"m{k}" for k in range(K)]
    order = GOLD[f"{case}/order"]
    assert list(df.index) == [names[i] for i in order]
    assert list(df.columns) == ["rank", "elpd_loo", "p_loo", "elpd_diff", "weight", "se", "dse", "warning", "scale"]
    got_diff = np.array([df.loc[n, "elpd_diff"] for n in names], dtype=float)
    got_dse = np.array([df.loc[n, "dse"] for n in names], dtype=float)
    want_diff, want_dse = GOLD[f"{case}/elpd_diff"], GOLD[f"{case}/dse"]
    assert np.all(np.abs(got_diff - want_diff) <= 1e-12 * np.abs(want_diff)), (got_diff, want_diff)
    assert np.all(np.abs(got_dse - want_dse) <= 1e-12 * np.abs(want_dse)), (got_dse, want_dse)
    w = np.array([df.loc[n, "weight"] for n in names])
    want = GOLD[f"{case}/pseudo_bma"]
    assert np.all(np.abs(w - want) <= 1e-12 * np.abs(want) + 1e-300), (w, want)
    assert (df["scale"] == scale).all()


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("device", [False, True])
def test_stacking_against_reference(case, device):
    _, K, _, scale, _ = CASES[case]
    df, x = table(case, device=device)
    names = [f"m{k}" for k in range(K)]
    w = np.array([df.loc[n, "weight"] for n in names], dtype=float)
    want = GOLD[f"{case}/stacking"]
    s = SCALE_MUL[scale]
    f_dev, f_ref = stacking_objective(x, w, s), stacking_objective(x, want, s)
    assert f_dev <= f_ref + 1e-6 * abs(f_ref) + 1e-12, (f_dev, f_ref)
    assert np.max(np.abs(w - want)) <= 1e-4, (w, want)
    assert abs(w.sum() - 1.0) <= 1e-12
    df2, _ = table(case, device=device)
    assert np.array_equal(df2["weight"].to_numpy(), df["weight"].to_numpy())  # two calls, the same bits


@pytest.mark.parametrize("alpha", [1.0, 0.5, 2.0])
def test_gamma_draws_match_the_specified_stream(eng, alpha):
    seed = 0x0123456789ABCDEF
    got = eng.bb_gamma_draws(seed, alpha, 48, 300)
    want = gamma_draws(seed, alpha, 48, 300)
    assert got.shape == (48, 300) and np.all(got > 0)
    assert rel(got, want) <= 1e-13


@pytest.mark.parametrize("alpha", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bb_replicates_match_the_restatement(eng, alpha, dtype):
    import torch

    x = pointwise(5, 3, 2000, "log").astype(dtype)
    seed = 987654321987
    want = bb_z(x.astype(np.float64), 64, alpha, seed, -0.5)
    host = eng.bb_bootstrap(x, 64, alpha, seed, -0.5)
    dev = eng.bb_bootstrap(torch.from_numpy(x).cuda(), 64, alpha, seed, -0.5).cpu().numpy()
    assert rel(host, want) <= 1e-12
    assert np.array_equal(host, dev)


def test_results_do_not_depend_on_the_grid(eng):
    import torch

    x = torch.from_numpy(pointwise(6, 5, 300_000, "log")).cuda()
    w = np.array([0.1, 0.2, 0.3, 0.15, 0.25])
    outs = []
    for cap in (0, 3, 37):
        eng.set_compare_grid(cap)
        outs.append((eng.compare_moments(x, 2).cpu().numpy(), eng.stacking_eval(x, w, -1.0),
                     eng.bb_bootstrap(x, 130, 0.7, 42, 1.0).cpu().numpy()))
    eng.set_compare_grid(0)
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0])
        assert o[1][0] == outs[0][1][0] and np.array_equal(o[1][1], outs[0][1][1])
        assert np.array_equal(o[2], outs[0][2])


def test_moments_and_stacking_eval_against_numpy(eng):
    x = pointwise(7, 6, 50_001, "deviance")
    m = eng.compare_moments(x, 4)
    for k in range(6):
        d = x[k] - x[4]
        assert rel(m[3 * k], x[k].sum()) <= 1e-12
        assert rel(m[3 * k + 2], np.sum((d - d.mean()) ** 2)) <= 1e-12 or k == 4
    assert m[3 * 4 + 2] == 0.0 and rel(m[18], x.max(axis=0).sum()) <= 1e-12
    w = np.array([0.3, 0.0, 0.1, 0.2, 0.25, 0.15])
    F, G = eng.stacking_eval(x, w, -0.5)
    xs = -0.5 * x.T
    e = np.exp(xs - xs.max(axis=1, keepdims=True))
    dd = e @ w
    assert rel(F, np.sum(np.log(dd))) <= 1e-12
    assert rel(G, (e / dd[:, None]).sum(axis=0)) <= 1e-12


@pytest.mark.parametrize("alpha", BB_ALPHAS)
def test_bb_weights_agree_with_reference_statistically(alpha):
    import pyloo_amd as pl

    seed, K, N, scale, kind = BB_INPUT
    x = pointwise(seed, K, N, scale, kind)
    w, ses = pl.compare_weights(x, method="bb-pseudo-bma", b_samples=BB_SAMPLES, alpha=alpha, seed=2024, scale=scale)
    from pyloo_amd.engine import get_engine

    z = get_engine().bb_bootstrap(x, BB_SAMPLES, alpha, 2024, 1.0)
    wr = np.exp(z - z.max(axis=1, keepdims=True))
    wr /= wr.sum(axis=1, keepdims=True)
    mc_se = np.sqrt(2.0) * wr.std(axis=0) / np.sqrt(BB_SAMPLES) + 1e-12
    want = GOLD[f"bb_a{alpha:g}/weights"]
    assert np.all(np.abs(w - want) < 5 * mc_se), (w, want, mc_se)
    want_ses = GOLD[f"bb_a{alpha:g}/ses"]
    assert np.all(np.abs(ses - want_ses) < 0.25 * want_ses), (ses, want_ses)
    assert abs(w.sum() - 1.0) <= 1e-12


def test_loo_compare_on_device_loo_vectors_at_scale():
    """N = 10^6, K = 4, B = 1000: the pointwise vectors stay on the device (the kernels read the stacked matrix in place)."""
    import torch

    import pyloo_amd as pl
    from pyloo_amd.engine import get_engine

    g = torch.Generator(device="cuda").manual_seed(3)
    common = torch.randn(1_000_000, device="cuda", dtype=torch.float64, generator=g)
    d = {}
    for k in range(4):
        v = -1.2 - 0.001 * k + 0.6 * common + 0.25 * torch.randn(1_000_000, device="cuda", dtype=torch.float64, generator=g)
        d[f"m{k}"] = elpd_data(v, "log", float(v.sum()))
    for method in ("bb-pseudo-bma", "stacking"):
        df = pl.loo_compare(d, method=method, seed=11)
        assert "(matrix read in place)" in get_engine().last_kernels()
        w = df["weight"].to_numpy(dtype=float)
        assert np.all(np.isfinite(w)) and abs(w.sum() - 1.0) <= 1e-12, w
        assert np.all(np.isfinite(df["dse"].to_numpy(dtype=float)))


def test_frozen_engine_refuses_to_grow():
    from pyloo_amd._capi import EngineError
    from pyloo_amd.engine import Engine

    e = Engine(0)
    try:
        x = pointwise(8, 3, 5000, "log")
        e.bb_bootstrap(x, 64, 1.0, 1)
        e.set_frozen(True)
        e.bb_bootstrap(x, 64, 1.0, 1)  # same shape: no new workspace
        with pytest.raises(EngineError) as err:
            e.bb_bootstrap(pointwise(8, 3, 400_000, "log"), 640, 1.0, 1)
        assert err.value.code == -6
        e.set_frozen(False)
    finally:
        e.close()


def test_model_limit(eng):
    import pyloo_amd as pl
    from pyloo_amd._capi import EngineError

    x = np.random.default_rng(0).normal(size=(65, 10))
    with pytest.raises(ValueError, match="64"):
        pl.compare_weights(x)
    with pytest.raises(EngineError) as err:
        eng.compare_moments(x, 0)
    assert err.value.code == -4
    w, _ = pl.compare_weights(x[:64], method="pseudo-bma")
    assert abs(w.sum() - 1) < 1e-12


def test_loo_compare_of_loo_from_matrix_results():
    """ELPDData of pl.loo_from_matrix (NumPy loo_i) compare end to end."""
    import pyloo_amd as pl

    rng = np.random.default_rng(9)
    mats = {f"m{k}": -0.5 * (rng.normal(size=(40, 1)) - 0.1 * k + 0.3 * rng.normal(size=(40, 400))) ** 2 for k in range(3)}
    pre = {n: pl.loo_from_matrix(m, pointwise=True) for n, m in mats.items()}
    a = pl.loo_compare(pre)
    assert isinstance(a, pd.DataFrame) and a["rank"].tolist() == [0, 1, 2]
    assert abs(a["weight"].sum() - 1) < 1e-12
