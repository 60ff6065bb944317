"""Approximate-posterior LOO on the GPU (``pla_gather_draws`` / ``pla_psis_loo_draws``, ``pl.loo_approximate_posterior``): the gather
bitwise NumPy's ``ll[:, idx]`` on every route, the pass bitwise ``pla_psis_loo`` of that matrix, the results against the reference's
own numbers (tests/golden/approx_posterior.npz), block-size independence, frozen engines and graph capture."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["psis_psis", "psir_psis", "nonfinite", "sis_sis", "psis_tis", "psir_tis", "sis_psis", "psir_sis", "f32", "nan", "heavy",
         "psis_sis", "sis_tis", "heavy_sis", "heavy_tis"]
METHODS = {0: "psis", 1: "sis", 2: "tis"}
SCALES = {1: "log", -1: "negative_log", -2: "deviance"}
RTOL, ATOL = 1e-9, 1e-10  # tests/test_gpu_parity.py
RTOL_TIED = 1e-8  # rows resampled with replacement (tied draws): tests/test_gpu_subsample.py


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


@pytest.fixture(scope="module")
def gold(golden):
    return golden("approx_posterior")


def case(z, name):
    reff, m, sv = z[f"{name}__meta"]
    return z[f"{name}__ll"], z[f"{name}__idx"], float(reff), METHODS[int(m)], SCALES[int(sv)]


def as_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(getattr(x, "values", x))


def close(a, b, what, rtol=RTOL, atol=ATOL):
    a, b = as_numpy(a).astype(np.float64), np.asarray(b, dtype=np.float64)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


def lds_max(dt):
    from pyloo_amd import _capi

    return _capi.load_library().pla_gather_lds_max_draws(_capi.dtype_code(dt))


def layouts(ll):
    """The matrix as the four inputs the calls take: host / device, draws fastest / observations fastest."""
    import torch

    flipped = np.ascontiguousarray(ll.T)
    return {"host": ll, "host_obs": flipped.T, "device": torch.as_tensor(ll).cuda(), "device_obs": torch.as_tensor(flipped).cuda().T}


def index_for(src, idx):
    import torch

    return torch.as_tensor(idx).cuda() if hasattr(src, "is_cuda") else idx


# ---------------------------------------------------------------------------------------------------- the gather
SHAPES = [(1, 8), (7, 100), (1000, 4000), (1000, 4097), (300, "lds_max"), (300, "lds_max + 1"), (100003, 100)]


@pytest.mark.parametrize("N,S", SHAPES)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_gather_bitwise_numpy(eng, N, S, dt):
    if isinstance(S, str):
        S = lds_max(dt) + (1 if S.endswith("1") else 0)
    rng = np.random.default_rng(N * 31 + S)
    ll = (rng.normal(size=(N, S)) * rng.uniform(0.1, 50, size=(N, 1))).astype(dt)
    indices = {
        "permutation": rng.permutation(S),
        "replacement": rng.integers(0, S, size=S),
        "short": rng.integers(0, S, size=max(2, S // 3 + 1)),
        "long": rng.integers(0, S, size=S + S // 2 + 3),
    }
    srcs = layouts(ll)
    for kind, idx in indices.items():
        want = ll[:, idx]
        for where, src in srcs.items():
            got, nrep = eng.gather_draws(src, index_for(src, idx))
            assert np.array_equal(as_numpy(got), want), (kind, where)
            assert int(as_numpy(nrep).reshape(-1)[0]) == 0, (kind, where)
            if hasattr(got, "is_cuda"):
                assert got.dtype == src.dtype and got.is_contiguous()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_gather_nan_inf_and_strided_views(eng, dt):
    import torch

    rng = np.random.default_rng(7)
    N, S = 777, 2 * 1500
    wide = rng.normal(size=(N, S)).astype(dt)
    wide[rng.random((N, S)) < 0.01] = np.nan
    wide[0, 0] = np.inf
    wide[1, 2] = -np.inf
    ll = wide[:, ::2]  # a non-contiguous strided view
    idx = rng.integers(0, ll.shape[1], size=ll.shape[1])
    idx[:3] = [0, 1, 0]  # the infinities are selected (one of them twice)
    picked = ll[:, idx]
    nan_count = int(np.isnan(picked).sum())
    assert nan_count > 0
    want = np.where(np.isnan(picked), dt(-1e10), picked)
    assert np.isposinf(want[0, 0]) and np.isneginf(want[1, 1]) and np.isposinf(want[0, 2])
    got, nrep = eng.gather_draws(ll, idx)
    assert np.array_equal(got, want) and nrep == nan_count
    t = torch.as_tensor(wide).cuda()[:, ::2]
    got, nrep = eng.gather_draws(t, torch.as_tensor(idx).cuda())
    assert np.array_equal(got.cpu().numpy(), want) and int(nrep.item()) == nan_count
    t_obs = torch.as_tensor(np.ascontiguousarray(wide.T)).cuda().T[:, ::2]  # observations fastest, every other draw
    got, nrep = eng.gather_draws(t_obs, torch.as_tensor(idx).cuda())
    assert np.array_equal(got.cpu().numpy(), want) and int(nrep.item()) == nan_count


def test_device_index_is_clamped_and_host_index_checked(eng):
    import torch

    rng = np.random.default_rng(3)
    ll = rng.normal(size=(50, 64))
    idx = np.array([-5, 0, 63, 64, 1000, 7])
    got, _ = eng.gather_draws(torch.as_tensor(ll).cuda(), torch.as_tensor(idx).cuda())
    assert np.array_equal(got.cpu().numpy(), ll[:, np.clip(idx, 0, 63)])
    for src in (ll, torch.as_tensor(ll).cuda()):
        with pytest.raises(IndexError, match=r"draw indices must lie in \[0, 64\)"):
            eng.gather_draws(src, idx)


def test_routes_by_shape(eng):
    """The route the launcher picks: row + 32-bit index within 80 KB of LDS -> <lds+index>; the row alone -> <lds>; longer rows ->
    <global>; observations fastest -> <tile>."""
    import torch

    def route(t, n_out):
        eng.gather_draws(t, torch.arange(n_out, device="cuda") % t.shape[1])
        return eng.last_kernels()

    for dt in (torch.float64, torch.float32):
        esz, top = (8, lds_max(np.float64)) if dt == torch.float64 else (4, lds_max(np.float32))
        z = lambda n, s: torch.zeros((n, s), dtype=dt, device="cuda")  # noqa: E731
        assert "gather_draws_kernel<lds+index>" in route(z(1000, 4000), 4000)  # 4000 e + 16 000 <= 81 920
        fit = (80 * 1024 - 4096 * esz) // 4  # the longest index that still fits beside a row of 4096 draws
        assert "gather_draws_kernel<lds+index>" in route(z(300, 4096), fit)
        assert "gather_draws_kernel<lds>" in route(z(300, 4096), fit + 1)
        assert "gather_draws_kernel<lds>" in route(z(300, top), top)
        assert "gather_draws_kernel<global>" in route(z(300, top + 1), top + 1)
        assert "gather_draws_kernel<tile>" in route(z(4000, 300).T, 4000)
        assert "gather_draws_kernel<global>" in route(z(300, 2 * 4000)[:, ::2], 4000)  # neither stride is 1


def test_host_matrix_in_several_blocks(eng):
    """A host matrix above the 1 GiB staging block (70 000 x 2000 f64: two blocks of the upload loop, buffers reused), both host
    layouts: the gather bitwise NumPy's, the pass bitwise the device call's."""
    import torch

    N, S = 70_000, 2000
    t = torch.empty((N, S), dtype=torch.float64, device="cuda")
    eng.fill_synthetic(t, seed=0x53, k_lo=0.05, k_hi=0.6)
    ll = t.cpu().numpy()
    assert ll.nbytes > 1 << 30
    idx = np.random.default_rng(13).integers(0, S, size=S)
    want = ll[:, idx]
    ref = eng.psis_loo_draws(t, torch.as_tensor(idx).cuda(), tail(S), "psis", 1.0, 0.7)
    for where, src in (("host", ll), ("host_obs", np.ascontiguousarray(ll.T).T)):
        got, nrep = eng.gather_draws(src, idx)
        assert np.array_equal(got, want) and nrep == 0, where
        assert "blocks of observations uploaded" in eng.last_kernels()
        assert_same_pass(eng.psis_loo_draws(src, idx, tail(S), "psis", 1.0, 0.7), ref, where)


# ---------------------------------------------------------------------------------------------------- the pass
def tail(n_out):
    from pyloo_amd.base import tail_count_for

    return tail_count_for(n_out, 1.0)


def assert_same_pass(res, ref, what):
    import torch

    torch.cuda.synchronize()
    for key in ("loo_i", "diag", "lppd_i"):
        assert np.array_equal(as_numpy(res[key]), as_numpy(ref[key])), (what, key)
    for slot in (0, 1, 2, 3, 4, 6):
        np.testing.assert_allclose(as_numpy(res["agg"])[slot], as_numpy(ref["agg"])[slot], rtol=1e-12, err_msg=f"{what} agg[{slot}]")


@pytest.mark.parametrize("method", ["psis", "sis", "tis"])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_pass_bitwise_psis_loo_of_the_numpy_gather(eng, method, dt):
    import torch

    N, S = 3000, 4000
    t = torch.empty((N, S), dtype=torch.float64, device="cuda")
    eng.fill_synthetic(t, seed=21, k_lo=0.05, k_hi=1.2)
    ll = t.cpu().numpy().astype(dt)
    rng = np.random.default_rng(5)
    for kind, idx in (("replacement", rng.integers(0, S, size=S)), ("short", rng.integers(0, S, size=2500)),
                      ("long", rng.integers(0, S, size=5000))):
        M = tail(len(idx)) if method == "psis" else 0
        ref = eng.psis_loo(torch.as_tensor(np.ascontiguousarray(ll[:, idx])).cuda(), M, method, 1.0, 0.7)
        for where, src in layouts(ll).items():
            res = eng.psis_loo_draws(src, index_for(src, idx), M, method, 1.0, 0.7)
            assert_same_pass(res, ref, (kind, where))
            assert int(as_numpy(res["n_replaced"]).reshape(-1)[0]) == 0


def test_large_matrix_equals_loo_of_the_numpy_gather(eng):
    """N = 200 000 x S = 4000 f64, index with replacement: pointwise outputs bitwise pla_psis_loo of NumPy's gather uploaded."""
    import torch

    N, S, M = 200_000, 4000, 190
    t = torch.empty((N, S), dtype=torch.float64, device="cuda")
    eng.fill_synthetic(t, seed=0x52, k_lo=0.01, k_hi=0.05)
    idx = np.random.default_rng(12).integers(0, S, size=S)
    res = eng.psis_loo_draws(t, torch.as_tensor(idx).cuda(), M, "psis", 1.0, 0.7)
    assert "gather_draws_kernel" in eng.last_kernels()
    gathered = torch.as_tensor(np.ascontiguousarray(t.cpu().numpy()[:, idx])).cuda()
    ref = eng.psis_loo(gathered, M, "psis", 1.0, 0.7)
    assert_same_pass(res, ref, "large")


def test_identity_and_evenly_spaced_indices(eng):
    import torch

    from pyloo_amd.loo_subsample import _thin

    N, S = 3000, 4000
    t = torch.empty((N, S), dtype=torch.float64, device="cuda")
    eng.fill_synthetic(t, seed=23, k_lo=0.05, k_hi=1.2)
    ref = eng.psis_loo(t, tail(S), "psis", 1.0, 0.7)
    res = eng.psis_loo_draws(t, torch.arange(S, device="cuda"), tail(S), "psis", 1.0, 0.7)
    assert_same_pass(res, ref, "identity")
    n = 1000
    cols = np.linspace(0, S - 1, n, dtype=int)
    ref = eng.psis_loo(_thin(t, n), tail(n), "psis", 1.0, 0.7)
    res = eng.psis_loo_draws(t, cols, tail(n), "psis", 1.0, 0.7)
    assert_same_pass(res, ref, "evenly spaced")


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from pyloo_amd.engine import get_engine
eng = get_engine(0)
rng = np.random.default_rng(5)
ll = (-rng.uniform(0.01, 0.1, size=(3000, 1)) * rng.exponential(size=(3000, 1000)) + rng.normal(size=(3000, 1))).astype(np.float64)
idx = rng.integers(0, 1000, size=1000)
out = []
for src in (ll, np.ascontiguousarray(ll.T).T, torch.as_tensor(ll).cuda(), torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T):
    r = eng.psis_loo_draws(src, idx, 190, "psis", 1.0, 0.7)
    out += [np.asarray(r[k].cpu() if hasattr(r[k], "cpu") else r[k]) for k in ("diag", "loo_i", "lppd_i", "agg")]
    g, _ = eng.gather_draws(src, idx)
    out.append(np.asarray(g.cpu() if hasattr(g, "cpu") else g))
np.savez(sys.argv[2], *out)
"""


def test_block_size_independence(tmp_path):
    """A one-megabyte ingest block (PLA_INGEST_BLOCK_MB=1: 131 observations per gathered block of the device matrices) gives
    bitwise the default's outputs; so do host and device input and the two layouts among each other.  The variable cuts only the
    device-resident inputs: the host inputs are one block here (their block is a fixed 1 GiB; several host blocks:
    test_host_matrix_in_several_blocks).  The block sizes are compared with array_equal on ALL of agg: slot 7, the count of rows
    left to the general kernel, is summed over the blocks by the call, and that equality is what holds it to be so."""
    outs = []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = dict(os.environ, **env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            outs.append([z[k] for k in sorted(z.files, key=lambda s: int(s.split("_")[1]))])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    first = outs[0][:5]
    for k in range(1, 4):  # the other sources against the first
        for j, (a, b) in enumerate(zip(first, outs[0][5 * k:5 * k + 5])):
            if j == 3:  # agg
                np.testing.assert_allclose(a[[0, 1, 2, 3, 4, 6]], b[[0, 1, 2, 3, 4, 6]], rtol=1e-12)
            else:
                assert np.array_equal(a, b), (k, j)


# ---------------------------------------------------------------------------------------------------- the reference's numbers
def check_result(res, z, name, pointwise):
    p = f"{name}__"
    ll, _, _, method, scale = case(z, name)
    tied = str(z[p + "resample"]) == "psir"
    rtol = RTOL_TIED if tied else RTOL
    close(res["elpd_loo"], z[p + "elpd_loo"], "elpd_loo", rtol=rtol)
    close(res["se"], z[p + "se"], "se", rtol=1e-8)
    close(res["p_loo"], z[p + "p_loo"], "p_loo", rtol=1e-8, atol=1e-6)
    close(res["p_loo_se"], z[p + "p_loo_se"], "p_loo_se", rtol=1e-8)
    close(res["looic"], z[p + "looic"], "looic", rtol=rtol)
    assert res["n_data_points"] == ll.shape[0] and res["n_samples"] == ll.shape[1]
    assert bool(res["warning"]) == bool(z[p + "warning"])
    if method == "psis":
        assert res["good_k"] == pytest.approx(float(z[p + "good_k"]), rel=1e-15)
    if pointwise:
        close(res["loo_i"], z[p + "loo_i"], "loo_i", rtol=rtol)
        close(res["pareto_k" if method == "psis" else "ess"], z[p + "diag"], "diag", rtol=rtol)


def expected_warnings(z, name):
    from test_approx_posterior_host import expected_warnings as host_expected

    return host_expected(z, name)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("pointwise", [True, False])
def test_golden_front(gold, monkeypatch, name, pointwise):
    """pl.loo_approximate_posterior on a (chain, draw, obs) array with the reference's recorded index: the matrix reaches the engine
    observations-fastest, as stack_samples gives it."""
    import importlib

    import pyloo_amd as pl
    from pyloo_amd.utils import SimpleInferenceData

    ll, idx, reff, method, scale = case(gold, name)
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_approximate_posterior"), "importance_resample",
                        lambda log_p, log_q, method="psis", seed=None: idx)
    arr = np.ascontiguousarray(ll.T).reshape(1, ll.shape[1], ll.shape[0])
    data = SimpleInferenceData(log_likelihood={"obs": arr}, posterior={"mu": np.zeros((1, ll.shape[1]))})
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_approximate_posterior(data, gold[f"{name}__log_p"], gold[f"{name}__log_q"], pointwise=pointwise, reff=reff,
                                           scale=scale, method=method)
    assert [str(w.message) for w in rec] == expected_warnings(gold, name)
    check_result(res, gold, name, pointwise)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("layout", ["draws", "obs", "host"])
def test_golden_from_matrix(eng, gold, name, layout):
    import torch

    import pyloo_amd as pl

    ll, idx, reff, method, scale = case(gold, name)
    if layout == "host":
        src, index = ll, idx
    else:
        src = torch.as_tensor(ll).cuda() if layout == "draws" else torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T
        index = torch.as_tensor(idx).cuda()
    got, nrep = eng.gather_draws(src, index)
    picked = ll[:, idx]
    assert np.array_equal(as_numpy(got), np.where(np.isnan(picked), ll.dtype.type(-1e10), picked))
    assert int(as_numpy(nrep).reshape(-1)[0]) == int(np.isnan(picked).sum())
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_approximate_posterior_from_matrix(src, index, reff=reff, scale=scale, method=method, pointwise=True)
    assert [str(w.message) for w in rec] == expected_warnings(gold, name)
    check_result(res, gold, name, True)


@pytest.mark.parametrize("resample_method", ["psis", "psir", "sis"])
def test_front_equals_from_matrix_with_the_same_seed(gold, resample_method):
    """End to end: the seeded front is bitwise the matrix entry point with importance_resample's index for that seed."""
    import pyloo_amd as pl
    from pyloo_amd.utils import SimpleInferenceData

    ll = gold["psir_psis__ll"]
    log_p, log_q = gold["psir_psis__log_p"], gold["psir_psis__log_q"]
    arr = np.ascontiguousarray(ll.T).reshape(1, ll.shape[1], ll.shape[0])
    data = SimpleInferenceData(log_likelihood={"obs": arr}, posterior={"mu": np.zeros((1, ll.shape[1]))})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = pl.loo_approximate_posterior(data, log_p, log_q, pointwise=True, seed=41, resample_method=resample_method)
        idx = pl.importance_resample(log_p, log_q, method=resample_method, seed=41)
        b = pl.loo_approximate_posterior_from_matrix(arr.reshape(ll.shape[1], ll.shape[0]).T, idx, reff=1.0, pointwise=True)
    assert (resample_method == "psir") == (len(np.unique(idx)) < len(idx))
    assert np.array_equal(as_numpy(a["loo_i"]), as_numpy(b["loo_i"])) and np.array_equal(as_numpy(a["pareto_k"]), as_numpy(b["pareto_k"]))
    for key in ("elpd_loo", "se", "p_loo", "p_loo_se", "looic", "looic_se", "good_k", "warning"):
        assert a[key] == b[key], key


# ---------------------------------------------------------------------------------------------------- frozen engines, graphs
def test_frozen_engine_and_graph_capture():
    """The device call is captured in a graph once the engine is sized and frozen, and replays on new data bitwise like an eager
    call; a call that must grow is refused."""
    import torch

    from pyloo_amd._capi import EngineError
    from pyloo_amd.engine import Engine

    own = Engine(0)
    try:
        N, S, M = 4000, 4000, 190
        t = torch.empty((N, S), dtype=torch.float64, device="cuda")
        own.fill_synthetic(t, seed=31)
        idx = torch.as_tensor(np.random.default_rng(2).integers(0, S, size=S)).cuda()
        warm = own.psis_loo_draws(t, idx, M, "psis", 1.0, 0.7)
        torch.cuda.synchronize()
        own.set_frozen(True)
        longer = torch.as_tensor(np.random.default_rng(3).integers(0, S, size=2 * S)).cuda()
        with pytest.raises(EngineError) as err:
            own.psis_loo_draws(t, longer, M, "psis", 1.0, 0.7)
        assert err.value.code == -6
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = own.psis_loo_draws(t, idx, M, "psis", 1.0, 0.7)
        own.fill_synthetic(t, seed=33)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        fresh = own.psis_loo_draws(t, idx, M, "psis", 1.0, 0.7)
        torch.cuda.synchronize()
        for key in ("diag", "loo_i", "lppd_i", "agg", "n_replaced"):
            assert torch.equal(out[key], fresh[key]), key
        assert not torch.equal(out["loo_i"], warm["loo_i"])
    finally:
        own.set_frozen(False)
        own.close()
