"""Leave-one-group-out on the GPU (``pla_group_sum`` / ``pla_psis_loo_groups``, ``pl.loo_group``): group sums bitwise NumPy's
``ll[members].sum(axis=0)``, the LOGO results against the reference's own numbers (tests/golden/loo_group.npz), singleton groups
against ``loo``, block-size independence, frozen engines and graph capture."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["int_f64", "int_f32", "str", "singleton", "heavy", "nan", "sis", "tis", "big"]
METHODS = {0: "psis", 1: "sis", 2: "tis"}
SCALES = {1: "log", -1: "negative_log", -2: "deviance"}
RTOL, ATOL = 1e-9, 1e-10  # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


@pytest.fixture(scope="module")
def gold(golden):
    return golden("loo_group")


def case(z, name):
    reff, m, sv = z[f"{name}__meta"]
    return z[f"{name}__ll"], z[f"{name}__ids"], float(reff), METHODS[int(m)], SCALES[int(sv)]


def as_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(getattr(x, "values", x))


def close(a, b, what, rtol=RTOL, atol=ATOL):
    a, b = as_numpy(a).astype(np.float64), np.asarray(b, dtype=np.float64)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


def check_result(res, z, name, pointwise):
    p = f"{name}__"
    method = case(z, name)[3]
    close(res["elpd_logo"], z[p + "elpd_logo"], "elpd_logo")
    close(res["se"], z[p + "se"], "se", rtol=1e-8)
    close(res["p_logo"], z[p + "p_logo"], "p_logo", rtol=1e-8, atol=1e-6)
    close(res["p_logo_se"], z[p + "p_logo_se"], "p_logo_se", rtol=1e-8)
    close(res["logoic"], z[p + "logoic"], "logoic")
    assert res["n_groups"] == len(z[p + "labels"]) and res["n_samples"] == z[p + "ll"].shape[1]
    assert bool(res["warning"]) == bool(z[p + "warning"])
    if method == "psis":
        assert res["good_k"] == pytest.approx(float(z[p + "good_k"]), rel=1e-15)
    if pointwise:
        close(res["logo_i"], z[p + "logo_i"], "logo_i")
        close(res["pareto_k" if method == "psis" else "ess"], z[p + "diag"], "diag")


def expected_warnings(z, name):
    _, _, _, method, _ = case(z, name)
    p = f"{name}__"
    out = []
    if bool(z[p + "has_nan"]):
        out.append("NaN values detected in log-likelihood. These will be ignored in the LOGO calculation.")
    if method != "psis":
        out.append(f"Using {method.upper()} for LOGO computation. Note that PSIS is the recommended method as it is typically more "
                   "efficient and reliable.")
    if method == "psis" and bool(z[p + "warning"]):
        gk = float(z[p + "good_k"])
        out.append(f"Estimated shape parameter of Pareto distribution is greater than {gk:.2f} for {int(z[p + 'n_high'])} groups. "
                   "This indicates that importance sampling may be unreliable because the marginal posterior and LOGO posterior are "
                   "very different.")
    if method != "psis" and bool(z[p + "warning"]):
        out.append(f"Low effective sample size detected (minimum ESS: {float(z[p + 'min_diag']):.1f}). This indicates that the "
                   "importance sampling approximation may be unreliable. Consider using PSIS which is more robust to such cases.")
    return out


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("pointwise", [True, False])
def test_golden_front(gold, name, pointwise):
    """pl.loo_group on a (chain, draw, obs) array: the matrix reaches the engine observations-fastest, as stack_samples gives it."""
    import pyloo_amd as pl
    from pyloo_amd.utils import SimpleInferenceData

    ll, ids, reff, method, scale = case(gold, name)
    arr = np.ascontiguousarray(ll.T).reshape(1, ll.shape[1], ll.shape[0])  # one chain: (chain, draw, obs)
    data = SimpleInferenceData(log_likelihood={"obs": arr}, posterior={"mu": np.zeros((1, ll.shape[1]))})
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_group(data, ids, pointwise=pointwise, reff=reff, scale=scale, method=method)
    assert [str(w.message) for w in rec] == expected_warnings(gold, name)
    check_result(res, gold, name, pointwise)
    if pointwise:
        assert list(np.asarray(getattr(res["logo_i"], "coords", {"group": gold[f"{name}__labels"]})["group"])) == list(
            gold[f"{name}__labels"])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("layout", ["draws", "obs"])
def test_golden_device(eng, gold, name, layout):
    """Group sums bitwise the reference's (NumPy's), LOGO results within the parity tolerances, device tensors in both layouts."""
    import torch

    import pyloo_amd as pl

    ll, ids, reff, method, scale = case(gold, name)
    t = torch.as_tensor(ll).cuda() if layout == "draws" else torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T
    index = pl.group_index(ids, device=t.device)
    sums, nrep = eng.group_sum(t, index)
    assert np.array_equal(sums.cpu().numpy(), gold[f"{name}__sums"]), name
    assert (int(nrep.item()) > 0) == bool(gold[f"{name}__has_nan"])
    host_sums, host_nrep = eng.group_sum(ll, pl.group_index(ids))
    assert np.array_equal(host_sums, gold[f"{name}__sums"]) and host_nrep == int(nrep.item())
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_group_from_matrix(t, ids if gold[f"{name}__ids"].dtype.kind in "U" else torch.as_tensor(ids).cuda(),
                                       reff=reff, scale=scale, method=method, pointwise=True)
    assert [str(w.message) for w in rec] == expected_warnings(gold, name)
    check_result(res, gold, name, True)


def reference_sums(ll, index):
    off, mem = index.offsets, index.members
    return np.stack([ll[mem[off[g]:off[g + 1]]].sum(axis=0) for g in range(index.n_groups)])


def labels_of(kind, N, G, rng):
    if kind == "contiguous":
        return np.minimum(np.arange(N) * G // max(N, 1), G - 1)
    if kind == "scattered":
        ids = np.arange(N) % G
        rng.shuffle(ids)
        return ids
    ids = rng.integers(0, G, size=N)  # skewed: one group holds half the observations
    ids[rng.random(N) < 0.5] = 0
    return ids


@pytest.mark.parametrize("N,S", [(1, 8), (7, 100), (7, 20000), (1000, 4000), (1000, 4097), (1000, 20000), (100003, 8), (100003, 100)])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_group_sums_bitwise_numpy(eng, N, S, dt):
    import torch

    import pyloo_amd as pl

    rng = np.random.default_rng(N * 31 + S)
    ll = (rng.normal(size=(N, S)) * rng.uniform(0.1, 50, size=(N, 1))).astype(dt)
    td = torch.as_tensor(ll).cuda()
    to = torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T
    for G in sorted({1, 3, 1000, N}):
        if G > N:
            continue
        for kind in ("contiguous", "scattered", "skewed"):
            index = pl.group_index(labels_of(kind, N, G, rng))
            want = reference_sums(ll, index)
            dindex = index.to(td.device)
            for t in (td, to):
                got, nrep = eng.group_sum(t, dindex)
                assert np.array_equal(got.cpu().numpy(), want), (G, kind, t.stride())
                assert int(nrep.item()) == 0
            got, _ = eng.group_sum(ll, index)
            assert np.array_equal(got, want), (G, kind, "host")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_group_sums_nan_and_strided_views(eng, dt):
    import torch

    import pyloo_amd as pl

    rng = np.random.default_rng(7)
    N, S = 777, 2 * 1500
    wide = rng.normal(size=(N, S)).astype(dt)
    hit = rng.random((N, S)) < 0.01
    wide[hit] = np.nan
    wide[0, 0] = np.inf
    wide[1, 2] = -np.inf
    ll = wide[:, ::2]  # a non-contiguous strided view
    nan_count = int(np.isnan(ll).sum())
    index = pl.group_index(rng.integers(0, 40, size=N))
    want = reference_sums(np.where(np.isnan(ll), dt(-1e10), ll), index)
    got, nrep = eng.group_sum(ll, index)
    assert np.array_equal(got, want, equal_nan=True) and nrep == nan_count
    t = torch.as_tensor(wide).cuda()[:, ::2]
    got, nrep = eng.group_sum(t, index.to(t.device))
    assert np.array_equal(got.cpu().numpy(), want, equal_nan=True) and int(nrep.item()) == nan_count


def test_singletons_equal_loo(eng):
    """Every group a singleton: bitwise the pointwise outputs of pla_psis_loo; aggregates within 1e-12 (another reduction order
    is allowed).  A permuted labelling gives the same numbers, reordered."""
    import torch

    import pyloo_amd as pl

    N, S, M = 3000, 4000, 190
    t = torch.empty((N, S), dtype=torch.float64, device="cuda")
    eng.fill_synthetic(t, seed=21, k_lo=0.05, k_hi=1.2)
    ref = eng.psis_loo(t, M, "psis", 1.0, 0.7)
    res = eng.psis_loo_groups(t, pl.group_index(torch.arange(N, device="cuda")), M, "psis", 1.0, 0.7)
    torch.cuda.synchronize()
    assert torch.equal(res["logo_i"], ref["loo_i"]) and torch.equal(res["diag"], ref["diag"]) and torch.equal(res["lppd_i"], ref["lppd_i"])
    for slot in (0, 1, 2, 3, 4, 6):
        np.testing.assert_allclose(res["agg"][slot].item(), ref["agg"][slot].item(), rtol=1e-12)
    perm = np.random.default_rng(3).permutation(N)
    res_p = eng.psis_loo_groups(t, pl.group_index(perm), M, "psis", 1.0, 0.7)  # observation i has label perm[i]
    order = torch.as_tensor(np.argsort(perm)).cuda()  # group g = observation argsort(perm)[g]
    for a, b in (("logo_i", "loo_i"), ("diag", "diag"), ("lppd_i", "lppd_i")):
        assert torch.equal(res_p[a], ref[b][order]), a
    a = pl.loo_group_from_matrix(t, np.arange(N), pointwise=True)
    b = pl.loo_from_matrix(t, pointwise=True)
    assert torch.equal(a["logo_i"], b["loo_i"])
    np.testing.assert_allclose(a["elpd_logo"], b["elpd_loo"], rtol=1e-12)


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import pyloo_amd as pl
from pyloo_amd.engine import get_engine
eng = get_engine(0)
rng = np.random.default_rng(5)
ll = (-rng.uniform(0.01, 0.1, size=(3000, 1)) * rng.exponential(size=(3000, 1000)) + rng.normal(size=(3000, 1))).astype(np.float64)
index = pl.group_index(rng.integers(0, 400, size=3000))
out = []
for src in (ll, torch.as_tensor(ll).cuda(), torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T):
    r = eng.psis_loo_groups(src, index, 190, "psis", 1.0, 0.7)
    out += [np.asarray(r[k].cpu() if hasattr(r[k], "cpu") else r[k]) for k in ("diag", "logo_i", "lppd_i", "agg")]
    s, _ = eng.group_sum(src, index)
    out.append(np.asarray(s.cpu() if hasattr(s, "cpu") else s))
np.savez(sys.argv[2], *out)
"""


def test_block_size_independence(tmp_path):
    """A one-megabyte ingest block (PLA_INGEST_BLOCK_MB=1: 131 groups per block of group sums -- four blocks of the 400 -- and 131
    observations per transposed block of the observations-fastest matrix) gives bitwise the default's outputs."""
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


def test_large_matrix_equals_loo_of_numpy_sums(eng):
    """N = 200 000 x S = 4000 f64, 2000 random groups: pointwise outputs bitwise pla_psis_loo of NumPy's group sums uploaded."""
    import torch

    import pyloo_amd as pl

    N, S, G, M = 200_000, 4000, 2000, 190
    t = torch.empty((N, S), dtype=torch.float64, device="cuda")
    eng.fill_synthetic(t, seed=0x51, k_lo=0.01, k_hi=0.05)
    ids = np.random.default_rng(11).integers(0, G, size=N)
    index = pl.group_index(ids)
    res = eng.psis_loo_groups(t, index.to(t.device), M, "psis", 1.0, 0.7)
    sums = torch.as_tensor(reference_sums(t.cpu().numpy(), index)).cuda()
    ref = eng.psis_loo(sums, M, "psis", 1.0, 0.7)
    torch.cuda.synchronize()
    for a, b in (("logo_i", "loo_i"), ("diag", "diag"), ("lppd_i", "lppd_i")):
        assert torch.equal(res[a], ref[b]), a
    for slot in (0, 1, 2, 3, 4, 6):
        np.testing.assert_allclose(res["agg"][slot].item(), ref["agg"][slot].item(), rtol=1e-12)


def test_frozen_engine_and_graph_capture():
    """The device call (the engine pass loo_group_from_matrix runs; the front's ELPDData needs the host) is captured in a graph
    once the engine is sized and frozen, and replays on new data bitwise like an eager call; a call that must grow is refused."""
    import torch

    import pyloo_amd as pl
    from pyloo_amd._capi import EngineError
    from pyloo_amd.engine import Engine

    own = Engine(0)
    try:
        N, S, M = 4000, 4000, 190
        t = torch.empty((N, S), dtype=torch.float64, device="cuda")
        own.fill_synthetic(t, seed=31)
        labels = torch.as_tensor(np.random.default_rng(2).integers(0, 300, size=N)).cuda()
        index = pl.group_index(labels)
        assert index.on_device
        warm = own.psis_loo_groups(t, index, M, "psis", 1.0, 0.7)
        torch.cuda.synchronize()
        own.set_frozen(True)
        bigger = torch.empty((N, 2 * S), dtype=torch.float64, device="cuda")
        own.fill_synthetic(bigger, seed=32)
        with pytest.raises(EngineError) as err:
            own.psis_loo_groups(bigger, index, M, "psis", 1.0, 0.7)
        assert err.value.code == -6
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = own.psis_loo_groups(t, index, M, "psis", 1.0, 0.7)
        own.fill_synthetic(t, seed=33)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        fresh = own.psis_loo_groups(t, index, M, "psis", 1.0, 0.7)
        torch.cuda.synchronize()
        for key in ("diag", "logo_i", "lppd_i", "agg", "n_replaced"):
            assert torch.equal(out[key], fresh[key]), key
        assert not torch.equal(out["logo_i"], warm["logo_i"])
    finally:
        own.set_frozen(False)
        own.close()
