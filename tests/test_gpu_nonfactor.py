"""GPU tests of loo_nonfactor (csrc/pla_nonfactor.h): every golden case of the reference through both fronts, every route
against the NumPy restatement, the status words, bit-identity across grids, staging blocks, memory spaces and dtypes, and a
frozen engine with graph capture."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
from nonfactor_cases import CASES, case_inputs  # noqa: E402

import nonfactor_ref  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "nonfactor.npz")
FRONT_ONLY = ("requires the correct model specification", "Note that PSIS is the recommended",
              "Could not reliably determine the observation dimension")
ROUTE_NAMES = {1: "nonfactor_lds_kernel", 2: "nonfactor_blocked_kernel", 3: "(every draw)"}


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def eng():
    from pyloo_amd.engine import get_engine

    e = get_engine(0)
    yield e
    e.set_nonfactor_route(0)
    e.set_nonfactor_grid(0)


def close(a, b, tol):
    """|a - b| <= tol * max(1, |b|), with identical -inf / NaN patterns."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isneginf(a), np.isneginf(b)) and np.array_equal(np.isnan(a), np.isnan(b))
    m = np.isfinite(b)
    err = np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m]))
    assert err.size == 0 or err.max() <= tol, err.max()


def spd_draws(N, S, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 10, size=(N, 2))
    d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1))
    ls = rng.uniform(0.5, 1.5, size=S)
    cov = np.exp(-d[None] / ls[:, None, None]) + 0.1 * np.eye(N)[None]
    mu = rng.normal(size=(S, N))
    y = rng.normal(size=N)
    df = rng.uniform(3, 10, size=S)
    return y, mu, cov, df


def _dict_input(name):
    N, C, D, model, kind, dt, *_ = CASES[name]
    y, mu, mat, df = case_inputs(name)
    post = {"mu": mu.reshape(C, D, N), kind: mat.reshape(C, D, N, N)}
    if model == "student_t":
        post["df"] = df.reshape(C, D)
    return {"posterior": post, "observed_data": {"y": y}}


def _check_result(res, gold, name, pointwise=True):
    g = lambda k: gold[f"{name}__{k}"]  # noqa: E731
    for k in ("elpd_loo", "se", "p_loo", "p_loo_se", "looic", "looic_se"):
        np.testing.assert_allclose(res[k], g(k), rtol=1e-9, atol=1e-10, err_msg=k)
    assert bool(res["warning"]) == bool(g("warning"))
    assert res.attrs == {"is_mvn": True, "model_type": CASES[name][3]}
    if pointwise:
        close(res["loo_i"], g("loo_i"), 1e-9)
        method = CASES[name][6]
        if method == "psis":
            np.testing.assert_allclose(np.asarray(res["pareto_k"]), g("diag"), atol=1e-6)
            assert res["good_k"] == g("good_k")
        else:
            np.testing.assert_allclose(np.asarray(res["ess"]), g("diag"), rtol=1e-9)


@pytest.mark.parametrize("name", list(CASES))
def test_golden_case_dict_front(name, gold):
    import pyloo_amd as pl

    N, C, D, model, kind, dt, method, scale, reff, special, seed = CASES[name]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_nonfactor(_dict_input(name), pointwise=True, reff=reff, scale=scale, method=method, model_type=model,
                               var_name="y", **({"prec_var_name": "prec"} if kind == "prec" else {}))
    texts = [str(w.message) for w in rec if issubclass(w.category, UserWarning)]
    assert texts[0].startswith(f"loo_nonfactor() with model_type='{model}' requires")
    assert [t for t in texts if not any(f in t for f in FRONT_ONLY)] == list(gold[f"{name}__warnings"])
    _check_result(res, gold, name)
    assert list(res.index) == (["elpd_loo", "se", "p_loo", "p_loo_se", "n_samples", "n_data_points", "warning", "loo_i", "scale",
                                "looic", "looic_se", "pareto_k" if method == "psis" else "ess"] + (["good_k"] if method == "psis" else []))


@pytest.mark.parametrize("name", list(CASES))
def test_golden_case_tensor_front(name, gold, eng):
    import torch

    import pyloo_amd as pl

    N, C, D, model, kind, dt, method, scale, reff, special, seed = CASES[name]
    y, mu, mat, df = (torch.as_tensor(a).cuda() for a in case_inputs(name))
    ll, flags = pl.nonfactor_log_lik(y, mu, mat, None, df, model)
    assert ll.is_cuda and flags.is_cuda
    ref_ll = np.where(np.isnan(gold[f"{name}__ll"]), -np.inf, gold[f"{name}__ll"])
    got = ll.cpu().numpy()
    close(np.where(np.isnan(got), -np.inf, got), ref_ll, 1e-9)
    route = "nonfactor_lds_kernel" if N <= 138 else "nonfactor_blocked_kernel"
    assert eng.last_kernels().startswith(route)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        kw = {"prec": mat} if kind == "prec" else {"cov": mat}
        res = pl.loo_nonfactor_from_arrays(y, mu, df=df, model_type=model, reff=reff, scale=scale, method=method, pointwise=True, **kw)
    texts = [str(w.message) for w in rec if issubclass(w.category, UserWarning)]
    assert texts == list(gold[f"{name}__warnings"])
    _check_result(res, gold, name)


def test_docstring_example_shape(gold):
    """The 25-point spatial model of the reference docstring (2 chains x 100 draws) gives the golden numbers."""
    import pyloo_amd as pl

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = pl.loo_nonfactor(_dict_input("sp25_normal"), var_name="y", mu_var_name="mu", cov_var_name="cov", pointwise=True, reff=1.0)
    _check_result(res, gold, "sp25_normal")


@pytest.mark.parametrize("N", [1, 2, 3, 17, 64, 137, 138, 139, 500, 1024])
@pytest.mark.parametrize("model", ["normal", "student_t"])
def test_routes_against_restatement(N, model, eng):
    """Every route the shape allows agrees with the NumPy restatement on SPD input.  Tolerance 1e-9 up to the LDS bound; at
    N >= 500 the condition numbers (up to ~1e3) times N * eps allow 1e-8 between two factorisations."""
    import torch

    S = 6 if N >= 500 else 24
    y, mu, cov, df = spd_draws(N, S, seed=N)
    ref, rflags = nonfactor_ref.loglik(y, mu, cov, df, model)
    tol = 1e-9 if N < 500 else 1e-8
    args = [torch.as_tensor(a).cuda() for a in (y, mu, cov, df)]
    outs = {}
    for route in (1, 2, 3):
        eng.set_nonfactor_route(route)
        ll, flags = eng.nonfactor_log_lik(*args, model=model)
        torch.cuda.synchronize()
        kn = eng.last_kernels()
        expect = ROUTE_NAMES[route] if not (route == 1 and N > 138) else ROUTE_NAMES[2]
        assert expect in kn, kn
        fl = flags.cpu().numpy()
        assert np.array_equal(fl & ~nonfactor_ref.GENERAL, rflags)
        if route == 3:
            assert np.all(fl & nonfactor_ref.GENERAL)
        else:  # SPD input: the Cholesky routes decline no draw
            assert np.all((fl & nonfactor_ref.GENERAL) == 0), fl
        close(ll.cpu().numpy(), ref, tol)
        outs[route] = ll.cpu().numpy()
    for route in (2, 3):  # the forced routes agree with one another
        close(outs[route], outs[1], tol)


def test_too_many_observations():
    import pyloo_amd as pl

    N = 1025
    with pytest.raises(NotImplementedError, match="1024"):
        pl.nonfactor_log_lik(np.zeros(N), np.zeros((2, N)), np.zeros((2, N, N)))


def test_too_many_observations_c_abi(eng):
    """Past the Python guard, the C ABI itself refuses N = 1025 with PLA_ERR_UNSUPPORTED."""
    from pyloo_amd._capi import EngineError

    N = 1025
    with pytest.raises(EngineError) as err:
        eng.nonfactor_log_lik(np.zeros(N), np.zeros((2, N)), np.broadcast_to(np.eye(N), (2, N, N)))
    assert err.value.code == -4


@pytest.mark.parametrize("route", [0, 3])
def test_overflowing_column_stays_in_bounds(route, eng):
    """A finite asymmetric matrix whose elimination overflows to an all-NaN pivot column: the LU pivot stays at row k, the NaN
    propagates, and the row is NaN (-inf after the front) as numpy.linalg.inv's all-NaN inverse makes it in the reference."""
    big = 1e308
    bad = np.array([[1.0, -big, -big], [1.0, big, big], [1.0, big, big]])
    y, mu, cov, df = spd_draws(3, 4, seed=7)
    cov[2] = bad
    eng.set_nonfactor_route(route)
    for model in ("normal", "student_t"):
        ll, flags = eng.nonfactor_log_lik(y, mu, cov, df, model)
        ref, rflags = nonfactor_ref.loglik(y, mu, cov, df, model)
        assert not np.any(np.isfinite(ref[:, 2])) and not np.any(np.isfinite(ll[:, 2]))
        assert flags[2] & nonfactor_ref.GENERAL
        assert np.array_equal(flags & ~nonfactor_ref.GENERAL, rflags)
        close(np.where(np.isnan(ll), -np.inf, ll), np.where(np.isnan(ref), -np.inf, ref), 1e-9)
    import torch

    import pyloo_amd as pl

    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_nonfactor_from_arrays(*(torch.as_tensor(a).cuda() for a in (y, mu)), cov=torch.as_tensor(cov).cuda(), reff=1.0,
                                           pointwise=True)
    assert any("Invalid values detected" in str(w.message) for w in rec)
    assert res["n_samples"] == 4 and res.attrs["model_type"] == "normal"


def test_status_words_and_clamp(eng):
    """Singular, non-finite, df <= 0, asymmetric, indefinite and clamped draws: status bits and rows as the restatement."""
    rng = np.random.default_rng(3)
    N, S = 12, 10
    y, mu, cov, df = spd_draws(N, S, seed=5)
    cov[0, 4, :] = cov[0, :, 4] = 0.0            # singular
    cov[1, 2, 3] = np.nan                        # non-finite matrix
    mu[2, 5] = np.inf                            # non-finite mean
    df[3] = -1.0                                 # df <= 0
    cov[4, 0, 1] += 0.5                          # asymmetric
    q, _ = np.linalg.qr(rng.normal(size=(N, N)))
    lam = np.linspace(-1.0, 2.0, N)
    cov[5] = (q * lam) @ q.T                     # symmetric indefinite: general route; some c_i <= 0 are clamped
    for model in ("normal", "student_t"):
        ll, flags = eng.nonfactor_log_lik(y, mu, cov, df, model)
        ref, rflags = nonfactor_ref.loglik(y, mu, cov, df, model)
        assert np.array_equal(flags & ~nonfactor_ref.GENERAL, rflags), (flags, rflags)
        assert flags[0] & nonfactor_ref.SINGULAR and flags[0] & nonfactor_ref.GENERAL
        assert flags[4] & nonfactor_ref.GENERAL and flags[5] & nonfactor_ref.GENERAL
        assert flags[5] & nonfactor_ref.CLAMPED
        assert np.all(np.isneginf(ll[:, :3]))
        close(np.where(np.isnan(ll), -np.inf, ll), np.where(np.isnan(ref), -np.inf, ref), 1e-9)


def test_bit_identity(eng):
    """Grid caps 1, 7 and the default, host vs device input, f32 vs the same values as f64, and two repeat calls: same bits."""
    import torch

    for N in (40, 200):
        y, mu, cov, df = (a.astype(np.float32) for a in spd_draws(N, 30, seed=N + 1))
        base, bflags = eng.nonfactor_log_lik(y, mu, cov, df, "student_t")
        runs = []
        for cap in (1, 7, 0):
            eng.set_nonfactor_grid(cap)
            runs.append(eng.nonfactor_log_lik(y, mu, cov, df, "student_t"))
        eng.set_nonfactor_grid(0)
        runs.append(eng.nonfactor_log_lik(*(a.astype(np.float64) for a in (y, mu, cov, df)), model="student_t"))
        dev = eng.nonfactor_log_lik(*(torch.as_tensor(a).cuda() for a in (y, mu, cov, df)), model="student_t")
        runs.append(tuple(t.cpu().numpy() for t in dev))
        for ll, fl in runs:
            assert np.array_equal(ll.view(np.int64), base.view(np.int64))
            assert np.array_equal(fl, bflags)


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from pyloo_amd.engine import get_engine
from test_gpu_nonfactor import spd_draws
eng = get_engine(0)
out = []
for N in (25, 150):
    y, mu, cov, df = spd_draws(N, 64, seed=9)
    for model in ("normal", "student_t"):
        out += list(eng.nonfactor_log_lik(y, mu, cov, df, model))
np.savez(sys.argv[2], *out)
"""


def test_staging_block_independence(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 gives the default's bits: the 64 draws in one block at N = 25 (209 fit), and in 13 blocks of at most
    5 at N = 150."""
    outs = []
    for i, extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        path = tmp_path / f"o{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=dict(os.environ, **extra), capture_output=True,
                              text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            outs.append([z[k] for k in sorted(z.files, key=lambda s: int(s.split("_")[1]))])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_frozen_engine_and_graph_capture():
    import torch

    from pyloo_amd._capi import EngineError
    from pyloo_amd.engine import Engine

    own = Engine(0)
    try:
        y, mu, cov, df = (torch.as_tensor(a).cuda() for a in spd_draws(150, 40, seed=21))
        warm, _ = own.nonfactor_log_lik(y, mu, cov, df, "student_t")
        torch.cuda.synchronize()
        own.set_frozen(True)
        y2, mu2, cov2, df2 = (torch.as_tensor(a).cuda() for a in spd_draws(300, 40, seed=22))
        with pytest.raises(EngineError) as err:
            own.nonfactor_log_lik(y2, mu2, cov2, df2, "student_t")
        assert err.value.code == -6
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out, oflags = own.nonfactor_log_lik(y, mu, cov, df, "student_t")
        mu.add_(0.25)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        fresh, fflags = own.nonfactor_log_lik(y, mu, cov, df, "student_t")
        torch.cuda.synchronize()
        assert torch.equal(out, fresh) and torch.equal(oflags, fflags)
        assert not torch.equal(out, warm)
    finally:
        own.set_frozen(False)
        own.close()
