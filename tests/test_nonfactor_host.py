"""CPU tests of loo_nonfactor: the front's checks and warnings against the reference's texts, the closed-form beta, the NumPy
restatement against the reference goldens, the new kernels' resources and the ABI 7 exports."""

import os
import re
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
from nonfactor_cases import CASES, case_inputs  # noqa: E402

import nonfactor_ref  # noqa: E402

import pyloo_amd as pl  # noqa: E402


def _data(N=4, C=1, D=5, model="normal", drop=(), extra_obs=False):
    rng = np.random.default_rng(0)
    post = {"mu": rng.normal(size=(C, D, N)), "cov": np.broadcast_to(np.eye(N), (C, D, N, N)).copy(), "df": np.full((C, D), 5.0)}
    for k in drop:
        post.pop(k)
    obs = {"y": rng.normal(size=N)}
    if extra_obs:
        obs["z"] = rng.normal(size=N)
    return {"posterior": post, "observed_data": obs}


def _raises(exc, match, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(exc, match=match):
            pl.loo_nonfactor(**kw)


def test_model_type_checked_first():
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(ValueError, match=re.escape("Unsupported model_type: probit. Must be 'normal' or 'student_t'.")):
            pl.loo_nonfactor(_data(), model_type="probit")
    assert not rec


def test_argument_errors():
    _raises(TypeError, "observed_data group", data={"posterior": _data()["posterior"]})
    _raises(TypeError, "Valid scale values", data=_data(), scale="bits")
    _raises(ValueError, re.escape("Multiple variables found in observed_data: ['y', 'z']"), data=_data(extra_obs=True))
    _raises(ValueError, re.escape("Variable 'w' not found in observed_data group."), data=_data(), var_name="w")
    _raises(ValueError, re.escape("Posterior variable 'm' not found."), data=_data(), mu_var_name="m")
    _raises(ValueError, re.escape("Posterior variable 'K' not found."), data=_data(), cov_var_name="K")
    _raises(ValueError, re.escape("Posterior variable 'Q' not found."), data=_data(), prec_var_name="Q")
    _raises(ValueError, "Could not find posterior samples for covariance", data=_data(drop=("cov",)))
    bad = _data()
    bad["posterior"]["cov"] = bad["posterior"]["cov"][..., :3, :3]
    _raises(ValueError, re.escape("Covariance matrix 'cov' shape (3, 3) is incompatible with observed data size 4"), data=bad)
    bad = _data()
    bad["posterior"]["mu"] = bad["posterior"]["mu"][..., :3]
    _raises(ValueError, re.escape("Mean vector 'mu' shape (3,) is incompatible with observed data size 4."), data=bad)
    _raises(ValueError, "Invalid method 'xis'", data=_data(), method="xis", reff=1.0)
    _raises(ValueError, re.escape("Degrees of freedom variable 'nu' not found in posterior."), data=_data(), model_type="student_t",
            df_var_name="nu", reff=1.0)
    two_d = _data()
    two_d["observed_data"]["y"] = np.zeros((2, 2))
    _raises(ValueError, "must be 1-dimensional", data=two_d)


def test_validation_warnings_in_order():
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(ValueError):
            pl.loo_nonfactor(_data(drop=("cov",)), model_type="student_t", df_var_name="nu")
    texts = [str(w.message) for w in rec]
    assert texts[0].startswith("loo_nonfactor() with model_type='student_t' requires the correct model specification.")
    assert texts[1].startswith("Neither covariance nor precision matrix found in posterior.")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(ValueError):
            pl.loo_nonfactor(_data(), mu_var_name="m")
    assert str(rec[1].message).startswith("Mean vector 'm' not found in posterior.")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(ValueError):
            pl.loo_nonfactor(_data(), model_type="student_t", df_var_name="nu", reff=1.0)
    assert str(rec[1].message).startswith("Degrees of freedom variable 'nu' not found in posterior. Student-t models")


def test_too_many_observations_raise_before_the_engine():
    with pytest.raises(NotImplementedError, match="1024"):
        pl.nonfactor_log_lik(np.zeros(1025), np.zeros((1, 1025)), np.zeros((1, 1025, 1025)))


@pytest.mark.parametrize("N", [5, 50, 200])
def test_closed_form_beta(N):
    rng = np.random.default_rng(N)
    a = rng.normal(size=(N, N))
    P = a @ a.T + N * np.eye(N)
    y, mu = rng.normal(size=N), rng.normal(size=N)
    r = y - mu
    g = P @ r
    for i in range(0, N, max(1, N // 10)):
        closed = r @ g - g[i] ** 2 / P[i, i]
        assert abs(closed - nonfactor_ref.beta_by_deletion(y, mu, P, i)) <= 1e-12 * abs(r @ g)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_reference_goldens(name):
    with np.load(os.path.join(HERE, "golden", "nonfactor.npz")) as z:
        ref = z[f"{name}__ll"]
    N, C, D, model, *_ = CASES[name]
    y, mu, mat, df = case_inputs(name)
    ll, _ = nonfactor_ref.loglik(y, mu, mat, df, model)
    a, b = np.where(np.isnan(ll), -np.inf, ll), np.where(np.isnan(ref), -np.inf, ref)
    assert np.array_equal(np.isneginf(a), np.isneginf(b))
    m = np.isfinite(b)
    np.testing.assert_allclose(a[m], b[m], rtol=1e-9, atol=1e-9)


def test_nonfactor_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    assert "pla_k_nonfactor.hip" in isa_stats.KERNEL_UNITS
    text = "\n".join(isa_stats.compile_isa(units=["pla_k_nonfactor.hip"], out="/tmp/pla_isa_nonfactor.s"))
    blocks = re.split(r"\n\s+- \.", text[text.index("amdhsa.kernels"):])
    meta = {}
    for b in blocks:
        m = re.search(r"\.name:\s+(_ZN3pla\S*nonfactor_\S+)", b)
        if not m:
            continue
        vals = dict(re.findall(r"\.(vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", b))
        meta[m.group(1)] = {k: int(v) for k, v in vals.items()}
    assert len(meta) == 6, sorted(meta)  # lds, blocked and lu kernels, f64 and f32
    for name, r in meta.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 256, (name, r)
        limit = 80 * 1024 if "lds_kernel" in name else 64 * 1024  # LDS route: two workgroups per CU of 160 KiB
        assert r["group_segment_fixed_size"] <= limit, (name, r)


def test_abi7_exports():
    from pyloo_amd import _capi

    lib = _capi.load_library()
    assert lib.pla_abi_version() == 7
    for sym in ("pla_nonfactor_loglik", "pla_engine_set_nonfactor_route", "pla_engine_set_nonfactor_grid", "pla_nonfactor_lds_max_obs"):
        assert sym in _capi.SYMBOLS and hasattr(lib, sym)
    assert lib.pla_nonfactor_lds_max_obs() == 138
    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    assert "#define PLA_NONFACTOR_MAX_OBS 1024" in header and "#define PLA_MVN_STUDENT_T 1" in header


def test_cpu_tensors_take_the_host_path(monkeypatch):
    """CPU tensors are host memory: they reach the library as PLA_HOST (staged), never as device pointers."""
    torch = pytest.importorskip("torch")
    from pyloo_amd import _capi
    from pyloo_amd.engine import Engine

    seen = []

    class FakeLib:
        def pla_nonfactor_loglik(self, *args):
            seen.append(args[11])  # mem_space
            return 0

    eng = object.__new__(Engine)
    eng._lib, eng._h, eng.device = FakeLib(), None, 0
    N, S = 3, 4
    y, mu, cov = torch.zeros(N), torch.zeros(S, N), torch.eye(N).expand(S, N, N)
    ll, flags = eng.nonfactor_log_lik(y, mu, cov, None, "normal")
    assert seen == [_capi.PLA_HOST]
    assert isinstance(ll, np.ndarray) and ll.shape == (N, S) and flags.shape == (S,)


def test_restatement_of_an_overflowing_matrix():
    """numpy.linalg.inv of this finite matrix is all NaN (elimination overflows): the reference's row is NaN, so -inf."""
    big = 1e308
    bad = np.array([[[1.0, -big, -big], [1.0, big, big], [1.0, big, big]]])
    with np.errstate(all="ignore"):
        assert np.all(np.isnan(np.linalg.inv(bad[0])))
        ll, flags = nonfactor_ref.loglik(np.zeros(3), np.zeros((1, 3)), bad, None, "normal")
        llt, flagst = nonfactor_ref.loglik(np.zeros(3), np.zeros((1, 3)), bad, np.array([4.0]), "student_t")
    assert np.all(np.isnan(ll)) and flags[0] == 0
    assert np.all(np.isneginf(llt)) and flagst[0] == nonfactor_ref.BETA_NONFINITE  # beta is NaN: the beta warning
