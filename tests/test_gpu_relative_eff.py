"""Relative MCMC efficiency on the GPU (``pla_relative_eff``, ``Engine.relative_eff``, ``pl.relative_eff_from_matrix``) through the
C ABI.  The values are compared with the NumPy restatement of the rule (tests/ess_ref.py) at the parity tolerances of
tests/test_gpu_parity.py; layouts, memory spaces, grid sizes, repeated calls and gathered chains with one another bit for bit."""

import functools

import numpy as np
import pytest

import ess_ref
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-10  # tests/test_gpu_parity.py
DTYPES = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    e = get_engine(0)
    yield e
    e.set_ess_grid(0)


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def scalar(x):
    return int(host(x).reshape(-1)[0])


def cuda(a):
    import torch

    return torch.as_tensor(np.array(a, order="C")).cuda()  # (a copy: the shared references are read-only)


def show(what, got, want):
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    d = d[np.isfinite(d)]
    print(f"{what}: max |dev| = {d.max() if d.size else 0.0:.3e}")


def device_layouts(a):
    """draws fastest, observations fastest, and draws fastest with an odd pitch (rows that are not 16-byte aligned)."""
    import torch

    t = cuda(a)
    wide = torch.zeros((a.shape[0], a.shape[1] + 3), dtype=t.dtype, device="cuda")
    wide[:, :a.shape[1]] = t
    return {"draws": t, "obs": cuda(a.T).T, "pitch": wide[:, :a.shape[1]]}


@functools.lru_cache(maxsize=None)
def reference(n_chains, n, log, dtype, split):
    """(matrix, raw r_eff, margin, stop) of one parity case, computed once."""
    mat = ess_ref.parity_matrix(n_chains, n, log, DTYPES[dtype])
    r, margin, stop = ess_ref.relative_eff(mat, n_chains, log, split, cap=False)
    for a in (mat, r, margin, stop):
        a.setflags(write=False)
    return mat, r, margin, stop


def close(got, want, margin, what):
    """The parity check over the rows whose deciding margin is not at rounding level; at most 1 % may be left out."""
    keep = margin >= ess_ref.MARGIN_FLOOR
    assert (~keep).sum() <= 0.01 * keep.size, (what, "rows left out", int((~keep).sum()))
    show(what, got[keep], want[keep])
    np.testing.assert_allclose(got[keep], want[keep], rtol=RTOL, atol=ATOL, err_msg=what)


# ------------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n_chains,n", ess_ref.PARITY_SHAPES)
def test_parity_with_the_restatement(eng, n_chains, n, dtype):
    limit = eng.ess_lds_max_draws()
    assert limit == 4096
    for log in (True, False):
        for split in (False, True):
            if split and n // 2 < 4:
                continue
            mat, want, margin, stop = reference(n_chains, n, log, dtype, split)
            t = cuda(mat)
            what = f"{n_chains}x{n} {dtype} log={log} split={split}"
            raw = eng.relative_eff(t, n_chains, log=log, split=split, cap=False)
            analysed = n_chains * (2 * (n // 2) if split else n)
            assert ("LDS" in eng.last_kernels()) == (analysed <= limit), eng.last_kernels()
            got = host(raw["r_eff"])
            assert got.dtype == np.float64 and got.shape == (mat.shape[0],) and scalar(raw["n_invalid"]) == 0
            close(got, want, margin, what)
            capped = host(eng.relative_eff(t, n_chains, log=log, split=split, cap=True)["r_eff"])
            assert np.array_equal(capped, np.minimum(got, 1.0)), what
            if not log and n >= 250:
                assert np.any(got > 1.0) and np.any(mat < 0)  # (antithetic rows: the raw ratio is above 1; negative values)
            if not split and (n_chains, n) in ((4, 250), (4, 1000)):
                assert stop.max() >= n  # (a row at phi = 0.99 whose chains have not mixed runs every lag)


# ------------------------------------------------------------------------------------------------------------ 2. invalid rows
@pytest.mark.parametrize("n_chains,n", [(2, 40), (1, 4100)])
def test_invalid_rows_give_nan_and_are_counted(eng, n_chains, n):
    mat = ess_ref.ar1_rows(np.random.default_rng(31), 9, n_chains, n, 0.5, log=True)
    base = host(eng.relative_eff(cuda(mat), n_chains)["r_eff"])
    bad = mat.copy()
    bad[1] = -1.25                  # constant
    bad[3] = -np.inf                # likelihood 0 everywhere
    bad[4, 7] = np.nan
    bad[6, n_chains * n - 1] = np.inf
    bad[7, ::3] = -np.inf           # likelihood 0 at some draws: an ordinary row
    want, margin, _ = ess_ref.relative_eff(bad, n_chains)
    for name, src in list(device_layouts(bad).items()) + [("host", bad)]:
        res = eng.relative_eff(src, n_chains)
        got = host(res["r_eff"])
        assert np.isnan(got[[1, 3, 4, 6]]).all() and scalar(res["n_invalid"]) == 4, name
        for i in (0, 2, 5, 8):
            assert got[i] == base[i], (name, i)  # (the neighbours keep their bits)
        assert np.isfinite(got[7]) and margin[7] >= ess_ref.MARGIN_FLOOR
        np.testing.assert_allclose(got[7], want[7], rtol=RTOL, atol=ATOL)
    # without log: a constant that no sum of the row reproduces exactly, and -inf, are invalid too
    raw = ess_ref.ar1_rows(np.random.default_rng(32), 4, n_chains, n, 0.5, log=False)
    raw[0] = 0.1
    raw[2, 5] = -np.inf
    res = eng.relative_eff(cuda(raw), n_chains, log=False)
    got = host(res["r_eff"])
    assert np.isnan(got[[0, 2]]).all() and np.isfinite(got[[1, 3]]).all() and scalar(res["n_invalid"]) == 2


# -------------------------------------------------------------------------------------------------- 3. bit-for-bit equalities
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n_chains,n,split", [(4, 250, False), (2, 33, True), (1, 4097, False)])
def test_layouts_memory_spaces_and_repeats_give_the_same_bits(eng, n_chains, n, split, dtype):
    mat = reference(n_chains, n, True, dtype, split)[0]
    first = host(eng.relative_eff(cuda(mat), n_chains, split=split, cap=False)["r_eff"])
    assert np.isfinite(first).all()
    for name, t in device_layouts(mat).items():
        got = host(eng.relative_eff(t, n_chains, split=split, cap=False)["r_eff"])
        assert np.array_equal(got, first), name
        assert ("transpose_rows_kernel" in eng.last_kernels()) == (name == "obs"), eng.last_kernels()
    for name, a in (("host", mat), ("host obs-fastest", np.ascontiguousarray(mat.T).T)):
        res = eng.relative_eff(a, n_chains, split=split, cap=False)
        assert isinstance(res["r_eff"], np.ndarray) and res["n_invalid"] == 0
        assert np.array_equal(res["r_eff"], first), name
    assert np.array_equal(host(eng.relative_eff(cuda(mat), n_chains, split=split, cap=False)["r_eff"]), first)


@pytest.mark.parametrize("n_obs", [1, 3, 257])
def test_grid_of_one_workgroup_gives_the_same_bits(eng, n_obs):
    """One workgroup (one wavefront) takes every row in turn, the ragged end included; by default a workgroup takes one."""
    for n_chains, n, rows in ((4, 250, n_obs), (2, 33, n_obs), (1, 4100, min(n_obs, 3))):
        rng = np.random.default_rng(500 + n_obs + n)
        mat = np.concatenate([ess_ref.ar1_rows(rng, rows, n_chains, n, phi) for phi in (0.0, 0.9)])[1::2][:rows]
        for layout, t in device_layouts(mat).items():
            if layout == "pitch" or (layout == "obs" and rows == 1):
                continue
            try:
                eng.set_ess_grid(0)
                free = host(eng.relative_eff(t, n_chains, cap=False)["r_eff"])
                eng.set_ess_grid(1)
                one = host(eng.relative_eff(t, n_chains, cap=False)["r_eff"])
                eng.set_ess_grid(2)
                two = host(eng.relative_eff(t, n_chains, cap=False)["r_eff"])
            finally:
                eng.set_ess_grid(0)
            assert np.isfinite(free).all() and np.array_equal(one, free) and np.array_equal(two, free), (n_chains, n, layout)


def test_unsorted_chain_id_equals_the_gathered_matrix(eng):
    import pyloo_amd as pl

    rng = np.random.default_rng(41)
    ll = ess_ref.ar1_rows(rng, 6, 3, 50, 0.5)
    chain_id = np.tile([7, 2, 5], 50)
    mixed = np.ascontiguousarray(ll.reshape(6, 3, 50)[:, [2, 0, 1], :].transpose(0, 2, 1).reshape(6, 150))
    assert np.array_equal(mixed[:, np.argsort(chain_id, kind="stable")], ll)
    want = host(eng.relative_eff(cuda(ll), 3)["r_eff"])
    got = pl.relative_eff_from_matrix(cuda(mixed), chain_id=chain_id)
    assert hasattr(got, "detach") and got.is_cuda and np.array_equal(host(got), want)
    got = pl.relative_eff_from_matrix(mixed, chain_id=chain_id)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert np.array_equal(host(pl.relative_eff_from_matrix(cuda(ll), n_chains=3)), want)
    assert np.array_equal(pl.relative_eff(np.ascontiguousarray(ll.T.reshape(3, 50, 6))), want)  # (chain, draw, obs)


# ---------------------------------------------------------------------------------------------------------- 4. scale invariance
def test_a_constant_added_to_a_log_row_changes_nothing(eng):
    mat, want, margin, _ = reference(4, 250, True, "f64", False)
    shift = (np.arange(mat.shape[0])[:, None] - 7.0) * 113.25
    got = host(eng.relative_eff(cuda(mat + shift), 4, cap=False)["r_eff"])
    close(got, want, margin, "shifted rows")


# ----------------------------------------------------------------------------------------------------------------- 5. end to end
def test_loo_with_the_mean_efficiency_equals_the_oracle():
    import pyloo_amd as pl

    ll = ess_ref.ar1_rows(np.random.default_rng(51), 64, 4, 250, 0.5)
    r_ref, margin, _ = ess_ref.relative_eff(ll, 4)
    assert margin.min() >= ess_ref.MARGIN_FLOOR
    t = cuda(ll)
    r = pl.relative_eff_from_matrix(t, n_chains=4)
    reff = float(r.mean())
    np.testing.assert_allclose(reff, r_ref.mean(), rtol=RTOL)
    assert 0.2 < reff < 0.6 and orc.tail_count(1000, reff) == orc.tail_count(1000, r_ref.mean()) != orc.tail_count(1000, 1.0)
    res = pl.loo_from_matrix(t, reff=reff, pointwise=True)
    ref = orc.loo_arrays(ll, float(r_ref.mean()))
    show("loo_i", host(res["loo_i"]), ref["loo_i"])
    np.testing.assert_allclose(host(res["loo_i"]), ref["loo_i"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(host(res["pareto_k"]), ref["khat"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(float(res["elpd_loo"]), ref["elpd_loo"], rtol=RTOL)
