"""Host side of ``relative_eff`` without a GPU.  The yardstick first: the NumPy restatement of the rule (tests/ess_ref.py), its
two autocovariance routes against each other and against what the estimator must give on rows of known efficiency.  Then the
feature: the C exports and their argument checks, the front's argument checks, chain labels, and ingestion through a stand-in
engine on the restatement, and the generated code of the new kernels."""

import importlib
import os
import re
import sys

import numpy as np
import pytest

import ess_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((4, 250), (1, 1000), (4, 1000), (2, 33), (3, 4))


# ------------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("log", [True, False])
def test_direct_and_fft_autocovariances_agree(log):
    worst, ran_every_lag = 0.0, False
    for ci, (C, n) in enumerate(SHAPES):
        for fi, phi in enumerate(ess_ref.FAMILIES.values()):
            mat = ess_ref.ar1_rows(np.random.default_rng(1000 + 10 * ci + fi), 4, C, n, phi, log)
            for split in (False, True):
                if split and n // 2 < 4:
                    continue
                a, margin, stop = ess_ref.relative_eff(mat, C, log, split, cap=False)
                b, _, stop_b = ess_ref.relative_eff(mat, C, log, split, cap=False, fft=True)
                assert np.all(np.isfinite(a)) and np.all(a > 0) and np.array_equal(stop, stop_b)
                worst = max(worst, float(np.max(np.abs(a - b) / np.abs(a))))
                ran_every_lag = ran_every_lag or bool(np.any(stop >= (n // 2 if split else n)))
    assert worst <= 1e-12, worst
    assert ran_every_lag  # (the families hold rows that Geyer's rule never stops: chains at phi = 0.99 that have not mixed)


def test_iid_rows_have_efficiency_one():
    mat = ess_ref.ar1_rows(np.random.default_rng(2), 200, 4, 250, 0.0, log=False)
    r = ess_ref.relative_eff(mat, 4, log=False, cap=False)[0]
    assert abs(r.mean() - 1.0) <= 0.1, r.mean()
    assert np.all(ess_ref.relative_eff(mat[:20], 4, log=False, cap=True)[0] <= 1.0)


def test_ar1_rows_have_the_textbook_efficiency():
    phi = 0.5
    mat = ess_ref.ar1_rows(np.random.default_rng(3), 40, 4, 1000, phi, log=False)
    r = ess_ref.relative_eff(mat, 4, log=False, cap=False)[0]
    want = (1 - phi) / (1 + phi)
    assert abs(r.mean() - want) <= 0.2 * want, (r.mean(), want)
    anti = ess_ref.relative_eff(ess_ref.ar1_rows(np.random.default_rng(4), 10, 4, 1000, -0.5, log=False), 4, log=False, cap=False)[0]
    assert np.all(anti > 1.0)  # (antithetic chains: the raw ratio is above 1, the cap returns 1)


def test_split_equals_unsplit_on_the_presplit_array():
    for C, n0, log in ((4, 250, True), (2, 33, False), (3, 9, True)):
        mat = ess_ref.ar1_rows(np.random.default_rng(5), 6, C, n0, 0.5, log)
        n = n0 // 2
        x = mat.reshape(6, C, n0)
        pre = np.stack([x[:, :, :n], x[:, :, n0 - n:]], axis=2).reshape(6, 2 * C * n)  # (the middle draw of an odd chain is gone)
        assert np.array_equal(ess_ref.relative_eff(mat, C, log, split=True)[0], ess_ref.relative_eff(pre, 2 * C, log, split=False)[0])


def test_invalid_rows_and_scale_invariance_of_the_restatement():
    mat = ess_ref.ar1_rows(np.random.default_rng(6), 6, 2, 40, 0.5, log=True)
    base = ess_ref.relative_eff(mat, 2)[0]
    shifted = ess_ref.relative_eff(mat + np.arange(6)[:, None] * 100.0 - 300.0, 2)[0]
    assert np.allclose(shifted, base, rtol=1e-9, atol=1e-10)
    bad = mat.copy()
    bad[0] = -1.25
    bad[1] = -np.inf
    bad[2, 7] = np.nan
    bad[3, 9] = np.inf
    bad[4, ::3] = -np.inf  # (likelihood 0 at some draws: an ordinary row)
    r = ess_ref.relative_eff(bad, 2)[0]
    assert np.isnan(r[:4]).all() and np.isfinite(r[4]) and r[5] == base[5]


def test_no_row_of_the_gpu_parity_cases_is_decided_at_rounding_level():
    """tests/test_gpu_relative_eff.py may leave out rows whose deciding margin is below MARGIN_FLOOR: its seeds leave out none."""
    smallest = np.inf
    for C, n in ess_ref.PARITY_SHAPES:
        for dtype in (np.float64, np.float32):
            for log in (True, False):
                mat = ess_ref.parity_matrix(C, n, log, dtype)
                assert mat.dtype == dtype and (log or (mat < 0).any())
                for split in (False, True):
                    if split and n // 2 < 4:
                        continue
                    r, margin, _ = ess_ref.relative_eff(mat, C, log, split, cap=False)
                    assert np.isfinite(r).all()
                    smallest = min(smallest, float(margin.min()))
    print(f"smallest deciding margin of the parity cases: {smallest:.3e}")
    assert smallest >= ess_ref.MARGIN_FLOOR


# ------------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (as tests/test_capi_abi.py: a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


def test_new_symbols_in_header_binding_and_library(lib):
    from pyloo_amd import _capi
    from pyloo_amd import build as b

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    for sym, n_args in (("pla_relative_eff", 13), ("pla_engine_set_ess_grid", 2), ("pla_ess_lds_max_draws", 0)):
        assert sym in _capi.SYMBOLS and hasattr(lib, sym)
        assert re.search(r"\bint " + sym + r"\(", header)
        assert len(getattr(lib, sym).argtypes) == n_args
    assert "pla_relative_eff" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"#define PLA_ABI_VERSION {lib.pla_abi_version()}" in header and lib.pla_abi_version() == _capi.ABI_VERSION == 7
    assert "pla_k_ess.hip" in b.SOURCES
    assert lib.pla_ess_lds_max_draws() == 4096
    for name, value in (("PLA_ESS_LOG", 1), ("PLA_ESS_SPLIT", 2), ("PLA_ESS_CAP", 4)):
        assert f"#define {name} {value}" in header and getattr(_capi, name) == value


def _ess(lib, eng=None, x=1, dtype=0, n_obs=10, n_draws=40, so=40, sd=1, n_chains=4, flags=1, space=1, out=1):
    """(status, text); x = out = 1: pointers that are never followed (every call here fails its argument checks first)."""
    rc = lib.pla_relative_eff(eng, x, dtype, n_obs, n_draws, so, sd, n_chains, flags, space, None, out, None)
    return rc, lib.pla_last_error().decode()


def test_null_engine_and_argument_errors(lib):
    assert _ess(lib) == (-1, "engine is NULL")
    for kwargs, code, word in (
        (dict(n_chains=3), -1, "does not divide"),
        (dict(n_chains=0), -1, "n_chains"),
        (dict(n_chains=20), -1, "at least 4"),          # 2 draws per chain
        (dict(n_chains=8, flags=3), -1, "after the split"),  # 5 draws per chain, 2 after the split
        (dict(flags=8), -1, "flags"),
        (dict(dtype=5), -1, "dtype"),
        (dict(space=3), -1, "mem_space"),
        (dict(n_obs=0), -1, "n_obs"),
        (dict(x=None), -1, "x is NULL"),
        (dict(out=None), -1, "r_eff"),
        (dict(so=0), -1, "strides"),
    ):
        rc, text = _ess(lib, **kwargs)
        assert rc == code and word in text, (kwargs, rc, text)
    assert _ess(lib, n_chains=10)[1] == "engine is NULL"          # (4 draws per chain pass)
    assert _ess(lib, n_chains=5, flags=7)[1] == "engine is NULL"  # (8 draws per chain, 4 after the split)
    assert lib.pla_engine_set_ess_grid(None, 1) == -1


# -------------------------------------------------------------------------------------------------------------------- the front
@pytest.fixture()
def fake(monkeypatch):
    eng = ess_ref.OracleEssEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.relative_eff"), "get_engine", lambda device=None: eng)
    return eng


def test_argument_checks_come_before_the_engine(monkeypatch):
    import pyloo_amd as pl

    def no_engine(device=None):
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(importlib.import_module("pyloo_amd.relative_eff"), "get_engine", no_engine)
    ll = ess_ref.ar1_rows(np.random.default_rng(7), 3, 4, 10, 0.5)
    cases = (
        (dict(n_chains=3), ValueError, "does not divide"),
        (dict(n_chains=0), ValueError, "n_chains"),
        (dict(chain_id=np.repeat([0, 1, 2], [14, 13, 13])), ValueError, "unequal"),
        (dict(chain_id=np.zeros(39, dtype=int)), ValueError, "length n_draws"),
        (dict(chain_id=np.repeat([0.0, 1.0], 20)), TypeError, "integer"),
        (dict(n_chains=20), ValueError, "at least 4"),
        (dict(n_chains=8, split=True), ValueError, "after the split"),
    )
    for kwargs, exc, text in cases:
        with pytest.raises(exc, match=text):
            pl.relative_eff_from_matrix(ll, **kwargs)
    with pytest.raises(TypeError, match="float32 or float64"):
        pl.relative_eff_from_matrix(np.zeros((3, 40), dtype=np.int64))
    with pytest.raises(TypeError, match="float32 or float64"):
        pl.relative_eff_from_matrix(np.zeros((3, 40), dtype=np.float16))
    for bad in (np.zeros(40), np.zeros((2, 3, 40))):
        with pytest.raises(ValueError, match="2-D"):
            pl.relative_eff_from_matrix(bad)


def test_front_passes_the_arguments_and_returns_the_vector(fake):
    import pyloo_amd as pl

    ll = ess_ref.ar1_rows(np.random.default_rng(8), 5, 4, 30, 0.5)
    r = pl.relative_eff_from_matrix(ll)
    assert isinstance(r, np.ndarray) and r.shape == (5,) and r.dtype == np.float64
    assert np.array_equal(r, ess_ref.relative_eff(ll, 4)[0])
    c = fake.calls[-1]
    assert (c["n_chains"], c["log"], c["split"], c["cap"]) == (4, True, False, True) and np.array_equal(c["x"], ll)
    r = pl.relative_eff_from_matrix(ll.astype(np.float32), n_chains=2, log=False, split=True, cap=False)
    c = fake.calls[-1]
    assert (c["n_chains"], c["log"], c["split"], c["cap"]) == (2, False, True, False) and c["x"].dtype == np.float32
    assert np.array_equal(r, ess_ref.relative_eff(ll.astype(np.float32), 2, False, True, False)[0])


def test_unsorted_chain_id_gathers_the_draws_chain_major(fake):
    import pyloo_amd as pl

    rng = np.random.default_rng(9)
    ll = ess_ref.ar1_rows(rng, 4, 3, 12, 0.5)
    # the draws of three chains interleaved as a sampler that writes one iteration of every chain at a time leaves them
    chain_id = np.tile([7, 2, 5], 12)
    mixed = ll.reshape(4, 3, 12)[:, [2, 0, 1], :].transpose(0, 2, 1).reshape(4, 36)  # label 7 = block 2, 2 = block 0, 5 = block 1
    r = pl.relative_eff_from_matrix(mixed, chain_id=chain_id)
    manual = mixed[:, np.argsort(chain_id, kind="stable")]
    assert np.array_equal(fake.calls[-1]["x"], manual) and np.array_equal(manual, ll) and fake.calls[-1]["n_chains"] == 3
    assert np.array_equal(r, ess_ref.relative_eff(ll, 3)[0])
    # labels that are chain-major already: the matrix goes to the engine as it is; n_chains comes from the labels
    pl.relative_eff_from_matrix(ll, n_chains=99, chain_id=np.repeat([4, 8, 9], 12))
    assert np.array_equal(fake.calls[-1]["x"], ll) and fake.calls[-1]["n_chains"] == 3


def test_relative_eff_on_dicts_and_chain_draw_arrays(fake):
    import pyloo_amd as pl

    rng = np.random.default_rng(10)
    arr = -3.0 + 0.7 * rng.standard_normal((2, 20, 3, 5))  # (chain, draw, *obs)
    want = ess_ref.relative_eff(np.moveaxis(arr.reshape(40, 3, 5), 0, -1).reshape(15, 40), 2)[0].reshape(3, 5)
    a = pl.relative_eff(arr)
    b = pl.relative_eff({"log_likelihood": {"y": arr}, "posterior": {"mu": np.zeros((2, 20))}}, var_name="y")
    for r in (a, b):
        assert np.shape(r) == (3, 5) and np.array_equal(np.asarray(r), want)
    assert fake.calls[-1]["n_chains"] == 2 and fake.calls[-1]["log"] is True and fake.calls[-1]["split"] is False
    s = pl.relative_eff(arr[:, :, 0, :], split=True, cap=False)
    assert np.shape(s) == (5,) and fake.calls[-1]["split"] is True and fake.calls[-1]["cap"] is False
    with pytest.raises(ValueError, match="at least 4"):
        pl.relative_eff(arr[:, :3])


def test_reff_none_is_untouched():
    """The feature is additive: ``reff=None`` still goes to ``loo._relative_efficiency`` (ArviZ's posterior ESS)."""
    import inspect

    from pyloo_amd import loo

    assert "relative_eff" not in inspect.getsource(loo).replace("_relative_efficiency", "")


# ------------------------------------------------------------------------------------------------------------- the generated code
def test_new_kernels_use_no_scratch_and_the_lds_they_declare(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    assert "pla_k_ess.hip" in isa_stats.KERNEL_UNITS and isa_stats.unit_of("ess_row_kernel") == ["pla_k_ess.hip"]
    lines = isa_stats.compile_isa(out=str(tmp_path / "ess.s"), units=["pla_k_ess.hip"])
    names = [k for k in isa_stats.all_kernels(lines) if "ess_" in k]
    assert len(names) == 4, names  # two dtypes x (LDS, global workspace)
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert not isa_stats.masked_spills(lines, k[2:]), name
        # on chip the LDS admits a wavefront per SIMD (five per CU) whatever the registers: the row in flight sits in 128 of them
        assert res["NumVgprs"] + res.get("NumAgprs", 0) <= (512 if "Lb1" in k else 128), (name, res)
        # a wavefront's row: 4096 f64; five workgroups of one wavefront share a CU's 160 KiB
        assert res.get("LDSByteSize", 0) == (32768 if "Lb1" in k else 0), (name, res)
