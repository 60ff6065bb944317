"""Host side of ``loo_lfo(..., mode="backward")`` without a GPU.  The yardstick first: the NumPy restatement of backward PSIS-LFO-CV
(tests/lfo_bw_ref.py) against a model whose predictive densities are known in closed form, so that a sign or off-by-one error that
restatement and kernel shared could not hide.  Then the feature: the front through the oracle-backed stand-in engine (the walk, the
refit protocol, the warnings, the errors), forward calls that still reach an engine which does not know ``mode``, the flag of the C
ABI, and the generated code of the new kernel unit."""

import importlib
import os
import re
import shutil
import sys
import warnings

import numpy as np
import pytest

import lfo_bw_ref
import lfo_ref
from oracle import psis_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."
K_TEXT = "Estimated shape parameter of Pareto distribution is greater than"
C = lfo_ref.CHUNK


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def test_ratios_are_the_forward_rule_on_the_reversed_rows_negated():
    rng = np.random.default_rng(31)
    ll = lfo_ref.draw_ll(rng, 2 * C + 20, 5)
    last = 2 * C + 11
    lr = lfo_bw_ref.ratios(ll, last, last + 1)
    assert np.all(lr[0] == 0.0) and np.array_equal(lr[1], -ll[last - 1]) and np.array_equal(lr[2], -(ll[last - 1] + ll[last - 2]))
    # the chunks are counted from the fit downward: q = C + 1 is carry[1] + a_C, with carry[1] the sequential sum of C rows
    total = np.zeros(5)
    for q in range(C):
        total = total + ll[last - 1 - q]
    assert np.array_equal(lr[C], -total) and np.array_equal(lr[C + 1], -(total + ll[last - 1 - C]))
    # exact sums: the negated cumulative sum of the reversed rows
    exact = rng.integers(-4096, 4096, size=(C + 9, 3)).astype(np.float64) / 64.0
    want = -np.vstack([np.zeros((1, 3)), np.cumsum(exact[::-1], axis=0)])
    assert np.array_equal(lfo_bw_ref.ratios(exact, C + 9, C + 10), want)


def test_pass_geometry_exact_step_and_nan_count():
    ll = lfo_ref.draw_ll(np.random.default_rng(32), 30, 200)
    full = lfo_bw_ref.lfo_pass(ll, 30, 10, 3)  # the fit to all rows: t_0 = 27, no step is exact
    assert list(full["t"]) == list(range(27, 17, -1)) and np.all(full["diag"] != 0.0)
    assert np.array_equal(full["ratios"][0], -((ll[29] + ll[28]) + ll[27]))
    lw, k = orc.psis_row(full["ratios"][0], orc.tail_count(200, 1.0))
    assert full["diag"][0] == k and full["elpd_i"][0] == orc.lse(lw + ((ll[27] + ll[28]) + ll[29])) - orc.lse(lw)
    part = lfo_bw_ref.lfo_pass(ll, 20, 6, 3)  # a fit to the first 20: step 0 is t = 20, exact, and its window lies past `last`
    assert list(part["t"]) == [20, 19, 18, 17, 16, 15] and part["diag"][0] == 0.0
    assert part["elpd_i"][0] == orc.lse((ll[20] + ll[21]) + ll[22]) - np.log(200)
    assert np.array_equal(part["ratios"][1], -ll[19])
    near = lfo_bw_ref.lfo_pass(ll, 28, 4, 3)  # last within M of the end: t_0 = 27 = last - 1, not exact
    assert list(near["t"]) == [27, 26, 25, 24] and near["diag"][0] != 0.0 and np.array_equal(near["ratios"][0], -ll[27])
    assert lfo_bw_ref.first_high([9.0, 0.1, np.nan, 0.8], 0.7, 0) == 0 and lfo_bw_ref.first_high([9.0, 0.1, np.nan, 0.8], 0.7, 1) == 3
    assert lfo_bw_ref.first_high([0.1, np.nan], 0.7, 0) == 2
    bad = ll.copy()
    bad[14, 1] = np.nan  # below the lowest step: never read
    bad[15, 0] = np.nan  # the lowest step's first row
    bad[22, 7] = np.nan  # the last row of step 0's window
    bad[23, 7] = np.nan  # above it: never read
    assert lfo_bw_ref.lfo_pass(bad, 20, 6, 3)["n_replaced"] == 2


def _conjugate(seed, M, flip=False):
    """y ~ N(mu, 1), mu ~ N(0, 10^2): the backward walk of the restatement against the closed-form predictive densities.
    Returns (max |elpd_t - exact_t|, refits)."""
    N, L, S = 60, 10, 4000
    y = np.random.default_rng(100 + seed).normal(0.5, 1.0, N)
    rng = np.random.default_rng(seed)  # the posterior draws of each fit, in walk order

    def fit(n):
        prec = n + 1.0 / 100.0
        mu = rng.normal(y[:n].sum() / prec, prec ** -0.5, S)
        return -0.5 * np.log(2 * np.pi) - 0.5 * (y[:, None] - mu[None, :]) ** 2

    def exact(t):  # log p(y_t .. y_{t+M-1} | y_<t) by the chain rule: each factor N(post mean, 1 + post var)
        out = 0.0
        for m in range(M):
            prec = (t + m) + 1.0 / 100.0
            mean, var = y[:t + m].sum() / prec, 1.0 + 1.0 / prec
            out += -0.5 * np.log(2 * np.pi * var) - 0.5 * (y[t + m] - mean) ** 2 / var
        return out

    keep = lfo_bw_ref.ratios
    if flip:
        lfo_bw_ref.ratios = lambda ll, last, n_q: -keep(ll, last, n_q)
    try:
        w = lfo_bw_ref.lfo_walk(fit(N), L, M, fit, 0.7)
    finally:
        lfo_bw_ref.ratios = keep
    want = np.array([exact(t) for t in range(L, N - M + 1)])
    return float(np.max(np.abs(w["elpd"] - want))), w["refits"]


@pytest.mark.parametrize("M", [1, 4])
def test_known_answer_conjugate_normal(M):
    """Measured on the CPU, seeds 1-3, S = 4000: max |elpd_t - exact_t| = 0.024-0.053 at M = 1 and 0.035-0.081 at M = 4 (Monte Carlo
    error of 4000 draws and of the importance weights), against >= 0.28 and >= 0.57 with the ratio's sign flipped; the walks refit
    at t = 18; 27; 29 and 13.  The bound 0.15 per step is about twice the worst right value and half the smallest wrong one."""
    for seed in (1, 2, 3):
        dev, refits = _conjugate(seed, M)
        wrong, _ = _conjugate(seed, M, flip=True)
        print(f"M={M} seed={seed}: max dev {dev:.3f}, wrong sign {wrong:.3f}, refits at {refits}")
        assert dev <= 0.15, (M, seed, dev)
        assert wrong > 0.15, (M, seed, wrong)
        assert refits == sorted(refits, reverse=True)


# -------------------------------------------------------------------------------------------------------------------- the front
@pytest.fixture()
def fake(monkeypatch):
    eng = lfo_bw_ref.OracleLfoEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_lfo"), "get_engine", lambda device=None: eng)
    return eng


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


def _gen(t, s, N, k_lo=0.05, k_hi=0.25):
    return lfo_ref.draw_ll(np.random.default_rng(500 + t), N, s, k_lo=k_lo, k_hi=k_hi)


@pytest.mark.parametrize("M", [1, 4])
def test_walk_with_refits_of_changing_draw_counts(fake, M):
    import pyloo_amd as pl

    N, L, thr = 48, 5, 0.5

    def make():
        seen = []

        def refit(t):  # in turn: a (matrix, reff) tuple; a log-likelihood alone, with another draw count
            seen.append(t)
            return (_gen(t, 90 + t, N), 0.8) if len(seen) % 2 else _gen(t, 90 + 2 * t, N)

        return refit, seen

    ll0 = _gen(N, 120, N)
    want = lfo_bw_ref.lfo_walk(ll0, L, M, make()[0], thr)
    refit, seen = make()
    res, msgs = quiet(pl.loo_lfo_from_matrix, ll0, L, M, refit=refit, k_threshold=thr, pointwise=True, mode="backward")
    assert len(want["refits"]) >= 2 and want["refits"] == sorted(want["refits"], reverse=True), want["refits"]
    assert res["refits"] == want["refits"] == seen and res["n_refits"] == len(seen) and res.lfo_mode == "backward"
    np.testing.assert_array_equal(np.asarray(res["lfo_i"])[L:N - M + 1], want["elpd"])
    np.testing.assert_array_equal(np.asarray(res["pareto_k"])[L:N - M + 1], want["k"])
    assert res["elpd_lfo"] == want["elpd"].sum() and res["n_data_points"] == N - M - L + 1 and res["n_samples"] == 120
    for t in res["refits"]:  # the k recorded at a refit step is the one that asked for it
        assert res["pareto_k"][t] > thr
    # the first pass serves the full fit; every later one starts at its fit's own step and goes down to L
    assert [c["first"] for c in fake.calls] == [N] + seen and all(c["mode"] == "backward" and c["horizon"] == M for c in fake.calls)
    assert [c["n_steps"] for c in fake.calls] == [N - M - L + 1] + [t - L + 1 for t in seen]
    assert fake.calls[1]["shape"][1] == 90 + seen[0] and fake.calls[1]["tail_count"] == orc.tail_count(90 + seen[0], 0.8)
    assert fake.calls[2]["tail_count"] == orc.tail_count(90 + 2 * seen[1], 0.8)  # (no reff of its own: the current one)
    assert not any(K_TEXT in m for m in msgs)
    assert list(res.index) == ["elpd_lfo", "se", "n_samples", "n_data_points", "warning", "lfo_i", "scale", "L", "M", "k_threshold",
                               "n_refits", "refits", "pareto_k", "good_k"]


def test_refit_at_the_very_first_step(fake):
    """With the full fit step N - M has already removed M rows: a threshold below its k asks for a refit there (first_high = 0),
    and with -inf every step is refitted and exact."""
    import pyloo_amd as pl

    N, L, M = 14, 4, 2
    mats = {t: lfo_ref.draw_ll(np.random.default_rng(100 + t), N, 50 + t) for t in range(L, N + 1)}
    called = []

    def refit(t):
        called.append(t)
        return mats[t]

    res, _ = quiet(pl.loo_lfo_from_matrix, mats[N], L, M, refit=refit, k_threshold=-np.inf, pointwise=True, mode="backward")
    steps = list(range(N - M, L - 1, -1))
    assert res["refits"] == steps == called and res["n_samples"] == 50 + N
    for t in steps:
        assert np.asarray(res["lfo_i"])[t] == orc.lse(mats[t][t] + mats[t][t + 1]) - np.log(50 + t), t
    first = lfo_bw_ref.lfo_pass(mats[N], N, N - M - L + 1, M, tail_count=orc.tail_count(50 + N, 1.0))
    assert res["pareto_k"][N - M] == first["diag"][0] != 0.0  # (the k that asked for the first refit)
    assert fake.calls[0]["first"] == N and fake.calls[1]["first"] == N - M


def test_without_refit_every_step_uses_the_full_fit_and_the_warnings(fake):
    import pyloo_amd as pl

    N, L, M = 30, 4, 1
    ll = _gen(N, 200, N, k_lo=0.05, k_hi=0.4)
    want = lfo_bw_ref.lfo_walk(ll, L, M)
    n_high = int(np.sum(want["k"] > 0.7))
    assert 0 < n_high < want["k"].size
    res, msgs = quiet(pl.loo_lfo_from_matrix, ll, L, M, pointwise=True, mode="backward")
    hit = [m for m in msgs if K_TEXT in m]
    assert len(hit) == 1 and f"0.70 for {n_high} steps." in hit[0] and res["warning"] and len(fake.calls) == 1
    np.testing.assert_array_equal(np.asarray(res["lfo_i"])[L:N - M + 1], want["elpd"])
    np.testing.assert_array_equal(np.asarray(res["pareto_k"])[L:N - M + 1], want["k"])
    assert np.all(np.isnan(np.asarray(res["lfo_i"])[:L])) and np.all(np.isnan(np.asarray(res["lfo_i"])[N - M + 1:]))
    calm, msgs = quiet(pl.loo_lfo_from_matrix, ll, L, M, k_threshold=np.inf, mode="backward")
    assert not msgs and not calm["warning"]
    bad = ll.copy()
    bad[7, 3] = np.nan
    bad[1, 0] = np.nan  # (below L: never read)
    _, msgs = quiet(pl.loo_lfo_from_matrix, bad, L, M, k_threshold=np.inf, mode="backward")
    assert msgs.count(NAN_TEXT) == 1
    bad = ll.copy()
    bad[1, 0] = np.nan
    _, msgs = quiet(pl.loo_lfo_from_matrix, bad, L, M, k_threshold=np.inf, mode="backward")
    assert not msgs


def test_error_cases(fake):
    import pyloo_amd as pl

    ll = lfo_ref.draw_ll(np.random.default_rng(20), 12, 40)
    with pytest.raises(ValueError, match="mode must be"):
        pl.loo_lfo_from_matrix(ll, 3, mode="combined")
    with pytest.raises(ValueError, match="mode must be"):
        pl.loo_lfo(np.zeros((2, 20, 12)), 3, reff=1.0, mode="sideways")
    with pytest.raises(ValueError, match="exceeds"):
        pl.loo_lfo_from_matrix(ll, 10, 3, mode="backward")
    assert not fake.calls
    with pytest.raises(ValueError, match="expected all 12"):
        pl.loo_lfo_from_matrix(ll, 3, refit=lambda t: ll[:11], k_threshold=-np.inf, mode="backward")
    assert len(fake.calls) == 1


def test_forward_calls_reach_an_engine_that_does_not_know_mode(monkeypatch):
    """tests/lfo_ref.py's stand-in has no ``mode`` parameter: a forward call that passed one would be a TypeError."""
    import pyloo_amd as pl

    eng = lfo_ref.OracleLfoEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_lfo"), "get_engine", lambda device=None: eng)
    ll = lfo_ref.draw_ll(np.random.default_rng(21), 15, 60)
    want = lfo_ref.lfo_walk(ll, 4, 2)
    for kwargs in ({}, {"mode": "forward"}):
        res, _ = quiet(pl.loo_lfo_from_matrix, ll, 4, 2, pointwise=True, **kwargs)
        assert res["elpd_lfo"] == want["elpd"].sum() and res.lfo_mode == "forward"
    with pytest.raises(TypeError):
        pl.loo_lfo_from_matrix(ll, 4, 2, mode="backward")


# ------------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (as tests/test_capi_abi.py: a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


BW = 0x100


def _lfo(lib, eng=None, ll=1, dtype=0, n_obs=100, n_draws=50, so=50, sd=1, last=100, n_steps=20, horizon=2, method=BW, tail=15, thr=0.7,
         space=1):
    """(status, text); ll = 1: a pointer that is never followed (every call here fails its argument checks first)."""
    rc = lib.pla_lfo(eng, ll, dtype, n_obs, n_draws, so, sd, last, n_steps, horizon, method, tail, thr, space, None, None, None, None, None)
    return rc, lib.pla_last_error().decode()


def test_flag_in_header_binding_and_library(lib):
    from pyloo_amd import _capi
    from pyloo_amd import build as b

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    assert re.search(r"^#define PLA_LFO_BACKWARD 0x100$", header, re.M) and _capi.PLA_LFO_BACKWARD == BW
    assert f"#define PLA_ABI_VERSION {lib.pla_abi_version()}" in header and lib.pla_abi_version() == _capi.ABI_VERSION == 7
    assert len(lib.pla_lfo.argtypes) == 19 and "pla_k_lfo_bw.hip" in b.SOURCES
    assert "PLA_LFO_BACKWARD" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_flag_with_a_null_engine_and_argument_errors(lib):
    assert _lfo(lib) == (-1, "engine is NULL")
    for kwargs, code, word in (
        (dict(last=0), -1, "last"),
        (dict(last=101), -1, "last"),
        (dict(horizon=0), -1, "horizon"),
        (dict(horizon=101), -1, "horizon"),
        (dict(n_steps=0), -1, "n_steps"),
        (dict(n_steps=100), -1, "n_steps"),           # t_0 = 98: 99 steps at most
        (dict(last=30, n_steps=32), -1, "n_steps"),   # t_0 = 30: 31 steps at most
        (dict(n_draws=1, so=1), -1, "n_draws"),
        (dict(method=BW | 1), -4, "method"),
        (dict(method=BW | 2), -4, "method"),
        (dict(method=BW | 7), -1, "method"),
        (dict(method=0x200), -1, "method"),
        (dict(method=0x300), -1, "method"),
        (dict(dtype=5), -1, "dtype"),
        (dict(space=3), -1, "mem_space"),
        (dict(ll=None), -1, "ll"),
        (dict(thr=float("nan")), -1, "k_threshold"),
        (dict(so=0), -1, "strides"),
    ):
        rc, text = _lfo(lib, **kwargs)
        assert rc == code and word in text, (kwargs, rc, text)
    assert _lfo(lib, n_steps=99)[1] == "engine is NULL" and _lfo(lib, last=30, n_steps=31)[1] == "engine is NULL"
    assert _lfo(lib, last=99, n_steps=99)[1] == "engine is NULL"  # (last within the horizon of the end: t_0 = 98 still)


# ------------------------------------------------------------------------------------------------------------- the generated code
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_backward_kernels_use_no_scratch_and_spill_no_scalars(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    lines = isa_stats.compile_isa(out=str(tmp_path / "lfo_bw.s"), units=["pla_k_lfo_bw.hip"])
    names = isa_stats.all_kernels(lines)
    # scan: totals / ratios x 16-byte / element loads x two dtypes; predict: two load modes x registers / streamed x two dtypes;
    # first-high -- the carries are forward mode's kernel, and none of its kernels is compiled a second time here
    assert len(names) == 8 + 8 + 1 and all("lfo_bw_" in k for k in names), names
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert not isa_stats.masked_spills(lines, k[2:]), name
        regs = res["NumVgprs"] + res.get("NumAgprs", 0)
        assert regs <= (256 if "lfo_bw_predict" in k else 128), (name, res)
