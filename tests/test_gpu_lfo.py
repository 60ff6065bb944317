"""PSIS leave-future-out CV on the GPU (``pla_lfo_ratios``, ``pla_lfo``, ``Engine.lfo``, ``pl.loo_lfo_from_matrix``) through the C
ABI.  The log ratios are compared bit for bit with the restatement of the documented summation rule (tests/lfo_ref.py); k and
the pointwise predictive densities with the CPU oracle at the parity tolerances of tests/test_gpu_parity.py; layouts, memory
spaces, block sizes and repeated calls with one another bit for bit."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import lfo_ref
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-9, 1e-10  # tests/test_gpu_parity.py
C = lfo_ref.CHUNK


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def scalar(x):
    return int(host(x).reshape(-1)[0])


def cuda(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def show(what, got, want):
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    d = d[np.isfinite(d)]
    print(f"{what}: max |dev| = {d.max() if d.size else 0.0:.3e}")


def device_layouts(a):
    """draws fastest, observations fastest, and draws fastest with an odd pitch (rows that are not 16-byte aligned)."""
    import torch

    wide = torch.zeros((a.shape[0], a.shape[1] + 3), dtype=torch.as_tensor(a).dtype, device="cuda")
    wide[:, :a.shape[1]] = cuda(a)
    return {"draws": cuda(a), "obs": cuda(a.T).T, "pitch": wide[:, :a.shape[1]]}


# ------------------------------------------------------------------------------------------------------------- 1. the log ratios
@pytest.mark.parametrize("s,dtype", [(s, np.float64) for s in (5, 64, 100, 257, 4096, 4097)] + [(257, np.float32), (4097, np.float32)])
def test_ratios_equal_the_documented_rule_bitwise(eng, s, dtype):
    rng = np.random.default_rng(1000 + s)
    n = 7 + 2 * C + 1
    ll = lfo_ref.draw_ll(rng, n, s, dtype)
    ll[3, 1] = np.nan
    ll[9, s - 1] = np.nan
    ll[C + 5, 2] = np.nan
    ll[11, 0] = -np.inf
    t = cuda(ll)
    for first in (0, 1, 7):
        for n_steps in (1, 2, C - 1, C, C + 1, 2 * C + 1):
            want = lfo_ref.ratios(ll, first, n_steps)
            n_nan = int(np.isnan(ll[first:first + n_steps - 1]).sum())
            res = eng.lfo_ratios(t, first, n_steps)
            got = host(res["ratios"])
            assert got.dtype == np.float64 and got.shape == (n_steps, s)
            assert np.array_equal(got, want, equal_nan=True), (first, n_steps, np.argwhere(got != want)[:4])
            assert scalar(res["n_replaced"]) == n_nan, (first, n_steps)
            assert ("16-byte" in eng.last_kernels()) == (s % (2 if dtype == np.float64 else 4) == 0), eng.last_kernels()
    # -inf propagates from its row on, NaN counts as -1e10
    got = host(eng.lfo_ratios(t, 7, 2 * C + 1)["ratios"])
    assert np.all(got[5:, 0] == -np.inf) and np.isfinite(got[4, 0]) and got[3, s - 1] < -0.9e10
    # host input (both layouts) and the observations-fastest device layout: the same bits
    want = lfo_ref.ratios(ll, 1, 2 * C + 1)
    for src in (ll, np.ascontiguousarray(ll.T).T, cuda(ll.T).T):
        res = eng.lfo_ratios(src, 1, 2 * C + 1)
        assert np.array_equal(host(res["ratios"]), want, equal_nan=True)
        assert scalar(res["n_replaced"]) == int(np.isnan(ll[1:2 * C + 1]).sum())


# ------------------------------------------------------------------------------------------------------------------ 2. the pass
def make_case(name):
    """(ll, first, n_steps, M, reff)."""
    if name == "s257_max":  # n_steps at its maximum for every M: the last window ends on row N - 1
        return lfo_ref.draw_ll(np.random.default_rng(1), 90, 257), 7, None, (1, 2, 4), 1.0
    if name == "s4096_below_max":
        return lfo_ref.draw_ll(np.random.default_rng(2), 60, 4096), 5, 40, (2,), 1.0
    if name == "s4097":
        return lfo_ref.draw_ll(np.random.default_rng(3), 50, 4097), 0, None, (1, 4), 0.8
    if name == "s1000_f32":
        return lfo_ref.draw_ll(np.random.default_rng(4), 80, 1000, np.float32), 3, None, (1, 2), 1.0
    if name == "wide_ratios":  # ratios that span far more than 709 nats: the tail floor log(DBL_MIN) binds
        return 60.0 * lfo_ref.draw_ll(np.random.default_rng(5), 70, 500, k_lo=0.5, k_hi=1.5), 4, None, (1, 2), 1.0
    if name == "constant_rows":  # rows constant over the draws: constant ratios (k = inf) at the first steps, one more further on
        ll = lfo_ref.draw_ll(np.random.default_rng(6), 40, 300)
        ll[6] = -1.5
        ll[7] = -0.25
        ll[20] = -2.0
        return ll, 6, None, (1, 4), 1.0
    raise KeyError(name)


CASES = ["s257_max", "s4096_below_max", "s4097", "s1000_f32", "wide_ratios", "constant_rows"]


@pytest.mark.parametrize("name", CASES)
def test_pass_against_the_oracle(eng, name):
    ll, first, n_steps_given, horizons, reff = make_case(name)
    n, s = ll.shape
    tail = orc.tail_count(s, reff)
    t = cuda(ll)
    for M in horizons:
        n_steps = n - first - M + 1 if n_steps_given is None else n_steps_given
        ref = lfo_ref.lfo_pass(ll, first, n_steps, M, reff)
        k_ref = ref["diag"]
        if name == "wide_ratios":
            lr = ref["ratios"][-1]
            assert lr.max() - lr.min() > 709.0
        if name == "constant_rows":
            assert np.isinf(k_ref[1]) and np.isinf(k_ref[2]) and np.isfinite(k_ref[3:]).all()
        # a threshold no reference k comes near, so that a rounding-level difference cannot move first_high
        thr = 0.7
        assert np.all(np.abs(k_ref[np.isfinite(k_ref)] - thr) > 1e-3), (name, M)
        for src in (t, ll):
            res = eng.lfo(src, first, n_steps, M, tail, thr)
            k, elpd = host(res["diag"]), host(res["elpd_i"])
            show(f"{name} M={M} k", k, k_ref)
            show(f"{name} M={M} elpd", elpd, ref["elpd_i"])
            assert k[0] == 0.0 and np.array_equal(np.isinf(k), np.isinf(k_ref)) and np.all(k[np.isinf(k)] > 0)
            fin = np.isfinite(k_ref)
            np.testing.assert_allclose(k[fin], k_ref[fin], rtol=RTOL, atol=ATOL, err_msg=f"{name} M={M}")
            np.testing.assert_allclose(elpd, ref["elpd_i"], rtol=RTOL, atol=ATOL, err_msg=f"{name} M={M}")
            assert scalar(res["first_high"]) == ref["first_high"] == lfo_ref.first_high(k, thr)
            assert scalar(res["n_replaced"]) == 0
        assert ("registers" in eng.last_kernels()) == (s <= 4096), eng.last_kernels()


def test_first_high_thresholds_nan_count_and_errors(eng):
    from pyloo_amd._capi import EngineError

    ll = lfo_ref.draw_ll(np.random.default_rng(7), 50, 400, k_lo=0.4, k_hi=1.4)
    ll[12, 5] = np.nan   # inside the steps
    ll[2, 0] = np.nan    # before `first`: never read
    ll[49, 399] = np.nan  # the last row of the last window
    tail = orc.tail_count(400, 1.0)
    ref = lfo_ref.lfo_pass(ll, 4, 45, 2)
    assert ref["n_replaced"] == 2
    k_ref = ref["diag"]
    for thr in (-np.inf, 0.45, 0.7, np.inf):
        fin = k_ref[np.isfinite(k_ref)]
        assert np.all(np.abs(fin - thr) > 1e-3) or np.isinf(thr)
        for src in (cuda(ll), ll, cuda(ll.T).T):
            res = eng.lfo(src, 4, 45, 2, tail, thr)
            assert scalar(res["first_high"]) == lfo_ref.first_high(k_ref, thr), thr
            assert scalar(res["n_replaced"]) == 2
            np.testing.assert_allclose(host(res["elpd_i"]), ref["elpd_i"], rtol=RTOL, atol=ATOL)
    assert lfo_ref.first_high(k_ref, -np.inf) == 1 and lfo_ref.first_high(k_ref, np.inf) == 45
    for kwargs, code in ((dict(n_steps=46), -1), (dict(first=-1), -1), (dict(horizon=0), -1), (dict(method="sis"), -4),
                         (dict(tail_count=400), -1)):
        args = dict(first=4, n_steps=45, horizon=2, tail_count=tail, k_threshold=0.7, method="psis")
        args.update(kwargs)
        with pytest.raises(EngineError) as err:
            eng.lfo(cuda(ll), **args)
        assert err.value.code == code, kwargs


# ------------------------------------------------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("s,dtype", [(256, np.float64), (257, np.float64), (4100, np.float64), (260, np.float32)])
def test_layouts_and_memory_spaces_agree_bitwise(eng, s, dtype):
    """Draws fastest (16-byte loads when the rows allow), the same with an odd pitch (element loads), observations fastest
    (transposed block by block) and the two host layouts: one summation order, the same bits; twice the same call, too."""
    ll = lfo_ref.draw_ll(np.random.default_rng(50 + s), C + 30, s, dtype)
    ll[40, 3] = np.nan
    first, M = 3, 3
    n_steps = ll.shape[0] - first - M + 1
    tail = orc.tail_count(s, 1.0)
    srcs = dict(device_layouts(ll), host_draws=ll, host_obs=np.ascontiguousarray(ll.T).T)
    outs, texts = {}, {}
    for key, src in srcs.items():
        res = eng.lfo(src, first, n_steps, M, tail, 0.7)
        outs[key] = [host(res[k]) for k in ("diag", "elpd_i")] + [scalar(res["first_high"]), scalar(res["n_replaced"])]
        outs[key].append(host(eng.lfo_ratios(src, first, n_steps)["ratios"]))
        texts[key] = eng.last_kernels()
    again = eng.lfo(srcs["draws"], first, n_steps, M, tail, 0.7)
    assert np.array_equal(host(again["diag"]), outs["draws"][0]) and np.array_equal(host(again["elpd_i"]), outs["draws"][1])
    for key, out in outs.items():
        for a, b in zip(out, outs["draws"]):
            assert np.array_equal(a, b, equal_nan=True), key
    assert outs["draws"][3] == 1
    assert "element loads" in texts["pitch"], texts


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import lfo_ref
from pyloo_amd.engine import get_engine
eng = get_engine(0)
ll = lfo_ref.draw_ll(np.random.default_rng(9), 205, 4097)
ll[77, 11] = np.nan
out = []
for t in (torch.as_tensor(ll).cuda(), torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T):
    r = eng.lfo(t, 4, 200, 2, 193, 0.7)
    out += [r[k].cpu().numpy() for k in ("diag", "elpd_i", "first_high", "n_replaced")]
    out.append(eng.lfo_ratios(t, 4, 200)["ratios"].cpu().numpy())
np.savez(sys.argv[2], *out)
"""


def test_block_size_independence(tmp_path):
    """S = 4097 with 200 steps is 6.5 MB of ratios: PLA_INGEST_BLOCK_MB=1 cuts them into four blocks of one chunk each (31 rows
    fit, a block is a whole chunk at least), the last one ragged, and the carry goes from block to block.  Every output is the
    default's (one block), bit for bit, in both layouts, and the ratios are those of the documented rule."""
    outs = []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        env.update(env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            outs.append([z[k] for k in sorted(z.files, key=lambda s: int(s.split("_")[1]))])
    assert len(outs[0]) == 10
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    for j in range(5):  # the two layouts among each other
        assert np.array_equal(outs[0][j], outs[0][5 + j])
    assert int(outs[1][3][0]) == 1
    ll = lfo_ref.draw_ll(np.random.default_rng(9), 205, 4097)
    ll[77, 11] = np.nan
    assert np.array_equal(outs[1][4], lfo_ref.ratios(ll, 4, 200))


# -------------------------------------------------------------------------------------------------------------- 4. frozen engine
def test_frozen_engine():
    import torch

    from pyloo_amd._capi import EngineError
    from pyloo_amd.engine import Engine

    own = Engine(0)
    try:
        ll = lfo_ref.draw_ll(np.random.default_rng(12), 150, 1000)
        tail = orc.tail_count(1000, 1.0)
        for src in (cuda(ll), cuda(ll.T).T):
            warm = own.lfo(src, 10, 130, 3, tail, 0.7)
            torch.cuda.synchronize()
            own.set_frozen(True)
            again = own.lfo(src, 10, 130, 3, tail, 0.7)
            assert torch.equal(again["elpd_i"], warm["elpd_i"]) and torch.equal(again["diag"], warm["diag"])
            assert torch.equal(again["first_high"], warm["first_high"])
            torch.cuda.synchronize()
            own.set_frozen(False)
        own.set_frozen(True)
        big = lfo_ref.draw_ll(np.random.default_rng(13), 400, 1000)
        with pytest.raises(EngineError) as err:
            own.lfo(cuda(big), 10, 380, 3, tail, 0.7)
        assert err.value.code == -6
        torch.cuda.synchronize()
    finally:
        own.set_frozen(False)
        own.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. front
def test_front_on_the_device_against_the_walk():
    import pyloo_amd as pl

    N, L, M = 60, 8, 2
    gen = lambda t: lfo_ref.draw_ll(np.random.default_rng(700 + t), N, 500 + 4 * t, k_lo=0.3, k_hi=1.1)  # noqa: E731
    thr = 0.6
    seen = []

    def refit(t):  # deterministic: the matrix of a fit is keyed by n_train; device tensors, in turn alone and with a reff
        seen.append(t)
        m = cuda(gen(t))
        return (m, 0.9) if len(seen) % 2 else m

    seen_ref = []

    def refit_ref(t):
        seen_ref.append(t)
        return (gen(t), 0.9) if len(seen_ref) % 2 else gen(t)

    want = lfo_ref.lfo_walk(gen(L), L, M, refit_ref, thr, 1.0)
    assert len(want["refits"]) >= 2, want["refits"]
    # no k the walk compares lies near the threshold: a rounding-level difference cannot move a refit
    fin = want["k"][np.isfinite(want["k"])]
    assert np.all(np.abs(fin - thr) > 1e-3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = pl.loo_lfo_from_matrix(cuda(gen(L)), L, M, refit=refit, k_threshold=thr, pointwise=True)
    assert res["refits"] == want["refits"] == seen and res["n_refits"] == len(seen) and not rec
    lfo_i, k = np.asarray(res["lfo_i"])[L:N - M + 1], np.asarray(res["pareto_k"])[L:N - M + 1]
    show("front lfo_i", lfo_i, want["elpd"])
    show("front k", k, want["k"])
    np.testing.assert_allclose(lfo_i, want["elpd"], rtol=RTOL, atol=ATOL)
    assert np.array_equal(np.isinf(k), np.isinf(want["k"]))
    np.testing.assert_allclose(k[np.isfinite(k)], fin, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(res["elpd_lfo"], want["elpd"].sum(), rtol=1e-9)
    np.testing.assert_allclose(res["se"], (want["elpd"].size * np.var(want["elpd"])) ** 0.5, rtol=1e-9)
    assert res["n_samples"] == 500 + 4 * L and res["n_data_points"] == N - M - L + 1
    # a .T view of an (S, N) buffer is read in place; without a refit the Pareto warning counts the steps
    buf = cuda(gen(L).T)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        plain = pl.loo_lfo_from_matrix(buf.T, L, M, k_threshold=thr, pointwise=True)
    ref = lfo_ref.lfo_walk(gen(L), L, M, None, thr, 1.0)
    n_high = int(np.sum(ref["k"] > thr))
    assert n_high > 0 and any(f"for {n_high} steps" in str(w.message) for w in rec) and plain["warning"]
    np.testing.assert_allclose(np.asarray(plain["lfo_i"])[L:N - M + 1], ref["elpd"], rtol=RTOL, atol=ATOL)
