"""LOO-PIT on the GPU (``pla_loo_pit``, ``Engine.loo_pit``, ``pl.loo_pit``) through the C ABI: the reference's numbers
(tests/golden/loo_pit.npz), the kernels' shape edges and layouts against the NumPy restatement (tests/pit_ref.py), exactness and
determinism, block-size independence, the log-weights input, SIS / TIS, frozen engines and the front."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import pit_ref
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-9  # the bound tests/test_gpu_metrics.py holds e_loo-derived values to
CASES = ["edges_s500_r1", "poisson_s500_r1", "s1000_r0p7", "s1000_r1_f32", "s100_r1", "s4000_r1"]


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


@pytest.fixture(scope="module")
def gold():
    return pit_ref.load_golden()


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def cuda(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def show(what, got, want):
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    d = d[np.isfinite(d)]
    print(f"{what}: max |dev| = {d.max() if d.size else 0.0:.3e}")


def make(rng, n, s, dtype=np.float64):
    """Continuous log-likelihood rows (no ties in the tail), normal predictive draws, observations inside them."""
    k = rng.uniform(0.05, 0.9, size=(n, 1))
    ll = (-k * rng.exponential(size=(n, s)) - 1.0 - rng.uniform(size=(n, 1))).astype(dtype)
    mu = rng.normal(size=(n, 1))
    yh = (mu + rng.normal(size=(n, s))).astype(dtype)
    y = (mu + rng.normal(size=(n, 1))).reshape(n)
    return ll, yh, y


# ------------------------------------------------------------------------------------------------------------- 1. golden parity
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", CASES)
def test_golden_parity(eng, gold, name, where):
    c = gold[name]
    ll, yh, y = c["ll"], c["yh"], c["y"]
    M = orc.tail_count(ll.shape[1], c["reff"])
    if where == "device":
        res = eng.loo_pit(cuda(ll), cuda(yh), cuda(y), M, "psis")
    else:
        res = eng.loo_pit(ll, yh, y, M, "psis")
    le, lt, k, nrep = host(res["pit_le"]), host(res["pit_lt"]), host(res["diag"]), int(host(res["n_replaced"]).reshape(-1)[0])
    assert nrep == int(np.isnan(ll).sum())
    assert "pit_wave_kernel" in eng.last_kernels() and "pit_prepare" in eng.last_kernels()
    if ll.dtype == np.float64:
        want_le, want_lt = pit_ref.golden_expected(c)
        show(f"{name} {where} pit_le", le, want_le)
        show(f"{name} {where} pit_lt", lt, want_lt)
        np.testing.assert_allclose(le, want_le, rtol=0, atol=ATOL)
        np.testing.assert_allclose(lt, want_lt, rtol=0, atol=ATOL)
        np.testing.assert_allclose(k, c["k"], rtol=1e-9)
    else:
        # f32: the PIT computed in f64 from the fixture's weights rounded to f32; the bound is the weights' own tolerance in
        # tests/test_gpu_parity.py::test_golden_weights (rtol 2e-7, atol 1e-7 on lw) propagated to first order
        lw32 = c["lw"].astype(np.float32).astype(np.float64)
        want_le, want_lt = pit_ref.pit_from_log_weights(lw32, yh, y)
        w = np.exp(lw32 - np.max(lw32, axis=1, keepdims=True))
        w /= w.sum(axis=1, keepdims=True)
        bound = (w * (2e-7 * np.abs(lw32) + 1e-7)).sum(axis=1)
        show(f"{name} {where} pit_le (bounds {bound.min():.2e} .. {bound.max():.2e})", le, want_le)
        assert np.all(np.abs(le - want_le) <= bound), (np.abs(le - want_le), bound)
        assert np.all(np.abs(lt - want_lt) <= bound), (np.abs(lt - want_lt), bound)
        np.testing.assert_allclose(k, c["k"], rtol=1e-9)  # (the kernels widen f32 on load: the k of the upcast data)


# ------------------------------------------------------------------------------------------ 2. shapes at the kernels' edges
@pytest.fixture(scope="module")
def shape_refs():
    return {}


def shape_case(cache, s, dtype):
    key = (s, np.dtype(dtype).name)
    if key not in cache:
        ll, yh, y = make(np.random.default_rng(1000 + s), 300, s, dtype)
        cache[key] = (ll, yh, y, pit_ref.loo_pit(ll.astype(np.float64), yh, y, 1.0))
    return cache[key]


@pytest.mark.parametrize("s,dtype", [(s, np.float64) for s in (5, 64, 100, 257, 4095, 4096, 4097, 5000)] + [(257, np.float32), (4097, np.float32)])
def test_shapes_at_the_kernel_edges(eng, shape_refs, s, dtype):
    """Wave remainder (5, 100, 257), whole waves (64), the register-row limit (4095, 4096 | 4097), the split weights route (4097,
    5000), odd S in f32 (rows not 16-byte aligned: element loads), N = 1, 3, 65, 300 (not multiples of the waves per workgroup)."""
    ll, yh, y, ref = shape_case(shape_refs, s, dtype)
    M = orc.tail_count(s, 1.0)
    for n in (1, 3, 65, 300):
        res = eng.loo_pit(cuda(ll[:n]), cuda(yh[:n]), cuda(y[:n]), M, "psis")
        le, lt = host(res["pit_le"]), host(res["pit_lt"])
        text = eng.last_kernels()
        assert ("registers" if s <= 4096 else "streamed") in text, text
        if dtype == np.float32:
            assert "element loads" in text, text
            lw32 = ref["lw"][:n].astype(np.float32).astype(np.float64)
            want_le, want_lt = pit_ref.pit_from_log_weights(lw32, yh[:n], y[:n])
            w = np.exp(lw32 - np.max(lw32, axis=1, keepdims=True))
            w /= w.sum(axis=1, keepdims=True)
            bound = (w * (2e-7 * np.abs(lw32) + 1e-7)).sum(axis=1)
            assert np.all(np.abs(le - want_le) <= bound) and np.all(np.abs(lt - want_lt) <= bound), (s, n)
        else:
            assert ("16-byte loads" if s % 2 == 0 else "element loads") in text, text
            show(f"S={s} N={n}", le, ref["pit_le"][:n])
            np.testing.assert_allclose(le, ref["pit_le"][:n], rtol=0, atol=ATOL, err_msg=f"S={s} N={n}")
            np.testing.assert_allclose(lt, ref["pit_lt"][:n], rtol=0, atol=ATOL, err_msg=f"S={s} N={n}")
            np.testing.assert_allclose(host(res["diag"]), ref["diag"][:n], rtol=1e-8, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------- 3. layouts
def device_layouts(a):
    import torch

    wide = torch.zeros((a.shape[0], 2 * a.shape[1]), dtype=torch.as_tensor(a).dtype, device="cuda")
    wide[:, ::2] = cuda(a)
    return {"draws": cuda(a), "obs": cuda(a.T).T, "strided": wide[:, ::2]}


def test_device_layouts(eng):
    ll, yh, y = make(np.random.default_rng(7), 65, 257)
    ref = pit_ref.loo_pit(ll, yh, y, 1.0)
    M = orc.tail_count(257, 1.0)
    lls, yhs = device_layouts(ll), device_layouts(yh)
    lws = device_layouts(ref["lw"])
    outs = {}
    for a, tl in lls.items():
        for b, ty in yhs.items():
            assert tl.stride() != ty.stride() or a == b
            res = eng.loo_pit(tl, ty, cuda(y), M, "psis")
            outs[a, b] = (host(res["pit_le"]), host(res["pit_lt"]))
            text = eng.last_kernels()
            assert ("pit_prepare_tile_kernel" if a == "obs" else "pit_prepare_row_kernel") in text, text
            assert ("transpose_rows_kernel (y_hat)" in text) == (b == "obs"), text
            assert ("strided" in text.split("->")[-1]) == (b == "strided"), text
            np.testing.assert_allclose(outs[a, b][0], ref["pit_le"], rtol=0, atol=ATOL, err_msg=f"{a}/{b}")
            np.testing.assert_allclose(outs[a, b][1], ref["pit_lt"], rtol=0, atol=ATOL, err_msg=f"{a}/{b}")
            # the log-weights input reads both in place: wave kernel, lane kernel or the strided wave kernel
            r2 = eng.loo_pit(lws[a], ty, cuda(y), 0, "psis", kind="log_weights")
            text = eng.last_kernels()
            want = "pit_lane_kernel" if (a, b) == ("obs", "obs") else "pit_wave_kernel"
            assert want in text and (("strided" in text) == (a != b or a == "strided")), (a, b, text)
            np.testing.assert_allclose(host(r2["pit_le"]), ref["pit_le"], rtol=0, atol=ATOL, err_msg=f"lw {a}/{b}")
            np.testing.assert_allclose(host(r2["pit_lt"]), ref["pit_lt"], rtol=0, atol=ATOL, err_msg=f"lw {a}/{b}")
    # the layout of the log-likelihood does not reach the bits: the prepare kernels write the same block
    for a in lls:
        for b in yhs:
            assert np.array_equal(outs[a, b][0], outs["draws", b][0]) and np.array_equal(outs[a, b][1], outs["draws", b][1])
    assert np.array_equal(outs["draws", "obs"][0], outs["draws", "draws"][0])  # (transposed into the draws-fastest route)
    assert np.array_equal(outs["draws", "strided"][0], outs["draws", "draws"][0])  # (the strided loads: the same summation order)


def test_host_layouts(eng):
    from pyloo_amd import _capi
    from pyloo_amd._capi import EngineError

    ll, yh, y = make(np.random.default_rng(8), 65, 257)
    ref = pit_ref.loo_pit(ll, yh, y, 1.0)
    M = orc.tail_count(257, 1.0)
    flip = lambda a: np.ascontiguousarray(a.T).T  # noqa: E731
    base = eng.loo_pit(ll, yh, y, M, "psis")
    for a in (ll, flip(ll)):
        for b in (yh, flip(yh)):
            res = eng.loo_pit(a, b, y, M, "psis")
            assert "staged in blocks" in eng.last_kernels()
            np.testing.assert_allclose(res["pit_le"], ref["pit_le"], rtol=0, atol=ATOL)
            assert np.array_equal(res["pit_le"], base["pit_le"]) and np.array_equal(res["pit_lt"], base["pit_lt"])
            assert np.array_equal(res["diag"], base["diag"])
            r2 = eng.loo_pit(flip(ref["lw"]) if a is not ll else ref["lw"], b, y, 0, "psis", kind="log_weights")
            np.testing.assert_allclose(r2["pit_le"], ref["pit_le"], rtol=0, atol=ATOL)
    # any other strides: PLA_ERR_UNSUPPORTED through the C ABI (the Python handle would copy such a view first)
    import ctypes as C

    wide = np.zeros((65, 514))
    wide[:, ::2] = ll
    out = np.empty(65)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = eng._lib.pla_loo_pit(eng._h, p(wide), p(yh), p(y), _capi.PLA_F64, 65, 257, 514, 2, 257, 1, 0, 0, M, _capi.PLA_HOST, None, p(out),
                              None, None, None)
    assert rc == -4
    rc = eng._lib.pla_loo_pit(eng._h, p(ll), p(wide), p(y), _capi.PLA_F64, 65, 257, 257, 1, 514, 2, 0, 0, M, _capi.PLA_HOST, None, p(out),
                              None, None, None)
    assert rc == -4
    # argument errors
    for args in ((None, p(yh), p(y), p(out)), (p(ll), None, p(y), p(out)), (p(ll), p(yh), None, p(out)), (p(ll), p(yh), p(y), None)):
        rc = eng._lib.pla_loo_pit(eng._h, args[0], args[1], args[2], _capi.PLA_F64, 65, 257, 257, 1, 257, 1, 0, 0, M, _capi.PLA_HOST, None,
                                  args[3], None, None, None)
        assert rc == -1
    bad = dict(n_draws=1, kind=2, method=3, so=0, ysd=-1)
    for key in bad:
        s = 1 if key == "n_draws" else 257
        rc = eng._lib.pla_loo_pit(eng._h, p(ll), p(yh), p(y), _capi.PLA_F64, 65, s, 0 if key == "so" else 257, 1, 257,
                                  -1 if key == "ysd" else 1, 2 if key == "kind" else 0, 3 if key == "method" else 0, M, _capi.PLA_HOST,
                                  None, p(out), None, None, None)
        assert rc == -1, key
    with pytest.raises(EngineError):
        eng.loo_pit(ll, yh, y, 300, "psis")  # tail count beyond the row


# ------------------------------------------------------------------------------------------------ 4. exactness and determinism
def test_exactness_and_determinism(eng, gold):
    e = gold["edges_s500_r1"]
    M = orc.tail_count(500, 1.0)
    for src in ((e["ll"], e["yh"], e["y"]), (cuda(e["ll"]), cuda(e["yh"]), cuda(e["y"]))):
        res = eng.loo_pit(*src, M, "psis")
        le, lt = host(res["pit_le"]), host(res["pit_lt"])
        assert le[0] == 0.0 and lt[0] == 0.0 and le[1] == 1.0 and lt[1] == 1.0  # y beyond every draw: exactly
        assert le[6] == 0.0 and lt[6] == 0.0  # a NaN observation is never counted
        assert np.array_equal(le, lt)  # no draw equals its observation here: the same bits
        count = float((e["yh"][2] <= e["y"][2]).sum()) / 500.0
        assert abs(le[2] - count) <= 1e-12 and np.isinf(host(res["diag"])[2])  # constant log-likelihood: uniform weights
        again = eng.loo_pit(*src, M, "psis")
        for key in ("pit_le", "pit_lt", "diag"):
            assert np.array_equal(host(res[key]), host(again[key]), equal_nan=True), key
    p = gold["poisson_s500_r1"]
    res = eng.loo_pit(cuda(p["ll"]), cuda(p["yh"]), cuda(p["y"]), M, "psis")
    le, lt = host(res["pit_le"]), host(res["pit_lt"])
    want_le, want_lt = pit_ref.golden_expected(p)
    assert np.all(lt < le)
    np.testing.assert_allclose(le, want_le, rtol=0, atol=ATOL)
    np.testing.assert_allclose(lt, want_lt, rtol=0, atol=ATOL)
    # a larger tie-free matrix on every route of the weights input: the same bits in both outputs
    ll, yh, y = make(np.random.default_rng(9), 130, 1000)
    for t in (cuda(yh), cuda(yh.T).T):
        res = eng.loo_pit(cuda(ll), t, cuda(y), orc.tail_count(1000, 1.0), "psis")
        assert np.array_equal(host(res["pit_le"]), host(res["pit_lt"]))
    # 16-byte loads and element loads (a base that is not 16-byte aligned) sum in the same order: the same bits
    import torch

    lw, _ = eng.importance_weights(-cuda(ll), orc.tail_count(1000, 1.0), "psis")
    flat = torch.empty(130 * 1000 + 1, dtype=torch.float64, device="cuda")
    off = flat[1:].view(130, 1000)
    off.copy_(cuda(yh))
    assert off.data_ptr() % 16 == 8
    r16 = eng.loo_pit(lw, cuda(yh), cuda(y), 0, "psis", kind="log_weights")
    assert "16-byte loads" in eng.last_kernels()
    r8 = eng.loo_pit(lw, off, cuda(y), 0, "psis", kind="log_weights")
    assert "element loads" in eng.last_kernels()
    assert np.array_equal(host(r16["pit_le"]), host(r8["pit_le"])) and np.array_equal(host(r16["pit_lt"]), host(r8["pit_lt"]))
    # weights of -inf carry nothing; a row of them, or of NaN, gives NaN
    lw = np.log(np.full((3, 100), 0.01))
    lw[0, ::2] = -np.inf
    lw[1] = -np.inf
    lw[2] = np.nan
    yh3 = np.tile(np.arange(100.0), (3, 1))
    for kind in ("draws", "obs"):
        a, b = (cuda(lw), cuda(yh3)) if kind == "draws" else (cuda(lw.T).T, cuda(yh3.T).T)
        r = eng.loo_pit(a, b, cuda(np.full(3, 49.5)), 0, "psis", kind="log_weights")
        le = host(r["pit_le"])
        assert le[0] == 0.5 and np.isnan(le[1]) and np.isnan(le[2]), (kind, le)


# -------------------------------------------------------------------------------------------------- 5. block-size independence
CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from pyloo_amd.engine import get_engine
eng = get_engine(0)
rng = np.random.default_rng(5)
n, s = 700, 1000
ll = (-rng.uniform(0.05, 0.9, size=(n, 1)) * rng.exponential(size=(n, s)) - 1.0).astype(np.float64)
ll[13, 7] = np.nan
ll[650, 999] = np.nan
yh = rng.normal(size=(n, s))
y = rng.normal(size=n)
out = []
for t in (torch.as_tensor(yh).cuda(), torch.as_tensor(np.ascontiguousarray(yh.T)).cuda().T):
    r = eng.loo_pit(torch.as_tensor(ll).cuda(), t, torch.as_tensor(y).cuda(), 95, "psis")
    out += [r[k].cpu().numpy() for k in ("pit_le", "pit_lt", "diag", "n_replaced")]
np.savez(sys.argv[2], *out)
"""


def test_block_size_independence(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 cuts the 700 x 1000 f64 device matrix into six blocks of 131 observations, the last one ragged (45);
    every output and the NaN count are the default's (one block), bit for bit, for both layouts of the predictive draws."""
    outs = []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        env.update(env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            outs.append([z[k] for k in sorted(z.files, key=lambda s: int(s.split("_")[1]))])
    assert len(outs[0]) == 8
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert int(outs[0][3][0]) == 2 and int(outs[1][7][0]) == 2
    for j in range(4):  # the two layouts of y_hat among each other
        assert np.array_equal(outs[0][j], outs[0][4 + j])


# --------------------------------------------------------------------------------------------------------- 6. the log-weights input
def test_log_weights_input(eng):
    ll, yh, y = make(np.random.default_rng(10), 70, 1000)
    M = orc.tail_count(1000, 1.0)
    tll, tyh, ty = cuda(ll), cuda(yh), cuda(y)
    full = eng.loo_pit(tll, tyh, ty, M, "psis")
    lw, k = eng.importance_weights(-tll, M, "psis")
    res = eng.loo_pit(lw, tyh, ty, 0, "psis", kind="log_weights")
    assert res["diag"] is None and int(host(res["n_replaced"])[0]) == 0
    assert "read in place" in eng.last_kernels() and "prepare" not in eng.last_kernels()
    assert np.array_equal(host(res["pit_le"]), host(full["pit_le"])) and np.array_equal(host(res["pit_lt"]), host(full["pit_lt"]))
    assert np.array_equal(host(k), host(full["diag"]))
    shifted = eng.loo_pit(lw + 37.5, tyh, ty, 0, "psis", kind="log_weights")
    np.testing.assert_allclose(host(shifted["pit_le"]), host(full["pit_le"]), rtol=0, atol=ATOL)
    np.testing.assert_allclose(host(shifted["pit_lt"]), host(full["pit_lt"]), rtol=0, atol=ATOL)
    # an observations-fastest pair, read in place by the lane kernel
    pair = eng.loo_pit(cuda(host(lw).T).T, cuda(yh.T).T, ty, 0, "psis", kind="log_weights")
    assert "pit_lane_kernel" in eng.last_kernels()
    np.testing.assert_allclose(host(pair["pit_le"]), host(full["pit_le"]), rtol=0, atol=ATOL)
    np.testing.assert_allclose(host(pair["pit_lt"]), host(full["pit_lt"]), rtol=0, atol=ATOL)
    # host arrays
    hres = eng.loo_pit(host(lw), yh, y, 0, "psis", kind="log_weights")
    assert np.array_equal(hres["pit_le"], host(full["pit_le"])) and hres["n_replaced"] == 0


# -------------------------------------------------------------------------------------------------------------------- 7. methods
@pytest.mark.parametrize("method", ["sis", "tis"])
def test_sis_and_tis(eng, method):
    ll, yh, y = make(np.random.default_rng(11), 40, 1000)
    ref = pit_ref.loo_pit(ll, yh, y, 1.0, method)
    for src in ((ll, yh, y), (cuda(ll), cuda(yh), cuda(y))):
        res = eng.loo_pit(*src, 0, method)
        np.testing.assert_allclose(host(res["pit_le"]), ref["pit_le"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(host(res["pit_lt"]), ref["pit_lt"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(host(res["diag"]), ref["diag"], rtol=1e-9)  # (the effective sample size)


# -------------------------------------------------------------------------------------------------------------- 8. frozen engine
def test_frozen_engine():
    import torch

    from pyloo_amd._capi import EngineError
    from pyloo_amd.engine import Engine

    own = Engine(0)
    try:
        ll, yh, y = make(np.random.default_rng(12), 200, 1000)
        M = orc.tail_count(1000, 1.0)
        warm = own.loo_pit(cuda(ll), cuda(yh.T).T, cuda(y), M, "psis")
        torch.cuda.synchronize()
        own.set_frozen(True)
        again = own.loo_pit(cuda(ll), cuda(yh.T).T, cuda(y), M, "psis")
        assert torch.equal(again["pit_le"], warm["pit_le"]) and torch.equal(again["diag"], warm["diag"])
        ll2, yh2, y2 = make(np.random.default_rng(13), 500, 1000)
        with pytest.raises(EngineError) as err:
            own.loo_pit(cuda(ll2), cuda(yh2.T).T, cuda(y2), M, "psis")
        assert err.value.code == -6
        torch.cuda.synchronize()
    finally:
        own.set_frozen(False)
        own.close()


# ---------------------------------------------------------------------------------------------------------------------- 9. front
def test_front(eng):
    import pyloo_amd as pl

    rng = np.random.default_rng(14)
    chains, draws, obs = 2, 250, (5, 4)
    ll = -0.3 * rng.exponential(size=(chains, draws) + obs) - 1.0
    yh = rng.poisson(4.0, size=(chains, draws) + obs).astype(np.float64)
    y = rng.poisson(4.0, size=obs).astype(np.float64)
    data = {"log_likelihood": {"obs": ll}, "posterior_predictive": {"obs": yh}, "observed_data": {"obs": y},
            "posterior": {"mu": rng.normal(size=(1, chains * draws))}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = pl.loo_pit(data, seed=3)  # one chain in the posterior group: reff = 1
        stack = lambda a: np.moveaxis(a.reshape((chains * draws,) + obs), 0, -1).reshape(-1, chains * draws)  # noqa: E731
        mat = pl.loo_pit_from_matrix(stack(ll), stack(yh), y.reshape(-1), reff=1.0, seed=3)
        dev = pl.loo_pit_from_matrix(cuda(stack(ll)), cuda(stack(yh)), cuda(y.reshape(-1)), reff=1.0, seed=3)
    for v in (res.pit, res.pit_le, res.pit_lt, res.pareto_k):
        assert np.asarray(v).shape == obs
    for a, b in ((res.pit, mat.pit), (res.pit_le, mat.pit_le), (res.pit_lt, mat.pit_lt), (res.pareto_k, mat.pareto_k)):
        assert np.array_equal(np.asarray(a).reshape(-1), b)
    assert np.array_equal(dev.pit_le, mat.pit_le) and np.array_equal(dev.pit, mat.pit)
    ref = pit_ref.loo_pit(stack(ll), stack(yh), y.reshape(-1), 1.0)
    np.testing.assert_allclose(mat.pit_le, ref["pit_le"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(mat.pit_lt, ref["pit_lt"], rtol=0, atol=ATOL)
    assert np.all(mat.pit_lt <= mat.pit_le) and np.sum(mat.pit_lt < mat.pit_le) >= 10  # count data: ties
    assert np.all(mat.pit >= mat.pit_lt) and np.all(mat.pit <= mat.pit_le)
