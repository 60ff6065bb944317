"""LOO diagnostics on the GPU (``pla_loo_diag``, ``pla_loo_diag_weights``, ``Engine.loo_diag``, ``pl.loo_diagnostics``) and the
per-observation ``reff`` of ``pl.loo_from_matrix`` through the C ABI: the reference's weights (tests/golden/loo_pit.npz) through
the NumPy restatement (tests/diag_ref.py), the kernel's shape edges, load modes and layouts, the fused route against the kernel
alone bit for bit, row selection, block-size independence, the in-band values, frozen engines and the vector ``reff`` end to end.

Bounds.  k: rtol 1e-9 and elpd_i: atol 1e-9, the bounds of tests/test_gpu_loo_pit.py.  ess_w and var_log: rtol 1e-8 -- on the CPU
oracle a perturbation of 1e-10 of lw moves both by 1.0 - 1.25e-10 relative (S = 500 and 4000, k from 0 to 1.5) and the project
holds lw to 1e-10: two decades of margin.  A var_log at or below 1e-24 is the rounding noise of a constant row (the bound
tests/test_loo_diagnostics_host.py holds the restatement's constant rows to) and is held to that bound on both sides, not to a
ratio of two roundings."""

import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import diag_ref
import pit_ref
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("elpd_i", "ess_w", "var_log")
F64_CASES = ["edges_s500_r1", "poisson_s500_r1", "s1000_r0p7", "s100_r1", "s4000_r1"]


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


def show(what, got, want, relative=False):
    with np.errstate(all="ignore"):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        d = np.abs(got - want) / (np.abs(want) if relative else 1.0)
    d = d[np.isfinite(d)]
    print(f"{what}: max {'rel' if relative else 'abs'} dev = {d.max() if d.size else 0.0:.3e}")


def check(what, got, want):
    """The three values against the restatement at the bounds of the module docstring; NaN on both sides or on neither."""
    got = {k: host(got[k]) for k in KEYS}
    for k in KEYS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (what, k, got[k], want[k])
    ok = ~np.isnan(want["elpd_i"])
    show(f"{what} elpd_i", got["elpd_i"][ok], want["elpd_i"][ok])
    show(f"{what} ess_w", got["ess_w"][ok], want["ess_w"][ok], relative=True)
    np.testing.assert_allclose(got["elpd_i"][ok], want["elpd_i"][ok], rtol=0, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(got["ess_w"][ok], want["ess_w"][ok], rtol=1e-8, atol=0, err_msg=what)
    big = ok & (want["var_log"] > 1e-24)
    show(f"{what} var_log", got["var_log"][big], want["var_log"][big], relative=True)
    np.testing.assert_allclose(got["var_log"][big], want["var_log"][big], rtol=1e-8, atol=0, err_msg=what)
    assert np.all(got["var_log"][ok & ~big] <= 1e-24), (what, got["var_log"][ok & ~big])


def same_bits(a, b, keys=KEYS):
    return all(np.array_equal(host(a[k]), host(b[k]), equal_nan=True) for k in keys)


def make_ll(rng, n, s, dtype=np.float64):
    """Continuous log-likelihood rows with Pareto k between 0.05 and 0.9 (no ties in the tail)."""
    k = rng.uniform(0.05, 0.9, size=(n, 1))
    return (-k * rng.exponential(size=(n, s)) - 1.0 - rng.uniform(size=(n, 1))).astype(dtype)


# ------------------------------------------------------------------------------------------------------------- 1. golden parity
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", F64_CASES)
def test_golden_parity(eng, gold, name, where):
    c = gold[name]
    ll = c["ll"]
    assert ll.dtype == np.float64
    M = orc.tail_count(ll.shape[1], c["reff"])
    res = eng.loo_diag(cuda(ll) if where == "device" else ll, M, "psis")
    text = eng.last_kernels()
    assert "diag_wave_kernel" in text and "diag_prepare_row_kernel" in text, text
    assert int(host(res["n_replaced"]).reshape(-1)[0]) == int(np.isnan(ll).sum())
    want = diag_ref.from_log_weights(c["lw"], np.where(np.isnan(ll), -1e10, ll))
    check(f"{name} {where}", res, want)
    show(f"{name} {where} k", host(res["diag"]), c["k"], relative=True)
    np.testing.assert_allclose(host(res["diag"]), c["k"], rtol=1e-9)


# ------------------------------------------------------------------------------------------ 2. the kernel at its shape edges
EDGE_DRAWS = (5, 63, 64, 65, 127, 129, 255, 4095, 4096, 4097, 4100)


@pytest.fixture(scope="module")
def edge_refs():
    return {}


def edge_case(cache, s, dtype):
    """(lw, ll, restatement) of 300 rows: log weights of any normalisation, here -ll plus noise plus a row offset."""
    key = (s, np.dtype(dtype).name)
    if key not in cache:
        rng = np.random.default_rng(2000 + s)
        ll = make_ll(rng, 300, s, dtype)
        lw = (-ll.astype(np.float64) + 0.3 * rng.normal(size=(300, s)) + rng.normal(size=(300, 1)) * 20.0).astype(dtype)
        cache[key] = (lw, ll, diag_ref.from_log_weights(lw, ll))
    return cache[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("s", EDGE_DRAWS)
def test_kernel_edges(eng, edge_refs, s, dtype):
    """Wave remainders (5, 63, 65, 127, 129, 255), whole waves (64), the last register row (4095, 4096) and the first streamed
    ones (4097, 4100); 1, 5 and 300 rows (5: more than one workgroup's four waves, ragged).  The arithmetic is f64 on the values
    given, so the f64 bound holds for both dtypes.  An unaligned base and a padded pitch take element loads, .T views the strided
    mode: the same bits as the aligned call on the same values."""
    import torch

    lw, ll, ref = edge_case(edge_refs, s, dtype)
    vec = 16 // np.dtype(dtype).itemsize
    for n in (1, 5, 300):
        tl, tx = cuda(lw[:n]), cuda(ll[:n])
        base = eng.loo_diag_weights(tl, tx)
        text = eng.last_kernels()
        assert "diag_wave_kernel" in text and "read in place" in text and ("registers" if s <= 4096 else "streamed") in text, text
        assert ("16-byte loads" if s % vec == 0 else "element loads") in text, text
        check(f"S={s} N={n} {np.dtype(dtype).name}", base, {k: ref[k][:n] for k in KEYS})
        # an unaligned base: the views [:, 1:] of buffers one column wider
        wide = [torch.zeros((n, s + 1), dtype=tl.dtype, device="cuda") for _ in range(2)]
        wide[0][:, 1:] = tl
        wide[1][:, 1:] = tx
        off = eng.loo_diag_weights(wide[0][:, 1:], wide[1][:, 1:])
        assert "element loads" in eng.last_kernels(), eng.last_kernels()
        assert same_bits(off, base), (s, n, "unaligned base")
        # a padded pitch that is no multiple of the vector
        pad = [torch.zeros((n, s + vec + 1), dtype=tl.dtype, device="cuda") for _ in range(2)]
        pad[0][:, :s] = tl
        pad[1][:, :s] = tx
        pitched = eng.loo_diag_weights(pad[0][:, :s], pad[1][:, :s])
        assert "element loads" in eng.last_kernels(), eng.last_kernels()
        assert same_bits(pitched, base), (s, n, "padded pitch")
        # both matrices observations-fastest
        if n > 1:
            turned = eng.loo_diag_weights(cuda(lw[:n].T).T, cuda(ll[:n].T).T)
            assert "strided" in eng.last_kernels(), eng.last_kernels()
            assert same_bits(turned, base), (s, n, "strided")


def test_weights_entry_from_the_host_and_its_argument_errors(eng, edge_refs):
    from pyloo_amd import _capi

    lw, ll, ref = edge_case(edge_refs, 129, np.float64)
    dev = eng.loo_diag_weights(cuda(lw), cuda(ll))
    res = eng.loo_diag_weights(lw, ll)
    assert "staged in blocks" in eng.last_kernels()
    assert same_bits(res, dev)
    mixed = eng.loo_diag_weights(lw.astype(np.float32), ll)  # (promoted to one dtype)
    check("f32 weights, f64 ll", mixed, diag_ref.from_log_weights(lw.astype(np.float32), ll))
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.empty(300)
    wide = np.zeros((300, 258))
    call = lambda a, b, so, sd, s=129: eng._lib.pla_loo_diag_weights(eng._h, a, b, _capi.PLA_F64, 300, s, so, sd, 129, 1, _capi.PLA_HOST,  # noqa: E731
                                                                       None, p(out), None, None)
    assert call(p(wide), p(ll), 258, 2) == -4  # a draw stride on the host
    assert call(None, p(ll), 129, 1) == -1 and call(p(lw), None, 129, 1) == -1
    assert call(p(lw), p(ll), 0, 1) == -1 and call(p(lw), p(ll), 129, -1) == -1 and call(p(lw), p(ll), 129, 1, s=1) == -1
    assert call(p(lw), p(ll), 129, 1) == 0 and np.array_equal(out, res["elpd_i"])  # (the other outputs may be NULL)


# ------------------------------------------------------------------------------------------------------------- 3. the fused route
def fused_layouts(ll):
    return {"device draws": cuda(ll), "device obs": cuda(ll.T).T, "host draws": ll, "host obs": np.ascontiguousarray(ll.T).T}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,s,method", [(70, 1000, "psis"), (40, 4100, "psis"), (9, 8, "psis"), (70, 1000, "sis"), (70, 1000, "tis")])
def test_fused_route_is_the_kernel_on_the_weights_pass(eng, n, s, method, dtype):
    """``pla_loo_diag`` on ll is bit for bit ``pla_loo_diag_weights`` on (``importance_weights(-ll)``, ll), in every layout and
    memory space: S = 4100 takes the split weights route (tail count 193 <= 448), S = 8 has k = inf (a tail of 2 draws)."""
    ll = make_ll(np.random.default_rng(300 + s), n, s, dtype)
    M = orc.tail_count(s, 1.0) if method == "psis" else 0
    assert s != 4100 or M <= 448
    tll = cuda(ll)
    lw, k = eng.importance_weights(-tll, M, method)
    want = eng.loo_diag_weights(lw, tll)
    for name, mat in fused_layouts(ll).items():
        res = eng.loo_diag(mat, M, method)
        text = eng.last_kernels()
        assert "diag_wave_kernel" in text and ("diag_prepare_tile_kernel" if name.endswith("obs") else "diag_prepare_row_kernel") in text, text
        assert ("staged in blocks" in text) == name.startswith("host"), text
        assert same_bits(res, want), (name, method)
        assert np.array_equal(host(res["diag"]), host(k), equal_nan=True), name
        assert int(host(res["n_replaced"]).reshape(-1)[0]) == 0
    if s == 8:
        assert np.all(np.isinf(host(k)))
    if dtype == np.float64 and method == "psis":
        check(f"fused S={s}", want, diag_ref.loo_diag(ll, 1.0))
    if method != "psis":
        ref = diag_ref.loo_diag(ll.astype(np.float64), method=method)
        np.testing.assert_allclose(host(k), ref["diag"], rtol=1e-9 if dtype == np.float64 else 1e-4)
        if dtype == np.float64:
            check(f"fused {method}", want, ref)


# ------------------------------------------------------------------------------------------------------------------- 4. row_index
def test_row_index_gives_the_bits_of_the_full_call(eng):
    import torch

    from pyloo_amd import _capi

    ll = make_ll(np.random.default_rng(40), 130, 1000)
    ll[7, 3] = np.nan
    ll[99, 998] = np.nan
    M = orc.tail_count(1000, 0.6)
    rows = np.array([99, 3, 7, 129, 7, 0, 64, 99, 65, 7])
    full = eng.loo_diag(cuda(ll), M, "psis")
    keys = KEYS + ("diag",)
    for name, mat, idx in (("device, device list", cuda(ll), torch.as_tensor(rows).cuda()), ("device, host list", cuda(ll), rows.tolist()),
                           ("device obs-fastest", cuda(ll.T).T, torch.as_tensor(rows).cuda()), ("host", ll, rows)):
        res = eng.loo_diag(mat, M, "psis", rows=idx)
        assert ("diag_prepare_tile_kernel" in eng.last_kernels()) == (name == "device obs-fastest"), eng.last_kernels()
        for k in keys:
            assert np.array_equal(host(res[k]), host(full[k])[rows], equal_nan=True), (name, k)
        assert int(host(res["n_replaced"]).reshape(-1)[0]) == 5  # (row 7 three times, row 99 twice)
    assert int(host(full["n_replaced"])[0]) == 2
    # a device list out of range is clamped into the matrix; a host list is refused
    res = eng.loo_diag(cuda(ll), M, "psis", rows=torch.as_tensor([-5, 500, 3]).cuda())
    for k in keys:
        assert np.array_equal(host(res[k]), host(full[k])[[0, 129, 3]], equal_nan=True), k
    for bad in ([0, 130], [-1, 2]):
        with pytest.raises(IndexError):
            eng.loo_diag(ll, M, "psis", rows=bad)
        with pytest.raises(IndexError):
            eng.loo_diag(cuda(ll), M, "psis", rows=bad)
        idx = np.asarray(bad, dtype=np.int64)
        out = np.empty(2)
        p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = eng._lib.pla_loo_diag(eng._h, p(ll), _capi.PLA_F64, 130, 1000, 1000, 1, p(idx), 2, 0, M, _capi.PLA_HOST, None, p(out), None, None,
                                   None, None)
        assert rc == -1
    # an observations-fastest host matrix takes no row list (the Python handle copies such a matrix first)
    flipped = np.ascontiguousarray(ll.T)
    idx = np.asarray([1, 2], dtype=np.int64)
    rc = eng._lib.pla_loo_diag(eng._h, p(flipped), _capi.PLA_F64, 130, 1000, 1, 130, p(idx), 2, 0, M, _capi.PLA_HOST, None, p(out), None, None,
                               None, None)
    assert rc == -4
    with pytest.raises(_capi.EngineError):
        eng.loo_diag(ll, 1000, "psis")  # tail count beyond the row


# -------------------------------------------------------------------------------------------------- 5. block-size independence
CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from pyloo_amd.engine import get_engine
eng = get_engine(0)
rng = np.random.default_rng(5)
n, s = 300, 1000
ll = (-rng.uniform(0.05, 0.9, size=(n, 1)) * rng.exponential(size=(n, s)) - 1.0).astype(np.float64)
ll[13, 7] = np.nan
ll[290, 999] = np.nan
rows = torch.as_tensor(rng.integers(0, n, size=280)).cuda()
out = []
for t in (torch.as_tensor(ll).cuda(), torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T):
    for idx in (None, rows):
        for rep in range(2):
            r = eng.loo_diag(t, 95, "psis", rows=idx)
            out += [r[k].cpu().numpy() for k in ("diag", "elpd_i", "ess_w", "var_log", "n_replaced")]
np.savez(sys.argv[2], *out)
"""


def test_block_size_independence(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 cuts the 300 x 1000 f64 device matrix into three blocks of 131 observations, the last one ragged (38),
    and the 280 selected rows likewise: every output and the NaN count are the default's (one block), bit for bit, for both
    layouts; and two calls in one process give the same bits."""
    outs = []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        env.update(env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            outs.append([z[k] for k in sorted(z.files, key=lambda s: int(s.split("_")[1]))])
    assert len(outs[0]) == 40
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)
    one = outs[0]
    assert int(one[4][0]) == 2
    for base in (0, 10, 20, 30):  # the second call of a pair
        for j in range(5):
            assert np.array_equal(one[base + j], one[base + 5 + j], equal_nan=True)
    for j in range(5):  # the two layouts among each other, full and selected
        assert np.array_equal(one[j], one[20 + j], equal_nan=True) and np.array_equal(one[10 + j], one[30 + j], equal_nan=True)


# ----------------------------------------------------------------------------------------------------------------- 6. in-band values
def test_in_band_values(eng):
    s = 500
    rng = np.random.default_rng(60)
    ll = make_ll(rng, 6, s)
    ll[0, 3] = ll[0, 250] = np.nan   # counted, taken as -1e10 (the values of such a row: the golden edge case above)
    ll[1] = -np.inf              # every ll -inf: NaN
    ll[2] = -2.5                 # a constant row: uniform weights, k = inf
    M = orc.tail_count(s, 1.0)
    ref = diag_ref.loo_diag(ll, 1.0)
    for mat in (ll, cuda(ll), cuda(ll.T).T):
        res = eng.loo_diag(mat, M, "psis")
        assert int(host(res["n_replaced"]).reshape(-1)[0]) == int(np.isnan(ll).sum()) == 2
        got = {k: host(res[k]) for k in KEYS}
        assert all(np.isnan(got[k][1]) for k in KEYS)
        assert got["ess_w"][2] == float(s) and got["var_log"][2] <= 1e-24 and abs(got["elpd_i"][2] + 2.5) <= 1e-12
        assert np.isinf(host(res["diag"])[2])
        assert all(np.isfinite(got[k][0]) for k in KEYS) and got["elpd_i"][0] < -9e9
        keep = np.array([2, 3, 4, 5])
        check("in-band", {k: got[k][keep] for k in KEYS}, {k: ref[k][keep] for k in KEYS})
        assert np.all(got["ess_w"][keep] >= 1.0) and np.all(got["ess_w"][keep] <= s)
    # the kernel alone: single -inf entries on either side, rows of -inf or NaN weights, a NaN weight, a NaN ll
    lw = 0.5 * rng.normal(size=(8, 100))
    x = make_ll(rng, 8, 100)
    lw[0, ::2] = -np.inf         # weight 0 at every other draw
    x[0, 0] = np.inf             # ... whatever the ll there (where the ratio -ll is -inf, ll is +inf)
    x[1, 5] = -np.inf            # likelihood 0 at one draw
    lw[2] = -np.inf
    lw[3] = np.nan
    lw[4, 9] = np.nan
    x[5, 9] = np.nan
    x[6] = -np.inf
    lw[7] = 3.25                 # constant weights
    ref = diag_ref.from_log_weights(lw, x)
    assert np.isnan(ref["elpd_i"]).tolist() == [False, False, True, True, True, True, True, False]
    assert ref["ess_w"][7] == 100.0 and abs(ref["ess_w"][0] - diag_ref.from_log_weights(lw[:1, 1::2], x[:1, 1::2])["ess_w"][0]) <= 1e-9
    for a, b in ((cuda(lw), cuda(x)), (lw, x), (cuda(lw.T).T, cuda(x.T).T)):
        res = eng.loo_diag_weights(a, b)
        check("in-band weights", res, ref)
        assert host(res["ess_w"])[7] == 100.0


# -------------------------------------------------------------------------------------------------------------- 7. frozen engine
def test_frozen_engine():
    import torch

    from pyloo_amd._capi import EngineError
    from pyloo_amd.engine import Engine

    own = Engine(0)
    try:
        ll = make_ll(np.random.default_rng(70), 200, 1000)
        M = orc.tail_count(1000, 1.0)
        rows = torch.arange(0, 200, 3).cuda()
        warm = own.loo_diag(cuda(ll), M, "psis")
        warm_rows = own.loo_diag(cuda(ll.T).T, M, "psis", rows=rows)
        warm_w = own.loo_diag_weights(cuda(ll), cuda(ll))
        torch.cuda.synchronize()
        own.set_frozen(True)
        again = own.loo_diag(cuda(ll), M, "psis")
        again_rows = own.loo_diag(cuda(ll.T).T, M, "psis", rows=rows)
        again_w = own.loo_diag_weights(cuda(ll), cuda(ll))
        assert same_bits(again, warm, KEYS + ("diag",)) and same_bits(again_rows, warm_rows, KEYS + ("diag",)) and same_bits(again_w, warm_w)
        big = make_ll(np.random.default_rng(71), 500, 1000)
        with pytest.raises(EngineError) as err:
            own.loo_diag(cuda(big), M, "psis")
        assert err.value.code == -6
        torch.cuda.synchronize()
    finally:
        own.set_frozen(False)
        own.close()


# ------------------------------------------------------------------------------------------------ 8. a reff per observation
@pytest.fixture(scope="module")
def vector_case():
    """200 rows, S = 1000, four relative efficiencies and one observation with its own (a bucket of one row); the oracle's rows
    with each row's own tail count, once for the tests below."""
    rng = np.random.default_rng(80)
    ll = make_ll(rng, 200, 1000)
    r = rng.choice([0.25, 0.5, 0.8, 1.0], size=200)
    r[137] = 0.37
    ref = diag_ref.loo_diag(ll, r)
    loo_i = np.array([orc.lse(ref["lw"][i] + ll[i]) for i in range(200)])
    lppd_i = np.array([orc.lse(row, b_inv=1000) for row in ll])
    return ll, r, ref, loo_i, lppd_i


@pytest.mark.parametrize("where", ["host", "device", "device obs-fastest, host reff"])
def test_vector_reff_end_to_end(eng, vector_case, where):
    import pyloo_amd as pl

    ll, r, ref, loo_i, lppd_i = vector_case
    assert sorted(set(ref["M"].tolist())) == sorted({orc.tail_count(1000, v) for v in (0.25, 0.37, 0.5, 0.8, 1.0)})
    mat, rv = {"host": (ll, r), "device": (cuda(ll), cuda(r)), "device obs-fastest, host reff": (cuda(ll.T).T, r)}[where]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = pl.loo_from_matrix(mat, reff=rv, pointwise=True)
        d = pl.loo_diagnostics_from_matrix(mat, reff=rv)
    got_i, got_k = host(res["loo_i"]), host(res["pareto_k"])
    show(f"{where} loo_i", got_i, loo_i)
    np.testing.assert_allclose(got_i, loo_i, rtol=1e-9, atol=1e-10)   # the bounds of tests/test_gpu_parity.py
    np.testing.assert_allclose(got_k, ref["diag"], rtol=1e-9, atol=1e-10)
    agg = orc.loo_aggregate(loo_i, lppd_i, ref["diag"], 1000)
    np.testing.assert_allclose(res["elpd_loo"], agg["elpd_loo"], rtol=1e-9)
    np.testing.assert_allclose(res["se"], agg["se"], rtol=1e-8)
    np.testing.assert_allclose(res["p_loo"], agg["p_loo"], rtol=1e-8, atol=1e-6)
    assert res["n_data_points"] == 200 and res["n_samples"] == 1000
    # the diagnostics with every row's own tail
    want = diag_ref.front_values(ref, r)
    check(f"vector reff {where}", {"elpd_i": d.elpd_i, "ess_w": d.n_eff / r, "var_log": d.mcse_elpd_i ** 2 * r}, ref)
    np.testing.assert_allclose(d.n_eff, want["n_eff"], rtol=1e-8)
    np.testing.assert_allclose(d.mcse_elpd_i, want["mcse_elpd_i"], rtol=1e-8)
    np.testing.assert_allclose(d.mcse_elpd_loo, want["mcse_elpd_loo"], rtol=1e-8)
    np.testing.assert_allclose(d.pareto_k, ref["diag"], rtol=1e-9, atol=1e-10)
    assert np.array_equal(d.r_eff, r) and d.n_replaced == 0
    t = pl.pareto_k_table(d)
    assert int(t["Count"].sum()) == 200 and t["Min. n_eff"].iloc[0] == d.n_eff[d.pareto_k <= d.good_k].min()


def test_an_all_equal_vector_gives_the_bits_of_the_float(eng, vector_case):
    import pyloo_amd as pl

    ll = vector_case[0]
    for mat, rv in ((cuda(ll), cuda(np.full(200, 0.8))), (ll, np.full(200, 0.8)), (cuda(ll.T).T, np.full(200, 0.8))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vec = pl.loo_from_matrix(mat, reff=rv, pointwise=True)
            flt = pl.loo_from_matrix(mat, reff=0.8, pointwise=True)
            dv = pl.loo_diagnostics_from_matrix(mat, reff=rv)
            df = pl.loo_diagnostics_from_matrix(mat, reff=0.8)
        assert list(vec.index) == list(flt.index)
        for key in ("elpd_loo", "se", "p_loo", "p_loo_se", "looic", "looic_se"):
            assert vec[key] == flt[key], key
        assert np.array_equal(host(vec["loo_i"]), host(flt["loo_i"])) and np.array_equal(host(vec["pareto_k"]), host(flt["pareto_k"]))
        for key in ("pareto_k", "n_eff", "mcse_elpd_i", "elpd_i", "r_eff"):
            assert np.array_equal(getattr(dv, key), getattr(df, key)), key
        assert dv.mcse_elpd_loo == df.mcse_elpd_loo


def test_reff_none_runs_relative_eff_on_the_same_matrix(eng):
    import pyloo_amd as pl

    import torch

    t = torch.empty((120, 1000), dtype=torch.float64, device="cuda")
    eng.fill_synthetic_chains(t, seed=9, chains=4, rho=0.7)
    r = pl.relative_eff_from_matrix(t, n_chains=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        auto = pl.loo_diagnostics_from_matrix(t, reff=None, n_chains=4)
        given = pl.loo_diagnostics_from_matrix(t, reff=r)
    assert np.array_equal(auto.r_eff, host(r)) and np.array_equal(auto.n_eff, given.n_eff) and auto.mcse_elpd_loo == given.mcse_elpd_loo
    assert len(np.unique(auto.r_eff)) > 10 and np.all(auto.n_eff > 0) and np.all(auto.n_eff <= 1000)
    ref = diag_ref.loo_diag(host(t), host(r))
    check("reff=None", {"elpd_i": auto.elpd_i, "ess_w": auto.n_eff / auto.r_eff, "var_log": auto.mcse_elpd_i ** 2 * auto.r_eff}, ref)
