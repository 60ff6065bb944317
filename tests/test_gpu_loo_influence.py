"""LOO influence on the GPU (``pla_loo_influence``, ``Engine.loo_influence``, ``pl.loo_influence_from_matrix``): the reference's
weights (tests/golden/loo_pit.npz) through the NumPy restatement (tests/influence_ref.py), the kernel's shape edges, load modes
and layouts, position independence bit for bit (rows, columns, row selection, block size), the in-band
values, and the fronts end to end with the fused route against the kernel alone.

Bounds.  shift, m2, kl: absolute 1e-8 in standardised units -- the project holds lw to 1e-10, and on the CPU restatement a
perturbation of 1e-10 of the reference's lw (cases s4000_r1, edges_s500_r1, s100_r1, the five columns of
``influence_ref.make_theta``: normal, log-normal, offset, correlated) moves the three by at most 4.1e-11
(tests/test_loo_influence_host.py prints and holds the figure): two decades of margin, the derivation of
tests/test_gpu_loo_diagnostics.py.  ess_w: rtol 1e-8 and k: rtol 1e-9, the existing bounds.  NaN sits on both sides or on
neither; no case is excluded.  Kernel and restatement are handed the same ``center`` and ``scale``."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import influence_ref
import pit_ref
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("shift", "m2", "kl", "ess_w")
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
    """The four values against the restatement at the bounds of the module docstring; NaN on both sides or on neither."""
    got = {k: host(got[k]) for k in KEYS}
    for k in KEYS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (what, k, got[k], want[k])
    ok = ~np.isnan(want["kl"])
    for k in ("shift", "m2", "kl"):
        show(f"{what} {k}", got[k][ok], want[k][ok])
    show(f"{what} ess_w", got["ess_w"][ok], want["ess_w"][ok], relative=True)
    for k in ("shift", "m2", "kl"):
        np.testing.assert_allclose(got[k][ok], want[k][ok], rtol=0, atol=1e-8, err_msg=f"{what} {k}")
    np.testing.assert_allclose(got["ess_w"][ok], want["ess_w"][ok], rtol=1e-8, atol=0, err_msg=what)


def same_bits(a, b, keys=KEYS):
    return all(np.array_equal(host(a[k]), host(b[k]), equal_nan=True) for k in keys)


def make_ll(rng, n, s, dtype=np.float64):
    """Continuous log-likelihood rows with Pareto k between 0.05 and 0.9 (no ties in the tail)."""
    k = rng.uniform(0.05, 0.9, size=(n, 1))
    return (-k * rng.exponential(size=(n, s)) - 1.0 - rng.uniform(size=(n, 1))).astype(dtype)


def make_lw(rng, n, s, dtype=np.float64):
    """Log weights of any normalisation: -ll plus noise plus a row offset."""
    return (-make_ll(rng, n, s) + 0.3 * rng.normal(size=(n, s)) + rng.normal(size=(n, 1)) * 20.0).astype(dtype)


def wide_theta(rng, s, p):
    """p columns: the five of ``make_theta`` first, standard normal ones behind them."""
    th = rng.normal(size=(s, p))
    q = min(p, 5)
    th[:, :q] = influence_ref.make_theta(rng, s, q)
    return th


def kernel(eng, lw, theta, c, sc, **kw):
    return eng.loo_influence(lw, theta, c, sc, kind="log_weights", **kw)


# ------------------------------------------------------------------------------------------------------------- 1. golden parity
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", F64_CASES)
def test_golden_parity(eng, gold, name, where):
    c = gold[name]
    ll = c["ll"]
    assert ll.dtype == np.float64
    n, s = ll.shape
    M = orc.tail_count(s, c["reff"])
    theta = influence_ref.make_theta(np.random.default_rng(100 + s), s)
    cen, sc = influence_ref.center_scale(theta)
    dev = where == "device"
    res = eng.loo_influence(cuda(ll) if dev else ll, cuda(theta) if dev else theta, cen, sc, M, "psis", "loglik")
    text = eng.last_kernels()
    assert "influence_kernel<double" in text and "influence_prepare_kernel" in text and "diag_prepare_row_kernel" in text, text
    assert ("staged in blocks" in text) == (not dev), text
    assert int(host(res["n_replaced"]).reshape(-1)[0]) == int(np.isnan(ll).sum())
    check(f"{name} {where}", res, influence_ref.from_log_weights(c["lw"], theta, cen, sc))
    show(f"{name} {where} k", host(res["diag"]), c["k"], relative=True)
    np.testing.assert_allclose(host(res["diag"]), c["k"], rtol=1e-9)


# ------------------------------------------------------------------------------------------ 2. the kernel at its shape edges
EDGE_DRAWS = (5, 63, 64, 65, 127, 255, 4095, 4096, 4097)


@pytest.fixture(scope="module")
def edge_refs():
    return {}


def edge_case(cache, s, dtype, n=300, p=5):
    """(lw, theta, center, scale, restatement) of n rows, computed once per shape."""
    key = (s, np.dtype(dtype).name, n, p)
    if key not in cache:
        rng = np.random.default_rng(3000 + 7 * s + p)
        lw = make_lw(rng, n, s, dtype)
        theta = wide_theta(rng, s, p)
        cen, sc = influence_ref.center_scale(theta)
        cache[key] = (lw, theta, cen, sc, influence_ref.from_log_weights(lw, theta, cen, sc))
    return cache[key]


def layouts_give_the_same_bits(eng, tl, theta, cen, sc, base, vec, what):
    """An unaligned base, a padded pitch and a .T view of the weights take element loads; theta as a .T view of a (P, S) array
    goes through the same prepare kernel with other strides: the aligned call's bits."""
    import torch

    n, s = tl.shape
    turned = kernel(eng, tl, cuda(theta.T).T, cen, sc)
    assert same_bits(turned, base), (what, "theta.T")
    wide = torch.zeros((n, s + 1), dtype=tl.dtype, device="cuda")
    wide[:, 1:] = tl
    off = kernel(eng, wide[:, 1:], cuda(theta), cen, sc)
    assert "element loads" in eng.last_kernels(), eng.last_kernels()
    assert same_bits(off, base), (what, "unaligned base")
    pad = torch.zeros((n, s + vec + 1), dtype=tl.dtype, device="cuda")
    pad[:, :s] = tl
    pitched = kernel(eng, pad[:, :s], cuda(theta), cen, sc)
    assert ("element loads" in eng.last_kernels()) == (n > 1 or s % vec != 0), eng.last_kernels()  # (one row has no pitch)
    assert same_bits(pitched, base), (what, "padded pitch")
    if n > 1:
        flipped = kernel(eng, cuda(host(tl).T).T, cuda(theta), cen, sc)
        assert "element loads" in eng.last_kernels(), eng.last_kernels()
        assert same_bits(flipped, base), (what, ".T weights")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("s", EDGE_DRAWS)
def test_kernel_edges_along_the_draws(eng, edge_refs, s, dtype):
    """K-chunk remainders (5, 63, 65, 127, 255, 4095, 4097) and whole chunks (64, 4096); 1, 17 and 300 rows: less than a tile, a
    ragged second tile, and more tiles than one workgroup's four wavefronts (19, the last ragged).  The arithmetic is f64 on the
    values given, so the f64 bound holds for both dtypes."""
    lw, theta, cen, sc, ref = edge_case(edge_refs, s, dtype)
    vec = 16 // np.dtype(dtype).itemsize
    for n in (1, 17, 300):
        tl = cuda(lw[:n])
        base = kernel(eng, tl, cuda(theta), cen, sc)
        text = eng.last_kernels()
        assert f"influence_kernel<{'double' if dtype == np.float64 else 'float'}" in text and "read in place" in text, text
        assert ("16-byte loads" if s % vec == 0 else "element loads") in text and "1 column tiles" in text, text
        check(f"S={s} N={n} {np.dtype(dtype).name}", base, {k: ref[k][:n] for k in KEYS})
        layouts_give_the_same_bits(eng, tl, theta, cen, sc, base, vec, (s, n))
    res = kernel(eng, lw[:17], theta, cen, sc)  # from the host
    assert "staged in blocks" in eng.last_kernels() and same_bits(res, kernel(eng, cuda(lw[:17]), cuda(theta), cen, sc))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("p", (1, 15, 16, 17, 32, 33, 64, 65, 130))
def test_kernel_edges_along_the_quantities(eng, edge_refs, p, dtype):
    """One column tile (1, 15, 16), a panel of two (17, 32: ragged and whole), the 64-quantity panel (33, 64), two such panels
    (65) and three (130), at S = 257 (a K-chunk remainder of one draw) and 37 rows."""
    lw, theta, cen, sc, ref = edge_case(edge_refs, 257, dtype, n=37, p=p)
    tl = cuda(lw)
    base = kernel(eng, tl, cuda(theta), cen, sc)
    assert f"{1 if p <= 16 else 2 if p <= 32 else 4} column tiles" in eng.last_kernels(), eng.last_kernels()
    check(f"P={p} {np.dtype(dtype).name}", base, ref)
    layouts_give_the_same_bits(eng, tl, theta, cen, sc, base, 16 // np.dtype(dtype).itemsize, p)


@pytest.mark.parametrize("n", (15, 16, 33))
def test_kernel_edges_along_the_observations(eng, edge_refs, n):
    lw, theta, cen, sc, ref = edge_case(edge_refs, 100, np.float64, n=33, p=16)
    res = kernel(eng, cuda(lw[:n]), cuda(theta), cen, sc)
    check(f"N={n}", res, {k: ref[k][:n] for k in KEYS})


# ------------------------------------------------------------------------------------------ 3. position independence, bit for bit
def test_rows_and_columns_permuted(eng, edge_refs):
    rng = np.random.default_rng(31)
    for p in (5, 20, 70):  # (20: a panel of two column tiles; 70: columns change panels)
        lw, theta, cen, sc, _ = edge_case(edge_refs, 257, np.float64, n=37, p=p)
        base = kernel(eng, cuda(lw), cuda(theta), cen, sc)
        rp, cp = rng.permutation(37), rng.permutation(p)
        rows = kernel(eng, cuda(lw[rp]), cuda(theta), cen, sc)
        for k in KEYS:
            assert np.array_equal(host(rows[k]), host(base[k])[rp]), (p, k, "rows")
        cols = kernel(eng, cuda(lw), cuda(theta[:, cp]), cen[cp], sc[cp])
        for k in ("shift", "m2"):
            assert np.array_equal(host(cols[k]), host(base[k])[:, cp]), (p, k, "columns")
        assert np.array_equal(host(cols["kl"]), host(base["kl"])) and np.array_equal(host(cols["ess_w"]), host(base["ess_w"]))
        # a column alone and inside the matrix
        j = int(cp[0])
        alone = kernel(eng, cuda(lw), cuda(theta[:, j]), cen[j:j + 1], sc[j:j + 1])
        assert np.array_equal(host(alone["shift"])[:, 0], host(base["shift"])[:, j]) and np.array_equal(host(alone["m2"])[:, 0], host(base["m2"])[:, j])


def test_row_selection_gives_the_bits_of_the_full_call(eng):
    import torch

    rng = np.random.default_rng(32)
    ll = make_ll(rng, 130, 1000)
    ll[7, 3] = np.nan
    ll[99, 998] = np.nan
    theta = wide_theta(rng, 1000, 20)
    cen, sc = influence_ref.center_scale(theta)
    M = orc.tail_count(1000, 0.6)
    rows = np.array([99, 3, 7, 129, 7, 0, 64, 99, 65, 7])
    full = eng.loo_influence(cuda(ll), cuda(theta), cen, sc, M, "psis", "loglik")
    keys = KEYS + ("diag",)
    for name, mat, idx in (("device, device list", cuda(ll), torch.as_tensor(rows).cuda()), ("device, host list", cuda(ll), rows.tolist()),
                           ("device obs-fastest", cuda(ll.T).T, torch.as_tensor(rows).cuda()), ("host", ll, rows)):
        th = theta if name == "host" else cuda(theta)
        res = eng.loo_influence(mat, th, cen, sc, M, "psis", "loglik", rows=idx)
        for k in keys:
            assert np.array_equal(host(res[k]), host(full[k])[rows], equal_nan=True), (name, k)
        assert int(host(res["n_replaced"]).reshape(-1)[0]) == 5  # (row 7 three times, row 99 twice)
    assert int(host(full["n_replaced"])[0]) == 2
    for bad in ([0, 130], [-1, 2]):
        with pytest.raises(IndexError):
            eng.loo_influence(ll, theta, cen, sc, M, "psis", "loglik", rows=bad)
    with pytest.raises(ValueError):
        eng.loo_influence(ll, theta, cen, sc, 0, "psis", "log_weights", rows=[1])


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import influence_ref
from pyloo_amd.engine import get_engine
eng = get_engine(0)
rng = np.random.default_rng(5)
n, s = 300, 1000
ll = (-rng.uniform(0.05, 0.9, size=(n, 1)) * rng.exponential(size=(n, s)) - 1.0).astype(np.float64)
ll[13, 7] = np.nan
ll[290, 999] = np.nan
rows = torch.as_tensor(rng.integers(0, n, size=280)).cuda()
out = []
for p in (5, 70):
    theta = rng.normal(size=(s, p))
    cen, sc = influence_ref.center_scale(theta)
    for t in (torch.as_tensor(ll).cuda(), torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T):
        for idx in (None, rows):
            r = eng.loo_influence(t, torch.as_tensor(theta).cuda(), cen, sc, 95, "psis", "loglik", rows=idx)
            out += [r[k].cpu().numpy() for k in ("shift", "m2", "kl", "ess_w", "diag", "n_replaced")]
np.savez(sys.argv[2], *out)
"""


def test_block_size_independence(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 cuts the 300 x 1000 f64 device matrix into three blocks of 131 observations -- tiles restart
    mid-matrix, the last block is ragged (38) -- and the 280 selected rows likewise: every output and the NaN count are the
    default's (one block), bit for bit, for both layouts and for one column tile and two panels."""
    outs = []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        env.update(env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            outs.append([z[k] for k in sorted(z.files, key=lambda s: int(s.split("_")[1]))])
    assert len(outs[0]) == 48
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)
    one = outs[0]
    assert int(one[5][0]) == 2 and one[0].shape == (300, 5) and one[6].shape == (280, 5) and one[24].shape == (300, 70)
    for base in (0, 24):  # the two layouts among each other, full and selected
        for j in range(12):
            assert np.array_equal(one[base + j], one[base + 12 + j], equal_nan=True)


# ----------------------------------------------------------------------------------------------------------------- 4. special rows
def test_special_rows(eng):
    """-inf weights drop out, rows of no weight and rows with a NaN give NaN; a one-hot row gives z at that draw, kl = log S and
    ess_w = 1, a uniform row shift 0, m2 = (S - 1) / S, kl = 0 and ess_w = S.  The one-hot shift, m2 and ess_w and the uniform kl and
    ess_w are exact (weights of exactly 1, products with exactly 0); the one-hot kl is the device's log(S), held to two units in
    the last place of NumPy's."""
    s = 100
    rng = np.random.default_rng(41)
    theta = influence_ref.make_theta(rng, s, 3)
    cen, sc = influence_ref.center_scale(theta)
    z = (theta - cen) / sc
    lw = 0.5 * rng.normal(size=(20, s))
    lw[0, ::2] = -np.inf         # weight 0 at every other draw
    lw[1] = -np.inf
    lw[2] = np.nan
    lw[3, 9] = np.nan
    lw[4] = -np.inf
    lw[4, 37] = 12.5             # one-hot
    lw[5] = 3.25                 # uniform
    lw[6, 50] = np.inf
    lw[18] = -np.inf             # (a second tile)
    lw[18, 99] = -700.0
    ref = influence_ref.from_log_weights(lw, theta, cen, sc)
    bad = [1, 2, 3, 6]
    assert np.nonzero(np.isnan(ref["kl"]))[0].tolist() == bad
    for a, th in ((cuda(lw), cuda(theta)), (lw, theta), (cuda(lw.T).T, cuda(theta.T).T)):
        res = kernel(eng, a, th, cen, sc)
        check("special rows", res, ref)
        got = {k: host(res[k]) for k in KEYS}
        for r, d in ((4, 37), (18, 99)):
            assert np.array_equal(got["shift"][r], z[d]) and np.array_equal(got["m2"][r], z[d] * z[d]) and got["ess_w"][r] == 1.0
            np.testing.assert_allclose(got["kl"][r], np.log(float(s)), rtol=4.5e-16, atol=0)
        assert np.abs(got["shift"][5]).max() <= 1e-12 and np.abs(got["m2"][5] - (s - 1.0) / s).max() <= 1e-12
        assert got["kl"][5] == 0.0 and got["ess_w"][5] == float(s)
        half = influence_ref.from_log_weights(lw[:1, 1::2], theta[1::2], cen, sc)
        np.testing.assert_allclose(got["shift"][0], half["shift"][0], rtol=0, atol=1e-12)
        assert np.all(got["kl"][~np.isnan(got["kl"])] >= -1e-12) and np.all(got["ess_w"][~np.isnan(got["kl"])] >= 1.0)


def test_nan_log_likelihood_is_counted_and_taken_as_minus_1e10(eng):
    rng = np.random.default_rng(42)
    s = 500
    ll = make_ll(rng, 6, s)
    ll[0, 3] = ll[0, 250] = np.nan
    ll[2] = -2.5                 # a constant row: uniform weights, k = inf
    theta = influence_ref.make_theta(rng, s)
    cen, sc = influence_ref.center_scale(theta)
    M = orc.tail_count(s, 1.0)
    ref = influence_ref.loo_influence(ll, theta, 1.0, center=cen, scale=sc)
    for mat, th in ((ll, theta), (cuda(ll), cuda(theta)), (cuda(ll.T).T, cuda(theta))):
        res = eng.loo_influence(mat, th, cen, sc, M, "psis", "loglik")
        assert int(host(res["n_replaced"]).reshape(-1)[0]) == 2
        check("NaN ll", res, ref)
        got = {k: host(res[k]) for k in KEYS}
        assert got["ess_w"][2] == float(s) and got["kl"][2] == 0.0 and np.isinf(host(res["diag"])[2])
        assert np.all(np.isfinite(got["shift"][0])) and np.isfinite(got["kl"][0])


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,s,method", [(70, 1000, "psis"), (40, 4100, "psis"), (70, 1000, "sis"), (70, 1000, "tis")])
def test_fused_route_is_the_kernel_on_the_weights_pass(eng, n, s, method, dtype):
    """``kind="loglik"`` is bit for bit ``kind="log_weights"`` on ``importance_weights(-ll)``, in every layout and memory space
    (S = 4100 takes the split weights route)."""
    rng = np.random.default_rng(500 + s)
    ll = make_ll(rng, n, s, dtype)
    theta = wide_theta(rng, s, 18)
    cen, sc = influence_ref.center_scale(theta)
    M = orc.tail_count(s, 1.0) if method == "psis" else 0
    tll = cuda(ll)
    lw, k = eng.importance_weights(-tll, M, method)
    want = kernel(eng, lw, cuda(theta), cen, sc)
    for name, mat in {"device draws": tll, "device obs": cuda(ll.T).T, "host draws": ll, "host obs": np.ascontiguousarray(ll.T).T}.items():
        res = eng.loo_influence(mat, theta if name.startswith("host") else cuda(theta), cen, sc, M, method, "loglik")
        text = eng.last_kernels()
        assert "influence_kernel" in text and ("diag_prepare_tile_kernel" if name.endswith("obs") else "diag_prepare_row_kernel") in text, text
        assert ("staged in blocks" in text) == name.startswith("host"), text
        assert same_bits(res, want), (name, method)
        assert np.array_equal(host(res["diag"]), host(k), equal_nan=True), name
    if dtype == np.float64:
        check(f"fused {method} S={s}", want, influence_ref.loo_influence(ll, theta, 1.0, method=method, center=cen, scale=sc))


R2 = np.where(np.arange(90) % 3 == 0, 0.25, 0.8)  # two buckets, interleaved


@pytest.mark.parametrize("where", ["host", "device", "device obs-fastest"])
def test_fronts_end_to_end(eng, where):
    import pyloo_amd as pl

    rng = np.random.default_rng(51)
    ll = make_ll(rng, 90, 1000)
    ll *= 0.4  # (every k far below the threshold: no warning)
    theta = influence_ref.make_theta(rng, 1000)
    mat, th = {"host": (ll, theta), "device": (cuda(ll), cuda(theta)), "device obs-fastest": (cuda(ll.T).T, cuda(theta))}[where]
    for reff in (0.7, R2):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            res = pl.loo_influence_from_matrix(mat, th, reff=cuda(reff) if where == "device" and np.ndim(reff) else reff, names=list("abcde"))
        assert not [w for w in rec if "Pareto" in str(w.message) or "NaN" in str(w.message)]
        # (torch's column mean and sd on the device, NumPy's on the host: the restatement below takes the front's own)
        np.testing.assert_allclose(res.center, influence_ref.center_scale(theta)[0], rtol=1e-13)
        np.testing.assert_allclose(res.scale, influence_ref.center_scale(theta)[1], rtol=1e-9)
        ref = influence_ref.loo_influence(ll, theta, reff, center=res.center, scale=res.scale)
        want = influence_ref.front_values(ref, theta)
        check(f"{where} reff={'vector' if np.ndim(reff) else reff}", {"shift": res.shift, "m2": res.sd_ratio ** 2 + res.shift ** 2,
                                                                      "kl": res.kl, "ess_w": res.ess_w}, ref)
        np.testing.assert_allclose(res.pareto_k, ref["diag"], rtol=1e-9)
        np.testing.assert_allclose(res.sd_ratio, want["sd_ratio"], rtol=0, atol=1e-8)
        np.testing.assert_allclose((res.mean_loo - want["mean_loo"]) / res.scale, 0.0, rtol=0, atol=1e-8)  # (in units of the scale)
        # (|d distance| <= 2 P |shift| |R^+| |d shift|: five columns, shifts below 1, |R^+| = 1 / (1 - 0.8^2) = 2.8)
        np.testing.assert_allclose(res.distance, want["distance"], rtol=0, atol=3e-7)
        assert res.names == list("abcde") and res.n_replaced == 0 and res.shift.shape == (90, 5)
        if np.ndim(reff):
            assert sorted(set(ref["M"].tolist())) == sorted({orc.tail_count(1000, 0.25), orc.tail_count(1000, 0.8)})
    sub = pl.loo_influence_from_matrix(mat, th, reff=R2, rows=[5, 3, 88, 3])
    assert np.array_equal(sub.shift, res.shift[[5, 3, 88, 3]]) and np.array_equal(sub.pareto_k, res.pareto_k[[5, 3, 88, 3]])
    t = pl.influence_table(res, n=4)
    assert len(t) == 4 and t["distance"].iloc[0] == np.nanmax(res.distance) and set(t["column"]) <= set("abcde")


def test_argument_errors_of_the_entry(eng):
    import ctypes as C

    from pyloo_amd import _capi

    lw = np.zeros((4, 16))
    th, c, s = np.arange(16.0), np.zeros(1), np.ones(1)
    out = np.empty(4)
    p = lambda x: x.ctypes.data  # noqa: E731

    def call(**kw):
        a = _capi.InfluenceArgs(engine=eng._h.value, mat=p(lw), dtype=_capi.PLA_F64, kind=_capi.PLA_PIT_LOG_WEIGHTS, mem_space=_capi.PLA_HOST,
                                n_obs=4, n_draws=16, stride_obs=16, stride_draw=1, theta=p(th), n_quant=1, theta_stride_draw=1,
                                theta_stride_quant=1, center=p(c), scale=p(s), kl=p(out))
        for k, v in kw.items():
            setattr(a, k, v)
        return eng._lib.pla_loo_influence(C.byref(a))

    assert call() == 0 and np.all(out == 0.0)  # (uniform rows; the other outputs may be NULL)
    assert call(n_quant=0) == -1 and call(n_quant=1025) == -1 and call(theta=None) == -1 and call(mat=None) == -1
    assert call(kind=7) == -1 and call(n_draws=1) == -1 and call(stride_draw=0) == -1
    assert call(row_index=p(np.zeros(1, dtype=np.int64)), n_rows=1) == -1
    assert call(stride_obs=32, stride_draw=2) == -4 and call(n_quant=2, theta_stride_draw=3, theta_stride_quant=1) == -4
    assert call(kind=_capi.PLA_PIT_LOGLIK, method=_capi.PLA_PSIS, tail_count=16) == -1  # a tail longer than the row
