"""The GLM log-likelihood generator (csrc/pla_glm.h, ``pla_glm``) and its fronts on the GPU.

Bounds, each derived or the project's own:
  1. the GEMM      |eta - exact| <= gamma_{P+1} (sum_p |x_ip beta_sp| + |offset_i|), gamma_n = n u / (1 - n u), u = 2^-53, against the
                   restatement in np.longdouble: the standard dot-product bound, any order of summation, fused multiply-adds or not
  2. the densities |ll - restatement(kernel's own eta)| <= 1e-10 max(1, |ll|): device exp / log1p against libm on identical
                   arguments, the project's aim for pointwise outputs
  3. end to end    loo_i, lppd_i and k within 1e-9 of the oracle on the restatement's matrix (the existing bounds)
  4. same bits     every entry of ll under permuted rows and draws, row lists, layouts, memory spaces and block sizes
Largest deviations are printed (pytest -s)."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import glm_ref
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."
FAMILIES = ("gaussian", "binomial", "poisson")


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def cuda(a):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


def engine_vectors(m):
    """What the fronts hand to ``Engine.glm`` for a model of glm_ref.make_model."""
    fam = glm_ref.ENGINE_FAMILY[m["family"]]
    oc = None if m["family"] in ("gaussian", "bernoulli") else glm_ref.obs_const(fam, m["y"], m["trials"])
    dc = None if m["sigma"] is None else glm_ref.draw_const(m["sigma"])
    return fam, dict(y=m["y"], offset=m["offset"], trials=m["trials"], obs_const=oc, draw_scale=m["sigma"], draw_const=dc)


def front(m, where="host"):
    put = cuda if where == "device" else (lambda a: a)
    return (put(m["X"]), put(m["y"]), put(m["beta"]), m["family"]), dict(sigma=put(m["sigma"]), offset=put(m["offset"]), trials=put(m["trials"]))


# --------------------------------------------------------------------------------------------------------------------- 1. the GEMM
GEMM_N, GEMM_S = (1, 15, 16, 17, 33), (1, 2, 15, 16, 17, 250)


@pytest.mark.parametrize("p", (1, 3, 4, 5, 16, 17, 64, 65, 256))
def test_linear_predictor_within_the_dot_product_bound(eng, p):
    rng = np.random.default_rng(100 + p)
    X, beta, off = rng.normal(size=(33, p)), rng.normal(size=(250, p)), rng.normal(size=33)
    exact = glm_ref.linpred(X, beta, off, dtype=np.longdouble)
    bound = glm_ref.linpred_bound(X, beta, off)
    Xd, bd, od = cuda(X), cuda(beta), cuda(off)
    worst = 0.0
    full = None
    for n in GEMM_N:
        for s in GEMM_S:
            eta = host(eng.glm(Xd[:n], bd[:s], "linpred", offset=od[:n]))
            assert eta.shape == (n, s)
            err = np.abs(eta.astype(np.longdouble) - exact[:n, :s]).astype(np.float64)
            worst = max(worst, float((err / bound[:n, :s]).max()))
            assert np.all(err <= bound[:n, :s]), (n, s, p, float((err / bound[:n, :s]).max()))
            if (n, s) == (33, 250):
                full = eta
            if n == 17 and s in (1, 17):  # the host route, and no offset
                assert np.array_equal(eng.glm(X[:n], beta[:s], "linpred", offset=off[:n]), eta)
                plain = eng.glm(X[:n], beta[:s], "linpred")
                err = np.abs(plain.astype(np.longdouble) - glm_ref.linpred(X[:n], beta[:s], None, dtype=np.longdouble)).astype(np.float64)
                assert np.all(err <= glm_ref.linpred_bound(X[:n], beta[:s], None))
    # an entry does not depend on the shape of the call it is computed in
    for n in GEMM_N:
        for s in (1, 17):
            assert np.array_equal(host(eng.glm(Xd[:n], bd[:s], "linpred", offset=od[:n])), full[:n, :s])
    text = eng.last_kernels()
    chunks = 1 if p <= 16 else 2 if p <= 32 else 4 if p <= 64 else 8
    assert f"{chunks} chunks of 16 predictors" in text and ("per panel" in text) == (p > 128), text
    print(f"P = {p}: largest |eta - exact| / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- 2. the densities
def density_case(rng, family, n=45, s=130):
    """eta of both signs up to |eta| = 40 (Poisson: 40 as well, exp(40) = 2.4e17), y = 0 among the outcomes."""
    X = np.column_stack([np.ones(n), np.linspace(-40.0, 40.0, n), rng.normal(size=n)])
    beta = np.column_stack([0.01 * rng.normal(size=s), np.linspace(-1.0, 1.0, s), 0.01 * rng.normal(size=s)])
    beta[0], beta[-1] = (0.0, -1.0, 0.0), (0.0, 1.0, 0.0)
    m = dict(X=X, beta=beta, family=family, sigma=None, trials=None, offset=0.01 * rng.normal(size=n))
    if family == "gaussian":
        m["sigma"] = np.exp(rng.normal(size=s))
        m["y"] = 10.0 * rng.normal(size=n)
    elif family == "binomial":
        m["trials"] = rng.integers(1, 30, size=n).astype(np.float64)
        m["y"] = np.floor(rng.uniform(size=n) * (m["trials"] + 1.0))
        m["y"][:3] = 0.0
    else:
        m["y"] = rng.poisson(3.0, size=n).astype(np.float64)
        m["y"][:3] = 0.0
    return m


@pytest.mark.parametrize("family", FAMILIES + ("bernoulli",))
def test_densities_against_the_restatement_on_the_kernels_own_eta(eng, family):
    import pyloo_amd as pl

    rng = np.random.default_rng(7)
    m = density_case(rng, "binomial" if family == "bernoulli" else family)
    if family == "bernoulli":
        m.update(family="bernoulli", trials=None, y=(m["y"] > 0).astype(np.float64))
    fam, v = engine_vectors(m)
    for where in ("device", "host"):
        a, k = front(m, where)
        ll = host(pl.glm_log_lik(*a, **k))
        eta = host(pl.glm_log_lik(*a, **k, linpred=True))
        assert np.abs(eta).max() >= 40.0 and eta.min() < -39.0
        want = glm_ref.density(fam, eta, m["y"], sigma=m["sigma"], trials=m["trials"], oc=v["obs_const"], dc=v["draw_const"])
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(want))
        dev = np.abs(ll - want) / np.maximum(1.0, np.abs(want))
        print(f"{family} ({where}): largest |ll - restatement| / max(1, |ll|) = {dev.max():.3e}")
        assert np.all(dev <= 1e-10), dev.max()


@pytest.mark.parametrize("family", FAMILIES)
def test_values_that_are_not_finite_propagate(eng, family):
    """inf and NaN entries of sigma, X and beta, handed to the engine directly (the fronts reject them): NaN where the restatement
    has NaN, inf where it has inf, on the linear predictor and on the density of the kernel's own eta."""
    rng = np.random.default_rng(8)
    m = glm_ref.make_model(rng, 21, 40, 6, family, with_offset=True)
    fam, v = engine_vectors(m)
    X, beta = m["X"].copy(), m["beta"].copy()
    X[2, 1], X[5, 3], X[9, 0], X[9, 4] = np.inf, np.nan, np.inf, -np.inf
    beta[4, 2], beta[17, 5], beta[30, 1] = np.nan, -np.inf, 0.0  # (inf times zero: row 2 meets draw 30)
    if family == "gaussian":
        v["draw_scale"] = v["draw_scale"].copy()
        v["draw_scale"][3], v["draw_scale"][8] = np.inf, np.nan
    for put in (cuda, lambda a: a):
        eta = host(eng.glm(put(X), put(beta), "linpred", offset=put(m["offset"])))
        ref_eta = glm_ref.linpred(X, beta, m["offset"])
        assert np.array_equal(np.isnan(eta), np.isnan(ref_eta)) and np.array_equal(np.isposinf(eta), np.isposinf(ref_eta))
        assert np.array_equal(np.isneginf(eta), np.isneginf(ref_eta)) and np.isnan(eta).sum() > 40 and np.isnan(eta[2, 30])
        ll = host(eng.glm(put(X), put(beta), fam, **{k: put(a) for k, a in v.items()}))
        want = glm_ref.density(fam, eta, m["y"], sigma=v["draw_scale"], trials=m["trials"], oc=v["obs_const"], dc=v["draw_const"])
        assert np.array_equal(np.isnan(ll), np.isnan(want)) and np.array_equal(np.isposinf(ll), np.isposinf(want))
        assert np.array_equal(np.isneginf(ll), np.isneginf(want))
        ok = np.isfinite(want)
        assert np.all(np.abs(ll[ok] - want[ok]) <= 1e-10 * np.maximum(1.0, np.abs(want[ok])))


# ------------------------------------------------------------------------------------------------ 3. end to end against the oracle
ORACLE = {}


def oracle_case(n, s, p, family):
    key = (n, s, p, family)
    if key not in ORACLE:
        m = glm_ref.make_model(np.random.default_rng(n * 7 + p), n, s, p, family, with_offset=True)
        ORACLE[key] = (m, orc.loo_pointwise(glm_ref.matrix_of(m), 1.0, "psis"))
    return ORACLE[key]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,s,p", [(37, 1000, 5), (19, 4000, 67), (5, 4100, 5)])
def test_end_to_end_against_the_oracle(eng, n, s, p, family, where):
    import pyloo_amd as pl

    m, ref = oracle_case(n, s, p, family)
    a, k = front(m, where)
    res, msgs = quiet(pl.loo_glm_from_design, *a, **k, pointwise=True)
    assert not msgs, msgs
    text = eng.last_kernels()
    assert text.startswith("glm_prepare_kernel -> glm_kernel<") and text.endswith("per block of observations"), text
    loo_i, khat = host(res["loo_i"]), host(res["pareto_k"])
    print(f"{family} {n} x {s} x {p} ({where}): loo_i {np.abs(loo_i - ref['loo_i']).max():.2e}, k {np.abs(khat - ref['diag']).max():.2e}")
    np.testing.assert_allclose(loo_i, ref["loo_i"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(khat, ref["diag"], rtol=0, atol=1e-9)
    fam, v = engine_vectors(m)
    put = cuda if where == "device" else (lambda x: x)
    raw = eng.glm(put(m["X"]), put(m["beta"]), fam, mode="loo", tail_count=orc.tail_count(s, 1.0), good_k=0.7,
                  **{key: put(x) for key, x in v.items()})
    np.testing.assert_allclose(host(raw["lppd_i"]), ref["lppd_i"], rtol=0, atol=1e-9)
    assert int(raw["n_replaced"]) == 0 and res["n_data_points"] == n and res["n_samples"] == s
    np.testing.assert_allclose(res["elpd_loo"], ref["loo_i"].sum(), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(res["p_loo"], ref["lppd_i"].sum() - ref["loo_i"].sum(), rtol=0, atol=1e-7)


# -------------------------------------------------------------------------------------------------------------------- 4. same bits
@pytest.fixture(scope="module")
def bit_models():
    rng = np.random.default_rng(31)
    return {f: glm_ref.make_model(rng, 53, 301, 7 if f != "poisson" else 70, f, with_offset=True) for f in FAMILIES}


@pytest.mark.parametrize("family", FAMILIES)
def test_ll_bits_do_not_depend_on_rows_draws_lists_layouts_or_memory_space(eng, bit_models, family):
    import torch

    import pyloo_amd as pl

    m = bit_models[family]
    n, s = 53, 301
    p = m["X"].shape[1]
    a, k = front(m, "device")
    base = host(pl.glm_log_lik(*a, **k))
    assert base.shape == (n, s)
    rng = np.random.default_rng(32)
    # permuted rows
    perm = rng.permutation(n)
    mp = dict(m, X=m["X"][perm], y=m["y"][perm], offset=m["offset"][perm], trials=None if m["trials"] is None else m["trials"][perm])
    a2, k2 = front(mp, "device")
    assert np.array_equal(host(pl.glm_log_lik(*a2, **k2)), base[perm])
    # permuted draws
    dperm = rng.permutation(s)
    md = dict(m, beta=m["beta"][dperm], sigma=None if m["sigma"] is None else m["sigma"][dperm])
    a3, k3 = front(md, "device")
    assert np.array_equal(host(pl.glm_log_lik(*a3, **k3)), base[:, dperm])
    # a row list that is unsorted and has repeats; as a tensor and as a list; a single row, a single draw
    rows = [52, 0, 17, 17, 3, 52, 16, 31]
    assert np.array_equal(host(pl.glm_log_lik(*a, **k, rows=rows)), base[rows])
    assert np.array_equal(host(pl.glm_log_lik(*a, **k, rows=torch.as_tensor(rows).cuda())), base[rows])
    one = dict(m, X=m["X"][40:41], y=m["y"][40:41], offset=m["offset"][40:41], trials=None if m["trials"] is None else m["trials"][40:41])
    a4, k4 = front(one, "device")
    assert np.array_equal(host(pl.glm_log_lik(*a4, **k4)), base[40:41])
    few = dict(m, beta=m["beta"][299:300], sigma=None if m["sigma"] is None else m["sigma"][299:300])
    a5, k5 = front(few, "device")
    assert np.array_equal(host(pl.glm_log_lik(*a5, **k5)), base[:, 299:300])
    # .T views and padded pitches of X and beta
    Xt = cuda(np.ascontiguousarray(m["X"].T)).T
    bt = cuda(np.ascontiguousarray(m["beta"].T)).T
    Xp = torch.zeros(n, p + 3, dtype=torch.float64, device="cuda")[:, :p].copy_(cuda(m["X"]))
    bp = torch.zeros(s, 2 * p, dtype=torch.float64, device="cuda")[:, ::2].copy_(cuda(m["beta"]))
    assert Xt.stride() == (1, n) and bt.stride() == (1, s) and Xp.stride() == (p + 3, 1) and bp.stride() == (2 * p, 2)
    for Xv, bv in ((Xt, bt), (Xp, bp), (Xt, bp)):
        assert np.array_equal(host(pl.glm_log_lik(Xv, a[1], bv, family, **k)), base)
        assert np.array_equal(host(pl.glm_log_lik(Xv, a[1], bv, family, **k, rows=rows)), base[rows])
    # host against device input, a host .T view included.  ll is a function of the vectors' entries: the two memory spaces are
    # handed the same obs_const / draw_const here (the fronts compute them with scipy and NumPy on the host, with torch on the
    # device, and those may differ in the last bit -- the fronts agree to that, not to the bit)
    fam, v = engine_vectors(m)
    dev = host(eng.glm(cuda(m["X"]), cuda(m["beta"]), fam, **{key: cuda(x) for key, x in v.items()}))
    assert np.array_equal(eng.glm(m["X"], m["beta"], fam, **v), dev)
    assert np.array_equal(eng.glm(np.ascontiguousarray(m["X"].T).T, np.ascontiguousarray(m["beta"].T).T, fam, **v), dev)
    assert np.array_equal(eng.glm(m["X"], m["beta"], fam, rows=rows, **v), dev[rows])
    ah, kh = front(m, "host")
    assert np.array_equal(pl.glm_log_lik(*ah, **kh), dev)  # (the host front hands over exactly these vectors)
    assert np.all(np.abs(base - dev) <= 1e-10 * np.maximum(1.0, np.abs(dev)))  # (the device front: the project's aim for pointwise outputs)


def loo_kernels(text):
    """The LOO kernels named by the fused route's text."""
    assert text.startswith("glm_prepare_kernel -> glm_kernel<") and text.endswith(" per block of observations"), text
    return text.split(" -> ", 2)[2][: -len(" per block of observations")]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("method", ["psis", "sis", "tis"])
@pytest.mark.parametrize("n,s,p", [(53, 301, 7), (40, 1000, 20), (6, 4100, 3)])
def test_fused_pass_equals_loo_from_matrix_on_the_generated_matrix(eng, n, s, p, method, where):
    import pyloo_amd as pl

    m = glm_ref.make_model(np.random.default_rng(n + s), n, s, p, "binomial", with_offset=True)
    a, k = front(m, where)
    fused, _ = quiet(pl.loo_glm_from_design, *a, **k, method=method, pointwise=True, reff=0.9)
    fused_text = loo_kernels(eng.last_kernels())
    ll = pl.glm_log_lik(*a, **k)
    # like with like: the block the fused pass consumes is device-resident, so is the yardstick's matrix
    plain, _ = quiet(pl.loo_from_matrix, cuda(host(ll)), method=method, pointwise=True, reff=0.9)
    plain_text = eng.last_kernels()
    diag = "pareto_k" if method == "psis" else "ess"
    assert list(fused.index) == list(plain.index)
    assert fused_text == plain_text, (fused_text, plain_text)  # the block takes the route a resident (N, S) f64 tensor takes
    for key in ("loo_i", diag):
        assert np.array_equal(host(fused[key]), host(plain[key])), (key, fused_text)
    for key in ("elpd_loo", "se", "p_loo", "p_loo_se", "looic", "looic_se"):
        np.testing.assert_allclose(fused[key], plain[key], rtol=1e-12, err_msg=key)
    assert fused["warning"] == plain["warning"] and fused["n_data_points"] == n
    if where == "host":  # the host matrix is staged in blocks of its own: the cross-route bound of tests/test_gpu_parity.py
        staged, _ = quiet(pl.loo_from_matrix, ll, method=method, pointwise=True, reff=0.9)
        for key in ("loo_i", diag):
            np.testing.assert_allclose(host(fused[key]), host(staged[key]), rtol=1e-11, atol=1e-12, err_msg=key)


# ----------------------------------------------------------------------------------------------------------------------- 5. blocks
CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import glm_ref
import pyloo_amd as pl
from pyloo_amd.engine import get_engine
eng = get_engine(0)
out, texts = [], []
rows = np.random.default_rng(3).integers(0, 3000, size=2500)
for family in ("gaussian", "binomial", "poisson"):
    m = glm_ref.make_model(np.random.default_rng(41), 3000, 1000, 8, family, with_offset=True)
    fam = glm_ref.ENGINE_FAMILY[family]
    oc = None if family == "gaussian" else glm_ref.obs_const(fam, m["y"], m["trials"])
    dc = None if m["sigma"] is None else glm_ref.draw_const(m["sigma"])
    off = m["offset"].copy()
    off[[7, 2990]] = np.nan
    v = dict(y=m["y"], offset=off, trials=m["trials"], obs_const=oc, draw_scale=m["sigma"], draw_const=dc)
    cu = lambda a: None if a is None else torch.as_tensor(a).cuda()
    for where in ("device", "host"):
        put = cu if where == "device" else (lambda a: a)
        vv = {k: put(a) for k, a in v.items()}
        for idx in (None, rows):
            r = eng.glm(put(m["X"]), put(m["beta"]), fam, rows=idx, mode="loo", tail_count=95, good_k=0.7, **vv)
            texts.append(eng.last_kernels())
            out += [np.asarray(r[k].cpu().numpy() if hasattr(r[k], "cpu") else r[k]).reshape(-1) for k in ("diag", "loo_i", "lppd_i", "agg", "n_replaced")]
        ll = eng.glm(put(m["X"]), put(m["beta"]), fam, rows=rows[:40], **vv)
        out.append(np.asarray(ll.cpu().numpy() if hasattr(ll, "cpu") else ll))
np.savez(sys.argv[2], *out)
open(sys.argv[2] + ".txt", "w").write("\n".join(texts))
"""


def test_block_size_independence(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 cuts the 3000 x 1000 pass into 23 blocks of 131 observations -- tiles of 16 restart mid-matrix, the last
    block is ragged -- and the 2500 listed rows likewise: the route says "per block of observations" and every pointwise output,
    the NaN count and the matrix entries are the default's (one block) bit for bit, host and device; the aggregates to 1e-12."""
    outs, texts = [], []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        env.update(env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            outs.append([z[k] for k in sorted(z.files, key=lambda s: int(s.split("_")[1]))])
        texts.append(open(str(path) + ".txt").read().split("\n"))
    assert len(outs[0]) == 3 * 2 * 11 and texts[0] == texts[1]
    assert all(t.endswith("per block of observations") and t.startswith("glm_prepare_kernel -> glm_kernel<") for t in texts[1])
    for j, (a, b) in enumerate(zip(*outs)):
        if j % 11 in (3, 8):  # the aggregates
            np.testing.assert_allclose(a, b, rtol=1e-12, equal_nan=True)
        else:
            assert np.array_equal(a, b, equal_nan=True), j
    one = outs[0]
    for f in range(3):
        dev, hst = one[22 * f: 22 * f + 11], one[22 * f + 11: 22 * f + 22]
        assert int(dev[4][0]) == 2000 and int(hst[4][0]) == 2000 and dev[0].shape == (3000,) and dev[5].shape == (2500,)
        for j, (a, b) in enumerate(zip(dev, hst)):  # host against device input
            if j in (3, 8):
                np.testing.assert_allclose(a, b, rtol=1e-12, equal_nan=True)
            else:
                assert np.array_equal(a, b, equal_nan=True), j


# ------------------------------------------------------------------------------------------------------------------ 6. NaN counting
def test_nan_is_counted_replaced_and_warned_about(eng, monkeypatch):
    import pyloo_amd as pl

    m = glm_ref.make_model(np.random.default_rng(51), 40, 500, 4, "poisson", with_offset=True)
    fam, v = engine_vectors(m)
    off = m["offset"].copy()
    off[[3, 38]] = np.nan
    ll = glm_ref.matrix_of(m)
    ll[[3, 38]] = -1e10
    ref = orc.loo_pointwise(ll, 1.0, "psis")
    for put in (cuda, lambda a: a):
        vv = {k: put(a) for k, a in dict(v, offset=off).items()}
        r = eng.glm(put(m["X"]), put(m["beta"]), fam, mode="loo", tail_count=orc.tail_count(500, 1.0), good_k=0.7, **vv)
        assert int(r["n_replaced"]) == 2 * 500
        ok = np.ones(40, dtype=bool)
        ok[[3, 38]] = False
        np.testing.assert_allclose(host(r["loo_i"])[ok], ref["loo_i"][ok], rtol=0, atol=1e-9)
        np.testing.assert_allclose(host(r["loo_i"])[~ok], ref["loo_i"][~ok], rtol=1e-12)
        mat = host(eng.glm(put(m["X"]), put(m["beta"]), fam, **vv))  # the matrix mode passes the NaN through
        assert np.isnan(mat[[3, 38]]).all() and np.isfinite(mat[ok]).all()
    # the front's warning: the NaN injected behind its checks
    real = eng.glm

    def with_nan(X, beta, family, **kw):
        kw["offset"] = off
        return real(X, beta, family, **kw)

    monkeypatch.setattr(eng, "glm", with_nan)
    a, k = front(m, "host")
    res, msgs = quiet(pl.loo_glm_from_design, *a, **k)
    assert msgs.count(NAN_TEXT) == 1 and res["n_data_points"] == 40


# --------------------------------------------------------------------------------------------------------------- 7. subsampled LOO
@pytest.mark.parametrize("estimator", ["diff_srs", "hh_pps", "srs"])
def test_loo_subsample_glm_on_the_device(eng, estimator):
    import pyloo_amd as pl

    m = glm_ref.make_model(np.random.default_rng(61), 400, 500, 6, "gaussian", with_offset=True)
    a, k = front(m, "device")
    ll = pl.glm_log_lik(*a, **k)
    np.random.seed(11)
    (got, idx, est), msgs = quiet(pl.loo_subsample_glm, *a, **k, observations=50, loo_approximation="lpd", estimator=estimator,
                                  loo_approximation_draws=100, pointwise=True)
    np.random.seed(11)
    (want, widx, west), wmsgs = quiet(pl.loo_subsample_from_matrix, ll, observations=50, loo_approximation="lpd", estimator=estimator,
                                      loo_approximation_draws=100, pointwise=True)
    assert np.array_equal(idx.idx, widx.idx) and np.array_equal(idx.m_i, widx.m_i) and msgs == wmsgs
    np.testing.assert_allclose(np.array(est[:4], dtype=float), np.array(west[:4], dtype=float), rtol=1e-9)
    for key in ("elpd_loo", "se", "p_loo", "p_loo_se", "subsampling_SE"):
        np.testing.assert_allclose(got[key], want[key], rtol=1e-9, err_msg=key)
    np.testing.assert_allclose(got["loo_i"], want["loo_i"], rtol=1e-9, equal_nan=True)
    # "plpd": the log-likelihood at the posterior mean, no warning; it never sees a matrix
    np.random.seed(12)
    (p_got, p_idx, p_est), msgs = quiet(pl.loo_subsample_glm, *a, **k, observations=50, loo_approximation="plpd", estimator=estimator)
    # (no fallback and no warning about one; the diagnostics of the 50 sampled rows may speak, as they do for "lpd" above)
    assert not any("PLPD" in t or "approximate" in t for t in msgs), msgs
    assert p_got["subsample_size"] == len(p_idx.idx) and np.isfinite(p_got["elpd_loo"])
    plpd = host(pl.glm_plpd(*a, **k))
    want_plpd = glm_ref.log_lik(m["X"], m["y"], m["beta"].mean(0).reshape(1, -1), "gaussian", m["sigma"].mean().reshape(1), m["offset"])[:, 0]
    np.testing.assert_allclose(plpd, want_plpd, rtol=0, atol=1e-10)
    full = float(quiet(pl.loo_from_matrix, ll)[0]["elpd_loo"])
    if estimator != "hh_pps":  # (the Hansen-Hurwitz estimate normalises its probabilities within the sample, as the reference does)
        assert abs(p_got["elpd_loo"] - full) <= 6.0 * p_got["se"] + 6.0 * p_got["subsampling_SE"]
