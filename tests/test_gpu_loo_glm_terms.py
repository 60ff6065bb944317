"""The GLM generator with group-level terms (csrc/pla_glm_terms.h, ``pla_glm_grouped``) and ``groups=`` of its fronts on the GPU.

Bounds, each the issue's, derived or the project's own:
  1. the terms     eta with terms == the device's own eta without them, the terms added in NumPy f64 in the specified order: the same
                   roundings in the same order, so bit for bit
  2. the densities |ll - restatement(kernel's own eta)| <= 1e-10 max(1, |ll|), the bound of tests/test_gpu_loo_glm.py
  3. same bits     every entry under permuted rows and draws, relabelled groups, layouts of u, row lists, memory spaces, block sizes
  4. no terms      the new entry with n_terms = 0 gives the bits of pla_glm
  5. fused pass    pointwise outputs == loo_from_matrix(glm_log_lik(groups=...)); aggregates to 1e-12 relative (the existing test's)
  6. end to end    loo_i, lppd_i and k within 1e-9 of the oracle on the restatement's matrix (the existing bounds)
Largest deviations are printed (pytest -s)."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import glm_ref
import glmm_ref
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


def put_terms(terms, put):
    return [tuple(put(v) for v in glmm_ref.split(t)) for t in terms]


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


def engine_vectors(m):
    """What the fronts hand to ``Engine.glm`` for a model of glmm_ref.make_model."""
    fam = glm_ref.ENGINE_FAMILY[m["family"]]
    oc = None if m["family"] in ("gaussian", "bernoulli") else glm_ref.obs_const(fam, m["y"], m["trials"])
    dc = None if m["sigma"] is None else glm_ref.draw_const(m["sigma"])
    return fam, dict(y=m["y"], offset=m["offset"], trials=m["trials"], obs_const=oc, draw_scale=m["sigma"], draw_const=dc)


def front(m, where="host"):
    put = cuda if where == "device" else (lambda a: a)
    return ((put(m["X"]), put(m["y"]), put(m["beta"]), m["family"]),
            dict(sigma=put(m["sigma"]), offset=put(m["offset"]), trials=put(m["trials"]), groups=put_terms(m["terms"], put)))


def terms_route(text, n_terms):
    assert text.startswith("glm_prepare_kernel -> glm_terms_prepare_kernel -> glm_terms_kernel<") and f"{n_terms} group-level terms>" in text, text


# -------------------------------------------------------------------------------------------- 1. the linear predictor, bit for bit
# Axes of the issue and the values taken: N and S in {1, 15, 16, 17, 33} x {1, 15, 16, 17, 250}, all 25 pairs at T = 2, G = 7; at
# (N, S) = (17, 17) and (33, 250) every T in {1, 2, 8} x G in {1, 2, 7, N} with z mixed, all given and all null; every P in
# {1, 17, 65, 130} (130: the panel route).  Indices are unsorted inside a tile, group G - 1 is held by the last row only, terms 0
# and 1 share one index vector.
LIN_N, LIN_S = (1, 15, 16, 17, 33), (1, 15, 16, 17, 250)


def linpred_terms(rng, n, s, n_terms, g, z_mode):
    terms, _ = glmm_ref.make_terms(rng, n, s, [g] * n_terms, [z_mode == "given" or (z_mode == "mixed" and t % 2 == 1) for t in range(n_terms)])
    if n_terms > 1:
        terms[1] = (terms[0][0], *terms[1][1:])  # two terms share one index vector
    return terms


@pytest.mark.parametrize("p", (1, 17, 65, 130))
def test_linear_predictor_with_terms_bit_for_bit(eng, p):
    import pyloo_amd as pl

    rng = np.random.default_rng(200 + p)
    X, beta, off = rng.normal(size=(33, p)), rng.normal(size=(250, p)), rng.normal(size=33)
    y = np.zeros(33)
    Xd, bd, od, yd = cuda(X), cuda(beta), cuda(off), cuda(y)
    cases = [(n, s, 2, 7, "mixed") for n in LIN_N for s in LIN_S]
    cases += [(n, s, t, g, z) for n, s in ((17, 17), (33, 250)) for t in (1, 2, 8) for g in (1, 2, 7, n) for z in ("mixed", "given", "null")]
    for n, s, n_terms, g, z_mode in cases:
        terms = linpred_terms(rng, n, s, n_terms, g, z_mode)
        if g > 1 and n > 1:
            first = terms[0][0]
            assert first[-1] == g - 1 and np.all(first[:-1] < g - 1) and (n < 4 or g < 3 or np.any(np.diff(first[:-1]) < 0))
        base = host(pl.glm_log_lik(Xd[:n], yd[:n], bd[:s], "gaussian", sigma=np.ones(s), offset=od[:n], linpred=True))
        want = glmm_ref.add_terms(base, terms)
        got = host(pl.glm_log_lik(Xd[:n], yd[:n], bd[:s], "gaussian", sigma=np.ones(s), offset=od[:n], linpred=True, groups=put_terms(terms, cuda)))
        assert got.shape == (n, s) and np.array_equal(got, want), (n, s, p, n_terms, g, z_mode, np.abs(got - want).max())
        assert not np.array_equal(got, base)
        if (n, s) == (17, 17) and g == 7:  # the host route
            assert np.array_equal(pl.glm_log_lik(X[:n], y[:n], beta[:s], "gaussian", sigma=np.ones(s), offset=off[:n], linpred=True, groups=terms), want)
    text = eng.last_kernels()
    chunks = 1 if p <= 16 else 2 if p <= 32 else 4 if p <= 64 else 8
    terms_route(text, cases[-1][2])
    assert f"{chunks} chunks of 16 predictors" in text and ("per panel" in text) == (p > 128), text


def test_image_rows_past_2_to_the_31_elements(eng):
    """sum G * s_pad = 2^31 + 16 elements: the last group's image row lies past what a 32-bit index reaches.  u is an overlapping
    view with strides (1, 1), u[s, j] = w[s + j], so the call's input is 1 GiB and the image 16 GiB of engine memory."""
    import torch

    s, g, n = 16, 2 ** 27 + 1, 20
    rng = np.random.default_rng(5)
    w = torch.randn(g + s, dtype=torch.float64, device="cuda")
    u = torch.as_strided(w, (s, g), (1, 1))
    index = rng.integers(0, g, size=n)
    index[[0, 7, -1]] = g - 1, 2 ** 27 - 3, 0
    X, beta = rng.normal(size=(n, 3)), rng.normal(size=(s, 3))
    base = host(eng.glm(cuda(X), cuda(beta), "linpred"))
    got = host(eng.glm(cuda(X), cuda(beta), "linpred", groups=[(cuda(index), u, None)]))
    picked = host(w[torch.as_tensor(index[:, None] + np.arange(s)[None, :], device="cuda")])
    assert np.array_equal(got, base + picked)


# ---------------------------------------------------------------------------------------------------------------- 2. the densities
def density_case(rng, family, n=45, s=130):
    """eta of both signs up to |eta| = 40 with the terms in it, y = 0 among the outcomes."""
    X = np.column_stack([np.ones(n), np.linspace(-38.0, 38.0, n), rng.normal(size=n)])
    beta = np.column_stack([0.01 * rng.normal(size=s), np.linspace(-1.0, 1.0, s), 0.01 * rng.normal(size=s)])
    beta[0], beta[-1] = (0.0, -1.0, 0.0), (0.0, 1.0, 0.0)
    terms, _ = glmm_ref.make_terms(rng, n, s, (6, 4), (False, True))
    terms[0][1][0, terms[0][0][0]], terms[0][1][-1, terms[0][0][0]] = 2.0, -2.0  # (row 0 has x = -38: eta = 38 + 2 and -38 - 2 there)
    terms[1][2][0] = 0.0
    m = dict(X=X, beta=beta, family=family, sigma=None, trials=None, offset=0.01 * rng.normal(size=n), terms=terms)
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
        terms_route(eng.last_kernels(), 2)
        eta = host(pl.glm_log_lik(*a, **k, linpred=True))
        assert np.abs(eta).max() >= 39.0 and eta.min() < -39.0
        want = glm_ref.density(fam, eta, m["y"], sigma=m["sigma"], trials=m["trials"], oc=v["obs_const"], dc=v["draw_const"])
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(want))
        dev = np.abs(ll - want) / np.maximum(1.0, np.abs(want))
        print(f"{family} ({where}): largest |ll - restatement| / max(1, |ll|) = {dev.max():.3e}")
        assert np.all(dev <= 1e-10), dev.max()


# -------------------------------------------------------------------------------------------------------------- 3. the order rule
@pytest.fixture(scope="module")
def bit_models():
    rng = np.random.default_rng(31)
    out = {}
    for f in FAMILIES:
        m = glmm_ref.make_model(rng, 53, 301, 7 if f != "poisson" else 70, f, sizes=(9, 9, 4), slopes=(False, True, True))
        m["terms"][1] = (m["terms"][0][0], *m["terms"][1][1:])  # two terms share one index vector
        out[f] = m
    return out


def take_rows(m, sel):
    pick = lambda v: None if v is None else v[sel]  # noqa: E731
    terms = [(i[sel], u, pick(z)) for i, u, z in map(glmm_ref.split, m["terms"])]
    return dict(m, X=m["X"][sel], y=m["y"][sel], offset=pick(m["offset"]), trials=pick(m["trials"]), terms=terms)


@pytest.mark.parametrize("family", FAMILIES)
def test_bits_do_not_depend_on_rows_draws_labels_layouts_lists_or_memory_space(eng, bit_models, family):
    import torch

    import pyloo_amd as pl

    m = bit_models[family]
    n, s = 53, 301
    a, k = front(m, "device")
    base = host(pl.glm_log_lik(*a, **k))
    assert base.shape == (n, s)
    rng = np.random.default_rng(32)
    # permuted rows, g and z along
    perm = rng.permutation(n)
    a2, k2 = front(take_rows(m, perm), "device")
    assert np.array_equal(host(pl.glm_log_lik(*a2, **k2)), base[perm])
    # permuted draws: beta, sigma and every u_t
    dperm = rng.permutation(s)
    md = dict(m, beta=m["beta"][dperm], sigma=None if m["sigma"] is None else m["sigma"][dperm],
              terms=[(i, u[dperm], z) for i, u, z in map(glmm_ref.split, m["terms"])])
    a3, k3 = front(md, "device")
    assert np.array_equal(host(pl.glm_log_lik(*a3, **k3)), base[:, dperm])
    # relabelled groups: new label lab[j] for group j, the columns of u permuted along
    relabelled = []
    for i, u, z in map(glmm_ref.split, m["terms"]):
        lab = rng.permutation(u.shape[1])
        u2 = np.empty_like(u)
        u2[:, lab] = u
        relabelled.append((lab[i], u2, z))
    a4, k4 = front(dict(m, terms=relabelled), "device")
    assert np.array_equal(host(pl.glm_log_lik(*a4, **k4)), base)
    # .T views and padded pitches of u_t
    views = []
    for i, u, z in map(glmm_ref.split, m["terms"]):
        g = u.shape[1]
        ut = cuda(np.ascontiguousarray(u.T)).T
        up = torch.zeros(s, 2 * g + 3, dtype=torch.float64, device="cuda")[:, 1:2 * g:2].copy_(cuda(u))
        assert ut.stride() == (1, s) and up.stride() == (2 * g + 3, 2)
        views.append(((cuda(i), ut, cuda(z)), (cuda(i), up, cuda(z))))
    for pick in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):
        kk = dict(k, groups=[views[t][c] for t, c in enumerate(pick)])
        assert np.array_equal(host(pl.glm_log_lik(*a, **kk)), base)
    # a row list that is unsorted and has repeats; one row, one draw
    rows = [52, 0, 17, 17, 3, 52, 16, 31]
    assert np.array_equal(host(pl.glm_log_lik(*a, **k, rows=rows)), base[rows])
    assert np.array_equal(host(pl.glm_log_lik(*a, **k, rows=torch.as_tensor(rows).cuda())), base[rows])
    a5, k5 = front(take_rows(m, slice(40, 41)), "device")
    assert np.array_equal(host(pl.glm_log_lik(*a5, **k5)), base[40:41])
    few = dict(m, beta=m["beta"][299:300], sigma=None if m["sigma"] is None else m["sigma"][299:300],
               terms=[(i, u[299:300], z) for i, u, z in map(glmm_ref.split, m["terms"])])
    a6, k6 = front(few, "device")
    assert np.array_equal(host(pl.glm_log_lik(*a6, **k6)), base[:, 299:300])
    # host against device input given the same vectors, a host .T view of u included
    fam, v = engine_vectors(m)
    dev = host(eng.glm(cuda(m["X"]), cuda(m["beta"]), fam, groups=put_terms(m["terms"], cuda), **{key: cuda(x) for key, x in v.items()}))
    assert np.array_equal(eng.glm(m["X"], m["beta"], fam, groups=m["terms"], **v), dev)
    turned = [(i, np.ascontiguousarray(u.T).T, z) for i, u, z in map(glmm_ref.split, m["terms"])]
    assert np.array_equal(eng.glm(m["X"], m["beta"], fam, groups=turned, **v), dev)
    assert np.array_equal(eng.glm(m["X"], m["beta"], fam, groups=m["terms"], rows=rows, **v), dev[rows])
    ah, kh = front(m, "host")
    assert np.array_equal(pl.glm_log_lik(*ah, **kh), dev)  # (the host front hands over exactly these vectors)
    assert np.all(np.abs(base - dev) <= 1e-10 * np.maximum(1.0, np.abs(dev)))  # (the device front computes its constants with torch)
    # a device index out of range is clamped into [0, G) on load
    i0, u0, _ = glmm_ref.split(m["terms"][0])
    wild = i0.copy()
    wild[[2, 30]] = -5, 1000
    clamped = np.clip(wild, 0, u0.shape[1] - 1)
    one = lambda idx: host(eng.glm(cuda(m["X"]), cuda(m["beta"]), "linpred", groups=[(cuda(idx), cuda(u0), None)]))  # noqa: E731
    assert np.array_equal(one(wild), one(clamped))


# ------------------------------------------------------------------------------------------------------------------- 4. no terms
@pytest.mark.parametrize("where", ["host", "device"])
def test_no_terms_through_the_new_entry_are_pla_glms_bits(eng, where):
    m = glm_ref.make_model(np.random.default_rng(33), 53, 301, 7, "binomial", with_offset=True)
    fam, v = engine_vectors(m)
    put = cuda if where == "device" else (lambda x: x)
    vv = {key: put(x) for key, x in v.items()}
    plain = host(eng.glm(put(m["X"]), put(m["beta"]), fam, **vv))
    none = host(eng.glm(put(m["X"]), put(m["beta"]), fam, groups=[], **vv))
    assert "glm_prepare_kernel -> glm_kernel<" in eng.last_kernels()
    assert np.array_equal(plain, none)
    kw = dict(mode="loo", tail_count=orc.tail_count(301, 1.0), good_k=0.7)
    r0 = eng.glm(put(m["X"]), put(m["beta"]), fam, **kw, **vv)
    r1 = eng.glm(put(m["X"]), put(m["beta"]), fam, groups=[], **kw, **vv)
    for key in ("diag", "loo_i", "lppd_i", "agg"):
        assert np.array_equal(host(r0[key]), host(r1[key])), key
    assert int(r0["n_replaced"]) == int(r1["n_replaced"]) == 0


# ------------------------------------------------------------------------------------------------------------- 5. the fused pass
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("method", ["psis", "sis", "tis"])
@pytest.mark.parametrize("n,s,p", [(53, 301, 7), (40, 1000, 20), (6, 4100, 3)])
def test_fused_pass_equals_loo_from_matrix_on_the_generated_matrix(eng, n, s, p, method, where):
    import pyloo_amd as pl

    m = glmm_ref.make_model(np.random.default_rng(n + s), n, s, p, "binomial", sizes=(5, 3), slopes=(False, True))
    a, k = front(m, where)
    fused, _ = quiet(pl.loo_glm_from_design, *a, **k, method=method, pointwise=True, reff=0.9)
    text = eng.last_kernels()
    terms_route(text, 2)
    assert text.endswith(" per block of observations")
    fused_text = text.split(" -> ", 3)[3][: -len(" per block of observations")]
    ll = pl.glm_log_lik(*a, **k)
    plain, _ = quiet(pl.loo_from_matrix, cuda(host(ll)), method=method, pointwise=True, reff=0.9)
    plain_text = eng.last_kernels()
    diag = "pareto_k" if method == "psis" else "ess"
    assert list(fused.index) == list(plain.index)
    assert fused_text == plain_text, (fused_text, plain_text)
    for key in ("loo_i", diag):
        assert np.array_equal(host(fused[key]), host(plain[key])), (key, fused_text)
    for key in ("elpd_loo", "se", "p_loo", "p_loo_se", "looic", "looic_se"):
        np.testing.assert_allclose(fused[key], plain[key], rtol=1e-12, err_msg=key)
    assert fused["warning"] == plain["warning"] and fused["n_data_points"] == n


# ------------------------------------------------------------------------------------------------ 6. end to end against the oracle
# Seeds of glmm_ref.make_model for which the reference's own k of every row is finite (run through the oracle on the CPU for seeds
# 0, 1, 2, ...: the first that qualifies is kept, so no row is left out of the comparison)
ORACLE_SEEDS = {(37, 1000, 5, "gaussian"): 0, (37, 1000, 5, "binomial"): 0, (37, 1000, 5, "poisson"): 0,
                (5, 4100, 5, "gaussian"): 0, (5, 4100, 5, "binomial"): 0, (5, 4100, 5, "poisson"): 0}
ORACLE = {}


def oracle_case(n, s, p, family):
    key = (n, s, p, family)
    if key not in ORACLE:
        m = glmm_ref.make_model(np.random.default_rng(ORACLE_SEEDS[key]), n, s, p, family)
        ORACLE[key] = (m, orc.loo_pointwise(glmm_ref.matrix_of(m), 1.0, "psis"))
    return ORACLE[key]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,s,p", [(37, 1000, 5), (5, 4100, 5)])
def test_end_to_end_against_the_oracle(eng, n, s, p, family, where):
    import pyloo_amd as pl

    m, ref = oracle_case(n, s, p, family)
    assert np.all(np.isfinite(ref["diag"])) and np.all(np.isfinite(ref["loo_i"]))
    a, k = front(m, where)
    res, msgs = quiet(pl.loo_glm_from_design, *a, **k, pointwise=True)
    assert not [t for t in msgs if "Pareto" not in t], msgs
    terms_route(eng.last_kernels(), 2)
    loo_i, khat = host(res["loo_i"]), host(res["pareto_k"])
    print(f"{family} {n} x {s} x {p} ({where}): loo_i {np.abs(loo_i - ref['loo_i']).max():.2e}, k {np.abs(khat - ref['diag']).max():.2e}")
    np.testing.assert_allclose(loo_i, ref["loo_i"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(khat, ref["diag"], rtol=0, atol=1e-9)
    fam, v = engine_vectors(m)
    put = cuda if where == "device" else (lambda x: x)
    raw = eng.glm(put(m["X"]), put(m["beta"]), fam, mode="loo", tail_count=orc.tail_count(s, 1.0), good_k=0.7, groups=put_terms(m["terms"], put),
                  **{key: put(x) for key, x in v.items()})
    np.testing.assert_allclose(host(raw["lppd_i"]), ref["lppd_i"], rtol=0, atol=1e-9)
    assert int(raw["n_replaced"]) == 0 and res["n_data_points"] == n and res["n_samples"] == s
    np.testing.assert_allclose(res["elpd_loo"], ref["loo_i"].sum(), rtol=1e-12, atol=1e-9)


# ----------------------------------------------------------------------------------------------------------------------- 7. blocks
CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import glm_ref, glmm_ref
from pyloo_amd.engine import get_engine
eng = get_engine(0)
out, texts = [], []
rows = np.random.default_rng(3).integers(0, 3000, size=2500)
for family in ("gaussian", "binomial", "poisson"):
    m = glmm_ref.make_model(np.random.default_rng(41), 3000, 1000, 8, family, sizes=(40, 3000), slopes=(True, False))
    fam = glm_ref.ENGINE_FAMILY[family]
    oc = None if family == "gaussian" else glm_ref.obs_const(fam, m["y"], m["trials"])
    dc = None if m["sigma"] is None else glm_ref.draw_const(m["sigma"])
    index, draws, z = m["terms"][0]
    z = z.copy()
    z[[7, 2990]] = np.nan
    terms = [(index, draws, z), m["terms"][1]]
    v = dict(y=m["y"], offset=m["offset"], trials=m["trials"], obs_const=oc, draw_scale=m["sigma"], draw_const=dc)
    cu = lambda a: None if a is None else torch.as_tensor(a).cuda()
    for where in ("device", "host"):
        put = cu if where == "device" else (lambda a: a)
        vv = {k: put(a) for k, a in v.items()}
        gg = [tuple(put(x) for x in glmm_ref.split(t)) for t in terms]
        for idx in (None, rows):
            r = eng.glm(put(m["X"]), put(m["beta"]), fam, rows=idx, mode="loo", tail_count=95, good_k=0.7, groups=gg, **vv)
            texts.append(eng.last_kernels())
            out += [np.asarray(r[k].cpu().numpy() if hasattr(r[k], "cpu") else r[k]).reshape(-1) for k in ("diag", "loo_i", "lppd_i", "agg", "n_replaced")]
        ll = eng.glm(put(m["X"]), put(m["beta"]), fam, rows=rows[:40], groups=gg, **vv)
        out.append(np.asarray(ll.cpu().numpy() if hasattr(ll, "cpu") else ll))
np.savez(sys.argv[2], *out)
open(sys.argv[2] + ".txt", "w").write("\n".join(texts))
"""


def test_block_size_independence(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 cuts the 3000 x 1000 pass into 23 blocks of 131 observations, the 2500 listed rows likewise; the image of
    the group effects is written once per call and every block reads it: every pointwise output, the NaN count (two rows whose z is
    NaN) and the matrix entries are the default's (one block) bit for bit, host and device; the aggregates to 1e-12."""
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
    assert all(t.endswith("per block of observations") and "glm_terms_kernel<" in t for t in texts[1])
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


# ------------------------------------------------------------------------------------------------------------ 8. non-finite values
@pytest.mark.parametrize("family", FAMILIES)
def test_values_that_are_not_finite_in_u_and_z(eng, family, monkeypatch):
    """inf and NaN in u and z, handed to the engine directly (the fronts reject them): NaN and inf where the restatement has them
    -- inf times a zero z included --; the LOO route replaces and counts every NaN; the front warns with loo_from_matrix's text."""
    import pyloo_amd as pl

    rng = np.random.default_rng(8)
    m = glmm_ref.make_model(rng, 40, 500, 6, family, sizes=(6, 4), slopes=(False, True))
    fam, v = engine_vectors(m)
    (i0, u0, _), (i1, u1, z1) = map(glmm_ref.split, m["terms"])
    i0, u0, u1, z1 = i0.copy(), u0.copy(), u1.copy(), z1.copy()
    i0[2], i0[38] = 0, 1
    u0[3, i0[2]], u0[:, i0[38]] = np.inf, np.nan
    u1[7, i1[5]], u1[9, i1[5]] = -np.inf, np.nan
    z1[11], z1[12], z1[5] = np.inf, np.nan, 0.0  # (row 5: zero times -inf)
    terms = [(i0, u0), (i1, u1, z1)]
    for put in (cuda, lambda a: a):
        gg = put_terms(terms, put)
        vv = {k: put(a) for k, a in v.items()}
        base = host(eng.glm(put(m["X"]), put(m["beta"]), "linpred", offset=put(m["offset"])))
        eta = host(eng.glm(put(m["X"]), put(m["beta"]), "linpred", offset=put(m["offset"]), groups=gg))
        want_eta = glmm_ref.add_terms(base, terms)
        assert np.array_equal(eta, want_eta, equal_nan=True) and np.isnan(eta[5, 7]) and np.isinf(eta[2, 3]) and np.isnan(eta[38]).all()
        ll = host(eng.glm(put(m["X"]), put(m["beta"]), fam, groups=gg, **vv))
        want = glm_ref.density(fam, eta, m["y"], sigma=m["sigma"], trials=m["trials"], oc=v["obs_const"], dc=v["draw_const"])
        assert np.array_equal(np.isnan(ll), np.isnan(want)) and np.array_equal(np.isposinf(ll), np.isposinf(want))
        assert np.array_equal(np.isneginf(ll), np.isneginf(want))
        ok = np.isfinite(want)
        assert np.all(np.abs(ll[ok] - want[ok]) <= 1e-10 * np.maximum(1.0, np.abs(want[ok])))
        r = eng.glm(put(m["X"]), put(m["beta"]), fam, mode="loo", tail_count=orc.tail_count(500, 1.0), good_k=0.7, groups=gg, **vv)
        assert int(r["n_replaced"]) == int(np.isnan(want).sum()) >= 2 * 500
        clean = ~np.isnan(want).any(axis=1) & np.isfinite(want).all(axis=1)
        ref = orc.loo_pointwise(np.where(np.isnan(want), -1e10, want)[clean], 1.0, "psis")
        np.testing.assert_allclose(host(r["loo_i"])[clean], ref["loo_i"], rtol=0, atol=1e-9)
    # the front's warning: the NaN injected behind its checks
    real = eng.glm

    def with_nan(X, beta, family, **kw):
        kw["groups"] = terms
        return real(X, beta, family, **kw)

    monkeypatch.setattr(eng, "glm", with_nan)
    a, k = front(m, "host")
    res, msgs = quiet(pl.loo_glm_from_design, *a, **k)
    assert msgs.count(NAN_TEXT) == 1 and res["n_data_points"] == 40


# --------------------------------------------------------------------------------------------------------------- 9. subsampled LOO
@pytest.mark.parametrize("estimator", ["diff_srs", "hh_pps", "srs"])
def test_loo_subsample_glm_with_groups_on_the_device(eng, estimator):
    import pyloo_amd as pl

    m = glmm_ref.make_model(np.random.default_rng(61), 400, 500, 6, "gaussian", sizes=(20, 5), slopes=(False, True))
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
    # "plpd": the log-likelihood at the posterior means of beta, sigma and every u_t
    plpd = host(pl.glm_plpd(*a, **k))
    mean_terms = [(i, u.mean(0).reshape(1, -1), z) for i, u, z in map(glmm_ref.split, m["terms"])]
    want_plpd = glmm_ref.log_lik(m["X"], m["y"], m["beta"].mean(0).reshape(1, -1), "gaussian", m["sigma"].mean().reshape(1), m["offset"],
                                 None, mean_terms)[:, 0]
    np.testing.assert_allclose(plpd, want_plpd, rtol=0, atol=1e-10)
    np.random.seed(12)
    (p_got, p_idx, _), msgs = quiet(pl.loo_subsample_glm, *a, **k, observations=50, loo_approximation="plpd", estimator=estimator)
    assert not any("PLPD" in t or "approximate" in t for t in msgs), msgs
    assert p_got["subsample_size"] == len(p_idx.idx) and np.isfinite(p_got["elpd_loo"])
