"""The negative-binomial, gamma and probit densities of the GLM log-likelihood generator (``pla_glm`` family codes 4, 5, 6;
csrc/pla_glm.h, instantiated in pla_k_glm_families.hip and pla_k_glm_terms_families.hip) and their fronts on the GPU.

Bounds, each derived or the project's own:
  1. accuracy      |ll - mpmath(kernel's own eta, the handed constants)| <= 4 R u T on the grid of tests/glm_families_ref.py, with T
                   the sum of the magnitudes of the formula's terms, u = 2^-53 and R the NumPy restatement's own worst value of that
                   measure on the same grid (RESTATEMENT_FIGURE; tests/test_glm_families_host.py measures it)
  2. shapes        |ll - restatement(kernel's own eta)| <= 4 R u T for every shape, chunk count and the panel route
  3. same bits     every entry of ll under permuted rows and draws, row lists, layouts, memory spaces, block sizes, an empty list of terms
  4. end to end    the fused pass equals loo_from_matrix on the generated matrix bit for bit; loo_i and k within 1e-9 of the oracle on
                   the restatement's matrix (the bound of tests/test_gpu_loo_glm.py)
Largest deviations are printed (pytest -s).  Every test fails without the feature: the engine does not know the families."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import glm_families_ref as fref
import glm_ref
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."
FAMILIES = fref.ENGINE_FAMILIES


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
    """What the fronts hand to ``Engine.glm`` for a model of glm_families_ref.make_model (the host front's constants)."""
    fam = m["family"]
    dc = None if m["scale"] is None else fref.draw_const(m["scale"])
    return dict(y=m["y"], offset=m["offset"], trials=m["trials"], obs_const=fref.obs_const(fam, m["y"], m["trials"]), draw_scale=m["scale"],
                draw_const=dc)


def front(m, where="host", **more):
    (X, y, beta, family), kw = fref.front_call(m, **more)
    put = cuda if where == "device" else (lambda a: a)
    return (put(X), put(y), put(beta), family), {k: (put(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def within_bound(family, ll, want, T, factor=fref.GPU_FACTOR):
    m = fref.measure(ll, want, T)
    return float(m.max()), bool(np.all(m <= factor * fref.RESTATEMENT_FIGURE[family]))


# -------------------------------------------------------------------------------------------------------------------- 1. accuracy
@pytest.mark.parametrize("grid", FAMILIES + ("bernoulli_probit",))
def test_density_accuracy_against_mpmath_on_the_kernels_own_eta(eng, grid):
    g = fref.accuracy_grid(grid)
    fam = g["family"]
    v = dict(y=g["y"], trials=g["trials"], obs_const=g["oc"], draw_scale=g["scale"], draw_const=g["dc"])
    dv = {k: cuda(a) for k, a in v.items()}
    eta = host(eng.glm(cuda(g["X"]), cuda(g["beta"]), "linpred"))
    ll = host(eng.glm(cuda(g["X"]), cuda(g["beta"]), fam, **dv))
    text = eng.last_kernels()
    assert "glm_kernel<" + {"negbinomial": "negative binomial log", "gamma": "gamma log", "binomial_probit": "binomial probit"}[fam] in text, text
    assert np.abs(eta).max() >= 37.5 and (eta == 0.0).any() and (eta == 37.5).any() and (eta == -37.5).any()
    ref, T = fref.grid_reference(grid, eta)
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(ref))
    worst, ok = within_bound(fam, ll, ref, T)
    print(f"{grid}: largest |ll - mpmath| / (u T) = {worst:.2f} (restatement {fref.RESTATEMENT_FIGURE[fam]}, allowed "
          f"{fref.GPU_FACTOR * fref.RESTATEMENT_FIGURE[fam]})")
    assert ok, worst
    if fam == "binomial_probit":  # both tails at |eta| = 37.5 with y = 0 and y = trials: the finite values the reference has
        for e in (37.5, -37.5):
            j = int(np.where(eta[0] == e)[0][0])
            for i in (0, len(g["y"]) - 1):
                assert np.isfinite(ll[i, j]) and abs(ll[i, j] - ref[i, j]) <= 4.0 * fref.RESTATEMENT_FIGURE[fam] * fref.U * T[i, j] + 1e-300
    # host input given the same vectors: the same bits
    assert np.array_equal(eng.glm(g["X"], g["beta"], fam, **v), ll)


# ---------------------------------------------------------------------------------------------------------------------- 2. shapes
SHAPE_N, SHAPE_S = (1, 15, 16, 17, 33), (1, 2, 15, 16, 17, 250)


def compare_with_restatement(fam, ll, eta, m, v, rows=slice(None), draws=slice(None)):
    pick_o = lambda a: None if a is None else a[rows]  # noqa: E731
    pick_d = lambda a: None if a is None else a[draws]  # noqa: E731
    args = (fam, eta, m["y"][rows], pick_d(m["scale"]), pick_o(m["trials"]), pick_o(v["obs_const"]), pick_d(v["draw_const"]))
    want = fref.density(*args)
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(want))
    return within_bound(fam, ll, want, fref.magnitude(*args))


@pytest.mark.parametrize("family", FAMILIES)
def test_every_shape_equals_the_restatement_on_the_kernels_own_eta(eng, family):
    m = fref.make_model(np.random.default_rng(71), 33, 250, 5, family, with_offset=True)
    v = engine_vectors(m)
    Xd, bd = cuda(m["X"]), cuda(m["beta"])
    dv = {k: cuda(a) for k, a in v.items()}
    eta = host(eng.glm(Xd, bd, "linpred", offset=dv["offset"]))
    full = host(eng.glm(Xd, bd, family, **dv))
    worst, ok = compare_with_restatement(family, full, eta, m, v)
    assert ok, worst
    for n in SHAPE_N:
        for s in SHAPE_S:
            obs = {k: (None if a is None else a[:n]) for k, a in dv.items() if k in ("y", "offset", "trials", "obs_const")}
            drw = {k: (None if a is None else a[:s]) for k, a in dv.items() if k in ("draw_scale", "draw_const")}
            ll = host(eng.glm(Xd[:n], bd[:s], family, **obs, **drw))
            assert ll.shape == (n, s) and np.array_equal(ll, full[:n, :s]), (n, s)  # an entry does not depend on the shape of its call
    print(f"{family}: largest |ll - restatement| / (u T) = {worst:.2f}")


@pytest.mark.parametrize("p", (1, 16, 17, 64, 65, 130))
@pytest.mark.parametrize("family", FAMILIES)
def test_every_chunk_count_and_the_panel_route(eng, family, p):
    m = fref.make_model(np.random.default_rng(72 + p), 17, 33, p, family, with_offset=True)
    v = engine_vectors(m)
    dv = {k: cuda(a) for k, a in v.items()}
    eta = host(eng.glm(cuda(m["X"]), cuda(m["beta"]), "linpred", offset=dv["offset"]))
    ll = host(eng.glm(cuda(m["X"]), cuda(m["beta"]), family, **dv))
    text = eng.last_kernels()
    chunks = 1 if p <= 16 else 2 if p <= 32 else 4 if p <= 64 else 8
    assert f"{chunks} chunks of 16 predictors" in text and ("per panel" in text) == (p > 128), text
    worst, ok = compare_with_restatement(family, ll, eta, m, v)
    assert ok, (p, worst)


# ------------------------------------------------------------------------------------------------------------------- 3. same bits
@pytest.mark.parametrize("family", FAMILIES)
def test_ll_bits_do_not_depend_on_rows_draws_lists_layouts_or_memory_space(eng, family):
    import pyloo_amd as pl

    m = fref.make_model(np.random.default_rng(73), 53, 301, 7, family, with_offset=True)
    n, s = 53, 301
    a, k = front(m, "device")
    base = host(pl.glm_log_lik(*a, **k))
    assert base.shape == (n, s) and np.all(np.isfinite(base))
    rng = np.random.default_rng(74)
    perm, dperm = rng.permutation(n), rng.permutation(s)
    mp = dict(m, X=m["X"][perm], y=m["y"][perm], offset=m["offset"][perm], trials=None if m["trials"] is None else m["trials"][perm])
    a2, k2 = front(mp, "device")
    assert np.array_equal(host(pl.glm_log_lik(*a2, **k2)), base[perm])
    md = dict(m, beta=m["beta"][dperm], scale=None if m["scale"] is None else m["scale"][dperm])
    a3, k3 = front(md, "device")
    assert np.array_equal(host(pl.glm_log_lik(*a3, **k3)), base[:, dperm])
    rows = [52, 0, 17, 17, 3, 52, 16, 31]  # unsorted, with repeats
    assert np.array_equal(host(pl.glm_log_lik(*a, **k, rows=rows)), base[rows])
    Xt, bt = cuda(np.ascontiguousarray(m["X"].T)).T, cuda(np.ascontiguousarray(m["beta"].T)).T
    assert Xt.stride() == (1, n) and bt.stride() == (1, s)
    assert np.array_equal(host(pl.glm_log_lik(Xt, a[1], bt, a[3], **k)), base)
    assert np.array_equal(host(pl.glm_log_lik(Xt, a[1], bt, a[3], **k, rows=rows)), base[rows])
    # host against device input given the same constant vectors (the fronts compute them with scipy on the host, with torch on the
    # device, and those may differ in the last bit)
    v = engine_vectors(m)
    dev = host(eng.glm(cuda(m["X"]), cuda(m["beta"]), family, **{key: cuda(x) for key, x in v.items()}))
    assert np.array_equal(eng.glm(m["X"], m["beta"], family, **v), dev)
    assert np.array_equal(eng.glm(m["X"], m["beta"], family, rows=rows, **v), dev[rows])
    ah, kh = front(m, "host")
    assert np.array_equal(pl.glm_log_lik(*ah, **kh), dev)  # (the host front hands over exactly these vectors)
    T = fref.magnitude(family, host(pl.glm_log_lik(*ah, **kh, linpred=True)), m["y"], m["scale"], m["trials"], v["obs_const"], v["draw_const"])
    assert np.all(np.abs(base - dev) <= 1e-10 * np.maximum(1.0, T))  # (the device front's constants: the project's aim for pointwise outputs)


# ------------------------------------------------------------------------------------------------------------ 4. group-level terms
@pytest.mark.parametrize("family", FAMILIES)
def test_group_level_terms(eng, family):
    import pyloo_amd as pl

    rng = np.random.default_rng(75)
    n, s = 37, 130
    m = fref.make_model(rng, n, s, 5, family, with_offset=True)
    groups = [(rng.integers(0, 6, size=n), 0.3 * rng.normal(size=(s, 6))), (rng.integers(0, 4, size=n), 0.2 * rng.normal(size=(s, 4)), rng.normal(size=n))]
    v = engine_vectors(m)
    for where in ("device", "host"):
        put = cuda if where == "device" else (lambda x: x)
        a, k = front(m, where)
        gr = [tuple(put(np.asarray(x)) for x in term) for term in groups]
        eta = host(pl.glm_log_lik(*a, **k, linpred=True, groups=gr))
        ll = host(pl.glm_log_lik(*a, **k, groups=gr))
        assert "glm_terms_kernel<" in eng.last_kernels() and "2 group-level terms" in eng.last_kernels(), eng.last_kernels()
        plain_eta = host(pl.glm_log_lik(*a, **k, linpred=True))
        assert np.abs(eta - plain_eta).max() > 0.01  # (the terms are in)
        if where == "host":  # (the host front hands over the restatement's constants)
            worst, ok = compare_with_restatement(family, ll, eta, m, v)
            print(f"{family}: terms, largest |ll - restatement| / (u T) = {worst:.2f}")
            assert ok, worst
        assert np.array_equal(host(pl.glm_log_lik(*a, **k, groups=[])), host(pl.glm_log_lik(*a, **k)))


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
ORACLE = {}


def oracle_case(n, s, p, family):
    key = (n, s, p, family)
    if key not in ORACLE:
        m = fref.make_model(np.random.default_rng(n * 7 + p), n, s, p, family, with_offset=True)
        ORACLE[key] = (m, orc.loo_pointwise(fref.matrix_of(m), 1.0, "psis"))
    return ORACLE[key]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,s,p", [(37, 1000, 5), (5, 4100, 5)])
def test_end_to_end_against_the_oracle_and_loo_from_matrix(eng, n, s, p, family):
    import pyloo_amd as pl

    m, ref = oracle_case(n, s, p, family)
    for where in ("host", "device"):
        a, k = front(m, where)
        res, msgs = quiet(pl.loo_glm_from_design, *a, **k, pointwise=True)
        text = eng.last_kernels()
        assert text.startswith("glm_prepare_kernel -> glm_kernel<") and text.endswith("per block of observations"), text
        loo_i, khat = host(res["loo_i"]), host(res["pareto_k"])
        print(f"{family} {n} x {s} x {p} ({where}): loo_i {np.abs(loo_i - ref['loo_i']).max():.2e}, k {np.abs(khat - ref['diag']).max():.2e}")
        np.testing.assert_allclose(loo_i, ref["loo_i"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(khat, ref["diag"], rtol=0, atol=1e-9)
        assert res["n_data_points"] == n and res["n_samples"] == s and not any(NAN_TEXT in t for t in msgs)
        if where == "host":
            continue
        # like with like: the block the fused pass consumes is device-resident, so is the yardstick's matrix
        plain, plain_msgs = quiet(pl.loo_from_matrix, pl.glm_log_lik(*a, **k), pointwise=True)
        assert msgs == plain_msgs and list(res.index) == list(plain.index)
        for key in ("loo_i", "pareto_k"):
            assert np.array_equal(host(res[key]), host(plain[key])), key
        for key in ("elpd_loo", "se", "p_loo", "p_loo_se", "looic", "looic_se"):
            assert res[key] == plain[key], key
        assert res["warning"] == plain["warning"]


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import glm_families_ref as fref
from pyloo_amd.engine import get_engine
eng = get_engine(0)
out, texts = [], []
cu = lambda a: None if a is None else torch.as_tensor(a).cuda()
for family in fref.ENGINE_FAMILIES:
    m = fref.make_model(np.random.default_rng(41), 700, 500, 5, family, with_offset=True)
    v = dict(y=m["y"], offset=m["offset"], trials=m["trials"], obs_const=fref.obs_const(family, m["y"], m["trials"]), draw_scale=m["scale"],
             draw_const=None if m["scale"] is None else fref.draw_const(m["scale"]))
    r = eng.glm(cu(m["X"]), cu(m["beta"]), family, mode="loo", tail_count=67, good_k=0.7, **{k: cu(a) for k, a in v.items()})
    texts.append(eng.last_kernels())
    out += [r[k].cpu().numpy().reshape(-1) if hasattr(r[k], "cpu") else np.asarray(r[k]).reshape(-1) for k in ("diag", "loo_i", "lppd_i", "n_replaced")]
np.savez(sys.argv[2], *out)
open(sys.argv[2] + ".txt", "w").write("\n".join(texts))
"""


def test_block_size_independence(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 cuts the 700 x 500 pass into blocks of 262 observations, the last one ragged: every pointwise output
    of the three families is the default's (one block) bit for bit.  Each setting in a fresh process: the variable is read once."""
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
    assert len(outs[0]) == 3 * 4 and texts[0] == texts[1]
    assert all(t.endswith("per block of observations") and t.startswith("glm_prepare_kernel -> glm_kernel<") for t in texts[1])
    for j, (a, b) in enumerate(zip(*outs)):
        assert a.shape == b.shape and np.array_equal(a, b), j
        assert np.all(np.isfinite(a)) and (j % 4 != 3 or int(a[0]) == 0), j


@pytest.mark.parametrize("family", FAMILIES)
def test_nan_is_counted_replaced_and_warned_about(eng, monkeypatch, family):
    """A NaN offset on the device path, where the front cannot look (handed to the engine behind the front's checks)."""
    import pyloo_amd as pl

    m = fref.make_model(np.random.default_rng(51), 40, 500, 4, family, with_offset=True)
    off = m["offset"].copy()
    off[[3, 38]] = np.nan
    ll = fref.matrix_of(m)
    ll[[3, 38]] = -1e10
    ref = orc.loo_pointwise(ll, 1.0, "psis")
    real = eng.glm
    seen = []

    def with_nan(X, beta, fam, **kw):
        kw["offset"] = cuda(off)
        out = real(X, beta, fam, **kw)
        seen.append(int(out["n_replaced"]))
        return out

    monkeypatch.setattr(eng, "glm", with_nan)
    a, k = front(m, "device")
    res, msgs = quiet(pl.loo_glm_from_design, *a, **k, pointwise=True)
    assert msgs.count(NAN_TEXT) == 1 and seen == [2 * 500] and res["n_data_points"] == 40
    ok = np.ones(40, dtype=bool)
    ok[[3, 38]] = False
    np.testing.assert_allclose(host(res["loo_i"])[ok], ref["loo_i"][ok], rtol=0, atol=1e-9)
    np.testing.assert_allclose(host(res["loo_i"])[~ok], ref["loo_i"][~ok], rtol=1e-12)


# ------------------------------------------------------------------------------------------------- 6. the other fronts on the device
@pytest.mark.parametrize("family", FAMILIES)
def test_plpd_and_subsampled_loo_on_the_device(eng, family):
    import pyloo_amd as pl

    m = fref.make_model(np.random.default_rng(61), 300, 400, 4, family, with_offset=True)
    a, k = front(m, "device")
    plpd = host(pl.glm_plpd(*a, **k))
    mean = dict(m, beta=m["beta"].mean(0).reshape(1, -1), scale=None if m["scale"] is None else m["scale"].mean().reshape(1))
    np.testing.assert_allclose(plpd, fref.matrix_of(mean)[:, 0], rtol=0, atol=1e-10 * np.maximum(1.0, np.abs(fref.matrix_of(mean)[:, 0])).max())
    ll = pl.glm_log_lik(*a, **k)
    np.random.seed(11)
    (got, idx, est), msgs = quiet(pl.loo_subsample_glm, *a, **k, observations=40, loo_approximation="lpd", loo_approximation_draws=100,
                                  pointwise=True)
    np.random.seed(11)
    (want, widx, west), wmsgs = quiet(pl.loo_subsample_from_matrix, ll, observations=40, loo_approximation="lpd", loo_approximation_draws=100,
                                      pointwise=True)
    assert np.array_equal(idx.idx, widx.idx) and msgs == wmsgs
    for key in ("elpd_loo", "se", "p_loo", "subsampling_SE"):
        np.testing.assert_allclose(got[key], want[key], rtol=1e-9, err_msg=key)
