"""Host side of the group-level terms of the GLM fronts (``groups=`` / ``group_terms=`` of ``pyloo_amd/loo_glm.py``) without a GPU:
the fronts through an oracle-backed stand-in engine whose grouped call is the NumPy restatement (tests/glmm_ref.py) -- every
rejection before the first engine call, what is handed over, ``glm_plpd`` at the posterior means, ``ELPDData`` and warnings against
``loo_from_matrix`` on the restatement's matrix, calls without terms, the order of ``loo_glm``'s terms --, the C export
(``pla_glm_grouped``) and the generated code of the new kernels.

Without the feature every test fails at the unknown argument or the missing symbol."""

import ctypes as C
import importlib
import os
import re
import shutil
import sys
import warnings

import numpy as np
import pytest

import glm_ref
import glmm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOO calculation."
FAMILIES = ("gaussian", "bernoulli", "binomial", "poisson")
N, S, P = 14, 400, 5


@pytest.fixture()
def fake(monkeypatch):
    eng = glmm_ref.GroupedEngine()
    for name in ("pyloo_amd.loo", "pyloo_amd.loo_glm", "pyloo_amd.loo_subsample", "pyloo_amd.base"):
        monkeypatch.setattr(importlib.import_module(name), "get_engine", lambda device=None: eng)
    return eng


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


@pytest.fixture(scope="module")
def models():
    rng = np.random.default_rng(71)
    return {f: glmm_ref.make_model(rng, N, S, P, f, with_offset=f != "bernoulli") for f in FAMILIES}


def same_terms(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        (gi, gu, gz), (wi, wu, wz) = glmm_ref.split(g), glmm_ref.split(w)
        assert np.array_equal(gi, wi) and np.array_equal(gu, wu) and (gz is None) == (wz is None)
        assert wz is None or np.array_equal(gz, wz)


# ---------------------------------------------------------------------------------------------------------------------- the fronts
def test_every_rejection_comes_before_any_engine_call(fake, models):
    import pyloo_amd as pl

    m = models["poisson"]
    a, k = glmm_ref.front_args(m)
    (index, draws), (index1, draws1, z1) = m["terms"]
    bad_u = draws.copy()
    bad_u[3, 1] = np.inf
    bad_z = z1.copy()
    bad_z[2] = np.nan
    cases = [
        ([(index.astype(np.float64), draws)], TypeError, "index must hold integers"),
        ([(index % 2 == 0, draws)], TypeError, "index must hold integers"),
        ([(np.where(np.arange(N) == 4, -1, index), draws)], ValueError, "index must lie in [0, 5), got range [-1, 4]"),
        ([(np.where(np.arange(N) == 4, 5, index), draws)], ValueError, "index must lie in [0, 5), got range [0, 5]"),
        ([(index[:-1], draws)], ValueError, f"index needs {N} values"),
        ([(index1, draws1, z1[:-2])], ValueError, f"z needs {N} values"),
        ([(index, draws[:-1])], ValueError, f"draws must be a 2-D (n_draws, G) array with n_draws = {S}"),
        ([(index, draws.T)], ValueError, f"draws must be a 2-D (n_draws, G) array with n_draws = {S}"),
        ([(index, draws[:, 0])], ValueError, "draws must be a 2-D (n_draws, G) array"),
        ([(index, draws)] * 9, ValueError, "at most 8 group-level terms"),
        ([(index, draws[:, :0])], ValueError, "draws has no groups (G = 0)"),
        ([(index, bad_u)], ValueError, "groups[0]: draws holds values that are not finite"),
        ([(index, draws), (index1, draws1, bad_z)], ValueError, "groups[1]: z holds values that are not finite"),
        ([(index,)], ValueError, "groups[0] must be (index, draws) or (index, draws, z)"),
    ]
    for groups, kind, word in cases:
        kk = dict(k, groups=groups)
        for fn in (pl.loo_glm_from_design, pl.glm_log_lik, pl.glm_plpd, pl.loo_subsample_glm):
            with pytest.raises(kind) as err:
                fn(*a, **kk)
            assert word in str(err.value), (fn.__name__, word, str(err.value))
    assert fake.calls == []


def test_what_is_handed_to_the_engine_is_the_restatements(fake, models):
    import pyloo_amd as pl

    for f in FAMILIES:
        m = models[f]
        a, k = glmm_ref.front_args(m)
        fake.calls.clear()
        ll = pl.glm_log_lik(*a, **k)
        c = fake.calls[0]
        assert c["family"] == glm_ref.ENGINE_FAMILY[f] and c["mode"] == "matrix" and c["rows"] is None and c["has_groups"]
        same_terms(c["groups"], m["terms"])
        want_oc = None if f in ("gaussian", "bernoulli") else glm_ref.obs_const(glm_ref.ENGINE_FAMILY[f], m["y"], m["trials"])
        assert (c["obs_const"] is None) == (want_oc is None) and (want_oc is None or np.array_equal(c["obs_const"], want_oc)), f
        if f == "gaussian":
            assert np.array_equal(c["draw_const"], glm_ref.draw_const(m["sigma"])) and np.array_equal(c["draw_scale"], m["sigma"])
        else:
            assert c["draw_const"] is None and c["draw_scale"] is None
        assert np.array_equal(ll, glmm_ref.matrix_of(m)), f
        assert not np.array_equal(ll, glm_ref.matrix_of(m)), f  # (the terms matter)
        fake.calls.clear()
        eta = pl.glm_log_lik(*a, **k, linpred=True)
        assert fake.calls[0]["family"] == "linpred" and fake.calls[0]["y"] is None
        same_terms(fake.calls[0]["groups"], m["terms"])
        assert np.array_equal(eta, glmm_ref.linpred(m["X"], m["beta"], m["offset"], m["terms"]))
        rows = [9, 2, 2, 13, 0]
        assert np.array_equal(pl.glm_log_lik(*a, **k, rows=rows), glmm_ref.matrix_of(m)[rows])


def test_another_order_of_the_terms_is_another_order_of_additions(fake, models):
    """The documented caveat: the sum is taken in the order of the terms, so the reverse order may differ in the last bit and by
    no more -- two additions of numbers of size O(1): a few ulp."""
    import pyloo_amd as pl

    m = models["gaussian"]
    a, k = glmm_ref.front_args(m)
    eta = pl.glm_log_lik(*a, **k, linpred=True)
    back = pl.glm_log_lik(*a, **dict(k, groups=m["terms"][::-1]), linpred=True)
    assert np.array_equal(back, glmm_ref.linpred(m["X"], m["beta"], m["offset"], m["terms"][::-1]))
    assert np.all(np.abs(back - eta) <= 8 * 2.0 ** -52 * np.maximum(1.0, np.abs(eta)))


def test_plpd_is_the_log_likelihood_at_the_posterior_means(fake, models):
    import pyloo_amd as pl

    for f in FAMILIES:
        m = models[f]
        a, k = glmm_ref.front_args(m)
        fake.calls.clear()
        got, msgs = quiet(pl.glm_plpd, *a, **k)
        assert not msgs and len(fake.calls) == 1 and fake.calls[0]["n_draws"] == 1 and fake.calls[0]["mode"] == "matrix"
        sig = None if m["sigma"] is None else m["sigma"].mean().reshape(1)
        mean_terms = [(t[0], t[1].mean(0).reshape(1, -1), *t[2:]) for t in m["terms"]]
        same_terms(fake.calls[0]["groups"], mean_terms)
        want = glmm_ref.log_lik(m["X"], m["y"], m["beta"].mean(0).reshape(1, -1), f, sig, m["offset"], m["trials"], mean_terms)[:, 0]
        assert got.shape == (N,) and np.array_equal(got, want), f


@pytest.mark.parametrize("family", FAMILIES)
def test_elpd_data_equals_loo_from_matrix_on_the_restatements_matrix(fake, models, family):
    import pyloo_amd as pl

    m = models[family]
    a, k = glmm_ref.front_args(m)
    ll = glmm_ref.matrix_of(m)
    for kwargs in (dict(), dict(pointwise=True, reff=0.7), dict(method="sis", pointwise=True), dict(method="tis", scale="deviance")):
        fake.calls.clear()
        got, msgs = quiet(pl.loo_glm_from_design, *a, **k, **kwargs)
        want, want_msgs = quiet(pl.loo_from_matrix, ll, **kwargs)
        assert len(fake.calls) == 1 and fake.calls[0]["mode"] == "loo" and fake.calls[0]["has_groups"]
        assert list(got.index) == list(want.index) and msgs == want_msgs, (kwargs, msgs, want_msgs)
        assert got.method == want.method
        for key in want.index:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), (kwargs, key)


def test_high_k_and_nan_warnings_have_loo_from_matrix_texts(fake, models, monkeypatch):
    import pyloo_amd as pl

    m = dict(models["poisson"])
    m["y"] = m["y"].copy()
    m["y"][3] = 60.0  # an outlier: its Pareto k is high
    a, k = glmm_ref.front_args(m)
    got, msgs = quiet(pl.loo_glm_from_design, *a, **k, pointwise=True)
    want, want_msgs = quiet(pl.loo_from_matrix, glmm_ref.matrix_of(m), pointwise=True)
    assert any("Pareto" in t for t in msgs) and msgs == want_msgs and got["warning"] is True

    class NanEngine(glmm_ref.GroupedEngine):  # a NaN can only come out of the generator (the fronts reject what is not finite)
        def glm(self, *args, **kw):
            index, draws, _ = glmm_ref.split(kw["groups"][0])
            draws = draws.copy()
            draws[:, index[5]] = np.nan
            kw["groups"] = [(index, draws)] + list(kw["groups"][1:])
            return glmm_ref.GroupedEngine.glm(self, *args, **kw)

    eng = NanEngine()
    monkeypatch.setattr(importlib.import_module("pyloo_amd.loo_glm"), "get_engine", lambda device=None: eng)
    a, k = glmm_ref.front_args(models["poisson"])
    res, msgs = quiet(pl.loo_glm_from_design, *a, **k, pointwise=True)
    assert msgs.count(NAN_TEXT) == 1 and np.isfinite(res["elpd_loo"])


def test_no_terms_reach_the_existing_call_with_the_existing_arguments(fake, models):
    import pyloo_amd as pl

    m = models["binomial"]
    a, k = glmm_ref.front_args(m)
    plain = {key: v for key, v in k.items() if key != "groups"}
    for fn, extra in ((pl.glm_log_lik, {}), (pl.glm_log_lik, dict(linpred=True)), (pl.glm_plpd, {}), (pl.loo_glm_from_design, dict(pointwise=True)),
                      (pl.loo_subsample_glm, dict(observations=np.array([3, 5, 9]), loo_approximation="lpd"))):
        recorded = []
        for groups in ("absent", None, [], ()):
            fake.calls.clear()
            kk = dict(plain, **extra) if isinstance(groups, str) else dict(plain, groups=groups, **extra)
            quiet(fn, *a, **kk)
            assert fake.calls and not any(c["has_groups"] for c in fake.calls), (fn.__name__, groups)
            recorded.append(list(fake.calls))
        for other in recorded[1:]:
            assert len(other) == len(recorded[0])
            for c0, c1 in zip(recorded[0], other):
                assert set(c0) == set(c1)
                for key in c0:
                    both = (c0[key], c1[key])
                    same = all(v is None for v in both) or (not any(v is None for v in both) and np.array_equal(*both))
                    assert same, (fn.__name__, key)


def test_loo_glm_takes_the_terms_in_the_order_given(fake, models):
    import pyloo_amd as pl

    m = models["gaussian"]
    chains = 4
    beta, sigma = m["beta"], m["sigma"]
    (i0, u0), (i1, u1, z1) = m["terms"]
    post = {"beta": beta.reshape(chains, S // chains, P), "sigma": sigma.reshape(chains, S // chains),
            "school": u0.reshape(chains, S // chains, -1), "slope": u1.reshape(chains, S // chains, -1)}
    data = {"posterior": post}
    fake.calls.clear()
    got, _ = quiet(pl.loo_glm, data, m["X"], m["y"], "gaussian", ["beta"], sigma_name="sigma", offset=m["offset"], pointwise=True,
                   group_terms=[("school", i0), ("slope", i1, z1)])
    same_terms(fake.calls[0]["groups"], m["terms"])
    a, k = glmm_ref.front_args(m)
    want, _ = quiet(pl.loo_glm_from_design, *a, **k, pointwise=True)
    assert np.array_equal(got["loo_i"], want["loo_i"]) and got["elpd_loo"] == want["elpd_loo"]
    fake.calls.clear()
    quiet(pl.loo_glm, data, m["X"], m["y"], "gaussian", ["beta"], sigma_name="sigma", offset=m["offset"],
          group_terms=[("slope", i1, z1), ("school", i0)])
    same_terms(fake.calls[0]["groups"], m["terms"][::-1])
    fake.calls.clear()
    plain, _ = quiet(pl.loo_glm, data, m["X"], m["y"], "gaussian", ["beta"], sigma_name="sigma", offset=m["offset"])
    assert not fake.calls[0]["has_groups"] and plain["elpd_loo"] != want["elpd_loo"]
    with pytest.raises(ValueError, match="not found in posterior"):
        pl.loo_glm(data, m["X"], m["y"], "gaussian", ["beta"], sigma_name="sigma", group_terms=[("county", i0)])
    with pytest.raises(ValueError, match=r"group_terms\[0\] must be \(name, index\)"):
        pl.loo_glm(data, m["X"], m["y"], "gaussian", ["beta"], sigma_name="sigma", group_terms=[(i0, "school")])


@pytest.mark.parametrize("estimator", ["diff_srs", "srs"])
def test_subsample_equals_loo_subsample_from_matrix(fake, estimator):
    import pyloo_amd as pl

    m = glmm_ref.make_model(np.random.default_rng(72), 60, 300, 4, "poisson", sizes=(6, 4))
    a, k = glmm_ref.front_args(m)
    ll = glmm_ref.matrix_of(m)
    for obs, draws in ((12, None), (np.array([3, 50, 7, 8, 21, 22]), 64)):
        np.random.seed(5)
        (got, idx, est), msgs = quiet(pl.loo_subsample_glm, *a, **k, observations=obs, loo_approximation="lpd", estimator=estimator,
                                      loo_approximation_draws=draws, pointwise=True)
        np.random.seed(5)
        (want, widx, west), wmsgs = quiet(pl.loo_subsample_from_matrix, ll, observations=obs, loo_approximation="lpd", estimator=estimator,
                                          loo_approximation_draws=draws, pointwise=True)
        assert np.array_equal(idx.idx, widx.idx) and np.array_equal(idx.m_i, widx.m_i) and msgs == wmsgs
        for key in ("elpd_loo", "se", "p_loo", "p_loo_se", "subsampling_SE", "looic"):
            np.testing.assert_allclose(got[key], want[key], rtol=1e-12, err_msg=key)
        np.testing.assert_allclose(got["loo_i"], want["loo_i"], rtol=1e-12, equal_nan=True)
        assert all(c["has_groups"] for c in fake.calls)
    fake.calls.clear()
    quiet(pl.loo_subsample_glm, *a, **k, observations=10, loo_approximation="plpd", estimator=estimator)
    assert fake.calls[0]["n_draws"] == 1 and fake.calls[0]["groups"][0][1].shape == (1, 6)


# ------------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


def header_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    return [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_0-9]+)(?:\[[A-Z_]+\])?\s*(?:,|$)", decl.strip())]


def test_new_symbol_in_header_binding_and_library(lib):
    from pyloo_amd import _capi
    from pyloo_amd import build as b

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pla_glm_grouped" in _capi.SYMBOLS and hasattr(lib, "pla_glm_grouped") and len(lib.pla_glm_grouped.argtypes) == 1
    assert re.search(r"\bint pla_glm_grouped\(const pla_glm_grouped_args \*", header) and re.search(r"\bpla_glm_grouped\b", guide)
    assert "pla_k_glm_terms.hip" in b.SOURCES
    assert "#define PLA_GLM_MAX_TERMS 8\n" in header and _capi.GLM_MAX_TERMS == 8
    # pla_glm_args is what it was: 34 fields, 256 bytes; the new blocks are the header's, field for field
    assert C.sizeof(_capi.GlmArgs) == 256 and len(header_fields(header, "pla_glm_args")) == 34
    assert header_fields(header, "pla_glm_term") == [n for n, _ in _capi.GlmTerm._fields_]
    assert header_fields(header, "pla_glm_grouped_args") == [n for n, _ in _capi.GlmGroupedArgs._fields_]
    assert C.sizeof(_capi.GlmTerm) == 48 and C.sizeof(_capi.GlmGroupedArgs) == 8 + 256 + 8 + 8 * 48
    assert _capi.GlmGroupedArgs().glm.struct_size == 256
    assert lib.pla_abi_version() == _capi.ABI_VERSION


def test_argument_errors_each_have_their_own_message(lib):
    from pyloo_amd import _capi

    seen = set()

    def message(args):
        assert lib.pla_glm_grouped(C.byref(args)) == -1
        msg = lib.pla_last_error()
        assert msg not in seen, msg
        seen.add(msg)
        return msg

    assert lib.pla_glm_grouped(None) == -1 and lib.pla_last_error() == b"args is NULL"
    n, p, s, g = 4, 3, 16, 3
    buf = (C.c_double * 64)()
    index = (C.c_int32 * n)(0, 2, 1, 2)
    out = (C.c_double * (n * s))()
    args = _capi.GlmGroupedArgs(n_terms=1)
    base = _capi.GlmArgs(engine=1,  # (never followed: nothing below gets past the argument checks)
                         family=_capi.PLA_GLM_POISSON_LOG, mode=_capi.PLA_GLM_MODE_MATRIX, mem_space=_capi.PLA_HOST, n_obs=n, n_pred=p, n_draws=s,
                         x=C.addressof(buf), x_stride_obs=p, x_stride_pred=1, beta=C.addressof(buf), beta_stride_draw=p, beta_stride_pred=1,
                         y=C.addressof(buf), out=C.addressof(out), out_pitch=s)
    args.glm = base
    args.terms[0] = _capi.GlmTerm(group_index=C.addressof(index), u=C.addressof(buf), u_stride_draw=g, u_stride_group=1, n_groups=g)
    args.struct_size -= 8
    msg = message(args)
    assert b"struct_size" in msg and b"pla_glm_grouped_args" in msg and str(C.sizeof(_capi.GlmGroupedArgs)).encode() in msg
    args.struct_size += 8
    args.glm.struct_size = 8
    assert b"glm.struct_size is 8, pla_glm_args of this library has 256 bytes" in message(args)
    args.glm.struct_size = 256
    args.glm.family = 7
    assert b"bad family" in message(args)  # (the checks of pla_glm come first, with its words)
    args.glm.family = _capi.PLA_GLM_POISSON_LOG
    args.n_terms = 9
    assert b"n_terms must lie in [0, 8], got 9" in message(args)
    args.n_terms = -1
    assert b"n_terms must lie in [0, 8], got -1" in message(args)
    args.n_terms = 1
    args.terms[0].u = None
    assert b"term 0: u is NULL" in message(args)
    args.terms[0].u = C.addressof(buf)
    args.terms[0].n_groups = 0
    assert b"term 0: n_groups must lie in [1, 2^31), got 0" in message(args)
    args.terms[0].n_groups = g
    args.terms[0].group_index = None
    assert b"term 0: group_index is NULL" in message(args)
    args.terms[0].group_index = C.addressof(index)
    args.terms[0].u_stride_group = 0
    assert b"term 0: u strides must be positive" in message(args)
    args.terms[0].u_stride_group = 2
    assert lib.pla_glm_grouped(C.byref(args)) == -4 and b"term 0: PLA_HOST u must be dense" in lib.pla_last_error()
    args.terms[0].u_stride_group = 1
    index[1] = -1
    assert b"term 0: group_index[1] = -1 is outside [0, 3)" in message(args)
    index[1], index[3] = 2, g
    assert b"term 0: group_index[3] = 3 is outside [0, 3)" in message(args)
    index[3] = 2
    args.n_terms = 2  # the second term is checked like the first
    args.terms[1] = _capi.GlmTerm(group_index=C.addressof(index), u=C.addressof(buf), u_stride_draw=2, u_stride_group=1, n_groups=2)
    assert b"term 1: group_index[1] = 2 is outside [0, 2)" in message(args)


# ------------------------------------------------------------------------------------------------------------- the generated code
# wavefronts per SIMD of glm_terms_kernel<family, chunks, panel>, as the compiler's resource report gives them
WAVES = {
    ("linpred", 1, 0): 6, ("linpred", 2, 0): 5, ("linpred", 4, 0): 3, ("linpred", 8, 0): 2, ("linpred", 8, 1): 3,
    ("gaussian", 1, 0): 5, ("gaussian", 2, 0): 4, ("gaussian", 4, 0): 3, ("gaussian", 8, 0): 2, ("gaussian", 8, 1): 3,
    ("binomial", 1, 0): 4, ("binomial", 2, 0): 4, ("binomial", 4, 0): 3, ("binomial", 8, 0): 2, ("binomial", 8, 1): 3,
    ("poisson", 1, 0): 5, ("poisson", 2, 0): 4, ("poisson", 4, 0): 3, ("poisson", 8, 0): 2, ("poisson", 8, 1): 3,
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_new_kernels_use_no_scratch_and_keep_the_stated_occupancy(tmp_path):
    """no scratch and no LDS in any kernel of the unit, the MFMA chain of the kernel without terms (four steps per
    chunk, the tile loop not duplicated), and the wavefronts per SIMD the table above states for every instantiation."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    lines = isa_stats.compile_isa(out=str(tmp_path / "glm_terms.s"), units=["pla_k_glm_terms.hip"])
    names = [k for k in isa_stats.all_kernels(lines) if "glm_" in k]
    assert len(names) == 1 + 20 and not any("glm_prepare_kernel" in k for k in names), names  # (the prepare kernel of beta is not built twice)
    family = {0: "linpred", 1: "gaussian", 2: "binomial", 3: "poisson"}
    seen = set()
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert not isa_stats.masked_spills(lines, k[2:]) and total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert res.get("LDSByteSize", 0) == 0, (name, res)
        regs = res["NumVgprs"] + res.get("NumAgprs", 0)
        if "prepare" in k:
            assert regs <= 64, (name, res)
            continue
        fam, nch, panel = (int(v) for v in re.search(r"Li(\d)ELi(\d)ELb([01])E", k).groups())
        start = next(i for i, l in enumerate(lines) if l.startswith(k + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[i]))
        mfma = sum(l.strip().startswith("v_mfma_f64_16x16x4_f64") for l in lines[start:end])
        assert mfma == 4 * nch, (name, mfma)
        waves = WAVES[(family[fam], nch, panel)]
        seen.add((family[fam], nch, panel))
        assert regs <= 512 // waves // 8 * 8 and res.get("Occupancy", 0) == waves, (name, res, waves)
    assert seen == set(WAVES)
