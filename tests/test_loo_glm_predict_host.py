"""Host-side tests of ``loo_glm_predict`` (no GPU): the exports and the binding, the fronts' validation, the restatement's discrete
distribution functions against scipy, and the generated code of the predictive kernels."""

import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import glm_predict_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()  # (a failed build or a symbol the library does not export is a failure, not a skip)
    from pyloo_amd import _capi

    return _capi.load_library()


def test_exports_binding_and_sources(lib):
    import pyloo_amd as pl
    from pyloo_amd import _capi
    from pyloo_amd import build as b

    for name in ("LooGlmPredict", "loo_glm_predict", "loo_glm_predict_from_design"):
        assert name in pl.__all__ and hasattr(pl, name)
    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    for name in ("pla_glm_predict", "pla_glm_predict_segment"):
        assert name in _capi.SYMBOLS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, header)
    assert "pla_k_glm_predict.hip" in b.SOURCES and "pla_k_glm_predict_families.hip" in b.SOURCES
    assert lib.pla_glm_predict_segment() == ref.SEG == pl.engine.Engine.glm_predict_segment()
    assert lib.pla_abi_version() == _capi.ABI_VERSION  # (a pure addition)
    # the binding's struct is the header's, field for field; pla_glm_args did not grow
    body = re.search(r"typedef struct pla_glm_predict_args \{(.*?)\} pla_glm_predict_args;", header, flags=re.S).group(1)
    declared = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert declared == [name for name, _ in _capi.GlmPredictArgs._fields_], declared
    assert C.sizeof(_capi.GlmArgs) == 256 and C.sizeof(_capi.GlmPredictArgs) == 8 + 256 + 8 * (len(declared) - 2)
    assert len(lib.pla_glm_predict.argtypes) == 1


def test_abi_argument_errors(lib):
    from pyloo_amd import _capi

    def code(a):
        return lib.pla_glm_predict(C.byref(a)), lib.pla_last_error()

    assert lib.pla_glm_predict(None) == -1
    a = _capi.GlmPredictArgs()
    a.struct_size -= 8
    rc, msg = code(a)
    assert rc == -1 and b"struct_size" in msg and str(C.sizeof(_capi.GlmPredictArgs)).encode() in msg
    a = _capi.GlmPredictArgs()
    a.glm.struct_size = 8
    rc, msg = code(a)
    assert rc == -1 and b"glm.struct_size" in msg
    a = _capi.GlmPredictArgs(kind=2)
    rc, msg = code(a)
    assert rc == -1 and b"kind" in msg
    a = _capi.GlmPredictArgs(kind=_capi.PLA_PIT_LOG_WEIGHTS)
    a.glm.family = _capi.PLA_GLM_LINPRED
    rc, msg = code(a)
    assert rc == -1 and b"LINPRED" in msg
    a.glm.family = _capi.PLA_GLM_POISSON_LOG
    rc, msg = code(a)
    assert rc == -1 and b"engine is NULL" in msg  # (glm_check's own order from here on)
    a.glm.engine = 1  # (never followed: nothing below gets past the argument checks)
    a.glm.n_obs, a.glm.n_pred, a.glm.n_draws = 2, 300, 16
    rc, msg = code(a)
    assert rc == -1 and b"n_pred must lie in [1, 256]" in msg
    a.glm.n_pred, a.glm.n_draws = 3, 1
    rc, msg = code(a)
    assert rc == -1 and b"n_draws" in msg
    buf = (C.c_double * 64)()
    a.glm.n_draws = 16
    a.glm.x = a.glm.beta = a.glm.y = C.addressof(buf)
    a.glm.x_stride_obs, a.glm.x_stride_pred, a.glm.beta_stride_draw, a.glm.beta_stride_pred = 3, 1, 3, 1
    a.glm.mem_space = _capi.PLA_DEVICE
    rc, msg = code(a)
    assert rc == -1 and b"log_weights is NULL" in msg
    a.log_weights = C.addressof(buf)
    a.lw_stride_obs, a.lw_stride_draw = 16, 0
    rc, msg = code(a)
    assert rc == -1 and b"strides must be positive" in msg
    a.lw_stride_obs, a.lw_stride_draw = 1, 16
    rc, msg = code(a)
    assert rc == -4 and b"unit stride along the draws" in msg
    a.lw_stride_obs, a.lw_stride_draw = 8, 1
    rc, msg = code(a)
    assert rc == -1 and b"lw_stride_obs" in msg
    a.lw_stride_obs = 16
    a.glm.family, a.glm.draw_scale, a.glm.draw_const, a.pit_lt = _capi.PLA_GLM_GAMMA_LOG, C.addressof(buf), C.addressof(buf), C.addressof(buf)
    rc, msg = code(a)
    assert rc == -4 and b"PLA_GLM_GAMMA_LOG" in msg
    a.kind, a.glm.family, a.glm.method, a.glm.tail_count = _capi.PLA_PIT_LOGLIK, _capi.PLA_GLM_POISSON_LOG, _capi.PLA_PSIS, 16
    rc, msg = code(a)
    assert rc == -1 and b"tail_count" in msg


def test_front_validation():
    import pyloo_amd as pl

    rng = np.random.default_rng(0)
    X, beta, y = rng.normal(size=(6, 2)), rng.normal(size=(40, 2)), np.arange(6.0)
    f = pl.loo_glm_predict_from_design
    with pytest.raises(ValueError, match="family must be one of"):
        f(X, y, beta, "student")
    with pytest.raises(ValueError, match="beta must be"):
        f(X, y, beta[:, :1], "poisson")
    with pytest.raises(ValueError, match="y needs 6 values"):
        f(X, y[:5], beta, "poisson")
    with pytest.raises(ValueError, match="non-negative integers"):
        f(X, y - 0.5, beta, "poisson")
    with pytest.raises(ValueError, match="needs sigma"):
        f(X, y, beta, "gaussian")
    with pytest.raises(ValueError, match="at least two draws"):
        f(X, y, beta[:1], "poisson")
    with pytest.raises(ValueError, match="randomized must be"):
        f(X, y, beta, "poisson", randomized="yes")
    with pytest.raises(ValueError, match="gamma family has no PIT"):
        f(X, y + 1.0, beta, "gamma", shape=np.ones(40), randomized=True)
    with pytest.raises(NotImplementedError, match="group-level terms"):
        f(X, y, beta, "poisson", groups=[(np.zeros(6, dtype=int), np.zeros((40, 1)))])
    with pytest.raises(NotImplementedError, match="group-level terms"):
        pl.loo_glm_predict(None, X, y, "poisson", ["b"], group_terms=[("u", np.zeros(6, dtype=int))])
    with pytest.raises(ValueError, match="link of the poisson family"):
        f(X, y, beta, "poisson", link="probit")
    with pytest.raises(ValueError, match="reff must be"):
        f(X, y, beta, "poisson", reff=None)
    from pyloo_amd.engine import Engine

    with pytest.raises(ValueError, match="linpred"):
        Engine.glm_predict(None, X, beta, "linpred")


@pytest.mark.parametrize("fam", ref.DISCRETE)
def test_restated_recurrence_against_scipy(fam):
    """|eta| <= 8, y and trials <= 1024: the downward product recurrence from exp(ll) deviates from scipy's pdtr / bdtr / nbdtr by
    at most 1e-10 absolutely (its error is that of exp(ll), about |ll| u)."""
    rng = np.random.default_rng(len(fam))
    n, S = 160, 9
    eta = np.tile(np.linspace(-8.0, 8.0, S), (n, 1)) + rng.uniform(-0.5, 0.5, size=(n, 1)) * (np.abs(np.linspace(-8.0, 8.0, S)) < 7.4)
    trials = None
    if fam in ("binomial", "binomial_probit"):
        trials = np.concatenate([[1.0, 1.0, 7.0, 1024.0, 1024.0], rng.integers(1, 1025, size=n - 5).astype(np.float64)])
        y = np.concatenate([[0.0, 1.0, 7.0, 0.0, 1024.0], np.floor(rng.uniform(size=n - 5) * (trials[5:] + 1.0))])
    else:
        y = np.concatenate([[0.0, 1.0, 2.0, 17.0, 1000.0, 1024.0], rng.integers(0, 1025, size=n - 6).astype(np.float64)])
    scale = np.linspace(0.4, 6.0, S) if fam == "negbinomial" else None
    assert np.abs(eta).max() <= 8.0 and y.max() <= 1024
    _, _, f_le, f_lt = ref.point(fam, eta, y, scale, trials)
    s_le, s_lt = ref.scipy_cdf(fam, eta, y, scale, trials)
    assert np.all(np.isfinite(f_le)) and np.all(np.isfinite(f_lt)) and np.all(f_lt <= f_le) and np.all(f_le <= 1.0)
    assert np.abs(f_le - s_le).max() <= 1e-10, np.abs(f_le - s_le).max()
    assert np.abs(f_lt - s_lt).max() <= 1e-10, np.abs(f_lt - s_lt).max()


def test_restated_gaussian_against_scipy():
    from scipy.special import ndtr

    t = np.linspace(-12.0, 12.0, 481)
    lo = ref.ndtr_tail(t)
    assert np.abs(np.where(t < 0, lo, 1.0 - lo) - ndtr(t)).max() <= 1e-15


# ------------------------------------------------------------------------------------------------------------- the generated code
# registers (VGPR + AGPR, as the assembler accounts them) and wavefronts per SIMD of glm_predict_kernel<FAM, NCH, PANEL>; beside them
# the generator's waves for the same chunk count: 4, 4, 3, 2 and 2 for the panels
PINNED = {
    (1, 1, False): (144, 3), (1, 2, False): (152, 3), (1, 4, False): (168, 3), (1, 8, False): (200, 2), (1, 8, True): (188, 2),
    (2, 1, False): (182, 2), (2, 2, False): (190, 2), (2, 4, False): (206, 2), (2, 8, False): (238, 2), (2, 8, True): (204, 2),
    (3, 1, False): (156, 3), (3, 2, False): (164, 3), (3, 4, False): (180, 2), (3, 8, False): (212, 2), (3, 8, True): (196, 2),
    (4, 1, False): (176, 2), (4, 2, False): (184, 2), (4, 4, False): (200, 2), (4, 8, False): (232, 2), (4, 8, True): (196, 2),
    (5, 1, False): (125, 4), (5, 2, False): (133, 3), (5, 4, False): (134, 3), (5, 8, False): (166, 3), (5, 8, True): (156, 3),
    (6, 1, False): (176, 2), (6, 2, False): (184, 2), (6, 4, False): (200, 2), (6, 8, False): (232, 2), (6, 8, True): (204, 2),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_predictive_kernels_use_no_scratch_and_keep_the_stated_occupancy(tmp_path):
    """no scratch, no LDS allocation and no scalar register in a vector lane in any kernel of the two units;
    one MFMA chain of four steps per chunk; at least two wavefronts per SIMD everywhere, the figures pinned per instantiation."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    units = ["pla_k_glm_predict.hip", "pla_k_glm_predict_families.hip"]
    lines = isa_stats.compile_isa(out=str(tmp_path / "glm_predict.s"), units=units)
    names = [k for k in isa_stats.all_kernels(lines) if "glm_predict" in k]
    # row maxima, combine; six families x (1, 2, 4, 8 chunks in registers + panels of 8)
    assert len(names) == 2 + 30, names
    seen = {}
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert not isa_stats.masked_spills(lines, k[2:]) and total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert res.get("LDSByteSize", 0) == 0, (name, res)
        regs = res["NumVgprs"] + res.get("NumAgprs", 0)
        if "predict_kernel" not in k:
            assert regs <= 64, (name, res)
            continue
        fam, nch, panel = re.search(r"Li(\d)ELi(\d)ELb([01])E", k).groups()
        start = next(i for i, l in enumerate(lines) if l.startswith(k + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[i]))
        mfma = sum(l.strip().startswith("v_mfma_f64_16x16x4_f64") for l in lines[start:end])
        assert mfma == 4 * int(nch), (name, mfma)
        seen[(int(fam), int(nch), panel == "1")] = (regs, res["Occupancy"])
    assert seen == PINNED, seen
