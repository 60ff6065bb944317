"""Host side of the cluster-marginal GLM fronts (``pyloo_amd/loo_glm_marginal.py``) without a GPU: the fronts through a stand-in
engine whose marginal call is the NumPy restatement (tests/glm_marginal_ref.py) -- every rejection before the first engine call,
what is handed over, the order of the rows, the nodes with and without ``u``, the ``idata`` front --, the restatement against the
closed form of the Gaussian family, the C export (``pla_glm_marginal``) and the generated code of the new kernels.

Without the feature every test but the two against the closed form, which exercise the restatement alone, fails at the missing
module, symbol or source file."""

import ctypes as C
import importlib
import os
import re
import shutil
import sys
import warnings

import numpy as np
import pytest

import fake_xarray
import glm_marginal_ref as ref
import glm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (3, 1, 5, 2, 4, 1)
S, P = 300, 3


@pytest.fixture()
def fake(monkeypatch):
    eng = ref.MarginalEngine()
    for name in ("pyloo_amd.loo", "pyloo_amd.loo_glm", "pyloo_amd.loo_subsample", "pyloo_amd.base", "pyloo_amd.loo_group"):
        monkeypatch.setattr(importlib.import_module(name), "get_engine", lambda device=None: eng)
    return eng


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args, **kwargs)
    return out, [str(w.message) for w in rec]


@pytest.fixture(scope="module")
def models():
    rng = np.random.default_rng(181)
    return {f: ref.make_clustered(rng, SIZES, S, P, f, slope=f == "poisson", n_terms=2 if f == "binomial" else 0)
            for f in ("gaussian", "binomial", "poisson")}


def front_args(m, **more):
    labels = 10 * m["cluster"] + 7  # (labels are not 0 .. C - 1)
    return ((m["X"], m["y"], m["beta"], m["family"], labels, m["tau"]),
            dict(z=m["z"], sigma=m["sigma"], offset=m["offset"], trials=m["trials"], groups=m["terms"], **more))


def restated(m, nodes, logw):
    import pyloo_amd as pl

    index = pl.group_index(m["cluster"])
    fam = glm_ref.ENGINE_FAMILY[m["family"]]
    mem = index.members  # (the linear predictor of the member rows, as the stand-in engine forms it)
    rest = ref.glmm_ref.add_terms(glm_ref.linpred(m["X"][mem], m["beta"], None if m["offset"] is None else m["offset"][mem]), m["terms"],
                                  rows=mem)
    return ref.quadrature(rest, index.offsets, index.members, fam, m["y"], m["tau"], nodes, logw, z=m["z"], trials=m["trials"],
                          oc=glm_ref.obs_const(fam, m["y"], m["trials"]), sigma=m["sigma"])


# ---------------------------------------------------------------------------------------------------------------------- the fronts
def test_every_rejection_comes_before_any_engine_call(fake, models):
    import pyloo_amd as pl

    m = models["poisson"]
    a, k = front_args(m)
    n, c = len(m["y"]), len(SIZES)
    u = np.random.default_rng(3).normal(size=(S, c))
    bad_tau = m["tau"].copy()
    bad_tau[4] = 0.0
    inf_tau = m["tau"].copy()
    inf_tau[1] = np.inf
    flat_u = u.copy()
    flat_u[:, 2] = 1.5

    def call(fn, cluster=a[4], tau=a[5], **kw):
        return fn(*a[:4], cluster, tau, **dict(k, **kw))

    cases = [
        (dict(cluster=a[4][:-1]), ValueError, f"cluster needs {n} values, one per row of X, got {n - 1}"),
        (dict(cluster=a[4].astype(np.float64)), TypeError, "cluster must hold integers"),
        (dict(tau=m["tau"][:-1]), ValueError, f"tau needs {S} values, one per draw, got {S - 1}"),
        (dict(tau=bad_tau), ValueError, "tau must be finite and positive"),
        (dict(tau=inf_tau), ValueError, "tau must be finite and positive"),
        (dict(u=u[:-1]), ValueError, f"u must be (n_draws, C) = ({S}, {c})"),
        (dict(u=u[:, :-1]), ValueError, f"u must be (n_draws, C) = ({S}, {c})"),
        (dict(u=flat_u), ValueError, "u does not vary within a cluster"),
        (dict(loc=np.zeros(c - 1)), ValueError, f"loc needs {c} values, one per cluster, got {c - 1}"),
        (dict(scale=np.ones(c + 1)), ValueError, f"scale needs {c} values, one per cluster, got {c + 1}"),
        (dict(scale=np.where(np.arange(c) == 1, 0.0, 1.0)), ValueError, "scale must be finite and positive"),
        (dict(u=u, loc=np.zeros(c)), ValueError, "give u, or loc and scale, not both"),
        (dict(u=u, scale=np.ones(c)), ValueError, "give u, or loc and scale, not both"),
        (dict(n_nodes=0), ValueError, "n_nodes must be an integer between 1 and 32, got 0"),
        (dict(n_nodes=33), ValueError, "n_nodes must be an integer between 1 and 32, got 33"),
        (dict(z=m["z"][:-1]), ValueError, f"z needs {n} values"),
        (dict(offset=np.zeros(n - 1)), ValueError, f"offset needs {n} values"),  # (what _prepare checks)
        (dict(groups=[(m["cluster"],)]), ValueError, "groups[0] must be (index, draws) or (index, draws, z)"),  # (_prepare_groups)
    ]
    for kw, kind, word in cases:
        with pytest.raises(kind) as err:
            call(pl.glm_marginal_log_lik, **kw)
        assert word in str(err.value), (word, str(err.value))
        kw = {("node_scale" if key == "scale" else key): v for key, v in kw.items()}
        with pytest.raises(kind) as err:
            call(pl.loo_glm_marginal_from_design, **kw)
        assert word in str(err.value), (word, str(err.value))
    with pytest.raises(ValueError, match="reff must be a positive float"):
        call(pl.loo_glm_marginal_from_design, reff=None)
    assert fake.calls == []


def test_what_is_handed_to_the_engine_and_the_order_of_the_rows(fake, models):
    import pyloo_amd as pl

    for f, m in models.items():
        a, k = front_args(m)
        fake.calls.clear()
        got, msgs = quiet(pl.glm_marginal_log_lik, *a, **k, n_nodes=9)
        assert not msgs and len(fake.calls) == 1
        c = fake.calls[0]
        fam = glm_ref.ENGINE_FAMILY[f]
        assert c["op"] == "glm_marginal" and c["family"] == fam and c["mode"] == "matrix"
        # rows in the order of the sorted labels; the index is over the rows of X
        index = c["index"]
        assert np.array_equal(index.labels, 10 * np.arange(len(SIZES)) + 7) and index.n_obs == len(m["y"])
        assert np.array_equal(np.diff(index.offsets), SIZES)
        # the constants of the fronts of loo_glm, tau and z as given
        oc = glm_ref.obs_const(fam, m["y"], m["trials"])
        assert (c["obs_const"] is None) == (oc is None) and (oc is None or np.array_equal(c["obs_const"], oc))
        if f == "gaussian":
            assert np.array_equal(c["draw_scale"], m["sigma"]) and np.array_equal(c["draw_const"], glm_ref.draw_const(m["sigma"]))
        assert np.array_equal(c["tau"], m["tau"]) and (c["z"] is None) == (m["z"] is None)
        # without u: loc = 0 and scale = mean(tau)
        nodes, logw = ref.gauss_hermite(np.zeros(len(SIZES)), np.full(len(SIZES), m["tau"].mean()), 9)
        assert np.array_equal(c["nodes"], nodes) and np.array_equal(c["log_weights"], logw)
        assert got.shape == (len(SIZES), S) and np.array_equal(got, restated(m, nodes, logw))
        # with u: its posterior mean and standard deviation per cluster
        u = 0.3 + np.random.default_rng(5).normal(size=(S, len(SIZES))) * np.arange(1, len(SIZES) + 1)
        fake.calls.clear()
        quiet(pl.glm_marginal_log_lik, *a, **k, u=u)
        nodes, logw = ref.gauss_hermite(u.mean(0), u.std(0, ddof=1), 15)
        assert np.array_equal(fake.calls[0]["nodes"], nodes) and np.array_equal(fake.calls[0]["log_weights"], logw)
        # loc and scale as given
        fake.calls.clear()
        quiet(pl.glm_marginal_log_lik, *a, **k, loc=np.arange(6.0), scale=np.arange(1.0, 7.0), n_nodes=1)
        assert np.array_equal(fake.calls[0]["nodes"], np.arange(6.0)[:, None])


def test_cluster_that_is_a_conditional_term_warns(fake, models):
    import pyloo_amd as pl

    m = models["gaussian"]
    a, k = front_args(m)
    u = 0.1 * np.random.default_rng(9).normal(size=(S, 70))
    _, msgs = quiet(pl.glm_marginal_log_lik, *a, **dict(k, groups=[(a[4], u)]))
    assert len(msgs) == 1 and "cluster is also the index of groups[0]" in msgs[0] and "counted twice" in msgs[0]
    _, msgs = quiet(pl.glm_marginal_log_lik, *a, **dict(k, groups=[(a[4] // 2, u)]))
    assert not msgs


@pytest.mark.parametrize("family", ("gaussian", "binomial", "poisson"))
def test_elpd_data_equals_loo_group_on_the_restatements_matrix(fake, models, family):
    import pyloo_amd as pl

    m = models[family]
    a, k = front_args(m)
    mll, _ = quiet(pl.glm_marginal_log_lik, *a, **k)
    labels = np.unique(a[4])
    for kwargs in (dict(), dict(pointwise=True, reff=0.7), dict(method="sis", pointwise=True), dict(method="tis", scale="deviance")):
        fake.calls.clear()
        got, msgs = quiet(pl.loo_glm_marginal_from_design, *a, **k, **kwargs)
        want, want_msgs = quiet(pl.loo_group_from_matrix, mll, labels, **kwargs)  # one group per row
        assert len(fake.calls) == 1 and fake.calls[0]["op"] == "glm_marginal" and fake.calls[0]["mode"] == "loo"
        assert list(got.index) == list(want.index) and msgs == want_msgs, (kwargs, msgs, want_msgs)
        assert got.method == want.method
        for key in want.index:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), (kwargs, key)


def test_idata_front_picks_the_variables(fake, models):
    import pyloo_amd as pl

    m = models["gaussian"]
    chains, c = 4, len(SIZES)
    u = 0.2 * np.random.default_rng(11).normal(size=(S, c)) + np.arange(c)
    shaped = lambda v, *dims: fake_xarray.DataArray(v.reshape(chains, S // chains, *v.shape[1:]), dims=("chain", "draw", *dims))  # noqa: E731
    post = {"beta": shaped(m["beta"], "coef"), "sigma": shaped(m["sigma"]), "tau_school": shaped(m["tau"]), "school": shaped(u, "school"),
            "tau_other": shaped(2.0 * m["tau"])}
    data = {"posterior": post}
    a, k = front_args(m)
    got, _ = quiet(pl.loo_glm_marginal, data, m["X"], m["y"], "gaussian", ["beta"], a[4], "school", "tau_school", sigma_name="sigma",
                   offset=m["offset"], pointwise=True)
    call = fake.calls[-1]
    assert np.array_equal(call["tau"], m["tau"]) and np.array_equal(call["draw_scale"], m["sigma"])
    nodes, _ = ref.gauss_hermite(u.mean(0), u.std(0, ddof=1), 15)
    assert np.array_equal(call["nodes"], nodes)
    want, _ = quiet(pl.loo_glm_marginal_from_design, *a, **k, u=u, pointwise=True)
    assert np.array_equal(np.asarray(got["logo_i"]), np.asarray(want["logo_i"])) and got["elpd_logo"] == want["elpd_logo"]
    quiet(pl.loo_glm_marginal, data, m["X"], m["y"], "gaussian", ["beta"], a[4], None, "tau_other", sigma_name="sigma")
    assert np.array_equal(fake.calls[-1]["tau"], 2.0 * m["tau"])
    assert np.array_equal(fake.calls[-1]["nodes"], ref.gauss_hermite(np.zeros(c), np.full(c, 2.0 * m["tau"].mean()), 15)[0])
    with pytest.raises(ValueError, match="tau_name must name a scalar variable"):
        pl.loo_glm_marginal(data, m["X"], m["y"], "gaussian", ["beta"], a[4], "school", "school", sigma_name="sigma")
    with pytest.raises(ValueError, match="not found in posterior"):
        pl.loo_glm_marginal(data, m["X"], m["y"], "gaussian", ["beta"], a[4], "county", "tau_school", sigma_name="sigma")


# ------------------------------------------------------------------------------------------------- the scheme against a closed form
# the largest |restatement - closed form| over the cells of the model below (8 clusters of 5 rows, 200 draws,
# 32 nodes, seed 18), measured on the CPU; the bound of the test is 100 times that.
MEASURED_32 = {False: 7.11e-15, True: 5.33e-15}


@pytest.mark.parametrize("slope", (False, True))
def test_restatement_against_the_gaussian_closed_form(slope):
    import pyloo_amd as pl

    m = ref.gaussian_model(np.random.default_rng(18), 8, 5, 200, slope)
    index = pl.group_index(m["cluster"])
    rest = m["rest"][index.members]
    exact = ref.gaussian_closed_form(rest, index.offsets, index.members, m["y"], m["sigma"], m["tau"], m["z"])
    err = {}
    for n_nodes in (15, 32):
        nodes, logw = ref.gauss_hermite(m["u"].mean(0), m["u"].std(0, ddof=1), n_nodes)
        mll = ref.quadrature(rest, index.offsets, index.members, "gaussian", m["y"], m["tau"], nodes, logw, z=m["z"], sigma=m["sigma"])
        err[n_nodes] = np.abs(mll - exact).max()
    print(f"slope={slope}: max |mll - closed form| = {err[32]:.3e} at 32 nodes, {err[15]:.3e} at 15")
    assert MEASURED_32[slope] < 1e-6  # (the project's accuracy target: above it the scheme or the restatement is wrong)
    assert err[32] <= 100 * MEASURED_32[slope]
    assert err[15] > err[32]  # the nodes really vary


# --------------------------------------------------------------------------------------------------------------------- the C export
@pytest.fixture(scope="module")
def lib():
    from pyloo_amd.build import build

    build()
    from pyloo_amd import _capi

    return _capi.load_library()


def header_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    return [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_0-9]+)(?:\[[A-Z_]+\])?\s*(?:,|$)", decl.strip())]


def test_new_symbols_in_header_binding_and_library(lib):
    from pyloo_amd import _capi
    from pyloo_amd import build as b

    header = open(os.path.join(ROOT, "include", "pyloo_amd.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("pla_glm_marginal", "pla_glm_marginal_segment"):
        assert name in _capi.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\b" % name, guide)
    assert re.search(r"\bint pla_glm_marginal\(const pla_glm_marginal_args \*", header)
    assert "pla_k_glm_marginal.hip" in b.SOURCES
    assert header_fields(header, "pla_glm_marginal_args") == [n for n, _ in _capi.GlmMarginalArgs._fields_]
    assert C.sizeof(_capi.GlmMarginalArgs) == 8 + C.sizeof(_capi.GlmGroupedArgs) + 9 * 8
    args = _capi.GlmMarginalArgs()
    assert args.struct_size == C.sizeof(_capi.GlmMarginalArgs) and args.grouped.struct_size == C.sizeof(_capi.GlmGroupedArgs)
    assert args.grouped.glm.struct_size == 256 and C.sizeof(_capi.GlmArgs) == 256  # (the existing blocks are what they were)
    assert lib.pla_glm_marginal_segment() == ref.L
    assert lib.pla_abi_version() == _capi.ABI_VERSION  # (a pure addition)


def test_argument_errors_each_have_their_own_message(lib):
    from pyloo_amd import _capi

    seen = set()

    def message(args):
        assert lib.pla_glm_marginal(C.byref(args)) == -1
        msg = lib.pla_last_error()
        assert msg not in seen, msg
        seen.add(msg)
        return msg

    assert lib.pla_glm_marginal(None) == -1 and lib.pla_last_error() == b"args is NULL"
    n, p, s, c, q = 5, 2, 16, 2, 3
    buf = (C.c_double * 64)(*([1.0] * 64))
    offsets = (C.c_int64 * (c + 1))(0, 3, 5)
    members = (C.c_int64 * n)(0, 2, 4, 1, 3)
    out = (C.c_double * (c * s))()
    base = _capi.GlmArgs(engine=1,  # (never followed: nothing below gets past the argument checks)
                         family=_capi.PLA_GLM_POISSON_LOG, mode=_capi.PLA_GLM_MODE_MATRIX, mem_space=_capi.PLA_HOST, n_obs=n, n_pred=p,
                         n_draws=s, x=C.addressof(buf), x_stride_obs=p, x_stride_pred=1, beta=C.addressof(buf), beta_stride_draw=p,
                         beta_stride_pred=1, y=C.addressof(buf), out=C.addressof(out), out_pitch=s)
    args = _capi.GlmMarginalArgs(n_clusters=c, n_members=n, cluster_offsets=C.addressof(offsets), members=C.addressof(members),
                                 tau=C.addressof(buf), n_nodes=q, nodes=C.addressof(buf), log_weights=C.addressof(buf))
    args.grouped.glm = base
    # the size of the block at each of the three levels
    args.struct_size -= 8
    msg = message(args)
    assert b"struct_size" in msg and b"pla_glm_marginal_args" in msg and str(C.sizeof(_capi.GlmMarginalArgs)).encode() in msg
    args.struct_size += 8
    args.grouped.struct_size = 16
    assert b"grouped.struct_size is 16, pla_glm_grouped_args of this library has" in message(args)
    args.grouped.struct_size = C.sizeof(_capi.GlmGroupedArgs)
    args.grouped.glm.struct_size = 8
    assert b"grouped.glm.struct_size is 8, pla_glm_args of this library has 256 bytes" in message(args)
    args.grouped.glm.struct_size = 256
    # a NULL engine, and the checks of pla_glm with its words
    args.grouped.glm.engine = None
    assert b"engine is NULL" in message(args)
    args.grouped.glm.engine = 1
    args.grouped.glm.family = 7
    assert b"bad family" in message(args)
    args.grouped.glm.family = _capi.PLA_GLM_LINPRED
    assert b"needs a likelihood, not PLA_GLM_LINPRED" in message(args)
    args.grouped.glm.family = _capi.PLA_GLM_POISSON_LOG
    args.grouped.glm.row_index = C.addressof(members)
    args.grouped.glm.n_rows = 1
    assert b"glm.row_index must be NULL" in message(args)
    args.grouped.glm.row_index = None
    # the host lists and vectors
    for bad in (0, 33):
        args.n_nodes = bad
        assert b"n_nodes must lie in [1, 32], got %d" % bad in message(args)
    args.n_nodes = q
    args.n_clusters = -1
    assert b"n_clusters < 0" in message(args)
    args.n_clusters = c
    args.cluster_offsets = None
    assert b"cluster_offsets is NULL" in message(args)
    args.cluster_offsets = C.addressof(offsets)
    args.members = None
    assert b"members is NULL" in message(args)
    args.members = C.addressof(members)
    args.tau = None
    assert b"tau is NULL" in message(args)
    args.tau = C.addressof(buf)
    args.nodes = None
    assert b"nodes or log_weights is NULL" in message(args)
    args.nodes = C.addressof(buf)
    offsets[0] = 1
    assert b"cluster_offsets[0] must be 0, got 1" in message(args)
    offsets[0], offsets[1] = 0, 6
    assert b"cluster_offsets decrease at cluster 1" in message(args)
    offsets[1], offsets[2] = 3, 4
    assert b"cluster_offsets end at 4, n_members is 5" in message(args)
    offsets[2] = 5
    members[3] = n
    assert b"members[3] = 5 is outside [0, 5)" in message(args)
    members[3] = -1
    assert b"members[3] = -1 is outside [0, 5)" in message(args)
    members[3] = 1
    for i, bad in ((2, 0.0), (3, -1.0), (4, float("inf")), (5, float("nan"))):
        buf[i] = bad
        assert b"tau[%d] = " % i in message(args) and b"is not positive and finite" in lib.pla_last_error()
        buf[i] = 1.0
    args.grouped.glm.out = None
    assert b"out is NULL" in message(args)


# ------------------------------------------------------------------------------------------------------------- the generated code
# wavefronts per SIMD of glm_marginal_kernel<family, capacity> and glm_marginal_join_kernel<capacity>, as the
# compiler's resource report gives them
WAVES = {("gaussian", 8): 5, ("gaussian", 16): 3, ("gaussian", 32): 2, ("binomial", 8): 5, ("binomial", 16): 3, ("binomial", 32): 2,
         ("poisson", 8): 5, ("poisson", 16): 3, ("poisson", 32): 2, ("join", 8): 5, ("join", 16): 3, ("join", 32): 2}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_new_kernels_use_no_scratch_and_keep_the_stated_occupancy(tmp_path):
    """No scratch, no LDS, no scalar register spilled into vector lanes in any kernel of the unit, and the wavefronts per SIMD the
    table above states for every instantiation."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    lines = isa_stats.compile_isa(out=str(tmp_path / "glm_marginal.s"), units=["pla_k_glm_marginal.hip"])
    names = [k for k in isa_stats.all_kernels(lines) if "glm_" in k]
    assert len(names) == 12 and all("glm_marginal" in k for k in names), names  # (no kernel of the generator is built again)
    family = {1: "gaussian", 2: "binomial", 3: "poisson"}
    seen = set()
    for k in names:
        name, total, _, res = isa_stats.kernel_stats(lines, k[2:])
        assert res.get("ScratchSize", 0) == 0 and not any(op.startswith("scratch_") for op in total), (name, res)
        assert not isa_stats.masked_spills(lines, k[2:]) and total.get("v_writelane_b32", 0) == 0, (name, dict(total))
        assert res.get("LDSByteSize", 0) == 0, (name, res)
        assert not any(op.startswith("flat_") for op in total), (name, dict(total))  # (every access is global or scalar)
        if "join" in k:
            key = ("join", int(re.search(r"ILi(\d+)E", k).group(1)))
        else:
            fam, cap = (int(v) for v in re.search(r"ILi(\d)ELi(\d+)E", k).groups())
            key = (family[fam], cap)
        seen.add(key)
        regs = res["NumVgprs"] + res.get("NumAgprs", 0)
        waves = WAVES[key]
        assert regs <= 512 // waves // 8 * 8 and res.get("Occupancy", 0) == waves, (name, res, waves)
    assert seen == set(WAVES)
