"""The cluster-marginal GLM likelihood on the GPU (``pla_glm_marginal``, csrc/pla_glm_marginal.h) at the kernels' edges:

  5. parity          mll in matrix mode against the restatement (tests/glm_marginal_ref.py) on the device's own linear predictor,
                     |d| <= 1e-10 (1 + max_q (sum_i |ll_iq| + |prior_q| + |logw_q|)): the 1e-10 relative bound of a single density
                     carried through a sum and a log-sum-exp, which is 1-Lipschitz in the max norm
  6. cross-check     one node at 0 with log-weight 0 against Engine.group_sum of the conditional matrix
  7. order rule      labels, draw order, memory space, .T views and the block size leave every bit where it is
  8. LOO mode        the fused pass equals loo_from_matrix on the matrix bit for bit; the oracle; NaN; SIS
  9. bad structure   device members out of range and a decreasing pair of offsets

Draw counts 1, 2, 63, 64, 65, 250; cluster sizes 1, 2, L - 1, L, L + 1, 2 L + 1, mixed; 1, 2 and 7 clusters; 1, 2, 8, 9, 16, 17, 32
nodes; 1 and 17 predictors; 0 and 2 conditional terms; z given and null; the last cluster held by the last row only.
Without the feature every test fails at the missing engine call."""

import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import glm_marginal_ref as ref
import glm_ref
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_TEXT = "NaN values detected in log-likelihood. These will be ignored in the LOGO calculation."
L = ref.L
MIXED = (1, 2, L - 1, L, L + 1, 2 * L + 1, 1)


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    e = get_engine(0)
    assert e.glm_marginal_segment() == L
    return e


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


def engine_call(m, nodes, logw, put=lambda a: a):
    """What the fronts hand to ``Engine.glm_marginal`` for a model of glm_marginal_ref.make_clustered."""
    import pyloo_amd as pl

    fam = glm_ref.ENGINE_FAMILY[m["family"]]
    oc = None if m["family"] == "gaussian" else glm_ref.obs_const(fam, m["y"], m["trials"])
    dc = None if m["sigma"] is None else glm_ref.draw_const(m["sigma"])
    index = pl.group_index(m["cluster"])
    groups = None if m["terms"] is None else [tuple(put(t) for t in term) for term in m["terms"]]
    args = (put(m["X"]), put(m["beta"]), fam, index, put(m["tau"]), put(nodes), put(logw))
    kw = dict(z=put(m["z"]), y=put(m["y"]), offset=put(m["offset"]), trials=put(m["trials"]), obs_const=put(oc), draw_scale=put(m["sigma"]),
              draw_const=put(dc), groups=groups)
    return index, args, kw


def restate(eng, m, index, nodes, logw, with_bound=False):
    """The restatement on the device's own linear predictor of the member rows (bits that the generator's tests pin)."""
    fam = glm_ref.ENGINE_FAMILY[m["family"]]
    rest = eng.glm(m["X"], m["beta"], "linpred", offset=m["offset"], rows=index.members, **({} if m["terms"] is None else {"groups": m["terms"]}))
    oc = None if m["family"] == "gaussian" else glm_ref.obs_const(fam, m["y"], m["trials"])
    return ref.quadrature(rest, index.offsets, index.members, fam, m["y"], m["tau"], nodes, logw, z=m["z"], trials=m["trials"], oc=oc,
                          sigma=m["sigma"], with_bound=with_bound)


def within_bound(got, want, mag):
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True)
    frac = np.abs(got[fin] - want[fin]) / (1e-10 * (1.0 + mag[fin]))
    return float(frac.max()) if frac.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------- 5. parity
PARITY = [  # family, draws, cluster sizes, nodes, predictors, conditional terms, z, scale of eta
    ("gaussian", 250, MIXED, 15, 17, 2, True, 1.0),
    ("binomial", 250, MIXED, 32, 1, 0, False, 1.0),
    ("poisson", 250, MIXED, 8, 17, 2, True, 1.0),
    ("binomial", 65, (5, 1), 9, 1, 2, True, 40.0),
    ("poisson", 64, (3,), 16, 1, 0, False, 12.0),
    ("gaussian", 63, (2 * L + 1, 1), 17, 17, 0, False, 40.0),
    ("binomial", 1, (2, L + 1), 1, 1, 0, True, 1.0),
    ("poisson", 2, (L, L - 1, 1), 2, 17, 2, False, 1.0),
]
FRACTIONS = {}


@pytest.mark.parametrize("family, s, sizes, n_nodes, p, n_terms, slope, eta_scale", PARITY)
def test_matrix_against_the_restatement(eng, family, s, sizes, n_nodes, p, n_terms, slope, eta_scale):
    rng = np.random.default_rng(1000 + s + n_nodes)
    m = ref.make_clustered(rng, sizes, s, p, family, slope, n_terms, eta_scale)
    if family != "gaussian":
        m["y"][:: 3] = 0.0  # y = 0
    nodes, logw = ref.gauss_hermite(0.2 * rng.normal(size=len(sizes)), np.full(len(sizes), min(float(m["tau"].mean()), 2.0)), n_nodes)
    index, args, kw = engine_call(m, nodes, logw)
    got = eng.glm_marginal(*args, **kw)
    assert got.shape == (len(sizes), s) and "glm_marginal_kernel" in eng.last_kernels()
    assert ("glm_marginal_join_kernel" in eng.last_kernels()) == (max(sizes) > L)
    want, mag = restate(eng, m, index, nodes, logw, with_bound=True)
    frac = within_bound(got, want, mag)
    FRACTIONS[(family, s, n_nodes)] = frac
    print(f"parity {family} S={s} Q={n_nodes}: largest |d| / bound = {frac:.3e}; max |rest| = "
          f"{np.abs(host(eng.glm(m['X'], m['beta'], 'linpred'))).max():.1f}")
    assert frac <= 1.0
    dev = host(eng.glm_marginal(*engine_call(m, nodes, logw, cuda)[1], **engine_call(m, nodes, logw, cuda)[2]))
    assert np.array_equal(dev, got, equal_nan=True)  # host against device input


# ----------------------------------------------------------------------------------------------------------------- 6. cross-check
@pytest.mark.parametrize("family", ("gaussian", "binomial", "poisson"))
def test_one_node_at_zero_is_the_group_sum_of_the_conditional_matrix(eng, family):
    m = ref.make_clustered(np.random.default_rng(61), MIXED, 65, 17, family, slope=True, n_terms=2)
    c = len(MIXED)
    index, args, kw = engine_call(m, np.zeros((c, 1)), np.zeros((c, 1)))
    got = eng.glm_marginal(*args, **kw)
    cond = {k: v for k, v in kw.items() if k != "z"}
    ll = eng.glm(args[0], args[1], args[2], **cond)
    sums, nrep = eng.group_sum(ll, index)
    want = sums + (-ref.LOG_SQRT_2PI - np.log(m["tau"]))[None, :]
    mag = np.stack([np.abs(ll[index.members[index.offsets[g]:index.offsets[g + 1]]]).sum(0) for g in range(c)])
    mag = mag + np.abs(-ref.LOG_SQRT_2PI - np.log(m["tau"]))[None, :]
    assert nrep == 0 and within_bound(got, want, mag) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 7. the order rule
def test_bits_do_not_depend_on_labels_draw_order_layout_or_memory_space(eng):
    import pyloo_amd as pl

    rng = np.random.default_rng(71)
    for family in ("gaussian", "binomial", "poisson"):
        m = ref.make_clustered(rng, MIXED, 250, 17, family, slope=True, n_terms=2)
        c = len(MIXED)
        nodes, logw = ref.gauss_hermite(0.1 * rng.normal(size=c), np.full(c, 0.5), 9)
        index, args, kw = engine_call(m, nodes, logw)
        base = eng.glm_marginal(*args, **kw)
        # the clusters relabelled: the same partition under other labels; row g of the result is the cluster of label g
        perm = rng.permutation(c)
        m2 = dict(m, cluster=perm[m["cluster"]])
        _, args2, kw2 = engine_call(m2, nodes[np.argsort(perm)], logw[np.argsort(perm)])
        assert np.array_equal(eng.glm_marginal(*args2, **kw2)[perm], base, equal_nan=True)
        # the draws permuted
        dp = rng.permutation(250)
        m3 = dict(m, beta=m["beta"][dp], tau=m["tau"][dp], sigma=None if m["sigma"] is None else m["sigma"][dp],
                  terms=[(t[0], t[1][dp], *t[2:]) for t in m["terms"]])
        _, args3, kw3 = engine_call(m3, nodes, logw)
        assert np.array_equal(eng.glm_marginal(*args3, **kw3), base[:, dp], equal_nan=True)
        # .T views of X and beta, on the host and on the device; host against device input
        for put in (lambda a: a, cuda):
            _, a4, k4 = engine_call(m, nodes, logw, put)
            xt = np.asfortranarray(m["X"]) if put is not cuda else cuda(m["X"].T.copy()).T
            bt = np.asfortranarray(m["beta"]) if put is not cuda else cuda(m["beta"].T.copy()).T
            assert np.array_equal(host(eng.glm_marginal(xt, bt, *a4[2:], **k4)), base, equal_nan=True)
            assert np.array_equal(host(eng.glm_marginal(*a4, **k4)), base, equal_nan=True)
        # the front reaches the same bits
        mat = pl.glm_marginal_log_lik(m["X"], m["y"], m["beta"], family, m["cluster"], m["tau"], z=m["z"], loc=np.zeros(c), scale=np.full(c, 0.5),
                                      n_nodes=9, sigma=m["sigma"], offset=m["offset"], trials=m["trials"], groups=m["terms"])
        _, a5, k5 = engine_call(m, *ref.gauss_hermite(np.zeros(c), np.full(c, 0.5), 9))
        assert np.array_equal(mat, eng.glm_marginal(*a5, **k5), equal_nan=True)


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
import glm_marginal_ref as ref, glm_ref
import pyloo_amd as pl
from pyloo_amd.engine import get_engine
eng = get_engine(0)
rng = np.random.default_rng(77)
sizes = (150, 700, 1, 200, 148, 1)  # 1200 rows, one cluster of 700
out, texts = [], []
for family in ("gaussian", "binomial", "poisson"):
    m = ref.make_clustered(rng, sizes, 250, 5, family, True, 2)
    fam = glm_ref.ENGINE_FAMILY[family]
    oc = None if family == "gaussian" else glm_ref.obs_const(fam, m["y"], m["trials"])
    dc = None if m["sigma"] is None else glm_ref.draw_const(m["sigma"])
    nodes, logw = ref.gauss_hermite(np.zeros(len(sizes)), np.full(len(sizes), 0.4), 15)
    index = pl.group_index(m["cluster"])
    cu = lambda a: None if a is None else torch.as_tensor(a).cuda()
    for put in (cu, lambda a: a):
        kw = dict(z=put(m["z"]), y=put(m["y"]), offset=put(m["offset"]), trials=put(m["trials"]), obs_const=put(oc), draw_scale=put(m["sigma"]),
                  draw_const=put(dc), groups=[tuple(put(t) for t in term) for term in m["terms"]])
        a = (put(m["X"]), put(m["beta"]), fam, index, put(m["tau"]), put(nodes), put(logw))
        mat = eng.glm_marginal(*a, **kw)
        texts.append(eng.last_kernels())
        r = eng.glm_marginal(*a, **kw, mode="loo", tail_count=48, good_k=0.7)
        texts.append(eng.last_kernels())
        out += [np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v).reshape(-1) for v in (mat, r["diag"], r["loo_i"], r["lppd_i"], r["n_replaced"])]
np.savez(sys.argv[2], *out)
open(sys.argv[2] + ".txt", "w").write("\n".join(texts))
"""


def test_block_size_independence(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 holds 524 rows of 250 draws, 512 after the cut at a segment boundary: the cluster of 700 rows takes two
    blocks of its own and its sums travel in the carry.  The matrix, every pointwise output and the NaN count are the default's
    (one block) bit for bit, host and device."""
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
    assert len(outs[0]) == 3 * 2 * 5 and all("glm_marginal_join_kernel" in t for t in texts[0] + texts[1])
    # the variable reached the plan: one block by default; with 512 rows a block, the first cluster, the two runs of segments of the
    # cluster of 700, and the four clusters behind it
    assert all(t.endswith("; blocks of members: 1") for t in texts[0]) and all(t.endswith("; blocks of members: 4") for t in texts[1])
    for j, (a, b) in enumerate(zip(*outs)):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), j
    for f in range(3):  # host against device input
        for a, b in zip(outs[1][10 * f: 10 * f + 5], outs[1][10 * f + 5: 10 * f + 10]):
            assert np.array_equal(a, b, equal_nan=True)


# --------------------------------------------------------------------------------------------------------------------- 8. LOO mode
@pytest.mark.parametrize("method", ("psis", "sis"))
@pytest.mark.parametrize("where", ("host", "device"))
def test_fused_pass_equals_the_pass_over_the_matrix(eng, method, where):
    rng = np.random.default_rng(81)
    m = ref.make_clustered(rng, MIXED, 250, 5, "binomial", slope=True, n_terms=2)
    c = len(MIXED)
    nodes, logw = ref.gauss_hermite(np.zeros(c), np.full(c, 0.5), 15)
    _, args, kw = engine_call(m, nodes, logw, cuda if where == "device" else (lambda a: a))
    tail = orc.tail_count(250, 1.0) if method == "psis" else 0
    fused = eng.glm_marginal(*args, **kw, mode="loo", tail_count=tail, method=method, good_k=0.7)
    assert "glm_marginal_kernel" in eng.last_kernels() and "per block of clusters" in eng.last_kernels()
    split = eng.psis_loo(eng.glm_marginal(*args, **kw), tail, method, 1.0, 0.7)
    assert int(fused["n_replaced"]) == 0
    for key in ("diag", "loo_i", "lppd_i"):
        assert np.array_equal(host(fused[key]), host(split[key]), equal_nan=True), key
    np.testing.assert_allclose(host(fused["agg"]), host(split["agg"]), rtol=1e-12)


def test_end_to_end_against_the_oracle(eng):
    import pyloo_amd as pl

    rng = np.random.default_rng(82)
    sizes = tuple(int(v) for v in rng.integers(1, 9, size=40))
    m = ref.make_clustered(rng, sizes, 1000, 4, "poisson", slope=False, n_terms=0)
    m["tau"] = 0.5 * np.exp(0.1 * rng.normal(size=1000))
    index = pl.group_index(m["cluster"])
    nodes, logw = ref.gauss_hermite(np.zeros(40), np.full(40, m["tau"].mean()), 15)
    want = orc.loo_pointwise(restate(eng, m, index, nodes, logw), 1.0, "psis")
    for put in (lambda a: a, cuda):
        got, _ = quiet(pl.loo_glm_marginal_from_design, put(m["X"]), m["y"], m["beta"], "poisson", m["cluster"], m["tau"], offset=m["offset"],
                       pointwise=True)
        np.testing.assert_allclose(host(np.asarray(got["logo_i"])), want["loo_i"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(host(got["pareto_k"]), want["diag"], rtol=0, atol=1e-9)
        assert got["n_groups"] == 40 and got["n_samples"] == 1000


def test_nan_is_counted_replaced_and_warned_about(eng, monkeypatch):
    import pyloo_amd as pl

    rng = np.random.default_rng(83)
    sizes = (3, 1, 4, 2, 5, 1)
    m = ref.make_clustered(rng, sizes, 500, 4, "poisson", slope=False, n_terms=0)
    m["tau"] = 0.5 * np.exp(0.1 * rng.normal(size=500))
    nodes, logw = ref.gauss_hermite(np.zeros(6), np.full(6, 0.5), 7)
    X = m["X"].copy()
    row = int(np.flatnonzero(m["cluster"] == 2)[1])
    X[row, 1] = np.nan  # a NaN in X: the whole cluster 2 is NaN under every draw
    for put in (cuda, lambda a: a):
        index, args, kw = engine_call(dict(m, X=X), nodes, logw, put)
        r = eng.glm_marginal(*args, **kw, mode="loo", tail_count=orc.tail_count(500, 1.0), good_k=0.7)
        assert int(r["n_replaced"]) == 500
        mat = host(eng.glm_marginal(*args, **kw))  # the matrix mode passes the NaN through
        assert np.isnan(mat[2]).all() and np.isfinite(np.delete(mat, 2, axis=0)).all()
        want = orc.loo_pointwise(np.where(np.isnan(mat), -1e10, mat), 1.0, "psis")
        ok = np.arange(6) != 2
        np.testing.assert_allclose(host(r["loo_i"])[ok], want["loo_i"][ok], rtol=0, atol=1e-9)
        np.testing.assert_allclose(host(r["loo_i"])[~ok], want["loo_i"][~ok], rtol=1e-12)
    # the front's warning: the NaN injected behind its checks
    real = eng.glm_marginal

    def with_nan(Xc, *a, **k):
        return real(X, *a, **k)

    monkeypatch.setattr(eng, "glm_marginal", with_nan)
    _, msgs = quiet(pl.loo_glm_marginal_from_design, m["X"], m["y"], m["beta"], "poisson", m["cluster"], m["tau"], offset=m["offset"], n_nodes=7)
    assert msgs.count(NAN_TEXT) == 1


# ---------------------------------------------------------------------------------------------------------------- 9. bad structure
def test_device_lists_with_bad_structure_are_clamped(eng):
    """Device members out of range are clamped into [0, n_obs); a device pair of offsets that decreases or leaves [0, n_members] is an
    empty cluster, whose value is the log-sum-exp of prior plus log-weight alone; the other clusters are what they were."""
    import torch

    from pyloo_amd.loo_group import GroupIndex

    rng = np.random.default_rng(91)
    sizes = (4, 3, L + 2, 2)
    m = ref.make_clustered(rng, sizes, 65, 3, "binomial", slope=True, n_terms=0)
    n, c = len(m["y"]), len(sizes)
    nodes, logw = ref.gauss_hermite(np.zeros(c), np.full(c, 0.5), 9)
    index, args, kw = engine_call(m, nodes, logw, cuda)
    good = host(eng.glm_marginal(*args, **kw))
    off = np.asarray(index.offsets)  # [0, 4, 7, 7 + L + 2, n]
    # five clusters: (0, 4); (4, 3), which decreases; (3, 7), well formed, though it shares member 3 with the first; (7, 7 + L + 2),
    # the third cluster of the well-formed call; (7 + L + 2, n + 5), which leaves the list
    offsets = np.array([off[0], off[1], off[1] - 1, off[2], off[3], n + 5], dtype=np.int64)
    nodes5, logw5 = np.insert(nodes, 2, nodes[1], axis=0), np.insert(logw, 2, logw[1], axis=0)
    members = np.asarray(index.members).copy()
    members[1] = n + 7   # clamped to n - 1
    members[5] = -3      # clamped to 0
    bad = GroupIndex(np.arange(5), torch.as_tensor(offsets).cuda(), torch.as_tensor(members).cuda())
    got = host(eng.glm_marginal(args[0], args[1], args[2], bad, args[4], cuda(nodes5), cuda(logw5), **kw))
    assert got.shape == (5, 65)
    # the malformed pairs: the device's own value of a legal empty cluster with the same nodes (the restatement's, below, agrees
    # within the parity bound; NumPy's log and exp are not the device's to the bit)
    legal = GroupIndex(np.arange(5), torch.as_tensor(np.array([off[0], off[1], off[1], off[2], off[3], off[3]], dtype=np.int64)).cuda(),
                       torch.as_tensor(np.asarray(index.members)).cuda())
    empty = host(eng.glm_marginal(args[0], args[1], args[2], legal, args[4], cuda(nodes5), cuda(logw5), **kw))
    assert np.isfinite(empty[[1, 4]]).all() and np.array_equal(empty[3], good[2])
    assert np.array_equal(got[1], empty[1]) and np.array_equal(got[4], empty[4])
    assert np.array_equal(got[3], good[2])   # untouched: a cluster of more than one segment
    # the first and the third cluster hold a clamped member each: what the restatement gives with the clamped list
    clamped = np.clip(members, 0, n - 1)
    rest = eng.glm(m["X"], m["beta"], "linpred", offset=m["offset"], rows=clamped)
    want = ref.quadrature(rest, offsets, clamped, "binomial", m["y"], m["tau"], nodes5, logw5, z=m["z"], trials=m["trials"],
                          oc=glm_ref.obs_const("binomial", m["y"], m["trials"]), with_bound=True)
    assert within_bound(got, *want) <= 1.0
