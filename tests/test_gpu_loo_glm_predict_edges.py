"""The GLM predictive kernels (csrc/pla_glm_predict.h, csrc/pla_k_glm_predict.hip) at the family, chunk, strip, weight and launch
edges tests/test_gpu_loo_glm_predict.py leaves unrun.  The inputs and the launch rule are tests/glm_predict_edge_cases.py's;
tests/test_glm_predict_edges_host.py proves on the CPU that the shapes reach the regimes named here and that the inputs are fit
for the comparison.  Every comparison is against the NumPy restatement (tests/glm_predict_ref.py) on the kernel's own eta, or
against a call in a regime the other file validates, and prints its largest deviation over its bound (``pytest -s``).

==========================================================================  =====================================================
structure                                                                   test
==========================================================================  =====================================================
glm_predict_kernel<FAM, NCH, PANEL>: 6 families x (1, 2, 4, 8 chunks in     test_every_instantiation: P = 5, 17, 40, 100, 129,
registers, panels of 8)                                                     random weights and one-hot weights, the route text
the walk of up to 4096 turns, a lane's four rows rotated through it, all    test_mixed_counts_in_one_tile: counts 4096, 0, 200, 1
draws contributing; a segment and one tile, a segment less one draw         in one lane's rows; S = 255, 257, 300
the cap: a count of 4097 or -1 beside the walked rows                       test_count_outside_the_cap_...
the loop over a strip's segments: the sums zeroed again, the slot of        test_several_segments_per_wavefront: 8200 x 4100
`part`, the ragged last strip, the cut of a segment at the strip's end      (strips of 2, 2, ..., 1 segments), 131080 x 272 (one
                                                                            strip of a segment and a single tile)
the grid-stride loops of the row maxima and of the combine kernel           test_second_rounds_of_the_small_kernels: 2 097 452 x 2
NaN, +inf and all -inf weights                                              test_weights_that_are_not_finite
NaN and inf in X                                                            test_non_finite_rows_of_x
weights read in place at a padded pitch; strided X and beta; row lists      test_layouts
want_pit = 0                                                                test_without_pit
the integer atomic of the skipped rows over the blocks of a fused pass      test_skipped_counter_over_blocks (children)
==========================================================================  =====================================================

Not covered here: three or more segments per wavefront need n_rows x n_draws > 2 x 8192 x 16 x 256 (half a gigabyte of weights and
more); they take further turns of the loop the two-segment strips enter a second time, nothing else.

TOLERANCES.  Per element, and sums under one-hot weights: ``1e-10 max(1, |want|)``, the project's aim for pointwise outputs.
Weighted sums against long double, the terms from the restatement on the kernel's eta: a relative 1e-12 for the Gaussian and the
Poisson family; ``glm_predict_ref.weighted_bound`` for the four families whose terms pass through the device's lgamma / erfcx.
Re-arrangements: the same bits.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import glm_predict_edge_cases as ec
import glm_predict_ref as ref
import glm_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("gaussian", "poisson")  # weighted sums held to a relative 1e-12


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def cuda(a):
    import torch

    return None if a is None else torch.as_tensor(np.array(a, order="C")).cuda()  # (a copy: the builders' arrays are read-only)


def same(a):
    return a


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def run(eng, c, lw, put=same, pit=True, **over):
    """``Engine.glm_predict`` on a case of the builders (``over``: replacements of its arrays, ``rows``) -> a dict of NumPy arrays,
    ``n_pit_skipped`` an int, and the route text."""
    c = dict(c, **{k: v for k, v in over.items() if k != "rows"})
    out = eng.glm_predict(put(c["X"]), put(c["beta"]), c["family"], rows=over.get("rows"), log_weights=put(lw), pit=pit,
                          **ec.engine_kwargs(c, put))
    res = {f: (None if out[f] is None else host(out[f])) for f in ec.FIELDS}
    res["n_pit_skipped"] = int(host(out["n_pit_skipped"]).reshape(-1)[0])
    res["route"] = eng.last_kernels()
    return res


def kernel_eta(eng, c, **over):
    c = dict(c, **over)
    return host(eng.glm(c["X"], c["beta"], "linpred", offset=c["offset"]))


def element_bound(want):
    return 1e-10 * np.maximum(1.0, np.abs(want))


def sum_bound(fam, lw, term, want):
    return 1e-12 * np.abs(want) if fam in EXACT else ref.weighted_bound(lw, term)


def check(label, got, want, bound):
    """NaN where the reference has NaN, the same infinities, and elsewhere |got - want| <= bound (a bound of zero: equality)."""
    got, want, bound = (np.asarray(a, dtype=np.float64) for a in (got, want, bound))
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), label
    ok = np.isfinite(want)
    with np.errstate(all="ignore"):
        err = np.abs(got[ok] - want[ok])
        over = np.where(err == 0.0, 0.0, err / bound[ok])
    worst = float(over.max()) if over.size else 0.0
    print(f"{label}: largest |got - want| / bound = {worst:.3e} over {over.size} values")
    assert worst <= 1.0, (label, worst)
    return worst


def check_weighted(label, fam, res, eta, c, lw, rows=slice(None)):
    want, terms = ec.expected(fam, eta, c["y"], c["scale"], c["trials"], lw)
    worst = 0.0
    for f in ec.fields_of(fam):
        worst = max(worst, check(f"{label} {f}", res[f][rows], want[f], sum_bound(fam, lw, terms[f], want[f])))
    return want, terms, worst


# ---------------------------------------------------------------------------------------------------------- 1. every instantiation
@pytest.mark.parametrize("p", ec.PREDICTORS)
@pytest.mark.parametrize("fam", ec.FAMILIES)
def test_every_instantiation(eng, fam, p):
    """33 x 250 of each family at each chunk count: the four weighted outputs under random weights (5 % of them log -inf) against
    long double, the route text, and one-hot weights on a draw of the first and of the last tile against the per-element terms
    (the Gaussian mean: eta itself, bit for bit)."""
    s = 250
    c, lw = ec.case(fam, s, p), ec.weights(ec.N, s, 0, 0.05)
    assert np.isneginf(lw).sum() > 100
    eta = kernel_eta(eng, c)
    res = run(eng, c, lw)
    nch, panel = ec.chunks(p)
    want_route = f"glm_predict_kernel<{ec.ROUTE_NAME[fam]}, {nch} chunks of 16 predictors{' per panel' if panel else ' in registers'}>"
    assert want_route in res["route"], res["route"]
    assert res["n_pit_skipped"] == 0
    if fam == "gamma":
        assert res["pit_le"] is None and res["pit_lt"] is None
    _, terms, _ = check_weighted(f"{fam} P = {p}", fam, res, eta, c, lw)
    for s0 in (3, s - 1):
        hot = run(eng, c, ref.one_hot(ec.N, s, s0))
        for f in ec.fields_of(fam):
            check(f"{fam} P = {p} one-hot on draw {s0} {f}", hot[f], terms[f][:, s0], element_bound(terms[f][:, s0]))
        if fam == "gaussian":
            assert same_bits(hot["mean"], eta[:, s0]) and same_bits(hot["pit_le"], hot["pit_lt"])


# ------------------------------------------------------------------------------------------------------ 2. mixed counts in one tile
@pytest.mark.parametrize("s", ec.MIXED_DRAWS)
@pytest.mark.parametrize("fam", ec.DISCRETE)
def test_mixed_counts_in_one_tile(eng, fam, s):
    """Counts 4096, 0, 200 and 1 in the four rows one lane rotates through its walk, small counts around them, every draw
    contributing: against long double, from host and from device memory (the same bits)."""
    c, lw = ec.case(fam, s, ec.P, True), ec.weights(ec.N, s, 0, 0.05)
    eta = kernel_eta(eng, c)
    res = run(eng, c, lw)
    assert res["n_pit_skipped"] == 0
    want, _, _ = check_weighted(f"{fam} mixed counts S = {s}", fam, res, eta, c, lw)
    ok = ec.inside(res["pit_le"], res["pit_lt"])
    assert all(ok[r] for r in ec.INSIDE_ROWS[fam]) and 2 * ok.sum() >= ok.size
    dev = run(eng, c, lw, put=cuda)
    for f in ec.FIELDS:
        assert same_bits(dev[f], res[f]), f


@pytest.mark.parametrize("fam", ec.DISCRETE)
def test_count_outside_the_cap_is_skipped_and_leaves_its_tile_alone(eng, fam):
    """The row of count 4096 pushed to 4097 and to -1: one row skipped, its two PIT values NaN, its moments and every other row --
    the walked rows of its own lane and tile among them -- bit for bit those of the unmodified call."""
    c, lw = ec.case(fam, ec.S, ec.P, True), ec.weights(ec.N, ec.S, 0, 0.05)
    base = run(eng, c, lw)
    assert base["n_pit_skipped"] == 0 and np.all(np.isfinite(base["pit_le"]))
    others = np.arange(ec.N) != ec.CAP_ROW
    for bad in (4097.0, -1.0):
        y = c["y"].copy()
        y[ec.CAP_ROW] = bad
        for put in (same, cuda):
            got = run(eng, c, lw, put=put, y=y)
            assert got["n_pit_skipped"] == 1, (bad, got["n_pit_skipped"])
            assert np.isnan(got["pit_le"][ec.CAP_ROW]) and np.isnan(got["pit_lt"][ec.CAP_ROW])
            for f in ec.FIELDS:
                assert same_bits(got[f][others], base[f][others]), (bad, f)
            assert same_bits(got["mean"], base["mean"]) and same_bits(got["m2"], base["m2"]), bad


# ------------------------------------------------------------------------------------------- 3. several segments per wavefront
def device_model(fam, n, s, p, seed):
    """A model of glm_ref.make_model's kind drawn on the device (the Gaussian one with an intercept of 3: eta of one sign, see
    tests/glm_predict_edge_cases.py); the constants from the host's gammaln / log as the fronts compute them."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda *shape: torch.randn(*shape, generator=g, device="cuda", dtype=torch.float64)  # noqa: E731
    X = rand(n, p)
    X[:, 0] = 1.0
    b0 = 0.5 * rand(p) / np.sqrt(p)
    if fam == "gaussian":
        b0[0] += ec.GAUSSIAN_SHIFT
    beta = b0 + 0.15 * rand(s, p) / np.sqrt(p)
    offset = 0.3 * rand(n)
    eta0 = X @ b0 + offset
    if fam == "gaussian":
        scale = torch.exp(0.1 * rand(s))
        y = eta0 + rand(n)
    else:
        scale = None
        y = torch.poisson(torch.exp(eta0), generator=g)
    lw = 3.0 * rand(n, s)
    oc, dc = ref.constants(fam, host(y), None, None if scale is None else host(scale))
    return dict(family=fam, X=X, y=y, beta=beta, scale=scale, trials=None, offset=offset, oc=cuda(oc), dc=cuda(dc)), lw


ROW_KEYS = ("X", "y", "offset", "oc")


def device_call(eng, c, lw, a=None, b=None):
    c = dict(c, **{k: (None if c[k] is None else c[k][a:b]) for k in ROW_KEYS})
    out = eng.glm_predict(c["X"], c["beta"], c["family"], log_weights=lw[a:b], **ec.engine_kwargs(c))
    return out


def rows_on_host(eng, c, lw, rows):
    """The rows ``rows`` of a device model as a host case, the kernel's eta of them and their weights."""
    import torch

    idx = torch.as_tensor(rows, device="cuda")
    sub = dict(c, **{k: (None if c[k] is None else c[k][idx]) for k in ROW_KEYS})
    eta = host(eng.glm(sub["X"], sub["beta"], "linpred", offset=sub["offset"]))
    return {k: (host(v) if hasattr(v, "detach") else v) for k, v in sub.items()}, eta, host(lw[idx])


@pytest.mark.parametrize("fam,shape,blocks,rows", [
    ("gaussian", ec.STRIPS, ec.STRIPS_BLOCKS, ec.STRIPS_ROWS), ("poisson", ec.STRIPS, ec.STRIPS_BLOCKS, ec.STRIPS_ROWS),
    ("poisson", ec.TWO_SEGMENTS, ec.TWO_SEGMENTS_BLOCKS, ec.TWO_SEGMENTS_ROWS)],
    ids=["gaussian-8200x4100", "poisson-8200x4100", "poisson-131080x272"])
def test_several_segments_per_wavefront(eng, fam, shape, blocks, rows):
    """8200 x 4100: 9 strips of 2, ..., 2, 1 segments.  131080 x 272: one strip of a whole segment and a segment of a single tile,
    more rows than one round of the row-maximum kernel.  Every output of every row has the bits of calls on blocks of rows that
    have one segment per wavefront, and the first, a middle and the ragged last tile of rows match long double."""
    import torch

    n, s, p = shape
    assert ec.launch_rule(n, s)[2] == 2 and all(ec.launch_rule(b - a, s)[2] == 1 for a, b in blocks)
    c, lw = device_model(fam, n, s, p, seed=ec.seed_of(fam, n, s))
    full = device_call(eng, c, lw)
    parts = [device_call(eng, c, lw, a, b) for a, b in blocks]
    assert int(full["n_pit_skipped"]) == 0
    for f in ec.FIELDS:
        whole, pieces = full[f], torch.cat([q[f] for q in parts])
        assert whole.shape == (n,) and bool(torch.isfinite(whole).all()), f
        assert torch.equal(whole.view(torch.int64), pieces.view(torch.int64)), f
    sub, eta, lw_rows = rows_on_host(eng, c, lw, rows)
    res = {f: host(full[f])[list(rows)] for f in ec.FIELDS}
    check_weighted(f"{fam} {n} x {s} rows of three tiles", fam, res, eta, sub, lw_rows)


# -------------------------------------------------------------------------------------------- 4. the small kernels' second rounds
def test_second_rounds_of_the_small_kernels(eng):
    """2 097 452 x 2, Gaussian, P = 1: more rows than 8192 x 256 threads of the combine kernel and than 16 384 x 4 wavefronts of the
    row maxima.  Every row's mean, second moment and PIT against long double (eta positive: two positive terms per sum)."""
    import torch

    n, s, p = ec.SECOND_ROUNDS
    assert ec.combine_rounds(n) == 2 and ec.rowmax_rounds(n) > 1
    g = torch.Generator(device="cuda").manual_seed(ec.seed_of("second rounds"))
    X = 1.0 + 0.5 * torch.rand(n, p, generator=g, device="cuda", dtype=torch.float64)
    offset = 0.5 + torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    beta = torch.tensor([[1.0], [1.3]], device="cuda", dtype=torch.float64)
    sigma = np.array([0.9, 1.2])
    y = X[:, 0] * 1.1 + offset + torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
    lw = 3.0 * torch.randn(n, s, generator=g, device="cuda", dtype=torch.float64)
    c = dict(family="gaussian", X=X, y=y, beta=beta, scale=cuda(sigma), trials=None, offset=offset, oc=None, dc=cuda(glm_ref.draw_const(sigma)))
    out = device_call(eng, c, lw)
    eta = host(eng.glm(X, beta, "linpred", offset=offset))
    assert eta.shape == (n, s) and eta.min() > 0.0
    res = {f: host(out[f]) for f in ec.FIELDS}
    hc = dict(y=host(y), scale=sigma, trials=None)
    check_weighted(f"gaussian {n} x {s}", "gaussian", res, eta, hc, host(lw))
    assert same_bits(res["pit_le"], res["pit_lt"])


# ----------------------------------------------------------------------------------------------- 5. weights that are not finite
def test_weights_that_are_not_finite(eng):
    """A NaN weight, a +inf weight and a row of -inf alone: those rows are NaN in all four outputs, as the restatement's are; every
    other row, their tile neighbours included, has the bits of the clean call -- from host and from device memory."""
    c, clean = ec.case("poisson", ec.S, ec.P), ec.weights(ec.N, ec.S, 0, 0.05)
    lw = clean.copy()
    lw[4, 100], lw[20, 7], lw[30] = np.nan, np.inf, -np.inf
    poisoned = np.isin(np.arange(ec.N), (4, 20, 30))
    eta = kernel_eta(eng, c)
    want, _ = ec.expected("poisson", eta, c["y"], None, None, lw)
    for f in ec.FIELDS:
        assert np.all(np.isnan(want[f][poisoned])) and np.all(np.isfinite(want[f][~poisoned])), f
    base = run(eng, c, clean)
    for put in (same, cuda):
        got = run(eng, c, lw, put=put)
        assert got["n_pit_skipped"] == 0
        for f in ec.FIELDS:
            assert np.all(np.isnan(got[f][poisoned])), f
            assert same_bits(got[f][~poisoned], base[f][~poisoned]), f
    check_weighted("poisson with poisoned weights", "poisson", got, eta, c, lw)


# -------------------------------------------------------------------------------------------------- 6. a non-finite row of X
@pytest.mark.parametrize("fam", ["gaussian", "poisson"])
def test_non_finite_rows_of_x(eng, fam):
    """NaN in one entry of X and inf in another, handed to the engine directly (the fronts reject them): only those rows change,
    and they are NaN / inf where the restatement on the kernel's eta is."""
    c, lw = ec.case(fam, ec.S, ec.P), ec.weights(ec.N, ec.S, 0, 0.05)
    X = c["X"].copy()
    X[6, 2], X[22, 1] = np.nan, np.inf
    bad = np.isin(np.arange(ec.N), (6, 22))
    base = run(eng, c, lw)
    eta = kernel_eta(eng, c, X=X)
    assert np.all(np.isnan(eta[6])) and np.all(np.isinf(eta[22])) and np.all(np.isfinite(eta[~bad]))
    want, terms = ec.expected(fam, eta, c["y"], c["scale"], c["trials"], lw)
    assert np.isnan(want["mean"][6]) and not np.isfinite(want["mean"][22])
    for put in (same, cuda):
        got = run(eng, c, lw, put=put, X=X)
        for f in ec.FIELDS:
            assert same_bits(got[f][~bad], base[f][~bad]), f
            check(f"{fam} non-finite X {f}", got[f], want[f], sum_bound(fam, lw, terms[f], want[f]))
        assert np.isnan(got["mean"][6]) and not np.isfinite(got["mean"][22])


# ---------------------------------------------------------------------------------------------------------------------- 7. layouts
def test_layouts(eng):
    """Device weights read in place at a padded pitch and at an odd element offset, transposed and padded X and beta in both memory
    spaces, a row list as a list and as a CUDA tensor: the bits of the contiguous call."""
    import torch

    c, lw = ec.case("poisson", ec.S, ec.P), ec.weights(ec.N, ec.S, 0, 0.05)
    n, s = lw.shape
    base = run(eng, c, lw, put=cuda)
    assert base["route"].endswith("(weights read in place)"), base["route"]
    assert run(eng, c, lw)["route"].endswith("(weights staged in blocks)")

    def padded(a, pad=3, shift=0):
        flat = torch.full((a.shape[0] * (a.shape[1] + pad) + shift,), float("nan"), dtype=torch.float64, device="cuda")
        view = flat[shift:].view(a.shape[0], a.shape[1] + pad)[:, :a.shape[1]]
        view.copy_(cuda(a))
        assert view.stride() == (a.shape[1] + pad, 1) and view.data_ptr() % 16 == (8 * shift) % 16
        return view

    kw = ec.engine_kwargs(c, cuda)
    variants = {
        "padded weights": dict(lw=padded(lw)), "padded weights at an odd offset": dict(lw=padded(lw, shift=1)),
        "X.T view": dict(X=cuda(c["X"].T).T), "beta.T view": dict(beta=cuda(c["beta"].T).T),
        "padded X and beta": dict(X=padded(c["X"], 2), beta=padded(c["beta"], 1, 1)),
    }
    for name, v in variants.items():
        out = eng.glm_predict(v.get("X", cuda(c["X"])), v.get("beta", cuda(c["beta"])), "poisson", log_weights=v.get("lw", cuda(lw)), **kw)
        if "weights" in name:
            assert eng.last_kernels().endswith("(weights read in place)"), name
        for f in ec.FIELDS:
            assert same_bits(host(out[f]), base[f]), (name, f)
    host_variants = {"X.T view": dict(X=np.asfortranarray(c["X"])), "beta.T view": dict(beta=np.asfortranarray(c["beta"])),
                     "padded X and beta": dict(X=np.pad(c["X"], ((0, 0), (0, 2)))[:, :ec.P], beta=np.pad(c["beta"], ((0, 0), (0, 1)))[:, :ec.P]),
                     "padded weights": dict(lw=np.pad(lw, ((0, 0), (0, 3)))[:, :s])}
    for name, v in host_variants.items():
        got = run(eng, dict(c, **{k: a for k, a in v.items() if k != "lw"}), v.get("lw", lw))
        for f in ec.FIELDS:
            assert same_bits(got[f], base[f]), (name, f)
    rows = [31, 2, 2, 17, 0, 32, 2]
    for listed, put in ((rows, same), (rows, cuda), (torch.as_tensor(rows, device="cuda"), cuda)):
        got = run(eng, c, lw[rows], put=put, rows=listed)
        for f in ec.FIELDS:
            assert same_bits(got[f], base[f][rows]), (type(listed), f)


# ------------------------------------------------------------------------------------------------------------------ 8. pit=False
@pytest.mark.parametrize("fam", ["poisson", "binomial"])
def test_without_pit(eng, fam):
    """``pit=False``: nothing is walked and nothing is skipped, even with a count of 4097 present; the moments are the bits of the
    ``pit=True`` call."""
    c, lw = ec.case(fam, ec.S, ec.P, True), ec.weights(ec.N, ec.S, 0, 0.05)
    y = c["y"].copy()
    y[ec.CAP_ROW] = 4097.0
    for put in (same, cuda):
        full = run(eng, c, lw, put=put, y=y)
        bare = run(eng, c, lw, put=put, y=y, pit=False)
        assert full["n_pit_skipped"] == 1 and bare["n_pit_skipped"] == 0
        assert bare["pit_le"] is None and bare["pit_lt"] is None
        assert np.all(np.isfinite(bare["mean"])) and np.all(np.isfinite(bare["m2"]))
        assert same_bits(bare["mean"], full["mean"]) and same_bits(bare["m2"], full["m2"])


# ---------------------------------------------------------------------------------------------- 9. the skipped counter over blocks
CHILD = r"""
import sys, warnings, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import glm_ref
import pyloo_amd as pl
from pyloo_amd.engine import get_engine
m = glm_ref.make_model(np.random.default_rng(11), 300, 1000, 5, "poisson", with_offset=True)
for r in (5, 140, 299):
    m["y"][r] = 4097.0
    m["offset"][r] += np.log(4097.0)
out = {}
for where, put in (("host", lambda a: a), ("device", lambda a: torch.as_tensor(a, device="cuda"))):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = pl.loo_glm_predict_from_design(put(m["X"]), put(m["y"]), put(m["beta"]), "poisson", offset=put(m["offset"]))
    for f in ("mean", "var", "pit_le", "pit_lt", "pareto_k", "elpd_i"):
        out[where + "_" + f] = getattr(r, f)
    out[where + "_skipped"] = np.array(r.n_pit_skipped)
    out[where + "_route"] = np.array(get_engine(0 if where == "device" else None).last_kernels())
np.savez(sys.argv[2], **out)
"""


def test_skipped_counter_over_blocks(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 (read once: a fresh child) cuts the 300 x 1000 fused pass into blocks of 131 rows; the counts of 4097 in
    rows 5, 140 and 299 lie in three of them.  ``n_pit_skipped`` is 3 and every output is the one-block run's, bit for bit, from host
    and from device memory."""
    assert len({r // ((1 << 20) // (1000 * 8)) for r in (5, 140, 299)}) == 3
    runs = []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        env.update(env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            runs.append({k: z[k] for k in z.files})
    assert "glm_predict_kernel" in str(runs[0]["device_route"]) and "per block of observations" in str(runs[1]["device_route"])
    for run_ in runs:
        for where in ("host", "device"):
            assert int(run_[where + "_skipped"]) == 3, where
            nan = np.isnan(run_[where + "_pit_le"])
            assert np.array_equal(np.flatnonzero(nan), [5, 140, 299]) and np.array_equal(nan, np.isnan(run_[where + "_pit_lt"]))
            assert np.all(np.isfinite(run_[where + "_mean"]))
    for k in runs[0]:
        if not k.endswith("route"):
            assert same_bits(runs[0][k], runs[1][k]), k
    # (host against device is the other file's: the fronts take -lgamma(y + 1) from scipy on the host and from torch on the device,
    # which agree on the small counts there and differ in the last place at 4097)
