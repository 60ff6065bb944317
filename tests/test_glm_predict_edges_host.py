"""CPU half of the edge suite of ``loo_glm_predict``: the launch rule restated in tests/glm_predict_edge_cases.py yields the regimes
tests/test_gpu_loo_glm_predict_edges.py aims its shapes at, and the case builders' inputs are fit for a comparison -- on the NumPy
restatement alone, no GPU and no package import."""

import numpy as np
import pytest

import glm_predict_edge_cases as ec
import glm_predict_ref as ref


# ----------------------------------------------------------------------------------------------------------------- the launch rule
def test_launch_rule_gives_the_regimes_the_gpu_shapes_are_named_after():
    # (row_tiles, n_seg, strip_segs, n_strips, last_strip_segs)
    assert ec.launch_rule(8200, 4100) == (513, 17, 2, 9, 1)         # two segments per wavefront, a ragged last strip
    assert ec.launch_rule(4100, 4100)[2] == 1
    assert ec.launch_rule(131080, 272) == (8193, 2, 2, 1, 2)        # one strip of two segments
    assert ec.launch_rule(32770, 272)[2] == 1
    assert (272 - 16 * ec.SEG) == ec.TILE                           # ... the second of them a single tile of draws
    assert ec.launch_rule(200000, 4000)[1:] == (16, 16, 1, 16)      # the benchmark's shape: whole rows


def test_the_gpu_files_shapes_are_these():
    n, s, _ = ec.STRIPS
    assert ec.launch_rule(n, s)[2:] == (2, 9, 1)
    assert all(ec.launch_rule(b - a, s)[2] == 1 for a, b in ec.STRIPS_BLOCKS)
    assert ec.STRIPS_BLOCKS[0][0] == 0 and ec.STRIPS_BLOCKS[-1][1] == n and ec.STRIPS_BLOCKS[0][1] == ec.STRIPS_BLOCKS[1][0]
    assert max(ec.STRIPS_ROWS) == n - 1 and n % ec.TILE != 0
    n, s, _ = ec.TWO_SEGMENTS
    assert ec.launch_rule(n, s)[1:] == (2, 2, 1, 2) and n % ec.TILE != 0 and max(ec.TWO_SEGMENTS_ROWS) == n - 1
    assert all(b - a <= 32770 and ec.launch_rule(b - a, s)[2] == 1 for a, b in ec.TWO_SEGMENTS_BLOCKS)
    assert [a for a, _ in ec.TWO_SEGMENTS_BLOCKS][1:] == [b for _, b in ec.TWO_SEGMENTS_BLOCKS][:-1] and ec.TWO_SEGMENTS_BLOCKS[-1][1] == n
    assert n > 65536 and ec.rowmax_rounds(n) == 3 and ec.combine_rounds(n) == 1   # (it wraps the row maxima as well)
    # the smallest size that has more than one segment per wavefront: row_tiles * n_seg > 8192
    assert n * s > 8192 * 16 * 256 and ec.STRIPS[0] * ec.STRIPS[1] > 8192 * 16 * 256
    # every small case has one segment per wavefront
    for s in ec.MIXED_DRAWS + (250, 1000):
        assert ec.launch_rule(ec.N, s)[2] == 1
    assert [ec.launch_rule(ec.N, s)[1] for s in ec.MIXED_DRAWS] == [1, 2, 2]


def test_second_round_conditions_of_the_small_kernels():
    assert ec.ROWMAX_GRID * ec.ROWMAX_ROWS == 65536 and ec.COMBINE_GRID * ec.COMBINE_ROWS == 2097152
    assert ec.rowmax_rounds(65536) == 1 and ec.rowmax_rounds(65537) == 2
    assert ec.combine_rounds(2097152) == 1 and ec.combine_rounds(2097153) == 2
    n = ec.SECOND_ROUNDS[0]
    assert n > 2097152 and ec.combine_rounds(n) == 2 and ec.rowmax_rounds(n) > 2 and n % ec.COMBINE_ROWS != 0 and n % ec.TILE != 0
    assert ec.launch_rule(n, ec.SECOND_ROUNDS[1])[1:] == (1, 1, 1, 1)


def test_chunk_routes_of_the_predictor_counts():
    assert [ec.chunks(p) for p in ec.PREDICTORS] == [(1, False), (2, False), (4, False), (8, False), (8, True)]


# ------------------------------------------------------------------------------------------------------------------- the builders
def builder_cases():
    for fam in ec.FAMILIES:
        for p in ec.PREDICTORS:
            yield fam, 250, p, False
        yield fam, ec.S, ec.P, False
    for fam in ec.DISCRETE:
        for s in ec.MIXED_DRAWS:
            yield fam, s, ec.P, True


REFERENCE = {}


def reference(fam, s, p, planted):
    key = (fam, s, p, planted)
    if key not in REFERENCE:
        c = ec.case(fam, s, p, planted)
        lw = ec.weights(ec.N, s, 0, 0.05)
        eta = ec.eta_of(c)
        REFERENCE[key] = (c, eta) + ec.expected(fam, eta, c["y"], c["scale"], c["trials"], lw)
    return REFERENCE[key]


@pytest.mark.parametrize("fam,s,p,planted", list(builder_cases()))
def test_builders_references_are_finite_and_their_pit_values_inside_the_unit_interval(fam, s, p, planted):
    c, _, want, terms = reference(fam, s, p, planted)
    for f in ec.fields_of(fam):
        assert np.all(np.isfinite(want[f])) and np.all(np.isfinite(terms[f])), f
    assert np.all(c["y"] <= ref.MAX_COUNT) or fam in ("gaussian", "gamma")
    if fam in ec.DISCRETE:
        ok = ec.inside(want["pit_le"], want["pit_lt"])
        print(fam, s, p, planted, "rows inside (0, 1):", ok.sum(), "of", ok.size)
        assert 2 * ok.sum() >= ok.size
        if planted:
            assert all(ok[r] for r in ec.INSIDE_ROWS[fam]), [(r, want["pit_lt"][r], want["pit_le"][r]) for r in ec.INSIDE_ROWS[fam]]


@pytest.mark.parametrize("fam,s,p,planted", [k for k in builder_cases() if k[0] in ("gaussian", "poisson")])
def test_relative_bound_of_the_gaussian_and_poisson_sums_is_attainable(fam, s, p, planted):
    """1e-12 |W(term)| is at least the bound (S + 4) 2^-53 W(|term|) of a sum in any order: no cancellation in these inputs."""
    c, _, want, terms = reference(fam, s, p, planted)
    lw = ec.weights(ec.N, s, 0, 0.05)
    for f in ec.FIELDS:
        mag = ref.weighted(lw, [np.abs(terms[f])])[0]
        assert np.all(1e-12 * np.abs(want[f]) >= (s + 4) * 2.0 ** -53 * mag), f


@pytest.mark.parametrize("fam", ec.DISCRETE)
def test_planted_rows_are_where_the_module_says(fam):
    c = ec.case(fam, ec.S, ec.P, True)
    y, t = c["y"], c["trials"]
    if fam in ec.BINOMIAL:
        assert all((y[r], t[r]) == v for r, v in ec.PLANT_BINOMIAL.items()) and t.max() == 8192.0 and np.sum(t > 4096.0) == 1
        _, _, want, _ = reference(fam, ec.S, ec.P, True)
        assert want["pit_le"][17] == 1.0 and 0.0 < want["pit_lt"][17] < 1.0    # y = trials: the end of the support
        assert want["pit_lt"][21] == 0.0 and 0.0 < want["pit_le"][21] < 1.0    # y = 0
    else:
        assert all(y[r] == v for r, v in ec.PLANT_LOG.items())
    rows = sorted(ec.PLANT_LOG)
    assert rows == [17, 21, 25, 29] and all(r // ec.TILE == 1 and r % 4 == 1 for r in rows)  # one tile, one lane's four rows
    assert y[ec.CAP_ROW] == ref.MAX_COUNT and sorted(y[rows]) == [0.0, 1.0, 200.0, 4096.0]
    others = np.setdiff1d(np.arange(ec.TILE, 2 * ec.TILE), rows + [18])
    assert y[others].max() < 30.0


@pytest.mark.parametrize("fam,s,p,planted", [k for k in builder_cases() if k[0] != "gamma" and (k[3] or k[2] == ec.P)])
def test_distribution_functions_are_scipys_on_the_builders_eta(fam, s, p, planted):
    c, eta, _, terms = reference(fam, s, p, planted)
    s_le, s_lt = ref.scipy_cdf(fam, eta, c["y"], c["scale"], c["trials"])
    for name, got, want in (("pit_le", terms["pit_le"], s_le), ("pit_lt", terms["pit_lt"], s_lt)):
        err = np.abs(got - want)
        print(fam, s, planted, name, "against scipy:", err.max(), "at row", np.unravel_index(err.argmax(), err.shape)[0])
        assert err.max() <= 1e-10, (fam, name, err.max())


def test_weighted_bound_is_the_convex_combination_plus_the_summation_term():
    c, _, want, terms = reference("negbinomial", ec.S, ec.P, True)
    lw = ec.weights(ec.N, ec.S, 0, 0.05)
    b = ref.weighted_bound(lw, terms["mean"])
    t = np.abs(terms["mean"])
    assert np.all(b >= 1e-10 * np.maximum(1.0, t).min(axis=1)) and np.all(b <= 1.0001e-10 * np.maximum(1.0, t).max(axis=1) + 1e-13 * t.max(axis=1))
    hot = ref.weighted_bound(ref.one_hot(ec.N, ec.S, 7), terms["mean"])
    np.testing.assert_allclose(hot, 1e-10 * np.maximum(1.0, t[:, 7]) + (ec.S + 4) * 2.0 ** -53 * t[:, 7], rtol=1e-12)
