"""The inputs of tests/test_gpu_nonfactor_edges.py (tests/nonfactor_edge_cases.py) on the CPU alone, without a GPU: the properties
that make the comparison on the GPU meaningful.

(a) ``pivoting_draws``: LAPACK's partial pivoting swaps at least N / 4 rows of every draw at N >= 16 (and of one draw at least at
    N = 2, 3), so the LU kernel's swap loop, ``perm`` / ``qinv`` and the off-diagonal gather run; the restatement flags nothing
    and every row of both models is finite; a gather through the permutation in place of its inverse moves some c_i by more
    than 1 %.
(b) ``decline_batch``: a column Cholesky with the kernel's pivot rule stops at column m of the planted draw and nowhere in its
    neighbours; every |c_i| of the planted draw's inverse is above 1e-6, so which entries are clamped does not hang on rounding.
(c) ``mixed_batch``: the restatement's status words are the ones each draw is named after; the two asymmetric draws lie on either
    side of kNfSymTol by two decades.
(d) every matrix the GPU file compares values on has a 2-norm condition number of at most 1e3, the bound under which the
    project's tolerances (1e-9 below N = 500, 1e-8 above) were set.
(e) at N <= 300 the restatement (numpy.linalg.inv in f64) agrees to 1e-11 with a Gauss-Jordan inverse in 80-bit long double put
    through the same formulas: the reference itself is right on non-symmetric input.
(f) scaling: the restatement on (cov c, y sqrt c, mu sqrt c) is finite and equals the unscaled one minus 1/2 log c within 5e-14,
    and the relative pivot rule declines nothing at c = 1e-100, where an absolute threshold would decline every column."""

import numpy as np
import pytest

import nonfactor_edge_cases as ec
import nonfactor_ref as nr
from test_gpu_nonfactor import spd_draws

LD_TOL = 1e-11


def wide(inp):
    return [np.asarray(a, dtype=np.float64) for a in inp]


def assert_conditioned(mats, what):
    worst = max(ec.cond(m) for m in mats)
    assert worst <= ec.COND_BOUND, (what, worst)
    return worst


def rel_dev(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.float64)
    m = np.isfinite(b)
    assert np.array_equal(np.isfinite(a.astype(np.float64)), m)
    return float(np.max(np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m])))) if m.any() else 0.0


def assert_long_double(inp, refs, draws, what):
    """(e) for the finite, non-singular ``draws`` of ``inp``."""
    y, mu, mat, df = wide(inp)
    worst = 0.0
    for s in draws:
        P = ec.inverse_longdouble(mat[s])
        for model in ec.MODELS:
            if model == "student_t" and df[s] <= 0:
                continue
            worst = max(worst, rel_dev(ec.loglik_longdouble(y, mu[s], P, df[s], model), refs[model][0][:, s]))
    assert worst <= LD_TOL, (what, worst)
    return worst


def test_long_double_is_wider():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("N,dtype", [(N, "f8") for N in sorted(set(ec.PIVOT_N + ec.PIVOT_AUTO_N))] + [(N, "f4") for N in ec.PIVOT_F32_N])
def test_pivoting_draws(N, dtype):
    inp, refs = ec.pivot_case(N, dtype)
    y, mu, mat, df = wide(inp)
    assert mat.shape == (ec.pivot_s(N), N, N)
    swaps = [ec.swap_count(a) for a in mat]
    print(f"SWAPS N={N} {dtype} seed={ec.PIVOT_SEED[N]} " + " ".join(map(str, swaps)))
    if N >= 16:
        assert min(swaps) >= N / 4, swaps
    elif N > 1:
        assert max(swaps) >= 1, swaps
    if N > 1:
        assert all(not np.array_equal(a, a.T) for a in mat)
    if 16 <= N <= 513:  # the gather through q = qinv gives diag(a^-1); through perm instead it is off by far more than any tolerance
        for a in mat[:1]:
            c = np.diag(np.linalg.inv(a))
            np.testing.assert_allclose(ec.lu_gather(a), c, rtol=1e-9)
            assert np.max(np.abs(ec.lu_gather(a, inverse_permutation=False) - c) / c) > 1e-2
    assert_conditioned(mat, ("pivoting", N, dtype))
    for model in ec.MODELS:
        ll, fl = refs[model]
        assert not fl.any() and np.isfinite(ll).all(), (N, model)
    if N <= 300:
        worst = assert_long_double(inp, refs, range(mat.shape[0]), ("pivoting", N, dtype))
        print(f"LONGDOUBLE pivoting N={N} {dtype} {worst:.3e}")


def test_pivoting_launch_batch():
    """The 4100 3 x 3 draws of the launch-edge test: the same conditions, and rows that swap in a good share of them.  With three
    observations and a non-symmetric inverse a few Student-t entries have df + beta_i < 0 (sigma_i < 0, a NaN): the GPU test
    compares them as the front leaves them (-inf on both sides), and here none of them hangs on rounding."""
    inp = ec.pivoting_draws(ec.LAUNCH_N, ec.LAUNCH_S, ec.LAUNCH_SEED)
    refs = ec.references(inp)
    y, mu, mat, df = inp
    assert float(np.linalg.cond(mat).max()) <= ec.COND_BOUND
    assert sum(ec.swap_count(a) > 0 for a in mat) >= ec.LAUNCH_S // 4
    assert not refs["normal"][1].any() and np.isfinite(refs["normal"][0]).all()
    assert not refs["student_t"][1].any()
    P = np.linalg.inv(mat)
    r = y[None] - mu
    g = np.einsum("sij,sj->si", P, r)
    c = np.einsum("sii->si", P)
    assert c.min() > 0
    num = df[:, None] + np.einsum("si,si->s", r, g)[:, None] - g**2 / c
    assert np.abs(num).min() > 1e-4
    assert np.array_equal(np.isnan(refs["student_t"][0]), (num < 0).T) and not np.isinf(refs["student_t"][0]).any()
    assert 0 < (num < 0).sum() < 100
    spd = spd_draws(ec.LAUNCH_N, ec.LAUNCH_S, ec.LAUNCH_SEED)
    assert float(np.linalg.cond(spd[2]).max()) <= ec.COND_BOUND
    assert ec.LAUNCH_S > 2 * ec.LDS_GRID and ec.LAUNCH_S > 8 * ec.WS_SLOTS  # every workgroup takes several draws


@pytest.mark.parametrize("N", ec.PANEL_N)
def test_panel_draws(N):
    """SPD draws of the blocked route: (d), clean status words, and below N = 200 a Cholesky that declines no column (above, the
    bound on the condition number says so: a pivot below N eps C_jj needs a condition number of 1 / (N eps) > 1e12)."""
    for S in ec.panel_s(N):
        inp, refs = ec.panel_case(N, S)
        assert_conditioned(inp[2], ("panel", N, S))
        for model in ec.MODELS:
            ll, fl = refs[model]
            assert not fl.any() and np.isfinite(ll).all(), (N, S, model)
        if N < 200:
            assert all(ec.cholesky_decline_column(c) is None for c in inp[2])


def test_panel_counts_cover_the_wave_edges():
    """nb = 1, 2, 3, 5 panels (fewer tiles than the four waves, as many, one more), a whole and a padded last panel around
    N = 16 k, and 63 / 64 panels at the top."""
    nb = {N: -(-N // ec.TILE) for N in ec.PANEL_N}
    assert {1, 2, 3, 5, 9, 10, 63, 64} <= set(nb.values())
    assert {N % ec.TILE for N in ec.PANEL_N} >= {15, 0, 1}
    for k16 in (32, 144):
        assert {k16 - 1, k16, k16 + 1} <= set(ec.PANEL_N)


@pytest.mark.parametrize("N", sorted(ec.DECLINE_M))
def test_declining_at(N):
    worst_ld = 0.0
    for m in ec.DECLINE_M[N]:
        inp = ec.decline_batch(N, m, ec.DECLINE_SEED[N])
        y, mu, cov, df = inp
        one = ec.declining_at(N, m, ec.DECLINE_SEED[N])
        assert np.array_equal(one[2][0], cov[1]) and np.array_equal(one[1][0], mu[1]) and np.array_equal(one[0], y)
        assert [ec.cholesky_decline_column(c) for c in cov] == [None, m, None], (N, m)
        assert np.array_equal(cov[1], cov[1].T)
        assert_conditioned(cov, ("decline", N, m))
        c = np.diag(np.linalg.inv(cov[1]))
        assert np.abs(c).min() > 1e-6 and (c <= 0).any(), (N, m, np.abs(c).min())
        refs = ec.references(inp)
        for model in ec.MODELS:
            ll, fl = refs[model]
            assert fl.tolist() == [0, nr.CLAMPED, 0], (N, m, model, fl)
            assert np.isfinite(ll[:, [0, 2]]).all()
        assert np.isfinite(refs["normal"][0]).all()
        assert np.array_equal(np.isnan(refs["student_t"][0][:, 1]), c <= 0)  # sigma_i < 0 at the clamped entries
        worst_ld = max(worst_ld, assert_long_double(inp, refs, range(3), ("decline", N, m)))
    print(f"LONGDOUBLE decline N={N} {worst_ld:.3e}")
    assert {m % ec.TILE for m in ec.DECLINE_M[N]} >= {0, 1, 15} and N - 1 in ec.DECLINE_M[N]
    if N > ec.LDS_MAX_OBS:  # a later panel, the padded last panel (144 .. 159 holds 6 real columns), the last real column
        assert N % ec.TILE != 0 and {100, 143, 144, N - 1} <= set(ec.DECLINE_M[N]) and 144 // ec.TILE == (N - 1) // ec.TILE


def rel_asym(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(a - a.T) / np.maximum(np.abs(a), np.abs(a.T))
    return float(np.nanmax(np.where(np.isfinite(q), q, 0.0)))


@pytest.mark.parametrize("N", ec.MIXED_N)
def test_mixed_batch(N):
    inp = ec.mixed_batch(N, ec.MIXED_SEED[N])
    y, mu, mat, df = inp
    assert mat.shape == (12, N, N)
    refs = ec.references(inp)
    want = {"normal": np.zeros(12, dtype=np.int32), "student_t": np.zeros(12, dtype=np.int32)}
    for model in ec.MODELS:
        t = model == "student_t"
        want[model][ec.MIXED_NAN] = nr.NONFINITE | (nr.BETA_NONFINITE if t else 0)
        want[model][ec.MIXED_INF_MU] = nr.NONFINITE | (nr.BETA_NONFINITE if t else 0)
        want[model][ec.MIXED_SINGULAR] = nr.SINGULAR
        want[model][ec.MIXED_DF] = nr.DF_NONPOS if t else 0
        want[model][ec.MIXED_DECLINE] = nr.CLAMPED
        assert np.array_equal(refs[model][1], want[model]), (model, refs[model][1])
    # the NaN sits above the diagonal only; the two asymmetric draws straddle the tolerance
    assert np.isnan(mat[ec.MIXED_NAN]).sum() == 1 and np.isnan(np.triu(mat[ec.MIXED_NAN], 1)).sum() == 1
    assert rel_asym(mat[ec.MIXED_ASYM]) > 50 * ec.SYM_TOL and 0 < rel_asym(mat[ec.MIXED_NEAR_SYM]) < ec.SYM_TOL / 50
    plain = [s for s in range(12) if s not in (ec.MIXED_NAN, ec.MIXED_ASYM, ec.MIXED_DECLINE, ec.MIXED_SINGULAR, ec.MIXED_NEAR_SYM)]
    assert all(rel_asym(mat[s]) == 0.0 for s in plain)
    # the draws a Cholesky declines: column m of the planted one, the zero column of the singular one, no other
    declines = {s: ec.cholesky_decline_column(np.tril(mat[s]) + np.tril(mat[s], -1).T) for s in range(12) if s != ec.MIXED_NAN}
    assert declines.pop(ec.MIXED_DECLINE) == ec.MIXED_DECLINE_M[N] and declines.pop(ec.MIXED_SINGULAR) == 4
    assert all(v is None for v in declines.values())
    invertible = [s for s in range(12) if s not in (ec.MIXED_NAN, ec.MIXED_SINGULAR)]
    assert_conditioned(mat[invertible], ("mixed", N))
    c = np.diag(np.linalg.inv(mat[ec.MIXED_DECLINE]))
    assert np.abs(c).min() > 1e-6
    # inside the tolerance the asymmetry moves the restatement by at most 5e-15
    sym = [a.copy() for a in inp]
    sym[2][ec.MIXED_NEAR_SYM] = np.tril(mat[ec.MIXED_NEAR_SYM]) + np.tril(mat[ec.MIXED_NEAR_SYM], -1).T
    srefs = ec.references(sym)
    for model in ec.MODELS:
        a, b = refs[model][0][:, ec.MIXED_NEAR_SYM], srefs[model][0][:, ec.MIXED_NEAR_SYM]
        assert np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))) <= 5e-15
    worst = assert_long_double(inp, refs, [s for s in invertible if s != ec.MIXED_INF_MU], ("mixed", N))
    print(f"LONGDOUBLE mixed N={N} {worst:.3e}")
    # a NaN in y: every draw non-finite
    refs = ec.references(ec.nan_y_batch(N, ec.MIXED_SEED[N]))
    assert np.all(refs["normal"][1] == nr.NONFINITE) and np.all(refs["student_t"][1] == nr.NONFINITE | nr.BETA_NONFINITE)
    assert all(np.all(np.isneginf(refs[m][0])) for m in ec.MODELS)


def absolute_rule_declines(c, threshold=1e-30):
    a = np.array(c, dtype=np.float64)
    for j in range(a.shape[0]):
        if not a[j, j] > threshold:
            return True
        col = a[j + 1:, j] / np.sqrt(a[j, j])
        a[j + 1:, j + 1:] -= np.outer(col, col)
    return False


@pytest.mark.parametrize("N", ec.SCALE_N)
def test_scaled(N):
    base = spd_draws(N, 4, seed=N)
    assert_conditioned(base[2], ("scale", N))
    brefs = ec.references(base)
    for c in ec.SCALES:
        inp = ec.scaled(base, c)
        assert all(np.isfinite(a).all() for a in inp)
        assert_conditioned(inp[2], ("scale", N, c))
        assert all(ec.cholesky_decline_column(m) is None for m in inp[2])
        refs = ec.references(inp)
        for model in ec.MODELS:
            ll, fl = refs[model]
            assert not fl.any() and np.isfinite(ll).all()
            want = brefs[model][0] - 0.5 * np.log(c)
            assert np.max(np.abs(ll - want) / np.maximum(1.0, np.abs(want))) <= 5e-14, (N, c, model)
    assert all(absolute_rule_declines(m) for m in ec.scaled(base, 1e-100)[2])


@pytest.mark.parametrize("N", ec.SCALE_N)
def test_f32_ulp_batch(N):
    inp = ec.f32_ulp_batch(N, seed=N)
    mat = inp[2]
    assert mat.dtype == np.float32
    asym = [rel_asym(a.astype(np.float64)) for a in mat]
    assert asym[0] == asym[1] == asym[3] == 0.0 and 2.0 ** -24 <= asym[2] <= 2.0 ** -23 and asym[2] > 1e4 * ec.SYM_TOL
    assert_conditioned(mat, ("ulp", N))
    refs = ec.references(inp)
    for model in ec.MODELS:
        assert not refs[model][1].any() and np.isfinite(refs[model][0]).all()


@pytest.mark.parametrize("N", (17, 150))
def test_stride_batch(N):
    inp = ec.stride_batch(N, seed=N)
    refs = ec.references(inp)
    assert_conditioned(inp[2][[0, 2, 3, 4]], ("stride", N))
    assert rel_asym(inp[2][3]) > 1e-3
    assert refs["normal"][1].tolist() == [0, nr.NONFINITE, 0, 0, 0]
    assert refs["student_t"][1].tolist() == [0, nr.NONFINITE | nr.BETA_NONFINITE, 0, 0, 0]
    assert all(np.isfinite(np.delete(refs[m][0], 1, axis=1)).all() for m in ec.MODELS)
    # both strided layouts keep every written element inside their buffer and apart from one another
    S = 5
    for so, sd, size in ((1, N + 3, S * (N + 3)), (2 * S, 2, N * 2 * S)):
        idx = np.arange(N)[:, None] * so + np.arange(S)[None] * sd
        assert idx.max() < size and np.unique(idx).size == N * S and idx.size < size


@pytest.mark.parametrize("N,S,dtype", ec.BLOCK_CASES)
def test_block_batch(N, S, dtype):
    """PLA_INGEST_BLOCK_MB = 1: a block of 2^20 bytes holds one N x N matrix and no second one."""
    inp = ec.block_batch(N, S, dtype)
    item = np.dtype(ec.DTYPES[dtype]).itemsize
    assert inp[2].dtype == ec.DTYPES[dtype] and (S == 1 or max(1, (1 << 20) // (N * N * item)) == 1)
    assert_conditioned(inp[2], ("block", N, S, dtype))
    refs = ec.references(inp)
    for model in ec.MODELS:
        assert not refs[model][1].any() and np.isfinite(refs[model][0]).all()
    if S > 1:
        assert rel_asym(inp[2][1].astype(np.float64)) > 0.1 and all(rel_asym(inp[2][s].astype(np.float64)) == 0 for s in (0, 2))
