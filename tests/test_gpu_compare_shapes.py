"""loo_compare's kernels (csrc/pla_compare.h) at the edges of their work layout, on the MI355X: groups of models over
blockIdx.y / .z, short, single-column and widened tiles, several bootstrap launches, pitched input, and the numerics of the
moments (Welford / Chan) and stacking passes.  The references are tests/compare_stream.py: ``moments_reference`` and
``stacking_reference`` in ``math.fsum`` / ``np.longdouble`` arithmetic, ``bb_z`` on the restated gamma stream.

Tolerances: 1e-12 relative (the tolerance of test_gpu_compare.py) on sums that cancel nothing, the derived bound of
``test_m2_of_ill_conditioned_differences``, and bit equality where the header's "Determinism" paragraph promises it."""

import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

from compare_cases import pointwise  # noqa: E402
from compare_stream import (NumpyCompareEngine, bb_z, bb_z_from_gammas, gamma_draws, moments_reference,  # noqa: E402
                            stacking_objective, stacking_reference)

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
SCALES = (("log", 1.0), ("negative_log", -1.0), ("deviance", -0.5))  # a table's scale and the scale_mul that brings it to "log"
KS = (1, 2, 8, 9, 16, 17, 32, 33, 64)  # around the groups of 8 (moments) and of 16 (stacking, bootstrap) models
NS = (1, 2, 63, 255, 256, 257, 1023, 1024, 1025, 3000)  # waves without a column, a full tile, one column in the last tile
LARGE_NS = (2_097_152, 2_097_153, 2_500_001)  # the last N of 1024-column tiles, the first of 1280-column ones (1639 tiles)
BS = (1, 63, 64, 65, 130)
ALPHAS = (1.0, 0.5, 2.0)
SEED = 0x00C0FFEE12345678  # (both key words of the Philox stream are non-zero)


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    e = get_engine()
    e.set_compare_grid(0)
    return e


def relerr(got, want):
    """max |got - want| / |want|, taken in longdouble (0 where both are 0)."""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.longdouble)), np.atleast_1d(np.asarray(want, dtype=np.longdouble))
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), np.longdouble(1e-300)))) if got.size else 0.0


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()  # (NaN == NaN here, -0.0 != 0.0)


@functools.lru_cache(maxsize=None)
def gammas(alpha, B, N):
    """The restated gamma draws of (SEED, alpha, b < B, i < N): they do not depend on the matrix, so every K shares them."""
    G = gamma_draws(SEED, alpha, B, N)
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=1)
def large_gammas(N):
    G = gamma_draws(SEED, 1.0, 2, N)
    G.setflags(write=False)
    return G


def check_moments(got, x, best, what):
    """``compare_moments`` against ``moments_reference``: row sums, M2 and the sum of the maxima to 1e-12 relative, the mean of
    d to 1e-12 * max(|mean|, std), and the entries of the best model's own difference exactly 0."""
    got = host(got)
    K, N = x.shape
    ref = moments_reference(x, best)
    assert got.shape == (3 * K + 1,)
    others = [k for k in range(K) if k != best]
    e_sum = relerr(got[0:3 * K:3], ref[0:3 * K:3])
    e_max = relerr(got[3 * K], ref[3 * K])
    e_m2 = relerr(got[2:3 * K:3][others], ref[2:3 * K:3][others])
    mean, std = ref[1:3 * K:3], np.sqrt(ref[2:3 * K:3] / N)
    scale = np.maximum(np.abs(mean), std)
    diff = np.abs(got[1:3 * K:3].astype(np.longdouble) - mean)
    e_mean = float(np.max(diff[others] / scale[others])) if others else 0.0
    print(f"{what}: sum {e_sum:.2e} max {e_max:.2e} M2 {e_m2:.2e} mean {e_mean:.2e}")
    assert e_sum <= 1e-12 and e_max <= 1e-12, (what, e_sum, e_max)
    assert e_m2 <= 1e-12, (what, e_m2)
    assert np.all(diff <= 1e-12 * scale), (what, diff, scale)
    assert got[3 * best + 1] == 0.0 and got[3 * best + 2] == 0.0, (what, got[3 * best + 1], got[3 * best + 2])


def check_stacking(got, x, w, s, what):
    """``stacking_eval`` against ``stacking_reference``: every term of F is <= 0 and every term of G_k >= 0, nothing cancels."""
    F, G = got
    Fr, Gr = stacking_reference(x, w, s)
    e_f, e_g = relerr(F, Fr), relerr(G, Gr)
    print(f"{what}: F {e_f:.2e} G {e_g:.2e}")
    assert G.shape == (x.shape[0],)
    assert e_f <= 1e-12 and e_g <= 1e-12, (what, e_f, e_g)


def condition(x, G=None):
    """The largest condition number sum|t| / |sum t| among the row sums of x and, with gamma draws G, among the bootstrap's
    numerators sum_i G_bi x_ki."""
    x = np.asarray(x, dtype=np.float64)
    cond = np.abs(x).sum(axis=1) / np.abs(x.sum(axis=1))
    if G is not None:
        cond = np.concatenate((cond, ((G @ np.abs(x).T) / np.abs(G @ x.T)).ravel()))
    return float(cond.max())


def case_of(K, N):
    """What varies from case to case instead of a full cross product: dtype, scale, the best model, and (with N) B and alpha."""
    ik, i_n = KS.index(K), NS.index(N)
    dtype = (np.float64, np.float32)[(ik + i_n) % 2]
    scale, s = SCALES[(ik + i_n) % 3]
    second_group = 9 if K > 9 else K // 2  # (a model of the moments pass's second group of 8 where there is one)
    best = (0, K - 1, second_group)[(ik + 2 * i_n) % 3]
    return dtype, scale, s, best, BS[i_n % 5], ALPHAS[i_n % 3]


# ---- 1. model groups x tile edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_model_groups_and_tile_edges(eng, K, N):
    dtype, scale, s, best, B, alpha = case_of(K, N)
    x = pointwise(1000 + 100 * KS.index(K) + NS.index(N), K, N, scale).astype(dtype)
    xd = cuda(x)
    G = gammas(alpha, B, N)
    # pointwise() has values of both signs, so a sum of one or two of them can cancel.  The worst of these cases has a
    # condition number of 1406 (K = 17, N = 2); a few roundings of 2^-53 on either side, 2000 times, stay below 1e-12.
    assert condition(x, G) < 2000
    what = f"K={K} N={N} {np.dtype(dtype).name} {scale} best={best} B={B} alpha={alpha}"
    check_moments(eng.compare_moments(x, best), x, best, what + " moments host")
    check_moments(eng.compare_moments(xd, best), x, best, what + " moments device")
    w = np.random.default_rng(7 * K + N).dirichlet(np.ones(K))
    assert np.all(w > 0)
    check_stacking(eng.stacking_eval(x, w, s), x, w, s, what + " stacking host")
    check_stacking(eng.stacking_eval(xd, w, s), x, w, s, what + " stacking device")
    z_host = eng.bb_bootstrap(x, B, alpha, SEED, s)
    z_dev = eng.bb_bootstrap(xd, B, alpha, SEED, s)
    e_z = relerr(z_host, bb_z_from_gammas(G, x, s))
    print(f"{what}: z {e_z:.2e}")
    assert z_host.shape == (B, K) and e_z <= 1e-12, (what, e_z)
    assert same_bits(z_host, z_dev), what


@pytest.mark.parametrize("K", (2, 3))
@pytest.mark.parametrize("N", LARGE_NS)
def test_model_groups_at_the_tile_width_threshold(eng, K, N):
    """Tiles widen from 1024 columns once N > 2 097 152.  The matrix is generated on the device by the recipe of
    ``compare_cases.pointwise``; every reference needs all of its K rows, which are copied back once."""
    import torch

    i_n = LARGE_NS.index(N)
    dtype = (torch.float64, torch.float32)[(K + i_n) % 2]
    scale, s = SCALES[(K + i_n) % 3]
    mul = {"log": 1.0, "negative_log": -1.0, "deviance": -2.0}[scale]
    best = (0, K - 1)[i_n % 2]
    g = torch.Generator(device="cuda").manual_seed(40 + 3 * i_n + K)
    common = torch.randn(N, device="cuda", dtype=torch.float64, generator=g)
    xd = torch.empty((K, N), device="cuda", dtype=dtype)
    for k in range(K):
        xd[k] = mul * (-1.2 - 0.08 / K * k + 0.6 * common + 0.5 * torch.randn(N, device="cuda", dtype=torch.float64, generator=g))
    del common
    x = xd.cpu().numpy()
    G = large_gammas(N)
    assert condition(x, G) < 2000
    what = f"K={K} N={N} {x.dtype.name} {scale} best={best}"
    check_moments(eng.compare_moments(xd, best), x, best, what + " moments")
    w = np.random.default_rng(K + i_n).dirichlet(np.ones(K))
    check_stacking(eng.stacking_eval(xd, w, s), x, w, s, what + " stacking")
    z_dev = eng.bb_bootstrap(xd, 2, 1.0, SEED, s)
    e_z = relerr(host(z_dev), bb_z_from_gammas(G, x, s))
    print(f"{what}: z {e_z:.2e}")
    assert e_z <= 1e-12, (what, e_z)
    assert same_bits(eng.bb_bootstrap(x, 2, 1.0, SEED, s), z_dev), what


# ---- 2. ill-conditioned differences ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (257, 50_001))
@pytest.mark.parametrize("c,s", ((1e3, 1e-1), (1e6, 1e-3)))
def test_m2_of_ill_conditioned_differences(eng, c, s, N):
    """Model 1 is the best one plus a constant plus small noise, so its difference d has |mean| / std = 1e4 or 1e9.

    Bound on M2, relative to the longdouble two-pass value: 16 * eps * (1 + |mean| / std).  An emulation of the kernel's order
    (Welford per lane, the xor butterfly of Chan merges, four waves, tiles in order) in NumPy stayed below
    2 * eps * (1 + |mean| / std) on every case tried, so the factor 16 leaves a margin of 8.  A one-pass sum of squares errs by
    about eps * (mean / std)^2: 2e-8 at (1e3, 1e-1), everything at (1e6, 1e-3), against bounds of 3.6e-11 and 3.6e-6.
    """
    best = 2
    x = pointwise(31, 3, N, "log")
    x[1] = x[best] + c + s * np.random.default_rng(32).normal(size=N)
    ref = moments_reference(x, best)
    mean, m2 = float(ref[3 + 1]), ref[3 + 2]
    std = float(np.sqrt(m2 / N))
    bound = 16 * EPS * (1 + abs(mean) / std)
    for name, xin in (("host", x), ("device", cuda(x))):
        got = host(eng.compare_moments(xin, best))
        err = relerr(got[3 + 2], m2)
        units = err / (EPS * (1 + abs(mean) / std))
        print(f"c={c:g} s={s:g} N={N} {name}: M2 error {err:.3e} = {units:.4f} eps (1 + |mean|/std), bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
        assert abs(got[3 + 1] - mean) <= 1e-12 * max(abs(mean), std)
        assert relerr(got[2], ref[2]) <= 1e-12 and got[3 * best + 2] == 0.0  # the ordinary model next to it
    # In units of eps * (1 + |mean| / std), against the bound's 16: a NumPy emulation of the kernel's order on these four inputs
    # gives 0.047 and 0.0026 at (1e3, 1e-1), 0.0042 and 0.0057 at (1e6, 1e-3), N = 257 and 50 001 (the rounding of d = x - x_best
    # itself accounts for most of it).  The figure of a run on an MI355X is what the print above shows; none is recorded here yet.


# ---- 3. stacking at the boundary, K = 1, NaN ---------------------------------------------------------------------------------------
def boundary_weights(K):
    """Every other weight exactly 0 (model 0 among them), the rest Dirichlet."""
    w = np.zeros(K)
    pos = np.arange(1, K, 2)
    w[pos] = np.random.default_rng(K).dirichlet(np.ones(pos.size))
    return w


@pytest.mark.parametrize("K", (5, 20))
def test_stacking_with_zero_weights(eng, K):
    """Weights on the boundary of the simplex: models of weight 0 are the column maximum in many columns, d stays positive."""
    x = pointwise(50 + K, K, 3000, "negative_log")
    w = boundary_weights(K)
    zero_is_max = np.isin(np.argmax(-x, axis=0), np.flatnonzero(w == 0))
    assert zero_is_max.sum() > 100 and (~zero_is_max).sum() > 100
    check_stacking(eng.stacking_eval(x, w, -1.0), x, w, -1.0, f"K={K} zero weights host")
    check_stacking(eng.stacking_eval(cuda(x), w, -1.0), x, w, -1.0, f"K={K} zero weights device")


def kinds(v):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 3, np.where(np.isposinf(v), 1, np.where(np.isneginf(v), 2, 0)))


# a column inside a tile, the first one of the last tile (which the masked lanes read again), the last one
@pytest.mark.parametrize("col", (1500, 2048, 2999))
@pytest.mark.parametrize("K", (5, 20))
def test_stacking_with_an_underflowing_mixture(eng, K, col):
    """In one column the only models of positive weight lie 800 below the maximum, whose weight is 0: exp(-800) == 0, d_i == 0,
    F is -inf, and G is exp(.) * (1 / d): inf for the models that did not underflow, NaN (0 * inf) for those that did."""
    x = pointwise(60 + K, K, 3000, "log")
    w = boundary_weights(K)
    x[w > 0, col] = x[0, col] - 800.0
    x[w == 0, col] = x[0, col] - np.arange(np.sum(w == 0))  # model 0 is the maximum, the other weightless ones a little below
    with np.errstate(divide="ignore", invalid="ignore"):
        F_ref, G_ref = NumpyCompareEngine().stacking_eval(x, w, 1.0)
    assert F_ref == -np.inf and set(kinds(G_ref)) == {1, 3}
    for xin in (x, cuda(x)):
        F, G = eng.stacking_eval(xin, w, 1.0)
        assert F == -np.inf
        assert np.array_equal(kinds(G), kinds(G_ref)), (G, G_ref)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_stacking_of_one_model(eng, dtype):
    """K = 1: e = 1 and d = w0 in every column, so F = N log w0 and G = N / w0."""
    N, w0 = 3000, 0.37
    x = pointwise(70, 1, N, "log").astype(dtype)
    for xin in (x, cuda(x)):
        F, G = eng.stacking_eval(xin, np.array([w0]), 1.0)
        assert relerr(F, N * np.log(np.longdouble(w0))) <= 1e-12 and relerr(G, [N / np.longdouble(w0)]) <= 1e-12, (F, G)


@pytest.mark.parametrize("K,j,best", ((5, 1, 3), (20, 17, 9)))
def test_a_nan_stays_in_its_model(eng, K, j, best):
    """A NaN in model j: its moments are NaN, those of every other model are bitwise what they are without it."""
    x = pointwise(80 + K, K, 3000, "log")
    clean = eng.compare_moments(x, best)
    x[j, 1234] = np.nan
    for xin in (x, cuda(x)):
        got = host(eng.compare_moments(xin, best))
        assert np.all(np.isnan(got[3 * j:3 * j + 3]))
        keep = np.ones(3 * K, dtype=bool)
        keep[3 * j:3 * j + 3] = False
        assert same_bits(got[:3 * K][keep], clean[:3 * K][keep])
        assert got[3 * best + 2] == 0.0


# ---- 4. several bootstrap launches -------------------------------------------------------------------------------------------------
def test_bootstrap_in_several_launches(eng):
    """The smallest shape at which the 64 MiB cap on the partials splits a call: the second launch starts at replicate b0 = 192
    and writes 8 replicates."""
    import torch

    K, N, B = 64, 516_097, 200
    tiles = -(-N // 1024)  # (N <= 2 097 152: tiles of 1024 columns)
    per_replicate = tiles * (K + 1) * 8
    nb = max(64, ((64 << 20) // per_replicate) // 64 * 64)
    assert tiles == 505 and nb == 192 and B > nb
    assert max(64, ((64 << 20) // (-(-(N - 1) // 1024) * (K + 1) * 8)) // 64 * 64) >= B  # one column fewer: one launch
    g = torch.Generator(device="cuda").manual_seed(5)
    xd = torch.empty((K, N), device="cuda", dtype=torch.float32)
    common = torch.randn(N, device="cuda", generator=g)
    for k in range(K):
        xd[k] = -1.2 - 0.08 / K * k + 0.6 * common + 0.5 * torch.randn(N, device="cuda", generator=g)
    z = host(eng.bb_bootstrap(xd, B, 1.0, SEED, 1.0))
    assert z.shape == (B, K) and np.all(np.isfinite(z))
    # a single-row call has K = 1 and fits in one launch; tiles depend on N alone and each model's sums are accumulated
    # independently, so it gives the bits of that model's column
    assert max(64, ((64 << 20) // (tiles * 2 * 8)) // 64 * 64) == 8256
    for k in (0, 15, 16, 63):
        assert same_bits(host(eng.bb_bootstrap(xd[k:k + 1], B, 1.0, SEED, 1.0))[:, 0], z[:, k]), k
    # the replicates on either side of the boundary, against the restated stream
    reps, models = np.array([0, 191, 192, 199]), [0, 63]
    rows = xd[models].cpu().numpy()
    e_z = relerr(z[np.ix_(reps, models)], bb_z(rows, B, 1.0, SEED, 1.0, replicates=reps))
    print(f"replicates {reps.tolist()} of models {models}: z {e_z:.2e}")
    assert condition(rows) < 2000 and e_z <= 1e-12, e_z
    # a grid cap changes nothing
    try:
        eng.set_compare_grid(37)
        assert same_bits(eng.bb_bootstrap(xd, B, 1.0, SEED, 1.0), z)
    finally:
        eng.set_compare_grid(0)
    # the host path, which reuses one output buffer between the launches
    xh = xd.cpu().numpy()
    del xd
    assert same_bits(eng.bb_bootstrap(xh, B, 1.0, SEED, 1.0), z)


# ---- 5. pitched input, grid independence beyond one group --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_pitched_input(eng, dtype):
    """Rows of a wider buffer (pitch N + 7, first element 3 in: not 16-byte aligned) give the bits of the contiguous copy."""
    K, N = 17, 3001
    x = pointwise(90, K, N, "deviance").astype(dtype)
    w = np.random.default_rng(91).dirichlet(np.ones(K))
    want = (eng.compare_moments(x, 16), eng.stacking_eval(x, w, -0.5), eng.bb_bootstrap(x, 65, 0.5, SEED, -0.5))
    wide = np.full((K, N + 7), np.nan, dtype=dtype)
    wide[:, 3:3 + N] = x
    wide_d = cuda(wide)
    for view in (wide[:, 3:3 + N], wide_d[:, 3:3 + N]):
        assert (view.stride(0) if hasattr(view, "stride") else view.strides[0] // view.itemsize) == N + 7
        got = (eng.compare_moments(view, 16), eng.stacking_eval(view, w, -0.5), eng.bb_bootstrap(view, 65, 0.5, SEED, -0.5))
        assert same_bits(got[0], want[0])
        assert got[1][0] == want[1][0] and same_bits(got[1][1], want[1][1])
        assert same_bits(got[2], want[2])
    assert same_bits(host(wide_d), wide)  # (nothing wrote into the buffer)


def test_results_do_not_depend_on_the_grid_beyond_one_group(eng):
    x = cuda(pointwise(6, 33, 300_000, "log"))
    w = np.random.default_rng(33).dirichlet(np.ones(33))
    outs = []
    try:
        for cap in (0, 3, 37):
            eng.set_compare_grid(cap)
            outs.append((host(eng.compare_moments(x, 20)), eng.stacking_eval(x, w, -1.0), host(eng.bb_bootstrap(x, 130, 0.7, 42, 1.0))))
    finally:
        eng.set_compare_grid(0)
    for o in outs[1:]:
        assert same_bits(o[0], outs[0][0])
        assert o[1][0] == outs[0][1][0] and same_bits(o[1][1], outs[0][1][1])
        assert same_bits(o[2], outs[0][2])


# ---- 6. the front at K > 16 ----------------------------------------------------------------------------------------------------------
def with_numpy_engine(monkeypatch, call):
    import pyloo_amd.compare as cmp

    fake = NumpyCompareEngine()
    with monkeypatch.context() as m:
        m.setattr(cmp, "get_engine", lambda device=None: fake)
        return call()


@pytest.mark.parametrize("K,scale", ((17, "deviance"), (33, "negative_log")))
def test_stacking_weights_beyond_one_group(monkeypatch, eng, K, scale):
    """The objective at the device's weights is no worse than at the NumPy engine's.  (Not the weights themselves: with this
    many correlated models the optimum is flat.)"""
    import pyloo_amd as pl

    x = pointwise(100 + K, K, 3000, scale)
    s = dict(SCALES)[scale]
    w, _ = pl.compare_weights(x, method="stacking", scale=scale)
    w_ref, _ = with_numpy_engine(monkeypatch, lambda: pl.compare_weights(x, method="stacking", scale=scale))
    f_dev, f_ref = stacking_objective(x, w, s), stacking_objective(x, w_ref, s)
    print(f"K={K}: f_dev - f_ref = {f_dev - f_ref:.3e} (f_ref {f_ref:.6f}), max |w - w_ref| = {np.max(np.abs(w - w_ref)):.2e}")
    assert f_dev <= f_ref + 1e-6 * abs(f_ref) + 1e-12, (f_dev, f_ref)
    assert w.shape == (K,) and np.all(w >= 0) and abs(w.sum() - 1.0) <= 1e-12


def test_bb_weights_beyond_one_group(monkeypatch, eng):
    """The stream is specified, so the device's weights and standard errors are those of the NumPy engine, to 1e-10 relative:
    two orders above the 1e-12 asked of z, of which they are a softmax and a mean over the replicates."""
    import pyloo_amd as pl

    x = pointwise(117, 17, 3000, "log", "close")
    kw = dict(method="bb-pseudo-bma", b_samples=200, alpha=1.0, seed=77, scale="log")
    w, ses = pl.compare_weights(x, **kw)
    w_ref, ses_ref = with_numpy_engine(monkeypatch, lambda: pl.compare_weights(x, **kw))
    e_w, e_ses = relerr(w, w_ref), relerr(ses, ses_ref)
    print(f"weights: rel {e_w:.2e} abs {np.max(np.abs(w - w_ref)):.2e} (smallest {w_ref.min():.2e}); ses: rel {e_ses:.2e}")
    assert e_w <= 1e-10 and e_ses <= 1e-10, (e_w, e_ses)
    assert abs(w.sum() - 1.0) <= 1e-12
