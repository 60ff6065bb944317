"""The three WAIC kernels (csrc/pla_waic.h) at the edges of their bookkeeping, each against tests/waic_ref.py and each with the
route it has to take read back from ``Engine.last_kernels``; run with ``-m gpu``.

The route rule (``launch_waic_typed`` / ``waic_impl``), restated in :func:`expected_route`: an observations-fastest device
matrix goes to ``waic_col_kernel``; otherwise ``waic_wave_kernel`` takes rows of unit draw stride on a 16-byte aligned base
with ``stride_obs % W == 0``, ``S % W == 0`` and ``64 W <= S <= 4096`` (W = 16 / itemsize), and ``waic_rows_kernel`` the rest.

Tolerances are those of tests/test_gpu_waic.py::check.  ``var_i`` alone gets one derived term, (8 u max|x|)^2 with u = 2^-53:
a two-pass variance about a mean that is off by d is too large by exactly d^2, the wave kernel's mean is ``sum * recip_fast(S)``
(at most 4 u relative), and the bound is twice that, squared -- 8e-25 for ordinary rows, 7.9e-11 for a row of nothing but
replaced entries (constant +-1e10), whose variance is therefore not required to come out as exactly 0.
"""

import ctypes as C
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from waic_ref import sanitise, waic_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-10
AGG_N, AGG_SUM, AGG_M2, AGG_P, AGG_N_HIGH, AGG_N_SLOW = 0, 1, 2, 3, 4, 7
DTYPES = [np.float64, np.float32]
GRID_WAVES = 16384  # waves of the largest waic_wave_kernel launch; waic_rows_kernel stops at 8192 workgroups


def vec(dtype):
    return 16 // np.dtype(dtype).itemsize


def low(dtype):
    """L: the shortest row the wave kernel takes (one 16-byte vector per lane)"""
    return 64 * vec(dtype)


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


@pytest.fixture
def forced_rows(monkeypatch):
    monkeypatch.setenv("PLA_FORCE_PATH", "1")  # read by the launcher at every call


# ---------------------------------------------------------------------------------------------------------------- inputs
def default_rows(rng, n, s, dtype):
    """c_i - a_i Exp(1), as tests/test_gpu_waic.py::test_seeded_vs_oracle"""
    return (-rng.uniform(0.05, 1.2, size=(n, 1)) * rng.exponential(size=(n, s)) + rng.normal(size=(n, 1))).astype(dtype)


def well_posed(want):
    """what makes the exact count of variances above 0.4 and the relative checks of the sums meaningful"""
    clear = np.all(np.abs(want["var_i"] - 0.4) > 1e-6)
    return clear and np.sum(np.abs(want["waic_i"])) < 10.0 * abs(np.sum(want["waic_i"]))


def reference(a, scale=1.0, wide=True):
    """waic_ref of a matrix, its preconditions asserted (before the GPU is touched)"""
    want = waic_ref(a, scale, wide=wide)
    assert well_posed(want), "a variance sits on the 0.4 threshold, or the sum of waic_i cancels"
    x, _, _ = sanitise(a)
    want["var_slack"] = (8.0 * 2.0 ** -53 * np.max(np.abs(x.astype(np.float64)), axis=1)) ** 2
    return want


@functools.lru_cache(maxsize=None)
def seeded(n, s, dtype, seed=0):
    """(matrix, reference) -- computed once, shared, read-only.  The first of a few seeds whose reference is well posed (a
    handful of rows with c_i of both signs can sum to nearly nothing)."""
    for attempt in range(8):
        a = default_rows(np.random.default_rng(100003 * n + 7 * s + 1000 * attempt + seed), n, s, dtype)
        if well_posed(waic_ref(a, 1.0)):
            break
    a.setflags(write=False)
    return a, reference(a)


# ---------------------------------------------------------------------------------------------------------------- helpers
def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def check(res, want, n_replaced=None):
    lppd, var, waic, agg = (host(res[k]) for k in ("lppd_i", "var_i", "waic_i", "agg"))
    n = len(want["waic_i"])
    np.testing.assert_allclose(lppd, want["lppd_i"], rtol=RTOL, atol=1e-12)
    bound = RTOL * np.abs(want["var_i"]) + 1e-13 + want["var_slack"]
    worst = int(np.argmax(np.abs(var - want["var_i"]) - bound))
    assert np.all(np.abs(var - want["var_i"]) <= bound), (worst, var[worst], want["var_i"][worst], bound[worst])
    np.testing.assert_allclose(waic, want["waic_i"], rtol=RTOL, atol=1e-10)
    assert agg.shape == (8,) and agg[AGG_N] == n
    np.testing.assert_allclose(agg[AGG_SUM], want["elpd_waic"], rtol=1e-10)
    np.testing.assert_allclose(np.sqrt(agg[AGG_M2]), want["se"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(agg[AGG_P], want["p_waic"], rtol=1e-10)
    assert int(agg[AGG_N_HIGH]) == want["n_high"]
    assert int(agg[AGG_N_SLOW]) == (want["n_nan"] + want["n_inf"] if n_replaced is None else n_replaced)


def expected_route(t):
    """The kernel the route rule gives a device tensor handed to ``pla_waic`` as it is."""
    import torch

    n, s = t.shape
    so, sd = t.stride()
    tn, w = ("double", 2) if t.dtype == torch.float64 else ("float", 4)
    if n > 1 and s > 1 and so == 1 and sd >= n:
        return f"waic_col_kernel<{tn}>"
    if sd == 1 and t.data_ptr() % 16 == 0 and so % w == 0 and s % w == 0 and 64 * w <= s <= 4096:
        return f"waic_wave_kernel<{tn}, {w}>"
    return f"waic_rows_kernel<{tn}>"


def kernel(name, dtype):
    tn, w = ("double", 2) if np.dtype(dtype) == np.float64 else ("float", 4)
    return {"wave": f"waic_wave_kernel<{tn}, {w}>", "rows": f"waic_rows_kernel<{tn}>", "col": f"waic_col_kernel<{tn}>"}[name]


def capi_waic(eng, m, scale=1.0, pointwise=True):
    """``pla_waic`` through ctypes with the strides of ``m`` as they are (elements): a CUDA tensor is read in place whatever its strides (where
    ``Engine.waic`` would copy), a NumPy array is uploaded.  ``pointwise=False`` passes NULL for the three pointwise outputs."""
    import torch

    from pyloo_amd import _capi

    n, s = m.shape
    if hasattr(m, "data_ptr"):
        so, sd = m.stride()
        mk = lambda k: torch.full((k,), float("nan"), dtype=torch.float64, device=m.device)  # noqa: E731
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        code, space, stream, ptr = (_capi.PLA_F64 if m.dtype == torch.float64 else _capi.PLA_F32), _capi.PLA_DEVICE, eng._stream(), p(m)
    else:
        so, sd = (x // m.itemsize for x in m.strides)
        mk = lambda k: np.full(k, np.nan)  # noqa: E731
        p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        code, space, stream, ptr = _capi.dtype_code(m.dtype), _capi.PLA_HOST, None, p(m)
    out = {k: mk(n) if pointwise else None for k in ("lppd_i", "var_i", "waic_i")}
    out["agg"] = mk(8)
    q = lambda x: None if x is None else p(x)  # noqa: E731
    rc = eng._lib.pla_waic(eng._h, ptr, code, n, s, so, sd, float(scale), space, stream, q(out["lppd_i"]), q(out["var_i"]),
                           q(out["waic_i"]), q(out["agg"]))
    assert rc == 0, rc
    return out


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared matrices are read-only)


def obs_fastest(a):
    """(N, S) view of an (S, N) device buffer"""
    return dev(a.T).T


def run(eng, t, want, route, scale=1.0, n_replaced=None):
    res = eng.waic(t, scale)
    names = eng.last_kernels()
    assert route in names, (route, names)
    check(res, want, n_replaced)
    return res


def same_bits(a, b, keys=("lppd_i", "var_i", "waic_i", "agg")):
    for k in keys:
        np.testing.assert_array_equal(host(a[k]).view(np.int64), host(b[k]).view(np.int64), err_msg=k)


# ------------------------------------------------------------------------------------------ a. route boundary, row lengths
S_EDGES = {
    "1": lambda L, W: 1, "2": lambda L, W: 2, "7": lambda L, W: 7, "255": lambda L, W: 255, "257": lambda L, W: 257,
    "L-W": lambda L, W: L - W, "L": lambda L, W: L, "L+1": lambda L, W: L + 1, "L+W": lambda L, W: L + W,
    "L+63W": lambda L, W: L + 63 * W, "2L": lambda L, W: 2 * L, "2L+W": lambda L, W: 2 * L + W,
    "4096-W": lambda L, W: 4096 - W, "4096": lambda L, W: 4096, "4096+W": lambda L, W: 4096 + W,
}
WAVE_EDGES = ["L", "L+W", "L+63W", "2L", "2L+W", "4096-W", "4096"]


def test_the_edge_lengths_lie_on_both_sides_of_the_rule():
    for dtype in DTYPES:
        L, W = low(dtype), vec(dtype)
        wave = [k for k, f in S_EDGES.items() if f(L, W) % W == 0 and L <= f(L, W) <= 4096]
        assert wave == WAVE_EDGES


@pytest.mark.parametrize("edge", list(S_EDGES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_route_boundary_and_row_lengths(eng, dtype, edge):
    L, W = low(dtype), vec(dtype)
    s = S_EDGES[edge](L, W)
    for n in (1, 9):
        a, want = seeded(n, s, dtype)
        t = dev(a)
        route = kernel("wave" if edge in WAVE_EDGES else "rows", dtype)
        assert expected_route(t) == route
        run(eng, t, want, route, n_replaced=0)


@pytest.mark.parametrize("edge", WAVE_EDGES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_wave_lengths_on_the_general_kernel(eng, forced_rows, dtype, edge):
    s = S_EDGES[edge](low(dtype), vec(dtype))
    for n in (1, 9):
        a, want = seeded(n, s, dtype)
        t = dev(a)
        assert expected_route(t) == kernel("wave", dtype)  # what it would take were it not for PLA_FORCE_PATH
        run(eng, t, want, kernel("rows", dtype), n_replaced=0)


# ---------------------------------------------------------------------------------------------------------------- b. layouts
def nan_buffer(shape, dtype):
    """Anything read outside the matrix is a NaN: replaced, counted, and 1e10 away from the row's values."""
    import torch

    return torch.full(shape, float("nan"), dtype=torch.float64 if np.dtype(dtype) == np.float64 else torch.float32, device="cuda")


def draws_layout(a, kind):
    """(device view holding ``a``, kernel it has to take)"""
    n, s = a.shape
    W, src = vec(a.dtype), dev(a)
    if kind == "compact":
        return src, "wave"
    if kind == "pitch S+W":
        buf = nan_buffer((n, s + W), a.dtype)
        view, route = buf[:, :s], "wave"
    elif kind == "pitch S+1":
        buf = nan_buffer((n, s + 1), a.dtype)
        view, route = buf[:, :s], "rows"
    elif kind == "misaligned":
        buf = nan_buffer((n * (s + W) + W,), a.dtype)
        view, route = buf[1:1 + n * (s + W)].view(n, s + W)[:, :s], "rows"
        assert view.data_ptr() % 16 != 0
    elif kind == "every second row":
        buf = nan_buffer((2 * n, s), a.dtype)
        view, route = buf[::2], "wave"
    elif kind == "every second draw":
        buf = nan_buffer((n, 2 * s), a.dtype)
        view, route = buf[:, ::2], "rows"
    else:
        raise KeyError(kind)
    view.copy_(src)
    return view, route


@pytest.mark.parametrize("s_of", ["L+W", "1000"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts(eng, dtype, s_of):
    import torch

    n, s = 70, (low(dtype) + vec(dtype) if s_of == "L+W" else 1000)
    a, want = seeded(n, s, dtype)
    compact = None
    for kind in ("compact", "pitch S+W", "pitch S+1", "misaligned", "every second row"):
        t, route = draws_layout(a, kind)
        assert expected_route(t) == kernel(route, dtype), kind
        res = run(eng, t, want, kernel(route, dtype), n_replaced=0)
        if kind == "compact":
            compact = res
        elif route == "wave":
            same_bits(res, compact)  # the same kernel on the same rows, found at other addresses
    # every second draw: read in place through the C entry point, copied by Engine.waic
    t, route = draws_layout(a, "every second draw")
    assert t.stride() == (2 * s, 2) and expected_route(t) == kernel("rows", dtype)
    res = capi_waic(eng, t)
    names = eng.last_kernels()
    assert kernel("rows", dtype) in names and "strided draws" in names, names
    check(res, want, n_replaced=0)
    same_bits(run(eng, t, want, kernel("wave", dtype), n_replaced=0), compact)
    # observations fastest
    t = obs_fastest(a)
    assert t.stride() == (1, n) and expected_route(t) == kernel("col", dtype)
    col = run(eng, t, want, kernel("col", dtype), n_replaced=0)
    buf = nan_buffer((s, n + 3), dtype)
    t = buf[:, :n].T
    t.copy_(dev(a))
    assert t.stride() == (1, n + 3) and expected_route(t) == kernel("col", dtype)
    same_bits(run(eng, t, want, kernel("col", dtype), n_replaced=0), col)
    # host arrays: uploaded block by block, then the kernels of the compact matrix
    res = eng.waic(a, 1.0)
    names = eng.last_kernels()
    assert kernel("wave", dtype) in names and names.endswith("(blocks of observations uploaded)"), names
    check(res, want, n_replaced=0)
    same_bits(res, compact)
    res = eng.waic(np.ascontiguousarray(a.T).T, 1.0)
    names = eng.last_kernels()
    assert names.endswith("(blocks of observations uploaded)"), names
    check(res, want, n_replaced=0)
    assert isinstance(compact["agg"], torch.Tensor) and isinstance(res["agg"], np.ndarray)


def test_route_text_of_the_transposing_ingestion():
    """PLA_INGEST_TRANSPOSE=1: an observations-fastest device matrix goes through transpose_rows_kernel to the kernels of the
    draws-fastest layout.  Own process: the knob is read once per process."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import test_gpu_waic_routes as T
from pyloo_amd.engine import get_engine
eng = get_engine(0)
for dtype in T.DTYPES:
    a, want = T.nonfinite_columns(dtype)
    T.run(eng, T.obs_fastest(a), want, "transpose_rows_kernel + " + T.kernel("rows", dtype))
    a, want = T.seeded(70, T.low(dtype) + T.vec(dtype), dtype)
    T.run(eng, T.obs_fastest(a), want, "transpose_rows_kernel + " + T.kernel("wave", dtype), n_replaced=0)
print("transposed ok")
""" % (os.path.dirname(tests), tests)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PLA_INGEST_TRANSPOSE="1"), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and "transposed ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------- c. column kernel tails
COL_SHAPES = [(257, s) for s in (2, 7, 8, 9, 23, 24, 25, 31, 47, 48, 49, 77)] + [(n, s) for n in (2, 255, 256, 257, 600) for s in (25, 49)]
COL_SHAPES = list(dict.fromkeys(COL_SHAPES))


@pytest.mark.parametrize("n,s", COL_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_kernel_tails(eng, dtype, n, s):
    """Three batches of eight draws in flight: rows that end inside the first, second and third batch of a round, on a round,
    and one draw either side; workgroups of 256 lanes with 0, 1, 255 dead ones."""
    a, want = seeded(n, s, dtype)
    t = obs_fastest(a)
    assert expected_route(t) == kernel("col", dtype)
    run(eng, t, want, kernel("col", dtype), scale=1.0, n_replaced=0)


# ------------------------------------------------------------------------------------------------ d. non-finite entries
NAN, PINF, NINF = np.nan, np.inf, -np.inf


@functools.lru_cache(maxsize=None)
def nonfinite_rows(dtype):
    """S = 3L/2 + W: one whole vector per lane and a partial second one (qfull = 1, 0 < qrem < 64), so that every lane holds
    copies of its first vector, lanes below qrem one fewer.  Non-finite entries in the first vector of lane 0 (draws 0, W - 1)
    and of lane 63 (63 W), in the last vector (S - W, S - 1) and inside the second vector of an early lane."""
    L, W = low(dtype), vec(dtype)
    s = 3 * L // 2 + W
    nvec = s // W
    assert nvec // 64 == 1 and 0 < nvec % 64 < 64
    pos = [0, W - 1, 63 * W, s - W, s - 1, L + 2 * W + 1]
    a = default_rows(np.random.default_rng(4242 + W), 12, s, dtype)
    for row, (p, v) in enumerate(zip(pos, (NAN, PINF, NINF, NINF, NAN, PINF)), start=1):  # rows 1..6: one entry each
        a[row, p] = v
    a[7, 0], a[7, s - 1] = PINF, NINF
    a[8, pos] = NAN
    a[9, :] = NAN
    a[10, :] = NINF
    a[11, pos] = (NINF, NAN, PINF, NAN, PINF, NINF)
    a.setflags(write=False)
    want = reference(a)
    assert want["n_nan"] == 2 + 6 + s + 2 and want["n_inf"] == 4 + 2 + s + 4
    return a, want


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_on_the_wave_kernel(eng, dtype):
    a, want = nonfinite_rows(dtype)
    run(eng, dev(a), want, kernel("wave", dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_on_the_general_kernel(eng, forced_rows, dtype):
    a, want = nonfinite_rows(dtype)
    run(eng, dev(a), want, kernel("rows", dtype))


@functools.lru_cache(maxsize=None)
def nonfinite_columns(dtype):
    """S = 27 (a round of 24 and three draws of the next batch), N = 300 (a second workgroup with 212 dead lanes): non-finite
    entries at the first and last draw of batches and of the row, in the first and last lane of workgroups and of the matrix."""
    n, s = 300, 27
    a = default_rows(np.random.default_rng(2727), n, s, dtype)
    kinds = (NAN, PINF, NINF)
    for j, d in enumerate((0, 7, 8, 23, 24, 26)):
        for k, o in enumerate((0, 255, 256, 299)):
            a[o, d] = kinds[(j + k) % 3]
    assert not np.isfinite(a[299, 26])
    a.setflags(write=False)
    want = reference(a)
    assert want["n_nan"] == 8 and want["n_inf"] == 16
    return a, want


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_on_the_column_kernel(eng, dtype):
    a, want = nonfinite_columns(dtype)
    run(eng, obs_fastest(a), want, kernel("col", dtype))


def replaced_warnings(matrix):
    import pyloo_amd as pl

    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        pl.waic_from_matrix(matrix)
    text = [str(w.message) for w in rec]
    return sum("NaN values detected" in m for m in text), sum("Infinite values detected" in m for m in text)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_replaced_count_raises_the_warnings(eng, dtype):
    """waic.py:109-135 warns once for NaN and once for infinite entries; the front hears of them through agg[AGG_N_SLOW] only."""
    a, _ = nonfinite_rows(dtype)
    col, _ = nonfinite_columns(dtype)
    clean, _ = seeded(9, low(dtype), dtype)
    for make in (dev, obs_fastest):
        assert replaced_warnings(make(a)) == (1, 1)
        assert replaced_warnings(make(col)) == (1, 1)
        assert replaced_warnings(make(a[[0, 1, 5]])) == (1, 0)   # NaN at draw 0 / at draw S - 1 of a row
        assert replaced_warnings(make(a[[0, 2, 3]])) == (0, 1)   # +inf at draw W - 1, -inf at draw 63 W
        assert replaced_warnings(make(clean)) == (0, 0)
    only_last = np.array(col[200:300])
    only_last[:, :] = np.where(np.isfinite(only_last), only_last, -1.0)
    only_last[99, 26] = NAN   # the last draw of the last observation, in a workgroup with dead lanes
    assert replaced_warnings(obs_fastest(only_last)) == (1, 0)
    assert replaced_warnings(dev(only_last)) == (1, 0)


# --------------------------------------------------------------------------------- e. more than one row per wave / workgroup
N_BIG = 2 * GRID_WAVES + 5


@functools.lru_cache(maxsize=None)
def big_case(dtype, s):
    """Rows r, r + 16384 and r + 32768 (r < 5) go through one wave of the capped grid: a NaN in a first vector of the second
    row of wave 3, +inf in its third row, -inf in the first row of the last wave."""
    W = vec(dtype)
    a = default_rows(np.random.default_rng(16384 + s), N_BIG, s, dtype)
    a[3 + GRID_WAVES, 5 * W] = NAN
    a[3 + 2 * GRID_WAVES, s - 1] = PINF
    a[GRID_WAVES - 1, 0] = NINF
    a.setflags(write=False)
    want = reference(a, wide=False)
    assert (want["n_nan"], want["n_inf"]) == (1, 2)
    return a, want


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_rows_per_wave(eng, dtype):
    a, want = big_case(dtype, low(dtype) + vec(dtype))
    t = dev(a)
    assert expected_route(t) == kernel("wave", dtype)
    first = run(eng, t, want, kernel("wave", dtype))
    same_bits(run(eng, t, want, kernel("wave", dtype)), first)


@pytest.mark.parametrize("dtype", DTYPES)
def test_five_rows_per_workgroup_of_the_general_kernel(eng, forced_rows, dtype):
    a, want = big_case(dtype, low(dtype) + vec(dtype))
    t = dev(a)
    first = run(eng, t, want, kernel("rows", dtype))
    same_bits(run(eng, t, want, kernel("rows", dtype)), first)


@pytest.mark.parametrize("dtype", DTYPES)
def test_many_workgroups_of_the_column_kernel(eng, dtype):
    a, want = big_case(dtype, 27)
    t = obs_fastest(a)
    first = run(eng, t, want, kernel("col", dtype))
    same_bits(run(eng, t, want, kernel("col", dtype)), first)


# ---------------------------------------------------------------------------------------- f. values that stress the arithmetic
@functools.lru_cache(maxsize=None)
def stress_rows(dtype, s):
    rng = np.random.default_rng(31337 + s)
    base = default_rows(rng, 2, s, np.float64)
    rows = {
        "far mean a": -100.0 + 0.01 * rng.normal(size=s),   # |mean| / sd = 1e4: a one-pass variance loses eight digits
        "far mean b": -100.0 + 0.01 * rng.normal(size=s),
        # the same family times 100: the same relative errors, and a variance of 1, where the absolute term of the tolerance
        # plays no part
        "far mean, unit sd": -1e4 + rng.normal(size=s),
        "ascending": np.sort(base[0]),            # column kernel: every batch brings a new running maximum
        "descending": np.sort(base[1])[::-1],     # ... or none after the first
        "dominant first": np.concatenate(([50.0], -rng.exponential(size=s - 1))),  # at S = L its copies fill lane 0 and are subtracted
        "dominant last": np.concatenate((-rng.exponential(size=s - 1), [50.0])),
        "wide span": np.concatenate(([0.0, -800.0], rng.uniform(-800.0, 0.0, size=s - 2))),  # more than 709 nats
    }
    a = np.stack(list(rows.values())).astype(dtype)
    a.setflags(write=False)
    want = reference(a)
    sd = np.sqrt(want["var_i"][:3])
    assert np.all(np.abs(a[:3].astype(np.float64).mean(axis=1)) / sd > 5e3)
    assert a[7].astype(np.float64).max() - a[7].astype(np.float64).min() > 709.0
    return a, want


@pytest.mark.parametrize("route", ["wave", "rows", "col"])
@pytest.mark.parametrize("s_of", ["L", "1000"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stress_values(eng, monkeypatch, dtype, s_of, route):
    a, want = stress_rows(dtype, low(dtype) if s_of == "L" else 1000)
    if route == "rows":
        monkeypatch.setenv("PLA_FORCE_PATH", "1")
    run(eng, obs_fastest(a) if route == "col" else dev(a), want, kernel(route, dtype), n_replaced=0)


# ------------------------------------------------------------------------------------- g. C ABI without pointwise outputs
@pytest.mark.parametrize("dtype", DTYPES)
def test_aggregates_without_pointwise_outputs(eng, dtype):
    """``agg`` alone: var_i and waic_i live in engine scratch (device input) -- the same bits as the full call."""
    a, want = nonfinite_rows(dtype)
    for t, route in ((dev(a), "wave"), (obs_fastest(a), "col"), (a, "wave")):
        full = capi_waic(eng, t, scale=-2.0)
        assert kernel(route, dtype) in eng.last_kernels()
        alone = capi_waic(eng, t, scale=-2.0, pointwise=False)
        assert kernel(route, dtype) in eng.last_kernels()
        same_bits(alone, full, keys=("agg",))
        same_bits(capi_waic(eng, t, scale=-2.0), full)  # (the scratch run left nothing behind)
        agg = host(full["agg"])
        assert agg[AGG_N] == 12 and int(agg[AGG_N_SLOW]) == want["n_nan"] + want["n_inf"]
        np.testing.assert_allclose(agg[AGG_SUM], -2.0 * want["elpd_waic"], rtol=1e-10)
        np.testing.assert_allclose(agg[AGG_P], want["p_waic"], rtol=1e-10)
        np.testing.assert_allclose(host(full["waic_i"]), -2.0 * want["waic_i"], rtol=RTOL, atol=1e-10)
