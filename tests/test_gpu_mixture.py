"""Mix-IS-LOO on the GPU: both passes on every route against the NumPy restatement (tests/mixis_ref.py) -- tile, row-length and
line-length edges, four layouts, f64 and f32 -- the routes taken, bit-identical results whatever the grid and from host or device
memory, wide ranges, non-finite entries, and the two fronts.

Tolerances: the project's own for log-sum-exp values (test_gpu_waic.py, test_gpu_kfold.py): pointwise rtol 1e-10 / atol 1e-12, sums
rtol 1e-10, standard errors rtol 1e-8 / atol 1e-9.  R is the register-row limit of pass 2 (kMixisRegDraws in pla_mixis.h)."""

import functools
import warnings

import numpy as np
import pytest

import pyloo_amd as pl
from mixis_ref import mixis
from pyloo_amd._capi import AGG_COUNT, AGG_M2_LOO, AGG_N, AGG_N_SLOW, AGG_SUM_LOO

pytestmark = pytest.mark.gpu
R = 4096
LAYOUTS = ("draws", "obs", "draw2", "row2")
NAN_TEXT = "NaN values detected in log-likelihood"


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    e = get_engine(0)
    e.set_mixis_grid(0)
    return e


def layout(a, kind):
    """A host matrix on the device: draws fastest, observations fastest (an (S, n) buffer seen as .T), every second draw of a
    wider NaN-filled buffer, or every second row of a taller one (test_gpu_kfold.py's four)."""
    import torch

    t = torch.from_numpy(np.array(a, order="C")).cuda()  # (a writable copy: the shared cases are read-only)
    if kind == "draws":
        return t
    if kind == "obs":
        return t.T.contiguous().T
    if kind == "draw2":
        buf = torch.full((t.shape[0], 2 * t.shape[1]), float("nan"), dtype=t.dtype, device="cuda")
        buf[:, ::2] = t
        return buf[:, ::2]
    buf = torch.full((2 * t.shape[0], t.shape[1]), float("nan"), dtype=t.dtype, device="cuda")
    buf[::2] = t
    return buf[::2]


def expected_routes(t):
    """The kernels the route rule of include/pyloo_amd.h gives this tensor: (pass 1, pass 2)."""
    import torch

    n, s = t.shape
    so, sd = t.stride()
    tn, vec = ("double", 2) if t.dtype == torch.float64 else ("float", 4)
    al = t.data_ptr() % 16 == 0
    if sd == 1:
        one = f"mixis_c_tile_kernel<{tn}, unit>"
        if s <= R:
            two = f"mixis_row_wave_kernel<{tn}, {vec if al and so % vec == 0 and s % vec == 0 else 1}>"
        else:
            two = f"mixis_row_stream_kernel<{tn}, {vec if al and so % vec == 0 else 1}>"
    elif so == 1:
        one = f"mixis_c_line_kernel<{tn}, {vec if al and sd % vec == 0 else 1}>"
        two = f"mixis_col_kernel<{tn}>"
    else:
        one, two = f"mixis_c_tile_kernel<{tn}, strided>", f"mixis_row_block_kernel<{tn}>"
    return one, two


@functools.lru_cache(maxsize=None)
def case(n, s, dtype, seed=0):
    """(matrix, restatement) -- computed once, shared, read-only"""
    a = np.random.default_rng(1000 * n + s + seed).normal(-1.5, 1.2, size=(n, s)).astype(dtype)
    a.setflags(write=False)
    return a, mixis(a)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def check(res, want, scale_value=1.0, n_replaced=0):
    np.testing.assert_allclose(host(res["c"]), want["c"], rtol=1e-10, atol=1e-12)
    loo_i = scale_value * want["elpd_i"]
    np.testing.assert_allclose(host(res["loo_i"]), loo_i, rtol=1e-10, atol=1e-12)
    agg = host(res["agg"])
    assert agg.shape == (AGG_COUNT,) and agg[AGG_N] == len(loo_i) and agg[AGG_N_SLOW] == n_replaced
    np.testing.assert_allclose(agg[AGG_SUM_LOO], loo_i.sum(), rtol=1e-10)
    np.testing.assert_allclose(agg[AGG_M2_LOO] ** 0.5, (len(loo_i) * np.var(loo_i)) ** 0.5, rtol=1e-8, atol=1e-9)
    others = [k for k in range(AGG_COUNT) if k not in (AGG_N, AGG_SUM_LOO, AGG_M2_LOO, AGG_N_SLOW)]
    np.testing.assert_array_equal(agg[others], 0.0)


def run(eng, t, want, **kw):
    """Both passes, the way ``Engine.mixis_loo`` runs them without a ``c``; returns the result and the kernels of the two calls."""
    first = eng.mixis_draw_lse(t)
    names = eng.last_kernels()
    res = eng.mixis_loo(t, c=first["c"], **kw)
    names += " | " + eng.last_kernels()
    one, two = expected_routes(t)
    assert one in names and two in names and "mixis_c_merge_kernel" in names and "kfold_final_kernel" in names, (names, one, two)
    check(res, want, kw.get("scale_value", 1.0))
    return res, names


# ---------------------------------------------------------------------------------------------------------------------- small cases
def test_two_by_two_and_single_observation(eng):
    ll = np.log(np.array([[1 / 2, 1 / 4], [1 / 8, 1 / 2]]))
    for kind in LAYOUTS:
        res = eng.mixis_loo(layout(ll, kind))
        np.testing.assert_allclose(host(res["loo_i"]), [np.log(4 / 13), np.log(4 / 17)], rtol=1e-12)
        np.testing.assert_allclose(host(res["c"]), [np.log(10), np.log(6)], rtol=1e-12)
    a, want = case(1, 257, np.float64)
    res = eng.mixis_loo(layout(a, "draws"))
    from oracle import psis_oracle as orc

    np.testing.assert_allclose(host(res["loo_i"])[0], orc.lse(a[0], b_inv=257), rtol=1e-10)
    check(res, want)


T = 256  # pla_mixis_tile_rows(N) for every N below (checked in the test)
TILE_EDGE_SIZES = (1, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", TILE_EDGE_SIZES)
def test_shapes_layouts_and_routes(eng, n, dtype):
    assert eng.mixis_tile_rows(n) == T
    for s in (1, 5, 63, 64, 65, 257):
        a, want = case(n, s, dtype)
        for kind in LAYOUTS:
            _, names = run(eng, layout(a, kind), want)
            if n > 1 and s > 1:  # the route each layout is meant to take (alignment picks the kernel's vector width)
                meant = {"draws": ("mixis_c_tile_kernel", ", unit>", "mixis_row_wave_kernel"),
                         "obs": ("mixis_c_line_kernel", "", "mixis_col_kernel"),
                         "draw2": ("mixis_c_tile_kernel", ", strided>", "mixis_row_block_kernel"),
                         "row2": ("mixis_c_tile_kernel", ", unit>", "mixis_row_wave_kernel")}[kind]
                assert all(m in names for m in meant), (kind, names)


def test_vector_width_follows_alignment(eng):
    a, want = case(70, 64, np.float64)
    _, names = run(eng, layout(a, "draws"), want)
    assert "mixis_row_wave_kernel<double, 2>" in names
    _, names = run(eng, layout(case(64, 70, np.float64)[0], "obs"), case(64, 70, np.float64)[1])
    assert "mixis_c_line_kernel<double, 2>" in names
    a, want = case(70, 65, np.float32)
    _, names = run(eng, layout(a, "draws"), want)
    assert "mixis_row_wave_kernel<float, 1>" in names
    _, names = run(eng, layout(case(65, 70, np.float32)[0], "obs"), case(65, 70, np.float32)[1])
    assert "mixis_c_line_kernel<float, 1>" in names


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("s", [R - 1, R, R + 1])
def test_row_length_edges_of_pass_two(eng, s, dtype):
    a, want = case(70, s, dtype)
    for kind in ("draws", "obs"):
        _, names = run(eng, layout(a, kind), want)
        if kind == "draws":
            assert ("mixis_row_wave_kernel" if s <= R else "mixis_row_stream_kernel") in names


def test_rows_whose_c_does_not_fit_lds(eng):
    a, want = case(70, 20000, np.float32)
    _, names = run(eng, layout(a, "draws"), want)
    assert "mixis_row_stream_kernel<float, 4>" in names
    run(eng, layout(a, "obs"), want)


@pytest.mark.parametrize("n", [5000, 70001])
def test_long_lines_of_pass_one(eng, n):
    for dtype in (np.float64, np.float32):
        a, want = case(n, 7, dtype)
        _, names = run(eng, layout(a, "obs"), want)
        assert "mixis_c_line_kernel" in names and "mixis_col_kernel" in names


def test_scale_and_a_given_c(eng):
    import ctypes as C

    import torch

    a, want = case(65, 257, np.float64)
    t = layout(a, "draws")
    first = eng.mixis_draw_lse(t)
    assert first["n_replaced"].tolist() == [0, 0]
    given = eng.mixis_loo(t, c=first["c"], scale_value=-2.0)
    check(given, want, -2.0)
    own = eng.mixis_loo(t, scale_value=-2.0)
    for key in ("c", "loo_i", "agg"):
        assert torch.equal(given[key], own[key]), key
    # the C entry point without a c: both passes in one call, the same bits
    loo_i, agg = torch.zeros(65, dtype=torch.float64, device="cuda"), torch.zeros(AGG_COUNT, dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rc = eng._lib.pla_mixis_loo(eng._h, p(t), 0, 65, 257, t.stride(0), t.stride(1), None, -2.0, 1, eng._stream(), p(loo_i), p(agg))
    assert rc == 0
    names = eng.last_kernels()
    assert "mixis_c_tile_kernel<double, unit> + mixis_c_merge_kernel, then mixis_lse_c_kernel + mixis_row_wave_kernel" in names
    assert torch.equal(loo_i, given["loo_i"]) and torch.equal(agg, given["agg"])
    only_agg = eng.mixis_loo(t, pointwise=False)
    assert only_agg["loo_i"] is None
    np.testing.assert_allclose(host(only_agg["agg"])[AGG_SUM_LOO], want["elpd_i"].sum(), rtol=1e-10)
    assert eng.mixis_loo(t, aggregate=False)["agg"] is None


# ------------------------------------------------------------------------------------------------------------------- the same bits
def test_results_do_not_depend_on_the_grid(eng):
    import torch

    a, want = case(5000, 300, np.float64)
    try:
        for kind in LAYOUTS:
            t = layout(a, kind)
            base = eng.mixis_loo(t)
            check(base, want)
            for grid in (1, 3, 37):
                eng.set_mixis_grid(grid)
                got = eng.mixis_loo(t)
                for key in ("c", "loo_i", "agg"):
                    assert torch.equal(got[key], base[key]), (kind, grid, key)
                eng.set_mixis_grid(0)
    finally:
        eng.set_mixis_grid(0)


def same_bits_host_device(eng, a, want, blocks):
    """A host ndarray and the same values in a contiguous, 16-byte aligned device tensor of the same layout: the same bits."""
    for kind, h in (("draws", np.array(a)), ("obs", np.ascontiguousarray(a.T).T)):
        dev = eng.mixis_loo(layout(a, kind), scale_value=-1.0)
        got = eng.mixis_loo(h, scale_value=-1.0)
        assert "staged in blocks" in eng.last_kernels()
        assert isinstance(got["loo_i"], np.ndarray)
        check(got, want, -1.0)
        for key in ("c", "loo_i", "agg"):
            np.testing.assert_array_equal(got[key], host(dev[key]), err_msg=f"{kind} {key} {blocks}")
        first = eng.mixis_draw_lse(h)
        np.testing.assert_array_equal(first["c"], host(dev["c"]))
        assert first["n_replaced"].tolist() == [0, 0]
        one_call = eng.mixis_loo(h, c=first["c"], scale_value=-1.0, pointwise=False)
        assert one_call["loo_i"] is None
        np.testing.assert_array_equal(one_call["agg"], got["agg"])


def test_host_and_device_give_the_same_bits(eng):
    for dtype in (np.float64, np.float32):
        a, want = case(515, 257, dtype)
        same_bits_host_device(eng, a, want, "one block")


def test_host_matrix_staged_in_several_blocks(eng, monkeypatch):
    """1 MiB blocks: 256 rows (f64) and 768 rows (f32) of 257 draws, so 1027 observations come in 5 and 2 blocks of whole tiles, the
    last one ragged and of odd length (the observations-fastest slab is padded to 16 bytes and still sums as the device does)."""
    monkeypatch.setenv("PLA_INGEST_BLOCK_MB", "1")
    for dtype in (np.float64, np.float32):
        a, want = case(1027, 257, dtype)
        same_bits_host_device(eng, a, want, "several blocks")
    a = np.array(case(1027, 257, np.float64)[0])
    a[300, 5], a[1026, 200] = np.nan, np.inf  # counted once each, in whichever block they lie
    want = mixis(a)
    for h in (a, np.ascontiguousarray(a.T).T):
        first = eng.mixis_draw_lse(h)
        assert first["n_replaced"].tolist() == [1, 1]
        check(eng.mixis_loo(h, c=first["c"]), want, n_replaced=2)


# ------------------------------------------------------------------------------------------------------------ ranges and non-finite
def test_wide_ranges_stay_finite(eng):
    a = np.array(case(70, 65, np.float64)[0])
    a[11, 5] = -800.0   # one observation of draw 5 dominates c[5]; the rest of the column is O(1)
    a[12, 9] = -800.0   # row 12 at draw 9: -ll - c = 800 - 1600, the rest of the row O(1) -- a span above 709 nats
    a[13, 9] = -1600.0
    want = mixis(a)
    assert np.ptp(-a[12] - want["c"]) > 709 and np.all(np.isfinite(want["elpd_i"]))
    for kind in LAYOUTS:
        res, _ = run(eng, layout(a, kind), want)
        assert bool(res["loo_i"].isfinite().all()) and bool(res["c"].isfinite().all())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_non_finite_entries_are_clamped_and_counted(eng, dtype):
    a = np.array(case(70, 65, dtype)[0])
    a[3, 7], a[40, 21], a[69, 64] = np.nan, np.inf, -np.inf  # at most one per draw: c stays exactly representable
    want = mixis(a)
    assert want["n_replaced"].tolist() == [1, 2] and np.all(np.isfinite(want["elpd_i"]))
    for kind in LAYOUTS:
        t = layout(a, kind)
        first = eng.mixis_draw_lse(t)
        assert first["n_replaced"].tolist() == [1, 2], kind
        np.testing.assert_allclose(host(first["c"]), want["c"], rtol=1e-10, atol=1e-12)
        res = eng.mixis_loo(t, c=first["c"])
        check(res, want, n_replaced=3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = pl.loo_mixture_from_matrix(layout(a, "draws"), pointwise=True)
    assert sum(NAN_TEXT in str(w.message) for w in rec) == 1
    np.testing.assert_allclose(host(out["loo_i"]), want["loo_i"], rtol=1e-10, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------- the fronts
def test_from_matrix_on_a_cuda_tensor(eng):
    a, want = case(65, 257, np.float32)
    with pytest.warns(UserWarning, match="Mix-IS-LOO requires"):
        res = pl.loo_mixture_from_matrix(layout(a, "obs"), scale="deviance", pointwise=True)
    assert res["loo_i"].is_cuda and res["pareto_k"].is_cuda and not bool(res["pareto_k"].any())
    np.testing.assert_allclose(host(res["loo_i"]), -2 * want["elpd_i"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(res["elpd_loo"], -2 * want["elpd_i"].sum(), rtol=1e-10)
    np.testing.assert_allclose(res["se"], (65 * np.var(-2 * want["elpd_i"])) ** 0.5, rtol=1e-8, atol=1e-9)
    assert res["warning"] is False and "p_loo" not in res and "mixture posterior" in str(res)


def test_front_on_a_chain_draw_obs_grid(eng):
    ll = np.random.default_rng(9).normal(-1.0, 0.8, size=(2, 50, 3, 4))
    with pytest.warns(UserWarning, match="Mix-IS-LOO requires"):
        res = pl.loo_mixture({"log_likelihood": {"y": ll}}, pointwise=True)
    want = mixis(np.moveaxis(ll.reshape(100, 3, 4), 0, -1).reshape(12, 100))
    assert np.asarray(res["loo_i"]).shape == (3, 4)
    np.testing.assert_allclose(np.asarray(res["loo_i"]).reshape(-1), want["loo_i"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(res["elpd_loo"], want["loo_i"].sum(), rtol=1e-10)
    np.testing.assert_allclose(res["se"], (12 * np.var(want["loo_i"])) ** 0.5, rtol=1e-8, atol=1e-9)
    np.testing.assert_array_equal(np.asarray(res["pareto_k"]), np.zeros((3, 4)))
