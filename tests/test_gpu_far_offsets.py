"""Every strided entry point on views whose rows or lines lie past 2^32 and 2^33 bytes -- for f32 past element 2^31 -- from the
pointer the library is given (tests/far_views.py), and one true-size f32 matrix of more than 2^31 elements; run with ``-m gpu``.

Each case runs the engine method on the far view and on its twin, a small tensor of the same layout class, and asserts that
both took the same kernels (``Engine.last_kernels``), that the wrapper handed the far view over with its own pointer and strides,
that the two results are equal bit for bit (the kernels are documented as independent of position, grid and pitch), that the
NaN counters are exactly the planted count, and that the far result meets the CPU reference of the operation at the tolerance
of the entry point's own GPU test file.

Where the NaN goes.  The arena is poisoned with NaN, so a mis-addressed read shows as a NaN the library counts (or as a NaN
result).  An entry point that replaces and counts NaN gets one in the last row or line, the one past 2^33 bytes.  An entry point
whose result for a row with a NaN is itself NaN (psis_loo, importance_weights, e_loo, relative_eff) would hide a wrong read of
that very row behind the planted one: on the row layouts its NaN goes into the row before the last, which lies past 2^32 bytes,
and the last row stays clean.  The comparison passes (compare_moments, stacking_eval, bb_bootstrap), mm_transform and glm carry
a NaN into everything the row or draw touches and count nothing: they get none.

Shapes moved from the issue's table, each to the nearest shape for which ``far_layout`` has a pitch (a line of n elements holds
offset 2^32 only if a multiple of 16 bytes lies in a window of n * itemsize / (lines / 2) bytes):
  * psis_loo on lines: (70, 527), not (70, 543) -- 527 = 16 * 32 + 15 is still shorter than one ring of the tile kernel's sweep
    and leaves draws behind the last whole step;
  * mixis on lines_odd: (66, 204), not (65, 257) -- the same kernels (``expected_routes`` of tests/test_gpu_mixture.py);
  * mixis otherwise: (66, 257) and, on lines, (66, 258), not (65, 257) -- with an odd count the last row or line is the one that
    holds offset 2^33 and so STARTS below it; an even count adds one that lies wholly past 2^33 bytes, where for f32 the row's
    own start offset passes element 2^31 (a row offset narrowed to ``int`` in ``mixis_row_wave_kernel`` went unnoticed at 65 rows).
And two to the nearest row length that selects the kernel meant: psis_loo and importance_weights at (9, 4224), not (9, 4100) -- the
chunked wave kernel asks for a last chunk of a whole wave of 16-byte vectors (128 doubles behind the 4096 of the first chunk;
``launch_typed`` in csrc/pla_k_general.hip), and 4100 goes to the general kernel.

Where the bits may differ.  ``e_loo_quantile_kernel<T, 512>`` (one workgroup per observation) adds the weights with floating-point
LDS atomics from eight waves and is not reproducible from one call to the next on the same tensor (tests/test_gpu_e_loo_routes.py,
``QUANT_ULPS``; here two calls on the twin at (9, 4100) f64 differed by up to 4.7e-14).  ``test_e_loo_and_quantiles`` reads the route
text: rows that ``e_loo_quantile_wave_kernel`` took are compared bit for bit, every other row within ``QUANT_ULPS``.
"""

import ctypes as C

import numpy as np
import pytest

import diag_ref
import ess_ref
import far_views as fv
from far_views import (DIAG, DRAWS, E_LOO, ESS, F4, F8, GROUPS, INFLUENCE, KFOLD, LFO, MIXIS, PIT, PSIS_LINES, PSIS_ROWS, SECOND, WAIC,
                       WEIGHTS)
import glm_ref
import group_gather_ref
import influence_ref
import lfo_bw_ref
import lfo_ref
import mixis_ref
import nonfactor_ref
import pit_ref
from compare_stream import gamma_draws, bb_z_from_gammas
from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu


def ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


class Arena:
    """The arena and the far views of the running case (poisoned again when the case ends)."""

    def __init__(self):
        self.t = fv.new_arena()
        self.views = []

    def far(self, a, kind, shift=0):
        v = fv.far_view(self.t, a, kind, shift)
        self.views.append(v)
        return v

    def pitched(self, a, shift=0):
        v = fv.far_pitched(self.t, a, shift)
        self.views.append(v)
        return v

    def clean(self):
        fv.repoison(self.t, *self.views)
        self.views = []


@pytest.fixture(scope="module")
def arena_of_module():
    import torch

    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()  # (what earlier modules of the run still hold is not this module's)
    holder = Arena()  # (an allocation failure is an error of the test, not a skip)
    yield holder
    peak = torch.cuda.max_memory_allocated() - before
    del holder.t
    torch.cuda.empty_cache()
    assert peak < 17 * 2 ** 30, peak


@pytest.fixture
def arena(arena_of_module):
    yield arena_of_module
    arena_of_module.clean()


# ----------------------------------------------------------------------------------------------------------------- helpers
def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def scalar(x):
    return int(host(x).reshape(-1)[0])


def same_bits(what, a, b, keys):
    for k in keys:
        x, y = host(a[k]), host(b[k])
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (what, k, np.argwhere(~((x == y) | (np.isnan(x) & np.isnan(y))))[:5])


def plant(a, kind, counted=True):
    """One NaN in the last row or line of ``a``, the one past 2^33 bytes; ``counted=False``: on the row layouts in the row before the
    last (module docstring).  Returns ``a``."""
    n, s = a.shape
    if kind.startswith("lines"):
        a[n // 2, s - 1] = np.nan
    else:
        a[n - 1 if counted else n - 2, s // 2] = np.nan
    return a


def taken_in_place(view, layout, rows=None):
    """The wrapper hands ``view`` to the library as it is: its own pointer, its own strides."""
    from pyloo_amd.engine import _DeviceSpace

    t, so, sd = _DeviceSpace.matrix(view, layout, rows)
    assert t.data_ptr() == view.data_ptr() and (so, sd) == tuple(view.stride()) and max(so, sd) * view.element_size() > 2 ** 20, (so, sd)


def both(eng, far, near, call):
    """``call`` on the far view and on its twin: (far result, twin result, the kernels both took)."""
    a = call(far)
    ka = eng.last_kernels()
    b = call(near)
    kb = eng.last_kernels()
    assert ka == kb, (ka, kb)
    return a, b, ka


def close(a, b, rtol=1e-9, atol=1e-10, what=""):
    from test_gpu_parity import close as parity_close

    parity_close(host(a), b, rtol, atol, what)


def seeded_ll(n, s, dt, seed, k_hi=0.9):
    """c_i - a_i Exp(1): rows with Pareto k between 0.05 and ``k_hi`` (tests/test_gpu_parity.py::test_seeded_vs_oracle)."""
    rng = np.random.default_rng(seed)
    return (-rng.uniform(0.05, k_hi, size=(n, 1)) * rng.exponential(size=(n, s)) + rng.normal(size=(n, 1))).astype(dt)


# ------------------------------------------------------------------------------------------------------------------ psis_loo
def loo_reference(ll, method):
    ref = orc.loo_pointwise(ll.astype(np.float64), 1.0, method)
    return ref


def planted_row_counted(agg, ref, n, fast):
    """The counters of ``agg``: every observation reduced, exactly the planted row with a diagnostic that is not finite, and -- where a
    wave kernel ran -- that row among those that left its fast path."""
    from pyloo_amd._capi import AGG_N, AGG_N_NONFINITE, AGG_N_SLOW

    agg = host(agg)
    assert int(np.sum(~np.isfinite(ref["diag"]))) == 1
    assert agg[AGG_N] == n and agg[AGG_N_NONFINITE] == 1, agg
    if fast:
        assert 1 <= agg[AGG_N_SLOW] <= n, agg


def check_loo(res, ref, what):
    close(res["diag"], ref["diag"], what=f"{what} diag")
    close(res["loo_i"], ref["loo_i"], what=f"{what} loo_i")
    close(res["lppd_i"], ref["lppd_i"], what=f"{what} lppd_i")


@pytest.mark.parametrize("shape", PSIS_ROWS, ids=ids)
def test_psis_loo_rows(eng, arena, shape):
    """The one-chunk (S = 1000) and chunked (S = 4224) wave kernels with the fit kernel, and the general kernel for the NaN row and
    for rows that are not 16-byte aligned (rows_odd); sis and tis on the aligned rows."""
    from pyloo_amd.engine import _LOO

    n, s, dt, kind = shape
    ll = plant(seeded_ll(n, s, dt, 11 * s + n), kind, counted=False)
    far, near = arena.far(ll, kind), fv.twin(ll, kind)
    taken_in_place(far, _LOO)
    M = orc.tail_count(s, 1.0)
    for method in ("psis", "sis", "tis") if kind == "rows" else ("psis",):
        a, b, text = both(eng, far, near, lambda t: eng.psis_loo(t, M if method == "psis" else 0, method, 1.0, 0.7))
        print(shape, method, text)
        if kind == "rows_odd":
            assert text.startswith("rows_kernel<"), text
        elif method == "psis":
            assert text.startswith("wave_loo_chunked_kernel<" if s > 4096 else "wave_loo_kernel<") and "slow_rows_kernel" in text, text
        else:  # (the SIS / TIS wave kernel keeps a row in registers: up to 4096 draws)
            assert text.startswith("is_wave_kernel<" if s <= 4096 else "rows_kernel<"), text
        same_bits((shape, method), a, b, ("diag", "loo_i", "lppd_i", "agg"))
        ref = loo_reference(ll, method)
        check_loo(a, ref, (shape, method))
        planted_row_counted(a["agg"], ref, n, fast=kind == "rows" and text.startswith(("wave_loo", "is_wave")))


@pytest.mark.parametrize("pipe", [None, "0"])
@pytest.mark.parametrize("shape", PSIS_LINES, ids=ids)
def test_psis_loo_lines(eng, arena, shape, pipe, monkeypatch):
    """Observations fastest: the lane-per-observation kernels of pla_col.h (f32) and tile_loo_kernel (f64), streamed and with
    PLA_PIPE=0 back to back."""
    from pyloo_amd.engine import _LOO

    if pipe is not None:
        monkeypatch.setenv("PLA_PIPE", pipe)
    n, s, dt, kind = shape
    ll = plant(seeded_ll(n, s, dt, 13 * s + n), kind)
    far, near = arena.far(ll, kind), fv.twin(ll, kind)
    taken_in_place(far, _LOO)
    M = orc.tail_count(s, 1.0)
    a, b, text = both(eng, far, near, lambda t: eng.psis_loo(t, M, "psis", 1.0, 0.7))
    print(shape, pipe, text)
    assert ("tile_loo_kernel" if dt == F8 else "col_sweep_kernel") in text, text
    if dt == F8:
        assert ("fit_rows_stream_kernel" in text) == (pipe is None), text
    # (the lists of these kernels are appended to in whatever order the waves arrive: the results do not depend on it)
    same_bits(shape, a, b, ("diag", "loo_i", "lppd_i", "agg"))
    ref = loo_reference(ll, "psis")
    check_loo(a, ref, shape)
    planted_row_counted(a["agg"], ref, n, fast=True)


# ------------------------------------------------------------------------------------------------------- importance_weights
@pytest.mark.parametrize("shape", WEIGHTS, ids=ids)
def test_importance_weights(eng, arena, shape):
    """The weights mode of the wave kernels; at S = 4224 the chunked kernel with the split pass of pla_lwout.h behind it."""
    from pyloo_amd.engine import _WEIGHTS

    n, s, dt, kind = shape
    lr = plant(-seeded_ll(n, s, dt, 17 * s + n), kind, counted=False)
    far, near = arena.far(lr, kind), fv.twin(lr, kind)
    taken_in_place(far, _WEIGHTS)
    M = orc.tail_count(s, 1.0)
    (lw, k), (lw2, k2), text = both(eng, far, near, lambda t: eng.importance_weights(t, M, "psis"))
    if s <= 4096:
        assert text.startswith("wave_loo_kernel<") and "weights" in text, text
    else:  # (draws fastest: the split pass; observations fastest: transposed block by block into the fused chunked kernel)
        assert text.startswith("wave_loo_chunked_kernel<") and "weights" in text and ("lw_output_kernel" in text) == (kind == "rows"), text
    same_bits(shape, {"lw": lw, "k": k}, {"lw": lw2, "k": k2}, ("lw", "k"))
    want_lw, want_k = orc.psislw(lr.astype(np.float64), 1.0)
    close(k, want_k, what="k")
    if dt == F4:  # (tests/test_gpu_parity.py::test_golden_weights: the reference on the upcast data, rounded to f32)
        close(lw, want_lw.astype(np.float32), rtol=2e-7, atol=1e-7, what="lw")
    else:
        close(lw, want_lw, what="lw")


# --------------------------------------------------------------------------------------------------------------------- waic
@pytest.mark.parametrize("shape", WAIC, ids=ids)
def test_waic(eng, arena, shape):
    """waic_wave_kernel (S = 1000 on aligned rows), waic_rows_kernel (the other rows) and waic_col_kernel (lines)."""
    from pyloo_amd.engine import _LOO
    from test_gpu_waic_routes import check, expected_route, reference

    n, s, dt, kind = shape
    ll = plant(seeded_ll(n, s, dt, 19 * s + n, k_hi=1.2), kind)
    want = reference(ll)
    far, near = arena.far(ll, kind), fv.twin(ll, kind)
    taken_in_place(far, _LOO)
    assert expected_route(far) == expected_route(near)
    a, b, text = both(eng, far, near, lambda t: eng.waic(t, 1.0))
    assert expected_route(far) in text, (expected_route(far), text)
    same_bits(shape, a, b, ("lppd_i", "var_i", "waic_i", "agg"))
    check(a, want, n_replaced=1)


# ------------------------------------------------------------------------------------------------ loo_diag, loo_diag_weights
@pytest.mark.parametrize("shape", DIAG, ids=ids)
def test_loo_diag_and_loo_diag_weights(eng, arena, shape):
    """pla_diag.h: the fused route (weights pass, then the diagnostics kernel) and the kernel alone on two matrices with strides of
    their own."""
    from pyloo_amd.engine import _LOO_DIAG
    from test_gpu_loo_diagnostics import check

    n, s, dt, kind = shape
    ll = plant(seeded_ll(n, s, dt, 23 * s + n), kind)
    far, near = arena.far(ll, kind), fv.twin(ll, kind)
    taken_in_place(far, _LOO_DIAG)
    M = orc.tail_count(s, 1.0)
    a, b, text = both(eng, far, near, lambda t: eng.loo_diag(t, M, "psis"))
    assert ("diag_prepare_row_kernel" if kind == "rows" else "diag_prepare_tile_kernel") in text and "wave_loo_kernel<" in text, text
    assert "diag_wave_kernel" in text, text
    same_bits(shape, a, b, ("diag", "elpd_i", "ess_w", "var_log"))
    assert scalar(a["n_replaced"]) == 1 == scalar(b["n_replaced"])
    want = diag_ref.loo_diag(ll, 1.0, "psis", M=M)
    if dt == F8:
        check(str(shape), a, want)
    np.testing.assert_allclose(host(a["diag"]), want["diag"], rtol=1e-9 if dt == F8 else 1e-4)
    # the kernel alone: the log weights far in one layout, the log-likelihood in the other
    clean = np.where(np.isnan(ll), np.dtype(dt).type(-1e10), ll)
    lw = want["lw"].astype(dt)
    other = "lines" if kind == "rows" else "rows"
    fl, fll = arena.far(lw, kind), arena.far(clean, other, 3 * SECOND // 2)
    nl, nll = fv.twin(lw, kind), fv.twin(clean, other)
    c = eng.loo_diag_weights(fl, fll)
    kc = eng.last_kernels()
    d = eng.loo_diag_weights(nl, nll)
    assert kc == eng.last_kernels() and "in place" in kc, (kc, eng.last_kernels())
    same_bits(shape, c, d, ("elpd_i", "ess_w", "var_log"))
    if dt == F8:
        check(f"{shape} weights", c, diag_ref.from_log_weights(lw, clean))


# -------------------------------------------------------------------------------------------------------------------- mixis
@pytest.mark.parametrize("shape", MIXIS, ids=ids)
def test_mixis(eng, arena, shape):
    """All seven kernels of pla_mixis.h: the unit, strided and line kernels of pass 1; the wave, stream, column and block kernels
    of pass 2."""
    from pyloo_amd.engine import _IN_PLACE
    from test_gpu_mixture import case, check, expected_routes

    n, s, dt, kind = shape
    ll = plant(np.array(case(n, s, np.dtype(dt).type)[0]), kind)
    ll[0, 0] = -np.inf
    want = mixis_ref.mixis(ll)
    far, near = arena.far(ll, kind), fv.twin(ll, kind)
    taken_in_place(far, _IN_PLACE)
    one, two = expected_routes(far)
    assert (one, two) == expected_routes(near)
    a, b, text = both(eng, far, near, eng.mixis_draw_lse)
    assert one in text, (one, text)
    same_bits(shape, a, b, ("c", "n_replaced"))
    assert host(a["n_replaced"]).tolist() == [1, 1]
    a2, b2, text = both(eng, far, near, lambda t: eng.mixis_loo(t, c=a["c"]))
    assert two in text, (two, text)
    same_bits(shape, a2, b2, ("loo_i", "agg"))
    check(a2, want, n_replaced=2)
    a3, b3, text = both(eng, far, near, lambda t: eng.mixis_loo(t))  # (both passes in one call)
    same_bits(shape, a3, a2, ("loo_i", "c", "agg"))
    same_bits(shape, a3, b3, ("loo_i", "c", "agg"))


# -------------------------------------------------------------------------------------------------------------------- e_loo
@pytest.mark.parametrize("shape", E_LOO, ids=ids)
def test_e_loo_and_quantiles(eng, arena, shape):
    """pla_eloo.h: x, log_weights and log_ratios as three far views of equal strides, 2^20 + 64 elements apart."""
    from test_gpu_e_loo import same
    from test_gpu_e_loo_routes import QUANT_ULPS, bitwise

    n, s, dt, kind = shape
    rng = np.random.default_rng(29 * s + n)
    lr = (rng.uniform(0.1, 0.9, size=(n, 1)) * rng.exponential(size=(n, s))).astype(dt)
    x = plant((rng.normal(size=(n, s)) * 2.0 + 0.3).astype(dt), kind, counted=False)
    lw = orc.psislw(lr.astype(np.float64), 1.0)[0].astype(dt)
    fars = [arena.far(m, kind, j * SECOND) for j, m in enumerate((x, lw, lr))]
    nears = [fv.twin(m, kind) for m in (x, lw, lr)]
    assert fars[0].stride() == fars[1].stride() == fars[2].stride()
    kept = eng._promoted(fars, "x, log_weights and log_ratios", own_strides=False)[1]
    assert [t.data_ptr() for t in kept] == [t.data_ptr() for t in fars] and kept[0].stride() == fars[0].stride()
    a = eng.e_loo(*fars)
    ka = eng.last_kernels()
    b = eng.e_loo(*nears)
    assert ka == eng.last_kernels(), (ka, eng.last_kernels())
    assert ka.startswith("e_loo_wave_kernel<" if kind == "rows" else "e_loo_rows_kernel<"), ka  # (the wave kernel: aligned rows of unit stride)
    keys = ("mean", "var", "k_mean", "k_var", "k_none")
    same_bits(shape, a, b, keys)
    probs = np.array([0.01, 0.25, 0.5, 0.975])
    qa = eng.e_loo_quantiles(fars[0], fars[1], probs)
    kq = eng.last_kernels()
    qb = eng.e_loo_quantiles(nears[0], nears[1], probs)
    assert kq == eng.last_kernels(), (kq, eng.last_kernels())
    wave = kind == "rows" and s <= 4096  # (launch_e_loo_quantiles: unit stride, 16-byte aligned rows, at most 4096 draws)
    assert kq.startswith("e_loo_quantile_wave_kernel<" if wave else "e_loo_quantile_kernel<"), kq
    bad = n // 2 if kind == "lines" else n - 2
    ok = np.arange(n) != bad
    if wave:  # (the row with the NaN is declined and goes to the general kernel)
        bitwise(host(qa)[ok], host(qb)[ok], f"{shape}: quantiles of the wave kernel's rows")
    bitwise(host(qa), host(qb), f"{shape}: quantiles", QUANT_ULPS)
    want = orc.e_loo_arrays(x.astype(np.float64), lw.astype(np.float64), lr.astype(np.float64), probs=probs)
    rtol = 1e-9 if dt == F8 else 2e-5  # (tests/test_gpu_e_loo.py::test_golden_rows)
    got = {k: host(a[k]) for k in keys}
    same(got["mean"], want["mean"], rtol, "mean")
    same(got["var"], want["var"], rtol * 10, "variance")
    for key in ("k_mean", "k_var", "k_none"):
        same(got[key], want[key], 1e-14, key)
    assert np.flatnonzero(np.isnan(got["mean"])).tolist() == [bad]
    for q in (qa, qb):
        np.testing.assert_allclose(host(q)[ok], want["quant"][ok], rtol=1e-9 if dt == F8 else 3e-5, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------ loo_pit
@pytest.mark.parametrize("shape", PIT, ids=ids)
def test_loo_pit(eng, arena, shape):
    """The log-likelihood in one far layout and the predictive draws in the other: each matrix with its own strides."""
    n, s, dt, kind = shape
    other = "lines" if kind == "rows" else "rows"
    rng = np.random.default_rng(31 * s + n + len(kind))
    ll = plant(seeded_ll(n, s, dt, 31 * s + n), kind)
    y_hat = rng.normal(size=(n, s)).astype(dt)
    y = rng.normal(size=n)
    far = (arena.far(ll, kind), arena.far(y_hat, other, 3 * SECOND // 2))
    near = (fv.twin(ll, kind), fv.twin(y_hat, other))
    kept = eng._promoted(list(far), "mat and y_hat", own_strides=True, host_obs=True)[1]
    assert [(t.data_ptr(), t.stride()) for t in kept] == [(t.data_ptr(), t.stride()) for t in far]
    M = orc.tail_count(s, 1.0)
    a = eng.loo_pit(*far, y, M, "psis", "loglik")
    ka = eng.last_kernels()
    b = eng.loo_pit(*near, y, M, "psis", "loglik")
    assert ka == eng.last_kernels(), (ka, eng.last_kernels())
    assert ("pit_prepare_row_kernel" if kind == "rows" else "pit_prepare_tile_kernel") in ka and "pit_wave_kernel<" in ka, ka
    assert ("transpose_rows_kernel (y_hat)" in ka) == (kind == "rows"), ka  # (y_hat in the other layout: observations fastest)
    same_bits(shape, a, b, ("pit_le", "pit_lt", "diag"))
    assert scalar(a["n_replaced"]) == 1 == scalar(b["n_replaced"])
    want = pit_ref.loo_pit(ll.astype(np.float64), y_hat.astype(np.float64), y)
    if dt == F8:
        np.testing.assert_allclose(host(a["pit_le"]), want["pit_le"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(host(a["pit_lt"]), want["pit_lt"], rtol=0, atol=1e-9)
    else:  # (tests/test_gpu_loo_pit.py::test_golden_parity: the weights rounded to f32, their own tolerance propagated to first order)
        lw32 = want["lw"].astype(np.float32).astype(np.float64)
        want_le, want_lt = pit_ref.pit_from_log_weights(lw32, y_hat, y)
        wn = np.exp(lw32 - np.max(lw32, axis=1, keepdims=True))
        wn /= wn.sum(axis=1, keepdims=True)
        bound = (wn * (2e-7 * np.abs(lw32) + 1e-7)).sum(axis=1)
        assert np.all(np.abs(host(a["pit_le"]) - want_le) <= bound) and np.all(np.abs(host(a["pit_lt"]) - want_lt) <= bound)
    np.testing.assert_allclose(host(a["diag"]), want["diag"], rtol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------- lfo
@pytest.mark.parametrize("shape", LFO, ids=ids)
def test_lfo_ratios_and_lfo(eng, arena, shape):
    """The scan and carry kernels (two whole chunks and nine rows), the predict kernel, forward and backward."""
    from pyloo_amd.engine import _LFO

    n, s, dt, kind = shape
    first = 7
    ll = plant(lfo_ref.draw_ll(np.random.default_rng(37 * s + n), n, s, np.dtype(dt).type), kind)
    ll[n - 3, 1] = np.nan  # (a row the ratios read: their sums stop before the last row)
    far, near = arena.far(ll, kind), fv.twin(ll, kind)
    taken_in_place(far, _LFO)
    n_steps = n - first
    a, b, text = both(eng, far, near, lambda t: eng.lfo_ratios(t, first, n_steps))
    assert lfo_ref.CHUNK == fv.LC  # (what makes n two whole chunks and nine rows)
    assert "lfo_scan_kernel<" in text and "lfo_carry_kernel" in text, text
    same_bits(shape, a, b, ("ratios",))
    want = lfo_ref.ratios(ll, first, n_steps)
    assert np.array_equal(host(a["ratios"]), want, equal_nan=True)
    assert scalar(a["n_replaced"]) == int(np.isnan(ll[first:first + n_steps - 1]).sum()) == scalar(b["n_replaced"])
    tail = orc.tail_count(s, 1.0)
    for mode, ref_pass, start in (("forward", lfo_ref.lfo_pass, first), ("backward", lfo_bw_ref.lfo_pass, n)):
        ref = ref_pass(ll, start, n_steps, 1)
        a, b, text = both(eng, far, near, lambda t: eng.lfo(t, start, n_steps, 1, tail, 0.7, mode=mode))
        name = "lfo_" if mode == "forward" else "lfo_bw_"
        assert name + "scan_kernel<" in text and "lfo_carry_kernel" in text and name + "predict_kernel<" in text, text
        assert text.startswith("transpose_rows_kernel") == (kind == "lines"), text
        same_bits((shape, mode), a, b, ("diag", "elpd_i", "first_high", "n_replaced"))
        assert scalar(a["n_replaced"]) == ref["n_replaced"] >= 2
        k, k_ref = host(a["diag"]), ref["diag"]
        assert np.array_equal(np.isinf(k), np.isinf(k_ref))
        fin = np.isfinite(k_ref)
        np.testing.assert_allclose(k[fin], k_ref[fin], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(host(a["elpd_i"]), ref["elpd_i"], rtol=1e-9, atol=1e-10)


# ------------------------------------------------------------------------------------------------------------- relative_eff
@pytest.mark.parametrize("shape", ESS, ids=ids)
def test_relative_eff(eng, arena, shape):
    """pla_ess.h: four chains of 250 draws."""
    from pyloo_amd.engine import _LFO

    n, s, dt, kind = shape
    mat = ess_ref.ar1_rows(np.random.default_rng(41 * s + n), n, 4, s // 4, 0.5).astype(dt)
    plant(mat, kind, counted=False)
    far, near = arena.far(mat, kind), fv.twin(mat, kind)
    taken_in_place(far, _LFO)
    a, b, text = both(eng, far, near, lambda t: eng.relative_eff(t, 4))
    assert "ess_row_kernel<" in text and text.startswith("transpose_rows_kernel") == (kind == "lines"), text
    same_bits(shape, a, b, ("r_eff", "n_invalid"))
    bad = n // 2 if kind == "lines" else n - 2
    got = host(a["r_eff"])
    assert scalar(a["n_invalid"]) == 1 and np.flatnonzero(np.isnan(got)).tolist() == [bad]
    ok = np.arange(n) != bad
    want, margin, _ = ess_ref.relative_eff(mat[ok].astype(np.float64) if dt == F8 else mat[ok], 4)
    assert np.all(margin >= ess_ref.MARGIN_FLOOR)
    np.testing.assert_allclose(got[ok], want, rtol=1e-9, atol=1e-10)


# ------------------------------------------------------------------------------------------------------------ loo_influence
@pytest.mark.parametrize("theta_kind", ["rows", "lines"])
@pytest.mark.parametrize("shape", INFLUENCE, ids=ids)
def test_loo_influence(eng, arena, shape, theta_kind):
    """pla_influence.h: the matrix far on rows and on lines, the 21 quantities far as well -- one draw per far row, or as the ``.T``
    view of a buffer with one quantity per far line (21, not 20: an odd number of lines puts one on offset 2^32 and the last on
    2^33).  (A draw stride of 2^29 doubles would need 4 GiB per draw: the 1000 draws
    lie 8.6 MB apart instead, the first below 2^32 bytes and the last past 2^33.)"""
    from pyloo_amd.engine import _DeviceSpace, _LOO_DIAG
    from test_gpu_loo_influence import check

    n, s, dt, kind = shape
    rng = np.random.default_rng(43 * s + n)
    ll = plant(seeded_ll(n, s, dt, 43 * s + n), kind)
    theta = rng.normal(size=(s, 21))
    theta[:, :5] = influence_ref.make_theta(rng, s, 5)
    cen, sc = influence_ref.center_scale(theta)
    far, near = arena.far(ll, kind), fv.twin(ll, kind)
    taken_in_place(far, _LOO_DIAG)
    th_far, th_near = arena.far(theta, theta_kind, 2 * SECOND), fv.twin(theta, theta_kind)
    kept, strides = _DeviceSpace.dense(th_far)
    assert kept.data_ptr() == th_far.data_ptr() and tuple(strides) == tuple(th_far.stride())
    M = orc.tail_count(s, 1.0)
    a = eng.loo_influence(far, th_far, cen, sc, M, "psis", "loglik")
    ka = eng.last_kernels()
    b = eng.loo_influence(near, th_near, cen, sc, M, "psis", "loglik")
    assert ka == eng.last_kernels(), (ka, eng.last_kernels())
    assert ka.startswith("influence_prepare_kernel") and "influence_kernel<" in ka, ka
    assert ("diag_prepare_row_kernel" if kind == "rows" else "diag_prepare_tile_kernel") in ka, ka
    same_bits(shape, a, b, ("shift", "m2", "kl", "ess_w", "diag"))
    assert scalar(a["n_replaced"]) == 1 == scalar(b["n_replaced"])
    if dt == F8:
        want = influence_ref.loo_influence(ll, theta, M=M, center=cen, scale=sc)
        check(str(shape), a, want)
        np.testing.assert_allclose(host(a["diag"]), want["diag"], rtol=1e-9)


# ------------------------------------------------------------------------------------------------ group_sum, psis_loo_groups
@pytest.mark.parametrize("shape", GROUPS, ids=ids)
def test_group_sum_and_psis_loo_groups(eng, arena, shape):
    """pla_group.h: 40 observations in 5 interleaved groups."""
    from pyloo_amd.engine import _LOO
    from pyloo_amd.loo_group import group_index

    n, s, dt, kind = shape
    ll = plant(seeded_ll(n, s, dt, 47 * s + n, k_hi=0.6) / 4, kind)
    index = group_index(np.arange(n) % 5)
    far, near = arena.far(ll, kind), fv.twin(ll, kind)
    taken_in_place(far, _LOO)
    (sa, ca), (sb, cb), text = both(eng, far, near, lambda t: eng.group_sum(t, index.to(t.device)))
    assert "group_sum_kernel" in text and ("read in place" in text) == (kind == "rows") == (not text.startswith("transpose_rows_kernel")), text
    same_bits(shape, {"s": sa}, {"s": sb}, ("s",))
    want, n_nan = group_gather_ref.group_sums(ll, np.asarray(index.offsets), np.asarray(index.members))
    assert n_nan == 1 == scalar(ca) == scalar(cb)
    assert np.array_equal(host(sa), want)
    M = orc.tail_count(s, 1.0)
    a, b, text = both(eng, far, near, lambda t: eng.psis_loo_groups(t, index.to(t.device), M, "psis", 1.0, 0.7))
    assert "group_sum_kernel" in text and "then wave_loo_kernel<" in text, text
    same_bits(shape, a, b, ("diag", "logo_i", "lppd_i", "agg"))
    assert scalar(a["n_replaced"]) == 1 == scalar(b["n_replaced"])
    ref = orc.loo_pointwise(want.astype(np.float64), 1.0, "psis")
    close(a["diag"], ref["diag"], what="diag")
    close(a["logo_i"], ref["loo_i"], what="logo_i")
    close(a["lppd_i"], ref["lppd_i"], what="lppd_i")


# ------------------------------------------------------------------------------------------------ gather_draws, psis_loo_draws
@pytest.mark.parametrize("shape", DRAWS, ids=ids)
def test_gather_draws_and_psis_loo_draws(eng, arena, shape):
    """pla_draws.h: 300 indices, the last draw among them."""
    import torch

    from pyloo_amd.engine import _IN_PLACE

    n, s, dt, kind = shape
    ll = plant(seeded_ll(n, s, dt, 53 * s + n), kind)
    idx = np.random.default_rng(s).integers(0, s, size=300)
    idx[7], idx[299], idx[100] = s - 1, s - 1, s // 2  # (the planted NaN of either layout is gathered)
    dev_idx = torch.from_numpy(idx).cuda()
    far, near = arena.far(ll, kind), fv.twin(ll, kind)
    taken_in_place(far, _IN_PLACE)
    (ga, ca), (gb, cb), text = both(eng, far, near, lambda t: eng.gather_draws(t, dev_idx))
    assert text.startswith("gather_draws_kernel<lds" if kind == "rows" else "gather_draws_kernel<tile>") and "read in place" in text, text
    same_bits(shape, {"g": ga}, {"g": gb}, ("g",))
    want, n_nan = group_gather_ref.gather(ll, idx)
    assert n_nan >= 1 and scalar(ca) == n_nan == scalar(cb)
    assert np.array_equal(host(ga), want)
    M = orc.tail_count(300, 1.0)
    a, b, text = both(eng, far, near, lambda t: eng.psis_loo_draws(t, dev_idx, M, "psis", 1.0, 0.7))
    assert text.startswith("gather_draws_kernel<") and "then wave_loo_kernel<" in text, text
    same_bits(shape, a, b, ("diag", "loo_i", "lppd_i", "agg"))
    assert scalar(a["n_replaced"]) == n_nan == scalar(b["n_replaced"])
    check_loo(a, orc.loo_pointwise(want.astype(np.float64), 1.0, "psis"), shape)


# -------------------------------------------------------------------------------------------------------------------- kfold
@pytest.mark.parametrize("form", ["compact", "full"])
@pytest.mark.parametrize("shape", KFOLD, ids=ids)
def test_kfold(eng, arena, shape, form):
    """pla_kfold.h, all three task routes in one call: the full fit and the first fold source on far rows (``kfold_wave_kernel``), the
    second source on far lines (``kfold_lane_kernel``), the third with neither stride 1 (``kfold_block_kernel``), each with a far
    offset of its own; compact sources of three rows and full-form ones of nine."""
    from test_gpu_kfold import check_agg, check_pointwise, expected

    n, s, dt, kind = shape
    folds = np.arange(n) % 3 + 1
    full = plant(seeded_ll(n, s, dt, 59 * s + n), kind)
    mats = []
    for k in range(3):
        m = seeded_ll(n, s, dt, 61 * s + n + k)
        mats.append(m if form == "full" else np.ascontiguousarray(m[folds == k + 1]))
    if form == "compact":  # (a compact source has three rows: the least a far view takes)
        assert all(m.shape[0] == 3 for m in mats)
    fars = [arena.far(full, kind)] + [arena.far(m, k, (j + 1) * SECOND // 2) for j, (m, k) in enumerate(zip(mats, fv.KFOLD_SOURCES))]
    nears = [fv.twin(full, kind)] + [fv.twin(m, k) for m, k in zip(mats, fv.KFOLD_SOURCES)]
    f = __import__("torch").from_numpy(folds).cuda()
    plan = eng._kfold_plan(fars[0], fars[1:], f)
    assert plan["table"][0].tolist() == [t.data_ptr() for t in fars]
    assert plan["table"][3].tolist() == [t.stride(0) for t in fars] and plan["table"][4].tolist() == [t.stride(1) for t in fars]
    a = eng.kfold(fars[0], fars[1:], f)
    ka = eng.last_kernels()
    b = eng.kfold(nears[0], nears[1:], f)
    assert ka == eng.last_kernels(), (ka, eng.last_kernels())
    for route in ("kfold_wave_kernel", "kfold_lane_kernel", "kfold_block_kernel"):
        assert route in ka, ka
    assert "3 launches" in ka, ka
    same_bits(shape, a, b, ("elpd_i", "lpd_full_i", "p_i", "kfold_i", "agg"))
    lpd, elpd = expected(full, mats, folds)
    g = check_pointwise(a, lpd, elpd)
    check_agg(g, n_nan=1)


# ---------------------------------------------------------------------------------------------------------------------- glm
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("family", ["linpred", "gaussian", "binomial"])
def test_glm(eng, arena, family, transposed):
    """glm_prepare_kernel and glm_load_x: X (33, 17) with row 32 past 2^33 bytes and beta (250, 17) with its draws far apart; then
    both as ``.T`` views of buffers whose 17 predictors lie far apart."""
    from pyloo_amd.engine import _DeviceSpace
    from test_gpu_loo_glm import engine_vectors

    rng = np.random.default_rng(67 + len(family))
    m = glm_ref.make_model(rng, 33, 250, 17, "gaussian" if family == "linpred" else family, with_offset=True)
    fam, v = engine_vectors(m)
    if family == "linpred":
        fam, v = "linpred", dict(offset=m["offset"])
    if transposed:
        fx, fb = arena.far(m["X"], "lines"), arena.far(m["beta"], "lines", 2 * SECOND)
        nx, nb = fv.twin(m["X"], "lines"), fv.twin(m["beta"], "lines")
    else:
        fx, fb = arena.pitched(m["X"]), arena.pitched(m["beta"], 2 * SECOND)
        nx, nb = fv.twin_pitched(m["X"]), fv.twin_pitched(m["beta"])
    for t in (fx, fb):
        kept, strides = _DeviceSpace.dense(t)
        assert kept.data_ptr() == t.data_ptr() and tuple(strides) == tuple(t.stride()) and max(strides) * 8 > 2 ** 20
    a = eng.glm(fx, fb, fam, **v)
    ka = eng.last_kernels()
    b = eng.glm(nx, nb, fam, **v)
    assert ka == eng.last_kernels(), (ka, eng.last_kernels())
    assert ka.startswith("glm_prepare_kernel -> glm_kernel<") and "written in place" in ka, ka
    got = host(a)
    assert np.array_equal(got, host(b)) and np.all(np.isfinite(got))
    if family == "linpred":
        exact = glm_ref.linpred(m["X"], m["beta"], m["offset"], dtype=np.longdouble)
        err = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
        assert np.all(err <= glm_ref.linpred_bound(m["X"], m["beta"], m["offset"]))
    else:  # (tests/test_gpu_loo_glm.py: the density of the kernel's own linear predictor)
        eta = host(eng.glm(fx, fb, "linpred", offset=m["offset"]))
        want = glm_ref.density(fam, eta, m["y"], sigma=m["sigma"], trials=m["trials"], oc=v["obs_const"], dc=v["draw_const"])
        assert np.all(np.abs(got - want) <= 1e-10 * np.maximum(1.0, np.abs(want)))


# ------------------------------------------------------------------------------------------------------------- nonfactor
def nonfactor_call(eng, y, mu, mat, df, model):
    """``pla_nonfactor_loglik`` with the pitches of ``mu`` and ``mat`` as they are (``Engine.nonfactor_log_lik`` makes its inputs
    contiguous, so a far pitch reaches the library only through the C ABI)."""
    import torch

    from pyloo_amd import _capi

    S, N = mu.shape
    assert mu.stride(1) == 1 and mat.stride(2) == 1 and mat.stride(1) == N
    ll = torch.empty((N, S), dtype=torch.float64, device="cuda")
    flags = torch.empty(S, dtype=torch.int32, device="cuda")
    code = {"normal": _capi.PLA_MVN_NORMAL, "student_t": _capi.PLA_MVN_STUDENT_T}[model]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(eng._lib.pla_nonfactor_loglik(eng._h, y.data_ptr(), mu.data_ptr(), mat.data_ptr(), df.data_ptr() if model == "student_t" else None,
                                              _capi.PLA_F64 if mu.dtype == torch.float64 else _capi.PLA_F32, N, S, mu.stride(0), mat.stride(0),
                                              code, _capi.PLA_DEVICE, stream, ll.data_ptr(), S, 1, flags.data_ptr()))
    return ll, flags


@pytest.mark.parametrize("case", [(17, F8, 1, "normal"), (17, F4, 1, "student_t"), (150, F4, 2, "normal"), (150, F8, 2, "student_t"),
                                  (17, F8, 3, "student_t"), (150, F4, 3, "normal")], ids=ids)
def test_nonfactor_log_lik(arena, case):
    """pla_nonfactor.h with ``mat_pitch`` and ``mu_pitch`` far: five draws on the LDS route (N = 17), the blocked route (N = 150) and
    the forced general route."""
    import torch

    from pyloo_amd.engine import get_engine
    from test_gpu_nonfactor import ROUTE_NAMES, close as nf_close, spd_draws

    N, dt, route, model = case
    eng = get_engine(0)
    y, mu, cov, df = (a.astype(dt) for a in spd_draws(N, 5, seed=N))
    ref, rflags = nonfactor_ref.loglik(y.astype(np.float64), mu.astype(np.float64), cov.astype(np.float64), df.astype(np.float64), model)
    yd, dfd = torch.from_numpy(y).cuda(), torch.from_numpy(df).cuda()
    fm, fc = arena.pitched(mu, 2 * SECOND), arena.pitched(cov)
    nm, nc = fv.twin_pitched(mu), fv.twin_pitched(cov)
    assert fm.stride(0) * fm.element_size() > 2 ** 28 and fc.stride(0) * fc.element_size() > 2 ** 28
    try:
        eng.set_nonfactor_route(route)
        a = nonfactor_call(eng, yd, fm, fc, dfd, model)
        ka = eng.last_kernels()
        b = nonfactor_call(eng, yd, nm, nc, dfd, model)
        assert ka == eng.last_kernels() and ROUTE_NAMES[route] in ka, (ka, eng.last_kernels())
    finally:
        eng.set_nonfactor_route(0)
    assert np.array_equal(host(a[0]), host(b[0]), equal_nan=True) and np.array_equal(host(a[1]), host(b[1]))
    assert np.array_equal(host(a[1]) & ~nonfactor_ref.GENERAL, rflags)
    nf_close(host(a[0]), ref, 1e-9)  # (f32 input is widened on load: the reference on the same values)


# ------------------------------------------------------------------------------------------------------------------ compare
@pytest.mark.parametrize("dt", [F8, F4])
def test_compare_passes(eng, arena, dt):
    """pla_compare.h with ``pitch`` far: three models of 300 observations."""
    from compare_cases import pointwise
    from test_gpu_compare_shapes import SEED, check_moments, check_stacking, condition, relerr, same_bits as bits

    x = pointwise(71, 3, 300, "deviance").astype(dt)
    w = np.random.default_rng(71).dirichlet(np.ones(3))
    G = gamma_draws(SEED, 0.5, 65, 300)
    assert condition(x, G) < 2000  # (what makes 1e-12 hold: tests/test_gpu_compare_shapes.py)
    far, near = arena.pitched(x), fv.twin_pitched(x)
    sp, kept, dims = eng._compare_input(far)
    assert kept.data_ptr() == far.data_ptr() and dims[3] == far.stride(0) and far.stride(0) * far.element_size() > 2 ** 28
    a, b, text = both(eng, far, near, lambda t: eng.compare_moments(t, 1))
    assert text.startswith("compare_moments_kernel<"), text
    assert bits(a, b)
    check_moments(a, x, 1, f"moments {dt}")
    (Fa, Ga), (Fb, Gb), text = both(eng, far, near, lambda t: eng.stacking_eval(t, w, -0.5))
    assert text.startswith("stacking_eval_kernel<"), text
    assert Fa == Fb and bits(Ga, Gb)
    check_stacking((Fa, Ga), x, w, -0.5, f"stacking {dt}")
    za, zb, text = both(eng, far, near, lambda t: eng.bb_bootstrap(t, 65, 0.5, SEED, -0.5))
    assert text.startswith("bb_bootstrap_kernel<"), text
    assert bits(za, zb)
    assert relerr(host(za), bb_z_from_gammas(G, x, -0.5)) <= 1e-12


# ------------------------------------------------------------------------------------------------------------- mm_transform
@pytest.mark.parametrize("with_map", [False, True])
def test_mm_transform(eng, arena, with_map):
    """mm_affine_kernel and mm_map_kernel with ``x_batch_stride`` far: B = 3 batches of (257, 17) (``Engine.mm_transform`` makes
    ``x`` contiguous, so a far batch stride reaches the library only through the C ABI)."""
    import torch

    from pyloo_amd import _capi
    from test_gpu_moment_match import close as mm_close

    B, S, D = 3, 257, 17
    rng = np.random.default_rng(73)
    x = rng.normal(size=(B, S, D))
    m0, m1, pre = rng.normal(size=(B, D)), rng.normal(size=(B, D)), rng.uniform(0.5, 2.0, size=(B, D))
    mapping = rng.normal(size=(B, D, D)) / np.sqrt(D) if with_map else None
    dev = [None if a is None else torch.from_numpy(a).cuda() for a in (m0, pre, mapping, m1)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(xv):
        assert xv.stride(1) == D and xv.stride(2) == 1
        out = torch.empty((B, S, D), dtype=torch.float64, device="cuda")
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _capi.check(eng._lib.pla_mm_transform(eng._h, xv.data_ptr(), xv.stride(0), ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), None, ptr(dev[3]),
                                              B, S, D, 0, S, stream, out.data_ptr()))
        return out

    far, near = arena.pitched(x), fv.twin_pitched(x)
    assert far.stride(0) * 8 > 2 ** 31
    a, b, text = both(eng, far, near, run)
    assert text == ("mm_map_kernel" if with_map else "mm_affine_kernel"), text
    assert torch.equal(a, b)
    z = (x - m0[:, None]) * pre[:, None]
    want = (np.einsum("bsd,bed->bse", z, mapping) if with_map else z) + m1[:, None]
    mm_close(host(a), want, 1e-10, 1e-11, what="transform")


# ------------------------------------------------------------------------------------------- a small stride, a large index
def test_true_size_f32_matrix_past_element_2_31(eng, arena):
    """The other half: rows of unit stride whose element index passes 2^31.  The top of the arena as a contiguous f32 matrix of
    540 001 x 4000 (2.16e9 elements, 8.64 GB), a NaN in its very last element and a constant row at 536 871, the first row whose
    elements all lie past element 2^31; then the same numbers transposed into the bottom of the arena and read observations
    fastest by the column kernels.  (The bottom copy ends 168 MB below the top one: the arena's halves are 8.59 GB and 8.86 GB.)"""
    import torch

    from test_gpu_parity import close as parity_close
    from test_gpu_waic_routes import RTOL as WAIC_RTOL
    from waic_ref import waic_ref

    N, S = 540_001, 4000
    assert 536_871 * S >= 2 ** 31 > 536_870 * S
    nbytes = N * S * 4
    start = (fv.ARENA_BYTES - nbytes) // 256 * 256
    assert nbytes <= start  # the two copies do not overlap
    try:
        t = fv.strided_view(arena.t, torch.float32, (N, S), (S, 1), start)
        eng.fill_synthetic(t, seed=20262, k_lo=0.05, k_hi=1.1)
        t[N - 1, S - 1] = float("nan")
        t[536_871] = -3.0
        M = orc.tail_count(S, 1.0)
        b = eng.psis_loo(t, M, "psis", 1.0, 0.7)
        rows_text = eng.last_kernels()
        w = eng.waic(t, 1.0)
        assert "waic_wave_kernel" in eng.last_kernels(), eng.last_kernels()
        low = fv.strided_view(arena.t, torch.float32, (S, N), (N, 1), 0)
        low.copy_(t.T)
        view = low.T
        assert view.shape == (N, S) and view.stride() == (1, N)
        a = eng.psis_loo(view, M, "psis", 1.0, 0.7)
        assert "col_sweep_kernel" in eng.last_kernels() and "col_sweep_kernel" not in rows_text, (eng.last_kernels(), rows_text)
        wc = eng.waic(view, 1.0)
        assert "waic_col_kernel" in eng.last_kernels(), eng.last_kernels()
        torch.cuda.synchronize()
        for key in ("diag", "loo_i", "lppd_i"):  # (tests/test_gpu_parity.py::test_column_kernels_on_observation_fastest_matrices)
            x, y = host(a[key]), host(b[key])
            assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(np.isinf(x), np.isinf(y)), key
            ok = np.isfinite(y)
            np.testing.assert_allclose(x[ok], y[ok], rtol=1e-10, atol=1e-11, err_msg=key)
        idx = np.r_[0:20, 536_860:536_885, 539_980:N]
        sample = t[torch.from_numpy(idx).cuda()].cpu().numpy()
        assert np.isnan(sample).sum() == 1 and np.all(sample[20 + 11] == -3.0)
        ref = orc.loo_arrays(sample.astype(np.float64), 1.0)
        for res in (a, b):
            parity_close(host(res["diag"])[idx], ref["khat"], what="khat")
            parity_close(host(res["loo_i"])[idx], ref["loo_i"], what="loo_i")
            parity_close(host(res["lppd_i"])[idx], ref["lppd_i"], what="lppd_i")
        want = waic_ref(sample, 1.0)
        for res in (w, wc):
            assert int(host(res["agg"])[7]) == 1 and int(host(res["agg"])[0]) == N
            np.testing.assert_allclose(host(res["lppd_i"])[idx], want["lppd_i"], rtol=WAIC_RTOL, atol=1e-12)
            np.testing.assert_allclose(host(res["waic_i"])[idx], want["waic_i"], rtol=WAIC_RTOL, atol=1e-10)
    finally:
        arena.t.fill_(0xFF)  # the whole arena: both copies lay outside the far views' bookkeeping
