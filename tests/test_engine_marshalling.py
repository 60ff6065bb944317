"""What ``Engine`` hands to the C ABI for host (NumPy) input: every scalar and, for pointers, which array they address.

No library is loaded: the engine is built with ``object.__new__`` around a fake ``_lib`` that records each ``pla_*`` call.
The expectations are written out by hand from include/pyloo_amd.h and the documented layout rules, not derived from the
code under test."""

import ctypes as C
import itertools
import types

import numpy as np
import pytest

from pyloo_amd import _capi
from pyloo_amd.engine import Engine

H = 0x1234  # the engine handle the fake engine carries
F64, F32, HOST = 0, 1, 0
PSIS, SIS, TIS = 0, 1, 2
DTYPES = [np.float64, np.float32]
CODE = {np.float64: F64, np.float32: F32}


def _addr(a):
    """The address a pointer argument carries: None, an integer, a ``c_void_p`` or a ``byref``."""
    if a is None or isinstance(a, int):
        return a
    if hasattr(a, "_obj"):
        return C.addressof(a._obj)
    return a.value


def _fields(s):
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Array):
            v = [_fields(e) for e in v]
        elif isinstance(v, C.Structure):
            v = _fields(v)
        out[name] = v
    return out


class Recorder:
    """``pla_*`` functions that store ``(name, args)`` and return 0.  ``writes[name][position or field]``: an int64 written
    through that pointer; ``peek[name][position] = (dtype, count)``: what the pointer addresses, copied during the call."""

    def __init__(self, writes=None, peek=None):
        self.calls, self.seen = [], {}
        self._writes, self._peek = writes or {}, peek or {}

    def __getattr__(self, name):
        if not name.startswith("pla_"):
            raise AttributeError(name)

        def call(*args):
            writes = self._writes.get(name, {})
            if len(args) == 1 and hasattr(args[0], "_obj") and isinstance(args[0]._obj, C.Structure):
                rec = _fields(args[0]._obj)
                flat = rec.get("glm", rec)
                for field, value in writes.items():
                    C.c_int64.from_address(flat[field]).value = value
                self.calls.append((name, rec))
                return 0
            norm = [_addr(a) if (hasattr(a, "_obj") or isinstance(a, C.c_void_p)) else a for a in args]
            for pos, value in writes.items():
                C.c_int64.from_address(norm[pos]).value = value
            for pos, (dtype, count) in self._peek.get(name, {}).items():
                self.seen[name, pos] = np.ctypeslib.as_array(C.cast(norm[pos], C.POINTER(np.ctypeslib.as_ctypes_type(dtype))),
                                                             (count,)).copy()
            self.calls.append((name, norm))
            return 0

        return call


class Other:
    """A pointer to memory of the engine's own: not NULL and none of the given arrays (a copy, an internal buffer)."""

    def __init__(self, *not_these):
        self.not_these = [a.ctypes.data for a in not_these]


def make(writes=None, peek=None):
    eng = object.__new__(Engine)
    eng._lib, eng._h, eng.device = Recorder(writes, peek), C.c_void_p(H), 0
    return eng, eng._lib


def expect(call, name, want):
    got_name, got = call
    assert got_name == name
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray):
            assert g == w.ctypes.data, f"argument {i}: not the address of the expected array"
        elif isinstance(w, Other):
            assert isinstance(g, int) and g != 0 and g not in w.not_these, f"argument {i}: {g!r}"
        elif w is None:
            assert g is None, f"argument {i}: {g!r} is not NULL"
        else:
            assert g is not None and g == w and isinstance(g, float) == isinstance(w, float), f"argument {i}: {g!r} != {w!r}"


def expect_fields(rec, want):
    for k, w in want.items():
        expect(("f", [rec[k]]), "f", [w])


def out_f64(x, shape):
    assert isinstance(x, np.ndarray) and x.dtype == np.float64 and x.shape == tuple(shape) and x.flags.c_contiguous
    return x


def last(lib, n=1):
    assert len(lib.calls) == n, [c[0] for c in lib.calls]
    return lib.calls[-1]


# ---------------------------------------------------------------------------------------------------------- layouts
def _loo_matrix_args(a, rows=None):
    """(call name, [mat, dtype, n, s, stride_obs, stride_draw]) of ``psis_loo(a, rows=rows)``."""
    eng, lib = make(peek={"pla_psis_loo": {1: (a.dtype.type if a.dtype.kind == "f" else np.float64, a.size)},
                          "pla_psis_loo_rows": {1: (a.dtype.type if a.dtype.kind == "f" else np.float64, a.size)}})
    eng.psis_loo(a, rows=rows)
    name, args = last(lib)
    return name, args[1:7], lib.seen[name, 1]


@pytest.mark.parametrize("dt", DTYPES)
def test_layouts_taken_in_place(dt):
    a = np.arange(35, dtype=dt).reshape(5, 7)
    name, got, _ = _loo_matrix_args(a)
    expect((name, got), "pla_psis_loo", [a, CODE[dt], 5, 7, 7, 1])
    one = np.arange(7, dtype=dt).reshape(1, 7)
    expect(_loo_matrix_args(one)[:2], "pla_psis_loo", [one, CODE[dt], 1, 7, 7, 1])
    pitched = np.zeros((5, 9), dtype=dt)[:, :7]
    expect(_loo_matrix_args(pitched)[:2], "pla_psis_loo", [pitched, CODE[dt], 5, 7, 9, 1])
    obs = np.zeros((7, 5), dtype=dt).T  # observations fastest
    expect(_loo_matrix_args(obs)[:2], "pla_psis_loo", [obs, CODE[dt], 5, 7, 1, 5])
    padded = np.zeros((7, 8), dtype=dt)[:, :5].T
    expect(_loo_matrix_args(padded)[:2], "pla_psis_loo", [padded, CODE[dt], 5, 7, 1, 8])


@pytest.mark.parametrize("dt", DTYPES)
def test_layouts_that_are_copied(dt):
    base = np.arange(35, dtype=dt).reshape(7, 5)
    obs = base.T
    name, got, data = _loo_matrix_args(obs, rows=[4, 0])  # a row selection: no observations-fastest
    expect((name, got), "pla_psis_loo_rows", [Other(base), CODE[dt], 5, 7, 7, 1])
    assert np.array_equal(data, np.ascontiguousarray(obs).ravel())
    a = np.arange(35, dtype=dt).reshape(5, 7)
    name, got, data = _loo_matrix_args(a[::-1])
    expect((name, got), "pla_psis_loo", [Other(a), CODE[dt], 5, 7, 7, 1])
    assert np.array_equal(data, a[::-1].ravel())
    name, got, data = _loo_matrix_args(a[:, ::2])
    expect((name, got), "pla_psis_loo", [Other(a), CODE[dt], 5, 4, 4, 1])
    assert np.array_equal(data, a[:, ::2].ravel())


def test_a_matrix_of_integers_is_taken_as_f64():
    a = np.arange(35, dtype=np.int64).reshape(5, 7)
    name, got, data = _loo_matrix_args(a)
    expect((name, got), "pla_psis_loo", [Other(a), F64, 5, 7, 7, 1])
    assert data.dtype == np.float64 and np.array_equal(data, np.arange(35.0))


@pytest.mark.parametrize("dt", DTYPES)
def test_weights_passes_copy_an_observations_fastest_matrix(dt):
    base = np.arange(35, dtype=dt).reshape(7, 5)
    obs, c = base.T, np.zeros((5, 7), dtype=dt)
    eng, lib = make(peek={"pla_importance_weights": {1: (dt, 35)}, "pla_loo_diag_weights": {1: (dt, 35)}})
    lw, diag = eng.importance_weights(obs, 4, "tis")
    assert lw.dtype == dt and lw.shape == (5, 7) and lw.flags.c_contiguous
    expect(last(lib), "pla_importance_weights", [H, Other(base), CODE[dt], 5, 7, 7, 1, TIS, 4, HOST, None, lw, out_f64(diag, (5,))])
    assert np.array_equal(lib.seen["pla_importance_weights", 1], np.ascontiguousarray(obs).ravel())
    r = eng.loo_diag_weights(obs, c)
    assert sorted(r) == ["elpd_i", "ess_w", "var_log"]
    expect(last(lib, 2), "pla_loo_diag_weights", [H, Other(base), c, CODE[dt], 5, 7, 7, 1, 7, 1, HOST, None] +
           [out_f64(r[k], (5,)) for k in ("elpd_i", "ess_w", "var_log")])
    assert np.array_equal(lib.seen["pla_loo_diag_weights", 1], np.ascontiguousarray(obs).ravel())


# ---------------------------------------------------------------------------------------------------------- LOO, WAIC
@pytest.mark.parametrize("dt", DTYPES)
def test_psis_loo(dt):
    a = np.zeros((5, 7), dtype=dt)
    eng, lib = make()
    r = eng.psis_loo(a, 3, "sis", 2.0, 0.5)
    assert sorted(r) == ["agg", "diag", "loo_i", "lppd_i"] and not r["agg"].any()
    expect(last(lib), "pla_psis_loo", [H, a, CODE[dt], 5, 7, 7, 1, SIS, 3, 2.0, 0.5, HOST, None] +
           [out_f64(r[k], (5,)) for k in ("diag", "loo_i", "lppd_i")] + [out_f64(r["agg"], (8,))])
    r = eng.psis_loo(a, pointwise=False)
    assert r["diag"] is None and r["loo_i"] is None and r["lppd_i"] is None
    expect(last(lib, 2), "pla_psis_loo", [H, a, CODE[dt], 5, 7, 7, 1, PSIS, 0, 1.0, 0.7, HOST, None, None, None, None, out_f64(r["agg"], (8,))])
    r = eng.psis_loo(a, aggregate=False)
    assert r["agg"] is None
    expect(last(lib, 3), "pla_psis_loo", [H, a, CODE[dt], 5, 7, 7, 1, PSIS, 0, 1.0, 0.7, HOST, None] +
           [out_f64(r[k], (5,)) for k in ("diag", "loo_i", "lppd_i")] + [None])


@pytest.mark.parametrize("dt", DTYPES)
def test_psis_loo_rows(dt):
    a = np.zeros((5, 7), dtype=dt)
    idx = np.array([4, 0, 4], dtype=np.int64)
    eng, lib = make(peek={"pla_psis_loo_rows": {7: (np.int64, 2)}})
    r = eng.psis_loo(a, 3, "psis", 1.0, 0.7, rows=idx)
    expect(last(lib), "pla_psis_loo_rows", [H, a, CODE[dt], 5, 7, 7, 1, idx, 3, PSIS, 3, 1.0, 0.7, HOST, None] +
           [out_f64(r[k], (3,)) for k in ("diag", "loo_i", "lppd_i")] + [out_f64(r["agg"], (8,))])
    r = eng.psis_loo(a, rows=[3, 1], pointwise=False, aggregate=False)  # a list becomes an int64 array of the engine's
    assert r == {"diag": None, "loo_i": None, "lppd_i": None, "agg": None}
    expect(last(lib, 2), "pla_psis_loo_rows", [H, a, CODE[dt], 5, 7, 7, 1, Other(idx), 2, PSIS, 0, 1.0, 0.7, HOST, None, None, None, None, None])
    assert lib.seen["pla_psis_loo_rows", 7].tolist() == [3, 1]


@pytest.mark.parametrize("dt", DTYPES)
def test_waic(dt):
    obs = np.zeros((7, 5), dtype=dt).T
    idx = np.array([2, 2], dtype=np.int64)
    eng, lib = make()
    r = eng.waic(obs, 2.0)
    assert sorted(r) == ["agg", "lppd_i", "var_i", "waic_i"] and not r["agg"].any()
    expect(last(lib), "pla_waic", [H, obs, CODE[dt], 5, 7, 1, 5, 2.0, HOST, None] +
           [out_f64(r[k], (5,)) for k in ("lppd_i", "var_i", "waic_i")] + [out_f64(r["agg"], (8,))])
    r = eng.waic(obs, pointwise=False)
    expect(last(lib, 2), "pla_waic", [H, obs, CODE[dt], 5, 7, 1, 5, 1.0, HOST, None, None, None, None, out_f64(r["agg"], (8,))])
    a = np.zeros((5, 7), dtype=dt)
    r = eng.waic(a, -2.0, aggregate=False, rows=idx)
    assert r["agg"] is None
    expect(last(lib, 3), "pla_waic_rows", [H, a, CODE[dt], 5, 7, 7, 1, idx, 2, -2.0, HOST, None] +
           [out_f64(r[k], (2,)) for k in ("lppd_i", "var_i", "waic_i")] + [None])
    eng.waic(obs, rows=idx)  # copied: a row selection takes no observations-fastest matrix
    expect((lib.calls[-1][0], lib.calls[-1][1][:7]), "pla_waic_rows", [H, Other(obs), CODE[dt], 5, 7, 7, 1])


@pytest.mark.parametrize("dt", DTYPES)
def test_reduce_pointwise(dt):
    d, l, p = (np.zeros(6) for _ in range(3))
    eng, lib = make()
    agg = eng.reduce_pointwise(d, l, p, 0.6)
    assert not agg.any()
    expect(last(lib), "pla_reduce_pointwise", [H, d, l, p, 6, 0.6, HOST, None, out_f64(agg, (8,))])
    d2 = d.astype(dt)  # taken as f64
    eng.reduce_pointwise(d2, l, p, 0.6)
    expect(last(lib, 2), "pla_reduce_pointwise", [H, d2 if dt == np.float64 else Other(d2), l, p, 6, 0.6, HOST, None, Other(agg)])


# ---------------------------------------------------------------------------------------------------------- groups, draws
def _index():
    return types.SimpleNamespace(offsets=np.array([0, 2, 5], dtype=np.int64), members=np.array([3, 1, 0, 2, 4], dtype=np.int64), n_groups=2)


@pytest.mark.parametrize("dt", DTYPES)
def test_group_sum_and_psis_loo_groups(dt):
    obs = np.zeros((7, 5), dtype=dt).T
    gi = _index()
    eng, lib = make(writes={"pla_group_sum": {13: 7}, "pla_psis_loo_groups": {20: 7}})
    out, nrep = eng.group_sum(obs, gi)
    assert type(nrep) is int and nrep == 7
    assert out.dtype == dt and out.shape == (2, 7) and out.flags.c_contiguous
    expect(last(lib), "pla_group_sum", [H, obs, CODE[dt], 5, 7, 1, 5, gi.offsets, gi.members, 2, HOST, None, out, Other(out)])
    r = eng.psis_loo_groups(obs, gi, 3, "tis", 2.0, 0.5)
    assert sorted(r) == ["agg", "diag", "logo_i", "lppd_i", "n_replaced"] and type(r["n_replaced"]) is int and r["n_replaced"] == 7
    assert not r["agg"].any()
    expect(last(lib, 2), "pla_psis_loo_groups", [H, obs, CODE[dt], 5, 7, 1, 5, gi.offsets, gi.members, 2, TIS, 3, 2.0, 0.5, HOST, None] +
           [out_f64(r[k], (2,)) for k in ("diag", "logo_i", "lppd_i")] + [out_f64(r["agg"], (8,)), Other(r["agg"])])
    r = eng.psis_loo_groups(np.zeros((5, 7), dtype=dt), gi, pointwise=False, aggregate=False)
    assert lib.calls[-1][1][16:20] == [None, None, None, None] and lib.calls[-1][1][3:7] == [5, 7, 7, 1]


@pytest.mark.parametrize("dt", DTYPES)
def test_gather_draws_and_psis_loo_draws(dt):
    a = np.zeros((5, 7), dtype=dt)
    idx = np.array([6, 0, 6, 2], dtype=np.int64)
    eng, lib = make(writes={"pla_gather_draws": {12: 7}, "pla_psis_loo_draws": {19: 7}})
    out, nrep = eng.gather_draws(a, idx)
    assert type(nrep) is int and nrep == 7
    assert out.dtype == dt and out.shape == (5, 4) and out.flags.c_contiguous
    expect(last(lib), "pla_gather_draws", [H, a, CODE[dt], 5, 7, 7, 1, idx, 4, HOST, None, out, Other(out)])
    obs = np.zeros((7, 5), dtype=dt).T
    r = eng.psis_loo_draws(obs, idx, 2, "psis", 1.5, 0.6)
    assert sorted(r) == ["agg", "diag", "loo_i", "lppd_i", "n_replaced"] and type(r["n_replaced"]) is int and r["n_replaced"] == 7
    assert not r["agg"].any()
    expect(last(lib, 2), "pla_psis_loo_draws", [H, obs, CODE[dt], 5, 7, 1, 5, idx, 4, PSIS, 2, 1.5, 0.6, HOST, None] +
           [out_f64(r[k], (5,)) for k in ("diag", "loo_i", "lppd_i")] + [out_f64(r["agg"], (8,)), Other(r["agg"])])
    r = eng.psis_loo_draws(a, [1], pointwise=False, aggregate=False)
    assert lib.calls[-1][1][15:19] == [None, None, None, None] and lib.calls[-1][1][8] == 1


# ---------------------------------------------------------------------------------------------------------- Mix-IS
@pytest.mark.parametrize("dt", DTYPES)
def test_mixis(dt):
    obs = np.zeros((7, 8), dtype=dt)[:, :5].T
    eng, lib = make()
    r = eng.mixis_draw_lse(obs)
    assert sorted(r) == ["c", "n_replaced"]
    assert r["n_replaced"].dtype == np.int64 and r["n_replaced"].shape == (2,) and not r["n_replaced"].any() and not r["c"].any()
    expect(last(lib), "pla_mixis_draw_lse", [H, obs, CODE[dt], 5, 7, 1, 8, HOST, None, out_f64(r["c"], (7,)), r["n_replaced"]])
    c = np.ones(7)
    r = eng.mixis_loo(obs, c, 2.0)
    assert sorted(r) == ["agg", "c", "loo_i"] and r["c"] is c and not r["agg"].any() and not r["loo_i"].any()
    expect(last(lib, 2), "pla_mixis_loo", [H, obs, CODE[dt], 5, 7, 1, 8, c, 2.0, HOST, None, out_f64(r["loo_i"], (5,)), out_f64(r["agg"], (8,))])
    r = eng.mixis_loo(obs, None, pointwise=False, aggregate=False)  # pass 1 runs first
    assert [n for n, _ in lib.calls[2:]] == ["pla_mixis_draw_lse", "pla_mixis_loo"]
    expect(lib.calls[-1], "pla_mixis_loo", [H, obs, CODE[dt], 5, 7, 1, 8, out_f64(r["c"], (7,)), 1.0, HOST, None, None, None])
    with pytest.raises(ValueError, match=r"c must have one entry per draw: expected \(7,\), got \(6,\)"):
        eng.mixis_loo(obs, np.ones(6))


# ---------------------------------------------------------------------------------------------------------- weighted expectations
def test_e_loo_promotes_to_one_dtype():
    x32, lw64, lr32 = np.zeros((5, 7), np.float32), np.zeros((5, 7)), np.zeros((5, 7), np.float32)
    keys = ("mean", "var", "k_mean", "k_var", "k_none")
    eng, lib = make()
    r = eng.e_loo(x32, lw64, lr32, 11)
    assert tuple(r) == keys
    expect(last(lib), "pla_e_loo", [H, Other(x32), lw64, Other(lr32), F64, 5, 7, 7, 1, 11, HOST, None] + [out_f64(r[k], (5,)) for k in keys])
    lw32 = np.zeros((5, 7), np.float32)
    r = eng.e_loo(x32, lw32)
    expect(last(lib, 2), "pla_e_loo", [H, x32, lw32, None, F32, 5, 7, 7, 1, 20, HOST, None] + [out_f64(r[k], (5,)) for k in keys])
    obs = np.zeros((7, 5)).T  # always passed draws-fastest
    r = eng.e_loo(obs, lw64)
    expect(last(lib, 3), "pla_e_loo", [H, Other(obs), lw64, None, F64, 5, 7, 7, 1, 20, HOST, None] + [out_f64(r[k], (5,)) for k in keys])


def test_e_loo_quantiles_promotes_to_one_dtype():
    x32, lw64, lw32 = np.zeros((5, 7), np.float32), np.zeros((5, 7)), np.zeros((5, 7), np.float32)
    eng, lib = make(peek={"pla_e_loo_quantiles": {8: (np.float64, 2)}})
    q = eng.e_loo_quantiles(x32, lw64, [0.1, 0.9])
    expect(last(lib), "pla_e_loo_quantiles", [H, Other(x32), lw64, F64, 5, 7, 7, 1, Other(lw64), 2, HOST, None, out_f64(q, (5, 2))])
    assert lib.seen["pla_e_loo_quantiles", 8].tolist() == [0.1, 0.9]
    q = eng.e_loo_quantiles(x32, lw32, 0.5)
    expect(last(lib, 2), "pla_e_loo_quantiles", [H, x32, lw32, F32, 5, 7, 7, 1, Other(lw32), 1, HOST, None, out_f64(q, (5, 1))])


@pytest.mark.parametrize("dt", DTYPES)
def test_loo_pit(dt):
    mat, y_hat, y = np.zeros((5, 7), dtype=dt), np.zeros((7, 5), dtype=dt).T, np.zeros(5)
    eng, lib = make(writes={"pla_loo_pit": {19: 7}})
    r = eng.loo_pit(mat, y_hat, y, 3, "sis")
    assert sorted(r) == ["diag", "n_replaced", "pit_le", "pit_lt"] and type(r["n_replaced"]) is int and r["n_replaced"] == 7
    expect(last(lib), "pla_loo_pit", [H, mat, y_hat, y, CODE[dt], 5, 7, 7, 1, 1, 5, 0, SIS, 3, HOST, None] +
           [out_f64(r[k], (5,)) for k in ("pit_le", "pit_lt", "diag")] + [Other(r["diag"])])
    r = eng.loo_pit(y_hat, mat, y, kind="log_weights")
    assert r["diag"] is None and r["n_replaced"] == 7
    expect(last(lib, 2), "pla_loo_pit", [H, y_hat, mat, y, CODE[dt], 5, 7, 1, 5, 7, 1, 1, PSIS, 0, HOST, None,
                                         out_f64(r["pit_le"], (5,)), out_f64(r["pit_lt"], (5,)), None, Other(y)])
    if dt == np.float32:  # a mixed pair is taken as f64: the f32 matrix is copied, the f64 one stays
        m64 = np.zeros((5, 7))
        eng.loo_pit(m64, y_hat, y)
        expect((lib.calls[-1][0], lib.calls[-1][1][:11]), "pla_loo_pit", [H, m64, Other(y_hat), y, F64, 5, 7, 7, 1, 1, 5])
    with pytest.raises(ValueError, match="y has 4 values for 5 observations"):
        eng.loo_pit(mat, y_hat, np.zeros(4))
    with pytest.raises(ValueError, match="kind must be 'loglik' or 'log_weights', got 'x'"):
        eng.loo_pit(mat, y_hat, y, kind="x")


# ---------------------------------------------------------------------------------------------------------- diagnostics
@pytest.mark.parametrize("dt", DTYPES)
def test_loo_diag(dt):
    obs = np.zeros((7, 5), dtype=dt).T
    idx = np.array([1, 3], dtype=np.int64)
    keys = ("diag", "elpd_i", "ess_w", "var_log")
    eng, lib = make(writes={"pla_loo_diag": {17: 7}})
    r = eng.loo_diag(obs, 3, "tis")
    assert sorted(r) == sorted(keys + ("n_replaced",)) and type(r["n_replaced"]) is int and r["n_replaced"] == 7
    expect(last(lib), "pla_loo_diag", [H, obs, CODE[dt], 5, 7, 1, 5, None, 5, TIS, 3, HOST, None] + [out_f64(r[k], (5,)) for k in keys] +
           [Other(r["diag"])])
    r = eng.loo_diag(obs, rows=idx)
    assert r["n_replaced"] == 7
    expect(last(lib, 2), "pla_loo_diag", [H, Other(obs), CODE[dt], 5, 7, 7, 1, idx, 2, PSIS, 0, HOST, None] + [out_f64(r[k], (2,)) for k in keys] +
           [Other(r["diag"])])


@pytest.mark.parametrize("dt", DTYPES)
def test_loo_influence(dt):
    mat = np.zeros((7, 5), dtype=dt).T
    theta = np.zeros((3, 7)).T  # (n_draws, P) seen through .T
    center, scale = np.zeros(3), np.ones(3)
    idx = np.array([4, 0], dtype=np.int64)
    eng, lib = make(writes={"pla_loo_influence": {"n_replaced": 7}})
    r = eng.loo_influence(mat, theta, center, scale, 3, "sis")
    assert sorted(r) == ["diag", "ess_w", "kl", "m2", "n_replaced", "shift"] and type(r["n_replaced"]) is int and r["n_replaced"] == 7
    name, rec = last(lib)
    assert name == "pla_loo_influence"
    expect_fields(rec, dict(struct_size=C.sizeof(_capi.InfluenceArgs), engine=H, mat=mat, dtype=CODE[dt], kind=0, method=SIS, mem_space=HOST,
                            n_obs=5, n_draws=7, stride_obs=1, stride_draw=5, row_index=None, n_rows=5, tail_count=3, theta=theta, n_quant=3,
                            theta_stride_draw=1, theta_stride_quant=7, center=center, scale=scale, stream=None,
                            shift=out_f64(r["shift"], (5, 3)), m2=out_f64(r["m2"], (5, 3)), kl=out_f64(r["kl"], (5,)),
                            ess_w=out_f64(r["ess_w"], (5,)), diag=out_f64(r["diag"], (5,)), n_replaced=Other(r["diag"])))
    dense = np.zeros((7, 3))
    r = eng.loo_influence(mat, dense, center, scale, rows=idx)
    expect_fields(last(lib, 2)[1], dict(mat=Other(mat), stride_obs=7, stride_draw=1, row_index=idx, n_rows=2, theta=dense, theta_stride_draw=3,
                                        theta_stride_quant=1, shift=out_f64(r["shift"], (2, 3)), diag=out_f64(r["diag"], (2,)), kind=0, method=PSIS))
    r = eng.loo_influence(mat, np.zeros(7), [0.0], [1.0], kind="log_weights")  # log weights: draws-fastest only, no diag
    assert r["diag"] is None
    expect_fields(last(lib, 3)[1], dict(mat=Other(mat), stride_obs=7, stride_draw=1, kind=1, n_quant=1, theta_stride_draw=1, theta_stride_quant=1,
                                        diag=None, shift=out_f64(r["shift"], (5, 1)), row_index=None, n_rows=5))
    strided = np.zeros((7, 6))[:, ::2]  # neither dense nor the .T of a dense array: copied
    eng.loo_influence(mat, strided, center, scale)
    expect_fields(lib.calls[-1][1], dict(theta=Other(strided), theta_stride_draw=3, theta_stride_quant=1))
    with pytest.raises(ValueError, match=r"theta must be \(n_draws, P\) with n_draws = 7, got \(6, 3\)"):
        eng.loo_influence(mat, np.zeros((6, 3)), center, scale)
    with pytest.raises(ValueError, match="center and scale need 3 values"):
        eng.loo_influence(mat, theta, np.zeros(2), scale)
    with pytest.raises(ValueError, match="rows= needs kind='loglik'"):
        eng.loo_influence(mat, theta, center, scale, kind="log_weights", rows=idx)


# ---------------------------------------------------------------------------------------------------------- GLM
def test_glm_matrix_mode():
    X, beta = np.zeros((3, 5)).T, np.zeros((7, 3))
    y, off, dsc = np.zeros(5), np.zeros(5), np.ones(7)
    eng, lib = make()
    out = eng.glm(X, beta, "gaussian", y=y, offset=off, draw_scale=dsc)
    name, rec = last(lib)
    assert name == "pla_glm"
    expect_fields(rec, dict(struct_size=C.sizeof(_capi.GlmArgs), engine=H, family=1, mode=0, method=PSIS, mem_space=HOST, stream=None,
                            x=X, n_obs=5, n_pred=3, x_stride_obs=1, x_stride_pred=5, beta=beta, n_draws=7, beta_stride_draw=3,
                            beta_stride_pred=1, y=y, offset=off, trials=None, obs_const=None, draw_scale=dsc, draw_const=None,
                            row_index=None, n_rows=5, tail_count=0, scale_value=1.0, good_k=0.7, out=out_f64(out, (5, 7)), out_pitch=7,
                            diag=None, loo_i=None, lppd_i=None, agg=None, n_replaced=None))
    idx = np.array([4, 0], dtype=np.int64)
    out = eng.glm(np.zeros((5, 6))[:, ::2], beta.T.copy().T, "poisson", y=y, rows=idx)  # strided X is copied, beta is a .T view
    rec = last(lib, 2)[1]
    expect_fields(rec, dict(family=3, x_stride_obs=3, x_stride_pred=1, beta_stride_draw=1, beta_stride_pred=7, row_index=idx, n_rows=2,
                            out=out_f64(out, (2, 7)), out_pitch=7))
    for bad, text in ((dict(family="x"), "family must be one of"), (dict(family="poisson", mode="x"), "mode must be 'matrix' or 'loo', got 'x'")):
        with pytest.raises(ValueError, match=text):
            eng.glm(X, beta, **bad)
    with pytest.raises(ValueError, match=r"beta must be \(n_draws, P\) with P = 3, got \(7, 2\)"):
        eng.glm(X, np.zeros((7, 2)), "poisson")
    with pytest.raises(ValueError, match="y needs 5 values, got 4"):
        eng.glm(X, beta, "poisson", y=np.zeros(4))
    with pytest.raises(ValueError, match="draw_scale needs 7 values, got 5"):
        eng.glm(X, beta, "gaussian", y=y, draw_scale=np.zeros(5))


def test_glm_loo_mode_and_group_terms():
    X, beta, y, trials = np.zeros((5, 3)), np.zeros((7, 3)), np.zeros(5), np.ones(5)
    g1, u1, z1 = np.zeros(5, dtype=np.int32), np.zeros((4, 7)).T, np.ones(5)
    g2, u2 = np.zeros(5, dtype=np.int32), np.zeros((7, 2))
    eng, lib = make(writes={"pla_glm_grouped": {"n_replaced": 7}, "pla_glm": {"n_replaced": 7}})
    r = eng.glm(X, beta, "binomial", y=y, trials=trials, mode="loo", tail_count=3, method="tis", scale_value=2.0, good_k=0.5,
                groups=[(g1, u1, z1), (g2, u2)])
    assert sorted(r) == ["agg", "diag", "loo_i", "lppd_i", "n_replaced"] and type(r["n_replaced"]) is int and r["n_replaced"] == 7
    name, rec = last(lib)
    assert name == "pla_glm_grouped" and rec["struct_size"] == C.sizeof(_capi.GlmGroupedArgs) and rec["n_terms"] == 2
    expect_fields(rec["glm"], dict(struct_size=C.sizeof(_capi.GlmArgs), engine=H, family=2, mode=1, method=TIS, mem_space=HOST, stream=None,
                                   x=X, x_stride_obs=3, x_stride_pred=1, beta=beta, beta_stride_draw=3, beta_stride_pred=1, y=y, trials=trials,
                                   tail_count=3, scale_value=2.0, good_k=0.5, out=None, out_pitch=0, n_rows=5,
                                   diag=out_f64(r["diag"], (5,)), loo_i=out_f64(r["loo_i"], (5,)), lppd_i=out_f64(r["lppd_i"], (5,)),
                                   agg=out_f64(r["agg"], (8,)), n_replaced=Other(r["agg"])))
    expect_fields(rec["terms"][0], dict(group_index=g1, z=z1, u=u1, u_stride_draw=1, u_stride_group=7, n_groups=4))
    expect_fields(rec["terms"][1], dict(group_index=g2, z=None, u=u2, u_stride_draw=2, u_stride_group=1, n_groups=2))
    r = eng.glm(X, beta, "poisson", y=y, mode="loo", pointwise=False, groups=[])
    name, rec = last(lib, 2)
    assert name == "pla_glm_grouped" and rec["n_terms"] == 0 and r["n_replaced"] == 7
    expect_fields(rec["glm"], dict(diag=None, loo_i=None, lppd_i=None, agg=out_f64(r["agg"], (8,))))
    r = eng.glm(X, beta, "poisson", y=y, mode="loo", aggregate=False)
    name, rec = last(lib, 3)
    assert name == "pla_glm" and r["agg"] is None and type(r["n_replaced"]) is int and r["n_replaced"] == 7
    expect_fields(rec, dict(agg=None, diag=out_f64(r["diag"], (5,))))
    with pytest.raises(ValueError, match=r"draws of term 0 must be \(n_draws, G\) with n_draws = 7 and G >= 1, got \(6, 2\)"):
        eng.glm(X, beta, "poisson", y=y, groups=[(g1, np.zeros((6, 2)))])
    with pytest.raises(ValueError, match="index and z of term 1 need 5 values"):
        eng.glm(X, beta, "poisson", y=y, groups=[(g1, u1), (g2[:4], u2)])
    with pytest.raises(ValueError, match="at most 8 group-level terms are supported, got 9"):
        eng.glm(X, beta, "poisson", y=y, groups=[(g1, u1)] * 9)


# ---------------------------------------------------------------------------------------------------------- leave-future-out, ESS
@pytest.mark.parametrize("dt", DTYPES)
def test_lfo(dt):
    obs = np.zeros((7, 5), dtype=dt).T
    eng, lib = make(writes={"pla_lfo_ratios": {12: 7}, "pla_lfo": {17: 7, 18: 3}})
    r = eng.lfo_ratios(obs, 2, 3)
    assert sorted(r) == ["n_replaced", "ratios"] and type(r["n_replaced"]) is int and r["n_replaced"] == 7
    expect(last(lib), "pla_lfo_ratios", [H, obs, CODE[dt], 5, 7, 1, 5, 2, 3, HOST, None, out_f64(r["ratios"], (3, 7)), Other(r["ratios"])])
    r = eng.lfo(obs, 1, 3, 2, 4, 0.6, "sis")
    assert sorted(r) == ["diag", "elpd_i", "first_high", "n_replaced"]
    assert type(r["first_high"]) is int and r["first_high"] == 7 and type(r["n_replaced"]) is int and r["n_replaced"] == 3
    assert not r["diag"].any() and not r["elpd_i"].any()
    expect(last(lib, 2), "pla_lfo", [H, obs, CODE[dt], 5, 7, 1, 5, 1, 3, 2, SIS, 4, 0.6, HOST, None, out_f64(r["diag"], (3,)),
                                     out_f64(r["elpd_i"], (3,)), Other(r["diag"]), Other(r["diag"])])
    assert lib.calls[-1][1][17] != lib.calls[-1][1][18]
    one = np.zeros((1, 7), dtype=dt)
    eng.lfo(one, 1, 1, mode="backward")
    expect((lib.calls[-1][0], lib.calls[-1][1][:15]), "pla_lfo", [H, one, CODE[dt], 1, 7, 7, 1, 1, 1, 1, PSIS | 0x100, 0, 0.7, HOST, None])
    eng.lfo(one, 1, 1, method="tis", mode="backward")
    assert lib.calls[-1][1][10] == 0x102
    for call in (lambda: eng.lfo(obs, 1, 0), lambda: eng.lfo_ratios(obs, 1, 0)):
        with pytest.raises(ValueError, match="n_steps must be at least 1"):
            call()
    with pytest.raises(ValueError, match="mode must be 'forward' or 'backward', got 'x'"):
        eng.lfo(obs, 1, 1, mode="x")


@pytest.mark.parametrize("dt", DTYPES)
def test_relative_eff_flag_words(dt):
    a = np.zeros((5, 8), dtype=dt)
    eng, lib = make(writes={"pla_relative_eff": {12: 7}})
    for log, split, cap in itertools.product((False, True), repeat=3):
        r = eng.relative_eff(a, 4, log, split, cap)
        assert sorted(r) == ["n_invalid", "r_eff"] and type(r["n_invalid"]) is int and r["n_invalid"] == 7 and not r["r_eff"].any()
        expect(lib.calls[-1], "pla_relative_eff", [H, a, CODE[dt], 5, 8, 8, 1, 4, 1 * log + 2 * split + 4 * cap, HOST, None,
                                                   out_f64(r["r_eff"], (5,)), Other(r["r_eff"])])
    eng.relative_eff(a)
    assert lib.calls[-1][1][7:9] == [1, 5]  # one chain; log and cap


# ---------------------------------------------------------------------------------------------------------- model comparison
@pytest.mark.parametrize("dt", DTYPES)
def test_compare_passes(dt):
    wide = np.zeros((3, 9), dtype=dt)
    x = wide[:, :7]  # pitched rows keep their pitch
    eng, lib = make()
    out = eng.compare_moments(x, 2)
    expect(last(lib), "pla_compare_moments", [H, x, CODE[dt], 3, 7, 9, 2, HOST, None, out_f64(out, (10,))])
    cols = np.zeros((3, 14), dtype=dt)[:, ::2]  # strided columns are copied
    out = eng.compare_moments(cols, 0)
    expect(last(lib, 2), "pla_compare_moments", [H, Other(cols), CODE[dt], 3, 7, 7, 0, HOST, None, out_f64(out, (10,))])
    w = np.full(3, 1 / 3)
    f, g = eng.stacking_eval(x, w, 2.0)
    assert type(f) is float and g.shape == (3,)
    expect(last(lib, 3), "pla_stacking_eval", [H, x, CODE[dt], 3, 7, 9, 2.0, w, HOST, None, Other(w, g)])
    with pytest.raises(ValueError, match="expected 3 weights, got 2"):
        eng.stacking_eval(x, np.ones(2))
    z = eng.bb_bootstrap(x, 11, 0.5, -1, 2.0)
    expect(last(lib, 4), "pla_bb_bootstrap", [H, x, CODE[dt], 3, 7, 9, 2.0, 11, 0.5, 2**64 - 1, HOST, None, out_f64(z, (11, 3))])
    one = np.zeros((1, 7), dtype=dt)
    eng.compare_moments(one, 0)
    assert lib.calls[-1][1][3:6] == [1, 7, 7]
    eng.compare_moments(np.zeros((3, 7), dtype=np.int32), 0)
    assert lib.calls[-1][1][2] == F64
    with pytest.raises(ValueError, match=r"expected a 2-D \(n_models, n_obs\) array"):
        eng.compare_moments(np.zeros(7), 0)


# ---------------------------------------------------------------------------------------------------------- non-factorised
def test_nonfactor_log_lik():
    y, mu, mat, df = np.zeros(3), np.zeros((4, 3)), np.zeros((4, 3, 3)), np.ones(4)
    eng, lib = make()
    ll, flags = eng.nonfactor_log_lik(y, mu, mat)
    assert flags.dtype == np.int32 and flags.shape == (4,)
    expect(last(lib), "pla_nonfactor_loglik", [H, y, mu, mat, None, F64, 3, 4, 3, 9, 0, HOST, None, out_f64(ll, (3, 4)), 4, 1, flags])
    f = np.float32
    y32, mu32, mat32, df32 = y.astype(f), mu.astype(f), mat.astype(f), df.astype(f)
    ll, flags = eng.nonfactor_log_lik(y32, mu32, mat32, df32, "student_t")
    expect(last(lib, 2), "pla_nonfactor_loglik", [H, y32, mu32, mat32, df32, F32, 3, 4, 3, 9, 1, HOST, None, out_f64(ll, (3, 4)), 4, 1, flags])
    ll, flags = eng.nonfactor_log_lik(y32, mu, mat, df, "student_t")  # mixed: all f64
    expect(last(lib, 3), "pla_nonfactor_loglik", [H, Other(y32), mu, mat, df, F64, 3, 4, 3, 9, 1, HOST, None, out_f64(ll, (3, 4)), 4, 1, flags])


# ---------------------------------------------------------------------------------------------------------- errors
def test_index_errors():
    a = np.zeros((5, 7))
    eng, lib = make()
    for call in (lambda r: eng.psis_loo(a, rows=r), lambda r: eng.waic(a, rows=r), lambda r: eng.loo_diag(a, rows=r),
                 lambda r: eng.loo_influence(a, np.zeros(7), [0.0], [1.0], rows=r), lambda r: eng.glm(np.zeros((5, 2)), np.zeros((7, 2)), "linpred", rows=r)):
        with pytest.raises(IndexError, match=r"row indices must lie in \[0, 5\), got range \[0, 5\]"):
            call([0, 5])
        with pytest.raises(IndexError, match=r"row indices must lie in \[0, 5\), got range \[-1, 2\]"):
            call([2, -1])
    for call in (lambda d: eng.gather_draws(a, d), lambda d: eng.psis_loo_draws(a, d)):
        with pytest.raises(IndexError, match=r"draw indices must lie in \[0, 7\), got range \[-1, 3\]"):
            call([3, -1])
        with pytest.raises(IndexError, match=r"draw indices must lie in \[0, 7\), got range \[7, 7\]"):
            call([7])
        with pytest.raises(ValueError, match="draw_index is empty"):
            call([])
    assert lib.calls == []
    assert Engine._host_draws([3, 0, 3], 4).tolist() == [3, 0, 3]


def test_shape_errors():
    a, v = np.zeros((5, 7)), np.zeros(7)
    eng, lib = make()
    gi = _index()
    for call in (lambda: eng.psis_loo(v), lambda: eng.waic(v), lambda: eng.importance_weights(v), lambda: eng.group_sum(v, gi),
                 lambda: eng.psis_loo_groups(v, gi), lambda: eng.gather_draws(v, [0]), lambda: eng.psis_loo_draws(v, [0]),
                 lambda: eng.mixis_draw_lse(v), lambda: eng.mixis_loo(v), lambda: eng.loo_diag(np.zeros((5, 7, 2))),
                 lambda: eng.lfo_ratios(v, 1, 1), lambda: eng.lfo(v, 1, 1), lambda: eng.relative_eff(v),
                 lambda: eng.loo_influence(v, v, [0.0], [1.0])):
        with pytest.raises(ValueError, match=r"expected a 2-D \(n_obs, n_draws\) array"):
            call()
    b = np.zeros((5, 6))
    for call in (lambda: eng.e_loo(a, b), lambda: eng.e_loo(a, a, b), lambda: eng.e_loo(v, v)):
        with pytest.raises(ValueError, match="x, log_weights and log_ratios must be 2-D arrays of one shape"):
            call()
    for call in (lambda: eng.e_loo_quantiles(a, b, 0.5), lambda: eng.e_loo_quantiles(v, v, 0.5)):
        with pytest.raises(ValueError, match="x and log_weights must be 2-D arrays of one shape"):
            call()
    for call in (lambda: eng.loo_pit(a, b, np.zeros(5)), lambda: eng.loo_pit(v, v, np.zeros(5))):
        with pytest.raises(ValueError, match="mat and y_hat must be 2-D arrays of one shape"):
            call()
    for call in (lambda: eng.loo_diag_weights(a, b), lambda: eng.loo_diag_weights(v, v)):
        with pytest.raises(ValueError, match="lw and ll must be 2-D arrays of one shape"):
            call()
    with pytest.raises(ValueError, match=r"expected a 2-D \(n_obs, P\) array X"):
        eng.glm(v, a, "linpred")
    assert lib.calls == []


def test_kfold_rejects_mixed_dtypes_before_it_touches_a_device():
    pytest.importorskip("torch")
    eng, lib = make()
    with pytest.raises(TypeError, match=r"the full and the fold matrices must share one dtype, float64 or float32; got \['float32', 'float64'\]"):
        eng._kfold_plan(np.zeros((4, 3)), [np.zeros((2, 3), dtype=np.float32), np.zeros((2, 3))], np.array([1, 1, 2, 2]))
    with pytest.raises(ValueError, match=r"expected 2-D \(n_obs, n_draws\) matrices"):
        eng._kfold_plan(np.zeros(4), [np.zeros((2, 3))], np.array([1, 1, 2, 2]))
    assert lib.calls == []
