"""``e_loo`` / ``e_loo_quantiles`` on every kernel route (``-m gpu``).

``pla_k_eloo.hip`` picks one of four arrangements of the kernels in ``pla_eloo.h`` per call; ``Engine.last_kernels()`` names
the one that ran, and every case here asserts it:

    e_loo_wave_kernel<T, own> + e_loo_rows_kernel<T, 256, list>    contiguous draws, 16-byte aligned x / lw / lr,
                                                                   stride_obs % vec == 0, S % vec == 0, 64 vec <= S <= 2^20
    e_loo_rows_kernel<T, 256>                                      anything else
    e_loo_quantile_wave_kernel<T> + e_loo_quantile_kernel<T, 512>  the same conditions and S <= 4096
    e_loo_quantile_kernel<T, 512>                                  anything else

(vec = 2 for f64, 4 for f32.)  Every result is held against the float64 oracle (``oracle/psis_oracle.py``) on the f64 data
(f32 input: its exact f64 upcast).  The weighted mean is held to a bound scaled to the problem, not to its
own size, so that rows whose mean is near 0 are checked too: |got - ref| <= C_MEAN * sum(w |x|), ref = math.fsum(w x) with
the weights normalised in f64.  NaN / inf patterns must match exactly; the k values agree to 1e-14 (they take a handful of
closed-form values: the reference's degenerate GPD fit).  ``PLA_FORCE_PATH=1`` forces the general kernels: the second,
independent implementation that the fast routes are compared with row for row.  Every call of the layout, grid-stride and
edge-row cases runs twice and must give the same bits."""

import math

import numpy as np
import pytest

from oracle import psis_oracle as orc

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
VEC = {F64: 2, F32: 4}
KEYS = ("mean", "var", "k_mean", "k_var", "k_none")
PROBS = np.array([0.05, 0.25, 0.5, 0.9, 0.975])
# |mean - fsum(w x)| / sum(w |x|): both e_loo kernels accumulate in f64 (worst measured on an MI355X over this file: 1.6e-15)
C_MEAN = 1e-12
Q_RTOL, Q_ATOL = 1e-9, 1e-12


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


# ---- routes -----------------------------------------------------------------------------------------------------------------
def tname(dt):
    return "double" if dt == F64 else "float"


def eloo_wave_ok(S, dt):
    v = VEC[dt]
    return S % v == 0 and 64 * v <= S <= 1 << 20


def quant_wave_ok(S, dt):
    return eloo_wave_ok(S, dt) and S <= 4096


def eloo_route(dt, wave, own=True):
    t = tname(dt)
    if wave:
        return (f"e_loo_wave_kernel<{t}, {'own ratios' if own else 'ratios = log-weights'}> + "
                f"e_loo_rows_kernel<{t}, 256, list> (declined rows)")
    return f"e_loo_rows_kernel<{t}, 256> (one workgroup per observation)"


def quant_route(dt, wave):
    t = tname(dt)
    if wave:
        return f"e_loo_quantile_wave_kernel<{t}> + e_loo_quantile_kernel<{t}, 512> (declined rows)"
    return f"e_loo_quantile_kernel<{t}, 512> (one workgroup per observation)"


def run_e_loo(eng, route, *args, **kw):
    res = eng.e_loo(*args, **kw)
    assert eng.last_kernels() == route
    return {k: np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v, dtype=np.float64) for k, v in res.items()}


def run_quant(eng, route, x, lw, probs):
    q = eng.e_loo_quantiles(x, lw, probs)
    assert eng.last_kernels() == route
    return np.asarray(q.cpu().numpy() if hasattr(q, "cpu") else q, dtype=np.float64)


def forced(monkeypatch, fn):
    """``fn()`` with the general kernels only."""
    with monkeypatch.context() as m:
        m.setenv("PLA_FORCE_PATH", "1")
        return fn()


# ---- bitwise comparison, twice-run ------------------------------------------------------------------------------------------
# Run-to-run spread of the quantiles of e_loo_quantile_kernel<T, 512> (the general quantile kernel, and the declined rows of the
# wave route).  That kernel is NOT bitwise reproducible: it builds its per-row histograms of weights with floating-point LDS
# atomics from eight waves (cum2k in the kernel, hist in mass_select, pla_eloo.h) and collects the members of the crossing bin
# into a list in atomic order, so the order of the additions -- and with it the last bits of the weight below the crossing --
# changes from run to run; the interpolation (e_loo.py:554) divides by the weight of one draw and magnifies that.  Measured on
# an MI355X between runs over 512 rows x 33 levels: up to 1990 ulp at S = 2000 f64, 630 at 4000 f32, 35 318 at 8192 f64 (the
# rows too long to keep in registers, which settle the crossing by the radix descent alone).  Every other output is bitwise reproducible: the wave kernels own a row per wave (their LDS atomics come from one wave,
# in program order), and the e_loo kernels reduce in a fixed order.
QUANT_ULPS = 1 << 16


def ulps(a, b):
    """Distance in units in the last place of two f64 arrays (NaN against NaN: 0; opposite signs: the sum of both distances
    from 0, capped at 2^62)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ia, ib = (np.where(v.view(np.int64) < 0, -(v.view(np.int64) & 0x7FFFFFFFFFFFFFFF), v.view(np.int64)) for v in (a, b))
    ia, ib = (np.clip(v, -(1 << 62), 1 << 62) for v in (ia, ib))
    return np.where(np.isnan(a) & np.isnan(b), 0, np.abs(ia - ib))


def bitwise(got, want, what, max_ulps=0):
    """The same bits (``max_ulps``: at most that many units in the last place apart), NaN where NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern"
    d = ulps(got, want)
    bad = d > max_ulps
    if bad.any():
        i = np.flatnonzero(bad)[0]
        raise AssertionError(f"{what}: {bad.sum()} entries differ, e.g. flat index {i}: {got.ravel()[i]!r} vs {want.ravel()[i]!r} "
                             f"({d.max()} ulp at most, {max_ulps} allowed)")


def twice(fn, what, max_ulps=0):
    """``fn()`` run twice: both runs must give the same bits (all five e_loo outputs / the quantiles: ``max_ulps``)."""
    a, b = fn(), fn()
    if isinstance(a, dict):
        for k in a:
            bitwise(b[k], a[k], f"{what}: second run, {k}")
    else:
        bitwise(b, a, f"{what}: second run", max_ulps)
    return a


# ---- oracle -----------------------------------------------------------------------------------------------------------------
def f64(a):
    return np.asarray(a, dtype=np.float64)


def weights(lw_row):
    with np.errstate(all="ignore"):
        return np.exp(lw_row - orc.lse(lw_row))


def oracle_rows(x, lw, lr, rows, tail_len=20):
    """e_loo's five outputs for the listed rows, plus sum(w |x|) (the scale of the mean's bound)."""
    out = {k: np.empty(len(rows)) for k in KEYS + ("scale",)}
    for j, i in enumerate(rows):
        xi, lwi = f64(x[i]), f64(lw[i])
        lri = lwi if lr is None else f64(lr[i])
        w = weights(lwi)
        with np.errstate(all="ignore"):
            wx = w * xi
            if np.isfinite(wx).all():
                out["mean"][j], out["scale"][j] = math.fsum(wx), math.fsum(np.abs(wx))
            else:  # (the pattern: NaN / +-inf as numpy's sum gives it, e_loo.py:430-437)
                out["mean"][j], out["scale"][j] = wx.sum(), np.nan
            out["var"][j] = orc.weighted_variance_row(xi, w)
            out["k_mean"][j] = orc.k_hat_row(xi, lri, tail_len)
            out["k_var"][j] = orc.k_hat_row(xi**2, lri, tail_len)
            out["k_none"][j] = orc.k_hat_row(None, lri, tail_len)
    return out


def same(got, want, rtol, what, atol=1e-12):
    got, want = f64(got), f64(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern {got} vs {want}"
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), f"{what}: inf pattern"
    ok = np.isfinite(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rtol, atol=atol, err_msg=what)


def mean_error(got, ref):
    """|got - ref| / sum(w |x|) of the rows with a finite reference (0 where they are equal)."""
    ok = np.isfinite(ref["mean"])
    err, scale = np.abs(got[ok] - ref["mean"][ok]), ref["scale"][ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, np.where(scale > 0, err / scale, np.inf))


MEAN_ERRS = []  # worst |mean - ref| / sum(w |x|) of every check (read by whoever wants the figure)


def check_e_loo(got, ref, what, var_rtol=1e-8):
    """``got``: the five outputs of the rows the oracle ``ref`` was computed for."""
    same(got["mean"], ref["mean"], 0.0, f"{what}: mean pattern", atol=np.inf)
    rel = mean_error(got["mean"], ref)
    MEAN_ERRS.append((what, float(rel.max(initial=0.0))))
    assert np.all(rel <= C_MEAN), f"{what}: mean off by {rel.max():.3g} sum(w|x|) (row {np.argmax(rel)})"
    same(got["var"], ref["var"], var_rtol, f"{what}: variance")
    for k in ("k_mean", "k_var", "k_none"):
        same(got[k], ref[k], 1e-14, f"{what}: {k}")


def pick(res, rows):
    return {k: v[rows] for k, v in res.items()}


def interp_at(xs, ww, p, k):
    """The reference's answer (e_loo.py:548-554) had the crossing been found at sorted position k."""
    if k >= len(xs):
        return xs[-1]
    if k == 0:
        return xs[0]
    return xs[k - 1] + (xs[k] - xs[k - 1]) * (p - ww[k - 1]) / (ww[k] - ww[k - 1])


LEVEL_TOL = 1e-12  # (a cumulative sum of at most 8192 weights that add up to 1 is good to ~S eps = 1e-12)


def level_of(got, xi, w, p):
    """Whether ``got`` is the reference's interpolation (e_loo.py:552-554) at a level within LEVEL_TOL of ``p``.  Where the draw
    that crosses the level holds a tiny part of the mass, the answer moves by (its gap to the draw below) / (its weight) per unit
    of level, and the rounding of the cumulative weights -- the oracle's cumsum and the kernels' sums alike -- is all that
    decides it: e.g. one weight of 99.9 % and the level 1 - 1e-12, whose answer lies between the two largest draws of weight
    5e-7 each (measured: 1.1e-7 apart from the oracle in x, 5e-14 in level)."""
    order = np.argsort(xi, kind="stable")
    xs, ws = xi[order], w[order]
    ww = np.cumsum(ws) / np.sum(ws)
    k = int(np.searchsorted(xs, got, side="left"))
    if not (0 < k < len(xs)) or not (xs[k - 1] <= got <= xs[k]) or xs[k] == xs[k - 1]:
        return False
    implied = ww[k - 1] + (got - xs[k - 1]) / (xs[k] - xs[k - 1]) * (ww[k] - ww[k - 1])
    return abs(implied - p) <= LEVEL_TOL


def check_quant(q, x, lw, probs, rows, what, exact=False):
    """Weighted quantiles of the listed rows (``q``: one line per row) against the oracle.  Rows with equal draws follow the
    stable-argsort rule of test_gpu_e_loo.test_golden_rows.  ``exact``: the levels sit exactly on a cumulative weight, where the
    oracle's cumsum decides the crossing by rounding -- either bracketing answer is accepted."""
    probs = np.atleast_1d(probs)
    for j, i in enumerate(rows):
        xi, w = f64(x[i]), weights(f64(lw[i]))
        for jp, p in enumerate(probs):
            got = q[j, jp]
            cands = [orc.weighted_quantile_row(xi, w, p)]
            if exact or np.unique(xi).size < xi.size:
                cands.append(orc.weighted_quantile_row(xi, w, p, stable=True))
            if exact:
                order = np.argsort(xi, kind="stable")
                xs, ww = xi[order], np.cumsum(w[order]) / np.sum(w[order])
                k = int(np.searchsorted(ww, p, side="left"))
                cands += [interp_at(xs, ww, p, k), interp_at(xs, ww, p, k + 1)]
            ok = any(np.isclose(got, c, rtol=Q_RTOL, atol=Q_ATOL) or (np.isnan(got) and np.isnan(c)) for c in cands)
            assert ok or level_of(got, xi, w, p), f"{what}: row {i} level {p!r}: {got!r}, oracle {cands}"


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def make_inputs(rng, N, S, dt):
    lr = rng.uniform(0.1, 0.9, size=(N, 1)) * rng.exponential(size=(N, S))
    x = rng.normal(size=(N, S)) * 2.0 + 0.3
    lw = lr + 0.2 * rng.normal(size=(N, S))
    return x.astype(dt), lw.astype(dt), lr.astype(dt)


def spoil(x, lw, rows, S):
    """Rows the fast kernels decline: NaN / inf among the draws or the log-weights, in turns."""
    for n, i in enumerate(rows):
        s = (7 * i + 3) % S
        if n % 3 == 0:
            x[i, s] = np.nan
        elif n % 3 == 1:
            x[i, s] = -np.inf if n % 2 else np.inf
        else:
            lw[i, s] = np.nan


# ---- (a) route boundaries on S ----------------------------------------------------------------------------------------------
BOUNDARY = ([(F64, S) for S in (126, 127, 128, 130, 4092, 4096, 4097, 4100)]
            + [(F32, S) for S in (252, 255, 256, 260, 4092, 4096, 4097, 4100)])


@pytest.mark.parametrize("dt,S", BOUNDARY, ids=lambda v: getattr(v, "__name__", str(v)))
def test_route_boundaries(eng, dt, S):
    rng = np.random.default_rng(S * 3 + VEC[dt])
    N = 6
    x, lw, lr = make_inputs(rng, N, S, dt)
    x[N - 1, S // 2] = np.nan  # (one row for the declined-rows kernel behind the wave kernel)
    wave = eloo_wave_ok(S, dt)
    rows = list(range(N))
    res = run_e_loo(eng, eloo_route(dt, wave, own=True), x, lw, lr)
    check_e_loo(res, oracle_rows(x, lw, lr, rows), f"S={S} own ratios")
    res = run_e_loo(eng, eloo_route(dt, wave, own=False), x, lw)
    check_e_loo(res, oracle_rows(x, lw, None, rows), f"S={S} ratios = log-weights")
    q = run_quant(eng, quant_route(dt, quant_wave_ok(S, dt)), x, lw, PROBS)
    check_quant(q[: N - 1], x, lw, PROBS, rows[: N - 1], f"S={S} quantiles")


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("extra", [0, 1], ids=["2^20", "2^20+vec"])
def test_route_longest_rows(eng, torch, dt, extra):
    S = (1 << 20) + extra * VEC[dt]
    rng = np.random.default_rng(20 + extra)
    x, lw, lr = make_inputs(rng, 1, S, dt)  # (one row: the oracle sorts a million draws six times per call)
    t = [torch.from_numpy(a).cuda() for a in (x, lw, lr)]
    res = run_e_loo(eng, eloo_route(dt, extra == 0, own=True), *t)
    check_e_loo(res, oracle_rows(x, lw, lr, [0]), f"S={S}")
    res = run_e_loo(eng, eloo_route(dt, extra == 0, own=False), t[0], t[1])
    check_e_loo(res, oracle_rows(x, lw, None, [0]), f"S={S} ratios = log-weights")


# ---- (b) device layouts -----------------------------------------------------------------------------------------------------
def layouts(torch, a, S):
    """name -> (device view of the host matrix a, True when the fast routes may take it)."""
    n = a.shape[0]
    out = {"contiguous": (torch.from_numpy(a).cuda(), True)}
    big = torch.zeros((n, S + 4), dtype=torch.from_numpy(a).dtype, device="cuda")
    big[:, 1 : S + 1] = torch.from_numpy(a).cuda()
    out["misaligned"] = (big[:, 1 : S + 1], False)                  # data pointer one element past a 16-byte boundary
    pitch = torch.zeros((n, S + 1), dtype=big.dtype, device="cuda")
    pitch[:, :S] = torch.from_numpy(a).cuda()
    out["pitch S+1"] = (pitch[:, :S], False)                        # stride_obs % vec != 0
    out["obs fastest"] = (torch.from_numpy(a).cuda().t().contiguous().t(), False)
    return out


@pytest.mark.parametrize("dt,S", [(F64, 1000), (F32, 2000)], ids=["f64", "f32"])
def test_device_layouts(eng, torch, monkeypatch, dt, S):
    rng = np.random.default_rng(S)
    N = 80
    x, lw, lr = make_inputs(rng, N, S, dt)
    spoil(x, lw, range(3, N, 11), S)
    x[5] = 1.5                                                      # constant draws
    lw[6] = 0.0                                                     # constant weights (np.quantile's branch)
    host = run_e_loo(eng, eloo_route(dt, True), x, lw, lr)
    host_q = run_quant(eng, quant_route(dt, True), x, lw, PROBS)
    gen = forced(monkeypatch, lambda: run_e_loo(eng, eloo_route(dt, False), x, lw, lr))
    gen_q = forced(monkeypatch, lambda: run_quant(eng, quant_route(dt, False), x, lw, PROBS))
    rows = list(range(N))
    ref = oracle_rows(x, lw, lr, rows)
    check_e_loo(host, ref, "host")
    check_e_loo(gen, ref, "host, general kernel")
    fin = [i for i in rows if np.isfinite(x[i]).all() and np.isfinite(lw[i]).all()]
    check_quant(host_q[fin], x, lw, PROBS, fin, "host quantiles")
    check_quant(gen_q[fin], x, lw, PROBS, fin, "host quantiles, general kernel")
    lx, lwl, lrl = layouts(torch, x, S), layouts(torch, lw, S), layouts(torch, lr, S)
    for name in lx:
        tx, fast = lx[name]
        tw, tr = lwl[name][0], lrl[name][0]
        res = twice(lambda: run_e_loo(eng, eloo_route(dt, fast), tx, tw, tr), name)
        q = twice(lambda: run_quant(eng, quant_route(dt, fast), tx, tw, PROBS), name + " quantiles", QUANT_ULPS)
        # the same kernel reads the same numbers in the same order: the same bits as the host call of that route
        for k in KEYS:
            bitwise(res[k], (host if fast else gen)[k], f"{name}: {k}")
        bitwise(q, host_q if fast else gen_q, f"{name}: quantiles", QUANT_ULPS)
    # mixed dtypes: x f32 with f64 weights and ratios is computed in f64 (the upcast), on the fast route
    x32, lw64, lr64 = x.astype(F32), f64(lw), f64(lr)
    tx, tw, tr = (torch.from_numpy(a).cuda() for a in (x32, lw64, lr64))
    res = twice(lambda: run_e_loo(eng, eloo_route(F64, True), tx, tw, tr), "mixed")
    q = twice(lambda: run_quant(eng, quant_route(F64, True), tx, tw, PROBS), "mixed quantiles", QUANT_ULPS)
    want = run_e_loo(eng, eloo_route(F64, True), f64(x32), lw64, lr64)
    for k in KEYS:
        bitwise(res[k], want[k], f"mixed: {k}")
    bitwise(q, run_quant(eng, quant_route(F64, True), f64(x32), lw64, PROBS), "mixed: quantiles", QUANT_ULPS)


# ---- (c) grid-stride loops --------------------------------------------------------------------------------------------------
def weights_all(lw):
    with np.errstate(all="ignore"):
        w = np.exp(lw - lw.max(axis=1, keepdims=True))
        return w / w.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("dt,S,N", [(F64, 128, 40_000), (F32, 256, 70_000)], ids=["f64", "f32"])
def test_grid_stride(eng, torch, monkeypatch, dt, S, N):
    """More rows than the wave grids (8192 x 4 and 4096 x 4 waves), the general grid (16 384 workgroups) and the declined-rows
    grids (2048 workgroups) hold: every grid-stride loop runs more than once."""
    rng = np.random.default_rng(N)
    x, lw, lr = make_inputs(rng, N, S, dt)
    spoil(x, lw, range(5, N, 13), S)                                # > 2048 declined rows all over the matrix
    flat = np.arange(3, N, 17)
    lwq = lw.copy()
    lwq[flat] = 0.0                                                 # constant weights: declined by the quantile wave kernel
    t = [torch.from_numpy(a).cuda() for a in (x, lw, lr, lwq)]
    res = twice(lambda: run_e_loo(eng, eloo_route(dt, True), t[0], t[1], t[2]), "e_loo")
    q = twice(lambda: run_quant(eng, quant_route(dt, True), t[0], t[3], PROBS), "quantiles", QUANT_ULPS)
    gen = forced(monkeypatch, lambda: run_e_loo(eng, eloo_route(dt, False), t[0], t[1], t[2]))
    gen_q = forced(monkeypatch, lambda: run_quant(eng, quant_route(dt, False), t[0], t[3], PROBS))
    # every row against the general kernels
    xd = f64(x)
    scale = (weights_all(f64(lw)) * np.abs(xd)).sum(axis=1)
    same(res["mean"], gen["mean"], 0.0, "mean pattern", atol=np.inf)
    ok = np.isfinite(gen["mean"])
    gap = np.abs(res["mean"][ok] - gen["mean"][ok])
    assert np.all(gap <= 2 * C_MEAN * scale[ok]), f"mean: wave vs general {np.max(gap / scale[ok]):.3g} sum(w|x|)"
    same(res["var"], gen["var"], 1e-8, "variance: wave vs general")
    for k in ("k_mean", "k_var", "k_none"):
        same(res[k], gen[k], 1e-14, f"{k}: wave vs general")
    same(q, gen_q, Q_RTOL, "quantiles: wave vs general", atol=Q_ATOL)
    # a seeded sample and the rows around the grid sizes against the oracle
    rows = set(rng.choice(N, 24, replace=False).tolist()) | set(range(5, 60, 13)) | set(flat[:3].tolist())
    rows |= {r + d for r in (2048, 16384, 32768, 65536) for d in (-1, 0, 1) if r + d < N}
    rows = sorted(rows)
    check_e_loo(pick(res, rows), oracle_rows(x, lw, lr, rows), "sample")
    fin = [i for i in rows if np.isfinite(x[i]).all() and np.isfinite(lwq[i]).all()]
    check_quant(q[fin], x, lwq, PROBS, fin, "sample quantiles")


# ---- (d) host staging blocks ------------------------------------------------------------------------------------------------
def test_host_staging_blocks(eng, torch):
    """A host call is staged in blocks of 2^29 bytes of rows (pla_capi_loo.hip): at S = 8192 f64 that is 8192 rows a block, and
    8192 + 64 rows span two."""
    S, per = 8192, (1 << 29) // (8 * 8192)
    N = per + 64
    rng = np.random.default_rng(8192)
    x = rng.random((N, S)) * 4.0 - 1.0
    lw = rng.random((N, S)) * -3.0
    lr = rng.random((N, S)) * 2.0
    res = run_e_loo(eng, eloo_route(F64, True), x, lw, lr)
    q = run_quant(eng, quant_route(F64, False), x, lw, PROBS)
    lo, hi = per - 4, per + 4                                       # both sides of the block boundary
    t = [torch.from_numpy(np.ascontiguousarray(a[lo:hi])).cuda() for a in (x, lw, lr)]
    dev = run_e_loo(eng, eloo_route(F64, True), *t)
    dev_q = run_quant(eng, quant_route(F64, False), t[0], t[1], PROBS)
    for k in KEYS:
        bitwise(res[k][lo:hi], dev[k], f"rows {lo}..{hi - 1}: {k}")
    bitwise(q[lo:hi], dev_q, f"rows {lo}..{hi - 1}: quantiles", QUANT_ULPS)
    rows = sorted(set(rng.choice(N, 8, replace=False).tolist()) | {0, per - 1, per, N - 1})
    check_e_loo(pick(res, rows), oracle_rows(x, lw, lr, rows), "staged")
    check_quant(q[rows], x, lw, PROBS, rows, "staged quantiles")


# ---- (e) tail_len -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_tail_len(eng, monkeypatch, dt):
    import pyloo_amd as pl

    S, N = 256, 8
    rng = np.random.default_rng(77)
    x, lw, lr = make_inputs(rng, N, S, dt)
    lr[1, :30] = lr[1].max()                                        # 30 equal ratios at the top: allclose up to tail_len 30
    x[2] = np.round(x[2])                                           # few distinct values
    x[3, :40] = x[3].max()                                          # 40 equal largest draws
    lr[4] = 0.5                                                     # constant ratios
    x[5, 9] = np.nan
    x[6, :S // 2], x[6, S // 2:] = 2.0, -1.0                        # two values
    lr[7, S // 3] = lr[7].max() + 40.0                              # one ratio dominates
    rows = list(range(N))
    for tl in (5, 6, 19, 21, 64, 65, S - 1, S, S + 10):
        ref = oracle_rows(x, lw, lr, rows, tail_len=tl)
        for general in (False, True):
            fn = lambda: run_e_loo(eng, eloo_route(dt, not general), x, lw, lr, tail_len=tl)  # noqa: B023
            res = forced(monkeypatch, fn) if general else fn()
            for k in ("k_mean", "k_var", "k_none"):
                same(res[k], ref[k], 1e-14, f"tail_len={tl} {'general' if general else 'wave'}: {k}")
        # the fronts: ratios as weights, k of h = x and of the ratios alone
        ref2 = oracle_rows(x, lr, None, rows, tail_len=tl)
        same(np.asarray(pl.compute_pareto_k(x, lr, tail_len=tl)), ref2["k_mean"], 1e-14, f"compute_pareto_k tail_len={tl}")
        assert eng.last_kernels() == eloo_route(dt, True, own=False)
        for i in (0, 1, 6):
            same([pl.k_hat(x[i], lr[i], tail_len=tl)], [ref2["k_mean"][i]], 1e-14, f"k_hat row {i}, tail_len={tl}")
            same([pl.k_hat(None, lr[i], tail_len=tl)], [ref2["k_none"][i]], 1e-14, f"k_hat(None) row {i}, tail_len={tl}")


# ---- (f) quantile edge rows on the wave route -------------------------------------------------------------------------------
def allclose_gap(S, f):
    """d such that one weight of 1 + d among S - 1 weights of 1 sits f times np.allclose's tolerance away from w[0]
    (normalised: d / (S + d) = f (atol + rtol / (S + d)))."""
    return f * (1e-8 * S + 1e-5) / (1.0 - f * 1e-8)


def edge_rows(rng, S, dt):
    N = 18
    x = rng.normal(size=(N, S)) * 2.0 + 0.3
    lw = 0.5 * rng.exponential(size=(N, S))
    x[0, S // 3] = 1e12                                             # one far draw: the other draws share a bin or two
    x[1] = rng.normal(size=S) * (1e300 if dt == F64 else 1e37)     # range beyond what the bins are built for (f32: its widest)
    x[2, rng.choice(S, 100, replace=False)] = np.median(x[2])       # > 64 equal draws at the median
    x[3] = np.sort(x[3])
    x[4] = -np.sort(-x[4])
    x[5] = -0.75                                                    # constant draws
    x[6] = np.where(rng.random(S) < 0.3, 1.0, 4.0)                  # two values
    lw[7] = 0.0
    lw[7, 17] = np.log(999.0 * (S - 1))                             # one weight holds 99.9 % of the mass
    lw[8, rng.choice(S, S // 2, replace=False)] = -np.inf           # zero weights on half the row
    for i, f in ((9, 0.5), (10, 2.0)):                              # both sides of np.allclose(w, w[0]) (e_loo.py:536)
        lw[i] = 0.0
        lw[i, S // 2] = np.log1p(allclose_gap(S, f))
    x[11, 123] = np.nan
    lw[12, 45] = np.nan
    x[13] = np.round(x[13], 1)                                      # many ties
    lw[14] = np.log(rng.integers(1, 4, size=S))                     # small integer weights
    lw[15, :S // 2] -= 40.0                                         # half the row with negligible weight
    x[16] = np.abs(x[16]) * 1e-9                                    # tiny positive draws
    x, lw = x.astype(dt), lw.astype(dt)
    w9, w10 = weights(f64(lw[9])), weights(f64(lw[10]))
    assert np.allclose(w9, w9[0]) and not np.allclose(w10, w10[0])  # (the construction sits where it should)
    return x, lw


LEVELS = {
    "ends": np.array([1e-12, 1.0 - 1e-12]),
    "duplicated, unsorted": np.array([0.9, 0.5, 0.5, 0.1, 0.25, 0.999]),
    "scalar": 0.5,
    "257 levels": np.random.default_rng(257).permutation(np.linspace(0.002, 0.998, 257)),
}


@pytest.mark.parametrize("dt,S", [(F64, 2000), (F32, 4000)], ids=["f64", "f32"])
def test_quantile_edge_rows(eng, torch, monkeypatch, dt, S):
    rng = np.random.default_rng(S + 1)
    x, lw = edge_rows(rng, S, dt)
    N = x.shape[0]
    rows = list(range(N))
    tx, tw = torch.from_numpy(x).cuda(), torch.from_numpy(lw).cuda()
    # the draws' own e_loo, too: all five outputs (ratios = log-weights)
    res = twice(lambda: run_e_loo(eng, eloo_route(dt, True, own=False), tx, tw), "edge rows e_loo")
    check_e_loo(res, oracle_rows(x, lw, None, rows), "edge rows")
    fin = [i for i in rows if np.isfinite(x[i]).all()]              # (NaN among the draws: outside what is compared)
    for name, probs in LEVELS.items():
        q = twice(lambda: run_quant(eng, quant_route(dt, True), tx, tw, probs), name, QUANT_ULPS)  # noqa: B023
        assert q.shape == (N, np.atleast_1d(probs).size)
        gen = forced(monkeypatch, lambda: run_quant(eng, quant_route(dt, False), tx, tw, probs))  # noqa: B023
        check_quant(q[fin], x, lw, probs, fin, f"{name}, wave route")
        check_quant(gen[fin], x, lw, probs, fin, f"{name}, general kernel")
        bitwise(q[11], gen[11], f"{name}: NaN draws (declined: the general kernel's answer)", QUANT_ULPS)
    # levels exactly on a row's cumulative weight (integer weights, distinct draws): either bracketing answer
    for i in (3, 14):
        xi, w = f64(x[i]), weights(f64(lw[i]))
        order = np.argsort(xi, kind="stable")
        ww = np.cumsum(w[order]) / np.sum(w[order])
        probs = ww[[0, 10, S // 3, S // 2, S - 20]]
        one = (torch.from_numpy(x[i : i + 1].copy()).cuda(), torch.from_numpy(lw[i : i + 1].copy()).cuda())
        q = twice(lambda: run_quant(eng, quant_route(dt, True), one[0], one[1], probs), f"row {i}, exact levels", QUANT_ULPS)  # noqa: B023
        check_quant(q, x, lw, probs, [i], f"row {i}, exact levels", exact=True)
