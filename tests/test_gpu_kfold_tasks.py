"""The ragged log-mean-exp of k-fold (csrc/pla_kfold.h) where one wave, lane or workgroup takes several tasks; run with ``-m gpu``.

The three kernels walk one task list by grid stride and the launcher (csrc/pla_k_kfold.hip) caps their grids: 16 384 waves on the
wave route, 8192 x 256 lanes on the lane route, 8192 workgroups on the block route (``GRID_WAVES``, ``GRID_LANES``,
``GRID_BLOCKS`` below -- the task counts of this file follow from them).  Past those counts a wave streams its next task's row
into the registers of the row it is summing, a lane carries its source cursor into a second sweep and a workgroup starts over on
another source.  ``pla_kfold_lme`` is called directly on hand-built task lists: a few distinct rows per source, tens of
thousands of tasks cycling over them, every task compared with tests/kfold_ref.py at the project's log-mean-exp tolerances
(rtol 1e-10 / atol 1e-12, NaN in the same places: tests/test_gpu_kfold.py) and, bit for bit, with every other task that names
the same row and with a call short enough that nothing chains ("the same row gives the same bits wherever it lies").

Every source is a view inside a NaN-filled allocation with guard rows on both sides and ``out`` has sentinel bands on both
sides: a row the kernel failed to clamp reads NaN the test owns, a store it failed to drop lands in a band the test looks at.
"""

import ctypes as C
import functools
import re

import numpy as np
import pytest

from kfold_ref import lme_ref
from test_gpu_kfold import check_agg, padded

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
GRID_WAVES = 16384       # kfold_wave_kernel: 2048 * 8 waves at the most
GRID_LANES = 8192 * 256  # kfold_lane_kernel: 8192 workgroups of 256 lanes, a task per lane
GRID_BLOCKS = 8192       # kfold_block_kernel: a task per workgroup
RTOL, ATOL = 1e-10, 1e-12
SENTINEL = -123456.789
BAND = 64  # sentinel slots on either side of ``out``
KERNEL = {"wave": "kfold_wave_kernel", "lane": "kfold_lane_kernel", "block": "kfold_block_kernel"}


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


def vec(dtype):
    return 16 // np.dtype(dtype).itemsize


# ---------------------------------------------------------------------------------------------------------------- inputs
def shifted_rows(rng, s, dtype):
    """Eight rows of ``s`` draws on which a wrong or stale maximum shows: near 0, about -2000, about +900, a span of 850 nats,
    one dominant draw, and the maximum at the last draw, at draw 0 and at the end of the last whole 16-byte vector."""
    a = rng.normal(-2.0, 1.5, size=(8, s))
    a[1] -= 2000.0
    a[2] += 900.0
    a[3] = rng.permutation(np.linspace(-800.0, 50.0, s))
    a[4] = rng.normal(-30.0, 1.0, size=s)
    a[4, rng.integers(s)] = 40.0
    a[5] -= 2000.0
    a[5, -1] = -1990.0
    a[6] -= 2000.0
    a[6, 0] = -1985.0
    a[7] += 900.0
    a[7, max(s // vec(dtype) * vec(dtype) - 1, 0)] = 915.0
    return a.astype(dtype)


def nonfinite_positions(s, dtype):
    """draw 0, the last draw of the last whole vector, the s % VEC draws behind it, draws 63 VEC and 64 VEC (lane 63 -> lane 0)"""
    v = vec(dtype)
    whole = s // v * v
    return sorted({0, max(whole - 1, 0), *range(whole, s), *(p for p in (63 * v, 64 * v) if p < s)})


def nonfinite_rows(rng, s, dtype):
    """Two clean rows (about -2000 and +900); a NaN, a +inf, a -inf at each of :func:`nonfinite_positions` of a row about
    -2000; all NaN; all -inf; NaN beside a +inf; NaN among draws below -1e10."""
    rows = [rng.normal(-2000.0, 1.5, size=s), rng.normal(900.0, 1.5, size=s)]
    for p in nonfinite_positions(s, dtype):
        for bad in (np.nan, np.inf, -np.inf):
            r = rng.normal(-2000.0, 1.5, size=s)
            r[p] = bad
            rows.append(r)
    rows += [np.full(s, np.nan), np.full(s, -np.inf)]
    if s > 1:
        r = rng.normal(-2000.0, 1.5, size=s)
        r[0], r[1] = np.nan, np.inf
        rows.append(r)
        r = rng.normal(-2000.0, 1.5, size=s)
        r[-1], r[-2] = np.inf, np.nan
        rows.append(r)
        r = np.full(s, -3e10) - rng.uniform(0.0, 1e9, size=s)
        r[s // 2] = np.nan
        rows.append(r)
    return np.array(rows).astype(dtype)


@functools.lru_cache(maxsize=None)
def rows_and_reference(kind, s, dtype, seed=0):
    """(rows, lme, lme with NaN -> -1e10, NaN entries per row) -- computed once, shared, read-only"""
    rng = np.random.default_rng(1000003 * seed + 16 * s + vec(dtype))
    a = (shifted_rows if kind == "shifted" else nonfinite_rows)(rng, s, dtype)
    plain, _ = lme_ref(a, nan_fix=False)
    fixed, n_nan = lme_ref(a, nan_fix=True)
    for x in (a, plain, fixed, n_nan):
        x.setflags(write=False)
    return a, plain, fixed, n_nan


# ---------------------------------------------------------------------------------------------------------------- harness
class Source:
    """A host (n, S) matrix on the device as a view inside a NaN-filled allocation, guard rows before and after it.

    ``wave``: draws fastest, rows on 16-byte pitches (the guards cover 4096 draws on either side); ``lane``: observations
    fastest, an (S, n) buffer seen as .T; ``block``: every second draw of a buffer twice as wide."""

    def __init__(self, a, layout, want=None, n_nan=None):
        import torch

        n, s = a.shape
        t = torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared rows are read-only)
        full = lambda *shape: torch.full(shape, float("nan"), dtype=t.dtype, device="cuda")  # noqa: E731
        if layout == "wave":
            pitch = -(-s // vec(a.dtype)) * vec(a.dtype)
            g = max(2, -(-4096 // pitch))
            self.buf = full(g + n + g, pitch)
            self.buf[g:g + n, :s] = t
            first, self.stride_row, self.stride_draw = g * pitch, pitch, 1
        elif layout == "lane":
            g = 2
            self.buf = full(s, g + n + g)
            self.buf[:, g:g + n] = t.T
            first, self.stride_row, self.stride_draw = g, 1, g + n + g
        else:
            g = 2
            self.buf = full(g + n + g, 2 * s)
            self.buf[g:g + n, ::2] = t
            first, self.stride_row, self.stride_draw = g * 2 * s, 2 * s, 2
        self.base = self.buf.data_ptr() + first * a.itemsize
        self.host, self.layout, self.n_rows, self.n_draws, self.dtype = a, layout, n, s, a.dtype.type
        self.want = want      # lme of every row, as this source is flagged
        self.n_nan = n_nan    # NaN entries of every row that count as replaced (None: none do)


def source(layout, s, dtype, kind="shifted", flagged=False, seed=0):
    a, plain, fixed, n_nan = rows_and_reference(kind, s, dtype, seed)
    return Source(a, layout, fixed if flagged else plain, n_nan if flagged else None)


class Run:
    pass


def launch(eng, table, dtype, nan_flag, offsets, task_row, task_out, n_out):
    """One ``pla_kfold_lme`` call: (``out`` with its bands, the replaced count, ``last_kernels``)"""
    import torch

    from pyloo_amd import _capi

    dev = [torch.from_numpy(x).cuda() for x in (offsets, task_row, task_out)]
    out = torch.full((BAND + n_out + BAND,), SENTINEL, dtype=torch.float64, device="cuda")
    nrep = torch.full((1,), -7, dtype=torch.int64, device="cuda")  # (zeroed by the call)
    pn = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    pt = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rc = eng._lib.pla_kfold_lme(eng._h, *(pn(x) for x in table), len(table[0]), _capi.PLA_F32 if dtype == np.float32 else _capi.PLA_F64,
                                1 if nan_flag else 0, *(pt(x) for x in dev), task_row.size, _capi.PLA_DEVICE, eng._stream(),
                                C.c_void_p(out.data_ptr() + 8 * BAND), n_out, pt(nrep))
    assert rc == 0, eng._lib.pla_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(nrep.item()), eng.last_kernels()


def run(eng, sources, rows, nan_flag=False, edit=None, n_rows=None, seed=1):
    """``pla_kfold_lme`` on ``sources`` with the tasks ``rows[k]`` (row numbers, any length, repeats) of source k; ``task_out`` a
    permutation of the tasks.  ``edit(task_row, task_out, offsets, r)`` may overwrite entries (and states in ``r.row`` /
    ``r.slot`` what is to come of them), ``n_rows`` the table's row counts."""
    counts = np.array([len(r) for r in rows], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_out = int(offsets[-1])
    task_row = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows])
    task_out = np.random.default_rng(seed).permutation(n_out).astype(np.int64)
    r = Run()
    r.src = np.repeat(np.arange(len(sources)), counts)
    r.row = task_row.copy()   # the row every task is to read
    r.slot = task_out.copy()  # the slot it is to write (-1: none)
    if edit is not None:
        edit(task_row, task_out, offsets, r)
    dt = sources[0].dtype
    assert all(s.dtype == dt for s in sources)
    table = [np.array([s.base for s in sources], dtype=np.uint64),
             np.array([s.n_rows for s in sources] if n_rows is None else n_rows, dtype=np.int64),
             np.array([s.n_draws for s in sources], dtype=np.int64),
             np.array([s.stride_row for s in sources], dtype=np.int64),
             np.array([s.stride_draw for s in sources], dtype=np.int64)]
    o, r.n_replaced, r.kernels = launch(eng, table, dt, nan_flag, offsets, task_row, task_out, n_out)
    r.launches = int(re.search(r"; (\d+) launch(?:es)?\)", r.kernels).group(1))
    sent = np.float64(SENTINEL).view(np.int64)
    for band in (o[:BAND], o[BAND + n_out:]):
        assert np.all(band.view(np.int64) == sent), "a store outside [0, n_out)"
    r.out = o[BAND:BAND + n_out]
    written = np.zeros(n_out, dtype=bool)
    written[r.slot[r.slot >= 0]] = True
    assert np.all(r.out[~written].view(np.int64) == sent), "a slot no task names was written"
    r.got = r.out[np.where(r.slot >= 0, r.slot, 0)]  # per task (tasks without a slot: checked above, left out below)
    r.sources = sources
    return r


def same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.int64) == np.ascontiguousarray(b).view(np.int64)) | (np.isnan(a) & np.isnan(b))


def check(eng, r, nan_flag=False, baseline=True):
    """Every task against the yardstick; every task bit for bit against the first task that names its row and against a call
    that passes every distinct row once.  Returns the expected values per task."""
    sources = r.sources
    width = max(s.n_rows for s in sources)
    want = np.full((len(sources), width), np.nan)
    for k, s in enumerate(sources):
        want[k, :s.n_rows] = s.want
    live = r.slot >= 0
    src, row, got = r.src[live], r.row[live], r.got[live]
    exp = want[src, row]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
    np.testing.assert_allclose(got, exp, rtol=RTOL, atol=ATOL, equal_nan=True)
    key = src * width + row
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    same = same_bits(got, got[first][inverse])
    assert same.all(), ("tasks of one row differ", int(np.argmin(same)), int((~same).sum()))
    if baseline:
        used = [k for k, s in enumerate(sources) if s.n_rows > 0 and np.any(r.src == k)]
        once = run(eng, [sources[k] for k in used], [np.arange(sources[k].n_rows) for k in used], nan_flag and used[0] == 0)
        assert once.out.size < GRID_BLOCKS  # nothing chains on any route
        bits = np.full((len(sources), width), np.nan)
        for i, k in enumerate(used):
            bits[k, :sources[k].n_rows] = once.got[once.src == i]
        same = same_bits(got, bits[src, row])
        assert same.all(), ("a chained task differs from the row on its own", int(np.argmin(same)), int((~same).sum()))
    return exp


def cycle(rng, n_rows, count):
    return rng.integers(0, n_rows, size=count)


def tasks_of(rng, sources, counts):
    return [cycle(rng, s.n_rows, c) for s, c in zip(sources, counts)]


def only(r, *layouts):
    """the kernels of exactly these routes ran, one launch each"""
    for layout, name in KERNEL.items():
        assert (name in r.kernels) == (layout in layouts), r.kernels
    assert r.launches == len(layouts), r.kernels


# -------------------------------------------------------------------------------------- 1. several tasks per wave, changing length
# (S, tasks) in task order: the first sixteen thousand tasks are the waves' first, the next their second, the last five a third
WAVE_FIRST = [(4096, 2000), (257, 1000), (1, 1000), (3, 1000), (65, 1000), (64, 2000), (2, 1000), (128, 1000), (4, 1000), (5, 1000),
              (127, 1000), (129, 1000), (63, 2384)]
WAVE_SECOND = [(1, 1000), (7, 1000), (63, 1000), (4096, 1000), (4095, 1000), (64, 1000), (65, 1000), (64, 1000), (3, 1000),
               (257, 1000), (4096, 1000), (2, 1000), (129, 1000), (5, 1000), (4095, 2384 + 5)]
PAIRS = {(4096, 1), (4096, 7), (257, 63), (1, 4096), (3, 4095), (65, 64), (64, 65), (2, 3), (64, 64)}


@pytest.mark.parametrize("dt", DTYPES)
def test_wave_takes_rows_of_changing_length(eng, dt):
    plan = WAVE_FIRST + WAVE_SECOND
    assert sum(c for _, c in WAVE_FIRST) == GRID_WAVES and sum(c for _, c in plan) == 2 * GRID_WAVES + 5
    assert {s for s, _ in plan} == {1, 2, 3, 4, 5, 7, 63, 64, 65, 127, 128, 129, 257, 4095, 4096}
    length = np.repeat([s for s, _ in plan], [c for _, c in plan])
    pairs = set(zip(length[:-GRID_WAVES].tolist(), length[GRID_WAVES:].tolist()))  # (row in the registers, row streamed in)
    assert PAIRS <= pairs, PAIRS - pairs
    assert (1, 4095) in set(zip(length[GRID_WAVES:-GRID_WAVES].tolist(), length[2 * GRID_WAVES:].tolist()))  # second -> third
    rng = np.random.default_rng(41)
    sources = [source("wave", s, dt, seed=i) for i, (s, _) in enumerate(plan)]
    r = run(eng, sources, tasks_of(rng, sources, [c for _, c in plan]))
    only(r, "wave")
    check(eng, r)
    assert r.n_replaced == 0


# -------------------------------------------------------------------------------------------------- 2. stepping over other routes
MIXED_FIRST = [("lane", 7, 100), ("wave", 4096, 1900), ("wave", 257, 1000), ("wave", 1, 1000), ("wave", 3, 1000), ("wave", 65, 1000),
               ("wave", 64, 2000), ("block", 255, 100), ("wave", 2, 900), ("wave", 128, 1000), ("wave", 4, 1000), ("wave", 5, 1000),
               ("wave", 127, 1000), ("wave", 129, 1000), ("wave", 63, 2384)]
MIXED_SECOND = [("wave", 1, 50), ("block", 257, 100), ("wave", 1, 850), ("wave", 7, 1000), ("wave", 63, 1000), ("wave", 4096, 1000),
                ("wave", 4095, 1000), ("wave", 64, 1000), ("wave", 65, 1000), ("wave", 64, 1000), ("lane", 257, 100), ("wave", 3, 900),
                ("wave", 257, 1000), ("wave", 4096, 1000), ("wave", 2, 1000), ("wave", 129, 1000), ("wave", 5, 1000),
                ("wave", 4095, 2384 + 200)]


@pytest.mark.parametrize("dt", DTYPES)
def test_wave_steps_over_tasks_of_other_routes(eng, dt):
    plan = MIXED_FIRST + MIXED_SECOND
    assert sum(c for _, _, c in MIXED_FIRST) == GRID_WAVES and sum(c for _, _, c in plan) == 2 * GRID_WAVES + 200
    wave = np.repeat([layout == "wave" for layout, _, _ in plan], [c for _, _, c in plan])
    a, b, c = wave[:200], wave[GRID_WAVES:GRID_WAVES + 200], wave[2 * GRID_WAVES:]
    assert np.any(a & ~b & c)   # second task of another route, the third a wave task again
    assert np.any(~a & ~b & c)  # two tasks in a row to step over
    assert np.any(~a & b & c)
    assert np.any(~wave[200:GRID_WAVES] & ~wave[GRID_WAVES + 200:2 * GRID_WAVES])  # ... and no third task behind them
    rng = np.random.default_rng(43)
    sources = [source(layout, s, dt, seed=i) for i, (layout, s, _) in enumerate(plan)]
    r = run(eng, sources, tasks_of(rng, sources, [c for _, _, c in plan]))
    only(r, "wave", "lane", "block")
    check(eng, r)


# ------------------------------------------------------------------------------------------- 3. several sweeps of the lane kernel
# source boundaries inside a wave's 64 tasks on the first sweep (tasks 1000 and 70 037) and on the second (20, 97 and 194 tasks in)
LANE_PLAN = [(7, 1000), (257, 69037), (7, 500000), (257, GRID_LANES + 20 - 570037), (7, 77), (257, 97), (7, 3)]


@pytest.mark.parametrize("dt", DTYPES)
def test_lane_kernel_sweeps_twice(eng, dt):
    ends = np.cumsum([c for _, c in LANE_PLAN])
    assert ends[-1] == GRID_LANES + 64 * 3 + 5
    assert [int(e) % 64 for e in ends[:2]] == [40, 21] and [int(e) - GRID_LANES for e in ends[3:]] == [20, 97, 194, 197]
    rng = np.random.default_rng(47)
    sources = []
    for i, (s, _) in enumerate(LANE_PLAN):
        parts = [rows_and_reference("shifted", s, dt, seed=100 + 3 * i + j) for j in range(3)]  # 24 rows
        sources.append(Source(np.concatenate([p[0] for p in parts]), "lane", np.concatenate([p[1] for p in parts])))
    r = run(eng, sources, tasks_of(rng, sources, [c for _, c in LANE_PLAN]))
    only(r, "lane")
    check(eng, r)


# ------------------------------------------------------------------------------- 4. several tasks per workgroup of the block kernel
BLOCK_PLAN = [(1, 2000), (255, 2000), (4097, 2000), (256, 2192), (257, 3000), (1, 2000), (4097, 3192), (255, 5)]


@pytest.mark.parametrize("n_tasks", [GRID_BLOCKS + 5, 2 * GRID_BLOCKS + 5])
@pytest.mark.parametrize("dt", DTYPES)
def test_block_kernel_takes_several_tasks(eng, dt, n_tasks):
    assert sum(c for _, c in BLOCK_PLAN[:4]) == GRID_BLOCKS and sum(c for _, c in BLOCK_PLAN) == 2 * GRID_BLOCKS + 5
    plan = BLOCK_PLAN if n_tasks > 2 * GRID_BLOCKS else BLOCK_PLAN[:4] + [(257, 5)]
    assert sum(c for _, c in plan) == n_tasks
    rng = np.random.default_rng(53)
    sources = [source("block", s, dt, seed=i) for i, (s, _) in enumerate(plan)]
    r = run(eng, sources, tasks_of(rng, sources, [c for _, c in plan]))
    only(r, "block")
    check(eng, r)


# ------------------------------------------------------------------------------------------------- 5. non-finite entries, chained
NONFINITE_S = (1, 3, 5, 65, 4095, 4096)


def nonfinite_sources(layout, s0, dt):
    """source 0 (S = s0) is the one the flag applies to; one more source per length without it"""
    def both(flagged):
        return [source(layout, s0, dt, "nonfinite", flagged=flagged)] + [source(layout, s, dt, "nonfinite", seed=1) for s in NONFINITE_S]

    return both(True), both(False)


def replaced(r):
    first = r.src == 0
    return int(r.sources[0].n_nan[r.row[first]].sum())


@pytest.mark.parametrize("s0", NONFINITE_S)
@pytest.mark.parametrize("dt", DTYPES)
def test_nonfinite_rows_in_a_waves_chain(eng, dt, s0):
    flagged, plain = nonfinite_sources("wave", s0, dt)
    counts = [30000] + [1667] * 5 + [1665]
    assert 2 * GRID_WAVES <= sum(counts) == 40000 <= 3 * GRID_WAVES
    rows = tasks_of(np.random.default_rng(59 + s0), flagged, counts)
    r = run(eng, flagged, rows, nan_flag=True)
    only(r, "wave")
    exp = check(eng, r, nan_flag=True)
    # 0: a clean row; 1: NaN taken as -1e10 and a finite result; 2: a NaN result; 3: -inf entries, a finite result
    nan_in = np.concatenate([np.isnan(s.host).any(axis=1)[w] for s, w in zip(flagged, rows)])
    finite_in = np.concatenate([np.isfinite(s.host).all(axis=1)[w] for s, w in zip(flagged, rows)])
    cls = np.where(np.isnan(exp), 2, np.where(finite_in, 0, np.where(nan_in & (r.src == 0), 1, 3)))
    pairs = set(zip(cls[:-GRID_WAVES].tolist(), cls[GRID_WAVES:].tolist()))
    assert {(1, 0), (0, 1), (2, 0), (0, 2)} <= pairs, pairs
    # first, middle and last in a chain (the flagged source's tasks end before the waves' third)
    assert {0, 1, 2} <= set(cls[:GRID_WAVES].tolist()) and {0, 1, 2} <= set(cls[GRID_WAVES:2 * GRID_WAVES].tolist())
    assert {0, 2} <= set(cls[2 * GRID_WAVES:].tolist())
    assert r.n_replaced == replaced(r) > 0  # (the NaN of the other sources and the slots past a row count nothing)
    # without the flag nothing is replaced and nothing counted
    r = run(eng, plain, rows, nan_flag=False)
    exp = check(eng, r)
    assert r.n_replaced == 0 and np.all(np.isnan(exp[nan_in]))


@pytest.mark.parametrize("layout", ["lane", "block"])
@pytest.mark.parametrize("dt", DTYPES)
def test_nonfinite_rows_on_the_other_layouts(eng, dt, layout):
    for s0 in NONFINITE_S:
        flagged, plain = nonfinite_sources(layout, s0, dt)
        rows = tasks_of(np.random.default_rng(61 + s0), flagged, [150] + [40] * 6)
        r = run(eng, flagged, rows, nan_flag=True)
        only(r, layout)
        check(eng, r, nan_flag=True)
        assert r.n_replaced == replaced(r) > 0
        r = run(eng, plain, rows, nan_flag=False)
        check(eng, r)
        assert r.n_replaced == 0


# ------------------------------------------------------------------------------------------------------------------- 6. bounds
# "near": one row / one slot outside -- the NaN guard rows and the sentinel bands; "far": 2^40 away
ROWS_OUTSIDE = {"near": (-1, None), "far": (-2 ** 40, 2 ** 40)}   # (None: the source's n_rows)
SLOTS_OUTSIDE = {"near": (-1, None), "far": (2 ** 40, 2 ** 40)}   # (None: n_out)


@pytest.mark.parametrize("reach", ["near", "far"])
@pytest.mark.parametrize("layout", ["wave", "lane", "block"])
@pytest.mark.parametrize("dt", DTYPES)
def test_rows_are_clamped_and_stores_outside_dropped(eng, dt, layout, reach):
    """task_row below 0 / at or past n_rows reads row 0 / the last row; task_out outside [0, n_out) stores nothing; a source
    without rows is skipped with its tasks; a source without tasks in the middle of the table changes nothing."""
    sources = [source(layout, 65, dt), source(layout, 7, dt, seed=1), source(layout, 3, dt, seed=2), source(layout, 5, dt, seed=3)]
    n_rows = [sources[0].n_rows, 0, sources[2].n_rows, sources[3].n_rows]
    rng = np.random.default_rng(67)
    rows = tasks_of(rng, sources, [100, 20, 0, 100])
    low, high = ROWS_OUTSIDE[reach]
    s_low, s_high = SLOTS_OUTSIDE[reach]

    def edit(task_row, task_out, offsets, r):
        assert offsets[2] == offsets[3] == 120
        n_out = int(offsets[-1])
        for k in (0, 3):
            t = int(offsets[k])
            last = sources[k].n_rows - 1
            task_row[t + 3], r.row[t + 3] = low, 0
            task_row[t + 7], r.row[t + 7] = (last + 1 if high is None else high), last
            task_row[t + 64], r.row[t + 64] = low, 0  # (the first task of a wave's 64 on the lane route)
            task_out[t + 11], r.slot[t + 11] = s_low, -1
            task_out[t + 13], r.slot[t + 13] = (n_out if s_high is None else s_high), -1
        r.slot[offsets[1]:offsets[2]] = -1  # the source without rows

    r = run(eng, sources, rows, edit=edit, n_rows=n_rows)
    only(r, layout)
    check(eng, r, baseline=False)
    assert (r.slot < 0).sum() == 24 and np.isfinite(r.got[r.slot >= 0]).all()
    clean = run(eng, [sources[0], sources[3]], [rows[0], rows[3]])  # the same rows without the edits: the same bits
    keep = r.slot[r.src != 1] >= 0
    both = clean.row == r.row[r.src != 1]
    assert same_bits(clean.got[keep & both], r.got[r.src != 1][keep & both]).all()


# --------------------------------------------------------------------------------------------------------- 7. through Engine.kfold
@pytest.mark.parametrize("dt", DTYPES)
def test_engine_kfold_with_two_tasks_per_wave(eng, dt):
    """N = 16 384 + 37 observations, so 2 N tasks: every wave takes two, most of them from two sources."""
    n = GRID_WAVES + 37
    rng = np.random.default_rng(71)
    folds = rng.integers(1, 4, size=n)
    shift = np.choose(np.arange(n) % 3, [0.0, -2000.0, 900.0])
    full = (rng.normal(-1.5, 1.5, size=(n, 96)) + shift[:, None]).astype(dt)
    mats = [(rng.normal(-2.5, 2.0, size=(int(np.sum(folds == k + 1)), s)) + shift[folds == k + 1, None]).astype(dt)
            for k, s in enumerate((7, 65, 257))]
    res = eng.kfold(padded(full), [padded(m) for m in mats], folds)
    kern = eng.last_kernels()
    assert kern.startswith("kfold_wave_kernel<%s> (matrices read in place; 1 launch)" % ("double" if dt == np.float64 else "float")), kern
    g = {k: v.cpu().numpy() for k, v in res.items()}
    elpd = np.empty(n)
    for k, m in enumerate(mats):
        elpd[folds == k + 1] = lme_ref(m)[0]
    np.testing.assert_allclose(g["lpd_full_i"], lme_ref(full)[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(g["elpd_i"], elpd, rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(g["p_i"], g["lpd_full_i"] - g["elpd_i"])
    np.testing.assert_array_equal(g["kfold_i"], g["elpd_i"])
    check_agg(g)
