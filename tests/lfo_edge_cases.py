"""TEST INFRASTRUCTURE ONLY: the case table of the leave-future-out edge suites.

``tests/test_lfo_edges_host.py`` proves, on the CPU reference alone, the properties that make a comparison on these inputs
meaningful (finite k, no tie inside a Pareto tail, thresholds in a gap, the geometric claim each case is named after);
``tests/test_gpu_lfo_edges.py`` runs the same inputs through ``Engine.lfo``.  The inputs are defined here, once.

A case is one pass: ``mode`` "forward" (``anchor`` = first) or "backward" (``anchor`` = last), a matrix drawn by
``lfo_ref.draw_ll(default_rng(seed), n, s, dtype, k_lo, k_hi)`` and then ``cells``, the non-finite entries, written into it as
``(row, draws, value)`` with ``draws`` an index or a ``(start, stop, step)`` slice.

The constants of the kernels the geometry is computed from (csrc/pla_lfo.h, include/pyloo_amd.h):

    LANES = 64 lanes of a wavefront, each owning vectors of V = 16 / itemsize draws: vector q of lane l is draws
    V (l + 64 q) .. + V - 1;  nq = ceil(S / (64 V)) vectors per lane, of which the first n3 = nq - 1 lie inside the row for every
    lane ("whole") and the last is clamped;  rows of at most REG_DRAWS = 64 x 64 draws sit in registers, longer ones are
    streamed;  the register route walks the whole vectors in batches of BATCH = 16 / V;  the future rows are added four at a
    time (ROWS_IN_FLIGHT);  the predict grid is at most PREDICT_GRID workgroups of PREDICT_WAVES wavefronts, a wavefront per
    step;  first_high is one workgroup of FIRST_HIGH_THREADS;  the sums are chunks of lfo_ref.CHUNK rows and a block of steps
    is whole chunks.

Seeds: ``zlib.crc32`` of the case's name, except the cases listed in ``RESEEDED`` -- their first seed put two equal log ratios
into a Pareto tail (property (b) of the host file), where the smoothed weight of the tied draws is the implementation's choice.
"""

import collections
import functools
import zlib

import numpy as np

import lfo_bw_ref
import lfo_ref
from oracle import psis_oracle as orc

LANES = 64
SLOTS = 64
REG_DRAWS = LANES * SLOTS
ROWS_IN_FLIGHT = 4
PREDICT_GRID, PREDICT_WAVES = 8192, 4
FIRST_HIGH_THREADS = 256
C = lfo_ref.CHUNK
DTYPES = {"f8": np.float64, "f4": np.float32}
NINF, PINF, NAN = -np.inf, np.inf, np.nan

Case = collections.namedtuple("Case", "name group mode seed n s dtype anchor n_steps M k_lo k_hi cells")

RESEEDED = {  # name -> seed (see the module docstring); all of them sums of f32 rows
    "route-fw-f4-S4095-M3": 1, "route-fw-f4-S4095-M6": 1, "route-fw-f4-S4096-M3": 1, "route-fw-f4-S4096-M6": 1,
    "route-bw-f4-S4096-M3-last37": 1, "route-fw-f4-S4099-M3": 4,
}


def vec(dtype):
    return 16 // np.dtype(DTYPES[dtype]).itemsize


def batch(dtype):
    return 16 // vec(dtype)


def nq(s, dtype):
    return -(-s // (LANES * vec(dtype)))


def n3(s, dtype):
    return nq(s, dtype) - 1


def route(s):
    return "registers" if s <= REG_DRAWS else "streamed"


def loads(s, dtype):
    """of a matrix whose rows are 16-byte aligned (a contiguous device tensor, a staged block)."""
    return "16-byte loads" if s % vec(dtype) == 0 else "element loads"


def last_whole_vector(s, dtype):
    """[lo, hi): the draws of the lanes' last whole vectors (the ones the padded slots of a batch load again)."""
    w = LANES * vec(dtype)
    return (n3(s, dtype) - 1) * w, n3(s, dtype) * w


def groups_of_rows(M):
    """(groups of the four-rows-in-flight loop over rows 1 .. M - 1, padded rows of the last group)."""
    g = -(-(M - 1) // ROWS_IN_FLIGHT)
    return g, g * ROWS_IN_FLIGHT - (M - 1)


def seed_of(name):
    return RESEEDED.get(name, zlib.crc32(name.encode()))


def geometry(case):
    """dict(t0, q0, j_min, lo, hi, rows): the first step's row, last - t0, the first step first_high looks at, the lowest and
    highest row the pass may read, and per step the rows of its window as (first row, one past the last)."""
    if case.mode == "forward":
        t = case.anchor + np.arange(case.n_steps)
        return {"t0": case.anchor, "q0": 0, "j_min": 1, "lo": case.anchor, "hi": case.anchor + case.n_steps + case.M - 2, "t": t}
    t0 = min(case.anchor, case.n - case.M)
    t = t0 - np.arange(case.n_steps)
    return {"t0": t0, "q0": case.anchor - t0, "j_min": 1 if case.anchor == t0 else 0, "lo": t0 - case.n_steps + 1, "hi": t0 + case.M - 1,
            "t": t}


def ratio_rows(case):
    """[lo, hi): the rows that enter a log-ratio sum of the pass."""
    if case.mode == "forward":
        return case.anchor, case.anchor + case.n_steps - 1
    return geometry(case)["lo"], case.anchor  # (backward a step's own row is in its sum)


def counting_steps(case, row):
    """The steps that count the NaN entries of ``row`` (exactly one for a row the pass reads): step 0 the whole of its window,
    every other step its window's last row (forward) or first row (backward)."""
    g = geometry(case)
    out = []
    for j, t in enumerate(g["t"]):
        if j == 0:
            hit = t <= row < t + case.M
        else:
            hit = row == (t + case.M - 1 if case.mode == "forward" else t)
        if hit:
            out.append(j)
    return out


@functools.lru_cache(maxsize=None)
def matrix(case):
    ll = lfo_ref.draw_ll(np.random.default_rng(case.seed), case.n, case.s, DTYPES[case.dtype], k_lo=case.k_lo, k_hi=case.k_hi)
    for row, draws, value in case.cells:
        ll[row, slice(*draws) if isinstance(draws, tuple) else draws] = value
    ll.setflags(write=False)
    return ll


def tail(case):
    return orc.tail_count(case.s, 1.0)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The CPU reference of the case, computed once and left unchanged."""
    fn = lfo_ref.lfo_pass if case.mode == "forward" else lfo_bw_ref.lfo_pass
    ref = fn(matrix(case), case.anchor, case.n_steps, case.M)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def importance_steps(case):
    g = geometry(case)
    return [j for j, t in enumerate(g["t"]) if not (j == 0 and g["j_min"] == 1)]


def tied_steps(case, ref=None):
    """The importance steps with two equal log ratios among the tail_count + 1 largest (the guard of ``reference()`` in
    tests/test_gpu_lfo_bw.py)."""
    ref = ref or reference(case)
    m = tail(case)
    return [j for j in importance_steps(case) if not np.all(np.diff(np.sort(ref["ratios"][j])[-m - 1:]) > 0)]


def gap_around(k, j_min, thr):
    """The width of the gap between the finite k of the steps first_high looks at in which ``thr`` lies, and how far ``thr`` is from
    its nearer edge (inf where there is no k on a side)."""
    v = k[j_min:][np.isfinite(k[j_min:])]
    below, above = v[v <= thr], v[v > thr]
    lo = below.max() if below.size else -np.inf
    hi = above.min() if above.size else np.inf
    return hi - lo, min(thr - lo, hi - thr)


def threshold(case, ref=None):
    """The middle of the widest gap between the finite k of the steps first_high looks at (the rule of ``threshold_for`` in
    tests/test_gpu_lfo_bw.py): no rounding-level difference can move first_high.  0.7 for a pass of the exact step alone."""
    k = (ref or reference(case))["diag"][geometry(case)["j_min"]:]
    v = np.sort(k[np.isfinite(k)])
    if v.size < 2:
        return 0.7
    i = int(np.argmax(np.diff(v)))
    return 0.5 * (v[i] + v[i + 1])


def first_high(case, k, thr):
    j_min = geometry(case)["j_min"]
    return lfo_bw_ref.first_high(k, thr, j_min)


# ---------------------------------------------------------------------------------------------------------------------- builders
def _case(name, group, mode, n, s, dtype, anchor, n_steps, M, cells=(), k_lo=0.05, k_hi=0.6):
    return Case(name, group, mode, seed_of(name), n, s, dtype, anchor, n_steps, M, k_lo, k_hi, tuple(cells))


FIRST, STEPS = 4, 30  # passes of about 30 rows
N_BW = 44             # backward: last = N_BW (no step is exact) or N_BW - 7 (a refit)


def forward(name, group, s, dtype, M, cells=None, n_steps=STEPS, spare=0, **kw):
    """n_steps at its maximum when spare = 0: the last window ends on row n - 1.  ``cells(first, n_steps, M, n)``."""
    n = FIRST + n_steps + M - 1 + spare
    return _case(f"{name}-fw-{dtype}-S{s}-M{M}", group, "forward", n, s, dtype, FIRST, n_steps, M,
                 cells(FIRST, n_steps, M, n) if cells else (), **kw)


def backward(name, group, s, dtype, M, back=7, cells=None, n_steps=STEPS, n=N_BW, **kw):
    """last = n - back.  ``cells(t0, lo, hi, n)``: the first step's row, the lowest and the highest row of the pass."""
    last = n - back
    t0 = min(last, n - M)
    made = cells(t0, t0 - n_steps + 1, t0 + M - 1, n) if cells else ()
    return _case(f"{name}-bw-{dtype}-S{s}-M{M}-last{last}", group, "backward", n, s, dtype, last, n_steps, M, made, **kw)


# 1. the horizon (rows 1 .. M - 1 go four at a time): the first group full, a second of one row and three padded ones, two groups
# minus one row, two full groups, a third group
HORIZON_M = (5, 6, 8, 9, 10)
HORIZON_SHAPES = (("f8", 257), ("f8", 4100), ("f4", 1028))

# 2. route x dtype x load width (of a matrix with aligned rows)
ROUTE_TABLE = (("f4", 255, "registers", "element loads"), ("f4", 4095, "registers", "element loads"),
               ("f4", 256, "registers", "16-byte loads"), ("f4", 4096, "registers", "16-byte loads"),
               ("f4", 4100, "streamed", "16-byte loads"), ("f4", 4099, "streamed", "element loads"),
               ("f8", 128, "registers", "16-byte loads"), ("f8", 4094, "registers", "16-byte loads"),
               ("f8", 4095, "registers", "element loads"), ("f8", 40, "registers", "16-byte loads"))

# 3. the batches of the register route: n3 on a batch boundary, the same with a full last vector, one past it
BATCH_TABLE = (("f8", 1026, 8, False), ("f8", 1152, 8, True), ("f8", 1154, 9, False),
               ("f4", 1028, 4, False), ("f4", 1280, 4, True), ("f4", 1284, 5, False))  # (dtype, S, n3, the last vector is full)

# 4. NaN accounting
NAN_M = (2, 5, 6, 9)
NAN_S = (257, 1154, 4100)
NAN_MID = 15  # the step whose counted row holds the middle NaN entries


def nan_draws(s, dtype="f8"):
    """draw 0, a draw inside the lanes' last whole vector (lane 37, its last element), draw S - 1 (in the clamped vector)."""
    lo, _ = last_whole_vector(s, dtype)
    return 0, lo + 37 * vec(dtype) + vec(dtype) - 1, s - 1


def _nan_forward(s):
    def cells(first, n_steps, M, n):
        last_only, in_step0, middle = first + n_steps + M - 2, first, first + NAN_MID + M - 1
        out = [(r, d, NAN) for r in (last_only, in_step0, middle) for d in nan_draws(s)]
        return out + [(first - 1, 3, NAN), (n - 1, 3, NAN)]  # (spare = 1: row n - 1 lies past the last window)
    return cells


def _nan_backward(s):
    def cells(t0, lo, hi, n):
        out = [(r, d, NAN) for r in (lo, hi, t0 - NAN_MID) for d in nan_draws(s)]
        out.append((lo - 1, 3, NAN))
        if hi + 1 < n:
            out.append((hi + 1, 3, NAN))
        return out
    return cells


# 5. non-finite future terms, in rows that enter no ratio sum (forward: rows >= first + n_steps - 1; backward: rows >= last)
INF_S = (300, 4100)


def _build():
    cases = []
    for dtype, s in HORIZON_SHAPES:
        for M in HORIZON_M:
            cases.append(forward("horizon", "horizon", s, dtype, M))
            cases.append(backward("horizon", "horizon", s, dtype, M, back=0, k_lo=0.02, k_hi=0.2))
            cases.append(backward("horizon", "horizon", s, dtype, M, back=7, k_lo=0.02, k_hi=0.2))
    for dtype, s, _, _ in ROUTE_TABLE:
        cases.append(forward("route", "route", s, dtype, 3))
        cases.append(forward("route", "route", s, dtype, 6))
        cases.append(backward("route", "route", s, dtype, 3, back=7, k_lo=0.02, k_hi=0.2))  # step 0 is exact
        cases.append(backward("route", "route", s, dtype, 6, back=0, k_lo=0.02, k_hi=0.2))  # no step is
    for dtype, s, _, _ in BATCH_TABLE:
        cases.append(forward("batch", "batch", s, dtype, 5))
        cases.append(backward("batch", "batch", s, dtype, 5, back=7, k_lo=0.02, k_hi=0.2))
    for s in NAN_S:
        for M in NAN_M:
            cases.append(forward("nan", "nan", s, "f8", M, cells=_nan_forward(s), spare=1))
            cases.append(backward("nan", "nan", s, "f8", M, back=7, cells=_nan_backward(s), k_lo=0.02, k_hi=0.2))
    for s in INF_S:
        # (i) -inf on every third draw of the top row of the last (forward) / first (backward) step's window, +inf in the row below it
        cases.append(forward("inf_mix", "inf_mix", s, "f8", 3, cells=lambda f, ns, M, n: [(n - 1, (0, None, 3), NINF), (n - 2, 7, PINF)]))
        cases.append(backward("inf_mix", "inf_mix", s, "f8", 3, cells=lambda t0, lo, hi, n: [(hi, (0, None, 3), NINF), (hi - 1, 7, PINF)],
                              k_lo=0.02, k_hi=0.2))
        # (ii) that row -inf as a whole: an importance step (forward; backward M = 9) and the exact step (backward M = 3)
        cases.append(forward("inf_row", "inf_row", s, "f8", 3, cells=lambda f, ns, M, n: [(n - 1, (None,), NINF)]))
        for M in (3, 9):
            cases.append(backward("inf_row", "inf_row", s, "f8", M, cells=lambda t0, lo, hi, n: [(hi, (None,), NINF)], k_lo=0.02, k_hi=0.2))
        # (iii) the exact step alone
        cases.append(forward("inf_exact", "inf_exact", s, "f8", 3, n_steps=1, cells=lambda f, ns, M, n: [(f + M - 1, (None,), NINF)]))
        # (iv) two -inf entries in one ratio row (the draws drop out of every later step): forward only -- backward the ratio of
        # such a draw is +inf, and the reference's weights are NaN from that row on
        cases.append(forward("inf_ratio", "inf_ratio", s, "f8", 3, cells=lambda f, ns, M, n: [(11, 0, NINF), (11, 5, NINF)]))
    return cases


# 6. the predict grid wraps: five wavefronts take a second step
WRAP_STEPS = PREDICT_GRID * PREDICT_WAVES + 5
WRAP_S, WRAP_M = 100, 2
_n = FIRST + WRAP_STEPS + WRAP_M - 1
WRAP_FW = _case("wrap-fw", "wrap", "forward", _n, WRAP_S, "f8", FIRST, WRAP_STEPS, WRAP_M, k_lo=0.001, k_hi=0.003, cells=(
    (FIRST + 2 + WRAP_M - 1, 50, NAN),                              # counted by step 2, whose wavefront takes a second step
    (FIRST + (WRAP_STEPS - 4) + WRAP_M - 1, 0, NAN), (_n - 1, 99, NAN)))  # counted by wrapped steps only (the fourth last, the last)
_n = WRAP_STEPS + 3  # last = n - 1: t_0 = n - 2 (q0 = 1), the lowest step is row 2
WRAP_BW = _case("wrap-bw", "wrap", "backward", _n, WRAP_S, "f8", _n - 1, WRAP_STEPS, WRAP_M, k_lo=0.001, k_hi=0.003, cells=(
    (_n - 1, 50, NAN),             # the top of step 0's window (>= last: in no ratio); its wavefront takes a second step
    (2, 0, NAN), (2, 99, NAN)))    # the lowest step's own row: counted by the last wrapped step, in no ratio
del _n

# 7. first_high beyond one stride of the workgroup
HIGH_STEPS, HIGH_S, HIGH_M = 600, 100, 3
# (seeds searched for: k has to cross late -- a crossing beyond step 256 and one beyond 512, each with a gap around it)
HIGH_FW = _case("high-fw", "high", "forward", 700, HIGH_S, "f8", FIRST, HIGH_STEPS, HIGH_M, k_lo=0.01, k_hi=0.05)._replace(seed=11)
HIGH_BW = _case("high-bw", "high", "backward", 700, HIGH_S, "f8", 699, HIGH_STEPS, HIGH_M, k_lo=0.01, k_hi=0.05)._replace(seed=6)  # q0 = 2
# (threshold, first_high of the reference): every threshold in the middle of a gap of the reference's k, an answer in each of
# HIGH_RANGES (a thread's first, second and third iteration; none), tests/test_lfo_edges_host.py proves both.  The last
# threshold of HIGH_BW lies below k_0: step 0 is no exact step there, and the answer is 0.
HIGH_RANGES = ((2, 256), (257, 512), (513, 599), (600, 600))
HIGH_THRESHOLDS = {"high-fw": ((-0.0678, 6), (0.2863, 29), (0.5175, 85), (0.5319, 111), (0.6822, 490), (0.7234, 596), (0.9, 600)),
                   "high-bw": ((0.5028, 4), (0.6809, 135), (0.7026, 462), (0.8257, 484), (0.8519, 595), (1.2, 600), (-0.25, 0))}

# 8. the block hand-over with a long window (child processes: PLA_INGEST_BLOCK_MB unset against 1)
BLOCK_S, BLOCK_STEPS, BLOCK_N, BLOCK_SEED = 4097, 200, 213, 9
BLOCK_M = (6, 9)
BLOCK_LAST = BLOCK_N - 7
BLOCK_NAN = ((69, 11), (70, 4096), (144, 11), (146, 0))


def block_matrix():
    ll = lfo_ref.draw_ll(np.random.default_rng(BLOCK_SEED), BLOCK_N, BLOCK_S, k_lo=0.02, k_hi=0.2)
    for r, d in BLOCK_NAN:
        ll[r, d] = np.nan
    return ll


def block_cases():
    """[(mode, anchor, M)] of the calls a child makes, in order."""
    return [(mode, FIRST if mode == "forward" else BLOCK_LAST, M) for mode in ("forward", "backward") for M in BLOCK_M]


def block_steps_per_block(block_mb=1):
    """Steps (forward) or q (backward) per block under PLA_INGEST_BLOCK_MB: the block's size in f64 ratios, whole chunks, one at least."""
    rows = (block_mb << 20) // (BLOCK_S * 8)
    return max(C, rows // C * C)


CASES = _build()
BY_NAME = {c.name: c for c in CASES + [WRAP_FW, WRAP_BW, HIGH_FW, HIGH_BW]}
assert len(BY_NAME) == len(CASES) + 4


def group(name):
    return [c for c in CASES if c.group == name]
