"""The inputs of tests/test_gpu_lfo_edges.py (tests/lfo_edge_cases.py) on the CPU reference alone, without a GPU: the properties
that make the comparison on the GPU meaningful, and the geometric claim every case is named after, computed from the constants
the library documents (csrc/pla_lfo.h, include/pyloo_amd.h).

(a) k of the reference is finite at every importance step and elpd at every step, except where a case is built otherwise -- and
    then exactly there: the non-finite future terms give NaN elpd at the steps named below; a NaN entry in a ratio row of a
    BACKWARD pass counts as -1e10, its draw's ratio is +1e10, and three (two) such draws carry all the weight: fewer than five
    draws in the tail, k = +inf by the reference's rule, from that row's step on.
(b) no two log ratios among the tail_count + 1 largest of an importance step are equal (with a tie the smoothed weight of the
    tied draws is the implementation's choice, and elpd moves at 1e-6).  An assertion, for every case: no case is dropped.
(c) every threshold first_high is asked with lies in a gap of at least 2e-3 between the reference's finite k.
(d) the geometry."""

import numpy as np
import pytest

import lfo_edge_cases as ec
import lfo_ref

C = lfo_ref.CHUNK
IDS = [c.name for c in ec.CASES]
LONG = [ec.WRAP_FW, ec.WRAP_BW, ec.HIGH_FW, ec.HIGH_BW]


def infinite_k_from(case):
    """The first step whose k the case is built to make +inf (see (a)), or None."""
    if case.mode == "backward" and case.group == "nan":
        return ec.NAN_MID
    if case.name == "wrap-bw":
        return case.n_steps - 1
    return None


def nan_elpd_steps(case):
    """The steps whose elpd the case is built to make NaN."""
    last = case.n_steps - 1
    if case.group == "inf_mix":  # the +inf row lies in two windows, the -inf entries alone leave a step finite
        return [last - 1, last] if case.mode == "forward" else [0, 1]
    if case.group == "inf_row":
        return [last] if case.mode == "forward" else [0]
    if case.group == "inf_exact":
        return [0]
    return []


@pytest.mark.parametrize("case", ec.CASES + LONG, ids=IDS + [c.name for c in LONG])
def test_reference_is_finite_untied_and_its_thresholds_lie_in_gaps(case):
    ref = ec.reference(case)
    g = ec.geometry(case)
    k, elpd = ref["diag"], ref["elpd_i"]
    imp = np.array(ec.importance_steps(case), dtype=np.int64)
    # (a)
    first_inf = infinite_k_from(case)
    want_inf = np.zeros(case.n_steps, dtype=bool)
    if first_inf is not None:
        want_inf[first_inf:] = True
    assert np.array_equal(np.isposinf(k[imp]), want_inf[imp]) and np.isfinite(k[imp][~want_inf[imp]]).all(), case.name
    assert (k[0] == 0.0) == (g["j_min"] == 1)
    want_nan = np.zeros(case.n_steps, dtype=bool)
    want_nan[nan_elpd_steps(case)] = True
    assert np.array_equal(np.isnan(elpd), want_nan) and np.isfinite(elpd[~want_nan]).all(), (case.name, np.flatnonzero(~np.isfinite(elpd)))
    # (b)
    assert ec.tied_steps(case, ref) == [], case.name
    # (c)
    if case.group == "high":
        pairs = ec.HIGH_THRESHOLDS[case.name]
    else:
        pairs = [(ec.threshold(case, ref), None)]
    for thr, want in pairs:
        if imp.size < 2 and case.group != "high":
            continue  # (one k or none: any threshold is far from it, or nothing is compared)
        gap, nearest = ec.gap_around(k, g["j_min"], thr)
        assert gap >= 2e-3 and nearest >= 1e-3, (case.name, thr, gap, nearest)
        if want is not None:
            assert ec.first_high(case, k, thr) == want, (case.name, thr)


def test_horizon_geometry():
    """The four-rows-in-flight loop walks rows 1 .. M - 1 behind the window's first row.  M = 5: its first group full (M = 2 .. 4, all
    the older files run, leave it ragged); 6: a second group of one row and three padded ones; 8: two groups minus one row; 9: two
    full groups; 10: a third group.  Forward the last window ends on row n - 1; backward ``last = n - 7`` with M = 9 begins at
    q0 = 2."""
    assert ec.HORIZON_M == (5, 6, 8, 9, 10)
    assert [ec.groups_of_rows(M) for M in ec.HORIZON_M] == [(1, 0), (2, 3), (2, 1), (2, 0), (3, 3)]
    cases = ec.group("horizon")
    assert len(cases) == 3 * len(ec.HORIZON_M) * len(ec.HORIZON_SHAPES)
    for c in cases:
        g = ec.geometry(c)
        assert g["lo"] >= 0 and g["hi"] <= c.n - 1
        if c.mode == "forward":
            assert g["hi"] == c.n - 1
        else:
            assert c.anchor in (c.n, c.n - 7) and g["q0"] == (c.M if c.anchor == c.n else max(0, c.M - 7))
    assert any(c.mode == "backward" and c.M == 9 and ec.geometry(c)["q0"] == 2 and ec.geometry(c)["j_min"] == 0 for c in cases)
    shapes = {(c.dtype, c.s): (ec.route(c.s), ec.loads(c.s, c.dtype)) for c in cases}
    assert shapes == {("f8", 257): ("registers", "element loads"), ("f8", 4100): ("streamed", "16-byte loads"),
                      ("f4", 1028): ("registers", "16-byte loads")}


def test_groups_of_rows():
    assert [ec.groups_of_rows(M) for M in (1, 2, 3, 4)] == [(0, 0), (1, 3), (1, 2), (1, 1)]
    assert {ec.groups_of_rows(c.M)[0] for c in ec.CASES if c.group in ("nan", "route", "batch")} == {1, 2}


def test_route_table_geometry():
    for dtype, s, route, loads in ec.ROUTE_TABLE:
        assert (ec.route(s), ec.loads(s, dtype)) == (route, loads), (dtype, s)
    v4, v8 = ec.vec("f4"), ec.vec("f8")
    assert (v4, v8, ec.batch("f4"), ec.batch("f8")) == (4, 2, 4, 8) and ec.REG_DRAWS == 4096
    assert ec.nq(256, "f4") == 1 and 256 == ec.LANES * v4          # one vector per lane, every lane's full
    assert ec.nq(4096, "f4") == ec.SLOTS // v4 == 16                # all 16 register vectors, full
    assert ec.nq(128, "f8") == 1 and 128 == ec.LANES * v8
    assert ec.nq(4094, "f8") == ec.SLOTS // v8 == 32 and 4094 % (ec.LANES * v8) != 0  # the last vector part full
    assert ec.n3(4094, "f8") == 31 and ec.n3(4095, "f4") == 15      # the last, ragged batch: q0 + u stops at NQ - 1
    assert 40 // v8 == 20 and ec.LANES - 20 == 44                   # fewer draws than lanes: 44 lanes clamp
    assert len(ec.group("route")) == 4 * len(ec.ROUTE_TABLE)


def test_batch_table_geometry():
    for dtype, s, n3, full in ec.BATCH_TABLE:
        assert ec.n3(s, dtype) == n3 and (s % (ec.LANES * ec.vec(dtype)) == 0) == full and ec.route(s) == "registers", (dtype, s)
        assert n3 in (ec.batch(dtype), ec.batch(dtype) + 1)  # on the batch boundary, one past it
    assert ec.n3(1154, "f8") == 9


def test_nan_case_geometry():
    """Nine NaN entries the pass counts -- three draws (draw 0, one inside the lanes' last whole vector, draw S - 1 in the clamped
    vector) in three rows (one only the last step's window reaches, one inside step 0's window that is not the row every step
    counts, one in the middle) -- and one or two just outside what the pass may read."""
    cases = ec.group("nan")
    assert len(cases) == 2 * len(ec.NAN_M) * len(ec.NAN_S)
    for c in cases:
        g = ec.geometry(c)
        ll = ec.matrix(c)
        rows = sorted({r for r, _, _ in c.cells})
        inside = [r for r in rows if g["lo"] <= r <= g["hi"]]
        outside = [r for r in rows if r not in inside]
        assert len(inside) == 3 and all(0 <= r < c.n for r in rows)
        assert outside in ([g["lo"] - 1, g["hi"] + 1], [g["lo"] - 1]) and (len(outside) == 2 or g["hi"] == c.n - 1)
        lo, hi = ec.last_whole_vector(c.s, c.dtype)
        d0, dv, dl = ec.nan_draws(c.s)
        assert d0 == 0 and lo <= dv < hi and dl == c.s - 1 and dl >= ec.n3(c.s, c.dtype) * ec.LANES * ec.vec(c.dtype)
        for r in inside:
            assert list(np.flatnonzero(np.isnan(ll[r]))) == [d0, dv, dl]
            assert len(ec.counting_steps(c, r)) == 1
        owners = sorted(ec.counting_steps(c, r)[0] for r in inside)
        assert owners == [0, ec.NAN_MID, c.n_steps - 1], (c.name, owners)
        # the last step's row is in no other window; step 0's row is not the one step 0 would count as an ordinary step
        windows = [(t, t + c.M) for t in g["t"]]
        only_last = [r for r in inside if [j for j, (a, b) in enumerate(windows) if a <= r < b] == [c.n_steps - 1]]
        assert len(only_last) == 1
        r0 = [r for r in inside if ec.counting_steps(c, r) == [0]][0]
        assert r0 != (g["t0"] + c.M - 1 if c.mode == "forward" else g["t0"])
        assert ec.reference(c)["n_replaced"] == 9
        if c.mode == "forward":
            assert only_last == [c.n - 2] and c.n - 1 in outside  # "row n - 2 is in the last window only", n - 1 in none


def test_non_finite_rows_enter_no_ratio():
    for c in ec.CASES:
        if c.group not in ("inf_mix", "inf_row", "inf_exact"):
            continue
        lo, hi = ec.ratio_rows(c)
        g = ec.geometry(c)
        for r, _, _ in c.cells:
            assert not lo <= r < hi and g["lo"] <= r <= g["hi"], c.name
    for c in ec.group("inf_row") + ec.group("inf_exact"):
        (r, _, v), = c.cells
        assert np.all(ec.matrix(c)[r] == -np.inf)
    assert {ec.geometry(c)["j_min"] for c in ec.group("inf_row") if c.mode == "backward"} == {0, 1}  # an importance step, the exact step
    for c in ec.group("inf_ratio"):
        lo, hi = ec.ratio_rows(c)
        assert all(lo <= r < hi for r, _, _ in c.cells) and np.isfinite(ec.reference(c)["elpd_i"]).all()
    assert {c.s for c in ec.CASES if c.group.startswith("inf")} == {300, 4100} and ec.route(300) != ec.route(4100)


def test_wrap_geometry():
    """n_steps exceeds 8192 x 4 by five: wavefronts 0 .. 4 of the grid take steps 0 .. 4 and then 32768 .. 32772.  One NaN entry is
    counted by a FIRST step of such a wavefront (a count that has to survive the second iteration), two by wrapped steps."""
    cap = ec.PREDICT_GRID * ec.PREDICT_WAVES
    for c in (ec.WRAP_FW, ec.WRAP_BW):
        assert c.n_steps == cap + 5 > cap and c.M == 2 and c.s == 100
        owners = sorted(j for r, _, _ in c.cells for j in ec.counting_steps(c, r))
        assert len(owners) == 3 and owners[0] < 5 and all(j >= cap for j in owners[1:]), owners
        assert ec.reference(c)["n_replaced"] == 3
        g = ec.geometry(c)
        assert g["lo"] >= 0 and g["hi"] == c.n - 1
    assert ec.geometry(ec.WRAP_BW)["q0"] == 1


def test_first_high_thresholds_reach_every_iteration_of_a_thread():
    stride = ec.FIRST_HIGH_THREADS
    for c in (ec.HIGH_FW, ec.HIGH_BW):
        k = ec.reference(c)["diag"]
        j_min = ec.geometry(c)["j_min"]
        answers = [a for _, a in ec.HIGH_THRESHOLDS[c.name]]
        assert c.n_steps == 600 > 2 * stride
        for lo, hi in ec.HIGH_RANGES:
            assert any(lo <= a <= hi for a in answers), (c.name, lo, hi)
        # a later step above the threshold that a lower-numbered thread owns: the minimum over the threads decides, not the order
        assert any(a < c.n_steps and any(k[j] > thr and (j - j_min) % stride < (a - j_min) % stride for j in range(a + 1, c.n_steps))
                   for thr, a in ec.HIGH_THRESHOLDS[c.name])
        # and one the SAME thread meets again in a later iteration (it has to stop at its first)
        assert any(a + stride < c.n_steps and np.any(k[a + stride::stride] > thr) for thr, a in ec.HIGH_THRESHOLDS[c.name])
    assert ec.geometry(ec.HIGH_BW)["q0"] == 2 and 0 in [a for _, a in ec.HIGH_THRESHOLDS["high-bw"]]


def test_block_geometry():
    """PLA_INGEST_BLOCK_MB = 1 holds 31 rows of 4097 f64 ratios: a block is one chunk of 64 steps.  Every NaN row lies in windows
    of steps on both sides of a block boundary, in one mode at least; with M >= 5 a window reaches several rows into the next block."""
    per = ec.block_steps_per_block(1)
    assert per == C and (1 << 20) // (ec.BLOCK_S * 8) == 31 and ec.BLOCK_STEPS > 3 * per
    assert ec.block_steps_per_block(4096) >= ec.BLOCK_STEPS + max(ec.BLOCK_M)  # the default: one block
    ll = ec.block_matrix()
    assert ll.shape == (ec.BLOCK_N, ec.BLOCK_S) and int(np.isnan(ll).sum()) == len(ec.BLOCK_NAN)
    shared = {r: set() for r, _ in ec.BLOCK_NAN}
    for mode, anchor, M in ec.block_cases():
        assert M >= 5
        if mode == "forward":
            assert anchor + ec.BLOCK_STEPS + M - 1 <= ec.BLOCK_N
            t = anchor + np.arange(ec.BLOCK_STEPS)
            blk = np.arange(ec.BLOCK_STEPS) // per
        else:
            t0 = min(anchor, ec.BLOCK_N - M)
            t = t0 - np.arange(ec.BLOCK_STEPS)
            assert t[-1] >= 0
            blk = (anchor - t) // per  # (blocks are chunks of q = last - t)
        for r in shared:
            blocks = {int(b) for tj, b in zip(t, blk) if tj <= r < tj + M}
            if len(blocks) > 1:
                shared[r].add(mode)
    assert all(shared.values()), shared
    assert {m for v in shared.values() for m in v} == {"forward", "backward"}
