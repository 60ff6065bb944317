"""The leave-future-out kernels (csrc/pla_lfo.h, csrc/pla_lfo_bw.h) at the horizons, draw counts, non-finite inputs and launch sizes
where their loops change shape, in both modes through ``Engine.lfo(..., mode=...)``.  The inputs are the table of
tests/lfo_edge_cases.py; tests/test_lfo_edges_host.py proves on the CPU reference alone that they are fit for the comparison
(finite k, no tie inside a Pareto tail, thresholds in a gap) and that each case has the geometry it is named after.

k and elpd_i against tests/lfo_ref.py / tests/lfo_bw_ref.py on the CPU oracle at the parity tolerances of tests/test_gpu_parity.py;
the NaN pattern of elpd_i, the +inf pattern of k, ``n_replaced`` and ``first_high`` exactly; the four sources of one matrix
(device draws fastest, the same with an odd pitch, device observations fastest, host) bit for bit with one another; and after
every call ``Engine.last_kernels()`` has to name the route and the load width the case is aimed at.

==========================================================================  =====================================================
structure                                                                   test
==========================================================================  =====================================================
lfo_future / lfo_bw_future: rows 1 .. M - 1 four at a time, a row past the  test_horizon: M = 5, 6, 8, 9, 10 on the element-load
window loaded again from row M - 1, neither added nor counted; the `m`      register route, the streamed route and f32; forward
loop of the register route                                                  to row n - 1, backward from last = n and n - 7
<T, VEC, REG>: f32 / f64 x element / 16-byte loads x registers / streamed;  test_route_dtype_and_load_width: ROUTE_TABLE with M = 3
one vector per lane, all register vectors full, fewer draws than lanes      and 6
the register route's batches of 8 (f64) / 4 (f32) whole vectors, padded     test_batch_edges: n3 = 8, 8 (full last vector), 9 and
slots repeating the last whole vector                                       4, 4, 5; test_route_...: n3 = 31 and 15 (ragged batch)
NaN entries counted once each: the last (first) row of every window, the    test_nan_accounting: draw 0, a draw of the lanes' last
whole window of step 0; not by padded rows, padded slots, clamped lanes     whole vector, draw S - 1, in three rows; NaN outside
+-inf future terms; a step no draw of which has a finite a = lw + f         test_non_finite_future_terms, test_routes_agree_...
the predict grid's cap of 8192 x 4 wavefronts, n_nan carried over `j += nw` test_predict_grid_wrap: 32773 steps
first_high: 256 threads stride over the steps and stop at their first hit   test_first_high_beyond_one_stride: 600 steps
blocks of whole chunks; a staged block carries nb + M - 1 rows              test_block_hand_over_with_a_long_window (children)
==========================================================================  =====================================================

Not covered here: the scan kernels' own grid-stride loops begin a second round at more than 2^22 (chunk, draw-block) units -- 2^28
rows of ratios at the least, far beyond a test of a few seconds; views past 2^31 elements are tests/test_gpu_far_offsets.py's.
"""

import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lfo_edge_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-9, 1e-10  # tests/test_gpu_parity.py
ROUTE = re.compile(r"lfo_(bw_)?predict_kernel<(\w+), (16-byte loads|element loads), (registers|streamed)>")
KEYS = ("diag", "elpd_i", "first_high", "n_replaced")


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def scalar(x):
    return int(host(x).reshape(-1)[0])


def cuda(a):
    import torch

    return torch.as_tensor(np.array(a, order="C")).cuda()  # (a copy: the case table's matrices are read-only)


def sources(ll):
    """Device draws fastest, the same with an odd pitch (rows that are not 16-byte aligned: element loads), device observations
    fastest (transposed block by block), host."""
    import torch

    draws = cuda(ll)
    wide = torch.zeros((ll.shape[0], ll.shape[1] + 3), dtype=draws.dtype, device="cuda")
    wide[:, :ll.shape[1]] = draws
    return {"draws": draws, "pitch": wide[:, :ll.shape[1]], "obs": cuda(ll.T).T, "host": ll}


def show(what, got, want):
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    d = d[np.isfinite(d)]
    print(f"{what}: max |dev| = {d.max() if d.size else 0.0:.3e}")


def call(eng, case, src, thr, key):
    """One pass; the route text has to name the case's mode, dtype, route and the source's load width."""
    res = eng.lfo(src, case.anchor, case.n_steps, case.M, ec.tail(case), thr, mode=case.mode)
    text = eng.last_kernels()
    m = ROUTE.search(text)
    assert m, text
    want = (case.mode == "backward", "double" if case.dtype == "f8" else "float",
            "element loads" if key == "pitch" else ec.loads(case.s, case.dtype), ec.route(case.s))
    assert (m.group(1) is not None, m.group(2), m.group(3), m.group(4)) == want, (case.name, key, text)
    return [host(res["diag"]), host(res["elpd_i"]), scalar(res["first_high"]), scalar(res["n_replaced"])]


def check(case, out, thr, what):
    ref = ec.reference(case)
    k, elpd, high, n_rep = out
    k_ref, e_ref = ref["diag"], ref["elpd_i"]
    show(f"{what} k", k, k_ref)
    show(f"{what} elpd", elpd, e_ref)
    assert k.shape == elpd.shape == (case.n_steps,)
    assert np.array_equal(np.isinf(k), np.isinf(k_ref)) and np.all(k[np.isinf(k)] > 0), what
    fin = np.isfinite(k_ref)
    np.testing.assert_allclose(k[fin], k_ref[fin], rtol=RTOL, atol=ATOL, err_msg=what)
    assert (k[0] == 0.0) == (ec.geometry(case)["j_min"] == 1), what  # (exact: the fit's own step, and only that)
    nan = np.isnan(e_ref)
    assert np.array_equal(np.isnan(elpd), nan), (what, "NaN at", np.flatnonzero(np.isnan(elpd)), "reference", np.flatnonzero(nan), elpd[nan])
    np.testing.assert_allclose(elpd[~nan], e_ref[~nan], rtol=RTOL, atol=ATOL, err_msg=what)
    assert high == ec.first_high(case, k_ref, thr) == ec.first_high(case, k, thr), what
    assert n_rep == ref["n_replaced"], (what, n_rep, ref["n_replaced"])


def run_case(eng, case):
    """Every source against the reference, and the sources bit for bit with one another."""
    thr = ec.threshold(case)
    outs = {}
    for key, src in sources(ec.matrix(case)).items():
        outs[key] = call(eng, case, src, thr, key)
        check(case, outs[key], thr, f"{case.name} {key}")
    for key, out in outs.items():
        for a, b in zip(out, outs["draws"]):
            assert np.array_equal(a, b, equal_nan=True), (case.name, key)
    return outs["draws"]


def ids(cases):
    return [c.name for c in cases]


# ----------------------------------------------------------------------------------------------------------------- 1. the shapes
@pytest.mark.parametrize("case", ec.group("horizon"), ids=ids(ec.group("horizon")))
def test_horizon(eng, case):
    run_case(eng, case)


@pytest.mark.parametrize("case", ec.group("route"), ids=ids(ec.group("route")))
def test_route_dtype_and_load_width(eng, case):
    run_case(eng, case)


@pytest.mark.parametrize("case", ec.group("batch"), ids=ids(ec.group("batch")))
def test_batch_edges(eng, case):
    run_case(eng, case)


# -------------------------------------------------------------------------------------------------------- 2. non-finite entries
@pytest.mark.parametrize("case", ec.group("nan"), ids=ids(ec.group("nan")))
def test_nan_accounting(eng, case):
    """Nine NaN entries inside what the pass reads and one or two just outside: each counted once, by every source."""
    assert ec.reference(case)["n_replaced"] == 9
    run_case(eng, case)


INF_CASES = [c for c in ec.CASES if c.group.startswith("inf")]


@pytest.mark.parametrize("case", INF_CASES, ids=ids(INF_CASES))
def test_non_finite_future_terms(eng, case):
    """(i) -inf on every third draw and one +inf: NaN where the reference's is; (ii), (iii) a step every draw of which has
    a = lw + f = -inf (an observation of likelihood 0 under every draw) gives NaN on both routes, as the reference's
    logsumexp does; (iv) two -inf entries in a ratio row: the draws drop out, the pass stays at parity."""
    run_case(eng, case)


def test_routes_agree_on_non_finite_steps(eng):
    """The same non-finite entries at S = 300 (registers) and S = 4100 (streamed): NaN at the same steps."""
    pattern = {}
    for case in INF_CASES:
        res = eng.lfo(cuda(ec.matrix(case)), case.anchor, case.n_steps, case.M, ec.tail(case), 0.7, mode=case.mode)
        assert ec.route(case.s) in eng.last_kernels()
        pattern.setdefault(case.name.replace(f"-S{case.s}-", "-"), {})[ec.route(case.s)] = np.flatnonzero(np.isnan(host(res["elpd_i"]))).tolist()
    assert len(pattern) == len(INF_CASES) // 2
    for name, by_route in pattern.items():
        assert sorted(by_route) == ["registers", "streamed"] and by_route["registers"] == by_route["streamed"], (name, by_route)


# ------------------------------------------------------------------------------------------------------------ 3. launch edges
@pytest.mark.parametrize("case", [ec.WRAP_FW, ec.WRAP_BW], ids=["forward", "backward"])
def test_predict_grid_wrap(eng, case):
    """32773 steps, a wavefront per step, at most 8192 x 4 wavefronts: five take a second step.  Every step against the reference
    (computed once), the device matrix read in place; one NaN entry is counted by such a wavefront's first step, two by wrapped steps."""
    assert case.n_steps > ec.PREDICT_GRID * ec.PREDICT_WAVES
    thr = ec.threshold(case)
    out = call(eng, case, cuda(ec.matrix(case)), thr, "draws")
    assert "per block of steps" in eng.last_kernels() and "transpose" not in eng.last_kernels()
    check(case, out, thr, case.name)
    assert out[3] == 3


@pytest.mark.parametrize("case", [ec.HIGH_FW, ec.HIGH_BW], ids=["forward", "backward"])
def test_first_high_beyond_one_stride(eng, case):
    """600 steps for 256 threads: answers in a thread's first, second and third iteration and none, with later steps above the
    threshold in the same thread and in lower-numbered ones; backward with q0 = 2 also the answer 0."""
    srcs = sources(ec.matrix(case))
    answers = []
    for thr, want in ec.HIGH_THRESHOLDS[case.name]:
        out = call(eng, case, srcs["draws"], thr, "draws")
        check(case, out, thr, f"{case.name} thr={thr}")
        assert out[2] == want, (thr, out[2], want)
        answers.append(out[2])
        assert scalar(eng.lfo(srcs["host"], case.anchor, case.n_steps, case.M, ec.tail(case), thr, mode=case.mode)["first_high"]) == want
    for lo, hi in ec.HIGH_RANGES:
        assert any(lo <= a <= hi for a in answers)
    assert (0 in answers) == (case.mode == "backward")


# ------------------------------------------------------------------------------------------------------------ 4. block hand-over
CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import lfo_edge_cases as ec
from pyloo_amd.engine import get_engine
eng = get_engine(0)
ll = ec.block_matrix()
out = []
for mode, anchor, M in ec.block_cases():
    for t in (torch.as_tensor(ll).cuda(), torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T):
        r = eng.lfo(t, anchor, ec.BLOCK_STEPS, M, 193, 0.7, mode=mode)
        out += [r[k].cpu().numpy().reshape(-1) for k in ("diag", "elpd_i", "first_high", "n_replaced")]
np.savez(sys.argv[2], *out)
"""


def test_block_hand_over_with_a_long_window(tmp_path):
    """S = 4097 with 200 steps under PLA_INGEST_BLOCK_MB=1: blocks of one chunk of 64 steps, and with M = 6 and 9 the windows of
    a block's last steps reach up to eight rows into the next block's rows (forward; backward into the previous block's), so a
    staged block carries nb + M - 1 rows.  NaN entries lie in rows that the windows on both sides of a boundary share.  Every
    output is the default's (one block) bit for bit, both modes, both device layouts, and the layouts agree with one another."""
    outs = []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        env.update(env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            outs.append([z[k] for k in sorted(z.files, key=lambda s: int(s.split("_")[1]))])
    cases = ec.block_cases()
    assert len(outs[0]) == len(outs[1]) == len(cases) * 2 * len(KEYS)
    for i, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(a, b, equal_nan=True), (cases[i // (2 * len(KEYS))], KEYS[i % len(KEYS)])
    nan_rows = [r for r, _ in ec.BLOCK_NAN]
    for c, (mode, anchor, M) in enumerate(cases):
        base = c * 2 * len(KEYS)
        for j in range(len(KEYS)):  # the two layouts among each other
            assert np.array_equal(outs[1][base + j], outs[1][base + len(KEYS) + j], equal_nan=True), (mode, M, KEYS[j])
        if mode == "forward":
            lo, hi = anchor, anchor + ec.BLOCK_STEPS + M - 2
        else:
            t0 = min(anchor, ec.BLOCK_N - M)
            lo, hi = t0 - ec.BLOCK_STEPS + 1, t0 + M - 1
        assert int(outs[1][base + 3][0]) == sum(lo <= r <= hi for r in nan_rows) == len(nan_rows), (mode, M)
        assert np.isfinite(outs[1][base + 1]).all()
