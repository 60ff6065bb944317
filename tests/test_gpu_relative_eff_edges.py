"""Relative MCMC efficiency on the GPU at the internal strides of csrc/pla_ess.h and of ``pla_relative_eff``.  Every value is
compared with the NumPy restatement (tests/ess_ref.py) at the parity tolerances of tests/test_gpu_parity.py, through the ``close``
rule of tests/test_gpu_relative_eff.py; the matrices have 3, 5 or 15 rows, so that rule leaves no row out, and every test
asserts that no deciding margin is below ``ess_ref.MARGIN_FLOOR``.  Grids, layouts, blocks and a frozen engine bit for bit.

Which structure each group of shapes (``ess_ref.EDGE_SHAPES`` and the two loop-end tables) is aimed at:

=====================================================================  ===========================================================
structure                                                              shapes (chains, draws per chain)
=====================================================================  ===========================================================
lane l owns draws l, l + 64, ... of a chain (kWave)                    "wave": n = 63 / 64 / 65 at C = 1 and 3
the sweeps (ess_lag, ess_finish) issue kEssBatch x 64 = 512 draws a    "sweep": n = 511 / 512 / 513 at C = 1 and 2; (1, 1023),
step; a slot past the end adds fma(0, 0, acc)                          (1, 1025), (2, 1027) split into halves of 511 / 512 / 513
ess_load takes kEssLoadBatch x 64 = 1024 draws a step (split rows,     "load": (1, 2050) split: n = 1025; (2, 2049) split: n = 1024,
the long route)                                                        the middle draw skipped; (3, 1366) on the long route
ess_fetch / ess_commit hold the row in 64 register slots; a slot       "limit": C n = 4096 at (8, 512) (64, 64) (1024, 4); 4095 at
past the end re-reads the last draw                                    (3, 1365) (7, 585); 4098 / 4097 / 4100 just above the limit
the route is chosen from the ANALYSED draws                            "route": (2, 2049) long unsplit, on chip split; (1, 4098)
                                                                       and (1, 8192) long both ways
the Geyer loop runs t < n - 1, a pair of lags per sweep                "tiny": n = 5 .. 11 and halves of 4 / 5 draws; UNMIXED_SHAPES
                                                                       (rows that run every lag, odd and even n)
tau = max(tau, 1 / log10(C n))                                         ALTERNATING_SHAPES (rows that reach the floor)
a workgroup takes several rows and fetches the next one ahead;         test_invalid_rows_inside_a_workgroup: set_ess_grid 1, 2, 3
n_bad is added once per workgroup                                      over seven rows, three of them invalid
pla_relative_eff loops over blocks of observations-fastest device      test_block_size_independence (PLA_INGEST_BLOCK_MB = 1 in a
input: d_out + r0, one counter for all blocks, d_in reused             child process)
d_ess / d_in are grown on demand                                       test_frozen_engine
=====================================================================  ===========================================================
"""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ess_ref
from test_gpu_relative_eff import ATOL, DTYPES, RTOL, close, cuda, device_layouts, host, scalar, show

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_CASES = []  # (group, chains, draws): each shape once, under the first group that names it
for _group, _shapes in ess_ref.EDGE_SHAPES.items():
    EDGE_CASES += [(_group, c, n) for c, n in _shapes if (c, n) not in [k[1:] for k in EDGE_CASES]]


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    e = get_engine(0)
    yield e
    e.set_ess_grid(0)


def analysed_draws(n_chains, n, split):
    return n_chains * (2 * (n // 2) if split else n)


def splits(n):
    return (False, True) if n // 2 >= 4 else (False,)


@functools.lru_cache(maxsize=None)
def reference(family, n_chains, n, log, dtype, split):
    """(matrix, raw r_eff, margin, stop) of one case, computed once: family "parity" (parity_matrix's rows), "unmixed" or
    "alternating"."""
    if family == "parity":
        mat = ess_ref.parity_matrix(n_chains, n, log, DTYPES[dtype])
    else:
        mat = ess_ref.loop_end_matrix(family, n_chains, n, log, DTYPES[dtype])
    r, margin, stop = ess_ref.relative_eff(mat, n_chains, log, split, cap=False)
    for a in (mat, r, margin, stop):
        a.setflags(write=False)
    return mat, r, margin, stop


def check_case(eng, family, n_chains, n, log, dtype, split):
    """Values through close(), the route text, n_invalid == 0 and the cap bit for bit; returns (raw, capped, reference tuple)."""
    ref = reference(family, n_chains, n, log, dtype, split)
    mat, want, margin, _ = ref
    assert margin.min() >= ess_ref.MARGIN_FLOOR, (family, n_chains, n, log, dtype, split, margin.min())
    what = f"{family} {n_chains}x{n} {dtype} log={log} split={split}"
    t = cuda(mat)
    raw = eng.relative_eff(t, n_chains, log=log, split=split, cap=False)
    assert ("LDS" in eng.last_kernels()) == (analysed_draws(n_chains, n, split) <= eng.ess_lds_max_draws()), (what, eng.last_kernels())
    got = host(raw["r_eff"])
    assert got.dtype == np.float64 and got.shape == (mat.shape[0],) and scalar(raw["n_invalid"]) == 0, what
    close(got, want, margin, what)
    capped = host(eng.relative_eff(t, n_chains, log=log, split=split, cap=True)["r_eff"])
    assert np.array_equal(capped, np.minimum(got, 1.0)), what
    return got, capped, ref


# ------------------------------------------------------------------------------------------------ 1. parity at the kernel's strides
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("group,n_chains,n", EDGE_CASES, ids=[f"{g}-{c}x{n}" for g, c, n in EDGE_CASES])
def test_parity_at_the_strides(eng, group, n_chains, n, dtype):
    assert eng.ess_lds_max_draws() == 4096
    assert (n_chains, n) in ess_ref.EDGE_SHAPES[group]
    for log in (True, False):
        for split in splits(n):
            got, _, (mat, _, _, _) = check_case(eng, "parity", n_chains, n, log, dtype, split)
            assert mat.shape[0] == (15 if n_chains * n <= 4000 else 5) and np.isfinite(got).all()


def test_the_route_flips_with_the_split_flag(eng):
    """(2, 2049): 4098 analysed draws unsplit take the long route, 4 x 1024 = 4096 split stay on chip -- the shape of the matrix
    in memory is the same.  (1, 4098) and (1, 8192) are long both ways (the routes themselves are asserted per parity case)."""
    limit = eng.ess_lds_max_draws()
    assert analysed_draws(2, 2049, False) == limit + 2 and analysed_draws(2, 2049, True) == limit
    assert analysed_draws(1, 4098, True) == limit + 2 and analysed_draws(1, 8192, True) == 2 * limit
    t = cuda(reference("parity", 2, 2049, True, "f64", False)[0])
    eng.relative_eff(t, 2, split=False)
    assert "global workspace" in eng.last_kernels() and "LDS" not in eng.last_kernels()
    eng.relative_eff(t, 2, split=True)
    assert "LDS" in eng.last_kernels() and "global workspace" not in eng.last_kernels()


# ----------------------------------------------------------------------------------------------------------- 2. the loop's two ends
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n_chains,n", ess_ref.UNMIXED_SHAPES)
def test_unmixed_rows_run_every_lag(eng, n_chains, n, dtype):
    for log in (True, False):
        for split in splits(n):
            na = n // 2 if split else n
            stop = reference("unmixed", n_chains, n, log, dtype, split)[3]
            assert (stop == (na if na % 2 == 0 else na - 1)).all(), (n_chains, n, log, split, stop)  # (the last lag the rule allows)
            got, _, _ = check_case(eng, "unmixed", n_chains, n, log, dtype, split)
            assert np.isfinite(got).all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n_chains,n", ess_ref.ALTERNATING_SHAPES)
def test_alternating_rows_reach_the_floor_of_tau(eng, n_chains, n, dtype):
    for log in (True, False):
        for split in splits(n):
            cn = analysed_draws(n_chains, n, split)
            want = reference("alternating", n_chains, n, log, dtype, split)[1]
            np.testing.assert_allclose(want, np.log10(cn), rtol=0, atol=1e-12)
            got, capped, _ = check_case(eng, "alternating", n_chains, n, log, dtype, split)
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
            if cn > 10:
                assert (capped == 1.0).all(), (n_chains, n, log, split, capped)


# ------------------------------------------------------------------------ 3. one workgroup, several rows, invalid rows among them
@pytest.mark.parametrize("n_chains,n,split", [(4, 250, False), (2, 33, True), (1, 4100, False)])
def test_invalid_rows_inside_a_workgroup(eng, n_chains, n, split):
    """On chip with the next row fetched ahead, on chip with rows read straight into LDS, and the long route.  With a grid of 1, 2
    or 3 workgroups over seven rows a workgroup meets invalid rows between valid ones (grid 3: one workgroup takes rows 0, 3, 6 --
    nothing but invalid rows -- and adds its count once).  A row's result depends on the row alone."""
    rng = np.random.default_rng(600 + n)
    mat = np.concatenate([ess_ref.ar1_rows(rng, 4, n_chains, n, 0.0), ess_ref.ar1_rows(rng, 3, n_chains, n, 0.9)])[[0, 4, 1, 5, 2, 6, 3]]
    # the entries that make a row invalid lie where a neighbour's read could stray: the draw just before row 1, a constant above
    # every maximum of rows 2 and 4, and the draw just behind row 5 (a register slot past the end of a row must not look there)
    mat[0, n_chains * n - 1] = np.nan
    mat[3] = 0.5
    mat[6, 0] = np.inf
    assert mat[[1, 2, 4, 5]].max() < 0.5
    valid, invalid = [1, 2, 4, 5], [0, 3, 6]
    want, margin, _ = ess_ref.relative_eff(mat, n_chains, split=split, cap=False)
    assert np.isnan(want[invalid]).all() and margin[valid].min() >= ess_ref.MARGIN_FLOOR
    alone = {i: host(eng.relative_eff(cuda(mat[i:i + 1]), n_chains, split=split, cap=False)["r_eff"])[0] for i in valid}
    layouts = device_layouts(mat)
    try:
        eng.set_ess_grid(0)
        base = host(eng.relative_eff(layouts["draws"], n_chains, split=split, cap=False)["r_eff"])
        np.testing.assert_allclose(base[valid], want[valid], rtol=RTOL, atol=ATOL)
        for grid in (0, 1, 2, 3):
            eng.set_ess_grid(grid)
            for name in ("draws", "obs"):
                for repeat in range(2):  # (the counter starts from zero in every call: 3 again, not 6)
                    res = eng.relative_eff(layouts[name], n_chains, split=split, cap=False)
                    got = host(res["r_eff"])
                    what = (n_chains, n, split, grid, name, repeat)
                    assert ("transpose_rows_kernel" in eng.last_kernels()) == (name == "obs"), what
                    assert np.isnan(got[invalid]).all() and scalar(res["n_invalid"]) == 3, (what, got, scalar(res["n_invalid"]))
                    for i in valid:
                        assert got[i] == base[i] and got[i] == alone[i], (what, i, got[i], base[i], alone[i])
    finally:
        eng.set_ess_grid(0)


# ------------------------------------------------------------------------- 4. layouts and memory spaces at the new shapes, bit for bit
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n_chains,n,split", [(8, 512, False), (2, 2049, True), (2, 2049, False), (3, 1366, False), (3, 1365, False)])
def test_layouts_and_memory_spaces_give_the_same_bits(eng, n_chains, n, split, dtype):
    """(At (3, 1365) the last register slot of a lane lies past the row: behind it is the next row, staging, or the zeros of the
    odd pitch, which are above every maximum of a log row.)"""
    mat = reference("parity", n_chains, n, True, dtype, split)[0]
    first = host(eng.relative_eff(cuda(mat), n_chains, split=split, cap=False)["r_eff"])
    assert np.isfinite(first).all()
    for name, t in device_layouts(mat).items():
        got = host(eng.relative_eff(t, n_chains, split=split, cap=False)["r_eff"])
        assert np.array_equal(got, first), name
        assert ("transpose_rows_kernel" in eng.last_kernels()) == (name == "obs"), eng.last_kernels()
    for name, a in (("host", mat), ("host obs-fastest", np.ascontiguousarray(mat.T).T)):
        res = eng.relative_eff(a, n_chains, split=split, cap=False)
        assert isinstance(res["r_eff"], np.ndarray) and res["n_invalid"] == 0
        assert np.array_equal(res["r_eff"], first), name


# --------------------------------------------------------------------------------------------------------- 5. block-size independence
CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import ess_ref
from pyloo_amd.engine import get_engine
eng = get_engine(0)
eng.set_timing(True)
out = []
# (rows, chains, draws, dtype, invalid rows: in the first and the last block and on both sides of a block boundary, split too?)
CASES = ((300, 4, 250, np.float64, (5, 130, 131, 299), True),
         (300, 4, 250, np.float32, (5, 261, 262, 299), False),
         (70, 1, 4100, np.float64, (2, 30, 31, 61, 62, 69), False))
for rows, C, n, dtype, bad, with_split in CASES:
    for log in (True, False):
        rng = np.random.default_rng(900 + rows + n + (5 if log else 0))
        mat = np.concatenate([ess_ref.ar1_rows(rng, rows // 2, C, n, phi, log) for phi in (0.0, 0.9)]).astype(dtype)
        for k, i in enumerate(bad):
            if k % 3 == 0:
                mat[i, 7 * k + 1] = np.nan
            elif k % 3 == 1:
                mat[i] = mat[i, 0]
            else:
                mat[i, C * n - 1] = np.inf
        obs = torch.as_tensor(np.ascontiguousarray(mat.T)).cuda().T
        draws = torch.as_tensor(mat).cuda()
        for split in ((False, True) if with_split else (False,)):
            eng.kernel_ms()
            r = eng.relative_eff(obs, C, log=log, split=split, cap=False)
            launches = eng.kernel_ms()[1]
            assert "transpose_rows_kernel" in eng.last_kernels(), eng.last_kernels()
            eng.kernel_ms()
            d = eng.relative_eff(draws, C, log=log, split=split, cap=False)
            assert eng.kernel_ms()[1] == 1 and "transpose_rows_kernel" not in eng.last_kernels()
            out += [r["r_eff"].cpu().numpy(), r["n_invalid"].cpu().numpy(), np.array([launches]),
                    d["r_eff"].cpu().numpy(), d["n_invalid"].cpu().numpy(), np.array(sorted(bad))]
np.savez(sys.argv[2], *out)
"""


def test_block_size_independence(tmp_path):
    """PLA_INGEST_BLOCK_MB=1 cuts the observations-fastest device matrices into blocks: 300 x (4, 250) f64 (8000 bytes a row) into
    131 + 131 + 38 rows, the same as f32 into 262 + 38, 70 x (1, 4100) f64 (32 800 bytes a row, the long route) into 31 + 31 + 8;
    invalid rows lie in the first and the last block and on both sides of a block boundary.  The timed launches -- one per block --
    prove that the variable reached the plan.  r_eff (NaN pattern included) and n_invalid are the default's (one block) bit for
    bit, and both equal the draws-fastest call on the same values, which runs in place in one launch.

    Host matrices are staged in fixed 1 GiB blocks that the variable does not change: a host case of more than one block would
    need a matrix of gigabytes at an O(C n^2) cost per row, and is out of scope here."""
    outs = []
    for i, env_extra in enumerate(({}, {"PLA_INGEST_BLOCK_MB": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        env.update(env_extra)
        path = tmp_path / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            outs.append([z[k] for k in sorted(z.files, key=lambda s: int(s.split("_")[1]))])
    # calls in the child's order: f64 (log, not) x (unsplit, split); f32 (log, not); long (log, not)
    blocks = [3, 3, 3, 3, 2, 2, 3, 3]
    assert len(outs[0]) == len(outs[1]) == 6 * len(blocks)
    for j, want_blocks in enumerate(blocks):
        one = dict(zip(("obs", "obs_bad", "launches", "draws", "draws_bad", "bad"), outs[0][6 * j:6 * j + 6]))
        cut = dict(zip(("obs", "obs_bad", "launches", "draws", "draws_bad", "bad"), outs[1][6 * j:6 * j + 6]))
        assert int(one["launches"][0]) == 1 and int(cut["launches"][0]) == want_blocks, (j, one["launches"], cut["launches"])
        bad = one["bad"]
        assert np.array_equal(np.flatnonzero(np.isnan(one["draws"])), bad), j
        assert int(one["draws_bad"].reshape(-1)[0]) == bad.size, j
        for name, r, count in (("one block", one["obs"], one["obs_bad"]), ("blocks", cut["obs"], cut["obs_bad"]),
                               ("draws fastest, blocks set", cut["draws"], cut["draws_bad"])):
            assert np.array_equal(r, one["draws"], equal_nan=True), (j, name, np.flatnonzero(r != one["draws"]))
            assert int(count.reshape(-1)[0]) == bad.size, (j, name, count)


# ------------------------------------------------------------------------------------------------------------------ 6. frozen engine
def test_frozen_engine():
    import torch

    from pyloo_amd._capi import EngineError
    from pyloo_amd.engine import Engine

    own = Engine(0)
    try:
        rng = np.random.default_rng(70)
        short = ess_ref.ar1_rows(rng, 40, 4, 250, 0.5)
        long = ess_ref.ar1_rows(rng, 3, 1, 4100, 0.5)
        calls = ((cuda(short), 4), (cuda(short.T).T, 4), (cuda(long), 1))
        warm = [host(own.relative_eff(t, c, cap=False)["r_eff"]) for t, c in calls]
        assert all(np.isfinite(w).all() for w in warm) and np.array_equal(warm[0], warm[1])
        torch.cuda.synchronize()
        own.set_frozen(True)
        again = [host(own.relative_eff(t, c, cap=False)["r_eff"]) for t, c in calls]
        assert all(np.array_equal(a, w) for a, w in zip(again, warm))
        big = cuda(ess_ref.ar1_rows(np.random.default_rng(71), 600, 1, 4100, 0.0))  # (512 workspace slots where three were warm)
        with pytest.raises(EngineError) as err:
            own.relative_eff(big, 1)
        assert err.value.code == -6
        assert np.array_equal(host(own.relative_eff(calls[0][0], 4, cap=False)["r_eff"]), warm[0])
        torch.cuda.synchronize()
    finally:
        own.set_frozen(False)
        own.close()


# ------------------------------------------------------------------------------------------- 7. the boundary of the argument check
def test_split_needs_four_draws_a_half_chain(eng):
    from pyloo_amd._capi import EngineError

    mat = ess_ref.parity_matrix(1, 7, True)
    with pytest.raises(EngineError) as err:
        eng.relative_eff(cuda(mat), 1, split=True)  # (three draws a half chain)
    assert err.value.code == -1 and "at least 4" in str(err.value)
    res = eng.relative_eff(cuda(ess_ref.parity_matrix(1, 8, True)), 1, split=True)  # (four: accepted; the values are in section 1)
    assert np.isfinite(host(res["r_eff"])).all() and scalar(res["n_invalid"]) == 0
    show("(1, 7) unsplit", host(eng.relative_eff(cuda(mat), 1, cap=False)["r_eff"]), ess_ref.relative_eff(mat, 1, cap=False)[0])
