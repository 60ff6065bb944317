"""``group_sum_kernel`` (csrc/pla_group.h) at the member counts, draw counts, block boundaries and index lists where its branches
change.  Every value is compared bit for bit with the member-by-member NumPy sums of tests/group_gather_ref.py, every NaN count
exactly, and ``Engine.last_kernels()`` has to name the vector leg the case is aimed at.  No tolerances.

=====================================================================  ===========================================================
branch                                                                 test
=====================================================================  ===========================================================
the two-batches-in-flight loop (kGroupBatch = 8) on the fresh path:    test_batch_edges: one group of each size 1..34, 64, 65, 129
the seed, x alone, x and y, the element tail behind them               (contiguous and scattered rows), NaN in the seed, at both
                                                                       ends of a batch and in the last member, inf + -inf
a lane owns VEC draws, a wave 64 vectors, a workgroup 256; VEC = 1     test_batch_edges: S around 64 and 256 vectors for VEC = 2
when S % VEC != 0; rows shorter than a wave                            (f64) and 4 (f32), S % VEC != 0, S = 2 and 6
VEC from the base address, the pitch and S of a matrix read in place   test_vector_legs_in_place: pitched views (the pad is NaN: a
                                                                       read past the row would be counted), a base 8 / 4 bytes off
P.blocked: lower bound per group and block, `cont`, acc read back      test_blocked_path: block_edge_index over blocks of 32 / 64
from `out`, lo == hi on a started group, groups that start later,      rows and a ragged one, PLA_INGEST_BLOCK_MB unset and 1 in
end on a block's last row, lie in the ragged block; empty groups       child processes, against the plain reference; then
zeroed in the first block only; blocks of groups in psis_loo_groups    psis_loo_groups over three blocks of groups
the clamps of device lists: offsets, members, the row in the block     test_device_lists_are_clamped (in place), test_blocked_path
                                                                       (ascending list, blocked); host lists refused
=====================================================================  ===========================================================
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import group_gather_ref as ref
from test_group_gather_ref_host import BATCH_EDGE_DRAWS, N_BATCH, N_BLOCK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = {np.float64: 2, np.float32: 4}
WIDE, ELEMENT = "16-byte loads", "element loads"
IN_PLACE = "group_sum_kernel (matrix read in place; %s)"
ROUTES = {"host": "group_sum_kernel (blocks of observations uploaded; %s)", "draws": IN_PLACE,
          "obs": "transpose_rows_kernel + group_sum_kernel (blocks of observations; %s)"}


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


def wrap(index, device=None):
    """A GroupIndex of hand-built lists (``group_index`` never gives empty groups or lists out of range)."""
    import pyloo_amd as pl

    off, mem = (np.asarray(a, dtype=np.int64) for a in index)
    return pl.GroupIndex(np.arange(len(off) - 1), off, mem).to(device)


def sources(ll):
    import torch

    return {"host": ll, "draws": torch.as_tensor(ll).cuda(), "obs": torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T}


def run(eng, src, index):
    """(sums, NaN count, route text) of one group_sum call, on the host"""
    device = src.device if hasattr(src, "is_cuda") else None
    sums, nrep = eng.group_sum(src, wrap(index, device))
    text = eng.last_kernels()
    if device is None:
        return sums, nrep, text
    return sums.cpu().numpy(), int(nrep.item()), text


def same(got, want):
    """Bit for bit, NaN (of inf + -inf) only where the reference has it"""
    nan = np.isnan(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


# ---------------------------------------------------------------------------------------------------- batch edges, in place
@pytest.mark.parametrize("dt,S", [(dt, S) for dt, draws in BATCH_EDGE_DRAWS.items() for S in draws],
                         ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_batch_edges(eng, dt, S):
    leg = WIDE if S % VEC[dt] == 0 else ELEMENT
    for kind in ("contiguous", "scattered"):
        index = ref.batch_edge_index(N_BATCH, kind)
        ll = ref.batch_edge_matrix(N_BATCH, S, dt, index)
        want, n_nan = ref.group_sums(ll, *index)
        nan = np.isnan(want)
        assert n_nan >= 6 and nan.any() and not nan[:, :S - 1].any()  # NaN sums in the inf + -inf draw and only there
        for name, src in sources(ll).items():
            got, nrep, text = run(eng, src, index)
            assert text == ROUTES[name] % leg, (kind, name, text)
            assert same(got, want), (kind, name, np.argwhere(got != want)[:5])
            assert not np.isnan(got[:, :S - 1]).any() and nrep == n_nan, (kind, name, nrep, n_nan)


# ---------------------------------------------------------------------------------------------------- vector legs in place
#            dtype, S, pitch (0: contiguous, the base one element off), leg
VIEW_CASES = [(np.float64, 130, 132, WIDE), (np.float64, 130, 133, ELEMENT), (np.float64, 129, 132, ELEMENT),
              (np.float32, 260, 264, WIDE), (np.float32, 260, 262, ELEMENT), (np.float64, 130, 0, ELEMENT), (np.float32, 260, 0, ELEMENT)]


@pytest.mark.parametrize("dt,S,pitch,leg", VIEW_CASES, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_vector_legs_in_place(eng, dt, S, pitch, leg):
    import torch

    index = ref.batch_edge_index(N_BATCH, "scattered")
    ll = ref.batch_edge_matrix(N_BATCH, S, dt, index)
    want, n_nan = ref.group_sums(ll, *index)
    dense = torch.as_tensor(ll).cuda()
    base, base_nrep, base_text = run(eng, dense, index)
    assert base_text == IN_PLACE % (WIDE if S % VEC[dt] == 0 else ELEMENT) and same(base, want) and base_nrep == n_nan
    if pitch:
        buf = torch.full((N_BATCH, pitch), float("nan"), dtype=dense.dtype, device="cuda")  # a read past a row's end is a counted NaN
        view = buf[:, :S]
        view.copy_(dense)
        assert view.stride() == (pitch, 1) and view.data_ptr() % 16 == 0
    else:
        flat = torch.full((N_BATCH * S + 1,), float("nan"), dtype=dense.dtype, device="cuda")
        view = flat[1:].view(N_BATCH, S)
        view.copy_(dense)
        assert view.stride() == (S, 1) and view.data_ptr() % 16 == ll.itemsize
    got, nrep, text = run(eng, view, index)
    assert text == IN_PLACE % leg, text
    assert np.array_equal(got.view(np.uint8), base.view(np.uint8)) and nrep == n_nan


# ---------------------------------------------------------------------------------------------------- device lists as they come
# offsets below 0, past offsets[G] and decreasing, empty groups, members of -3 and N + 5 (216 rows)
WILD_OFFSETS = [-2, 3, 3, 50, 7, 9, 9]
WILD_MEMBERS = [-3, 0, 4, 2, 5, N_BLOCK + 5, 7, 1, N_BLOCK - 1]
# the same with every group ascending behind the clamp, for the blocked route (blocks of 32 rows)
ASCENDING_OFFSETS = [-2, 4, 4, 11, 9, 50, 16, 16]
ASCENDING_MEMBERS = [-3, 0, 5, 31, 32, 40, 70, 100, 191, 192, 215, N_BLOCK - 1, N_BLOCK + 5, N_BLOCK + 5, N_BLOCK + 7, N_BLOCK + 9]


def test_wild_lists_stay_inside_their_arrays():
    """What the kernel's clamps make of the two lists, restated on the host: every position it reads lies inside `members`
    (offsets[G] entries are there), every row inside the matrix, and the blocked list is ascending behind the clamp."""
    for off, mem in ((WILD_OFFSETS, WILD_MEMBERS), (ASCENDING_OFFSETS, ASCENDING_MEMBERS)):
        assert 0 <= off[-1] == len(mem) and min(off) < 0 and max(off) > off[-1] and min(mem) == -3 and N_BLOCK + 5 in mem
        fixed = ref.clamped(off, mem, N_BLOCK)
        assert fixed.offsets[-1] <= 2 * len(mem) and fixed.members.min() == 0 and fixed.members.max() == N_BLOCK - 1
        assert (np.diff(fixed.offsets) == 0).sum() >= 2
    assert all(np.all(np.diff(g) >= 0) for g in ref.groups_of(ref.clamped(ASCENDING_OFFSETS, ASCENDING_MEMBERS, N_BLOCK)))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_device_lists_are_clamped(eng, dt):
    from pyloo_amd._capi import EngineError

    S = 40
    ll = ref.block_edge_matrix(N_BLOCK, S, dt, ref.block_edge_index(N_BLOCK, 32), 32)
    for off, mem in ((WILD_OFFSETS, WILD_MEMBERS), (ASCENDING_OFFSETS, ASCENDING_MEMBERS)):
        want, n_nan = ref.group_sums(ll, *ref.clamped(off, mem, N_BLOCK))
        got, nrep, text = run(eng, sources(ll)["draws"], (off, mem))
        assert text == IN_PLACE % WIDE and same(got, want) and nrep == n_nan
        assert not got[np.diff(ref.clamped(off, mem, N_BLOCK).offsets) == 0].any()  # empty groups are zeros
        # the host is told what is wrong with them, one fault at a time too
        good = ref.clamped(off, mem, N_BLOCK)
        bad_lists = [(off, mem), ([-1] + list(good.offsets[1:]), good.members), (good.offsets, [-3] + list(good.members[1:])),
                     (good.offsets, list(good.members[:-1]) + [N_BLOCK + 5]), (off, good.members)]
        for lists in bad_lists:
            with pytest.raises(EngineError) as err:
                eng.group_sum(ll, wrap(lists))
            assert err.value.code == -1, lists  # PLA_ERR_ARG


# ---------------------------------------------------------------------------------------------------- blocked path
BLOCKED_SHAPES = [(4096, "f8", WIDE), (4095, "f8", ELEMENT), (4096, "f4", WIDE)]  # S, dtype, leg: blocks of 32, 32, 64 rows

CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import group_gather_ref as ref
import pyloo_amd as pl
from pyloo_amd import _capi
from pyloo_amd.base import tail_count_for
from pyloo_amd.engine import get_engine
eng = get_engine(0)
N = 216
out = {"env": np.array(_capi.env_overrides())}
wrap = lambda ix: pl.GroupIndex(np.arange(len(ix[0]) - 1), np.asarray(ix[0], dtype=np.int64), np.asarray(ix[1], dtype=np.int64)).to("cuda")
for S, dt in ((4096, "f8"), (4095, "f8"), (4096, "f4")):
    B = (1 << 20) // (S * np.dtype(dt).itemsize)
    key = f"{dt}_{S}_"
    holes = ref.block_edge_index(N, B, empty=True)
    ll = ref.block_edge_matrix(N, S, np.dtype(dt).type, holes, B)
    t = torch.as_tensor(np.ascontiguousarray(ll.T)).cuda().T
    sums, nrep = eng.group_sum(t, wrap(holes))
    out[key + "route"] = np.array(eng.last_kernels())
    out[key + "sums"], out[key + "nrep"] = sums.cpu().numpy(), nrep.cpu().numpy()
    r = eng.psis_loo_groups(t, wrap(ref.block_edge_index(N, B, min_groups=2 * B + 5)), tail_count_for(S, 1.0), "psis", 1.0, 0.7)
    out[key + "psis_route"] = np.array(eng.last_kernels())
    for k in ("logo_i", "diag", "lppd_i", "n_replaced"):
        out[key + k] = r[k].cpu().numpy()
    if (S, dt) == (4096, "f8"):
        sums, nrep = eng.group_sum(t, wrap((eval(sys.argv[3]), eval(sys.argv[4]))))
        out["wild_sums"], out["wild_nrep"] = sums.cpu().numpy(), nrep.cpu().numpy()
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def blocked_runs(tmp_path_factory):
    """The child's outputs with PLA_INGEST_BLOCK_MB unset (one block) and 1 (blocks of (1 << 20) // (S * itemsize) rows)."""
    runs = []
    for i, block_mb in enumerate((None, "1")):
        env = {k: v for k, v in os.environ.items() if k != "PLA_INGEST_BLOCK_MB"}
        if block_mb:
            env["PLA_INGEST_BLOCK_MB"] = block_mb
        path = tmp_path_factory.mktemp("blocked") / f"out{i}.npz"
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path), repr(ASCENDING_OFFSETS), repr(ASCENDING_MEMBERS)], env=env,
                              capture_output=True, text=True, timeout=240)
        assert proc.returncode == 0, proc.stderr[-3000:]
        with np.load(path) as z:
            runs.append({k: z[k] for k in z.files})
    return runs


@pytest.mark.parametrize("S,dt,leg", BLOCKED_SHAPES)
def test_blocked_path(blocked_runs, S, dt, leg):
    one_block, blocked = blocked_runs
    assert "PLA_INGEST_BLOCK_MB" not in str(one_block["env"]) and "PLA_INGEST_BLOCK_MB" in str(blocked["env"])
    B = (1 << 20) // (S * np.dtype(dt).itemsize)
    assert B == (64 if dt == "f4" else 32) and N_BLOCK % B == 24
    holes = ref.block_edge_index(N_BLOCK, B, empty=True)
    ll = ref.block_edge_matrix(N_BLOCK, S, np.dtype(dt).type, holes, B)
    want, n_nan = ref.group_sums(ll, *holes)
    assert n_nan > 0 and not np.isnan(want).any()
    empty = np.diff(holes.offsets) == 0
    assert empty.sum() == 3 and empty[0] and empty[-1]
    many = ref.block_edge_index(N_BLOCK, B, min_groups=2 * B + 5)
    many_nan = int(np.isnan(ll[many.members]).sum())
    key = f"{dt}_{S}_"
    for run_ in (one_block, blocked):
        assert str(run_[key + "route"]) == ROUTES["obs"] % leg
        got = run_[key + "sums"]
        assert got.dtype == want.dtype and got.shape == want.shape
        assert not got[empty].any(), "an empty group is not zero"
        assert np.array_equal(got, want), ("groups that differ", np.flatnonzero((got != want).any(axis=1)))
        assert int(run_[key + "nrep"][0]) == n_nan
        assert "blocks of observations" in str(run_[key + "psis_route"]) and "per block of groups" in str(run_[key + "psis_route"])
        assert int(run_[key + "n_replaced"][0]) == many_nan
        assert run_[key + "logo_i"].shape == (2 * B + 5,)  # three blocks of groups under the one-megabyte setting
    # a replaced entry (-1e10 in one draw of a sum) leaves that group one draw that carries all the weight and no tail to fit: such
    # groups are held to the same bits only, every other group to finite numbers as well
    whole = np.array([not np.isnan(ll[g]).any() for g in ref.groups_of(many)])
    assert 0 < (~whole).sum() < len(whole) // 2
    for k in ("logo_i", "diag", "lppd_i"):
        a, b = one_block[key + k], blocked[key + k]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), k
        assert np.isfinite(a[whole]).all(), k


def test_blocked_path_device_lists(blocked_runs):
    """The ascending wild list on the blocked route: the lower-bound search runs over the clamped members, and the row is clamped
    into the block."""
    holes = ref.block_edge_index(N_BLOCK, 32, empty=True)
    ll = ref.block_edge_matrix(N_BLOCK, 4096, np.float64, holes, 32)
    want, n_nan = ref.group_sums(ll, *ref.clamped(ASCENDING_OFFSETS, ASCENDING_MEMBERS, N_BLOCK))
    assert n_nan > 0
    for run_ in blocked_runs:
        assert np.array_equal(run_["wild_sums"], want) and int(run_["wild_nrep"][0]) == n_nan
