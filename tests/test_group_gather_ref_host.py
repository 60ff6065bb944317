"""The NumPy references of tests/group_gather_ref.py among each other, on the CPU: the member-by-member group sums against NumPy's
own ``ll[members].sum(axis=0)``, the block-by-block emulation of the kernel's blocked algorithm against the member-by-member
sums (the algorithm keeps the order of the adds whatever the block size), and the index builders against the list of branches
they are meant to reach."""

import numpy as np
import pytest

import group_gather_ref as ref

# draws per row of the batch-edge tests (tests/test_gpu_loo_group_edges.py): the wave (64 vectors) and workgroup (256 vectors) edges
# at VEC = 2 (f64) / 4 (f32), the element leg, tiny rows
BATCH_EDGE_DRAWS = {
    np.float64: (126, 128, 130, 510, 512, 514, 63, 65, 255, 257, 2, 6),
    np.float32: (252, 256, 260, 1020, 1024, 1028, 253, 254, 255, 2, 6),
}
N_BATCH = 200  # rows of the batch-edge matrices
N_BLOCK = 216  # rows of the block-edge matrices: six blocks of 32 or three of 64, and a ragged block of 24


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["contiguous", "scattered"])
def test_group_sums_are_numpys(dt, kind):
    index = ref.batch_edge_index(N_BATCH, kind)
    assert tuple(len(g) for g in ref.groups_of(index)) == ref.BATCH_EDGE_SIZES
    assert all(np.all(np.diff(g) > 0) for g in ref.groups_of(index))
    for S in BATCH_EDGE_DRAWS[dt]:
        ll = ref.batch_edge_matrix(N_BATCH, S, dt, index)
        got, n_nan = ref.group_sums(ll, *index)
        fixed = np.where(np.isnan(ll), dt(-1e10), ll)
        with np.errstate(invalid="ignore"):
            want = np.stack([fixed[g].sum(axis=0) for g in ref.groups_of(index)])
        assert got.dtype == dt and np.array_equal(got, want, equal_nan=True), S
        assert n_nan == int(np.isnan(ll[index.members]).sum()) >= 6
        nan = np.isnan(want)
        assert nan.any() and not nan[:, :S - 1].any(), S  # inf + -inf in the last draw, nowhere else


def test_clamped_restates_the_kernel_clamp():
    got = ref.clamped([-2, 3, 3, 50, 7, 9, 9], [-3, 0, 4, 2, 5, 25, 7, 1, 19], 20)
    assert got.offsets.tolist() == [0, 3, 3, 9, 9, 11, 11]
    assert [g.tolist() for g in ref.groups_of(got)] == [[0, 0, 4], [], [2, 5, 19, 7, 1, 19], [], [1, 19], []]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("B", [32, 64])
@pytest.mark.parametrize("empty", [False, True])
def test_blocked_sums_keep_the_order(dt, B, empty):
    index = ref.block_edge_index(N_BLOCK, B, empty=empty)
    for S in (40, 7):
        ll = ref.block_edge_matrix(N_BLOCK, S, dt, index, B)
        ll *= np.random.default_rng(B).uniform(0.1, 50, size=(N_BLOCK, 1)).astype(dt)  # (row scales: the order shows in the last bit)
        want, n_nan = ref.group_sums(ll, *index)
        assert n_nan == int(np.isnan(ll[index.members]).sum()) > 0
        for rows in (B, N_BLOCK, 1, 5):
            got, got_nan = ref.blocked_group_sums(ll, *index, rows)
            assert np.array_equal(got, want) and got_nan == n_nan, (S, rows)
        lengths = np.diff(index.offsets)
        assert ((lengths == 0).sum() == 3 and lengths[0] == lengths[-1] == 0) if empty else lengths.min() > 0
        assert not want[lengths == 0].any()


def test_blocked_sums_nan_placements():
    """The NaN of block_edge_matrix lie where its docstring says, for both block sizes."""
    for B in (32, 64):
        index = ref.block_edge_index(N_BLOCK, B)
        ll = ref.block_edge_matrix(N_BLOCK, 40, np.float64, index, B)
        rows = set(np.flatnonzero(np.isnan(ll).any(axis=1)).tolist())
        groups = ref.groups_of(index)
        firsts = {int(g[0]) for g in groups}
        continued = {int(m) for g in groups for m in g if m // B > g[0] // B}
        assert rows & firsts and rows & continued and N_BLOCK - 1 in rows
        assert len(rows) == 5 and int(np.isnan(ll).sum()) == 15


@pytest.mark.parametrize("B", [32, 64])
def test_block_edge_index_reaches_every_branch(B):
    index = ref.block_edge_index(N_BLOCK, B)
    groups = ref.groups_of(index)
    counts = ref.block_edge_properties(index, B)
    nb = counts.shape[1]
    assert nb == -(-N_BLOCK // B) >= 4 and N_BLOCK % B != 0  # the last block is ragged
    assert np.array_equal(counts.sum(axis=1), np.diff(index.offsets))
    total = counts.sum(axis=1)
    first = (counts > 0).argmax(axis=1)
    # (a) exactly one whole block
    assert any(counts[g].max() == B == total[g] and groups[g][0] % B == 0 for g in range(len(groups)))
    # (b) one member in every block
    assert any((counts[g] == 1).all() for g in range(len(groups)))
    # (c) block 0 and block 3, none between
    assert any(counts[g, 0] > 0 and counts[g, 3] > 0 and not counts[g, 1:3].any() for g in range(len(groups)))
    # (d) wholly in the ragged last block
    assert any(counts[g, nb - 1] == total[g] for g in range(len(groups)) if total[g] > 1)
    # (e) continued path: c members in a block behind the group's first
    for c in ref.CONTINUED_COUNTS:
        assert any(c in counts[g, first[g] + 1:] for g in range(len(groups))), c
    # (f) fresh path: c members in the group's first block, more behind it
    for c in ref.FRESH_COUNTS:
        assert any(counts[g, first[g]] == c and total[g] > c for g in range(len(groups))), c
    # (g) singletons at the block corners
    singles = {int(g[0]) for g in groups if len(g) == 1}
    assert {0, B - 1, B, N_BLOCK - 1} <= singles
    # (h) a group that ends on the last row of a block
    assert any(g[-1] % B == B - 1 for g in groups)
    # a group that starts in a later block, and one with a whole block on the continued path
    assert any(first[g] > 0 for g in range(len(groups)))
    assert any(B in counts[g, first[g] + 1:] for g in range(len(groups)))


def test_block_edge_index_variants():
    for B in (32, 64):
        plain = ref.block_edge_index(N_BLOCK, B)
        many = ref.block_edge_index(N_BLOCK, B, min_groups=2 * B + 5)
        assert len(many.offsets) - 1 == 2 * B + 5 > len(plain.offsets) - 1
        assert np.array_equal(many.members[:len(plain.members)], plain.members)
        holes = ref.block_edge_index(N_BLOCK, B, empty=True)
        assert len(holes.offsets) == len(plain.offsets) + 3 and np.array_equal(holes.members, plain.members)


def test_gather_reference():
    ll = np.arange(12, dtype=np.float32).reshape(3, 4)
    ll[1, 2] = np.nan
    ll[2, 0] = np.inf
    got, n_nan = ref.gather(ll, [-5, 2, 2, 9, 0])
    assert n_nan == 2 and got.dtype == np.float32
    assert np.array_equal(got, np.array([[0, 2, 2, 3, 0], [4, -1e10, -1e10, 7, 4], [np.inf, 10, 10, 11, np.inf]], dtype=np.float32))
