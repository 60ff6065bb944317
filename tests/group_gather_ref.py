"""Plain NumPy references of the two index-list passes in front of the PSIS-LOO pass -- the group sums of ``pla_group_sum``
(csrc/pla_group.h) and the draw gather of ``pla_gather_draws`` (csrc/pla_draws.h) -- and the index lists that put the branches of
those kernels at their edges.  NumPy only; nothing here calls the library.

Contracts restated: ``group_sums`` is ``ll[members].sum(axis=0)`` in the dtype of ``ll``, one add per member in ascending order,
seeded with the first member's row; ``gather`` is ``ll[:, idx]``; in both NaN becomes ``dtype(-1e10)`` and is counted.

An index is the pair ``(offsets, members)`` of int64 arrays of a ``GroupIndex``: group g holds ``members[offsets[g]:offsets[g + 1]]``.
Groups may share rows: the kernel sums every group on its own, and the builders use that to keep the matrices at a few hundred rows.
"""

import collections

import numpy as np

BATCH = 8  # kGroupBatch of csrc/pla_group.h: member rows per batch of loads
BATCH_EDGE_SIZES = tuple(range(1, 35)) + (64, 65, 129)  # one group of each
CONTINUED_COUNTS = (1, 7, 8, 9, 15, 16, 17, 24, 25)  # members in a later block: the batch loop's edges when acc comes from `out`
FRESH_COUNTS = (1, 2, 8, 9, 10, 16, 17, 18, 25)  # members in the first block: the edges when the first member seeds acc

Index = collections.namedtuple("Index", "offsets members")


def _fix(x):
    """NaN -> dtype(-1e10), as the kernels do on load (group sums) or on store (gather)."""
    return np.where(np.isnan(x), x.dtype.type(-1e10), x)


def _index(groups):
    offsets = np.zeros(len(groups) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(g) for g in groups])
    members = np.concatenate([np.asarray(g, dtype=np.int64) for g in groups]) if offsets[-1] else np.zeros(0, dtype=np.int64)
    return Index(offsets, members)


def groups_of(index):
    off, mem = index
    return [mem[off[g]:off[g + 1]] for g in range(len(off) - 1)]


# ---------------------------------------------------------------------------------------------------- group sums
def group_sums(ll, offsets, members):
    """``(sums, n_nan)``: ``sums[g]`` built member by member in ``ll.dtype`` (an empty group gives zeros); ``n_nan`` is the NaN
    count of ``ll[members]``."""
    G = len(offsets) - 1
    out = np.zeros((G, ll.shape[1]), dtype=ll.dtype)
    n_nan = 0
    with np.errstate(invalid="ignore"):  # inf + -inf
        for g in range(G):
            mem = members[offsets[g]:offsets[g + 1]]
            if len(mem) == 0:
                continue
            n_nan += int(np.isnan(ll[mem]).sum())
            acc = _fix(ll[mem[0]]).copy()
            for m in mem[1:]:
                acc = acc + _fix(ll[m])
            assert acc.dtype == ll.dtype
            out[g] = acc
    return out, n_nan


def clamped(offsets, members, n_obs):
    """The clamp the kernel documents for device lists (csrc/pla_group.h), restated: ``(offsets, members)`` that are in range and
    select the rows the kernel reads."""
    offsets, members = np.asarray(offsets, dtype=np.int64), np.asarray(members, dtype=np.int64)
    G = len(offsets) - 1
    nm = max(int(offsets[G]), 0)
    lo = np.clip(offsets[:-1], 0, nm)
    hi = np.array([np.clip(offsets[g + 1], lo[g], nm) for g in range(G)], dtype=np.int64)
    mem = np.clip(members, 0, n_obs - 1)
    return _index([mem[lo[g]:hi[g]] for g in range(G)])


def _lower_bound(members, lo, hi, key):
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if members[mid] < key:
            lo = mid + 1
        else:
            hi = mid
    return lo


def blocked_group_sums(ll, offsets, members, rows_per_block):
    """The blocked algorithm of the kernel, block by block over ``ll[r0:r0 + rows_per_block]``: per group a lower-bound search for
    its members inside the block (the lists are ascending), the partial sum of the earlier blocks read back from ``out`` when
    members came before this block, empty groups zeroed in the first block only.  ``out`` starts as NaN, so an entry that no
    block writes shows.  Returns ``(sums, n_nan)``; on ascending lists it has to equal :func:`group_sums` bit for bit."""
    N, S = ll.shape
    G = len(offsets) - 1
    out = np.full((G, S), np.nan, dtype=ll.dtype)
    n_nan = 0
    with np.errstate(invalid="ignore"):
        for r0 in range(0, N, rows_per_block):
            block = ll[r0:r0 + rows_per_block]
            for g in range(G):
                lo, hi = int(offsets[g]), int(offsets[g + 1])
                empty, cont = lo == hi, False
                if not empty:
                    a = _lower_bound(members, lo, hi, r0)
                    b = _lower_bound(members, a, hi, r0 + len(block))
                    cont = a != lo
                    lo, hi = a, b
                if lo == hi:
                    if empty and r0 == 0:
                        out[g] = 0
                    continue
                rows = block[members[lo:hi] - r0]
                n_nan += int(np.isnan(rows).sum())
                rows = _fix(rows)
                if cont:
                    acc, rest = out[g].copy(), rows
                else:
                    acc, rest = rows[0].copy(), rows[1:]
                for x in rest:
                    acc = acc + x
                out[g] = acc
    return out, n_nan


def batch_edge_index(n_obs, kind):
    """One group of each size in ``BATCH_EDGE_SIZES`` (1..34, 64, 65, 129) over ``n_obs >= 129`` rows.  ``kind="contiguous"``:
    consecutive rows; ``kind="scattered"``: the rows dealt out by a fixed permutation, every group's members ascending.  The groups
    take their rows one behind the other and wrap around, so below 853 rows they share some."""
    assert n_obs >= max(BATCH_EDGE_SIZES) and kind in ("contiguous", "scattered")
    perm = np.random.default_rng(20241).permutation(n_obs)
    groups, at = [], 0
    for k in BATCH_EDGE_SIZES:
        if kind == "contiguous":
            start = at % (n_obs - k + 1)
            groups.append(np.arange(start, start + k))
        else:
            groups.append(np.sort(perm[(at + np.arange(k)) % n_obs]))
        at += k
    return _index(groups)


def batch_edge_matrix(n_obs, S, dtype, index, seed=0):
    """An (n_obs, S) matrix for a ``batch_edge_index``, row scales from 0.1 to 50 so that the order of the adds shows in the last
    bit.  Of the 25-member group, the first member, the first and the last of the first two batches behind it (members 1, 8, 9,
    16) and the last member (24) carry a NaN each, in draws below S - 1.  Draw S - 1 holds +inf in member 3 and -inf in member 5
    of the 34-member group: the sums that take both are NaN there, and those are the only NaN of the sums."""
    rng = np.random.default_rng(77 * S + seed)
    ll = (rng.normal(size=(n_obs, S)) * rng.uniform(0.1, 50, size=(n_obs, 1))).astype(dtype)
    groups = groups_of(index)
    g25, g34 = groups[BATCH_EDGE_SIZES.index(25)], groups[BATCH_EDGE_SIZES.index(34)]
    for k, pos in enumerate((0, 1, BATCH, BATCH + 1, 2 * BATCH, 24)):
        ll[g25[pos], (5 * k) % (S - 1)] = np.nan
    ll[g34[3], S - 1] = np.inf
    ll[g34[5], S - 1] = -np.inf
    return ll


def block_edge_index(n_obs, B, empty=False, min_groups=0):
    """Ascending groups for blocks of ``B`` rows (``n_obs`` = at least four blocks, the last one ragged with at least 6 rows;
    ``B >= 32``).  With ``nb`` blocks, ``R`` rows in the last one and ``nf = nb - 1`` whole blocks, the groups are, in this order:

    * whole      block 1 from its first to its last row (a)(h)
    * every      row 3 of every block (b)
    * gap        2 rows of block 0, 3 rows of block 3, none between (c): a started group with ``lo == hi`` in blocks 1 and 2
    * ragged     all ``R`` rows of the last block (d): it starts in the last block
    * ragged5    rows 1, 2, 3 and the last two of the last block (d)
    * cont_c     for c in ``CONTINUED_COUNTS``, twice: 2 rows of whole block p, then c rows of block p + 1 (every other row where
                 they fit, else consecutive) (e); p runs over the whole blocks, so most of these start in a later block
    * fresh_c    for c in ``FRESH_COUNTS``, twice: the last c rows of whole block p (h), then 3 rows of a later block -- the ragged
                 one for every other group (f)
    * single     rows 0, B - 1, B and n_obs - 1 (g)
    * tail3      the last 3 rows of block 0 (h)
    * into_end   2 rows of block 0 and the last 4 rows of block 1 (h)
    * span       rows B - 10 .. 2 B + 9: ten rows, a whole block on the continued path, ten rows
    * straddle   for every block boundary, the last row of one block and the first of the next

    ``min_groups``: singletons of rows 0, 1, ... are appended until there are that many groups.  ``empty``: the device variant,
    with an empty group put at the first, a middle and the last position."""
    nb = -(-n_obs // B)
    R = n_obs - (nb - 1) * B
    nf = nb - 1
    assert nb >= 4 and 6 <= R < B and B >= 32
    row = lambda b, offs: b * B + np.asarray(offs)  # noqa: E731
    groups = [row(1, np.arange(B)), np.array([b * B + 3 for b in range(nb)]),
              np.concatenate([row(0, [4, 9]), row(3, [0, 2, 5])]), row(nb - 1, np.arange(R)), row(nb - 1, [1, 2, 3, R - 2, R - 1])]
    for rep in range(2):
        for i, c in enumerate(CONTINUED_COUNTS):
            p = (i + 2 * rep) % (nf - 1)
            later = 2 * np.arange(c) + rep if 2 * c + rep <= B else np.arange(c) + rep
            groups.append(np.concatenate([row(p, [5 + rep, 11]), row(p + 1, later)]))
    for rep in range(2):
        for i, c in enumerate(FRESH_COUNTS):
            p = (i + rep) % (nf - 1)
            q = nb - 1 if (i + rep) % 2 else p + 1 + (i % (nf - 1 - p))
            groups.append(np.concatenate([row(p, np.arange(B - c, B)), row(q, [0, 2, 4] if q == nb - 1 else [1, B // 2, B - 1])]))
    groups += [np.array([r]) for r in (0, B - 1, B, n_obs - 1)]
    groups += [row(0, [B - 3, B - 2, B - 1]), np.concatenate([row(0, [0, 1]), row(1, np.arange(B - 4, B))]),
               np.arange(B - 10, 2 * B + 10)]
    groups += [np.array([b * B - 1, b * B]) for b in range(1, nb)]
    k = 0
    while len(groups) < min_groups:
        groups.append(np.array([k % n_obs]))
        k += 1
    for g in groups:
        assert np.all(np.diff(g) > 0) and g[0] >= 0 and g[-1] < n_obs
    if empty:
        none = np.zeros(0, dtype=np.int64)
        groups = [none] + groups[:len(groups) // 2] + [none] + groups[len(groups) // 2:] + [none]
    return _index(groups)


def block_edge_properties(index, B):
    """``counts[g, b]``: the members of group g inside block b (rows ``[b B, (b + 1) B)``)."""
    off, mem = index
    nb = int(mem.max()) // B + 1
    counts = np.zeros((len(off) - 1, nb), dtype=np.int64)
    for g, m in enumerate(groups_of(index)):
        np.add.at(counts[g], m // B, 1)
    return counts


def block_edge_matrix(n_obs, S, dtype, index, B, seed=0):
    """An (n_obs, S) log-likelihood matrix (values a PSIS pass can take) for ``index`` -- a ``block_edge_index`` without empty
    groups in front -- with NaN in a first member (the gap group's), in members read on the continued path (the gap group's first
    in block 3, a cont_c group's second batch) and in the last member of the ragged block, each in three draws."""
    rng = np.random.default_rng(1000 * S + B + seed)
    ll = (-rng.uniform(0.01, 0.1, size=(n_obs, 1)) * rng.exponential(size=(n_obs, S)) + rng.normal(size=(n_obs, 1))).astype(dtype)
    groups = [g for g in groups_of(index) if len(g)]
    gap = groups[2]
    cont25 = groups[5 + CONTINUED_COUNTS.index(25)]
    assert gap[0] // B == 0 and gap[2] // B == 3 and len(cont25) == 27
    for k, r in enumerate((gap[0], gap[2], cont25[2 + BATCH], cont25[-1], n_obs - 1)):
        ll[r, [k % S, (S // 2 + 3 * k) % S, S - 1 - k % S]] = np.nan
    return ll


# ---------------------------------------------------------------------------------------------------- gather
def gather(ll, idx):
    """``(ll[:, clip(idx)]`` with NaN written as -1e10, the NaN count of that matrix)``."""
    picked = ll[:, np.clip(np.asarray(idx, dtype=np.int64), 0, ll.shape[1] - 1)]
    return _fix(picked), int(np.isnan(picked).sum())
