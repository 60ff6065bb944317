"""The layouts of tests/far_views.py, checked on the CPU with ``far_layout`` alone (no GPU, no 16 GiB tensor): for every shape
tests/test_gpu_far_offsets.py uses, properties (a) to (d) of the module docstring, the alignment of each kind, and that views
used together in one case do not overlap."""

import numpy as np
import pytest

import far_views as fv

LAYOUTS = fv.all_layouts()
ROOM = fv.ARENA_BYTES - fv.ORIGIN


def ids(v):
    return "-".join(str(x) for x in v)


def runs(n, s, itemsize, kind, shift=0):
    """(start, end) bytes from ``ORIGIN`` of every row or line, and the view's own offset."""
    off, _ = fv.far_layout(n, s, itemsize, kind, shift)
    return off, fv.far_extent(n, s, itemsize, kind, shift)


def test_every_shape_of_the_gpu_file_is_listed():
    assert len(LAYOUTS) > 60
    assert {k for _, _, _, k in LAYOUTS} == set(fv.KINDS)
    assert {i for _, _, i, _ in LAYOUTS} == {4, 8}


@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
def test_far_layout_properties(layout):
    n, s, itemsize, kind = layout
    off, ext = runs(n, s, itemsize, kind)
    rel = [(a - off, b - off) for a, b in ext]  # from the view's own pointer
    span = (rel[0][1] - rel[0][0]) // itemsize
    assert rel[0][0] == 0 and all(b[0] > a[1] for a, b in zip(rel, rel[1:])), "runs overlap"
    assert any(b <= 2 ** 32 for _, b in rel), "(a) no run wholly below 2^32"
    if span >= 64:
        assert any(a <= 2 ** 32 < b for a, b in rel), "(b) no run contains offset 2^32"
        assert any(a <= 2 ** 33 < b for a, b in rel), "(c) no run contains offset 2^33"
    # (shorter runs: the last one holds offset 2^33 or lies past it all the same)
    assert rel[-1][1] > 2 ** 33 and rel[-1][0] >= 2 ** 33 - span * itemsize  # the planted NaN of the last run lies at or past 2^33 ...
    if itemsize == 4:
        assert (rel[-1][1] - 4) // 4 >= 2 ** 31  # ... for f32 at an element index that leaves 31 bits
    else:
        assert (rel[-1][1] - 8) // 8 < 2 ** 31  # (f64: this arena cannot reach element 2^31)
    assert off + rel[-1][1] <= ROOM - fv.RESERVE, "(d) the last element lies outside the arena"
    # strides and pointer
    _, (so, sd) = fv.far_layout(n, s, itemsize, kind)
    far, near = max(so, sd), min(so, sd)
    al = 16 // itemsize
    if kind.endswith("_odd"):
        assert off == itemsize and far % al == 1 and near == 1
    else:
        assert off == 0 and far % al == 0 and near == (2 if kind == "both" else 1)
    assert (so > sd) == (not kind.startswith("lines"))
    if kind.startswith("lines"):
        assert far >= n  # observations fastest as the library understands it: stride_draw >= n_obs


@pytest.mark.parametrize("case", fv.TOGETHER, ids=lambda c: ids(c[0]) + f"+{len(c) - 1}")
def test_views_of_one_case_do_not_overlap(case):
    spans = []
    for n, s, dt, kind, shift in case:
        itemsize = np.dtype(dt).itemsize
        assert shift * itemsize + itemsize <= fv.RESERVE
        off, ext = runs(n, s, itemsize, kind, shift)
        assert off == (shift + kind.endswith("_odd")) * itemsize
        assert ext[-1][1] <= ROOM, "the shifted view leaves the arena"
        spans += ext
    spans.sort()
    assert all(b[0] >= a[1] for a, b in zip(spans, spans[1:])), "two views of one case share bytes"


def test_shapes_without_a_pitch_are_refused():
    """What moved two shapes of the issue's table: no multiple of 16 bytes puts a line of 70 elements on offset 2^32 when there are 543
    lines, nor a line of 65 f32 one element off when there are 257."""
    for n, s, itemsize, kind in ((70, 543, 4, "lines"), (70, 543, 8, "lines"), (65, 257, 4, "lines_odd"), (66, 257, 4, "lines_odd")):
        with pytest.raises(ValueError, match="no pitch"):
            fv.far_layout(n, s, itemsize, kind)
    with pytest.raises(ValueError, match="three rows or lines"):
        fv.far_layout(2, 1000, 4, "rows")


def test_twin_is_of_the_same_layout_class():
    import torch

    a = np.arange(9 * 40, dtype=np.float32).reshape(9, 40)
    for kind in fv.KINDS:
        t = fv.twin(a, kind, device="cpu")
        _, (so, sd) = fv.far_layout(9, 1000, 4, kind)
        assert torch.equal(t, torch.from_numpy(a))
        assert ((t.stride(0) == 1), (t.stride(1) == 1)) == ((so == 1), (sd == 1))
        assert (t.data_ptr() % 16 == 0) == (not kind.endswith("_odd"))
        for st, far in zip(t.stride(), (so, sd)):
            assert st % 4 == far % 4 or st == far or kind == "both"  # (both: the strided routes ask nothing of the pitch)
    p = fv.twin_pitched(np.zeros((3, 5, 7)), device="cpu")
    assert p.stride() == (38, 7, 1)
