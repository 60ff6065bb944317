"""TEST INFRASTRUCTURE ONLY: small matrices whose rows or lines lie billions of elements apart.

A 32-bit product or offset in a kernel's address arithmetic shows only when a matrix element lies 2^31 elements or 2^32
bytes from the pointer the library was given.  Such a matrix need not be large: ``far_view`` places a *small* matrix into
one *large, otherwise untouched* allocation (the arena, ``ARENA_BYTES`` of ``torch.uint8``) with a row or line pitch of
hundreds of megabytes, so that a case reads a few megabytes and runs in milliseconds.

Every far view starts ``ORIGIN = 2^33`` bytes into the arena (plus a small shift), never at byte 0, and the arena is
filled with the byte 0xFF -- a NaN in f32 and in f64 -- before the first case.  This is deliberate: an offset that is
sign-extended from 32 bits then lands in the lower half of the arena, one that wraps unsigned lands just above ``ORIGIN``;
either way the wrong read stays inside memory the test owns and has poisoned, and comes back as a NaN that the library
counts and replaces.  On a machine shared with others the test has to detect such a defect without risking an access
outside its own allocation.

The layouts (``far_layout``), strides in elements as ``(stride_obs, stride_draw)`` of an (n, s) matrix:

=========  ===========  ==========================================================================================
kind       strides      pointer and pitch
=========  ===========  ==========================================================================================
rows       (P, 1)       P a multiple of 16 / itemsize; the view's pointer 16-byte aligned
rows_odd   (P + 1, 1)   the pointer moved by one element (the element-load routes)
lines      (1, Q)       Q >= n, a multiple of 16 / itemsize
lines_odd  (1, Q + 1)   the pointer moved by one element
both       (P, 2)       neither stride is 1 (the strided and general routes)
=========  ===========  ==========================================================================================

P or Q is chosen so that, in bytes from the view's own pointer, (a) at least one row or line lies wholly below 2^32,
(b) a row or line of 64 elements or more contains offset 2^32, (c) one contains offset 2^33 -- for f32 that is element
2^31 -- and (d) the last element lies inside the arena.  Rows or lines shorter than 64 elements hold the two offsets where a
pitch allows it; where none does, the first lies below 2^32 and the last wholly past 2^33.  A shape for which no multiple of
16 bytes meets (b) and (c) is refused (``ValueError``): the caller moves to the nearest shape that has one.

For f64 the element offsets cannot reach 2^31 inside this arena (2^31 doubles are 2^34 bytes, and a view has 2^33 + 2^28
bytes above ``ORIGIN``): f64 views test byte offsets only.

``tests/test_far_views_host.py`` proves (a) to (d) for every shape the GPU file uses, without a GPU.

No GPU work happens at import; torch is imported by the functions that need it.
"""

import numpy as np

from lfo_ref import CHUNK

ARENA_BYTES = 2 ** 34 + 2 ** 28
ORIGIN = 2 ** 33
RESERVE = 2 ** 24 + 2 ** 16  # bytes at the top of the arena kept free for the shifts of second and third views of one case
KINDS = ("rows", "rows_odd", "lines", "lines_odd", "both")
T32, T33 = 2 ** 32, 2 ** 33


def _runs(n, s, kind):
    """(number of rows or lines, elements one of them spans, 1 for the odd kinds)."""
    if kind in ("rows", "rows_odd"):
        return n, s, int(kind == "rows_odd")
    if kind in ("lines", "lines_odd"):
        return s, n, int(kind == "lines_odd")
    if kind == "both":
        return n, 2 * s - 1, 0
    raise ValueError(f"unknown kind {kind!r}")


def _pitch_bytes(m, span_bytes, itemsize, odd, strict):
    """The largest pitch (bytes; a multiple of 16, plus one element for the odd kinds) with one run starting in
    (2^32 - span, 2^32], one in (2^33 - span, 2^33] and the last run ending inside the arena; ``strict``: neither run
    starts exactly on the power of two.  None when there is none."""
    room = ARENA_BYTES - ORIGIN - RESERVE
    extra = itemsize * odd
    for i in range(1, m):  # run i takes offset 2^32: a small i is a large pitch
        hi = T32 // i
        lo = (T32 - span_bytes) // i + 1  # i * pitch > 2^32 - span
        pb = (hi - extra) // 16 * 16 + extra
        while pb >= lo and pb > span_bytes:
            j = T33 // pb
            ok = j < m and T33 - j * pb < span_bytes and (m - 1) * pb + span_bytes + extra <= room
            if ok and strict and (i * pb == T32 or j * pb == T33):
                ok = False
            if ok:
                return pb
            pb -= 16
    return None


def far_layout(n, s, itemsize, kind, shift=0):
    """``(byte offset from ORIGIN, (stride_obs, stride_draw))`` of the far (n, s) matrix of ``kind``, strides in elements.
    ``shift``: further elements between ``ORIGIN`` and the view (a second matrix of the same case)."""
    m, span, odd = _runs(n, s, kind)
    if m < 3:
        raise ValueError("a far view needs three rows or lines: one below 2^32, one at 2^32, one at 2^33")
    pb = _pitch_bytes(m, span * itemsize, itemsize, odd, True) or _pitch_bytes(m, span * itemsize, itemsize, odd, False)
    if pb is None and span < 64:  # short runs: the first wholly below 2^32, the last wholly past 2^33, as far apart as the arena allows
        extra = itemsize * odd
        pb = ((ARENA_BYTES - ORIGIN - RESERVE - span * itemsize - extra) // (m - 1) - extra) // 16 * 16 + extra
        if (m - 1) * pb <= T33:
            pb = None
    if pb is None:
        raise ValueError(f"no pitch puts {m} runs of {span} elements of {itemsize} bytes across 2^32 and 2^33 inside the arena")
    if shift * itemsize + odd * itemsize > RESERVE:
        raise ValueError("shift beyond the reserve")
    pitch = pb // itemsize
    offset = (odd + shift) * itemsize
    if kind in ("rows", "rows_odd"):
        return offset, (pitch, 1)
    if kind in ("lines", "lines_odd"):
        return offset, (1, pitch)
    return offset, (pitch, 2)


def far_extent(n, s, itemsize, kind, shift=0):
    """The byte intervals ``[(lo, hi), ...]`` from ``ORIGIN`` that the runs of the far view cover, one per row or line."""
    off, (so, sd) = far_layout(n, s, itemsize, kind, shift)
    m, span, _ = _runs(n, s, kind)
    pitch = max(so, sd) * itemsize
    return [(off + r * pitch, off + r * pitch + span * itemsize) for r in range(m)]


def _torch_dtype(a):
    import torch

    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(a.dtype)]


def new_arena(device="cuda"):
    """The arena, every byte 0xFF."""
    import torch

    arena = torch.empty(ARENA_BYTES, dtype=torch.uint8, device=device)
    arena.fill_(0xFF)
    return arena


def strided_view(arena, dtype, shape, strides, byte_offset):
    """A view of the arena's bytes as ``dtype`` with the given strides (elements), ``byte_offset`` from the arena's start."""
    import torch

    itemsize = torch.empty((), dtype=dtype).element_size()
    assert byte_offset % itemsize == 0
    last = byte_offset + (sum((n - 1) * st for n, st in zip(shape, strides)) + 1) * itemsize
    assert 0 <= byte_offset and last <= arena.numel(), "view outside the arena"
    return torch.as_strided(arena.view(dtype), tuple(shape), tuple(strides), byte_offset // itemsize)


def far_view(arena, a, kind, shift=0):
    """The host matrix ``a`` (n, s; f32 or f64 ndarray) copied into its far view of the arena; returns the view."""
    import torch

    a = np.ascontiguousarray(a)
    n, s = a.shape
    off, strides = far_layout(n, s, a.itemsize, kind, shift)
    view = strided_view(arena, _torch_dtype(a), (n, s), strides, ORIGIN + off)
    view.copy_(torch.from_numpy(a).to(arena.device))
    return view


def far_pitched(arena, a, shift=0):
    """The host array ``a`` (m, ...) with its leading dimension far apart (the ``rows`` layout of the (m, rest) matrix) and the
    others dense: a pitch, a batch stride."""
    import torch

    a = np.ascontiguousarray(a)
    inner = int(np.prod(a.shape[1:]))
    off, (pitch, _) = far_layout(a.shape[0], inner, a.itemsize, "rows", shift)
    dense = [int(np.prod(a.shape[d + 1:])) for d in range(1, a.ndim)]
    view = strided_view(arena, _torch_dtype(a), a.shape, [pitch] + dense, ORIGIN + off)
    view.copy_(torch.from_numpy(a).to(arena.device))
    return view


def twin_pitched(a, device="cuda"):
    """``a`` (m, ...) on the device with a leading pitch of ``rest + 16 / itemsize`` elements, the padding NaN."""
    import torch

    a = np.ascontiguousarray(a)
    inner = int(np.prod(a.shape[1:]))
    al = 16 // a.itemsize
    pitch = -(-inner // al) * al + al
    buf = torch.full((a.shape[0] * pitch,), float("nan"), dtype=_torch_dtype(a), device=device)
    dense = [int(np.prod(a.shape[d + 1:])) for d in range(1, a.ndim)]
    view = torch.as_strided(buf, a.shape, [pitch] + dense, 0)
    view.copy_(torch.from_numpy(a).to(device))
    return view


def byte_runs(arena, view):
    """A uint8 view of the arena over the bytes ``view`` (2-D or 3-D, innermost dimension dense or a 2-D view with one unit
    stride) covers, one row per run, padding between the elements of a run included."""
    import torch

    isz = view.element_size()
    start = view.data_ptr() - arena.data_ptr()
    dims = sorted(zip(view.stride(), view.shape))  # the far dimension last
    stride, count = dims[-1]
    run = sum(st * (n - 1) for st, n in dims[:-1]) + 1
    assert run <= stride and run * isz <= 2 ** 26, "one far dimension only"
    assert start >= 0 and start + ((count - 1) * stride + run) * isz <= arena.numel()
    return torch.as_strided(arena, (count, run * isz), (stride * isz, 1), start)


def repoison(arena, *views):
    """Fill what the views cover with 0xFF again."""
    for v in views:
        byte_runs(arena, v).fill_(0xFF)


def twin(a, kind, device="cuda"):
    """``a`` on the device in a small buffer of the far view's layout class: pitch ``S + 16 / itemsize``, or ``S + 1`` with the
    pointer moved by one element (``S`` rounded up to a multiple of ``16 / itemsize`` first, so that the pitch is a multiple of
    16 bytes, or one element more, as the far one is), the same for lines, ``(2 S + 2, 2)`` for ``both``.  The padding is NaN."""
    import torch

    a = np.ascontiguousarray(a)
    n, s = a.shape
    al = 16 // a.itemsize
    odd = int(kind.endswith("_odd"))
    if kind in ("rows", "rows_odd"):
        strides = (-(-s // al) * al + (1 if odd else al), 1)
    elif kind in ("lines", "lines_odd"):
        strides = (1, -(-n // al) * al + (1 if odd else al))
    elif kind == "both":
        strides = (2 * s + 2, 2)
    else:
        raise ValueError(f"unknown kind {kind!r}")
    size = odd + (n - 1) * strides[0] + (s - 1) * strides[1] + 1
    buf = torch.full((size + al,), float("nan"), dtype=_torch_dtype(a), device=device)
    view = torch.as_strided(buf, (n, s), strides, odd)
    view.copy_(torch.from_numpy(a).to(device))
    return view


# --------------------------------------------------------------------------------------------------------------
F4, F8 = "float32", "float64"
LC = CHUNK  # lfo_chunk_rows() of csrc/pla_k_lfo.hip, restated by tests/lfo_ref.py
# elements between the far views of one case (e_loo: x, log_weights, log_ratios): 2^20, and 64 more, since 2^20 itself is a multiple of
# the line pitch of the (9, 4100) views (2^18 doubles) and would lay the lines of one view on those of the other
SECOND = 2 ** 20 + 64

# ---- the shapes of every test of tests/test_gpu_far_offsets.py: (n, s, dtype, kind); tests/test_far_views_host.py proves the layout
# properties of each
PSIS_ROWS = [(9, 1000, dt, k) for dt in (F4, F8) for k in ("rows", "rows_odd")] + [(9, 4224, F8, k) for k in ("rows", "rows_odd")]
PSIS_LINES = [(70, 527, F4, "lines"), (70, 527, F8, "lines")]
WEIGHTS = [(9, 1000, dt, k) for dt in (F4, F8) for k in ("rows", "lines")] + [(9, 4224, F8, k) for k in ("rows", "lines")]
WAIC = [(9, s, dt, k) for s in (257, 1000, 4100) for dt in (F4, F8) for k in ("rows", "rows_odd", "lines")]
DIAG = [(9, 1000, dt, k) for dt in (F4, F8) for k in ("rows", "lines")]
# (66 rows, 258 lines: an even count puts one whole row or line past 2^33 bytes, so that for f32 a row START leaves 31 bits too)
MIXIS = ([(66, 257, dt, k) for dt in (F8, F4) for k in ("rows", "rows_odd", "both")] + [(66, 258, dt, "lines") for dt in (F8, F4)]
         + [(66, 204, dt, "lines_odd") for dt in (F8, F4)]
         + [(9, 4100, dt, "rows") for dt in (F8, F4)])
E_LOO = [(9, 1000, dt, k) for dt in (F8, F4) for k in ("rows", "rows_odd", "lines")] + [(9, 4100, F8, k) for k in ("rows", "rows_odd", "lines")]
PIT = [(17, 1000, dt, k) for dt in (F8, F4) for k in ("rows", "lines")]
LFO = [(2 * LC + 9, 257, dt, k) for dt in (F8, F4) for k in ("rows", "rows_odd", "lines")]
ESS = [(9, 1000, dt, k) for dt in (F8, F4) for k in ("rows", "lines")]
INFLUENCE = [(17, 1000, dt, k) for dt in (F8, F4) for k in ("rows", "lines")]
GROUPS = [(40, 1000, dt, k) for dt in (F8, F4) for k in ("rows", "lines")]
DRAWS = [(9, 1000, dt, k) for dt in (F8, F4) for k in ("rows", "lines")]
KFOLD = [(9, 500, dt, "rows") for dt in (F8, F4)]
KFOLD_SOURCES = ("rows", "lines", "both")  # the layouts of the three fold sources: the wave, lane and block routes of pla_kfold.h
PITCHED = {  # leading dimension x dense rest, the ``rows`` layout: what far_pitched builds
    "glm X": (33, 17, F8), "glm beta": (250, 17, F8), "theta": (1000, 21, F8),
    "nonfactor mat 17": (5, 17 * 17, F8), "nonfactor mu 17": (5, 17, F8), "nonfactor mat 150": (5, 150 * 150, F4), "nonfactor mu 150": (5, 150, F4),
    "nonfactor mat 150 f64": (5, 150 * 150, F8), "nonfactor mat 17 f32": (5, 17 * 17, F4), "nonfactor mu 17 f32": (5, 17, F4),
    "nonfactor mu 150 f64": (5, 150, F8),
    "compare f64": (3, 300, F8), "compare f32": (3, 300, F4), "mm x": (3, 257 * 17, F8),
}
TRANSPOSED = {"glm X.T": (33, 17, F8), "glm beta.T": (250, 17, F8), "theta.T": (1000, 21, F8)}  # the ``lines`` layout
# views used together in one case, as (n, s, dtype, kind, shift): they must not overlap
TOGETHER = ([[(n, s, dt, k, j * SECOND) for j in range(3)] for n, s, dt, k in E_LOO]
            + [[(9, 500, dt, "rows", 0)] + [(m, 500, dt, k, (j + 1) * SECOND // 2) for j, k in enumerate(KFOLD_SOURCES)]
               for dt in (F8, F4) for m in (9, 3)]
            + [[(9, 1000, dt, a, 0), (9, 1000, dt, b, 3 * SECOND // 2)] for dt in (F8, F4) for a, b in (("rows", "lines"), ("lines", "rows"))]
            + [[(17, 1000, dt, a, 0), (17, 1000, dt, b, 3 * SECOND // 2)] for dt in (F8, F4) for a, b in (("rows", "lines"), ("lines", "rows"))]
            + [[(17, 1000, F8, k, 0), (1000, 21, F8, tk, 2 * SECOND)] for k in ("rows", "lines") for tk in ("rows", "lines")]
            + [[(33, 17, F8, k, 0), (250, 17, F8, k, 2 * SECOND)] for k in ("rows", "lines")]
            + [[(5, n * n, dt, "rows", 0), (5, n, dt, "rows", 2 * SECOND)] for n, dt in ((17, F8), (17, F4), (150, F8), (150, F4))])


def all_layouts():
    """Every (n, s, itemsize, kind) this file builds a far view of."""
    out = set()
    for group in (PSIS_ROWS, PSIS_LINES, WEIGHTS, WAIC, DIAG, MIXIS, E_LOO, PIT, LFO, ESS, INFLUENCE, GROUPS, DRAWS, KFOLD, [(m, 500, dt, k) for m in (9, 3) for dt in (F8, F4) for k in KFOLD_SOURCES]):
        out |= {(n, s, np.dtype(dt).itemsize, k) for n, s, dt, k in group}
    out |= {(m, inner, np.dtype(dt).itemsize, "rows") for m, inner, dt in PITCHED.values()}
    out |= {(m, inner, np.dtype(dt).itemsize, "lines") for m, inner, dt in TRANSPOSED.values()}
    return sorted(out)
