"""``gather_draws_kernel`` (csrc/pla_draws.h) at the row lengths, index lengths, pitches and base addresses where its routes and
vector legs change.  Every value is compared bit for bit with ``ll[:, idx]`` (tests/group_gather_ref.py), every NaN count exactly,
and ``Engine.last_kernels()`` has to name the route and the vector leg the case is aimed at.  No tolerances.

=====================================================================  ===========================================================
branch                                                                 test
=====================================================================  ===========================================================
the LDS staging: 16-byte loads of n_draws / VEC vectors, then the      test_lds_legs: pitched views whose pitch is a multiple of
element tail loop; VEC = 1 from the base of `in` or `out`, the pitch,  VEC and whose row is not (the tail holds NaN and is
or n_out % VEC != 0                                                    gathered), odd pitches, bases 8 / 4 bytes off, `out=` too
the index loop over 512 threads, vectors of VEC outputs                test_index_length_around_the_workgroup: n_out = 1..4 and
                                                                       around 512 and 1024, on <lds+index> and <global>
row + 32-bit index within 80 KB: <lds+index>, else <lds>               test_lds_budget_boundary: n_out = fit, fit + 1, fit + VEC
rows strided over a grid of 2048 workgroups, the barrier between rows  test_rows_over_the_grid: N = 2047 .. 4097
64 x 16 tiles, both remainders; one row is no tile                     test_tile_remainders: N and n_out around the tile, a
                                                                       pitched observations-fastest view, N = 1 on <global>
=====================================================================  ===========================================================
"""

import numpy as np
import pytest

import group_gather_ref as ref

pytestmark = pytest.mark.gpu

VEC = {np.float64: 2, np.float32: 4}
WIDE, ELEMENT = "16-byte loads", "element loads"
LDS_IDX, LDS, GLOBAL, TILE = ("gather_draws_kernel<%s>" % r for r in ("lds+index", "lds", "global", "tile"))


@pytest.fixture(scope="module")
def eng():
    from pyloo_amd.engine import get_engine

    return get_engine(0)


def matrix(N, S, dt, seed, nan_columns=()):
    """Random values, +-inf in the first row, NaN in every other row of ``nan_columns`` and at a few random places."""
    rng = np.random.default_rng(seed)
    ll = (rng.normal(size=(N, S)) * rng.uniform(0.1, 50, size=(N, 1))).astype(dt)
    ll[rng.random((N, S)) < 0.02] = np.nan
    for c in nan_columns:
        ll[::2, c] = np.nan
    ll[0, 0], ll[0, S - 1] = np.inf, -np.inf
    return ll


def check(eng, src, ll, idx, route, leg=None, out=None):
    """One gather_draws call on a device matrix against the reference: values, count, route text."""
    import torch

    got, nrep = eng.gather_draws(src, torch.as_tensor(np.asarray(idx, dtype=np.int64)).cuda(), out=out)
    text = eng.last_kernels()
    want, n_nan = ref.gather(ll, idx)
    what = (tuple(ll.shape), len(idx), text)
    assert route + " " in text and text.endswith("(matrix read in place)"), what
    assert (leg is None and "loads" not in text) or (leg is not None and text.count("loads") == 1 and leg in text), what
    if out is not None:
        assert got is out
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (what, np.argwhere(got != want)[:5])
    assert int(nrep.item()) == n_nan, (what, int(nrep.item()), n_nan)
    return n_nan


def pitched(ll, pitch):
    """``buf[:, :S]`` of a NaN-filled (N, pitch) buffer: a read past a row's end would be a counted NaN"""
    import torch

    buf = torch.full((ll.shape[0], pitch), float("nan"), dtype=torch.as_tensor(ll).dtype, device="cuda")
    view = buf[:, :ll.shape[1]]
    view.copy_(torch.as_tensor(ll))
    assert view.stride() == (pitch, 1) and view.data_ptr() % 16 == 0
    return view


def off_base(shape, dt):
    """A contiguous NaN-filled tensor of ``shape`` whose base lies one element behind a 16-byte boundary"""
    import torch

    flat = torch.full((int(np.prod(shape)) + 1,), float("nan"), dtype=torch.as_tensor(np.zeros(1, dtype=dt)).dtype, device="cuda")
    t = flat[1:].view(*shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == np.dtype(dt).itemsize
    return t


# ---------------------------------------------------------------------------------------------------- pitched and unaligned LDS legs
#           dtype, S, what (a pitch, "base": `in` one element off, "out": `out=` one element off), the leg when n_out % VEC == 0
LDS_CASES = [(np.float64, 131, 134, WIDE), (np.float64, 130, 133, ELEMENT), (np.float64, 131, 133, ELEMENT), (np.float64, 130, "base", ELEMENT),
             (np.float64, 130, "out", ELEMENT), (np.float32, 257, 264, WIDE), (np.float32, 258, 264, WIDE), (np.float32, 259, 264, WIDE),
             (np.float32, 256, 262, ELEMENT), (np.float32, 256, "base", ELEMENT), (np.float32, 256, "out", ELEMENT)]


@pytest.mark.parametrize("dt,S,how,leg", LDS_CASES, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_lds_legs(eng, dt, S, how, leg):
    import torch

    N, vec = 5, VEC[dt]
    tail = list(range(S - S % vec, S)) or [S - 1]  # the elements behind the last whole vector of a row
    ll = matrix(N, S, dt, S, nan_columns=tail + [7])
    rng = np.random.default_rng(S + 1)
    for n_out in (S + vec - S % vec, S + vec - S % vec + 1, vec, 1):
        idx = rng.integers(0, S, size=n_out)
        idx[:len(tail) + 2][:n_out] = (tail + [7, 0])[:n_out]  # the tail and the NaN column are gathered
        if how == "out":
            src, out = torch.as_tensor(ll).cuda(), off_base((N, n_out), dt)
        else:
            src, out = (off_base((N, S), dt) if how == "base" else pitched(ll, how)), None
            if how == "base":
                src.copy_(torch.as_tensor(ll))
        n_nan = check(eng, src, ll, idx, LDS_IDX, leg if n_out % vec == 0 else ELEMENT, out=out)
        assert n_nan > 0


# ---------------------------------------------------------------------------------------------------- index length around the workgroup
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_index_length_around_the_workgroup(eng, dt):
    import torch

    N, S = 5, 64
    ll = matrix(N, S, dt, 11)
    dense = torch.as_tensor(ll).cuda()
    wide = torch.full((N, 2 * S), float("nan"), dtype=dense.dtype, device="cuda")
    both_strided = wide[:, ::2]  # neither stride is 1
    both_strided.copy_(dense)
    assert both_strided.stride() == (2 * S, 2)
    rng = np.random.default_rng(12)
    for n_out in (1, 2, 3, 4, 511, 512, 513, 1023, 1024, 1025):
        idx = rng.integers(0, S, size=n_out)
        idx[0], idx[-1] = S - 1, 0  # the infinities of the first row, at both ends of the index
        check(eng, dense, ll, idx, LDS_IDX, WIDE if n_out % VEC[dt] == 0 else ELEMENT)
        check(eng, both_strided, ll, idx, GLOBAL)


# ---------------------------------------------------------------------------------------------------- LDS budget boundary
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_lds_budget_boundary(eng, dt):
    import torch

    N, S = 3, 4096
    fit = (80 * 1024 - S * np.dtype(dt).itemsize) // 4  # the longest index that fits beside the row
    assert fit % VEC[dt] == 0
    ll = matrix(N, S, dt, 21)
    dense = torch.as_tensor(ll).cuda()
    rng = np.random.default_rng(22)
    for n_out, route, leg in ((fit, LDS_IDX, WIDE), (fit + 1, LDS, ELEMENT), (fit + VEC[dt], LDS, WIDE), (fit - 1, LDS_IDX, ELEMENT)):
        idx = rng.integers(0, S, size=n_out)
        idx[-1] = S - 1
        assert check(eng, dense, ll, idx, route, leg) > 0


# ---------------------------------------------------------------------------------------------------- rows over the grid
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N", [2047, 2048, 2049, 4097])
def test_rows_over_the_grid(eng, dt, N):
    """More rows than the 2048 workgroups of the LDS routes: a workgroup takes rows b, b + 2048, b + 4096."""
    import torch

    S = 8
    ll = matrix(N, S, dt, N)
    ll[:, 0] = np.arange(N)  # every row differs from every other
    dense = torch.as_tensor(ll).cuda()
    rng = np.random.default_rng(N + 1)
    for n_out in (12, 13):
        check(eng, dense, ll, rng.integers(0, S, size=n_out), LDS_IDX, WIDE if n_out % VEC[dt] == 0 else ELEMENT)
    if dt == np.float32 and N in (2048, 2049):  # <lds>: an index that does not fit beside the row (f32 keeps the output at 168 MB)
        n_out = (80 * 1024 - S * 4) // 4 + 4
        check(eng, dense, ll, rng.integers(0, S, size=n_out), LDS, WIDE)


# ---------------------------------------------------------------------------------------------------- tile route remainders
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N", [2, 63, 64, 65, 129])
def test_tile_remainders(eng, dt, N):
    import torch

    S = 40
    ll = matrix(N, S, dt, 100 + N)
    flipped = torch.as_tensor(np.ascontiguousarray(ll.T)).cuda()
    obs = flipped.T
    buf = torch.full((S, N + 7), float("nan"), dtype=flipped.dtype, device="cuda")
    pitched_obs = buf[:, :N].T  # observations fastest, stride_draw > N
    pitched_obs.copy_(obs)
    assert obs.stride() == (1, N) and pitched_obs.stride() == (1, N + 7)
    one = buf[:, :1].T  # the first observation alone, with those strides: no tile
    assert tuple(one.shape) == (1, S) and one.stride(1) == N + 7
    rng = np.random.default_rng(N)
    for n_out in (1, 15, 16, 17, 33):
        idx = rng.integers(0, S, size=n_out)
        idx[0] = S - 1
        check(eng, obs, ll, idx, TILE)
        check(eng, pitched_obs, ll, idx, TILE)
        check(eng, one, ll[:1], idx, GLOBAL)
