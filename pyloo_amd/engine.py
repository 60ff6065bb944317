"""Python handle on one ``pla_engine`` (one GPU) and the array plumbing around the C ABI.

Inputs may be NumPy arrays (host memory: the library stages them through the device) or
torch CUDA tensors (device memory: zero copies, work is enqueued on torch's current stream
and results come back as CUDA tensors).  torch is used only for device memory and streams.

Every method has one body.  What differs between the two kinds of memory -- pointers, allocation,
counters, index lists, the stream -- lives in a memory-space object (:class:`_HostSpace`,
:class:`_DeviceSpace`); how a matrix argument may lie in memory is a :class:`_Layout`, declared
once below and named by the method that uses it:

======================================  ============  =========================  =========================================
method                                  layout        host array taken in place  CUDA tensor taken in place
======================================  ============  =========================  =========================================
psis_loo, waic                          _LOO          draws- or obs-fastest (1)  draws- or obs-fastest (1)
group_sum, psis_loo_groups              _LOO          draws- or obs-fastest      draws- or obs-fastest
loo_diag, loo_influence(loglik)         _LOO_DIAG     draws- or obs-fastest (1)  draws- or obs-fastest (2)
lfo_ratios, lfo, relative_eff           _LFO          draws- or obs-fastest      the same, rows that overlap copied
importance_weights                      _WEIGHTS      draws-fastest              draws- or obs-fastest, unchecked (3)
mixis_*, gather_draws, psis_loo_draws   _IN_PLACE     draws- or obs-fastest      any strides
loo_influence(log_weights)              _LOG_WEIGHTS  draws-fastest              any positive strides
e_loo, e_loo_quantiles                  promoted      contiguous copies          equal strides, else contiguous copies (4)
loo_pit                                 promoted      draws- or obs-fastest      own positive strides
loo_diag_weights                        promoted      draws-fastest              own positive strides
======================================  ============  =========================  =========================================

(1) with ``rows`` only draws-fastest.  (2) also with ``rows``.  (3) neither the dimensions, the device nor the dtype of
the tensor is checked.  (4) the tensors are not checked for being CUDA tensors; the other promoted pairs are.
Any other layout is copied.  ``stride_obs`` of a one-row CUDA tensor is passed as torch reports it (_LOO, _WEIGHTS,
_IN_PLACE, promoted), as ``n_draws`` (_LFO) or as ``max(n_draws, 1)`` (_LOO_DIAG, _LOG_WEIGHTS); of a one-row host array
always as ``n_draws``.

Outputs: the pointwise vectors of psis_loo, waic, psis_loo_groups, psis_loo_draws and glm(mode="loo") are allocated for
``pointwise``, on the device also for ``aggregate`` alone.  ``agg`` is zero-filled by waic, reduce_pointwise and mixis_loo
in both spaces, by psis_loo, psis_loo_groups and psis_loo_draws on the host only, by glm and kfold nowhere.  The Mix-IS,
lfo and relative_eff vectors are zero-filled, every other output is uninitialised memory for the library to write.
"""

import collections
import ctypes as C
import threading

import numpy as np

from . import _capi
from ._capi import AGG_COUNT, METHOD_CODES, PLA_DEVICE, PLA_HOST, check, dtype_code, load_library

_engines = {}
_lock = threading.Lock()


def _is_torch_tensor(a):
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")


def _host(a):
    """An array or a tensor (of any device) as an ndarray."""
    return a.detach().cpu().numpy() if _is_torch_tensor(a) else np.asarray(a)


def _ptr(x):
    """The address of an array or tensor, None for None (a ``void *`` argument or struct entry)."""
    if x is None:
        return None
    return x.data_ptr() if _is_torch_tensor(x) else x.ctypes.data


def _code(x):
    """The dtype code of an array or tensor (a tensor that is not float64 counts as float32)."""
    if _is_torch_tensor(x):
        import torch

        return _capi.PLA_F64 if x.dtype == torch.float64 else _capi.PLA_F32
    return dtype_code(x.dtype)


def _of_length(v, n, what):
    if n is not None and len(v) != n:
        raise ValueError(what.format(n=n, got=len(v)))
    return v


# host_obs: a host array with the observations fastest is taken in place (never together with ``rows``); device: "library"
# (draws or observations fastest in place, else a copy), "positive" (any positive strides) or "in place" (any strides);
# sees_rows: ``rows`` rules out an observations-fastest CUDA tensor; one_row: stride_obs of a one-row CUDA tensor is
# max(n_draws, one_row), None: as torch reports it; no_overlap: rows of a CUDA tensor that overlap are copied apart;
# checked: a tensor must be 2-D, CUDA, f64 or f32.
_Layout = collections.namedtuple("_Layout", "host_obs device sees_rows one_row no_overlap checked", defaults=(False, None, False, True))
_LOO = _Layout(True, "library", sees_rows=True)
_LOO_DIAG = _Layout(True, "library", one_row=1)
_LFO = _Layout(True, "library", one_row=0, no_overlap=True)
_WEIGHTS = _Layout(False, "library", checked=False)
_IN_PLACE = _Layout(True, "in place")
_LOG_WEIGHTS = _Layout(False, "positive", one_row=1)


def _host_obs_fastest(a):
    n, s = a.shape
    return n > 1 and s > 1 and a.strides[0] == a.itemsize and a.strides[1] % a.itemsize == 0 and a.strides[1] >= n * a.itemsize


def _as_2d_host(a, allow_obs_fastest=False):
    a = np.asarray(a)
    if a.dtype not in (np.float64, np.float32):
        a = a.astype(np.float64)
    if a.ndim != 2:
        raise ValueError("expected a 2-D (n_obs, n_draws) array")
    if allow_obs_fastest and _host_obs_fastest(a):
        return a  # a (chain, draw, *obs) buffer viewed as (obs, sample): the library takes it as it is
    if a.shape[1] > 1 and a.strides[1] != a.itemsize:
        a = np.ascontiguousarray(a)
    if a.shape[0] > 1 and (a.strides[0] % a.itemsize != 0 or a.strides[0] < 0):
        a = np.ascontiguousarray(a)
    return a


def _host_strides(a):
    """(stride_obs, stride_draw) in elements of a host matrix prepared by :func:`_as_2d_host`."""
    n, s = a.shape
    if _host_obs_fastest(a):
        return 1, a.strides[1] // a.itemsize
    return (a.strides[0] // a.itemsize if n > 1 else s), 1


def _host_rows(rows, n_obs):
    """Index list as contiguous int64, range-checked like NumPy indexing would (no negative wrap-around:
    loo_subsample.py:266-271 rejects indices outside [0, n))."""
    idx = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n_obs):
        raise IndexError(f"row indices must lie in [0, {n_obs}), got range [{idx.min()}, {idx.max()}]")
    return idx


def _host_draws(draw_index, n_draws):
    """Draw index as contiguous int64, range-checked like :func:`_host_rows` (no negative wrap-around)."""
    idx = np.ascontiguousarray(np.asarray(draw_index).reshape(-1), dtype=np.int64)
    if idx.size == 0:
        raise ValueError("draw_index is empty")
    if idx.min() < 0 or idx.max() >= n_draws:
        raise IndexError(f"draw indices must lie in [0, {n_draws}), got range [{idx.min()}, {idx.max()}]")
    return idx


def _draws_fastest(t):
    """ArviZ keeps log-likelihoods as (chain, draw, *obs): the (obs, sample) view of such a buffer has the
    observations fastest.  The entry points of the library take that layout as it is (a tiled transpose kernel
    feeds the row kernels block by block); this copy is only for layouts the library would walk with strides
    (if the copy does not fit, the strided general kernel takes them)."""
    import torch

    if t.dim() == 2 and t.shape[1] > 1 and t.stride(1) != 1:
        try:
            return t.contiguous()
        except torch.OutOfMemoryError:  # pragma: no cover - needs a nearly full device
            return t
    return t


def _library_layout(t, rows=None):
    """Layouts the library reads fast without a copy: draws fastest, or observations fastest (stride 1 along
    the observations, no row selection); anything else goes through :func:`_draws_fastest`."""
    if t.dim() == 2 and t.shape[0] > 1 and t.shape[1] > 1 and t.stride(0) == 1 and t.stride(1) >= t.shape[0] and rows is None:
        return t
    return _draws_fastest(t)


class _HostSpace:
    """Host memory: NumPy arrays, which the library stages through the device.  Counters are one int64 passed by pointer
    and read back as ``int``; index lists are range-checked."""

    mem_space, stream, device = PLA_HOST, None, None
    ptr, rows, draws, strides = staticmethod(_ptr), staticmethod(_host_rows), staticmethod(_host_draws), staticmethod(_host_strides)

    @staticmethod
    def new(shape, dtype="float64", zero=False):
        return (np.zeros if zero else np.empty)(shape, dtype=dtype)

    def counter(self):
        return self.new(1, "int64", zero=True)

    @staticmethod
    def read(counter):
        return int(counter[0])

    @staticmethod
    def f64(x):
        return np.asarray(x, dtype=np.float64)

    @staticmethod
    def vector(v, n=None, what="", dtype="float64"):
        """``v`` as a contiguous 1-D array (None stays None) of ``n`` values, else ``ValueError(what)``."""
        return None if v is None else _of_length(np.ascontiguousarray(np.asarray(v, dtype=dtype).reshape(-1)), n, what)

    @staticmethod
    def index(index):
        """(offsets, members) of a GroupIndex as contiguous int64 arrays."""
        return tuple(np.ascontiguousarray(_host(a), dtype=np.int64) for a in (index.offsets, index.members))

    @staticmethod
    def matrix(a, layout, rows):
        a = _as_2d_host(a, layout.host_obs and rows is None)
        return (a, *_host_strides(a))

    @staticmethod
    def dense(a):
        """A (rows, P) matrix and its strides: as it lies, as the ``.T`` view of a dense (P, rows) array, else a copy."""
        if a.flags.c_contiguous:
            return a, (a.shape[1], 1)
        if a.T.flags.c_contiguous:
            return a, (1, a.shape[0])
        return np.ascontiguousarray(a), (a.shape[1], 1)

    @staticmethod
    def promoted(mats, names, own_strides, host_obs):
        mats = [np.asarray(m) for m in mats]
        if any(m.ndim != 2 or m.shape != mats[0].shape for m in mats):
            raise ValueError(f"{names} must be 2-D arrays of one shape")
        dt = np.float32 if all(m.dtype == np.float32 for m in mats) else np.float64
        if not own_strides:
            return [np.ascontiguousarray(m, dtype=dt) for m in mats]
        return [_as_2d_host(m if m.dtype == dt else m.astype(dt), host_obs) for m in mats]


class _DeviceSpace:
    """The memory of one GPU: CUDA tensors, read in place; work goes onto torch's current stream and nothing is
    synchronised.  Counters are one-element int64 tensors and come back as they are; index lists that are CUDA tensors
    already are trusted (the kernels clamp)."""

    mem_space = PLA_DEVICE
    ptr = staticmethod(_ptr)

    def __init__(self, engine, device):
        self._engine, self.device = engine, device

    @property
    def stream(self):
        return self._engine._stream().value

    def new(self, shape, dtype="float64", zero=False):
        import torch

        return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, dtype) if isinstance(dtype, str) else dtype,
                                                      device=self.device)

    def counter(self):
        return self.new(1, "int64", zero=True)

    @staticmethod
    def read(counter):
        return counter

    def f64(self, x):
        import torch

        return torch.as_tensor(x, device=self.device).to(torch.float64)

    def vector(self, v, n=None, what="", dtype="float64"):
        import torch

        if v is None:
            return None
        return _of_length(torch.as_tensor(v, device=self.device).to(getattr(torch, dtype)).reshape(-1).contiguous(), n, what)

    def rows(self, rows, n_obs):
        import torch

        if _is_torch_tensor(rows):  # already on the device: the kernels clamp, the caller vouches for the range
            return rows.to(device=self.device, dtype=torch.int64).contiguous().reshape(-1)
        return torch.from_numpy(_host_rows(rows, n_obs)).to(self.device)

    def draws(self, draw_index, n_draws):
        import torch

        if _is_torch_tensor(draw_index) and draw_index.is_cuda:  # used as it is: the kernel clamps, the caller vouches for the range
            idx = draw_index.to(device=self.device, dtype=torch.int64).contiguous().reshape(-1)
            if idx.numel() == 0:
                raise ValueError("draw_index is empty")
            return idx
        if _is_torch_tensor(draw_index):
            draw_index = draw_index.numpy()
        return torch.from_numpy(_host_draws(draw_index, n_draws)).to(self.device)

    def index(self, index):
        import torch

        return tuple((a if _is_torch_tensor(a) else torch.from_numpy(np.asarray(a))).to(device=self.device, dtype=torch.int64).contiguous()
                     for a in (index.offsets, index.members))

    @staticmethod
    def strides(t):
        return t.stride()

    @staticmethod
    def matrix(t, layout, rows):
        import torch

        if layout.checked:
            if t.dim() != 2 or not t.is_cuda:
                raise ValueError("expected a 2-D CUDA tensor")
            if t.dtype not in (torch.float64, torch.float32):
                raise TypeError(f"unsupported dtype {t.dtype}")
        if layout.device == "library":
            t = _library_layout(t, rows if layout.sees_rows else None)
            if layout.no_overlap and t.shape[1] > 1 and t.stride(1) == 1 and t.shape[0] > 1 and t.stride(0) < t.shape[1]:
                t = t.contiguous()  # (rows that overlap: an expanded tensor)
        elif layout.device == "positive" and min(t.stride()) <= 0:
            t = t.contiguous()
        n, s = t.shape
        return t, (t.stride(0) if n > 1 or layout.one_row is None else max(s, layout.one_row)), t.stride(1)

    @staticmethod
    def dense(t):
        t = t if min(t.stride()) > 0 else t.contiguous()
        return t, t.stride()

    @staticmethod
    def promoted(mats, names, own_strides, host_obs):
        import torch

        if (any(not _is_torch_tensor(m) or m.dim() != 2 or m.shape != mats[0].shape for m in mats)
                or (own_strides and not all(m.is_cuda for m in mats))):
            raise ValueError(f"{names} must be 2-D CUDA tensors of one shape")
        dt = torch.float64 if any(m.dtype == torch.float64 for m in mats) else torch.float32
        mats = [m.to(dt) for m in mats]
        if own_strides:
            return [m if min(m.stride()) > 0 else m.contiguous() for m in mats]
        if any(m.stride() != mats[0].stride() for m in mats) or mats[0].stride(1) <= 0:
            mats = [m.contiguous() for m in mats]
        return mats


_HOST = _HostSpace()


def _pointwise(sp, m, pointwise, aggregate, count=3):
    """The pointwise outputs of a LOO-type pass; a device pass takes them for the aggregate alone too."""
    if pointwise or (aggregate and sp.device is not None):
        return [sp.new(m) for _ in range(count)]
    return [None] * count


class Engine:
    """One engine per (process, device).  Use :func:`get_engine`."""

    def __init__(self, device=0):
        lib = load_library()
        n = _capi.device_count()
        if n <= 0:
            raise RuntimeError(
                "pyloo_amd needs an AMD GPU (MI355X / gfx950): no HIP device is visible. "
                "There is no CPU fallback."
            )
        h = C.c_void_p()
        check(lib.pla_engine_create(int(device), C.byref(h)))
        self._lib = lib
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pla_engine_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        import torch

        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    _host_draws = staticmethod(_host_draws)

    def _space(self, x):
        """The memory space of an input: the device of a tensor, the host for anything else."""
        return _DeviceSpace(self, x.device) if _is_torch_tensor(x) else _HOST

    def _matrix(self, x, layout, rows=None):
        """An (n_obs, n_draws) matrix argument under ``layout`` -> ``(space, matrix, (dtype code, n_obs, n_draws, stride_obs,
        stride_draw))``: the matrix as the library is to read it (to be kept alive over the call) and the five arguments that
        follow its pointer in every entry point."""
        sp = self._space(x)
        a, so, sd = sp.matrix(x, layout, rows)
        return sp, a, (_code(a), a.shape[0], a.shape[1], so, sd)

    def _promoted(self, mats, names, own_strides, host_obs=False):
        """Two or three matrices of one shape, promoted to one dtype (f64 if any is) -> ``(space, matrices, dtype code, n_obs,
        n_draws)``.  ``own_strides``: each keeps its layout and is passed with ``space.strides`` of its own; otherwise all share
        the strides of the first."""
        sp = self._space(mats[0])
        mats = sp.promoted(mats, names, own_strides, host_obs)
        return sp, mats, _code(mats[0]), mats[0].shape[0], mats[0].shape[1]

    # ------------------------------------------------------------------ LOO pass
    def psis_loo(self, ll, tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True,
                 rows=None):
        """Fused pass over an (n_obs, n_draws) log-likelihood matrix (``pla_psis_loo``).

        Returns ``dict(diag, loo_i, lppd_i, agg)`` -- NumPy arrays for NumPy input, CUDA tensors
        for CUDA-tensor input (``agg`` included; nothing is synchronised in that case).
        ``rows``: optional observation indices; the pass then runs over those rows only
        (``pla_psis_loo_rows``) and the outputs have one entry per index.
        """
        mcode = METHOD_CODES[method]
        sp, a, dims = self._matrix(ll, _LOO, rows)
        idx = None if rows is None else sp.rows(rows, dims[1])
        m = dims[1] if idx is None else len(idx)
        diag, loo_i, lppd_i = _pointwise(sp, m, pointwise, aggregate)
        agg = sp.new(AGG_COUNT, zero=sp.device is None) if aggregate else None  # (the device pass writes every slot)
        p = sp.ptr
        tail = (mcode, int(tail_count), float(scale_value), float(good_k), sp.mem_space, sp.stream, p(diag), p(loo_i), p(lppd_i), p(agg))
        if idx is None:
            check(self._lib.pla_psis_loo(self._h, p(a), *dims, *tail))
        else:
            check(self._lib.pla_psis_loo_rows(self._h, p(a), *dims, p(idx), m, *tail))
        return {"diag": diag, "loo_i": loo_i, "lppd_i": lppd_i, "agg": agg}

    # ------------------------------------------------------------------ leave-one-group-out
    def group_sum(self, ll, index):
        """(n_obs, n_draws) matrix + :class:`~pyloo_amd.loo_group.GroupIndex` -> ``(sums, n_replaced)`` (``pla_group_sum``):
        ``sums[g]`` = the rows of group g's members added in ascending order, in the matrix's dtype (bitwise NumPy's
        ``ll[members].sum(axis=0)``), NaN counted as -1e10.  NumPy in -> ``(ndarray, int)``; CUDA tensor in -> ``(tensor, int64
        tensor of one element)``, nothing synchronised."""
        G = int(index.n_groups)
        sp, a, dims = self._matrix(ll, _LOO)
        off, mem = sp.index(index)
        out = sp.new((G, dims[2]), a.dtype)
        nrep = sp.counter()
        p = sp.ptr
        check(self._lib.pla_group_sum(self._h, p(a), *dims, p(off), p(mem), G, sp.mem_space, sp.stream, p(out), p(nrep)))
        return out, sp.read(nrep)

    def psis_loo_groups(self, ll, index, tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True):
        """Leave-one-group-out pass (``pla_psis_loo_groups``): group sums, then the PSIS / SIS / TIS pass over them.

        Returns ``dict(diag, logo_i, lppd_i, agg, n_replaced)`` with one pointwise entry per group -- NumPy arrays (and an int)
        for NumPy input, CUDA tensors for CUDA-tensor input (nothing synchronised)."""
        mcode = METHOD_CODES[method]
        G = int(index.n_groups)
        sp, a, dims = self._matrix(ll, _LOO)
        off, mem = sp.index(index)
        diag, logo_i, lppd_i = _pointwise(sp, G, pointwise, aggregate)
        agg = sp.new(AGG_COUNT, zero=sp.device is None) if aggregate else None
        nrep = sp.counter()
        p = sp.ptr
        check(self._lib.pla_psis_loo_groups(self._h, p(a), *dims, p(off), p(mem), G, mcode, int(tail_count), float(scale_value),
                                            float(good_k), sp.mem_space, sp.stream, p(diag), p(logo_i), p(lppd_i), p(agg), p(nrep)))
        return {"diag": diag, "logo_i": logo_i, "lppd_i": lppd_i, "agg": agg, "n_replaced": sp.read(nrep)}

    # ------------------------------------------------------------------ approximate posteriors: draws through an index
    def gather_draws(self, ll, draw_index, out=None):
        """(n_obs, n_draws) matrix + draw index -> ``(matrix, n_replaced)`` (``pla_gather_draws``): bitwise ``ll[:, draw_index]`` in
        the matrix's dtype, draws contiguous, NaN written as -1e10 and counted.  NumPy in -> ``(ndarray, int)``; CUDA tensor in ->
        ``(tensor, int64 tensor of one element)``, nothing synchronised.  ``out``: a contiguous CUDA tensor to write into."""
        sp, a, dims = self._matrix(ll, _IN_PLACE)
        n, s = dims[1:3]
        idx = sp.draws(draw_index, s)
        m = len(idx)
        if out is None or sp.device is None:
            out = sp.new((n, m), a.dtype)
        elif tuple(out.shape) != (n, m) or out.dtype != a.dtype or not out.is_contiguous() or out.device != a.device:
            raise ValueError("out must be a contiguous tensor of shape (n_obs, len(draw_index)) with the matrix's dtype and device")
        nrep = sp.counter()
        p = sp.ptr
        check(self._lib.pla_gather_draws(self._h, p(a), *dims, p(idx), m, sp.mem_space, sp.stream, p(out), p(nrep)))
        return out, sp.read(nrep)

    def psis_loo_draws(self, ll, draw_index, tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True):
        """PSIS / SIS / TIS pass over ``ll[:, draw_index]`` (``pla_psis_loo_draws``) without materialising that matrix: blocks of
        observations are gathered into the bounded staging buffer and passed on.  ``tail_count`` refers to ``len(draw_index)``.

        Returns ``dict(diag, loo_i, lppd_i, agg, n_replaced)`` -- NumPy arrays (and an int) for NumPy input, CUDA tensors for
        CUDA-tensor input (nothing synchronised)."""
        mcode = METHOD_CODES[method]
        sp, a, dims = self._matrix(ll, _IN_PLACE)
        idx = sp.draws(draw_index, dims[2])
        diag, loo_i, lppd_i = _pointwise(sp, dims[1], pointwise, aggregate)
        agg = sp.new(AGG_COUNT, zero=sp.device is None) if aggregate else None
        nrep = sp.counter()
        p = sp.ptr
        check(self._lib.pla_psis_loo_draws(self._h, p(a), *dims, p(idx), len(idx), mcode, int(tail_count), float(scale_value),
                                           float(good_k), sp.mem_space, sp.stream, p(diag), p(loo_i), p(lppd_i), p(agg), p(nrep)))
        return {"diag": diag, "loo_i": loo_i, "lppd_i": lppd_i, "agg": agg, "n_replaced": sp.read(nrep)}

    # ------------------------------------------------------------------ k-fold cross-validation
    @staticmethod
    def _kfold_host_matrix(a):
        a = a.detach().numpy() if _is_torch_tensor(a) else np.asarray(a)
        if a.ndim != 2:
            raise ValueError("expected 2-D (n_obs, n_draws) matrices")
        return a if a.dtype in (np.float64, np.float32) else a.astype(np.float64)

    @staticmethod
    def _kfold_upload(a, device, rows=None):
        """A host matrix on the device in the layout it has in memory (observations fastest stays so), cut to ``rows`` first."""
        import torch

        if _host_obs_fastest(a):
            base = a.T if rows is None else a.T[:, rows]
            return torch.from_numpy(np.ascontiguousarray(base)).to(device).T
        return torch.from_numpy(np.ascontiguousarray(a if rows is None else a[rows])).to(device)

    def kfold(self, ll_full, fold_log_liks, folds, scale_value=1.0, nan_flag=True):
        """K-fold cross-validation from per-fold log-likelihoods (``pla_kfold_lme`` + ``pla_kfold_reduce``).

        ``ll_full`` (N, S): the full fit.  ``fold_log_liks``: K matrices, matrix k (label k + 1) holding the held-out
        log-likelihood under fold k's draws, compact ``(n_val_k, S_k)`` with the rows in ascending observation order or full
        ``(N, S_k)`` (told apart by ``shape[0]``).  ``folds`` (N,): labels 1..K.  NumPy arrays or CUDA tensors of ONE float
        dtype; CUDA tensors are read in place through their strides, NumPy matrices are uploaded (full-form ones cut to their
        held-out rows first).  The task index is built with torch on the device: the observations in a stable sort by fold.
        Host ``folds`` are checked (labels 1..K, the rows of a compact matrix = the size of its fold: ``ValueError``); ``folds``
        given as a CUDA tensor are TRUSTED, so that nothing synchronises: labels outside 1..K are clamped and a compact matrix
        of the wrong height is read with clamped rows -- memory-safe, but the caller vouches for them (the fronts of
        ``pyloo_amd.loo_kfold`` check on the host first).

        Returns ``dict(elpd_i, lpd_full_i, p_i, kfold_i, agg)``: CUDA tensors when ``ll_full`` is one (nothing synchronised),
        ndarrays otherwise.  ``agg`` as documented at ``pla_kfold_reduce``; ``nan_flag``: NaN of the full fit counts as -1e10."""
        plan = self._kfold_plan(ll_full, fold_log_liks, folds)
        out, nrep = self._kfold_lme(plan, nan_flag)
        return self._kfold_finish(plan, out, nrep, scale_value)

    def _kfold_plan(self, ll_full, fold_log_liks, folds):
        """The matrices on the device, the task index and the source table of one :meth:`kfold` call."""
        import torch

        mats = [ll_full] + list(fold_log_liks)
        K = len(mats) - 1
        if K < 1:
            raise ValueError("need at least one fold matrix")
        on_device = [_is_torch_tensor(m) and m.is_cuda for m in mats]
        mats = [m if d else self._kfold_host_matrix(m) for m, d in zip(mats, on_device)]
        if any(m.ndim != 2 for m in mats):
            raise ValueError("expected 2-D (n_obs, n_draws) matrices")
        kinds = {str(m.dtype).split(".")[-1] for m in mats}
        if len(kinds) != 1 or not kinds <= {"float32", "float64"}:
            raise TypeError(f"the full and the fold matrices must share one dtype, float64 or float32; got {sorted(kinds)}")
        f32 = kinds == {"float32"}
        N = int(mats[0].shape[0])
        if N < 1 or any(int(m.shape[1]) < 1 for m in mats):
            raise ValueError("empty matrix")
        dev = next((m.device for m, d in zip(mats, on_device) if d), torch.device("cuda", self.device))
        full_form = [int(m.shape[0]) == N for m in mats[1:]]
        folds_dev = _is_torch_tensor(folds) and folds.is_cuda
        fh = None
        if not folds_dev or any(f and not d for f, d in zip(full_form, on_device[1:])):
            fh = _host(folds).reshape(-1).astype(np.int64)
            if fh.size != N:
                raise ValueError(f"Length of folds ({fh.size}) must match observations ({N})")
            if fh.min() < 1 or fh.max() > K:
                raise ValueError("Fold indices must be the integers 1..K")
            counts_h = np.bincount(fh - 1, minlength=K)
            for k, m in enumerate(mats[1:]):
                if not full_form[k] and int(m.shape[0]) != counts_h[k]:
                    raise ValueError(f"fold {k + 1}: matrix has {int(m.shape[0])} rows, expected {counts_h[k]} (held-out) or {N} (full form)")
        for k in range(K):  # host matrices go up, full-form ones as their held-out rows only
            if not on_device[k + 1]:
                rows = np.where(fh == k + 1)[0] if full_form[k] else None
                mats[k + 1] = self._kfold_upload(mats[k + 1], dev, rows)
                full_form[k] = False
        if not on_device[0]:
            mats[0] = self._kfold_upload(mats[0], dev)
        f = folds.to(device=dev, dtype=torch.int64).reshape(-1) if folds_dev else torch.from_numpy(fh).to(dev)
        if f.numel() != N:
            raise ValueError(f"Length of folds ({f.numel()}) must match observations ({N})")
        # ---- the task index: source 0 takes every observation, source k the observations of fold k in ascending order
        ar = torch.arange(N, dtype=torch.int64, device=dev)
        order = torch.argsort(f, stable=True)
        lab = (f[order] - 1).clamp_(0, K - 1)
        counts = torch.bincount(lab, minlength=K)[:K]
        ends = torch.cumsum(counts, 0)
        pos = ar - (ends - counts)[lab]
        is_full = torch.tensor(full_form, dtype=torch.bool).to(dev)
        task_row = torch.cat([ar, torch.where(is_full[lab], order, pos)])
        task_out = torch.cat([ar, order + N])
        offsets = torch.cat([torch.tensor([0, N], dtype=torch.int64).to(dev), ends + N])
        # ---- the source table (host arrays; the library uploads it)
        shp = lambda m, i: int(m.shape[i])  # noqa: E731
        base = np.array([m.data_ptr() for m in mats], dtype=np.uint64)
        n_rows = np.array([shp(m, 0) for m in mats], dtype=np.int64)
        n_draws = np.array([shp(m, 1) for m in mats], dtype=np.int64)
        for i, m in enumerate(mats):
            if (shp(m, 1) > 1 and m.stride(1) <= 0) or (shp(m, 0) > 1 and m.stride(0) < 0):
                mats[i] = m.contiguous()
                base[i] = mats[i].data_ptr()
        s_row = np.array([m.stride(0) if shp(m, 0) > 1 else 0 for m in mats], dtype=np.int64)
        s_draw = np.array([m.stride(1) if shp(m, 1) > 1 else 1 for m in mats], dtype=np.int64)
        return {"mats": mats, "N": N, "K": K, "f32": f32, "dev": dev, "host_out": not on_device[0], "offsets": offsets,
                "task_row": task_row, "task_out": task_out, "table": (base, n_rows, n_draws, s_row, s_draw)}

    def _kfold_lme(self, plan, nan_flag=True):
        """The ragged pass (``pla_kfold_lme``): ``(out, n_replaced)``, ``out[:N]`` the full fit's values, ``out[N:]`` the held-out ones."""
        N, sp = plan["N"], _DeviceSpace(self, plan["dev"])
        out = sp.new(2 * N)
        nrep = sp.counter()
        p = sp.ptr
        check(self._lib.pla_kfold_lme(self._h, *(p(a) for a in plan["table"]), plan["K"] + 1, _code(plan["mats"][0]),
                                      1 if nan_flag else 0, p(plan["offsets"]), p(plan["task_row"]), p(plan["task_out"]), 2 * N,
                                      sp.mem_space, sp.stream, p(out), 2 * N, p(nrep)))
        return out, nrep

    def _kfold_finish(self, plan, out, nrep, scale_value):
        """The finishing pass (``pla_kfold_reduce``) and the result dictionary of :meth:`kfold`."""
        N, sp = plan["N"], _DeviceSpace(self, plan["dev"])
        lpd_full_i, elpd_i = out[:N], out[N:]
        p_i, kfold_i, agg = sp.new(N), sp.new(N), sp.new(AGG_COUNT)
        p = sp.ptr
        check(self._lib.pla_kfold_reduce(self._h, p(elpd_i), p(lpd_full_i), N, float(scale_value), p(nrep), sp.mem_space, sp.stream,
                                         p(p_i), p(kfold_i), p(agg)))
        res = {"elpd_i": elpd_i, "lpd_full_i": lpd_full_i, "p_i": p_i, "kfold_i": kfold_i, "agg": agg}
        if not plan["host_out"]:
            return res
        return {k: v.cpu().numpy() for k, v in res.items()}

    # ------------------------------------------------------------------ moment matching
    @staticmethod
    def _mm_input(t, shape, what):
        """A contiguous float64 CUDA tensor of the given shape (copied only when it is not one already)."""
        import torch

        if not _is_torch_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: expected a CUDA tensor")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.to(torch.float64).contiguous()

    @staticmethod
    def mm_check_dim(n_dim, matrices):
        """The limits of the moment-matching kernels: ``ValueError`` beyond them."""
        if matrices and n_dim > _capi.PLA_MM_MAX_COV_DIM:
            raise ValueError(f"moment matching with cov=True takes at most {_capi.PLA_MM_MAX_COV_DIM} parameters, got {n_dim} "
                             "(use cov=False)")
        if n_dim > _capi.PLA_MM_MAX_DIM:
            raise ValueError(f"moment matching takes at most {_capi.PLA_MM_MAX_DIM} parameters, got {n_dim}")

    def mm_moments(self, upars, lw, cov=False):
        """``upars`` (B, S, D), ``lw`` (B, S) log weights, CUDA f64 -> ``(stats, covs)`` (``pla_mm_moments``): ``stats`` (B, 4, D) =
        plain mean, weighted mean ``sum exp(lw) x``, ``np.var`` and the raw weighted second moment of ``shift_and_scale``;
        ``covs`` (B, 2, D, D) = ``np.cov(rowvar=False)`` and ``np.cov(aweights=exp(lw))``, or None without ``cov``.  Nothing is
        synchronised; the bits depend neither on B nor on the grid."""
        if not _is_torch_tensor(upars) or upars.dim() != 3:
            raise ValueError("upars: expected a (B, S, D) CUDA tensor")
        B, S, D = (int(v) for v in upars.shape)
        self.mm_check_dim(D, cov)
        x = self._mm_input(upars, (B, S, D), "upars")
        w = self._mm_input(lw, (B, S), "lw")
        sp = self._space(x)
        stats = sp.new((B, 4, D))
        covs = sp.new((B, 2, D, D)) if cov else None
        p = sp.ptr
        check(self._lib.pla_mm_moments(self._h, p(x), p(w), B, S, D, 1 if cov else 0, sp.stream, p(stats), p(covs)))
        return stats, covs

    def mm_transform(self, x, m0, m1, pre=None, mapping=None, post_div=None, rows=None):
        """``out[b, s] = (((x[b, s] - m0[b]) * pre[b]) @ mapping[b].T) / post_div[b] + m1[b]`` for the rows ``s`` in ``rows = (lo, hi)``
        (default: all), ``x[b, s]`` for the others (``pla_mm_transform``).  ``x`` is (B, S, D), or (S, D) shared by every b;
        ``m0`` / ``m1`` / ``pre`` / ``post_div`` (B, D), ``mapping`` (B, D, D); CUDA f64.  Returns a new (B, S, D) tensor."""
        if not _is_torch_tensor(m0) or m0.dim() != 2:
            raise ValueError("m0: expected a (B, D) CUDA tensor")
        B, D = (int(v) for v in m0.shape)
        self.mm_check_dim(D, mapping is not None)
        shared = x.dim() == 2
        S = int(x.shape[-2])
        x = self._mm_input(x, (S, D) if shared else (B, S, D), "x")
        vec = lambda t, what: None if t is None else self._mm_input(t, (B, D), what)  # noqa: E731
        m0, m1, pre, post_div = vec(m0, "m0"), vec(m1, "m1"), vec(pre, "pre"), vec(post_div, "post_div")
        mapping = None if mapping is None else self._mm_input(mapping, (B, D, D), "mapping")
        lo, hi = (0, S) if rows is None else (int(rows[0]), int(rows[1]))
        sp = self._space(x)
        out = sp.new((B, S, D))
        p = sp.ptr
        check(self._lib.pla_mm_transform(self._h, p(x), 0 if shared else S * D, p(m0), p(pre), p(mapping), p(post_div), p(m1), B, S, D,
                                         lo, hi, sp.stream, p(out)))
        return out

    def mm_ratios(self, mode, a, b, c=None, jac=None):
        """The ratio assembly of moment matching (``pla_mm_ratios``), CUDA f64, ``a`` and ``b`` (B, S):
        ``"update"``: a = ll_new, b = lp_new, c = lp_orig (S,) -> (2B, S), rows [0, B) ``-ll + lp - lp_orig``, rows [B, 2B)
        ``lp - lp_orig``, NaN -> -inf; ``"split"``: a = ll_half, b = lp_half, c = lp_half_inv (B, S), jac (B, 2) -> (B, S);
        ``"sum"``: ``a + b`` with NaN / +inf -> -inf; ``"finish"``: a = ll, b = lw -> (B, 2) = ``logsumexp(ll + lw)``,
        ``logsumexp(ll) - log S``."""
        code = {"update": 0, "split": 1, "sum": 2, "finish": 3}[mode]
        if not _is_torch_tensor(a) or a.dim() != 2:
            raise ValueError("a: expected a (B, S) CUDA tensor")
        B, S = (int(v) for v in a.shape)
        a, b = self._mm_input(a, (B, S), "a"), self._mm_input(b, (B, S), "b")
        if code == 0:
            c = self._mm_input(c, (S,), "c")
        elif code == 1:
            c, jac = self._mm_input(c, (B, S), "c"), self._mm_input(jac, (B, 2), "jac")
        else:
            c = jac = None
        sp = self._space(a)
        out = sp.new({0: (2 * B, S), 1: (B, S), 2: (B, S), 3: (B, 2)}[code])
        p = sp.ptr
        check(self._lib.pla_mm_ratios(self._h, code, p(a), p(b), p(c), p(jac), B, S, sp.stream, p(out)))
        return out

    # ------------------------------------------------------------------ weights pass
    def importance_weights(self, logw, tail_count=0, method="psis"):
        """(n_obs, n_draws) log ratios -> (lw, diag) (``pla_importance_weights``)."""
        mcode = METHOD_CODES[method]
        sp, a, dims = self._matrix(logw, _WEIGHTS)
        n, s = dims[1:3]
        lw = sp.new((n, s), a.dtype)
        diag = sp.new(n)
        p = sp.ptr
        check(self._lib.pla_importance_weights(self._h, p(a), *dims, mcode, int(tail_count), sp.mem_space, sp.stream, p(lw), p(diag)))
        return lw, diag

    # ------------------------------------------------------------------ WAIC pass
    def waic(self, ll, scale_value=1.0, pointwise=True, aggregate=True, rows=None):
        """(n_obs, n_draws) log-likelihood -> ``dict(lppd_i, var_i, waic_i, agg)`` (``pla_waic``; the
        slots of ``agg`` are documented in include/pyloo_amd.h).  ``rows``: optional observation indices
        (``pla_waic_rows``), one output entry per index."""
        sp, a, dims = self._matrix(ll, _LOO, rows)
        idx = None if rows is None else sp.rows(rows, dims[1])
        m = dims[1] if idx is None else len(idx)
        lppd_i, var_i, waic_i = _pointwise(sp, m, pointwise, aggregate)
        agg = sp.new(AGG_COUNT, zero=True) if aggregate else None
        p = sp.ptr
        tail = (float(scale_value), sp.mem_space, sp.stream, p(lppd_i), p(var_i), p(waic_i), p(agg))
        if idx is None:
            check(self._lib.pla_waic(self._h, p(a), *dims, *tail))
        else:
            check(self._lib.pla_waic_rows(self._h, p(a), *dims, p(idx), m, *tail))
        return {"lppd_i": lppd_i, "var_i": var_i, "waic_i": waic_i, "agg": agg}

    # ------------------------------------------------------------------ Mix-IS-LOO passes
    def mixis_draw_lse(self, ll):
        """Pass 1 of Mix-IS-LOO (``pla_mixis_draw_lse``): (n_obs, n_draws) log-likelihood -> ``dict(c, n_replaced)`` with
        ``c[s] = log sum_i exp(-ll[i, s])`` and the counts of NaN and of infinite entries met, where the matrix lives."""
        sp, a, dims = self._matrix(ll, _IN_PLACE)
        c = sp.new(dims[2], zero=True)
        nrep = sp.new(2, "int64", zero=True)
        p = sp.ptr
        check(self._lib.pla_mixis_draw_lse(self._h, p(a), *dims, sp.mem_space, sp.stream, p(c), p(nrep)))
        return {"c": c, "n_replaced": nrep}

    def mixis_loo(self, ll, c=None, scale_value=1.0, pointwise=True, aggregate=True):
        """Mix-IS-LOO (``pla_mixis_loo``): ``dict(loo_i, c, agg)`` with ``loo_i = scale * (LSE_s(-c) - LSE_s(-ll[i, s] - c[s]))``.
        ``c``: the result of :meth:`mixis_draw_lse` (computed when None); the slots of ``agg`` are documented in
        include/pyloo_amd.h."""
        sp, a, dims = self._matrix(ll, _IN_PLACE)
        n, s = dims[1:3]
        if c is None:
            c = self.mixis_draw_lse(ll)["c"]
        elif sp.device is None:
            c = np.ascontiguousarray(c, dtype=np.float64)
        else:
            import torch

            c = torch.as_tensor(c, dtype=torch.float64, device=sp.device).contiguous()
        if c.shape != (s,):
            raise ValueError(f"c must have one entry per draw: expected ({s},), got {tuple(c.shape)}")
        loo_i = sp.new(n, zero=True) if pointwise else None
        agg = sp.new(AGG_COUNT, zero=True) if aggregate else None
        p = sp.ptr
        check(self._lib.pla_mixis_loo(self._h, p(a), *dims, p(c), float(scale_value), sp.mem_space, sp.stream, p(loo_i), p(agg)))
        return {"loo_i": loo_i, "c": c, "agg": agg}

    def set_mixis_grid(self, max_workgroups):
        """Cap the workgroups per launch of the Mix-IS-LOO passes (0: the library's choice); the results do not depend on it."""
        check(self._lib.pla_engine_set_mixis_grid(self._h, int(max_workgroups)))

    @staticmethod
    def mixis_tile_rows(n_obs):
        """Rows per partial of pass 1 for ``n_obs`` observations (``pla_mixis_tile_rows``)."""
        rc = load_library().pla_mixis_tile_rows(int(n_obs))
        if rc < 0:
            check(rc)
        return rc

    # ------------------------------------------------------------------ weighted expectations
    def e_loo(self, x, log_weights, log_ratios=None, tail_len=20):
        """(n_obs, n_draws) draws ``x`` + log-weights (+ raw log ratios) -> ``dict(mean, var, k_mean, k_var, k_none)``
        (``pla_e_loo``: e_loo.py:214-236 per observation).  NumPy in -> NumPy out; CUDA tensors in -> CUDA tensors out."""
        mats = [x, log_weights] + ([log_ratios] if log_ratios is not None else [])
        sp, mats, code, n, s = self._promoted(mats, "x, log_weights and log_ratios", own_strides=False)
        keys = ("mean", "var", "k_mean", "k_var", "k_none")
        out = {k: sp.new(n) for k in keys}
        p = sp.ptr
        check(self._lib.pla_e_loo(self._h, p(mats[0]), p(mats[1]), p(mats[2]) if len(mats) > 2 else None, code, n, s,
                                  *sp.strides(mats[0]), int(tail_len), sp.mem_space, sp.stream, *(p(out[k]) for k in keys)))
        return out

    def e_loo_quantiles(self, x, log_weights, probs):
        """(n_obs, n_draws) draws + log-weights, quantile levels -> (n_obs, n_probs) weighted quantiles (``pla_e_loo_quantiles``:
        e_loo.py:468-515, 534-554)."""
        pr = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
        sp, mats, code, n, s = self._promoted([x, log_weights], "x and log_weights", own_strides=False)
        out = sp.new((n, pr.size))
        p = sp.ptr
        check(self._lib.pla_e_loo_quantiles(self._h, p(mats[0]), p(mats[1]), code, n, s, *sp.strides(mats[0]), p(pr), pr.size,
                                            sp.mem_space, sp.stream, p(out)))
        return out

    # ------------------------------------------------------------------ LOO-PIT
    def loo_pit(self, mat, y_hat, y, tail_count=0, method="psis", kind="loglik"):
        """(n_obs, n_draws) log-likelihood (``kind="loglik"``) or log weights (``kind="log_weights"``), the predictive draws
        ``y_hat`` of the same shape and the observed ``y`` [n_obs] -> ``dict(pit_le, pit_lt, diag, n_replaced)`` (``pla_loo_pit``).
        The two matrices are promoted to one dtype (f64 if either is) and passed with their own strides.  NumPy in -> NumPy out
        (and an int); CUDA tensors in -> CUDA tensors out, nothing synchronised.  ``diag`` is None for log weights."""
        mcode = METHOD_CODES[method]
        if kind not in ("loglik", "log_weights"):
            raise ValueError(f"kind must be 'loglik' or 'log_weights', got {kind!r}")
        kcode = _capi.PLA_PIT_LOGLIK if kind == "loglik" else _capi.PLA_PIT_LOG_WEIGHTS
        sp, mats, code, n, s = self._promoted([mat, y_hat], "mat and y_hat", own_strides=True, host_obs=True)
        yv = sp.vector(y, n, "y has {got} values for {n} observations")
        pit_le, pit_lt = sp.new(n), sp.new(n)
        diag = sp.new(n) if kind == "loglik" else None
        nrep = sp.counter()
        p = sp.ptr
        check(self._lib.pla_loo_pit(self._h, p(mats[0]), p(mats[1]), p(yv), code, n, s, *sp.strides(mats[0]), *sp.strides(mats[1]),
                                    kcode, mcode, int(tail_count), sp.mem_space, sp.stream, p(pit_le), p(pit_lt), p(diag), p(nrep)))
        return {"pit_le": pit_le, "pit_lt": pit_lt, "diag": diag, "n_replaced": sp.read(nrep)}

    # ------------------------------------------------------------------ LOO diagnostics
    def loo_diag(self, ll, tail_count=0, method="psis", rows=None):
        """(n_obs, n_draws) log-likelihood -> ``dict(diag, elpd_i, ess_w, var_log, n_replaced)`` (``pla_loo_diag``): the Pareto k
        (ESS for SIS / TIS) of the leave-one-out weights, the pointwise elpd, the effective sample size ``1 / sum w^2`` of the
        weights and the log-scale variance of the estimate, per observation.  ``rows``: optional observation indices, one output
        entry per index.  NumPy in -> NumPy out (and an int); CUDA tensor in -> CUDA tensors out, nothing synchronised."""
        mcode = METHOD_CODES[method]
        sp, a, dims = self._matrix(ll, _LOO_DIAG, rows)
        idx = None if rows is None else sp.rows(rows, dims[1])
        m = dims[1] if idx is None else len(idx)
        out = [sp.new(m) for _ in range(4)]
        nrep = sp.counter()
        p = sp.ptr
        check(self._lib.pla_loo_diag(self._h, p(a), *dims, p(idx), m, mcode, int(tail_count), sp.mem_space, sp.stream,
                                     p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(nrep)))
        return {"diag": out[0], "elpd_i": out[1], "ess_w": out[2], "var_log": out[3], "n_replaced": sp.read(nrep)}

    def loo_diag_weights(self, lw, ll):
        """Log weights of any normalisation and the log-likelihood, two (n_obs, n_draws) matrices -> ``dict(elpd_i, ess_w, var_log)``
        (``pla_loo_diag_weights``).  The matrices are promoted to one dtype (f64 if either is) and passed with their own strides.
        NumPy in -> NumPy out; CUDA tensors in -> CUDA tensors out, nothing synchronised."""
        sp, mats, code, n, s = self._promoted([lw, ll], "lw and ll", own_strides=True)
        out = [sp.new(n) for _ in range(3)]
        p = sp.ptr
        check(self._lib.pla_loo_diag_weights(self._h, p(mats[0]), p(mats[1]), code, n, s, *sp.strides(mats[0]), *sp.strides(mats[1]),
                                             sp.mem_space, sp.stream, p(out[0]), p(out[1]), p(out[2])))
        return {"elpd_i": out[0], "ess_w": out[1], "var_log": out[2]}

    # ------------------------------------------------------------------ LOO influence
    def loo_influence(self, mat, theta, center, scale, tail_count=0, method="psis", kind="loglik", rows=None):
        """(n_obs, n_draws) log-likelihood (``kind="loglik"``) or log weights (``kind="log_weights"``) and the draw-wise quantities
        ``theta`` (n_draws, P) with their ``center`` and ``scale`` [P] -> ``dict(shift, m2, kl, ess_w, diag, n_replaced)``
        (``pla_loo_influence``): per observation the standardised leave-one-out mean shift and second moment of every quantity
        (m, P), the KL divergence of the weighted draws from the unweighted ones and the effective sample size of the weights;
        ``diag`` is the Pareto k (ESS for SIS / TIS), None for log weights.  ``rows``: optional observation indices
        (``kind="loglik"``), one output row per index.  NumPy in -> NumPy out (and an int); CUDA tensor in -> CUDA tensors out,
        nothing synchronised when ``theta``, ``center`` and ``scale`` are device-resident too (host arrays beside a CUDA matrix are
        uploaded with a synchronous copy first).  ``theta`` is taken as f64 with its own strides, a ``.T`` view included."""
        mcode = METHOD_CODES[method]
        if kind not in ("loglik", "log_weights"):
            raise ValueError(f"kind must be 'loglik' or 'log_weights', got {kind!r}")
        loglik = kind == "loglik"
        if rows is not None and not loglik:
            raise ValueError("rows= needs kind='loglik'")
        args = _capi.InfluenceArgs(engine=self._h.value, kind=_capi.PLA_PIT_LOGLIK if loglik else _capi.PLA_PIT_LOG_WEIGHTS, method=mcode,
                                   tail_count=int(tail_count))
        sp, t, (args.dtype, n, s, args.stride_obs, args.stride_draw) = self._matrix(mat, _LOO_DIAG if loglik else _LOG_WEIGHTS, rows)
        th = sp.f64(theta)
        th = th.reshape(-1, 1) if th.ndim == 1 else th
        if th.ndim != 2 or th.shape[0] != s:
            raise ValueError(f"theta must be (n_draws, P) with n_draws = {s}, got {tuple(th.shape)}")
        th, (std, stq) = sp.dense(th)
        nq = th.shape[1]
        cv, sv = sp.vector(center), sp.vector(scale)
        if len(cv) != nq or len(sv) != nq:
            raise ValueError(f"center and scale need {nq} values")
        idx = None if rows is None else sp.rows(rows, n)
        m = n if idx is None else len(idx)
        out = {"shift": sp.new((m, nq)), "m2": sp.new((m, nq)), "kl": sp.new(m), "ess_w": sp.new(m),
               "diag": sp.new(m) if loglik else None, "n_replaced": sp.counter()}
        p = sp.ptr
        args.mem_space, args.stream = sp.mem_space, sp.stream
        args.theta_stride_draw, args.theta_stride_quant = std, (stq if nq > 1 else 1)
        args.mat, args.n_obs, args.n_draws = p(t), n, s
        args.row_index, args.n_rows = p(idx), m
        args.theta, args.n_quant, args.center, args.scale = p(th), nq, p(cv), p(sv)
        for k in ("shift", "m2", "kl", "ess_w", "diag", "n_replaced"):
            setattr(args, k, p(out[k]))
        check(self._lib.pla_loo_influence(C.byref(args)))
        out["n_replaced"] = sp.read(out["n_replaced"])
        return out

    # ------------------------------------------------------------------ GLM log-likelihood generator
    def glm(self, X, beta, family, y=None, offset=None, trials=None, obs_const=None, draw_scale=None, draw_const=None, rows=None,
            mode="matrix", tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True, groups=None):
        """The log-likelihood of a generalised linear model from its design matrix ``X`` (n_obs, P), the coefficient draws ``beta``
        (n_draws, P) and the family (``pla_glm``): ``"linpred"`` (eta itself), ``"gaussian"``, ``"binomial"`` (logit link), ``"poisson"``
        (log link), ``"negbinomial"`` (log link), ``"gamma"`` (log link), ``"binomial_probit"``.  ``y``, ``offset``, ``trials``,
        ``obs_const`` are [n_obs], ``draw_scale`` and ``draw_const`` [n_draws] (Gaussian sigma, negative-binomial phi, gamma shape);
        the constants are the caller's (include/pyloo_amd.h).  ``rows``: optional observation indices, one output row per index.
        ``mode="matrix"`` returns the (m, n_draws) matrix; ``mode="loo"`` consumes it block by block in the PSIS-LOO pass and returns
        ``dict(diag, loo_i, lppd_i, agg, n_replaced)``.  NumPy ``X`` -> NumPy out; CUDA tensor -> CUDA tensors, everything else is
        moved to the device of ``X`` first.  ``X`` and ``beta`` are taken as f64 with their own strides, ``.T`` views included.
        ``groups``: group-level terms, a sequence of ``(index, draws)`` or ``(index, draws, z)`` -- ``index`` [n_obs] integers in
        ``[0, G)``, ``draws`` (n_draws, G) with its own strides, ``z`` [n_obs] or None (1) --, added to the linear predictor in the
        order given (``pla_glm_grouped``; an empty sequence goes through that entry with no terms, None through ``pla_glm``)."""
        sp, args, terms, keep, m, s = self._glm_block(X, beta, family, y, offset, trials, obs_const, draw_scale, draw_const, rows, mode,
                                                      tail_count, method, scale_value, good_k, groups)

        def run():
            if groups is None:
                check(self._lib.pla_glm(C.byref(args)))
            else:
                check(self._lib.pla_glm_grouped(C.byref(self._glm_grouped(args, terms))))

        return self._glm_finish(sp, args, m, s, mode == "loo", pointwise, aggregate, run, keep)

    def _glm_block(self, X, beta, family, y, offset, trials, obs_const, draw_scale, draw_const, rows, mode, tail_count, method,
                   scale_value, good_k, groups):
        """The argument block of ``pla_glm`` without its outputs, in the memory space of ``X`` -> ``(space, block, terms, what to keep
        alive over the call, rows of the call, n_draws)``; ``terms``: one tuple of ``pla_glm_term`` entries per term of ``groups``."""
        fam = {"linpred": _capi.PLA_GLM_LINPRED, "gaussian": _capi.PLA_GLM_GAUSSIAN, "binomial": _capi.PLA_GLM_BINOMIAL_LOGIT,
               "poisson": _capi.PLA_GLM_POISSON_LOG, "negbinomial": _capi.PLA_GLM_NEGBINOMIAL_LOG, "gamma": _capi.PLA_GLM_GAMMA_LOG,
               "binomial_probit": _capi.PLA_GLM_BINOMIAL_PROBIT}
        if family not in fam:
            raise ValueError(f"family must be one of {sorted(fam)}, got {family!r}")
        if mode not in ("matrix", "loo"):
            raise ValueError(f"mode must be 'matrix' or 'loo', got {mode!r}")
        loo = mode == "loo"
        args = _capi.GlmArgs(engine=self._h.value, family=fam[family], mode=_capi.PLA_GLM_MODE_LOO if loo else _capi.PLA_GLM_MODE_MATRIX,
                             method=METHOD_CODES[method], tail_count=int(tail_count), scale_value=float(scale_value), good_k=float(good_k))
        sp = self._space(X)
        if sp.device is not None and (X.dim() != 2 or not X.is_cuda):
            raise ValueError("expected a 2-D CUDA tensor X")
        xt = sp.f64(X)
        if xt.ndim != 2:
            raise ValueError("expected a 2-D (n_obs, P) array X")
        bt = sp.f64(beta)
        if bt.ndim != 2 or bt.shape[1] != xt.shape[1]:
            raise ValueError(f"beta must be (n_draws, P) with P = {xt.shape[1]}, got {tuple(bt.shape)}")
        (xt, xs), (bt, bs) = sp.dense(xt), sp.dense(bt)
        n, npred = xt.shape
        s = bt.shape[0]
        idx = None if rows is None else sp.rows(rows, n)
        p = sp.ptr
        args.mem_space, args.stream = sp.mem_space, sp.stream
        keep = [xt, bt, idx]
        for count, vecs in ((n, {"y": y, "offset": offset, "trials": trials, "obs_const": obs_const}),
                            (s, {"draw_scale": draw_scale, "draw_const": draw_const})):
            for k, v in vecs.items():
                v = sp.vector(v, count, k + " needs {n} values, got {got}")
                keep.append(v)
                setattr(args, k, p(v))
        m = n if idx is None else len(idx)
        args.x, args.n_obs, args.n_pred = p(xt), n, npred
        args.x_stride_obs, args.x_stride_pred = max(int(xs[0]), 1), max(int(xs[1]), 1)
        args.beta, args.n_draws = p(bt), s
        args.beta_stride_draw, args.beta_stride_pred = max(int(bs[0]), 1), max(int(bs[1]), 1)
        args.row_index, args.n_rows = p(idx), m
        terms = []
        if groups is not None:
            if len(groups) > _capi.GLM_MAX_TERMS:
                raise ValueError(f"at most {_capi.GLM_MAX_TERMS} group-level terms are supported, got {len(groups)}")
            for t, term in enumerate(groups):
                gi, u, z = (*term, None)[:3]
                gi = sp.vector(gi, dtype="int32")
                u = sp.f64(u)
                u, us = sp.dense(u) if u.ndim == 2 else (u, None)
                z = sp.vector(z)
                if us is None or u.shape[0] != s or u.shape[1] < 1:
                    raise ValueError(f"draws of term {t} must be (n_draws, G) with n_draws = {s} and G >= 1, got {tuple(u.shape)}")
                if len(gi) != n or (z is not None and len(z) != n):
                    raise ValueError(f"index and z of term {t} need {n} values")
                keep += [gi, u, z]
                terms.append((p(gi), p(z), p(u), max(int(us[0]), 1), max(int(us[1]), 1), int(u.shape[1])))

        return sp, args, terms, keep, m, s

    @staticmethod
    def _glm_grouped(args, terms):
        grouped = _capi.GlmGroupedArgs(n_terms=len(terms))
        grouped.glm = args
        for t, (gp, zp, up, sd, sg, ng) in enumerate(terms):
            grouped.terms[t] = _capi.GlmTerm(group_index=gp, z=zp, u=up, u_stride_draw=sd, u_stride_group=sg, n_groups=ng)
        return grouped

    @staticmethod
    def _glm_finish(sp, args, m, s, loo, pointwise, aggregate, run, keep):
        """The outputs of a GLM call of ``m`` rows into ``args``, then ``run()``: the matrix, or the dict of the fused LOO pass."""
        p = sp.ptr
        if not loo:
            out = sp.new((m, s))
            args.out, args.out_pitch = p(out), s
            run()
            del keep
            return out
        diag, loo_i, lppd_i = _pointwise(sp, m, pointwise, aggregate)
        res = {"diag": diag, "loo_i": loo_i, "lppd_i": lppd_i, "agg": sp.new(AGG_COUNT) if aggregate else None, "n_replaced": sp.counter()}
        for k, v in res.items():
            setattr(args, k, p(v))
        run()
        del keep
        res["n_replaced"] = sp.read(res["n_replaced"])
        return res

    def glm_marginal(self, X, beta, family, index, tau, nodes, log_weights, z=None, y=None, offset=None, trials=None, obs_const=None,
                     draw_scale=None, draw_const=None, mode="matrix", tail_count=0, method="psis", scale_value=1.0, good_k=0.7,
                     pointwise=True, aggregate=True, groups=None):
        """The cluster-marginal log-likelihood of a multilevel GLM (``pla_glm_marginal``): per cluster of ``index`` (a
        :class:`~pyloo_amd.loo_group.GroupIndex` over the rows of ``X``) the likelihood of its observations with the cluster's own
        effect ``u ~ N(0, tau_s^2)`` -- entering the linear predictor of :meth:`glm` as ``z_i u`` -- integrated out by quadrature on
        ``nodes`` / ``log_weights`` (C, n_nodes).  ``tau`` is [n_draws], ``z`` [n_obs] or None (1); everything else is :meth:`glm`'s,
        ``family="linpred"`` and ``rows`` excepted.  ``mode="matrix"`` returns the (C, n_draws) matrix, ``mode="loo"`` the dict of
        the fused PSIS-LOO pass with one entry per cluster.  A CUDA ``X`` waits once for the offsets of ``index``."""
        if family not in ("gaussian", "binomial", "poisson"):
            raise ValueError(f"glm_marginal needs a likelihood: family must be 'gaussian', 'binomial' or 'poisson', got {family!r}")
        sp, args, terms, keep, n, s = self._glm_block(X, beta, family, y, offset, trials, obs_const, draw_scale, draw_const, None, mode,
                                                      tail_count, method, scale_value, good_k, groups)
        n_clusters = int(index.n_groups)
        if int(index.n_obs) != n:
            raise ValueError(f"index covers {int(index.n_obs)} observations, X has {n} rows")
        off, mem = sp.index(index)
        tau = sp.vector(tau, s, "tau needs {n} values, one per draw, got {got}")
        z = sp.vector(z, n, "z needs {n} values, got {got}")
        nodes, log_weights = sp.f64(nodes), sp.f64(log_weights)
        if nodes.ndim != 2 or nodes.shape[0] != n_clusters or tuple(log_weights.shape) != tuple(nodes.shape):
            raise ValueError(f"nodes and log_weights must be (n_clusters, n_nodes) with n_clusters = {n_clusters}, got "
                             f"{tuple(nodes.shape)} and {tuple(log_weights.shape)}")
        n_nodes = int(nodes.shape[1])
        if not 1 <= n_nodes <= _capi.GLM_MARGINAL_MAX_NODES:
            raise ValueError(f"n_nodes must lie in [1, {_capi.GLM_MARGINAL_MAX_NODES}], got {n_nodes}")
        nodes, log_weights = (a.contiguous() if sp.device is not None else np.ascontiguousarray(a) for a in (nodes, log_weights))
        keep += [off, mem, tau, z, nodes, log_weights]
        p = sp.ptr
        marg = _capi.GlmMarginalArgs(n_clusters=n_clusters, n_members=n, cluster_offsets=p(off), members=p(mem), z=p(z), tau=p(tau),
                                     n_nodes=n_nodes, nodes=p(nodes), log_weights=p(log_weights))

        def run():
            marg.grouped = self._glm_grouped(args, terms)
            check(self._lib.pla_glm_marginal(C.byref(marg)))

        return self._glm_finish(sp, args, n_clusters, s, mode == "loo", pointwise, aggregate, run, keep)

    @staticmethod
    def glm_marginal_segment():
        """Members per segment of the summation rule of ``pla_glm_marginal`` (``pla_glm_marginal_segment``)."""
        return load_library().pla_glm_marginal_segment()

    def glm_predict(self, X, beta, family, y=None, offset=None, trials=None, obs_const=None, draw_scale=None, draw_const=None, rows=None,
                    tail_count=0, method="psis", log_weights=None, pit=True):
        """The leave-one-out predictive moments and PIT of a generalised linear model from its design matrix, the draws and the
        family, every argument as :meth:`glm` takes it (``pla_glm_predict``) -> ``dict(mean, m2, pit_le, pit_lt, diag, elpd_i,
        n_replaced, n_pit_skipped)``, one entry per row of the call.  ``log_weights=None``: the weights are PSIS / SIS / TIS of the
        model's own log-likelihood, generated and consumed block by block; ``diag`` is their Pareto k (ESS for SIS / TIS).
        ``log_weights`` (m, n_draws), of any normalisation with unit stride along the draws: used as they are, ``diag`` and
        ``elpd_i`` are None.  ``pit=False`` (always for ``"gamma"``): the two PIT values are None and nothing is walked for them."""
        if family == "linpred":
            raise ValueError("glm_predict needs a likelihood, not family='linpred'")
        sp, args, _, keep, m, s = self._glm_block(X, beta, family, y, offset, trials, obs_const, draw_scale, draw_const, rows, "loo",
                                                  tail_count, method, 1.0, 0.7, None)
        loglik = log_weights is None
        pred = _capi.GlmPredictArgs(kind=_capi.PLA_PIT_LOGLIK if loglik else _capi.PLA_PIT_LOG_WEIGHTS)
        p = sp.ptr
        if not loglik:
            lw = sp.f64(log_weights)
            if lw.ndim != 2 or tuple(lw.shape) != (m, s):
                raise ValueError(f"log_weights must be (rows of the call, n_draws) = ({m}, {s}), got {tuple(lw.shape)}")
            lw, ls = sp.dense(lw)
            if s > 1 and int(ls[1]) != 1:
                lw = lw.contiguous() if sp.device is not None else np.ascontiguousarray(lw)
                ls = (s, 1)
            keep.append(lw)
            pred.log_weights, pred.lw_stride_obs, pred.lw_stride_draw = p(lw), max(int(ls[0]), s), 1
        want_pit = pit and family != "gamma"
        out = {"mean": sp.new(m), "m2": sp.new(m), "pit_le": sp.new(m) if want_pit else None, "pit_lt": sp.new(m) if want_pit else None,
               "diag": sp.new(m) if loglik else None, "elpd_i": sp.new(m) if loglik else None, "n_replaced": sp.counter(),
               "n_pit_skipped": sp.counter()}
        for k, v in out.items():
            setattr(pred, k, p(v))
        pred.glm = args
        check(self._lib.pla_glm_predict(C.byref(pred)))
        del keep
        out["n_replaced"], out["n_pit_skipped"] = sp.read(out["n_replaced"]), sp.read(out["n_pit_skipped"])
        return out

    @staticmethod
    def glm_predict_segment():
        """Tiles of 16 draws per segment of the summation rule of ``pla_glm_predict`` (``pla_glm_predict_segment``)."""
        return load_library().pla_glm_predict_segment()

    # ------------------------------------------------------------------ leave-future-out CV
    def lfo_ratios(self, ll, first, n_steps):
        """Log ratios of leave-future-out CV (``pla_lfo_ratios``): ``dict(ratios, n_replaced)`` with ``ratios[j, s]`` the sum of rows
        ``first .. first + j - 1`` of the (n_obs, n_draws) log-likelihood ``ll``, always float64, in the summation order
        include/pyloo_amd.h documents.  NumPy in -> NumPy out (and an int); CUDA tensor in -> CUDA tensors out, nothing synchronised."""
        sp, a, dims = self._matrix(ll, _LFO)
        first, n_steps = int(first), int(n_steps)
        if n_steps < 1:
            raise ValueError("n_steps must be at least 1")
        out = sp.new((n_steps, dims[2]))
        nrep = sp.counter()
        p = sp.ptr
        check(self._lib.pla_lfo_ratios(self._h, p(a), *dims, first, n_steps, sp.mem_space, sp.stream, p(out), p(nrep)))
        return {"ratios": out, "n_replaced": sp.read(nrep)}

    def lfo(self, ll, first, n_steps, horizon=1, tail_count=0, k_threshold=0.7, method="psis", mode="forward"):
        """One pass of PSIS leave-future-out CV over the steps ``first .. first + n_steps - 1`` of one fit (``pla_lfo``):
        ``dict(diag, elpd_i, first_high, n_replaced)``.  ``diag[0] = 0`` (the fit's own step is exact); ``first_high`` is the
        smallest ``j >= 1`` with ``diag[j] > k_threshold``, else ``n_steps``.  NumPy in -> NumPy out (and two ints); CUDA tensor in
        -> CUDA tensors out (``first_high`` and ``n_replaced`` one int64 each), nothing synchronised.

        ``mode="backward"`` (``PLA_LFO_BACKWARD``): ``first`` is ``last``, the number of observations the fit saw; step j is
        ``t_j = min(last, n_obs - horizon) - j``, its log ratios remove the rows ``t_j .. last - 1``, only a step with ``t_j = last``
        is exact, and ``first_high`` may be 0 when step 0 is not."""
        if mode not in ("forward", "backward"):
            raise ValueError(f"mode must be 'forward' or 'backward', got {mode!r}")
        mcode = METHOD_CODES[method] | (_capi.PLA_LFO_BACKWARD if mode == "backward" else 0)
        sp, a, dims = self._matrix(ll, _LFO)
        first, n_steps, horizon = int(first), int(n_steps), int(horizon)
        if n_steps < 1:
            raise ValueError("n_steps must be at least 1")
        diag, elpd = sp.new(n_steps, zero=True), sp.new(n_steps, zero=True)
        high, nrep = sp.counter(), sp.counter()
        p = sp.ptr
        check(self._lib.pla_lfo(self._h, p(a), *dims, first, n_steps, horizon, mcode, int(tail_count), float(k_threshold),
                                sp.mem_space, sp.stream, p(diag), p(elpd), p(high), p(nrep)))
        return {"diag": diag, "elpd_i": elpd, "first_high": sp.read(high), "n_replaced": sp.read(nrep)}

    # ------------------------------------------------------------------ relative MCMC efficiency
    def relative_eff(self, x, n_chains=1, log=True, split=False, cap=True):
        """Relative efficiency of every row of an (n_obs, n_draws) matrix of ``n_chains`` equal chains stacked chain-major
        (``pla_relative_eff``): ``dict(r_eff, n_invalid)``.  Invalid rows (NaN or +inf entries, constant rows) give NaN and are
        counted.  NumPy in -> NumPy out (and an int); CUDA tensor in -> CUDA tensors out (``n_invalid`` one int64), nothing
        synchronised."""
        sp, a, dims = self._matrix(x, _LFO)
        flags = (_capi.PLA_ESS_LOG if log else 0) | (_capi.PLA_ESS_SPLIT if split else 0) | (_capi.PLA_ESS_CAP if cap else 0)
        r = sp.new(dims[1], zero=True)
        ninv = sp.counter()
        p = sp.ptr
        check(self._lib.pla_relative_eff(self._h, p(a), *dims, int(n_chains), flags, sp.mem_space, sp.stream, p(r), p(ninv)))
        return {"r_eff": r, "n_invalid": sp.read(ninv)}

    def set_ess_grid(self, max_workgroups):
        """Cap the workgroups per launch of the relative-efficiency pass (0: the library's choice); the results do not depend on it."""
        check(self._lib.pla_engine_set_ess_grid(self._h, int(max_workgroups)))

    @staticmethod
    def ess_lds_max_draws():
        """Analysed draws per row up to which the relative-efficiency pass keeps the row on chip (``pla_ess_lds_max_draws``)."""
        return load_library().pla_ess_lds_max_draws()

    # ------------------------------------------------------------------ model comparison
    def _compare_input(self, x):
        """``(space, matrix, (dtype code, K, N, pitch))`` of a (n_models, n_obs) matrix: rows with unit stride, a pitch of at least
        n_obs (copied otherwise)."""
        sp = self._space(x)
        if sp.device is not None:
            import torch

            if x.dim() != 2 or not x.is_cuda:
                raise ValueError("expected a 2-D (n_models, n_obs) CUDA tensor")
            if x.dtype not in (torch.float64, torch.float32):
                x = x.to(torch.float64)
            K, N = x.shape
            if (N > 1 and x.stride(1) != 1) or (K > 1 and x.stride(0) < N):
                x = x.contiguous()
            return sp, x, (_code(x), K, N, (x.stride(0) if K > 1 else N))
        a = np.asarray(x)
        if a.dtype not in (np.float64, np.float32):
            a = a.astype(np.float64)
        if a.ndim != 2:
            raise ValueError("expected a 2-D (n_models, n_obs) array")
        K, N = a.shape
        if (N > 1 and a.strides[1] != a.itemsize) or (K > 1 and (a.strides[0] % a.itemsize or a.strides[0] < N * a.itemsize)):
            a = np.ascontiguousarray(a)
        return sp, a, (_code(a), K, N, (a.strides[0] // a.itemsize if K > 1 else N))

    def compare_moments(self, x, best):
        """(n_models, n_obs) pointwise values -> ``out[3K + 1]`` (``pla_compare_moments``): ``out[3k]`` = sum of row k,
        ``out[3k + 1]`` / ``out[3k + 2]`` = mean / M2 of ``x[k] - x[best]`` (dse = sqrt(M2)), ``out[3K]`` = sum of the column
        maxima.  NumPy in -> ndarray; CUDA tensor in -> CUDA tensor (nothing synchronised)."""
        sp, x, dims = self._compare_input(x)
        out = sp.new(3 * dims[1] + 1)
        check(self._lib.pla_compare_moments(self._h, sp.ptr(x), *dims, int(best), sp.mem_space, sp.stream, sp.ptr(out)))
        return out

    def stacking_eval(self, x, weights, scale_mul=1.0):
        """One evaluation of the stacking objective (``pla_stacking_eval``): returns ``(F, G)`` on the host, F = sum_i log d_i and
        G[k] = sum_i e_ik / d_i with e_ik = exp(s x_ik - max_k s x_ik), d_i = sum_k w_k e_ik, s = ``scale_mul``."""
        sp, x, dims = self._compare_input(x)
        K = dims[1]
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != K:
            raise ValueError(f"expected {K} weights, got {w.size}")
        out = np.empty(K + 1)
        check(self._lib.pla_stacking_eval(self._h, sp.ptr(x), *dims, float(scale_mul), _ptr(w), sp.mem_space, sp.stream, _ptr(out)))
        return float(out[0]), out[1:].copy()

    def bb_bootstrap(self, x, n_boot, alpha=1.0, seed=0, scale_mul=1.0):
        """Bayesian-bootstrap replicates ``z`` (n_boot, n_models) of ``N * s * sum_i G_bi x_ik / sum_i G_bi`` with Gamma(alpha)
        weights drawn in the kernel from the Philox stream keyed by ``seed`` (``pla_bb_bootstrap``).  NumPy in -> ndarray;
        CUDA tensor in -> CUDA tensor (nothing synchronised)."""
        sp, x, dims = self._compare_input(x)
        B = int(n_boot)
        z = sp.new((B, dims[1]))
        check(self._lib.pla_bb_bootstrap(self._h, sp.ptr(x), *dims, float(scale_mul), B, float(alpha), int(seed) & (2**64 - 1),
                                         sp.mem_space, sp.stream, sp.ptr(z)))
        return z

    def bb_gamma_draws(self, seed, alpha, n_boot, n_obs):
        """The gamma stream of :meth:`bb_bootstrap` on its own (``pla_bb_gamma_draws``): (n_boot, n_obs) ndarray of G_bi."""
        out = np.empty((int(n_boot), int(n_obs)))
        check(self._lib.pla_bb_gamma_draws(self._h, int(seed) & (2**64 - 1), float(alpha), int(n_boot), int(n_obs), PLA_HOST, None,
                                           _ptr(out)))
        return out

    def set_compare_grid(self, max_workgroups):
        """Cap on the workgroups per launch of the comparison passes (0: the library's choice).  The results do not depend on it."""
        check(self._lib.pla_engine_set_compare_grid(self._h, int(max_workgroups)))

    # ------------------------------------------------------------------ non-factorised LOO
    def nonfactor_log_lik(self, y, mu, mat, df=None, model="normal"):
        """Conditional log-likelihood of a joint multivariate normal / Student-t model (``pla_nonfactor_loglik``).

        ``y`` (N,), ``mu`` (S, N), ``mat`` (S, N, N) -- one covariance matrix per draw, inverted whatever it holds, as the
        reference does --, ``df`` (S,) for ``model="student_t"``.  NumPy arrays (staged by the library in blocks of draws) or
        CUDA tensors (read in place; non-contiguous ones are made contiguous once).  Mixed f32 / f64 inputs are all taken as
        f64.  Returns ``(ll, flags)``: ``ll`` (N, S) float64 with the draws fastest, ``flags`` (S,) int32 status words
        (``PLA_NF_*``); CUDA tensors when any input is one (nothing synchronised), ndarrays otherwise (CPU tensors included)."""
        code = {"normal": _capi.PLA_MVN_NORMAL, "student_t": _capi.PLA_MVN_STUDENT_T}[model]
        arrays = [y, mu, mat] + ([df] if code == _capi.PLA_MVN_STUDENT_T else [])
        on_device = [a for a in arrays if _is_torch_tensor(a) and a.is_cuda]
        if on_device:
            import torch

            sp = self._space(on_device[0])  # (CPU tensors are copied to its device)
            f64 = not all(a.dtype == torch.float32 if _is_torch_tensor(a) else np.asarray(a).dtype == np.float32 for a in arrays)
            dt = torch.float64 if f64 else torch.float32
            arrays = [(a if _is_torch_tensor(a) else torch.as_tensor(np.asarray(a))).to(device=sp.device, dtype=dt).contiguous()
                      for a in arrays]
        else:  # host memory -- NumPy arrays and CPU tensors -- goes through the library's staging (PLA_HOST)
            sp = _HOST
            arrays = [a.detach().numpy() if _is_torch_tensor(a) else np.asarray(a) for a in arrays]
            dt = np.float32 if all(a.dtype == np.float32 for a in arrays) else np.float64
            arrays = [np.ascontiguousarray(a, dtype=dt) for a in arrays]
        S, N = arrays[1].shape
        ll = sp.new((N, S))
        flags = sp.new(S, "int32")
        p = sp.ptr
        check(self._lib.pla_nonfactor_loglik(self._h, p(arrays[0]), p(arrays[1]), p(arrays[2]), p(arrays[3]) if len(arrays) > 3 else None,
                                             _code(arrays[0]), N, S, N, N * N, code, sp.mem_space, sp.stream, p(ll), S, 1, p(flags)))
        return ll, flags

    def set_nonfactor_route(self, route):
        """0: automatic; 1 / 2 / 3: the LDS, blocked (engine-memory) or general route wherever the shape allows it (tests)."""
        check(self._lib.pla_engine_set_nonfactor_route(self._h, int(route)))

    def set_nonfactor_grid(self, max_workgroups):
        """Cap on the workgroups of the non-factorised LOO kernels (0: the library's choice).  The results do not depend on it."""
        check(self._lib.pla_engine_set_nonfactor_grid(self._h, int(max_workgroups)))

    # ------------------------------------------------------------------ reductions
    def reduce_pointwise(self, diag, loo_i, lppd_i, good_k):
        sp = self._space(loo_i)
        if sp.device is None:
            diag, loo_i, lppd_i = (np.ascontiguousarray(x, dtype=np.float64) for x in (diag, loo_i, lppd_i))
        agg = sp.new(AGG_COUNT, zero=True)
        p = sp.ptr
        check(self._lib.pla_reduce_pointwise(self._h, p(diag), p(loo_i), p(lppd_i), len(loo_i), float(good_k), sp.mem_space, sp.stream,
                                             p(agg)))
        return agg

    # ------------------------------------------------------------------ bench helpers
    def fill_synthetic(self, t, seed, row0=0, k_lo=0.05, k_hi=0.60, heavy_lo=0.0, heavy_hi=0.0):
        n, s = t.shape
        assert t.is_contiguous()
        check(self._lib.pla_fill_synthetic(self._h, _ptr(t), _code(t), n, s, int(row0), int(seed),
                                           k_lo, k_hi, heavy_lo, heavy_hi, self._stream()))

    def fill_synthetic_chains(self, t, seed, row0=0, chains=4, rho=0.9, offset_sd=0.3, k_lo=0.05, k_hi=0.60):
        """Rows as MCMC delivers them: chain-major stack of AR(1) chains with per-chain offsets (``pla_fill_synthetic_chains``)."""
        n, s = t.shape
        assert t.is_contiguous()
        check(self._lib.pla_fill_synthetic_chains(self._h, _ptr(t), _code(t), n, s, int(row0), int(seed), int(chains),
                                                  float(rho), float(offset_sd), k_lo, k_hi, self._stream()))

    def set_frozen(self, on):
        """Frozen: calls that would reallocate engine workspace fail (EngineError -6) instead of invalidating the
        raw pointers a captured HIP graph holds (include/pyloo_amd.h, "HIP graphs")."""
        check(self._lib.pla_engine_set_frozen(self._h, 1 if on else 0))

    def set_timing(self, on):
        check(self._lib.pla_engine_set_timing(self._h, 1 if on else 0))

    def kernel_ms(self):
        ms, k = C.c_double(0), C.c_int64(0)
        check(self._lib.pla_engine_kernel_ms(self._h, C.byref(ms), C.byref(k)))
        return ms.value, k.value

    def first_kernel_ms(self):
        """Accumulated time of the first (dominant) kernel of the two-kernel PSIS-LOO passes since the last call."""
        ms, k = C.c_double(0), C.c_int64(0)
        check(self._lib.pla_engine_first_kernel_ms(self._h, C.byref(ms), C.byref(k)))
        return ms.value, k.value

    def last_kernels(self):
        """Which kernels the last PSIS-LOO / weights / group / e_loo / WAIC call launched (text; for benchmark records and
        tests).  After ``waic``: ``waic_wave_kernel<T, W>``, ``waic_rows_kernel<T>`` or ``waic_col_kernel<T>``, behind
        ``transpose_rows_kernel + `` on the ``PLA_INGEST_TRANSPOSE`` path and followed by ``(blocks of observations uploaded)``
        for a host matrix."""
        buf = C.create_string_buffer(512)
        check(self._lib.pla_engine_last_kernels(self._h, buf, 512))
        return buf.value.decode("utf-8", "replace")

    def stream_gave_up(self):
        """Streamed passes since the last call in which the fit kernel stopped waiting for the sweep (``pla_engine_stream_stats``;
        synchronises the device).  0 in a healthy run."""
        n = C.c_int64(0)
        check(self._lib.pla_engine_stream_stats(self._h, C.byref(n)))
        return int(n.value)

    def aggregate_pack(self, agg, rank, world, table):
        """``table`` (world x 8, this engine's device) = zeros except row ``rank`` = ``agg``: one kernel on the current stream."""
        check(self._lib.pla_aggregate_pack(self._h, _ptr(agg), int(rank), int(world), _ptr(table), self._stream()))

    def aggregate_merge(self, table, world, out):
        """``out`` (8) = the per-rank aggregate rows of ``table`` merged (Chan, Golub & LeVeque): one kernel on the current stream."""
        check(self._lib.pla_aggregate_merge(self._h, _ptr(table), int(world), _ptr(out), self._stream()))


def get_engine(device=None):
    """Process-wide engine for ``device`` (default: torch's current CUDA device, else 0)."""
    if device is None:
        device = 0
        try:
            import torch

            if torch.cuda.is_available():
                device = torch.cuda.current_device()
        except Exception:
            device = 0
    with _lock:
        eng = _engines.get(device)
        if eng is None:
            eng = _engines[device] = Engine(device)
        return eng
