"""``loo_moment_match()`` -- moment matching for the observations with a high Pareto k, with the reference's signature and result
(pyloo/loo_moment_match.py:34-653, the callback path; pyloo/split_moment_match.py:20-263), batched over the observations.

The reference works one observation at a time.  Only the iterations of ONE observation are sequential; here all observations above
the threshold walk the stages in lock step and the device work of a stage runs once for the whole batch:

* ``pla_mm_moments``: the plain and weighted first and second moments of every active observation's draws;
* ``pla_mm_transform``: the affine map of the draws (shift / shift-and-scale / shift-and-cov, and the two halves of the split step);
* the model evaluations: the caller's callbacks;
* ``pla_mm_ratios``: the ratios with their NaN / +inf rules, stacked for ONE ``Engine.importance_weights`` call (PSIS on rows);
* the accept / reject decision ``k_new < k`` and the D x D factorisations (``cholesky``, ``inv``, ``det``, the product for
  ``total_mapping``) in host NumPy on the B * D^2 numbers copied back -- they are tiny, and the ``LinAlgError`` -> identity fallback
  is then the reference's own.

Everything the reference does around that is kept: the validation of the callbacks and of what they return (messages included), the
default ``k_threshold``, the stage order, the accumulation of the totals, the ``break`` / ``continue`` rules around a failing callback,
both ``max_iters`` warnings, the split step when ``split and iterind > 1``, ``update_loo_data_i`` and the two closing warnings.  Its
oddities are kept too: with D = 1 ``np.cov`` is 0-d, ``np.linalg.cholesky`` raises and the mapping is the identity; the closing
warning reads ``ks`` (loo_moment_match.py:639), an alias of the array ``update_loo_data_i`` writes into, so in effect it looks at
the UPDATED k values; ``kfi`` stays 0 for an observation that no stage improved; ``p_loo`` is the sum of
``p_loo_i``, which starts at zero when the input has none.

Deliberate departures from the reference:

* A ``PyMCWrapper`` model raises ``NotImplementedError`` (there is no PyMC here; ``loo(moment_match=True)`` stays as it is), and
  ``compute_updated_r_eff``, which only the wrapper path uses, is not carried over.
* ``r_eff_i`` is the ``r_eff`` argument, a scalar.  The reference derives it from ArviZ's ESS when ``log_lik_i`` returns a 2-D array
  (a case its own validation rejects first); here that case raises a ``TypeError`` that points to ``r_eff``.
* ``p_loo_i`` is stored in the result's index (``out["p_loo_i"]``; the reference sets an attribute).
* With ``batched=True`` the callbacks see all active observations at once; a callback that raises then fails the stage for all of
  them (with ``batched=False``, the reference's protocol, for the one observation it was called for).
* The reference logs per observation while it goes; the messages here come per stage.

Data: if ``unconstrain_pars`` returns a torch CUDA tensor everything stays on that device and the callbacks receive CUDA tensors
(no copies); if it returns a NumPy array it is uploaded once and the callbacks receive NumPy arrays (one copy per call).  All
arithmetic is float64.  Limits: D <= 64 with ``cov=True``, D <= 1024 with ``cov=False`` (``ValueError``).

``last_trace`` holds, after every call, per processed observation the stage decisions (``"sh+sc-co-"``: shift accepted, scale and
covariance rejected; ``!`` a failed stage), every intermediate k and whether the split step ran.
"""

import inspect
import logging
import warnings
from copy import deepcopy

import numpy as np

from .base import ISMethod, parse_method, tail_count_for
from .engine import Engine, _is_torch_tensor, get_engine

__all__ = ["loo_moment_match", "loo_moment_match_split", "shift", "shift_and_scale", "shift_and_cov", "update_quantities_i"]

_log = logging.getLogger(__name__)

last_trace = {}

_STAGES = (("sh", "mean shift", "Mean shift"), ("sc", "scale shift", "Mean and scale shift"), ("co", "covariance shift", "Covariance shift"))


# ----------------------------------------------------------------------------------------------------------------- validation
def _validate_custom_function(func, expected_args, name):
    """The signature check of loo_moment_match.py:1101-1116: ``**kwargs`` covers every expected argument."""
    params = inspect.signature(func).parameters
    if not any(p.kind == inspect.Parameter.VAR_KEYWORD for p in params.values()):
        missing = [a for a in expected_args if a not in params]
        if missing:
            raise ValueError(f"Custom function '{name}' is missing required parameters: {missing}. "
                             f"Expected signature should include: {expected_args}")
    return True


def _validate_output(array, name, expected_ndim=None):
    """loo_moment_match.py:1119-1157 for ndarrays and CUDA tensors: not None, numeric, no NaN, the expected number of dimensions.
    Returns a float64 ndarray, or the float64 tensor."""
    if array is None:
        raise ValueError(f"Function returned None for {name}. Please check your custom function implementation.")
    if _is_torch_tensor(array):
        import torch

        array = array.to(torch.float64)
        has_nan, ndim = bool(torch.isnan(array).any()), array.dim()
    else:
        try:
            array = np.asarray(array, dtype=np.float64)
        except Exception as e:
            raise ValueError(f"Could not convert {name} to numpy array: {e}. Please ensure your function returns numeric data.") from e
        has_nan, ndim = bool(np.any(np.isnan(array))), array.ndim
    if has_nan:
        raise ValueError(f"NaN values detected in {name}. Please check your function for division by"
                         " zero, log of negative values, or other numerical issues.")
    if expected_ndim is not None and ndim != expected_ndim:
        raise ValueError(f"Expected {expected_ndim} dimensions for {name}, got {ndim}. Please reshape your output accordingly.")
    return array


def _is_pymc_wrapper(model):
    return any(c.__name__ == "PyMCWrapper" for c in type(model).__mro__)


def _refuse_wrapper(model):
    if _is_pymc_wrapper(model):
        raise NotImplementedError("loo_moment_match with a PyMCWrapper model is outside the scope of pyloo_amd: pass the five "
                                  "callbacks (post_draws, log_lik_i, unconstrain_pars, log_prob_upars_fn, log_lik_i_upars_fn)")


# ------------------------------------------------------------------------------------------------------------ the model's side
class _Callbacks:
    """The caller's ``log_prob_upars_fn`` / ``log_lik_i_upars_fn`` / ``log_lik_i`` behind one protocol: CUDA (B, S, D) in, CUDA
    (B, S) float64 out plus ``{b: exception}`` for the observations whose evaluation failed (their rows hold zeros)."""

    def __init__(self, model, log_prob_upars_fn, log_lik_i_upars_fn, log_lik_i, batched, on_device, device, kwargs):
        self.model, self.lp_fn, self.ll_fn, self.ll0_fn = model, log_prob_upars_fn, log_lik_i_upars_fn, log_lik_i
        self.batched, self.on_device, self.device, self.kwargs = batched, on_device, device, kwargs

    def _arg(self, U):
        return U if self.on_device else U.detach().cpu().numpy()

    def _rows(self, B, S, call_all, call_one, name_of, wrap, check_nan=True):
        """``call_all()`` (batched: a (B, S) result) or ``call_one(b)`` per observation (an (S,) result), validated as the
        reference validates (``wrap(b, e)`` turns a failure into the reference's ``ValueError``)."""
        import torch

        out = torch.zeros((B, S), dtype=torch.float64, device=self.device)
        errors = {}
        if self.batched:
            try:
                res = call_all()
                if res is None:
                    raise ValueError(f"Function returned None for {name_of(0)}. Please check your custom function implementation.")
                res = res.to(torch.float64) if _is_torch_tensor(res) else _from_numpy(res)
                if tuple(res.shape) != (B, S):
                    raise ValueError(f"Expected shape {(B, S)} for the batched {name_of(0)}, got {tuple(res.shape)}.")
                out = res.to(self.device).contiguous()
                for b in (torch.nonzero(torch.isnan(out).any(dim=1)).reshape(-1).tolist() if check_nan else ()):
                    errors[b] = wrap(b, ValueError(f"NaN values detected in {name_of(b)}. Please check your function for division by"
                                                   " zero, log of negative values, or other numerical issues."))
            except Exception as e:
                errors = {b: wrap(b, e) for b in range(B)}
            return out, errors
        for b in range(B):
            try:
                row = call_one(b)
                if check_nan:
                    row = _validate_output(row, name_of(b), expected_ndim=1)
                row = (row if _is_torch_tensor(row) else _from_numpy(row)).reshape(-1)
                if row.numel() != S:
                    raise ValueError(f"Expected {S} values for {name_of(b)}, got {row.numel()}.")
                out[b] = row.to(self.device)
            except Exception as e:
                errors[b] = wrap(b, e)
        return out, errors

    def log_prob(self, U, name="log_prob_new", check_nan=True):
        B, S = int(U.shape[0]), int(U.shape[1])
        arg = self._arg(U)
        wrap = lambda b, e: _chain(ValueError(f"Error computing log probability: {e}. Make sure your"  # noqa: E731
                                              " log_prob_upars_fn function returns a 1D array of log probabilities."), e)
        return self._rows(B, S, lambda: self.lp_fn(self.model, upars=arg, **self.kwargs),
                          lambda b: self.lp_fn(self.model, upars=arg[b], **self.kwargs), lambda b: name, wrap, check_nan)

    def log_lik(self, U, obs, check_nan=True):
        B, S = int(U.shape[0]), int(U.shape[1])
        arg = self._arg(U)
        wrap = lambda b, e: _chain(ValueError(f"Error computing log likelihood for observation {obs[b]}: {e}. Make sure"  # noqa: E731
                                              " your log_lik_i_upars_fn function returns a 1D array of log likelihoods."), e)
        return self._rows(B, S, lambda: self.ll_fn(self.model, upars=arg, i=self._obs_arg(obs), **self.kwargs),
                          lambda b: self.ll_fn(self.model, upars=arg[b], i=int(obs[b]), **self.kwargs),
                          lambda b: f"log_liki_new for obs {obs[b]}", wrap, check_nan)

    def _obs_arg(self, obs):
        if not self.on_device:
            return np.asarray(obs, dtype=np.int64)
        import torch

        return torch.as_tensor(np.asarray(obs, dtype=np.int64), device=self.device)

    def log_lik_original(self, obs, S):
        """``log_lik_i(model, i)`` of every observation of the batch.  A failure raises, as in the reference."""
        import torch

        def check_2d(res, limit):
            if len(getattr(res, "shape", np.shape(res))) > limit:
                raise TypeError("log_lik_i returned an array with a chain dimension.  pyloo_amd does not derive the relative efficiency "
                                "from it: return the stacked (S,) draws and pass r_eff= to loo_moment_match")

        out = torch.empty((len(obs), S), dtype=torch.float64, device=self.device)
        if self.batched:
            res = self.ll0_fn(self.model, self._obs_arg(obs), **self.kwargs)
            check_2d(res, 2)
            try:
                res = _validate_output(res, f"log_lik for observations {list(obs)}", expected_ndim=2)
                if tuple(res.shape) != (len(obs), S):
                    raise ValueError(f"Expected shape {(len(obs), S)}, got {tuple(res.shape)}.")
            except Exception as e:
                raise ValueError(f"Error computing log likelihood for observations {list(obs)}: {e}. Make sure your log_lik_i function "
                                 "returns the log likelihood for the specified observations as a (B, S) array.") from e
            return (res if _is_torch_tensor(res) else _from_numpy(res)).to(self.device).contiguous()
        for b, i in enumerate(obs):
            res = self.ll0_fn(self.model, int(i), **self.kwargs)
            check_2d(res, 1)
            try:
                row = _validate_output(res, f"log_lik for observation {i}", expected_ndim=1)
                if len(row) != S:
                    raise ValueError(f"Expected {S} values, got {len(row)}.")
            except Exception as e:
                raise ValueError(f"Error computing log likelihood for observation {i}: {e}. Make sure your log_lik_i function returns "
                                 "the log likelihood for the specified observation as a 1D array.") from e
            out[b] = (row if _is_torch_tensor(row) else _from_numpy(row)).to(self.device)
        return out


def _chain(err, cause):
    err.__cause__ = cause
    return err


def _h(t):
    """Device -> host float64 ndarray."""
    return t.detach().cpu().numpy()


def _from_numpy(a):
    """``torch.from_numpy`` of a float64 C-contiguous copy when ``a`` is not one already (or is read-only)."""
    import torch

    a = np.asarray(a, dtype=np.float64)
    if not (a.flags.c_contiguous and a.flags.writeable):
        a = np.array(a, dtype=np.float64, order="C")
    return torch.from_numpy(a)


def _d(a, device):
    return _from_numpy(a).to(device)


# ------------------------------------------------------------------------------------------------------------- the transforms
def _mappings(covs, warn=True):
    """``chol(wcov).T @ inv(chol(cov).T)`` per observation (loo_moment_match.py:895-908), the identity where NumPy refuses."""
    B, _, D, _ = covs.shape
    out = np.empty((B, D, D))
    for b in range(B):
        covv, wcovv = (covs[b, 0], covs[b, 1]) if D > 1 else (covs[b, 0].reshape(()), covs[b, 1].reshape(()))  # (np.cov of one column is 0-d)
        try:
            chol1 = np.linalg.cholesky(wcovv)
            chol2 = np.linalg.cholesky(covv)
            out[b] = chol1.T @ np.linalg.inv(chol2.T)
        except np.linalg.LinAlgError as e:
            if warn:
                warnings.warn(f"Cholesky decomposition failed during covariance matching: {e}. Using identity mapping instead.",
                              stacklevel=4)
            out[b] = np.eye(D)
    return out


def _transform(eng, U, lw, kind):
    """One stage's transform of a CUDA batch: ``(U_new, shift, scaling or None, mapping or None)``, the last three on the host."""
    dev = U.device
    stats, covs = eng.mm_moments(U, lw, cov=kind == "co")
    st = _h(stats)
    mean, wmean = st[:, 0], st[:, 1]
    sh = wmean - mean
    if kind == "sh":  # upars + shift, in that form
        return eng.mm_transform(U, _d(-sh, dev), _d(np.zeros_like(sh), dev)), sh, None, None
    if kind == "sc":
        with np.errstate(all="ignore"):
            scaling = np.sqrt(st[:, 3] / st[:, 2])
        return eng.mm_transform(U, _d(mean, dev), _d(wmean, dev), pre=_d(scaling, dev)), sh, scaling, None
    mapping = _mappings(_h(covs))
    return eng.mm_transform(U, _d(mean, dev), _d(wmean, dev), mapping=_d(mapping, dev)), sh, None, mapping


def _as_batch(upars, lwi):
    """The public transforms take (S, D) with (S,) or (B, S, D) with (B, S), ndarray or CUDA tensor: ``(U, lw, single, on_device)``."""
    import torch

    on_device = _is_torch_tensor(upars) and upars.is_cuda
    if not on_device and not torch.cuda.is_available():
        get_engine()  # raises: no CPU fallback
    dev = upars.device if on_device else torch.device("cuda", get_engine().device)
    conv = lambda a: (a if _is_torch_tensor(a) else _from_numpy(a)).to(device=dev, dtype=torch.float64)  # noqa: E731
    U, lw = conv(upars), conv(lwi)
    single = U.dim() == 2
    if single:
        U, lw = U[None], lw[None]
    if U.dim() != 3 or lw.dim() != 2 or tuple(lw.shape) != tuple(U.shape[:2]):
        raise ValueError("expected upars (S, D) with lwi (S,), or upars (B, S, D) with lwi (B, S)")
    return U.contiguous(), lw.contiguous(), single, on_device


def _public_transform(upars, lwi, kind):
    U, lw, single, on_device = _as_batch(upars, lwi)
    eng = get_engine(U.device.index)
    new, sh, scaling, mapping = _transform(eng, U, lw, kind)
    out = {"upars": new if on_device else _h(new), "shift": _d(sh, U.device) if on_device else sh}
    if scaling is not None:
        out["scaling"] = _d(scaling, U.device) if on_device else scaling
    if mapping is not None:
        out["mapping"] = _d(mapping, U.device) if on_device else mapping
    return {k: v[0] for k, v in out.items()} if single else out


def shift(upars, lwi):
    """Shift the draws to their weighted mean (loo_moment_match.py:814-836): ``dict(upars, shift)``.  ``upars`` (S, D) with ``lwi``
    (S,), or a batch (B, S, D) with (B, S); NumPy in, NumPy out -- CUDA tensors in, CUDA tensors out."""
    return _public_transform(upars, lwi, "sh")


def shift_and_scale(upars, lwi):
    """Shift to the weighted mean and match the marginal variances (loo_moment_match.py:839-870): ``dict(upars, shift, scaling)``."""
    return _public_transform(upars, lwi, "sc")


def shift_and_cov(upars, lwi):
    """Shift to the weighted mean and match the covariance (loo_moment_match.py:873-914): ``dict(upars, shift, mapping)``; D <= 64."""
    return _public_transform(upars, lwi, "co")


# ---------------------------------------------------------------------------------------------------------- update_quantities
def _update_batch(eng, cb, U, obs, lp_orig, M, method):
    """loo_moment_match.py:743-811 for a CUDA batch: ``(lw, lwf, k, kf, ll, errors)``; k and kf on the host."""
    B = int(U.shape[0])
    lp, err_lp = cb.log_prob(U)
    ll, err_ll = cb.log_lik(U, obs)
    errors = {**err_ll, **err_lp}  # (the reference evaluates log_prob first: its failure is the one reported)
    lr2 = eng.mm_ratios("update", ll, lp, lp_orig)
    lw2, k2 = eng.importance_weights(lr2, M, method)
    k2 = _h(k2)
    return lw2[:B], lw2[B:], k2[:B], k2[B:], ll, errors


def update_quantities_i(model, upars, i, orig_log_prob, r_eff_i, converter=None, log_prob_upars_fn=None, log_lik_i_upars_fn=None,
                        method="psis", verbose=False, batched=False, **kwargs):
    """New weights, Pareto k and log-likelihood of observation ``i`` at transformed draws (loo_moment_match.py:656-811):
    ``dict(lwi, lwfi, ki, kfi, log_liki)``.  ``upars`` (S, D) with a scalar ``i``, or (B, S, D) with ``i`` (B,); ``batched`` says whether
    the callbacks take the whole batch.  NumPy in, NumPy out -- CUDA tensors in, CUDA tensors out."""
    import torch

    _refuse_wrapper(model)
    if log_prob_upars_fn is None or log_lik_i_upars_fn is None:
        raise ValueError("log_prob_upars_fn and log_lik_i_upars_fn must be provided when not using PyMCWrapper")
    method = parse_method(method)
    on_device = _is_torch_tensor(upars) and upars.is_cuda
    if not on_device and not torch.cuda.is_available():
        get_engine()  # raises: no CPU fallback
    dev = upars.device if on_device else torch.device("cuda", get_engine().device)
    U = (upars if _is_torch_tensor(upars) else _from_numpy(upars)).to(device=dev, dtype=torch.float64)
    single = U.dim() == 2
    U = (U[None] if single else U).contiguous()
    obs = [int(i)] if single else [int(v) for v in (i.tolist() if hasattr(i, "tolist") else i)]
    S = int(U.shape[1])
    lp_orig = (orig_log_prob if _is_torch_tensor(orig_log_prob) else _from_numpy(orig_log_prob))
    lp_orig = lp_orig.to(device=dev, dtype=torch.float64).reshape(-1)
    eng = get_engine(dev.index)
    cb = _Callbacks(model, log_prob_upars_fn, log_lik_i_upars_fn, None, batched and not single, on_device, dev, kwargs)
    M = tail_count_for(S, r_eff_i) if method == ISMethod.PSIS else 0
    lw, lwf, k, kf, ll, errors = _update_batch(eng, cb, U, obs, lp_orig, M, method.value)
    if errors:
        raise errors[min(errors)]
    conv = (lambda t: t) if on_device else _h
    out = {"lwi": conv(lw), "lwfi": conv(lwf), "ki": k, "kfi": kf, "log_liki": conv(ll)}
    return {key: v[0] for key, v in out.items()} if single else out


# ---------------------------------------------------------------------------------------------------------------- split step
def _split_batch(eng, cb, upars, mean, cov, tshift, tscale, tmap, obs, M, method, want_full=True):
    """split_moment_match.py:132-263 for a batch: ``upars`` (S, D) CUDA, the original draws; ``mean`` (D,) their mean (host);
    the totals (B, D), (B, D), (B, D, D) on the host.  Returns ``(lw, lwf or None, ll, errors)``."""
    dev = upars.device
    B, S = len(obs), int(upars.shape[0])
    half = S // 2
    m = np.broadcast_to(mean, tshift.shape)
    inv = np.empty_like(tmap)
    jac = np.empty((B, 2))
    errors = {}
    for b in range(B):
        try:
            inv[b] = np.linalg.inv(tmap[b]) if cov else np.eye(tmap.shape[1])
            with np.errstate(all="ignore"):
                jac[b] = np.sum(np.log(tscale[b])), np.log(np.abs(np.linalg.det(tmap[b])))
        except Exception as e:  # (a singular total mapping: the reference's np.linalg.inv raises inside its split step)
            errors[b] = e
            inv[b], jac[b] = np.eye(tmap.shape[1]), 0.0
    fwd = eng.mm_transform(upars, _d(m, dev), _d(tshift + m, dev), pre=_d(tscale, dev), mapping=_d(tmap, dev) if cov else None,
                           rows=(0, half))
    bwd = eng.mm_transform(upars, _d(m, dev), _d(m - tshift, dev), mapping=_d(inv, dev) if cov else None, post_div=_d(tscale, dev),
                           rows=(half, S))
    # (the reference's split step does not validate what the callbacks return: NaN flows into the rules of the ratio kernel)
    lp_f, e1 = cb.log_prob(fwd, "log_prob_half_trans", check_nan=False)
    lp_b, e2 = cb.log_prob(bwd, "log_prob_half_trans_inv", check_nan=False)
    ll, e3 = cb.log_lik(fwd, obs, check_nan=False)
    for b, e in {**e3, **e2, **e1}.items():
        errors.setdefault(b, e)
    raw = eng.mm_ratios("split", ll, lp_f, lp_b, _d(jac, dev))
    lw, _ = eng.importance_weights(raw, M, method)
    lwf = None
    if want_full:
        lwf, _ = eng.importance_weights(eng.mm_ratios("sum", lw, ll), M, method)
    return lw, lwf, ll, errors


def loo_moment_match_split(model, upars, cov, total_shift, total_scaling, total_mapping, i, r_eff_i, log_prob_upars_fn=None,
                           log_lik_i_upars_fn=None, method="psis", batched=False, **kwargs):
    """The split step (split_moment_match.py:20-263): the first half of the draws under the accumulated transform, the second half
    under its inverse, combined by multiple importance sampling.  ``upars`` (S, D), the ORIGINAL draws; the totals (D,), (D,),
    (D, D) with a scalar ``i``, or (B, D), (B, D), (B, D, D) with ``i`` (B,).  Returns ``dict(lwi, lwfi, log_liki, r_eff_i)``; NumPy
    in, NumPy out -- CUDA tensors in, CUDA tensors out.  ``None`` totals stand for no shift, unit scaling, identity mapping."""
    import torch

    _refuse_wrapper(model)
    if log_prob_upars_fn is None or log_lik_i_upars_fn is None:
        raise ValueError("When not using PyMCWrapper, you must provide the following functions: "
                         "log_prob_upars_fn and log_lik_i_upars_fn")
    method = parse_method(method)
    on_device = _is_torch_tensor(upars) and upars.is_cuda
    if not on_device and not torch.cuda.is_available():
        get_engine()  # raises: no CPU fallback
    dev = upars.device if on_device else torch.device("cuda", get_engine().device)
    U = (upars if _is_torch_tensor(upars) else _from_numpy(upars)).to(device=dev, dtype=torch.float64)
    if U.dim() != 2:
        raise ValueError("upars: expected the original (S, D) draws")
    U = U.contiguous()
    S, D = int(U.shape[0]), int(U.shape[1])
    single = np.ndim(i) == 0
    obs = [int(i)] if single else [int(v) for v in (i.tolist() if hasattr(i, "tolist") else i)]
    B = len(obs)
    host = lambda a: _h(a) if _is_torch_tensor(a) else np.asarray(a, dtype=np.float64)  # noqa: E731
    tshift = np.zeros((B, D)) if total_shift is None else host(total_shift).reshape(B, D)
    tscale = np.ones((B, D)) if total_scaling is None else host(total_scaling).reshape(B, D)
    tmap = np.broadcast_to(np.eye(D), (B, D, D)).copy() if total_mapping is None else host(total_mapping).reshape(B, D, D)
    eng = get_engine(dev.index)
    eng.mm_check_dim(D, bool(cov))
    cb = _Callbacks(model, log_prob_upars_fn, log_lik_i_upars_fn, None, batched and not single, on_device, dev, kwargs)
    M = tail_count_for(S, r_eff_i) if method == ISMethod.PSIS else 0
    mean = _h(eng.mm_moments(U[None], torch.zeros((1, S), dtype=torch.float64, device=dev))[0])[0, 0]
    lw, lwf, ll, errors = _split_batch(eng, cb, U, mean, bool(cov), tshift, tscale, tmap, obs, M, method.value)
    if errors:
        raise errors[min(errors)]
    conv = (lambda t: t) if on_device else _h
    out = {"lwi": conv(lw), "lwfi": conv(lwf), "log_liki": conv(ll)}
    out = {k: v[0] for k, v in out.items()} if single else out
    out["r_eff_i"] = r_eff_i
    return out


# ------------------------------------------------------------------------------------------------------------------ the front
def _values(x):
    return getattr(x, "values", x)


def _summary(pareto_k, original_ks, k_threshold, verbose):
    """The closing log lines (loo_moment_match.py:1042-1098)."""
    better = np.where(pareto_k < original_ks)[0]
    if len(better):
        _log.info(f"Improved Pareto k for {len(better)} observations. Average improvement:"
                  f" {np.mean(original_ks[better] - pareto_k[better]):.4f}")
        if verbose:
            for idx in better:
                _log.info(f"  Observation {idx}: {original_ks[idx]:.4f} -> {pareto_k[idx]:.4f} (improvement:"
                          f" {original_ks[idx] - pareto_k[idx]:.4f})")
    else:
        _log.info("No improvements in Pareto k values")
    high = np.where(pareto_k > k_threshold)[0]
    if len(high):
        _log.info(f"{len(high)} observations still have Pareto k > {k_threshold}")
        if verbose:
            for idx in high:
                _log.info(f"  Observation {idx}: Pareto k = {pareto_k[idx]:.4f}")


def _run_chunk(eng, cb, upars, mean, lp_orig, obs, ks, M, method, max_iters, k_threshold, split, cov, verbose):
    """All observations of one chunk through the iterations in lock step.  Returns per observation ``(elpd, lpd, k, kf)`` and
    fills ``last_trace``."""
    import torch

    dev = upars.device
    B, (S, D) = len(obs), (int(v) for v in upars.shape)
    ll = cb.log_lik_original(obs, S).clone()  # (it may be the caller's own tensor; accepted rows are written into it)
    lw, initial_k = eng.importance_weights(-ll, M, method)
    for i, k0 in zip(obs, _h(initial_k)):
        _log.info(f"Observation {i}: Initial Pareto k = {k0:.4f}")
    U = upars[None].expand(B, S, D).contiguous()
    ki = np.array([ks[i] for i in obs], dtype=np.float64)
    kfi = np.zeros(B)
    tshift, tscale = np.zeros((B, D)), np.ones((B, D))
    tmap = np.broadcast_to(np.eye(D), (B, D, D)).copy()
    iterind = np.ones(B, dtype=np.int64)
    alive = np.ones(B, dtype=bool)
    trace = {i: {"decisions": "", "ks": [], "split": False, "loop_ks": []} for i in obs}
    kinds = _STAGES if cov else _STAGES[:2]
    while True:
        act = [b for b in range(B) if alive[b] and iterind[b] <= max_iters and ki[b] > k_threshold]
        for b in range(B):
            if alive[b]:
                trace[obs[b]]["loop_ks"].append(float(ki[b]))
                alive[b] = b in act  # (an observation that left the loop does not come back)
        if not act:
            break
        for b in act:
            if iterind[b] == max_iters:
                warnings.warn("Maximum number of moment matching iterations reached. Increasing max_iters may improve accuracy.",
                              stacklevel=3)
        improved = np.zeros(B, dtype=bool)
        for tag, what, title in kinds:
            if not act:
                break
            sel = torch.as_tensor(act, device=dev)
            whole = len(act) == B
            Ua, lwa = (U, lw) if whole else (U.index_select(0, sel), lw.index_select(0, sel))
            new, sh, scaling, mapping = _transform(eng, Ua, lwa, tag)
            lw_n, _, k_n, kf_n, ll_n, errors = _update_batch(eng, cb, new, [obs[b] for b in act], lp_orig, M, method)
            take, still = [], []
            for a, b in enumerate(act):
                i = obs[b]
                if a in errors:
                    trace[i]["decisions"] += tag + "!"
                    warnings.warn(f"Error during {what} for observation {i}: {errors[a]}. Skipping this transformation.", stacklevel=3)
                    if tag == "sh" or not improved[b]:
                        alive[b] = False  # break
                    continue  # (after an improvement: on to the next iteration)
                still.append(b)
                trace[i]["ks"].append(float(k_n[a]))
                if k_n[a] < ki[b]:
                    _log.info(f"Observation {i}: {title} improved Pareto k from {ki[b]:.4f} to {k_n[a]:.4f}")
                    trace[i]["decisions"] += tag + "+"
                    take.append(a)
                    tshift[b] += sh[a]
                    if scaling is not None:
                        tscale[b] *= scaling[a]
                    if mapping is not None:
                        tmap[b] = mapping[a] @ tmap[b]
                    ki[b], kfi[b] = k_n[a], kf_n[a]
                    iterind[b] += 1
                    improved[b] = True
                else:
                    trace[i]["decisions"] += tag + "-"
                    if verbose:
                        _log.info(f"{title} did not improve Pareto k: {ki[b]:.4f} vs {k_n[a]:.4f}")
            if take:
                if len(take) == B:
                    U, lw, ll = new, lw_n, ll_n.clone()  # (ll_n may be the caller's own tensor)
                else:
                    src = torch.as_tensor(take, device=dev)
                    dst = torch.as_tensor([act[a] for a in take], device=dev)
                    U.index_copy_(0, dst, new.index_select(0, src))
                    lw.index_copy_(0, dst, lw_n.index_select(0, src))
                    ll.index_copy_(0, dst, ll_n.index_select(0, src))
            act = still
        for b in act:  # (those that went through every stage)
            if not improved[b]:
                _log.info(f"Observation {obs[b]}: No further improvement after {iterind[b] - 1} iterations. Final Pareto k = {ki[b]:.4f}")
                alive[b] = False
    if max_iters == 1:
        for _ in obs:
            warnings.warn("Maximum number of moment matching iterations reached with max_iters=1."
                          " Increasing max_iters may improve accuracy.", stacklevel=3)
    todo = [b for b in range(B) if split and iterind[b] > 1]
    if todo:
        for b in todo:
            _log.info(f"Performing split transformation for observation {obs[b]}")
        lw_s, _, ll_s, errors = _split_batch(eng, cb, upars, mean, cov, tshift[todo], tscale[todo], tmap[todo], [obs[b] for b in todo], M,
                                             method, want_full=False)
        good = [a for a in range(len(todo)) if a not in errors]
        for a, e in errors.items():
            warnings.warn(f"Split transformation failed for observation {obs[todo[a]]}: {e}. "
                          "Using the last successful transformation instead.", stacklevel=3)
        if good:
            src = torch.as_tensor(good, device=dev)
            dst = torch.as_tensor([todo[a] for a in good], device=dev)
            lw, ll = lw.clone(), ll.clone()
            lw.index_copy_(0, dst, lw_s.index_select(0, src))
            ll.index_copy_(0, dst, ll_s.index_select(0, src))
            for a in good:
                trace[obs[todo[a]]]["split"] = True
    fin = _h(eng.mm_ratios("finish", ll, lw))
    last_trace.update(trace)
    return fin[:, 0], fin[:, 1], ki, kfi


def loo_moment_match(model, loo_data, post_draws=None, log_lik_i=None, unconstrain_pars=None, log_prob_upars_fn=None,
                     log_lik_i_upars_fn=None, max_iters=30, k_threshold=None, split=True, cov=True, method="psis", verbose=False,
                     r_eff=1.0, batched=False, batch_size=None, **kwargs):
    """Moment matching for the observations of ``loo_data`` whose Pareto k exceeds ``k_threshold`` (pyloo.loo_moment_match, the
    callback path).  Returns an updated deep copy of ``loo_data``; the input is left untouched.

    ``model`` is whatever the callbacks understand.  ``post_draws(model)`` -> the posterior draws; ``unconstrain_pars(model, pars)``
    -> the (S, D) unconstrained draws, a NumPy array or a torch CUDA tensor (which decides what the other callbacks receive and
    where the data lives); ``log_prob_upars_fn(model, upars)`` -> (S,) log density; ``log_lik_i(model, i)`` -> (S,) log-likelihood of
    observation ``i`` at the original draws; ``log_lik_i_upars_fn(model, upars, i)`` -> the same at ``upars``.  With ``batched=True``
    the last three take the active observations together: ``upars`` (B, S, D), ``i`` (B,), returning (B, S).  ``batch_size`` caps B
    (default: B * S * D * 8 bytes within 1 GiB).  ``r_eff`` is the relative efficiency handed to PSIS (a scalar).  ``max_iters``,
    ``k_threshold`` (default ``min(1 - 1 / log10(S), 0.7)``), ``split``, ``cov``, ``method``, ``verbose`` and ``**kwargs`` (passed to
    every callback) as in the reference.  See the module docstring for the deviations and the limits on D."""
    _log.setLevel(logging.INFO if verbose else logging.WARNING)
    _refuse_wrapper(model)
    method = parse_method(method)
    kind = loo_data.method
    loo_data = deepcopy(loo_data)
    loo_data.method = kind
    required = {"post_draws": post_draws, "log_lik_i": log_lik_i, "unconstrain_pars": unconstrain_pars,
                "log_prob_upars_fn": log_prob_upars_fn, "log_lik_i_upars_fn": log_lik_i_upars_fn}
    missing = [name for name, func in required.items() if func is None]
    if missing:
        raise ValueError("When not using PyMCWrapper, you must provide all the following"
                         f" functions: {', '.join(required.keys())}. Missing: {', '.join(missing)}")
    _validate_custom_function(post_draws, ["model"], "post_draws")
    _validate_custom_function(log_lik_i, ["model", "i"], "log_lik_i")
    _validate_custom_function(unconstrain_pars, ["model", "pars"], "unconstrain_pars")
    _validate_custom_function(log_prob_upars_fn, ["model", "upars"], "log_prob_upars_fn")
    _validate_custom_function(log_lik_i_upars_fn, ["model", "upars", "i"], "log_lik_i_upars_fn")
    try:
        pars = post_draws(model, **kwargs)
        upars = _validate_output(unconstrain_pars(model, pars=pars, **kwargs), "upars", expected_ndim=2)
    except Exception as e:
        raise ValueError(f"Error getting unconstrained parameters: {e}. Make sure your "
                         "post_draws and unconstrain_pars functions are implemented correctly.") from e
    S, D = (int(v) for v in upars.shape)
    Engine.mm_check_dim(D, bool(cov))
    if k_threshold is None:
        k_threshold = min(1 - 1 / np.log10(S), 0.7)
    if "pareto_k" not in loo_data:
        raise ValueError("Moment matching requires pointwise LOO results with Pareto k values. "
                         "Please recompute LOO with pointwise=True before using moment_match=True.")
    try:
        lp_orig = log_prob_upars_fn(model, upars=upars, **kwargs)
        lp_orig = _validate_output(lp_orig, "orig_log_prob", expected_ndim=1)
    except Exception as e:
        raise ValueError(f"Error computing log probabilities: {e}. Make sure your "
                         "log_prob_upars_fn function is implemented correctly.") from e
    import torch

    on_device = _is_torch_tensor(upars) and upars.is_cuda
    if on_device:
        dev = upars.device
        eng = get_engine(dev.index)
        upars = upars.contiguous()
    else:
        eng = get_engine()  # raises without a GPU: there is no CPU fallback
        dev = torch.device("cuda", eng.device)
        upars = (upars if _is_torch_tensor(upars) else _from_numpy(upars)).to(dev).contiguous()
    cb = _Callbacks(model, log_prob_upars_fn, log_lik_i_upars_fn, log_lik_i, batched, on_device, dev, kwargs)
    lp_orig = (lp_orig if _is_torch_tensor(lp_orig) else _from_numpy(lp_orig)).to(dev).contiguous()

    pareto_k = np.array(_values(loo_data["pareto_k"]), dtype=np.float64)
    shape = pareto_k.shape
    pareto_k = pareto_k.reshape(-1)
    ks = pareto_k.copy()
    has_pointwise = "loo_i" in loo_data
    loo_i = np.array(_values(loo_data["loo_i"]), dtype=np.float64).reshape(-1) if has_pointwise else None
    p_loo_i = np.array(_values(loo_data["p_loo_i"]), dtype=np.float64).reshape(-1) if "p_loo_i" in loo_data else np.zeros_like(ks)
    bad_obs = np.where(ks > k_threshold)[0]
    _log.info(f"Found {len(bad_obs)} observations with Pareto k > {k_threshold}")
    kfs = np.zeros_like(ks)
    last_trace.clear()
    M = tail_count_for(S, r_eff) if method == ISMethod.PSIS else 0
    if batch_size is None:
        batch_size = max(1, (1 << 30) // (S * D * 8))
    batch_size = max(1, int(batch_size))
    mean = None
    if len(bad_obs):
        mean = _h(eng.mm_moments(upars[None], torch.zeros((1, S), dtype=torch.float64, device=dev))[0])[0, 0]
    for c0 in range(0, len(bad_obs), batch_size):
        obs = [int(i) for i in bad_obs[c0:c0 + batch_size]]
        elpd, lpd, k_new, kf_new = _run_chunk(eng, cb, upars, mean, lp_orig, obs, ks, M, method.value, max_iters, k_threshold, split,
                                              bool(cov), verbose)
        for a, i in enumerate(obs):  # update_loo_data_i (loo_moment_match.py:917-1039); the sums follow once, below
            if has_pointwise:
                _log.info(f"Observation {i}: ELPD changed from {loo_i[i]:.4f} to {elpd[a]:.4f} (diff: {elpd[a] - loo_i[i]:.4f})")
                loo_i[i] = elpd[a]
                p_loo_i[i] = lpd[a] - elpd[a]
            else:
                loo_data["elpd_loo"] = elpd[a]
                loo_data["p_loo"] = lpd[a] - elpd[a]
            _log.info(f"Observation {i}: Pareto k changed from {pareto_k[i]:.4f} to {k_new[a]:.4f} (improvement: {pareto_k[i] - k_new[a]:.4f})")
            pareto_k[i] = k_new[a]
            kfs[i] = kf_new[a]
    if len(bad_obs):
        if has_pointwise:
            n = loo_data["n_data_points"]
            loo_data["elpd_loo"] = np.sum(loo_i)
            loo_data["p_loo"] = np.sum(p_loo_i)
            loo_data["se"] = (n * np.var(loo_i)) ** 0.5
            loo_data["p_loo_se"] = (n * np.var(p_loo_i)) ** 0.5
        if "looic" in loo_data:
            loo_data["looic"] = -2 * loo_data["elpd_loo"]
            if "se" in loo_data:
                loo_data["looic_se"] = 2 * loo_data["se"]
    _store(loo_data, "pareto_k", pareto_k.reshape(shape))
    if has_pointwise:
        _store(loo_data, "loo_i", loo_i.reshape(shape))
        if "p_loo_i" in loo_data:
            _store(loo_data, "p_loo_i", p_loo_i.reshape(shape))
        else:
            like = loo_data["loo_i"]
            loo_data["p_loo_i"] = p_loo_i.reshape(shape)
            if hasattr(like, "values") and hasattr(like, "dims"):
                loo_data["p_loo_i"] = type(like)(p_loo_i.reshape(shape), dims=like.dims, coords=like.coords)
    _summary(pareto_k, ks, k_threshold, verbose)
    # (the reference tests ``ks``, which ALIASES the array update_loo_data_i writes into: in effect the updated values)
    if np.any(pareto_k > k_threshold):
        warnings.warn("Some Pareto k estimates are still above the threshold. "
                      "The model may be misspecified or the data may be highly influential.", stacklevel=2)
    if not split and np.any(kfs > k_threshold):
        warnings.warn("The accuracy of self-normalized importance sampling may be bad. "
                      "Setting split=True will likely improve accuracy.", stacklevel=2)
    return loo_data


def _store(loo_data, key, values):
    """Write a pointwise vector back where it came from: into the DataArray's buffer, or as a new ndarray."""
    cur = loo_data[key]
    if hasattr(cur, "values") and not isinstance(cur, np.ndarray):
        cur.values[...] = values
    else:
        loo_data[key] = values
