"""``relative_eff()`` -- the relative MCMC efficiency of the likelihood, one value per observation, on the HIP engine: the
``r_eff = relative_eff(exp(log_lik), chain_id)`` of R-loo: the ``reff`` that ``loo``, ``loo_from_matrix`` and ``loo_diagnostics``
take as a vector (every observation then has its own tail length) and whose mean the other PSIS entry points take.  The
reference has no such function (its ``reff=None`` asks ArviZ for the ESS of the posterior).

The estimator is Stan's effective sample size for the mean (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021; Geyer 1992's
initial positive and monotone sequences) without rank normalisation, on ``exp(log_lik - row maximum)``; include/pyloo_amd.h
states it in full.  ``split=False`` is R-loo's ``relative_eff``, ``split=True`` the split-chain convention of ArviZ / posterior.

    r = pl.relative_eff_from_matrix(ll, n_chains=4)
    res = pl.loo_from_matrix(ll, reff=r)
    d = pl.loo_diagnostics_from_matrix(ll, reff=r)   # n_eff and the Monte Carlo error of every loo_i (loo_diagnostics.py)

Out of scope: per-observation tail lengths inside the PSIS kernels (the engine takes one per pass: a vector is run bucket by
bucket of equal tail length, ``base.tail_buckets``), rank-normalised / bulk / tail ESS, and any change to what ``reff=None``
does in ``loo``.
"""

import numpy as np

from .engine import _is_torch_tensor, get_engine
from .utils import get_log_likelihood, stack_samples, to_inference_data, wrap_obs

__all__ = ["relative_eff", "relative_eff_from_matrix"]


def _chain_order(chain_id, n_draws):
    """``(n_chains, order)`` of a chain label per draw: ``order`` gathers the draws chain-major (chains by ascending label, the
    draws of a chain in their given order); None when they are chain-major already."""
    cid = np.asarray(chain_id.detach().cpu().numpy() if _is_torch_tensor(chain_id) else chain_id)
    if cid.ndim != 1 or cid.shape[0] != n_draws:
        raise ValueError(f"chain_id must be a vector of length n_draws = {n_draws}, got shape {tuple(cid.shape)}")
    if cid.dtype.kind not in "iu":
        raise TypeError(f"chain_id must be an integer vector, got dtype {cid.dtype}")
    _, counts = np.unique(cid, return_counts=True)
    if np.any(counts != counts[0]):
        raise ValueError(f"chains of unequal length: chain_id has {counts.tolist()} draws per chain")
    order = np.argsort(cid, kind="stable")
    return int(counts.size), (None if np.array_equal(order, np.arange(n_draws)) else order)


def _check(shape, n_chains, split):
    n_draws = int(shape[1])
    if int(n_chains) != n_chains or n_chains < 1:
        raise ValueError(f"n_chains must be a positive integer, got {n_chains}")
    n_chains = int(n_chains)
    if n_draws % n_chains != 0:
        raise ValueError(f"n_chains = {n_chains} does not divide n_draws = {n_draws}")
    n = n_draws // n_chains
    if split:
        n //= 2
    if n < 4:
        raise ValueError(f"a chain has {n} draws{' after the split' if split else ''}: at least 4 are needed")
    return n_chains


def relative_eff_from_matrix(ll, n_chains=4, chain_id=None, log=True, split=False, cap=True):
    """Relative efficiency ``ESS / n_draws`` of every row of an ``(n_obs, n_draws)`` matrix, float32 or float64: a torch CUDA
    tensor (read in place with the draws or the observations contiguous, so a ``.T`` view of an ``(n_draws, n_obs)`` buffer is not
    copied) or a NumPy array (uploaded in blocks).  Returns ``(n_obs,)`` float64 of the same kind.

    The draws are ``n_chains`` chains of equal length stacked chain-major (chain ``c`` is draws ``[c n, (c + 1) n)``, as ``loo()``
    stacks ``(chain, draw)``), or labelled by ``chain_id``, an integer vector of length ``n_draws`` (unequal chains: ``ValueError``;
    labels that are not chain-major: the draws are gathered first).  ``log=True``: the matrix holds log-likelihoods and
    ``exp(ll - row maximum)`` is analysed; ``log=False``: the values as given.  ``split=True`` replaces every chain by its first and
    last halves (a middle draw of an odd chain is dropped).  ``cap=True`` returns at most 1, as R-loo does.  A chain needs at least
    4 draws after the split.  Rows with a NaN or +inf entry and constant rows give NaN."""
    shape = tuple(ll.shape) if hasattr(ll, "shape") else ()
    if len(shape) != 2:
        raise ValueError("ll must be a 2-D (n_obs, n_draws) matrix")
    tensor = _is_torch_tensor(ll)
    if tensor:
        import torch

        if ll.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"ll must be float32 or float64, got {ll.dtype}")
    else:
        ll = np.asarray(ll)
        if ll.dtype not in (np.float32, np.float64):
            raise TypeError(f"ll must be float32 or float64, got {ll.dtype}")
    order = None
    if chain_id is not None:
        n_chains, order = _chain_order(chain_id, shape[1])
    n_chains = _check(shape, n_chains, split)
    if tensor and not ll.is_cuda:
        tensor, ll = False, ll.numpy()
    if order is not None:
        if tensor:
            import torch

            ll = ll.index_select(1, torch.as_tensor(order, device=ll.device))
        else:
            ll = np.take(ll, order, axis=1)
    eng = get_engine(ll.device.index if tensor else None)
    return eng.relative_eff(ll, n_chains, log=bool(log), split=bool(split), cap=bool(cap))["r_eff"]


def relative_eff(data, var_name=None, split=False, cap=True):
    """Relative efficiency of the likelihood ``exp(log_lik)`` of every observation (see :func:`relative_eff_from_matrix`).

    ``data``: InferenceData (with ArviZ), a dict of groups, or a ``(chain, draw, *obs)`` array, as ``loo()`` takes them; the
    chains are its first dimension.  Returns an array shaped like the observation dimensions."""
    log_likelihood = get_log_likelihood(to_inference_data(data), var_name=var_name)
    sizes = getattr(log_likelihood, "sizes", None)
    n_chains = int(sizes["chain"]) if sizes is not None and "chain" in sizes else int(np.shape(getattr(log_likelihood, "values", log_likelihood))[0])
    matrix, obs_shape, obs_dims, coords = stack_samples(log_likelihood)
    r = relative_eff_from_matrix(matrix, n_chains=n_chains, log=True, split=split, cap=cap)
    return wrap_obs(r, obs_shape, obs_dims, coords, "r_eff")
