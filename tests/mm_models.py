"""A model with analytic callbacks for the moment-matching tests (TEST INFRASTRUCTURE ONLY).

``y_i ~ N(mu, sigma)`` with the unconstrained parameters ``theta = (mu, log sigma, nuisance...)``; with D = 1 there is only ``mu`` and
sigma is fixed.  ``mu ~ N(0, 10)``, ``log sigma ~ N(0, 2)``, every nuisance dimension ``~ N(0, 1)``.  The draws come from a seeded
normal approximation of the posterior.  In the correlated variant the sampler's parameters are ``upars = theta @ inv(mix)`` for a
fixed matrix ``mix``: the model sees ``theta = upars @ mix``, so the draws are correlated and the covariance stage of moment matching
has something to match.

The five callbacks have the reference's signatures.  They take NumPy arrays or torch tensors (the result is of the same kind), a
single observation -- ``upars`` (S, D) with a scalar ``i`` -- or a batch -- ``upars`` (B, S, D) with ``i`` (B,), returning (B, S).
"""

import math

import numpy as np

OUTLIERS = (6.0, -5.0, 4.5, 3.5)
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


class NormalModel:
    def __init__(self, y, upars, mix=None, sigma=1.0):
        self.y = np.asarray(y, dtype=np.float64)
        self.upars = np.asarray(upars, dtype=np.float64)
        self.mix = None if mix is None or np.size(mix) == 0 else np.asarray(mix, dtype=np.float64)
        self.sigma = float(sigma)
        self.n, self.sum_y, self.sum_yy = len(self.y), float(self.y.sum()), float((self.y**2).sum())
        self.device = None  # set by to_device(): post_draws then hands out CUDA tensors
        self._dev = {}

    def to_device(self, device="cuda"):
        import torch

        self.device = torch.device(device)
        self._dev = {"y": torch.from_numpy(self.y).to(self.device), "upars": torch.from_numpy(self.upars).to(self.device),
                     "mix": None if self.mix is None else torch.from_numpy(self.mix).to(self.device)}
        return self

    def const(self, name, like):
        """``y`` / ``mix`` of the kind of ``like``."""
        if _is_tensor(like):
            if not self._dev or self._dev["y"].device != like.device:
                import torch

                self._dev = {"y": torch.from_numpy(self.y).to(like.device), "upars": None,
                             "mix": None if self.mix is None else torch.from_numpy(self.mix).to(like.device)}
            return self._dev[name]
        return getattr(self, name)


def make_model(S, D, seed, mixed=False, n_regular=12):
    """Seeded data (``n_regular`` N(0, 1) points and the four planted outliers) and draws from the normal approximation."""
    rng = np.random.default_rng(seed)
    y = np.concatenate([rng.normal(0.0, 1.0, n_regular), OUTLIERS])
    n = len(y)
    sd = y.std(ddof=1)
    theta = rng.normal(size=(S, D))
    if D == 1:
        theta[:, 0] = y.mean() + theta[:, 0] * sd / math.sqrt(n)
        return NormalModel(y, theta, None, sigma=sd)
    theta[:, 0] = y.mean() + theta[:, 0] * sd / math.sqrt(n)
    theta[:, 1] = math.log(sd) + theta[:, 1] / math.sqrt(2.0 * n)
    mix = None
    upars = theta
    if mixed:
        mix = np.eye(D) + 0.6 * rng.uniform(-1.0, 1.0, size=(D, D)) / math.sqrt(D)
        upars = theta @ np.linalg.inv(mix)
    return NormalModel(y, upars, mix)


def _theta(model, upars):
    mix = model.const("mix", upars)
    th = upars if mix is None else upars @ mix
    mu = th[..., 0]
    if th.shape[-1] == 1:
        return mu, None, None
    return mu, th[..., 1], th[..., 2:]


def _xp(a):
    if _is_tensor(a):
        import torch

        return torch
    return np


def post_draws(model, **kwargs):
    return model._dev["upars"] if model.device is not None else model.upars


def unconstrain_pars(model, pars, **kwargs):
    return pars


def log_prob_upars(model, upars, **kwargs):
    """Unnormalised log posterior density at ``upars`` (..., S, D) -> (..., S)."""
    xp = _xp(upars)
    mu, ls, rest = _theta(model, upars)
    if ls is None:
        s2 = model.sigma**2
        return -0.5 * (model.sum_yy - 2.0 * mu * model.sum_y + model.n * mu * mu) / s2 - 0.5 * (mu / 10.0) ** 2
    lp = -model.n * ls - 0.5 * (model.sum_yy - 2.0 * mu * model.sum_y + model.n * mu * mu) * xp.exp(-2.0 * ls)
    lp = lp - 0.5 * (mu / 10.0) ** 2 - 0.5 * (ls / 2.0) ** 2
    if rest.shape[-1]:
        lp = lp - 0.5 * (rest * rest).sum(-1)
    return lp


def log_lik_i_upars(model, upars, i, **kwargs):
    """Log-likelihood of observation ``i`` (a scalar, or (B,) for ``upars`` (B, S, D)) at ``upars``."""
    xp = _xp(upars)
    y = model.const("y", upars)
    yi = y[i]
    if getattr(yi, "ndim", 0) == 1:
        yi = yi[:, None]
    mu, ls, _ = _theta(model, upars)
    if ls is None:
        return -_HALF_LOG_2PI - math.log(model.sigma) - 0.5 * ((yi - mu) / model.sigma) ** 2
    return -_HALF_LOG_2PI - ls - 0.5 * (yi - mu) ** 2 * xp.exp(-2.0 * ls)


def log_lik_i(model, i, **kwargs):
    """Log-likelihood of observation ``i`` (or of the observations ``i`` (B,)) at the original draws."""
    up = post_draws(model)
    if getattr(i, "ndim", 0) == 1:
        up = up[None]
    return log_lik_i_upars(model, up, i)


CALLBACKS = dict(post_draws=post_draws, log_lik_i=log_lik_i, unconstrain_pars=unconstrain_pars, log_prob_upars_fn=log_prob_upars,
                 log_lik_i_upars_fn=log_lik_i_upars)
