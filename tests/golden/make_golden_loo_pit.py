#!/usr/bin/env python3
"""Golden vectors for the LOO-PIT values from the REAL reference.

Run only in the build container:  ``python tests/golden/make_golden_loo_pit.py``  -> loo_pit.npz

The reference has no ``loo_pit`` of its own; what ArviZ computes there is, per observation,
``exp(logsumexp(where(y_hat <= y, lw, -inf)))`` with ``lw`` the normalised smoothed log weights.  Here ``lw`` and the Pareto k
come from the reference's own ``psislw(-ll, reff)`` (NaN log-likelihoods replaced by -1e10 first, loo.py:218-227) and the sum from
its own ``utils._logsumexp``, both loaded in place with the loader of make_golden.py.  Only inputs and the numbers those
functions return are written.  The f32 case stores f32 inputs and the reference's numbers on their f64 upcast.

The log-likelihood rows are ``-k Exp(1) + c`` from a continuous generator: no row has tied values in its tail (checked below),
because tied tail draws get their smoothed quantiles in the order of NumPy's unstable argsort, and for the PIT that order matters."""

import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


def ll_rows(rng, n, s, dtype=np.float64):
    k = rng.uniform(0.1, 0.8, size=(n, 1))
    c = -1.0 - rng.uniform(0.0, 2.0, size=(n, 1))
    return (-k * rng.exponential(size=(n, s)) + c).astype(dtype)


def normal_case(rng, n, s, dtype=np.float64):
    ll = ll_rows(rng, n, s, dtype)
    mu, sd = rng.normal(size=(n, 1)), rng.uniform(0.5, 2.0, size=(n, 1))
    yh = (mu + sd * rng.normal(size=(n, s))).astype(dtype)
    y = (mu + sd * rng.normal(size=(n, 1))).reshape(n)
    return ll, yh, y


def reference_pit(mods, ll, yh, y, reff):
    ll = ll.astype(np.float64)  # f32 input: the parity target is the reference on the f64-upcast data, as in make_golden.py
    clean = np.where(np.isnan(ll), -1e10, ll)  # loo.py:218-227
    lw, k = mods["psis"].psislw(-clean, reff)
    lse = mods["utils"]._logsumexp
    with np.errstate(all="ignore"):
        le = np.exp(lse(np.where(yh <= y[:, None], lw, -np.inf), axis=-1))
        lt = np.exp(lse(np.where(yh < y[:, None], lw, -np.inf), axis=-1))
    return np.asarray(lw), np.asarray(k, dtype=np.float64), np.asarray(le, dtype=np.float64), np.asarray(lt, dtype=np.float64)


def main():
    warnings.simplefilter("ignore")
    mods = mg.load_reference()
    rng = np.random.default_rng(20261019)
    cases = {}
    cases["s100_r1"] = normal_case(rng, 8, 100) + (1.0,)
    cases["s1000_r0p7"] = normal_case(rng, 4, 1000) + (0.7,)
    cases["s4000_r1"] = normal_case(rng, 2, 4000) + (1.0,)
    cases["s1000_r1_f32"] = normal_case(rng, 4, 1000, np.float32) + (1.0,)
    # count data: Poisson draws, integer observations -- ties between draws and observation in every row
    n, s = 4, 500
    ll = ll_rows(rng, n, s)
    lam = np.array([0.5, 3.0, 8.0, 40.0]).reshape(n, 1)
    yh = rng.poisson(lam, size=(n, s)).astype(np.float64)
    y = np.array([0.0, 3.0, 7.0, 41.0])
    cases["poisson_s500_r1"] = (ll, yh, y, 1.0)
    # edge rows, S = 500
    n, s = 8, 500
    ll, yh, y = normal_case(rng, n, s)
    y[0] = yh[0].min() - 1.0          # below every draw
    y[1] = yh[1].max() + 1.0          # above every draw
    ll[2] = -1.25                     # constant log-likelihood: k = inf, uniform weights
    ll[3, 17] = np.nan                # a NaN log-likelihood: counts as -1e10
    yh[4, 5] = np.nan                 # a NaN draw is never counted
    yh[4, 300] = np.nan
    yh[5, 7] = np.inf                 # infinite draws compare as they are
    yh[5, 8] = -np.inf
    y[6] = np.nan                     # a NaN observation: nothing is counted
    cases["edges_s500_r1"] = (ll, yh, y, 1.0)

    out = {"names": np.array(sorted(cases))}
    for name, (ll, yh, y, reff) in cases.items():
        m = int(np.ceil(min(ll.shape[1] / 5.0, 3 * (ll.shape[1] / reff) ** 0.5)))  # base.py:139-141
        for r in np.where(np.isnan(ll), ll.dtype.type(-1e10), ll):
            tail = np.sort(-r)[-(m + 1):]  # the smoothed draws and the cutoff
            assert np.unique(tail).size in (tail.size, 1), name  # no ties among them (a constant row apart)
        lw, k, le, lt = reference_pit(mods, ll, yh, y, reff)
        assert lw.dtype == np.float64
        out[name + "_ll"], out[name + "_yh"], out[name + "_y"], out[name + "_reff"] = ll, yh, y, np.array(reff)
        out[name + "_lw"], out[name + "_k"], out[name + "_pit_le"], out[name + "_pit_lt"] = lw, k, le, lt
        print(name, ll.shape, ll.dtype, "k", np.round(k, 3), "le", np.round(le, 4), "lt", np.round(lt, 4))
    path = os.path.join(HERE, "loo_pit.npz")
    np.savez_compressed(path, **out)
    print("wrote loo_pit.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
