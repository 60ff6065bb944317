"""NumPy restatement of the cluster-marginal GLM likelihood (include/pyloo_amd.h, ``pla_glm_marginal``): the quadrature of
csrc/pla_glm_marginal.h in the kernel's order of operations, segments included, on a linear predictor ``rest`` handed in; the closed
form of the Gaussian family; generators of clustered test models; and a stand-in engine whose marginal call is this restatement.
TEST INFRASTRUCTURE ONLY."""

import numpy as np

import glm_ref
import glmm_ref

L = 128  # pla_glm_marginal_segment(): tests that have the library assert the two agree
LOG_SQRT_2PI = 0.91893853320467274178


def quadrature(rest, offsets, members, family, y, tau, nodes, logw, z=None, trials=None, oc=None, sigma=None, dc=None, seg=L,
               with_bound=False):
    """``mll`` (C, S) from ``rest`` (N', S), row j the linear predictor of observation ``members[j]``; ``family`` is the engine's.
    Per cluster and node: the segment sums from zero in member order, added in order of k starting from segment 0; then
    ``(logw + prior) + sum`` and the log-sum-exp over the nodes in order of q.  ``with_bound``: also the (C, S) magnitude
    ``max_q (sum_i |ll_iq| + |prior_q| + |logw_q|)`` of the parity bound."""
    rest = np.asarray(rest, dtype=np.float64)
    offsets, members = np.asarray(offsets), np.asarray(members)
    tau = np.asarray(tau, dtype=np.float64)
    nodes, logw = np.asarray(nodes, dtype=np.float64), np.asarray(logw, dtype=np.float64)
    n_clusters, n_nodes, n_draws = len(offsets) - 1, nodes.shape[1], rest.shape[1]
    out = np.empty((n_clusters, n_draws))
    mag = np.zeros((n_clusters, n_draws))
    pick = lambda v, rows: None if v is None else np.asarray(v, dtype=np.float64)[rows]  # noqa: E731
    with np.errstate(all="ignore"):
        lt = -LOG_SQRT_2PI - np.log(tau)
        for c in range(n_clusters):
            lo, hi = int(offsets[c]), int(offsets[c + 1])
            if not 0 <= lo <= hi <= len(members):
                lo = hi = 0  # (a device pair out of range or decreasing: an empty cluster)
            e = np.empty((n_nodes, n_draws))
            for q in range(n_nodes):
                total, absum = None, np.zeros(n_draws)
                for k0 in range(lo, hi, seg):
                    k1 = min(k0 + seg, hi)
                    src = np.clip(members[k0:k1], 0, len(np.asarray(y)) - 1)
                    if z is None:
                        eta = rest[k0:k1] + nodes[c, q]
                    else:
                        eta = rest[k0:k1] + (np.asarray(z, dtype=np.float64)[src] * nodes[c, q])[:, None]
                    ll = glm_ref.density(family, eta, np.asarray(y)[src], sigma=sigma, trials=pick(trials, src), oc=pick(oc, src), dc=dc)
                    part = np.zeros(n_draws)
                    for row in ll:  # (in member order, from zero)
                        part = part + row
                    absum += np.abs(ll).sum(0)
                    total = part if total is None else total + part
                if total is None:
                    total = np.zeros(n_draws)
                t = nodes[c, q] / tau
                prior = lt - 0.5 * (t * t)
                e[q] = (logw[c, q] + prior) + total
                mag[c] = np.maximum(mag[c], absum + np.abs(prior) + np.abs(logw[c, q]))
            m = e.max(0)
            acc = np.zeros(n_draws)
            for q in range(n_nodes):
                acc = acc + np.exp(e[q] - m)
            out[c] = np.where(m == -np.inf, -np.inf, m + np.log(acc))
    return (out, mag) if with_bound else out


def gauss_hermite(loc, scale, n_nodes):
    """The adaptive rule of the fronts: ``node = loc + sqrt(2) scale x_q``, ``logw = log w_q + x_q^2 + log(sqrt(2) scale)``."""
    x, w = np.polynomial.hermite.hermgauss(n_nodes)
    loc, scale = np.asarray(loc, dtype=np.float64)[:, None], np.asarray(scale, dtype=np.float64)[:, None]
    return loc + np.sqrt(2.0) * scale * x[None, :], (np.log(w) + x * x)[None, :] + np.log(np.sqrt(2.0) * scale)


def gaussian_closed_form(rest, offsets, members, y, sigma, tau, z=None):
    """``mll`` (C, S) of the Gaussian family in closed form: ``y_c - rest_c ~ N(0, sigma_s^2 I + tau_s^2 z z')``."""
    rest, y = np.asarray(rest, dtype=np.float64), np.asarray(y, dtype=np.float64)
    sigma, tau = np.asarray(sigma, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    out = np.empty((len(offsets) - 1, rest.shape[1]))
    for c in range(len(offsets) - 1):
        rows = np.arange(offsets[c], offsets[c + 1])
        src = np.asarray(members)[rows]
        zc = np.ones(len(rows)) if z is None else np.asarray(z, dtype=np.float64)[src]
        r = y[src][:, None] - rest[rows]  # (n, S)
        n, zz, zr, rr = len(rows), zc @ zc, zc @ r, (r * r).sum(0)
        s2, t2 = sigma * sigma, tau * tau
        logdet = n * np.log(s2) + np.log1p(t2 * zz / s2)
        quad = (rr - t2 * zr * zr / (s2 + t2 * zz)) / s2
        out[c] = -0.5 * n * np.log(2.0 * np.pi) - 0.5 * logdet - 0.5 * quad
    return out


def gaussian_model(rng, n_clusters, rows, n_draws, slope):
    """The model of DESIGN.md section 18: ``n_clusters`` clusters of ``rows`` rows, an intercept and a covariate, a cluster effect on
    the intercept or (``slope``) on the covariate ``z``; ``tau`` and ``sigma`` jittered log-normally over the draws, ``u`` drawn from
    its conditional posterior per draw.  Returns a dict with ``rest`` (N, S) = ``X beta``."""
    n = n_clusters * rows
    cluster = np.repeat(np.arange(n_clusters), rows)
    X = np.column_stack([np.ones(n), rng.normal(size=n)])
    z = rng.normal(size=n) if slope else None
    zc = np.ones(n) if z is None else z
    u0 = 0.7 * rng.normal(size=n_clusters)
    y = X @ np.array([0.3, -0.5]) + zc * u0[cluster] + 0.8 * rng.normal(size=n)
    beta = np.array([0.3, -0.5]) + 0.1 * rng.normal(size=(n_draws, 2))
    sigma = 0.8 * np.exp(0.1 * rng.normal(size=n_draws))
    tau = 0.7 * np.exp(0.15 * rng.normal(size=n_draws))
    rest = X @ beta.T
    u = np.empty((n_draws, n_clusters))
    for c in range(n_clusters):
        rows_c = cluster == c
        prec = (zc[rows_c] @ zc[rows_c]) / sigma**2 + 1.0 / tau**2
        mean = (zc[rows_c] @ (y[rows_c][:, None] - rest[rows_c])) / sigma**2 / prec
        u[:, c] = mean + rng.normal(size=n_draws) / np.sqrt(prec)
    return dict(X=X, y=y, beta=beta, sigma=sigma, tau=tau, z=z, u=u, cluster=cluster, rest=rest)


def make_clustered(rng, sizes, n_draws, p, family, slope, n_terms=0, eta_scale=1.0):
    """A clustered model for the kernels' edges: cluster c has ``sizes[c]`` rows, scattered over the observations (the labels are
    shuffled, the last cluster is held by the last row only when its size is 1); glmm_ref.make_model's data with ``n_terms``
    conditional terms, ``tau`` per draw and the covariate ``z`` of the integrated effect where ``slope`` says so."""
    n = int(np.sum(sizes))
    model = glmm_ref.make_model(rng, n, n_draws, p, family, sizes=(4, 3)[:n_terms], slopes=(False, True)[:n_terms])
    if eta_scale != 1.0:
        model["beta"] = model["beta"] * eta_scale
    labels = np.repeat(np.arange(len(sizes)), sizes)
    head = rng.permutation(labels[:-1]) if sizes[-1] == 1 else rng.permutation(labels)
    model["cluster"] = np.concatenate([head, labels[-1:]]) if sizes[-1] == 1 else head
    model["tau"] = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), size=n_draws))
    model["z"] = rng.normal(size=n) if slope else None
    if n_terms == 0:
        model["terms"] = None
    return model


class MarginalEngine(glmm_ref.GroupedEngine):
    """The stand-in of glmm_ref with ``Engine.glm_marginal``: the restatement on what it is handed; records calls."""

    def glm_marginal(self, X, beta, family, index, tau, nodes, log_weights, z=None, y=None, offset=None, trials=None, obs_const=None,
                     draw_scale=None, draw_const=None, mode="matrix", tail_count=0, method="psis", scale_value=1.0, good_k=0.7,
                     pointwise=True, aggregate=True, **extra):
        assert set(extra) <= {"groups"}, extra
        self.calls.append(dict(op="glm_marginal", family=family, mode=mode, tail_count=tail_count, method=method, y=y, offset=offset,
                               trials=trials, obs_const=obs_const, draw_scale=draw_scale, draw_const=draw_const, index=index,
                               tau=tau, nodes=nodes, log_weights=log_weights, z=z, groups=extra.get("groups"), good_k=good_k,
                               scale_value=scale_value, n_draws=np.asarray(beta).shape[0]))
        members = np.asarray(index.members)
        X = np.asarray(X)
        rest = glmm_ref.add_terms(glm_ref.linpred(X[members], beta, None if offset is None else np.asarray(offset)[members]),
                                  extra.get("groups"), rows=members)
        mll = quadrature(rest, index.offsets, members, family, y, tau, nodes, log_weights, z=z, trials=trials, oc=obs_const,
                         sigma=draw_scale, dc=draw_const)
        if mode == "matrix":
            return mll
        bad = np.isnan(mll)
        res = self.psis_loo(np.where(bad, -1e10, mll), tail_count, method, scale_value, good_k)
        res["n_replaced"] = int(bad.sum())
        return res

    def psis_loo_groups(self, ll, index, tail_count=0, method="psis", scale_value=1.0, good_k=0.7, pointwise=True, aggregate=True):
        """``Engine.psis_loo_groups`` for the comparison with ``loo_group_from_matrix``: group sums in member order, then the pass."""
        ll = np.asarray(ll, dtype=np.float64)
        bad = np.isnan(ll)
        ll = np.where(bad, -1e10, ll)
        off, mem = np.asarray(index.offsets), np.asarray(index.members)
        sums = np.stack([ll[mem[off[g]:off[g + 1]]].sum(0) for g in range(index.n_groups)])
        res = self.psis_loo(sums, tail_count, method, scale_value, good_k)
        return {"diag": res["diag"], "logo_i": res["loo_i"], "lppd_i": res["lppd_i"], "agg": res["agg"], "n_replaced": int(bad.sum())}
