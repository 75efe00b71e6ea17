"""The joint Laplace posterior with held-out entries and its per-row covariance (vlgp_joint_posterior), and the predictive
scores under a supplied covariance (vlgp_predictive_cov, vlgp_calibration_cov), stated in NumPy on top of
tests/joint_numpy.py, tests/predictive_numpy.py and tests/calibration_numpy.py.  Written from the definitions, dense and
independent of the package.

  masked unit   a held-out entry (t, n) is dropped: its term of ll and of sum |terms| is 0, res = cur = 0, so it is absent
                from grad f, H and laplace; what y holds there is replaced before anything reads it.
  cov           cov[t, l, l'] = G_l[t, :] (H^-1)_{l l'} G_l'[t, :]' from the dense inverse of H at the mode.
  s2            max(0, a_n' cov[t] a_n); NaN where that, or m, is not finite.
  scores        vlgp_predictive's and vlgp_calibration's entry with this m, s2 and rate = exp(min(m + s2 / 2, 10)); an
                entry without finite moments has NaN lpd and rate (predictive) or is skipped (calibration).
"""
import numpy as np
from scipy.linalg import cho_solve
from scipy.special import erfc, gammaln

import calibration_numpy as CN
import joint_numpy as JN
import predictive_numpy as PN


class MaskedUnit(JN.Unit):
    """joint_numpy.Unit without the entries of ``held`` (bool (T, N); None: nothing held out)."""

    def __init__(self, u, a, b, noise, gauss, G_in, held=None):
        super().__init__(u, a, b, noise, gauss, G_in)
        self.held = np.zeros(self.y.shape, bool) if held is None else np.asarray(held, bool)
        self.y = np.where(self.held, 0.0, self.y)  # (never enters a sum: the two methods below drop the entry)

    def terms(self, x):
        lp, eta = super().terms(x)
        return np.where(self.held, 0.0, lp), eta

    def res_cur(self, beta):
        res, cur = super().res_cur(beta)
        return np.where(self.held, 0.0, res), np.where(self.held, 0.0, cur)


def cov_rows(U, H):
    """cov (T, L, L) from the dense inverse of H (D, D)."""
    Hinv = cho_solve((np.linalg.cholesky(H), True), np.eye(U.D))
    cov = np.empty((U.y.shape[0], U.L, U.L))
    for l in range(U.L):
        for m in range(U.L):
            block = Hinv[U.start[l]:U.start[l + 1], U.start[m]:U.start[m + 1]]
            cov[:, l, m] = np.einsum("ti,ij,tj->t", U.G[l], block, U.G[m])
    return cov


def statement(units, a, b, noise, gauss, prior, held=None, tol=1e-20, beta=None):
    """What vlgp_joint_posterior reports for a list of unit dicts: joint_numpy.statement's per-unit dicts (no draws) plus
    ``cov`` (T, L, L).  ``held``: None for a plain set, started at the mean-field centres, or bool (rows, N) over the
    concatenated rows for a masked set, started at beta = 0.  ``beta``: stacked vectors to evaluate at instead."""
    out, row = [], 0
    for i, u in enumerate(units):
        T = u["y"].shape[0]
        U = MaskedUnit(u, a, b, noise, gauss, prior[T], None if held is None else held[row:row + T])
        row += T
        if beta is not None:
            bt, dec, n, conv = np.asarray(beta[i], float), np.nan, 0, True
        else:
            start = JN.mean_field_start(U, u) if held is None else np.zeros(U.D)
            bt, dec, n, conv = JN.newton(U, start, tol)
        res = JN.summary(U, bt)
        res.update(beta=bt, ranks=U.ranks, decrement=dec, n_newton=n, converged=conv, unit=U, cov=cov_rows(U, res["H"]))
        out.append(res)
    return out


# ---- scores under a supplied mean and covariance ----------------------------------------------------------------------
def moments(x, mu, cov, a, b):
    """``(m, s2, ok)``, (T, N) each, for mu (T, L) and cov (T, L, L); ok: both finite (s2 and m are NaN where not)."""
    with np.errstate(invalid="ignore"):
        m = mu @ a + (np.einsum("tpn,pn->tn", x, b) if x is not None else b[0])
        q = np.einsum("ln,tlm,mn->tn", a, cov, a)
    ok = np.isfinite(m) & np.isfinite(q)
    return np.where(ok, m, np.nan), np.where(ok, np.maximum(q, 0.0), np.nan), ok


def lpd_rate(y, x, mu, cov, a, b, noise, gauss, n_nodes):
    """predictive_numpy.lpd_rate with s2 from cov: ``(lpd, rate)``, NaN where the moments are not finite."""
    m, s2, ok = moments(x, mu, cov, a, b)
    m0, s0 = np.where(ok, m, 0.0), np.where(ok, s2, 0.0)
    lam = np.exp(np.minimum(m0 + 0.5 * s0, 10.0))
    nz = noise + s0
    lg = -0.5 * np.log(2 * np.pi * nz) - (y - m0) ** 2 / (2 * nz)
    plug = y * np.log(lam) - lam - gammaln(y + 1.0)
    quad = s0 >= 1e-30
    with np.errstate(all="ignore"):
        lp = np.where(quad, PN.poisson_lognormal(y, m0, np.where(quad, s0, 1.0), n_nodes), plug)
    return np.where(ok, np.where(gauss, lg, lp), np.nan), np.where(ok, np.where(gauss, m0, lam), np.nan)


def cal_entries(y, x, mu, cov, a, b, noise, gauss, n_nodes, max_count=4096):
    """calibration_numpy.entries with s2 from cov: ``(lo, hi, pearson, skip)``; skipped where the moments are not finite."""
    m, s2, ok = moments(x, mu, cov, a, b)
    m0, s0 = np.where(ok, m, 0.0), np.where(ok, s2, 0.0)
    lam = np.exp(np.minimum(m0 + 0.5 * s0, 10.0))
    mean, var = np.where(gauss, m0, lam), np.where(gauss, noise + s0, lam + lam * lam * np.expm1(s0))
    g = np.broadcast_to(gauss, y.shape)
    u = 0.5 * erfc(-(y - m0) / np.sqrt(2.0 * var))
    lo, hi, skip = np.where(g, u, 0.0), np.where(g, u, 0.0), np.zeros(y.shape, dtype=bool)
    p = ~g
    lo[p], hi[p], skip[p] = CN.count_cdf(y[p], m0[p], s0[p], mean[p], n_nodes, max_count)
    skip = skip | ~ok
    with np.errstate(invalid="ignore"):
        return np.where(skip, np.nan, lo), np.where(skip, np.nan, hi), (y - mean) ** 2 / var, skip


def _per_replica(units, mu, cov, fn):
    """fn(unit, mu rows, cov rows) -> tuple of (T, N) arrays, concatenated over the units, for every replica: a list over
    the replicas of such tuples over the concatenated rows.  mu (n_rep, rows, L), cov (n_rep, rows, L, L)."""
    bounds = np.cumsum([0] + [u["y"].shape[0] for u in units])
    out = []
    for k in range(mu.shape[0]):
        got = [fn(u, mu[k, r0:r1], cov[k, r0:r1]) for u, r0, r1 in zip(units, bounds[:-1], bounds[1:])]
        out.append(tuple(np.concatenate([g[j] for g in got]) for j in range(len(got[0]))))
    return out


def score_predictive(units, mu, cov, a, b, noise, gauss, n_nodes, groups=None, held=None):
    """``(lpd, rate, sums)`` of vlgp_predictive_cov in the layout of the set: plain (mu, cov with one replica; (rows, N)
    twice and (N, 4)), group replicas (``groups``: a column and a slot per (replica, channel) pair) or masked (``held``
    bool (n_rep, rows, N): NaN where no replica holds the entry out, sums (n_rep, N, 4))."""
    y = np.concatenate([u["y"] for u in units])
    reps = _per_replica(units, mu, cov, lambda u, m, c: lpd_rate(u["y"], u["x"], m, c, a, b, noise, gauss, n_nodes))
    if groups is not None:
        cols_l, cols_r, sums = [], [], []
        for k, g in enumerate(groups):
            s = PN.sums4(y, reps[k][0], reps[k][1], gauss)
            for n in g:
                cols_l.append(reps[k][0][:, n])
                cols_r.append(reps[k][1][:, n])
                sums.append(s[n])
        return np.stack(cols_l, axis=1), np.stack(cols_r, axis=1), np.stack(sums)
    if held is not None:
        lpd_all, rate_all = np.full(y.shape, np.nan), np.full(y.shape, np.nan)
        sums = np.zeros((held.shape[0], y.shape[1], 4))
        for k in range(held.shape[0]):
            sums[k] = PN.sums4(y, reps[k][0], reps[k][1], gauss, held[k])
            lpd_all[held[k]], rate_all[held[k]] = reps[k][0][held[k]], reps[k][1][held[k]]
        return lpd_all, rate_all, sums
    return reps[0][0], reps[0][1], PN.sums4(y, reps[0][0], reps[0][1], gauss)


def score_calibration(units, mu, cov, a, b, noise, gauss, n_nodes, n_bins, levels, max_count=4096, groups=None, held=None):
    """``(cdf, sums, terms)`` of vlgp_calibration_cov in the layout of the set, as calibration_numpy's score_plain,
    score_groups and score_masked return them."""
    reps = _per_replica(units, mu, cov,
                        lambda u, m, c: cal_entries(u["y"], u["x"], m, c, a, b, noise, gauss, n_nodes, max_count))
    cols = [CN.columns(lo, hi, pearson, skip, n_bins, levels) for lo, hi, pearson, skip in reps]
    if groups is not None:
        cdf, terms = [], []
        for k, g in enumerate(groups):
            for n in g:
                cdf.append(np.stack([reps[k][0][:, n], reps[k][1][:, n]], axis=-1))
                terms.append(cols[k][:, n])
        terms = np.stack(terms, axis=1)
        return np.stack(cdf, axis=1), terms.sum(axis=0), terms
    if held is not None:
        cdf = np.full(held.shape[1:] + (2,), np.nan)
        terms = []
        for k in range(held.shape[0]):
            terms.append(np.where(held[k][..., None], cols[k], 0.0))
            cdf[held[k]] = np.stack([reps[k][0], reps[k][1]], axis=-1)[held[k]]
        terms = np.stack(terms)
        return cdf, terms.sum(axis=1), terms
    return np.stack([reps[0][0], reps[0][1]], axis=-1), cols[0].sum(axis=0), cols[0]
