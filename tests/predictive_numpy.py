"""The posterior-predictive density of vlgp_amd/evaluation.py (vlgp_predictive) stated in NumPy, vectorised over entries,
and the scoring of plain, group-replica and masked layouts with it (tests/test_predictive_host.py,
tests/test_gpu_predictive.py).  The steps are the definition's, in its order; the log-sum-exp takes the largest term
out first and adds the nodes in order."""
import numpy as np
from scipy.special import gammaln

from oracle import vlgp_oracle as O

NEWTON_STEPS = 8


def hermite_nodes(n):
    x, w = np.polynomial.hermite.hermgauss(n)
    return np.sqrt(2.0) * x, np.log(w / np.sqrt(np.pi)) + x * x


def ex(e):
    return np.exp(np.minimum(e, 10.0))


def mode(y, m, s2):
    """The centre of the rule: the definition's start and its eight Newton steps."""
    with np.errstate(divide="ignore"):
        e = np.where(y > ex(m), np.minimum(np.log(np.where(y > 0, y, 1.0)), m + y * s2), m)
    for _ in range(NEWTON_STEPS):
        x = ex(e)
        e = e - (y - x - (e - m) / s2) / (-x - 1.0 / s2)
    return e


def poisson_lognormal(y, m, s2, n_nodes):
    """log int Poisson(y | ex(eta)) N(eta; m, s2) d eta by the mode-centred rule; s2 > 0.  Broadcasts."""
    y, m, s2 = np.broadcast_arrays(*(np.asarray(t, dtype=float) for t in (y, m, s2)))
    z, lwa = hermite_nodes(n_nodes)
    e = mode(y, m, s2)
    h = s2 * ex(e) + 1.0
    tau = np.sqrt(s2) / np.sqrt(h)
    eta = e[..., None] + tau[..., None] * z
    c = np.minimum(eta, 10.0)
    t = lwa + y[..., None] * c - np.exp(c) - (eta - m[..., None]) ** 2 / (2.0 * s2[..., None])
    top = t.max(axis=-1)
    acc = np.zeros_like(top)
    for q in range(n_nodes):
        acc = acc + np.exp(t[..., q] - top)
    return -0.5 * np.log(h) + (top + np.log(acc)) - gammaln(y + 1.0)


def lpd_rate(y, x, mu, v, a, b, noise, gauss, vb, n_nodes):
    """``(lpd, rate)``, (T, N) each, of a unit's entries under the posterior mu, v (T, L)."""
    m = O.linear_predictor(x, mu, a, b)
    s2 = (v @ a ** 2) if vb else np.zeros_like(m)
    lam = np.exp(np.minimum(m + 0.5 * s2, 10.0))
    nz = noise + s2
    lg = -0.5 * np.log(2 * np.pi * nz) - (y - m) ** 2 / (2 * nz)
    plug = y * np.log(lam) - lam - gammaln(y + 1.0)
    quad = s2 >= 1e-30
    with np.errstate(all="ignore"):  # (the entries the quadrature does not serve are computed and dropped)
        lp = np.where(quad, poisson_lognormal(y, m, np.where(quad, s2, 1.0), n_nodes), plug)
    return np.where(gauss, lg, lp), np.where(gauss, m, lam)


def sums4(y, lpd, rate, gauss, keep=None):
    """(N, 4) in vlgp_loglik's slots with ``sum lpd`` first, over the entries of ``keep`` (default all)."""
    keep = np.ones(y.shape, dtype=bool) if keep is None else keep
    last = np.where(gauss, y * y, gammaln(y + 1.0))
    return np.stack([np.where(keep, t, 0.0).sum(axis=0) for t in (lpd, y, rate, last)], axis=1)


def score_plain(units, a, b, noise, gauss, vb, n_nodes):
    """``(lpd, rate, sums)`` of a plain set: the units' rows concatenated."""
    got = [lpd_rate(u["y"], u["x"], u["mu"], u["v"], a, b, noise, gauss, vb, n_nodes) for u in units]
    lpd, rate = (np.concatenate([g[k] for g in got]) for k in (0, 1))
    return lpd, rate, sums4(np.concatenate([u["y"] for u in units]), lpd, rate, gauss)


def score_groups(units, groups, mu, v, a, b, noise, gauss, vb, n_nodes):
    """Group replicas: mu, v (n_rep, rows, L) of the replicas; one column and one slot per (replica, channel) pair in
    the order of the concatenated groups.  ``(lpd, rate, sums)``: (rows, n_pairs) twice and (n_pairs, 4)."""
    y = np.concatenate([u["y"] for u in units])
    bounds = np.cumsum([0] + [u["y"].shape[0] for u in units])
    cols_l, cols_r, sums = [], [], []
    for k, g in enumerate(groups):
        got = [lpd_rate(u["y"], u["x"], mu[k, r0:r1], v[k, r0:r1], a, b, noise, gauss, vb, n_nodes)
               for u, r0, r1 in zip(units, bounds[:-1], bounds[1:])]
        lpd, rate = (np.concatenate([t[j] for t in got]) for j in (0, 1))
        s = sums4(y, lpd, rate, gauss)
        for n in g:
            cols_l.append(lpd[:, n])
            cols_r.append(rate[:, n])
            sums.append(s[n])
    return np.stack(cols_l, axis=1), np.stack(cols_r, axis=1), np.stack(sums)


def score_masked(units, held, mu, v, a, b, noise, gauss, vb, n_nodes):
    """Masked replicas: held bool (n_rep, rows, N), mu, v (n_rep, rows, L).  ``(lpd, rate, sums)``: (rows, N) twice, NaN
    where no replica holds the entry out, and (n_rep, N, 4) over each replica's held-out entries."""
    y = np.concatenate([u["y"] for u in units])
    bounds = np.cumsum([0] + [u["y"].shape[0] for u in units])
    lpd_all, rate_all = np.full(y.shape, np.nan), np.full(y.shape, np.nan)
    sums = np.zeros((held.shape[0], y.shape[1], 4))
    for k in range(held.shape[0]):
        got = [lpd_rate(u["y"], u["x"], mu[k, r0:r1], v[k, r0:r1], a, b, noise, gauss, vb, n_nodes)
               for u, r0, r1 in zip(units, bounds[:-1], bounds[1:])]
        lpd, rate = (np.concatenate([t[j] for t in got]) for j in (0, 1))
        sums[k] = sums4(y, lpd, rate, gauss, held[k])
        lpd_all[held[k]], rate_all[held[k]] = lpd[held[k]], rate[held[k]]
    return lpd_all, rate_all, sums


def brute_force(y, m, sigma, points=2_000_001):
    """log int Poisson(y | ex(eta)) N(eta; m, sigma^2) d eta by a trapezoid of ``points`` points over the union of
    m +- 12 sigma and mode +- 40 tau; scalars."""
    s2 = sigma * sigma
    e = float(mode(np.float64(y), np.float64(m), np.float64(s2)))
    tau = sigma / np.sqrt(s2 * float(ex(e)) + 1.0)
    lo, hi = min(m - 12 * sigma, e - 40 * tau), max(m + 12 * sigma, e + 40 * tau)
    eta = np.linspace(lo, hi, points)
    c = np.minimum(eta, 10.0)
    f = y * c - np.exp(c) - (eta - m) ** 2 / (2 * s2)
    top = f.max()
    g = np.exp(f - top)
    area = (g.sum() - 0.5 * (g[0] + g[-1])) * (eta[1] - eta[0])
    return top + np.log(area) - 0.5 * np.log(2 * np.pi * s2) - gammaln(y + 1.0)
