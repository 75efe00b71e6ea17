"""The calibration sums of vlgp_amd/evaluation.py (vlgp_calibration) stated in NumPy/SciPy with the node tables and the
masses of tests/predictive_numpy.py, and the scoring of plain, group-replica and masked layouts with them
(tests/test_calibration_host.py, tests/test_gpu_calibration.py).  The steps are the definition's, in its order: the
masses of an entry are added in the order of the counts 0, 1, ..."""
import numpy as np
from scipy.special import erfc, gammaln, pdtr

import predictive_numpy as PN
from oracle import vlgp_oracle as O


def mass(j, m, s2, lam, n_nodes):
    """p(j): exp of vlgp_predictive's lpd at y = j -- the mode-centred rule, or the plug-in mass when s2 < 1e-30."""
    j = np.full(np.shape(m), float(j))
    quad = s2 >= 1e-30
    plug = j * np.log(lam) - lam - gammaln(j + 1.0)
    with np.errstate(all="ignore"):  # (the entries the quadrature does not serve are computed and dropped)
        lp = np.where(quad, PN.poisson_lognormal(j, m, np.where(quad, s2, 1.0), n_nodes), plug)
    return np.exp(lp)


def valid_count(y, max_count):
    with np.errstate(invalid="ignore"):
        return np.isfinite(y) & (y >= 0) & (y <= max_count) & (y == np.floor(y))


def count_cdf(y, m, s2, lam, n_nodes, max_count=4096):
    """``(lo, hi, skip)`` of Poisson entries (any shape): lo = F(y - 1), hi = F(y), both clipped to <= 1; NaN and skip
    for y negative, no integer, not finite or > max_count."""
    y, m, s2, lam = (np.asarray(t, dtype=float).ravel() for t in np.broadcast_arrays(y, m, s2, lam))
    ok = valid_count(y, max_count)
    k = np.where(ok, y, -1.0)
    lo, pk = np.zeros(y.shape), np.zeros(y.shape)
    for j in range(int(k.max(initial=-1.0)) + 1):
        idx = np.flatnonzero(k >= j)
        p = mass(j, m[idx], s2[idx], lam[idx], n_nodes)
        below = k[idx] > j
        lo[idx[below]] += p[below]
        pk[idx[~below]] = p[~below]
    hi = np.minimum(lo + pk, 1.0)
    lo = np.minimum(lo, 1.0)
    return np.where(ok, lo, np.nan), np.where(ok, hi, np.nan), ~ok


def moments(y, x, mu, v, a, b, noise, gauss, vb):
    """``(m, s2, mean, var)``, (T, N) each: vlgp_predictive's m, s2 and rate, and the predictive variance."""
    m = O.linear_predictor(x, mu, a, b)
    s2 = (v @ a ** 2) if vb else np.zeros_like(m)
    lam = np.exp(np.minimum(m + 0.5 * s2, 10.0))
    return m, s2, np.where(gauss, m, lam), np.where(gauss, noise + s2, lam + lam * lam * np.expm1(s2))


def entries(y, x, mu, v, a, b, noise, gauss, vb, n_nodes, max_count=4096):
    """``(lo, hi, pearson, skip)``, (T, N) each, of a unit's entries under the posterior mu, v (T, L)."""
    m, s2, mean, var = moments(y, x, mu, v, a, b, noise, gauss, vb)
    g = np.broadcast_to(gauss, y.shape)
    u = 0.5 * erfc(-(y - m) / np.sqrt(2.0 * var))
    lo, hi, skip = np.where(g, u, 0.0), np.where(g, u, 0.0), np.zeros(y.shape, dtype=bool)
    p = ~g
    lo[p], hi[p], skip[p] = count_cdf(y[p], m[p], s2[p], mean[p], n_nodes, max_count)
    with np.errstate(invalid="ignore"):
        return lo, hi, (y - mean) ** 2 / var, skip


def columns(lo, hi, pearson, skip, n_bins, levels):
    """The W = n_bins + len(levels) + 3 terms of every entry: (..., W)."""
    J, levels = int(n_bins), np.asarray(levels, dtype=float).reshape(-1)
    lo_, hi_ = np.where(skip, 0.0, lo), np.where(skip, 0.0, hi)
    out = np.zeros(lo.shape + (J + len(levels) + 3,))
    wide = hi_ > lo_
    w = np.where(wide, hi_ - lo_, 1.0)
    point = np.minimum(J - 1, np.floor(lo_ * J)).astype(int)
    for j in range(J):
        step = np.clip(((j + 1) / J - lo_) / w, 0.0, 1.0) - np.clip((j / J - lo_) / w, 0.0, 1.0)
        out[..., j] = np.where(wide, step, (point == j) * 1.0)
    for c, level in enumerate(levels):
        a = (1.0 - level) / 2.0
        out[..., J + c] = (hi_ >= a) & (lo_ < 1.0 - a)
    out[..., J + len(levels)] = np.where(skip, 0.0, pearson)
    out[..., J + len(levels) + 1] = 1.0
    out[skip] = 0.0
    out[..., J + len(levels) + 2] = skip
    return out


def edge_margin(lo, hi, skip, n_bins, levels):
    """The smallest distance of a scored entry from a discontinuity of its columns: hi from a, lo from 1 - a for every
    level, and lo from the inner bin edges 1 / J ... (J - 1) / J where hi == lo (the bin of a point mass; 0 and 1 are no
    discontinuities: the first and the last bin take them)."""
    use = ~skip & np.isfinite(lo)
    lo, hi = lo[use], hi[use]
    d = [np.inf]
    for level in np.asarray(levels, dtype=float).reshape(-1):
        a = (1.0 - level) / 2.0
        d += [np.abs(hi - a).min(initial=np.inf), np.abs(lo - (1.0 - a)).min(initial=np.inf)]
    point = lo[hi == lo]
    for j in range(1, int(n_bins)):
        d.append(np.abs(point - j / n_bins).min(initial=np.inf))
    return float(min(d))


def _unit_entries(units, mu, v, a, b, noise, gauss, vb, n_nodes, max_count):
    """The entries of the units' concatenated rows under mu, v (rows, L)."""
    bounds = np.cumsum([0] + [u["y"].shape[0] for u in units])
    got = [entries(u["y"], u["x"], mu[r0:r1], v[r0:r1], a, b, noise, gauss, vb, n_nodes, max_count)
           for u, r0, r1 in zip(units, bounds[:-1], bounds[1:])]
    return tuple(np.concatenate([g[k] for g in got]) for k in range(4))


def score_plain(units, a, b, noise, gauss, vb, n_nodes, n_bins, levels, max_count=4096):
    """``(cdf (rows, N, 2), sums (N, W), terms (rows, N, W))`` of a plain set under the units' own mu, v."""
    mu, v = (np.concatenate([u[k] for u in units]) for k in ("mu", "v"))
    lo, hi, pearson, skip = _unit_entries(units, mu, v, a, b, noise, gauss, vb, n_nodes, max_count)
    terms = columns(lo, hi, pearson, skip, n_bins, levels)
    return np.stack([lo, hi], axis=-1), terms.sum(axis=0), terms


def score_groups(units, groups, mu, v, a, b, noise, gauss, vb, n_nodes, n_bins, levels, max_count=4096):
    """Group replicas: mu, v (n_rep, rows, L); one column and one slot per (replica, channel) pair in the order of the
    concatenated groups.  ``(cdf (rows, n_pairs, 2), sums (n_pairs, W), terms (rows, n_pairs, W))``."""
    cdf, terms = [], []
    for k, g in enumerate(groups):
        lo, hi, pearson, skip = _unit_entries(units, mu[k], v[k], a, b, noise, gauss, vb, n_nodes, max_count)
        t = columns(lo, hi, pearson, skip, n_bins, levels)
        for n in g:
            cdf.append(np.stack([lo[:, n], hi[:, n]], axis=-1))
            terms.append(t[:, n])
    terms = np.stack(terms, axis=1)
    return np.stack(cdf, axis=1), terms.sum(axis=0), terms


def score_masked(units, held, mu, v, a, b, noise, gauss, vb, n_nodes, n_bins, levels, max_count=4096):
    """Masked replicas: held bool (n_rep, rows, N), mu, v (n_rep, rows, L).  ``(cdf (rows, N, 2), NaN where no replica
    holds the entry out, sums (n_rep, N, W) over each replica's held-out entries, terms (n_rep, rows, N, W))``."""
    cdf = np.full(held.shape[1:] + (2,), np.nan)
    terms = []
    for k in range(held.shape[0]):
        lo, hi, pearson, skip = _unit_entries(units, mu[k], v[k], a, b, noise, gauss, vb, n_nodes, max_count)
        terms.append(np.where(held[k][..., None], columns(lo, hi, pearson, skip, n_bins, levels), 0.0))
        cdf[held[k]] = np.stack([lo, hi], axis=-1)[held[k]]
    terms = np.stack(terms)
    return cdf, terms.sum(axis=1), terms


def truth_cdf(k, m, sigma, points=36001, half_width=9.0):
    """F(k) = P(Y <= k) of the Poisson-lognormal by a trapezoid of ``points`` points on z in [-half_width, half_width]:
    int pdtr(k, ex(m + sigma z)) phi(z) dz; F(-1) = 0.  Scalars."""
    if k < 0:
        return 0.0
    z = np.linspace(-half_width, half_width, points)
    f = pdtr(k, PN.ex(m + sigma * z)) * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
    return float((f.sum() - 0.5 * (f[0] + f[-1])) * (z[1] - z[0]))


def central_quantile(masses, p):
    """q_p = min{k : F(k) >= p} from the masses p(0), p(1), ... added in order; len(masses) if never reached."""
    F = 0.0
    for k, pk in enumerate(masses):
        F += pk
        if F >= p:
            return k
    return len(masses)
