"""The forward prediction of vlgp_amd.evaluation (vlgp_forecast) stated in NumPy, for the tests of the device kernels and
of the public path.  Written from the definitions, independent of the package.

For one unit and latent l: G (T_in x r) the prior factor bound to the unit's length cut to its leading non-zero columns,
G_ext (n_ext x R) the rows of the same factorisation at the unobserved bins, mu, v, w the unit's posterior columns.
  g[t] = sum_n a[l, n] res[t, n];  res = y - exp(min(eta + 1/2 (a^2).v, 10)) Poisson, (y - eta) / noise Gaussian;
  eta = a.mu + (b x); the v term dropped when vb is false
  H = I_r + G' diag(w) G = Lc Lc',  beta = H^-1 G' (g + w o mu)
  mu_ext = G_ext[:, :r] beta,  v_ext[t] = |Lc^-1 G_ext[t, :r]'|^2 + sum_{c >= r} G_ext[t, c]^2  (0 when vb is false)
  fit_terms = (|G beta - mu|^2, |mu|^2)
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular


def rank(G):
    """Number of leading columns of a (T, R) factor up to its last non-zero one (at least 1)."""
    nz = np.flatnonzero(np.any(G != 0.0, axis=0))
    return int(nz[-1]) + 1 if nz.size else 1


def gradient(y, x, mu, v, a, b, noise, gauss, vb=True):
    """(T, L) working gradient g; x (T, P, N) or None for x == 1."""
    eta = mu @ a + (np.einsum("tpn,pn->tn", x, b) if x is not None else b[0][None, :])
    s = 0.5 * (v @ a ** 2) if vb else 0.0
    res = np.where(gauss, (y - eta) / noise, y - np.exp(np.minimum(eta + s, 10.0)))
    return res @ a.T


def weight_posterior(G, w, z):
    """(beta, Lc) for a compact factor G (T, r), w (T) and z = g + w o mu (T)."""
    H = np.eye(G.shape[1]) + G.T @ (w[:, None] * G)
    Lc = np.linalg.cholesky(H)
    return cho_solve((Lc, True), G.T @ z), Lc


def variance_rows(Lc, rows):
    """|Lc^-1 row'|^2 for every row of `rows` (n, r)."""
    return np.sum(solve_triangular(Lc, rows.T, lower=True) ** 2, axis=0)


def extend(G_in, G_ext, mu, w, z, vb=True):
    """One (unit, latent): G_in (T_in, R), G_ext (n_ext, R) full-width, mu, w, z (T_in).
    Returns mu_ext (n_ext), v_ext (n_ext), fit_terms (2), beta (r), H (r, r)."""
    r = rank(G_in)
    G = G_in[:, :r]
    beta, Lc = weight_posterior(G, w, z)
    mu_ext = G_ext[:, :r] @ beta
    if vb:
        v_ext = variance_rows(Lc, G_ext[:, :r]) + np.sum(G_ext[:, r:] ** 2, axis=1)
    else:
        v_ext = np.zeros(G_ext.shape[0])
    d = G @ beta - mu
    return mu_ext, v_ext, np.array([d @ d, mu @ mu]), beta, Lc @ Lc.T


def forecast_unit(u, a, b, noise, gauss, G_in, G_ext, vb=True):
    """One unit dict (y, x or None, mu, v, w) under G_in (L, T_in, R), G_ext (L, n_ext, R).
    Returns mu_ext (n_ext, L), v_ext (n_ext, L), fit_terms (L, 2), the betas and the matrices H per latent."""
    L = a.shape[0]
    g = gradient(u["y"], u.get("x"), u["mu"], u["v"], a, b, noise, gauss, vb)
    z = g + u["w"] * u["mu"]
    parts = [extend(G_in[l], G_ext[l], u["mu"][:, l], u["w"][:, l], z[:, l], vb) for l in range(L)]
    return (np.stack([p[0] for p in parts], axis=1), np.stack([p[1] for p in parts], axis=1),
            np.stack([p[2] for p in parts]), [p[3] for p in parts], [p[4] for p in parts])


def statement(units, a, b, noise, gauss, prior, ext, vb=True):
    """Everything vlgp_forecast reports for a list of unit dicts under prior = {T_in: (L, T_in, R)} and
    ext = {T_in: (L, n_ext, R)}: mu_ext, v_ext (sum n_ext, L) unit-major, fit_terms (units, L, 2), and the largest
    cond(I + H) over the tasks (H as defined above already holds the identity once)."""
    mus, vs, terms, cond = [], [], [], 0.0
    for u in units:
        T = u["y"].shape[0]
        m, v, t, _, Hs = forecast_unit(u, a, b, noise, gauss, prior[T], ext[T], vb)
        mus.append(m)
        vs.append(v)
        terms.append(t)
        cond = max([cond] + [float(np.linalg.cond(np.eye(len(H)) + H)) for H in Hs])
    return np.concatenate(mus), np.concatenate(vs), np.stack(terms), cond
