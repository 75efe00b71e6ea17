"""The importance weights of vlgp_amd.evaluation.marginal_loglik (vlgp_marginal) stated in NumPy, for the tests of the
device kernels and of the public path.  Written from the definitions, independent of the package.

For one unit of length T and latent l: G (T x r) the prior factor bound to the unit's length cut to its leading non-zero
columns, mu, v, w the unit's posterior columns, eps (R x K) standard normals of which rows >= r are not read.
  g, z = g + w o mu as in forecast_numpy;  H = I_r + G' diag(w) G = Lc Lc',  m = H^-1 G' z
  draw k:  d = Lc^-T eps[:r, k],  beta_k = m + d,  x_k[:, l] = G beta_k
  c[l, k] = -1/2 |beta_k|^2 + 1/2 |eps_k|^2 - 1/2 log det H
  ll[k] = sum_t sum_n log p(y[t, n] | eta = a[:, n] . x_k[t] + (b x)_tn)           (no v term)
    Poisson y eta - exp(min(eta, 10)) - lgamma(y + 1);  Gaussian -1/2 log(2 pi noise) - (y - eta)^2 / (2 noise)
  log_w[k] = ll[k] + sum_l c[l, k]
The scale of a log_w's rounding error is the sum of the absolute values of what is added into it: every log p(y[t, n] | .)
and the three addends of every c[l, k].
"""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import gammaln

from forecast_numpy import gradient, rank, weight_posterior


def draws(G_in, w, z, eps):
    """One (unit, latent): G_in (T, R), w, z (T), eps (R, K).  Returns beta (r, K), c (K), its absolute addends summed
    (K), and the three pieces m (r), Lc (r, r), log det H."""
    r = rank(G_in)
    G = G_in[:, :r]
    m, Lc = weight_posterior(G, w, z)
    e = eps[:r]
    beta = m[:, None] + solve_triangular(Lc.T, e, lower=False)
    logdet = 2.0 * np.sum(np.log(np.diag(Lc)))
    b2, e2 = np.sum(beta ** 2, axis=0), np.sum(e ** 2, axis=0)
    return beta, -0.5 * b2 + 0.5 * e2 - 0.5 * logdet, 0.5 * b2 + 0.5 * e2 + 0.5 * abs(logdet), (m, Lc, logdet)


def loglik_terms(y, x, paths, a, b, noise, gauss):
    """(K, T, N) log p(y[t, n] | eta) under paths (K, T, L); x (T, P, N) or None for x == 1."""
    eta = paths @ a + (np.einsum("tpn,pn->tn", x, b) if x is not None else b[0][None, :])[None]
    lp = y * eta - np.exp(np.minimum(eta, 10.0)) - gammaln(y + 1.0)
    lg = -0.5 * np.log(2.0 * np.pi * noise) - (y - eta) ** 2 / (2.0 * noise)
    return np.where(gauss, lg, lp)


def unit_weights(u, a, b, noise, gauss, G_in, eps, vb=True):
    """One unit dict (y, x or None, mu, v, w) under G_in (L, T, R) and eps (L, R, K).
    Returns log_w (K), ll (K), c (L, K) and the sum of absolute terms behind every log_w (K)."""
    L = a.shape[0]
    g = gradient(u["y"], u.get("x"), u["mu"], u["v"], a, b, noise, gauss, vb)
    z = g + u["w"] * u["mu"]
    K = eps.shape[2]
    paths = np.empty((K, u["y"].shape[0], L))
    c, scale = np.empty((L, K)), np.zeros(K)
    for l in range(L):
        beta, c[l], c_abs, _ = draws(G_in[l], u["w"][:, l], z[:, l], eps[l])
        paths[:, :, l] = (G_in[l][:, :beta.shape[0]] @ beta).T
        scale += c_abs
    terms = loglik_terms(u["y"], u.get("x"), paths, a, b, noise, gauss)
    ll = terms.sum(axis=(1, 2))
    csum = np.zeros(K)
    for l in range(L):
        csum = csum + c[l]
    return ll + csum, ll, c, scale + np.abs(terms).sum(axis=(1, 2))


def statement(units, a, b, noise, gauss, prior, eps, vb=True):
    """Everything vlgp_marginal reports for a list of unit dicts under prior = {T: (L, T, R)} and eps (units, L, R, K):
    log_w (units, K), parts (units, K, 2) = {ll, sum_l c}, and the sum of absolute terms behind every log_w (units, K)."""
    out = [unit_weights(u, a, b, noise, gauss, prior[u["y"].shape[0]], eps[i], vb) for i, u in enumerate(units)]
    log_w = np.stack([o[0] for o in out])
    parts = np.stack([np.stack([o[1], o[2].sum(axis=0)], axis=1) for o in out])
    return log_w, parts, np.stack([o[3] for o in out])
