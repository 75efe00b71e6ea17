"""The variational lower bound of vlgp_amd.evaluation.elbo stated in NumPy (numpy.linalg: lstsq, slogdet, inv), for the
tests of the device kernels and of the host assembly.  Written from the definitions, independent of the package.

For one unit, latent l, G (T x r) the prior factor with its all-zero columns dropped, w = w[:, l], mu = mu[:, l]:
H = I_r + G' diag(w) G, S = H^-1, beta = argmin |G beta - mu|, KL = 1/2 (tr S + beta'beta - r + log det H).
Expected log-likelihood of y[t, n] with eta = a[:, n] . mu[t] + b[:, n] . x[t, :, n], s = 1/2 (a[:, n]^2) . v[t]:
Poisson y eta - exp(min(eta + s, 10)) - lgamma(y + 1); Gaussian -1/2 log(2 pi noise) - ((y - eta)^2 + 2 s) / (2 noise).
"""
import numpy as np
from scipy.special import gammaln


def compact(G):
    """Drop the all-zero columns of a (T, R) factor."""
    return G[:, np.any(G != 0.0, axis=0)]


def kl_terms(G, w, mu):
    """(log det H, tr S, beta'beta, |mu - G beta|^2, r) for a factor whose zero columns are already dropped."""
    r = G.shape[1]
    H = np.eye(r) + G.T @ (w[:, None] * G)
    sign, logdet = np.linalg.slogdet(H)
    assert sign > 0
    S = np.linalg.inv(H)
    beta = np.linalg.lstsq(G, mu, rcond=None)[0]
    res = mu - G @ beta
    return logdet, float(np.trace(S)), float(beta @ beta), float(res @ res), r


def kl_from_terms(t):
    logdet, tr_s, bb, _, r = t
    return 0.5 * (tr_s + bb - r + logdet)


def row_terms(y, x, mu, v, a, b, noise, gauss, vb=True):
    """(T, N, 4) summands of the row pass: E_q log p | y | rate (Gaussian: eta) | y s (Gaussian: s / noise)."""
    T, N = y.shape
    eta = mu @ a + (np.einsum("tpn,pn->tn", x, b) if x is not None else b[0][None, :])
    s = 0.5 * (v @ a ** 2) if vb else np.zeros((T, N))
    lam = np.exp(np.minimum(eta + s, 10.0))
    ep = y * eta - lam - gammaln(y + 1.0)
    eg = -0.5 * np.log(2.0 * np.pi * noise) - ((y - eta) ** 2 + 2.0 * s) / (2.0 * noise)
    out = np.empty((T, N, 4))
    out[:, :, 0] = np.where(gauss, eg, ep)
    out[:, :, 1] = y
    out[:, :, 2] = np.where(gauss, eta, lam)
    out[:, :, 3] = np.where(gauss, s / noise, y * s)
    return out


def statement(units, a, b, noise, gauss, chol, vb=True):
    """Everything the device reports for a list of unit dicts (y, x or None, mu, v, w) under chol = {T: (L, T, R)}:
    row_sums (N, 4), their absolute-value sums (the scale of a sum's rounding error), row_ell (rows), terms
    (units, L, 4), ranks (units, L), kl (units, L), mu_sq (units, L)."""
    L = a.shape[0]
    rows = [row_terms(u["y"], u.get("x"), u["mu"], u["v"], a, b, noise, gauss, vb) for u in units]
    allrows = np.concatenate(rows, axis=0)
    out = {"row_sums": allrows.sum(axis=0), "row_abs": np.abs(allrows).sum(axis=0),
           "row_ell": allrows[:, :, 0].sum(axis=1)}
    terms = np.empty((len(units), L, 4))
    ranks = np.empty((len(units), L), dtype=np.int64)
    kl = np.empty((len(units), L))
    for i, u in enumerate(units):
        T = u["y"].shape[0]
        for l in range(L):
            t = kl_terms(compact(chol[T][l]), u["w"][:, l], u["mu"][:, l])
            terms[i, l] = t[:4]
            ranks[i, l] = t[4]
            kl[i, l] = kl_from_terms(t)
    out.update(terms=terms, ranks=ranks, kl=kl, mu_sq=np.array([np.sum(u["mu"] ** 2, axis=0) for u in units]))
    return out
