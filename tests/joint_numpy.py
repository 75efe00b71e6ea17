"""The joint Laplace posterior of vlgp_amd.evaluation.joint_posterior (vlgp_joint_laplace) stated in NumPy, for the tests
of the device kernels and of the public path.  Written from the definitions, independent of the package.

For one unit of T rows: G_l (T x r_l) the prior factor bound to the unit's length cut to its leading non-zero columns,
the stacked index (l, i) latent-major, D = sum_l r_l, Gs (T x D) the factors side by side.
  x[:, l] = G_l beta_l,  eta = x a + (b x)                                                        (no v term)
  Poisson   lam = exp(min(eta, 10)),  ll = y eta - lam - lgamma(y + 1),  res = y - lam,  cur = lam
  Gaussian  ll = -1/2 log(2 pi noise) - (y - eta)^2 / (2 noise),  res = (y - eta) / noise,  cur = 1 / noise
  f(beta) = 1/2 |beta|^2 - sum ll,  grad_l f = beta_l - G_l' (res a')[:, l]
  H[(l, i), (l', j)] = delta + sum_t G_l[t, i] c[t, l, l'] G_l'[t, j],  c[t, l, l'] = sum_n a[l, n] a[l', n] cur[t, n]
  Newton: d = H^-1 grad f, halved until f(beta - s d) <= f(beta) - 1e-4 s grad f' d, until grad f' H^-1 grad f <= tol
  laplace = ll(beta) - 1/2 |beta|^2 - 1/2 log det H(beta)
  mu[:, l] = G_l beta_l,  v[t, l] = G_l[t] (H^-1)_ll G_l[t]'
  draw k: beta_k = beta + Lc^-T eps_k,  c_k = -1/2 |beta_k|^2 + 1/2 |eps_k|^2 - 1/2 log det H,  log_w = ll(beta_k) + c_k
The scale of a sum's rounding error is the sum of the absolute values of what is added into it.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular
from scipy.special import gammaln

from forecast_numpy import gradient, rank, weight_posterior


class Unit:
    """One unit dict (y, x or None) under G_in (L, T, R): the stacked factor and the model's pieces at a beta (D)."""

    def __init__(self, u, a, b, noise, gauss, G_in):
        self.y, self.a, self.b, self.noise, self.gauss = np.asarray(u["y"], float), a, b, noise, np.asarray(gauss, bool)
        x = u.get("x")
        self.off = np.einsum("tpn,pn->tn", x, b) if x is not None else np.tile(b[0], (self.y.shape[0], 1))
        self.L = a.shape[0]
        self.ranks = [rank(G_in[l]) for l in range(self.L)]
        self.G = [G_in[l][:, :r] for l, r in enumerate(self.ranks)]
        self.start = np.concatenate([[0], np.cumsum(self.ranks)]).astype(int)
        self.D = int(self.start[-1])

    def split(self, beta):
        return [beta[self.start[l]:self.start[l + 1]] for l in range(self.L)]

    def paths(self, beta):
        """x (..., T, L) for beta (D) or (D, K) -> (K, T, L)."""
        cols = [G @ bl for G, bl in zip(self.G, self.split(beta))]
        return np.stack(cols, axis=-1) if beta.ndim == 1 else np.stack([c.T for c in cols], axis=-1)

    def terms(self, x):
        """log p(y[t, n] | eta) for paths x (..., T, L), and eta."""
        eta = x @ self.a + self.off
        lp = self.y * eta - np.exp(np.minimum(eta, 10.0)) - gammaln(self.y + 1.0)
        lg = -0.5 * np.log(2.0 * np.pi * self.noise) - (self.y - eta) ** 2 / (2.0 * self.noise)
        return np.where(self.gauss, lg, lp), eta

    def ll(self, beta):
        return float(self.terms(self.paths(beta))[0].sum())

    def f(self, beta):
        return 0.5 * float(beta @ beta) - self.ll(beta)

    def res_cur(self, beta):
        eta = self.terms(self.paths(beta))[1]
        lam = np.exp(np.minimum(eta, 10.0))
        return (np.where(self.gauss, (self.y - eta) / self.noise, self.y - lam),
                np.where(self.gauss, 1.0 / self.noise + 0.0 * eta, lam))

    def grad(self, beta):
        g = self.res_cur(beta)[0] @ self.a.T
        return beta - np.concatenate([G.T @ g[:, l] for l, G in enumerate(self.G)])

    def hessian(self, beta):
        cur = self.res_cur(beta)[1]
        c = np.einsum("ln,mn,tn->tlm", self.a, self.a, cur)
        H = np.eye(self.D)
        for l in range(self.L):
            for m in range(self.L):
                H[self.start[l]:self.start[l + 1], self.start[m]:self.start[m + 1]] += self.G[l].T @ (c[:, l, m, None] * self.G[m])
        return H

    def abs_terms(self, beta):
        """The sum of the absolute values of what is added into f, ll and laplace at beta."""
        return float(np.abs(self.terms(self.paths(beta))[0]).sum() + 0.5 * beta @ beta)


def mean_field_start(U, u, vb=False):
    """The stacked mean-field centres m_l = H_l^-1 G_l'(g + w o mu)_l from the unit's mu, w (the v term dropped)."""
    g = gradient(U.y, u.get("x"), u["mu"], u["v"], U.a, U.b, U.noise, U.gauss, vb)
    z = g + u["w"] * u["mu"]
    return np.concatenate([weight_posterior(U.G[l], u["w"][:, l], z[:, l])[0] for l in range(U.L)])


def newton(U, beta0, tol=1e-20, max_iter=200):
    """The mode from beta0: (beta, decrement, factorisations, converged).  Full steps halved against the sufficient-decrease
    test; near the mode, where f no longer resolves the decrease, the full step is taken."""
    beta, n = np.array(beta0, float), 0
    while True:
        g, H = U.grad(beta), U.hessian(beta)
        Lc = np.linalg.cholesky(H)
        d = cho_solve((Lc, True), g)
        dec = float(g @ d)
        n += 1
        if dec <= tol:
            return beta, dec, n, True
        if n >= max_iter:
            return beta, dec, n, False
        f0, s = U.f(beta), 1.0
        while s > 2.0 ** -30 and not U.f(beta - s * d) <= f0 - 1e-4 * s * dec + 2.0 ** -46 * U.abs_terms(beta - s * d):
            s *= 0.5
        if s <= 2.0 ** -30:
            return beta, dec, n, False
        beta = beta - s * d


def summary(U, beta):
    """What follows from a beta: dict of laplace, ll, beta_sq, logdet, mu (T, L), v (T, L), Lc, H and scale (the sum of
    absolute terms behind laplace)."""
    H = U.hessian(beta)
    Lc = np.linalg.cholesky(H)
    logdet = 2.0 * float(np.sum(np.log(np.diag(Lc))))
    Hinv = cho_solve((Lc, True), np.eye(U.D))
    v = np.stack([np.einsum("ti,ij,tj->t", U.G[l], Hinv[U.start[l]:U.start[l + 1], U.start[l]:U.start[l + 1]], U.G[l])
                  for l in range(U.L)], axis=1)
    ll, b2 = U.ll(beta), float(beta @ beta)
    return {"laplace": ll - 0.5 * b2 - 0.5 * logdet, "ll": ll, "beta_sq": b2, "logdet": logdet, "mu": U.paths(beta), "v": v,
            "Lc": Lc, "H": H, "scale": U.abs_terms(beta) + 0.5 * abs(logdet)}


def draws(U, beta, Lc, eps):
    """eps (L, R, K), rows >= r_l not read.  Returns log_w (K), ll (K), c (K), the sum of absolute terms behind log_w (K)
    and the draws beta_k (D, K)."""
    e = np.concatenate([eps[l][:r] for l, r in enumerate(U.ranks)], axis=0)
    bk = beta[:, None] + solve_triangular(Lc.T, e, lower=False)
    logdet = 2.0 * float(np.sum(np.log(np.diag(Lc))))
    b2, e2 = np.sum(bk ** 2, axis=0), np.sum(e ** 2, axis=0)
    c = -0.5 * b2 + 0.5 * e2 - 0.5 * logdet
    terms = U.terms(U.paths(bk))[0]
    ll = terms.sum(axis=(1, 2))
    return ll + c, ll, c, np.abs(terms).sum(axis=(1, 2)) + 0.5 * b2 + 0.5 * e2 + 0.5 * abs(logdet), bk


def statement(units, a, b, noise, gauss, prior, eps=None, tol=1e-20, beta=None):
    """Everything vlgp_joint_laplace reports for a list of unit dicts (y, x or None, mu, v, w) under
    prior = {T: (L, T, R)}: a list of per-unit dicts with summary's keys plus beta (D), ranks, decrement, n_newton,
    converged and, with eps (units, L, R, K), log_w, ll_k, c_k, scale_k.  beta: a list of stacked vectors to evaluate at
    instead of the mode (the device's own, for the draws)."""
    out = []
    for i, u in enumerate(units):
        U = Unit(u, a, b, noise, gauss, prior[u["y"].shape[0]])
        if beta is None:
            bt, dec, n, conv = newton(U, mean_field_start(U, u), tol)
        else:
            bt, dec, n, conv = np.asarray(beta[i], float), np.nan, 0, True
        res = summary(U, bt)
        res.update(beta=bt, ranks=U.ranks, decrement=dec, n_newton=n, converged=conv, unit=U)
        if eps is not None:
            res["log_w"], res["ll_k"], res["c_k"], res["scale_k"], _ = draws(U, bt, res["Lc"], eps[i])
        out.append(res)
    return out


def stack_beta(beta_dev, ranks):
    """The device's (L, R) layout of one unit cut to the stacked vector (D)."""
    return np.concatenate([beta_dev[l, :r] for l, r in enumerate(ranks)])
