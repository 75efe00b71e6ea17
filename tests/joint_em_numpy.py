"""The M-step under a full Gaussian posterior per row (vlgp_mstep_cov) and the Laplace EM loop around it
(vlgp_amd.refit_joint), stated in NumPy on top of tests/joint_cov_numpy.py.  Written from the definitions, dense and
independent of the package.

  moments   q[t, :, n] = C_t a_n, s2[t, n] = a_n . q[t, :, n], eta = mu a + x b, r = exp(min(eta + s2 / 2, 10)).
  Poisson   grad_a = mu'y_n - sum_t r_tn (mu_t + q_tn), nhess_a = sum_t r_tn [(mu_t + q_tn)(mu_t + q_tn)' + C_t];
            grad_b = x_n'(y_n - r_n), nhess_b = x_n' diag(r_n) x_n; Newton step with jitter eps, or learning_rate * grad
            when the system does not factor or use_hessian is off; steps clipped to da_bound / db_bound.
  Gaussian  a_n = (mu'mu + sum_t C_t)^-1 mu'(y_n - x_n b_n), then b_n = (x_n'x_n)^-1 x_n'(y_n - mu a_n), b_n[1:] = 0.
  noise     var(y - eta) at the parameters entering the last iteration.
  loop      E_k = sum of laplace under params_k; stop when E_k - E_{k-1} <= tol |E_k| (keeping the better of the two) or at
            k == max_iter; else params_{k+1} = mstep_cov(post_k).
"""
import numpy as np
import scipy.linalg as sla

import joint_cov_numpy as JC


def capped_exp(e):
    return np.exp(np.minimum(e, 10.0))


def _spd_solve(H, g):
    return sla.solve(H, g, assume_a="pos")


def split_cov(cov):
    """v (T, L), the diagonal of cov, and cov with its diagonal set to zero.  Every sum below takes the two parts one after
    the other, the diagonal part written as the reference writes its v terms (vlgp/core.py:181-235): a cov without
    off-diagonal entries then adds exact zeros to the reference's own arithmetic, and the golden fixtures of the
    reference hold for this statement to the last bit of a, so also for the steps da, db of a converged iteration,
    which are differences of nearly equal numbers."""
    L = cov.shape[1]
    v = np.ascontiguousarray(np.diagonal(cov, axis1=1, axis2=2))
    off = cov.copy()
    off[:, np.arange(L), np.arange(L)] = 0.0
    return v, off


def row_moments(mu, cov, a):
    """q (T, L, N) and s2 (T, N) of the header."""
    v, off = split_cov(cov)
    q_off = np.einsum("tlm,mn->tln", off, a)
    q = v[:, :, None] * a[None, :, :] + q_off
    return q, v @ a ** 2 + np.einsum("ln,tln->tn", a, q_off)


def rate_of(x, mu, cov, a, b):
    eta = mu @ a + np.einsum("tpn,pn->tn", x, b)
    return capped_exp(eta + 0.5 * row_moments(mu, cov, a)[1]), eta


def grad_hess_a(y_n, mu, cov, a, b, x, n):
    """grad_a (L) and nhess_a (L, L) of Poisson channel n at (a, b)."""
    q = row_moments(mu, cov, a)[0][:, :, n]
    r = rate_of(x, mu, cov, a, b)[0][:, n]
    shifted = mu + q
    g = mu.T @ y_n - shifted.T @ r
    H = shifted.T @ (r[:, None] * shifted) + np.einsum("t,tlm->lm", r, cov)
    return g, H  # (the plain form: the tests compare it with finite differences and with mstep_cov's split sums)


def mstep_cov(y, x, mu, cov, a, b, gauss, n_iter, use_hessian=True, eps=1e-8, learning_rate=1.0, da_bound=5.0, db_bound=5.0,
              noise=None):
    """y (rows, N), x (rows, P, N), mu (rows, L), cov (rows, L, L): all units concatenated.  Returns (a, b, da, db, noise);
    the inputs are not modified.  The number of systems that did not factor is left in ``mstep_cov.n_failed``."""
    a, b = np.array(a, dtype=float), np.array(b, dtype=float)
    L, N = a.shape
    P = b.shape[0]
    da, db = np.zeros_like(a), np.zeros_like(b)
    mstep_cov.n_failed = 0
    if n_iter < 1:
        return a, b, da, db, noise
    v, off = split_cov(cov)
    M = mu.T @ mu
    M[np.diag_indices(L)] += v.sum(axis=0)
    M = M + off.sum(axis=0)
    for _ in range(n_iter):
        rate, eta = rate_of(x, mu, cov, a, b)
        q = row_moments(mu, cov, a)[0]
        noise = np.var(y - eta, axis=0)
        for n in range(N):
            xn = x[:, :, n]
            if not gauss[n]:
                shifted = mu + q[:, :, n]
                g_a = mu.T @ y[:, n] - shifted.T @ rate[:, n]
                step = learning_rate * g_a
                if use_hessian:
                    h_a = shifted.T @ (rate[:, n:n + 1] * shifted)
                    h_a[np.diag_indices(L)] += rate[:, n] @ v
                    h_a = h_a + np.einsum("t,tlm->lm", rate[:, n], off)
                    try:
                        step = _spd_solve(h_a + eps * np.eye(L), g_a)
                    except (np.linalg.LinAlgError, ValueError):
                        mstep_cov.n_failed += 1
                step = np.clip(step, -da_bound, da_bound)
                da[:, n] = step
                a[:, n] += step
                g_b = xn.T @ (y[:, n] - rate[:, n])
                step = learning_rate * g_b
                if use_hessian:
                    h_b = xn.T @ (rate[:, n:n + 1] * xn)
                    try:
                        step = _spd_solve(h_b + eps * np.eye(P), g_b)
                    except (np.linalg.LinAlgError, ValueError):
                        mstep_cov.n_failed += 1
                step = np.clip(step, -db_bound, db_bound)
                db[:, n] = step
                b[:, n] += step
            else:
                a[:, n] = _spd_solve(M, mu.T @ (y[:, n] - xn @ b[:, n]))
                b[:, n] = _spd_solve(xn.T @ xn, xn.T @ (y[:, n] - mu @ a[:, n]))
                b[1:, n] = 0
    return a, b, da, db, noise


def cat_units(units, N):
    """y (rows, N) and x (rows, P, N) of a list of unit dicts; a missing x is the constant regressor."""
    y = np.concatenate([u["y"] for u in units]).astype(float)
    x = np.concatenate([u["x"] if u.get("x") is not None else np.ones((u["y"].shape[0], 1, N)) for u in units])
    return y, x


def posterior(units, a, b, noise, gauss, prior, newton_tol=1e-20):
    """The E-step: joint_cov_numpy.statement's per-unit dicts and, over the concatenated rows, mu and cov."""
    st = JC.statement(units, a, b, noise, gauss, prior, tol=newton_tol)
    return st, np.concatenate([s["mu"] for s in st]), np.concatenate([s["cov"] for s in st])


def refit(units, a, b, noise, gauss, prior, m_iter, max_iter=20, tol=1e-6, newton_tol=1e-20, trace_hook=None, **m_kw):
    """The loop of refit_joint.  Returns a dict: a, b, noise, da, db (None before the first M-step), mu, cov over the
    concatenated rows, the per-unit statement ``post`` of the returned parameters, ``trace`` (laplace, n_newton,
    converged per iteration) and ``kept``, the index of the iteration whose parameters are returned.  ``trace_hook(k,
    evidence)`` may replace an evidence before the rules read it (the tests drive the stop rules with it)."""
    N = a.shape[1]
    y, x = cat_units(units, N)
    cur = (np.array(a, float), np.array(b, float), np.array(noise, float), None, None)
    trace = {"laplace": [], "n_newton": [], "converged": []}
    prev, k = None, 0
    while True:
        st, mu, cov = posterior(units, cur[0], cur[1], cur[2], gauss, prior, newton_tol)
        ev = float(sum(s["laplace"] for s in st))
        if trace_hook is not None:
            ev = float(trace_hook(k, ev))
        trace["laplace"].append(ev)
        trace["n_newton"].append(max(int(s["n_newton"]) for s in st))
        trace["converged"].append(all(bool(s["converged"]) for s in st))
        kept = k
        if prev is not None and ev - prev[4] <= tol * abs(ev):
            if not ev >= prev[4]:
                cur, st, mu, cov = prev[:4]
                kept = k - 1
            break
        if k == max_iter:
            break
        prev = (cur, st, mu, cov, ev)
        out = mstep_cov(y, x, mu, cov, cur[0], cur[1], gauss, m_iter, **m_kw)
        cur = (out[0], out[1], out[4], out[2], out[3])
        k += 1
    return {"a": cur[0], "b": cur[1], "noise": cur[2], "da": cur[3], "db": cur[4], "mu": mu, "cov": cov, "post": st,
            "trace": trace, "kept": kept}


def tiny_problem(seed=3):
    """The seeded tiny problem of the loop tests: ichol factors, 2 latents, 8 channels of which 2 Gaussian, 6 ragged trials
    of 20 - 40 bins, a random start of the loading.  Returns (units, params, gauss) as test_gpu_marginal._problem does."""
    from test_gpu_marginal import _problem

    rng = np.random.default_rng(seed)
    lengths = [int(t) for t in rng.integers(20, 41, size=6)]
    units, params, gauss = _problem(lengths, 8, 2, [5e-3, 2e-2], seed=seed, n_gauss=2, rank=12)
    return units, params, gauss
