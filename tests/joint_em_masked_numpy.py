"""The covariance M-step with missing observations (vlgp_mstep_cov_masked) and the Laplace EM loop around it
(vlgp_amd.refit_joint(..., missing=)), stated in NumPy on top of tests/joint_em_numpy.py and tests/joint_cov_numpy.py.

No new arithmetic.  The update of channel n is ``joint_em_numpy.mstep_cov``'s on that channel's observed rows: the rows
are taken out of every array before a sum is formed -- no select, no zero coefficient in the Newton sums, the missing rows
are simply not there.  The E-step is ``joint_cov_numpy.statement`` with ``held=missing``, whose
likelihood terms leave the held entries out.  ``missing`` is True where y is absent; y is never read there."""
import numpy as np

import joint_cov_numpy as JC
import joint_em_numpy as EM
import masked_fit_numpy as MF  # noqa: F401  (the diagonal case of this statement: tests/test_joint_em_masked_host.py)


def mstep_cov_masked(y, x, mu, cov, a, b, missing, n_iter, use_hessian=True, eps=1e-8, learning_rate=1.0, da_bound=5.0,
                     db_bound=5.0, noise=None):
    """y (rows, N), x (rows, P, N), mu (rows, L), cov (rows, L, L), missing (rows, N) bool.  Returns (a, b, da, db, noise)
    after ``n_iter`` Newton iterations with every (Poisson) channel on its observed rows only; ``noise`` is the variance
    of y - eta over those rows.  A channel without an observed row keeps a, b and noise; its steps are 0.  The number of
    systems that did not factor is left in ``mstep_cov_masked.n_failed``; the inputs are not modified.

    ``joint_em_numpy.mstep_cov`` line by line -- the rate, eta and q of all channels at once, then channel by channel --
    with the rows of channel n taken out of every array before its sums are formed, and ``np.var``'s own two passes
    (mean, then the centred squares) over the channel's rows.  With no entry missing every operand is that statement's:
    the same bits."""
    a, b = np.array(a, dtype=float), np.array(b, dtype=float)
    L, N = a.shape
    P = b.shape[0]
    missing = np.asarray(missing, dtype=bool)
    obs = ~missing
    n_obs = obs.sum(axis=0)
    noise = np.ones(N) if noise is None else np.array(noise, dtype=float)
    da, db = np.zeros_like(a), np.zeros_like(b)
    mstep_cov_masked.n_failed = 0
    if n_iter < 1:
        return a, b, da, db, noise
    y = np.where(missing, 0.0, y)  # (what y holds there is not read: the rows are taken out below)
    v, off = EM.split_cov(cov)
    for _ in range(n_iter):
        rate, eta = EM.rate_of(x, mu, cov, a, b)
        q = EM.row_moments(mu, cov, a)[0]
        res = y - eta
        mean = np.where(obs, res, 0.0).sum(axis=0, keepdims=True) / np.maximum(n_obs, 1)
        dev = np.where(obs, res - mean, 0.0)
        var = (dev * dev).sum(axis=0) / np.maximum(n_obs, 1)
        noise = np.where(n_obs > 0, var, noise)
        for n in range(N):
            if n_obs[n] == 0:
                continue
            rows = obs[:, n]
            # (rows first, then the column: the operands keep the strides they have in that statement, on which NumPy's
            # choice of a matrix-vector routine, and with it the last bit, depends)
            xn, mun, yn, rn, vn, offn = x[rows][:, :, n], mu[rows], y[rows][:, n], rate[rows][:, n], v[rows], off[rows]
            shifted = mun + q[rows][:, :, n]
            g_a = mun.T @ yn - shifted.T @ rn
            step = learning_rate * g_a
            if use_hessian:
                h_a = shifted.T @ (rn[:, None] * shifted)
                h_a[np.diag_indices(L)] += rn @ vn
                h_a = h_a + np.einsum("t,tlm->lm", rn, offn)
                try:
                    step = EM._spd_solve(h_a + eps * np.eye(L), g_a)
                except (np.linalg.LinAlgError, ValueError):
                    mstep_cov_masked.n_failed += 1
            step = np.clip(step, -da_bound, da_bound)
            da[:, n] = step
            a[:, n] += step
            g_b = xn.T @ (yn - rn)
            step = learning_rate * g_b
            if use_hessian:
                h_b = xn.T @ (rn[:, None] * xn)
                try:
                    step = EM._spd_solve(h_b + eps * np.eye(P), g_b)
                except (np.linalg.LinAlgError, ValueError):
                    mstep_cov_masked.n_failed += 1
            step = np.clip(step, -db_bound, db_bound)
            db[:, n] = step
            b[:, n] += step
    return a, b, da, db, noise


def masked_Q(y_n, x_n, mu, cov, a_n, b_n, miss_n):
    """Q(a_n, b_n) = sum over the observed rows of y (a.mu + x b) - exp(a.mu + x b + a'C_t a / 2), below the clamp, and the
    sum of the absolute values of its terms (the scale its finite differences are held to)."""
    rows = ~miss_n
    lin = mu[rows] @ a_n + x_n[rows] @ b_n
    ex = lin + 0.5 * np.einsum("l,tlm,m->t", a_n, cov[rows], a_n)
    assert ex.max() < 10.0
    return float(np.sum(y_n[rows] * lin - np.exp(ex))), float(np.sum(np.abs(y_n[rows] * lin) + np.exp(ex)))


def grad_hess_a_masked(y_n, x_n, mu, cov, a_n, b_n, miss_n):
    """grad_a (L) and nhess_a (L, L) of a Poisson channel over its observed rows: joint_em_numpy.grad_hess_a on them."""
    rows = ~miss_n
    return EM.grad_hess_a(y_n[rows], mu[rows], cov[rows], a_n[:, None], b_n[:, None], x_n[rows][:, :, None], 0)


def posterior_masked(units, missing, a, b, noise, gauss, prior, newton_tol=1e-20):
    """The E-step: joint_cov_numpy.statement with the missing entries held out; per-unit dicts, mu and cov over all rows.
    ``missing``: one (T, N) bool array per unit."""
    held = np.concatenate([np.asarray(m, dtype=bool) for m in missing])
    st = JC.statement(units, a, b, noise, gauss, prior, tol=newton_tol, held=held)
    return st, np.concatenate([s["mu"] for s in st]), np.concatenate([s["cov"] for s in st])


def refit_masked(units, missing, a, b, noise, gauss, prior, m_iter, max_iter=20, tol=1e-6, newton_tol=1e-20, trace_hook=None,
                 **m_kw):
    """``joint_em_numpy.refit`` with ``posterior_masked`` as the E-step and ``mstep_cov_masked`` as the M-step: the same
    rules, the same dict.  ``missing``: one (T, N) bool array per unit.  E_k is the evidence of the observed entries."""
    N = a.shape[1]
    assert not np.any(gauss)
    y, x = EM.cat_units(units, N)
    M = np.concatenate([np.asarray(m, dtype=bool) for m in missing])
    cur = (np.array(a, float), np.array(b, float), np.array(noise, float), None, None)
    trace = {"laplace": [], "n_newton": [], "converged": []}
    prev, k = None, 0
    while True:
        st, mu, cov = posterior_masked(units, missing, cur[0], cur[1], cur[2], gauss, prior, newton_tol)
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
        out = mstep_cov_masked(y, x, mu, cov, cur[0], cur[1], M, m_iter, noise=cur[2], **m_kw)
        cur = (out[0], out[1], out[4], out[2], out[3])
        k += 1
    return {"a": cur[0], "b": cur[1], "noise": cur[2], "da": cur[3], "db": cur[4], "mu": mu, "cov": cov, "post": st,
            "trace": trace, "kept": kept}


def tiny_problem(seed=3, fraction=0.3):
    """joint_em_numpy.tiny_problem without Gaussian channels (2 latents, 8 Poisson channels, 6 ragged trials of 20 - 40
    bins, a random start of the loading) and a seeded mask of about ``fraction`` of the entries per trial.  Returns
    (units, params, gauss, missing)."""
    from test_gpu_marginal import _problem

    rng = np.random.default_rng(seed)
    lengths = [int(t) for t in rng.integers(20, 41, size=6)]
    units, params, gauss = _problem(lengths, 8, 2, [5e-3, 2e-2], seed=seed, n_gauss=0, rank=12)
    missing = [rng.random(u["y"].shape) < fraction for u in units]
    return units, params, gauss, missing
