"""The hyperparameter step of the Laplace EM loop (vlgp_joint_posterior_moments, vlgp_amd.gp.optimize_joint,
vlgp_amd.refit_joint(..., hstep=True)), stated in NumPy on top of tests/joint_cov_numpy.py and tests/joint_em_numpy.py.
Written from the definitions, dense and independent of the package.

For a unit of T rows and latent l: m = G_l beta_l (column l of mu), Sigma_ll the r_l x r_l diagonal block of H^-1 at the
mode, W = config["window"].
  windows    the starts of a unit are s = k W, k = 0 ... T // W - 1, and one more at s = T - W when T % W != 0 (it overlaps its
             neighbour, as the reference's cut lets segments overlap); a unit with T < W has none.  n_w counts them all.
  moments    S_l = sum over units and starts of  m[s:s+W] m[s:s+W]' + G_l[s:s+W] Sigma_ll G_l[s:s+W]'        (L, W, W)
  objective  K = sigma_l^2 exp(-omega D2) + gp_noise I, D2_ij = (dt (i - j))^2,
             ll_l = -1/2 tr(K^-1 S_l) - n_w / 2 log|K|,
             d ll_l / d ln omega = 1/2 tr[(K^-1 S_l K^-1 - n_w K^-1) dK],  dK = -omega D2 o sigma_l^2 exp(-omega D2)
             -- the reference's gp.elbo(params, [0, 1, 0], t, mu, post_cov) summed over the windows with post_cov held fixed.
  optimiser  oracle.hstep_arrays' in every respect but the objective: L-BFGS-B on log(sigma^2, omega, gp_noise) within
             log((1e-3, 1), omega_bound, (gp_noise / 2, 2 gp_noise)), the gradient non-zero in ln omega only; omega[l] is
             taken over unless the result is close to a bound; sigma[l] = sqrt(sigma^2), which does not move.
  loop       joint_em_numpy.refit (or refit_masked) with this step after the M-step and the prior factors rebuilt
             (oracle.ichol_gauss at the new omega) before the next E-step; the better-of-the-last-two rule restores omega
             and the factors with a, b, noise.
"""
import math

import numpy as np
from scipy.linalg import cho_solve
from scipy.optimize import minimize

import joint_cov_numpy as JC
import joint_em_masked_numpy as EMM
import joint_em_numpy as EM
from oracle import vlgp_oracle as O


def window_starts(T, W):
    if T < W:
        return []
    starts = [k * W for k in range(T // W)]
    if T % W:
        starts.append(T - W)
    return starts


def n_windows(lengths, W):
    return sum(len(window_starts(int(T), W)) for T in lengths)


def latent_blocks(s):
    """[(m (T), G_l (T, r_l), Sigma_ll (r_l, r_l))] of one of joint_cov_numpy.statement's per-unit dicts."""
    U = s["unit"]
    Hinv = cho_solve((np.linalg.cholesky(s["H"]), True), np.eye(U.D))
    return [(s["mu"][:, l], U.G[l], Hinv[U.start[l]:U.start[l + 1], U.start[l]:U.start[l + 1]]) for l in range(U.L)]


def window_moments(st, W, parts=False):
    """S (L, W, W) and n_w from the per-unit dicts; ``parts=True``: (mean part, covariance part, n_w) instead."""
    L = st[0]["unit"].L
    Sm, Sc, n_w = np.zeros((L, W, W)), np.zeros((L, W, W)), 0
    for s in st:
        starts = window_starts(s["mu"].shape[0], W)
        n_w += len(starts)
        for l, (m, G, Sig) in enumerate(latent_blocks(s)):
            for s0 in starts:
                Sm[l] += np.outer(m[s0:s0 + W], m[s0:s0 + W])
                Sc[l] += G[s0:s0 + W] @ Sig @ G[s0:s0 + W].T
    return (Sm, Sc, n_w) if parts else (Sm + Sc, n_w)


def objective(logp, S_l, n_w, dt=1.0):
    """(ll, dll (3)) of one latent at logp = log(sigma^2, omega, gp_noise); (-inf, 0) where K does not factor."""
    sig2, om, eps = np.exp(np.asarray(logp, float))
    W = S_l.shape[0]
    t = np.arange(W) * dt
    D2 = (t[:, None] - t[None, :]) ** 2
    K0 = sig2 * np.exp(-om * D2)
    try:
        Lc = np.linalg.cholesky(K0 + eps * np.eye(W))
    except np.linalg.LinAlgError:
        return -np.inf, np.zeros(3)
    Kinv = cho_solve((Lc, True), np.eye(W))
    KS = cho_solve((Lc, True), S_l)
    ll = -0.5 * np.trace(KS) - n_w * np.sum(np.log(np.diag(Lc)))
    A = KS @ Kinv - n_w * Kinv
    dll = np.zeros(3)
    dll[1] = 0.5 * np.sum(A * (-om * D2 * K0))
    return float(ll), dll


def hstep(S, n_w, sigma, omega, gp_noise, omega_bound, dt=1.0):
    """(sigma, omega, fun (L), nit (L)): oracle.hstep_arrays with ``objective``."""
    sigma, omega = np.array(sigma, float), np.array(omega, float)
    fun, nit = np.zeros(omega.size), np.zeros(omega.size, int)
    bounds = np.log(np.array([(1e-3, 1.0), tuple(omega_bound), (gp_noise / 2, gp_noise * 2)]))
    for l in range(omega.size):
        start = np.log(np.array([sigma[l] ** 2, omega[l], gp_noise]))

        def neg(logp, l=l):
            ll, dll = objective(logp, S[l], n_w, dt)
            return -ll, -dll

        res = minimize(neg, start, jac=True, bounds=bounds)
        sig2, om, _ = np.exp(res.x)
        if not np.any(np.isclose(om, omega_bound)):
            omega[l] = om
        sigma[l] = math.sqrt(sig2)
        fun[l], nit[l] = -res.fun, res.nit
    return sigma, omega, fun, nit


def build_prior(lengths, omega, sigma, rank):
    """{T: (L, T, rank)}: oracle.ichol_gauss per latent, scaled by sigma."""
    return {int(T): np.stack([O.ichol_gauss(int(T), omega[l], rank) * sigma[l] for l in range(len(omega))])
            for T in sorted(set(int(T) for T in lengths))}


def refit_hstep(units, a, b, noise, gauss, prior, omega, sigma, rank, gp_noise, omega_bound, window, m_iter, dt=1.0,
                missing=None, max_iter=20, tol=1e-6, newton_tol=1e-20, trace_hook=None, omega_hook=None, **m_kw):
    """joint_em_numpy.refit (``missing`` per unit: refit_masked) with the hyperparameter step after the M-step.  The dict
    of that loop plus ``omega``, ``sigma``, ``prior`` (those of the returned parameters) and ``trace["omega"]``.
    ``omega_hook(k, omega)`` may replace the omega that iteration k runs on, after the optimiser found it and before the
    factors are built (the device test pins the loop to the device's own omega with it: L-BFGS-B at SciPy's default
    tolerances is not a continuous function of the moments' last bits, see tests/test_gpu_joint_hstep.py)."""
    N = a.shape[1]
    lengths = [u["y"].shape[0] for u in units]
    if n_windows(lengths, window) == 0:
        raise ValueError("no unit as long as the window")
    y, x = EM.cat_units(units, N)
    held = None if missing is None else np.concatenate([np.asarray(m, bool) for m in missing])
    # (parameters: a, b, noise, da, db, omega, sigma, prior)
    cur = (np.array(a, float), np.array(b, float), np.array(noise, float), None, None, np.array(omega, float),
           np.array(sigma, float), prior)
    trace = {"laplace": [], "n_newton": [], "converged": [], "omega": []}
    prev, k = None, 0
    while True:
        st = JC.statement(units, cur[0], cur[1], cur[2], gauss, cur[7], tol=newton_tol, held=held)
        mu, cov = np.concatenate([s["mu"] for s in st]), np.concatenate([s["cov"] for s in st])
        ev = float(sum(s["laplace"] for s in st))
        if trace_hook is not None:
            ev = float(trace_hook(k, ev))
        trace["laplace"].append(ev)
        trace["n_newton"].append(max(int(s["n_newton"]) for s in st))
        trace["converged"].append(all(bool(s["converged"]) for s in st))
        trace["omega"].append(cur[5].copy())
        kept = k
        if prev is not None and ev - prev[4] <= tol * abs(ev):
            if not ev >= prev[4]:
                cur, st, mu, cov = prev[:4]
                kept = k - 1
            break
        if k == max_iter:
            break
        prev = (cur, st, mu, cov, ev)
        if missing is None:
            out = EM.mstep_cov(y, x, mu, cov, cur[0], cur[1], gauss, m_iter, **m_kw)
        else:
            out = EMM.mstep_cov_masked(y, x, mu, cov, cur[0], cur[1], held, m_iter, noise=cur[2], **m_kw)
        S, n_w = window_moments(st, window)
        sg, om, _, _ = hstep(S, n_w, cur[6], cur[5], gp_noise, omega_bound, dt)
        if omega_hook is not None:
            om = np.array(omega_hook(k + 1, om), float)
        cur = (out[0], out[1], out[4], out[2], out[3], om, sg, build_prior(lengths, om, sg, rank))
        k += 1
    return {"a": cur[0], "b": cur[1], "noise": cur[2], "da": cur[3], "db": cur[4], "omega": cur[5], "sigma": cur[6],
            "prior": cur[7], "mu": mu, "cov": cov, "post": st, "trace": trace, "kept": kept}
