"""NumPy restatement of the speckled hold-out (tests/test_speckled_host.py, tests/test_gpu_speckled.py): the oracle's
E-step (oracle.vlgp_oracle.estep_unit) from a zero start with the working residual and the curvature multiplied by the
mask of observed entries, then every held-out entry predicted and scored with the definitions of vlgp_amd/evaluation.py."""
import numpy as np

from heldout_numpy import rate_ll
from oracle import vlgp_oracle as O


def estep_masked(y, x, a, b, noise, gauss, G, observed, n_iter, dmu_bound=5.0, vb=True, start=None):
    """``n_iter`` sweeps of estep_unit from mu = v = w = 0 (or from ``start``, a (mu, v, w) triple that is left alone) with
    the likelihood terms of the entries where ``observed`` (T, N) is False removed: res and U are 0 there.  Returns
    (mu, v, w, dmu, n_failed)."""
    y = np.asarray(y, dtype=float)
    obs = np.asarray(observed, dtype=float)
    T, L = y.shape[0], a.shape[0]
    mu, v, w, dmu = (np.zeros((T, L)) for _ in range(4))
    if start is not None:
        mu, v, w = (np.array(s, dtype=float) for s in start)
    eye = np.eye(G.shape[-1])
    pois = ~gauss
    asq = a ** 2
    xb = np.einsum("tpn,pn->tn", x, b)
    gnoise = noise[gauss]
    n_failed = 0
    for _ in range(n_iter):
        eta = mu @ a + xb
        rate = O.capped_exp(eta + 0.5 * (v @ asq))
        res = np.empty_like(y)
        res[:, pois] = y[:, pois] - rate[:, pois]
        res[:, gauss] = (y[:, gauss] - eta[:, gauss]) / gnoise
        res *= obs
        for l in range(L):
            Gl = G[l]
            WG = w[:, l:l + 1] * Gl
            H = Gl.T @ WG
            u = Gl @ (Gl.T @ (res @ a[l])) - mu[:, l]
            try:
                rhs = WG.T @ u
                sol = O._spd_solve(eye + H, rhs)
                step = u - Gl @ rhs + Gl @ (H @ sol)
                np.clip(step, -dmu_bound, dmu_bound, out=step)
            except Exception:
                step = np.zeros(T)
                n_failed += 1
            dmu[:, l] = step
            mu[:, l] += step
        eta = mu @ a + xb
        rate = O.capped_exp(eta + 0.5 * (v @ asq))
        curv = np.empty_like(y)
        curv[:, pois] = rate[:, pois]
        curv[:, gauss] = 1.0 / gnoise
        curv *= obs
        w = curv @ asq.T
        if vb:
            for l in range(L):
                Gl = G[l]
                H = Gl.T @ (w[:, l:l + 1] * Gl)
                try:
                    sol = O._spd_solve(eye + H, H)
                    v[:, l] = np.sum(Gl * (Gl - Gl @ H + Gl @ (H @ sol)), axis=1)
                except Exception:
                    n_failed += 1
    return mu, v, w, dmu, n_failed


def restated(trials, params, config, held, n_iter=None):
    """``held``: bool (n_rep, rows, N) over the concatenated rows.  Returns the posterior ``mu, v, w`` (n_rep, rows, L),
    ``rate`` (rows, N) at the held-out entries (NaN elsewhere; the last replica that holds an entry out writes it),
    ``ll`` (n_rep, N) summed over each replica's held-out entries, and the number of failed solves."""
    a, b, noise = params["a"], params["b"], params["noise"]
    L = params["zdim"]
    gauss = np.asarray(params["likelihood"]) == "gaussian"
    vb = config["method"] == "VB"
    n_iter = config["max_iter"] if n_iter is None else n_iter
    rows = sum(tr["y"].shape[0] for tr in trials)
    n_rep, N = held.shape[0], held.shape[2]
    post = {k: np.zeros((n_rep, rows, L)) for k in ("mu", "v", "w")}
    rate = np.full((rows, N), np.nan)
    ll = np.zeros((n_rep, N))
    bad, r0 = 0, 0
    for tr in trials:
        T = tr["y"].shape[0]
        G = O.build_prior([T], params["omega"], params["sigma"], 50)[T]
        for k in range(n_rep):
            out = held[k, r0:r0 + T]
            mu, v, w, _, nf = estep_masked(tr["y"], tr["x"], a, b, noise, gauss, G, ~out, n_iter, config["dmu_bound"], vb)
            bad += nf
            post["mu"][k, r0:r0 + T], post["v"][k, r0:r0 + T], post["w"][k, r0:r0 + T] = mu, v, w
            r, l_ = rate_ll(tr["y"], tr["x"], mu, v, a, b, noise, gauss, vb)
            rate[r0:r0 + T][out] = r[out]
            ll[k] += np.where(out, l_, 0.0).sum(axis=0)
        r0 += T
    return post, rate, ll, bad
