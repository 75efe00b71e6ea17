"""NumPy restatement of the fit with missing observations (tests/test_masked_fit_host.py, tests/test_gpu_masked_fit.py).

No new arithmetic for the M-step: the update of channel n IS the pinned oracle's ``O.mstep_arrays`` called on that
channel's observed rows with N = 1, channel by channel.  The E-step is ``speckled_numpy.estep_masked`` (the oracle's
sweep with the working residual and the curvature multiplied by the mask of observed entries) from a warm start.  The EM
loop and the fit from a given initialisation compose them with the oracle's ``constrain_loading``, ``constrain_latent``,
``hstep`` and ``cut_trials``, in the order of ``O.vem`` / ``O.fit_given_init``.  ``missing`` is True where y is absent."""
import numpy as np
import scipy.linalg as sla

from oracle import vlgp_oracle as O


def mstep_masked(y, x, mu, v, a, b, missing, n_iter, noise=None, **kw):
    """(a, b, da, db, noise) after ``n_iter`` Newton iterations with every channel on its observed rows only.  A
    channel without an observed row keeps a, b and noise; its steps are 0.  ``kw``: ``O.mstep_arrays``'s options."""
    L, N = a.shape
    noise = np.ones(N) if noise is None else np.asarray(noise, dtype=float)
    out = [np.array(a, dtype=float), np.array(b, dtype=float), np.zeros_like(a), np.zeros_like(b),
           np.array(noise, dtype=float)]
    if n_iter < 1:
        return tuple(out)
    pois = np.zeros(1, dtype=bool)
    for n in range(N):
        rows = ~missing[:, n]
        if not rows.any():
            continue
        got = O.mstep_arrays(y[rows, n:n + 1], x[rows][:, :, n:n + 1], mu[rows], v[rows], a[:, n:n + 1], b[:, n:n + 1],
                             pois, n_iter, noise=noise[n:n + 1], **kw)
        for dst, val in zip(out[:4], got[:4]):
            dst[:, n] = val[:, 0]
        out[4][n] = got[4][0]
    return tuple(out)


def estep_masked_warm(y, x, mu, v, w, a, b, noise, gauss, G, observed, n_iter, dmu_bound=5.0, vb=True):
    """``speckled_numpy.estep_masked`` from the given ``mu, v, w`` (not modified).  y is read at observed entries only:
    what it holds elsewhere (NaN) meets a select, not a product.  Returns (mu, v, w, dmu, n_failed)."""
    obs = np.asarray(observed, dtype=bool)
    y = np.where(obs, np.asarray(y, dtype=float), 0.0)
    mu, v, w = (np.array(arr, dtype=float) for arr in (mu, v, w))
    T, L = mu.shape
    dmu = np.zeros((T, L))
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
        res = np.where(obs, res, 0.0)
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
        w = curvature_masked(x, mu, v, a, b, noise, gauss, obs)
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


def curvature_masked(x, mu, v, a, b, noise, gauss, observed):
    """``O.curvature_unit`` over the observed channels of every row."""
    asq = a ** 2
    eta = O.linear_predictor(x, mu, a, b)
    rate = O.capped_exp(eta + 0.5 * (v @ asq))
    curv = np.where(gauss, 1.0 / np.where(gauss, noise, 1.0), rate)
    return np.where(observed, curv, 0.0) @ asq.T


def update_w(trials, params, config=None):
    g = O._gauss_mask(params)
    for tr in trials:
        tr["w"] = curvature_masked(tr["x"], tr["mu"], tr["v"], params["a"], params["b"], params["noise"], g, ~tr["missing"])


def estep(trials, params, config):
    g = O._gauss_mask(params)
    if config["Eniter"] < 1:
        return
    for tr in trials:
        mu, v, w, dmu, _ = estep_masked_warm(tr["y"], tr["x"], tr["mu"], tr["v"], tr["w"], params["a"], params["b"],
                                             params["noise"], g, params["cholesky"][tr["y"].shape[0]], ~tr["missing"],
                                             config["Eniter"], config["dmu_bound"], config["method"] == "VB")
        tr["mu"][...] = mu
        tr["v"][...] = v
        tr["dmu"][...] = dmu
        tr["w"] = w


def mstep(trials, params, config):
    if config["Mniter"] < 1:
        return
    cat = lambda k: np.concatenate([tr[k] for tr in trials], axis=0)  # noqa: E731
    a, b, da, db, noise = mstep_masked(cat("y"), cat("x"), cat("mu"), cat("v"), params["a"], params["b"], cat("missing"),
                                       config["Mniter"], noise=params["noise"], use_hessian=config["use_hessian"],
                                       eps=config["eps"], learning_rate=config["learning_rate"],
                                       da_bound=config["da_bound"], db_bound=config["db_bound"])
    params["a"][...] = a
    params["b"][...] = b
    params["da"][...] = da
    params["db"][...] = db
    params["noise"] = noise


def vem(trials, params, config):
    """``O.vem`` with the masked E- and M-step: same order, same stopping rule."""
    for it in range(config["max_iter"]):
        n_mu = sla.norm(np.concatenate([tr["mu"] for tr in trials], axis=0))
        n_a, n_b = sla.norm(params["a"]), sla.norm(params["b"])
        O.constrain_loading(trials, params, config)
        estep(trials, params, config)
        O.constrain_latent(trials, params, config)
        mstep(trials, params, config)
        O.hstep(trials, params, config)
        n_dmu = sla.norm(np.concatenate([tr["dmu"] for tr in trials], axis=0))
        tol = config["tol"]
        done = n_dmu < tol * n_mu and sla.norm(params["da"]) < tol * n_a and sla.norm(params["db"]) < tol * n_b
        if done and it + 1 >= config["min_iter"]:
            break


def infer(trials, params, config):
    keep = config["Eniter"]
    config["Eniter"] = config["max_iter"]
    try:
        estep(trials, params, config)
    finally:
        config["Eniter"] = keep


def fit_given_init(trials, missing, params, config):
    """``O.fit_given_init`` with missing observations: every trial holds y, x, mu; params holds a, b, noise.  Trial
    lengths are multiples of the window, so the segments (views, ``O.cut_trials``) tile the trials."""
    window = config["window"]
    params.setdefault("da", np.zeros_like(params["a"]))
    params.setdefault("db", np.zeros_like(params["b"]))
    for tr, m in zip(trials, missing):
        assert not window or tr["y"].shape[0] % window == 0
        tr["missing"] = np.asarray(m, dtype=bool)
    O.fill_trials(trials)
    O.make_cholesky(trials, params, config)
    update_w(trials, params, config)
    O.update_v(trials, params, config)
    segs = O.cut_trials(trials, window)
    if window:
        masks = [tr["missing"][s:s + window] for tr in trials for s in range(0, tr["y"].shape[0], window)]
        for sg, m in zip(segs, masks):
            sg["missing"] = m
    O.make_cholesky(segs, params, config)
    O.fill_trials(segs)
    vem(segs, params, config)
    O.make_cholesky(trials, params, config)
    update_w(trials, params, config)
    O.update_v(trials, params, config)
    infer(trials, params, config)
    return {"trials": trials, "params": params, "config": config}


def random_missing(trials, fraction, seed):
    """One bool (T, N) array per trial, True with probability ``fraction``, seeded."""
    rng = np.random.default_rng(seed)
    return [rng.random(tr["y"].shape) < fraction for tr in trials]


def heldout_bits_per_spike(trials, missing, params, vb=True):
    """Score of the fitted rate at the missing entries against the per-channel constant-rate null (the channel's mean
    over its OBSERVED entries), in bits per spike over the missing entries of all channels."""
    from heldout_numpy import rate_ll

    gauss = O._gauss_mask(params)
    y = np.concatenate([tr["y"] for tr in trials])
    M = np.concatenate(missing)
    ll = np.concatenate([rate_ll(tr["y"], tr["x"], tr["mu"], tr["v"], params["a"], params["b"], params["noise"], gauss,
                                 vb)[1] for tr in trials])
    null_rate = np.where(M, 0.0, y).sum(axis=0) / (~M).sum(axis=0)
    from scipy.special import gammaln

    ll_null = y * np.log(null_rate)[None, :] - null_rate[None, :] - gammaln(y + 1.0)
    spikes = y[M].sum()
    return float((ll[M].sum() - ll_null[M].sum()) / (spikes * np.log(2.0)))
