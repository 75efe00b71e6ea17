"""The lag moments of vlgp_amd/evaluation.py (vlgp_lag_moments) stated in NumPy, and the summary built on them
(tests/test_lag_host.py, tests/test_gpu_lag.py).  Dense, one unit at a time.

One unit (a trial, or a window of a tiling cut) of T rows, lags k = 0 ... K, prior factors G_l (T, R) (columns past the
effective rank are zero and change nothing):
  seen_tn: the entries the posterior was inferred from -- every entry of a plain set, the entries a masked replica does
           NOT hold out;  live_tn: the entries that are scored -- every entry of a plain set, the held-out ones of a replica
  rate_tn = exp(min(eta_tn + 1/2 sum_l a_ln^2 v_tl, 10)),  eta = a_n . mu_t + x_tn . b_n   (the v term dropped when vb == 0)
  w_tl = sum_{n seen at t} a_ln^2 (rate_tn Poisson, 1 / noise_n Gaussian)                     update_w's formula
  H_l = I + G_l' diag(w_.l) G_l = Lc Lc',  u_t = Lc^-1 G_l[t]',  c_l(t, s) = u_t . u_s          (c == 0 when vb == 0)
  q_n(t, s) = sum_l a_ln^2 c_l(t, s)
  m, e, d = y - e as pair_numpy.row_terms has them under C_t = diag(v_t): the predictive mean uses the STORED v
  resid[k, n] = sum d_tn d_{t+k,n},  model[k, n] = sum s_tn s_{t+k,n} f(q_n(t, t+k)),  count[k, n] = the pairs summed,
  over the t with t + k inside the same unit and both entries live; s = e, f = expm1 Poisson; s = 1, f = identity
  Gaussian; at k = 0 model += e_tn Poisson, noise_n Gaussian.
live enters by selection: what y holds at an entry that is not live is never read into arithmetic.  A unit one of whose
H_l has no Cholesky factor (or is not finite) adds nothing to any sum; n_failed counts such (unit, latent) pairs."""
import numpy as np


def weights(x, mu, v, a, b, noise, gauss, seen, vb=True):
    """``w`` (T, L) of one unit recomputed from its ``mu, v`` over the entries ``seen`` (T, N) bool."""
    gauss = np.asarray(gauss, dtype=bool)
    asq = a ** 2
    eta = mu @ a + (np.einsum("tpn,pn->tn", x, b) if x is not None else b[0][None, :])
    rate = np.exp(np.minimum(eta + (0.5 * (v @ asq) if vb else 0.0), 10.0))
    curv = np.where(gauss, 1.0 / np.where(gauss, noise, 1.0), rate)
    return np.where(seen, curv, 0.0) @ asq.T


def cross_factor(G, w):
    """``u`` (T, R) with ``c(t, s) = u_t . u_s`` for one latent: G (T, R), w (T).  None when H has no factor."""
    H = np.eye(G.shape[1]) + G.T @ (w[:, None] * G)
    if not np.isfinite(H).all():
        return None
    try:
        Lc = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(Lc, G.T).T


def row_terms(y, x, mu, v, a, b, noise, gauss, vb=True):
    """``(d, e, s)`` (T, N each): residual, predictive mean and scale under the stored ``v`` (0 when vb == 0)."""
    gauss = np.asarray(gauss, dtype=bool)
    m = mu @ a + (np.einsum("tpn,pn->tn", x, b) if x is not None else b[0][None, :])
    s2 = (v @ a ** 2) if vb else np.zeros_like(m)
    lam = np.exp(np.minimum(m + 0.5 * np.maximum(s2, 0.0), 10.0))
    e = np.where(gauss, m, lam)
    with np.errstate(invalid="ignore"):
        d = y - e
    return d, e, np.where(gauss, 1.0, lam)


def unit_moments(unit, par, G, max_lag, vb=True, live=None, seen=None):
    """``(resid, model, count, n_bad)`` of one unit: (K + 1, N) each and the latents whose H could not be factored
    (then the three are zero).  unit: y, x (or None), mu, v; G (L, T, R); live, seen (T, N) bool."""
    a, b, noise, gauss = par["a"], par["b"], par["noise"], np.asarray(par["gauss"], dtype=bool)
    y, x, mu, v = unit["y"], unit.get("x"), unit["mu"], unit["v"]
    T, N = y.shape
    L, K = a.shape[0], int(max_lag)
    live = np.ones((T, N), dtype=bool) if live is None else np.asarray(live, dtype=bool)
    seen = np.ones((T, N), dtype=bool) if seen is None else np.asarray(seen, dtype=bool)
    resid, model, count = (np.zeros((K + 1, N)) for _ in range(3))
    c, asq = np.zeros((L, T, T)), a ** 2
    if vb:
        w = weights(x, mu, v, a, b, noise, gauss, seen, vb)
        us = [cross_factor(G[l][:T], w[:, l]) for l in range(L)]
        n_bad = sum(u is None for u in us)
        if n_bad:
            return resid, model, count, n_bad
        c = np.stack([u @ u.T for u in us])
    d, e, s = row_terms(y, x, mu, v, a, b, noise, gauss, vb)
    ex = np.where(gauss, noise, e)
    for k in range(min(K, T - 1) + 1):
        for t in range(T - k):
            both = live[t] & live[t + k]
            qk = c[:, t, t + k] @ asq
            f = np.where(gauss, qk, np.expm1(qk))
            term = s[t] * s[t + k] * f + (ex[t] if k == 0 else 0.0)
            with np.errstate(invalid="ignore"):
                dd = d[t] * d[t + k]
            resid[k] += np.where(both, dd, 0.0)
            model[k] += np.where(both, term, 0.0)
            count[k] += both
    return resid, model, count, 0


def lag_moments(units, par, prior, max_lag, vb=True, live=None, seen=None):
    """``(resid, model, count, n_failed)`` over the units in order.  prior: ``{T: G (L, T, R)}``; live, seen: one (T, N)
    bool array per unit, or None (every entry; ``seen`` defaults to the complement of a given ``live``)."""
    N, K = par["a"].shape[1], int(max_lag)
    resid, model, count = (np.zeros((K + 1, N)) for _ in range(3))
    n_failed = 0
    for i, un in enumerate(units):
        lv = None if live is None else live[i]
        sn = seen[i] if seen is not None else (None if lv is None else ~np.asarray(lv, dtype=bool))
        r, m, c, bad = unit_moments(un, par, prior[un["y"].shape[0]], K, vb, lv, sn)
        resid, model, count, n_failed = resid + r, model + m, count + c, n_failed + bad
    return resid, model, count, n_failed


def summary(resid, model, count):
    """The composition of evaluation._lag_summary, restated entry by entry: a dict of the same keys."""
    K1, N = resid.shape
    out = {k: np.full((K1, N), np.nan) for k in ("residual_acf", "model_acf", "excess_acf", "se_null")}
    out["dispersion"], out["rms_excess"] = np.full(N, np.nan), np.full(N, np.nan)
    every = []
    for n in range(N):
        if not count[0, n] > 0:
            continue
        var = model[0, n] / count[0, n]
        if model[0, n] > 0:
            out["dispersion"][n] = resid[0, n] / model[0, n]
        for k in range(K1):
            if count[k, n] > 0:
                out["se_null"][k, n] = 1.0 / np.sqrt(count[k, n])
                if var > 0:
                    out["residual_acf"][k, n] = resid[k, n] / count[k, n] / var
                    out["model_acf"][k, n] = model[k, n] / count[k, n] / var
                    out["excess_acf"][k, n] = out["residual_acf"][k, n] - out["model_acf"][k, n]
        ex = out["excess_acf"][1:, n]
        ex = ex[np.isfinite(ex)]
        if ex.size:
            out["rms_excess"][n] = np.sqrt(np.mean(ex ** 2))
            every.extend(ex)
    out["n_scored"] = len(every)
    out["rms_excess_all"] = float(np.sqrt(np.mean(np.square(every)))) if every else float("nan")
    scored = count > 0
    out["resid"], out["model"], out["count"] = (np.where(scored, x, np.nan) for x in (resid, model, count))
    return out
