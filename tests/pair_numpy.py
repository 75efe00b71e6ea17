"""The pair moments of vlgp_amd/evaluation.py (vlgp_pair_moments, vlgp_pair_moments_cov) stated in NumPy, and the
summaries built on them (tests/test_pair_host.py, tests/test_gpu_pair.py).  One row at a time would be the definition;
the arrays below are that, vectorised over the rows.

Row t has the posterior N(mu_t, C_t) of its latents; c_t[n, m] = a_n' C_t a_m.
  m_tn = a_n . mu_t + x_tn . b_n,  s2_tn = c_t[n, n]
  e_tn = exp(min(m + max(0, s2) / 2, 10)) Poisson (the rate of vlgp_predictive / vlgp_predictive_cov), m Gaussian
  s_tn = e_tn Poisson, 1 Gaussian;  f = expm1 when both channels are Poisson, else the identity
  K_t[n, m] = s_tn s_tm f(c_t[n, m]);  K_t[n, n] += e_tn Poisson, noise_n Gaussian;  d_tn = y_tn - e_tn
  resid[n, m] = sum_t live_tn live_tm d_tn d_tm,  model[n, m] = sum_t live_tn live_tm K_t[n, m]
live enters by selection: what y holds at an entry that is not live is never multiplied."""
import numpy as np


def diag_cov(v):
    """(rows, L) variances -> (rows, L, L) diagonal covariances."""
    v = np.asarray(v, dtype=float)
    out = np.zeros(v.shape + (v.shape[1],))
    idx = np.arange(v.shape[1])
    out[:, idx, idx] = v
    return out


def dead_rows(mu, cov):
    """The rule of a supplied posterior: a row whose mu or cov holds a non-finite value is dead for all channels."""
    return ~(np.isfinite(mu).all(axis=1) & np.isfinite(cov.reshape(len(mu), -1)).all(axis=1))


def row_terms(y, x, mu, cov, a, b, noise, gauss):
    """``(d (T, N), K (T, N, N))`` of rows with finite moments: residuals and predictive covariances."""
    gauss = np.asarray(gauss, dtype=bool)
    m = mu @ a + (np.einsum("tpn,pn->tn", x, b) if x is not None else b[0][None, :])
    c = a.T @ (cov @ a)  # (T, N, N): c[t, n, m] = a_n' C_t a_m
    s2 = np.einsum("tnn->tn", c)
    lam = np.exp(np.minimum(m + 0.5 * np.maximum(s2, 0.0), 10.0))
    e = np.where(gauss, m, lam)
    s = np.where(gauss, 1.0, lam)
    both = ~gauss[:, None] & ~gauss[None, :]
    K = s[:, :, None] * s[:, None, :] * np.where(both, np.expm1(c), c)
    idx = np.arange(len(gauss))
    K[:, idx, idx] += np.where(gauss, noise, lam)
    with np.errstate(invalid="ignore"):
        d = y - e
    return d, K


def pair_sums(d, K, live):
    """``(resid, model)``, (N, N) each, over the rows of d (T, N), K (T, N, N) with live (T, N) bool."""
    dl = np.where(live, d, 0.0)
    both = live[:, :, None] & live[:, None, :]
    return dl.T @ dl, np.where(both, K, 0.0).sum(axis=0)


def pair_moments(y, x, mu, cov, a, b, noise, gauss, live=None):
    """``(resid, model, count)`` of concatenated rows: y (T, N), x (T, P, N) or None (x == 1), mu (T, L), cov (T, L, L), live
    (T, N) bool (default: every entry).  Dead rows (``dead_rows``) add nothing and are not counted."""
    T, N = y.shape
    live = np.ones((T, N), dtype=bool) if live is None else np.asarray(live, dtype=bool)
    keep = ~dead_rows(mu, cov)
    live = live & keep[:, None]
    d, K = np.zeros((T, N)), np.zeros((T, N, N))
    d[keep], K[keep] = row_terms(y[keep], None if x is None else x[keep], mu[keep], cov[keep], a, b, noise, gauss)
    resid, model = pair_sums(d, K, live)
    lf = live.astype(float)
    return resid, model, lf.T @ lf


def summary(resid, model, count):
    """The composition of evaluation._pair_summary, restated: a dict of the same keys."""
    N = resid.shape[0]
    scored = np.nan_to_num(count, nan=0.0) > 0
    R, Mo, Cn = (np.where(scored, x, np.nan) for x in (resid, model, count))
    out = {"resid": R, "model": Mo, "count": Cn}
    corr_r, corr_m = np.full((N, N), np.nan), np.full((N, N), np.nan)
    for n in range(N):
        for m in range(N):
            vv = Mo[n, n] * Mo[m, m]
            if scored[n, m] and vv > 0:
                corr_r[n, m], corr_m[n, m] = R[n, m] / np.sqrt(vv), Mo[n, m] / np.sqrt(vv)
    out["residual_corr"], out["model_corr"], out["excess_corr"] = corr_r, corr_m, corr_r - corr_m
    with np.errstate(divide="ignore", invalid="ignore"):
        out["se_null"] = 1.0 / np.sqrt(Cn)
        out["dispersion"] = np.array([R[n, n] / Mo[n, n] if Mo[n, n] > 0 else np.nan for n in range(N)])
    low = np.array([out["excess_corr"][n, m] for n in range(N) for m in range(n)])
    low = low[np.isfinite(low)]
    out["n_pairs"] = int(low.size)
    out["rms_excess"] = float(np.sqrt(np.mean(low ** 2))) if low.size else float("nan")
    out["mean_excess"] = float(np.mean(low)) if low.size else float("nan")
    return out
