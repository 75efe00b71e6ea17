"""The H-step objective of one latent, term by term, in plain NumPy at extended precision.

For log-parameters (sigma^2, omega, eps) and a window of T bins of width dt, with K = sigma^2 exp(-omega D^2) + eps I,
dK = dK / dln(omega) and, per segment i, S_i = diag sqrt(w_i), A_i = I + S_i K S_i (csrc/hstep_lr.h's header,
tools/lr_proto.py: seg_terms_dense):

    K block       logdet = log det K,  tr_kic = tr(K^-1 C),  tr_q = tr(K^-1 dK K^-1 C),  C = sum_i mu_i mu_i'
    per segment   tr_i = tr(A_i^-1),   cs_i = sum_jk s_j s_k dK_jk (A_i^-1)_jk
    assembled as hstep_round_finish does:
                  ll  = -1/2 tr_kic - 1/2 sum_i tr_i - M / 2 logdet
                  dll =  1/2 (tr_q - sum_i cs_i)

which is gp.obj_func's (ll, dll[1]) (oracle.gp_objective) since tr(K^-1 S_i) = tr(A_i^-1) and
tr(K^-1 S_i K^-1 dK) = tr(K^-1 dK) - cs_i.  A set that repeats a few distinct segments is priced once per distinct segment
(`counts`).  Everything runs in numpy.longdouble (64-bit mantissa on x86-64) with a Cholesky written out here, because LAPACK
has no such type; tests/test_hstep_host.py holds it to oracle.gp_objective and to 40-digit mpmath.
"""
import numpy as np

LD = np.longdouble


def se_kernel(T, dt, logp):
    """K (jitter on the diagonal) and dK / dln(omega), longdouble."""
    sigmasq, omega, eps = (np.exp(LD(x)) for x in np.asarray(logp, dtype=float))
    t = np.arange(T).astype(LD) * LD(dt)
    d2 = (t[:, None] - t[None, :]) ** 2
    ks = sigmasq * np.exp(-omega * d2)
    return ks + eps * np.eye(T, dtype=LD), -omega * d2 * ks


def chol_inverse(a):
    """(A^-1, log det A) of a symmetric positive definite longdouble matrix through its Cholesky factor."""
    n = a.shape[0]
    l = np.array(a, dtype=LD)
    for k in range(n):  # right-looking, one rank-1 update of the trailing block per column
        if not l[k, k] > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % k)
        l[k, k] = np.sqrt(l[k, k])
        l[k + 1:, k] /= l[k, k]
        l[k + 1:, k + 1:] -= np.outer(l[k + 1:, k], l[k + 1:, k])
    l = np.tril(l)
    x = np.eye(n, dtype=LD)  # X = L^-1 by forward substitution, all columns at once
    for i in range(n):
        x[i] = (x[i] - l[i, :i] @ x[:i]) / l[i, i]
    return x.T @ x, 2 * np.log(np.diag(l)).sum()


def k_terms(logp, T, dt, c, mu=None):
    """(logdet, tr_kic, tr_q) of the K block for the second-moment matrix c = sum_i mu_i mu_i'; with mu (D, T) also the
    shares of its rows, quad_i = mu_i' K^-1 mu_i and gq_i = alpha_i' dK alpha_i, alpha_i = K^-1 mu_i."""
    k, dk = se_kernel(T, dt, logp)
    ki, logdet = chol_inverse(k)
    out = (logdet, (ki * c).sum(), ((ki @ dk @ ki) * c).sum())
    if mu is None:
        return out
    al = mu @ ki
    return out + ((al * mu).sum(1), ((al @ dk) * al).sum(1))


def seg_terms(logp, T, dt, w):
    """(tr, cs) per row of w, shape (D, T): the per-segment terms, which do not depend on mu."""
    k, dk = se_kernel(T, dt, logp)
    tr, cs = [], []
    for wi in np.atleast_2d(w):
        s = np.sqrt(np.asarray(wi, dtype=float).astype(LD))
        if not s.any():  # A = I
            tr.append(LD(T))
            cs.append(LD(0))
            continue
        ss = s[:, None] * s[None, :]
        ai, _ = chol_inverse(np.eye(T, dtype=LD) + ss * k)
        tr.append(np.trace(ai))
        cs.append((ss * dk * ai).sum())
    return np.array(tr, dtype=LD), np.array(cs, dtype=LD)


def evaluate(logp, T, dt, mu, w, counts=None):
    """One evaluation over a set of segments of one latent.  mu, w: (D, T), one row per DISTINCT segment; counts: how often
    each occurs in the set (default: once).  Returns a dict of the terms above, of the segments' shares quad_i, gq_i of
    tr_kic, tr_q (all longdouble) and of ll, dll (float)."""
    mu = np.atleast_2d(np.asarray(mu, dtype=float)).astype(LD)
    w = np.atleast_2d(np.asarray(w, dtype=float))
    n = np.ones(len(mu), dtype=LD) if counts is None else np.asarray(counts).astype(LD)
    c = (mu * n[:, None]).T @ mu
    logdet, tr_kic, tr_q, quad, gq = k_terms(logp, T, dt, c, mu)
    tr, cs = seg_terms(logp, T, dt, w)
    m = n.sum()
    ll = -0.5 * tr_kic - 0.5 * (n * tr).sum() - 0.5 * m * logdet
    dll = 0.5 * (tr_q - (n * cs).sum())
    return dict(logdet=logdet, tr_kic=tr_kic, tr_q=tr_q, quad=quad, gq=gq, tr=tr, cs=cs, counts=n, ll=float(ll), dll=float(dll))


def objective(logp, T, dt, mu, w, counts=None):
    r = evaluate(logp, T, dt, mu, w, counts)
    return r["ll"], r["dll"]
