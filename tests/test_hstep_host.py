"""tests/hstep_numpy.py, the reference of tests/test_gpu_hstep_shapes.py, held to two references of its own (no GPU):
oracle.gp_objective (gp.obj_func restated with LAPACK) and 40-digit mpmath.

The helper is used at 1e-9 on |ll| and on max(|dll|, 1e-3 |ll|) (1e-8 on the latter above 64 bins), so its own error has
to stay below 1e-10: REF_TOL.  oracle.gp_objective was measured against 40-digit arithmetic at 1e-14 ... 9e-13 (ll) and
6e-14 ... 1.3e-11 (dll) for eps in 1e-4 ... 1e-3 and 7.5e-11 at eps = 1e-6, so the comparison with it runs at
eps >= 1e-4 and at 1e-10 as well; the mpmath subset takes both ends of every parameter range the shape cases use
(sigma^2 0.05 ... 20, eps 1e-5 ... 1e-2, omega from a rank-4 kernel to 0.5, w = 0 and 1e6 among 10^U(-3, 2)).
"""
import numpy as np
import pytest

import hstep_numpy as H
from oracle import vlgp_oracle as O

REF_TOL = 1e-10  # a tenth of the tolerance the helper is used at


def _set(seed, T, D, extreme=False):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((D, T))
    w = 10.0 ** rng.uniform(-3, 2, (D, T))
    if extreme:
        w[0] = 0.0
        w[-1, rng.choice(T, min(3, T), replace=False)] = 1e6
    return mu, w


def _close(got, want, tag):
    ll, dll = got
    wl, wd = want
    assert abs(ll - wl) <= REF_TOL * abs(wl), (tag, "ll", abs(ll - wl) / abs(wl))
    scale = max(abs(wd), 1e-3 * abs(wl))
    assert abs(dll - wd) <= REF_TOL * scale, (tag, "dll", abs(dll - wd) / scale)


@pytest.mark.parametrize("T,dt,logp", [
    (4, 1.0, (1.0, 3e-3, 1e-4)), (7, 1.0, (0.6, 2e-2, 1e-3)), (24, 1.0, (1.0, 1e-3, 1e-4)), (50, 1.0, (0.3, 1e-2, 1e-4)),
    (50, 0.5, (2.0, 1.2e-2, 1e-3)), (63, 1.0, (1.0, 5e-3, 1e-4)), (64, 2.0, (1.0, 8e-4, 1e-4)), (65, 1.0, (1.0, 3e-3, 1e-4)),
    (100, 1.0, (0.6, 2e-2, 1e-3)), (139, 1.0, (1.0, 3e-3, 1e-3))])
def test_helper_vs_oracle_gp_objective(T, dt, logp):
    logp = np.log(np.array(logp))
    mu, w = _set(T, T, 3)
    want = O.gp_objective(logp, np.arange(T) * dt, mu.T, w.T)
    _close(H.objective(logp, T, dt, mu, w), (want[0], want[1][1]), (T, dt))
    assert want[1][0] == 0 and want[1][2] == 0


def test_counts_price_repeated_segments_once():
    T, logp = 24, np.log(np.array([1.0, 4e-3, 1e-4]))
    mu, w = _set(3, T, 3)
    idx = [0, 1, 2, 0, 1, 0]
    a = H.objective(logp, T, 1.0, mu[idx], w[idx])
    b = H.objective(logp, T, 1.0, mu, w, counts=[3, 2, 1])
    assert abs(a[0] - b[0]) <= 1e-15 * abs(a[0]) and abs(a[1] - b[1]) <= 1e-13 * max(abs(a[1]), 1e-3 * abs(a[0]))


def _mp_objective(mp, logp, T, dt, mu, w):
    """(ll, dll) from the terms of hstep_numpy's header in 40-digit arithmetic, inverses by mpmath's LU."""
    sigmasq, omega, eps = (mp.exp(mp.mpf(float(x))) for x in logp)
    K, dK = mp.matrix(T, T), mp.matrix(T, T)
    for i in range(T):
        for j in range(T):
            d2 = (mp.mpf(i - j) * mp.mpf(float(dt))) ** 2
            k = sigmasq * mp.exp(-omega * d2)
            K[i, j] = k + (eps if i == j else 0)
            dK[i, j] = -k * d2 * omega
    Ki = K ** -1
    logdet = mp.log(mp.det(K))
    ll, dll = mp.mpf(0), mp.mpf(0)
    for m in range(len(mu)):
        x = mp.matrix([mp.mpf(float(v)) for v in mu[m]])
        al = Ki * x
        s = [mp.sqrt(mp.mpf(float(v))) for v in w[m]]
        A = mp.matrix(T, T)
        for i in range(T):
            for j in range(T):
                A[i, j] = s[i] * K[i, j] * s[j] + (1 if i == j else 0)
        Ai = A ** -1
        tr = sum(Ai[i, i] for i in range(T))
        cs = sum(s[i] * s[j] * dK[i, j] * Ai[i, j] for i in range(T) for j in range(T))
        ll += -(x.T * al)[0] / 2 - tr / 2 - logdet / 2
        dll += ((al.T * dK * al)[0] - cs) / 2
    return float(ll), float(dll)


# (T, dt, sigma^2, omega, eps): every window class -- below 24 (generic under the dense switch), the 50-bin and the 64-bin
# round kernels at an odd and an even window, 65 ... 128 -- with both ends of sigma^2, omega and eps
MP_CASES = [(5, 1.0, 0.05, 0.5, 1e-5), (7, 1.0, 20.0, 1e-3, 1e-2), (16, 2.0, 1.0, 2e-2, 1e-5), (23, 1.0, 20.0, 0.5, 1e-5),
            (24, 1.0, 0.05, 2e-4, 1e-2), (33, 0.5, 1.0, 1e-2, 1e-4), (49, 1.0, 20.0, 2e-3, 1e-5), (50, 1.0, 0.05, 0.5, 1e-2),
            (50, 1.0, 1.0, 1.6e-2, 1e-5), (51, 1.0, 20.0, 5e-4, 1e-2), (64, 1.0, 0.05, 1e-2, 1e-5), (65, 1.0, 1.0, 3e-3, 1e-4)]


@pytest.mark.parametrize("T,dt,sigmasq,omega,eps", MP_CASES)
def test_helper_vs_mpmath(T, dt, sigmasq, omega, eps):
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 40
    logp = np.log(np.array([sigmasq, omega, eps]))
    mu, w = _set(1000 + T, T, 2, extreme=True)
    want = _mp_objective(mp, logp, T, dt, mu, w)
    _close(H.objective(logp, T, dt, mu, w), want, (T, dt, sigmasq, omega, eps))
    # the two kinds of set that isolate a kernel: mu = 0 (segment terms alone) and w = 0 (K block alone: tr = T, cs = 0)
    r = H.evaluate(logp, T, dt, mu, np.zeros_like(w))
    assert np.all(r["tr"] == T) and np.all(r["cs"] == 0)
    r0 = H.evaluate(logp, T, dt, np.zeros_like(mu), w)
    assert r0["tr_kic"] == 0 and r0["tr_q"] == 0
