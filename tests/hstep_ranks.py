"""Host-side mirrors of what csrc/hstep.hip decides before a low-rank H-step round, for tests/test_gpu_hstep_shapes.py:
the rank prediction (lr_host_rank, lr_thresholds), the LDS carve (lr_geom of csrc/hstep_lr.h) and the rule that leaves
the tables in global memory (`tabg`, the lambda wgs of launch_hstep_impl).  The device's own report
(Engine.hstep_plan) confirms every value a case takes from here.
"""
import functools

import numpy as np

LR_RCAP, LR_RH, LR_NPAIR, LR_NW = 32, 20, 576, 4
LR_TOL = 1e-12  # default of VLGP_HSTEP_LR_TOL; the host predicts at half of it
KBLK = {50: 1240 + 50 * 50 + 120, 64: 1792 + 64 * 66}  # HRoundK<50, 4, true>::KBLK, HRoundK<64, 4, false>::KBLK (doubles)


def parity_ranks(T, dt, omega, tol=0.5 * LR_TOL):
    """(even, odd): ranks of the two folded blocks of exp(-omega D^2) under the pivoted Cholesky of lr_host_rank (largest
    residual diagonal first, lowest index on ties, stop at <= tol)."""
    h, nt = T // 2, (T + 1) // 2
    d = np.arange(T) * dt
    kv = np.exp(-omega * d * d)
    ranks = []
    for par, n in ((0, nt), (1, h)):
        if n == 0:
            ranks.append(0)
            continue
        t = np.arange(n)
        d1, d2 = np.abs(t[:, None] - t[None, :]), T - 1 - t[:, None] - t[None, :]
        if par == 0:
            s = np.ones(n)
            if T & 1:
                s[h] = np.sqrt(0.5)  # the middle row of an odd window
            km = s[:, None] * s[None, :] * (kv[d1] + kv[d2])
        else:
            km = kv[d1] - kv[d2]
        diag = km.diagonal().copy()
        g = np.zeros((n, n))
        r = 0
        while r < n:
            p = int(np.argmax(diag))
            bv = diag[p]
            if not bv > tol:
                break
            gk = (km[:, p] - g[:, :r] @ g[p, :r]) / np.sqrt(bv)
            g[:, r] = gk
            diag = np.where(diag >= 0.0, diag - gk * gk, diag)
            diag[p] = -1.0
            r += 1
        ranks.append(r)
    return tuple(ranks)


def host_rank(T, dt, omega, tol=0.5 * LR_TOL):
    """lr_host_rank: the two ranks summed; LR_RCAP + 1 when a block exceeds the per-parity capacity LR_RH."""
    re, ro = parity_ranks(T, dt, omega, tol)
    return LR_RCAP + 1 if max(re, ro) > LR_RH else re + ro


@functools.lru_cache(maxsize=None)
def thresholds(T, dt):
    """lr_thresholds: om[r] = the largest omega whose predicted rank is <= r, r = 0 ... LR_RCAP (0.0: none), by bisection in
    ln(omega) as the library does it (to 1e-9 here, which is all a case needs: it takes its omega from the middle of a
    rank's interval)."""
    om = []
    lo0, hi0 = np.log(1e-14), np.log(1e8)
    for r in range(LR_RCAP + 1):
        lo = np.log(om[-1]) if om and om[-1] > 0.0 else lo0
        hi = hi0
        if host_rank(T, dt, np.exp(lo)) > r:
            om.append(0.0)
            continue
        while hi - lo > 1e-9:
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if host_rank(T, dt, np.exp(mid)) <= r else (lo, mid)
        om.append(float(np.exp(lo)))
    return tuple(om)


def rcap_of(T, dt, omega):
    """The columns the launcher grants an evaluation: its predicted rank clamped to >= 4, or 0 for a rough one (> LR_RCAP)."""
    om = thresholds(T, dt)
    r = 0
    while r <= LR_RCAP and not omega <= om[r]:
        r += 1
    return 0 if r > LR_RCAP else max(r, 4)


@functools.lru_cache(maxsize=None)
def reachable(T, dt=1.0):
    """{rank: omega} for every predicted rank 0 ... LR_RCAP some omega gives at this window: omega from the middle (in
    ln omega) of the rank's interval, moved inside it to a point where the prediction at the device's own tolerance
    agrees when there is one.  A rank whose interval is empty (the prediction jumps over it) is absent."""
    om = thresholds(T, dt)
    out = {}
    for r in range(LR_RCAP + 1):
        lo = max((o for o in om[:r] if o > 0.0), default=0.0)
        if om[r] <= 0.0 or (lo > 0.0 and om[r] / lo - 1.0 < 1e-6):
            continue
        a, b = np.log(lo if lo > 0.0 else 1e-14), np.log(om[r])
        # (at most a factor four wide: the full rank of a short window and the lowest rank have no second end worth the name)
        a, b = (a, min(b, a + np.log(4.0))) if lo > 0.0 else (b - np.log(4.0), b)
        for f in (0.5, 0.4, 0.6, 0.3, 0.7, 0.2, 0.8):
            x = float(np.exp(a + f * (b - a)))
            if host_rank(T, dt, x) == r and host_rank(T, dt, x, LR_TOL) == r:
                out[r] = x
                break
        else:
            x = float(np.exp(0.5 * (a + b)))
            if host_rank(T, dt, x) == r:
                out[r] = x
    return out


def rank_class(rmax):
    return 16 if rmax <= 16 else 24 if rmax <= 24 else 28 if rmax <= 28 else 32


def xs_per_wave(rc):
    if rc > 28:  # class 32 inverts row-wise: one lane per row
        return 64
    gb = 4 if rc <= 16 else 5
    bs, lps = (rc + gb - 1) // gb, gb * (gb + 1) // 2
    return ((64 // lps) * gb * bs + 1) & ~1


def geom_total(r, TC, tab_global, rc):
    """lr_geom(r, 4 NK, LR_NW, tab_global, rc).total: doubles of LDS of a segment group."""
    ntp = 4 * (7 if TC == 50 else 8)
    ldu = LR_RCAP if tab_global else ((r + 1) | 1)
    nps = (r * (r + 1) // 2 + 2) | 1
    o_mp = 0 if tab_global else ((2 * ntp * ldu + 1) & ~1)
    o_xb = (o_mp + 16 * nps + 1) & ~1
    o_codes = o_xb + max(LR_NW * xs_per_wave(rc), LR_NW * 32 + 2)
    return o_codes + (min(r * (r + 1) // 2 + 32, LR_NPAIR) + 3) // 4


def round_lds(rmax, TC):
    """(tabg, dynamic LDS in doubles) of the low-rank launch compiled for rmax: the tables stay in global memory when that
    lets one more workgroup share a CU and fewer than three would otherwise."""
    rc = rank_class(rmax)

    def wgs(n):
        n = max(n, KBLK[TC], 2 * 64 * LR_NW)
        return (160 * 1024) // ((n * 8 + 80 + 511) & ~511)

    need_l, need_g = geom_total(rmax, TC, False, rc), geom_total(rmax, TC, True, rc)
    tabg = rc >= 28 and rmax < LR_RCAP and wgs(need_g) > wgs(need_l) and wgs(need_l) < 3
    return int(tabg), max(need_g if tabg else need_l, KBLK[TC], 2 * 64 * LR_NW)


def generic_tier(T):
    """(nw, tm_global, huge) of the generic kernels, from the launcher's byte formulas."""
    ls = T | 1
    huge = T * ls * 8 > 150 * 1024
    tm_global = (T * ls + 3 * T * T) * 8 > 150 * 1024
    nw = 4 if huge else (2 if 2 * (T * ls + 2 * T) * 8 <= 160 * 1024 else 1)
    return nw, int(tm_global), int(huge)
