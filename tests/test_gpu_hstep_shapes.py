"""The H-step objective at every compiled round kernel, rank class, window and segment count, judged per kernel.

launch_hstep_impl (csrc/hstep.hip) chooses among hstep_round_lr<50 | 64, 4, 16 | 24 | 28 | 32, TABG, TABF> behind
hstep_lr_tables, hstep_round_mfma<50, 4, true> and <64, 4>, both on one ticket counter (a mixed round),
hstep_moment_kernel<50 | 64> and hstep_w_latent_major, hstep_prep_big / hstep_seg_big (windows 65 ... 128) and the generic
hstep_prep_kernel / hstep_seg_kernel in four LDS tiers.  The other H-step tests reach these at window 50 and at whatever
ranks a few omegas give; this module walks them:

  a  low-rank, window 50: every rank 4 ... 32 and one below the clamp; inside a bracket (w latent-major), and with
     VLGP_HSTEP_NO_WLM=1, bit for bit                 g  rounds of 2 ... 16 evaluations of mixed ranks, each bit for bit
  b  the same at window 64; 63 at the class edges         what it gives alone; 17 sliced by the engine, refused by the C entry
  c  VLGP_HSTEP_FUSE_TABLES=1 at every rank 4 ... 24,   h  the dense round at 24 ... 50 | 51 ... 64 bins, rank-4-smooth to omega
     bit for bit (rides with a, b); above 24: not fused   0.5; below 24 bins under VLGP_HSTEP_DENSE=1: the generic kernels
  d  which ranks 25 ... 31 leave the tables in global   i  mixed rounds: one rough among three, three among four, rough first
     memory: TABG_RANKS                                    and last; members bit for bit what the pure rounds give; the counters
  e  windows 4 ... 57 at their lowest rank, at the      j  65 ... 128 on the big kernels and under VLGP_HSTEP_GENERIC_SEG=1; the
     16 | 17 edge and at their highest (full rank up to    generic tiers at 69 | 70, 99 | 100, 129, 138 | 139; window 50 under
     32 bins)                                              VLGP_HSTEP_GENERIC=1
  f  segment counts 1 ... 33 (low-rank), 1 ... 7        k  bin widths 0.5 and 2 at window 64
     (dense), 63 ... 65 and 1037 (moment kernel)

Every case ASSERTS through Engine.hstep_plan (vlgp_debug_hstep_plan: what the launcher noted as it decided) the path, the
compiled window, the rank class, rcap of every evaluation, tabg, fused, the dynamic LDS, nb, wlm and the generic tier it
names, so a retune of the size rule or of the LDS rule cannot silently take coverage away.  The rank of an evaluation is
fixed on the host (tests/hstep_ranks.py: lr_host_rank's pivot rule at half the device's tolerance, omega from the middle of
the rank's interval).

Reference: tests/hstep_numpy.py (longdouble; held to oracle.gp_objective and 40-digit mpmath by tests/test_hstep_host.py).
Three kinds of evaluation per shape, one latent each, so that each kernel is judged on its own scale: latent 0 has mu = 0
(ll = -1/2 sum tr - M/2 log det K, dll = -1/2 sum cs: the segment kernels alone), latent 1 has w = 0 (A = I, tr = T, cs = 0:
the K block, the moment kernels and the padding correction alone), latent 2 has both, mu ~ N(0, 1), w = 10^U(-3, 2); where
w is not zero one segment has w = 0 and one has three entries at 1e6.  Tolerances: 1e-9 on |ll|, 1e-9 on
max(|dll|, 1e-3 |ll|), 1e-8 on the latter above 64 bins (as tests/test_gpu_parity.py).  sigma^2 runs over 0.05 ... 20; eps
is the decade at or above sigma^2 T / 1e6 within 1e-5 ... 1e-2: cond(K) <= sigma^2 T / eps <= 1e6 leaves fp64 a factor ten
below the tolerance.  Sets of eight or more segments repeat 7 distinct ones (coprime to 4, 16 and 64).

Not reachable, asserted by test_census: hstep_round_lr<50, 4, 32, true> (at window <= 50 no rank 29 ... 31 gains a third
workgroup per CU from tables in global memory); the per-parity capacity LR_RH = 20 binding before the total 32 (rank 32
splits 16 + 16, the first rough rank 17 + 16), hence also the dense re-run after an overflow (hstat[3], plan["rerun"]): the
host predicts at half the device's tolerance with the same pivot rule.  No rank 2 ... 32 is skipped at windows 50, 63, 64.

Measured on an MI355X (profiles/hstep_shapes/measured_errors.txt, every case; worst evaluation of each): round kernels
(a ... i, k) ll at most 5.0e-12, dll 3.1e-10 (e-T25-r2; a-T50-r12 2.3e-10, b-T63-r32 2.6e-10); big kernels ll 4.7e-10, dll
1.4e-9 (both j-big-T96; the tolerances there are 1e-9 and 1e-8); generic kernels ll 5.0e-12, dll 5.6e-10
(j-big-T65-genericseg).  Every plan, every bit-for-bit variant and every tabg prediction held.

Two findings, neither an arithmetic defect:
  * The low-rank round drops the kernel's residual below VLGP_HSTEP_LR_TOL = 1e-12; cs takes the residual's derivative
    times s_j s_k (A^-1)_jk, which reaches 1 / eps where eps w >> 1.  With the 1e6 bins also on the latent with mu = 0 (the
    segment kernels on their own scale) the lowest rank of four windows missed 1e-9 on max(|dll|, 1e-3 |ll|): e-T4-r1
    1.24e-7, e-T5-r1 4.1e-9, e-T7-r1 4.5e-9, e-T25-r2 1.26e-9.  The same truncation in exact arithmetic on the host
    (tools/lr_proto.py: pchol_tangent at 1e-12, seg_terms_lr) gives 1.2e-7, 4.1e-9, 4.5e-9, 1.3e-9, and 1e-15 or less at
    1e-14: the case asks of the approximation what its tolerance does not give, the kernel computes it faithfully.  The
    1e6 bins therefore stand where the quadratic term carries the scale (latent 2); the tolerance is part of the
    headline's bits and stays.
  * An evaluation is NOT always bit-identical alone and inside a round compiled for a higher register class (the classes
    invert M in different block layouts).  In the first run of this module: rank 17 alone (class 24) against the class-32
    round (4, 17, 32) differed by 3.3e-14 of |ll| at window 50, 1.6e-15 at 64; ranks 9 and 16 (class 16) against the round
    (9, 16, 24, 29) by at most 1.3e-14; ranks 4, 5, 24, 28, 29 and 32 of those rounds did not differ; several of a round
    of fifteen ranks spread over all classes did, the first of them by 7.5e-14.  Within one class every evaluation of a
    round of 2, 15 or 16 equals its call alone bit for bit, which is what the n_eval cases assert (class 16, 24, 28 and
    32); the rounds of mixed classes (4, 17, 32), (5, 28), (9, 16, 24, 29) are held to the reference.
"""
import ctypes
import functools
import os
import re
import zlib

import numpy as np
import pytest

import hstep_numpy as H
import hstep_ranks as R

gpu = pytest.mark.gpu  # per test: the table, census, sensitivity and conditioning checks run without a GPU

STAGE = 1e-9    # tests/test_gpu_parity.py
DLL_TOL = 1e-9
DLL_TOL_LONG = 1e-8  # windows above 64 bins (test_hstep_objective_other_windows_vs_oracle)
SWITCHES = ("VLGP_HSTEP_DENSE", "VLGP_HSTEP_GENERIC", "VLGP_HSTEP_LOWRANK", "VLGP_HSTEP_GENERIC_SEG", "VLGP_HSTEP_FUSE_TABLES",
            "VLGP_HSTEP_NO_WLM", "VLGP_HSTEP_LR_TOL")
LOWRANK = {"VLGP_HSTEP_LOWRANK": "1"}  # hold the low-rank round against the size rule
DENSE = {"VLGP_HSTEP_DENSE": "1"}
FUSE = {"VLGP_HSTEP_FUSE_TABLES": "1"}
NO_WLM = {"VLGP_HSTEP_NO_WLM": "1"}
S2 = (1.0, 0.05, 20.0, 0.3, 5.0)
ROUGH = 0.3  # an omega far above rank 32 at every window from 34 bins
# d. the ranks whose round leaves the tables in global memory, per compiled window (csrc/hstep.hip: tabg)
TABG_RANKS = {50: (25, 26, 27), 64: (25, 26, 27, 31)}
PLAN_ZERO = dict(rerun=0, TC=0, nb=0, wlm=0, n_lr=0, n_rough=0, rmax=0, rc=0, tabg=0, fused=0, lds=0, rcap=[0] * 16, nw=0,
                 tm_global=0, huge=0)


def eps_for(s2, T):
    return float(min(1e-2, max(1e-5, 10.0 ** np.ceil(np.log10(s2 * T / 1e6) - 1e-9))))


def ev(lat, omega, s2, T):
    return dict(lat=lat, omega=float(omega), s2=s2, eps=eps_for(s2, T))


def kinds(T, omega, s2):
    """The three kinds of evaluation at one omega."""
    return [ev(l, omega, s2, T) for l in (0, 1, 2)]


def expected_plan(c, env=None, bracket=False, evals=None):
    """The plan a case names, from its window, sizes, omegas and switches."""
    env = c["env"] if env is None else env
    evals = c["evals"] if evals is None else evals
    T, M = c["T"], c["M"]
    p = dict(PLAN_ZERO, rcap=[0] * 16)
    dense = "VLGP_HSTEP_DENSE" in env
    if T > 64 or "VLGP_HSTEP_GENERIC" in env or T < (24 if dense else 4):
        if 64 < T <= 128 and "VLGP_HSTEP_GENERIC_SEG" not in env and "VLGP_HSTEP_GENERIC" not in env:
            return dict(p, path="big")
        nw, tm, huge = R.generic_tier(T)
        return dict(p, path="generic", nw=nw, tm_global=tm, huge=huge)
    assert dense or "VLGP_HSTEP_LOWRANK" in env, c["id"]  # (else the size rule decides)
    p.update(TC=50 if T <= 50 else 64, wlm=int(bracket and "VLGP_HSTEP_NO_WLM" not in env))
    rcap = [0 if dense else R.rcap_of(T, c["dt"], e["omega"]) for e in evals]
    n_lr = sum(r > 0 for r in rcap)
    if n_lr == 0:
        return dict(p, path="dense", nb=(M + 3) // 4)
    rmax = max(rcap)
    tabg, lds = R.round_lds(rmax, p["TC"])
    return dict(p, path="mixed" if n_lr < len(evals) else "lowrank", nb=(M + 15) // 16, n_lr=n_lr, n_rough=len(evals) - n_lr,
                rmax=rmax, rc=R.rank_class(rmax), tabg=tabg, fused=int("VLGP_HSTEP_FUSE_TABLES" in env and rmax <= 24), lds=lds,
                rcap=rcap + [0] * (16 - len(rcap)))


def case(cid, T, evals, M=19, dt=1.0, env=None, also=(), path=None, alone=False, names=None):
    """also: variants (tag, extra switches, bracket) whose results must equal the case's bit for bit; alone: every evaluation
    is called alone as well; names: plan fields the table states as literals (checked against the derived plan)."""
    c = dict(id=cid, T=T, dt=dt, M=M, distinct=min(M, 7), evals=list(evals), also=list(also), alone=alone,
             env=dict(LOWRANK if env is None and T <= 64 else (env or {})))
    assert 1 <= len(c["evals"]) <= 16, cid
    c["expect"] = expected_plan(c)
    c["names"] = dict(names or {}, path=path)
    return c


def build_table():
    m = []
    BRACKET = [("bracket", {}, True), ("bracket-nowlm", NO_WLM, True)]
    # a, b (and c, d with them): every rank at the two compiled windows, the three kinds at each
    for tag, T in (("a", 50), ("b", 64)):
        re = R.reachable(T)
        TC = 50 if T <= 50 else 64
        for r in range(4, 33):
            also = BRACKET + ([("fused", FUSE, False)] if r <= 24 or r == 26 else [])
            names = dict(TC=TC, rc=R.rank_class(r), tabg=int(r in TABG_RANKS[TC]), rmax=r)
            m.append(case("%s-T%d-r%d" % (tag, T, r), T, kinds(T, re[r], S2[r % 5]), also=also, path="lowrank", names=names))
        m.append(case("%s-T%d-below-clamp" % (tag, T), T, kinds(T, 1e-7, 1.0), also=BRACKET, path="lowrank",
                      names=dict(rmax=4, rc=16)))
    re = R.reachable(63)
    for r in (4, 16, 17, 24, 25, 28, 29, 31, 32):  # an odd window: the middle row of the even block is scaled by 1 / sqrt 2
        m.append(case("b-T63-r%d" % r, 63, kinds(63, re[r], S2[r % 5]), also=[("bracket", {}, True)], path="lowrank",
                      names=dict(TC=64, rc=R.rank_class(r), tabg=int(r in TABG_RANKS[64]))))
    # e. windows through the round kernels: lowest rank, the 16 | 17 edge, the highest rank <= 32 (full rank up to 32 bins)
    for T in (4, 5, 7, 16, 23, 24, 25, 33, 49, 51, 52, 57):
        re = R.reachable(T)
        lo, hi = min(re), max(re)
        assert hi == min(T, 32), (T, hi)
        for r in sorted({lo, hi} | {r for r in (16, 17) if lo < r < hi}):
            m.append(case("e-T%d-r%d" % (T, r), T, kinds(T, re[r], S2[(T + r) % 5]), path="lowrank",
                          names=dict(TC=50 if T <= 50 else 64, rmax=max(r, 4))))
    # f. segment counts: groups of sixteen (low-rank), of four (dense), the moment kernel's 64 chunks and stages of sixteen
    re = R.reachable(50)
    for M in (1, 15, 16, 17, 31, 32, 33):
        m.append(case("f-lr-M%d" % M, 50, kinds(50, re[12], 1.0), M=M, path="lowrank"))
    for M in (1, 3, 4, 5, 7):
        m.append(case("f-dense-M%d" % M, 50, kinds(50, 0.1, 1.0), M=M, env=DENSE, path="dense"))
    for M in (63, 64, 65, 1037):
        m.append(case("f-moment-M%d" % M, 50, kinds(50, re[8], 1.0), M=M, also=[("bracket", {}, True)], path="lowrank"))
    m.append(case("f-moment64-M65", 64, kinds(64, R.reachable(64)[9], 1.0), M=65, path="lowrank"))
    m.append(case("f-moment64-M1037-dense", 64, kinds(64, 0.05, 1.0), M=1037, env=DENSE, also=[("bracket", {}, True)], path="dense"))
    # g. rounds of several evaluations: compiled for the largest rank, stably sorted by rank, one mailbox
    for T in (50, 64):
        re = R.reachable(T)
        for ranks in ((4, 17, 32), (5, 28), (9, 16, 24, 29)):
            m.append(case("g-T%d-ranks%s" % (T, "-".join(map(str, ranks))), T,
                          [ev((2, 0, 1)[i % 3], re[r], S2[i % 5], T) for i, r in enumerate(ranks)], path="lowrank",
                          names=dict(rmax=max(ranks), rc=R.rank_class(max(ranks)))))
    # n_eval = 2, 15, 16 (the mailbox full to index 47): repeated latents, a distinct (latent, sigma^2, omega) per evaluation, in
    # an order the rank sort permutes; every evaluation also alone, bit for bit -- the ranks of a round stay within ONE
    # register class, so that alone the same instantiation runs (the docstring: across classes the bits differ)
    re = R.reachable(50)
    for tag, n, order in (("2", 2, (18, 23)), ("15", 15, (11, 6, 4, 15, 9, 7, 13, 16, 14, 5, 8, 12, 10, 4, 16)),
                          ("16", 16, (11, 6, 4, 15, 9, 7, 13, 16, 14, 5, 8, 12, 10, 4, 16, 9)),
                          ("16-class28", 16, (26, 25, 28, 27) * 4), ("16-class32", 16, (30, 29, 32, 31) * 4)):
        evals = [ev(i % 3, re[r], S2[i % 5], 50) for i, r in enumerate(order)]
        assert len(evals) == n and len({(e["lat"], e["s2"], e["omega"]) for e in evals}) == n
        m.append(case("g-n_eval%s" % tag, 50, evals, alone=True, path="lowrank",
                      names=dict(rmax=max(order), rc=R.rank_class(min(order)))))
    # h. the dense round: <50, ONESET> at 24 ... 50 bins, <64> at 51 ... 64, from a rank-4 kernel to omega 0.5
    for T in (24, 25, 49, 50, 51, 63, 64):
        m.append(case("h-dense-T%d" % T, T, kinds(T, R.reachable(T)[4], 1.0) + kinds(T, 0.5, 5.0), env=DENSE,
                      also=[("bracket", {}, True)], path="dense", names=dict(TC=50 if T <= 50 else 64)))
    for T in (4, 12, 23):
        m.append(case("h-dense-T%d-generic" % T, T, kinds(T, 0.02, 1.0), env=DENSE, M=5, path="generic", names=dict(nw=2)))
    # j. above 64 bins: the workgroup-per-segment kernels, the generic kernels at the edges of their LDS tiers
    for T in (65, 96, 127, 128):
        m.append(case("j-big-T%d" % T, T, kinds(T, 3e-3, 1.0) + [ev(2, 2e-2, 0.3, T)], M=3, path="big"))
        m.append(case("j-big-T%d-genericseg" % T, T, kinds(T, 3e-3, 1.0), M=3, env={"VLGP_HSTEP_GENERIC_SEG": "1"}, path="generic"))
    for T, tier in ((69, (2, 0, 0)), (70, (2, 1, 0)), (99, (2, 1, 0)), (100, (1, 1, 0)), (129, (1, 1, 0)), (138, (1, 1, 0)),
                    (139, (4, 1, 1))):
        env = {"VLGP_HSTEP_GENERIC_SEG": "1"} if T <= 128 else {}
        m.append(case("j-generic-T%d" % T, T, kinds(T, 3e-3, 1.0), M=5 if T < 129 else 3, env=env, path="generic",
                      names=dict(zip(("nw", "tm_global", "huge"), tier))))
    for M in (1, 2, 3):  # two waves per workgroup: a full one and a half-empty one
        m.append(case("j-generic-T50-M%d" % M, 50, kinds(50, 3e-3, 1.0), M=M, env={"VLGP_HSTEP_GENERIC": "1"}, path="generic",
                      names=dict(nw=2, tm_global=0, huge=0)))
    # k. other bin widths at the 64-bin kernels (tests/test_gpu_parity.py has three at 50)
    for dt in (0.5, 2.0):
        m.append(case("k-T64-dt%g" % dt, 64, kinds(64, R.reachable(64, dt)[20], 1.0), dt=dt, path="lowrank",
                      names=dict(TC=64, rmax=20, rc=24)))
    return m


def build_mixed():
    """i. mixed rounds: (id, window, evaluations); R = a rough evaluation (the dense kernel), a number = that rank."""
    m = []
    for T in (50, 64):
        re = R.reachable(T)
        for tag, spec in (("1of3", (12, "R", 20)), ("3of4", ("R", 27, "R", "R")), ("first-last", ("R", 9, 32, "R"))):
            evals = [ev(i % 3, ROUGH if r == "R" else re[r], S2[i % 5], T) for i, r in enumerate(spec)]
            m.append(case("i-T%d-%s" % (T, tag), T, evals, path="mixed",
                          names=dict(n_rough=sum(r == "R" for r in spec), rmax=max(r for r in spec if r != "R"))))
    return m


TABLE = build_table()
MIXED = build_mixed()
BY_ID = {c["id"]: c for c in TABLE + MIXED}
IDS = [c["id"] for c in TABLE]
assert len(BY_ID) == len(TABLE) + len(MIXED)


# ------------------------------------------------------------------ sets and their reference
@functools.lru_cache(maxsize=None)
def segments(cid):
    """(mu, w), each (distinct, T, 3): the distinct segments of the case's set, latent = kind."""
    c = BY_ID[cid]
    T, D, M = c["T"], c["distinct"], c["M"]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    mu = rng.standard_normal((D, T, 3))
    w = 10.0 ** rng.uniform(-3, 2, (D, T, 3))
    hot = rng.choice(T, min(3, T), replace=False)
    if D >= 3:
        w[(M - 1) % D - 2] = 0.0            # one segment without curvature
        w[(M - 1) % D - 1, hot, 2] = 1e6    # one with a few bins that pin the posterior (latent 2 only: the docstring's finding)
    elif D == 2:
        w[0, hot, 2] = 1e6
    w[(M - 1) % D, T - 1] = 100.0  # the set's last segment: the sensitivity check zeroes this row (the top of w's range: it
                                   # has to show beside the other bins even where K has rank 2)
    mu[:, :, 0] = 0.0
    w[:, :, 1] = 0.0
    return mu, w


def counts_of(c, M=None):
    M = c["M"] if M is None else M
    return np.bincount(np.arange(M) % c["distinct"], minlength=c["distinct"])


def units_of(c):
    mu, w = segments(c["id"])
    T = c["T"]
    return [dict(y=np.zeros((T, 2)), mu=mu[m % c["distinct"]].copy(), w=w[m % c["distinct"]].copy(), v=np.zeros((T, 3)))
            for m in range(c["M"])]


def arrays(evals):
    return (np.array([e["lat"] for e in evals], dtype=np.int32),
            np.log(np.array([[e["s2"], e["omega"], e["eps"]] for e in evals])))


def reference_of(c, mu, w, evals=None, counts=None):
    lat, logp = arrays(c["evals"] if evals is None else evals)
    counts = counts_of(c) if counts is None else counts
    return [H.evaluate(lp, c["T"], c["dt"], mu[:, :, l], w[:, :, l], counts) for l, lp in zip(lat, logp)]


@functools.lru_cache(maxsize=None)
def reference(cid):
    c = BY_ID[cid]
    return reference_of(c, *segments(cid))


def errors(c, ll, dll, ref):
    """Per evaluation: |ll - ref| / |ref| and |dll - ref| / max(|dll ref|, 1e-3 |ll ref|)."""
    e_ll = np.array([abs(a - r["ll"]) / abs(r["ll"]) for a, r in zip(ll, ref)])
    e_dll = np.array([abs(a - r["dll"]) / max(abs(r["dll"]), 1e-3 * abs(r["ll"])) for a, r in zip(dll, ref)])
    return e_ll, e_dll


def dll_tol(c):
    return DLL_TOL if c["T"] <= 64 else DLL_TOL_LONG


# ------------------------------------------------------------------ the table itself (no GPU)
def test_table_names_what_the_mirrors_derive():
    assert len(IDS) == len(set(IDS))
    for c in TABLE + MIXED:
        for k, v in c["names"].items():
            assert c["expect"][k] == v, (c["id"], k, v, c["expect"])
        for e in c["evals"]:
            assert 0.05 <= e["s2"] <= 20.0 and 1e-5 <= e["eps"] <= 1e-2 and e["s2"] * c["T"] / e["eps"] <= 1e6 * (1 + 1e-9), c["id"]
    for T in (50, 63, 64):  # every rank is walked: none is skipped by the prediction, and the device's tolerance agrees
        re = R.reachable(T)
        assert sorted(re) == list(range(2, 33)), (T, sorted(re))
    for tag, T in (("a", 50), ("b", 64)):
        for r in range(4, 33):
            c = BY_ID["%s-T%d-r%d" % (tag, T, r)]
            assert c["expect"]["rcap"][:3] == [r] * 3 and R.host_rank(T, 1.0, c["evals"][0]["omega"]) == r
    for T in (50, 64):
        assert R.host_rank(T, 1.0, 1e-7) < 4 and R.rcap_of(T, 1.0, 1e-7) == 4  # a true rank below the clamp
        assert R.rcap_of(T, 1.0, ROUGH) == 0
    for TC, ranks in TABG_RANKS.items():
        assert tuple(r for r in range(4, 33) if R.round_lds(r, TC)[0]) == ranks
    # the tier edges of the generic kernels, from the launcher's two byte formulas
    tiers = {T: R.generic_tier(T) for T in range(4, 201)}
    assert min(T for T, t in tiers.items() if t[1]) == 70 and min(T for T, t in tiers.items() if t[0] == 1) == 100
    assert min(T for T, t in tiers.items() if t[2]) == 139 and all(t[0] == 4 for t in tiers.values() if t[2])


def test_plan_report_layout_is_the_headers():
    from vlgp_amd import _lib

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vlgp_hip.h")) as f:
        defs = {k: int(v) for k, v in re.findall(r"^#define (VLGP_\w+) (-?\d+)\b", f.read(), re.M)}
    assert {k[len("VLGP_HP_"):]: v for k, v in defs.items() if k.startswith("VLGP_HP_")} == _lib.HP
    slots = sorted(_lib.HP.values())
    assert slots == list(range(len(slots))) and _lib.HP["RCAP"] == slots[-1]
    assert defs["VLGP_HSTEP_PLAN_LEN"] == _lib.HSTEP_PLAN_LEN == _lib.HP["RCAP"] + 16
    assert {k[len("VLGP_PATH_HSTEP_"):].lower(): v for k, v in defs.items() if k.startswith("VLGP_PATH_HSTEP_")} == \
        {k: i for i, k in enumerate(_lib.HSTEP_PATHS)}


def plans_of(c):
    yield c["expect"]
    for _, extra, bracket in c["also"]:
        yield expected_plan(c, dict(c["env"], **extra), bracket)


def test_census():
    """The declared plans of the table cover every compiled H-step instantiation, but the one no rank can take."""
    lr, dense, moment, tiers, paths, wlm = set(), set(), set(), set(), set(), set()
    for c in TABLE + MIXED:
        for p in plans_of(c):
            paths.add(p["path"])
            if p["path"] in ("lowrank", "mixed"):
                lr.add((p["TC"], p["rc"], bool(p["tabg"]), bool(p["fused"])))
                assert p["rmax"] < R.LR_RCAP or not p["tabg"]  # rank 32: LDU > LR_RCAP, the zero column lies outside the table
            if p["path"] in ("dense", "mixed"):
                dense.add(p["TC"])
            if p["path"] in ("lowrank", "mixed", "dense"):
                moment.add(p["TC"])
                wlm.add((p["path"], p["wlm"]))
            if p["path"] == "generic":
                tiers.add((p["nw"], p["tm_global"], p["huge"]))
    want = {(TC, rc, False, False) for TC in (50, 64) for rc in (16, 24, 28, 32)}  # hstep_round_lr<T, 4, RC> behind hstep_lr_tables
    want |= {(TC, rc, False, True) for TC in (50, 64) for rc in (16, 24)}          # <T, 4, RC, false, true>: TABF
    want |= {(50, 28, True, False), (64, 28, True, False), (64, 32, True, False)}  # <T, 4, RC, true>: TABG
    assert lr == want, (lr ^ want)
    # compiled, taken by no reachable rank: at window <= 50 the ranks 29 ... 31 keep their tables in LDS
    assert all(not R.round_lds(r, 50)[0] for r in (29, 30, 31)) and (50, 32, True, False) not in lr
    assert dense == {50, 64} and moment == {50, 64}            # hstep_round_mfma<50, 4, true>, <64, 4>; hstep_moment_kernel
    assert {("lowrank", 0), ("lowrank", 1), ("dense", 0), ("dense", 1)} <= wlm  # hstep_w_latent_major and the strided reads
    assert paths == {"lowrank", "dense", "mixed", "big", "generic"}    # hstep_prep_big / hstep_seg_big
    assert tiers == {(2, 0, 0), (2, 1, 0), (1, 1, 0), (4, 1, 1)}       # hstep_prep_kernel / hstep_seg_kernel, four LDS tiers
    # the per-parity capacity cannot bind before the total: the largest low-rank omega and the smallest rough one
    for T in (33, 50, 63, 64):
        om = R.thresholds(T, 1.0)[R.LR_RCAP]
        assert R.parity_ranks(T, 1.0, om) == (16, 16) and R.parity_ranks(T, 1.0, om * 1.01) == (17, 16), T
    for c in TABLE + MIXED:  # every window of the table, at the omegas it uses
        for e in c["evals"]:
            if c["T"] <= 64 and R.rcap_of(c["T"], c["dt"], e["omega"]):
                assert max(R.parity_ranks(c["T"], c["dt"], e["omega"])) <= R.LR_RH


@pytest.mark.parametrize("cid", IDS + [c["id"] for c in MIXED])
def test_every_case_is_sensitive_and_well_conditioned(cid):
    """On the reference alone.  Sensitivity: leaving out the set's last segment, zeroing the last row of that segment's w
    (judged on the kind with mu = 0, whose scale the segment kernels make) or taking omega at the threshold of the rank
    below moves ll or dll of every evaluation concerned by at least 100 x the tolerance -- no case can pass with a dropped
    tail or a truncated factor.  Conditioning: one ulp on every mu and w moves no result by more than a tenth of it."""
    c = BY_ID[cid]
    mu, w = segments(cid)
    ref = reference(cid)
    tol = (STAGE, dll_tol(c))
    moved = lambda other: [max(a / tol[0], b / tol[1]) for a, b in zip(*errors(c, [o["ll"] for o in other],
                                                                               [o["dll"] for o in other], ref))]
    last = (c["M"] - 1) % c["distinct"]
    # (the shares of one segment: no second pass over the set)
    dropped = [dict(ll=r["ll"] + 0.5 * float(r["quad"][last] + r["tr"][last] + r["logdet"]),
                    dll=r["dll"] - 0.5 * float(r["gq"][last] - r["cs"][last])) for r in ref]
    if c["M"] > 1:
        assert min(moved(dropped)) >= 100, (cid, "last segment", moved(dropped))
    for e, r in zip(c["evals"], ref):
        if e["lat"] != 0:
            continue
        wz = w[last, :, 0].copy()
        wz[-1] = 0.0
        tr, cs = H.seg_terms(np.log([e["s2"], e["omega"], e["eps"]]), c["T"], c["dt"], wz)
        zeroed = dict(ll=r["ll"] + 0.5 * float(r["tr"][last] - tr[0]), dll=r["dll"] + 0.5 * float(r["cs"][last] - cs[0]))
        m = max(abs(zeroed["ll"] - r["ll"]) / abs(r["ll"]) / tol[0],
                abs(zeroed["dll"] - r["dll"]) / max(abs(r["dll"]), 1e-3 * abs(r["ll"])) / tol[1])
        assert m >= 100, (cid, "last row of w", m)
    if c["expect"]["path"] in ("lowrank", "mixed"):
        om = R.thresholds(c["T"], c["dt"])
        below = []
        for e, rc in zip(c["evals"], c["expect"]["rcap"]):
            lower = [o for o in om[:rc] if 0.0 < o < e["omega"]]
            below.append(dict(e, omega=max(lower)) if rc and lower else None)
        if any(below):
            other = reference_of(c, mu, w, [b or e for b, e in zip(below, c["evals"])])
            assert min(m for m, b in zip(moved(other), below) if b) >= 100, (cid, "omega of the rank below", moved(other))
    rng = np.random.default_rng(1)
    ulp = lambda a: np.where(a == 0.0, 0.0, np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf)))  # (a zero stays)
    worst = max(moved(reference_of(c, ulp(mu), ulp(w))))
    print("hstep-shapes %-26s one-ulp perturbation of mu and w: %.1e of the tolerance" % (cid, worst))
    assert worst <= 0.1, (cid, worst)


# ------------------------------------------------------------------ on the device
@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def switch_to(eng, env, want):
    """The handle holds exactly the switches `want` (the library reads them at creation and on reload only)."""
    for name in SWITCHES[:-1]:
        if name in want:
            env.setenv(name, want[name])
        else:
            env.delenv(name, raising=False)
    eng.reload_switches()
    for name in SWITCHES[:-1]:
        assert eng.switch(name) == float(name in want), name
    assert eng.switch("VLGP_HSTEP_LR_TOL") == R.LR_TOL


def call(eng, c, evals=None, bracket=False):
    lat, logp = arrays(c["evals"] if evals is None else evals)
    if bracket:
        eng.hstep_begin(0, c["T"])
    try:
        ll, dll = eng.hstep_objective(0, c["T"], c["dt"], lat, logp)
    finally:
        if bracket:
            eng.hstep_end()
    plan = eng.hstep_plan()
    assert plan["path"] == eng.last_hstep_path
    return ll, dll, plan


def assert_plan(c, plan, want, tag=""):
    assert plan == want, (c["id"], tag, {k: (plan[k], want[k]) for k in want if plan[k] != want[k]})


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def check_and_report(c, ll, dll, ref, plan=None, tag=""):
    e_ll, e_dll = errors(c, ll, dll[:, 1], ref)
    print("hstep-shapes %-26s%s ll %.2e  dll %.2e" % (c["id"], tag, e_ll.max(), e_dll.max())
          + ("  plan %s rcap %s" % ({k: v for k, v in plan.items() if v and k != "rcap"}, plan["rcap"][:len(ll)]) if plan else ""))
    for i in range(len(ref)):
        assert e_ll[i] <= STAGE and e_dll[i] <= dll_tol(c), (c["id"], tag, i, e_ll[i], e_dll[i])  # (a NaN fails)
    assert np.all(dll[:, 0] == 0) and np.all(dll[:, 2] == 0), c["id"]


@gpu
@pytest.mark.parametrize("cid", IDS)
def test_shapes_vs_numpy(V, cid, clean_env):
    """One case of the table: its plan, every evaluation against the reference, once more for the same bits, then its
    variants (bracket, strided w, fused tables) and its evaluations alone, bit for bit."""
    c = BY_ID[cid]
    with V.Engine(2, 3, 1, 50) as eng:
        switch_to(eng, clean_env, c["env"])
        eng.upload(0, units_of(c))
        ll, dll, plan = call(eng, c)
        assert_plan(c, plan, c["expect"])
        check_and_report(c, ll, dll, reference(cid), plan)
        assert same_bits(call(eng, c), (ll, dll)), cid  # repeatable bit for bit
        for tag, extra, bracket in c["also"]:
            env = dict(c["env"], **extra)
            switch_to(eng, clean_env, env)
            got = call(eng, c, bracket=bracket)
            assert_plan(c, got[2], expected_plan(c, env, bracket), tag)
            assert same_bits(got, (ll, dll)), (cid, tag, got[0] - ll, got[1][:, 1] - dll[:, 1])
        if c["alone"]:
            switch_to(eng, clean_env, c["env"])
            differ = []
            for i, e in enumerate(c["evals"]):
                one = call(eng, c, [e])
                assert one[2]["rcap"][0] == c["expect"]["rcap"][i] and one[2]["n_lr"] == 1 and one[2]["rc"] == plan["rc"]
                if not (one[0][0] == ll[i] and np.array_equal(one[1][0], dll[i])):
                    differ.append((i, one[2]["rc"], (one[0][0] - ll[i]) / abs(ll[i]), one[1][0, 1] - dll[i, 1]))
            assert not differ, (cid, "evaluations that differ alone: (index, class alone, ll rel, dll abs)", differ)


@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in MIXED])
def test_mixed_rounds_are_their_pure_rounds_bitwise(V, cid, clean_env):
    """i. a mixed round against the reference; its low-rank members equal the round of those members alone, its rough
    members the all-dense round, bit for bit; the counters move by what ran."""
    c = BY_ID[cid]
    lr = [i for i, r in enumerate(c["expect"]["rcap"][:len(c["evals"])]) if r]
    rough = [i for i in range(len(c["evals"])) if i not in lr]
    with V.Engine(2, 3, 1, 50) as eng:
        switch_to(eng, clean_env, c["env"])
        eng.upload(0, units_of(c))
        s0 = eng.hstep_stats()
        ll, dll, plan = call(eng, c)
        s1 = eng.hstep_stats()
        assert_plan(c, plan, c["expect"])
        assert list(s1 - s0) == [len(lr), sum(c["expect"]["rcap"]), len(rough), 0]
        check_and_report(c, ll, dll, reference(cid), plan)
        assert same_bits(call(eng, c), (ll, dll)), cid
        low = call(eng, c, [c["evals"][i] for i in lr])
        assert low[2]["path"] == "lowrank" and low[2]["rc"] == plan["rc"] and low[2]["lds"] == plan["lds"]
        assert np.array_equal(low[0], ll[lr]) and np.array_equal(low[1], dll[lr]), (cid, low[0] - ll[lr])
        switch_to(eng, clean_env, DENSE)
        s2 = eng.hstep_stats()
        dense = call(eng, c)
        assert dense[2]["path"] == "dense" and list(eng.hstep_stats() - s2) == [0, 0, len(c["evals"]), 0]
        assert np.array_equal(dense[0][rough], ll[rough]) and np.array_equal(dense[1][rough], dll[rough]), cid


@gpu
def test_plan_entry_validates_and_reports(V, clean_env):
    c = BY_ID["a-T50-r12"]
    with V.Engine(2, 3, 1, 50) as eng:
        switch_to(eng, clean_env, c["env"])
        assert eng.hstep_plan() == dict(PLAN_ZERO, path="none")  # before the first call
        with pytest.raises(V.VlgpError):
            eng._ck(eng.lib.vlgp_debug_hstep_plan(eng.h, None))
        eng.upload(0, units_of(c))
        _, _, plan = call(eng, c)
        assert_plan(c, plan, c["expect"])
        assert eng.hstep_plan() == plan  # reading it changes nothing
        with pytest.raises(V.VlgpError):
            eng.hstep_objective(0, 49, 1.0, [0], np.log([[1.0, 1e-3, 1e-4]]))  # not the set's window: refused before any launch
        assert eng.hstep_plan() == plan


@gpu
def test_seventeen_evaluations(V, clean_env):
    """The engine slices 17 evaluations into 16 + 1; the C entry refuses them and launches nothing."""
    c = BY_ID["g-n_eval16"]
    evals = c["evals"] + [ev(1, R.reachable(50)[18], 1.0, 50)]
    lat, logp = arrays(evals)
    with V.Engine(2, 3, 1, 50) as eng:
        switch_to(eng, clean_env, c["env"])
        eng.upload(0, units_of(c))
        ll, dll = eng.hstep_objective(0, 50, 1.0, lat, logp)
        plan = eng.hstep_plan()  # (of the second slice)
        assert plan["n_lr"] == 1 and plan["rcap"][0] == 18 and plan["path"] == "lowrank"
        ref = reference(c["id"]) + reference_of(c, *segments(c["id"]), evals[16:])
        e_ll, e_dll = errors(c, ll, dll[:, 1], ref)
        print("hstep-shapes %-26s ll %.2e  dll %.2e" % ("g-n_eval17-sliced", e_ll.max(), e_dll.max()))
        assert e_ll.max() <= STAGE and e_dll.max() <= DLL_TOL
        first = call(eng, c)
        assert np.array_equal(first[0], ll[:16]) and np.array_equal(first[1], dll[:16])
        stats = eng.hstep_stats()
        out_ll, out_dll = np.full(17, 7.0), np.full((17, 3), 7.0)
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        rc = eng.lib.vlgp_hstep_objective(eng.h, 0, 50, 1.0, 17, lat.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), dp(logp),
                                          dp(out_ll), dp(out_dll))
        assert rc == -1  # VLGP_ERR_ARG
        assert np.all(out_ll == 7.0) and np.all(out_dll == 7.0) and np.array_equal(eng.hstep_stats(), stats)
        assert eng.hstep_plan() == first[2]  # the report of the call before it
        assert same_bits(call(eng, c), first)  # and the handle is still good
