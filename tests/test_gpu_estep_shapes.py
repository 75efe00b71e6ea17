"""The E-step at every compiled rank, window length and unit geometry, judged per (unit, latent) column.

csrc/estep_split.hip and csrc/estep_lane.h compile the lane-per-task kernels esplit_lane<KIND, RTOP> (rank cases 4, 6, 8 ... 14,
RTOP 13 and 14), the wave-per-task classes esplit_latent<16 | 20 | 24 | 32>, the mixed launches esplit_mix<KIND, 20 | 24 | 32, 13>,
the row passes (CS 1, 2, 4) and the y pass (NJ 4, 8, lane-per-row); csrc/estep_fast.hip, estep.hip and estep_long.hip the
other families.  The other E-step tests reach these at T = 50 and at whatever ranks their random omega gives; this module
walks them:

  a  lane-per-task ranks 1 ... 14, RTOP 13 and 14       f  ragged sets (lengths 1 ... 64), long split at 65, 128, 129
  b  wave-per-task ranks 2 ... 32, shared and own G      g  channels N = 1 ... 1025, latents L = 1 ... 10, regressors
  c  mixed launches at maxra 20, 24, 32 and MIX=0       h  vb off, update_w and update_v alone
  d  window lengths T = 1 ... 64 on lane, wave, fast     i  the fast kernel at LT x RA, the generic kernel at each LT (L 2 ... 33)
  e  unit counts: 64-unit groups, 4-unit groups, two to four stream lanes (bit for bit against one lane)

Every case fixes the rank of every latent on the host (omega found with oracle.ichol_gauss), ASSERTS it on the device through
get_prior(T, with_rank=True), and ASSERTS through Engine.estep_plan (vlgp_debug_estep_plan: launch_estep's own dispatch,
reporting instead of launching) the family, the classes, RTOP, maxra, shared G, the stream lanes and their cuts, CS and NJ
it names, so a retune of plan_estep_split cannot silently take the coverage away.

Reference: oracle.estep_unit on inputs prepared as _random_problem (tests/test_gpu_parity.py) prepares them.  mu, v, w are
compared PER (unit, latent) COLUMN -- max over t of |got - ref| over the column's own max |ref|; dmu on the column's mu
scale -- at the stage tolerance 1e-9 after one sweep and after three (the last sweep has its own instantiations).  Every
unit is compared; sets of many units repeat 7 distinct ones (7 is coprime to 4 and 64: every lane and tail position holds a
known unit), two cases hold all-distinct units.  test_every_case_is_well_conditioned checks on the oracle alone that one
ulp on every mu moves no column by more than a tenth of the tolerance.

Not reachable: rank 1 beside a rank-14 latent (rank 1 needs T <= 2), so rank 1 runs in the RTOP = 13 instantiation only.

Measured on an MI355X (profiles/estep_shapes/measured_errors.txt, every case): mu 1.6e-10, dmu 1.6e-10 (both case
e-distinct130, 130 distinct units), v 1.8e-11, w 8.0e-12 at worst; nothing was found wrong.
"""
import functools
import zlib

import numpy as np
import pytest

from oracle import vlgp_oracle as O
from test_gpu_rates import STAGE

gpu = pytest.mark.gpu  # per test: the matrix and conditioning checks run without a GPU

SWEEPS = (1, 3)
RANK = 50
SWITCHES = ("VLGP_ESTEP_SPLIT", "VLGP_ESTEP_LSPLIT", "VLGP_ESTEP_LANEPT", "VLGP_ESTEP_NO_SHARED_G", "VLGP_ESTEP_MIX",
            "VLGP_ESTEP_LANES", "VLGP_ESTEP_GENERIC")
SWITCH_DEFAULT = {"VLGP_ESTEP_SPLIT": -1.0, "VLGP_ESTEP_LSPLIT": -1.0, "VLGP_ESTEP_LANEPT": -1.0, "VLGP_ESTEP_NO_SHARED_G": 0.0,
                  "VLGP_ESTEP_MIX": -1.0, "VLGP_ESTEP_LANES": 0.0, "VLGP_ESTEP_GENERIC": 0.0}
T_EDGES = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 49, 50, 63, 64)
M_LANE = (1, 2, 63, 64, 65, 127, 128, 129, 200)
M_WAVE = (1, 3, 4, 5, 8, 9)
LANE_RANK_CASES = (4, 6, 8, 9, 10, 11, 12, 13, 14)  # esplit_lane_body: a rank runs in the smallest case that holds it
LANE_RMAX = 14


# ------------------------------------------------------------------ ranks fixed on the host
@functools.lru_cache(maxsize=None)
def rank_at(T, log_omega):
    return int(np.any(O.ichol_gauss(T, 10.0 ** log_omega, RANK) != 0, axis=0).sum())


@functools.lru_cache(maxsize=None)
def omega_for(T, r):
    """An omega at which ichol_gauss(T, omega, 50) builds exactly r columns: bisection (the rank grows with omega), then a
    scan of the last bracket where it is not monotone."""
    lo, hi = -7.0, 1.5
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        k = rank_at(T, mid)
        if k == r:
            return 10.0 ** mid
        lo, hi = (mid, hi) if k < r else (lo, mid)
    for x in np.linspace(-7.0, 1.5, 400):
        if rank_at(T, float(x)) == r:
            return 10.0 ** float(x)
    raise AssertionError("no omega gives rank %d at T = %d" % (r, T))


def ranks_near(T, cap=LANE_RMAX):
    """Five ranks for a window of T bins: the largest possible up to `cap`, the one below, the middle, and the lowest."""
    if T == 1:
        return [1] * 5
    if T == 2:
        return [2, 1, 2, 1, 2]
    low = 3 if T == 64 else 2
    hi = min(T, cap)
    return [hi, max(low, hi - 1), max(low, (hi + 1) // 2), low, min(hi, low + 1)]


# ------------------------------------------------------------------ what a case expects to be planned
def lt_split(L):
    return 3 if L <= 3 else 5 if L <= 5 else 8 if L <= 8 else 10


def expected_lanes(M, want, lane_latents):
    """plan_estep_split's rule as the cases state it: a part is at least 64 units (lane-per-task latents) or 8, cuts at
    multiples of 64 or 4."""
    n = want if want else 1
    while n > 1 and M < (64 if lane_latents else 8) * n:
        n -= 1
    cm = 63 if lane_latents else 3
    cuts = [min(M, (M * h // n + cm) & ~cm) for h in range(n)] + [M]
    return n, cuts


def expected_plan(c, ranks):
    """The plan a case names, from its sizes, ranks (per latent, the largest over the set's priors) and switches."""
    env, N, L = c["env"], c["N"], c["L"]
    what = c["what"]
    if c["family"] == "fast":
        rmax = max(ranks)
        return dict(family="fast", LT=lt_split(L), RP=16 if rmax <= 16 else 32, RA=16 if rmax <= 16 else 24 if rmax <= 24 else 32)
    if c["family"] == "generic":
        return dict(family="generic", small=1,
                    LT=next(lt for lt in (2, 3, 5, 8, 10, 16, 32, 64) if L <= lt))
    if c["family"] == "long":
        return dict(family="long")
    uniform = len(set(c["lengths"])) == 1
    prior = what != "update_w"
    if not prior:
        ranks = [0] * L
    rmax = max(ranks)
    exp = dict(decline="taken", LT=lt_split(L), REC=(2 * lt_split(L) + 4) & ~1, CS=4 if N >= 64 else 2 if N >= 32 else 1,
               NJ=(0 if N > 128 else 4 if N <= 64 else 8) if what == "estep" else -1)
    if c["family"] == "long_split":
        exp.update(family="long_split", n_lanes=1, cuts=[0, c["M"]])
        return exp
    use_lane = prior and uniform and env.get("VLGP_ESTEP_LANEPT") != "0" and "VLGP_ESTEP_NO_SHARED_G" not in env
    classes = ["lane" if use_lane and r <= LANE_RMAX else "lo" if r <= 16 else "hi" for r in ranks]
    mix_on = env.get("VLGP_ESTEP_MIX") != "0"
    if mix_on and "lane" in classes and ("lo" in classes or "hi" in classes):
        classes = ["lo" if k == "lane" and r == 14 else k for k, r in zip(classes, ranks)]
    mix = mix_on and "lane" in classes and ("lo" in classes or "hi" in classes)
    maxra = 16 if rmax <= 16 else 20 if rmax <= 20 else 24 if rmax <= 24 else 32
    lane_ranks = [r for k, r in zip(classes, ranks) if k == "lane"]
    n_lanes, cuts = expected_lanes(c["M"], int(env.get("VLGP_ESTEP_LANES", 0)), bool(lane_ranks))
    exp.update(family="split_mixed" if mix else "split", maxra=maxra, use_lane=int(use_lane), classes=classes, mix=int(mix),
               ranks=list(ranks),
               maxra_hi=(max(20, maxra) if mix else maxra) if ("hi" in classes or mix) else 0,
               rtop=0 if not lane_ranks else 13 if mix or max(lane_ranks) <= 13 else 14,
               lo_shared_g=int("lo" in classes and not mix and prior and uniform and "VLGP_ESTEP_NO_SHARED_G" not in env),
               n_lanes=n_lanes, cuts=cuts)
    return exp


def gauss_edges(N):
    """Gaussian channels at the first, the last and the wave-edge positions."""
    return tuple(sorted({n for n in (0, 63, 64, 127, 128, N - 1) if 0 <= n < N}))


def case(cid, ranks=None, T=50, M=7, N=24, P=1, gauss=None, env=None, lengths=None, distinct=7, family=None, what="estep",
         vb=True, omegas=None, L=None, forced=True):
    lengths = list(lengths) if lengths is not None else [T] * M
    M = len(lengths)
    uniform = len(set(lengths)) == 1
    L = len(ranks) if ranks is not None else (L if L is not None else len(omegas))
    e = dict(env or {})
    if forced and "VLGP_ESTEP_GENERIC" not in e:
        e.setdefault("VLGP_ESTEP_SPLIT", "1")
    if gauss is None:
        gauss = (1, 9, 14, 22) if N == 24 else gauss_edges(N)
    gauss = tuple(sorted(set(g for g in gauss if 0 <= g < N)))
    if family is None:
        family = "split"
    distinct = min(distinct, M) if uniform else M
    c = dict(id=cid, ranks=list(ranks) if ranks is not None else None, lengths=lengths, M=M, N=N, L=L, P=P, gauss=gauss, env=e,
             distinct=distinct, family=family, what=what, vb=vb, omegas=omegas, T=lengths[0] if uniform else None)
    if ranks is not None:
        assert uniform, cid
        c["expect"] = expected_plan(c, ranks)
    else:
        c["expect"] = None  # ragged or given omegas: the ranks come from the oracle's priors (expectation(c))
    return c


def build_matrix():
    m = []
    S13 = ([2, 3, 4, 5, 6], [7, 8, 9, 10, 11], [12, 13, 3, 9, 6])
    S14 = ([2, 3, 4, 5, 14], [7, 8, 9, 10, 14], [6, 11, 12, 13, 14])
    # a. lane-per-task: every rank in the RTOP = 13 and in the RTOP = 14 instantiation (a rank-14 latent in an all-lane launch
    # selects the latter); M = 70: one full group of 64 units and a tail of 6
    for i, r in enumerate(S13):
        m.append(case("a-rtop13-%d" % i, r, M=70))
    for i, r in enumerate(S14):
        m.append(case("a-rtop14-%d" % i, r, M=70))
    m.append(case("a-rank14-alone", [14], M=70))
    m.append(case("a-rank1-T2", [1] * 5, T=2, M=70))
    m.append(case("a-rank1-T1", [1] * 5, T=1, M=70))
    m.append(case("a-distinct70", [14, 13, 9, 6, 2], M=70, distinct=70))
    # b. wave-per-task: every rank 15 ... 32 (each class with odd and even ranks and its top), and 2 ... 14 in the class-16
    # launch with G shared per workgroup (LANEPT=0) and staged per wave (NO_SHARED_G=1)
    for r in ([15, 16, 15, 16, 15], [17, 18, 19, 20, 17], [21, 22, 23, 24, 21], [25, 26, 27, 28, 25], [29, 30, 31, 32, 29]):
        m.append(case("b-ranks%d-%d" % (min(r), max(r)), r, M=9, env={"VLGP_ESTEP_LANEPT": "0"}))
    for i, r in enumerate(S13[:2] + ([12, 13, 14, 3, 8],)):
        m.append(case("b-lo-sharedg-%d" % i, r, M=9, env={"VLGP_ESTEP_LANEPT": "0"}))
        m.append(case("b-lo-owng-%d" % i, r, M=9, env={"VLGP_ESTEP_NO_SHARED_G": "1"}))
    m.append(case("b-ranks15-16-owng", [15, 16, 15, 16, 15], M=9, env={"VLGP_ESTEP_NO_SHARED_G": "1"}))
    # c. mixed launches: lane ranks <= 13 beside rank 14, 15, 16 latents that ride with the waves, at each hi class; and the
    # separate launches (MIX=0)
    for tag, r in (("20", [5, 9, 13, 14, 18]), ("24", [4, 11, 15, 16, 22]), ("32", [6, 12, 14, 16, 29]), ("20-nohi", [3, 10, 13, 15, 16])):
        m.append(case("c-mix%s" % tag, r, M=70))
        m.append(case("c-mix%s-off" % tag, r, M=70, env={"VLGP_ESTEP_MIX": "0"}))
    # d. window lengths, a rank at min(T, 14) in each: lane-per-task (M = 66: a full group and a tail), wave-per-task with
    # shared G (M = 9), the fast kernel (default dispatch, M = 5)
    for T in T_EDGES:
        m.append(case("d-T%d-lane" % T, ranks_near(T), T=T, M=66))
        m.append(case("d-T%d-wave" % T, ranks_near(T), T=T, M=9, env={"VLGP_ESTEP_LANEPT": "0"}))
        m.append(case("d-T%d-fast" % T, ranks_near(T), T=T, M=5, forced=False, family="fast"))
    m.append(case("d-T64-wave-hi", [32, 25, 17, 16, 3], T=64, M=9, env={"VLGP_ESTEP_LANEPT": "0"}))
    # e. unit counts: the 64-unit groups of the lane launch, the 4-unit groups of the shared-G launch, stream lanes
    for M in M_LANE:
        m.append(case("e-M%d-lane" % M, [14, 11, 8, 5, 2], M=M))
    m.append(case("e-distinct130", [13, 10, 7, 4, 2], M=130, distinct=130))
    for M in M_WAVE:
        m.append(case("e-M%d-wave" % M, [16, 15, 12, 7, 2], M=M, env={"VLGP_ESTEP_LANEPT": "0"}))
    for lanes in (2, 3, 4):
        for M in (129, 130, 192, 200):
            m.append(case("e-M%d-lane-lanes%d" % (M, lanes), [14, 11, 8, 5, 2], M=M, env={"VLGP_ESTEP_LANES": str(lanes)}))
        for M in (9, 16, 17):
            m.append(case("e-M%d-wave-lanes%d" % (M, lanes), [16, 15, 12, 7, 2], M=M,
                          env={"VLGP_ESTEP_LANEPT": "0", "VLGP_ESTEP_LANES": str(lanes)}))
    # (the M above give at most three lanes: a part is at least 64 or 8 units.  Four lanes need M >= 256 or 32)
    m.append(case("e-M256-lane-lanes4", [14, 11, 8, 5, 2], M=256, env={"VLGP_ESTEP_LANES": "4"}))
    m.append(case("e-M32-wave-lanes4", [16, 15, 12, 7, 2], M=32, env={"VLGP_ESTEP_LANEPT": "0", "VLGP_ESTEP_LANES": "4"}))
    # f. ragged sets: no single prior, so neither lane launches nor shared G; the long split
    om5 = [3e-3, 8e-3, 1.7e-2, 1e-3, 3e-2]
    m.append(case("f-ragged", lengths=[1, 2, 63, 64, 17, 50, 33, 2, 64], omegas=om5))
    m.append(case("f-ragged-hi", lengths=[64, 1, 50, 63, 2, 31], omegas=[3.5e-2, 8e-3, 2.2e-2, 1e-3, 3e-2]))
    m.append(case("f-ragged-Tmax65", lengths=[1, 2, 63, 64, 65, 50], omegas=om5, env={"VLGP_ESTEP_LSPLIT": "1"}, family="long_split"))
    for T in (65, 128, 129):
        m.append(case("f-T%d-lsplit" % T, lengths=[T] * 3, omegas=om5, env={"VLGP_ESTEP_LSPLIT": "1"}, family="long_split"))
    # g. channels (CS 1 | 2 | 4 at 32, 64; NJ 4 | 8 | lane-per-row at 64, 128), latents (LT 3, 5, 8, 10 exact and padded),
    # regressors (the HASXB passes) on either side of N = 64
    for N in (1, 15, 16, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1024):
        m.append(case("g-N%d" % N, [13, 9, 6, 4, 2], N=N, M=9))
    m.append(case("g-N24-allgauss", [13, 9, 6, 4, 2], N=24, M=9, gauss=range(24)))
    m.append(case("g-N1025-declined", [13, 9, 6, 4, 2], N=1025, M=3, family="fast"))
    for L in range(1, 11):
        m.append(case("g-L%d" % L, ([13, 2, 9, 14, 6, 11, 4, 8, 12, 3] * 2)[:L], M=9))
        m.append(case("g-L%d-wave" % L, ([16, 2, 9, 15, 6, 11, 4, 8, 12, 3] * 2)[:L], M=9, env={"VLGP_ESTEP_LANEPT": "0"}))
    for N in (33, 100):
        m.append(case("g-N%d-P2" % N, [13, 9, 6, 4, 2], N=N, P=2, M=9))
        m.append(case("g-N%d-P2-mix" % N, [13, 9, 6, 14, 18], N=N, P=2, M=9))
    # h. vb off (the last sweep factors nothing), update_w and update_v alone
    m.append(case("h-novb-lane", S14[2], M=70, vb=False))
    m.append(case("h-novb-wave", [17, 18, 19, 20, 17], M=9, vb=False, env={"VLGP_ESTEP_LANEPT": "0"}))
    m.append(case("h-novb-T64-lane", ranks_near(64), T=64, M=66, vb=False))
    m.append(case("h-novb-T3-wave", ranks_near(3), T=3, M=9, vb=False, env={"VLGP_ESTEP_LANEPT": "0"}))
    for what in ("update_w", "update_v"):
        m.append(case("h-%s-lane" % what, S14[2], M=70, what=what))
        m.append(case("h-%s-mix" % what, [5, 9, 13, 14, 18], M=70, what=what))
        m.append(case("h-%s-wave" % what, [29, 30, 31, 32, 16], M=9, what=what, env={"VLGP_ESTEP_LANEPT": "0"}))
        m.append(case("h-%s-fast" % what, [13, 9, 6, 4, 2], M=5, what=what, forced=False, family="fast"))
    # i. the fast kernel at LT x RA (nine or ten latents: RA = 16 only, declined above), the generic kernel on a slice
    for L in (3, 5, 8, 10):
        for top in (16, 23, 30):
            fam = "generic" if L > 8 and top > 16 else "fast"
            m.append(case("i-fast-L%d-r%d" % (L, top), ([top, 2, 9, 14, 6, 11, 4, 8, 12, 3])[:L], M=5, forced=False, family=fam))
    gen = {"VLGP_ESTEP_GENERIC": "1"}
    m.append(case("i-generic-ranks", [14, 13, 18, 29, 2], M=5, env=gen, family="generic"))
    for T in (1, 2, 3, 33, 64):
        m.append(case("i-generic-T%d" % T, ranks_near(T), T=T, M=5, env=gen, family="generic"))
    for N in (1, 64, 129):
        m.append(case("i-generic-N%d" % N, [13, 9, 6, 4, 2], N=N, M=5, env=gen, family="generic"))
    for L in (2, 3, 8, 16, 17):  # (with the cases above: LT 2, 3, 5, 8, 16, 32; i-fast-L10-r23 declines to LT 10)
        m.append(case("i-generic-L%d" % L, ([13, 2, 9, 14, 6, 11, 4, 8, 12, 3] * 2)[:L], M=5, env=gen, family="generic"))
    # LT 64; T = 8 keeps 33 latents' state within the LDS form (SMALL) the other generic cases run
    m.append(case("i-generic-L33", ([8, 2, 5, 3, 7, 4, 6] * 5)[:33], T=8, M=5, env=gen, family="generic"))
    return m


# Cases whose first draw of the data was ill conditioned ON THE ORACLE (test_every_case_is_well_conditioned: one ulp on mu
# moved a column by more than 1e-10): they draw again with this salt in the seed.
SALT = {"d-T33-fast": 1, "e-distinct130": 3, "e-M192-lane-lanes3": 1, "e-M256-lane-lanes4": 1, "e-M9-wave-lanes4": 1, "g-L4": 1, "i-fast-L3-r30": 1}

MATRIX = build_matrix()
assert len({c["id"] for c in MATRIX}) == len(MATRIX)
BY_ID = {c["id"]: c for c in MATRIX}
IDS = [c["id"] for c in MATRIX]


# ------------------------------------------------------------------ problems and references
def make_problem(c):
    """Data on the model of _random_problem (tests/test_gpu_parity.py): loadings 0.4 randn (scaled by 5 / L above ten
    latents), b about log 0.3, smooth latents, rates capped at e^3, w and v consistent with mu.  `distinct` units; unit m of
    the set is distinct[m % distinct]."""
    N, L, P = c["N"], c["L"], c["P"]
    rng = np.random.default_rng(zlib.crc32(("%s:%d" % (c["id"], SALT.get(c["id"], 0))).encode()))
    a = 0.4 * rng.standard_normal((L, N))
    if L > 10:
        a *= 5.0 / L
    if N > 32:  # w sums a^2 over the channels: keep it in the range of the N = 24 cases (the sweeps amplify rounding with it)
        a *= np.sqrt(32.0 / N)
    b = np.log(0.3) + 0.2 * rng.standard_normal((P, N))
    noise = 0.5 + rng.random(N)
    gauss = np.zeros(N, dtype=bool)
    gauss[list(c["gauss"])] = True
    sigma = 0.8 + 0.4 * rng.random(L)
    if c["omegas"] is not None:
        omega = np.array(c["omegas"], dtype=float)
    else:
        omega = np.array([omega_for(c["T"], r) for r in c["ranks"]])
    chol = O.build_prior(c["lengths"], omega, sigma, RANK)
    units = []
    for T in c["lengths"][:c["distinct"]]:
        z = np.stack([np.sin(np.linspace(0, (2 + l) * np.pi, T) + rng.random() * 6) for l in range(L)], 1)
        x = np.ones((T, P, N))
        if P > 1:
            x[:, 1:, :] = 0.3 * rng.standard_normal((T, P - 1, N))
        eta = z @ a + np.einsum("tpn,pn->tn", x, b)
        y = rng.poisson(np.exp(np.minimum(eta, 3))).astype(float)
        y[:, gauss] = eta[:, gauss] + 0.7 * rng.standard_normal((T, int(gauss.sum())))
        u = {"y": y, "x": x, "mu": z + 0.3 * rng.standard_normal((T, L))}
        u["w"] = O.curvature_unit(y, x, u["mu"], np.zeros_like(u["mu"]), a, b, noise, gauss)
        u["v"] = O.variance_unit(u["w"], np.zeros_like(u["mu"]), chol[T])[0]
        units.append(u)
    host_ranks = {T: [int(np.any(G[l] != 0, axis=0).sum()) for l in range(L)] for T, G in chol.items()}
    return dict(a=a, b=b, noise=noise, gauss=gauss, omega=omega, sigma=sigma, chol=chol, units=units, ranks=host_ranks)


def reference(c, p, units, n_iter):
    """Per unit (mu, v, w, dmu) as the oracle has them after the case's call; None where the call leaves a field alone."""
    out = []
    for u in units:
        G = p["chol"][u["y"].shape[0]]
        if c["what"] == "estep":
            mu, v, w, dmu, bad = O.estep_unit(u["y"], u["x"], u["mu"], u["v"], u["w"], p["a"], p["b"], p["noise"], p["gauss"], G,
                                              n_iter, vb=c["vb"])
            assert bad == 0
            out.append(dict(mu=mu, v=v, w=w, dmu=dmu))
        elif c["what"] == "update_w":
            out.append(dict(w=O.curvature_unit(u["y"], u["x"], u["mu"], u["v"], p["a"], p["b"], p["noise"], p["gauss"])))
        else:
            out.append(dict(v=O.variance_unit(u["w"], u["v"], G)[0]))
    return out


def sweeps_of(c):
    return SWEEPS if c["what"] == "estep" else (0,)


_cache = {}


def problem_and_reference(cid):
    """Computed once per case, shared, read-only."""
    if cid not in _cache:
        c = BY_ID[cid]
        p = make_problem(c)
        want = {n: reference(c, p, p["units"], n) for n in sweeps_of(c)}
        for u in p["units"] + [r for rs in want.values() for r in rs]:
            for arr in u.values():
                arr.setflags(write=False)
        _cache[cid] = (p, want)
    return _cache[cid]


def expectation(c, p):
    """The case's expected plan: stated with its ranks, or (ragged sets, given omegas) from the oracle's priors."""
    if c["expect"] is not None:
        return c["expect"]
    L = c["L"]
    return expected_plan(c, [max(p["ranks"][T][l] for T in p["ranks"]) for l in range(L)])


def column_errors(got, ref):
    """Per latent column of one unit: max_t |got - ref| over the column's max |ref|; dmu on the column's mu scale."""
    out = {}
    for k, r in ref.items():
        scale = np.abs(ref["mu"] if k == "dmu" else r).max(axis=0)
        out[k] = np.abs(got[k] - r).max(axis=0) / np.maximum(scale, 1e-300)
    return out


# ------------------------------------------------------------------ without a GPU
def test_matrix_names_every_compiled_case():
    """From the plans the cases expect (the GPU tests assert the device agrees)."""
    split = [c for c in MATRIX if c["expect"] and c["expect"]["family"] in ("split", "split_mixed") and c["what"] == "estep"]
    lane_case = lambda r: next(k for k in LANE_RANK_CASES if r <= k)
    reached = {(lane_case(r), c["expect"]["rtop"]) for c in split for r, k in zip(c["ranks"], c["expect"]["classes"])
               if k == "lane"}
    assert reached == {(k, t) for k in LANE_RANK_CASES for t in (13, 14) if k <= t}, reached
    lane_ranks = {(r, c["expect"]["rtop"]) for c in split if not c["expect"]["mix"]
                  for r, k in zip(c["ranks"], c["expect"]["classes"]) if k == "lane"}
    assert lane_ranks >= {(r, 13) for r in range(1, 14)} | {(r, 14) for r in range(2, 15)}
    # wave classes: the launch a latent rides in (16 for lo; maxra_hi for hi and for lo in a mixed launch)
    wave = set()
    for c in split:
        e = c["expect"]
        for r, k in zip(c["ranks"], e["classes"]):
            if k != "lane":
                cls = 16 if k == "lo" and not e["mix"] else e["maxra_hi"]
                wave.add((cls, r % 2, r == cls))
    assert wave >= {(cls, odd, top) for cls in (16, 20, 24, 32) for odd, top in ((1, False), (0, False), (0, True))}, wave
    plain = {r for c in split if not c["expect"]["mix"] for r, k in zip(c["ranks"], c["expect"]["classes"]) if k != "lane"}
    assert plain >= set(range(2, 33))
    for shared in (0, 1):  # ranks 2 ... 14 in the class-16 launch, G shared and per wave
        lo = {r for c in split if c["expect"]["lo_shared_g"] == shared and not c["expect"]["mix"]
              for r, k in zip(c["ranks"], c["expect"]["classes"]) if k == "lo"}
        assert lo >= set(range(2, 17)), (shared, lo)
    assert {c["expect"]["maxra_hi"] for c in split if c["expect"]["mix"]} == {20, 24, 32}
    assert {c["expect"]["maxra_hi"] for c in split if not c["expect"]["mix"]} >= {0, 20, 24, 32}
    assert {(c["expect"]["LT"], c["L"] == c["expect"]["LT"]) for c in split} == {(lt, ex) for lt in (3, 5, 8, 10) for ex in (False, True)}
    assert {(c["expect"]["CS"], c["expect"]["NJ"]) for c in split} == {(1, 4), (2, 4), (4, 4), (4, 8), (4, 0)}
    assert {c["N"] for c in split} >= {1, 15, 16, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1024}
    fast = [c["expect"] for c in MATRIX if c["expect"] and c["expect"]["family"] == "fast"]
    assert {(e["LT"], e["RA"]) for e in fast} == {(lt, ra) for lt in (3, 5, 8) for ra in (16, 24, 32)} | {(10, 16)}
    assert {c["expect"]["LT"] for c in MATRIX if c["family"] == "generic"} == {2, 3, 5, 8, 10, 16, 32, 64}
    for path, fam in (("lane", "split"), ("wave", "split"), ("fast", "fast")):
        ts = {c["T"] for c in MATRIX if c["id"].startswith("d-T") and c["id"].endswith(path) and c["expect"]["family"] == fam}
        assert ts == set(T_EDGES), (path, ts)
    for c in MATRIX:
        if c["id"].startswith("d-T") and c["T"] > 2:
            assert max(c["ranks"]) == min(c["T"], LANE_RMAX) or c["id"] == "d-T64-wave-hi"
    assert {c["M"] for c in split if c["id"].startswith("e-M") and c["id"].endswith("-lane")} == set(M_LANE)
    assert {c["M"] for c in split if c["id"].startswith("e-M") and c["id"].endswith("-wave")} == set(M_WAVE)
    for c in split:  # stream lanes: no part is empty, cuts on the workgroup's unit count
        e = c["expect"]
        step = 64 if "lane" in e["classes"] else 4
        assert all(b > a for a, b in zip(e["cuts"], e["cuts"][1:])) and all(x % step == 0 for x in e["cuts"][1:-1]), c["id"]
    assert {(c["M"], c["expect"]["n_lanes"]) for c in split if "-lane-lanes" in c["id"]} >= {(129, 2), (192, 3), (200, 3), (256, 4)}
    assert {(c["M"], c["expect"]["n_lanes"]) for c in split if "-wave-lanes" in c["id"]} >= {(9, 1), (16, 2), (17, 2), (32, 4)}
    assert BY_ID["e-M256-lane-lanes4"]["expect"]["cuts"] == [0, 64, 128, 192, 256]
    assert BY_ID["e-M32-wave-lanes4"]["expect"]["cuts"] == [0, 8, 16, 24, 32]
    assert {c["distinct"] for c in MATRIX if c["id"] in ("a-distinct70", "e-distinct130")} == {70, 130}
    assert {c["vb"] for c in MATRIX} == {True, False} and {c["what"] for c in MATRIX} == {"estep", "update_w", "update_v"}


# What the device reported (Engine.estep_plan) for one case of each distinct shape of plan, written out: expected_plan
# above derives every case's expectation from plan_estep_split's rules as the cases state them, and these pin it.
LITERAL_PLANS = {
    "a-rtop14-0": dict(family="split", decline="taken", LT=5, REC=14, maxra=16, use_lane=1, mix=0, maxra_hi=0, rtop=14,
        lo_shared_g=0, n_lanes=1, cuts=[0, 70], CS=1, NJ=4, ranks=[2, 3, 4, 5, 14], classes=["lane", "lane", "lane", "lane",
        "lane"]),
    "c-mix20": dict(family="split_mixed", decline="taken", LT=5, REC=14, maxra=20, use_lane=1, mix=1, maxra_hi=20, rtop=13,
        lo_shared_g=0, n_lanes=1, cuts=[0, 70], CS=1, NJ=4, ranks=[5, 9, 13, 14, 18], classes=["lane", "lane", "lane", "lo",
        "hi"]),
    "c-mix20-off": dict(family="split", decline="taken", LT=5, REC=14, maxra=20, use_lane=1, mix=0, maxra_hi=20, rtop=14,
        lo_shared_g=0, n_lanes=1, cuts=[0, 70], CS=1, NJ=4, ranks=[5, 9, 13, 14, 18], classes=["lane", "lane", "lane", "lane",
        "hi"]),
    "c-mix24": dict(family="split_mixed", decline="taken", LT=5, REC=14, maxra=24, use_lane=1, mix=1, maxra_hi=24, rtop=13,
        lo_shared_g=0, n_lanes=1, cuts=[0, 70], CS=1, NJ=4, ranks=[4, 11, 15, 16, 22], classes=["lane", "lane", "lo", "lo",
        "hi"]),
    "b-ranks17-20": dict(family="split", decline="taken", LT=5, REC=14, maxra=20, use_lane=0, mix=0, maxra_hi=20, rtop=0,
        lo_shared_g=0, n_lanes=1, cuts=[0, 9], CS=1, NJ=4, ranks=[17, 18, 19, 20, 17], classes=["hi", "hi", "hi", "hi", "hi"]),
    "b-lo-owng-2": dict(family="split", decline="taken", LT=5, REC=14, maxra=16, use_lane=0, mix=0, maxra_hi=0, rtop=0,
        lo_shared_g=0, n_lanes=1, cuts=[0, 9], CS=1, NJ=4, ranks=[12, 13, 14, 3, 8], classes=["lo", "lo", "lo", "lo", "lo"]),
    "e-M200-lane-lanes3": dict(family="split", decline="taken", LT=5, REC=14, maxra=16, use_lane=1, mix=0, maxra_hi=0, rtop=14,
        lo_shared_g=0, n_lanes=3, cuts=[0, 128, 192, 200], CS=1, NJ=4, ranks=[14, 11, 8, 5, 2], classes=["lane", "lane", "lane",
        "lane", "lane"]),
    "e-M17-wave-lanes2": dict(family="split", decline="taken", LT=5, REC=14, maxra=16, use_lane=0, mix=0, maxra_hi=0, rtop=0,
        lo_shared_g=1, n_lanes=2, cuts=[0, 8, 17], CS=1, NJ=4, ranks=[16, 15, 12, 7, 2], classes=["lo", "lo", "lo", "lo",
        "lo"]),
    "e-M256-lane-lanes4": dict(family="split", decline="taken", LT=5, REC=14, maxra=16, use_lane=1, mix=0, maxra_hi=0, rtop=14,
        lo_shared_g=0, n_lanes=4, cuts=[0, 64, 128, 192, 256], CS=1, NJ=4, ranks=[14, 11, 8, 5, 2], classes=["lane", "lane",
        "lane", "lane", "lane"]),
    "f-ragged": dict(family="split", decline="taken", LT=5, REC=14, maxra=32, use_lane=0, mix=0, maxra_hi=32, rtop=0,
        lo_shared_g=0, n_lanes=1, cuts=[0, 9], CS=1, NJ=4, ranks=[11, 16, 22, 8, 29], classes=["lo", "lo", "hi", "lo", "hi"]),
    "f-T65-lsplit": dict(family="long_split", decline="taken", LT=5, REC=14, maxra=32, use_lane=0, mix=0, maxra_hi=0, rtop=0,
        lo_shared_g=0, n_lanes=1, cuts=[0, 3], CS=1, NJ=4, ranks=[11, 17, 24, 8, 29], classes=["lo", "hi", "hi", "lo", "hi"]),
    "g-N129": dict(family="split", decline="taken", LT=5, REC=14, maxra=16, use_lane=1, mix=0, maxra_hi=0, rtop=13,
        lo_shared_g=0, n_lanes=1, cuts=[0, 9], CS=4, NJ=0, ranks=[13, 9, 6, 4, 2], classes=["lane", "lane", "lane", "lane",
        "lane"]),
    "g-N100-P2-mix": dict(family="split_mixed", decline="taken", LT=5, REC=14, maxra=20, use_lane=1, mix=1, maxra_hi=20,
        rtop=13, lo_shared_g=0, n_lanes=1, cuts=[0, 9], CS=4, NJ=8, ranks=[13, 9, 6, 14, 18], classes=["lane", "lane", "lane",
        "lo", "hi"]),
    "h-update_w-mix": dict(family="split", decline="taken", LT=5, REC=14, maxra=16, use_lane=0, mix=0, maxra_hi=0, rtop=0,
        lo_shared_g=0, n_lanes=1, cuts=[0, 70], CS=1, NJ=-1, ranks=[0, 0, 0, 0, 0], classes=["lo", "lo", "lo", "lo", "lo"]),
    "i-fast-L8-r23": dict(family="fast", decline="small set", LT=8, RP=32, RA=24),
    "i-generic-L17": dict(family="generic", decline="VLGP_ESTEP_GENERIC", LT=32, small=1, rg=8),
}


def test_expected_plans_of_distinct_shapes_are_these_literals():
    for cid, literal in LITERAL_PLANS.items():
        c = BY_ID[cid]
        exp = expectation(c, problem_and_reference(cid)[0])
        assert exp == {k: literal[k] for k in exp}, (cid, exp, literal)
        if exp["family"] in ("split", "split_mixed"):  # (the other families' cases name fewer fields)
            assert set(exp) == set(literal), (cid, set(literal) - set(exp))


def test_plan_report_layout_is_the_headers():
    """Engine.estep_plan decodes the report with _lib.EP / ESPLIT / ECLASS: they are the header's VLGP_EP_*, VLGP_ESPLIT_*
    and VLGP_ECLASS_* (csrc/ctx.h asserts its own slots against the same defines when the library is compiled)."""
    import os
    import re

    from vlgp_amd import _lib
    from vlgp_amd.engine import Engine

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vlgp_hip.h")) as f:
        defs = {k: int(v) for k, v in re.findall(r"^#define (VLGP_\w+) (-?\d+)\b", f.read(), re.M)}
    group = lambda prefix: {k[len(prefix):]: v for k, v in defs.items() if k.startswith(prefix)}
    assert group("VLGP_EP_") == _lib.EP and defs["VLGP_ESTEP_PLAN_LEN"] == _lib.ESTEP_PLAN_LEN
    assert group("VLGP_ESPLIT_") == {k: i for i, k in enumerate(_lib.ESPLIT)}
    assert group("VLGP_ECLASS_") == {k: i for i, k in enumerate(_lib.ECLASS)}
    assert len(Engine.ESPLIT_DECLINES) == len(_lib.ESPLIT) and len(Engine.ECLASSES) == len(_lib.ECLASS)
    slots = sorted(_lib.EP.values())
    assert _lib.EP["CS"] - _lib.EP["CUT"] == 5 and _lib.EP["CLASS"] - _lib.EP["RANK"] == 16  # VLGP_E_LANES + 1 cuts, 16 latents
    assert _lib.ESTEP_PLAN_LEN == _lib.EP["CLASS"] + 16 and slots == sorted(set(slots))


@pytest.mark.parametrize("cid", IDS)
def test_every_case_is_well_conditioned(cid):
    """On the oracle alone: a random +-1 ulp perturbation of every mu moves no column of mu, v, w or dmu by more than a
    tenth of the tolerance, after one and after three sweeps; and the host's ranks are the ones the case names."""
    c = BY_ID[cid]
    p, want = problem_and_reference(cid)
    if c["ranks"] is not None:
        assert p["ranks"][c["T"]] == c["ranks"], (cid, p["ranks"])
    rng = np.random.default_rng(1)
    moved = []
    for u in p["units"]:
        mv = dict(u)
        mv["mu"] = np.nextafter(u["mu"], np.where(rng.random(u["mu"].shape) < 0.5, -np.inf, np.inf))
        moved.append(mv)
    worst = {}
    for n in sweeps_of(c):
        for ref, mv in zip(want[n], reference(c, p, moved, n)):
            assert all(np.all(np.isfinite(r)) for r in ref.values())
            for k, e in column_errors(mv, ref).items():
                worst[(n, k)] = max(worst.get((n, k), 0.0), float(e.max()))
    print("estep-shapes %-26s one-ulp perturbation of mu: %s" % (cid, {k: "%.1e" % v for k, v in worst.items()}))
    assert max(worst.values()) < 0.1 * STAGE, (cid, worst)


# ------------------------------------------------------------------ on the device
@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture
def clean_env(monkeypatch):
    """The library reads its switches when a handle is created: every handle below is created after its case's setting."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def set_case_switches(c, env, extra=None):
    want = dict(SWITCH_DEFAULT)
    for name, value in list(c["env"].items()) + list((extra or {}).items()):
        env.setenv(name, value)
        want[name] = float(value)
    return want


def units_of(c, p):
    return [p["units"][m % c["distinct"]] for m in range(c["M"])]


def open_case(V, c, p, switches):
    """A handle holding the case's set, parameters and priors, its switches, ranks and (returned) plan asserted."""
    eng = V.Engine(c["N"], c["L"], c["P"], RANK, p["gauss"])
    try:
        for name, value in switches.items():
            assert eng.switch(name) == value, (c["id"], name)
        eng.set_params(p["a"], p["b"], p["noise"])
        eng.build_prior(sorted(set(c["lengths"])), p["omega"], p["sigma"])
        eng.upload(0, units_of(c, p))
        for T, ranks in p["ranks"].items():
            G, rk = eng.get_prior(T, with_rank=True)
            assert list(rk) == ranks and (c["ranks"] is None or ranks == c["ranks"]), (c["id"], T, list(rk), ranks)
            assert np.array_equal(G, p["chol"][T]), (c["id"], T)
    except BaseException:
        eng.close()
        raise
    return eng


def assert_plan(eng, c, p, n_iter):
    plan = eng.estep_plan(0, n_iter, what=c["what"], vb=c["vb"])
    for k, want in expectation(c, p).items():
        assert plan[k] == want, (c["id"], k, want, plan)
    if "cuts" in plan:
        assert plan["cuts"][0] == 0 and plan["cuts"][-1] == c["M"] and len(plan["cuts"]) == plan["n_lanes"] + 1
        assert all(b > a for a, b in zip(plan["cuts"], plan["cuts"][1:])), (c["id"], plan)  # no part is empty
    return plan


def run_case(V, c, p, n_iter, switches):
    """The case's call on a fresh handle: (per-unit dicts of mu, v, w, dmu, the plan)."""
    eng = open_case(V, c, p, switches)
    with eng:
        plan = assert_plan(eng, c, p, n_iter)
        if c["what"] == "estep":
            assert eng.estep(0, n_iter, vb=c["vb"]) == 0
        elif c["what"] == "update_w":
            eng.update_w(0)
        else:
            assert eng.update_v(0) == 0
        assert eng.last_estep_path == plan["family"], (c["id"], eng.last_estep_path, plan)
        got = eng.download(0)
    off = np.concatenate([[0], np.cumsum(c["lengths"])])
    return [{k: a[s:e] for k, a in got.items()} for s, e in zip(off[:-1], off[1:])], plan


def report_and_check(c, n_iter, got, want, plan=None):
    worst = {}
    for m, g in enumerate(got):
        ref = want[m % c["distinct"]]
        for k, e in column_errors(g, ref).items():
            assert e.shape == (c["L"],)
            worst[k] = max(worst.get(k, 0.0), float(e.max())) if np.all(np.isfinite(e)) else float("nan")
    print("estep-shapes %-26s sweeps %d  " % (c["id"], n_iter) + "  ".join("%s %.2e" % kv for kv in worst.items())
          + ("  plan %s" % plan if plan is not None else ""))
    for m, g in enumerate(got):
        ref = want[m % c["distinct"]]
        for k, e in column_errors(g, ref).items():
            assert np.all(e < STAGE), (c["id"], n_iter, k, m, int(np.argmax(e)), float(e.max()))  # (a NaN fails)
        for k in set(g) - set(ref):  # update_w / update_v leave the other fields as uploaded
            if k != "dmu":
                assert np.array_equal(g[k], units_of(c, _cache[c["id"]][0])[m][k]), (c["id"], k, m)


@gpu
def test_plan_entry_validates_and_reports(V, clean_env):
    c = BY_ID["c-mix20"]
    p, _ = problem_and_reference(c["id"])
    with open_case(V, c, p, set_case_switches(c, clean_env)) as eng:
        with pytest.raises(V.VlgpError):
            eng.estep_plan(3, 2)  # an empty set
        with pytest.raises(V.VlgpError):
            eng.estep_plan(99, 2)  # no such set
        with pytest.raises(V.VlgpError):
            eng.estep_plan(0, -1)
        with pytest.raises(V.VlgpError):
            eng._ck(eng.lib.vlgp_debug_estep_plan(eng.h, 0, 15, 2, None))
        before = eng.download(0)
        plan = assert_plan(eng, c, p, 2)  # the handle is still usable; nothing ran
        assert eng.last_estep_path == "none"
        after = eng.download(0)
        assert all(np.array_equal(before[k], after[k]) for k in ("mu", "v", "w"))
        assert plan["classes"] == ["lane", "lane", "lane", "lo", "hi"] and plan["ranks"] == c["ranks"]
        assert eng.estep_plan(0, 0, what="update_w")["classes"] == ["lo"] * 5  # no prior in this mode: every rank is 0
        # a staged set runs one launch_estep per stage: there is no single plan, and the entry says so
        eng.set_overlaps(0, [0, 35, 70], np.zeros((0, 3), dtype=np.int32), [0, 0, 0])
        with pytest.raises(V.VlgpError):
            eng.estep_plan(0, 2)


@gpu
@pytest.mark.parametrize("cid", IDS)
def test_shapes_vs_oracle(V, cid, clean_env):
    """One case of the matrix: its switches, ranks and plan, then every column of every unit at 1e-9 after one sweep and
    after three (update_w / update_v: the one call)."""
    c = BY_ID[cid]
    p, want = problem_and_reference(cid)
    switches = set_case_switches(c, clean_env)
    for n_iter in sweeps_of(c):
        got, plan = run_case(V, c, p, n_iter, switches)
        if cid == "g-N1025-declined":
            assert plan["decline"] == "N > 1024"
        report_and_check(c, n_iter, got, want[n_iter], plan if n_iter == sweeps_of(c)[0] else None)


@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in MATRIX if "-lanes" in c["id"]])
def test_stream_lanes_equal_one_lane_bitwise(V, cid, clean_env):
    """The units are independent inside a call: the set cut over stream lanes gives, bit for bit, the one-lane result."""
    c = BY_ID[cid]
    p, want = problem_and_reference(cid)
    got, plan = run_case(V, c, p, 3, set_case_switches(c, clean_env))
    one = dict(c, env=dict(c["env"], VLGP_ESTEP_LANES="1"))
    one["expect"] = expected_plan(one, c["ranks"])
    ref, plan1 = run_case(V, one, p, 3, set_case_switches(one, clean_env))
    assert plan1["n_lanes"] == 1
    for g, r in zip(got, ref):
        for k in ("mu", "v", "w", "dmu"):
            assert np.array_equal(g[k], r[k]), (cid, k)


@gpu
@pytest.mark.parametrize("cid", ["c-mix24", "c-mix20-nohi"])
def test_mixed_launch_equals_separate_launches_bitwise(V, cid, clean_env):
    """Where no latent changes its kind of task (no rank-14 latent moves from a lane to a wave), the mixed launch and the
    separate ones (VLGP_ESTEP_MIX=0) do the same arithmetic per task."""
    on, off = BY_ID[cid], BY_ID[cid + "-off"]
    assert 14 not in on["ranks"] and on["ranks"] == off["ranks"]
    p, _ = problem_and_reference(cid)
    a, plan_on = run_case(V, on, p, 3, set_case_switches(on, clean_env))
    b, plan_off = run_case(V, off, p, 3, set_case_switches(off, clean_env))
    assert plan_on["family"] == "split_mixed" and plan_off["family"] == "split" and plan_on["classes"] == plan_off["classes"]
    for g, r in zip(a, b):
        for k in ("mu", "v", "w", "dmu"):
            assert np.array_equal(g[k], r[k]), (cid, k)
