"""The case table of tests/test_gpu_joint_em.py (vlgp_mstep_cov on the device against tests/joint_em_numpy.py), its problems
and their references, shared with tests/test_joint_em_host.py, which checks without a GPU that the table names every
compiled size and that every case is well conditioned.

csrc/mstep_cov.hip compiles mstep_cov_accum<LT, PT> for LT in {2, 3, 5, 8, 10} x PT in {1, 2, 4, 8}; the launch geometry is
plan()'s of csrc/mstep.hip (channel tiles, row slices, workgroups along the rows) with row tiles of MC_TILE rows of
(mu | cov) in LDS.  The PREP, noise, reduce and solve kernels are mstep.hip's, which tests/test_gpu_mstep_shapes.py walks.
"""
import os
import re

import numpy as np

import joint_em_numpy as EM
from test_gpu_mstep_shapes import LT_OF, PT_OF, FIXED_OF, CHANNEL_GEOMETRY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = (1, 3)
# rows of (mu | cov) per LDS tile: read from the source, so a retune moves the row cases with it
MC_TILE = int(re.search(r"#define MC_TILE (\d+)", open(os.path.join(ROOT, "vlgp_amd", "csrc", "mstep_cov.hip")).read()).group(1))
WG_ROWS = 64  # plan(): one workgroup along the rows per 64 rows, until the cap of one per compute unit binds

GEOMETRY = dict(CHANNEL_GEOMETRY)
GEOMETRY[130] = (130, 3, 448, 1)  # three slices of 130 lanes fill 448 threads best (390 / 448)

BASE = [50, 120, 64, 50, 50]  # 334 rows: 6 workgroups of 56 rows
SIX = (1, 4, 9, 13, 18, 23)   # Gaussian channels of the N = 24 cases
COVS = ("full", "rank1", "zero")


def ragged(total, tile):
    """Unit lengths summing to `total` whose interior boundaries fall on no multiple of `tile`."""
    out, left, k = [], total, 0
    while left > 0:
        t = min((37, 50, 23, 64, 41, 19)[k % 6], left)
        if t < left and (total - left + t) % tile == 0:
            t -= 1
        out.append(t)
        left -= t
        k += 1
    inner = np.cumsum(out)[:-1]
    assert sum(out) == total and not np.any(inner % tile == 0), out
    return out


def case(cid, N, L, lengths, P=1, gauss=(), cov="full", one_wg=False, G=None):
    gauss = tuple(sorted(set(g for g in gauss if 0 <= g < N)))
    CT, S, nthr, tiles = GEOMETRY[N]
    fixed = FIXED_OF.get(L, 0) if P == 1 else 0
    exp = dict(LT=LT_OF[L], PT=PT_OF[P], CT=CT, S=S, nthr=nthr, tiles=tiles, fixed=fixed,
               anyg=int(fixed == 0 or len(gauss) > 0), noise_passes=int(len(gauss) > 0 or P > 2))
    if G is not None:
        exp["G"] = G
    # (the keys test_gpu_mstep_shapes.set_case_switches and assert_plan read)
    return dict(id=cid, N=N, L=L, P=P, lengths=list(lengths), rows=int(sum(lengths)), gauss=gauss, cov=cov, one_wg=one_wg,
                G=G, generic=False, x_nonunit=False, all_gauss=len(gauss) == N, expect=exp)


def build_matrix():
    m = []
    # a. every latent bucket, exact and padded, x == 1: mixed likelihoods (both solve branches, sum_t C_t in the Gaussian
    # channels' Gram matrix, the noise by passes) and Poisson alone (the register-resident solves, the moments noise)
    for L in (1, 2, 3, 4, 5, 7, 8, 10):
        m.append(case("a-L%d-mixed" % L, 24, L, BASE, gauss=SIX))
    for L in (2, 3, 5, 8, 10):
        m.append(case("a-L%d-poisson" % L, 24, L, BASE))
    m.append(case("a-L5-allgauss", 24, 5, BASE, gauss=range(24)))
    m.append(case("a-L10-allgauss", 24, 10, BASE, gauss=range(24)))
    # b. regressor buckets with real regressors, exact and padded, at a small and a large latent bucket
    for L in (3, 7):
        for P in (2, 3, 8):
            m.append(case("b-L%d-P%d" % (L, P), 24, L, BASE, P=P))
    # ... and the rest of the LT x PT product, so that every compiled instantiation is launched (the PT = 4 and 8 ones of
    # LT = 2, 5, 10 have spill code of their own)
    for L, P in ((2, 2), (2, 8), (5, 3), (5, 8), (10, 2), (10, 3), (10, 8)):
        m.append(case("b-L%d-P%d" % (L, P), 24, L, BASE, P=P, gauss=SIX if (L, P) in ((5, 8), (10, 2)) else ()))
    m.append(case("b-L2-P3-mixed", 24, 2, BASE, P=3, gauss=SIX))
    m.append(case("b-L5-P2-mixed", 24, 5, BASE, P=2, gauss=SIX))
    # c. channel geometry: one channel, the wave edges, idle lanes beside three slices
    for N in (1, 63, 65, 130):
        m.append(case("c-N%d" % N, N, 3, [50, 37, 43], gauss=(0, N - 1) if N > 1 else ()))
    # d. the covariances: rank one, exactly zero (full with strong off-diagonals is every other case)
    for L in (3, 5, 8):
        for kind in ("rank1", "zero"):
            m.append(case("d-L%d-%s" % (L, kind), 24, L, BASE, gauss=SIX if L == 5 else (), cov=kind))
    # e. row geometry.  One row; the 64-row edges of the workgroup count; the LDS row tile in ONE workgroup: one below, at,
    # one above, and three tiles with a short last one; three workgroups along the rows, boundaries off the tile
    m.append(case("e-rows1", 20, 5, [1], G=1))
    for rows in (WG_ROWS - 1, WG_ROWS, WG_ROWS + 1):
        m.append(case("e-rows%d" % rows, 20, 5, ragged(rows, MC_TILE), G=-(-rows // WG_ROWS)))
    for rows in (MC_TILE - 1, MC_TILE, MC_TILE + 1, 2 * MC_TILE + 8):
        m.append(case("e-rows%d-onewg" % rows, 20, 5, ragged(rows, MC_TILE), one_wg=True, G=1, gauss=(3, 11)))
    m.append(case("e-rows%d-3wg" % (3 * WG_ROWS), 20, 5, ragged(3 * WG_ROWS, MC_TILE), G=3))
    m.append(case("e-rows%d-3wg-L10" % (3 * WG_ROWS - 5), 20, 10, ragged(3 * WG_ROWS - 5, MC_TILE), G=3, gauss=(3, 11)))
    return m


def compiled_buckets():
    """(LT values, PT values) the launchers of csrc/mstep_cov.hip dispatch to, read from their switch statements."""
    src = open(os.path.join(ROOT, "vlgp_amd", "csrc", "mstep_cov.hip")).read()
    lts = sorted(int(v) for v in re.findall(r"case \d+: return launch_cov_accum_p<(\d+)>", src))
    pts = sorted(int(v) for v in re.findall(r"case \d+: hipLaunchKernelGGL\(\(mstep_cov_accum<LT, (\d+)>\)", src))
    return lts, pts


MATRIX = build_matrix()
assert len({c["id"] for c in MATRIX}) == len(MATRIX)
BY_ID = {c["id"]: c for c in MATRIX}


def make_cov(kind, v, rng):
    """(rows, L, L) from per-row variances v (rows, L): 'full' = D (0.8 11' + 0.2 I) D with D = diag(+-sqrt(v)), correlations
    of +-0.8 between every pair; 'rank1' = u u' with u = +-sqrt(v); 'zero'."""
    rows, L = v.shape
    d = np.sqrt(v) * np.where(rng.random((rows, L)) < 0.5, -1.0, 1.0)
    outer = d[:, :, None] * d[:, None, :]
    if kind == "zero":
        return np.zeros((rows, L, L))
    if kind == "rank1":
        return outer
    return outer * (0.8 + 0.2 * np.eye(L))


def make_problem(c):
    """test_gpu_mstep_shapes.make_problem's data (smooth latents plus noise, regressors 0.3 randn beside the constant one)
    with a covariance per row whose variances are 0.02 ... 0.07, and a second (mu, v) that the set itself holds and that
    vlgp_mstep_cov must not read."""
    import test_gpu_mstep_shapes as MS

    p = MS.make_problem(c, seed=sum(map(ord, c["id"])))
    rng = np.random.default_rng(sum(map(ord, c["id"])) + 1)
    p["cov"] = np.ascontiguousarray(make_cov(c["cov"], p["v"], rng))
    p["set_mu"] = p["mu"] + 1.0 + rng.random(p["mu"].shape)
    p["set_v"] = 3.0 * p["v"]
    return p


_cache = {}


def problem_and_reference(cid):
    """The case's problem and the statement's (a, b, da, db, noise) per iteration count: computed once, shared, read-only."""
    if cid not in _cache:
        p = make_problem(BY_ID[cid])
        want = {n: EM.mstep_cov(p["y"], p["x"], p["mu"], p["cov"], p["a"], p["b"], p["gauss"], n) for n in ITERS}
        for arr in list(p.values()) + [w for ws in want.values() for w in ws]:
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _cache[cid] = (p, want)
    return _cache[cid]
