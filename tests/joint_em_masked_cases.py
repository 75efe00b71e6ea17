"""The case table of tests/test_gpu_joint_em_masked.py (vlgp_mstep_cov_masked on the device against
tests/joint_em_masked_numpy.py), its problems, masks and references, shared with tests/test_joint_em_masked_host.py, which
checks without a GPU that the table names every compiled size and that every case is well conditioned.

csrc/mstep_cov.hip compiles mstep_cov_accum_masked<LT, PT> for the matrix of the unmasked kernel, LT in {2, 3, 5, 8, 10} x
PT in {1, 2, 4, 8}, and launches it with that kernel's geometry (tests/joint_em_cases.py).  A lane reads the 32-bit half
of its row's mask word: the channel counts walk both halves of a word, a second and a third word.  All channels are
Poisson: a masked handle has no Gaussian channel.
"""
import numpy as np

import joint_em_cases as CS
import joint_em_masked_numpy as EMM
from test_gpu_mstep_shapes import FIXED_OF, LT_OF, PT_OF

ITERS = CS.ITERS
MC_TILE = CS.MC_TILE
# N -> (CT, S, nthr, tiles) of plan(): joint_em_cases' and the channel counts around a mask word's halves (the
# best-filled multiple of 64 threads, the smallest at a tie: 4 x 31 of 128, 4 x 32 of 128, 15 x 33 of 512)
GEOMETRY = dict(CS.GEOMETRY)
GEOMETRY.update({31: (31, 4, 128, 1), 32: (32, 4, 128, 1), 33: (33, 15, 512, 1)})
MASKS = ("random", "dead-channel", "dead-row", "dead-unit")
PADDED = {2: 1, 5: 4, 8: 7, 10: 9}  # L = LT - 1 (the bucket of three latents holds L = 3 alone: L = 2 is LT = 2's exact case)


def case(cid, N, L, lengths, P=1, cov="full", mask="random", one_wg=False, G=None):
    CT, S, nthr, tiles = GEOMETRY[N]
    fixed = FIXED_OF.get(L, 0) if P == 1 else 0
    # (what vlgp_debug_mstep_plan reports for the handle: noise_passes is the unmasked M-step's; the masked one always
    # takes the two passes)
    exp = dict(LT=LT_OF[L], PT=PT_OF[P], CT=CT, S=S, nthr=nthr, tiles=tiles, fixed=fixed, anyg=int(fixed == 0),
               noise_passes=int(P > 2))
    if G is not None:
        exp["G"] = G
    return dict(id=cid, N=N, L=L, P=P, lengths=list(lengths), rows=int(sum(lengths)), gauss=(), cov=cov, mask=mask,
                one_wg=one_wg, G=G, generic=False, x_nonunit=False, all_gauss=False, expect=exp)


def build_matrix():
    m = []
    # a. every compiled (LT, PT), exact (L = LT) and padded (L = LT - 1), P = PT with real regressors, on the ragged
    # 334-row layout: six workgroups along the rows
    for LT in (2, 3, 5, 8, 10):
        for PT in (1, 2, 4, 8):
            m.append(case("a-L%d-P%d" % (LT, PT), 24, LT, CS.BASE, P=PT))
            if LT in PADDED:
                m.append(case("a-L%d-P%d" % (PADDED[LT], PT), 24, PADDED[LT], CS.BASE, P=PT))
    # c. channel geometry: one channel; the two halves of a mask word (bits 30 | 31 | 32, 62 | 63), a second word (64),
    # a third (129); a partly filled channel tile beside three slices
    for N in (1, 31, 32, 33, 63, 64, 65, 130):
        m.append(case("c-N%d" % N, N, 3, [50, 37, 43]))
    # d. the covariances: rank one, exactly zero (full with strong off-diagonals is every other case)
    for L in (3, 5):
        for kind in ("rank1", "zero"):
            m.append(case("d-L%d-%s" % (L, kind), 24, L, CS.BASE, cov=kind))
    # e. the LDS row tile in ONE workgroup: one below, at, one above
    for rows in (MC_TILE - 1, MC_TILE, MC_TILE + 1):
        m.append(case("e-rows%d-onewg" % rows, 20, 5, CS.ragged(rows, MC_TILE), one_wg=True, G=1))
    # f. the masks: a channel without an observed row (in the second half of a word and in a second word), a row and a
    # whole unit with every entry missing -- each on top of the random 30 %
    m.append(case("f-dead-channel-N24", 24, 5, CS.BASE, mask="dead-channel"))
    m.append(case("f-dead-channel-N65", 65, 3, [50, 37, 43], mask="dead-channel"))
    m.append(case("f-dead-channel-P2", 24, 4, CS.BASE, P=2, mask="dead-channel"))
    m.append(case("f-dead-row", 24, 3, CS.BASE, mask="dead-row"))
    m.append(case("f-dead-unit", 24, 5, CS.BASE, mask="dead-unit"))
    return m


MATRIX = build_matrix()
assert len({c["id"] for c in MATRIX}) == len(MATRIX)
BY_ID = {c["id"]: c for c in MATRIX}
DEAD_CHANNEL = {24: 17, 65: 64}  # the channel a "dead-channel" mask blanks


def make_mask(c, rng):
    """(rows, N) bool, True = missing: about 30 % at random, then what the case names."""
    rows, N = c["rows"], c["N"]
    M = rng.random((rows, N)) < 0.3
    if c["mask"] == "dead-channel":
        M[:, DEAD_CHANNEL[N]] = True
    elif c["mask"] == "dead-row":
        M[[0, rows // 2, rows - 1]] = True
    elif c["mask"] == "dead-unit":
        s = int(np.sum(c["lengths"][:2]))
        M[s:s + c["lengths"][2]] = True
    return M


def make_problem(c):
    """joint_em_cases.make_problem's data (a covariance per row, a second (mu, v) that the set holds and the call must not
    read) and the case's mask."""
    p = CS.make_problem(c)
    p["missing"] = make_mask(c, np.random.default_rng(sum(map(ord, c["id"])) + 2))
    return p


def statement(p, n_iter, **kw):
    return EMM.mstep_cov_masked(p["y"], p["x"], p["mu"], p["cov"], p["a"], p["b"], p["missing"], n_iter,
                                noise=np.ones(p["a"].shape[1]), **kw)


_cache = {}


def problem_and_reference(cid):
    """The case's problem and the statement's (a, b, da, db, noise) per iteration count: computed once, shared, read-only."""
    if cid not in _cache:
        p = make_problem(BY_ID[cid])
        want = {}
        for n in ITERS:
            want[n] = statement(p, n)
            assert EMM.mstep_cov_masked.n_failed == 0, cid
        for arr in list(p.values()) + [w for ws in want.values() for w in ws]:
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _cache[cid] = (p, want)
    return _cache[cid]
