"""Without a GPU: the case table of tests/test_gpu_support_shapes.py (tests/support_cases.py) against the sources it was
derived from, the exactness of every exact-by-construction case, and the condition of every measured reference.

  * the table has a case on each side of every edge the launchers of csrc/misc.hip and csrc/prior.hip define;
  * for every exact case the float64 statement equals the np.longdouble one, and on a sample fractions.Fraction;
  * every measured allowance of the posterior draws stays below the tolerance of the existing test (1e-10);
  * the prior cases do what their names say: the smooth latent stops before R, the rough one fills it, ranks differ
    between the lengths of a many-length call.
"""
from fractions import Fraction as Fr

import numpy as np
import pytest

import support_cases as CS
import support_numpy as S

E = CS.E


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble))


# ---- the edges ---------------------------------------------------------------------------------------------------------
def test_the_edges_are_read_and_consistent():
    """Relations between the constants read from the sources, no values: a retune moves the cases, it does not break this."""
    assert 1 <= E["PROJ_ROWS"] <= E["PROJ_THREADS"] and E["PROJ_THREADS"] % 64 == 0
    assert E["MAP_LT"] == sorted(set(E["MAP_LT"])) and 1 <= E["MAP_LT"][0] and E["MAP_LT"][-1] < 64 and len(E["MAP_LT"]) >= 2
    assert E["GRID_MAX"] >= 1 and E["NORMS_PER_WG"] % 256 == 0 and E["PRIOR_SLOTS"] >= 1
    assert 1 <= E["ICH_T_WAVE"] < E["ICH_T_256"] < CS.T_E <= E["ICH_T_LDS"]
    assert CS.prior_lds(CS.T_E - 1) <= CS.LDS_DEFAULT < CS.prior_lds(CS.T_E)
    assert CS.prior_lds(E["ICH_T_LDS"]) <= CS.LDS_CU  # the longest length held in LDS fits a CU
    # VLGP_MAX_RANK = 64 bounds the one-wave kernel's request below the launcher's `lds_wave <= 60 * 1024`: that test is
    # always true, there is no length or rank that takes its other side, hence no case for it
    assert CS.prior_plan(E["ICH_T_WAVE"], 64)["lds"] < 60 * 1024 <= CS.LDS_DEFAULT


def test_projection_table_straddles_every_edge():
    by_n = {k["N"]: k for k in CS.PROJECT if not k["real"] and k["L"] == 4 and k["rows"] == 2 * E["PROJ_ROWS"] + 2}
    R, below, top = E["PROJ_ROWS"], CS.PROJECT_N_64K, CS.PROJECT_N_MAX
    assert {1, 2, R - 1, R, below, below + 1, below + 2, top} <= set(by_n)
    # the default ceiling: last N below, first above
    assert CS.project_lds(below) <= CS.LDS_DEFAULT < CS.project_lds(below + 1)
    assert not by_n[below]["raised"] and by_n[below + 1]["raised"]
    # a CU's LDS: the launcher has no cap, so no case may ask for more than a CU can grant, and one case asks for the most
    # it can (the far side of that edge, the strided column loop at N > threads and the M-step's largest N need the cap)
    assert CS.project_lds(top) <= CS.LDS_CU < CS.project_lds(top + 1) and below < top
    for k in CS.PROJECT:
        assert k["lds"] <= CS.LDS_CU and k["G"] == -(-k["rows"] // k["rpw"])
    assert {k["N"] & 1 for k in CS.PROJECT} == {0, 1}                                          # N | 1 changes N or not
    assert {k["G"] % 4 for k in CS.PROJECT if k["N"] == 20} == {0, 1, 2, 3}                      # every tail of the fold
    assert any(k["G"] >= 8 for k in CS.PROJECT)                                                # two trips of the fold of four
    assert {1, R - 1, R, R + 1} <= {k["rows"] for k in CS.PROJECT} and any(k["rows"] % k["rpw"] for k in CS.PROJECT)
    nl = sorted(R * k["L"] for k in CS.PROJECT if k["N"] == 20 and k["rows"] == 2 * R + 2)     # threads with work: (row, latent)
    assert nl[0] < E["PROJ_THREADS"] < nl[1] < nl[-1] == R * 64
    assert sum(k["real"] for k in CS.PROJECT) == 1


def test_map_table_straddles_every_edge():
    lts = E["MAP_LT"]
    by_class = {}
    for k in CS.MAP:
        by_class.setdefault(k["LT"], set()).add(k["L"])
    for lt in lts:
        assert lt in by_class[lt] and min(by_class[lt]) < lt, (lt, by_class)  # the class exact and padded
        assert lt + 1 in by_class[CS.map_class(lt + 1)]                       # and the first L past it
    assert max(by_class[0]) == 64 and min(by_class[0]) == lts[-1] + 1
    assert {1, 255, 256, 257} <= {k["rows"] for k in CS.MAP}
    assert {k["trips"] for k in CS.MAP} == {1, 2} and CS.grid_trips(CS.BIG_ROWS - 1) == 1 and CS.grid_trips(CS.BIG_ROWS) == 2
    assert {k["shift"] for k in CS.MAP} == {True, False} and sum(k["real"] for k in CS.MAP) == 1
    assert min(CS.OVERLAP_L) <= lts[0] and max(CS.OVERLAP_L) > lts[-1]


def test_cut_table_covers_the_launches():
    assert {k["P"] for k in CS.CUT} >= {1, 2, 3} and {k["N"] for k in CS.CUT} >= {1, 65}
    assert {k["window"] for k in CS.CUT} >= {1, 2, 50} and any(len(k["starts"]) == 1 for k in CS.CUT)
    assert any(k["y_trips"] > 1 for k in CS.CUT) and any(k["y_trips"] == 1 for k in CS.CUT)
    assert any(k["one_launch"] and not k["overlapping"] for k in CS.CUT)
    over = [k for k in CS.CUT if k["overlapping"]]
    assert all(not k["one_launch"] for k in over)  # an overlap always takes the unit-by-unit scatter
    assert any(len(set(k["starts"])) < len(k["starts"]) for k in over)
    assert any(k["starts"] != sorted(k["starts"]) for k in over)
    for k in CS.CUT:  # the later unit wins: sequential assignment differs from the reversed order on every overlapping case
        p = CS.cut_problem(k)
        fwd = S.merge(p["mu"], p["new_mu"], k["starts"], k["window"])
        n = len(k["starts"])
        rev_segs = np.concatenate([p["new_mu"][j * k["window"]:(j + 1) * k["window"]] for j in reversed(range(n))])
        rev = S.merge(p["mu"], rev_segs, k["starts"][::-1], k["window"])
        assert np.array_equal(fwd, rev) != k["overlapping"], k["id"]
        assert not np.all(p["x"] == 1.0)


def test_norms_table_straddles_every_edge():
    W = E["NORMS_PER_WG"]
    d = {k["id"]: k for k in CS.NORMS}
    assert {1, 255, 256, 257, W - 1, W, W + 1} <= {k["n"] for k in CS.NORMS if k["blocks"] is None}
    B = CS.NORMS_DEFAULT_BLOCKS
    assert d["d-n%d-default" % (B * W + 1)]["g"] == B and d["d-n%d-default" % (B * W + 1)]["trips"] == 2
    assert d["d-n%d-blocks1" % (W + 1)]["trips"] == 2 and d["d-n%d-blocks1" % (W + 1)]["loads_in_range"] == 1  # three of four out of range
    assert d["d-n%d-blocks1" % W]["trips"] == 1 and d["d-n%d-blocks1" % (2 * W + 1)]["trips"] == 3
    assert [d["d-n%d-blocks7" % n]["trips"] for n in (7 * W, 7 * W + 1, 14 * W + 769)] == [1, 2, 3]
    assert d["d-n%d-blocks7" % (14 * W + 769)]["loads_in_range"] == 1
    big = d["d-n%d-blocks1024" % (1024 * W + 1)]
    assert big["g"] == 1024 and big["fold_trips"] == 4 and big["trips"] == 2
    assert {k["loads_in_range"] for k in CS.NORMS} >= {1, 4}
    assert {k["fold_trips"] for k in CS.NORMS} == {1, 4}


def test_prior_table_straddles_every_edge():
    lengths = {T for k in CS.PRIOR for T in k["lengths"]}
    for edge in (E["ICH_T_WAVE"], E["ICH_T_256"], E["ICH_T_LDS"], CS.T_E - 1):
        assert edge + 1 in lengths and any(T <= edge for T in lengths), edge
    assert {E["ICH_T_256"], E["ICH_T_LDS"], CS.T_E - 1, CS.T_E, 1} <= lengths
    classes = {(p["wave"], p["nt"], p["raised"], p["global_scratch"]) for p in (CS.prior_plan(T, 50) for T in lengths)}
    assert classes == {(1, 64, 0, 0), (0, 256, 0, 0), (0, 1024, 0, 0), (0, 1024, 1, 0), (0, 1024, 0, 1)}  # (the kernels, not sizes)
    assert {k["R"] for k in CS.PRIOR} >= {1, 50, 64} and {k["L"] for k in CS.PRIOR} >= {1, 2, 16}
    counts = sorted(len(k["lengths"]) for k in CS.PRIOR if len(k["lengths"]) > 1)
    slots = E["PRIOR_SLOTS"]
    assert counts == [slots, slots + 1, slots + 1, 2 * slots + 2]  # one, two, three mailbox rounds; the lazy and the waited rebuild
    assert all(len(set(k["lengths"])) == len(k["lengths"]) and min(k["lengths"]) >= 2 and max(k["lengths"]) <= 140
               for k in CS.PRIOR if len(k["lengths"]) > 1)
    k16 = CS.PRIOR_BY_ID["e-L16-T%d" % CS.T_SHORT]
    assert len(set(k16["omega"])) == 16 and len(set(k16["sigma"])) == 16


@pytest.mark.parametrize("cid", [k["id"] for k in CS.PRIOR if k["kinds"]])
def test_prior_cases_stop_where_they_say(cid):
    k = CS.PRIOR_BY_ID[cid]
    T, R = k["lengths"][0], k["R"]
    for kind, om, sg in zip(k["kinds"], k["omega"], k["sigma"]):
        rank = CS.oracle_factor(T, om, sg, R)[1]
        if kind == "rough":
            assert rank == min(T, R), (cid, rank)
            # ... while the remaining rows T - i cross a multiple of 128 (a new leaf layout of the pairwise sum) when any lies in reach
            if T > 128 and T % 128 < R:
                assert any((T - i) % 128 == 0 for i in range(rank))
        elif R > 1 and T > 1:
            assert 1 <= rank < R, (cid, rank)


def test_prior_ranks_differ_between_lengths_and_compact_ranks_differ():
    for k in CS.PRIOR:
        if len(k["lengths"]) > 1:
            for om in (k["omega"], k["rebuild"]):
                if om is None:
                    continue
                ranks = [tuple(CS.oracle_factor(T, om[l], k["sigma"][l], k["R"])[1] for l in range(k["L"])) for T in k["lengths"]]
                assert len(set(ranks)) >= len(ranks) // 4, (k["id"], len(set(ranks)))
                assert all(a != b for a, b in zip(ranks, ranks[CS.E["PRIOR_SLOTS"]:]))  # slot j of two rounds never agrees
    for k in CS.COMPACT:
        ranks = [CS.oracle_factor(k["T"], k["omega"][l], k["sigma"][l], k["R"])[1] for l in range(3)]
        assert len(set(ranks)) == 3 and max(ranks) == k["R"], ranks
    for cid, G, ranks in CS.injected_factors():
        assert [S.factor_rank(G[l]) for l in range(G.shape[0])] == ranks, cid


# ---- exactness ---------------------------------------------------------------------------------------------------------
def _fraction_matmul(a, b, rows, cols):
    return {(i, j): sum(Fr(float(a[i, k])) * Fr(float(b[k, j])) for k in range(a.shape[1])) for i in rows for j in cols}


@pytest.mark.parametrize("cid", [k["id"] for k in CS.PROJECT if not k["real"]])
def test_projection_cases_are_exact(cid):
    k = CS.PROJECT_BY_ID[cid]
    y, proj, shift = CS.project_problem(k)
    mu, col = S.project(y, proj, shift)
    mu_l, col_l = S.project(y, proj, shift, np.longdouble)
    assert _same(mu, mu_l) and _same(col, col_l)
    assert np.all(y == np.round(y)) and np.all(proj * 256 == np.round(proj * 256)) and np.abs(proj).max() <= 4
    assert np.max(np.abs(y) @ np.abs(proj)) * 256 < 2.0 ** 40  # every partial sum, in units of 2^-8: far below 2^53
    rows, cols = sorted({0, k["rows"] - 1, k["rows"] // 2}), sorted({0, k["L"] - 1})
    fr = _fraction_matmul(y, proj, rows, cols)
    for (i, j), v in fr.items():
        assert Fr(float(mu[i, j])) == v - Fr(float(shift[j]))
    assert all(Fr(float(col[n])) == sum(Fr(float(v)) for v in y[:, n]) for n in {0, k["N"] - 1})


@pytest.mark.parametrize("cid", [k["id"] for k in CS.MAP if not k["real"]])
def test_map_cases_are_exact(cid):
    k = CS.MAP_BY_ID[cid]
    mu, mat, shift = CS.map_problem(k)
    if k["rows"] > 5000:  # the stride set: a slice of its head and its tail states the same
        mu = np.concatenate([mu[:300], mu[-300:]])
    got, got_l = S.latent_map(mu, mat, shift), S.latent_map(mu, mat, shift, np.longdouble)
    assert _same(got, got_l)
    # twice (a shared row of overlapping segments is mapped twice) is exact too
    assert _same(S.latent_map(got, mat, shift), S.latent_map(got_l, mat, shift, np.longdouble))
    sh = np.zeros(k["L"]) if shift is None else shift
    fr = _fraction_matmul(mu - sh[None, :], mat, (0, len(mu) - 1), sorted({0, k["L"] - 1}))
    assert all(Fr(float(got[i, j])) == v for (i, j), v in fr.items())


@pytest.mark.parametrize("cid", [k["id"] for k in CS.NORMS])
def test_norms_cases_are_exact(cid):
    mu = CS.norms_problem(CS.NORMS_BY_ID[cid])
    flat = mu.reshape(-1)
    want = int((flat.astype(np.int64) ** 2).sum())
    assert np.all(np.abs(flat) <= 8) and np.all(flat == np.round(flat)) and 64 * flat.size < 2 ** 53
    assert float(flat @ flat) == want and float(flat.astype(np.longdouble) @ flat.astype(np.longdouble)) == want
    assert sum(Fr(float(v)) ** 2 for v in flat[:2000]) == int((flat[:2000].astype(np.int64) ** 2).sum())


def test_cut_projection_is_exact():
    for k in CS.CUT:
        if k["y_trips"] > 1:
            continue
        p = CS.cut_problem(k)
        y = S.cut(p["y"], k["starts"], k["window"])
        assert _same(S.project(y, p["proj"], p["shift"])[0], S.project(y, p["proj"], p["shift"], np.longdouble)[0])


# ---- the derived bounds and the measured allowances --------------------------------------------------------------------
def test_real_valued_cases_have_a_bound_that_binds():
    k = next(c for c in CS.PROJECT if c["real"])
    y, proj, shift = CS.project_problem(k)
    b = S.project_bound(y, proj, shift)
    mu64, mu_l = S.project(y, proj, shift)[0], S.project(y, proj, shift, np.longdouble)[0]
    assert np.all(np.abs(mu64 - mu_l) <= b) and float(b.max()) < 1e-11  # float64 NumPy, one more order, is inside; the bound is tight
    k = next(c for c in CS.MAP if c["real"])
    mu, mat, shift = CS.map_problem(k)
    b = S.latent_map_bound(mu, mat, shift)
    assert np.all(np.abs(S.latent_map(mu, mat, shift) - S.latent_map(mu, mat, shift, np.longdouble)) <= b) and float(b.max()) < 1e-13


@pytest.mark.parametrize("cid", [k["id"] for k in CS.DRAWS])
def test_draw_references_are_conditioned(cid):
    k = CS.DRAW_BY_ID[cid]
    p, ref = CS.draw_problem(cid)
    assert ref["want"].dtype == np.longdouble and np.all(np.isfinite(ref["want"]))
    if k["compare"] == "measured":
        assert CS.FLOOR <= ref["allowance"] < CS.ALLOWANCE_CAP, (cid, ref["oracle_distance"])
    elif k["compare"] == "bits":
        assert not p["G"].any() and _same(ref["want"], np.broadcast_to(p["mu"], ref["want"].shape))
    else:
        assert not p["w"].any() and float(ref["bound"].max()) < 1e-13


def test_draw_table_covers_the_ranks_and_sizes():
    d = {k["id"]: CS.draw_problem(k["id"])[0]["ranks"] for k in CS.DRAWS}
    assert d["f-R1"] == [1, 1] and d["f-R2"] == [2, 2] and d["f-R64"][1] == 64 and d["f-R50"][1] == 50
    assert d["f-rank1-beside-full"] == [1, 8] and d["f-r64-T70"] == [64] and d["f-zero-factor"] == [1, 1]
    assert {k["T"] for k in CS.DRAWS} >= {1, 2, 257} and {k["n"] for k in CS.DRAWS} >= {1, 255, 256, 257, 1000}
    assert np.sum(CS.draw_problem("f-w1e6")[0]["w"] == 1e6) >= 3
