"""The held-out E-step's shape suite, host half: what the case table of tests/heldout_shape_cases.py must be for the device
half (tests/test_gpu_heldout_shapes.py) to mean what it says.

  - the table launches every exclusion instantiation csrc/estep_split.hip compiles, and has a case on each side of every edge
    of pass_cs, ya_nj, the 64-bit mask word and the 256-thread workgroups of esplit_excl_wconst and esplit_row_wconst;
  - in every case (but the two that say "no Gaussian channel") the record order differs from the channel order and some
    left-out channel's record index differs from its id -- the reason the suite exists: a pass that looked a channel's mask
    bit or x.b up by the record index would pass every held-out test whose Gaussian channels come last;
  - at N = 129 the record ids run through mask words 0, 1, 2 and back to 0: a word cache that only moved forward fails there;
  - the two restatements the device is compared with agree with each other where both apply, and are the E-steps of
    heldout_numpy.restated and speckled_numpy.restated;
  - every case is well conditioned on the oracle alone.
"""
import numpy as np
import pytest

import heldout_numpy as H
import heldout_shape_cases as C
import speckled_numpy as S


def test_table_launches_every_compiled_exclusion_instantiation():
    reached = set()
    for c in C.MATRIX:
        for form in c["forms"]:
            reached |= C.instantiations(c, form)
    k = C.compiled()
    assert k["LT"] == [3, 5, 8, 10] and k["ya"] == [(lt, nj) for lt in k["LT"] for nj in (4, 8)], k  # (what the cases were laid out for)
    # LT | EX_BY_ROW is one template value: the flag is a bit above every LT
    assert k["EX_BY_ROW"] > max(k["LT"]) and k["EX_BY_ROW"] & (k["EX_BY_ROW"] - 1) == 0, k
    assert reached <= C.compiled_instantiations(), sorted(reached - C.compiled_instantiations())
    for name in sorted(C.compiled_instantiations()):
        assert name in reached, "no case launches " + name
    assert len(C.compiled_instantiations()) == 4 * 2 * (2 * 2 * 3 + 2) + 4 * 2 * 2 + 2


def test_every_bucket_is_run_exact_and_padded_short_and_long_in_both_forms():
    got = {(C.lt_of(c["L"]), c["L"] == C.lt_of(c["L"]), c["family"], form) for c in C.MATRIX if c["id"].startswith("a-")
           for form in c["forms"]}
    assert got == {(lt, ex, fam, form) for lt in C.compiled()["LT"] for ex in (False, True) for fam in ("split", "long_split")
                   for form in ("groups", "rows")}
    assert {c["L"] for c in C.MATRIX if c["id"].startswith("a-") and c["vb"]} == set(range(1, 11))
    assert {(C.lt_of(c["L"]), c["family"]) for c in C.MATRIX if not c["vb"]} == {(lt, f) for lt in (5, 10) for f in ("split", "long_split")}
    assert {C.lt_of(c["L"]) for c in C.MATRIX if c["entries"] == "speckle" and c["gauss"]} == set(C.compiled()["LT"])
    assert {C.lt_of(c["L"]) for c in C.MATRIX if c["entries"] == "speckle" and not c["gauss"]} == {5, 10}
    assert {c["entries"] for c in C.MATRIX if C.lt_of(c["L"]) == 8} >= {"blank-rows", "empty-replica", "dead-channel"}


def test_both_sides_of_every_edge():
    k = C.compiled()
    for form in ("groups", "rows"):
        Ns = {c["N"] for c in C.MATRIX if form in c["forms"]}
        for edge in (k["cs2"], k["cs4"]):  # pass_cs: ntot >= edge
            assert {edge - 1, edge, edge + 1} <= Ns, (form, edge)
        for edge in (k["nj4_upto"], k["row_above"]):  # ya_nj: N <= edge; the mask word: (N + 63) >> 6
            assert {edge - 1, edge, edge + 1} <= Ns, (form, edge)
    assert {(C.pass_cs(c["N"]), C.ya_nj(c["N"])) for c in C.MATRIX} == {(1, 4), (2, 4), (4, 4), (4, 8), (4, 0)}
    assert {(c["N"] + 63) // 64 for c in C.MATRIX if "entries" in c["forms"]} >= {1, 3}
    # HASXB at every channel split and on the lane-per-row y pass, in every bucket
    assert {(C.lt_of(c["L"]), C.pass_cs(c["N"]), C.ya_nj(c["N"])) for c in C.MATRIX if c["P"] > 1} == \
        {(lt, cs, nj) for lt in k["LT"] for cs, nj in ((1, 4), (2, 4), (4, 8), (4, 0))}
    # esplit_excl_wconst: 16 threads per replica, 256 per workgroup
    reps = {c["n_rep"] for c in C.MATRIX if "groups" in c["forms"]}
    assert {16, 17} <= reps and max(reps) > 64 and min(reps) == 2, reps
    # esplit_row_wconst: one thread per replicated row
    rows = {c["n_rep"] * c["rows"] for c in C.MATRIX if "rows" in c["forms"] or (c["entries"] and c["gauss"])}
    assert 256 in rows and min(rows) < 64 and any(256 < r <= 260 for r in rows) and max(rows) > 512, sorted(rows)
    # the row-to-replica mapping
    one = [c for c in C.MATRIX if c["M"] == 1]
    assert {c["rows"] for c in one} >= {1, 63, 64, 65}
    assert {c["n_rep"] for c in one if c["rows"] == 1} == {2, 3, 70}
    c = C.BY_ID["d-3x50-N65"]
    assert c["rows"] == 150 and c["rows"] % 64 and C.pass_cs(c["N"]) == 4


def test_stream_lane_cases_cut_where_they_say():
    for cid in C.LANE_CASES:
        c = C.BY_ID[cid]
        exp = C.expected_plan(c, c["n_rep"] * c["M"])
        assert exp["n_lanes"] == int(c["env"]["VLGP_ESTEP_LANES"]) and exp["classes"] == ["lo"] * c["L"], (cid, exp)
        inner = exp["cuts"][1:-1]
        assert len(inner) == exp["n_lanes"] - 1
        if cid.endswith("inside"):
            assert all(cut % c["M"] for cut in inner), (cid, exp["cuts"])
        else:
            assert all(cut % c["M"] == 0 for cut in inner), (cid, exp["cuts"])
    assert {c["env"]["VLGP_ESTEP_LANES"] for c in C.MATRIX if c["id"] in C.LANE_CASES} == {"2", "3"}
    assert C.expected_plan(C.BY_ID["d-lanes3-inside"], 27)["cuts"] == [0, 12, 20, 27]
    assert C.expected_plan(C.BY_ID["d-lanes2-between"], 16)["cuts"] == [0, 8, 16]
    for c in C.MATRIX:  # every other case runs on one lane; the plan of each side of a comparison exists
        if c["id"] not in C.LANE_CASES:
            assert C.expected_plan(c, c["n_rep"] * c["M"])["n_lanes"] == 1, c["id"]
        assert C.expected_plan(c, c["M"])["family"] == c["family"]


@pytest.mark.parametrize("cid, form", C.RUNS)
def test_record_index_is_not_the_channel_id(cid, form):
    """ASSERTED, not assumed: the records are not in channel order, and a channel some replica leaves out sits at a record
    index that is not its id; a Gaussian channel lies before a left-out Poisson one; the groups mix both likelihoods."""
    c = C.BY_ID[cid]
    held = C.problem(cid)["held"][form]
    assert held.shape == (c["n_rep"], c["rows"], c["N"])
    order = C.record_order(c["N"], c["gauss"])
    assert sorted(order) == list(range(c["N"]))
    out = C.left_out_channels(held)
    assert out, cid
    if not c["gauss"]:
        assert "no Gaussian channel" in c["note"] and order == list(range(c["N"]))
        return
    assert order != list(range(c["N"]))
    moved = [n for n in out if order.index(n) != n]
    assert moved, (cid, out)
    pois_out = [n for n in out if n not in c["gauss"]]
    assert pois_out and min(c["gauss"]) < max(pois_out), (cid, out)
    assert any(n in c["gauss"] for n in out), (cid, out)
    if c["groups"] is not None:
        assert all(len(set(g)) == len(g) and g for g in c["groups"])
        if form == "rows":
            assert all(np.array_equal(held[k], np.isin(np.arange(c["N"]), g)[None].repeat(c["rows"], 0)) for k, g in enumerate(c["groups"]))


def test_groups_at_the_edges_hold_what_they_say():
    for c in C.MATRIX:
        if c["groups"] is None or c["N"] == 24:
            continue
        N, gauss, cs = c["N"], c["gauss"], C.pass_cs(c["N"])
        g0, g1, share, gs = c["groups"]
        edges = {n for n in C.EDGE_CHANNELS + (N - 1,) if n < N}
        assert edges <= set(g0) | set(g1), c["id"]
        for g in (g0, g1):
            assert any(n not in gauss for n in g), (c["id"], g)
        assert gs == sorted(gauss)  # this replica's Gaussian constant of w is 0
        pois = [n for n in range(N) if n not in gauss]
        part = cs // 2
        assert share == pois[len(pois) * part // cs:len(pois) * (part + 1) // cs] and share, c["id"]
        if c["id"].startswith("b-") or c["id"].startswith("d-"):
            assert any(n in gauss for n in g0 + g1), c["id"]  # the edge groups mix both likelihoods


def test_ids_at_129_channels_run_through_three_words_and_back():
    for c in C.MATRIX:
        if c["N"] != 129:
            continue
        assert c["gauss"] == (0, 63, 64, 127) and "back to 0" in c["note"]
        assert C.record_words(129, c["gauss"]) == [0, 1, 2, 0, 1], c["id"]
        # the last wave of the channel split goes from word 2 back to word 1, to a channel that a replica leaves out
        pois = C.wave_share(129, c["gauss"], 3, 4)
        assert {n >> 6 for n in pois} == {1, 2} and pois[-1] == 128 and sorted(c["gauss"])[3] == 127
        if c["groups"] is not None:
            out = set().union(*c["groups"])
            assert {0, 127, 128} <= out
            assert any(0 in g and 128 not in g for g in c["groups"])  # bit 0 of word 2 is not bit 0 of word 0
    assert sum(c["N"] == 129 for c in C.MATRIX) >= 9
    # for contrast: at 100 channels no wave of the split ever steps back a word, and the y pass holds its words in registers
    assert C.record_words(100, C.BY_ID["b-N100-L8"]["gauss"]) == [0, 1, 0, 1]


STEP_BACK = sorted(c["id"] for c in C.MATRIX if c["N"] == 129) + ["b-N100-L5-gauss-low"]


@pytest.mark.parametrize("cid, form", C.RUNS)
def test_the_two_wrong_lookups_would_leave_other_channels_out(cid, form):
    """The two mistakes the suite was laid out against, stated on the host (heldout_shape_cases.seen_left_out): the mask bit
    looked up by the record index in place of the id, and a word cache that reloads only when the word number grows.  Where
    either leaves another set of channels out than esplit_pass's left_out, the device cannot meet both the plain twin's bits and
    the restatement.  The first does in every pass of every case that has a Gaussian channel; the second where a lane's walk
    steps back a word: the cases of STEP_BACK, in the residual pass and the lane-per-row y pass."""
    c = C.BY_ID[cid]
    held = C.problem(cid)["held"][form]
    kinds = sorted({kind for kind, _ in C.walks(c)})
    assert kinds == (["SP_RES", "SP_W", "SP_YA"] if c["N"] > 128 else ["SP_RES", "SP_W"])
    assert C.caught_by(c, form, held, "id") == []
    assert C.caught_by(c, form, held, "record-index") == (kinds if c["gauss"] else []), cid
    back = C.caught_by(c, form, held, "forward-only")
    assert back == ([] if cid not in STEP_BACK else ["SP_RES", "SP_YA"] if c["N"] > 128 else ["SP_RES"]), (cid, back)
    order = C.record_order(c["N"], c["gauss"])
    steps_back = any(order[j] >> 6 < order[i] >> 6 for _, walk in C.walks(c) for i, j in zip(walk, walk[1:]))
    assert steps_back == (cid in STEP_BACK), cid


def test_reference_is_the_e_step_of_the_two_restatements():
    """restated_posterior from a zero start against heldout_numpy.restated and speckled_numpy.restated themselves, same bits
    (the suite's references are the same calls from the start of the source units)."""
    c = C.BY_ID["a-L4-short"]
    p = C.problem(c["id"])
    n = C.SWEEPS[-1]
    ref = C.restated_posterior(c, p, "groups", n, from_zero=True)
    rates, lls = H.restated(p["trials"], p["params"], p["config"], c["groups"], n)
    pair, par = 0, p["params"]
    for k, g in enumerate(c["groups"]):
        ll_sum = np.zeros(len(g))
        for m, tr in enumerate(p["trials"]):
            sl = slice(m * c["T"], (m + 1) * c["T"])
            r, ll = H.rate_ll(tr["y"], tr["x"], ref["mu"][k, sl], ref["v"][k, sl], par["a"], par["b"], par["noise"], p["gauss"], True)
            assert np.array_equal(r[:, g], rates[m][:, pair:pair + len(g)])
            ll_sum += ll[:, g].sum(axis=0)
        assert np.array_equal(ll_sum, lls[pair:pair + len(g)])
        pair += len(g)
    for cid in ("e-speckle-L5", "a-L4-short"):
        c = C.BY_ID[cid]
        p = C.problem(cid)
        form = c["forms"][-1]
        post, _, _, bad = S.restated(p["trials"], p["params"], p["config"], p["held"][form], n)
        assert bad == 0
        for key in ("mu", "v", "w"):
            assert np.array_equal(post[key], C.restated_posterior(c, p, form, n, from_zero=True)[key]), (cid, key)


@pytest.mark.parametrize("cid", C.GROUP_CASES)
def test_the_two_restatements_agree_on_row_constant_masks(cid):
    """Both are float64 statements of one E-step in different summation orders: they agree to a tenth of the tolerance they
    are held to as references, per column."""
    c = C.BY_ID[cid]
    for n in C.SWEEPS:
        err = C.column_errors(c, C.reference(cid, "rows", n), C.reference(cid, "groups", n))
        assert max(err.values()) < 0.1 * C.STAGE, (cid, n, err)


@pytest.mark.parametrize("cid, form", C.RUNS)
def test_every_case_is_well_conditioned(cid, form):
    """On the oracle alone, a condition on the inputs (a seed that fails it is replaced in SALT, the bound stays): one ulp, up
    or down at random, on every mu of the start moves no column of mu, v, w or dmu by more than a tenth of the tolerance, after
    one sweep and after three; and the host's prior ranks are the ones the case names."""
    c = C.BY_ID[cid]
    p = C.problem(cid)
    assert p["ranks"] == c["ranks"], (cid, p["ranks"])
    rng = np.random.default_rng(1)
    moved = [np.nextafter(t["mu"], np.where(rng.random(t["mu"].shape) < 0.5, -np.inf, np.inf)) for t in p["trials"]]
    worst = {}
    for n in C.SWEEPS:
        ref = C.reference(cid, form, n)
        assert all(np.all(np.isfinite(r)) for r in ref.values())
        for k, e in C.column_errors(c, C.restated_posterior(c, p, form, n, mu=moved), ref).items():
            worst[(n, k)] = e
    print("heldout-shapes %-22s %-7s one-ulp perturbation of mu: %s" % (cid, form, {k: "%.1e" % v for k, v in worst.items()}))
    assert max(worst.values()) < 0.1 * C.STAGE, (cid, form, worst)
