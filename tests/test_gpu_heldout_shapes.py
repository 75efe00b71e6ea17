"""The held-out E-step at every compiled exclusion instantiation of its row passes, with the channel order, the mask words and
the row-to-replica mapping where they can go wrong (the case table: tests/heldout_shape_cases.py; what makes it mean
something: tests/test_heldout_shapes_host.py).

A replicated set is run by the EXCL instantiations of csrc/estep_split.hip or not at all: esplit_pass<LT (| EX_BY_ROW), KIND,
HASXB, CS, true>, esplit_ya<LT (| EX_BY_ROW), NJ, true>, esplit_excl_wconst, esplit_row_wconst.  The other held-out tests
replicate sets of one to three latents whose Gaussian channels come last, where a channel's record index IS its id.  Here
every bucket, channel split and y pass runs with the Gaussian channels interleaved, per replica and per row, and is compared
three ways, with no tolerance but the project's:

  1. in BITS with the plain twin: the source units on a second handle whose loadings have the group's columns zeroed, forced
     onto the same family, its plan equal in family, LT, CS, NJ and classes.  The plain instantiations are held to the oracle
     by tests/test_gpu_estep_shapes.py; equal bits carry that over, and a dropped, doubled or misplaced channel has no
     tolerance to hide behind;
  2. in BITS between the forms: masks constant along the rows against group replicas, several stream lanes against one;
  3. with the restatement (heldout_shape_cases.restated_posterior: the E-steps of heldout_numpy.restated and
     speckled_numpy.restated) per (replica, unit, latent) column -- max over t of |got - ref| over the column's own max |ref|,
     dmu on the column's mu scale -- at heldout_numpy.STAGE = 1e-9 after one sweep and after three.  The masks by entry have
     no twin: this is their only reference.

Every case asserts the plan it expects through Engine.estep_plan on the replicated set; none is skipped or declined.  The
cases of (a) also score a log-likelihood per (replica, left-out channel) pair against the restated posterior.

Measured on an MI355X (profiles/heldout_shapes/measured_errors.txt, every case): mu 3.3e-11, dmu 3.2e-11, w 1.3e-12 (all case
c-N33-L8-P2, three sweeps), v 5.0e-12 (d-rows65, one sweep), the log-likelihood per pair 3.5e-14 at worst; every comparison in
bits held; nothing was found wrong.
"""
import numpy as np
import pytest

import heldout_numpy as H
import heldout_shape_cases as C
import test_gpu_estep_shapes as E

pytestmark = pytest.mark.gpu

SRC, REP = 0, 2  # set ids


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture
def clean_env(monkeypatch):
    """The library reads its switches when a handle is created: every handle below is created after its case's setting."""
    for name in E.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def with_lanes(c, lanes):
    return c if lanes is None else dict(c, env=dict(c["env"], VLGP_ESTEP_LANES=str(lanes)))


def open_engine(V, c, p, switches, a=None):
    """A handle holding the case's source units (set SRC), parameters (loadings `a` if given) and prior; its switches and the
    prior's ranks and bits asserted."""
    par = p["params"]
    eng = V.Engine(c["N"], c["L"], c["P"], C.RANK, p["gauss"])
    try:
        for name, value in switches.items():
            assert eng.switch(name) == value, (c["id"], name)
        eng.set_params(par["a"] if a is None else a, par["b"], par["noise"])
        eng.build_prior([c["T"]], par["omega"], par["sigma"])
        eng.upload(SRC, p["trials"])
        G, rk = eng.get_prior(c["T"], with_rank=True)
        assert list(rk) == c["ranks"], (c["id"], list(rk))
        assert np.array_equal(G, p["chol"][c["T"]]), c["id"]
    except BaseException:
        eng.close()
        raise
    return eng


def assert_plan(eng, set_id, c, n_units, n_iter):
    plan = eng.estep_plan(set_id, n_iter, vb=c["vb"])
    for k, want in C.expected_plan(c, n_units).items():
        assert plan[k] == want, (c["id"], k, want, plan)
    assert plan["cuts"][0] == 0 and plan["cuts"][-1] == n_units and len(plan["cuts"]) == plan["n_lanes"] + 1
    return plan


_runs = {}


def device_run(V, env, cid, form, n_iter, lanes=None):
    """The case's replicated set after n_iter sweeps: (mu, v, w, dmu as (n_rep, rows, L), the plan, the log-likelihood sums per
    pair or None).  Run once per (case, form, sweeps, lanes) and shared, read-only, by the comparisons."""
    key = (cid, form, n_iter, lanes)
    if key in _runs:
        return _runs[key]
    c = with_lanes(C.BY_ID[cid], lanes)
    p = C.problem(cid)
    switches = E.set_case_switches(c, env)
    with open_engine(V, c, p, switches) as eng:
        if form == "groups":
            eng.replicate(SRC, REP, groups=c["groups"])
        else:
            eng.replicate(SRC, REP, held_out=p["held"][form])
        plan = assert_plan(eng, REP, c, c["n_rep"] * c["M"], n_iter)
        assert eng.estep(REP, n_iter, C.DMU_BOUND, c["vb"]) == 0
        assert eng.last_estep_path == plan["family"] == c["family"], (cid, eng.last_estep_path, plan)
        got = {k: a.reshape(c["n_rep"], c["rows"], c["L"]) for k, a in eng.download(REP).items()}
        sums = eng.loglik(REP, vb=c["vb"])[0] if form == "groups" and cid.startswith("a-") else None
    for a in got.values():
        a.setflags(write=False)
    _runs[key] = (got, plan, sums)
    return _runs[key]


@pytest.mark.parametrize("cid, form", C.RUNS)
def test_shapes_vs_restatement(V, cid, form, clean_env):
    """One case in one form: its plan, then every (replica, unit, latent) column at 1e-9 after one sweep and after three."""
    c = C.BY_ID[cid]
    worst = {}
    for n in C.SWEEPS:
        got, plan, _ = device_run(V, clean_env, cid, form, n)
        worst[n] = C.column_errors(c, got, C.reference(cid, form, n))
        print("heldout-shapes %-22s %-7s sweeps %d  " % (cid, form, n) + "  ".join("%s %.2e" % kv for kv in worst[n].items())
              + ("  plan %s" % plan if n == C.SWEEPS[0] else ""))
    for n, errs in worst.items():
        for k, e in errs.items():
            assert e < C.STAGE, (cid, form, n, k, e)  # (a NaN comes out as inf)


@pytest.mark.parametrize("cid", C.GROUP_CASES)
def test_replica_equals_plain_twin_bitwise(V, cid, clean_env):
    """estep_split.hip's promise: a replica runs, bit for bit, what the same kernels run on a plain set with a[:, g] = 0."""
    c = C.BY_ID[cid]
    p = C.problem(cid)
    par = p["params"]
    for n in C.SWEEPS:
        rep, plan, _ = device_run(V, clean_env, cid, "groups", n)
        with open_engine(V, c, p, E.set_case_switches(c, clean_env)) as eng:
            for k, g in enumerate(c["groups"]):
                eng.set_params(C.zeroed(par["a"], g), par["b"], par["noise"])
                eng.upload(SRC, p["trials"])
                twin = eng.estep_plan(SRC, n, vb=c["vb"])
                assert twin["decline"] == "taken", (cid, twin)
                for key in C.SAME_AS_TWIN:
                    assert twin[key] == plan[key], (cid, key, twin, plan)
                assert eng.estep(SRC, n, C.DMU_BOUND, c["vb"]) == 0
                assert eng.last_estep_path == plan["family"], (cid, eng.last_estep_path)
                got = eng.download(SRC)
                for key in C.FIELDS:
                    assert np.array_equal(got[key], rep[key][k]), (cid, n, "replica %d" % k, key)


@pytest.mark.parametrize("cid", C.GROUP_CASES)
def test_row_constant_masks_equal_group_replicas_bitwise(V, cid, clean_env):
    for n in C.SWEEPS:
        rows, plan_r, _ = device_run(V, clean_env, cid, "rows", n)
        groups, plan_g, _ = device_run(V, clean_env, cid, "groups", n)
        assert plan_r == plan_g, (cid, plan_r, plan_g)
        for key in C.FIELDS:
            assert np.array_equal(rows[key], groups[key]), (cid, n, key)


@pytest.mark.parametrize("form", ("groups", "rows"))
@pytest.mark.parametrize("cid", C.LANE_CASES)
def test_stream_lanes_equal_one_lane_bitwise(V, cid, form, clean_env):
    """A replicated set cut over two or three stream lanes, inside a replica or between two: the row passes of a lane start at
    its first row (row_base = A.mu - X.mu_lm) and find the replica and the source row of each of theirs from there."""
    for n in C.SWEEPS:
        many, plan, _ = device_run(V, clean_env, cid, form, n)
        one, plan1, _ = device_run(V, clean_env, cid, form, n, lanes=1)
        assert plan["n_lanes"] == int(C.BY_ID[cid]["env"]["VLGP_ESTEP_LANES"]) and plan1["n_lanes"] == 1
        for key in C.FIELDS:
            assert np.array_equal(many[key], one[key]), (cid, form, n, key)


@pytest.mark.parametrize("cid", [c["id"] for c in C.MATRIX if c["id"].startswith("a-")])
def test_loglik_per_pair_of_the_latent_buckets(V, cid, clean_env):
    """vlgp_loglik behind the held-out E-step, per (replica, left-out channel) pair, against the scoring definitions of
    heldout_numpy.rate_ll on the restated posterior."""
    c = C.BY_ID[cid]
    p = C.problem(cid)
    par = p["params"]
    n = C.SWEEPS[-1]
    _, _, sums = device_run(V, clean_env, cid, "groups", n)
    ref = C.reference(cid, "groups", n)
    pairs = [(k, ch) for k, g in enumerate(c["groups"]) for ch in g]
    assert sums.shape == (len(pairs), 4)
    worst = 0.0
    for i, (k, ch) in enumerate(pairs):
        want = 0.0
        for m, tr in enumerate(p["trials"]):
            sl = slice(m * c["T"], (m + 1) * c["T"])
            want += H.rate_ll(tr["y"], tr["x"], ref["mu"][k, sl], ref["v"][k, sl], par["a"], par["b"], par["noise"], p["gauss"],
                              c["vb"])[1][:, ch].sum()
        worst = max(worst, abs(sums[i, 0] - want) / abs(want))
    print("heldout-shapes %-22s loglik per pair %.2e" % (cid, worst))
    assert worst < C.STAGE, (cid, worst)


def test_no_switch_sends_a_replicated_set_elsewhere(V, clean_env):
    """plan_estep_split: a replicated set runs here or nowhere.  With every switch that moves a plain set to another family
    set against it, the plan and the bits are those of the case."""
    for cid in ("a-L5-short", "a-L5-long"):
        c = C.BY_ID[cid]
        want, plan, _ = device_run(V, clean_env, cid, "groups", 3)
        away = dict(c, env=dict(c["env"], VLGP_ESTEP_SPLIT="0", VLGP_ESTEP_LSPLIT="0", VLGP_ESTEP_GENERIC="1"))
        p = C.problem(cid)
        with open_engine(V, away, p, E.set_case_switches(away, clean_env)) as eng:
            assert eng.estep_plan(SRC, 3, vb=True)["family"] not in ("split", "split_mixed", "long_split")
            eng.replicate(SRC, REP, groups=c["groups"])
            got_plan = eng.estep_plan(REP, 3, vb=True)
            assert got_plan == plan, (cid, got_plan, plan)
            assert eng.estep(REP, 3, C.DMU_BOUND, True) == 0 and eng.last_estep_path == c["family"]
            got = eng.download(REP)
        for key in C.FIELDS:
            assert np.array_equal(got[key].reshape(want[key].shape), want[key]), (cid, key)
