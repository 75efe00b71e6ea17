"""vlgp_mstep_cov_masked and vlgp_amd.refit_joint(..., missing=) on the device against their NumPy statement
(tests/joint_em_masked_numpy.py).

  a  every compiled (LT, PT) instantiation of mstep_cov_accum_masked, exact and padded, N = 1 ... 130 (both halves of a
     mask word, a second and a third word), the rows around the LDS row tile and over six workgroups, full / rank-one /
     zero covariances, random masks of 30 % and on top of them a channel without an observed row, rows and a whole unit
     without an observed entry (tests/joint_em_masked_cases.py): a, b, da, db, noise per channel after one and after three
     Newton iterations.  Every case asserts the plan it names (Engine.mstep_plan).
  b  y = NaN at every missing entry gives the bits of a finite y there
  c  an empty mask gives the bits of Engine.mstep_cov on the source set (noise: under VLGP_NOISE_PASSES)
  d  a diagonal cov against the masked Engine.mstep on a masked set holding that v
  e  two calls give the same bits
  f  the kinds of set, the limits and the arguments: each refusal with its status and text, the parameters bit-identical
     afterwards
  g  refit_joint(missing=) against the statement's loop, the trials of a fit carrying ``missing``, the untouched default
     path, and evaluation.joint_posterior(held_out=missing) on what it returns

The reference is the statement, for (c) and (d) the existing entry points; never the new code against itself.  Each
group's bound is a hundred times the largest error measured on an MI355X over its cases
(profiles/joint_em_masked/measured_errors.txt), and no looser than the stage tolerance 1e-9;
tests/test_joint_em_masked_host.py checks without a GPU that every case of (a) is conditioned for it.
"""
import ctypes as C

import numpy as np
import pytest

import joint_em_cases as CS
import joint_em_masked_cases as MC
import joint_em_masked_numpy as EMM
from test_gpu_mstep_shapes import assert_plan, channel_errors, params_of, set_case_switches, units_of
from test_gpu_rates import STAGE

gpu = pytest.mark.gpu

# measured on an MI355X, the worst case of each group (profiles/joint_em_masked/measured_errors.txt):
# a: a-L1-P8 after three iterations; d: diag-f-dead-channel-N24; g: the loop without a mask (with one: 2.28e-15)
MEASURED = {"a": 9.64e-15, "d": 1.13e-15, "g": 2.54e-15}
bound_of = lambda worst: min(100.0 * worst, STAGE)  # noqa: E731
BOUND = bound_of(MEASURED["a"])
BOUND_DIAG = bound_of(MEASURED["d"])
BOUND_LOOP = bound_of(MEASURED["g"])
SWITCHES = ("VLGP_MSTEP_GENERIC", "VLGP_MSTEP_WG_PER_CU", "VLGP_NOISE_PASSES", "VLGP_NO_MGRAPH")
CONFIG = {"Mniter": 5, "use_hessian": True, "eps": 1e-8, "learning_rate": 1.0, "da_bound": 5.0, "db_bound": 5.0,
          "method": "VB", "max_iter": 20, "dmu_bound": 5.0}
SRC, MASKED = 0, 2  # the plain upload and its masked fit set


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def report_and_check(tag, n_iter, got, want, bound):
    errs = channel_errors(got, want)
    print("joint-em-masked %-24s Mniter %d  " % (tag, n_iter) + "  ".join("%s %.2e" % (k, float(e.max())) for k, e in errs.items()))
    for k, e in errs.items():
        assert e.shape == (np.shape(want[0])[1],)
        assert np.all(e < bound), (tag, n_iter, k, int(np.argmax(e)), float(e.max()))  # (a NaN fails)


def set_units(p, y=None):
    """The set holds a mu and a v of its own that the call must not read."""
    return units_of(dict(p, mu=p["set_mu"], v=p["set_v"], y=p["y"] if y is None else y))


def masked_set(eng, units, missing):
    """Set SRC := the units, set MASKED := its masked fit set."""
    if MASKED in eng.sets:
        eng.free_units(MASKED)
    eng.upload(SRC, units)
    eng.replicate(SRC, MASKED, held_out=np.asarray(missing)[None])


def run_masked(V, c, p, n_iter, y=None, missing=None, **kw):
    with V.Engine(c["N"], c["L"], c["P"], 50) as eng:
        plan = assert_plan(eng, c)
        eng.set_params(p["a"], p["b"], np.ones(c["N"]))
        masked_set(eng, set_units(p, y), p["missing"] if missing is None else missing)
        assert eng.mstep_cov_masked(MASKED, p["mu"], p["cov"], n_iter, **kw) == 0  # no singular Newton system
        return params_of(eng), plan


def same_bits(got, want, what):
    for k, g1, g2 in zip(("a", "b", "da", "db", "noise"), got, want):
        assert np.array_equal(g1, g2), (what, k, float(np.max(np.abs(g1 - g2))))


# ---- a ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in MC.MATRIX])
def test_device_against_the_statement(V, cid, clean_env):
    c = MC.BY_ID[cid]
    p, want = MC.problem_and_reference(cid)
    set_case_switches(V, c, clean_env)
    for n_iter in MC.ITERS:
        got, plan = run_masked(V, c, p, n_iter)
        if n_iter == MC.ITERS[0]:
            tiles = -(-min(c["rows"], plan["rows_per_wg"]) // MC.MC_TILE)
            print("joint-em-masked %-24s plan %s, %d LDS row tile(s) per workgroup" % (cid, plan, tiles))
            if c["one_wg"]:
                assert tiles == -(-c["rows"] // MC.MC_TILE)
            elif c["rows"] == 334:
                assert plan["G"] == 6
        report_and_check(cid, n_iter, got, want[n_iter], BOUND)
        if c["mask"] == "dead-channel":  # keeps a, b, noise bit for bit and steps by 0
            d = MC.DEAD_CHANNEL[c["N"]]
            assert np.array_equal(got[0][:, d], p["a"][:, d]) and np.array_equal(got[1][:, d], p["b"][:, d])
            assert got[4][d] == 1.0 and not got[2][:, d].any() and not got[3][:, d].any()
    if c["mask"] == "dead-channel":
        # ... also without the jitter: its systems are the identity, not singular (run_masked asserts the count is 0)
        got, _ = run_masked(V, c, p, 3, eps=0.0)
        want0 = MC.statement(p, 3, eps=0.0)
        assert EMM.mstep_cov_masked.n_failed == 0
        report_and_check(cid + " eps=0", 3, got, want0, BOUND)
        d = MC.DEAD_CHANNEL[c["N"]]
        assert np.array_equal(got[0][:, d], p["a"][:, d]) and np.array_equal(got[1][:, d], p["b"][:, d]) and got[4][d] == 1.0


# ---- b ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", ["a-L5-P1", "a-L4-P2", "a-L10-P8", "c-N65", "c-N130", "f-dead-row"])
def test_nan_at_the_missing_entries_gives_the_same_bits(V, cid, clean_env):
    c = MC.BY_ID[cid]
    p, _ = MC.problem_and_reference(cid)
    finite, _ = run_masked(V, c, p, 3)
    holes, _ = run_masked(V, c, p, 3, y=np.where(p["missing"], np.nan, p["y"]))
    assert all(np.all(np.isfinite(arr)) for arr in holes)
    same_bits(holes, finite, cid)


# ---- c ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", ["a-L5-P1", "a-L3-P1", "a-L4-P2", "a-L10-P8", "c-N1", "c-N130", "e-rows%d-onewg" % (MC.MC_TILE + 1)])
def test_an_empty_mask_gives_the_bits_of_the_unmasked_call(V, cid, clean_env):
    c = MC.BY_ID[cid]
    p, _ = MC.problem_and_reference(cid)
    set_case_switches(V, c, clean_env)
    clean_env.setenv("VLGP_NOISE_PASSES", "1")  # the unmasked noise by its two passes, the form the masked call always takes
    for n_iter in MC.ITERS:
        with V.Engine(c["N"], c["L"], c["P"], 50) as eng:
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            masked_set(eng, set_units(p), np.zeros(p["y"].shape, bool))
            assert eng.mstep_cov(SRC, p["mu"], p["cov"], n_iter) == 0
            want = params_of(eng)
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            assert eng.mstep_cov_masked(MASKED, p["mu"], p["cov"], n_iter) == 0
            same_bits(params_of(eng), want, (cid, n_iter))


# ---- d ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", ["a-L3-P1", "a-L5-P1", "a-L9-P2", "f-dead-channel-N24"])
def test_a_diagonal_cov_is_the_masked_mstep_of_that_v(V, cid, clean_env):
    c = MC.BY_ID[cid]
    p = MC.make_problem(c)
    L = c["L"]
    cov = np.zeros(p["v"].shape + (L,))
    cov[:, np.arange(L), np.arange(L)] = p["v"]
    for n_iter in MC.ITERS:
        with V.Engine(c["N"], L, c["P"], 50) as eng:
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            masked_set(eng, units_of(p), p["missing"])
            assert eng.mstep(MASKED, n_iter) == 0
            want = params_of(eng)
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            masked_set(eng, set_units(p), p["missing"])
            assert eng.mstep_cov_masked(MASKED, p["mu"], cov, n_iter) == 0
            report_and_check("diag-" + cid, n_iter, params_of(eng), want, BOUND_DIAG)


# ---- e ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", ["a-L5-P1", "a-L7-P4", "f-dead-unit"])
def test_two_calls_give_the_same_bits(V, cid, clean_env):
    c = MC.BY_ID[cid]
    p, _ = MC.problem_and_reference(cid)
    runs = []
    with V.Engine(c["N"], c["L"], c["P"], 50) as eng:
        masked_set(eng, set_units(p), p["missing"])
        for _ in range(2):
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            assert eng.mstep_cov_masked(MASKED, p["mu"], p["cov"], 3) == 0
            runs.append(params_of(eng))
    same_bits(runs[0], runs[1], cid)


# ---- f ----------------------------------------------------------------------------------------------------------------
def refused(V, eng, call, status, text):
    before = eng.get_params()
    with pytest.raises(V.VlgpError, match="status %d.*%s" % (status, text)):
        call()
    for b4, now in zip(before, eng.get_params()):
        assert np.array_equal(b4, now, equal_nan=True)


def raw_call(eng, mu, cov, n_iter=1):
    dp = lambda arr: None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    eng._ck(eng.lib.vlgp_mstep_cov_masked(eng.h, MASKED, dp(mu), dp(cov), n_iter, 1, 1e-8, 1.0, 5.0, 5.0, None))


@gpu
def test_kinds_of_set(V, clean_env):
    import test_gpu_set_kinds as SK

    from oracle import vlgp_oracle as O

    rng = np.random.default_rng(3)  # (the problem of that module: two units of T bins, priors for T and the window W)
    p = {"a": 0.3 * rng.standard_normal((SK.L, SK.N)), "b": np.full((1, SK.N), -1.0), "noise": np.ones(SK.N)}
    p["units"] = [{"y": rng.poisson(0.4, (SK.T, SK.N)).astype(float), "x": None, "mu": 0.1 * rng.standard_normal((SK.T, SK.L)),
                   "v": np.ones((SK.T, SK.L)), "w": 0.5 + rng.random((SK.T, SK.L))} for _ in range(2)]
    p["prior"] = O.build_prior([SK.T, SK.W], np.array([2e-2, 5e-3, 1e-3]), np.ones(SK.L), 50)
    one = rng.random((2 * SK.T, SK.N)) < 0.3
    p["held"] = np.stack([one, ~one & (rng.random((2 * SK.T, SK.N)) < 0.3)])
    y_all = np.concatenate([u["y"] for u in p["units"]])

    def make(eng, kind):
        """test_gpu_set_kinds.make: sets 0 ... 3 emptied, set 0 := the plain upload, then the set of `kind`."""
        for sid in (1, 2, 3, 0):
            eng.free_units(sid)
        eng.upload(0, p["units"])
        if kind == "plain":
            return 0, 2 * SK.T
        if kind == "tiling":
            eng.cut(0, 1, np.array([0, SK.T]), SK.T)
            return 1, 2 * SK.T
        if kind == "copied":
            eng.cut(0, 1, np.array([0, SK.T, SK.T - SK.W, 2 * SK.T - SK.W]), SK.W)
            eng.set_overlaps(1, [0, 2, 4], [[0, 2, 2 * SK.W - SK.T], [1, 3, 2 * SK.W - SK.T]], [0, 0, 2])
            return 1, 4 * SK.W
        kw = {"groups": dict(groups=SK.GROUPS), "masked2": dict(held_out=p["held"]), "masked1": dict(held_out=p["held"][:1])}[kind]
        eng.replicate(0, 2, **kw)
        return 2, eng.sets[2][1]

    with SK.engine(V, p) as eng:
        for kind in SK.KINDS:
            sid, rows = make(eng, kind)
            mu = 0.3 * rng.standard_normal((rows, SK.L))
            cov = CS.make_cov("full", 0.02 + 0.05 * rng.random((rows, SK.L)), rng)
            if kind in ("plain", "tiling", "copied"):
                refused(V, eng, lambda: eng.mstep_cov_masked(sid, mu, cov, 1), -3,
                        r"vlgp_mstep_cov_masked takes a masked fit set \(set %d has no mask: vlgp_mstep_cov takes it\)" % sid)
            elif kind in ("groups", "masked2"):
                refused(V, eng, lambda: eng.mstep_cov_masked(sid, mu, cov, 1), -3,
                        SK.REPLICATED[len("status -3.*"):] % "vlgp_mstep_cov_masked")
            else:
                assert rows == 2 * SK.T and eng.mstep_cov_masked(sid, mu, cov, 2) == 0
                want = EMM.mstep_cov_masked(y_all, np.ones((rows, 1, SK.N)), mu, cov, p["a"], p["b"], p["held"][0], 2,
                                            noise=p["noise"])
                report_and_check("kind-" + kind, 2, params_of(eng), want, BOUND)


@gpu
def test_limits_and_arguments(V, clean_env):
    rng = np.random.default_rng(0)
    rows = 30

    def engine(L, P, gauss=None):
        eng = V.Engine(6, L, P, 20, gauss)
        eng.set_params(0.1 * rng.standard_normal((L, 6)), np.zeros((P, 6)), np.ones(6))
        x = np.ones((rows, P, 6))
        x[:, 1:] = rng.standard_normal((rows, P - 1, 6))
        masked_set(eng, [{"y": rng.poisson(1.0, (rows, 6)).astype(float), "x": x, "mu": np.zeros((rows, L)),
                          "v": np.zeros((rows, L)), "w": np.ones((rows, L))}], rng.random((rows, 6)) < 0.3)
        return eng, np.zeros((rows, L)), np.zeros((rows, L * (L + 1) // 2))

    call = lambda eng, mu, cov, n=1: eng.mstep_cov_masked(MASKED, mu, cov, n)  # noqa: E731
    eng, mu, cov = engine(3, 1, np.array([0, 0, 1, 0, 0, 0], dtype=bool))
    with eng:
        refused(V, eng, lambda: call(eng, mu, cov), -3, "vlgp_mstep_cov_masked: the handle has Gaussian channels")
    eng, mu, cov = engine(11, 1)
    with eng:
        refused(V, eng, lambda: call(eng, mu, cov), -3, r"vlgp_mstep_cov_masked: more than 10 latents \(L > 10\)")
    eng, mu, cov = engine(3, 9)
    with eng:
        refused(V, eng, lambda: call(eng, mu, cov), -3, r"vlgp_mstep_cov_masked: more than 8 regressors \(P > 8\)")
    clean_env.setenv("VLGP_MSTEP_GENERIC", "1")
    eng, mu, cov = engine(3, 1)
    with eng:
        refused(V, eng, lambda: call(eng, mu, cov), -3, "vlgp_mstep_cov_masked: VLGP_MSTEP_GENERIC is set")
    clean_env.delenv("VLGP_MSTEP_GENERIC")
    eng, mu, cov = engine(3, 1)
    with eng:
        refused(V, eng, lambda: raw_call(eng, None, cov), -1, "vlgp_mstep_cov_masked needs mu")
        refused(V, eng, lambda: raw_call(eng, mu, None), -1, "vlgp_mstep_cov_masked needs cov")
        refused(V, eng, lambda: call(eng, mu, cov, 0), -1, "vlgp_mstep_cov_masked: n_iter must be at least 1")
        bad = mu.copy()
        bad[17, 1] = np.nan
        bad[23, 0] = np.inf
        refused(V, eng, lambda: call(eng, bad, cov), -1, "vlgp_mstep_cov_masked: mu or cov of row 17 is not finite")
        badc = cov.copy()
        badc[rows - 1, 4] = np.nan
        refused(V, eng, lambda: call(eng, mu, badc), -1, "mu or cov of row %d is not finite" % (rows - 1))
        with pytest.raises(ValueError, match="symmetric"):
            full = np.zeros((rows, 3, 3))
            full[4, 1, 0] = 0.5
            call(eng, mu, full)
        with pytest.raises(ValueError, match="mu must be"):
            call(eng, mu[:-1], cov)
        # the source of the masked set is refused as the source it is, by the unmasked call as well
        refused(V, eng, lambda: eng.mstep_cov_masked(SRC, mu, cov, 1), -3, "source of a replicated set")
        assert call(eng, mu, cov) == 0  # ... and the handle still works
        assert eng.mstep(MASKED, 1) == 0


# ---- g ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    units, params, gauss, missing = EMM.tiny_problem()
    want = EMM.refit_masked(units, missing, params["a"], params["b"], params["noise"], gauss, params["cholesky"],
                            CONFIG["Mniter"], max_iter=3, tol=0.0)
    return {"units": units, "params": params, "gauss": gauss, "missing": missing, "want": want}


def loop_errors(fit, want):
    trace = fit["config"]["runtime"]["joint"]
    errs = {"laplace": np.max(np.abs(np.array(trace["laplace"]) - want["trace"]["laplace"]) / np.abs(want["trace"]["laplace"]))}
    got = (fit["params"]["a"], fit["params"]["b"], fit["params"]["da"], fit["params"]["db"], fit["params"]["noise"])
    ref = (want["a"], want["b"], want["da"], want["db"], want["noise"])
    errs.update({k: float(e.max()) for k, e in channel_errors(got, ref).items() if k in ("a", "b", "noise")})
    mu = np.concatenate([tr["mu"] for tr in fit["trials"]])
    cov = np.concatenate([tr["cov"] for tr in fit["trials"]])
    errs["mu"] = float(np.max(np.abs(mu - want["mu"])) / np.max(np.abs(want["mu"])))
    errs["cov"] = float(np.max(np.abs(cov - want["cov"])) / np.max(np.abs(want["cov"])))
    return errs


@gpu
def test_refit_joint_with_missing_follows_the_statements_loop(V, tiny, clean_env):
    import masked_fit_numpy as MF

    units, params, missing, want = tiny["units"], tiny["params"], tiny["missing"], tiny["want"]
    # the caller's y holds NaN at every missing entry: nothing of it may be read
    holes = [dict(u, y=np.where(m, np.nan, u["y"])) for u, m in zip(units, missing)]
    keep = [dict(u) for u in holes], dict(params), [m.copy() for m in missing]
    fit = V.refit_joint(holes, params, CONFIG, max_iter=3, tol=0.0, newton_tol=1e-20, verbose=False, missing=missing)
    for u, k in zip(holes, keep[0]):  # the caller's dicts are as they were
        assert set(u) == set(k) and all(u[key] is k[key] for key in k)
    assert set(params) == set(keep[1]) and all(params[key] is keep[1][key] for key in params)
    assert all(np.array_equal(m, k) for m, k in zip(missing, keep[2]))
    trace = fit["config"]["runtime"]["joint"]
    assert len(trace["laplace"]) == 4 and all(trace["converged"]) and "runtime" not in CONFIG
    errs = loop_errors(fit, want)
    # w of the returned mode: the curvature summed over the observed channels of every row
    for tr, u, m in zip(fit["trials"], units, missing):
        assert np.array_equal(tr["missing"], m) and tr["y"] is not None and np.all(np.isnan(tr["y"][m]))
        assert np.array_equal(tr["v"], np.diagonal(tr["cov"], axis1=1, axis2=2))
        x = np.ones((u["y"].shape[0], 1, params["ydim"]))
        w_ref = MF.curvature_masked(x, tr["mu"], tr["v"], fit["params"]["a"], fit["params"]["b"], fit["params"]["noise"],
                                    tiny["gauss"], ~m)
        errs["w"] = max(errs.get("w", 0.0), float(np.max(np.abs(tr["w"] - w_ref)) / np.max(np.abs(w_ref))))
    print("joint-em-masked refit_joint  " + "  ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < BOUND_LOOP, (k, e)
    # the trials of a fit carry their masks: the same call without the argument, bit for bit
    carried = V.refit_joint([dict(u, missing=m) for u, m in zip(holes, missing)], params, CONFIG, max_iter=3, tol=0.0,
                            newton_tol=1e-20, verbose=False)
    assert carried["config"]["runtime"]["joint"] == trace
    for key in ("a", "b", "noise", "da", "db"):
        assert np.array_equal(carried["params"][key], fit["params"][key]), key
    for t1, t2 in zip(carried["trials"], fit["trials"]):
        for key in ("mu", "v", "cov", "w", "missing"):
            assert np.array_equal(t1[key], t2[key]), key
    # the returned dicts are a start for the evaluation functions, which take the mask as held_out: the joint posterior of
    # the observed entries, run to the same Newton tolerance from the returned mu, w, has the last recorded evidence
    # (the mode is unique; STAGE relative, as two routes to one sum)
    plain = [{k: (u["y"] if k == "y" else v) for k, v in tr.items() if k != "missing"} for tr, u in zip(fit["trials"], units)]
    ev = V.evaluation.joint_posterior(plain, fit["params"], CONFIG, infer=False, held_out=missing, tol=1e-20)
    gap = abs(ev["total"] - trace["laplace"][-1]) / abs(trace["laplace"][-1])
    print("joint-em-masked refit_joint  evaluation.joint_posterior total %.12f, last recorded %.12f, relative gap %.2e"
          % (ev["total"], trace["laplace"][-1], gap))
    assert gap <= STAGE and ev["n_failed"] == 0
    with pytest.raises(ValueError, match="missing"):  # ... and keep refusing trials that carry `missing`
        V.evaluation.joint_posterior(fit["trials"], fit["params"], CONFIG, infer=False)


@gpu
def test_without_missing_refit_joint_runs_the_unmasked_path(V, tiny, clean_env, monkeypatch):
    """missing=None and no trial carrying one: the code path of before this argument existed -- no masked set is made, the
    M-step is Engine.mstep_cov on the plain set -- asserted by making the masked calls fail, and the result is that of
    joint_em_numpy's loop (tests/test_gpu_joint_em.py holds it to that statement on a problem with Gaussian channels).
    The bits against the parent's build were compared once: profiles/joint_em_masked/bits_parent_vs_this.txt."""
    import joint_em_numpy as EM

    units, params = tiny["units"], tiny["params"]

    def never(*args, **kwargs):
        raise AssertionError("the unmasked refit_joint touched a masked entry point")

    monkeypatch.setattr(V.Engine, "replicate", never)
    monkeypatch.setattr(V.Engine, "mstep_cov_masked", never)
    sets = []
    real = V.Engine.mstep_cov
    monkeypatch.setattr(V.Engine, "mstep_cov", lambda self, sid, *a, **k: (sets.append(sid), real(self, sid, *a, **k))[1])
    fit = V.refit_joint(units, params, CONFIG, max_iter=2, tol=0.0, newton_tol=1e-20, verbose=False)
    assert sets == [0, 0] and all("missing" not in tr for tr in fit["trials"])
    want = EM.refit(units, params["a"], params["b"], params["noise"], tiny["gauss"], params["cholesky"], CONFIG["Mniter"],
                    max_iter=2, tol=0.0)
    errs = loop_errors(fit, want)
    print("joint-em-masked refit_joint without missing  " + "  ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < BOUND_LOOP, (k, e)
