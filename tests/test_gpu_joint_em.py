"""vlgp_mstep_cov and vlgp_amd.refit_joint on the device against their NumPy statement (tests/joint_em_numpy.py).

  a  every compiled (LT, PT) bucket of mstep_cov_accum, exact and padded, mixed, Poisson and all-Gaussian likelihoods,
     N = 1 ... 130, the row geometry around the LDS row tile and the workgroup count, full / rank-one / zero covariances
     (tests/joint_em_cases.py) and the covariance of a real Engine.joint_posterior: a, b, da, db, noise per channel after
     one and after three Newton iterations.  Every case asserts the plan it names (Engine.mstep_plan).
  b  a diagonal cov against Engine.mstep on the same set holding that v
  c  two calls give the same bits
  d  refit_joint against the statement's loop, and evaluation.joint_posterior on what it returns
  e  the refusals, each with its status and text, the parameters bit-identical afterwards

The reference is the statement, for (b) the existing vlgp_mstep; never the new code against itself.  BOUND is a hundred
times the largest error measured on an MI355X over every case of (a), (b) and (d)
(profiles/joint_em/measured_errors.txt), and no looser than the stage tolerance 1e-9; tests/test_joint_em_host.py checks
without a GPU that every case of (a) is conditioned for it.
"""
import ctypes as C

import numpy as np
import pytest

import joint_em_cases as CS
import joint_em_numpy as EM
from test_gpu_mstep_shapes import assert_plan, channel_errors, params_of, set_case_switches, units_of
from test_gpu_rates import STAGE

gpu = pytest.mark.gpu

# measured on an MI355X, the worst case of each group (profiles/joint_em/measured_errors.txt):
MEASURED = {"a": 7.98e-14, "b": 2.58e-15, "d": 2.36e-15}
BOUND = min(100.0 * MEASURED["a"], STAGE)
BOUND_DIAG = min(100.0 * MEASURED["b"], STAGE)
BOUND_LOOP = min(100.0 * MEASURED["d"], STAGE)
SWITCHES = ("VLGP_MSTEP_GENERIC", "VLGP_MSTEP_WG_PER_CU", "VLGP_NOISE_PASSES", "VLGP_NO_MGRAPH")
CONFIG = {"Mniter": 5, "use_hessian": True, "eps": 1e-8, "learning_rate": 1.0, "da_bound": 5.0, "db_bound": 5.0,
          "method": "VB", "max_iter": 20, "dmu_bound": 5.0}


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
    print("joint-em %-24s Mniter %d  " % (tag, n_iter) + "  ".join("%s %.2e" % (k, float(e.max())) for k, e in errs.items()))
    for k, e in errs.items():
        assert e.shape == (np.shape(want[0])[1],)
        assert np.all(e < bound), (tag, n_iter, k, int(np.argmax(e)), float(e.max()))  # (a NaN fails)


def set_units(p):
    """The set holds a mu and a v of its own that the call must not read."""
    return units_of(dict(p, mu=p["set_mu"], v=p["set_v"]))


# ---- a ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CS.MATRIX])
def test_device_against_the_statement(V, cid, clean_env):
    c = CS.BY_ID[cid]
    p, want = CS.problem_and_reference(cid)
    set_case_switches(V, c, clean_env)
    for n_iter in CS.ITERS:
        with V.Engine(c["N"], c["L"], c["P"], 50, p["gauss"]) as eng:
            plan = assert_plan(eng, c)
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            eng.upload(0, set_units(p))
            assert eng.mstep_cov(0, p["mu"], p["cov"], n_iter) == 0  # no singular Newton system
            got = params_of(eng)
        if n_iter == CS.ITERS[0]:
            tiles = -(-min(c["rows"], plan["rows_per_wg"]) // CS.MC_TILE)
            print("joint-em %-24s plan %s, %d LDS row tile(s) per workgroup" % (cid, plan, tiles))
            if c["one_wg"]:
                assert tiles == -(-c["rows"] // CS.MC_TILE)
        if c["P"] > 1 and c["gauss"]:
            assert not got[1][1:, list(c["gauss"])].any()
        report_and_check(cid, n_iter, got, want[n_iter], BOUND)


@pytest.fixture(scope="module")
def tiny():
    units, params, gauss = EM.tiny_problem()
    return {"units": units, "params": params, "gauss": gauss}


def tiny_engine(V, t):
    p = t["params"]
    eng = V.Engine(p["ydim"], p["zdim"], p["xdim"], p["rank"], t["gauss"])
    eng.set_params(p["a"], p["b"], p["noise"])
    eng.upload(0, t["units"])
    for T, G in p["cholesky"].items():
        eng.set_prior(T, G)
    return eng


@gpu
def test_the_cov_of_a_real_joint_posterior(V, tiny, clean_env):
    """The device's own joint posterior handed to both sides: packed as it comes and as (rows, L, L)."""
    p = tiny["params"]
    y, x = EM.cat_units(tiny["units"], p["ydim"])
    with tiny_engine(V, tiny) as eng:
        post = eng.joint_posterior(0)
        assert post["n_failed"] == 0 and np.all(np.abs(post["cov"][:, 1, 0]) > 0)
        for n_iter in CS.ITERS:
            want = EM.mstep_cov(y, x, post["mu"], post["cov"], p["a"], p["b"], tiny["gauss"], n_iter)
            eng.set_params(p["a"], p["b"], p["noise"])
            assert eng.mstep_cov(0, post["mu"], post["cov"], n_iter) == 0
            got = params_of(eng)
            report_and_check("real-posterior", n_iter, got, want, BOUND)
            eng.set_params(p["a"], p["b"], p["noise"])
            from vlgp_amd.engine import pack_cov
            assert eng.mstep_cov(0, post["mu"], pack_cov(post["cov"], post["mu"].shape[0], p["zdim"]), n_iter) == 0
            for g1, g2 in zip(got, params_of(eng)):
                assert np.array_equal(g1, g2)


# ---- b ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("L", [3, 5, 10])
@pytest.mark.parametrize("mix", ["poisson", "mixed", "allgauss"])
def test_a_diagonal_cov_is_the_mstep_of_that_v(V, L, mix, clean_env):
    c = CS.BY_ID["a-L%d-%s" % (L, mix)] if mix != "allgauss" or L != 3 else CS.case("b-L3-allgauss", 24, 3, CS.BASE, gauss=range(24))
    p = CS.make_problem(c)
    cov = np.zeros(p["v"].shape + (L,))
    cov[:, np.arange(L), np.arange(L)] = p["v"]
    for n_iter in CS.ITERS:
        with V.Engine(c["N"], L, 1, 50, p["gauss"]) as eng:
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            eng.upload(0, units_of(p))
            assert eng.mstep(0, n_iter) == 0
            want = params_of(eng)
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            eng.upload(0, set_units(p))
            assert eng.mstep_cov(0, p["mu"], cov, n_iter) == 0
            report_and_check("diag-L%d-%s" % (L, mix), n_iter, params_of(eng), want, BOUND_DIAG)


# ---- c ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", ["a-L5-mixed", "b-L7-P3", "e-rows%d-3wg-L10" % (3 * CS.WG_ROWS - 5)])
def test_two_calls_give_the_same_bits(V, cid, clean_env):
    c = CS.BY_ID[cid]
    p, _ = CS.problem_and_reference(cid)
    runs = []
    with V.Engine(c["N"], c["L"], c["P"], 50, p["gauss"]) as eng:
        eng.upload(0, set_units(p))
        for _ in range(2):
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            assert eng.mstep_cov(0, p["mu"], p["cov"], 3) == 0
            runs.append(params_of(eng))
    for g1, g2 in zip(*runs):
        assert np.array_equal(g1, g2)


# ---- d ----------------------------------------------------------------------------------------------------------------
@gpu
def test_refit_joint_follows_the_statements_loop(V, tiny, clean_env):
    units, params, gauss = tiny["units"], tiny["params"], tiny["gauss"]
    want = EM.refit(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"], CONFIG["Mniter"], max_iter=3,
                    tol=0.0)
    keep = [dict(u) for u in units], dict(params)
    # (both sides run their Newton iterations to a decrement <= 1e-20, as tests/test_gpu_joint.py does: at the default
    # 1e-10 the two modes differ by where the iterations stopped, 1e-7 in mu, which the next M-step hands on)
    fit = V.refit_joint(units, params, CONFIG, max_iter=3, tol=0.0, newton_tol=1e-20, verbose=False)
    for u, k in zip(units, keep[0]):  # the caller's dicts are as they were
        assert set(u) == set(k) and all(u[key] is k[key] for key in k)
    assert set(params) == set(keep[1]) and all(params[key] is keep[1][key] for key in params)
    trace = fit["config"]["runtime"]["joint"]
    assert len(trace["laplace"]) == 4 and all(trace["converged"]) and "runtime" not in CONFIG
    errs = {"laplace": np.max(np.abs(np.array(trace["laplace"]) - want["trace"]["laplace"]) / np.abs(want["trace"]["laplace"]))}
    got = (fit["params"]["a"], fit["params"]["b"], fit["params"]["da"], fit["params"]["db"], fit["params"]["noise"])
    ref = (want["a"], want["b"], want["da"], want["db"], want["noise"])
    errs.update({k: float(e.max()) for k, e in channel_errors(got, ref).items() if k in ("a", "b", "noise")})
    mu = np.concatenate([tr["mu"] for tr in fit["trials"]])
    cov = np.concatenate([tr["cov"] for tr in fit["trials"]])
    errs["mu"] = float(np.max(np.abs(mu - want["mu"])) / np.max(np.abs(want["mu"])))
    errs["cov"] = float(np.max(np.abs(cov - want["cov"])) / np.max(np.abs(want["cov"])))
    print("joint-em refit_joint  " + "  ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < BOUND_LOOP, (k, e)
    for tr in fit["trials"]:
        assert np.array_equal(tr["v"], np.diagonal(tr["cov"], axis1=1, axis2=2)) and tr["w"].shape == tr["mu"].shape
        assert np.all(np.isfinite(tr["w"]))
    # the returned dicts are a start for the evaluation functions: their joint posterior, run to the same Newton tolerance
    # from the returned mu, w, has the last recorded evidence (the mode is unique; STAGE relative, as two routes to one sum)
    ev = V.evaluation.joint_posterior(fit["trials"], fit["params"], CONFIG, infer=False, cov=True, tol=1e-20)
    gap = abs(ev["total"] - trace["laplace"][-1]) / abs(trace["laplace"][-1])
    print("joint-em refit_joint  evaluation.joint_posterior total %.12f, last recorded %.12f, relative gap %.2e"
          % (ev["total"], trace["laplace"][-1], gap))
    assert gap <= STAGE and ev["n_failed"] == 0
    cov_ev = np.concatenate(ev["cov"])
    assert np.max(np.abs(cov_ev - cov)) <= STAGE * np.max(np.abs(cov))


# ---- e ----------------------------------------------------------------------------------------------------------------
def refused(V, eng, call, status, text):
    before = eng.get_params()
    with pytest.raises(V.VlgpError, match="status %d.*%s" % (status, text)):
        call()
    for b4, now in zip(before, eng.get_params()):
        assert np.array_equal(b4, now, equal_nan=True)


def raw_call(eng, mu, cov, n_iter=1):
    dp = lambda arr: None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    eng._ck(eng.lib.vlgp_mstep_cov(eng.h, 0, dp(mu), dp(cov), n_iter, 1, 1e-8, 1.0, 5.0, 5.0, None))


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
    # the rows each admitted kind holds: the upload's, the same rows as two windows of T, four windows of W stage-major
    starts = [0, SK.T, SK.T - SK.W, 2 * SK.T - SK.W]
    rows_of = {"plain": y_all, "tiling": y_all, "copied": np.concatenate([y_all[s0:s0 + SK.W] for s0 in starts])}
    gauss = np.zeros(SK.N, bool)
    with SK.engine(V, p) as eng:
        for kind in SK.KINDS:
            sid, rows, _ = SK.make(eng, p, kind)
            mu = 0.3 * rng.standard_normal((rows, SK.L))
            cov = CS.make_cov("full", 0.02 + 0.05 * rng.random((rows, SK.L)), rng)
            if kind in ("plain", "tiling", "copied"):
                # a cut reads its own rows of y: the statement on those rows, and the bits of a plain upload of them
                y = rows_of[kind]
                assert y.shape[0] == rows
                assert eng.mstep_cov(sid, mu, cov, 2) == 0
                got = params_of(eng)
                want = EM.mstep_cov(y, np.ones((rows, 1, SK.N)), mu, cov, p["a"], p["b"], gauss, 2)
                report_and_check("kind-" + kind, 2, got, want, BOUND)
                with SK.engine(V, p) as plain:
                    plain.upload(0, [{"y": y, "x": None, "mu": np.zeros((rows, SK.L)), "v": np.zeros((rows, SK.L)),
                                      "w": np.zeros((rows, SK.L))}])
                    assert plain.mstep_cov(0, mu, cov, 2) == 0
                    for g1, g2 in zip(got, params_of(plain)):
                        assert np.array_equal(g1, g2), kind
                eng.set_params(p["a"], p["b"], p["noise"])
            else:
                refused(V, eng, lambda: eng.mstep_cov(sid, mu, cov, 1), -3, SK.REPLICATED[len("status -3.*"):] % "vlgp_mstep_cov")


@gpu
def test_limits_and_arguments(V, clean_env):
    rng = np.random.default_rng(0)
    rows = 30

    def engine(L, P):
        eng = V.Engine(6, L, P, 20)
        eng.set_params(0.1 * rng.standard_normal((L, 6)), np.zeros((P, 6)), np.ones(6))
        x = np.ones((rows, P, 6))
        x[:, 1:] = rng.standard_normal((rows, P - 1, 6))
        eng.upload(0, [{"y": rng.poisson(1.0, (rows, 6)).astype(float), "x": x, "mu": np.zeros((rows, L)),
                        "v": np.zeros((rows, L)), "w": np.ones((rows, L))}])
        return eng, np.zeros((rows, L)), np.zeros((rows, L * (L + 1) // 2))

    eng, mu, cov = engine(11, 1)
    with eng:
        refused(V, eng, lambda: eng.mstep_cov(0, mu, cov, 1), -3, r"more than 10 latents \(L > 10\)")
    eng, mu, cov = engine(3, 9)
    with eng:
        refused(V, eng, lambda: eng.mstep_cov(0, mu, cov, 1), -3, r"more than 8 regressors \(P > 8\)")
    clean_env.setenv("VLGP_MSTEP_GENERIC", "1")
    eng, mu, cov = engine(3, 1)
    with eng:
        refused(V, eng, lambda: eng.mstep_cov(0, mu, cov, 1), -3, "VLGP_MSTEP_GENERIC is set")
    clean_env.delenv("VLGP_MSTEP_GENERIC")
    eng, mu, cov = engine(3, 1)
    with eng:
        refused(V, eng, lambda: raw_call(eng, None, cov), -1, "vlgp_mstep_cov needs mu")
        refused(V, eng, lambda: raw_call(eng, mu, None), -1, "vlgp_mstep_cov needs cov")
        refused(V, eng, lambda: eng.mstep_cov(0, mu, cov, 0), -1, "n_iter must be at least 1")
        bad = mu.copy()
        bad[17, 1] = np.nan
        bad[23, 0] = np.inf
        refused(V, eng, lambda: eng.mstep_cov(0, bad, cov, 1), -1, "mu or cov of row 17 is not finite")
        badc = cov.copy()
        badc[rows - 1, 4] = np.nan
        refused(V, eng, lambda: eng.mstep_cov(0, mu, badc, 1), -1, "mu or cov of row %d is not finite" % (rows - 1))
        with pytest.raises(ValueError, match="symmetric"):
            full = np.zeros((rows, 3, 3))
            full[4, 1, 0] = 0.5
            eng.mstep_cov(0, mu, full, 1)
        assert eng.mstep_cov(0, mu, cov, 1) == 0  # ... and the handle still works
