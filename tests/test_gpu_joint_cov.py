"""The joint Laplace posterior with its per-row covariance and held-out entries (vlgp_joint_posterior,
Engine.joint_posterior), the row scores under a supplied covariance (vlgp_predictive_cov, vlgp_calibration_cov) and the
posterior="joint" path of vlgp_amd.evaluation, against the NumPy statement of their definitions
(tests/joint_cov_numpy.py).

Tolerances.  The posterior follows tests/test_gpu_joint.py: sums relative to the sum of the absolute values of their
terms, entries (beta, mu, cov) relative to max(1, largest entry of the unit), both sides run to a decrement <= 1e-20.
TOL = 5e-13 is that file's bound, 100 times the error of v it measured (4.4e-15): a cov entry is the same two
substitutions and the same two-level sum as v over a block of H^-1 beside the diagonal one, so it may differ from the
dense inverse by what v does and no more; an error above that bound is not rounding (measured: cov at most 5.9e-15).
The scores follow tests/test_gpu_predictive.py (entries relative to max(1, |statement|)) and
tests/test_gpu_calibration.py (sums relative to the sum of their absolute terms; counts equal): the entry is theirs with
another m and s2.  Measured on one MI355X over the three forms of set at 1, 12 and 64 nodes: at most 3.55e-15 per entry
and 2.83e-15 per sum; SCORE_TOL is 100 times the largest.  Every case prints its errors
(profiles/joint_cov/measured_errors.txt).

A masked set starts its Newton iteration at beta = 0 where the plain set starts at the mean-field centres, so the set
with no bit set cannot be compared with the plain set bit for bit, nor at TOL: the two iterations reach the one mode by
different steps and each stops where its own decrement is <= 1e-20, that is within 1e-10 of the mode in the norm of H.
H >= I and a row of a prior factor has norm <= 1, so their beta and mu lie within START_TOL = 2e-10 of each other
(tests/test_gpu_joint.py's docstring has the same bound); cov and laplace are smooth in beta and are held to the same
figure.  Against the statement, which takes the same start as the device, the masked set with no bit set is held to TOL
like every other.  The bits that must be equal are asserted: beta, stats and mu of vlgp_joint_laplace on a plain set, its
v on the diagonal of cov, and a repeated call.

The public path runs its Newton iteration at evaluation's default tol = 1e-10.  A decrement <= 1e-10 bounds the
distance to the mode in the norm of H, and H >= I, by 1e-5; a row of a prior factor has norm <= 1 (sigma = 1), so no
latent moves by more than 1e-5 and no linear predictor by more than 1e-5 max_n sum_l |a_ln| < 2e-5 here; a log density
moves by at most (y + rate) times that.  PUBLIC_TOL = 1e-4 on |device - statement| / max(1, |statement|) for rates and
on sums relative to sum (y + rate) is five times that bound; measured errors are far smaller, since the last step
squares the decrement.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import calibration_numpy as CN
import heldout_numpy as H
import joint_cov_numpy as JC
import joint_numpy as JN
from oracle import vlgp_oracle as O
from test_gpu_calibration import check_margin, counts_equal, entry_err, sums_err
from test_gpu_joint import CASES, NEWTON_TOL, TOL
from test_gpu_marginal import SET, _engine, _problem

pytestmark = pytest.mark.gpu

SCORE_TOL = 3.6e-13  # 100 x the largest measured error of the scores (module docstring)
PUBLIC_TOL = 1e-4
START_TOL = 2e-10
REP = 2  # the set the replicas go to


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))


@functools.lru_cache(maxsize=None)
def _case(name):
    lengths, N, L, omega, n_gauss, history = CASES[name]
    units, params, gauss = _problem(lengths, N, L, omega, seed=11, n_gauss=n_gauss, history=history)
    return units, params, gauss


def _args(params, gauss):
    return params["a"], params["b"], params["noise"], gauss, params["cholesky"]


def _errors(name, dev, st, units):
    """Errors of Engine.joint_posterior's dict against the statement's per-unit dicts, printed; returns them."""
    err = {"beta": 0.0, "mu": 0.0, "cov": 0.0, "laplace": 0.0, "ll": 0.0, "logdet": 0.0}
    row = 0
    for i, s in enumerate(st):
        T = units[i]["y"].shape[0]
        err["beta"] = max(err["beta"], _rel(JN.stack_beta(dev["beta"][i], s["ranks"]), s["beta"]))
        err["mu"] = max(err["mu"], _rel(dev["mu"][row:row + T], s["mu"]))
        err["cov"] = max(err["cov"], _rel(dev["cov"][row:row + T], s["cov"]))
        for key in ("laplace", "ll", "logdet"):
            err[key] = max(err[key], abs(dev[key][i] - s[key]) / s["scale"])
        assert dev["D"][i] == sum(s["ranks"])
        row += T
    print("joint_cov errors [%s] units %d D %s newton %s: %s" % (name, len(st), dev["D"].tolist(), dev["n_newton"].tolist(),
                                                                  ", ".join("%s %.2e" % kv for kv in err.items())))
    return err


# ---- plain sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_plain_set_is_joint_laplace_with_the_statements_covariance(V, name):
    units, params, gauss = _case(name)
    L = params["zdim"]
    st = JC.statement(units, *_args(params, gauss))
    with _engine(V, units, params, gauss) as eng:
        lap = eng.joint_laplace(SET, max_iter=50, tol=NEWTON_TOL)
        dev = eng.joint_posterior(SET, max_iter=50, tol=NEWTON_TOL)
        again = eng.joint_posterior(SET, max_iter=50, tol=NEWTON_TOL)
    rows = sum(u["y"].shape[0] for u in units)
    assert dev["cov"].shape == (rows, L, L) and dev["n_failed"] == 0 and np.all(dev["converged"])
    for key in ("beta", "stats", "mu"):
        assert dev[key].tobytes() == lap[key].tobytes(), key
    assert np.ascontiguousarray(np.diagonal(dev["cov"], axis1=1, axis2=2)).tobytes() == lap["v"].tobytes()
    assert np.array_equal(dev["cov"], dev["cov"].transpose(0, 2, 1))
    for key in ("beta", "stats", "mu", "cov"):
        assert dev[key].tobytes() == again[key].tobytes(), key
    err = _errors(name, dev, st, units)
    for key, val in err.items():
        assert val <= TOL, (name, key, val)


# ---- masked sets ------------------------------------------------------------------------------------------------------
MASKED_CASES = ("L3_five_channels", "L3_seventy_mixed_regressors")  # (N = 70: two mask words)
MASKS = ("none", "row", "channel", "random")


def _mask(kind, rows, N):
    held = np.zeros((rows, N), bool)
    if kind == "row":
        held[70] = True  # (a row of the 64-bin unit: rows 8 ... 71)
    elif kind == "channel":
        held[:, N - 1] = True
    elif kind == "random":
        held = np.random.default_rng(3).random((rows, N)) < 0.2
    return held


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", MASKED_CASES)
def test_masked_set_equals_the_statement_and_never_reads_a_held_out_entry(V, name, kind):
    units, params, gauss = _case(name)
    rows, N = sum(u["y"].shape[0] for u in units), params["ydim"]
    held = _mask(kind, rows, N)
    st = JC.statement(units, *_args(params, gauss), held=held)
    poisoned, row = [], 0
    for u in units:  # NaN where held out; the regressors of the history case are built from the clean counts
        T = u["y"].shape[0]
        poisoned.append(dict(u, y=np.where(held[row:row + T], np.nan, u["y"])))
        row += T
    with _engine(V, poisoned, params, gauss) as eng:
        eng.replicate(SET, REP, held_out=held[None])
        dev = eng.joint_posterior(REP, max_iter=50, tol=NEWTON_TOL)
        eng.free_units(REP)
        plain = eng.joint_posterior(SET, max_iter=50, tol=NEWTON_TOL) if kind == "none" else None
    assert dev["n_failed"] == 0 and np.all(dev["converged"]) and np.all(dev["decrement"] <= NEWTON_TOL)
    for key in ("beta", "stats", "mu", "cov"):
        assert np.all(np.isfinite(dev[key])), key
    err = _errors("%s masked %s" % (name, kind), dev, st, units)
    for key, val in err.items():
        assert val <= TOL, (name, kind, key, val)
    if plain is not None:  # no bit set: the plain set's numbers, from another start (module docstring)
        gap = {key: _rel(dev[key], plain[key]) for key in ("beta", "mu", "cov")}
        scale = np.array([s["scale"] for s in st])
        gap["laplace"] = float(np.max(np.abs(dev["laplace"] - plain["laplace"]) / scale))
        print("joint_cov errors [%s no bit set against the plain set]: %s" % (name, ", ".join("%s %.2e" % kv for kv in gap.items())))
        assert max(gap.values()) <= START_TOL, gap


# ---- the scores under a supplied covariance ---------------------------------------------------------------------------
GROUPS = [[1, 3], [4]]
NODES = (1, 12, 64)
N_BINS, LEVELS = 10, (0.5, 0.9)


@functools.lru_cache(maxsize=None)
def _score_problem():
    """267 rows in five ragged units (two workgroups), N = 5 with two Gaussian channels, L = 3, and for up to two replicas a
    random mean and a random SPD covariance per row."""
    units, params, gauss = _problem([1, 7, 64, 65, 130], 5, 3, [2e-2, 5e-3, 1e-3], seed=11, n_gauss=2)
    units = [dict(u, x=np.ones((u["y"].shape[0], 1, 5))) for u in units]  # (the restatements take x as an array)
    rng = np.random.default_rng(17)
    rows = sum(u["y"].shape[0] for u in units)
    mu = 0.5 * rng.standard_normal((2, rows, 3))
    root = rng.standard_normal((2, rows, 3, 3))
    cov = 0.15 * (root @ root.transpose(0, 1, 3, 2)) + 0.01 * np.eye(3)
    held = np.zeros((2, rows, 5), bool)
    pick = rng.random((rows, 5))
    held[0], held[1] = pick < 0.3, (pick >= 0.3) & (pick < 0.5)
    return units, params, gauss, mu, cov, held


def _forms(eng, mu, cov, held):
    """(name, set, mu, cov, kwargs of the statement) of the three forms of set, made on `eng` one after the other."""
    rows = mu.shape[1]
    yield "plain", SET, mu[:1], cov[:1], {}
    eng.replicate(SET, REP, groups=GROUPS)
    yield "groups", REP, mu, cov, {"groups": GROUPS}
    eng.free_units(REP)
    eng.replicate(SET, REP, held_out=held)
    yield "masked", REP, mu, cov, {"held": held}
    eng.free_units(REP)
    assert rows == eng.sets[SET][1]


@pytest.mark.parametrize("n_nodes", NODES)
def test_predictive_cov_equals_the_statement_on_every_form_of_set(V, n_nodes):
    units, params, gauss, mu, cov, held = _score_problem()
    a, b, noise = params["a"], params["b"], params["noise"]
    with _engine(V, units, params, gauss) as eng:
        for form, sid, m, c, kw in _forms(eng, mu, cov, held):
            sums, rate, lpd = eng.predictive(sid, n_nodes=n_nodes, want_rate=True, want_lpd=True,
                                             mu=m.reshape(-1, 3), cov=c.reshape(-1, 3, 3))
            only_sums = eng.predictive(sid, n_nodes=n_nodes, mu=m.reshape(-1, 3), cov=c.reshape(-1, 3, 3))[0]
            want_lpd, want_rate, want_sums = JC.score_predictive(units, m, c, a, b, noise, gauss, n_nodes, **kw)
            errs = (entry_err(lpd, want_lpd), entry_err(rate, want_rate), entry_err(sums, want_sums))
            print("joint_cov errors [predictive_cov %s, %d nodes]: lpd %.2e, rate %.2e, sums %.2e" % ((form, n_nodes) + errs))
            assert max(errs) <= SCORE_TOL, (form, errs)
            assert only_sums.tobytes() == sums.tobytes()


@pytest.mark.parametrize("n_nodes", NODES)
def test_calibration_cov_equals_the_statement_on_every_form_of_set(V, n_nodes):
    units, params, gauss, mu, cov, held = _score_problem()
    a, b, noise = params["a"], params["b"], params["noise"]
    with _engine(V, units, params, gauss) as eng:
        for form, sid, m, c, kw in _forms(eng, mu, cov, held):
            sums, cdf = eng.calibration(sid, n_bins=N_BINS, levels=LEVELS, n_nodes=n_nodes, want_cdf=True,
                                        mu=m.reshape(-1, 3), cov=c.reshape(-1, 3, 3))
            want_cdf, want_sums, terms = JC.score_calibration(units, m, c, a, b, noise, gauss, n_nodes, N_BINS, LEVELS, **kw)
            check_margin(want_cdf, N_BINS, LEVELS)
            axis = 1 if form == "masked" else 0
            errs = (entry_err(cdf, want_cdf), sums_err(sums, want_sums, terms, axis))
            print("joint_cov errors [calibration_cov %s, %d nodes]: cdf %.2e, sums %.2e" % ((form, n_nodes) + errs))
            assert max(errs) <= SCORE_TOL, (form, errs)
            assert counts_equal(sums, want_sums, N_BINS), form


def test_a_diagonal_cov_and_the_sets_own_mu_are_the_mean_field_scores(V):
    """cov = diag(v) and the set's mu: vlgp_predictive(vb = 1) and vlgp_calibration(vb = 1), up to the order of the sum
    behind s2 (a_l (v_l a_l) here, v_l (a_l a_l) there) and the chain of the rate's argument."""
    units, params, gauss, _, _, _ = _score_problem()
    mu = np.concatenate([u["mu"] for u in units])
    v = np.concatenate([u["v"] for u in units])
    cov = np.zeros(v.shape + (3,))
    cov[:, np.arange(3), np.arange(3)] = v
    with _engine(V, units, params, gauss) as eng:
        want = eng.predictive(SET, n_nodes=12, vb=True, want_rate=True, want_lpd=True)
        got = eng.predictive(SET, n_nodes=12, want_rate=True, want_lpd=True, mu=mu, cov=cov)
        cal_want = eng.calibration(SET, n_bins=N_BINS, levels=LEVELS, vb=True, want_cdf=True)
        cal_got = eng.calibration(SET, n_bins=N_BINS, levels=LEVELS, want_cdf=True, mu=mu, cov=cov)
    errs = [entry_err(g, w) for g, w in zip(got, want)] + [entry_err(cal_got[1], cal_want[1])]
    print("joint_cov errors [diagonal cov against the mean-field scores]: %s" % ", ".join("%.2e" % e for e in errs))
    assert max(errs) <= SCORE_TOL
    assert counts_equal(cal_got[0], cal_want[0], N_BINS)
    assert entry_err(cal_got[0][:, :N_BINS + len(LEVELS) + 1], cal_want[0][:, :N_BINS + len(LEVELS) + 1]) <= SCORE_TOL


def test_entries_without_finite_moments_are_nan_or_skipped_and_counted(V):
    units, params, gauss, mu, cov, _ = _score_problem()
    a, b, noise = params["a"], params["b"], params["noise"]
    m, c = mu[:1].copy(), cov[:1].copy()
    c[0, 5] = np.nan            # a row of NaN covariance
    m[0, 100, 1] = np.nan       # a NaN mean
    c[0, 200, 2, 2] = np.inf    # an infinite variance
    bad = [5, 100, 200]
    with _engine(V, units, params, gauss) as eng:
        sums, rate, lpd = eng.predictive(SET, want_rate=True, want_lpd=True, mu=m[0], cov=c[0])
        csums, cdf = eng.calibration(SET, n_bins=N_BINS, levels=LEVELS, want_cdf=True, mu=m[0], cov=c[0])
    want_lpd, want_rate, want_sums = JC.score_predictive(units, m, c, a, b, noise, gauss, 12)
    assert np.all(np.isnan(lpd[bad])) and np.all(np.isnan(rate[bad]))
    assert max(entry_err(lpd, want_lpd), entry_err(rate, want_rate)) <= SCORE_TOL
    assert np.all(np.isnan(sums[:, [0, 2]])) and entry_err(sums[:, [1, 3]], want_sums[:, [1, 3]]) <= SCORE_TOL
    want_cdf, want_csums, terms = JC.score_calibration(units, m, c, a, b, noise, gauss, 12, N_BINS, LEVELS)
    assert np.all(np.isnan(cdf[bad])) and entry_err(cdf, want_cdf) <= SCORE_TOL
    assert np.all(np.isfinite(csums)) and np.all(csums[:, -1] == 3) and np.all(csums[:, -2] == 267 - 3)
    assert counts_equal(csums, want_csums, N_BINS) and sums_err(csums, want_csums, terms, 0) <= SCORE_TOL


# ---- refusals and optional outputs ------------------------------------------------------------------------------------
def test_refusals_by_status_and_text(V):
    from vlgp_amd.engine import dptr, hermite_nodes

    units, params, gauss = _problem([50, 50], 8, 2, [2e-2, 1e-3], seed=4)
    refusal = "status -3.*vlgp_joint_posterior refuses a replicated set"
    z, lwa = hermite_nodes(12)
    lev = np.array([0.5])
    with _engine(V, units, params, gauss) as eng:
        stats, mu, cov = np.empty((2, 8)), np.zeros((100, 2)), np.zeros((100, 3))
        eng.replicate(SET, REP, channels=[1, 3])
        with pytest.raises(V.engine.VlgpError, match=refusal):
            eng.joint_posterior(REP)
        eng.free_units(REP)
        held = np.zeros((2, 100, 8), dtype=bool)
        held[0, ::7, 2] = held[1, 1::7, 3] = True
        eng.replicate(SET, REP, held_out=held)
        with pytest.raises(V.engine.VlgpError, match=refusal):
            eng.joint_posterior(REP)
        eng.free_units(REP)
        with pytest.raises(V.engine.VlgpError, match="status -1.*tol"):
            eng.joint_posterior(SET, tol=0.0)
        with pytest.raises(V.engine.VlgpError, match="status -1.*max_iter"):
            eng.joint_posterior(SET, max_iter=0)
        with pytest.raises(V.engine.VlgpError, match="status -1.*vlgp_joint_posterior needs stats"):
            eng.check(eng.lib.vlgp_joint_posterior(eng.h, SET, 50, 1e-10, None, None, None, None, None))
        sums, csums = np.empty((8, 4)), np.empty((8, 10 + 1 + 3))
        for null, name in ((0, "mu"), (1, "cov")):
            pair = [dptr(mu), dptr(cov)]
            pair[null] = None
            with pytest.raises(V.engine.VlgpError, match="status -1.*vlgp_predictive_cov needs %s" % name):
                eng.check(eng.lib.vlgp_predictive_cov(eng.h, SET, 12, dptr(z), dptr(lwa), pair[0], pair[1], None, None,
                                                      dptr(sums)))
            with pytest.raises(V.engine.VlgpError, match="status -1.*vlgp_calibration_cov needs %s" % name):
                eng.check(eng.lib.vlgp_calibration_cov(eng.h, SET, 12, dptr(z), dptr(lwa), pair[0], pair[1], 10, 1, dptr(lev),
                                                       4096, None, dptr(csums)))
        with pytest.raises(ValueError, match="mu and cov go together"):
            eng.predictive(SET, mu=mu)
        # per-entry output from overlapping masks: the siblings' refusal
        both = np.zeros((2, 100, 8), dtype=bool)
        both[:, 3, 2] = True
        eng.replicate(SET, REP, held_out=both)
        two = (np.zeros((200, 2)), np.tile(np.array([1.0, 0.0, 1.0]), (200, 1)))
        with pytest.raises(V.engine.VlgpError, match="status -1.*vlgp_predictive_cov: the masks of set 2 overlap"):
            eng.predictive(REP, want_lpd=True, mu=two[0], cov=two[1])
        assert np.all(np.isfinite(eng.predictive(REP, mu=two[0], cov=two[1])[0]))
        eng.free_units(REP)


def test_left_out_outputs_change_nothing_in_the_others(V):
    from vlgp_amd.engine import dptr

    units, params, gauss = _problem([1, 7, 65], 5, 3, [2e-2, 5e-3, 1e-3], seed=11)
    rows, L, R = 73, 3, params["rank"]

    def call(eng, omit=()):
        out = {}

        def buf(key, *shape):
            if key in omit:
                return None
            out[key] = np.full(shape, -7.0)
            return dptr(out[key])

        n = C.c_int(-1)
        eng.check(eng.lib.vlgp_joint_posterior(eng.h, SET, 50, 1e-10, buf("beta", 3, L, R), buf("stats", 3, 8),
                                               buf("mu", rows, L), buf("cov", rows, 6),
                                               None if "n_failed" in omit else C.byref(n)))
        if "n_failed" not in omit:
            out["n_failed"] = np.array([n.value])
        return out

    with _engine(V, units, params, gauss) as eng:
        full = call(eng)
        assert all(np.all(np.isfinite(a)) and not np.any(a == -7.0) for a in full.values()) and full["n_failed"][0] == 0
        for omit in [("beta",), ("mu",), ("cov",), ("n_failed",), ("mu", "cov"), ("beta", "mu", "cov", "n_failed")]:
            got = call(eng, omit)
            assert sorted(got) == sorted(set(full) - set(omit)), omit
            for key, arr in got.items():
                assert arr.tobytes() == full[key].tobytes(), (omit, key)


def test_a_nan_in_w_fails_its_unit_alone(V):
    units, params, gauss = _problem([50, 30], 8, 2, [2e-2, 1e-3], seed=4)
    bad = [dict(u) for u in units]
    bad[1]["w"] = bad[1]["w"].copy()
    bad[1]["w"][3, 0] = np.nan
    with _engine(V, units, params, gauss) as eng:
        full = eng.joint_posterior(SET)
    with _engine(V, bad, params, gauss) as eng:
        dev = eng.joint_posterior(SET)
        csums, cdf = eng.calibration(SET, want_cdf=True, mu=dev["mu"], cov=dev["cov"])
    assert dev["n_failed"] == 1 and np.all(np.isnan(dev["stats"][1, :5]))
    assert np.all(np.isnan(dev["mu"][50:])) and np.all(np.isnan(dev["cov"][50:]))
    assert dev["mu"][:50].tobytes() == full["mu"][:50].tobytes() and dev["cov"][:50].tobytes() == full["cov"][:50].tobytes()
    assert np.all(csums[:, -1] == 30) and np.all(csums[:, -2] == 50) and np.all(np.isnan(cdf[50:]))


# ---- the public path --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _public():
    trials, params, config = H.problem(seed=3, M=3, T=40, N=8, L=2, max_iter=4)
    params["cholesky"] = O.build_prior([40], params["omega"], params["sigma"], params["rank"])
    return trials, params, config


def _statement_folds(trials, params, masks):
    """Per mask (rows, N): the joint posterior without it, mu (rows, L) and cov (rows, L, L), converged and n_newton."""
    gauss = np.zeros(params["ydim"], bool)
    units = [{"y": t["y"], "x": t["x"]} for t in trials]
    out = []
    for held in masks:
        st = JC.statement(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"], held=held)
        out.append((np.concatenate([s["mu"] for s in st]), np.concatenate([s["cov"] for s in st]),
                    np.array([s["converged"] for s in st])))
    return units, gauss, out


def _public_err(got, want, scale):
    return float(np.max(np.abs(got - want) / scale))


def test_leave_entries_out_under_the_joint_posterior(V):
    from vlgp_amd import evaluation as EV

    trials, params, config = _public()
    a, b, noise = params["a"], params["b"], params["noise"]
    got = EV.leave_entries_out(trials, params, config, n_folds=3, seed=1, predictive=True, posterior="joint")
    mean_field = EV.leave_entries_out(trials, params, config, n_folds=3, seed=1, predictive=True)
    assert set(got) == set(mean_field) | {"converged", "n_newton"} and got["density"] == "predictive"
    assert got["converged"].shape == got["n_newton"].shape == (3, 3) and np.all(got["converged"]) and got["n_failed"] == 0
    F = np.concatenate(got["folds"])
    masks = np.stack([F == k for k in range(3)])
    units, gauss, folds = _statement_folds(trials, params, masks)
    mu, cov = np.stack([f[0] for f in folds]), np.stack([f[1] for f in folds])
    lpd, rate, sums = JC.score_predictive(units, mu, cov, a, b, noise, gauss, 12, held=masks)
    y = np.concatenate([t["y"] for t in trials])
    scale = np.stack([np.where(m, y + rate, 0.0).sum(axis=0) for m in masks])
    errs = (entry_err(np.concatenate(got["rate"]), rate), _public_err(got["ll_per_fold"], sums[:, :, 0], scale))
    print("joint_cov errors [leave_entries_out joint]: rate %.2e, ll per fold %.2e; speckled_bps joint %.4f mean-field %.4f"
          % (errs + (got["speckled_bps"], mean_field["speckled_bps"])))
    assert max(errs) <= PUBLIC_TOL
    assert abs(got["speckled_bps"] - mean_field["speckled_bps"]) > 1e-6  # another posterior, not the same numbers


def test_calibration_under_the_joint_posterior(V):
    from vlgp_amd import evaluation as EV

    trials, params, config = _public()
    a, b, noise = params["a"], params["b"], params["noise"]
    rows, N = 120, 8
    y = np.concatenate([t["y"] for t in trials])
    for how, kw in (("entries", {"n_folds": 3, "seed": 1}), ("channels", {"groups": [[0, 5], [2], [7, 3, 1]]})):
        got = EV.calibration(trials, params, config, how=how, posterior="joint", **kw)
        if how == "entries":
            F = EV.entry_folds(rows, N, 3, 1)
            masks = np.stack([F == k for k in range(3)])
        else:
            masks = np.stack(list(EV._group_masks(kw["groups"], rows, N)))
        units, gauss, folds = _statement_folds(trials, params, masks)
        mu, cov = np.stack([f[0] for f in folds]), np.stack([f[1] for f in folds])
        cdf, sums, terms = JC.score_calibration(units, mu, cov, a, b, noise, gauss, 12, 10, (0.5, 0.9), held=masks)
        want = EV.calibration_from_sums(sums.sum(axis=0), 10, (0.5, 0.9))
        assert got["converged"].shape == (3, 3) and np.all(got["converged"]) and got["n_failed"] == 0
        assert np.array_equal(got["entries"], want["entries"]) and np.array_equal(got["skipped"], want["skipped"])
        assert np.array_equal(np.isnan(got["coverage"]), np.isnan(want["coverage"]))
        # a count of covered entries may differ by the entries whose lo or hi lies within 10 PUBLIC_TOL of the level's edge
        lo, hi = cdf[..., 0], cdf[..., 1]
        close = np.stack([np.nansum((np.abs(hi - (1 - c) / 2) < 10 * PUBLIC_TOL) | (np.abs(lo - (1 + c) / 2) < 10 * PUBLIC_TOL),
                                    axis=0) for c in (0.5, 0.9)], axis=1)
        moved = np.abs(np.nan_to_num(got["coverage"] - want["coverage"])) * want["entries"][:, None]
        assert np.all(moved <= close + 1e-9), (moved, close)
        errs = (float(np.nanmax(np.abs(got["pit"] - want["pit"]))), float(np.nanmax(np.abs(got["dispersion"] - want["dispersion"])
                                                                                     / np.maximum(1.0, want["dispersion"]))))
        print("joint_cov errors [calibration %s joint]: pit %.2e, dispersion %.2e" % ((how,) + errs))
        assert max(errs) <= 10 * PUBLIC_TOL  # (a PIT share divides an error of lo by the mass hi - lo, up to 10 here)
    in_sample = [dict(t, mu=np.zeros((40, 2)), v=np.zeros((40, 2)), w=np.ones((40, 2))) for t in trials]
    got = EV.calibration(in_sample, params, config, how="in_sample", posterior="joint")
    assert got["converged"].shape == (3,) and np.all(got["converged"]) and np.all(got["entries"] == rows)
    assert abs(float(np.sum(got["pit_all"])) - 1.0) < 1e-12 and y.shape == (rows, N)


def test_leave_group_out_and_joint_posterior_with_held_out(V):
    from vlgp_amd import evaluation as EV

    trials, params, config = _public()
    groups = [[0, 5], [2]]
    got = EV.leave_group_out(trials, params, config, groups=groups, predictive=True, posterior="joint")
    assert got["path"] == "joint" and got["channels"] == [0, 5, 2] and got["converged"].shape == (2, 3)
    assert np.all(got["converged"]) and all(r.shape == (40, 3) for r in got["rate"]) and np.all(np.isfinite(got["ll"]))
    masks = np.stack(list(EV._group_masks(groups, 120, 8)))
    units, gauss, folds = _statement_folds(trials, params, masks)
    mu, cov = np.stack([f[0] for f in folds]), np.stack([f[1] for f in folds])
    _, rate, sums = JC.score_predictive(units, mu, cov, params["a"], params["b"], params["noise"], gauss, 12, held=masks)
    want_ll = np.array([sums[0, 0, 0], sums[0, 5, 0], sums[1, 2, 0]])
    y = np.concatenate([t["y"] for t in trials])
    scale = (y + np.nan_to_num(rate)).sum(axis=0)[[0, 5, 2]]
    errs = (entry_err(np.concatenate(got["rate"]), rate[:, [0, 5, 2]]), _public_err(got["ll"], want_ll, scale))
    print("joint_cov errors [leave_group_out joint]: rate %.2e, ll %.2e" % errs)
    assert max(errs) <= PUBLIC_TOL
    # joint_posterior(held_out=): NaN at the held-out entries changes nothing, and cov's diagonal is v
    held = [m.copy() for m in np.split(masks[0] | (np.random.default_rng(2).random((120, 8)) < 0.2), 3)]
    clean = EV.joint_posterior(trials, params, config, held_out=held)
    dirty = EV.joint_posterior([dict(t, y=np.where(h, np.nan, t["y"])) for t, h in zip(trials, held)], params, config,
                               held_out=held)
    assert set(clean) == {"mu", "v", "cov", "laplace", "converged", "n_newton", "total", "laplace_bps", "n_failed"}
    for key in ("mu", "v", "cov"):
        assert all(c.tobytes() == d.tobytes() for c, d in zip(clean[key], dirty[key])), key
    assert clean["laplace"].tobytes() == dirty["laplace"].tobytes() and np.all(np.isfinite(clean["laplace"]))
    assert all(c.shape == (40, 2, 2) and np.array_equal(np.diagonal(c, axis1=1, axis2=2), v) for c, v in zip(clean["cov"], clean["v"]))
    st = JC.statement(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"], held=np.concatenate(held))
    assert max(_rel(c, s["cov"]) for c, s in zip(clean["cov"], st)) <= PUBLIC_TOL


def test_the_default_path_is_the_sequence_of_engine_calls_it_has_been(V):
    """leave_entries_out(predictive=True) without the new keyword: one masked replica set, one E-step, vlgp_predictive
    with the set's own mu, v.  Passes with and without the feature."""
    from vlgp_amd import evaluation as EV

    trials, params, config = _public()
    base = EV.leave_entries_out(trials, params, config, n_folds=3, seed=1, predictive=True)
    F = EV.entry_folds(120, 8, 3, 1)
    held = np.stack([F == k for k in range(3)])
    with EV._resident(trials, params, EV._zero_start(trials, 2), 0) as eng:
        eng.replicate(EV.SET_TEST, EV.SET_REPLICAS, held_out=held)
        eng.estep(EV.SET_REPLICAS, config["max_iter"], config["dmu_bound"], True)
        sums, rate, _ = eng.predictive(EV.SET_REPLICAS, n_nodes=12, vb=True, want_rate=True)
    assert base["ll_per_fold"].tobytes() == np.ascontiguousarray(sums[:, :, 0]).tobytes()
    assert np.concatenate(base["rate"]).tobytes() == rate.tobytes()


def test_posterior_mean_field_is_the_default(V):
    from vlgp_amd import evaluation as EV

    trials, params, config = _public()
    base = EV.leave_entries_out(trials, params, config, n_folds=3, seed=1, predictive=True)
    cal = EV.calibration(trials, params, config, how="entries", n_folds=3, seed=1)
    for call, ref, kw in ((EV.leave_entries_out, base, {"n_folds": 3, "seed": 1, "predictive": True}),
                          (EV.calibration, cal, {"how": "entries", "n_folds": 3, "seed": 1})):
        same = call(trials, params, config, posterior="mean_field", **kw)
        assert sorted(same) == sorted(ref)
        for key in ref:
            one, two = ref[key], same[key]
            if isinstance(one, list):
                assert all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(one, two)), key
            else:
                assert np.asarray(one).tobytes() == np.asarray(two).tobytes(), key
    with pytest.raises(ValueError, match="posterior='joint' needs predictive=True"):
        EV.leave_entries_out(trials, params, config, posterior="joint")
