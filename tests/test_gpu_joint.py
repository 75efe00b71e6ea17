"""The joint Laplace posterior on the device (vlgp_joint_laplace, Engine.joint_laplace, evaluation.joint_posterior,
marginal_loglik(proposal="joint"), cross_validate(proposal="joint")) against the NumPy statement of its definition
(tests/joint_numpy.py) and against closed forms.

Tolerance.  Sums (laplace, log_w and its parts) are compared relative to the sum of the absolute values of their terms,
as DESIGN.md section 2 takes its stage-wise tolerance; beta, mu and v, which are entries and not sums, relative to
max(1, largest absolute entry of the unit).  The mode is unique, so the two sides differ by where their iterations
stopped and by rounding alone: the agreement cases run both the device and the statement to a decrement <= 1e-20, which
bounds their distance in the norm of H by 2e-10, and in practice, Newton's last step squaring the decrement, far below it.
TOL is about 100 times the largest error measured over every case of this file (profiles/joint/measured_errors.txt; every
case prints its own).

Stationarity.  |grad f| <= 1e-6 is asserted on the beta of that same call.  At the default tol = 1e-10 it does NOT follow:
the decrement g' H^-1 g bounds |g| by sqrt(tol lambda_max(H)) alone, and lambda_max(H) is 1 ... 140 here; measured at
tol = 1e-10: up to 3.9e-5 (N = 70), 9.3e-6 (L = 3, N = 5), 9.1e-6 (D = 200).  The default call is therefore held to the
bound that does follow, |g| <= sqrt(tol lambda_max(H)), with lambda_max from NumPy.
"""
import numpy as np
import pytest

import joint_numpy as JN
from oracle import vlgp_oracle as O
from test_gpu_marginal import R, SET, _engine, _eps, _problem
from test_joint_host import shared_gaussian_problem

pytestmark = pytest.mark.gpu

TOL = 5e-13  # (largest measured: 4.4e-15, v of the L = 1 cases)
NEWTON_TOL = 1e-20


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))


def _errors(name, dev, st, units):
    """Errors of the device's dict against the statement's per-unit dicts, printed; returns them."""
    err = {"beta": 0.0, "mu": 0.0, "v": 0.0, "laplace": 0.0, "ll": 0.0, "logdet": 0.0}
    row = 0
    for i, s in enumerate(st):
        T = units[i]["y"].shape[0]
        err["beta"] = max(err["beta"], _rel(JN.stack_beta(dev["beta"][i], s["ranks"]), s["beta"]))
        err["mu"] = max(err["mu"], _rel(dev["mu"][row:row + T], s["mu"]))
        err["v"] = max(err["v"], _rel(dev["v"][row:row + T], s["v"]))
        err["laplace"] = max(err["laplace"], abs(dev["laplace"][i] - s["laplace"]) / s["scale"])
        err["ll"] = max(err["ll"], abs(dev["ll"][i] - s["ll"]) / s["scale"])
        err["logdet"] = max(err["logdet"], abs(dev["logdet"][i] - s["logdet"]) / s["scale"])
        for l, r in enumerate(s["ranks"]):
            assert not np.any(dev["beta"][i, l, r:]), "beta beyond the rank must be zero"
        assert dev["D"][i] == sum(s["ranks"])
        row += T
    print("joint errors [%s] units %d D %s newton %s: %s" % (name, len(st), dev["D"].tolist(), dev["n_newton"].tolist(),
                                                              ", ".join("%s %.2e" % kv for kv in err.items())))
    return err


def _grad_norms(dev, st):
    """|grad f| recomputed in NumPy from the device's own beta, per unit."""
    return np.array([np.linalg.norm(s["unit"].grad(JN.stack_beta(dev["beta"][i], s["ranks"]))) for i, s in enumerate(st)])


RAGGED = [1, 7, 64, 65, 130]
CASES = {
    # name: lengths, N, L, omega, n_gauss, history
    "L1_one_channel": (RAGGED, 1, 1, [2e-2], 0, 0),
    "L1_five_channels": (RAGGED, 5, 1, [5e-1], 0, 0),
    "L3_five_channels": (RAGGED, 5, 3, [2e-2, 5e-3, 1e-3], 0, 0),
    "L3_seventy_mixed_regressors": (RAGGED, 70, 3, [5e-1, 5e-3, 1e-3], 20, 1),
    "L4_T200_D200": ([200, 7], 5, 4, [1.0, 0.8, 0.6, 0.5], 0, 0),
    "L5_T200_D250": ([200, 7], 5, 5, [1.0, 0.8, 0.6, 0.5, 0.4], 0, 0),  # the factor's panel needs more than 64 KB of LDS
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_mode_equals_the_numpy_statement(V, name):
    lengths, N, L, omega, n_gauss, history = CASES[name]
    units, params, gauss = _problem(lengths, N, L, omega, seed=11, n_gauss=n_gauss, history=history)
    st = JN.statement(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"])
    D = [sum(s["ranks"]) for s in st]
    if name.startswith("L3"):
        assert min(D) < 8 and any(64 < d <= 141 for d in D), D
    if name.startswith("L4"):
        assert D[0] == 200
    if name.startswith("L5"):
        assert D[0] == 250
    with _engine(V, units, params, gauss) as eng:
        dev = eng.joint_laplace(SET, max_iter=50, tol=NEWTON_TOL)
        loose = eng.joint_laplace(SET, max_iter=50, tol=1e-10)
    assert dev["n_failed"] == 0 and np.all(dev["converged"]) and np.all(dev["decrement"] <= NEWTON_TOL)
    err = _errors(name, dev, st, units)
    for key, val in err.items():
        assert val <= TOL, (name, key, val)
    # independently of the statement: stationarity, from the returned beta alone
    gn = _grad_norms(dev, st)
    assert np.all(gn <= 1e-6), gn
    assert loose["n_failed"] == 0 and np.all(loose["converged"]) and np.all(loose["n_newton"] <= 50)
    gl = _grad_norms(loose, st)
    top = np.array([np.linalg.eigvalsh(s["H"])[-1] for s in st])
    print("joint |grad f| [%s]: tol 1e-20 %s; tol 1e-10 %s against sqrt(tol lambda_max) %s"
          % (name, np.array2string(gn, precision=2), np.array2string(gl, precision=2),
             np.array2string(np.sqrt(1e-10 * top), precision=2)))
    assert np.all(loose["decrement"] <= 1e-10) and np.all(gl <= 1.01 * np.sqrt(1e-10 * top))


@pytest.fixture(scope="module")
def exact(V):
    """The all-Gaussian shared-loading problem on the device: 130 joint draws, and vlgp_marginal's on the same normals."""
    units, a, b, noise, gauss, prior, closed = shared_gaussian_problem()
    params = {"ydim": 6, "zdim": 3, "xdim": 1, "rank": R, "a": a, "b": b, "noise": noise, "cholesky": prior}
    eps = _eps(units, 3, 130, seed=1)
    with _engine(V, units, params, gauss) as eng:
        dev = eng.joint_laplace(SET, eps=eps)
        mean_field = eng.marginal(SET, eps)[0]
    st = JN.statement(units, a, b, noise, gauss, prior, eps)
    return dev, mean_field, st, closed


def test_gaussian_shared_loadings_every_weight_is_the_closed_form(exact):
    dev, mean_field, st, closed = exact
    scale = np.array([s["scale_k"].min() for s in st])
    spread = float(np.max(np.ptp(dev["log_w"], axis=1) / scale))
    dist = float(np.max(np.abs(dev["log_w"] - closed[:, None]) / scale[:, None]))
    lap = float(np.max(np.abs(dev["laplace"] - closed) / scale))
    mf_spread = float(np.min(np.ptp(mean_field, axis=1)))
    print("joint errors [exact_gaussian] spread over k %.2e, log_w to the closed form %.2e, laplace to it %.2e; "
          "vlgp_marginal's spread %.3f nats" % (spread, dist, lap, mf_spread))
    assert dev["n_failed"] == 0 and np.all(dev["converged"])
    assert spread <= TOL and dist <= TOL and lap <= TOL
    assert mf_spread > 1e-3  # the mean-field proposal is NOT the posterior here: the two proposals differ


@pytest.fixture(scope="module")
def small(V):
    """Two short units, N = 8, L = 2, 130 draws; the statement evaluated at the device's own beta."""
    units, params, gauss = _problem([50, 30], 8, 2, [2e-2, 1e-3], seed=4)
    eps = _eps(units, 2, 130, seed=2)
    with _engine(V, units, params, gauss) as eng:
        before = eng.download(SET)
        pars = eng.get_params()
        full = eng.joint_laplace(SET, eps=eps)
        again = eng.joint_laplace(SET, eps=eps)
        single = {k: eng.joint_laplace(SET, eps=np.ascontiguousarray(eps[..., k:k + 1])) for k in (0, 63, 64, 129)}
        mode_only = eng.joint_laplace(SET)
        raw = np.empty((2, 8))
        eng.check(eng.lib.vlgp_joint_laplace(eng.h, SET, 50, 1e-10, 0, None, None, raw.ctypes.data_as(V._lib._dp), None, None,
                                             None, None, None))
        after = eng.download(SET)
        pars_after = eng.get_params()
    ranks = [JN.rank(params["cholesky"][T][l]) for T in (50, 30) for l in range(2)]
    beta = [JN.stack_beta(full["beta"][i], ranks[2 * i:2 * i + 2]) for i in range(2)]
    st = JN.statement(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"], eps, beta=beta)
    return {"full": full, "again": again, "single": single, "mode_only": mode_only, "raw": raw, "st": st,
            "state": (before, after), "pars": (pars, pars_after), "units": units, "params": params, "gauss": gauss, "eps": eps}


def test_draws_equal_the_statement_at_the_devices_own_mode(small):
    full, st = small["full"], small["st"]
    err = {"log_w": 0.0, "ll": 0.0, "c": 0.0}
    for i, s in enumerate(st):
        err["log_w"] = max(err["log_w"], float(np.max(np.abs(full["log_w"][i] - s["log_w"]) / s["scale_k"])))
        err["ll"] = max(err["ll"], float(np.max(np.abs(full["parts"][i, :, 0] - s["ll_k"]) / s["scale_k"])))
        err["c"] = max(err["c"], float(np.max(np.abs(full["parts"][i, :, 1] - s["c_k"]) / s["scale_k"])))
    print("joint errors [draws] K 130: %s" % ", ".join("%s %.2e" % kv for kv in err.items()))
    assert np.array_equal(full["parts"][:, :, 0] + full["parts"][:, :, 1], full["log_w"])
    for key, val in err.items():
        assert val <= TOL, (key, val)


def test_a_sample_does_not_depend_on_the_samples_beside_it_and_runs_repeat(small):
    full, again = small["full"], small["again"]
    for key in ("beta", "stats", "mu", "v", "log_w", "parts"):
        assert full[key].tobytes() == again[key].tobytes(), key
    for k, alone in small["single"].items():
        assert alone["log_w"].shape == (2, 1)
        assert alone["log_w"][:, 0].tobytes() == np.ascontiguousarray(full["log_w"][:, k]).tobytes(), k
        assert alone["parts"][:, 0].tobytes() == np.ascontiguousarray(full["parts"][:, k]).tobytes(), k
    assert small["mode_only"]["stats"].tobytes() == full["stats"].tobytes() == small["raw"].tobytes()
    assert "log_w" not in small["mode_only"]


def test_the_call_changes_no_state(small):
    before, after = small["state"]
    for key in before:
        assert before[key].tobytes() == after[key].tobytes(), key
    for one, two in zip(*small["pars"]):
        assert np.asarray(one).tobytes() == np.asarray(two).tobytes()


def test_one_factorisation_far_from_the_mode_is_not_a_failure(V):
    units, params, gauss = _problem([50, 30], 8, 2, [2e-2, 1e-3], seed=4)
    rng = np.random.default_rng(0)
    for u in units:
        u["mu"] = 3.0 * rng.standard_normal(u["mu"].shape)
    with _engine(V, units, params, gauss) as eng:
        dev = eng.joint_laplace(SET, max_iter=1, eps=_eps(units, 2, 3))
    assert dev["n_failed"] == 0 and not np.any(dev["converged"]) and np.all(dev["n_newton"] == 1)
    assert np.all(dev["decrement"] > 1e-10)
    for key in ("beta", "stats", "mu", "v", "log_w", "parts"):
        assert np.all(np.isfinite(dev[key])), key


def test_a_channel_above_the_clamp_gives_finite_outputs(V):
    units, params, gauss = _problem([50, 65], 8, 2, [2e-2, 1e-3], seed=4)
    params["b"][0, 3] = 12.0
    with _engine(V, units, params, gauss) as eng:
        dev = eng.joint_laplace(SET, eps=_eps(units, 2, 3))
    assert dev["n_failed"] == 0
    for key in ("beta", "stats", "mu", "v", "log_w", "parts"):
        assert np.all(np.isfinite(dev[key])), key


def test_a_nan_in_w_fails_its_unit_alone(V, small):
    units = [dict(u) for u in small["units"]]
    units[1]["w"] = units[1]["w"].copy()
    units[1]["w"][3, 0] = np.nan
    with _engine(V, units, small["params"], small["gauss"]) as eng:
        dev = eng.joint_laplace(SET, eps=small["eps"])
    full = small["full"]
    assert dev["n_failed"] == 1
    assert np.all(np.isnan(dev["stats"][1, :5])) and np.all(np.isnan(dev["log_w"][1]))
    assert np.all(np.isnan(dev["mu"][50:])) and np.all(np.isnan(dev["v"][50:]))
    assert dev["stats"][0].tobytes() == full["stats"][0].tobytes()
    assert dev["log_w"][0].tobytes() == full["log_w"][0].tobytes()
    assert dev["mu"][:50].tobytes() == full["mu"][:50].tobytes() and dev["v"][:50].tobytes() == full["v"][:50].tobytes()


def test_refusals_by_status_and_text(V):
    units, params, gauss = _problem([50, 50], 8, 2, [2e-2, 1e-3], seed=4)
    refusal = "status -3.*vlgp_joint_laplace refuses a replicated set"
    dp = V._lib._dp
    with _engine(V, units, params, gauss) as eng:
        stats = np.empty((2, 8))
        eng.replicate(SET, 2, channels=[1, 3])
        with pytest.raises(V.engine.VlgpError, match=refusal):
            eng.joint_laplace(2)
        eng.free_units(2)
        held = np.zeros((1, 100, 8), dtype=bool)
        held[0, ::7, 2] = True
        eng.replicate(SET, 2, held_out=held)
        with pytest.raises(V.engine.VlgpError, match=refusal):
            eng.joint_laplace(2)
        eng.free_units(2)
        with pytest.raises(V.engine.VlgpError, match="status -1.*tol"):
            eng.joint_laplace(SET, tol=0.0)
        with pytest.raises(V.engine.VlgpError, match="status -1.*max_iter"):
            eng.joint_laplace(SET, max_iter=0)
        with pytest.raises(V.engine.VlgpError, match="status -1.*stats"):
            eng.check(eng.lib.vlgp_joint_laplace(eng.h, SET, 50, 1e-10, 0, None, None, None, None, None, None, None, None))
        with pytest.raises(V.engine.VlgpError, match="status -1.*eps"):
            eng.check(eng.lib.vlgp_joint_laplace(eng.h, SET, 50, 1e-10, 3, None, None, stats.ctypes.data_as(dp), None, None,
                                                 None, None, None))
    L = 11
    omega = np.linspace(1.0, 0.5, L)
    prior = O.build_prior([200], omega, np.ones(L), R)
    rng = np.random.default_rng(0)
    unit = {"y": rng.poisson(1.0, (200, 3)).astype(float), "x": None, "mu": np.zeros((200, L)), "v": np.zeros((200, L)),
            "w": np.ones((200, L))}
    wide = {"ydim": 3, "zdim": L, "xdim": 1, "rank": R, "a": 0.1 * rng.standard_normal((L, 3)), "b": np.zeros((1, 3)),
            "noise": np.ones(3), "cholesky": prior}
    with _engine(V, [unit], wide, np.zeros(3, bool)) as eng:
        with pytest.raises(V.engine.VlgpError, match="status -3.*D = 550"):
            eng.joint_laplace(SET)


# ---- the public path ----------------------------------------------------------------------------------------------
def _poisson_trials():
    """6 trials x 60 bins x 12 Poisson channels, L = 3, loadings shared by every latent."""
    M, T, N, L = 6, 60, 12, 3
    rng = np.random.default_rng(0)
    omega = np.array([2e-2, 5e-3, 1e-3])
    a = 0.5 * rng.standard_normal((L, N))
    b = -np.ones((1, N))
    prior = O.build_prior([T], omega, np.ones(L), R)
    trials = []
    for _ in range(M):
        lat = np.stack([prior[T][l] @ rng.standard_normal(R) for l in range(L)], axis=1)
        trials.append({"y": rng.poisson(np.exp(lat @ a + b)).astype(float)})
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": a, "b": b, "noise": np.ones(N), "omega": omega, "sigma": np.ones(L),
              "rank": R, "likelihood": np.array(["poisson"] * N), "cholesky": prior}
    config = {"method": "VB", "max_iter": 30, "dmu_bound": 5.0}
    return trials, params, config


def test_joint_posterior_and_the_joint_proposal_of_marginal_loglik(V):
    from vlgp_amd import evaluation as EV

    trials, params, config = _poisson_trials()
    post = EV.joint_posterior(trials, params, config)
    assert set(post) == {"mu", "v", "laplace", "converged", "n_newton", "total", "laplace_bps", "n_failed"}
    assert len(post["mu"]) == 6 and all(m.shape == (60, 3) and v.shape == (60, 3) for m, v in zip(post["mu"], post["v"]))
    assert post["laplace"].shape == (6,) and np.all(post["converged"]) and post["n_failed"] == 0
    assert np.isfinite(post["total"]) and np.isfinite(post["laplace_bps"]) and all(np.all(v > 0) for v in post["v"])
    joint = EV.marginal_loglik(trials, params, config, n_samples=130, seed=0, proposal="joint")
    mean_field = EV.marginal_loglik(trials, params, config, n_samples=130, seed=0)
    assert set(joint) == set(mean_field) | {"laplace", "converged"}
    assert set(mean_field) == {"log_w", "iwae", "elbo_mc", "ess", "total", "elbo", "gap", "marginal_bps", "n_failed"}
    assert joint["laplace"].tobytes() == post["laplace"].tobytes()
    print("ESS of 130: joint %s, posterior %s" % (np.round(joint["ess"], 1), np.round(mean_field["ess"], 1)))
    assert joint["ess"].min() > mean_field["ess"].min()
    # the statement on the same normals: iwae - laplace is a property of the mode and the draws, not of the device
    units = [{"y": t["y"], "x": None, "mu": np.zeros((60, 3)), "v": np.zeros((60, 3)), "w": np.ones((60, 3))} for t in trials]
    rng = np.random.default_rng(0)
    eps = np.concatenate([rng.standard_normal((6, 3, R, kc)) for kc in (64, 64, 2)], axis=3)
    st = JN.statement(units, params["a"], params["b"], params["noise"], np.zeros(12, bool), params["cholesky"], eps)
    want = np.array([EV.weights_summary(s["log_w"])[0] - s["laplace"] for s in st])
    se = np.sqrt((130.0 / joint["ess"] - 1.0) / 130.0)  # of log mean_k w, by the delta method
    print("iwae - laplace: device %s, statement %s, s.e. %s" % (joint["iwae"] - joint["laplace"], want, se))
    assert np.all(np.abs(joint["iwae"] - (joint["laplace"] + want)) <= 5.0 * se)


def test_cross_validate_with_the_joint_proposal_repeats(V):
    from vlgp_amd import synth
    from vlgp_amd.model_selection import cross_validate

    trials = synth.make_trials(6, 100, 12, 2, seed=3)
    one, two = [cross_validate(trials, [1, 2], score="marginal_bps", proposal="joint", n_trial_folds=2, max_iter=3,
                               min_iter=3) for _ in range(2)]
    assert one["errors"] == [] and one["score"] == "marginal_bps"
    assert np.all(np.isfinite(one["marginal_bps"])) and np.all(one["ess_min"] >= 1.0)
    print("cross_validate joint marginal_bps %s ess_min %s" % (one["marginal_bps"].tolist(), one["ess_min"].tolist()))
    for key in ("marginal_bps", "mean_marginal_bps", "ess_min", "n_failed"):
        assert np.asarray(one[key]).tobytes() == np.asarray(two[key]).tobytes(), key
