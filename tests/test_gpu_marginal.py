"""The importance weights of the marginal likelihood on the device (vlgp_marginal, vlgp_amd.evaluation.marginal_loglik,
cross_validate(score="marginal_bps")) against the NumPy statement of their definition (tests/marginal_numpy.py).

Tolerance.  STAGE = 1e-9 is the project's stage-wise tolerance.  A log_w is a sum of T N
log-likelihood terms and 3 L addends of c that may cancel, so its error is taken relative to the sum of the absolute
values of those terms (marginal_numpy.statement returns it), as test_gpu_elbo.py takes its row sums.  The measured errors
are printed by every case and recorded in profiles/marginal/measured_errors.txt.
"""
import numpy as np
import pytest

import forecast_numpy as FN
import marginal_numpy as MN
from heldout_numpy import lagged
from oracle import vlgp_oracle as O
from test_marginal_host import exact_gaussian_problem

pytestmark = pytest.mark.gpu

STAGE = 1e-9
SET = 0
R = 50


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _problem(lengths, N, L, omega, seed, n_gauss=0, history=0, vb=True, clamp_channel=None, rank=R):
    """Units with a given posterior (mu, v, w random and positive where they must be), parameters and the oracle's prior
    factors of `omega` with `rank` columns, injected from the host.  clamp_channel: a channel whose linear predictor lies
    above the clamp."""
    from vlgp_amd import synth

    rng = np.random.default_rng(seed)
    trials = synth.make_trials(len(lengths), max(lengths), N, min(L, 3), seed=seed, n_gauss=n_gauss, lengths=lengths)
    P = 1 + history
    gauss = np.zeros(N, bool)
    if n_gauss:
        gauss[N - n_gauss:] = True
    a = 0.3 * rng.standard_normal((L, N)) * (5.0 / L if L > 10 else 1.0)
    y = np.concatenate([t["y"] for t in trials])
    b = np.zeros((P, N))
    b[0] = np.where(gauss, y.mean(0), np.log(np.maximum(y.mean(0), 1e-3)))
    if clamp_channel is not None:
        b[0, clamp_channel] = 14.0
    if history:
        b[1:] = -0.05 * rng.random((history, N))
    noise = np.where(gauss, 0.5 + rng.random(N), 1.0)
    omega = np.asarray(omega, dtype=float)
    prior = O.build_prior(sorted(set(lengths)), omega, np.ones(L), rank)
    units = []
    for t in trials:
        T = t["y"].shape[0]
        units.append({"y": t["y"], "x": lagged(t["y"], history) if history else None,
                      "mu": 0.3 * rng.standard_normal((T, L)),
                      "v": 0.05 * rng.random((T, L)) if vb else np.zeros((T, L)), "w": rng.uniform(0.05, 2.0, (T, L))})
    params = {"ydim": N, "zdim": L, "xdim": P, "a": a, "b": b, "noise": noise, "omega": omega, "sigma": np.ones(L),
              "rank": rank, "likelihood": np.where(gauss, "gaussian", "poisson"), "cholesky": prior}
    return units, params, gauss


def _engine(V, units, params, gauss, rank=None):
    """An engine of `rank` columns (default: the problem's own, params["rank"]) holding the units, parameters and factors."""
    eng = V.Engine(params["ydim"], params["zdim"], params["xdim"], params["rank"] if rank is None else rank, gauss)
    eng.set_params(params["a"], params["b"], params["noise"])
    eng.upload(SET, units)
    for T, G in params["cholesky"].items():
        eng.set_prior(T, G)
    return eng


def _device(V, units, params, gauss, eps, vb=True):
    with _engine(V, units, params, gauss) as eng:
        return eng.marginal(SET, eps, vb=vb, want_parts=True)


def _eps(units, L, K, seed=1, rank=R):
    return np.random.default_rng(seed).standard_normal((len(units), L, rank, K))


def _compare(name, dev, st):
    """Errors of the device arrays against the statement relative to the sum of absolute terms, printed, then asserted."""
    log_w, bad, parts = dev
    want, want_parts, scale = st
    assert bad == 0 and log_w.shape == want.shape and np.all(np.isfinite(log_w))
    err = {"log_w": float(np.max(np.abs(log_w - want) / scale)),
           "ll": float(np.max(np.abs(parts[:, :, 0] - want_parts[:, :, 0]) / scale)),
           "sum_c": float(np.max(np.abs(parts[:, :, 1] - want_parts[:, :, 1]) / scale))}
    print("marginal errors [%s] units %d K %d: %s" % (name, log_w.shape[0], log_w.shape[1],
                                                      ", ".join("%s %.2e" % kv for kv in err.items())))
    assert np.array_equal(parts[:, :, 0] + parts[:, :, 1], log_w)  # (the stated order: ll + sum_l c)
    for key, val in err.items():
        assert val <= STAGE, (name, key, val)


RANK_OMEGA = [1e-4, 1e-3, 5e-3, 2e-2, 1e-1, 5e-1]  # (test_gpu_elbo's "ranks_around_14_and_32")
CASES = {
    # name: lengths, N, L, omega, n_gauss, history, vb, clamp_channel, K
    "ragged_mixed": ([1, 50, 64, 65, 130], 14, 3, [2e-2, 5e-3, 1e-3], 4, 0, True, None, 5),
    "one_latent": ([50, 70, 50], 14, 1, [5e-3], 0, 0, True, None, 5),
    "twelve_latents": ([50] * 3, 14, 12, np.linspace(2e-2, 1e-3, 12), 0, 0, True, None, 5),
    "one_channel": ([50, 70], 1, 2, [2e-2, 1e-3], 0, 0, True, None, 5),
    "regressors_xdim3": ([50, 80], 10, 3, [2e-2, 5e-3, 1e-3], 2, 2, True, None, 5),
    "ranks_around_8_multiples": ([64] * 3, 12, 6, RANK_OMEGA, 0, 0, True, None, 5),
    "long_rank50": ([1000, 1000, 1000], 10, 2, [1e-3, 2e-3], 0, 0, True, None, 3),
    "above_the_clamp": ([50, 65], 8, 2, [2e-2, 1e-3], 0, 0, True, 3, 5),
    "map": ([50, 80, 50], 14, 3, [2e-2, 5e-3, 1e-3], 3, 0, False, None, 5),
    "rank_64_61_and_1": ([70, 130], 10, 3, [0.5, 1.5, 3.0], 2, 0, True, None, 5),
}
# Engines of 64 columns: the rough omega of the case fills all 64, and every column from the listed rank on is zeroed (as
# tests/joint_shapes.py cuts its factors): marginal_task with every lane live, a rank that is no multiple of 8, and rank 1.
CUT_RANKS = {"rank_64_61_and_1": [64, 61, 1]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_weights_equal_the_numpy_statement(V, name):
    lengths, N, L, omega, n_gauss, history, vb, clamp, K = CASES[name]
    rank = 64 if name in CUT_RANKS else R
    units, params, gauss = _problem(lengths, N, L, omega, seed=11, n_gauss=n_gauss, history=history, vb=vb,
                                    clamp_channel=clamp, rank=rank)
    for l, r in enumerate(CUT_RANKS.get(name, ())):
        for G in params["cholesky"].values():
            assert np.all(np.any(G[l] != 0.0, axis=0))  # (all 64 columns filled before the cut)
            G[l][:, r:] = 0.0
    ranks = np.array([[FN.rank(params["cholesky"][T][l]) for l in range(L)] for T in sorted(set(lengths))])
    if name.startswith("ranks"):
        r = ranks[0]
        assert r.min() < 8 and np.any((r > 8) & (r < 16)) and np.any((r > 16) & (r < 32)) and r.max() > 32, r
    if name.startswith("long"):
        assert ranks.max() == 50
    if clamp is not None:
        assert np.all(units[0]["mu"] @ params["a"][:, clamp] + params["b"][0, clamp] > 10.0)
    eps = _eps(units, L, K, rank=rank)
    st = MN.statement(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"], eps, vb=vb)
    with _engine(V, units, params, gauss) as eng:
        dev = eng.marginal(SET, eps, vb=vb, want_parts=True)
        dev_ranks = eng.unit_ranks(SET)
    if name in CUT_RANKS:
        assert np.array_equal(ranks, [CUT_RANKS[name]] * 2) and np.array_equal(dev_ranks, [CUT_RANKS[name]] * len(units))
    _compare(name, dev, st)


@pytest.fixture(scope="module")
def small(V):
    """Two short units, N = 8, L = 2, K = 130 draws: the device's answer and the statement's, shared by the tests
    below and left unchanged."""
    units, params, gauss = _problem([50, 30], 8, 2, [2e-2, 1e-3], seed=4)
    eps = _eps(units, 2, 130, seed=2)
    st = MN.statement(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"], eps)
    with _engine(V, units, params, gauss) as eng:
        by_K = {K: eng.marginal(SET, np.ascontiguousarray(eps[..., :K]), want_parts=True) for K in (1, 63, 64, 65, 130)}
        again = eng.marginal(SET, eps, want_parts=True)
        single = {k: eng.marginal(SET, np.ascontiguousarray(eps[..., k:k + 1]))[0] for k in (0, 63, 64, 129)}
        ranks = eng.unit_ranks(SET)
        hollow = eps.copy()
        for u in range(len(units)):
            for l in range(2):
                hollow[u, l, ranks[u, l]:] = np.nan
        hollow_out = eng.marginal(SET, hollow, want_parts=True)
    return {"units": units, "params": params, "gauss": gauss, "eps": eps, "st": st, "by_K": by_K, "again": again,
            "single": single, "ranks": ranks, "hollow": hollow_out}


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
def test_sample_counts_around_the_chunk_of_64(small, K):
    st = tuple(x[:, :K] for x in small["st"])
    _compare("K=%d" % K, small["by_K"][K], st)


def test_two_calls_give_the_same_bits(small):
    one, two = small["by_K"][130], small["again"]
    assert one[0].tobytes() == two[0].tobytes() and one[2].tobytes() == two[2].tobytes() and one[1] == two[1] == 0


def test_a_sample_does_not_depend_on_the_samples_beside_it(small):
    """Sample k of the K = 130 call is the K = 1 call on that sample's normals, bit for bit; and the first samples of a
    longer call are those of a shorter one."""
    full = small["by_K"][130][0]
    for k, alone in small["single"].items():
        assert alone.shape == (2, 1) and alone[:, 0].tobytes() == np.ascontiguousarray(full[:, k]).tobytes(), k
    for K in (1, 63, 64, 65):
        assert np.array_equal(small["by_K"][K][0], full[:, :K]), K


def test_eps_rows_beyond_the_rank_are_never_read(small):
    assert small["ranks"].max() < R
    got, want = small["hollow"], small["by_K"][130]
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[2]))
    assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()


def test_exact_posterior_on_the_device(V):
    """The exactness case of test_marginal_host.py: every weight equals the dense closed form, so the spread of log_w
    over k and its distance to the closed form are both rounding -- within STAGE of the sum of absolute terms."""
    units, a, b, noise, gauss, prior, closed = exact_gaussian_problem()
    params = {"ydim": 6, "zdim": 3, "xdim": 1, "rank": R, "a": a, "b": b, "noise": noise, "cholesky": prior}
    eps = _eps(units, 3, 70, seed=1)
    scale = MN.statement(units, a, b, noise, gauss, prior, eps)[2]
    log_w, bad, _ = _device(V, units, params, gauss, eps)
    spread = float(np.max(np.ptp(log_w, axis=1) / scale.min(axis=1)))
    dist = float(np.max(np.abs(log_w - closed[:, None]) / scale))
    print("marginal errors [exact_gaussian] spread over k %.2e, distance to the closed form %.2e" % (spread, dist))
    assert bad == 0 and spread <= STAGE and dist <= STAGE


def test_singular_pair_is_counted_and_nan_not_a_fault(V, small):
    """A negative w makes I + G'WG indefinite for one (unit, latent): that unit's log_w is NaN and the pair is counted;
    the other unit keeps its bits; the set's state is the same bits before and after."""
    units = [dict(u) for u in small["units"]]
    units[1]["w"] = units[1]["w"].copy()
    units[1]["w"][:, 1] = -50.0
    with _engine(V, units, small["params"], small["gauss"]) as eng:
        before = eng.download(SET)
        log_w, bad, parts = eng.marginal(SET, small["eps"], want_parts=True)
        after = eng.download(SET)
    assert bad == 1
    assert np.all(np.isnan(log_w[1])) and np.all(np.isnan(parts[1, :, 1]))
    assert log_w[0].tobytes() == small["by_K"][130][0][0].tobytes()
    for key in before:
        assert before[key].tobytes() == after[key].tobytes(), key


def test_admission_is_that_of_vlgp_elbo(V, small):
    """A replicated set and a masked set of one replica are refused by name with status -3; a tiling cut is taken."""
    units, params, gauss = _problem([50, 50], 8, 2, [2e-2, 1e-3], seed=4)
    refusal = "status -3.*vlgp_marginal refuses a replicated set"
    with _engine(V, units, params, gauss) as eng:
        eps = _eps(units, 2, 3)
        plain = eng.marginal(SET, eps)[0]
        eng.replicate(SET, 2, channels=[1, 3])
        with pytest.raises(V.engine.VlgpError, match=refusal):
            eng.marginal(2, _eps(units * 2, 2, 3))
        eng.free_units(2)
        held = np.zeros((1, 100, 8), dtype=bool)
        held[0, ::7, 2] = True
        eng.replicate(SET, 2, held_out=held)
        with pytest.raises(V.engine.VlgpError, match=refusal):
            eng.marginal(2, eps)
        eng.free_units(2)
        eng.cut(SET, 1, np.array([0, 50]), 50)
        cut = eng.marginal(1, eps)[0]
        with pytest.raises(V.engine.VlgpError, match="status -1.*n_samples"):
            eng.check(eng.lib.vlgp_marginal(eng.h, SET, 1, 0, None, None, None, None))
        with pytest.raises(V.engine.VlgpError, match="status -1.*eps"):
            eng.check(eng.lib.vlgp_marginal(eng.h, SET, 1, 3, None, None, None, None))
    assert np.all(np.isfinite(plain)) and cut.tobytes() == plain.tobytes()


# ---- the public path ----------------------------------------------------------------------------------------------
def _poisson_problem():
    """M = 4, T = 60, N = 12, L = 2, Poisson, rates far below the clamp (the problem of test_marginal_host.py, without
    its CPU convergence: the device infers)."""
    M, T, N, L = 4, 60, 12, 2
    rng = np.random.default_rng(0)
    omega = np.array([5e-3, 2e-2])
    t = np.arange(T)
    a = 0.5 * rng.standard_normal((L, N))
    b = np.log(0.5) + 0.3 * rng.standard_normal((1, N))
    trials = []
    for _ in range(M):
        lat = np.stack([np.linalg.cholesky(np.exp(-om * (t[:, None] - t[None, :]) ** 2) + 1e-8 * np.eye(T))
                        @ rng.standard_normal(T) for om in omega], axis=1)
        trials.append({"y": rng.poisson(np.exp(lat @ a + b)).astype(float)})
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": a, "b": b, "noise": np.ones(N), "omega": omega, "sigma": np.ones(L),
              "rank": R, "likelihood": np.array(["poisson"] * N), "cholesky": O.build_prior([T], omega, np.ones(L), R)}
    config = {"method": "VB", "max_iter": 30, "dmu_bound": 5.0}
    return trials, params, config


SEED_PUBLIC = 0


def test_marginal_loglik_infers_or_takes_the_stored_posterior(V):
    """infer=True and infer=False after an identical inference agree bit for bit; total >= elbo - 5 s.e. for the committed
    seed (Jensen: E iwae >= elbo, the s.e. from the spread of log_w); the caller's dicts are untouched."""
    from vlgp_amd import evaluation as EV

    trials, params, config = _poisson_problem()
    keep_y = [t["y"].copy() for t in trials]
    keep_p = {k: np.array(v, copy=True) for k, v in params.items() if isinstance(v, np.ndarray)}
    cold = EV.marginal_loglik(trials, params, config, n_samples=130, seed=SEED_PUBLIC)
    assert all(set(t) == {"y"} and np.array_equal(t["y"], y0) for t, y0 in zip(trials, keep_y))
    assert all(np.array_equal(params[k], v) for k, v in keep_p.items()) and set(params["cholesky"]) == {60}
    assert set(cold) == {"log_w", "iwae", "elbo_mc", "ess", "total", "elbo", "gap", "marginal_bps", "n_failed"}
    # the identical inference, by hand: the posterior marginal_loglik inferred, stored in the dicts
    with V.Engine.for_params(params) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(SET, EV._zero_start(trials, 2))
        eng.set_prior(60, params["cholesky"][60])
        assert eng.estep(SET, config["max_iter"], config["dmu_bound"], True) == 0
        state = eng.download(SET, ("mu", "v", "w"))
    fitted = [dict(t, **{k: state[k][60 * i:60 * (i + 1)] for k in state}) for i, t in enumerate(trials)]
    warm = EV.marginal_loglik(fitted, params, config, n_samples=130, seed=SEED_PUBLIC, infer=False)
    for key in cold:
        assert np.asarray(cold[key]).tobytes() == np.asarray(warm[key]).tobytes(), key
    assert cold["log_w"].shape == (4, 130) and cold["n_failed"] == 0
    se = math_sqrt_sum_var(cold["log_w"])
    print("marginal_loglik: total %.4f elbo %.4f gap %.4f (s.e. %.4f) bps %.4f ess %s" % (
        cold["total"], cold["elbo"], cold["gap"], se, cold["marginal_bps"], np.round(cold["ess"], 1)))
    assert cold["total"] >= cold["elbo"] - 5.0 * se
    assert cold["gap"] == cold["total"] - cold["elbo"] and np.isfinite(cold["marginal_bps"])
    assert np.all(cold["ess"] >= 1.0) and np.all(cold["ess"] <= 130.0) and np.all(cold["iwae"] >= cold["elbo_mc"])
    first = EV.marginal_loglik(trials, params, config, n_samples=70, seed=SEED_PUBLIC)
    assert first["log_w"].shape == (4, 70)  # (the normals come in chunks of 64: a whole leading chunk does not move)
    assert np.array_equal(first["log_w"][:, :64], cold["log_w"][:, :64])


def math_sqrt_sum_var(log_w):
    """Standard error of sum_u mean_k log_w[u, k]."""
    return float(np.sqrt(np.sum(np.var(log_w, axis=1) / log_w.shape[1])))


def test_cross_validate_scores_by_marginal_bps(V):
    from vlgp_amd import synth
    from vlgp_amd.model_selection import cross_validate

    trials = synth.make_trials(6, 100, 12, 2, seed=3)
    runs = [cross_validate(trials, [1, 2], score="marginal_bps", n_trial_folds=2, max_iter=3, min_iter=3) for _ in range(2)]
    one, two = runs
    assert set(one) == {"n_factors", "trial_folds", "score", "marginal_bps", "mean_marginal_bps", "ess_min", "n_failed",
                        "best", "errors"}
    assert one["errors"] == [] and one["score"] == "marginal_bps" and one["best"] in (1, 2)
    assert one["marginal_bps"].shape == (2, 2) and one["ess_min"].shape == (2, 2)
    assert np.all(np.isfinite(one["marginal_bps"])) and np.all(np.isfinite(one["mean_marginal_bps"]))
    assert np.all(one["ess_min"] >= 1.0) and np.all(one["ess_min"] <= 80.0)
    print("cross_validate marginal_bps %s ess_min %s" % (one["marginal_bps"].tolist(), one["ess_min"].tolist()))
    for key in ("marginal_bps", "mean_marginal_bps", "ess_min", "n_failed"):
        assert np.asarray(one[key]).tobytes() == np.asarray(two[key]).tobytes(), key
