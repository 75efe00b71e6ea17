"""Fit with missing observations, host side: what ``fit(..., missing=)`` refuses, that ``missing=None`` is today's call
path, the restatement (tests/masked_fit_numpy.py) against the oracle where they must agree, the recovery of held-out
rates by the restated fit, ``cross_validate`` cutting ``missing`` with the training trials, and the header / documents."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RELAXED = ("vlgp_update_w", "vlgp_update_v", "vlgp_norms", "vlgp_norms_begin", "vlgp_norms_end", "vlgp_apply_latent_map",
           "vlgp_latent_moments", "vlgp_hstep_prepare", "vlgp_hstep_begin", "vlgp_hstep_objective", "vlgp_hstep_end",
           "vlgp_mstep", "vlgp_mstep_begin", "vlgp_mstep_end")


def small(M=3, T=40, N=6, L=2, seed=5):
    from vlgp_amd import synth

    trials = synth.make_trials(M, T, N, L, seed=seed)
    return trials, [np.random.default_rng(seed).random((T, N)) < 0.2 for _ in trials]


@pytest.mark.parametrize("kwargs, text", [
    (dict(lik=["poisson"] * 5 + ["gaussian"]), "Gaussian"),
    (dict(lik="gaussian"), "Gaussian"),
    (dict(history=1), "history"),
    (dict(constrain_loading="svd"), "svd"),
    (dict(track_elbo=True), "track_elbo"),
    (dict(window=30), "multiples of window"),
])
def test_fit_with_missing_refuses(kwargs, text):
    import vlgp_amd

    trials, missing = small()
    kwargs.setdefault("window", 20)
    with pytest.raises(ValueError, match=text):
        vlgp_amd.fit(trials, 2, missing=missing, verbose=False, **kwargs)


def test_fit_with_missing_refuses_several_ranks():
    import vlgp_amd

    class Comm:
        world = 2

    trials, missing = small()
    with pytest.raises(ValueError, match="one rank"):
        vlgp_amd.fit(trials, 2, missing=missing, verbose=False, window=20, comm=Comm())


@pytest.mark.parametrize("how", ["short list", "shape", "dtype"])
def test_fit_with_missing_checks_the_mask(how):
    import vlgp_amd

    trials, missing = small()
    if how == "short list":
        missing = missing[:-1]
    elif how == "shape":
        missing[1] = missing[1][:-1]
    else:
        missing[1] = missing[1].astype(float)
    with pytest.raises(ValueError, match="missing"):
        vlgp_amd.fit(trials, 2, missing=missing, verbose=False, window=20)


def test_fit_with_missing_refuses_a_channel_never_observed():
    import vlgp_amd

    trials, missing = small()
    y_before = [tr["y"].copy() for tr in trials]
    for m in missing:
        m[:, 3] = True
    with pytest.raises(ValueError, match=r"\[3\].*no observed entry"):
        vlgp_amd.fit(trials, 2, missing=missing, verbose=False, window=20)
    assert all(np.array_equal(tr["y"], y0) for tr, y0 in zip(trials, y_before))


def test_missing_none_is_todays_call_path(monkeypatch):
    """No mask: FitSession runs no masked-only step -- neither the masked argument check nor the mask normalisation, and
    no ``Engine.replicate``, without which a session cannot make a masked set -- and reaches the engine."""
    from vlgp_amd import api, util

    class Reached(Exception):
        pass

    def plain_engine(params, device=0):
        raise Reached()

    def masked_only(*args, **kwargs):
        raise AssertionError("missing=None took a masked-only step")

    monkeypatch.setattr(api.E.Engine, "for_params", staticmethod(plain_engine))
    monkeypatch.setattr(api, "_masked_inputs", masked_only)
    monkeypatch.setattr(util, "_per_trial_entries", masked_only)
    monkeypatch.setattr(api, "_per_trial_entries", masked_only)
    monkeypatch.setattr(api.E.Engine, "replicate", masked_only)
    trials, _ = small()
    with pytest.raises(Reached):
        api.fit(trials, 2, verbose=False)
    with pytest.raises(Reached):
        api.fit(trials, 2, verbose=False, missing=None)
    assert api.FitSession.finish is not None and "missing" not in trials[0]
    assert all("missing" not in tr for tr in trials)


def test_segment_dicts_are_trial_major_views_of_the_trials_and_of_the_y_given():
    """The function the device cut (``_segments``) and the masked fit's host cut share: views of the trial arrays, y
    sliced from the y handed in, trial-major order, every dmu a view of one block."""
    from vlgp_amd.api import _segment_dicts

    window, N, L = 40, 4, 2
    rng = np.random.default_rng(3)
    trials = [{"y": rng.poisson(1.0, (T, N)).astype(float), "x": np.ones((T, 1, N)), "mu": rng.standard_normal((T, L)),
               "w": rng.random((T, L)), "v": rng.random((T, L))} for T in (40, 80, 40)]
    ys = [tr["y"] + 100.0 for tr in trials]  # another y than the trials' own
    segs = _segment_dicts(trials, ys, [range(0, tr["y"].shape[0], window) for tr in trials], window)
    assert len(segs) == 4 and all(list(sg) == ["y", "x", "mu", "w", "v", "dmu"] for sg in segs)
    owner, start = [0, 1, 1, 2], [0, 0, 40, 0]
    for sg, i, s0 in zip(segs, owner, start):
        for k in ("x", "mu", "w", "v"):
            assert sg[k].shape[0] == window and np.shares_memory(sg[k], trials[i][k])
            assert np.array_equal(sg[k], trials[i][k][s0:s0 + window])
        assert np.shares_memory(sg["y"], ys[i]) and not np.shares_memory(sg["y"], trials[i]["y"])
        for j in set(range(3)) - {i}:
            assert not np.shares_memory(sg["mu"], trials[j]["mu"])
    segs[2]["mu"][...] = 7.0  # a view: writes go through to rows 40 ... 79 of the second trial
    assert np.all(trials[1]["mu"][40:] == 7.0) and not np.any(trials[1]["mu"][:40] == 7.0)
    assert np.array_equal(np.concatenate([sg["y"] for sg in segs]), np.concatenate(ys))
    assert np.array_equal(np.concatenate([sg["mu"] for sg in segs]), np.concatenate([tr["mu"] for tr in trials]))
    block = segs[0]["dmu"].base
    assert block.shape == (4, window, L) and not block.any()
    assert all(sg["dmu"].base is block and np.shares_memory(sg["dmu"], block[i]) and sg["dmu"].shape == (window, L)
               for i, sg in enumerate(segs))
    segs[3]["dmu"][...] = 1.0
    assert block[3].all() and not block[:3].any()


@pytest.mark.parametrize("what", ["loglik", "elbo"])
def test_scores_of_every_entry_refuse_a_fit_with_missing(what):
    from vlgp_amd import evaluation

    trials, missing = small()
    for tr, m in zip(trials, missing):
        tr["missing"] = m
    with pytest.raises(ValueError, match="missing"):
        getattr(evaluation, what)({"trials": trials, "params": {"zdim": 2}, "config": {}})


def problem(seed=7, M=2, T=40, N=5, L=2, P=1):
    from vlgp_amd import synth

    trials = synth.make_trials(M, T, N, L, seed=seed)
    rng = np.random.default_rng(seed)
    y = np.concatenate([tr["y"] for tr in trials])
    x = np.ones((y.shape[0], P, N))
    if P > 1:
        x[:, 1:] = 0.3 * rng.standard_normal((y.shape[0], P - 1, N))
    mu = 0.3 * rng.standard_normal((y.shape[0], L))
    v = 0.05 + 0.05 * rng.random((y.shape[0], L))
    a = 0.3 * rng.standard_normal((L, N))
    b = np.zeros((P, N))
    b[0] = np.log(np.maximum(y.mean(0), 1e-2))
    return y, x, mu, v, a, b, rng


def test_restated_mstep_without_a_hole_is_the_oracles():
    import masked_fit_numpy as MF
    from oracle import vlgp_oracle as O

    y, x, mu, v, a, b, _ = problem(P=2)
    want = O.mstep_arrays(y, x, mu, v, a, b, np.zeros(y.shape[1], dtype=bool), 3)
    got = MF.mstep_masked(y, x, mu, v, a, b, np.zeros(y.shape, dtype=bool), 3)
    for g, w in zip(got, want):
        assert np.abs(g - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0)


def test_restated_mstep_reads_observed_rows_only_and_keeps_an_empty_channel():
    import masked_fit_numpy as MF

    y, x, mu, v, a, b, rng = problem()
    missing = rng.random(y.shape) < 0.3
    missing[:, 2] = True
    noise = 0.5 + rng.random(y.shape[1])
    want = MF.mstep_masked(y, x, mu, v, a, b, missing, 2, noise=noise)
    got = MF.mstep_masked(np.where(missing, np.nan, y), x, mu, v, a, b, missing, 2, noise=noise)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    a1, b1, da, db, n1 = got
    assert np.array_equal(a1[:, 2], a[:, 2]) and np.array_equal(b1[:, 2], b[:, 2]) and n1[2] == noise[2]
    assert not da[:, 2].any() and not db[:, 2].any() and np.abs(da[:, 0]).max() > 0


def test_restated_estep_from_zero_is_the_speckled_one():
    import heldout_numpy as H
    import masked_fit_numpy as MF
    import speckled_numpy as S
    from oracle import vlgp_oracle as O

    trials, params, config = H.problem(seed=11, M=1, T=60, N=8, L=2)
    tr = trials[0]
    gauss = np.zeros(8, dtype=bool)
    G = O.build_prior([60], params["omega"], params["sigma"], 50)[60]
    obs = np.random.default_rng(2).random(tr["y"].shape) >= 0.25
    want = S.estep_masked(tr["y"], tr["x"], params["a"], params["b"], params["noise"], gauss, G, obs, 3)
    z = np.zeros((60, 2))
    got = MF.estep_masked_warm(np.where(obs, tr["y"], np.nan), tr["x"], z, z, z, params["a"], params["b"], params["noise"],
                               gauss, G, obs, 3)
    for g, w in zip(got[:4], want[:4]):
        assert np.abs(g - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0)
    # a warm start continues: 2 + 1 sweeps are 3 sweeps
    mid = MF.estep_masked_warm(tr["y"], tr["x"], z, z, z, params["a"], params["b"], params["noise"], gauss, G, obs, 2)
    end = MF.estep_masked_warm(tr["y"], tr["x"], mid[0], mid[1], mid[2], params["a"], params["b"], params["noise"], gauss,
                               G, obs, 1)
    for g, w in zip(end[:3], want[:3]):
        assert np.abs(g - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0)


def recovery_problem(seed=1, M=4, window=25, N=12, L=2):
    """Four trials of 2 x 25 bins, 12 channels, 2 latents, 20 % of the entries missing; the initialisation is
    preprocess.initialize on copies of y filled with the channel's observed mean, as FitSession does it."""
    import masked_fit_numpy as MF
    from vlgp_amd import get_config, synth
    from vlgp_amd.preprocess import get_params, initialize

    trials = synth.make_trials(M, 2 * window, N, L, seed=seed)
    missing = MF.random_missing(trials, 0.2, seed)
    n_obs = sum((~m).sum(0) for m in missing)
    y_mean = sum(np.where(m, 0.0, t["y"]).sum(0) for t, m in zip(trials, missing)) / n_obs
    work = [{"y": np.where(m, y_mean[None], t["y"])} for t, m in zip(trials, missing)]
    config = get_config(max_iter=5, window=window)
    params = get_params(work, L, omega_bound=config["omega_bound"])
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        initialize(work, params, config)
    finally:
        np.random.set_state(state)
    params.pop("transform", None)
    for k in ("a", "b", "noise", "omega", "sigma"):
        params[k] = np.array(params[k], dtype=float)
    for t, w, m in zip(trials, work, missing):
        t["x"] = np.ones((t["y"].shape[0], 1, N))
        t["mu"] = w["mu"]
        t["y"] = np.where(m, np.nan, t["y"])  # the restated fit never reads a missing entry
    return trials, missing, params, config


def test_restated_masked_fit_predicts_the_missing_entries():
    """Five EM iterations of the restated masked fit; the fitted rate at the missing entries must beat the per-channel
    constant-rate null by at least 0.01 bits per spike (a condition on the method, not a tuned tolerance).
    Measured on the CPU this was written on: 0.370 bits per spike (seed 1; seeds 0, 2, 3: 0.433, 0.459, 0.681)."""
    import masked_fit_numpy as MF

    trials, missing, params, config = recovery_problem()
    truth = __import__("vlgp_amd").synth.make_trials(4, 50, 12, 2, seed=1)
    MF.fit_given_init(trials, missing, params, config)
    for tr, full in zip(trials, truth):
        assert np.all(np.isfinite(tr["mu"])) and np.all(np.isfinite(tr["v"]))
        tr["y"] = full["y"]  # the held-out truth, for the score alone
    bps = MF.heldout_bits_per_spike(trials, missing, params)
    print("restated masked fit: %.3f bits per spike at the missing entries" % bps)
    assert bps >= 0.01


@pytest.mark.parametrize("constrain_latent", [False, "both"])
def test_whole_fit_problem_is_one_where_the_restatement_is_continuous(constrain_latent):
    """The condition the whole-fit comparison of tests/test_gpu_masked_fit.py rests on, on the restatement alone: omega
    moved by 1e-10 (relative, opposite signs per latent) after each of the first two H-steps -- a hundred times what the
    device's H-step differs from the oracle's by -- moves a, omega, mu by less than a tenth of the trajectory tolerance 1e-6.
    (Measured: 2e-10, 5e-11, 7e-11.  Not so at every seed: at seed 5 a change of 1e-12 flips a pivot of the prior's
    incomplete Cholesky factor and moves omega by 4.0e-6.)"""
    import masked_fit_numpy as MF
    from conftest import relerr
    from oracle import vlgp_oracle as O
    from test_gpu_masked_fit import fit_problem

    def run(rel):
        base, missing, a0, b0 = fit_problem()
        N, L = a0.shape[1], a0.shape[0]
        ref = [{"y": tr["y"].copy(), "x": np.ones((tr["y"].shape[0], 1, N)), "mu": tr["mu"].copy()} for tr in base]
        params = O.make_params(ref, L, a=a0.copy(), b=b0.copy())
        calls, plain = [0], O.hstep

        def moved(trials, p, c):
            plain(trials, p, c)
            calls[0] += 1
            if rel and calls[0] <= 2:
                p["omega"] = p["omega"] * (1 + rel * np.array([1.0, -1.0]))
                O.make_cholesky(trials, p, c)

        O.hstep = moved
        try:
            MF.fit_given_init(ref, missing, params, O.make_config(max_iter=3, min_iter=3, window=40,
                                                                  constrain_latent=constrain_latent))
        finally:
            O.hstep = plain
        return params, np.concatenate([tr["mu"] for tr in ref])

    (p0, mu0), (p1, mu1) = run(0.0), run(1e-10)
    moves = {"omega": relerr(p1["omega"], p0["omega"]), "a": relerr(p1["a"], p0["a"]), "mu": relerr(mu1, mu0)}
    print("whole-fit problem, omega moved by 1e-10: " + "  ".join("%s %.1e" % kv for kv in moves.items()))
    assert max(moves.values()) < 1e-7, moves


def test_cross_validate_cuts_missing_with_the_training_trials(monkeypatch):
    from vlgp_amd import model_selection as MS

    trials, missing = small(M=6)
    for i, m in enumerate(missing):
        m[0, 0] = bool(i % 2)
    seen = []

    def fake_fit(train, n_factors, missing=None, **kwargs):
        assert missing is not None and len(missing) == len(train)
        for tr, m in zip(train, missing):
            src = [i for i, t in enumerate(trials) if np.array_equal(t["y"], tr["y"])]
            assert len(src) == 1 and m is MS_missing[src[0]]
        seen.append(len(train))
        return {"params": {}, "config": {}}

    def fake_score(test, params, config, **kwargs):
        return {"co_bps": 0.0, "bits_per_spike": np.zeros(trials[0]["y"].shape[1]), "n_failed": 0}

    MS_missing = missing
    monkeypatch.setattr(MS, "fit", fake_fit)
    monkeypatch.setattr(MS, "leave_group_out", fake_score)
    out = MS.cross_validate(trials, [2], n_trial_folds=3, n_channel_folds=2, missing=missing)
    assert out["errors"] == [] and seen == [4, 4, 4]


def test_header_and_documents_name_the_masked_fit_set():
    header = open(os.path.join(ROOT, "include", "vlgp_hip.h")).read()
    assert "#define VLGP_ABI_VERSION 3" in header
    assert "masked fit set" in header
    block = header[header.index("masked fit set"):]
    para = re.search(r"masked fit set.*?\*/", header, flags=re.S).group(0)
    for name in RELAXED:
        assert name in para, name
    for name in ("vlgp_elbo", "vlgp_forecast", "vlgp_project_units"):
        assert name in para, name
    assert block
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "missing=" in readme and "The fit itself takes no mask" not in readme
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Fit with missing observations" in integration
    for topic in ("Gaussian", "history", "overlapping", "rank", "ELBO", "forecast"):
        assert re.search(topic, integration[integration.index("Fit with missing observations"):], flags=re.I), topic
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "K_MASKED" in design
