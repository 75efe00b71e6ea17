"""The pair moments on the device (vlgp_pair_moments, vlgp_pair_moments_cov, Engine.pair_moments) and
evaluation.residual_correlation against the NumPy statement (tests/pair_numpy.py).

Shapes: N in {1, 2, 63, 64, 65, 130} -- one channel tile, its edges, and three tiles with a partial one and tile pairs off
the diagonal --, L in {1, 3, 5, 10, 16}, and row counts around the 32 rows a workgroup takes of a small set
(tests/test_pair_host.py holds the layout to that): 1, 31, 32, 33, and three ragged units spanning four chunks.  Poisson
and Gaussian channels alternate, so every kind of pair occurs inside a tile and across tiles.

Tolerance.  err = max |device - statement| / max(1, largest |statement| entry) per matrix.  Both sides add products of
doubles over at most a few hundred rows and differ in the order of the sums and in the last bits of exp and expm1; the
largest error measured on one MI355X over every case of this file is 3.22e-15 (the point posterior of three ragged units,
N = 2, L = 16; profiles/pair_moments/measured_errors.txt has every line), and TOL is a hundred times that, far below the
project's stage tolerance of 1e-9.  Every case prints its error."""
import copy
import functools

import numpy as np
import pytest

import heldout_numpy as H
import pair_numpy as PN
from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu

TOL = 3.3e-13  # 100 x the largest measured error, 3.22e-15 (module docstring)
CHUNK = 32   # rows a workgroup takes of a small set (PAIR_MIN_CHUNK, csrc/call_block.h)
SET, REP, R = 0, 2, 10


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _err(got, want):
    return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))


@functools.lru_cache(maxsize=None)
def _problem(lengths, N, L, P, seed=0):
    """Units with a random posterior, parameters, alternating likelihoods, and per-row covariances of four kinds."""
    rng = np.random.default_rng(seed + 1000 * N + 10 * L + sum(lengths))
    gauss = (np.arange(N) % 2 == 1)
    a = 0.3 * rng.standard_normal((L, N)) * (5.0 / L if L > 10 else 1.0)
    b = np.concatenate([np.where(gauss, 0.5, 0.3)[None] + 0.2 * rng.standard_normal((1, N)),
                        -0.05 * rng.random((P - 1, N))])
    noise = np.where(gauss, 0.5 + rng.random(N), 1.0)
    units = []
    for T in lengths:
        x = None if P == 1 else np.concatenate([np.ones((T, 1, N)), rng.poisson(0.5, (T, P - 1, N)).astype(float)], axis=1)
        mu = 0.4 * rng.standard_normal((T, L))
        eta = mu @ a + (b[0] if x is None else np.einsum("tpn,pn->tn", x, b))
        y = np.where(gauss, eta + rng.standard_normal((T, N)), rng.poisson(np.exp(eta)).astype(float))
        units.append({"y": y, "x": x, "mu": mu, "v": 0.02 + 0.2 * rng.random((T, L)), "w": rng.uniform(0.05, 2.0, (T, L))})
    rows = sum(lengths)
    B = 0.3 * rng.standard_normal((rows, L, L))
    u = 0.4 * rng.standard_normal((rows, L))
    covs = {"full": B @ B.transpose(0, 2, 1) + 0.01 * np.eye(L), "rank_one": u[:, :, None] * u[:, None, :],
            "zero": np.zeros((rows, L, L)), "diagonal": PN.diag_cov(np.concatenate([un["v"] for un in units]))}
    return units, dict(a=a, b=b, noise=noise, gauss=gauss), covs, 0.4 * rng.standard_normal((rows, L))


def _cat(units, key):
    if key == "x" and units[0]["x"] is None:
        return None
    return np.concatenate([u[key] for u in units])


def _engine(V, units, par):
    L, N = par["a"].shape
    eng = V.Engine(N, L, par["b"].shape[0], R, par["gauss"])
    eng.set_params(par["a"], par["b"], par["noise"])
    eng.upload(SET, units)
    return eng


def _state(eng, sets=(SET,)):
    """Everything a read-only call must leave alone, as bytes."""
    return [x.tobytes() for x in eng.get_params()] + [v.tobytes() for s in sets for v in eng.download(s).values()]


def _statement(units, par, mu, cov, live=None):
    return PN.pair_moments(_cat(units, "y"), _cat(units, "x"), mu, cov, par["a"], par["b"], par["noise"], par["gauss"], live)


def _same_bits(one, two):
    return all(u.tobytes() == w.tobytes() for u, w in zip(one, two))


def _symmetric(pair):
    return all(np.array_equal(m, np.swapaxes(m, -1, -2)) for m in pair)


PLAIN = [((33,), N, 3, 1) for N in (1, 2, 63, 64, 65, 130)] + [((31,), 65, L, 1) for L in (1, 5, 10, 16)] + \
        [((1,), 65, 3, 2), ((32,), 64, 5, 2), ((40, 50, 33), 130, 5, 2), ((40, 50, 33), 2, 16, 1)]


@pytest.mark.parametrize("lengths, N, L, P", PLAIN)
def test_plain_set_under_every_posterior(V, lengths, N, L, P):
    units, par, covs, mu2 = _problem(lengths, N, L, P)
    mu, v = _cat(units, "mu"), _cat(units, "v")
    rows = sum(lengths)
    errs = {}
    with _engine(V, units, par) as eng:
        before = _state(eng)
        own = {vb: eng.pair_moments(SET, vb=vb) for vb in (True, False)}
        assert _same_bits(own[True], eng.pair_moments(SET, vb=True))
        given = {kind: eng.pair_moments(SET, mu=mu2, cov=cov) for kind, cov in covs.items()}
        assert _same_bits(given["full"], eng.pair_moments(SET, mu=mu2, cov=eng_pack(V, covs["full"], L)))
        own_as_cov = eng.pair_moments(SET, mu=mu, cov=covs["diagonal"])
        assert _state(eng) == before
    for vb in (True, False):
        want = _statement(units, par, mu, PN.diag_cov(v if vb else 0.0 * v))
        assert want[2].min() == want[2].max() == rows
        errs["own vb %d" % vb] = max(_err(g, w) for g, w in zip(own[vb], want))
        assert _symmetric(own[vb]) and own[vb][0].shape == (N, N)
    off = ~np.eye(N, dtype=bool)
    assert np.all(own[False][1][off] == 0.0)  # (a point posterior: no covariance between channels, exactly)
    for kind, cov in covs.items():
        want = _statement(units, par, mu2, cov)
        errs[kind] = max(_err(g, w) for g, w in zip(given[kind], want))
        assert _symmetric(given[kind])
    assert np.all(given["zero"][1][off] == 0.0)
    errs["diagonal cov against own v"] = max(_err(g, w) for g, w in zip(own_as_cov, own[True]))
    print("measured pair errors [plain rows %s N %d L %d P %d]: %s" % (list(lengths), N, L, P,
                                                                        ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, errs


def eng_pack(V, cov, L):
    """The packed form of a (rows, L, L) covariance: both forms are taken and give the same bits."""
    return V.engine.pack_cov(cov, len(cov), L)


def _masks(kind, n_rep, rows, N, seed=5):
    held = np.zeros((n_rep, rows, N), dtype=bool)
    if kind == "folds":  # channel folds, constant along the rows: replica k holds the channels n % n_rep == k
        for k in range(n_rep):
            held[k][:, k::n_rep] = True
    elif kind == "speckled":  # ... with one replica that holds nothing out
        held = np.random.default_rng(seed).random((n_rep, rows, N)) < 0.4
        held[n_rep - 1] = False
    return held


MASKED = [("folds", 2, (40, 50, 33), 65, 3, 1), ("speckled", 3, (40, 50, 33), 130, 5, 2), ("speckled", 2, (33,), 64, 10, 1),
          ("folds", 3, (31,), 130, 1, 1)]


@pytest.mark.parametrize("kind, n_rep, lengths, N, L, P", MASKED)
def test_masked_set_scores_the_pairs_each_replica_holds_out(V, kind, n_rep, lengths, N, L, P):
    """Own mu, v after an E-step (so that the replicas' posteriors differ), and supplied mu, cov that differ per replica:
    replica k reads its own rows of the posterior, the source's rows of y and x, and its own mask."""
    units, par, covs, mu2 = _problem(lengths, N, L, P)
    rows = sum(lengths)
    held = _masks(kind, n_rep, rows, N)
    mu_rep =np.concatenate([mu2 + 0.1 * k for k in range(n_rep)])
    cov_rep = np.concatenate([covs["full"] * (1.0 + 0.5 * k) for k in range(n_rep)])
    prior = O.build_prior(sorted(set(lengths)), np.linspace(2e-2, 1e-3, L), np.ones(L), R)
    with _engine(V, units, par) as eng:
        for T, G in prior.items():
            eng.set_prior(T, G)
        eng.replicate(SET, REP, held_out=held)
        eng.estep(REP, 2, 5.0, True)
        before = _state(eng, (SET, REP))
        post = eng.download(REP, ("mu", "v"))
        own = eng.pair_moments(REP, vb=True)
        given = eng.pair_moments(REP, mu=mu_rep, cov=cov_rep)
        assert _same_bits(own, eng.pair_moments(REP, vb=True)) and _same_bits(given, eng.pair_moments(REP, mu=mu_rep, cov=cov_rep))
        assert _state(eng, (SET, REP)) == before
    assert own[0].shape == given[1].shape == (n_rep, N, N) and _symmetric(own) and _symmetric(given)
    assert np.abs(post["mu"][:rows] - post["mu"][rows:2 * rows]).max() > 1e-3
    errs = []
    for k in range(n_rep):
        sl = slice(k * rows, (k + 1) * rows)
        want_own = _statement(units, par, post["mu"][sl], PN.diag_cov(post["v"][sl]), held[k])
        want_given = _statement(units, par, mu_rep[sl], cov_rep[sl], held[k])
        errs += [_err(own[i][k], want_own[i]) for i in (0, 1)] + [_err(given[i][k], want_given[i]) for i in (0, 1)]
        if not held[k].any():
            assert not own[0][k].any() and not own[1][k].any() and not given[0][k].any() and not given[1][k].any()
    print("measured pair errors [masked %s x %d rows %s N %d L %d P %d]: %.2e" % (kind, n_rep, list(lengths), N, L, P, max(errs)))
    assert max(errs) <= TOL


def test_what_y_holds_at_an_entry_that_is_not_live_is_never_read(V):
    """NaN in y wherever no replica holds the entry out: the same bits as with the finite y, own v and supplied cov."""
    lengths, N, L = (40, 33), 130, 3
    units, par, covs, mu2 = _problem(lengths, N, L, 1)
    rows = sum(lengths)
    held = _masks("speckled", 3, rows, N, seed=6)
    seen = held.any(axis=0)
    dirty, at = copy.deepcopy(units), 0
    for u in dirty:
        T = u["y"].shape[0]
        u["y"] = np.where(seen[at:at + T], u["y"], np.nan)
        at += T
    mu_rep, cov_rep = np.tile(mu2, (3, 1)), np.tile(covs["full"], (3, 1, 1))
    got = []
    for us in (units, dirty):
        with _engine(V, us, par) as eng:
            eng.replicate(SET, REP, held_out=held)
            got.append(eng.pair_moments(REP, vb=True) + eng.pair_moments(REP, mu=mu_rep, cov=cov_rep))
    assert np.isnan(_cat(dirty, "y")).sum() > 1000 and all(np.all(np.isfinite(g)) for g in got[1])
    assert _same_bits(got[0], got[1])


@pytest.mark.parametrize("masked", [False, True])
def test_dead_rows_of_a_supplied_posterior_drop_out(V, masked):
    """NaN in every row of one trial's mu (a failed joint posterior) and in one entry of another row's cov: the statement
    on the arrays with those rows removed."""
    lengths, N, L = (40, 50, 33), 65, 3
    units, par, covs, mu2 = _problem(lengths, N, L, 2)
    rows = sum(lengths)
    n_rep = 2 if masked else 1
    held = _masks("speckled", 3, rows, N)[:2] if masked else np.ones((1, rows, N), dtype=bool)
    mu, cov = np.tile(mu2, (n_rep, 1)), np.tile(covs["full"], (n_rep, 1, 1))
    mu[40:90, 1] = np.nan  # (the second trial, in the first replica)
    cov[(n_rep - 1) * rows + 100, 2, 0] = cov[(n_rep - 1) * rows + 100, 0, 2] = np.inf
    with _engine(V, units, par) as eng:
        sid = SET
        if masked:
            eng.replicate(SET, REP, held_out=held)
            sid = REP
        got = eng.pair_moments(sid, mu=mu, cov=cov)
    got = [g.reshape(n_rep, N, N) for g in got]
    errs = []
    y, x = _cat(units, "y"), _cat(units, "x")
    for k in range(n_rep):
        keep = ~PN.dead_rows(mu[k * rows:(k + 1) * rows], cov[k * rows:(k + 1) * rows])
        assert 0 < (~keep).sum() <= 51
        want = PN.pair_moments(y[keep], x[keep], mu[k * rows:(k + 1) * rows][keep], cov[k * rows:(k + 1) * rows][keep], par["a"],
                               par["b"], par["noise"], par["gauss"], held[k][keep])
        errs += [_err(got[i][k], want[i]) for i in (0, 1)]
        assert all(np.all(np.isfinite(g[k])) for g in got)
    print("measured pair errors [dead rows, masked %d]: %.2e" % (masked, max(errs)))
    assert max(errs) <= TOL


def test_refusals_leave_everything_as_it_was(V):
    """A copied cut and group replicas are refused with their reasons, null outputs and a null mu or cov before anything is
    written; parameters and the contents of every set are the same bytes afterwards."""
    from vlgp_amd._lib import dptr

    units, par, covs, mu2 = _problem((40, 40), 8, 3, 1)
    N, L = 8, 3
    with _engine(V, units, par) as eng:
        eng.cut(SET, 1, np.array([0, 40, 15, 55]), 25)
        eng.set_overlaps(1, [0, 2, 4], [[0, 2, 10], [1, 3, 10]], [0, 0, 2])
        eng.replicate(SET, REP, groups=[[1, 3], [5]])
        before = _state(eng, (SET, 1, REP))
        mu_c, cov_c = np.zeros((100, L)), np.zeros((100, L, L))
        for kw in ({}, {"mu": mu_c, "cov": cov_c}):
            name = "vlgp_pair_moments_cov" if kw else "vlgp_pair_moments"
            with pytest.raises(V.VlgpError, match="status -3.*%s on a copied cut: merge it and score the source set" % name):
                eng.pair_moments(1, **kw)
        mu_g, cov_g = np.zeros((160, L)), np.zeros((160, L, L))
        for kw in ({}, {"mu": mu_g, "cov": cov_g}):
            with pytest.raises(V.VlgpError, match="status -3.*replicate with held_out=: a pair needs both channels in one replica"):
                eng.pair_moments(REP, **kw)
        out = np.full((N, N), 7.0)
        mu, cov = mu2, V.engine.pack_cov(covs["full"], 80, L)
        eng.free_units(REP)
        eng.free_units(1)
        lib, h = eng.lib, eng.h
        assert lib.vlgp_pair_moments(h, SET, 1, None, dptr(out)) == -1 and b"needs resid and model" in lib.vlgp_last_error(h)
        assert lib.vlgp_pair_moments(h, SET, 1, dptr(out), None) == -1
        assert lib.vlgp_pair_moments_cov(h, SET, dptr(mu), dptr(cov), dptr(out), None) == -1
        assert lib.vlgp_pair_moments_cov(h, SET, None, dptr(cov), dptr(out), dptr(out)) == -1 and b"needs mu" in lib.vlgp_last_error(h)
        assert lib.vlgp_pair_moments_cov(h, SET, dptr(mu), None, dptr(out), dptr(out)) == -1 and b"needs cov" in lib.vlgp_last_error(h)
        assert np.all(out == 7.0)
        with pytest.raises(ValueError, match="go together"):
            eng.pair_moments(SET, mu=mu2)
        assert _state(eng, (SET,)) == before[:5 + 4]
        tiling = eng.pair_moments(SET)
        eng.cut(SET, 1, np.array([0, 40]), 40)
        assert _same_bits(tiling, eng.pair_moments(1))  # (a tiling cut is the source's rows)


# ---- evaluation.residual_correlation end to end ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _public():
    """Three trials of 40 bins, N = 8, L = 2; four E-step iterations from a zero start give the posterior they carry."""
    from vlgp_amd import evaluation as EV

    trials, params, config = H.problem(seed=3, M=3, T=40, N=8, L=2, max_iter=4)
    params["cholesky"] = O.build_prior([40], params["omega"], params["sigma"], params["rank"])
    with EV._resident(trials, params, EV._zero_start(trials, 2), 0) as eng:
        assert eng.estep(EV.SET_TEST, 4, config["dmu_bound"], True) == 0
        post = eng.download(EV.SET_TEST, ("mu", "v", "w"))
    for i, tr in enumerate(trials):
        for key in post:
            tr[key] = post[key][40 * i:40 * (i + 1)].copy()
    return trials, params, config


def _par(params):
    return dict(a=params["a"], b=params["b"], noise=params["noise"], gauss=np.asarray(params["likelihood"]) == "gaussian")


def _same_summary(got, want):
    err = 0.0
    for key, w in want.items():
        g, w = np.asarray(got[key], dtype=float), np.asarray(w, dtype=float)
        assert np.array_equal(np.isnan(g), np.isnan(w)), key
        if np.isfinite(w).any():
            err = max(err, float(np.nanmax(np.abs(g - w)) / max(1.0, float(np.nanmax(np.abs(w))))))
    return err


@pytest.mark.parametrize("posterior", ["mean_field", "joint"])
def test_residual_correlation_in_sample(V, posterior):
    from vlgp_amd import evaluation as EV

    trials, params, config = copy.deepcopy(_public())
    got = EV.residual_correlation(trials, params, config, posterior=posterior)
    if posterior == "joint":
        with EV._posterior(trials, params, config, False, None, 0) as (eng, _):
            post = eng.joint_posterior(EV.SET_TEST)
        mu, cov = post["mu"], post["cov"]
        assert got["converged"].shape == (3,) and np.all(got["converged"])
    else:
        mu, cov = _cat(trials, "mu"), PN.diag_cov(_cat(trials, "v"))
    want = PN.summary(*_statement(trials, _par(params), mu, cov))
    err = _same_summary(got, want)
    print("measured pair errors [residual_correlation in_sample %s]: %.2e; rms_excess %.4f over %d pairs"
          % (posterior, err, got["rms_excess"], got["n_pairs"]))
    assert err <= TOL and got["n_failed"] == 0 and got["n_pairs"] == 28
    assert np.all(got["count"] == 120)  # (a plain set: every row in every pair)


@pytest.mark.parametrize("posterior", ["mean_field", "joint"])
def test_residual_correlation_of_channel_folds(V, posterior):
    """The folds held out one replica each, the latents inferred without them, the pairs inside a fold scored under the
    posterior the engine inferred (the same calls, made here); a pair across folds or outside them is never scored."""
    from vlgp_amd import evaluation as EV

    trials, params, config = copy.deepcopy(_public())
    groups = [[0, 5, 6], [2, 3], [7]]
    got = EV.residual_correlation(trials, params, config, how="channels", groups=groups, posterior=posterior)
    masks = np.stack(list(EV._group_masks(groups, 120, 8)))
    total = np.zeros((3, 8, 8))
    with EV._resident(trials, params, EV._zero_start(trials, 2), 0) as eng:
        # (the joint posterior takes one replica at a time, the mean-field E-step all folds as the replicas of one set)
        for k0, k1 in ((0, 1), (1, 2), (2, 3)) if posterior == "joint" else ((0, 3),):
            eng.replicate(EV.SET_TEST, EV.SET_REPLICAS, held_out=masks[k0:k1])
            assert eng.estep(EV.SET_REPLICAS, config["max_iter"], config["dmu_bound"], True) == 0
            if posterior == "joint":
                post = eng.joint_posterior(EV.SET_REPLICAS)
                mu, cov = post["mu"], post["cov"]
            else:
                post = eng.download(EV.SET_REPLICAS, ("mu", "v"))
                mu, cov = post["mu"], PN.diag_cov(post["v"])
            eng.free_units(EV.SET_REPLICAS)
            for k in range(k0, k1):
                sl = slice((k - k0) * 120, (k - k0 + 1) * 120)
                total += np.stack(_statement(trials, _par(params), mu[sl], cov[sl], masks[k]))
    want = PN.summary(*total)
    err = _same_summary(got, want)
    print("measured pair errors [residual_correlation channels %s]: %.2e; rms_excess %.4f over %d pairs"
          % (posterior, err, got["rms_excess"], got["n_pairs"]))
    assert err <= TOL and got["n_failed"] == 0 and got["n_pairs"] == 4
    inside = np.zeros((8, 8), dtype=bool)
    for g in groups:
        inside[np.ix_(g, g)] = True
    assert np.all(got["count"][inside] == 120) and np.all(np.isnan(got["count"][~inside]))
    assert np.all(np.isnan(got["excess_corr"][~inside])) and np.all(np.isfinite(got["excess_corr"][inside]))
    if posterior == "joint":
        assert got["converged"].shape == (3, 3) and np.all(got["converged"])
