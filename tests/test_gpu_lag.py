"""The lag moments on the device (vlgp_lag_moments, Engine.lag_moments) and evaluation.residual_autocorrelation against
the NumPy statement (tests/lag_numpy.py).  The shapes are the table of tests/lag_cases.py.

Tolerance.  err = max |device - statement| / max(1, largest |statement| entry), per lag of a table; ``count`` must match
exactly.
Both sides add products of doubles over at most a few hundred rows and differ in the order of the sums, in the Cholesky
factor's arithmetic (fused multiply-adds, a left-looking order) and in the last bits of exp and expm1;
tests/test_lag_host.py shows that no case is moved by more than rounding when its inputs move by an ulp.  TOL is a hundred
times the largest error measured on one MI355X over every case of this file
(profiles/lag_moments/measured_errors.txt has every line).  Every case prints its error."""
import copy
import functools

import numpy as np
import pytest

import heldout_numpy as H
import lag_cases as LC
import lag_numpy as LN
from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2.1e-13  # 100 x the largest measured error, 2.06e-15 (lag1 at vb = 0; module docstring)
SET, CUT, REP = 0, 1, 2


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _err(got, want):
    """Per lag (the rows of a table): the sums of a long lag are a hundredth of lag 0's and are held to their own size."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.maximum(1.0, np.max(np.abs(want), axis=1))))


def _errs(got, want):
    assert np.array_equal(got[2], want[2]), "count"
    return max(_err(got[0], want[0]), _err(got[1], want[1]))


def _engine(V, units, par, prior, R):
    L, N = par["a"].shape
    eng = V.Engine(N, L, par["b"].shape[0], R, par["gauss"])
    eng.set_params(par["a"], par["b"], par["noise"])
    eng.upload(SET, units)
    for T, G in prior.items():
        eng.set_prior(T, G)
    return eng


def _state(eng, sets=(SET,)):
    """Everything a read-only call must leave alone, as bytes."""
    return [x.tobytes() for x in eng.get_params()] + [v.tobytes() for s in sets for v in eng.download(s).values()]


def _same_bits(one, two):
    return all(np.asarray(u).tobytes() == np.asarray(w).tobytes() for u, w in zip(one, two))


@pytest.mark.parametrize("name", LC.PLAIN)
def test_plain_set(V, name):
    units, par, prior, R = LC.problem(name)
    lengths, N, L, P, K = LC.CASES[name][:5]
    with _engine(V, units, par, prior, R) as eng:
        before = _state(eng)
        got = {vb: eng.lag_moments(SET, K, vb=vb) for vb in (True, False)}
        assert _same_bits(got[True], eng.lag_moments(SET, K, vb=True))
        assert _state(eng) == before
    errs = {}
    for vb in (True, False):
        want = LC.statement(name, vb)
        assert got[vb][3] == want[3] == 0 and got[vb][0].shape == (K + 1, N)
        assert np.array_equal(want[2], np.repeat([[sum(max(T - k, 0) for T in lengths)] for k in range(K + 1)], N, axis=1))
        errs["vb %d" % vb] = _errs(got[vb], want)
    assert not got[False][1][1:].any()  # (a point posterior: no covariance across rows, exactly)
    print("measured lag errors [plain %s rows %s N %d L %d P %d K %d]: %s" % (name, list(lengths), N, L, P, K,
                                                                                ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("name", LC.MASKED)
def test_masked_set_scores_what_each_replica_holds_out(V, name):
    """Own mu, v after an E-step (so that the replicas' posteriors differ): replica k reads its own rows of the posterior, the
    source's rows of y and x, w over the entries it does not hold out and the pairs of the entries it does."""
    units, par, prior, R = LC.problem(name)
    lengths, N, L, P, K = LC.CASES[name][:5]
    rows = sum(lengths)
    held = LC.masks(name)
    n_rep = len(held)
    with _engine(V, units, par, prior, R) as eng:
        eng.replicate(SET, REP, held_out=held)
        eng.estep(REP, 2, 5.0, True)
        before = _state(eng, (SET, REP))
        post = eng.download(REP, ("mu", "v"))
        got = eng.lag_moments(REP, K)
        assert _same_bits(got, eng.lag_moments(REP, K))
        assert _state(eng, (SET, REP)) == before
    assert got[0].shape == (n_rep, K + 1, N) and got[3] == 0
    assert np.abs(post["mu"][:rows] - post["mu"][rows:2 * rows]).max() > 1e-3
    errs = []
    for k in range(n_rep):
        sl = slice(k * rows, (k + 1) * rows)
        want = LN.lag_moments(LC.with_posterior(units, post["mu"][sl], post["v"][sl]), par, prior, K,
                              live=LC.per_unit(held[k], lengths))
        errs.append(_errs([g[k] for g in got[:3]], want))
        dead = ~held[k].any(axis=0)
        assert not got[2][k][:, dead].any() and not got[0][k][:, dead].any() and not got[1][k][:, dead].any()
    assert not held[n_rep - 1].any() or name != "speckled"  # (a replica that holds nothing out: all zeros, checked above)
    print("measured lag errors [masked %s x %d rows %s N %d L %d P %d K %d]: %.2e" % (name, n_rep, list(lengths), N, L, P, K, max(errs)))
    assert max(errs) <= TOL


def test_what_y_holds_at_an_entry_that_is_not_live_is_never_read(V):
    """NaN in y wherever no replica holds the entry out: the same bits as with the finite y."""
    name = "speckled"
    units, par, prior, R = LC.problem(name)
    lengths, K = LC.CASES[name][0], LC.CASES[name][4]
    held = LC.masks(name)
    seen = LC.per_unit(held.any(axis=0), lengths)
    dirty = [dict(u, y=np.where(s, u["y"], np.nan)) for u, s in zip(units, seen)]
    got = []
    for us in (units, dirty):
        with _engine(V, us, par, prior, R) as eng:
            eng.replicate(SET, REP, held_out=held)
            got.append(eng.lag_moments(REP, K))
    assert _same_bits(got[0], got[1]) and np.isfinite(got[0][0]).all() and got[0][2].any()


def test_an_all_live_mask(V):
    """A masked set that holds every entry out scores every pair, as the plain set does: ``resid`` and ``count`` are the
    plain set's bits.  Its posterior saw nothing, so its w is 0 and ``model`` is the prior's: against the statement."""
    name = "folds"
    units, par, prior, R = LC.problem(name)
    lengths, N, K = LC.CASES[name][0], LC.CASES[name][1], LC.CASES[name][4]
    with _engine(V, units, par, prior, R) as eng:
        plain = eng.lag_moments(SET, K)
        eng.replicate(SET, REP, held_out=np.ones((1, sum(lengths), N), dtype=bool))
        post = eng.download(REP, ("mu", "v"))
        got = eng.lag_moments(REP, K)
    assert np.array_equal(post["mu"], np.concatenate([u["mu"] for u in units]))  # (a replica starts from the source's)
    assert got[0][0].tobytes() == plain[0].tobytes() and got[2][0].tobytes() == plain[2].tobytes()
    want = LN.lag_moments(LC.with_posterior(units, post["mu"], post["v"]), par, prior, K,
                          live=[np.ones((T, N), dtype=bool) for T in lengths])
    err = _errs([g[0] for g in got[:3]], want)
    print("measured lag errors [all-live mask]: %.2e" % err)
    assert err <= TOL


def test_a_unit_without_a_factor_drops_out(V):
    """A NaN in v of one row makes that row's w NaN for every latent: every H_l of its unit has no factor, n_failed counts
    them, the unit is in no sum and the other units add what they add without it."""
    name = "chunks"
    units, par, prior, R = LC.problem(name)
    lengths, N, L, P, K = LC.CASES[name][:5]
    broken = [dict(u) for u in units]
    broken[2] = dict(units[2], v=units[2]["v"].copy())
    broken[2]["v"][77, 1] = np.nan
    with _engine(V, broken, par, prior, R) as eng:
        got = eng.lag_moments(SET, K)
    want = LN.lag_moments(broken, par, prior, K)
    rest = LN.lag_moments(units[:2] + units[3:], par, prior, K)
    assert got[3] == want[3] == L and np.array_equal(want[2], rest[2]) and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    err = max(_errs(got, want), _errs(got, rest))
    print("measured lag errors [a unit without a factor]: %.2e" % err)
    assert err <= TOL


def test_a_tiling_cut_counts_no_pair_across_windows(V):
    name = "chunks"
    _, par, _, R = LC.problem(name)
    N, L, K, W = LC.CASES[name][1], LC.CASES[name][2], LC.CASES[name][4], 64
    rng = np.random.default_rng(11)
    units = [{"y": rng.poisson(1.0, (T, N)).astype(float), "x": None, "mu": 0.3 * rng.standard_normal((T, L)),
              "v": 0.05 + 0.1 * rng.random((T, L)), "w": np.ones((T, L))} for T in (128, 192)]
    prior = {T: np.stack([LC.JS.factor(T, om, R, 9 + l) for l, om in enumerate(np.geomspace(2.0, 0.02, L))]) for T in (W, 128, 192)}
    with _engine(V, units, par, prior, R) as eng:
        eng.cut(SET, CUT, np.arange(0, 320, W), W)
        got = eng.lag_moments(CUT, K)
        whole = eng.lag_moments(SET, K)
    rows = LC.per_unit(np.concatenate([u["y"] for u in units]), [W] * 5)
    windows = [{"y": y, "x": None, "mu": m, "v": v} for y, m, v in zip(
        rows, LC.per_unit(np.concatenate([u["mu"] for u in units]), [W] * 5), LC.per_unit(np.concatenate([u["v"] for u in units]), [W] * 5))]
    want = LN.lag_moments(windows, par, prior, K)
    assert np.array_equal(got[2], np.repeat([[5 * max(W - k, 0)] for k in range(K + 1)], N, axis=1))
    assert np.array_equal(whole[2][:, 0], [sum(max(T - k, 0) for T in (128, 192)) for k in range(K + 1)])
    err = _errs(got, want)
    print("measured lag errors [tiling cut]: %.2e" % err)
    assert err <= TOL and got[3] == 0


def test_lag_zero_at_the_fixed_point_is_the_diagonal_of_the_pair_moments(V):
    """update_w / update_v iterated to the fixed point v = diag S(w(v)): c_l(t, t) = v_tl, so lag 0 is the diagonal of
    Engine.pair_moments, which reads the stored v."""
    name = "folds"
    units, par, prior, R = LC.problem(name)
    K = LC.CASES[name][4]
    with _engine(V, units, par, prior, R) as eng:
        for _ in range(60):
            eng.update_w(SET)
            assert eng.update_v(SET) == 0
        v = eng.download(SET, ("v",))["v"]
        eng.update_w(SET)
        eng.update_v(SET)
        moved = float(np.abs(eng.download(SET, ("v",))["v"] - v).max())
        lag = eng.lag_moments(SET, K)
        resid, model = eng.pair_moments(SET)
    err = max(_err(lag[0][0], np.diagonal(resid)), _err(lag[1][0], np.diagonal(model)))
    print("measured lag errors [lag 0 against pair_moments at the fixed point, v still moving by %.1e]: %.2e" % (moved, err))
    assert moved <= 1e-14 and err <= TOL


def test_refusals_leave_everything_as_it_was(V):
    from vlgp_amd._lib import dptr

    units, par, prior, R = LC.problem("folds")
    N, K = LC.CASES["folds"][1], 3
    with _engine(V, units, par, prior, R) as eng:
        eng.cut(SET, CUT, np.array([0, 40, 15, 55]), 25)
        eng.replicate(SET, REP, groups=[[1, 3], [5]])
        before = _state(eng, (SET, CUT, REP))
        with pytest.raises(V.VlgpError, match="status -3.*vlgp_lag_moments on a copied cut: merge it and score the source set"):
            eng.lag_moments(CUT, K)
        with pytest.raises(V.VlgpError, match="status -3.*replicate with held_out="):
            eng.lag_moments(REP, K)
        with pytest.raises(V.VlgpError, match="status -1.*max_lag = 65, need 0 <= max_lag <= 64"):
            eng.lag_moments(SET, 65)
        with pytest.raises(ValueError, match="max_lag"):
            eng.lag_moments(SET, -1)
        out = np.full((K + 1, N), 7.0)
        lib, h = eng.lib, eng.h
        assert lib.vlgp_lag_moments(h, SET, 1, K, None, dptr(out), dptr(out), None) == -1
        assert b"needs resid, model and count" in lib.vlgp_last_error(h) and np.all(out == 7.0)
        assert lib.vlgp_lag_moments(h, SET, 1, -1, dptr(out), dptr(out), dptr(out), None) == -1 and np.all(out == 7.0)
        assert _state(eng, (SET, CUT, REP)) == before
        eng.free_units(REP)
        eng.free_units(CUT)
        two, three = out.copy(), out.copy()
        assert lib.vlgp_lag_moments(h, SET, 1, K, dptr(out), dptr(two), dptr(three), None) == 0  # (n_failed may be null)
        assert _same_bits((out, two, three), eng.lag_moments(SET, K)[:3])
    with _engine(V, units, par, {}, R) as eng:
        with pytest.raises(V.VlgpError, match="no prior factor for unit length"):
            eng.lag_moments(SET, K)


# ---- evaluation.residual_autocorrelation end to end ----------------------------------------------------------------------
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


def test_residual_autocorrelation_in_sample(V):
    from vlgp_amd import evaluation as EV

    trials, params, config = copy.deepcopy(_public())
    got = EV.residual_autocorrelation(trials, params, config, max_lag=41)
    want = LN.summary(*LN.lag_moments(trials, _par(params), params["cholesky"], 41)[:3])
    err = _same_summary(got, want)
    print("measured lag errors [residual_autocorrelation in_sample]: %.2e; rms_excess_all %.4f over %d" % (err, got["rms_excess_all"], got["n_scored"]))
    assert err <= TOL and got["n_failed"] == 0 and got["n_scored"] == 39 * 8
    assert np.all(got["count"][:40] == 3 * (40 - np.arange(40))[:, None]) and np.all(np.isnan(got["count"][40:]))
    assert np.all(np.isnan(got["excess_acf"][40:])) and np.all(got["model_acf"][0] == 1.0)


def test_residual_autocorrelation_of_channel_folds(V):
    """The folds held out one replica each, the latents inferred without them, every channel scored in the replica that
    held it out under the posterior the engine inferred (the same calls, made here); a channel of no fold is never scored."""
    from vlgp_amd import evaluation as EV

    trials, params, config = copy.deepcopy(_public())
    groups, K = [[0, 5, 6], [2, 3], [7]], 6
    got = EV.residual_autocorrelation(trials, params, config, max_lag=K, how="channels", groups=groups)
    masks = np.stack(list(EV._group_masks(groups, 120, 8)))
    total = np.zeros((3, K + 1, 8))
    with EV._resident(trials, params, EV._zero_start(trials, 2), 0) as eng:
        eng.replicate(EV.SET_TEST, EV.SET_REPLICAS, held_out=masks)
        assert eng.estep(EV.SET_REPLICAS, config["max_iter"], config["dmu_bound"], True) == 0
        post = eng.download(EV.SET_REPLICAS, ("mu", "v"))
    for k in range(3):
        sl = slice(k * 120, (k + 1) * 120)
        total += np.stack(LN.lag_moments(LC.with_posterior(trials, post["mu"][sl], post["v"][sl]), _par(params), params["cholesky"],
                                         K, live=LC.per_unit(masks[k], [40] * 3))[:3])
    want = LN.summary(*total)
    err = _same_summary(got, want)
    print("measured lag errors [residual_autocorrelation channels]: %.2e; rms_excess_all %.4f over %d" % (err, got["rms_excess_all"], got["n_scored"]))
    assert err <= TOL and got["n_failed"] == 0 and got["n_scored"] == 6 * K
    inside = np.isin(np.arange(8), sum(groups, []))
    assert np.all(got["count"][:, inside] == 3 * (40 - np.arange(K + 1))[:, None]) and np.all(np.isnan(got["count"][:, ~inside]))
