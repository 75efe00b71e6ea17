"""Posterior-predictive scores on the device (vlgp_predictive, Engine.predictive, the predictive= keyword of
vlgp_amd.evaluation and cross_validate) against the NumPy restatement of their definition (tests/predictive_numpy.py).

Shapes: 3 units of 70, 300 and 70 rows -- 440 rows, two workgroups, the second one partial -- N = 14 with and without 2
Gaussian channels, L = 3, with and without regressors (history = 2).  The posterior of the plain-set cases is random with
v uniform in [0, 1) and the loadings are scaled until m = a.mu + b x spans about -8 ... 11, both sides of the clamp of
trunc_exp; the counts hold zeros and values up to 30.

Tolerance of the entry-wise comparison, on |device - numpy| / max(1, |numpy|).  Both sides run the same steps in double
precision; they differ in the library behind exp, log and lgamma, in fused multiply-adds and in the order of the
log-sum-exp (online on the device).  A term of the sum is lwa + y c - exp(c) - (eta - m)^2 / (2 s2) with exp(c) up to
2.2e4 and the quadratic up to a few hundred, so a rounding of 2^-53 of those is 1e-12 absolute before the cancellation
that leaves lpd; the Newton iterate carries a few ulp into every node.  Measured on one MI355X
(profiles/predictive/measured_errors.txt): at most 8.2e-15 on the plain sets at 1, 12, 20 and 64 nodes and 1.2e-14 on the
replicas; ENTRY_TOL is 100 times the largest of them, well inside the ceiling of 1e-9.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
from scipy.special import gammaln

import heldout_numpy as H
import predictive_numpy as PN
import speckled_numpy as S
from conftest import relerr
from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [70, 300, 70]
CASES = {"poisson": dict(n_gauss=0, history=0), "mixed": dict(n_gauss=2, history=0),
         "history": dict(n_gauss=0, history=2), "mixed-history": dict(n_gauss=2, history=2)}
NODES = (1, 12, 20, 64)
ENTRY_TOL = 1.2e-12  # 100 x the largest measured error (module docstring)
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def scaled(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


@functools.lru_cache(maxsize=None)
def _dense(case, wide=True):
    """Units with a random posterior and, with ``wide``, loadings and counts that reach both sides of the clamp."""
    kw = CASES[case]
    trials, params, config = H.problem(seed=17, M=3, T=300, N=14, L=3, lengths=LENGTHS, max_iter=2, **kw)
    rng = np.random.default_rng(5)
    N, L, ng = 14, 3, kw["n_gauss"]
    if wide:
        params["a"] = 1.1 * rng.standard_normal((L, N))
        params["b"][0, :N - ng] = rng.uniform(-1.5, 4.5, N - ng)
    for tr in trials:
        T = tr["y"].shape[0]
        if wide:
            cnt = rng.integers(0, 31, (T, N - ng)).astype(float)
            cnt[rng.random(cnt.shape) < 0.4] = 0.0
            tr["y"][:, :N - ng] = cnt
            tr["x"] = H.lagged(tr["y"], kw["history"])
            if kw["history"]:  # (30 spikes a bin back must not swamp the predictor)
                tr["x"][:, 1:, :] *= 0.1
        tr["mu"] = (1.1 if wide else 1.0) * rng.standard_normal((T, L))
        tr["v"] = rng.random((T, L))
        tr["w"] = np.zeros((T, L))
    return trials, params, config


def dense(case, wide=True):
    trials, params, config = _dense(case, wide)
    return copy.deepcopy(trials), copy.deepcopy(params), dict(config)


def gauss_of(params):
    return np.asarray(params["likelihood"]) == "gaussian"


def resident(trials, params, zero_start=False):
    """An engine holding the trials as set 0 (their own posterior, or a zero start), the parameters and the priors."""
    from vlgp_amd.api import bind_priors
    from vlgp_amd.engine import Engine

    L = params["zdim"]
    eng = Engine.for_params(params)
    eng.set_params(params["a"], params["b"], params["noise"])
    zeros = lambda t: np.zeros((t["y"].shape[0], L))  # noqa: E731
    eng.upload(0, [{"y": t["y"], "x": t.get("x"), "mu": zeros(t) if zero_start else t["mu"],
                    "v": zeros(t) if zero_start else t["v"], "w": None} for t in trials])
    bind_priors(eng, trials, dict(params))
    return eng


@functools.lru_cache(maxsize=None)
def _plain_reference(case, n_nodes):
    trials, params, _ = _dense(case)
    return PN.score_plain(trials, params["a"], params["b"], params["noise"], gauss_of(params), True, n_nodes)


@pytest.mark.parametrize("case", sorted(CASES))
def test_plain_set_matches_the_restatement(V, case):
    trials, params, _ = dense(case)
    gauss = gauss_of(params)
    m = np.concatenate([O.linear_predictor(t["x"], t["mu"], params["a"], params["b"]) for t in trials])[:, ~gauss]
    assert m.min() < -7.0 and (m > 10.0).sum() >= 5, (m.min(), m.max())  # both sides of the clamp
    y = np.concatenate([t["y"] for t in trials])[:, ~gauss]
    assert y.min() == 0.0 and y.max() == 30.0
    with resident(trials, params) as eng:
        for n_nodes in NODES:
            want_lpd, want_rate, want_sums = _plain_reference(case, n_nodes)
            sums, rate, lpd = eng.predictive(0, n_nodes=n_nodes, want_rate=True, want_lpd=True)
            assert sums.shape == (14, 4) and rate.shape == lpd.shape == (440, 14)
            errs = (scaled(lpd, want_lpd), scaled(rate, want_rate), scaled(sums, want_sums))
            print("measured predictive %-13s n_nodes %2d  lpd %.2e  rate %.2e  sums %.2e" % ((case, n_nodes) + errs))
            assert np.all(np.isfinite(lpd)) and max(errs) <= ENTRY_TOL, (n_nodes, errs)
            only_sums, no_rate, no_lpd = eng.predictive(0, n_nodes=n_nodes)
            assert no_rate is None and no_lpd is None and np.array_equal(only_sums, sums)


@pytest.mark.parametrize("case", ["poisson", "mixed-history"])
def test_zero_variance_reproduces_the_plug_in_score(V, case):
    """vb = 0, and vb = 1 with v = 0: lpd is the plug-in log-likelihood of vlgp_loglik's own rate.  Per entry the two
    sides may differ by the libraries behind log and lgamma: 2 ulp each on either side of y log rate, rate and
    lgamma(y + 1).  The sums come from the same device expressions in the same order: relative 1e-13.  Columns 1 ... 3
    of the sums are vlgp_loglik's for any v."""
    trials, params, _ = dense(case)
    pois = ~gauss_of(params)
    y = np.concatenate([t["y"] for t in trials])
    flat = copy.deepcopy(trials)
    for t in flat:
        t["v"] = np.zeros_like(t["v"])
    for units, vb in ((trials, False), (flat, True)):
        with resident(units, params) as eng:
            ref_sums, ref_rate = eng.loglik(0, vb=vb, want_rate=True)
            sums, rate, lpd = eng.predictive(0, n_nodes=12, vb=vb, want_rate=True, want_lpd=True)
        assert np.array_equal(rate, ref_rate)
        r, yp = ref_rate[:, pois], y[:, pois]
        terms = np.abs(yp * np.log(r)) + r + gammaln(yp + 1.0)
        ll = yp * np.log(r) - r - gammaln(yp + 1.0)
        assert np.all(np.abs(lpd[:, pois] - ll) <= 4 * ULP * terms + ULP * np.abs(ll))
        assert np.all(np.abs(sums - ref_sums) <= 1e-13 * np.abs(ref_sums))
    with resident(trials, params) as eng:  # any v: the sums of y, of the rate and of lgamma(y + 1) or y^2
        ref_sums, _ = eng.loglik(0)
        sums, _, _ = eng.predictive(0, n_nodes=12)
    assert np.all(np.abs(sums[:, 1:] - ref_sums[:, 1:]) <= 1e-13 * np.abs(ref_sums[:, 1:]))
    assert np.all(sums[pois, 0] != ref_sums[pois, 0])


GROUPS = [[3, 12], [7]]


@pytest.mark.parametrize("case", ["mixed", "history"])
def test_group_replicas_match_the_restatement_under_their_own_posterior(V, case):
    trials, params, config = dense(case, wide=False)
    L = params["zdim"]
    with resident(trials, params, zero_start=True) as eng:
        eng.replicate(0, 2, groups=GROUPS)
        assert eng.estep(2, 2, config["dmu_bound"], True) == 0
        post = {k: v.reshape(2, 440, L) for k, v in eng.download(2, ("mu", "v")).items()}
        sums, rate, lpd = eng.predictive(2, n_nodes=12, want_rate=True, want_lpd=True)
        ref_sums, ref_rate = eng.loglik(2, want_rate=True)
    want = PN.score_groups(trials, GROUPS, post["mu"], post["v"], params["a"], params["b"], params["noise"],
                           gauss_of(params), True, 12)
    assert sums.shape == (3, 4) and rate.shape == lpd.shape == (440, 3)
    errs = (scaled(lpd, want[0]), scaled(rate, want[1]), scaled(sums, want[2]))
    print("measured predictive groups %-8s lpd %.2e  rate %.2e  sums %.2e" % ((case,) + errs))
    assert max(errs) <= ENTRY_TOL
    assert np.array_equal(rate, ref_rate) and np.array_equal(sums[:, 1:], ref_sums[:, 1:])


def masks(rng, rows, N):
    """Three replicas: two disjoint random masks, the first also holding row 5 out entirely, and an empty one."""
    F = rng.integers(0, 4, (rows, N))
    held = np.stack([F == 0, F == 1, np.zeros((rows, N), dtype=bool)])
    held[0, 5], held[1, 5] = True, False
    return held


@pytest.mark.parametrize("case", ["mixed", "history"])
def test_masked_replicas_score_their_held_out_entries_only(V, case):
    trials, params, config = dense(case, wide=False)
    L, N = params["zdim"], params["ydim"]
    held = masks(np.random.default_rng(2), 440, N)
    with resident(trials, params, zero_start=True) as eng:
        eng.replicate(0, 2, held_out=held)
        assert eng.estep(2, 2, config["dmu_bound"], True) == 0
        post = {k: v.reshape(3, 440, L) for k, v in eng.download(2, ("mu", "v")).items()}
        sums, rate, lpd = eng.predictive(2, n_nodes=12, want_rate=True, want_lpd=True)
        eng.free_units(2)
        both = held.copy()
        both[1, 9, 3] = both[0, 9, 3] = True  # one entry held out twice
        eng.replicate(0, 2, held_out=both)
        for kw in (dict(want_lpd=True), dict(want_rate=True)):
            with pytest.raises(V.VlgpError, match="status -1.*vlgp_predictive.*overlap"):
                eng.predictive(2, **kw)
        twice, no_rate, no_lpd = eng.predictive(2)
        assert twice.shape == (3, N, 4) and no_rate is None and no_lpd is None and np.all(np.isfinite(twice))
    want = PN.score_masked(trials, held, post["mu"], post["v"], params["a"], params["b"], params["noise"],
                           gauss_of(params), True, 12)
    never = ~held.any(axis=0)
    assert np.array_equal(np.isnan(lpd), never) and np.array_equal(np.isnan(rate), never)
    errs = (scaled(lpd[~never], want[0][~never]), scaled(rate[~never], want[1][~never]), scaled(sums, want[2]))
    print("measured predictive masked %-8s lpd %.2e  rate %.2e  sums %.2e" % ((case,) + errs))
    assert max(errs) <= ENTRY_TOL
    assert np.all(sums[2] == 0.0) and np.all(sums[:2, :, 0] != 0.0)


def test_jensen_against_the_expected_log_likelihood_of_vlgp_elbo(V):
    """log E_q p(y | eta) >= E_q log p(y | eta), entry by entry, so the row sums of lpd bound vlgp_elbo's row_ell -- an
    independent kernel -- from above; 1e-6 per entry covers the quadrature (20 nodes: 2e-8)."""
    trials, params, _ = dense("mixed", wide=False)
    a = params["a"]
    m = np.concatenate([O.linear_predictor(t["x"], t["mu"], a, params["b"]) for t in trials])
    sd = np.sqrt(np.concatenate([t["v"] for t in trials]) @ a ** 2)
    assert np.all(m + 3 * sd < 10.0)
    with resident(trials, params) as eng:
        _, _, lpd = eng.predictive(0, n_nodes=20, want_lpd=True)
        row_ell = eng.elbo(0, want_rows=True)[3]
    gap = lpd.sum(axis=1) - row_ell
    print("measured predictive jensen gap per row: min %.3e  mean %.3e" % (gap.min(), gap.mean()))
    assert np.all(gap >= -1e-6 * 14) and gap.mean() > 1e-3


def test_same_bits_refusals_and_an_untouched_handle(V):
    trials, params, _ = dense("mixed-history")
    z, lwa = V.evaluation.hermite_nodes(12)
    dp = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    with resident(trials, params) as eng:
        before = (eng.download(0), eng.get_params())
        one = eng.predictive(0, n_nodes=20, want_rate=True, want_lpd=True)
        two = eng.predictive(0, n_nodes=20, want_rate=True, want_lpd=True)
        assert all(np.array_equal(x, y) for x, y in zip(one, two))
        sums = np.full((14, 4), 7.0)
        for n_nodes in (0, 65):
            rc = eng.lib.vlgp_predictive(eng.h, 0, 1, n_nodes, dp(z), dp(lwa), None, None, dp(sums))
            assert rc == -1
            with pytest.raises(V.VlgpError, match=r"status -1.*vlgp_predictive.*n_nodes = %d" % n_nodes):
                eng.check(rc)
        for args in ((None, dp(lwa), dp(sums)), (dp(z), None, dp(sums)), (dp(z), dp(lwa), None)):
            rc = eng.lib.vlgp_predictive(eng.h, 0, 1, 12, args[0], args[1], None, None, args[2])
            assert rc == -1
            with pytest.raises(V.VlgpError, match="status -1.*vlgp_predictive needs z, lwa and sums"):
                eng.check(rc)
        assert np.all(sums == 7.0)
        eng.cut(0, 1, np.array([0, 20]), 50)  # two windows that do not tile the set: a copied cut
        with pytest.raises(V.VlgpError, match="status -3.*vlgp_predictive on a copied cut"):
            eng.predictive(1)
        eng.free_units(1)
        after = (eng.download(0), eng.get_params())
        assert all(np.array_equal(before[0][k], after[0][k]) for k in before[0])
        assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
        assert all(np.array_equal(x, y) for x, y in zip(eng.predictive(0, n_nodes=20, want_rate=True, want_lpd=True), one))


def same_dict(x, y):
    assert list(x) == list(y)
    for key in x:
        for p, q in zip(*((v if isinstance(v, list) else [v]) for v in (x[key], y[key]))):
            assert np.array_equal(np.asarray(p), np.asarray(q), equal_nan=np.asarray(p).dtype.kind == "f"), key
    return True


def test_forward_prediction_scores_the_returned_posterior(V):
    trials, params, config = H.problem(seed=11, M=4, T=80, n_gauss=2, history=2, max_iter=3)
    ev, nf = V.evaluation, 12
    got = ev.forward_prediction(trials, params, config, nf, predictive=True, n_nodes=20)
    plain = ev.forward_prediction(trials, params, config, nf)
    assert got["density"] == "predictive" and "density" not in plain
    assert same_dict(plain, ev.forward_prediction(trials, params, config, nf, predictive=False))
    assert set(got) == set(plain) | {"density"}
    gauss = gauss_of(params)
    ll = np.zeros(params["ydim"])
    for tr, mu, v, rate in zip(trials, got["mu_ahead"], got["v_ahead"], got["rate"]):
        lpd, r = PN.lpd_rate(tr["y"][-nf:], tr["x"][-nf:], mu, v, params["a"], params["b"], params["noise"], gauss, True, 20)
        ll += lpd.sum(axis=0)
        assert scaled(rate, r) <= ENTRY_TOL
    assert scaled(got["ll"], ll) <= ENTRY_TOL
    for key in ("mu_ahead", "v_ahead", "rate"):
        assert all(np.array_equal(p, q) for p, q in zip(got[key], plain[key])), key
    assert np.array_equal(got["n_spikes"], plain["n_spikes"]) and np.array_equal(got["ll_null"], plain["ll_null"], equal_nan=True)
    assert np.all(got["ll"] != plain["ll"]) and got["fp_bps"] != plain["fp_bps"]


@functools.lru_cache(maxsize=None)
def _six_trials():
    return H.problem(seed=11, n_gauss=2)


def test_leave_group_out_scores_the_restated_latents(V):
    trials, params, config = copy.deepcopy(_six_trials())
    groups = [[0, 5, 13], [2]]
    a, b, noise, gauss, L = params["a"], params["b"], params["noise"], gauss_of(params), params["zdim"]
    want = np.zeros(4)
    for tr in trials:
        T = tr["y"].shape[0]
        G = O.build_prior([T], params["omega"], params["sigma"], 50)[T]
        i = 0
        for g in groups:
            a0 = a.copy()
            a0[:, g] = 0.0
            zero = np.zeros((T, L))
            mu, v = O.estep_unit(tr["y"], tr["x"], zero, zero, zero, a0, b, noise, gauss, G, config["max_iter"],
                                 config["dmu_bound"], True)[:2]
            lpd = PN.lpd_rate(tr["y"], tr["x"], mu, v, a, b, noise, gauss, True, 12)[0]
            for n in g:
                want[i] += lpd[:, n].sum()
                i += 1
    got = V.evaluation.leave_group_out(trials, params, config, groups=groups, predictive=True)
    plain = V.evaluation.leave_group_out(trials, params, config, groups=groups)
    assert got["density"] == "predictive" and got["n_failed"] == 0 and set(got) == set(plain) | {"density"}
    assert same_dict(plain, V.evaluation.leave_group_out(trials, params, config, groups=groups, predictive=False))
    err = relerr(got["ll"], want)
    print("measured predictive leave_group_out ll %.2e" % err)
    assert err < H.STAGE
    assert np.array_equal(got["ll_null"], plain["ll_null"], equal_nan=True) and np.all(got["ll"] != plain["ll"])
    assert got["co_bps"] == V.evaluation.co_bits_per_spike(got["ll"], got["ll_null"], got["n_spikes"])


def test_leave_entries_out_scores_the_restated_latents(V):
    trials, params, config = copy.deepcopy(_six_trials())
    ev = V.evaluation
    rows, N = sum(t["y"].shape[0] for t in trials), params["ydim"]
    F = ev.entry_folds(rows, N, 2, 0)
    held = np.stack([F == k for k in range(2)])
    post = S.restated(trials, params, config, held)[0]
    want = PN.score_masked(trials, held, post["mu"], post["v"], params["a"], params["b"], params["noise"],
                           gauss_of(params), True, 12)[2][:, :, 0]
    got = ev.leave_entries_out(trials, params, config, n_folds=2, seed=0, predictive=True)
    plain = ev.leave_entries_out(trials, params, config, n_folds=2, seed=0)
    assert got["density"] == "predictive" and got["n_failed"] == 0 and set(got) == set(plain) | {"density"}
    assert same_dict(plain, ev.leave_entries_out(trials, params, config, n_folds=2, seed=0, predictive=False))
    err = relerr(got["ll_per_fold"], want)
    print("measured predictive leave_entries_out ll_per_fold %.2e" % err)
    assert err < H.STAGE
    assert np.array_equal(got["ll_null"], plain["ll_null"], equal_nan=True)


def test_cross_validate_passes_the_density_through(V):
    from vlgp_amd import synth

    trials = synth.make_trials(6, 60, 8, 2, seed=41)
    kw = dict(n_trial_folds=2, n_channel_folds=2, max_iter=2, min_iter=2)
    cv = V.model_selection.cross_validate(trials, [1, 2], score="co_bps", predictive=True, **kw)
    assert cv["errors"] == [] and cv["co_bps"].shape == (2, 2) and np.all(np.isfinite(cv["co_bps"]))
    with pytest.raises(ValueError, match="marginal_bps"):
        V.model_selection.cross_validate(trials, [1], score="marginal_bps", predictive=True, **kw)
