"""Calibration of the predictive distribution on the device (vlgp_calibration, Engine.calibration,
evaluation.calibration) against the NumPy restatement of its definition (tests/calibration_numpy.py).

Shapes: two units of 150 and 151 rows -- 301 rows, two workgroups, the second one partial --, N = 70 (two mask words)
with 6 Gaussian channels, L = 3, regressors (history = 2), rates about 0.3 ... 5.  Planted: a count of 0; a count of 60 on
a row whose m is log 40 (61 masses); a row with v = 0 (the plug-in branch); vb = False is a run of its own.

Tolerance.  Both sides run the same steps in double precision; they differ in the library behind exp, log and lgamma, in
fused multiply-adds and in the order of the log-sum-exp, and an entry adds up to 61 masses.  The errors are
|device - numpy| / max(1, |numpy|) per entry and |device - numpy| / (sum of the absolute terms) per sum.  Measured on one
MI355X (profiles/calibration/measured_errors.txt): at most 6.3e-15 per entry and 7.7e-14 per sum (a bin of the 32-bin
histogram: an error of lo is divided by the mass hi - lo) over the plain set, the group replicas and the masked set at 1,
12 and 64 nodes; TOL is 100 times the largest of them.  The columns `covered`,
`entries` and `skipped` are counts and must be equal: the inputs are chosen -- and asserted, on the restatement -- to
keep every entry at least 1e-9 from a level and every point mass 1e-9 from a bin edge.
"""
import copy
import ctypes as C
import functools
import time

import numpy as np
import pytest

import calibration_numpy as CN
import heldout_numpy as H
from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [150, 151]
ROWS, N, L, NG = 301, 70, 3, 6
MEASURED = 7.71e-14  # the largest measured error (module docstring)
TOL = 100 * MEASURED
LEVELS4 = (0.5, 0.9, 0.99, 0.2)
CONFIGS = [(1, (), 1), (10, (0.5, 0.9), 12), (32, LEVELS4, 64)]  # n_bins, levels, n_nodes
GROUPS = [[3, 12, 65], [7, 69, 40]]
PLANT_ZERO, PLANT_BIG, PLANT_FLAT = (3, 0), (7, 1), 150 + 11  # (row, channel) twice and a row of the second unit


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@functools.lru_cache(maxsize=None)
def _problem():
    trials, params, config = H.problem(seed=23, M=2, T=151, N=N, L=L, n_gauss=NG, lengths=LENGTHS, history=2, max_iter=3)
    rng = np.random.default_rng(9)
    npois = N - NG
    params["b"][0, :npois] = np.log(rng.uniform(0.3, 5.0, npois))
    row0 = 0
    for tr in trials:
        T = tr["y"].shape[0]
        tr["y"][:, :npois] = rng.poisson(np.exp(params["b"][0, :npois]), (T, npois)).astype(float)
        if row0 == 0:
            tr["y"][PLANT_ZERO], tr["y"][PLANT_BIG] = 0.0, 60.0
        tr["x"] = H.lagged(tr["y"], 2)
        tr["mu"] = 0.8 * rng.standard_normal((T, L))
        tr["v"] = 0.6 * rng.random((T, L))
        tr["w"] = np.zeros((T, L))
        row0 += T
    first, a = trials[0], params["a"]
    r, n = PLANT_BIG  # m[r, n] = log 40
    m = O.linear_predictor(first["x"][r:r + 1], first["mu"][r:r + 1], a, params["b"])[0, n]
    first["mu"][r] += (np.log(40.0) - m) * a[:, n] / np.sum(a[:, n] ** 2)
    trials[1]["v"][PLANT_FLAT - 150] = 0.0
    return trials, params, config


def problem():
    trials, params, config = _problem()
    return copy.deepcopy(trials), copy.deepcopy(params), dict(config)


def gauss_of(params):
    return np.asarray(params["likelihood"]) == "gaussian"


def par(params):
    return params["a"], params["b"], params["noise"], gauss_of(params)


def resident(trials, params, zero_start=False):
    """An engine holding the trials as set 0 (their own posterior, or a zero start), the parameters and the priors."""
    from vlgp_amd.api import bind_priors
    from vlgp_amd.engine import Engine

    eng = Engine.for_params(params)
    eng.set_params(params["a"], params["b"], params["noise"])
    zeros = lambda t: np.zeros((t["y"].shape[0], params["zdim"]))  # noqa: E731
    eng.upload(0, [{"y": t["y"], "x": t.get("x"), "mu": zeros(t) if zero_start else t["mu"],
                    "v": zeros(t) if zero_start else t["v"], "w": None} for t in trials])
    bind_priors(eng, trials, dict(params))
    return eng


def entry_err(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok])), initial=0.0))


def sums_err(got, want, terms, axis):
    """|got - want| relative to the sum of the absolute terms of every sum (a sum without a term must be 0 exactly)."""
    den = np.abs(terms).sum(axis=axis)
    assert got.shape == want.shape == den.shape, (got.shape, want.shape, den.shape)
    assert np.all(got[den == 0.0] == 0.0)
    return float(np.max(np.abs(got - want) / np.where(den > 0.0, den, 1.0)))


def counts_equal(got, want, n_bins):
    """The columns covered | entries | skipped, which hold counts, are equal."""
    return np.array_equal(got[..., n_bins:-3], want[..., n_bins:-3]) and np.array_equal(got[..., -2:], want[..., -2:])


def check_margin(cdf, n_bins, levels):
    lo, hi = cdf[..., 0], cdf[..., 1]
    margin = CN.edge_margin(lo, hi, np.isnan(lo), n_bins, levels)
    assert margin > 1e-9, margin  # a condition on the inputs: choose another seed


@functools.lru_cache(maxsize=None)
def _plain_reference(config_index, vb=True):
    trials, params, _ = _problem()
    n_bins, levels, n_nodes = CONFIGS[config_index]
    return CN.score_plain(trials, *par(params), vb, n_nodes, n_bins, levels)


@pytest.mark.parametrize("config_index", range(len(CONFIGS)))
def test_plain_set_matches_the_restatement(V, config_index):
    trials, params, _ = problem()
    n_bins, levels, n_nodes = CONFIGS[config_index]
    want_cdf, want_sums, terms = _plain_reference(config_index)
    check_margin(want_cdf, n_bins, levels)
    y = np.concatenate([t["y"] for t in trials])
    assert y[PLANT_ZERO] == 0.0 and y[PLANT_BIG] == 60.0 and want_cdf[PLANT_ZERO][0] == 0.0
    with resident(trials, params) as eng:
        sums, cdf = eng.calibration(0, n_bins=n_bins, levels=levels, n_nodes=n_nodes, want_cdf=True)
        lpd = eng.predictive(0, n_nodes=n_nodes, want_lpd=True)[2]
        only_sums, none = eng.calibration(0, n_bins=n_bins, levels=levels, n_nodes=n_nodes)
    W = n_bins + len(levels) + 3
    assert sums.shape == (N, W) and cdf.shape == (ROWS, N, 2)
    errs = (entry_err(cdf, want_cdf), sums_err(sums, want_sums, terms, 0))
    print("measured calibration plain bins %2d levels %d nodes %2d  cdf %.2e  sums %.2e" % ((n_bins, len(levels), n_nodes) + errs))
    assert max(errs) <= TOL, errs
    assert counts_equal(sums, want_sums, n_bins)
    # the optional output changes no bit of the sums
    assert none is None and only_sums.tobytes() == sums.tobytes()
    # invariants
    lo, hi = cdf[..., 0], cdf[..., 1]
    assert np.all((0.0 <= lo) & (lo <= hi) & (hi <= 1.0))
    assert np.all(np.abs(sums[:, :n_bins].sum(axis=1) - sums[:, -2]) <= 1e-12 * sums[:, -2])
    assert np.all(sums[:, -2] == ROWS) and np.all(sums[:, -1] == 0.0)
    # consistency with vlgp_predictive: hi - lo is the mass of the observed count.  exp(lpd) answers a rounding of lpd
    # with p |ln p| 2^-53 <= 2^-53 / e, and hi - lo carries the rounding of hi <= 1: a few ulp of 1, 1e-14 absolute
    pois = ~gauss_of(params)
    open_ = pois[None, :] & (hi < 1.0)
    assert open_.sum() > 0.99 * pois.sum() * ROWS
    gap = np.abs((hi - lo) - np.exp(lpd))[open_]
    print("measured calibration plain nodes %2d  |(hi - lo) - exp(lpd)| %.2e" % (n_nodes, gap.max()))
    assert gap.max() <= 1e-14


def test_map_and_flat_rows_take_the_plug_in_mass(V):
    """vb = False, and the row with v = 0 under vb = True: the masses are the Poisson masses at the plug-in rate."""
    from scipy.stats import poisson

    trials, params, _ = problem()
    n_bins, levels, n_nodes = CONFIGS[1]
    want_cdf, want_sums, terms = _plain_reference(1, vb=False)
    check_margin(want_cdf, n_bins, levels)
    with resident(trials, params) as eng:
        sums, cdf = eng.calibration(0, n_bins=n_bins, levels=levels, n_nodes=n_nodes, vb=False, want_cdf=True)
        rate = eng.loglik(0, vb=False, want_rate=True)[1]
        flat_cdf = eng.calibration(0, n_nodes=n_nodes, want_cdf=True)[1][PLANT_FLAT]
        flat_rate = eng.loglik(0, want_rate=True)[1][PLANT_FLAT]
    errs = (entry_err(cdf, want_cdf), sums_err(sums, want_sums, terms, 0))
    print("measured calibration plain vb=0  cdf %.2e  sums %.2e" % errs)
    assert max(errs) <= TOL and counts_equal(sums, want_sums, n_bins)
    pois = ~gauss_of(params)
    y = np.concatenate([t["y"] for t in trials])
    assert np.max(np.abs(cdf[..., 1][:, pois] - poisson.cdf(y[:, pois], rate[:, pois]))) <= 1e-12
    assert np.max(np.abs(flat_cdf[pois, 0] - poisson.cdf(y[PLANT_FLAT, pois] - 1, flat_rate[pois]))) <= 1e-12


def test_group_replicas_match_the_restatement_under_their_own_posterior(V):
    trials, params, config = problem()
    with resident(trials, params, zero_start=True) as eng:
        eng.replicate(0, 2, groups=GROUPS)
        assert eng.estep(2, 3, config["dmu_bound"], True) == 0
        post = {k: v.reshape(2, ROWS, L) for k, v in eng.download(2, ("mu", "v")).items()}
        got = {i: eng.calibration(2, n_bins=c[0], levels=c[1], n_nodes=c[2], want_cdf=True) for i, c in enumerate(CONFIGS)}
    for i, (n_bins, levels, n_nodes) in enumerate(CONFIGS):
        want_cdf, want_sums, terms = CN.score_groups(trials, GROUPS, post["mu"], post["v"], *par(params), True, n_nodes,
                                                     n_bins, levels)
        check_margin(want_cdf, n_bins, levels)
        sums, cdf = got[i]
        assert sums.shape == (6, n_bins + len(levels) + 3) and cdf.shape == (ROWS, 6, 2)
        errs = (entry_err(cdf, want_cdf), sums_err(sums, want_sums, terms, 0))
        print("measured calibration groups bins %2d levels %d nodes %2d  cdf %.2e  sums %.2e"
              % ((n_bins, len(levels), n_nodes) + errs))
        assert max(errs) <= TOL and counts_equal(sums, want_sums, n_bins)
        assert np.all(sums[:, -2] == ROWS) and np.all(sums[:, -1] == 0.0)
        assert np.all(np.abs(sums[:, :n_bins].sum(axis=1) - ROWS) <= 1e-12 * ROWS)


def masks():
    """Two replicas with disjoint random masks, the first also holding row 5 out entirely."""
    F = np.random.default_rng(2).integers(0, 3, (ROWS, N))
    held = np.stack([F == 0, F == 1])
    held[0, 5], held[1, 5] = True, False
    return held


def test_masked_replicas_score_their_held_out_entries_only(V):
    trials, params, config = problem()
    held = masks()
    with resident(trials, params, zero_start=True) as eng:
        eng.replicate(0, 2, held_out=held)
        assert eng.estep(2, 3, config["dmu_bound"], True) == 0
        post = {k: v.reshape(2, ROWS, L) for k, v in eng.download(2, ("mu", "v")).items()}
        got = {i: eng.calibration(2, n_bins=c[0], levels=c[1], n_nodes=c[2], want_cdf=True) for i, c in enumerate(CONFIGS)}
        again = eng.calibration(2, n_bins=32, levels=LEVELS4, n_nodes=64, want_cdf=True)
        eng.free_units(2)
        both = held.copy()
        both[1, 9, 3] = both[0, 9, 3] = True  # one entry held out twice
        eng.replicate(0, 2, held_out=both)
        with pytest.raises(V.VlgpError, match="status -1.*vlgp_calibration.*overlap.*no cdf"):
            eng.calibration(2, want_cdf=True)
        twice, none = eng.calibration(2)
        assert twice.shape == (2, N, 15) and none is None and np.all(np.isfinite(twice))
        assert np.array_equal(twice[..., -2], both.sum(axis=1))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, got[2]))
    never = ~held.any(axis=0)
    for i, (n_bins, levels, n_nodes) in enumerate(CONFIGS):
        want_cdf, want_sums, terms = CN.score_masked(trials, held, post["mu"], post["v"], *par(params), True, n_nodes,
                                                     n_bins, levels)
        check_margin(want_cdf, n_bins, levels)
        sums, cdf = got[i]
        assert sums.shape == (2, N, n_bins + len(levels) + 3) and cdf.shape == (ROWS, N, 2)
        assert np.array_equal(np.isnan(cdf[..., 0]), never) and np.array_equal(np.isnan(cdf[..., 1]), never)
        errs = (entry_err(cdf, want_cdf), sums_err(sums, want_sums, terms, 1))
        print("measured calibration masked bins %2d levels %d nodes %2d  cdf %.2e  sums %.2e"
              % ((n_bins, len(levels), n_nodes) + errs))
        assert max(errs) <= TOL and counts_equal(sums, want_sums, n_bins)
        assert np.array_equal(sums[..., -2], held.sum(axis=1)) and np.all(sums[..., -1] == 0.0)
        assert np.all(np.abs(sums[..., :n_bins].sum(axis=-1) - sums[..., -2]) <= 1e-12 * sums[..., -2])


def test_skipped_entries_count_and_change_nothing_else(V):
    """y = max_count + 1, y = 2.5 and y = -1 with max_count = 8 on counts that are otherwise at most 8."""
    trials, params, _ = problem()
    pois = ~gauss_of(params)
    for t in trials:
        t["y"][:, pois] = np.minimum(t["y"][:, pois], 8.0)
    planted = copy.deepcopy(trials)
    plants = {(20, 4): 9.0, (160, 4): 2.5, (299, 33): -1.0}  # (row, channel): two in one slot, one in the last workgroup
    for (r, n), val in plants.items():
        planted[0 if r < 150 else 1]["y"][r if r < 150 else r - 150, n] = val
    kw = dict(n_bins=10, levels=(0.5, 0.9), n_nodes=12, max_count=8, want_cdf=True)
    with resident(trials, params) as eng:
        base_sums, base_cdf = eng.calibration(0, **kw)
    with resident(planted, params) as eng:
        t0 = time.perf_counter()
        sums, cdf = eng.calibration(0, **kw)
        took = time.perf_counter() - t0
    assert took < 5.0, took  # (milliseconds: the loop over counts is bounded by max_count)
    assert np.all(base_sums[:, -1] == 0.0) and np.all(base_sums[:, -2] == ROWS)
    hit = np.zeros((ROWS, N), dtype=bool)
    for r, n in plants:
        hit[r, n] = True
    assert np.array_equal(np.isnan(cdf[..., 0]), hit) and np.array_equal(np.isnan(cdf[..., 1]), hit)
    assert cdf[~hit].tobytes() == base_cdf[~hit].tobytes()
    assert np.array_equal(sums[:, -1], hit.sum(axis=0)) and np.array_equal(sums[:, -2], ROWS - hit.sum(axis=0))
    clean = ~hit.any(axis=0)
    assert sums[clean].tobytes() == base_sums[clean].tobytes()
    # the slots that lost entries: the run without the plants less the terms of those entries
    _, _, terms = CN.score_plain(trials, *par(params), True, 12, 10, (0.5, 0.9), max_count=8)
    want = base_sums - np.where(hit[..., None], terms, 0.0).sum(axis=0)
    want[:, -1] = hit.sum(axis=0)
    _, want_planted, terms_planted = CN.score_plain(planted, *par(params), True, 12, 10, (0.5, 0.9), max_count=8)
    assert np.array_equal(want_planted[:, -2:], want[:, -2:])
    err = sums_err(sums[~clean], want[~clean], terms_planted[:, ~clean], 0)
    print("measured calibration skips  sums of the slots that lost entries %.2e" % err)
    assert err <= TOL and counts_equal(sums, want, 10)


def test_same_bits_refusals_and_an_untouched_handle(V):
    trials, params, _ = problem()
    z, lwa = V.evaluation.hermite_nodes(12)
    lev = np.array([0.5, 0.9])
    dp = lambda arr: None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    with resident(trials, params) as eng:
        before = (eng.download(0), eng.get_params())
        one = eng.calibration(0, want_cdf=True)
        two = eng.calibration(0, want_cdf=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
        sums = np.full((N, 15), 7.0)

        def call(n_nodes=12, zz=z, ll=lwa, n_bins=10, n_levels=2, levels=lev, max_count=4096, out=sums):
            return eng.lib.vlgp_calibration(eng.h, 0, 1, n_nodes, dp(zz), dp(ll), n_bins, n_levels, dp(levels), max_count,
                                            None, dp(out))

        refused = [(dict(n_nodes=0), "n_nodes = 0"), (dict(n_nodes=65), "n_nodes = 65"), (dict(n_bins=0), "n_bins = 0"),
                   (dict(n_bins=33), "n_bins = 33"), (dict(n_levels=-1), "n_levels = -1"), (dict(n_levels=5), "n_levels = 5"),
                   (dict(max_count=0), "max_count = 0"), (dict(max_count=65537), "max_count = 65537"),
                   (dict(levels=np.array([0.5, 1.0])), r"levels\[1\] = 1"), (dict(levels=np.array([0.0, 0.5])), r"levels\[0\] = 0"),
                   (dict(levels=np.array([np.nan, 0.5])), r"levels\[0\] = nan"), (dict(levels=None), "needs levels"),
                   (dict(out=None), "needs z, lwa and sums"), (dict(zz=None), "needs z, lwa and sums"),
                   (dict(ll=None), "needs z, lwa and sums")]
        for kw, text in refused:
            rc = call(**kw)
            assert rc == -1, (kw, rc)
            with pytest.raises(V.VlgpError, match="status -1.*vlgp_calibration.*" + text):
                eng.check(rc)
        assert np.all(sums == 7.0)
        assert call(n_levels=0, levels=None, out=np.empty((N, 13))) == 0  # (no levels need no pointer)
        eng.cut(0, 1, np.array([0, 20]), 50)  # two windows that do not tile the set: a copied cut
        with pytest.raises(V.VlgpError, match="status -3.*vlgp_calibration on a copied cut"):
            eng.calibration(1)
        eng.free_units(1)
        after = (eng.download(0), eng.get_params())
        assert all(before[0][k].tobytes() == after[0][k].tobytes() for k in before[0])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before[1], after[1]))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(eng.calibration(0, want_cdf=True), one))


# ---- evaluation.calibration end to end -------------------------------------------------------------------------------
KEYS = ("pit", "pit_all", "coverage", "coverage_all", "dispersion", "dispersion_all")


@functools.lru_cache(maxsize=None)
def _small():
    """Three trials of 60 bins, N = 10 with two Gaussian channels, history 2; a dozen E-step iterations from a zero start
    give the posterior the trials carry."""
    trials, params, config = H.problem(seed=11, M=3, T=60, N=10, L=2, n_gauss=2, history=2, max_iter=12)
    with resident(trials, params, zero_start=True) as eng:
        assert eng.estep(0, 12, config["dmu_bound"], True) == 0
        post = eng.download(0, ("mu", "v"))
    for i, tr in enumerate(trials):
        tr["mu"], tr["v"] = post["mu"][60 * i:60 * (i + 1)].copy(), post["v"][60 * i:60 * (i + 1)].copy()
    return trials, params, config


def same_summary(got, want, n_failed=0):
    assert set(got) == set(want) | {"n_failed"} and got["n_failed"] == n_failed
    assert np.array_equal(got["entries"], want["entries"]) and np.array_equal(got["skipped"], want["skipped"])
    assert np.array_equal(got["levels"], want["levels"])
    err = max(float(np.max(np.abs(np.asarray(got[k]) - np.asarray(want[k])) / np.maximum(1.0, np.abs(want[k])))) for k in KEYS)
    assert err <= TOL, err
    return err


def test_calibration_in_sample(V):
    trials, params, config = copy.deepcopy(_small())
    ev = V.evaluation
    got = ev.calibration(trials, params, config, n_bins=8, levels=(0.5, 0.9, 0.99))
    cdf, sums, _ = CN.score_plain(trials, *par(params), True, 12, 8, (0.5, 0.9, 0.99))
    check_margin(cdf, 8, (0.5, 0.9, 0.99))
    err = same_summary(got, ev.calibration_from_sums(sums, 8, (0.5, 0.9, 0.99)))
    print("measured calibration evaluation in_sample %.2e" % err)
    assert got["pit"].shape == (10, 8) and np.all(got["entries"] == 180)


def test_calibration_of_co_smoothing(V):
    trials, params, config = copy.deepcopy(_small())
    ev = V.evaluation
    groups = ev.channel_folds(10, 2, seed=4)
    got = ev.calibration(trials, params, config, how="channels", n_folds=2, seed=4)
    assert ev.leave_group_out(trials, params, config, n_folds=2, seed=4)["groups"] == groups
    with resident(trials, params, zero_start=True) as eng:
        eng.replicate(0, 2, groups=groups)
        assert eng.estep(2, config["max_iter"], config["dmu_bound"], True) == 0
        post = {k: v.reshape(2, 180, 2) for k, v in eng.download(2, ("mu", "v")).items()}
    cdf, sums, _ = CN.score_groups(trials, groups, post["mu"], post["v"], *par(params), True, 12, 10, (0.5, 0.9))
    check_margin(cdf, 10, (0.5, 0.9))
    per_channel = np.zeros((10, 15))
    per_channel[[c for g in groups for c in g]] = sums
    err = same_summary(got, ev.calibration_from_sums(per_channel, 10, (0.5, 0.9)))
    print("measured calibration evaluation channels %.2e" % err)
    assert np.all(got["entries"] == 180)
    only = ev.calibration(trials, params, config, how="channels", groups=[[1, 4]])
    assert np.array_equal(only["entries"], np.where(np.isin(np.arange(10), [1, 4]), 180, 0)) and np.isnan(only["dispersion"][0])


def test_calibration_of_a_speckled_hold_out(V):
    trials, params, config = copy.deepcopy(_small())
    ev = V.evaluation
    F = ev.entry_folds(180, 10, 2, 6)
    held = np.stack([F == k for k in range(2)])
    got = ev.calibration(trials, params, config, how="entries", n_folds=2, seed=6)
    folds = ev.leave_entries_out(trials, params, config, n_folds=2, seed=6)["folds"]
    assert np.array_equal(np.concatenate(folds), F)
    with resident(trials, params, zero_start=True) as eng:
        eng.replicate(0, 2, held_out=held)
        assert eng.estep(2, config["max_iter"], config["dmu_bound"], True) == 0
        post = {k: v.reshape(2, 180, 2) for k, v in eng.download(2, ("mu", "v")).items()}
    cdf, sums, _ = CN.score_masked(trials, held, post["mu"], post["v"], *par(params), True, 12, 10, (0.5, 0.9))
    check_margin(cdf, 10, (0.5, 0.9))
    err = same_summary(got, ev.calibration_from_sums(sums[0] + sums[1], 10, (0.5, 0.9)))
    print("measured calibration evaluation entries %.2e" % err)
    assert np.all(got["entries"] == 180)


# ---- what the numbers mean ---------------------------------------------------------------------------------------------
def model_draws(seed=31, T=400, n=12, latents=2):
    """Counts drawn from the model itself: a known posterior mu, v > 0 and Poisson draws at rates exp(eta) with
    eta ~ N(m, s2) per entry; two units of T rows, every channel Poisson, no regressors beyond the constant."""
    rng = np.random.default_rng(seed)
    a = 0.5 * rng.standard_normal((latents, n))
    b = np.log(rng.uniform(0.5, 4.0, (1, n)))
    params = {"ydim": n, "zdim": latents, "xdim": 1, "a": a, "b": b, "noise": np.ones(n), "omega": np.full(latents, 1e-2),
              "sigma": np.ones(latents), "rank": 50, "likelihood": np.array(["poisson"] * n)}
    trials = []
    for _ in range(2):
        mu, v = 0.7 * rng.standard_normal((T, latents)), 0.1 + 0.5 * rng.random((T, latents))
        eta = mu @ a + b + np.sqrt(v @ a ** 2) * rng.standard_normal((T, n))
        trials.append({"y": rng.poisson(np.exp(eta)).astype(float), "x": np.ones((T, 1, n)), "mu": mu, "v": v})
    return trials, params


def test_data_drawn_from_the_model_are_calibrated(V):
    """Pooled dispersion within 1 +- 5 / sqrt(entries), the CLT width, for the restatement (a statement about the seed,
    true on the CPU) and for the device, which agree at TOL; the PIT histogram and the coverages within the same width
    of their nominal values."""
    trials, params = model_draws()
    n_entries = 2 * 400 * 12
    width = 5.0 / np.sqrt(n_entries)
    levels = (0.5, 0.9)
    cdf, sums, _ = CN.score_plain(trials, *par(params), True, 12, 10, levels)
    check_margin(cdf, 10, levels)
    want = V.evaluation.calibration_from_sums(sums, 10, levels)
    assert abs(want["dispersion_all"] - 1.0) <= width, want["dispersion_all"]
    got = V.evaluation.calibration(trials, params, {"method": "VB"}, n_bins=10, levels=levels)
    err = same_summary(got, want)
    print("measured calibration model draws: dispersion %.4f (device) %.4f (numpy), width %.4f, pit %s, coverage %s, err %.2e"
          % (got["dispersion_all"], want["dispersion_all"], width, np.round(got["pit_all"], 4), got["coverage_all"], err))
    assert abs(got["dispersion_all"] - 1.0) <= width
    assert np.all(np.abs(got["pit_all"] - 0.1) <= width * np.sqrt(0.1 * 0.9))
    assert np.all(got["coverage_all"] >= np.array(levels) - width)  # (a discrete interval covers at least its level)
    assert got["entries"].sum() == n_entries and got["skipped"].sum() == 0
