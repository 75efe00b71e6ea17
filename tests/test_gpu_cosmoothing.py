"""Leave-group-out replicas on the device (vlgp_replicate_groups, vlgp_loglik per pair, evaluation.leave_group_out,
model_selection.cross_validate) against a NumPy restatement: the oracle's E-step with the group's loadings zeroed from a
zero start, then every channel of the group predicted with its own loading (definitions: vlgp_amd/evaluation.py)."""
import copy

import numpy as np
import pytest
from scipy.special import gammaln

from conftest import relerr
from heldout_numpy import STAGE, problem, rate_ll, restated

pytestmark = pytest.mark.gpu

GROUPS = [[0, 5, 13], [2], [7, 8, 9, 10]]


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _assert_matches_restatement(got, trials, params, config, groups, path="batched"):
    chans = [c for g in groups for c in g]
    assert got["groups"] == groups and got["channels"] == chans
    assert got["group_of"] == [k for k, g in enumerate(groups) for _ in g]
    assert got["path"] == path and got["n_failed"] == 0
    want_rate, want_ll = restated(trials, params, config, groups)
    for g, w in zip(got["rate"], want_rate):
        assert g.shape == w.shape
        assert relerr(g, w) < STAGE
    assert relerr(got["ll"], want_ll) < STAGE
    gauss = (np.asarray(params["likelihood"]) == "gaussian")[chans]
    assert np.all(np.isnan(got["bits_per_spike"][gauss]))
    assert np.all(np.isfinite(got["bits_per_spike"][~gauss]))
    use = ~gauss & (got["n_spikes"] > 0)
    want = (got["ll"][use].sum() - got["ll_null"][use].sum()) / (got["n_spikes"][use].sum() * np.log(2.0))
    assert got["co_bps"] == pytest.approx(want, rel=1e-14)


@pytest.mark.parametrize("case", ["mixed", "ragged", "short", "map"])
def test_leave_group_out_matches_restatement(V, case):
    # (900 rows: no multiple of 64, so waves of the row passes straddle two replicas)
    kw = {"mixed": {"n_gauss": 3}, "ragged": {"lengths": [150, 120, 150, 120, 150, 120]}, "short": {"T": 50},
          "map": {"method": "MAP"}}[case]
    trials, params, config = problem(seed=11, **kw)
    got = V.evaluation.leave_group_out(trials, params, config, groups=GROUPS)
    _assert_matches_restatement(got, trials, params, config, GROUPS)


def test_group_of_several_gaussian_channels(V):
    # (the Gaussian channels are 11, 12, 13: the per-replica constant of w skips two terms of its chain for group 0)
    groups = [[11, 13, 4], [12], [0, 1]]
    trials, params, config = problem(seed=11, n_gauss=3)
    got = V.evaluation.leave_group_out(trials, params, config, groups=groups)
    _assert_matches_restatement(got, trials, params, config, groups)


@pytest.mark.parametrize("n_gauss", [0, 6])
def test_groups_on_both_sides_of_a_mask_word(V, n_gauss):
    # (n_gauss = 6: channels 64 ... 69 are Gaussian, so the constant of w reads the second mask word too)
    groups = [[63, 64, 69], [0, 1], [31, 32, 33, 65]]
    trials, params, config = problem(seed=29, M=3, T=80, N=70, L=2, n_gauss=n_gauss)
    got = V.evaluation.leave_group_out(trials, params, config, groups=groups)
    _assert_matches_restatement(got, trials, params, config, groups)


@pytest.mark.parametrize("shape", ["long", "short"])
def test_batched_equals_sequential_bit_for_bit(V, monkeypatch, shape):
    if shape == "long":
        monkeypatch.setenv("VLGP_ESTEP_LSPLIT", "1")
        trials, params, config = problem(seed=13, n_gauss=2)
    else:
        monkeypatch.setenv("VLGP_ESTEP_SPLIT", "1")
        trials, params, config = problem(seed=13, T=50, n_gauss=2)
    ev = V.evaluation

    def same(x, z):
        return (np.array_equal(x["ll"], z["ll"]) and np.array_equal(x["n_spikes"], z["n_spikes"])
                and all(np.array_equal(g, w) for g, w in zip(x["rate"], z["rate"])))

    base = ev.leave_group_out(trials, params, config, groups=GROUPS, path="batched")
    seq = ev.leave_group_out(trials, params, config, groups=GROUPS, path="sequential")
    assert base["path"] == "batched" and seq["path"] == "sequential"
    assert same(base, seq)
    for cap in (1, 2):
        assert same(ev.leave_group_out(trials, params, config, groups=GROUPS, path="batched", max_replicas=cap), base)
    assert same(ev.leave_group_out(trials, params, config, groups=GROUPS, path="batched"), base)


@pytest.mark.parametrize("channels", [None, [9, 2, 13]])
def test_singleton_groups_equal_leave_one_out(V, channels):
    trials, params, config = problem(seed=11, n_gauss=3)
    chans = list(range(params["ydim"])) if channels is None else channels
    one = V.evaluation.leave_one_out(trials, params, config, channels=channels)
    grp = V.evaluation.leave_group_out(trials, params, config, groups=[[c] for c in chans])
    assert grp["channels"] == one["channels"] == chans and grp["path"] == one["path"] == "batched"
    for key in ("ll", "n_spikes"):
        assert np.array_equal(grp[key], one[key]), key
    assert all(np.array_equal(g, w) for g, w in zip(grp["rate"], one["rate"]))


def test_engine_scores_pairs_in_channel_list_order(V):
    from vlgp_amd.api import bind_priors
    from vlgp_amd.engine import Engine

    trials, params, config = problem(seed=31, M=4, T=100, N=10, n_gauss=2)
    L, N = params["zdim"], params["ydim"]
    gauss = np.asarray(params["likelihood"]) == "gaussian"
    groups = [[8, 1], [4], [9, 0, 3]]  # (unsorted on purpose: the slots follow the list, not the channel numbers)
    chans = [c for g in groups for c in g]
    units = [{"y": t["y"], "x": None, "mu": np.zeros((t["y"].shape[0], L)), "v": None, "w": None} for t in trials]
    rows = sum(t["y"].shape[0] for t in trials)
    with Engine(N, L, 1, 50, gauss) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, units)
        bind_priors(eng, trials, dict(params))
        eng.replicate(0, 2, groups=groups)
        eng.estep(2, 3)
        post = eng.download(2, ("mu", "v"))
        sums, rate = eng.loglik(2, want_rate=True)
    assert post["mu"].shape == (len(groups) * rows, L)
    assert sums.shape == (len(chans), 4) and rate.shape == (rows, len(chans))
    y = np.concatenate([t["y"] for t in trials])
    x = np.ones((rows, 1, N))
    p = 0
    for k, g in enumerate(groups):
        mu, v = post["mu"][k * rows:(k + 1) * rows], post["v"][k * rows:(k + 1) * rows]
        r, ll = rate_ll(y, x, mu, v, params["a"], params["b"], params["noise"], gauss, True)
        for n in g:
            assert relerr(rate[:, p], r[:, n]) < 1e-12
            third = r[:, n].sum()
            fourth = (y[:, n] ** 2).sum() if gauss[n] else gammaln(y[:, n] + 1.0).sum()
            assert relerr(sums[p], [ll[:, n].sum(), y[:, n].sum(), third, fourth]) < 1e-12
            p += 1


def test_replicate_channels_are_singleton_groups(V):
    from vlgp_amd.api import bind_priors
    from vlgp_amd.engine import Engine

    trials, params, config = problem(seed=23, M=4, T=100, N=10)
    L, N = params["zdim"], params["ydim"]
    units = [{"y": t["y"], "x": None, "mu": np.zeros((t["y"].shape[0], L)), "v": None, "w": None} for t in trials]
    got = []
    with Engine(N, L, 1, 50) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, units)
        bind_priors(eng, trials, dict(params))
        for args, kw in (([1, 3, 5],), {}), ((), {"groups": [[1], [3], [5]]}):
            eng.replicate(0, 2, *args, **kw)
            eng.estep(2, 2)
            mu = eng.download(2, ("mu",))["mu"]
            sums, rate = eng.loglik(2, want_rate=True)
            got.append((mu, sums, rate))
            eng.free_units(2)
    assert got[0][0].shape == (3 * 400, L) and got[0][1].shape == (3, 4) and got[0][2].shape == (400, 3)
    for one, grp in zip(*got):
        assert np.array_equal(one, grp)


def test_bad_groups_are_refused_and_the_handle_lives_on(V):
    from vlgp_amd.api import bind_priors
    from vlgp_amd.engine import Engine

    trials, params, config = problem(seed=23, M=4, T=100, N=10)
    L, N = params["zdim"], params["ydim"]
    units = [{"y": t["y"], "x": None, "mu": np.zeros((t["y"].shape[0], L)), "v": None, "w": None} for t in trials]
    with Engine(N, L, 1, 50) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, units)
        bind_priors(eng, trials, dict(params))
        for bad, what in (([[1, 2], [], [3]], "replica 1"), ([[1], [4, 2, 4]], "replica 1"), ([[0, N]], "replica 0")):
            with pytest.raises(V.VlgpError, match=r"status -1.*" + what):
                eng.replicate(0, 2, groups=bad)
        eng.replicate(0, 2, groups=[[1, 3], [5]])
        eng.estep(2, 2)
        sums, rate = eng.loglik(2, want_rate=True)
        assert sums.shape == (3, 4) and rate.shape == (400, 3) and np.all(np.isfinite(sums))
        eng.free_units(2)
        eng.free_units(0)
    with pytest.raises(ValueError):
        V.evaluation.leave_group_out(trials, params, config, groups=[[0, 1], [1, 2]])
    with pytest.raises(ValueError):
        V.evaluation.leave_group_out(trials, params, config, groups=[list(range(N))])


def test_many_latents_take_the_sequential_path(V):
    trials, params, config = problem(seed=19, M=3, T=80, N=8, L=12, max_iter=3)
    groups = [[0, 5], [3]]
    got = V.evaluation.leave_group_out(trials, params, config, groups=groups)
    _assert_matches_restatement(got, trials, params, config, groups, path="sequential")


def test_cross_validate_end_to_end(V):
    from vlgp_amd import synth

    trials = synth.make_trials(8, 100, 12, 2, seed=41)
    before = copy.deepcopy(trials)
    kw = dict(n_trial_folds=2, n_channel_folds=3, max_iter=3, min_iter=3)
    cv = V.model_selection.cross_validate(trials, [1, 2], **kw)
    assert set(cv) >= {"n_factors", "trial_folds", "channel_folds", "co_bps", "bits_per_spike", "n_failed",
                       "mean_co_bps", "best", "errors"}
    assert cv["n_factors"] == [1, 2] and cv["errors"] == []
    assert cv["co_bps"].shape == (2, 2) and cv["bits_per_spike"].shape == (2, 2, 12)
    assert np.asarray(cv["mean_co_bps"]).shape == (2,) and np.all(np.isfinite(cv["co_bps"]))
    assert sorted(i for f in cv["trial_folds"] for i in f) == list(range(8)) and len(cv["trial_folds"]) == 2
    assert cv["channel_folds"] == V.evaluation.channel_folds(12, 3, 0)
    # every score again by hand, on the returned folds
    for f, test_idx in enumerate(cv["trial_folds"]):
        train = [{"y": trials[i]["y"].copy()} for i in range(8) if i not in test_idx]
        test = [{"y": trials[i]["y"].copy()} for i in test_idx]
        for c, n in enumerate(cv["n_factors"]):
            np.random.seed(0)  # (cross_validate seeds every fit with its `seed`: fit's start draws a subsample)
            fitted = V.fit(train_copy(train), n, verbose=False, max_iter=3, min_iter=3)
            got = V.evaluation.leave_group_out(test, fitted["params"], fitted["config"], groups=cv["channel_folds"])
            assert np.array_equal(cv["co_bps"][c, f], got["co_bps"]), (c, f)
            assert np.array_equal(cv["bits_per_spike"][c, f][got["channels"]], got["bits_per_spike"], equal_nan=True)
    # the argmax rule: largest mean, the smaller n_factors on a tie (which candidate that is, the data decide)
    assert np.array_equal(cv["mean_co_bps"], cv["co_bps"].mean(axis=1))
    m = cv["mean_co_bps"]
    assert cv["best"] == (1 if m[0] >= m[1] else 2)
    again = V.model_selection.cross_validate(trials, [1, 2], **kw)
    for key in ("co_bps", "bits_per_spike", "mean_co_bps", "n_failed"):
        assert np.array_equal(again[key], cv[key], equal_nan=True), key
    assert again["best"] == cv["best"] and again["trial_folds"] == cv["trial_folds"]
    # the caller's trials: the same bytes, no new keys
    assert len(trials) == len(before)
    for tr, old in zip(trials, before):
        assert sorted(tr) == sorted(old)
        for key in old:
            assert np.asarray(tr[key]).tobytes() == np.asarray(old[key]).tobytes()


def train_copy(train):
    return [{"y": tr["y"].copy()} for tr in train]
