"""Speckled hold-out on the device (vlgp_replicate_masked, the by-row mode of the split E-step's row passes, vlgp_loglik
per (replica, channel), evaluation.leave_entries_out, vlgp_amd.impute, cross_validate(score="speckled_bps")).

Two references.  A mask that is constant along the rows IS a channel group: the masked replicas must give the bits of
vlgp_replicate_groups -- posterior, sums and rates -- in every form of the row passes (the 16-lanes-per-row y pass at 4
and 8 channels per lane, the lane-per-row y pass, the residual and curvature passes at channel splits 1 and 4, with and
without x.b, short and long units).  A random speckle is compared with the NumPy restatement (tests/speckled_numpy.py:
the oracle's E-step with res and U multiplied by the observed mask) at heldout_numpy.STAGE, 1e-9, the project's tolerance
for one restated stage.  Every case prints what it measured; profiles/speckled/measured_errors.txt records one run.
"""
import copy
import functools

import numpy as np
import pytest

import heldout_numpy as H
import speckled_numpy as S
from conftest import relerr

pytestmark = pytest.mark.gpu

GROUPS = [[0, 5, 13], [2], [7, 8, 9, 10]]
SPLIT = ("split", "split_mixed")

# name -> (problem keywords, groups, environment switch, expected families, NJ of the y pass, CS of the row passes)
EQUAL_CASES = {
    "mixed": (dict(seed=11, n_gauss=3), GROUPS, None, ("long_split",), 4, 1),
    "short": (dict(seed=11, T=50), GROUPS, "VLGP_ESTEP_SPLIT", SPLIT, 4, 1),
    "long": (dict(seed=11, T=150), GROUPS, "VLGP_ESTEP_LSPLIT", ("long_split",), 4, 1),
    "words-g0": (dict(seed=29, M=3, T=80, N=70, L=2, n_gauss=0), [[63, 64, 69], [0, 1], [31, 32, 33, 65]], None,
                 ("long_split",), 8, 4),
    "words-g6": (dict(seed=29, M=3, T=80, N=70, L=2, n_gauss=6), [[63, 64, 69], [0, 1], [31, 32, 33, 65]], None,
                 ("long_split",), 8, 4),
    "lane-per-row": (dict(seed=31, M=2, T=70, N=130, L=2), [[0, 64, 129], [5], [127, 128, 63]], None, ("long_split",), 0, 4),
    "history": (dict(seed=11, history=2), GROUPS, None, ("long_split",), 4, 1),
}
# the random 5-fold speckles against the restatement
STAGE_CASES = {
    "mixed": dict(seed=11, n_gauss=3),
    "ragged": dict(seed=11, lengths=[150, 120, 150, 120, 150, 120]),
    "short": dict(seed=11, T=50),
    "map": dict(seed=11, method="MAP"),
    "history": dict(seed=11, history=2),
    "words": dict(seed=29, M=3, T=80, N=70, L=2, n_gauss=6),
}


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@functools.lru_cache(maxsize=None)
def _problem(items):
    return H.problem(**dict(items))


def problem(**kw):
    trials, params, config = _problem(tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())))
    return copy.deepcopy(trials), copy.deepcopy(params), dict(config)


def resident(trials, params):
    """An engine holding the trials from a zero start (set 0), the parameters and a prior for every length."""
    from vlgp_amd.api import bind_priors
    from vlgp_amd.engine import Engine

    L = params["zdim"]
    eng = Engine.for_params(params)
    eng.set_params(params["a"], params["b"], params["noise"])
    eng.upload(0, [{"y": t["y"], "x": t.get("x"), "mu": np.zeros((t["y"].shape[0], L)), "v": None, "w": None}
                   for t in trials])
    bind_priors(eng, trials, dict(params))
    return eng


def rows_of(trials):
    return sum(t["y"].shape[0] for t in trials)


def speckle(trials, params, n_folds=5, seed=0):
    from vlgp_amd.evaluation import entry_folds

    F = entry_folds(rows_of(trials), params["ydim"], n_folds, seed)
    return F, np.stack([F == k for k in range(n_folds)])


def cut(F, trials):
    b = np.cumsum([0] + [t["y"].shape[0] for t in trials])
    return [F[b[i]:b[i + 1]] for i in range(len(trials))]


@pytest.mark.parametrize("case", sorted(EQUAL_CASES))
def test_rowwise_constant_masks_equal_group_replicas_bit_for_bit(V, monkeypatch, case):
    kw, groups, switch, families, nj, cs = EQUAL_CASES[case]
    if switch:
        monkeypatch.setenv(switch, "1")
    trials, params, config = problem(**kw)
    rows, N = rows_of(trials), params["ydim"]
    vb = config["method"] == "VB"
    held = np.zeros((len(groups), rows, N), dtype=bool)
    for k, g in enumerate(groups):
        held[k][:, g] = True
    got = {}
    with resident(trials, params) as eng:
        for how, kwargs in (("groups", {"groups": groups}), ("masked", {"held_out": held})):
            eng.replicate(0, 2, **kwargs)
            plan = eng.estep_plan(2, config["max_iter"], vb=vb)
            assert plan["family"] in families and plan["NJ"] == nj and plan["CS"] == cs, plan
            bad = eng.estep(2, config["max_iter"], config["dmu_bound"], vb)
            assert bad == 0 and eng.last_estep_path == plan["family"]
            got[how] = (eng.download(2), eng.loglik(2, vb=vb, want_rate=True))
            eng.free_units(2)
    for key in ("mu", "v", "w", "dmu"):
        assert np.array_equal(got["groups"][0][key], got["masked"][0][key]), key
    (pair_sums, pair_rate), (sums, rate) = got["groups"][1], got["masked"][1]
    assert sums.shape == (len(groups), N, 4) and rate.shape == (rows, N)
    p = 0
    for k, g in enumerate(groups):
        for n in g:
            assert np.array_equal(sums[k, n], pair_sums[p]), (k, n)
            assert np.array_equal(rate[:, n], pair_rate[:, p]), (k, n)
            p += 1
    empty = np.ones((len(groups), N), dtype=bool)
    for k, g in enumerate(groups):
        empty[k, g] = False
    assert np.all(sums[empty] == 0.0)  # an empty (replica, channel) slot: four zeros
    never = ~held.any(axis=0)
    assert np.all(np.isnan(rate[never])) and np.all(np.isfinite(rate[~never]))


@functools.lru_cache(maxsize=None)
def _restated_speckle(case):
    trials, params, config = problem(**STAGE_CASES[case])
    F, held = speckle(trials, params)
    return S.restated(trials, params, config, held)


@pytest.mark.parametrize("case", sorted(STAGE_CASES))
def test_random_speckle_matches_restatement(V, case):
    trials, params, config = problem(**STAGE_CASES[case])
    F, held = speckle(trials, params)
    post, want_rate, want_ll, bad = _restated_speckle(case)
    assert bad == 0
    got = V.evaluation.leave_entries_out(trials, params, config, n_folds=5, seed=0)
    assert got["n_failed"] == 0
    assert all(np.array_equal(f, w) for f, w in zip(got["folds"], cut(F, trials)))
    rate = np.concatenate(got["rate"], axis=0)
    assert rate.shape == want_rate.shape and not np.isnan(rate).any()  # (five folds hold every entry out once)
    errs = (relerr(rate, want_rate), relerr(got["ll_per_fold"], want_ll), relerr(got["ll"], want_ll.sum(axis=0)))
    print("measured speckled %-8s rate %.2e  ll_per_fold %.2e  ll %.2e" % ((case,) + errs))
    assert max(errs) < H.STAGE
    gauss = np.asarray(params["likelihood"]) == "gaussian"
    assert np.array_equal(got["n_entries"], np.full(params["ydim"], rows_of(trials)))
    y = np.concatenate([t["y"] for t in trials])
    assert np.array_equal(got["n_spikes"][~gauss], y.sum(axis=0)[~gauss])  # (counts: exact in any order)
    assert np.all(np.abs(got["n_spikes"] - y.sum(axis=0)) <= 1e-12 * np.abs(y).sum(axis=0))  # (Gaussian: 900 roundings)
    assert np.all(np.isnan(got["bits_per_spike"][gauss])) and np.all(np.isfinite(got["bits_per_spike"][~gauss]))
    want = V.evaluation.co_bits_per_spike(got["ll"], got["ll_null"], got["n_spikes"])
    assert got["speckled_bps"] == want and np.isfinite(want)


def test_edges_empty_replica_blanked_rows_and_a_dead_channel(V):
    trials, params, config = problem(seed=11, n_gauss=3)
    rows, N, L = rows_of(trials), params["ydim"], params["zdim"]
    held = np.zeros((3, rows, N), dtype=bool)
    held[1, 150 + 40:150 + 60] = True           # replica 1: rows 40 ... 59 of trial 1 blanked entirely
    held[2][:, 4] = True                        # replica 2: channel 4 dead on every row
    held[2, 7, 12] = True                       # ... and one Gaussian entry
    post, want_rate, want_ll, bad = S.restated(trials, params, config, held)
    assert bad == 0
    with resident(trials, params) as eng:
        eng.replicate(0, 2, held_out=held)
        assert eng.estep(2, config["max_iter"], config["dmu_bound"], True) == 0
        got = {k: v.reshape(3, rows, L) for k, v in eng.download(2, ("mu", "v", "w")).items()}
        # (replicas 1 and 2 both hold channel 4 of the blanked rows out: the set as a whole gives sums and no rate)
        with pytest.raises(V.VlgpError, match="status -1.*overlap"):
            eng.loglik(2, want_rate=True)
        sums, _ = eng.loglik(2)
        eng.free_units(2)
        rates = {}
        for k in (1, 2):  # the rate of each with the empty replica beside it: no entry is held out twice there
            eng.replicate(0, 2, held_out=held[[0, k]])
            assert eng.estep(2, config["max_iter"], config["dmu_bound"], True) == 0
            two, rates[k] = eng.loglik(2, want_rate=True)
            assert np.array_equal(two, sums[[0, k]])
            eng.free_units(2)
    gauss = np.asarray(params["likelihood"]) == "gaussian"
    y, x = (np.concatenate([t[key] for t in trials]) for key in ("y", "x"))
    for k, rate in rates.items():
        want = H.rate_ll(y, x, post["mu"][k], post["v"][k], params["a"], params["b"], params["noise"], gauss, True)[0]
        assert np.array_equal(np.isnan(rate), ~held[k])  # (NaN where no replica holds the entry out)
        assert relerr(rate[held[k]], want[held[k]]) < H.STAGE
    for key in ("mu", "v", "w"):
        assert relerr(got[key], post[key]) < H.STAGE, key  # (replica 0, the empty mask: the plain E-step)
        assert np.all(np.isfinite(got[key]))
    blank = slice(150 + 40, 150 + 60)
    assert np.all(got["w"][1, blank] == 0.0)
    assert np.all(got["v"][1, blank] > 0.0) and np.all(got["v"][1, blank] <= 1.0)  # (sigma = 1: the prior variance at most)
    assert np.all(sums[0] == 0.0)
    assert relerr(sums[:, :, 0], want_ll) < H.STAGE
    used = np.zeros((3, N), dtype=bool)
    used[1] = True
    used[2, [4, 12]] = True
    assert np.all(sums[~used] == 0.0) and np.all(sums[used][:, 0] != 0.0)


@pytest.mark.parametrize("kw", [dict(seed=13, n_gauss=2), dict(seed=13, T=50, n_gauss=2)], ids=["long", "short"])
def test_chunks_and_repeats_give_the_same_bits(V, kw):
    trials, params, config = problem(**kw)
    ev = V.evaluation

    def same(x, z):
        return (all(np.array_equal(x[k], z[k], equal_nan=True) for k in ("ll", "ll_per_fold", "n_spikes", "bits_per_spike"))
                and x["speckled_bps"] == z["speckled_bps"] and all(np.array_equal(g, w) for g, w in zip(x["rate"], z["rate"])))

    base = ev.leave_entries_out(trials, params, config, n_folds=3, seed=5)
    for cap in (1, 2):
        assert same(ev.leave_entries_out(trials, params, config, n_folds=3, seed=5, max_replicas=cap), base), cap
    assert same(ev.leave_entries_out(trials, params, config, n_folds=3, seed=5), base)


def test_refusals_leave_a_working_handle(V):
    from vlgp_amd.engine import pack_mask
    import ctypes as C

    trials, params, config = problem(seed=23, M=4, T=100, N=10)
    rows, N = rows_of(trials), 10
    F, held = speckle(trials, params, n_folds=2)
    with resident(trials, params) as eng:
        words = pack_mask(held)
        words[1, 37, 0] |= np.uint64(1) << np.uint64(N)  # a bit at position N
        rc = eng.lib.vlgp_replicate_masked(eng.h, 0, 2, 2, words.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert rc == -1
        with pytest.raises(V.VlgpError, match=r"status -1.*replica 1.*row 37"):
            eng.check(rc)
        assert 2 not in eng.sets
        with pytest.raises(V.VlgpError, match="status -1"):
            eng.replicate(0, 2, held_out=held[:0])  # n_rep < 1
        both = held.copy()  # (which sets the replicate calls and the other entry points take: test_gpu_set_kinds.py)
        both[1, 3, 4] = both[0, 3, 4] = True  # one entry held out twice
        eng.replicate(0, 2, held_out=both)
        with pytest.raises(V.VlgpError, match="status -1.*overlap"):
            eng.loglik(2, want_rate=True)
        sums, _ = eng.loglik(2)  # (the sums alone are fine)
        assert sums.shape == (2, N, 4)
        eng.free_units(2)
        # ... and the handle still works
        eng.replicate(0, 2, held_out=held)
        assert eng.estep(2, 2) == 0
        sums, rate = eng.loglik(2, want_rate=True)
        assert np.all(np.isfinite(sums)) and not np.isnan(rate).any()
        with pytest.raises(ValueError):
            eng.replicate(0, 3, held_out=held.astype(int))
        with pytest.raises(ValueError):
            eng.replicate(0, 3, held_out=held, groups=[[1]])
        eng.free_units(2)
        eng.free_units(0)


def test_many_latents_are_refused_with_the_devices_reason(V):
    trials, params, config = problem(seed=19, M=3, T=80, N=8, L=12, max_iter=3)
    with pytest.raises(V.VlgpError, match=r"status -3.*split E-step.*L > 10"):
        V.evaluation.leave_entries_out(trials, params, config, n_folds=2)


def test_impute_is_the_one_fold_of_leave_entries_out(V):
    trials, params, config = problem(seed=11, n_gauss=3)
    rows, L = rows_of(trials), params["zdim"]
    missing = np.random.default_rng(4).random((rows, params["ydim"])) < 0.15
    missing[200:230, 3] = True     # a channel dead for part of a trial
    missing[400:404] = True        # four blanked bins
    got = V.impute(trials, params, config, cut(missing, trials))
    one = V.evaluation.leave_entries_out(trials, params, config, folds=cut(np.where(missing, 0, -1), trials))
    assert got["n_failed"] == one["n_failed"] == 0
    for g, w, m in zip(got["rate"], one["rate"], cut(missing, trials)):
        assert np.array_equal(g, w, equal_nan=True) and np.array_equal(np.isnan(g), ~m)
    assert np.array_equal(one["n_entries"], missing.sum(axis=0))
    with resident(trials, params) as eng:
        eng.replicate(0, 2, held_out=missing[None])
        eng.estep(2, config["max_iter"], config["dmu_bound"], True)
        post = eng.download(2, ("mu", "v", "w"))
    for key in ("mu", "v", "w"):
        assert np.array_equal(np.concatenate(got[key]), post[key]), key
        assert [g.shape for g in got[key]] == [(t["y"].shape[0], L) for t in trials]


def test_cross_validate_speckled_end_to_end(V):
    from vlgp_amd import synth

    trials = synth.make_trials(8, 100, 12, 2, seed=41)
    before = copy.deepcopy(trials)
    kw = dict(n_trial_folds=2, n_channel_folds=3, max_iter=3, min_iter=3, score="speckled_bps")
    cv = V.model_selection.cross_validate(trials, [1, 2], **kw)
    assert cv["errors"] == [] and cv["score"] == "speckled_bps" and cv["n_factors"] == [1, 2]
    assert cv["speckled_bps"].shape == (2, 2) and np.all(np.isfinite(cv["speckled_bps"]))
    assert cv["bits_per_spike"].shape == (2, 2, 12) and cv["n_failed"].shape == (2, 2)
    assert np.array_equal(cv["mean_speckled_bps"], cv["speckled_bps"].mean(axis=1))
    m = cv["mean_speckled_bps"]
    assert cv["best"] == (1 if m[0] >= m[1] else 2)
    again = V.model_selection.cross_validate(trials, [1, 2], **kw)
    for key in ("speckled_bps", "bits_per_spike", "mean_speckled_bps", "n_failed"):
        assert np.array_equal(again[key], cv[key], equal_nan=True), key
    for tr, old in zip(trials, before):
        assert sorted(tr) == sorted(old) and all(np.asarray(tr[k]).tobytes() == np.asarray(old[k]).tobytes() for k in old)
