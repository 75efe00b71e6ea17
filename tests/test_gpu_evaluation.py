"""Held-out evaluation on the device (vlgp_loglik, singleton replicas, vlgp_amd.evaluation) against a NumPy
restatement: the oracle's E-step with a[:, n] = 0 from a zero start, then channel n's plug-in rate with its own
loading, scored with the definitions of vlgp_amd/evaluation.py."""
import numpy as np
import pytest

from conftest import relerr
from heldout_numpy import STAGE, problem, rate_ll, restated
from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.mark.parametrize("case", ["poisson", "mixed", "history"])
def test_loglik_matches_restatement(V, case):
    kw = {"poisson": {}, "mixed": {"n_gauss": 3}, "history": {"history": 2}}[case]
    trials, params, config = problem(seed=5, **kw)
    rng = np.random.default_rng(1)
    L, N = params["zdim"], params["ydim"]
    for tr in trials:
        T = tr["y"].shape[0]
        tr["mu"] = 0.3 * rng.standard_normal((T, L))
        tr["v"] = 0.1 * rng.random((T, L))
    gauss = np.asarray(params["likelihood"]) == "gaussian"
    per = V.evaluation.loglik({"trials": trials, "params": params, "config": config}, per_channel=True)
    want = np.zeros(N)
    rates = []
    for tr in trials:
        r, ll = rate_ll(tr["y"], tr["x"], tr["mu"], tr["v"], params["a"], params["b"], params["noise"], gauss, True)
        want += ll.sum(0)
        rates.append(r)
    assert relerr(per, want) < 1e-12
    total = V.evaluation.loglik({"trials": trials, "params": params, "config": config})
    assert total == pytest.approx(want.sum(), rel=1e-12)
    # the rates themselves, through the engine
    from vlgp_amd.engine import Engine

    with Engine(N, L, params["xdim"], 50, gauss) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, [{"y": t["y"], "x": t["x"], "mu": t["mu"], "v": t["v"], "w": None} for t in trials])
        sums, rate = eng.loglik(0, vb=True, want_rate=True)
    assert relerr(rate, np.concatenate(rates)) < 1e-12
    assert np.array_equal(sums[:, 0], per)


@pytest.mark.parametrize("case", ["mixed", "ragged", "short", "map", "subset"])
def test_leave_one_out_matches_restatement(V, case):
    kw, channels = {}, None
    if case == "mixed":
        kw = {"n_gauss": 3}
    elif case == "ragged":
        kw = {"lengths": [150, 120, 150, 120, 150, 120]}
    elif case == "short":
        kw = {"T": 50}
    elif case == "map":
        kw = {"method": "MAP"}
    elif case == "subset":
        channels = [9, 2, 13]
    trials, params, config = problem(seed=11, **kw)
    got = V.evaluation.leave_one_out(trials, params, config, channels=channels)
    chans = list(range(params["ydim"])) if channels is None else channels
    assert got["channels"] == chans and got["path"] == "batched" and got["n_failed"] == 0
    want_rate, want_ll = restated(trials, params, config, [[c] for c in chans])
    for g, w in zip(got["rate"], want_rate):
        assert g.shape == w.shape
        assert relerr(g, w) < STAGE
    assert relerr(got["ll"], want_ll) < STAGE
    gauss = (np.asarray(params["likelihood"]) == "gaussian")[chans]
    assert np.all(np.isnan(got["bits_per_spike"][gauss]))
    assert np.all(np.isfinite(got["bits_per_spike"][~gauss]))


@pytest.mark.parametrize("shape", ["long", "short"])
def test_batched_equals_sequential_bit_for_bit(V, monkeypatch, shape):
    if shape == "long":
        monkeypatch.setenv("VLGP_ESTEP_LSPLIT", "1")
        trials, params, config = problem(seed=13, n_gauss=2)
    else:
        monkeypatch.setenv("VLGP_ESTEP_SPLIT", "1")
        trials, params, config = problem(seed=13, T=50, n_gauss=2)
    ev = V.evaluation
    base = ev.leave_one_out(trials, params, config, path="batched")
    seq = ev.leave_one_out(trials, params, config, path="sequential")
    assert base["path"] == "batched" and seq["path"] == "sequential"
    for key in ("ll", "n_spikes"):
        assert np.array_equal(base[key], seq[key]), key
    assert all(np.array_equal(g, w) for g, w in zip(base["rate"], seq["rate"]))
    for cap in (1, 3):
        other = ev.leave_one_out(trials, params, config, path="batched", max_replicas=cap)
        assert np.array_equal(other["ll"], base["ll"])
        assert all(np.array_equal(g, w) for g, w in zip(other["rate"], base["rate"]))
    again = ev.leave_one_out(trials, params, config, path="batched")
    assert np.array_equal(again["ll"], base["ll"])
    assert all(np.array_equal(g, w) for g, w in zip(again["rate"], base["rate"]))


def test_zero_loading_channel_reproduces_transform_from_zero(V):
    trials, params, config = problem(seed=17)
    n = 4
    params["a"][:, n] = 0.0
    got = V.evaluation.leave_one_out(trials, params, config, channels=[n, 7])
    gauss = np.asarray(params["likelihood"]) == "gaussian"
    for tr, g in zip(trials, got["rate"]):
        T = tr["y"].shape[0]
        G = O.build_prior([T], params["omega"], params["sigma"], 50)[T]
        z = np.zeros((T, params["zdim"]))
        mu, v, _, _, _ = O.estep_unit(tr["y"], tr["x"], z, z, z, params["a"], params["b"], params["noise"], gauss, G,
                                      config["max_iter"], config["dmu_bound"], True)
        r, _ = rate_ll(tr["y"], tr["x"], mu, v, params["a"], params["b"], params["noise"], gauss, True)
        assert relerr(g[:, 0], r[:, n]) < STAGE


def test_many_latents_take_the_sequential_path(V):
    trials, params, config = problem(seed=19, M=3, T=80, N=8, L=12, max_iter=3)
    got = V.evaluation.leave_one_out(trials, params, config, channels=[0, 5])
    assert got["path"] == "sequential"
    want_rate, want_ll = restated(trials, params, config, [[0], [5]])
    for g, w in zip(got["rate"], want_rate):
        assert relerr(g, w) < STAGE
    assert relerr(got["ll"], want_ll) < STAGE
    with pytest.raises(V.VlgpError):
        V.evaluation.leave_one_out(trials, params, config, channels=[0], path="batched")
