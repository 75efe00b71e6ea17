"""The three row scores (vlgp_loglik, vlgp_predictive, vlgp_calibration) walk a set's entries the same way (csrc/row_walk.h):
masks that are constant along the rows are leave-group-out, bit for bit, in every one of them.

N = 65 puts the last channel -- the Gaussian one -- alone in the second mask word; the singleton groups [[0], [63], [64]]
are held out once as group replicas and once as a masked set with those columns set on every row.  Rows in all: 1 (a
single lane), 256 (exactly one full workgroup) and 257 (one more lane in a second workgroup), the leading rows of the
two trials of one seeded problem.  Calibration has W = 6 columns, two groups of four with the second half empty.  Both
sides are the device's: everything is compared for equal bits, there is no tolerance.
"""
import functools

import numpy as np
import pytest

import heldout_numpy as H

pytestmark = pytest.mark.gpu

N, L, RANK = 65, 2, 8
GROUPS = [[0], [63], [64]]
LENGTHS = {1: [1], 256: [128, 128], 257: [128, 129]}  # the leading rows of the problem's trials (128 and 129 rows)
N_BINS, LEVELS, N_NODES = 2, (0.9,), 12


@functools.lru_cache(maxsize=None)
def _problem():
    trials, params, config = H.problem(seed=37, M=2, T=129, N=N, L=L, n_gauss=1, lengths=LENGTHS[257])
    params["rank"] = RANK
    return trials, params, config


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def scores(eng, set_id):
    ll, rate = eng.loglik(set_id, want_rate=True)
    pred, prate, lpd = eng.predictive(set_id, n_nodes=N_NODES, want_rate=True, want_lpd=True)
    cal, cdf = eng.calibration(set_id, n_bins=N_BINS, levels=LEVELS, n_nodes=N_NODES, want_cdf=True)
    return {"loglik": ll, "predictive": pred, "calibration": cal}, {"rate": rate, "pred_rate": prate, "lpd": lpd, "cdf": cdf}


@pytest.mark.parametrize("rows", sorted(LENGTHS))
def test_rowwise_constant_masks_score_as_group_replicas_bit_for_bit(rows):
    from vlgp_amd.api import bind_priors
    from vlgp_amd.engine import Engine

    whole, params, config = _problem()
    trials = [{"y": tr["y"][:T].copy(), "x": tr["x"][:T].copy()} for tr, T in zip(whole, LENGTHS[rows])]
    assert sum(t["y"].shape[0] for t in trials) == rows and params["likelihood"][64] == "gaussian"
    held = np.zeros((len(GROUPS), rows, N), dtype=bool)
    for k, g in enumerate(GROUPS):
        held[k][:, g] = True
    got = {}
    with Engine.for_params(params) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, [{"y": t["y"], "x": t.get("x"), "mu": np.zeros((t["y"].shape[0], L)), "v": None, "w": None}
                       for t in trials])
        bind_priors(eng, trials, dict(params))
        for how, kwargs in (("groups", {"groups": GROUPS}), ("masked", {"held_out": held})):
            eng.replicate(0, 2, **kwargs)
            assert eng.estep(2, 2, config["dmu_bound"], True) == 0
            got[how] = (eng.download(2, ("mu", "v", "w")),) + scores(eng, 2)
            eng.free_units(2)
    for key in ("mu", "v", "w"):  # (the two E-steps: test_gpu_speckled holds them equal at other shapes)
        assert same_bits(got["groups"][0][key], got["masked"][0][key]), ("E-step", key)
    (_, pair_sums, pair_entry), (_, sums, entry) = got["groups"], got["masked"]
    W = N_BINS + len(LEVELS) + 3
    for name, width in (("loglik", 4), ("predictive", 4), ("calibration", W)):
        assert pair_sums[name].shape == (len(GROUPS), width) and sums[name].shape == (len(GROUPS), N, width), name
        for p, (n,) in enumerate(GROUPS):
            assert same_bits(sums[name][p, n], pair_sums[name][p]), (name, p, n)
        assert same_bits(sums[name][~held.any(axis=1)], np.zeros((len(GROUPS) * (N - 1), width))), name  # (empty slots)
    assert np.all(pair_sums["calibration"][:, -2] == rows) and np.all(pair_sums["calibration"][:, -1] == 0.0)
    never = ~held.any(axis=0)
    for name, tail in (("rate", ()), ("pred_rate", ()), ("lpd", ()), ("cdf", (2,))):
        assert pair_entry[name].shape == (rows, len(GROUPS)) + tail and entry[name].shape == (rows, N) + tail, name
        for p, (n,) in enumerate(GROUPS):
            assert same_bits(entry[name][:, n], pair_entry[name][:, p]), (name, p, n)
        assert not np.isnan(pair_entry[name]).any() and np.all(np.isnan(entry[name][never])), name
