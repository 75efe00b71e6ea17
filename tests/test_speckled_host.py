"""Speckled hold-out, host side: the NumPy restatement against the leave-group-out one, entry folds, the packing of the
mask words, the score arithmetic from hand-made sums, the C ABI (vlgp_replicate_masked declared in the held-out block,
bound, ABI 3) and the score argument of cross_validate."""
import math
import os
import re

import numpy as np
import pytest
from scipy.special import gammaln

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vlgp_hip.h")


def test_rowwise_constant_masks_restate_leave_group_out():
    import heldout_numpy as H
    import speckled_numpy as S

    groups = [[0, 5, 13], [2], [7, 8, 9, 10]]
    trials, params, config = H.problem(seed=11, n_gauss=3, M=2)
    rows = sum(t["y"].shape[0] for t in trials)
    held = np.zeros((len(groups), rows, params["ydim"]), dtype=bool)
    for k, g in enumerate(groups):
        held[k][:, g] = True
    want_rate, want_ll = H.restated(trials, params, config, groups)
    post, rate, ll, bad = S.restated(trials, params, config, held)
    assert bad == 0
    want_rate = np.concatenate(want_rate, axis=0)
    p = 0
    for k, g in enumerate(groups):
        for n in g:
            err_r = np.abs(rate[:, n] - want_rate[:, p]).max() / np.abs(want_rate[:, p]).max()
            err_l = abs(ll[k, n] - want_ll[p]) / abs(want_ll[p])
            assert err_r <= 1e-12 and err_l <= 1e-12, (k, n, err_r, err_l)
            p += 1
    never = ~held.any(axis=0)
    assert np.all(np.isnan(rate[never])) and np.all(np.isfinite(rate[~never]))
    assert np.all(ll[~held.any(axis=1)] == 0.0)


@pytest.mark.parametrize("rows, n_ch, n_folds", [(30, 14, 5), (7, 3, 4), (1, 5, 5), (900, 14, 5), (13, 70, 3), (4, 4, 1)])
def test_entry_folds_are_the_stated_construction(rows, n_ch, n_folds):
    from vlgp_amd.evaluation import entry_folds

    f = entry_folds(rows, n_ch, n_folds, seed=3)
    assert f.shape == (rows, n_ch) and np.issubdtype(f.dtype, np.integer)
    assert np.array_equal(f, np.random.default_rng(3).permutation(rows * n_ch).reshape(rows, n_ch) % n_folds)
    sizes = np.bincount(f.ravel(), minlength=n_folds)
    assert len(sizes) == n_folds and sizes.max() - sizes.min() <= 1 and sizes.min() >= 1


def test_entry_folds_are_a_function_of_their_arguments():
    from vlgp_amd.evaluation import entry_folds

    assert np.array_equal(entry_folds(40, 6, 5, seed=7), entry_folds(40, 6, 5, seed=7))
    assert np.array_equal(entry_folds(40, 6, 5), entry_folds(40, 6, 5, seed=0))
    assert not np.array_equal(entry_folds(40, 6, 5, seed=7), entry_folds(40, 6, 5, seed=8))


@pytest.mark.parametrize("rows, n_ch, n_folds", [(5, 2, 0), (5, 2, 11), (5, 2, -1), (0, 3, 1), (3, 0, 1)])
def test_entry_folds_refuse_impossible_counts(rows, n_ch, n_folds):
    from vlgp_amd.evaluation import entry_folds

    with pytest.raises(ValueError):
        entry_folds(rows, n_ch, n_folds)


@pytest.mark.parametrize("N", [14, 64, 65, 130])
def test_mask_words_round_trip(N):
    from vlgp_amd.engine import pack_mask, unpack_mask

    mask = np.random.default_rng(N).random((3, 11, N)) < 0.3
    mask[0, 0] = True   # a row with every bit set, the last channel included
    mask[1, 1] = False
    words = pack_mask(mask)
    nw = (N + 63) // 64
    assert words.shape == (3, 11, nw) and words.dtype == np.uint64 and words.flags["C_CONTIGUOUS"]
    for k, r in ((0, 0), (1, 1), (2, 7)):
        for n in range(N):  # the layout the header states: bit n & 63 of word n >> 6
            assert ((int(words[k, r, n >> 6]) >> (n & 63)) & 1) == int(mask[k, r, n])
        assert int(words[k, r, nw - 1]) >> ((N - 1) % 64 + 1) == 0  # nothing at a position >= N
    assert np.array_equal(unpack_mask(words, N), mask)


def test_scores_from_hand_made_sums():
    from vlgp_amd.evaluation import co_bits_per_spike, entry_scores

    # channels: 0 Poisson, spikes in both folds; 1 Poisson, no held-out spike; 2 Gaussian; 3 Poisson, held out in fold 1 only
    y = [np.array([[2.0, 0.0, 0.3], [0.0, 0.0, -1.0], [1.0, 0.0, 0.5]]), np.array([[3.0, 0.0, 0.1, 4.0], [1.0, 0.0, 0.2, 1.0]])]
    sums = np.zeros((2, 4, 4))
    ll_model = np.array([[-3.5, -0.25, -2.0, 0.0], [-4.0, -0.5, -1.0, -2.5]])
    for k, yk in enumerate(y):
        for n in range(yk.shape[1]):
            lg = (yk[:, n] ** 2).sum() if n == 2 else gammaln(yk[:, n] + 1.0).sum()
            sums[k, n] = [ll_model[k, n], yk[:, n].sum(), 1.0, lg]
    n_entries = np.array([5, 5, 5, 2])
    got = entry_scores(sums, n_entries, gauss=[False, False, True, False])
    assert np.array_equal(got["ll_per_fold"], ll_model) and np.array_equal(got["n_entries"], n_entries)
    assert np.array_equal(got["ll"], ll_model[0] + ll_model[1])
    assert np.array_equal(got["n_spikes"][[0, 1, 3]], [7.0, 0.0, 5.0])
    # the null model by hand: a constant rate at the mean count over the held-out entries of the channel
    y0 = np.array([2.0, 0.0, 1.0, 3.0, 1.0])
    null0 = (y0 * math.log(y0.mean()) - y0.mean() - gammaln(y0 + 1.0)).sum()
    y3 = np.array([4.0, 1.0])
    null3 = (y3 * math.log(2.5) - 2.5 - gammaln(y3 + 1.0)).sum()
    assert got["ll_null"][0] == pytest.approx(null0, rel=1e-14) and got["ll_null"][3] == pytest.approx(null3, rel=1e-14)
    assert got["ll_null"][1] == 0.0 and np.isnan(got["ll_null"][2])
    assert got["bits_per_spike"][0] == pytest.approx((-7.5 - null0) / (7.0 * math.log(2.0)), rel=1e-14)
    assert got["bits_per_spike"][3] == pytest.approx((-2.5 - null3) / (5.0 * math.log(2.0)), rel=1e-14)
    assert np.isnan(got["bits_per_spike"][1]) and np.isnan(got["bits_per_spike"][2])
    pooled = (-7.5 - 2.5 - null0 - null3) / (12.0 * math.log(2.0))
    assert got["speckled_bps"] == pytest.approx(pooled, rel=1e-14)
    assert got["speckled_bps"] == co_bits_per_spike(got["ll"], got["ll_null"], got["n_spikes"])
    # a channel that is never held out: zeros in, NaN score, no warning-born garbage in the pool
    none = entry_scores(np.zeros((2, 1, 4)), [0])
    assert np.isnan(none["bits_per_spike"][0]) and none["ll_null"][0] == 0.0 and np.isnan(none["speckled_bps"])
    with pytest.raises(ValueError):
        entry_scores(np.zeros((2, 4)), [1, 1])


def test_memory_accounting_counts_mask_and_row_constant():
    from vlgp_amd.evaluation import REPLICA_BUDGET_BYTES, default_max_replicas

    rows, L = 40 * 1000, 5
    plain = default_max_replicas(rows, L)
    masked = default_max_replicas(rows, L, mask_channels=100)
    mixed = default_max_replicas(rows, L, mask_channels=100, gauss=True)
    assert plain > masked > mixed >= 1
    per = 10 * 8 * rows * L + 8 * rows * 2 + 8 * rows * L  # replica + two mask words per row + L doubles per row
    assert mixed == REPLICA_BUDGET_BYTES // per
    assert default_max_replicas(10 ** 9, 10, mask_channels=14, gauss=True) == 1


def test_header_declares_replicate_masked_in_the_held_out_block():
    from vlgp_amd import _lib

    text = open(HEADER).read()
    proto = "int vlgp_replicate_masked(vlgp_ctx* ctx, int src, int dst, int n_rep, const uint64_t* held_out);"
    assert text.count(proto) == 1
    block = text.index("/* ---- held-out evaluation ----")
    nxt = text.index("/* ---- parameters")
    units = text.index("int vlgp_replicate_units(")
    assert block < units < text.index(proto) < text.index("int vlgp_loglik(") < nxt
    last = [m.start() for m in re.finditer(r"^int vlgp_[a-z_0-9]+\(", text, flags=re.M)][-1]
    assert text.index("int vlgp_replicate_groups(") == last  # (not appended: the last prototype stays the last)
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3 and _lib.ABI_VERSION == 3
    assert "vlgp_replicate_masked" in _lib.EXPORTS
    res, args = _lib._SIGNATURES["vlgp_replicate_masked"]
    assert len(args) == 5


def test_built_library_exports_replicate_masked():
    from vlgp_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "vlgp_replicate_masked"), "libvlgp_hip.so lacks vlgp_replicate_masked"
    assert lib.vlgp_abi_version() == 3


def test_public_names():
    import vlgp_amd

    assert callable(vlgp_amd.impute) and "impute" in vlgp_amd.__all__
    for name in ("entry_folds", "entry_scores", "leave_entries_out", "impute"):
        assert name in vlgp_amd.evaluation.__all__


def test_cross_validate_refuses_an_unknown_score():
    import vlgp_amd

    trials = [{"y": np.zeros((10, 3))} for _ in range(4)]
    with pytest.raises(ValueError, match="score"):
        vlgp_amd.cross_validate(trials, [1], score="nonsense")


def test_bad_fold_and_mask_arrays_are_value_errors():
    import heldout_numpy as H
    from vlgp_amd import evaluation as ev

    trials, params, config = H.problem(seed=3, M=2, T=20, N=5)
    good = [np.zeros((20, 5), dtype=int) for _ in trials]
    for bad in (good[:1], [good[0], np.zeros((19, 5), dtype=int)], [good[0], np.zeros((20, 5))],
                [good[0], np.full((20, 5), -2)], [np.full((20, 5), -1)] * 2):
        with pytest.raises(ValueError):
            ev.leave_entries_out(trials, params, config, folds=bad)
    with pytest.raises(ValueError):
        ev.impute(trials, params, config, missing=good)  # (integers, not bool)
