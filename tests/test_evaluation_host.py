"""Held-out evaluation, host side: the C ABI declares and binds the new entry points, bits per spike from
vlgp_loglik's sums equals a direct NumPy computation, and the replica chunk planner covers every channel once."""
import math
import os
import re

import numpy as np
import pytest
from scipy.special import gammaln

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_binds_the_evaluation_entry_points():
    from vlgp_amd import _lib

    text = open(os.path.join(ROOT, "include", "vlgp_hip.h")).read()
    assert re.search(r"int vlgp_replicate_units\(vlgp_ctx\* ctx, int src, int dst, int n_rep, const int\* channel\);", text)
    assert re.search(r"int vlgp_loglik\(vlgp_ctx\* ctx, int set, int vb, double\* rate, double\* sums\);", text)
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3
    assert _lib.ABI_VERSION == 3
    assert "vlgp_replicate_units" in _lib.EXPORTS and "vlgp_loglik" in _lib.EXPORTS


def test_evaluation_is_exported():
    import vlgp_amd

    assert hasattr(vlgp_amd.evaluation, "leave_one_out") and hasattr(vlgp_amd.evaluation, "loglik")


def test_bits_per_spike_from_sums_equals_numpy():
    from vlgp_amd.evaluation import bits_per_spike

    rng = np.random.default_rng(0)
    T, N = 500, 6
    rate = np.exp(rng.normal(-1.0, 0.7, size=(T, N)))
    y = rng.poisson(rate).astype(float)
    y[:, 4] = 0.0  # a silent channel: NaN
    gauss = np.zeros(N, bool)
    gauss[5] = True
    lg = gammaln(y + 1.0)
    ll = y * np.log(rate) - rate - lg
    sums = np.stack([ll.sum(0), y.sum(0), rate.sum(0), lg.sum(0)], axis=1)
    got_ll, got_null, got_n, got_bps = bits_per_spike(sums, T, gauss)
    for n in range(N):
        if gauss[n] or y[:, n].sum() == 0:
            assert math.isnan(got_bps[n])
            continue
        ybar = y[:, n].mean()
        null = np.sum(y[:, n] * np.log(ybar) - ybar - lg[:, n])
        want = (ll[:, n].sum() - null) / (y[:, n].sum() * math.log(2.0))
        assert got_null[n] == pytest.approx(null, rel=1e-12)
        assert got_bps[n] == pytest.approx(want, rel=1e-10)
        assert got_n[n] == y[:, n].sum()
        assert got_ll[n] == sums[n, 0]


@pytest.mark.parametrize("n_ch,cap", [(1, 1), (14, 1), (14, 3), (14, 14), (14, 100), (100, 7)])
def test_chunk_planner_covers_every_channel_once(n_ch, cap):
    from vlgp_amd.evaluation import plan_chunks

    channels = list(np.random.default_rng(n_ch).permutation(n_ch))
    chunks = plan_chunks(channels, cap)
    assert all(1 <= len(c) <= cap for c in chunks)
    assert [c for ch in chunks for c in ch] == channels


def test_default_chunk_budget():
    from vlgp_amd.evaluation import REPLICA_BUDGET_BYTES, default_max_replicas

    # 40 trials x 1000 bins at L = 5: the 100 replicas of a 100-channel test set fit one chunk
    assert default_max_replicas(40 * 1000, 5) >= 100
    assert default_max_replicas(40 * 1000, 5) * 10 * 8 * 40 * 1000 * 5 <= REPLICA_BUDGET_BYTES
    assert default_max_replicas(10 ** 9, 10) == 1
