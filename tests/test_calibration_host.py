"""Calibration of the predictive distribution without a device: the NumPy restatement of its definition
(tests/calibration_numpy.py) against a dense trapezoid, the host summaries of the sums, the coverage rule against
brute-force quantiles, and the wiring of vlgp_calibration through the header, the binding and the public names."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.stats import norm

import calibration_numpy as CN
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "vlgp_hip.h")

M_GRID = (-3.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0)


def _grid(sigma):
    """(k, m) over M_GRID with k in {0, 1, 2, floor(lam / 2), floor(lam), floor(1.5 lam), floor(3 lam)}."""
    out = []
    for m in M_GRID:
        lam = np.exp(m + 0.5 * sigma * sigma)
        out += [(float(k), m) for k in sorted({0, 1, 2, int(lam / 2), int(lam), int(1.5 * lam), int(3 * lam)})]
    return out


# ten times the errors measured for this definition against the trapezoid (whose own floor is 1.2e-12):
# 12 nodes: 1.3e-12 at sigma 0.05 and 0.1, 1.9e-10 at 0.3, 8.0e-9 at 0.5, 1.2e-6 at 1.0; 32 nodes: 4.0e-11 at 1.0
@pytest.mark.parametrize("n_nodes, sigma, bound", [(12, 0.05, 8e-8), (12, 0.1, 8e-8), (12, 0.3, 8e-8), (12, 0.5, 8e-8),
                                                   (12, 1.0, 1.2e-5), (32, 1.0, 4e-10)])
def test_the_sum_of_mode_centred_masses_against_a_dense_trapezoid(n_nodes, sigma, bound):
    grid = _grid(sigma)
    k, m = (np.array(t) for t in zip(*grid))
    s2 = np.full(k.shape, sigma * sigma)
    lo, hi, skip = CN.count_cdf(k, m, s2, np.exp(np.minimum(m + 0.5 * s2, 10.0)), n_nodes, max_count=65536)
    assert not skip.any()
    want_lo = np.array([CN.truth_cdf(kk - 1, mm, sigma) for kk, mm in grid])
    want_hi = np.array([CN.truth_cdf(kk, mm, sigma) for kk, mm in grid])
    err = np.maximum(np.abs(lo - want_lo), np.abs(hi - want_hi))
    worst = int(np.argmax(err))
    print("measured calibration rule n_nodes %2d sigma %.2f: worst |error| %.3e at (k, m) = %r"
          % (n_nodes, sigma, err[worst], grid[worst]))
    assert err.max() <= bound, (err.max(), grid[worst])
    assert np.all(lo[k == 0] == 0.0) and np.all((0.0 <= lo) & (lo <= hi) & (hi <= 1.0))


def test_gaussian_channel_is_the_normal_distribution_function_with_both_variances():
    """u against scipy.stats.norm.cdf at 1e-15 relative.  The two sides round the argument of erfc differently (sqrt(2 var)
    here, sqrt(var) and a multiplication by sqrt(1/2) there: up to six roundings of 1.1e-16 between them) and u answers a
    relative change of its argument x = (y - m) / sd with the factor |x phi(x) / Phi(x)|, which is below 1 for x >= -0.75 and
    grows like x^2 in the lower tail; so the entries lie at x in [-0.75, 3]: six roundings and an ulp of erfc on either
    side stay inside 1e-15."""
    rng = np.random.default_rng(2)
    T, N, L = 40, 3, 2
    x = np.ones((T, 1, N))
    mu, v = rng.standard_normal((T, L)), rng.random((T, L))
    a, b, noise = rng.standard_normal((L, N)), rng.standard_normal((1, N)), 0.5 + rng.random(N)
    m, sd = mu @ a + b, np.sqrt(noise + v @ a ** 2)
    y = m + sd * rng.uniform(-0.75, 3.0, (T, N))
    lo, hi, pearson, skip = CN.entries(y, x, mu, v, a, b, noise, np.ones(N, dtype=bool), True, 12)
    want = norm.cdf(y, loc=m, scale=sd)
    assert np.array_equal(lo, hi) and not skip.any()
    err = np.max(np.abs(lo - want) / want)
    print("measured calibration gaussian u against norm.cdf: %.2e relative" % err)
    assert err <= 1e-15
    assert np.max(np.abs(pearson - ((y - m) / sd) ** 2)) <= 1e-12


def test_calibration_from_sums_normalises_pools_and_survives_empty_slots():
    from vlgp_amd.evaluation import calibration_from_sums

    #                pit0 pit1 pit2 cov50 cov90 pearson entries skipped
    sums = np.array([[1.0, 2.5, 0.5, 2.0, 4.0, 6.0, 4.0, 1.0],
                     [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0],
                     [3.0, 1.0, 2.0, 3.0, 5.0, 3.0, 6.0, 0.0]])
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a slot without an entry gives NaN, not a warning
        out = calibration_from_sums(sums, 3, (0.5, 0.9))
    assert set(out) == {"pit", "pit_all", "coverage", "coverage_all", "levels", "dispersion", "dispersion_all", "entries",
                        "skipped"}
    assert np.array_equal(out["pit"][0], [0.25, 0.625, 0.125]) and np.array_equal(out["pit"][2], [0.5, 1 / 6, 2 / 6])
    assert np.all(np.isnan(out["pit"][1])) and np.all(np.isnan(out["coverage"][1])) and np.isnan(out["dispersion"][1])
    assert np.array_equal(out["coverage"][[0, 2]], [[0.5, 1.0], [0.5, 5 / 6]])
    assert np.array_equal(out["dispersion"][[0, 2]], [1.5, 0.5]) and out["dispersion_all"] == 0.9
    assert np.array_equal(out["pit_all"], [0.4, 0.35, 0.25]) and np.array_equal(out["coverage_all"], [0.5, 0.9])
    assert np.array_equal(out["entries"], [4, 0, 6]) and np.array_equal(out["skipped"], [1, 2, 0])
    assert np.array_equal(out["levels"], [0.5, 0.9])
    assert abs(out["pit"][0].sum() - 1.0) <= 1e-15 and abs(out["pit_all"].sum() - 1.0) <= 1e-15
    # leading axes are kept (a masked set: (replica, channel, W)); no levels; nothing at all
    two = calibration_from_sums(np.stack([sums, sums]), 3, (0.5, 0.9))
    assert two["pit"].shape == (2, 3, 3) and two["entries"].shape == (2, 3) and np.array_equal(two["pit_all"], out["pit_all"])
    none = calibration_from_sums(sums[:, [0, 1, 2, 5, 6, 7]], 3, ())
    assert none["coverage"].shape == (3, 0) and none["coverage_all"].shape == (0,)
    empty = calibration_from_sums(np.zeros((2, 8)), 3, (0.5, 0.9))
    assert np.all(np.isnan(empty["pit_all"])) and np.isnan(empty["dispersion_all"])
    with pytest.raises(ValueError, match="columns"):
        calibration_from_sums(sums, 4, (0.5, 0.9))


def test_coverage_rule_is_the_central_quantile_interval():
    """hi >= a and lo < 1 - a  <=>  q_a <= y <= q_{1-a}, q_p = min{k : F(k) >= p} by brute force from the same masses, on
    every entry of a small random problem."""
    rng = np.random.default_rng(7)
    n = 300
    m, s2 = rng.uniform(-2.0, 3.0, n), rng.uniform(0.0, 0.8, n) * (rng.random(n) < 0.9)
    lam = np.exp(np.minimum(m + 0.5 * s2, 10.0))
    y = rng.poisson(lam * np.exp(0.7 * rng.standard_normal(n))).astype(float)
    levels = (0.5, 0.9, 0.99, 0.2)
    lo, hi, skip = CN.count_cdf(y, m, s2, lam, 12)
    assert not skip.any() and (s2 == 0.0).sum() >= 10
    cols = CN.columns(lo, hi, np.zeros(n), skip, 4, levels)
    kmax = int(y.max()) + 200
    masses = np.stack([CN.mass(j, m, s2, lam, 12) for j in range(kmax)], axis=1)
    seen = set()
    for c, level in enumerate(levels):
        a = (1.0 - level) / 2.0
        for i in range(n):
            q_lo, q_hi = CN.central_quantile(masses[i], a), CN.central_quantile(masses[i], 1.0 - a)
            assert q_hi < kmax
            inside = q_lo <= y[i] <= q_hi
            assert cols[i, 4 + c] == float(inside), (i, level, y[i], q_lo, q_hi, lo[i], hi[i])
            seen.add(inside)
    assert seen == {True, False}
    assert np.all(np.abs(cols[:, :4].sum(axis=1) - 1.0) <= 1e-12)  # every entry adds total mass 1 to the histogram


def test_skipped_entries_add_to_skipped_and_nothing_else():
    y = np.array([3.0, 9.0, 2.5, -1.0, np.nan, np.inf, 8.0])
    m, s2 = np.zeros(7), np.full(7, 0.25)
    lo, hi, skip = CN.count_cdf(y, m, s2, np.exp(m + 0.5 * s2), 12, max_count=8)
    assert np.array_equal(skip, [False, True, True, True, True, True, False])
    assert np.all(np.isnan(lo[skip])) and np.all(np.isnan(hi[skip])) and np.all(np.isfinite(hi[~skip]))
    cols = CN.columns(lo, hi, np.where(skip, np.nan, 1.0), skip, 5, (0.9,))
    assert np.array_equal(cols[skip], np.tile([0, 0, 0, 0, 0, 0, 0, 0, 1.0], (5, 1)))
    assert np.all(cols[~skip][:, -2] == 1.0) and np.all(cols[~skip][:, -1] == 0.0)


def test_header_binding_library_and_public_names():
    import vlgp_amd
    from vlgp_amd import _lib, evaluation

    text = open(HEADER).read()
    proto = re.search(r"int vlgp_calibration\(vlgp_ctx\* ctx, int set, int vb, int n_nodes, const double\* z, "
                      r"const double\* lwa,\s+int n_bins,\s+int n_levels, const double\* levels, int max_count, "
                      r"double\* cdf, double\* sums\);", text)
    assert proto, "include/vlgp_hip.h does not declare vlgp_calibration"
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3 and _lib.ABI_VERSION == 3
    assert "vlgp_calibration" in _lib.EXPORTS and len(_lib._SIGNATURES["vlgp_calibration"][1]) == 12
    lib = _lib.load()
    assert hasattr(lib, "vlgp_calibration") and lib.vlgp_abi_version() == 3
    assert "calibration" in evaluation.__all__ and "calibration_from_sums" in evaluation.__all__
    assert callable(vlgp_amd.Engine.calibration)


@pytest.mark.parametrize("kw, name", [(dict(n_bins=0), "n_bins"), (dict(n_bins=33), "n_bins"), (dict(n_bins=2.0), "n_bins"),
                                      (dict(levels=(0.1, 0.2, 0.3, 0.4, 0.5)), "levels"), (dict(levels=(0.5, 1.0)), "level"),
                                      (dict(levels=(0.0,)), "level"), (dict(levels=(np.nan,)), "level"),
                                      (dict(max_count=0), "max_count"), (dict(max_count=65537), "max_count"),
                                      (dict(n_nodes=0), "n_nodes"), (dict(n_nodes=65), "n_nodes")])
def test_arguments_are_checked_before_any_device_call(kw, name):
    """Engine.calibration with something that is no engine, evaluation.calibration with trials no device could take: the
    ValueError comes first."""
    from vlgp_amd import evaluation
    from vlgp_amd.engine import Engine

    with pytest.raises(ValueError, match=name):
        Engine.calibration(object(), 0, **kw)
    trials = [{"y": np.zeros((10, 3))}]
    for how in ("in_sample", "channels", "entries"):
        with pytest.raises(ValueError, match=name):
            evaluation.calibration(trials, {"ydim": 3, "zdim": 1}, {}, how=how, **kw)


def test_calibration_refuses_an_unknown_how_and_trials_with_missing():
    from vlgp_amd import evaluation

    trials = [{"y": np.zeros((10, 3)), "missing": np.zeros((10, 3), dtype=bool)}]
    with pytest.raises(ValueError, match="how"):
        evaluation.calibration(trials, {"ydim": 3, "zdim": 1}, {}, how="trials")
    with pytest.raises(ValueError, match="missing"):
        evaluation.calibration(trials, {"ydim": 3, "zdim": 1}, {})


@pytest.fixture(scope="module")
def layout_driver(tmp_path_factory):
    """tests/calibration_layout_driver.cpp as a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path_factory.mktemp("calibration_layout") / "calibration_layout_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vlgp_amd", "csrc"), os.path.join(ROOT, "tests", "calibration_layout_driver.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


@pytest.mark.parametrize("want_cdf", [False, True])
@pytest.mark.parametrize("n_bins, n_levels", [(1, 0), (10, 2), (32, 4), (2, 3)])
@pytest.mark.parametrize("slots, rows", [(1, 1), (6, 301), (140, 301)])
def test_calibration_layout(layout_driver, slots, rows, n_bins, n_levels, want_cdf):
    """The regions of the call's device block lie in order, without overlap, up to ``need``, each as large as the launcher
    and the copies use it: nodes 2 x 64, levels 4, cdf 2 per entry when wanted, sums (slots, 4 G), partials (slots, G, n_blk,
    4) with G = ceil(W / 4) groups for W = n_bins + n_levels + 3 columns."""
    n_rate, n_blk = rows * 3, (rows + 255) // 256
    done = subprocess.run([layout_driver] + [str(int(v)) for v in (slots, n_rate, n_blk, n_bins, n_levels, want_cdf)],
                          capture_output=True, timeout=60)
    assert done.returncode == 0, done.stderr.decode(errors="replace")[-3000:]
    got = dict((k, int(v)) for k, v in (ln.split(" ") for ln in done.stdout.decode().splitlines()))
    W = n_bins + n_levels + 3
    G = -(-W // 4)
    assert got["groups"] == G and 4 * G >= W > 4 * (G - 1)
    sizes = [("nodes", 128), ("levels", 4), ("cdf", 2 * n_rate if want_cdf else 0), ("sums", 4 * G * slots),
             ("part", slots * G * n_blk * 4)]
    at = 0
    for name, size in sizes:
        assert got[name] == at, (name, got)
        at += size
    assert got["need"] == at
