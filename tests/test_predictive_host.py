"""The posterior-predictive density without a device: the NumPy restatement of its definition (tests/predictive_numpy.py)
against a brute-force integral, its limiting cases, and the wiring of vlgp_predictive through the header, the binding
and the public names."""
import os
import re

import numpy as np
import pytest
from scipy.special import gammaln
from scipy.stats import norm

import predictive_numpy as PN
from conftest import ROOT
from oracle import vlgp_oracle as O

HEADER = os.path.join(ROOT, "include", "vlgp_hip.h")

M_GRID = (-8.0, -5.0, -3.0, -1.0, 0.0, 1.0, 2.5, 4.0, 5.0)
SIGMA_GRID = (0.02, 0.1, 0.3, 0.5, 0.7, 1.0)
Y_GRID = (0.0, 1.0, 2.0, 5.0, 10.0, 30.0, 100.0)


def test_mode_centred_rule_against_a_brute_force_integral():
    """Worst absolute error of lpd over the grid: <= 1e-5 at 12 nodes, <= 1e-7 at 20 (measured for this definition:
    1.5e-6 and 2.0e-8).  The reference is a 2M-point trapezoid of the same integrand, clamp included."""
    grid = [(y, m, s) for m in M_GRID for s in SIGMA_GRID for y in Y_GRID]
    y, m, s = (np.array(t) for t in zip(*grid))
    want = np.array([PN.brute_force(*p) for p in grid])
    for n_nodes, bound in ((12, 1e-5), (20, 1e-7)):
        err = np.abs(PN.poisson_lognormal(y, m, s * s, n_nodes) - want)
        worst = int(np.argmax(err))
        print("n_nodes = %d: worst |error| %.3e at (y, m, sigma) = %r" % (n_nodes, err[worst], grid[worst]))
        assert err.max() <= bound, (n_nodes, err.max(), grid[worst])


def test_the_rule_degrades_outside_its_regime_as_documented():
    """sigma = 3, m = 9, y = 0 at 12 nodes: an error of the order the documents state (0.06), far above the bound of the
    grid -- the accuracy figures hold in the stated regime only."""
    err = abs(float(PN.poisson_lognormal(0.0, 9.0, 9.0, 12)) - PN.brute_force(0.0, 9.0, 3.0))
    assert 0.02 < err < 0.2, err


@pytest.mark.parametrize("m, sigma", [(-2.0, 0.5), (1.0, 1.0), (3.0, 0.3), (0.0, 0.05)])
def test_it_is_a_density(m, sigma):
    y = np.arange(401.0)
    total = np.exp(PN.poisson_lognormal(y, m, sigma * sigma, 20)).sum()
    assert abs(total - 1.0) <= 1e-6, total


def test_zero_variance_is_the_plug_in_expression():
    rng = np.random.default_rng(0)
    T, N, L = 30, 5, 2
    y = rng.poisson(2.0, (T, N)).astype(float)
    x = np.ones((T, 1, N))
    mu, a, b = rng.standard_normal((T, L)), 0.5 * rng.standard_normal((L, N)), rng.standard_normal((1, N))
    gauss = np.zeros(N, dtype=bool)
    eta = O.linear_predictor(x, mu, a, b)
    plug = y * np.log(np.exp(np.minimum(eta, 10.0))) - np.exp(np.minimum(eta, 10.0)) - gammaln(y + 1.0)
    for v, vb in ((np.zeros((T, L)), True), (np.ones((T, L)), False)):
        lpd, rate = PN.lpd_rate(y, x, mu, v, a, b, np.ones(N), gauss, vb, 12)
        assert np.array_equal(lpd, plug) and np.array_equal(rate, np.exp(np.minimum(eta, 10.0)))


def test_one_node_is_the_laplace_form():
    rng = np.random.default_rng(1)
    y = rng.poisson(3.0, 200).astype(float)
    m, s2 = rng.uniform(-4, 4, 200), rng.uniform(0.01, 1.0, 200)
    e = PN.mode(y, m, s2)
    g = y * np.minimum(e, 10.0) - PN.ex(e) - (e - m) ** 2 / (2 * s2) - gammaln(y + 1.0)
    laplace = -0.5 * np.log(s2 * PN.ex(e) + 1.0) + g
    assert np.max(np.abs(PN.poisson_lognormal(y, m, s2, 1) - laplace)) <= 1e-12


def test_gaussian_channel_is_the_normal_density_with_both_variances():
    rng = np.random.default_rng(2)
    T, N, L = 40, 3, 2
    y, x = rng.standard_normal((T, N)), np.ones((T, 1, N))
    mu, v = rng.standard_normal((T, L)), rng.random((T, L))
    a, b, noise = rng.standard_normal((L, N)), rng.standard_normal((1, N)), 0.5 + rng.random(N)
    lpd, rate = PN.lpd_rate(y, x, mu, v, a, b, noise, np.ones(N, dtype=bool), True, 12)
    m = mu @ a + b
    want = norm.logpdf(y, loc=m, scale=np.sqrt(noise + v @ a ** 2))
    assert np.max(np.abs(lpd - want)) <= 1e-12 and np.array_equal(rate, m)


def test_header_binding_library_and_public_names():
    import vlgp_amd
    from vlgp_amd import _lib, evaluation

    text = open(HEADER).read()
    proto = re.search(r"int vlgp_predictive\(vlgp_ctx\* ctx, int set, int vb, int n_nodes, const double\* z, "
                      r"const double\* lwa,\s+double\* rate,\s+double\* lpd, double\* sums\);", text)
    assert proto, "include/vlgp_hip.h does not declare vlgp_predictive"
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3 and _lib.ABI_VERSION == 3
    assert "vlgp_predictive" in _lib.EXPORTS and len(_lib._SIGNATURES["vlgp_predictive"][1]) == 9
    lib = _lib.load()
    assert hasattr(lib, "vlgp_predictive") and lib.vlgp_abi_version() == 3
    assert "hermite_nodes" in evaluation.__all__ and callable(vlgp_amd.Engine.predictive)


def test_hermite_nodes_are_the_definitions_and_refuse_other_sizes():
    from vlgp_amd import evaluation

    for n in (1, 12, 64):
        z, lwa = evaluation.hermite_nodes(n)
        zz, ll = PN.hermite_nodes(n)
        assert np.array_equal(z, zz) and np.array_equal(lwa, ll) and np.all(np.isfinite(lwa))
        assert abs(np.exp(lwa - 0.5 * z * z).sum() - 1.0) <= 1e-12  # (the weights of a standard normal add to one)
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_nodes"):
            evaluation.hermite_nodes(bad)


def test_cross_validate_refuses_predictive_marginal_scores():
    import vlgp_amd

    trials = [{"y": np.zeros((10, 3))} for _ in range(4)]
    with pytest.raises(ValueError, match="marginal_bps"):
        vlgp_amd.cross_validate(trials, [1], score="marginal_bps", predictive=True)


def test_public_scores_check_n_nodes_before_any_device_work():
    from vlgp_amd import evaluation

    trials = [{"y": np.zeros((10, 3))}]
    with pytest.raises(ValueError, match="n_nodes"):
        evaluation.leave_group_out(trials, {"ydim": 3, "zdim": 1}, {}, predictive=True, n_nodes=0)
