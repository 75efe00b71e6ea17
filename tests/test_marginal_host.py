"""The importance-weighted marginal likelihood, CPU side: the NumPy restatement of its definitions
(tests/marginal_numpy.py) against dense closed forms and against the variational bound, and the pieces of the feature
that need no device."""
import math
import os
import re

import numpy as np
import pytest
from scipy.stats import multivariate_normal

import elbo_numpy as EN
import forecast_numpy as FN
import marginal_numpy as MN
from conftest import ROOT
from oracle import vlgp_oracle as O

STAGE = 1e-9
HEADER = os.path.join(ROOT, "include", "vlgp_hip.h")


def test_c_is_the_difference_of_two_dense_normal_log_densities():
    """c = log N(beta; 0, I) - log N(beta; m, H^-1), both from scipy's dense density, at rel 1e-12 (T = 12)."""
    T, K = 12, 7
    rng = np.random.default_rng(3)
    G_in = O.build_prior([T], np.array([2e-2]), np.ones(1), 50)[T][0]
    r = FN.rank(G_in)
    assert 1 < r < T
    w, z, eps = rng.uniform(0.1, 2.0, T), rng.standard_normal(T), rng.standard_normal((50, K))
    beta, c, c_abs, (m, Lc, _) = MN.draws(G_in, w, z, eps)
    H = Lc @ Lc.T
    for k in range(K):
        want = multivariate_normal.logpdf(beta[:, k], np.zeros(r), np.eye(r)) \
            - multivariate_normal.logpdf(beta[:, k], m, np.linalg.inv(H))
        print("draw %d: c %.12f dense %.12f rel %.2e" % (k, c[k], want, abs(c[k] - want) / abs(want)))
        assert abs(c[k] - want) <= 1e-12 * abs(want)
        assert abs(c[k]) <= c_abs[k]
    eps2 = eps.copy()
    eps2[r:] = np.nan  # (rows >= r are not read)
    assert np.array_equal(MN.draws(G_in, w, z, eps2)[1], c)


def exact_gaussian_problem(seed=5, M=3, T=24):
    """All-Gaussian channels with disjoint loading supports (L = 3, N = 6, noise >= 0.5): the model is jointly Gaussian,
    the channels of different latents are independent, and with w = sum_n a^2 / noise (the model's own curvature, which
    does not depend on mu) the proposal N(m, H^-1) IS the posterior of beta whatever mu holds -- one Newton step on a
    quadratic lands on its optimum.  Every importance weight then equals p(y).  Returns the units, the parameters, the
    prior and the dense closed form log N(y; bx, sum_l (a_l a_l') (x) G_l G_l' + diag(noise) (x) I) per unit."""
    L, N, R = 3, 6, 50
    rng = np.random.default_rng(seed)
    a = np.zeros((L, N))
    for l in range(L):
        a[l, 2 * l:2 * l + 2] = rng.uniform(0.5, 1.5, 2) * rng.choice([-1.0, 1.0], 2)
    b = rng.standard_normal((1, N))
    noise = 0.5 + rng.random(N)
    gauss = np.ones(N, bool)
    prior = O.build_prior([T], np.array([2e-2, 5e-3, 1e-3]), np.ones(L), R)
    cov = np.kron(np.diag(noise), np.eye(T))  # (channel-major: entry n T + t)
    for l in range(L):
        cov += np.kron(np.outer(a[l], a[l]), prior[T][l] @ prior[T][l].T)
    units, closed = [], []
    for _ in range(M):
        y = rng.multivariate_normal(np.repeat(b[0], T), cov).reshape(N, T).T.copy()
        units.append({"y": y, "x": None, "mu": rng.standard_normal((T, L)), "v": 0.1 * rng.random((T, L)),
                      "w": np.tile((a ** 2 / noise).sum(axis=1), (T, 1))})
        closed.append(multivariate_normal.logpdf(y.T.ravel(), np.repeat(b[0], T), cov))
    return units, a, b, noise, gauss, prior, np.array(closed)


def test_with_an_exact_posterior_every_weight_is_the_marginal_likelihood():
    units, a, b, noise, gauss, prior, closed = exact_gaussian_problem()
    eps = np.random.default_rng(1).standard_normal((len(units), 3, 50, 9))
    log_w, parts, scale = MN.statement(units, a, b, noise, gauss, prior, eps)
    err = np.abs(log_w - closed[:, None]) / scale
    print("exactness: closed form %s, max |log_w - closed| / sum|terms| %.2e, spread over k %.2e" % (
        closed, err.max(), np.max(np.ptp(log_w, axis=1) / scale.max(axis=1))))
    assert err.max() <= STAGE
    assert np.array_equal(parts[:, :, 0] + parts[:, :, 1], log_w)


SEED_K4096 = 2  # (checked on the CPU before it was committed: see the printed margins)


@pytest.fixture(scope="module")
def converged_poisson():
    """M = 4 units, T = 60, N = 12, L = 2, Poisson, rates far below the clamp, each unit converged with the oracle's
    E-step until off_fixed_point < 1e-20."""
    M, T, N, L, R = 4, 60, 12, 2, 50
    rng = np.random.default_rng(0)
    omega = np.array([5e-3, 2e-2])
    prior = O.build_prior([T], omega, np.ones(L), R)
    t = np.arange(T)
    a = 0.5 * rng.standard_normal((L, N))
    b = np.log(0.5) + 0.3 * rng.standard_normal((1, N))
    gauss, noise = np.zeros(N, bool), np.ones(N)
    x = np.ones((T, 1, N))
    zero = np.zeros((T, L))
    units = []
    for _ in range(M):
        lat = np.stack([np.linalg.cholesky(np.exp(-om * (t[:, None] - t[None, :]) ** 2) + 1e-8 * np.eye(T))
                        @ rng.standard_normal(T) for om in omega], axis=1)
        y = rng.poisson(np.exp(lat @ a + b)).astype(float)
        mu, v, w, _, bad = O.estep_unit(y, x, zero, zero, zero, a, b, noise, gauss, prior[T], 400, dmu_bound=1e300)
        assert bad == 0 and np.max(mu @ a + b) < 5.0
        u = {"y": y, "x": None, "mu": mu, "v": v, "w": w}
        terms = FN.forecast_unit(u, a, b, noise, gauss, prior[T], prior[T])[2]
        off = np.max(terms[:, 0] / terms[:, 1])
        print("off_fixed_point %.2e" % off)
        assert off < 1e-20
        units.append(u)
    return units, a, b, noise, gauss, prior


def test_mean_log_weight_meets_the_bound_within_its_standard_error(converged_poisson):
    """E_q log_w is the variational bound when mu, v, w are the E-step's fixed point: the mean over K = 4096 draws is
    within 5 standard errors of elbo_numpy's value for every unit, and the IWAE estimate is not below it."""
    units, a, b, noise, gauss, prior = converged_poisson
    K = 4096
    eps = np.random.default_rng(SEED_K4096).standard_normal((len(units), 2, 50, K))
    log_w, _, _ = MN.statement(units, a, b, noise, gauss, prior, eps)
    st = EN.statement(units, a, b, noise, gauss, prior)
    T = units[0]["y"].shape[0]
    from vlgp_amd.evaluation import weights_summary

    iwae, elbo_mc, ess = weights_summary(log_w)
    for i in range(len(units)):
        bound = st["row_ell"][i * T:(i + 1) * T].sum() - st["kl"][i].sum()
        se = np.std(log_w[i]) / math.sqrt(K)
        print("unit %d: elbo %.4f mean log_w %.4f (%.2f s.e., s.e. %.4f) iwae %.4f ess %.0f" % (
            i, bound, elbo_mc[i], (elbo_mc[i] - bound) / se, se, iwae[i], ess[i]))
        assert abs(elbo_mc[i] - bound) <= 5.0 * se
        assert iwae[i] >= elbo_mc[i]


def test_weights_summary_edge_cases():
    from vlgp_amd.evaluation import weights_summary

    lw = np.log(np.array([[1.0, 2.0, 3.0, 2.0]]))
    iwae, mc, ess = weights_summary(lw)
    assert abs(iwae[0] - math.log(2.0)) <= 1e-15 and abs(mc[0] - np.mean(lw)) <= 1e-15
    assert abs(ess[0] - 64.0 / 18.0) <= 1e-14
    far, far_mc, far_ess = weights_summary(lw - 1e5)  # (exp(-1e5) underflows: the shift keeps everything)
    assert abs(far[0] - (math.log(2.0) - 1e5)) <= 1e-10 and abs(far_ess[0] - 64.0 / 18.0) <= 1e-9
    assert abs(far_mc[0] - (mc[0] - 1e5)) <= 1e-10
    one = weights_summary(np.array([[-3.5], [2.0]]))  # K = 1: the estimate is the draw, one effective sample
    assert np.array_equal(one[0], [-3.5, 2.0]) and np.array_equal(one[1], [-3.5, 2.0]) and np.array_equal(one[2], [1.0, 1.0])
    flat = weights_summary(np.full(16, -7.0))  # (a 1-d input is one unit)
    assert abs(flat[0] - -7.0) <= 1e-14 and abs(flat[2] - 16.0) <= 1e-12
    mixed = weights_summary(np.array([[0.0, np.nan, 1.0], [0.0, 1.0, 2.0]]))
    for arr in mixed:
        assert np.isnan(arr[0]) and np.isfinite(arr[1])
    spike = weights_summary(np.array([0.0, -800.0, -900.0]))  # one draw carries the sum
    assert abs(spike[2] - 1.0) <= 1e-12 and abs(spike[0] + math.log(3.0)) <= 1e-12
    with pytest.raises(ValueError):
        weights_summary(np.zeros((2, 0)))


def test_marginal_loglik_refuses_missing_and_bad_sample_counts_before_any_device_call(monkeypatch):
    from vlgp_amd import engine, evaluation

    monkeypatch.setattr(engine.Engine, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device call")))
    config = {"method": "VB", "max_iter": 3, "dmu_bound": 5.0}
    with pytest.raises(ValueError, match="missing"):
        evaluation.marginal_loglik([{"y": np.zeros((9, 4)), "missing": np.zeros((9, 4), bool)}], {"zdim": 2}, config)
    for K in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="n_samples"):
            evaluation.marginal_loglik([{"y": np.zeros((9, 4))}], {"zdim": 2, "rank": 50}, config, n_samples=K)


def test_header_binding_and_library_name_vlgp_marginal():
    import vlgp_amd
    from vlgp_amd import _lib, evaluation, model_selection

    text = open(HEADER).read()
    proto = re.search(r"int vlgp_marginal\(vlgp_ctx\* ctx, int set, int vb, int n_samples, const double\* eps,\s+"
                      r"double\* log_w,\s+double\* parts,\s+int\* n_failed\);", text)
    assert proto
    block = text.index("/* ---- held-out evaluation ------")
    assert block < text.index("int vlgp_forecast(") < proto.start() < text.index("/* ---- parameters ------")
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"\bint (vlgp_[a-z_0-9]+)\s*\(", plain)[-1] == "vlgp_replicate_groups"
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3 and _lib.ABI_VERSION == 3
    assert "vlgp_marginal" in _lib.EXPORTS
    assert len(_lib._SIGNATURES["vlgp_marginal"][1]) == 8
    lib = _lib.load()  # (raises ImportError, naming the symbol, on a library built from an older tree)
    assert hasattr(lib, "vlgp_marginal") and lib.vlgp_abi_version() == 3
    assert "marginal_loglik" in evaluation.__all__ and "weights_summary" in evaluation.__all__
    assert callable(evaluation.marginal_loglik) and hasattr(vlgp_amd.Engine, "marginal")
    assert "marginal_bps" in model_selection.cross_validate.__doc__
