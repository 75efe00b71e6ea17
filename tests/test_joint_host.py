"""The NumPy statement of the joint Laplace posterior (tests/joint_numpy.py) held to closed forms, and the argument
checks of the Python functions built on vlgp_joint_laplace.  No GPU.

STAGE = 1e-9 is the project's stage-wise tolerance, taken relative to the sum of absolute terms.
"""
import inspect

import numpy as np
import pytest
from scipy.stats import multivariate_normal, norm

import joint_numpy as JN
from oracle import vlgp_oracle as O

STAGE = 1e-9
R = 50


def shared_gaussian_problem(seed=7, M=3, T=24, L=3, N=6):
    """All-Gaussian channels with SHARED loadings (every channel loads on every latent): the model is jointly Gaussian but
    the latents are coupled through the loadings, so the posterior of beta is the Gaussian N(beta_hat, H^-1) and no
    mean-field posterior equals it.  Returns the units (random mu, v; w the model's own diagonal curvature), a, b, noise,
    gauss, the prior and the dense closed form log N(y; b, sum_l (a_l a_l') (x) G_l G_l' + diag(noise) (x) I) per unit."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.4, 1.2, (L, N)) * rng.choice([-1.0, 1.0], (L, N))
    b = rng.standard_normal((1, N))
    noise = 0.5 + rng.random(N)
    gauss = np.ones(N, bool)
    prior = O.build_prior([T], np.array([2e-2, 5e-3, 1e-3])[:L], np.ones(L), R)
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


def poisson_problem(seed, T=60, L=3, N=12):
    """One Poisson unit: a ~ 0.5 N(0, 1), b = -1, latents drawn from the prior; a zero mean-field start."""
    rng = np.random.default_rng(seed)
    a = 0.5 * rng.standard_normal((L, N))
    b = -np.ones((1, N))
    prior = O.build_prior([T], np.array([2e-2, 5e-3, 1e-3])[:L], np.ones(L), R)
    lat = np.stack([prior[T][l] @ rng.standard_normal(R) for l in range(L)], axis=1)
    y = rng.poisson(np.exp(lat @ a + b)).astype(float)
    unit = {"y": y, "x": None, "mu": np.zeros((T, L)), "v": np.zeros((T, L)), "w": np.ones((T, L))}
    return unit, a, b, np.ones(N), np.zeros(N, bool), prior


def test_gaussian_shared_loadings_laplace_and_every_weight_are_the_closed_form():
    units, a, b, noise, gauss, prior, closed = shared_gaussian_problem()
    eps = np.random.default_rng(1).standard_normal((len(units), 3, R, 9))
    st = JN.statement(units, a, b, noise, gauss, prior, eps)
    for s, want in zip(st, closed):
        assert s["converged"]
        assert abs(s["laplace"] - want) <= STAGE * abs(want), (s["laplace"], want)
        assert np.max(np.abs(s["log_w"] - want)) <= STAGE * abs(want)
        assert np.ptp(s["log_w"]) <= STAGE * abs(want)
        assert np.array_equal(s["ll_k"] + s["c_k"], s["log_w"])


def test_gradient_and_hessian_by_finite_differences():
    unit, a, b, noise, gauss, prior = poisson_problem(3, T=20, L=2, N=5)
    gauss = np.array([0, 0, 0, 1, 1], bool)
    noise = np.array([1.0, 1.0, 1.0, 0.7, 1.3])
    U = JN.Unit(unit, a, b, noise, gauss, prior[20])
    rng = np.random.default_rng(0)
    beta = 0.3 * rng.standard_normal(U.D)
    g, H = U.grad(beta), U.hessian(beta)
    h = 1e-5
    for i in rng.choice(U.D, 6, replace=False):
        e = np.zeros(U.D)
        e[i] = h
        fd = (U.f(beta + e) - U.f(beta - e)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i])), (i, fd, g[i])
        fdH = (U.grad(beta + e) - U.grad(beta - e)) / (2 * h)
        assert np.max(np.abs(fdH - H[:, i])) <= 1e-6 * max(1.0, np.max(np.abs(H[:, i]))), i
    assert np.allclose(H, H.T, rtol=0, atol=1e-12 * np.max(np.abs(H)))
    blocks = U.res_cur(beta)[1] @ (a ** 2).T  # the engine's own w at these paths
    for l in range(U.L):
        sl = slice(U.start[l], U.start[l + 1])
        want = np.eye(U.ranks[l]) + U.G[l].T @ (blocks[:, l, None] * U.G[l])
        assert np.max(np.abs(H[sl, sl] - want)) <= 1e-12 * np.max(np.abs(want))


def test_c_is_the_log_ratio_of_prior_and_proposal_densities():
    unit, a, b, noise, gauss, prior = poisson_problem(5, T=30)
    U = JN.Unit(unit, a, b, noise, gauss, prior[30])
    beta, _, _, conv = JN.newton(U, np.zeros(U.D))
    s = JN.summary(U, beta)
    eps = np.random.default_rng(2).standard_normal((3, R, 7))
    _, _, c, _, bk = JN.draws(U, beta, s["Lc"], eps)
    cov = np.linalg.inv(s["H"])
    for k in range(7):
        want = norm.logpdf(bk[:, k]).sum() - multivariate_normal.logpdf(bk[:, k], beta, cov)
        assert abs(c[k] - want) <= 1e-8 * max(1.0, abs(want)), (k, c[k], want)
    assert conv and np.max(np.abs(U.grad(beta))) <= 1e-8


SEED_ESS = 1  # (chosen on the CPU before it was committed: the printed margins)


def test_joint_proposal_keeps_the_sample_size_the_block_diagonal_one_loses():
    """T = 60, L = 3, N = 12 Poisson, 256 draws, both proposals centred at the joint mode: N(beta_hat, H^-1) against the
    block-diagonal of the same H (the best case for a mean-field proposal)."""
    from vlgp_amd.evaluation import weights_summary

    unit, a, b, noise, gauss, prior = poisson_problem(SEED_ESS)
    U = JN.Unit(unit, a, b, noise, gauss, prior[60])
    beta, _, _, conv = JN.newton(U, np.zeros(U.D))
    s = JN.summary(U, beta)
    eps = np.random.default_rng(11).standard_normal((3, R, 256))
    log_w = JN.draws(U, beta, s["Lc"], eps)[0]
    Hb = np.zeros_like(s["H"])
    for l in range(U.L):
        sl = slice(U.start[l], U.start[l + 1])
        Hb[sl, sl] = s["H"][sl, sl]
    Lb = np.linalg.cholesky(Hb)
    log_wb = JN.draws(U, beta, Lb, eps)[0]
    iwae, _, ess = weights_summary(log_w)
    iwae_b, _, ess_b = weights_summary(log_wb)
    print("ESS of 256: joint %.1f, block-diagonal %.1f; laplace %.3f, joint iwae %.3f, block iwae %.3f"
          % (ess, ess_b, s["laplace"], iwae, iwae_b))
    assert conv and ess > ess_b  # (at the committed seed: 224 against 79)
    assert ess > 128.0  # a proposal that is the posterior up to its non-Gaussian remainder keeps most of its draws
    assert abs(s["laplace"] - iwae) < 0.5


def test_python_argument_checks_and_exports():
    import vlgp_amd
    from vlgp_amd import _lib, evaluation
    from vlgp_amd.model_selection import cross_validate

    assert "vlgp_joint_laplace" in _lib.EXPORTS and len(_lib._SIGNATURES["vlgp_joint_laplace"][1]) == 13
    lib = _lib.load()
    assert hasattr(lib, "vlgp_joint_laplace") and lib.vlgp_abi_version() == 3
    assert "joint_posterior" in evaluation.__all__ and callable(evaluation.joint_posterior)
    assert callable(vlgp_amd.Engine.joint_laplace)
    sig = inspect.signature(evaluation.marginal_loglik)
    assert sig.parameters["proposal"].default == "posterior"
    assert inspect.signature(cross_validate).parameters["proposal"].default == "posterior"
    sig = inspect.signature(evaluation.joint_posterior)
    assert sig.parameters["max_iter"].default == 50 and sig.parameters["tol"].default == 1e-10
    trials = [{"y": np.zeros((5, 3))}]
    params = {"zdim": 1, "rank": 5, "ydim": 3}
    config = {"method": "VB", "max_iter": 2, "dmu_bound": 1.0}
    with pytest.raises(ValueError, match="proposal must be"):
        evaluation.marginal_loglik(trials, params, config, proposal="laplace")
    with pytest.raises(ValueError, match="proposal must be"):
        cross_validate(trials, [1], score="marginal_bps", proposal="both")
    with pytest.raises(ValueError, match="applies to score='marginal_bps'"):
        cross_validate(trials, [1], score="co_bps", proposal="joint")
    holes = [dict(trials[0], missing=np.zeros((5, 3), bool))]
    with pytest.raises(ValueError):
        evaluation.joint_posterior(holes, params, config)
    with pytest.raises(ValueError):
        evaluation.marginal_loglik(holes, params, config, proposal="joint")
