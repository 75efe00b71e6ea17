"""What the GPU tests of the held-out evaluation share (tests/test_gpu_evaluation.py, tests/test_gpu_cosmoothing.py):
their seeded problems and the NumPy restatement of leave-group-out prediction -- the oracle's E-step with the group's
loadings zeroed from a zero start, then every channel of the group predicted with its own loading and scored with the
definitions of vlgp_amd/evaluation.py.  Leave-one-out is the same with singleton groups."""
import numpy as np
from scipy.special import gammaln

from oracle import vlgp_oracle as O

STAGE = 1e-9  # the tolerance of one restated stage


def lagged(y, history):
    """x (T, 1 + history, N): a column of ones, then each channel's own values 1 ... history bins back."""
    T, N = y.shape
    x = np.ones((T, 1 + history, N))
    for h in range(1, history + 1):
        x[h:, h, :] = y[:-h]
        x[:h, h, :] = 0.0
    return x


def problem(seed=3, M=6, T=150, N=14, L=3, n_gauss=0, lengths=None, history=0, method="VB", max_iter=4):
    from vlgp_amd import get_config, synth

    trials = synth.make_trials(M, T, N, min(L, 3), seed=seed, n_gauss=n_gauss, lengths=lengths)
    rng = np.random.default_rng(seed)
    for tr in trials:
        tr["x"] = lagged(tr["y"], history)
    P = 1 + history
    y = np.concatenate([tr["y"] for tr in trials])
    b = np.zeros((P, N))
    b[0] = np.log(np.maximum(y.mean(0), 1e-3))
    b[0, N - n_gauss:] = y[:, N - n_gauss:].mean(0) if n_gauss else b[0, N - n_gauss:]
    if history:
        b[1:] = -0.05 * rng.random((history, N))
    a = 0.3 * rng.standard_normal((L, N))
    if L > 10:  # (as test_gpu_parity's problems: eta = mu a in the range of the few-latent cases -- the E-step's Newton
        a *= 5.0 / L  # sweeps amplify rounding once rates grow, and the stage tolerance is about arithmetic, not conditioning)
    lik = np.array(["poisson"] * (N - n_gauss) + ["gaussian"] * n_gauss)
    noise = np.ones(N)
    noise[N - n_gauss:] = 0.5 + rng.random(n_gauss)
    omega = np.linspace(2e-2, 1e-3, L)
    params = {"ydim": N, "zdim": L, "xdim": P, "a": a, "b": b, "noise": noise, "omega": omega,
              "sigma": np.ones(L), "rank": 50, "likelihood": lik}
    return trials, params, get_config(max_iter=max_iter, method=method)


def rate_ll(y, x, mu, v, a, b, noise, gauss, vb):
    """Plug-in rate (Gaussian: eta) and log-likelihood, (T, N) each."""
    eta = O.linear_predictor(x, mu, a, b)
    lam = np.exp(np.minimum(eta + (0.5 * (v @ a ** 2) if vb else 0.0), 10.0))
    llp = y * np.log(lam) - lam - gammaln(y + 1.0)
    llg = -0.5 * np.log(2 * np.pi * noise) - (y - eta) ** 2 / (2 * noise)
    return np.where(gauss, eta, lam), np.where(gauss, llg, llp)


def restated(trials, params, config, groups, n_iter=None):
    """Per trial (T, n_pairs) rates and per pair ll, pairs in the order of the concatenated groups."""
    a, b, noise = params["a"], params["b"], params["noise"]
    L = params["zdim"]
    gauss = np.asarray(params["likelihood"]) == "gaussian"
    vb = config["method"] == "VB"
    n_iter = config["max_iter"] if n_iter is None else n_iter
    rates, lls = [], np.zeros(sum(len(g) for g in groups))
    for tr in trials:
        T = tr["y"].shape[0]
        G = O.build_prior([T], params["omega"], params["sigma"], 50)[T]
        cols, i = [], 0
        for g in groups:
            a0 = a.copy()
            a0[:, g] = 0.0
            z = np.zeros((T, L))
            mu, v, _, _, _ = O.estep_unit(tr["y"], tr["x"], z, z, z, a0, b, noise, gauss, G, n_iter,
                                          config["dmu_bound"], vb)
            r, ll = rate_ll(tr["y"], tr["x"], mu, v, a, b, noise, gauss, vb)
            for n in g:
                cols.append(r[:, n])
                lls[i] += ll[:, n].sum()
                i += 1
        rates.append(np.stack(cols, axis=1))
    return rates, lls
