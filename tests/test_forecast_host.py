"""Forward prediction, CPU side: the NumPy restatement of its definitions (tests/forecast_numpy.py) against the oracle's
E-step and variance update, and the pieces of the feature that need no device."""
import os
import re

import numpy as np
import pytest

import forecast_numpy as FN
from conftest import ROOT, relerr
from oracle import vlgp_oracle as O

STAGE = 1e-9
HEADER = os.path.join(ROOT, "include", "vlgp_hip.h")


@pytest.fixture(scope="module")
def converged():
    """One unit of T_in = 110 rows (a factor of length 120 cut to its first 110), N = 40, L = 2, after 60 oracle
    sweeps from zero, and the (unclipped) step of a 61st sweep."""
    T, nf, N, L = 120, 10, 40, 2
    omega = np.array([2e-3, 5e-3])
    rng = np.random.default_rng(0)
    full = O.build_prior([T], omega, np.ones(L), 50)[T]
    G_in, G_ext = np.ascontiguousarray(full[:, :T - nf]), np.ascontiguousarray(full[:, T - nf:])
    t = np.arange(T)
    lat = np.stack([np.linalg.cholesky(np.exp(-om * (t[:, None] - t[None, :]) ** 2) + 1e-8 * np.eye(T))
                    @ rng.standard_normal(T) for om in omega], axis=1)
    a = 0.8 * rng.standard_normal((L, N))
    b = np.log(0.3) + 0.3 * rng.standard_normal((1, N))
    y = rng.poisson(np.exp(lat @ a + b)).astype(float)[:T - nf]
    gauss, noise = np.zeros(N, bool), np.ones(N)
    x = np.ones((T - nf, 1, N))
    zero = np.zeros((T - nf, L))
    mu, v, w, _, bad = O.estep_unit(y, x, zero, zero, zero, a, b, noise, gauss, G_in, 60)
    assert bad == 0
    step = O.estep_unit(y, x, mu, v, w, a, b, noise, gauss, G_in, 1, dmu_bound=1e300)[3]
    unit = {"y": y, "x": x, "mu": mu, "v": v, "w": w}
    return unit, a, b, noise, gauss, G_in, G_ext, step


def test_restatement_meets_the_oracle_at_its_fixed_point(converged):
    """beta_hat = G'g and G beta_hat = mu once the E-step has converged.  The gap has a closed form: with u = G G'g - mu
    and the oracle's unclipped step = (I + G G'W)^-1 u, beta_hat - G'g = S G'W (mu - G G'g) = -G'(w o step) (push-through),
    and G beta_hat = mu + step.  So the bounds are the oracle's own next step carried through those two identities, plus
    STAGE for the rounding of the two solves; and that step itself must be at rounding level (1e-8 of |mu|: sixty Newton
    sweeps from zero, measured 1e-9 ... 1e-10)."""
    unit, a, b, noise, gauss, G_in, G_ext, step = converged
    g = FN.gradient(unit["y"], unit["x"], unit["mu"], unit["v"], a, b, noise, gauss)
    _, _, terms, betas, _ = FN.forecast_unit(unit, a, b, noise, gauss, G_in, G_ext)
    for l in range(2):
        G = G_in[l][:, :FN.rank(G_in[l])]
        fixed = G.T @ g[:, l]
        gap = np.abs(betas[l] - fixed).max()
        bound = np.abs(G.T @ (unit["w"][:, l] * step[:, l])).max() + STAGE * np.abs(fixed).max()
        print("latent %d: |beta - G'g| %.2e (bound %.2e, |beta| %.2e), |G beta - mu| rel %.2e, off_fixed_point %.2e" % (
            l, gap, bound, np.abs(fixed).max(), relerr(G @ betas[l], unit["mu"][:, l]), terms[l, 0] / terms[l, 1]))
        assert gap <= bound
        assert gap <= 1e-8 * np.abs(fixed).max()
        assert np.abs(G @ betas[l] - unit["mu"][:, l]).max() <= np.abs(step[:, l]).max() + STAGE * np.abs(unit["mu"][:, l]).max()
        assert terms[l, 0] / terms[l, 1] <= 1e-16  # (the square of 1e-8)


def test_restatement_variance_on_the_held_in_rows_is_the_oracles(converged):
    """With G_ext := G the variance of the extension is diag(G S G'): oracle.variance_unit, at STAGE."""
    unit, a, b, noise, gauss, G_in, _, _ = converged
    want, bad = O.variance_unit(unit["w"], unit["v"], G_in)
    assert bad == 0
    _, v_ext, _, _, _ = FN.forecast_unit(unit, a, b, noise, gauss, G_in, G_in)
    err = relerr(v_ext, want)
    print("v on the held-in rows: %.2e" % err)
    assert err <= STAGE


def test_without_data_the_extension_is_the_prior():
    """w = 0 and z = 0: beta_hat = 0 and H = I, so mu_ext = 0 and v_ext is the squared row norm of G_ext (the prior
    variance of those bins), columns beyond the held-in rank included."""
    full = O.build_prior([60], np.array([5e-3]), np.ones(1), 50)[60][0].copy()
    full[45:, FN.rank(full)] = np.linspace(0.1, 0.5, 15)  # (a column the held-in rows do not have)
    G_in, G_ext = full[:45], full[45:]
    r = FN.rank(G_in)
    assert r < FN.rank(full)
    zero = np.zeros(45)
    mu_ext, v_ext, terms, beta, _ = FN.extend(G_in, G_ext, zero, zero, zero)
    assert np.array_equal(mu_ext, np.zeros(15)) and np.array_equal(beta, np.zeros(r))
    assert np.max(np.abs(v_ext - np.sum(G_ext ** 2, axis=1))) <= 1e-15 * np.max(v_ext)
    assert np.array_equal(terms, np.zeros(2))
    assert np.array_equal(FN.extend(G_in, G_ext, zero, zero, zero, vb=False)[1], np.zeros(15))


@pytest.mark.parametrize("n_forward", [0, -3, 20, 25, 2.0, "3", None, True])
def test_forward_prediction_refuses_a_bad_horizon_before_any_device_call(monkeypatch, n_forward):
    from vlgp_amd import engine, evaluation

    def no_device(*args, **kw):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(engine.Engine, "__init__", no_device)
    trials = [{"y": np.zeros((30, 4))}, {"y": np.zeros((20, 4))}]
    before = [t["y"].copy() for t in trials]
    with pytest.raises(ValueError, match="n_forward"):
        evaluation.forward_prediction(trials, {"zdim": 2}, {"method": "VB", "max_iter": 5, "dmu_bound": 5.0}, n_forward)
    assert all(np.array_equal(t["y"], y0) for t, y0 in zip(trials, before))


def test_forecast_refuses_a_bad_horizon_before_any_device_call(monkeypatch):
    import vlgp_amd
    from vlgp_amd import engine

    monkeypatch.setattr(engine.Engine, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device call")))
    for n_ahead in (0, -1, 1.5, None):
        with pytest.raises(ValueError, match="n_ahead"):
            vlgp_amd.forecast([{"y": np.zeros((30, 4))}], {"zdim": 2}, {"method": "VB"}, n_ahead)


def test_header_binding_and_library_name_vlgp_forecast():
    import vlgp_amd
    from vlgp_amd import _lib, evaluation

    text = open(HEADER).read()
    proto = ("int vlgp_forecast(vlgp_ctx* ctx, int set, int vb, int n_lengths, const int* lengths, const int* n_ext,\n"
             "                  const double* G_ext, double* mu_ext, double* v_ext, double* fit_terms, int* n_failed);")
    assert proto in text
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3 and _lib.ABI_VERSION == 3
    assert "vlgp_forecast" in _lib.EXPORTS
    assert len(_lib._SIGNATURES["vlgp_forecast"][1]) == 11
    lib = _lib.load()  # (raises ImportError, naming the symbol, on a library built from an older tree)
    assert hasattr(lib, "vlgp_forecast") and lib.vlgp_abi_version() == 3
    assert "forward_prediction" in evaluation.__all__ and callable(vlgp_amd.forecast)
    assert hasattr(vlgp_amd.Engine, "forecast")
