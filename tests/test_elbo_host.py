"""The variational lower bound, host side: the NumPy statement of its definition (tests/elbo_numpy.py) against the dense
textbook formula and against the real reference's stored fit, the host assembly evaluation.elbo_from_terms, and the C
ABI's declaration and binding of vlgp_elbo."""
import math
import os
import re

import numpy as np
import pytest

import elbo_numpy as EN
from conftest import GOLDEN, ROOT


def test_low_rank_kl_equals_the_dense_formula_at_full_rank():
    """T = 12 bins, G the full Cholesky factor of K = SE kernel + 1e-9 I: 1/2 (tr S + beta'beta - r + log det H) equals
    1/2 [tr(K^-1 Sigma) + mu' K^-1 mu - T + log|K| - log|Sigma|] with Sigma = (K^-1 + W)^-1 = G S G'.  1e-7: the size of
    the jitter's own effect on the value (measured when the definition was written: 7.14935133 against 7.14935131)."""
    rng = np.random.default_rng(0)
    T = 12
    t = np.arange(T, dtype=float)
    K = np.exp(-0.05 * (t[:, None] - t[None, :]) ** 2) + 1e-9 * np.eye(T)
    G = np.linalg.cholesky(K)
    w = rng.uniform(0.1, 2.0, T)
    mu = G @ rng.standard_normal(T)
    terms = EN.kl_terms(G, w, mu)
    assert terms[4] == T
    assert terms[3] <= 1e-20 * float(mu @ mu)
    low = EN.kl_from_terms(terms)
    Kinv = np.linalg.inv(K)
    Sigma = np.linalg.inv(Kinv + np.diag(w))
    dense = 0.5 * (np.trace(Kinv @ Sigma) + mu @ Kinv @ mu - T + np.linalg.slogdet(K)[1] - np.linalg.slogdet(Sigma)[1])
    assert abs(low - dense) <= 1e-7 * abs(dense), (low, dense)
    assert low > 0.0


def test_definition_fits_the_reference_fit():
    """tests/golden/ref_result.npy is a fit of the real reference: its mu lies in the range of its prior factor
    (off_prior <= 1e-24) and diag(G S G') is the v it stored (1e-12), for every trial and latent."""
    from vlgp_amd import util as U

    res = U.load(os.path.join(GOLDEN, "ref_result.npy"))
    chol = res["params"]["cholesky"]
    worst_off, worst_v = 0.0, 0.0
    for tr in res["trials"]:
        T = tr["y"].shape[0]
        for l in range(res["params"]["zdim"]):
            G = EN.compact(np.asarray(chol[T][l]))
            w, mu = tr["w"][:, l], tr["mu"][:, l]
            _, _, _, resid, r = EN.kl_terms(G, w, mu)
            off = resid / max(float(mu @ mu), np.finfo(float).tiny)
            S = np.linalg.inv(np.eye(r) + G.T @ (w[:, None] * G))
            worst_off = max(worst_off, off)
            worst_v = max(worst_v, float(np.max(np.abs(np.einsum("tr,rs,ts->t", G, S, G) - tr["v"][:, l]))))
            assert EN.kl_from_terms(EN.kl_terms(G, w, mu)) > 0.0
    assert worst_off <= 1e-24, worst_off
    assert worst_v <= 1e-12, worst_v


def _terms_problem(seed=1, units=5, L=3, N=7, pad=0):
    """Random units with full-column-rank factors (optionally `pad` all-zero columns appended) and their statement."""
    rng = np.random.default_rng(seed)
    lengths = [20, 30, 20, 25, 30][:units]
    R = 6 + pad
    chol = {}
    for T in sorted(set(lengths)):
        G = np.zeros((L, T, R))
        for l in range(L):
            G[l, :, :4 + (l % 3)] = rng.standard_normal((T, 4 + (l % 3))) / np.sqrt(T)
        chol[T] = G
    gauss = np.zeros(N, bool)
    gauss[-2:] = True
    a = 0.3 * rng.standard_normal((L, N))
    b = 0.2 * rng.standard_normal((1, N))
    noise = 0.5 + rng.random(N)
    us = []
    for T in lengths:
        y = rng.poisson(1.0, size=(T, N)).astype(float)
        y[:, gauss] = rng.standard_normal((T, 2))
        us.append({"y": y, "x": None, "mu": 0.4 * rng.standard_normal((T, L)), "v": 0.05 * rng.random((T, L)),
                   "w": rng.uniform(0.1, 2.0, (T, L))})
    return us, a, b, noise, gauss, chol, lengths


def test_elbo_from_terms_totals_and_per_trial_split():
    from vlgp_amd.evaluation import elbo_from_terms

    us, a, b, noise, gauss, chol, lengths = _terms_problem()
    st = EN.statement(us, a, b, noise, gauss, chol, vb=True)
    off = np.concatenate([[0], np.cumsum(lengths)])
    out = elbo_from_terms(st["row_sums"], st["terms"], st["ranks"], vb=True, n_failed=0, mu_sq=st["mu_sq"],
                          row_ell=st["row_ell"], offsets=off)
    ell = st["row_sums"][:, 0].sum()
    assert out["ell"] == pytest.approx(ell, rel=1e-13)
    assert np.allclose(out["kl"], st["kl"], rtol=1e-13, atol=0.0)
    assert out["elbo"] == pytest.approx(ell - st["kl"].sum(), rel=1e-12)
    assert np.array_equal(out["ell_per_channel"], st["row_sums"][:, 0])
    assert out["kl"].shape == (len(us), a.shape[0]) and out["off_prior"].shape == out["kl"].shape
    assert np.allclose(out["off_prior"], st["terms"][:, :, 3] / st["mu_sq"], rtol=1e-13)
    assert np.all(out["off_prior"] > 1e-3)  # (a random mu is NOT in the range of G: reported, not hidden)
    assert out["n_failed"] == 0 and "log_joint" not in out
    per = out["elbo_per_trial"]
    assert per.shape == (len(us),)
    for i in range(len(us)):
        want = st["row_ell"][off[i]:off[i + 1]].sum() - st["kl"][i].sum()
        assert per[i] == pytest.approx(want, rel=1e-12)
    assert per.sum() == pytest.approx(out["elbo"], rel=1e-12)
    assert "elbo_per_trial" not in elbo_from_terms(st["row_sums"], st["terms"], st["ranks"])


def test_kl_does_not_depend_on_dropped_zero_columns():
    """A factor that keeps k all-zero columns has H = diag(H_r, I_k): tr S and r both grow by k, log det H and the
    minimum-norm beta do not change."""
    from vlgp_amd.evaluation import elbo_from_terms

    us, a, b, noise, gauss, chol, _ = _terms_problem(pad=3)
    st = EN.statement(us, a, b, noise, gauss, chol)
    L = a.shape[0]
    terms = np.empty_like(st["terms"])
    ranks = np.empty_like(st["ranks"])
    for i, u in enumerate(us):
        for l in range(L):
            t = EN.kl_terms(chol[u["y"].shape[0]][l], u["w"][:, l], u["mu"][:, l])  # zero columns kept
            terms[i, l], ranks[i, l] = t[:4], t[4]
    assert np.all(ranks == st["ranks"] + np.array([[2 + 3 - (l % 3) for l in range(L)]]))
    kept = elbo_from_terms(st["row_sums"], terms, ranks)
    dropped = elbo_from_terms(st["row_sums"], st["terms"], st["ranks"])
    assert np.allclose(kept["kl"], dropped["kl"], rtol=1e-12, atol=0.0)
    assert kept["elbo"] == pytest.approx(dropped["elbo"], rel=1e-12)


def test_elbo_from_terms_map_reports_the_log_joint():
    from vlgp_amd.evaluation import elbo_from_terms

    us, a, b, noise, gauss, chol, lengths = _terms_problem(seed=2)
    for u in us:
        u["v"] = np.zeros_like(u["v"])
    st = EN.statement(us, a, b, noise, gauss, chol, vb=False)
    off = np.concatenate([[0], np.cumsum(lengths)])
    out = elbo_from_terms(st["row_sums"], st["terms"], st["ranks"], vb=False, row_ell=st["row_ell"], offsets=off)
    assert math.isnan(out["elbo"]) and np.all(np.isnan(out["kl"])) and out["kl"].shape == st["kl"].shape
    ell = st["row_sums"][:, 0].sum()
    assert out["ell"] == pytest.approx(ell, rel=1e-13)
    assert out["log_joint"] == pytest.approx(ell - 0.5 * st["terms"][:, :, 2].sum(), rel=1e-12)
    assert "elbo_per_trial" not in out
    assert out["log_joint_per_trial"].sum() == pytest.approx(out["log_joint"], rel=1e-12)


def test_elbo_from_terms_counts_and_propagates_failures():
    from vlgp_amd.evaluation import elbo_from_terms

    us, a, b, noise, gauss, chol, lengths = _terms_problem(seed=3)
    st = EN.statement(us, a, b, noise, gauss, chol)
    terms = st["terms"].copy()
    terms[1, 2] = np.nan  # what the device leaves for a pair whose pivot was not positive
    off = np.concatenate([[0], np.cumsum(lengths)])
    out = elbo_from_terms(st["row_sums"], terms, st["ranks"], n_failed=1, mu_sq=st["mu_sq"], row_ell=st["row_ell"],
                          offsets=off)
    assert out["n_failed"] == 1
    assert math.isnan(out["kl"][1, 2]) and np.isnan(out["kl"]).sum() == 1
    assert math.isnan(out["elbo"]) and not math.isnan(out["ell"])
    assert math.isnan(out["elbo_per_trial"][1]) and np.isnan(out["elbo_per_trial"]).sum() == 1
    assert math.isnan(out["off_prior"][1, 2])
    with pytest.raises(ValueError):
        elbo_from_terms(st["row_sums"], terms, st["ranks"][:, :2])


def test_header_declares_and_binding_binds_vlgp_elbo():
    from vlgp_amd import _lib

    text = open(os.path.join(ROOT, "include", "vlgp_hip.h")).read()
    assert re.search(r"int vlgp_elbo\(vlgp_ctx\* ctx, int set, int vb, double\* row_sums, double\* row_ell, "
                     r"double\* kl_terms, int\* n_failed\);", text)
    assert "vlgp_elbo" in _lib.EXPORTS
    assert len(_lib._SIGNATURES["vlgp_elbo"][1]) == 7


def test_elbo_is_exported_and_fit_takes_track_elbo():
    import inspect

    import vlgp_amd
    from vlgp_amd.api import FitSession

    assert hasattr(vlgp_amd.evaluation, "elbo") and hasattr(vlgp_amd.evaluation, "elbo_from_terms")
    for fn in (vlgp_amd.fit, FitSession.__init__):
        assert inspect.signature(fn).parameters["track_elbo"].default is False
