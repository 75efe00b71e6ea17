"""Residual correlations without a device: the closed forms of the pair moments (tests/pair_numpy.py) against Monte Carlo,
their special cases, the host summaries, the wiring of vlgp_pair_moments through the header, the binding, the admission
table and the public names, the layout of the call's device block under the sanitizers, and a run that shows what the
score is for: a model with a latent removed leaves more excess correlation than the true one."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import calibration_numpy as CN
import pair_numpy as PN
from conftest import ROOT
from oracle import vlgp_oracle as O


def _mixed(rng, T, N, L, P=1):
    """A small mixed problem: Poisson and Gaussian channels interleaved, a full covariance per row."""
    gauss = (np.arange(N) % 2).astype(bool)
    a, b = 0.4 * rng.standard_normal((L, N)), 0.3 * rng.standard_normal((P, N))
    noise = 0.5 + rng.random(N)
    x = np.concatenate([np.ones((T, 1, N)), 0.2 * rng.standard_normal((T, P - 1, N))], axis=1)
    mu = 0.5 * rng.standard_normal((T, L))
    B = 0.3 * rng.standard_normal((T, L, L))
    cov = B @ B.transpose(0, 2, 1) + 0.02 * np.eye(L)
    m = mu @ a + np.einsum("tpn,pn->tn", x, b)
    y = np.where(gauss, m + rng.standard_normal((T, N)), rng.poisson(np.exp(m)).astype(float))
    return dict(y=y, x=x, mu=mu, cov=cov, a=a, b=b, noise=noise, gauss=gauss)


def test_the_closed_forms_against_monte_carlo():
    """E[d d'] of joint draws (latents from N(mu, C), counts and Gaussian observations from the latents) against K for one
    row: L = 3, two Poisson and two Gaussian channels, a full C, mixed pairs included, every entry within 5 standard
    errors (400 000 draws; at 2 000 000 the worst entry was 2.14 standard errors off)."""
    rng = np.random.default_rng(0)
    L, N, S = 3, 4, 400_000
    gauss = np.array([False, True, False, True])
    a, b, noise = 0.6 * rng.standard_normal((L, N)), 0.4 * rng.standard_normal((1, N)), np.array([1.0, 0.7, 1.0, 1.3])
    mu = 0.5 * rng.standard_normal((1, L))
    B = 0.5 * rng.standard_normal((L, L))
    C = (B @ B.T + 0.05 * np.eye(L))[None]
    z = mu[0] + rng.standard_normal((S, L)) @ np.linalg.cholesky(C[0]).T
    eta = z @ a + b[0]
    y = np.where(gauss, eta + np.sqrt(noise) * rng.standard_normal((S, N)), rng.poisson(np.exp(eta)).astype(float))
    d0, K = PN.row_terms(np.zeros((1, N)), np.ones((1, 1, N)), mu, C, a, b, noise, gauss)
    d = y - (0.0 - d0[0])  # (y - e: d0 = 0 - e)
    prod = d[:, :, None] * d[:, None, :]
    mean, se = prod.mean(axis=0), prod.std(axis=0) / np.sqrt(S)
    zscore = np.abs(mean - K[0]) / se
    print("measured pair closed forms against Monte Carlo: worst |z| %.2f over %d entries" % (zscore.max(), N * N))
    assert np.abs(d.mean(axis=0) / (d.std(axis=0) / np.sqrt(S))).max() <= 5.0  # (the predictive mean itself)
    assert zscore.max() <= 5.0, zscore


def test_a_point_posterior_has_no_pair_covariance():
    """cov = 0 (MAP, vb = 0): off-diagonal model exactly 0.0, diag(model) = sum of the rates for a Poisson channel and
    rows x noise for a Gaussian one."""
    p = _mixed(np.random.default_rng(1), 30, 6, 2)
    resid, model, count = PN.pair_moments(p["y"], p["x"], p["mu"], np.zeros_like(p["cov"]), p["a"], p["b"], p["noise"],
                                          p["gauss"])
    off = ~np.eye(6, dtype=bool)
    assert np.all(model[off] == 0.0) and np.all(count == 30)
    lam = np.exp(p["mu"] @ p["a"] + np.einsum("tpn,pn->tn", p["x"], p["b"]))
    assert np.allclose(np.diag(model)[~p["gauss"]], lam.sum(axis=0)[~p["gauss"]], rtol=1e-13, atol=0)
    assert np.allclose(np.diag(model)[p["gauss"]], 30 * p["noise"][p["gauss"]], rtol=1e-13, atol=0)
    assert np.array_equal(resid, resid.T)


def test_a_diagonal_covariance_is_the_mean_field_statement():
    """cov = diag(v): c[n, m] = sum_l a_ln v_l a_lm and s2 = (a ** 2) . v, written out without the covariance."""
    p = _mixed(np.random.default_rng(2), 25, 5, 3, P=2)
    v = 0.1 + 0.3 * np.random.default_rng(3).random((25, 3))
    a, g = p["a"], p["gauss"]
    m = p["mu"] @ a + np.einsum("tpn,pn->tn", p["x"], p["b"])
    s2 = v @ a ** 2
    lam = np.exp(m + 0.5 * s2)
    e, s = np.where(g, m, lam), np.where(g, 1.0, lam)
    want_r, want_m = np.zeros((5, 5)), np.zeros((5, 5))
    for t in range(25):
        for n in range(5):
            for k in range(5):
                c = float(np.sum(a[:, n] * v[t] * a[:, k]))
                f = np.expm1(c) if not (g[n] or g[k]) else c
                want_m[n, k] += s[t, n] * s[t, k] * f + ((p["noise"][n] if g[n] else lam[t, n]) if n == k else 0.0)
                want_r[n, k] += (p["y"][t, n] - e[t, n]) * (p["y"][t, k] - e[t, k])
    resid, model, _ = PN.pair_moments(p["y"], p["x"], p["mu"], PN.diag_cov(v), a, p["b"], p["noise"], g)
    assert np.abs(resid - want_r).max() <= 1e-12 * np.abs(want_r).max()
    assert np.abs(model - want_m).max() <= 1e-12 * np.abs(want_m).max()


def test_live_is_a_selection_and_dead_rows_drop_out():
    p = _mixed(np.random.default_rng(4), 20, 4, 2)
    live = np.random.default_rng(5).random((20, 4)) < 0.6
    y_nan = np.where(live, p["y"], np.nan)
    one = PN.pair_moments(p["y"], p["x"], p["mu"], p["cov"], p["a"], p["b"], p["noise"], p["gauss"], live)
    two = PN.pair_moments(y_nan, p["x"], p["mu"], p["cov"], p["a"], p["b"], p["noise"], p["gauss"], live)
    assert all(np.array_equal(u, w) for u, w in zip(one, two))
    assert np.array_equal(one[2], live.astype(float).T @ live.astype(float))
    mu, cov = p["mu"].copy(), p["cov"].copy()
    mu[3, 1], cov[7, 0, 1] = np.nan, np.inf
    keep = np.ones(20, dtype=bool)
    keep[[3, 7]] = False
    got = PN.pair_moments(p["y"], p["x"], mu, cov, p["a"], p["b"], p["noise"], p["gauss"], live)
    want = PN.pair_moments(p["y"][keep], p["x"][keep], p["mu"][keep], p["cov"][keep], p["a"], p["b"], p["noise"], p["gauss"],
                           live[keep])
    assert all(np.array_equal(u, w) for u, w in zip(got, want))


@pytest.mark.parametrize("gauss", [False, True])
def test_one_channel_against_the_pearson_terms_of_calibration(gauss):
    """model[0, 0] is the sum of calibration's predictive variances and resid[0, 0] the sum of its Pearson numerators, so
    for a single row ``dispersion`` IS calibration's Pearson term.  Over several rows the two differ by definition:
    calibration's dispersion is the mean of the per-entry ratios, this one the ratio of the two sums -- equal only where
    the predictive variance is the same in every row."""
    from vlgp_amd.evaluation import _pair_summary

    rng = np.random.default_rng(6)
    T, L = 12, 2
    a, b, noise, g = 0.5 * rng.standard_normal((L, 1)), rng.standard_normal((1, 1)), np.array([0.8]), np.array([gauss])
    x, mu, v = np.ones((T, 1, 1)), rng.standard_normal((T, L)), 0.2 * rng.random((T, L))
    y = rng.poisson(2.0, (T, 1)).astype(float)
    _, _, mean, var = CN.moments(y, x, mu, v, a, b, noise, g, True)
    resid, model, count = PN.pair_moments(y, x, mu, PN.diag_cov(v), a, b, noise, g)
    assert abs(model[0, 0] - var.sum()) <= 1e-13 * var.sum()
    assert abs(resid[0, 0] - ((y - mean) ** 2).sum()) <= 1e-13 * resid[0, 0]
    for t in range(T):
        r1, m1, c1 = PN.pair_moments(y[t:t + 1], x[t:t + 1], mu[t:t + 1], PN.diag_cov(v[t:t + 1]), a, b, noise, g)
        pearson = (y[t, 0] - mean[t, 0]) ** 2 / var[t, 0]
        assert abs(_pair_summary(r1, m1, c1)["dispersion"][0] - pearson) <= 1e-13 * max(pearson, 1.0)
    out = _pair_summary(resid, model, count)
    assert out["n_pairs"] == 0 and np.isnan(out["rms_excess"])
    if gauss:  # (v constant along the rows: the variance is too, and the two definitions agree)
        v[:] = v[0]
        _, _, mean, var = CN.moments(y, x, mu, v, a, b, noise, g, True)
        out = _pair_summary(*PN.pair_moments(y, x, mu, PN.diag_cov(v), a, b, noise, g))
        assert abs(out["dispersion"][0] - np.mean((y - mean) ** 2 / var)) <= 1e-13


def test_the_summaries_against_their_restatement():
    from vlgp_amd.evaluation import _pair_summary

    p = _mixed(np.random.default_rng(7), 40, 6, 2)
    live = np.zeros((40, 6), dtype=bool)
    live[:, [0, 2, 3]] = True  # (one channel fold: the other pairs are never scored)
    resid, model, count = PN.pair_moments(p["y"], p["x"], p["mu"], p["cov"], p["a"], p["b"], p["noise"], p["gauss"], live)
    got, want = _pair_summary(resid, model, count), PN.summary(resid, model, count)
    assert set(got) == set(want) == {"resid", "model", "count", "residual_corr", "model_corr", "excess_corr", "se_null",
                                     "dispersion", "n_pairs", "rms_excess", "mean_excess"}
    for key in want:
        assert np.allclose(got[key], want[key], rtol=1e-14, atol=0, equal_nan=True), key
    assert got["n_pairs"] == 3 and np.isnan(got["excess_corr"][1, 0]) and np.isnan(got["count"][1, 1])
    assert np.all(got["se_null"][np.ix_([0, 2, 3], [0, 2, 3])] == 1.0 / np.sqrt(40.0))
    assert np.array_equal(np.diag(got["residual_corr"])[[0, 2, 3]], got["dispersion"][[0, 2, 3]])
    nan_count = np.where(count > 0, count, np.nan)  # (NaN and 0 both mean: never scored)
    again = _pair_summary(resid, model, nan_count)
    assert all(np.array_equal(np.asarray(got[k]), np.asarray(again[k]), equal_nan=True) for k in got)
    with pytest.raises(ValueError, match="N, N"):
        _pair_summary(resid[:5], model, count)


def test_header_binding_admission_and_public_names():
    import vlgp_amd
    from vlgp_amd import _lib, evaluation

    header = open(os.path.join(ROOT, "include", "vlgp_hip.h")).read()
    assert "int vlgp_pair_moments(vlgp_ctx* ctx, int set, int vb, double* resid, double* model);" in header
    assert ("int vlgp_pair_moments_cov(vlgp_ctx* ctx, int set, const double* mu, const double* cov, double* resid, "
            "double* model);") in header
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", header).group(1)) == 3 and _lib.ABI_VERSION == 3
    for name, n_args in (("vlgp_pair_moments", 5), ("vlgp_pair_moments_cov", 6)):
        assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name][1]) == n_args
        assert hasattr(_lib.load(), name)
    # the sibling takes mu, cov where vlgp_predictive_cov takes them: after the set, as pointers to double
    assert _lib._SIGNATURES["vlgp_pair_moments_cov"][1][2:4] == _lib._SIGNATURES["vlgp_predictive_cov"][1][5:7]
    api = open(os.path.join(ROOT, "vlgp_amd", "csrc", "api.hip")).read()
    for name in ("vlgp_pair_moments", "vlgp_pair_moments_cov"):
        assert re.search(r"X\(%s, SET_ANY & ~\(SET_COPIED \| SET_GROUPS\),\s*\\\n\s*\"%s on a copied cut: merge it and "
                         r"score the source set\"\)" % (name, name), api), name
    eval_api = open(os.path.join(ROOT, "vlgp_amd", "csrc", "eval_api.hip")).read()
    assert "replicate with held_out=: a pair needs both channels in one replica" in eval_api
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "| `vlgp_pair_moments`, `vlgp_pair_moments_cov` | plain sets, tiling cuts, masked sets (a copied cut: " in design
    assert "pairs.hip" in open(os.path.join(ROOT, "vlgp_amd", "csrc", "Makefile")).read()
    assert "residual_correlation" in evaluation.__all__
    sig = inspect.signature(evaluation.residual_correlation).parameters
    assert list(sig) == ["trials", "params", "config", "how", "groups", "n_folds", "seed", "posterior", "n_iter", "device"]
    assert (sig["how"].default, sig["n_folds"].default, sig["posterior"].default) == ("in_sample", 5, "mean_field")
    assert list(inspect.signature(vlgp_amd.Engine.pair_moments).parameters) == ["self", "set_id", "vb", "mu", "cov"]


def test_residual_correlation_refuses_before_any_device_call():
    from vlgp_amd import evaluation

    params = {"ydim": 3, "zdim": 1}
    with pytest.raises(ValueError, match="how"):
        evaluation.residual_correlation([{"y": np.zeros((10, 3))}], params, {}, how="entries")
    with pytest.raises(ValueError, match="posterior"):
        evaluation.residual_correlation([{"y": np.zeros((10, 3))}], params, {}, posterior="laplace")
    with pytest.raises(ValueError, match="missing"):
        evaluation.residual_correlation([{"y": np.zeros((10, 3)), "missing": np.zeros((10, 3), dtype=bool)}], params, {})
    with pytest.raises(ValueError, match="group"):
        evaluation.residual_correlation([{"y": np.zeros((10, 3))}], params, {}, how="channels", groups=[[0, 1, 2]])


@pytest.fixture(scope="module")
def layout_driver(tmp_path_factory):
    """tests/pair_layout_driver.cpp as a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path_factory.mktemp("pair_layout") / "pair_layout_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vlgp_amd", "csrc"), os.path.join(ROOT, "tests", "pair_layout_driver.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


def _layout(exe, *args):
    done = subprocess.run([exe] + [str(int(v)) for v in args], capture_output=True, timeout=60)
    assert done.returncode == 0, done.stderr.decode(errors="replace")[-3000:]
    return {k: int(v) for k, v in (ln.split(" ") for ln in done.stdout.decode().splitlines())}


@pytest.mark.parametrize("rows, N, n_rep, post_rows, L", [(1, 1, 1, 0, 1), (31, 2, 1, 31, 3), (32, 63, 2, 64, 5),
                                                          (33, 64, 3, 99, 10), (96, 65, 1, 0, 16), (301, 130, 2, 602, 5),
                                                          (40000, 100, 1, 40000, 5), (40000, 100, 5, 0, 5),
                                                          (160000, 1000, 1, 160000, 64), (7, 23104, 1, 0, 2)])
def test_pair_layout(layout_driver, rows, N, n_rep, post_rows, L):
    """The regions lie in order, without overlap, up to ``need``, each as large as the kernels and the copies use it; the
    chunks cover the rows, none is empty, none is shorter than the smallest chunk unless it is the last, and the rule of
    DESIGN 4.19 sizes them: two workgroups per compute unit, the partials within 32 MiB when more than one chunk is cut."""
    n_cu = 256
    got = _layout(layout_driver, rows, N, n_rep, n_cu, post_rows, L)
    tiles = -(-N // 64)
    pairs = tiles * (tiles + 1) // 2
    assert (got["tiles"], got["tile_pairs"], got["min_chunk"]) == (tiles, pairs, 32)
    chunk, n_chunks = got["chunk_rows"], got["n_chunks"]
    assert chunk >= 32 and (n_chunks - 1) * chunk < rows <= n_chunks * chunk
    groups = pairs * n_rep
    want = -(-2 * n_cu // groups)
    cap = max((1 << 22) // (groups * 8192), 1)
    assert chunk == max(32, -(-rows // min(want, cap)))
    if n_chunks > 1:
        assert groups * n_chunks * 8192 * 8 <= 32 << 20 and groups * n_chunks <= 2 * n_cu + groups
    at = 0
    for name, size in (("part", groups * n_chunks * 2 * 64 * 64), ("resid", n_rep * N * N), ("model", n_rep * N * N)):
        assert got[name] == at, (name, got)
        at += size
    assert got["need"] == at
    npair = L * (L + 1) // 2
    assert (got["mu"], got["cov"], got["moments_need"]) == (at, at + post_rows * L, at + post_rows * (L + npair))
    assert got["lds_doubles"] == 3 * 64 * L + L + max(L, npair) + 128 + 128 + 64 and got["lds_doubles"] * 8 <= 160 * 1024


def test_small_sets_take_chunks_of_32_rows(layout_driver):
    """What tests/test_gpu_pair.py relies on for its row counts: below 32 x (chunks wanted) rows a workgroup takes 32."""
    for rows, n_chunks in ((1, 1), (31, 1), (32, 1), (33, 2), (96, 3), (97, 4)):
        for N in (1, 65, 130):
            got = _layout(layout_driver, rows, N, 1, 256, 0, 3)
            assert (got["chunk_rows"], got["n_chunks"]) == (32, n_chunks), (rows, N, got)


def _two_latent_data(seed=0):
    """10 trials x 40 bins x 12 Poisson channels drawn from a two-latent model; the prior factors of its latents."""
    rng = np.random.default_rng(seed)
    n_trials, T, N, L, rank = 10, 40, 12, 2, 20
    omega, sigma = np.array([2e-2, 5e-3]), np.ones(L)
    G = O.build_prior([T], omega, sigma, rank)[T]
    a = rng.standard_normal((L, N)) * np.array([[0.6], [0.4]])
    b = np.full((1, N), 0.8)
    trials = []
    for _ in range(n_trials):
        z = np.stack([G[l] @ rng.standard_normal(rank) for l in range(L)], axis=1)
        trials.append({"y": rng.poisson(np.exp(z @ a + b)).astype(float), "x": np.ones((T, 1, N))})
    return trials, a, b, G


def _oracle_rms_excess(trials, a, b, G, n_iter=30):
    """rms_excess of the trials under the oracle's E-step posterior (from zero) of the model a, b, G."""
    L, N = a.shape
    noise, gauss = np.ones(N), np.zeros(N, dtype=bool)
    mus, vs = [], []
    for tr in trials:
        T = tr["y"].shape[0]
        mu = np.zeros((T, L))
        w = O.curvature_unit(tr["y"], tr["x"], mu, np.zeros((T, L)), a, b, noise, gauss)
        v = O.variance_unit(w, np.zeros((T, L)), G)[0]
        mu, v = O.estep_unit(tr["y"], tr["x"], mu, v, w, a, b, noise, gauss, G, n_iter)[:2]
        mus.append(mu)
        vs.append(v)
    cat = lambda k: np.concatenate([tr[k] for tr in trials])
    resid, model, count = PN.pair_moments(cat("y"), cat("x"), np.concatenate(mus), PN.diag_cov(np.concatenate(vs)), a, b,
                                          noise, gauss)
    return PN.summary(resid, model, count)


def test_a_missing_latent_shows_as_excess_correlation():
    """The statement and the oracle alone: data from a two-latent model, the oracle's E-step under the true parameters
    with both latents and under the same parameters with the second latent removed.  Asserted: only that ``rms_excess``
    is larger for the truncated model at this seed (DESIGN 4.19 records both numbers)."""
    trials, a, b, G = _two_latent_data()
    full = _oracle_rms_excess(trials, a, b, G)
    less = _oracle_rms_excess(trials, a[:1], b, G[:1])
    print("measured pair usefulness: rms_excess %.4f (two latents, the truth) and %.4f (one latent removed); mean_excess "
          "%.4f and %.4f; %d pairs, se_null %.4f" % (full["rms_excess"], less["rms_excess"], full["mean_excess"],
                                                     less["mean_excess"], full["n_pairs"], full["se_null"][1, 0]))
    assert full["n_pairs"] == less["n_pairs"] == 66
    assert less["rms_excess"] > full["rms_excess"]
