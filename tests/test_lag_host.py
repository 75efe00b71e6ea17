"""The lag moments without a GPU: the statement (tests/lag_numpy.py) against its own identities, against Monte Carlo and
against what it is for; the summary; the bindings, the admission row and the refusals; the layout of the call's device
block walked by a stand-alone sanitized driver; and the conditioning of every case of the GPU table."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import lag_cases as LC
import lag_numpy as LN
import pair_numpy as PN
from conftest import ROOT
from oracle import vlgp_oracle as O


def _fixed_point(unit, par, G, n_iter=200):
    """v = diag S(w(mu, v)) iterated on the host: the unit with that v, and how far the last step moved it."""
    v = unit["v"].copy()
    for _ in range(n_iter):
        w = LN.weights(unit.get("x"), unit["mu"], v, par["a"], par["b"], par["noise"], par["gauss"], np.ones(unit["y"].shape, dtype=bool))
        new = np.stack([(LN.cross_factor(G[l], w[:, l]) ** 2).sum(axis=1) for l in range(G.shape[0])], axis=1)
        moved, v = float(np.abs(new - v).max()), new
    return dict(unit, v=v), moved


def test_lag_zero_at_the_fixed_point_is_the_diagonal_of_the_pair_moments():
    units, par, prior, _ = LC.problem("folds")
    fixed = []
    for u in units:
        f, moved = _fixed_point(u, par, prior[u["y"].shape[0]])
        assert moved <= 1e-15
        fixed.append(f)
    resid, model, count, bad = LN.lag_moments(fixed, par, prior, 4)
    cat = lambda k: np.concatenate([u[k] for u in fixed])  # noqa: E731
    pr, pm, pc = PN.pair_moments(cat("y"), None, cat("mu"), PN.diag_cov(cat("v")), par["a"], par["b"], par["noise"], par["gauss"])
    assert bad == 0 and np.array_equal(count[0], np.diagonal(pc))
    err = max(np.abs(resid[0] - np.diagonal(pr)).max() / np.abs(pr).max(), np.abs(model[0] - np.diagonal(pm)).max() / np.abs(pm).max())
    print("measured lag identities [lag 0 against pair_numpy's diagonal]: %.2e" % err)
    assert err <= 1e-13
    # away from the fixed point the two differ: lag 0 uses c(t, t), the pair moments the stored v
    off = LN.lag_moments(units, par, prior, 0)[1][0]
    off_pair = PN.pair_moments(*(np.concatenate([u[k] for u in units]) if k != "x" else None for k in ("y", "x", "mu")),
                               PN.diag_cov(np.concatenate([u["v"] for u in units])), par["a"], par["b"], par["noise"], par["gauss"])[1]
    assert np.abs(off - np.diagonal(off_pair)).max() > 1e-3


def test_a_point_posterior_and_a_lag_past_the_unit():
    units, par, prior, _ = LC.problem("one")  # lengths 1, 2, 5
    resid, model, count, bad = LN.lag_moments(units, par, prior, 6, vb=False)
    assert bad == 0 and not model[1:].any() and resid[1:5].any()
    assert np.array_equal(count[:, 0], [8, 5, 3, 2, 1, 0, 0])
    e = np.concatenate([LN.row_terms(u["y"], u["x"], u["mu"], u["v"], par["a"], par["b"], par["noise"], par["gauss"], vb=False)[1] for u in units])
    assert model[0, 0] == pytest.approx(e.sum(), rel=1e-15)
    s = LN.summary(resid, model, count)
    from vlgp_amd.evaluation import _lag_summary
    g = _lag_summary(resid, model, count)
    for key in s:
        assert np.array_equal(np.isnan(np.asarray(s[key], dtype=float)), np.isnan(np.asarray(g[key], dtype=float))), key
        assert np.allclose(np.asarray(s[key], dtype=float), np.asarray(g[key], dtype=float), rtol=1e-14, atol=0, equal_nan=True), key
    assert np.all(np.isnan(g["excess_acf"][5:])) and np.all(np.isnan(g["se_null"][5:])) and np.all(np.isfinite(g["excess_acf"][:5]))
    assert g["n_scored"] == 4 and set(g) == set(s)
    with pytest.raises(ValueError, match="K \\+ 1, N"):
        _lag_summary(resid[:3], model, count)
    dead = _lag_summary(resid, 0.0 * model, count)  # (no variance: nothing to normalise by)
    assert np.all(np.isnan(dead["residual_acf"])) and np.isnan(dead["rms_excess_all"]) and dead["n_scored"] == 0


def test_live_is_a_selection():
    """NaN in y at every entry that is not live changes no bit; the pairs counted are the pairs of live entries."""
    name = "speckled"
    units, par, prior, _ = LC.problem(name)
    lengths = LC.CASES[name][0]
    live = LC.per_unit(LC.masks(name)[0], lengths)
    dirty = [dict(u, y=np.where(lv, u["y"], np.nan)) for u, lv in zip(units, live)]
    one, two = LN.lag_moments(units, par, prior, 5, live=live), LN.lag_moments(dirty, par, prior, 5, live=live)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one[:3], two[:3])) and np.isfinite(one[0]).all()
    want = sum(np.stack([(lv[:len(lv) - k] & lv[k:]).sum(axis=0) for k in range(6)]) for lv in live)
    assert np.array_equal(one[2], want)
    # a unit whose H has no factor is in no sum
    broken = [dict(u) for u in units]
    broken[1] = dict(units[1], v=np.full_like(units[1]["v"], np.nan))
    got = LN.lag_moments(broken, par, prior, 5)
    assert got[3] == par["a"].shape[0] and all(np.array_equal(a, b) for a, b in zip(got[:3], LN.lag_moments(units[:1], par, prior, 5)[:3]))


def test_the_closed_forms_against_monte_carlo():
    """Latent paths from N(mu, S_l), counts from the Poisson (one Gaussian channel), 200 000 draws: the mean over the
    draws of sum_t d_t d_{t+k} against model[k, n], each within 4.5 standard errors of the Monte Carlo mean (16 comparisons:
    about one chance in ten thousand under the hypothesis that the formula is right).  Measured at this seed: the worst is
    2.08 standard errors."""
    rng = np.random.default_rng(7)
    T, N, L, R, K, D = 12, 4, 2, 6, 3, 200000
    gauss = np.array([False, False, True, False])
    par = dict(a=0.5 * rng.standard_normal((L, N)), b=np.array([[0.2, -0.3, 0.5, 0.6]]), noise=np.array([1.0, 1.0, 0.7, 1.0]), gauss=gauss)
    G = np.stack([O.ichol_gauss(T, om, R) for om in (0.05, 0.5)])
    unit = {"y": np.zeros((T, N)), "x": None, "mu": 0.5 * rng.standard_normal((T, L)), "v": np.full((T, L), 0.1)}
    unit, moved = _fixed_point(unit, par, G)
    assert moved <= 1e-15
    w = LN.weights(None, unit["mu"], unit["v"], par["a"], par["b"], par["noise"], gauss, np.ones((T, N), dtype=bool))
    z = np.stack([unit["mu"][:, l] + rng.standard_normal((D, R)) @ LN.cross_factor(G[l], w[:, l]).T for l in range(L)], axis=2)
    eta = z @ par["a"] + par["b"][0]
    y = np.where(gauss, eta + np.sqrt(par["noise"]) * rng.standard_normal(eta.shape), rng.poisson(np.exp(eta)))
    e = LN.row_terms(unit["y"], None, unit["mu"], unit["v"], par["a"], par["b"], par["noise"], gauss)[1]
    d = y - e
    _, model, count, bad = LN.lag_moments([unit], par, {T: G}, K)
    assert bad == 0 and np.abs(model[1:]).max() > 0.05  # (there is a lagged covariance to find)
    worst = 0.0
    for k in range(K + 1):
        x = (d[:, :T - k] * d[:, k:]).sum(axis=1)  # (D, N)
        se = x.std(axis=0, ddof=1) / np.sqrt(D)
        worst = max(worst, float(np.max(np.abs(x.mean(axis=0) - model[k]) / se)))
    print("measured lag Monte Carlo: worst |mean - model| / standard error over %d comparisons: %.2f" % ((K + 1) * N, worst))
    assert worst <= 4.5


def _recording(refractory, seed=0):
    """20 trials x 50 bins x 12 Poisson channels from a two-latent GP model; with ``refractory`` a count at bin t - 1
    divides the channel's rate at bin t by e^1.5, an effect the model has no term for."""
    rng = np.random.default_rng(seed)
    n_trials, T, N, L, rank = 20, 50, 12, 2, 20
    G = O.build_prior([T], np.array([2e-2, 5e-3]), np.ones(L), rank)[T]
    a = rng.standard_normal((L, N)) * np.array([[0.6], [0.4]])
    b = np.full((1, N), 0.3)
    trials = []
    for _ in range(n_trials):
        z = np.stack([G[l] @ rng.standard_normal(rank) for l in range(L)], axis=1)
        rate, y = np.exp(z @ a + b), np.zeros((T, N))
        for t in range(T):
            y[t] = rng.poisson(rate[t] * (np.exp(-1.5 * (y[t - 1] > 0)) if refractory and t else 1.0))
        trials.append({"y": y, "x": np.ones((T, 1, N))})
    return trials, a, b, G


def _oracle_summary(trials, a, b, G, K=5, n_iter=30):
    """The summary of the trials under the oracle's E-step posterior (from zero) of the model a, b, G."""
    L, N = a.shape
    par = dict(a=a, b=b, noise=np.ones(N), gauss=np.zeros(N, dtype=bool))
    units = []
    for tr in trials:
        T = tr["y"].shape[0]
        mu = np.zeros((T, L))
        w = O.curvature_unit(tr["y"], tr["x"], mu, np.zeros((T, L)), a, b, par["noise"], par["gauss"])
        v = O.variance_unit(w, np.zeros((T, L)), G)[0]
        mu, v = O.estep_unit(tr["y"], tr["x"], mu, v, w, a, b, par["noise"], par["gauss"], G, n_iter)[:2]
        units.append({"y": tr["y"], "x": tr["x"], "mu": mu, "v": v})
    return LN.summary(*LN.lag_moments(units, par, {trials[0]["y"].shape[0]: G}, K)[:3])


def test_a_refractory_effect_shows_as_excess_autocorrelation():
    """The statement and the oracle alone: two recordings drawn here from one two-latent GP model (vlgp_amd.synth draws
    Lorenz paths, which have no loadings or prior to score under), the second with a refractory dependence on the
    previous bin, each scored under the oracle's E-step posterior of the true parameters.  Measured at this seed:
    ``rms_excess_all`` 0.0585 well specified (se_null 0.0319 at lag 1) and 0.2176 with the refractory effect, whose mean
    excess at lag 1 is -0.238 against -0.059.  Asserted: a factor of two between them, and the sign at lag 1."""
    good = _oracle_summary(*_recording(False))
    bad = _oracle_summary(*_recording(True))
    print("measured lag usefulness: rms_excess_all %.4f (well specified) and %.4f (refractory); mean excess at lag 1 %.4f and "
          "%.4f; se_null at lag 1 %.4f; dispersion %.3f and %.3f" % (good["rms_excess_all"], bad["rms_excess_all"],
                                                                   good["excess_acf"][1].mean(), bad["excess_acf"][1].mean(),
                                                                   good["se_null"][1, 0], good["dispersion"].mean(), bad["dispersion"].mean()))
    assert good["n_scored"] == bad["n_scored"] == 60
    assert bad["rms_excess_all"] >= 2.0 * good["rms_excess_all"]
    assert bad["excess_acf"][1].mean() <= -3.0 * good["se_null"][1, 0] and abs(good["excess_acf"][1].mean()) <= 3.0 * good["se_null"][1, 0]


def test_header_binding_admission_and_public_names():
    import vlgp_amd
    from vlgp_amd import _lib, evaluation

    header = open(os.path.join(ROOT, "include", "vlgp_hip.h")).read()
    assert ("int vlgp_lag_moments(vlgp_ctx* ctx, int set, int vb, int max_lag, double* resid, double* model, double* count,\n"
            "                     int* n_failed);") in header
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", header).group(1)) == 3 and _lib.ABI_VERSION == 3
    assert "vlgp_lag_moments" in _lib.EXPORTS and len(_lib._SIGNATURES["vlgp_lag_moments"][1]) == 8
    assert hasattr(_lib.load(), "vlgp_lag_moments")
    assert _lib._SIGNATURES["vlgp_lag_moments"][1][-1] == _lib._SIGNATURES["vlgp_elbo"][1][-1]  # (n_failed: int*)
    api = open(os.path.join(ROOT, "vlgp_amd", "csrc", "api.hip")).read()
    assert re.search(r"X\(vlgp_lag_moments, SET_ANY & ~\(SET_COPIED \| SET_GROUPS\),\s*\\\n\s*\"vlgp_lag_moments on a copied cut: "
                     r"merge it and score the source set\"\)", api)
    assert "lags.hip" in open(os.path.join(ROOT, "vlgp_amd", "csrc", "Makefile")).read()
    assert "residual_autocorrelation" in evaluation.__all__
    sig = inspect.signature(evaluation.residual_autocorrelation).parameters
    assert list(sig) == ["trials", "params", "config", "max_lag", "how", "groups", "n_folds", "seed", "n_iter", "device"]
    assert (sig["max_lag"].default, sig["how"].default, sig["n_folds"].default) == (20, "in_sample", 5)
    assert list(inspect.signature(vlgp_amd.Engine.lag_moments).parameters) == ["self", "set_id", "max_lag", "vb"]


def test_residual_autocorrelation_refuses_before_any_device_call():
    from vlgp_amd import evaluation

    params, trials = {"ydim": 3, "zdim": 1}, [{"y": np.zeros((10, 3))}]
    with pytest.raises(ValueError, match="how"):
        evaluation.residual_autocorrelation(trials, params, {}, how="entries")
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="max_lag = %d, need 0 <= max_lag <= 64" % bad):
            evaluation.residual_autocorrelation(trials, params, {}, max_lag=bad)
    with pytest.raises(ValueError, match="missing"):
        evaluation.residual_autocorrelation([{"y": np.zeros((10, 3)), "missing": np.zeros((10, 3), dtype=bool)}], params, {})
    with pytest.raises(ValueError, match="group"):
        evaluation.residual_autocorrelation(trials, params, {}, how="channels", groups=[[0, 1, 2]])
    with pytest.raises(TypeError):
        evaluation.residual_autocorrelation(trials, params, {}, posterior="joint")
    # the workspace of c counts in the replica budget
    assert evaluation.default_max_replicas(160000, 5, mask_channels=100) > evaluation.default_max_replicas(
        160000, 5, mask_channels=100, extra_bytes=evaluation._lag_replica_bytes(160000, 5, 20))
    assert evaluation._lag_replica_bytes(160000, 5, 20) == 8 * 160000 * 5 * 22


@pytest.fixture(scope="module")
def layout_driver(tmp_path_factory):
    """tests/lag_layout_driver.cpp as a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path_factory.mktemp("lag_layout") / "lag_layout_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vlgp_amd", "csrc"), os.path.join(ROOT, "tests", "lag_layout_driver.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


def _layout(exe, *args):
    done = subprocess.run([exe] + [str(int(v)) for v in args], capture_output=True, timeout=60)
    assert done.returncode == 0, done.stderr.decode(errors="replace")[-3000:]
    return {k: int(v) for k, v in (ln.split(" ") for ln in done.stdout.decode().splitlines())}, done.stderr.decode()


@pytest.mark.parametrize("rows, N, L, n_rep, units, K, vb", [(1, 1, 1, 1, 1, 0, 1), (127, 63, 2, 1, 3, 1, 1), (128, 64, 5, 2, 4, 31, 1),
                                                             (129, 65, 8, 3, 2, 32, 0), (387, 100, 5, 1, 5, 20, 1),
                                                             (160, 130, 9, 3, 2, 63, 1), (160000, 100, 5, 1, 160, 20, 1),
                                                             (160000, 100, 5, 5, 160, 20, 1), (40000, 1000, 10, 2, 40, 64, 1)])
def test_lag_layout(layout_driver, rows, N, L, n_rep, units, K, vb):
    """The regions lie in order, without overlap, up to ``need``, each as large as the kernels and the copies use it; the
    chunks cover the rows, none is empty, none is shorter than the smallest chunk unless it is the last, and the rule of
    DESIGN 4.20 sizes them: eight waves per compute unit, the partials within 32 MiB when more than one chunk is cut."""
    n_cu, tasks = 256, n_rep * units * L
    got, _ = _layout(layout_driver, rows, N, L, n_rep, tasks, K, vb, n_cu, 64, 1)
    tiles, K1 = -(-N // 64), K + 1
    assert (got["tiles"], got["min_chunk"], got["lag_group"], got["lag_max"]) == (tiles, 128, 8, 64)
    chunk, n_chunks = got["chunk_rows"], got["n_chunks"]
    assert chunk >= 128 and (n_chunks - 1) * chunk < rows <= n_chunks * chunk
    groups = tiles * n_rep
    want, cap = -(-8 * n_cu // groups), max((1 << 22) // (groups * 3 * K1 * 64), 1)
    assert chunk == max(128, -(-rows // min(want, cap)))
    if n_chunks > 1:
        assert groups * n_chunks * 3 * K1 * 64 * 8 <= 32 << 20 and groups * n_chunks <= 8 * n_cu + groups
    at = 0
    for name, size in (("w", n_rep * rows * L if vb else 0), ("c", n_rep * rows * K1 * L if vb else 0),
                       ("flag", (tasks + 1) // 2 if vb else 0), ("part", groups * n_chunks * 3 * K1 * 64),
                       ("resid", n_rep * K1 * N), ("model", n_rep * K1 * N), ("count", n_rep * K1 * N)):
        assert got[name] == at, (name, got)
        at += size
    assert got["need"] == at and got["c_doubles"] == (n_rep * rows * K1 * L if vb else 0) and got["refusal"] == 0
    assert got["task_lds_doubles"] == 64 * 65 + (64 + K) * 65 + 8 + 64 + 64 and got["task_lds_doubles"] * 8 <= 160 * 1024
    assert got["moments_lds_bytes"] == 8 * 64 * (L + 2 * K1) + 4 * 64 * K1 <= 160 * 1024


def test_the_headline_workspace_and_what_the_call_refuses(layout_driver):
    """134 MB of c at the headline fold; rank 64 at max_lag 64 is the 100 KB of LDS the task kernel raises its limit for;
    a workspace past 4 GiB is refused with its bytes, a lag past 64, a rank past 64 and a second rank with theirs."""
    got, _ = _layout(layout_driver, 160000, 100, 5, 1, 800, 20, 1, 256, 50, 1)
    assert got["c_doubles"] * 8 == 134400000 and got["refusal"] == 0
    got, _ = _layout(layout_driver, 100, 10, 5, 1, 5, 64, 1, 256, 64, 1)
    assert got["task_lds_doubles"] * 8 == 100928
    got, said = _layout(layout_driver, 2000000, 100, 10, 1, 20000, 64, 1, 256, 50, 1)
    assert (got["refusal"], got["refusal_arg"]) == (-3, 8 * 2000000 * 65 * 10) and "need 10400000000 bytes of workspace" in said
    got, said = _layout(layout_driver, 2000000, 100, 10, 1, 20000, 64, 0, 256, 50, 1)
    assert got["refusal"] == 0 and got["c_doubles"] == 0  # (vb == 0 has no c)
    for K, rp, world, status, text in ((65, 10, 1, -1, "max_lag = 65, need 0 <= max_lag <= 64"), (-1, 10, 1, -1, "max_lag = -1"),
                                       (3, 65, 1, -3, "rank 65, at most 64"), (3, 10, 2, -3, "more than one rank (2)")):
        got, said = _layout(layout_driver, 100, 10, 5, 1, 5, K, 1, 256, rp, world)
        assert got["refusal"] == status and text in said, (K, rp, world, said)


def test_small_sets_take_chunks_of_128_rows(layout_driver):
    """What tests/test_gpu_lag.py relies on for its row counts: a small set is cut into chunks of 128 rows."""
    for rows, n_chunks in ((1, 1), (127, 1), (128, 1), (129, 2), (387, 4), (160, 2)):
        for N, n_rep in ((1, 1), (100, 1), (130, 3)):
            got, _ = _layout(layout_driver, rows, N, 5, n_rep, 5 * n_rep, 20, 1, 256, 30, 1)
            assert (got["chunk_rows"], got["n_chunks"]) == (128, n_chunks), (rows, N, got)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_every_gpu_case_is_well_conditioned(name):
    """mu and v moved up by one ulp each move no sum by more than 2e-14 of its lag's largest entry: a tenth of what
    tests/test_gpu_lag.py allows the device, so that tolerance measures the kernels and not the problem.  (An ulp of an
    input of size one is 2e-16; the sums pass it through exp and expm1 with arguments of a few units.)"""
    units, par, prior, _ = LC.problem(name)
    lengths, K = LC.CASES[name][0], LC.CASES[name][4]
    live = None if LC.CASES[name][-1] is None else LC.per_unit(LC.masks(name)[0], lengths)
    moved = [dict(u, mu=np.nextafter(u["mu"], np.inf), v=np.nextafter(u["v"], np.inf)) for u in units]
    one = LC.statement(name) if live is None else LN.lag_moments(units, par, prior, K, live=live)
    two = LN.lag_moments(moved, par, prior, K, live=live)
    assert np.array_equal(one[2], two[2]) and one[3] == two[3] == 0
    err = max(float(np.max(np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(a).max(axis=1)))) for a, b in zip(one[:2], two[:2]))
    print("measured lag conditioning [%s]: %.2e" % (name, err))
    assert err <= 2e-14
