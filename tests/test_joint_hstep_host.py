"""The hyperparameter step of the Laplace EM on the host: the NumPy statement (tests/joint_hstep_numpy.py) against the
reference's recorded ``gp.elbo``, against finite differences and against closed forms of the window moments;
``vlgp_amd.gp.optimize_joint`` against ``scipy.optimize.minimize`` on the statement's objective; what the step is good
for on a synthetic set; and the plumbing of ``vlgp_joint_posterior_moments``.  No GPU.

STAGE = 1e-9 is the project's stage-wise tolerance for two dense routes to the same number.

``optimize_joint`` and SciPy run L-BFGS-B from the same start on the same objective: the package's
``joint_window_objective`` is the statement's arithmetic, expression for expression, and csrc/lbfgsb.c takes SciPy's steps
bit for bit where it is bound to SciPy's BLAS (vlgp_amd/gp.py).  Measured here on the CPU over the cases below: the
largest |omega - omega_scipy| / omega_scipy is 0 -- equal bits in all eleven runs -- and every run takes SciPy's number
of iterations (profiles/joint_hstep/measured_errors.txt).  A hundred times the largest measured gap is 0: the test asks
for equal bits."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import joint_cov_numpy as JC
import joint_hstep_numpy as JH
from test_gpu_marginal import _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from gen_joint_hstep import post_cov_of  # noqa: E402  (the expression the fixture's post_cov was built with)

STAGE = 1e-9
OMEGA_TOL = 0.0  # 100 x the largest measured gap (module docstring)
BOUND = (5e-4, 5e-2)


# ---- the objective ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w8", "w50"])
def test_objective_reproduces_the_references_elbo(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "joint_hstep.npz"))
    mu, post_cov = g[name + "_mu"], post_cov_of(g[name + "_A"])
    S = sum(np.outer(mu[:, i], mu[:, i]) + post_cov[:, :, i] for i in range(mu.shape[1]))
    ll, dll = JH.objective(np.log(g[name + "_hyper"]), S, mu.shape[1], float(g[name + "_dt"]))
    want_ll, want_dll = float(g[name + "_ll"]), g[name + "_dll"]
    print("joint_hstep objective [%s]: ll rel %.2e, dll[1] rel %.2e" % (name, abs(ll - want_ll) / abs(want_ll),
                                                                        abs(dll[1] - want_dll[1]) / abs(want_dll[1])))
    assert abs(ll - want_ll) <= STAGE * abs(want_ll)
    assert abs(dll[1] - want_dll[1]) <= STAGE * abs(want_dll[1])
    assert dll[0] == 0.0 and dll[2] == 0.0 and want_dll[0] == 0.0 and want_dll[2] == 0.0


def _random_moments(W, n_w, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((W, 3 * W)) * np.exp(-0.02 * np.arange(W))[:, None]
    return n_w * (X @ X.T) / (3 * W)


@pytest.mark.parametrize("W", [2, 8, 50, 64])
def test_gradient_is_the_central_difference_of_the_objective(W):
    S = _random_moments(W, 7, W)
    for om in (1e-3, 1e-2, 4e-2):
        x = np.log(np.array([1.0, om, 1e-4]))
        h = 1e-5
        up, dn = x.copy(), x.copy()
        up[1] += h
        dn[1] -= h
        fd = (JH.objective(up, S, 7)[0] - JH.objective(dn, S, 7)[0]) / (2 * h)
        ll, dll = JH.objective(x, S, 7)
        # (a central difference of step h is off by h^2 |f'''| / 6 and by the rounding of f over h: 1e-6 relative holds both)
        assert abs(dll[1] - fd) <= 1e-6 * max(abs(fd), abs(ll)), (W, om, dll[1], fd)


# ---- the moments --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    units, params, gauss = _problem([9, 10, 11, 20, 21], 5, 2, [2e-2, 5e-3], seed=4, rank=6)
    st = JC.statement(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"])
    return units, params, gauss, st


def test_a_single_window_is_the_units_own_second_moment(small):
    st = small[3]
    for s in st:
        T = s["mu"].shape[0]
        S, n_w = JH.window_moments([s], T)
        assert n_w == 1
        for l, (m, G, Sig) in enumerate(JH.latent_blocks(s)):
            want = np.outer(m, m) + G @ Sig @ G.T
            assert np.max(np.abs(S[l] - want)) <= STAGE * max(1.0, np.max(np.abs(want)))


def test_the_diagonal_of_the_covariance_part_sums_cov_with_the_overlaps_multiplicity(small):
    st, W = small[3], 10
    _, Sc, n_w = JH.window_moments(st, W, parts=True)
    L = st[0]["unit"].L
    want = np.zeros((L, W))
    for s in st:
        for s0 in JH.window_starts(s["mu"].shape[0], W):
            want += np.diagonal(s["cov"], axis1=1, axis2=2)[s0:s0 + W].T  # (a row under two windows counts twice)
    assert n_w == 0 + 1 + 2 + 2 + 3
    got = np.diagonal(Sc, axis1=1, axis2=2)
    assert np.max(np.abs(got - want)) <= STAGE * max(1.0, np.max(np.abs(want)))
    S, _ = JH.window_moments(st, W)
    assert np.max(np.abs(S - S.transpose(0, 2, 1))) <= STAGE * np.max(np.abs(S))


@pytest.mark.parametrize("W", [2, 7, 50])
def test_window_count_against_a_hand_count(W):
    cases = {W - 1: [], W: [0], W + 1: [0, 1], 2 * W: [0, W], 2 * W + 1: [0, W, W + 1]}
    for T, starts in cases.items():
        assert JH.window_starts(T, W) == starts, (T, W)
    assert JH.n_windows(list(cases), W) == 0 + 1 + 2 + 2 + 3


# ---- optimize_joint against SciPy ---------------------------------------------------------------------------------------
def _scipy_omega(S, n_w, omega, gp_noise=1e-4):
    sig, om, fun, nit = JH.hstep(S, n_w, np.ones(len(omega)), omega, gp_noise, BOUND)
    return om, fun, nit


@pytest.mark.parametrize("W, L, seed", [(8, 1, 0), (25, 3, 1), (50, 5, 2), (64, 2, 3)])
def test_optimize_joint_is_scipys_minimize_on_the_statements_objective(W, L, seed, monkeypatch):
    from vlgp_amd import gp

    rng = np.random.default_rng(seed)
    n_w = 40
    t = np.arange(W)
    S = np.empty((L, W, W))
    for l, om_true in enumerate(np.geomspace(2e-3, 2e-2, L)):  # windows drawn from a GP of a known timescale
        K = np.exp(-om_true * (t[:, None] - t[None, :]) ** 2) + 1e-4 * np.eye(W)
        X = np.linalg.cholesky(K) @ rng.standard_normal((W, n_w))
        S[l] = X @ X.T
    omega0 = np.full(L, 8e-3)
    params = {"zdim": L, "dt": 1.0, "gp_noise": 1e-4, "sigma": np.ones(L), "omega": omega0.copy()}
    want, fun, nit = _scipy_omega(S, n_w, omega0)
    counts = []
    plain = gp.joint_window_objective

    def counted(logps, *a, **k):
        counts.append(len(logps))
        return plain(logps, *a, **k)

    monkeypatch.setattr(gp, "joint_window_objective", counted)
    got, reached = gp.optimize_joint(S, n_w, params, {"omega_bound": BOUND})
    gap = float(np.max(np.abs(got - want) / want))
    print("optimize_joint vs scipy [W %d L %d]: omega gap %.2e, scipy iterations %s, rounds %d, omega %s"
          % (W, L, gap, nit.tolist(), len(counts) - 1, got.tolist()))
    assert np.array_equal(params["omega"], omega0)  # (params is not modified)
    assert gap <= OMEGA_TOL and np.array_equal(got, want)
    assert np.all(np.abs(got - omega0) > 1e-4)  # (the optimiser moved: the case checks something)
    assert np.max(np.abs(reached - fun) / np.abs(fun)) <= STAGE


def test_optimize_joint_keeps_omega_at_a_bound_and_refuses_nan():
    from vlgp_amd import gp

    W = 20
    S = 30.0 * np.ones((1, W, W)) + 1e-3 * np.eye(W)[None]  # a constant path: the timescale runs to the lower bound
    params = {"zdim": 1, "dt": 1.0, "gp_noise": 1e-4, "sigma": np.ones(1), "omega": np.array([8e-3])}
    got, _ = gp.optimize_joint(S, 30, params, {"omega_bound": BOUND})
    assert got[0] == 8e-3
    assert _scipy_omega(S, 30, params["omega"])[0][0] == 8e-3
    with pytest.raises(ValueError, match="finite"):
        gp.optimize_joint(np.full((1, W, W), np.nan), 30, params, {"omega_bound": BOUND})


# ---- what the step is good for ------------------------------------------------------------------------------------------
USEFUL = {"seed": 6, "trials": 10, "T": 40, "N": 12, "omega_true": np.array([2e-2, 4e-3]), "window": 20, "rank": 10}


def useful_problem():
    """Counts drawn from two latent GPs of known timescales through a known loading; the factors of an omega four times
    off (the first latent too fast, the second too slow)."""
    c = USEFUL
    rng = np.random.default_rng(c["seed"])
    L, N, T = 2, c["N"], c["T"]
    a = rng.standard_normal((L, N)) * 0.6
    b = np.full((1, N), np.log(3.0))
    t = np.arange(T)
    units = []
    for _ in range(c["trials"]):
        lat = np.stack([np.linalg.cholesky(np.exp(-om * (t[:, None] - t[None, :]) ** 2) + 1e-6 * np.eye(T))
                        @ rng.standard_normal(T) for om in c["omega_true"]], axis=1)
        rate = np.exp(lat @ a + b)
        y = rng.poisson(rate).astype(float)
        # (a mean-field posterior at the truth to start the Newton iteration from, as a fit would leave one)
        units.append({"y": y, "x": None, "mu": lat, "v": np.zeros((T, L)), "w": rate @ (a ** 2).T})
    omega0 = c["omega_true"] * np.array([4.0, 0.25])
    return units, a, b, omega0


def test_refit_hstep_moves_every_timescale_towards_the_truth():
    c = USEFUL
    units, a, b, omega0 = useful_problem()
    N = a.shape[1]
    sigma = np.ones(2)
    prior = JH.build_prior([c["T"]], omega0, sigma, c["rank"])
    out = JH.refit_hstep(units, a, b, np.ones(N), np.zeros(N, bool), prior, omega0, sigma, c["rank"], 1e-4, (5e-4, 1e-1),
                         c["window"], 3, max_iter=4, tol=0.0, newton_tol=1e-12)
    before, after = np.abs(np.log(omega0 / c["omega_true"])), np.abs(np.log(out["omega"] / c["omega_true"]))
    print("refit_hstep: omega %s -> %s (truth %s), |ln ratio| %s -> %s, evidence %s"
          % (omega0.tolist(), out["omega"].tolist(), c["omega_true"].tolist(), before.tolist(), after.tolist(),
             out["trace"]["laplace"]))
    assert np.all(after < before)
    assert len(out["trace"]["omega"]) == len(out["trace"]["laplace"])
    assert np.array_equal(out["trace"]["omega"][out["kept"]], out["omega"])
    want = JH.build_prior([c["T"]], out["omega"], sigma, c["rank"])[c["T"]]
    assert np.array_equal(out["prior"][c["T"]], want)  # (the factors belong to the returned omega)


# ---- plumbing -----------------------------------------------------------------------------------------------------------
def test_abi_admission_and_python_surface():
    import inspect

    import vlgp_amd
    from vlgp_amd import _lib, gp

    name = "vlgp_joint_posterior_moments"
    assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name][1]) == 12
    assert _lib._SIGNATURES[name][1][:9] == _lib._SIGNATURES["vlgp_joint_posterior"][1]
    assert hasattr(_lib.load(), name)
    header = open(os.path.join(ROOT, "include", "vlgp_hip.h")).read()
    assert "int vlgp_joint_posterior_moments(vlgp_ctx* ctx, int set, int max_iter, double tol," in header
    api = open(os.path.join(ROOT, "vlgp_amd", "csrc", "api.hip")).read()
    assert "X(vlgp_joint_posterior_moments, NOT_REPLICATED | SET_MASKED_FIT, nullptr)" in api
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "| `vlgp_joint_posterior_moments` | not replicated, or a masked fit set |" in design
    assert inspect.signature(vlgp_amd.Engine.joint_posterior).parameters["window"].default is None
    assert inspect.signature(vlgp_amd.refit_joint).parameters["hstep"].default is False
    assert callable(gp.optimize_joint)


@pytest.fixture(scope="module")
def layout_driver(tmp_path_factory):
    """tests/joint_hstep_layout_driver.cpp as a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path_factory.mktemp("joint_hstep_layout") / "joint_hstep_layout_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vlgp_amd", "csrc"), os.path.join(ROOT, "tests", "joint_hstep_layout_driver.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


def _lines(exe, *args):
    done = subprocess.run([exe, args[0]] + [str(int(v)) for v in args[1:]], capture_output=True, timeout=60)
    assert done.returncode == 0, done.stderr.decode(errors="replace")[-3000:]
    return dict(ln.split(" ", 1) for ln in done.stdout.decode().splitlines())


@pytest.mark.parametrize("work, rows, L, M, W", [(10, 2, 1, 1, 2), (123456, 337, 3, 5, 50), (99, 160000, 5, 160, 64),
                                                  (77, 40, 2, 3, 0)])
def test_joint_moments_layout(layout_driver, work, rows, L, M, W):
    """vlgp_joint_posterior's block, then the partials (M, L, W, W) and S (L, W, W), in order, without overlap, up to need;
    W = 0 is vlgp_joint_posterior's block itself."""
    got = {k: int(v) for k, v in _lines(layout_driver, "layout", work, rows, L, M, W).items()}
    cov = work + 8 * M
    part = cov + rows * (L * (L + 1) // 2)
    assert got == {"work": 0, "stats": work, "cov": cov, "posterior_need": part, "part": part, "S": part + M * L * W * W,
                   "need": part + (M + 1) * L * W * W}


@pytest.mark.parametrize("window, rp, n_w, status, word", [(1, 5, 3, -1, "window = 1"), (65, 5, 3, -1, "window = 65"),
                                                            (-4, 5, 3, -1, "window = -4"), (50, 65, 3, -3, "rank 65"),
                                                            (50, 64, 0, -3, "as long as the window (50)"),
                                                            (1, 65, 0, -1, "window = 1"), (2, 64, 1, 0, ""),
                                                            (64, 1, 9, 0, "")])
def test_joint_moments_refusals_and_window_counts(layout_driver, window, rp, n_w, status, word):
    got = _lines(layout_driver, "refusal", window, rp, n_w)
    assert int(got["status"]) == status and word in got.get("text", "")
    if status:
        assert got["text"].startswith("vlgp_joint_posterior_moments: ")
    for T in (window - 1, window, window + 1, 2 * window, 2 * window + 1, 1000):
        if window >= 2 and T >= 0:
            assert int(_lines(layout_driver, "windows", T, window)["n"]) == len(JH.window_starts(T, window))


def test_refit_joint_hstep_refuses_before_an_engine_exists_and_touches_nothing(monkeypatch):
    import vlgp_amd
    from vlgp_amd import engine

    def no_engine(*args, **kwargs):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(engine.Engine, "for_params", no_engine)
    rng = np.random.default_rng(0)
    trials = [{"y": rng.poisson(1.0, (6, 3)).astype(float), "mu": rng.standard_normal((6, 2)), "w": rng.random((6, 2)),
               "v": rng.random((6, 2))} for _ in range(2)]
    params = {"ydim": 3, "zdim": 2, "xdim": 1, "rank": 4, "a": rng.standard_normal((2, 3)), "b": np.zeros((1, 3)),
              "noise": np.ones(3), "likelihood": np.array(["poisson"] * 3), "omega": np.ones(2), "sigma": np.ones(2),
              "gp_noise": 1e-4, "dt": 1}
    config = {"Mniter": 3, "use_hessian": True, "eps": 1e-8, "learning_rate": 1.0, "da_bound": 5.0, "db_bound": 5.0,
              "window": 4, "omega_bound": BOUND}
    keep = copy.deepcopy((trials, params, config))
    for cfg, par, match in ((dict(config, window=1), params, "need 2 <= window <= 64"),
                            (dict(config, window=65), params, "need 2 <= window <= 64"),
                            (config, dict(params, rank=65), "at most 64"),
                            (dict(config, window=7), params, r"no trial is as long as the window \(7\)")):
        with pytest.raises(ValueError, match=match):
            vlgp_amd.refit_joint(trials, par, cfg, verbose=False, hstep=True)
    with pytest.raises(AssertionError, match="an engine was created"):  # (sound arguments go on to the engine)
        vlgp_amd.refit_joint(trials, params, config, verbose=False, hstep=True)
    for got, want in zip((trials, params, config), keep):
        for a, b in zip(got if isinstance(got, list) else [got], want if isinstance(want, list) else [want]):
            assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
