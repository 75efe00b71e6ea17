"""The NumPy statement of vlgp_mstep_cov and of the Laplace EM loop (tests/joint_em_numpy.py) against the reference's golden
fixtures and against finite differences, the loop's rules, the ABI and Python surface, the host frame of the call and the
conditioning of the cases the GPU tests run (tests/joint_em_cases.py).  No GPU.

STAGE = 1e-9 is the project's stage-wise tolerance."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import joint_cov_numpy as JC
import joint_em_cases as CS
import joint_em_numpy as EM
from conftest import relerr
from oracle import vlgp_oracle as O
from test_gpu_rates import per_channel_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STAGE = 1e-9
# the bound the GPU tests hold the device to (tests/test_gpu_joint_em.py): the cases must be conditioned for it
from test_gpu_joint_em import BOUND  # noqa: E402


def diag_cov(v):
    L = v.shape[1]
    cov = np.zeros(v.shape + (L,))
    cov[:, np.arange(L), np.arange(L)] = v
    return cov


# ---- the statement against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p1", "p3", "mixed"])
def test_a_diagonal_cov_reproduces_the_reference_mstep(tag):
    """cov = diag(v): the outputs the real reference wrote into tests/golden/mstep_*.npz, Newton and gradient steps, one and
    twenty-five iterations, at the stage tolerance -- da and db of a converged iteration included, which are differences
    of nearly equal numbers and which only the same arithmetic reproduces: the statement gives oracle.mstep_arrays' bits."""
    g = dict(np.load(os.path.join(GOLDEN, "mstep_%s.npz" % tag)))
    cat = lambda k: np.concatenate(list(g[k]), axis=0)
    cov = diag_cov(cat("v"))
    for key in ("H_1", "H_25", "G_1", "G_25"):
        out = EM.mstep_cov(cat("y"), cat("x"), cat("mu"), cov, g["a"], g["b"], g["gauss"], int(key[2:]), key[0] == "H", 1e-8,
                           float(g["lr_" + key]))
        same = O.mstep_arrays(cat("y"), cat("x"), cat("mu"), cat("v"), g["a"], g["b"], g["gauss"], int(key[2:]), key[0] == "H",
                              1e-8, float(g["lr_" + key]))
        for k, arr, ref in zip(("a", "b", "da", "db", "noise"), out, same):
            assert relerr(arr, g["%s_%s" % (k, key)]) < STAGE, (tag, key, k)
            # ... and the project's oracle bit for bit: the off-diagonal part of every sum adds exact zeros to its arithmetic
            assert np.array_equal(arr, ref), (tag, key, k)


def _small(seed, L=3, N=4, T=60, P=2):
    rng = np.random.default_rng(seed)
    mu = 0.5 * rng.standard_normal((T, L))
    A = 0.25 * rng.standard_normal((T, L, L))
    cov = A @ A.transpose(0, 2, 1)  # full, PSD, off-diagonals of the size of the diagonal
    a = 0.4 * rng.standard_normal((L, N))
    b = np.log(0.5) + 0.2 * rng.standard_normal((P, N))
    x = np.ones((T, P, N))
    x[:, 1:] = 0.3 * rng.standard_normal((T, P - 1, N))
    y = rng.poisson(1.0, (T, N)).astype(float)
    return y, x, mu, cov, a, b


def test_gradient_and_hessian_are_the_derivatives_of_the_expected_log_likelihood():
    """Q(a_n) = sum_t y (a.mu + x b) - exp(a.mu + x b + a'C_t a / 2), below the clamp.  grad_a against central differences of
    Q (step h = 1e-5: truncation h^2 Q''' / 6 ~ 1e-10 of the scale S = sum |terms of Q|, rounding ~ 1e-16 S / h = 1e-11 S),
    nhess_a against central differences of the statement's own gradient (the same orders): both held at 1e-8 S."""
    y, x, mu, cov, a, b = _small(7)
    h = 1e-5
    for n in range(a.shape[1]):
        off = x[:, :, n] @ b[:, n]

        def Q(an):
            lin = mu @ an + off
            ex = lin + 0.5 * np.einsum("l,tlm,m->t", an, cov, an)
            assert ex.max() < 10.0
            return float(np.sum(y[:, n] * lin - np.exp(ex))), float(np.sum(np.abs(y[:, n] * lin) + np.exp(ex)))

        def grad(an):
            aa = a.copy()
            aa[:, n] = an
            return EM.grad_hess_a(y[:, n], mu, cov, aa, b, x, n)

        g, H = grad(a[:, n])
        S = Q(a[:, n])[1]
        for l in range(a.shape[0]):
            e = np.zeros(a.shape[0])
            e[l] = h
            fd = (Q(a[:, n] + e)[0] - Q(a[:, n] - e)[0]) / (2 * h)
            assert abs(fd - g[l]) < 1e-8 * S, (n, l, fd, g[l])
            fd_h = -(grad(a[:, n] + e)[0] - grad(a[:, n] - e)[0]) / (2 * h)
            assert np.max(np.abs(fd_h - H[l])) < 1e-8 * S, (n, l)
        assert np.max(np.abs(H - H.T)) < 1e-12 * S


def test_the_split_sums_of_mstep_cov_are_the_plain_gradient_and_hessian():
    """One Newton iteration of mstep_cov is a step H^-1 g with the plain-form g, H of grad_hess_a."""
    y, x, mu, cov, a, b = _small(11)
    gauss = np.zeros(a.shape[1], bool)
    out = EM.mstep_cov(y, x, mu, cov, a, b, gauss, 1, eps=0.0)
    for n in range(a.shape[1]):
        g, H = EM.grad_hess_a(y[:, n], mu, cov, a, b, x, n)
        assert np.max(np.abs(out[2][:, n] - np.linalg.solve(H, g))) < STAGE * max(1.0, np.max(np.abs(out[2][:, n])))


def test_gaussian_channels_solve_the_expected_normal_equations():
    """A Gaussian channel's a_n is the minimiser of E ||y_n - x b - z a||^2 under z_t ~ N(mu_t, C_t): (mu'mu + sum C) a =
    mu'(y - x b)."""
    y, x, mu, cov, a, b = _small(5, P=1)
    rng = np.random.default_rng(2)
    y = mu @ a + b[0] + 0.3 * rng.standard_normal(y.shape)
    gauss = np.ones(a.shape[1], bool)
    out = EM.mstep_cov(y, x, mu, cov, a, b, gauss, 1)
    M = mu.T @ mu + cov.sum(axis=0)
    for n in range(a.shape[1]):
        assert np.max(np.abs(M @ out[0][:, n] - mu.T @ (y[:, n] - b[0, n]))) < STAGE * np.max(np.abs(M))
    assert np.max(np.abs(out[4] - np.var(y - (mu @ a + b[0]), axis=0))) < 1e-14


# ---- the loop ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    units, params, gauss = EM.tiny_problem()
    args = (params["a"], params["b"], params["noise"], gauss, params["cholesky"])
    runs = {"eight": EM.refit(units, *args, 25, max_iter=8, tol=0.0)}
    return {"units": units, "params": params, "gauss": gauss, "args": args, "runs": runs}


def test_the_tiny_problem_has_the_shape_the_issue_names(tiny):
    lengths = [u["y"].shape[0] for u in tiny["units"]]
    assert len(lengths) == 6 and len(set(lengths)) > 1 and all(20 <= T <= 40 for T in lengths)
    assert tiny["params"]["a"].shape == (2, 8) and int(tiny["gauss"].sum()) == 2


def test_the_evidence_rises_at_each_of_the_first_eight_iterations(tiny):
    tr = tiny["runs"]["eight"]["trace"]
    assert len(tr["laplace"]) == 9 and all(tr["converged"])
    steps = np.diff(tr["laplace"])
    print("joint-em statement trace %s" % tr["laplace"])
    assert np.all(steps > 1e-3), steps  # (with room: the smallest step is a quarter of a nat, the evidence is good to 1e-9)


def test_stop_rule_and_the_better_of_the_last_two(tiny):
    units, args = tiny["units"], tiny["args"]
    base = tiny["runs"]["eight"]
    E = base["trace"]["laplace"]
    # the relative gain of iteration k: the loop stops at the first k whose gain is <= tol
    gains = [(E[k] - E[k - 1]) / abs(E[k]) for k in range(1, len(E))]
    k_stop = 3
    tol = 0.5 * (gains[k_stop - 2] + gains[k_stop - 1])
    assert gains[k_stop - 1] <= tol < min(gains[:k_stop - 1])
    run = EM.refit(units, *args, 25, max_iter=8, tol=tol)
    assert len(run["trace"]["laplace"]) == k_stop + 1 and run["kept"] == k_stop  # E_k >= E_{k-1}: the last one is kept
    assert run["trace"]["laplace"] == E[:k_stop + 1]
    # max_iter: iteration max_iter is evaluated and returned, no M-step after it
    run2 = EM.refit(units, *args, 25, max_iter=2, tol=0.0)
    assert len(run2["trace"]["laplace"]) == 3 and run2["kept"] == 2 and run2["trace"]["laplace"] == E[:3]
    # an evidence that falls: the parameters and the posterior of the iteration before come back
    fall = EM.refit(units, *args, 25, max_iter=8, tol=0.0, trace_hook=lambda k, ev: ev - 50.0 if k == 2 else ev)
    assert len(fall["trace"]["laplace"]) == 3 and fall["kept"] == 1
    one = EM.refit(units, *args, 25, max_iter=1, tol=0.0)
    for key in ("a", "b", "noise", "da", "db", "mu", "cov"):
        assert np.array_equal(fall[key], one[key]), key
    # without an M-step (max_iter = 0) the caller's parameters come back with their posterior
    zero = EM.refit(units, *args, 25, max_iter=0)
    assert zero["da"] is None and np.array_equal(zero["a"], args[0]) and len(zero["trace"]["laplace"]) == 1


def test_the_returned_posterior_is_that_of_the_returned_parameters(tiny):
    units, args = tiny["units"], tiny["args"]
    for run in (tiny["runs"]["eight"],
                EM.refit(units, *args, 25, max_iter=8, tol=0.0, trace_hook=lambda k, ev: ev - 50.0 if k == 2 else ev)):
        st = JC.statement(units, run["a"], run["b"], run["noise"], args[3], args[4])
        assert np.array_equal(np.concatenate([s["mu"] for s in st]), run["mu"])
        assert np.array_equal(np.concatenate([s["cov"] for s in st]), run["cov"])
        assert float(sum(s["laplace"] for s in st)) == run["trace"]["laplace"][run["kept"]]


# ---- bindings ---------------------------------------------------------------------------------------------------------
def test_abi_and_python_surface():
    import vlgp_amd
    from vlgp_amd import _lib

    text = open(os.path.join(ROOT, "include", "vlgp_hip.h")).read()
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3 and _lib.ABI_VERSION == 3
    decl = re.search(r"int vlgp_mstep_cov\(([^;]*)\);", text)
    assert decl and len(decl.group(1).split(",")) == 11
    assert "vlgp_mstep_cov" in _lib.EXPORTS and len(_lib._SIGNATURES["vlgp_mstep_cov"][1]) == 11
    assert hasattr(_lib.load(), "vlgp_mstep_cov")
    assert callable(vlgp_amd.Engine.mstep_cov) and callable(vlgp_amd.refit_joint) and "refit_joint" in vlgp_amd.__all__
    api = open(os.path.join(ROOT, "vlgp_amd", "csrc", "api.hip")).read()
    assert "X(vlgp_mstep_cov, NOT_REPLICATED, nullptr)" in api
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "| `vlgp_mstep_cov` | not replicated |" in design


def test_refit_joint_refuses_before_an_engine_exists_and_touches_nothing():
    import vlgp_amd

    rng = np.random.default_rng(0)
    trials = [{"y": rng.poisson(1.0, (6, 3)).astype(float), "mu": rng.standard_normal((6, 2)), "w": rng.random((6, 2)),
               "v": rng.random((6, 2))} for _ in range(2)]
    params = {"ydim": 3, "zdim": 2, "xdim": 1, "rank": 4, "a": rng.standard_normal((2, 3)), "b": np.zeros((1, 3)),
              "noise": np.ones(3), "likelihood": np.array(["poisson"] * 3), "omega": np.ones(2), "sigma": np.ones(2)}
    config = {"Mniter": 3, "use_hessian": True, "eps": 1e-8, "learning_rate": 1.0, "da_bound": 5.0, "db_bound": 5.0}
    keep = copy.deepcopy((trials, params, config))

    def same():
        for got, want in zip((trials, params, config), keep):
            for g, w in zip(got if isinstance(got, list) else [got], want if isinstance(want, list) else [want]):
                assert set(g) == set(w) and all(np.array_equal(g[k], w[k]) for k in w)

    with pytest.raises(ValueError, match="missing"):
        vlgp_amd.refit_joint([dict(trials[0], missing=np.zeros((6, 3), bool)), trials[1]], params, config, verbose=False)
    with pytest.raises(ValueError, match="comm"):
        vlgp_amd.refit_joint(trials, params, config, verbose=False, comm=object())
    for key in ("mu", "w"):
        with pytest.raises(ValueError, match="'mu' / 'w'"):
            vlgp_amd.refit_joint([{k: v for k, v in trials[0].items() if k != key}, trials[1]], params, config, verbose=False)
    same()


# ---- the host frame of the call ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_driver(tmp_path_factory):
    """tests/joint_em_frame_driver.cpp as a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path_factory.mktemp("joint_em_frame") / "joint_em_frame_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vlgp_amd", "csrc"), os.path.join(ROOT, "tests", "joint_em_frame_driver.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


def _run(exe, *args):
    done = subprocess.run([exe, args[0]] + [str(int(v)) for v in args[1:]], capture_output=True, timeout=60)
    assert done.returncode == 0, done.stderr.decode(errors="replace")[-3000:]
    return dict(ln.split(" ", 1) for ln in done.stdout.decode().splitlines())


@pytest.mark.parametrize("rows, L", [(1, 1), (301, 3), (40000, 5), (977, 10)])
def test_moments_lie_behind_the_flag_in_order_without_overlap(frame_driver, rows, L):
    got = {k: int(v) for k, v in _run(frame_driver, "layout", rows, L).items()}
    assert got == {"first": 0, "mu": 1, "cov": 1 + rows * L, "need": 1 + rows * L + rows * (L * (L + 1) // 2)}
    assert _run(frame_driver, "walk", rows, L) == {"ok": str(got["need"])}


@pytest.mark.parametrize("args, status, text", [
    ((10, 8, 0, 1, 1, 1, 1), 0, ""),
    ((11, 1, 0, 1, 1, 1, 1), -3, "more than 10 latents (L > 10)"),
    ((3, 9, 0, 1, 1, 1, 1), -3, "more than 8 regressors (P > 8)"),
    ((3, 1, 1, 1, 1, 1, 1), -3, "VLGP_MSTEP_GENERIC is set"),
    ((3, 1, 0, 2, 1, 1, 1), -3, "more than one rank"),
    ((3, 1, 0, 1, 0, 1, 1), -1, "needs mu"),
    ((3, 1, 0, 1, 1, 0, 1), -1, "needs cov"),
    ((3, 1, 0, 1, 1, 1, 0), -1, "n_iter must be at least 1"),
    ((11, 1, 0, 1, 0, 0, 0), -3, "more than 10 latents (L > 10)"),  # the limits of the kernels come first
])
def test_argument_checks_of_the_call(frame_driver, args, status, text):
    got = _run(frame_driver, "refuse", *args)
    assert int(got["status"]) == status and text in got.get("text", "") and got.get("text", "").startswith("vlgp_mstep_cov" if status else "")


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------
def test_matrix_names_every_compiled_size_and_geometry():
    exp = [c["expect"] for c in CS.MATRIX]
    lts, pts = CS.compiled_buckets()
    assert lts == [2, 3, 5, 8, 10] and pts == [1, 2, 4, 8]  # (L <= 10, P <= 8: what the issue asks to be compiled)
    assert {(e["LT"], e["PT"]) for e in exp} == {(lt, pt) for lt in lts for pt in pts}  # every instantiation is launched
    assert {(c["L"], c["expect"]["LT"]) for c in CS.MATRIX} >= {(1, 2), (2, 2), (3, 3), (4, 5), (5, 5), (7, 8), (8, 8), (10, 10)}
    assert {(c["P"], c["expect"]["PT"]) for c in CS.MATRIX} == {(1, 1), (2, 2), (3, 4), (8, 8)}
    assert {c["N"] for c in CS.MATRIX} >= {1, 63, 65, 130} and {c["cov"] for c in CS.MATRIX} == set(CS.COVS)
    assert any(c["all_gauss"] for c in CS.MATRIX) and any(c["gauss"] and not c["all_gauss"] for c in CS.MATRIX)
    assert {(e["fixed"], e["anyg"]) for e in exp} >= {(0, 1)} | {(f, g) for f in (3, 5, 8, 10) for g in (0, 1)}
    rows = {c["rows"] for c in CS.MATRIX}
    T, W = CS.MC_TILE, CS.WG_ROWS
    assert rows >= {1, W - 1, W, W + 1, T - 1, T, T + 1, 3 * W} and T < 2 * W  # (three workgroups: more than one tile's rows)
    for c in CS.MATRIX:
        assert c["P"] == 1 or c["rows"] >= 10 * c["P"], c["id"]  # x' diag(r) x has full rank: eps decides nothing
        inner = np.cumsum(c["lengths"])[:-1]
        if c["id"].startswith("e-"):
            assert not np.any(inner % T == 0), c["id"]
    # the LDS the launch asks for stays under 64 KB at every compiled size: tiles of (mu | cov) or the reduction buffer
    for lt in (2, 3, 5, 8, 10):
        assert (max(T * (lt + lt * (lt + 1) // 2), 8 * 512) + 64) * 8 < 64 * 1024


@pytest.mark.parametrize("cid", [c["id"] for c in CS.MATRIX])
def test_every_case_is_well_conditioned(cid):
    """On the statement alone: a random +-1 ulp perturbation of every mu and cov moves no channel's a, b or noise by more
    than a tenth of the bound the device is held to, after one and after three iterations; and the full covariances have
    the strong off-diagonals the case names."""
    p, want = CS.problem_and_reference(cid)
    c = CS.BY_ID[cid]
    rng = np.random.default_rng(1)
    ulp = lambda arr: np.nextafter(arr, np.where(rng.random(arr.shape) < 0.5, -np.inf, np.inf))
    moved_mu, moved_cov = ulp(p["mu"]), ulp(p["cov"])
    moved_cov = np.where(p["cov"] == 0.0, 0.0, moved_cov)
    moved_cov = np.tril(moved_cov) + np.tril(moved_cov, -1).transpose(0, 2, 1)
    worst = {}
    for n in CS.ITERS:
        base = want[n]
        moved = EM.mstep_cov(p["y"], p["x"], moved_mu, moved_cov, p["a"], p["b"], p["gauss"], n)
        ea, eb = per_channel_error(moved[0], moved[1], base[0], base[1])
        en = np.abs(moved[4] - base[4]) / np.maximum(np.abs(base[4]), 1e-300)
        worst[n] = (float(ea.max()), float(eb.max()), float(en.max()))
        assert all(np.all(np.isfinite(base[i])) for i in (0, 1, 4)) and EM.mstep_cov.n_failed == 0
    print("joint-em %-22s one-ulp perturbation of mu, cov (a, b, noise): %s" % (cid, worst))
    for n in CS.ITERS:
        assert max(worst[n]) < 0.1 * BOUND, (cid, n, worst[n])
    if c["cov"] == "full" and c["L"] > 1:
        d = np.sqrt(np.diagonal(p["cov"], axis1=1, axis2=2))
        corr = np.abs(p["cov"][:, 1, 0]) / (d[:, 1] * d[:, 0])
        assert np.all(corr > 0.79)
    if c["cov"] == "rank1":
        assert np.max(np.linalg.matrix_rank(p["cov"][:5])) == 1
    if c["cov"] == "zero":
        assert not p["cov"].any()
