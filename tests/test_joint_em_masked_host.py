"""The NumPy statement of vlgp_mstep_cov_masked and of the Laplace EM loop with missing observations
(tests/joint_em_masked_numpy.py) against the statements it restricts -- joint_em_numpy.mstep_cov with an empty mask,
masked_fit_numpy.mstep_masked with a diagonal covariance -- and against finite differences; the loop's rules; refit_joint's
refusals; the ABI and Python surface; the host frame of the call; the conditioning of the cases the GPU tests run
(tests/joint_em_masked_cases.py).  No GPU.

STAGE = 1e-9 is the project's stage-wise tolerance."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import joint_em_cases as CS
import joint_em_masked_cases as MC
import joint_em_masked_numpy as EMM
import joint_em_numpy as EM
import masked_fit_numpy as MF
from test_gpu_rates import per_channel_error
from test_joint_em_host import _small, diag_cov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = 1e-9
# the bound the GPU tests hold the device to (tests/test_gpu_joint_em_masked.py): the cases must be conditioned for it
from test_gpu_joint_em_masked import BOUND  # noqa: E402


def _mask(shape, seed, fraction=0.3):
    return np.random.default_rng(seed).random(shape) < fraction


# ---- the statement against the statements it restricts ----------------------------------------------------------------
@pytest.mark.parametrize("n_iter", [1, 3])
def test_an_empty_mask_is_the_unmasked_statement_exactly(n_iter):
    """Every channel on all rows, one by one, is joint_em_numpy.mstep_cov on all channels at once: the same bits, the noise
    included -- the per-channel sums of that statement do not depend on the other channels."""
    y, x, mu, cov, a, b = _small(13)
    gauss = np.zeros(a.shape[1], bool)
    want = EM.mstep_cov(y, x, mu, cov, a, b, gauss, n_iter)
    got = EMM.mstep_cov_masked(y, x, mu, cov, a, b, np.zeros(y.shape, bool), n_iter)
    for k, g, w in zip(("a", "b", "da", "db", "noise"), got, want):
        assert np.array_equal(g, w), (k, float(np.max(np.abs(g - w))))


@pytest.mark.parametrize("n_iter", [1, 3])
def test_a_diagonal_cov_is_the_masked_mean_field_statement(n_iter):
    """cov = diag(v): masked_fit_numpy.mstep_masked (the pinned oracle's M-step on each channel's observed rows).  The
    statement writes the diagonal part of every sum as the oracle writes its v terms and adds exact zeros for the rest
    (joint_em_numpy.split_cov), so the bound is that of two orders of the same sums: STAGE; measured gap 3.3e-16."""
    y, x, mu, cov, a, b = _small(17)
    v = np.ascontiguousarray(np.diagonal(cov, axis1=1, axis2=2))
    missing = _mask(y.shape, 5)
    missing[:, 2] = True  # ... and a channel without an observed row keeps a, b, noise on both sides
    noise = 0.5 + np.arange(a.shape[1], dtype=float)
    want = MF.mstep_masked(y, x, mu, v, a, b, missing, n_iter, noise=noise)
    got = EMM.mstep_cov_masked(y, x, mu, diag_cov(v), a, b, missing, n_iter, noise=noise)
    gap = max(float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1.0))) for g, w in zip(got, want))
    print("joint-em-masked diagonal cov against mstep_masked, Mniter %d: largest gap %.2e" % (n_iter, gap))
    assert gap < STAGE
    assert np.array_equal(got[0][:, 2], a[:, 2]) and np.array_equal(got[1][:, 2], b[:, 2]) and got[4][2] == noise[2]
    assert not got[2][:, 2].any() and not got[3][:, 2].any()


def test_what_y_holds_at_a_missing_entry_is_never_read():
    y, x, mu, cov, a, b = _small(19)
    missing = _mask(y.shape, 6)
    want = EMM.mstep_cov_masked(y, x, mu, cov, a, b, missing, 3)
    got = EMM.mstep_cov_masked(np.where(missing, np.nan, y), x, mu, cov, a, b, missing, 3)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_gradient_and_hessian_are_the_derivatives_of_the_masked_expected_log_likelihood():
    """Q(a_n) = sum over the observed rows of y (a.mu + x b) - exp(a.mu + x b + a'C_t a / 2).  grad_a against central
    differences of Q, nhess_a against central differences of the gradient, step h = 1e-5, both held at 1e-8 of the scale
    S = sum |terms of Q| (truncation h^2 Q''' / 6 ~ 1e-10 S, rounding 1e-16 S / h = 1e-11 S: tests/test_joint_em_host.py);
    and one Newton iteration of the statement at eps = 0 is the step H^-1 g."""
    y, x, mu, cov, a, b = _small(7)
    missing = _mask(y.shape, 8)
    h = 1e-5
    out = EMM.mstep_cov_masked(y, x, mu, cov, a, b, missing, 1, eps=0.0)
    for n in range(a.shape[1]):
        args = (y[:, n], x[:, :, n], mu, cov)
        g, H = EMM.grad_hess_a_masked(*args, a[:, n], b[:, n], missing[:, n])
        S = EMM.masked_Q(*args, a[:, n], b[:, n], missing[:, n])[1]
        for l in range(a.shape[0]):
            e = np.zeros(a.shape[0])
            e[l] = h
            fd = (EMM.masked_Q(*args, a[:, n] + e, b[:, n], missing[:, n])[0]
                  - EMM.masked_Q(*args, a[:, n] - e, b[:, n], missing[:, n])[0]) / (2 * h)
            assert abs(fd - g[l]) < 1e-8 * S, (n, l, fd, g[l])
            fd_h = -(EMM.grad_hess_a_masked(*args, a[:, n] + e, b[:, n], missing[:, n])[0]
                     - EMM.grad_hess_a_masked(*args, a[:, n] - e, b[:, n], missing[:, n])[0]) / (2 * h)
            assert np.max(np.abs(fd_h - H[l])) < 1e-8 * S, (n, l)
        assert np.max(np.abs(out[2][:, n] - np.linalg.solve(H, g))) < STAGE * max(1.0, np.max(np.abs(out[2][:, n])))
    # the missing rows really are left out: the gradient differs from the unmasked one
    g_all = EM.grad_hess_a(y[:, 0], mu, cov, a, b, x, 0)[0]
    assert np.max(np.abs(g_all - EMM.grad_hess_a_masked(y[:, 0], x[:, :, 0], mu, cov, a[:, 0], b[:, 0], missing[:, 0])[0])) > 1.0


# ---- the loop ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    units, params, gauss, missing = EMM.tiny_problem()
    args = (params["a"], params["b"], params["noise"], gauss, params["cholesky"])
    runs = {"five": EMM.refit_masked(units, missing, *args, 25, max_iter=5, tol=0.0)}
    return {"units": units, "missing": missing, "params": params, "gauss": gauss, "args": args, "runs": runs}


def test_the_tiny_problem_has_the_shape_the_issue_names(tiny):
    lengths = [u["y"].shape[0] for u in tiny["units"]]
    assert len(lengths) == 6 and len(set(lengths)) > 1 and all(20 <= T <= 40 for T in lengths)
    assert tiny["params"]["a"].shape == (2, 8) and not tiny["gauss"].any()
    frac = np.concatenate(tiny["missing"]).mean()
    assert 0.25 < frac < 0.35 and np.all((~np.concatenate(tiny["missing"])).sum(axis=0) > 0)


def test_the_loops_rules_hold_with_a_mask(tiny):
    units, missing, args = tiny["units"], tiny["missing"], tiny["args"]
    base = tiny["runs"]["five"]
    E = base["trace"]["laplace"]
    print("joint-em-masked statement trace %s" % E)
    assert len(E) == 6 and all(base["trace"]["converged"]) and base["kept"] == 5
    assert np.all(np.diff(E[:3]) > 1e-3)  # the first M-steps raise the evidence of the observed entries
    # the evidence is that of the observed entries: below (in magnitude) the evidence of all entries, whatever y holds
    full = EM.refit(units, *args, 25, max_iter=0)["trace"]["laplace"][0]
    assert abs(E[0]) < abs(full)
    # max_iter: iteration max_iter is evaluated and returned, no M-step after it
    run2 = EMM.refit_masked(units, missing, *args, 25, max_iter=2, tol=0.0)
    assert len(run2["trace"]["laplace"]) == 3 and run2["kept"] == 2 and run2["trace"]["laplace"] == E[:3]
    # the stop rule: the first k whose relative gain is <= tol, keeping the last one when the evidence did not fall
    gains = [(E[k] - E[k - 1]) / abs(E[k]) for k in range(1, len(E))]
    k_stop = 2
    tol = 0.5 * (gains[k_stop - 2] + gains[k_stop - 1])
    assert gains[k_stop - 1] <= tol < min(gains[:k_stop - 1])
    run = EMM.refit_masked(units, missing, *args, 25, max_iter=5, tol=tol)
    assert len(run["trace"]["laplace"]) == k_stop + 1 and run["kept"] == k_stop
    # an evidence that falls: the parameters and the posterior of the iteration before come back
    fall = EMM.refit_masked(units, missing, *args, 25, max_iter=5, tol=0.0, trace_hook=lambda k, ev: ev - 50.0 if k == 2 else ev)
    one = EMM.refit_masked(units, missing, *args, 25, max_iter=1, tol=0.0)
    assert len(fall["trace"]["laplace"]) == 3 and fall["kept"] == 1
    for key in ("a", "b", "noise", "da", "db", "mu", "cov"):
        assert np.array_equal(fall[key], one[key]), key
    # without an M-step the caller's parameters come back with their masked posterior
    zero = EMM.refit_masked(units, missing, *args, 25, max_iter=0)
    assert zero["da"] is None and np.array_equal(zero["a"], args[0]) and len(zero["trace"]["laplace"]) == 1
    # ... and y at the missing entries reaches nothing
    nan_units = [dict(u, y=np.where(m, np.nan, u["y"])) for u, m in zip(units, missing)]
    again = EMM.refit_masked(nan_units, missing, *args, 25, max_iter=1, tol=0.0)
    assert again["trace"]["laplace"] == one["trace"]["laplace"] and np.array_equal(again["a"], one["a"])


# ---- refit_joint's refusals -------------------------------------------------------------------------------------------
def test_refit_joint_refuses_before_an_engine_exists_and_touches_nothing(monkeypatch):
    import vlgp_amd
    from vlgp_amd import engine

    def no_engine(*args, **kwargs):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(engine.Engine, "for_params", no_engine)
    rng = np.random.default_rng(0)
    trials = [{"y": rng.poisson(1.0, (6, 3)).astype(float), "mu": rng.standard_normal((6, 2)), "w": rng.random((6, 2)),
               "v": rng.random((6, 2))} for _ in range(2)]
    params = {"ydim": 3, "zdim": 2, "xdim": 1, "rank": 4, "a": rng.standard_normal((2, 3)), "b": np.zeros((1, 3)),
              "noise": np.ones(3), "likelihood": np.array(["poisson"] * 3), "omega": np.ones(2), "sigma": np.ones(2)}
    config = {"Mniter": 3, "use_hessian": True, "eps": 1e-8, "learning_rate": 1.0, "da_bound": 5.0, "db_bound": 5.0}
    some = [rng.random((6, 3)) < 0.3 for _ in range(2)]
    keep = copy.deepcopy((trials, params, config, some))

    def refused(match, trials_=trials, params_=params, **kw):
        with pytest.raises(ValueError, match=match):
            vlgp_amd.refit_joint(trials_, params_, config, verbose=False, **kw)

    refused("missing", [dict(trials[0], missing=some[0]), trials[1]])  # some trials carry one, some do not
    refused("comm", missing=some, comm=object())
    refused("'mu' / 'w'", [{k: v for k, v in trials[0].items() if k != "w"}, trials[1]], missing=some)
    refused("Poisson channels only", params_=dict(params, likelihood=np.array(["poisson", "gaussian", "poisson"])), missing=some)
    dead = [m.copy() for m in some]
    for m in dead:
        m[:, 1] = True
    refused(r"channel\(s\) \[1\] have no observed entry", missing=dead)
    refused(r"channel\(s\) \[1\] have no observed entry", [dict(tr, missing=m) for tr, m in zip(trials, dead)])
    refused("missing", missing=some[:1])  # one array per trial
    refused("missing", missing=[m[:5] for m in some])  # ... of the trial's shape
    for got, want in zip((trials, params, config), keep[:3]):
        for g, w in zip(got if isinstance(got, list) else [got], want if isinstance(want, list) else [want]):
            assert set(g) == set(w) and all(np.array_equal(g[k], w[k]) for k in w)
    assert all(np.array_equal(m, k) for m, k in zip(some, keep[3]))


# ---- bindings and tables ----------------------------------------------------------------------------------------------
def test_abi_and_python_surface():
    import inspect

    import vlgp_amd
    from vlgp_amd import _lib

    text = open(os.path.join(ROOT, "include", "vlgp_hip.h")).read()
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3 and _lib.ABI_VERSION == 3
    decl = re.search(r"int vlgp_mstep_cov_masked\(([^;]*)\);", text)
    same = re.search(r"int vlgp_mstep_cov\(([^;]*)\);", text)
    norm = lambda m: [" ".join(a.split()) for a in m.group(1).split(",")]  # noqa: E731
    assert decl and norm(decl) == norm(same) and len(norm(decl)) == 11  # the argument list of vlgp_mstep_cov
    assert "vlgp_mstep_cov_masked" in _lib.EXPORTS
    assert _lib._SIGNATURES["vlgp_mstep_cov_masked"] == _lib._SIGNATURES["vlgp_mstep_cov"]
    assert hasattr(_lib.load(), "vlgp_mstep_cov_masked")
    assert callable(vlgp_amd.Engine.mstep_cov_masked)
    assert (inspect.signature(vlgp_amd.Engine.mstep_cov_masked).parameters.keys()
            == inspect.signature(vlgp_amd.Engine.mstep_cov).parameters.keys())
    assert inspect.signature(vlgp_amd.refit_joint).parameters["missing"].default is None
    api = open(os.path.join(ROOT, "vlgp_amd", "csrc", "api.hip")).read()
    assert re.search(r"X\(vlgp_mstep_cov_masked, SET_MASKED_FIT,\s*\\\n\s*\"vlgp_mstep_cov_masked takes a masked fit set", api)
    assert "X(vlgp_mstep_cov, NOT_REPLICATED, nullptr)" in api  # ... beside the unmasked row, which stays
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "| `vlgp_mstep_cov_masked` | a masked fit set |" in design
    assert "vlgp_mstep_cov_masked" in text[text.index("ONE replica (n_rep == 1) makes a masked fit set"):
                                           text.index("int vlgp_replicate_masked(")]


def test_the_launchers_name_the_whole_matrix_and_leave_the_old_lists():
    src = open(os.path.join(ROOT, "vlgp_amd", "csrc", "mstep_cov.hip")).read()
    lts = sorted(int(v) for v in re.findall(r"case \d+: return launch_cov_masked_p<(\d+)>", src))
    pts = sorted(int(v) for v in re.findall(r"case \d+: hipLaunchKernelGGL\(\(mstep_cov_accum_masked<LT, (\d+)>\)", src))
    assert (lts, pts) == CS.compiled_buckets() == ([2, 3, 5, 8, 10], [1, 2, 4, 8])
    assert "atomic" not in open(os.path.join(ROOT, "vlgp_amd", "csrc", "mstep_cov_accum.inc")).read()


# ---- the host frame of the call ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_driver(tmp_path_factory):
    """tests/joint_em_masked_frame_driver.cpp as a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path_factory.mktemp("joint_em_masked_frame") / "joint_em_masked_frame_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vlgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "joint_em_masked_frame_driver.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _run(exe, *args):
    done = subprocess.run([exe, args[0]] + [str(int(v)) for v in args[1:]], capture_output=True, timeout=60)
    assert done.returncode == 0, done.stderr.decode(errors="replace")[-3000:]
    return dict(ln.split(" ", 1) for ln in done.stdout.decode().splitlines())


@pytest.mark.parametrize("rows, L", [(1, 1), (334, 4), (977, 10)])
def test_the_moments_block_is_that_of_the_unmasked_call(frame_driver, rows, L):
    got = {k: int(v) for k, v in _run(frame_driver, "layout", rows, L).items()}
    assert got == {"first": 0, "mu": 1, "cov": 1 + rows * L, "need": 1 + rows * L + rows * (L * (L + 1) // 2)}
    assert _run(frame_driver, "walk", rows, L) == {"ok": str(got["need"])}


@pytest.mark.parametrize("args, status, text", [
    # n_gauss L P generic world mu cov n_iter
    ((0, 10, 8, 0, 1, 1, 1, 1), 0, ""),
    ((1, 3, 1, 0, 1, 1, 1, 1), -3, "the handle has Gaussian channels"),
    ((0, 11, 1, 0, 1, 1, 1, 1), -3, "more than 10 latents (L > 10)"),
    ((0, 3, 9, 0, 1, 1, 1, 1), -3, "more than 8 regressors (P > 8)"),
    ((0, 3, 1, 1, 1, 1, 1, 1), -3, "VLGP_MSTEP_GENERIC is set"),
    ((0, 3, 1, 0, 2, 1, 1, 1), -3, "more than one rank"),
    ((0, 3, 1, 0, 1, 0, 1, 1), -1, "needs mu"),
    ((0, 3, 1, 0, 1, 1, 0, 1), -1, "needs cov"),
    ((0, 3, 1, 0, 1, 1, 1, 0), -1, "n_iter must be at least 1"),
    ((2, 11, 9, 1, 2, 0, 0, 0), -3, "the handle has Gaussian channels"),  # the Gaussian channel first,
    ((0, 11, 1, 0, 1, 0, 0, 0), -3, "more than 10 latents (L > 10)"),      # then the limits of the kernels, then the arguments
])
def test_argument_checks_of_the_call(frame_driver, args, status, text):
    got = _run(frame_driver, "refuse", *args)
    assert int(got["status"]) == status and text in got.get("text", "")
    assert got.get("text", "").startswith("vlgp_mstep_cov_masked" if status else "")


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------
def test_matrix_names_every_compiled_size_geometry_and_mask():
    exp = [c["expect"] for c in MC.MATRIX]
    lts, pts = CS.compiled_buckets()
    assert {(e["LT"], e["PT"]) for e in exp} == {(lt, pt) for lt in lts for pt in pts}  # every instantiation is launched
    # exact and padded: L = LT, and L = LT - 1 wherever the bucket holds more than one latent count
    for pt, P in zip(pts, (1, 2, 4, 8)):
        assert {c["L"] for c in MC.MATRIX if c["P"] == P and c["id"].startswith("a-")} == {1, 2, 3, 4, 5, 7, 8, 9, 10}
    assert {c["N"] for c in MC.MATRIX} >= {1, 31, 32, 33, 63, 64, 65, 130}
    assert {c["cov"] for c in MC.MATRIX} == set(CS.COVS) and {c["mask"] for c in MC.MATRIX} == set(MC.MASKS)
    rows = {c["rows"] for c in MC.MATRIX}
    T = MC.MC_TILE
    assert rows >= {T - 1, T, T + 1, 334} and not any(c["gauss"] for c in MC.MATRIX)
    for c in MC.MATRIX:
        assert c["P"] == 1 or c["rows"] >= 10 * c["P"], c["id"]
    # a dead channel in the upper half of a mask word and in a second word
    assert MC.DEAD_CHANNEL[24] >> 5 == 0 and MC.DEAD_CHANNEL[24] > 15 and MC.DEAD_CHANNEL[65] >> 6 == 1


@pytest.mark.parametrize("cid", [c["id"] for c in MC.MATRIX])
def test_every_case_is_well_conditioned(cid):
    """On the statement alone: no Newton system fails to factor, a dead channel is exactly the one the case names and every
    other channel keeps at least twenty observed rows for each of its L + P unknowns' worth of data (so that eps decides
    nothing); a random +-1 ulp perturbation of every mu and cov moves no channel's a, b or noise by more than a tenth of
    the bound the device is held to, after one and after three iterations."""
    p, want = MC.problem_and_reference(cid)
    c = MC.BY_ID[cid]
    n_obs = (~p["missing"]).sum(axis=0)
    dead = np.flatnonzero(n_obs == 0)
    assert dead.tolist() == ([MC.DEAD_CHANNEL[c["N"]]] if c["mask"] == "dead-channel" else [])
    alive = n_obs > 0
    assert np.all(n_obs[alive] >= max(20, 3 * (c["L"] + c["P"]))), (cid, int(n_obs[alive].min()))
    frac = p["missing"][:, alive].mean()
    assert 0.2 < frac < 0.5, (cid, frac)
    if c["mask"] == "dead-row":
        assert p["missing"].all(axis=1).sum() == 3
    if c["mask"] == "dead-unit":
        s = int(np.sum(c["lengths"][:2]))
        assert p["missing"][s:s + c["lengths"][2]].all() and not p["missing"][:s].all(axis=1).any()
    rng = np.random.default_rng(1)
    ulp = lambda arr: np.nextafter(arr, np.where(rng.random(arr.shape) < 0.5, -np.inf, np.inf))  # noqa: E731
    moved_mu, moved_cov = ulp(p["mu"]), ulp(p["cov"])
    moved_cov = np.where(p["cov"] == 0.0, 0.0, moved_cov)
    moved_cov = np.tril(moved_cov) + np.tril(moved_cov, -1).transpose(0, 2, 1)
    worst = {}
    for n in MC.ITERS:
        base = want[n]
        moved = MC.statement(dict(p, mu=moved_mu, cov=moved_cov), n)
        assert EMM.mstep_cov_masked.n_failed == 0
        ea, eb = per_channel_error(moved[0], moved[1], base[0], base[1])
        en = np.abs(moved[4] - base[4]) / np.maximum(np.abs(base[4]), 1e-300)
        worst[n] = (float(ea.max()), float(eb.max()), float(en.max()))
        assert all(np.all(np.isfinite(base[i])) for i in (0, 1, 4))
        for d in dead:  # the dead channel keeps a, b, noise and steps by 0
            assert np.array_equal(base[0][:, d], p["a"][:, d]) and np.array_equal(base[1][:, d], p["b"][:, d])
            assert base[4][d] == 1.0 and not base[2][:, d].any() and not base[3][:, d].any()
    print("joint-em-masked %-22s one-ulp perturbation of mu, cov (a, b, noise): %s" % (cid, worst))
    for n in MC.ITERS:
        assert max(worst[n]) < 0.1 * BOUND, (cid, n, worst[n])
