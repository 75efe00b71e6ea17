"""The NumPy statement of vlgp_joint_posterior and of the _cov row scores (tests/joint_cov_numpy.py) against closed forms
and against the statements it extends, the ABI of the three entry points, and the layout of their device blocks.  No GPU.

STAGE = 1e-9 is the project's stage-wise tolerance for two dense routes to the same number; where
the two sides are the same arithmetic the test asks for equal bits."""
import os
import re
import subprocess

import numpy as np
import pytest

import joint_cov_numpy as JC
import joint_numpy as JN
import predictive_numpy as PN
from test_gpu_marginal import _problem
from test_joint_host import shared_gaussian_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = 1e-9


@pytest.fixture(scope="module")
def mixed():
    """Two short units, five channels of which two are Gaussian, three latents; a random 20 % mask with one whole row and
    one whole channel, and the masked and the plain statement."""
    units, params, gauss = _problem([7, 40], 5, 3, [2e-2, 5e-3, 1e-3], seed=11, n_gauss=2)
    rng = np.random.default_rng(5)
    held = rng.random((47, 5)) < 0.2
    held[9] = True
    held[:, 1] = True
    args = (params["a"], params["b"], params["noise"], gauss, params["cholesky"])
    return {"units": units, "params": params, "gauss": gauss, "held": held, "args": args,
            "plain": JC.statement(units, *args), "masked": JC.statement(units, *args, held=held)}


def test_the_diagonal_of_cov_is_v_and_cov_is_symmetric_psd(mixed):
    for st in (mixed["plain"], mixed["masked"]):
        for s in st:
            assert s["converged"]
            assert np.array_equal(np.diagonal(s["cov"], axis1=1, axis2=2), s["v"])  # (the same einsum on the same block)
            assert np.max(np.abs(s["cov"] - s["cov"].transpose(0, 2, 1))) <= STAGE * np.max(np.abs(s["cov"]))
            sym = 0.5 * (s["cov"] + s["cov"].transpose(0, 2, 1))
            assert np.linalg.eigvalsh(sym).min() >= -STAGE * np.max(np.abs(s["cov"]))


def test_the_plain_statement_is_joint_numpys(mixed):
    want = JN.statement(mixed["units"], *mixed["args"])
    for s, w in zip(mixed["plain"], want):
        for key in ("beta", "mu", "v"):
            assert np.array_equal(s[key], w[key]), key
        assert s["laplace"] == w["laplace"] and s["n_newton"] == w["n_newton"]


def test_gaussian_channels_one_step_and_the_dense_posterior_covariance():
    units, a, b, noise, gauss, prior, _ = shared_gaussian_problem()
    L, N = a.shape
    st = JC.statement(units, a, b, noise, gauss, prior)
    for u, s in zip(units, st):
        T = u["y"].shape[0]
        assert s["converged"] and s["n_newton"] == 2  # (one step, and the factorisation that finds the decrement zero)
        # x = (x_1 ... x_L) latent-major in T L-space: prior K = blockdiag(G_l G_l'), y[t, n] = sum_l a[l, n] x[t, l] + b + e
        K = np.zeros((L * T, L * T))
        for l in range(L):
            K[l * T:(l + 1) * T, l * T:(l + 1) * T] = prior[T][l] @ prior[T][l].T
        A = np.zeros((T * N, L * T))
        for t in range(T):
            for l in range(L):
                A[t * N:(t + 1) * N, l * T + t] = a[l]
        S = A @ K @ A.T + np.kron(np.eye(T), np.diag(noise))
        post = K - K @ A.T @ np.linalg.solve(S, A @ K)
        want = np.array([[[post[l * T + t, m * T + t] for m in range(L)] for l in range(L)] for t in range(T)])
        assert np.max(np.abs(s["cov"] - want)) <= STAGE * max(1.0, np.max(np.abs(want)))


def test_an_empty_mask_is_the_plain_set_and_poisoned_entries_change_nothing(mixed):
    units, args, held = mixed["units"], mixed["args"], mixed["held"]
    empty = JC.statement(units, *args, held=np.zeros_like(held))
    for s, u in zip(empty, units):  # (an empty mask starts at beta = 0: the plain unit from the same start)
        U = JN.Unit(u, *args[:4], args[4][u["y"].shape[0]])
        bt = JN.newton(U, np.zeros(U.D), 1e-20)[0]
        assert np.array_equal(s["beta"], bt)
        assert np.array_equal(s["cov"], JC.cov_rows(U, JN.summary(U, bt)["H"]))
    for s, w in zip(empty, mixed["plain"]):  # ... and the mode does not depend on the start
        assert np.max(np.abs(s["beta"] - w["beta"])) <= STAGE and np.max(np.abs(s["cov"] - w["cov"])) <= STAGE
    poisoned, row = [], 0
    for u in units:
        T = u["y"].shape[0]
        poisoned.append(dict(u, y=np.where(held[row:row + T], np.nan, u["y"])))
        row += T
    for s, w in zip(JC.statement(poisoned, *args, held=held), mixed["masked"]):
        for key in ("beta", "mu", "cov"):
            assert np.array_equal(s[key], w[key]), key
        assert s["laplace"] == w["laplace"] and np.isfinite(s["laplace"])


def test_held_out_entries_move_the_posterior(mixed):
    gap = max(float(np.max(np.abs(s["mu"] - w["mu"]))) for s, w in zip(mixed["masked"], mixed["plain"]))
    assert gap > 1e-3
    for s, w in zip(mixed["masked"], mixed["plain"]):  # fewer observations: no latent variance shrinks
        assert np.all(s["v"] >= w["v"] * (1.0 - STAGE))


def test_a_diagonal_cov_is_predictive_numpys_lpd(mixed):
    units, (a, b, noise, gauss, _) = mixed["units"], mixed["args"]
    mu = np.concatenate([u["mu"] for u in units])[None]
    v = np.concatenate([u["v"] for u in units])
    cov = np.zeros((1,) + v.shape + (v.shape[1],))
    cov[0, :, np.arange(3), np.arange(3)] = v.T
    lpd, rate, sums = JC.score_predictive(units, mu, cov, a, b, noise, gauss, 12)
    ones = [dict(u, x=np.ones((u["y"].shape[0], 1, 5))) for u in units]  # (predictive_numpy takes x as an array)
    want = PN.score_plain(ones, a, b, noise, gauss, True, 12)
    for got, ref in zip((lpd, rate, sums), want):
        assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))


def test_entries_without_finite_moments_are_nan_or_skipped(mixed):
    units, (a, b, noise, gauss, _) = mixed["units"], mixed["args"]
    st = mixed["plain"]
    mu = np.concatenate([s["mu"] for s in st])[None]
    cov = np.concatenate([s["cov"] for s in st])[None].copy()
    cov[0, 3] = np.nan
    lpd, rate, sums = JC.score_predictive(units, mu, cov, a, b, noise, gauss, 12)
    assert np.all(np.isnan(lpd[3])) and np.all(np.isnan(rate[3])) and np.all(np.isfinite(np.delete(lpd, 3, axis=0)))
    assert np.all(np.isnan(sums[:, 0])) and np.all(np.isfinite(sums[:, 1]))
    cdf, csums, _ = JC.score_calibration(units, mu, cov, a, b, noise, gauss, 12, 10, [0.5, 0.9])
    assert np.all(np.isnan(cdf[3])) and np.all(csums[:, -1] == 1) and np.all(csums[:, -2] == 46)
    assert np.all(np.isfinite(csums))


def test_abi_and_python_surface():
    import vlgp_amd
    from vlgp_amd import _lib

    text = open(os.path.join(ROOT, "include", "vlgp_hip.h")).read()
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3 and _lib.ABI_VERSION == 3
    for name, n_args in (("vlgp_joint_posterior", 9), ("vlgp_predictive_cov", 10), ("vlgp_calibration_cov", 13)):
        assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name][1]) == n_args
        assert hasattr(_lib.load(), name)
    assert callable(vlgp_amd.Engine.joint_posterior)
    api = open(os.path.join(ROOT, "vlgp_amd", "csrc", "api.hip")).read()
    assert "X(vlgp_joint_posterior, NOT_REPLICATED | SET_MASKED_FIT, nullptr)" in api
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "| `vlgp_joint_posterior` | not replicated, or a masked fit set |" in design


def test_cov_packing_round_trip_and_public_argument_checks():
    from vlgp_amd import engine as E
    from vlgp_amd import evaluation as EV

    rng = np.random.default_rng(0)
    c = rng.random((5, 3, 3))
    c = c + c.transpose(0, 2, 1)
    packed = E.pack_cov(c, 5, 3)
    assert packed.shape == (5, 6) and np.array_equal(packed[:, [0, 2, 5]], np.diagonal(c, axis1=1, axis2=2))
    assert packed[2, 4] == c[2, 2, 1] and np.array_equal(E.unpack_cov(packed, 3), c)
    assert np.array_equal(E.pack_cov(packed, 5, 3), packed)
    with pytest.raises(ValueError, match="cov must be"):
        E.pack_cov(c[:4], 5, 3)
    trials = [{"y": np.zeros((4, 2))}]
    params, config = {"ydim": 2, "zdim": 1}, {"method": "VB", "max_iter": 1, "dmu_bound": 1.0}
    for call in (EV.leave_entries_out, EV.leave_group_out):
        with pytest.raises(ValueError, match="posterior='joint' needs predictive=True"):
            call(trials, params, config, posterior="joint")
        with pytest.raises(ValueError, match="posterior must be"):
            call(trials, params, config, predictive=True, posterior="laplace")
    with pytest.raises(ValueError, match="posterior must be"):
        EV.calibration(trials, params, config, posterior="laplace")


@pytest.fixture(scope="module")
def layout_driver(tmp_path_factory):
    """tests/joint_cov_layout_driver.cpp as a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path_factory.mktemp("joint_cov_layout") / "joint_cov_layout_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vlgp_amd", "csrc"), os.path.join(ROOT, "tests", "joint_cov_layout_driver.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


def _regions(exe, *args):
    done = subprocess.run([exe, args[0]] + [str(int(v)) for v in args[1:]], capture_output=True, timeout=60)
    assert done.returncode == 0, done.stderr.decode(errors="replace")[-3000:]
    return dict((k, int(v)) for k, v in (ln.split(" ") for ln in done.stdout.decode().splitlines()))


@pytest.mark.parametrize("sibling, rows, L", [(0, 0, 3), (777, 1, 1), (1001, 301, 3), (128, 40000, 5)])
def test_moments_layout(layout_driver, sibling, rows, L):
    """mu (rows, L) then cov (rows, L (L + 1) / 2) behind the sibling's block, in order, without overlap, up to need."""
    got = _regions(layout_driver, "moments", sibling, rows, L)
    assert got == {"mu": sibling, "cov": sibling + rows * L, "need": sibling + rows * L + rows * (L * (L + 1) // 2)}


@pytest.mark.parametrize("work, rows, L, M", [(10, 1, 1, 1), (123456, 337, 3, 5), (99, 40000, 5, 40)])
def test_joint_posterior_layout(layout_driver, work, rows, L, M):
    got = _regions(layout_driver, "posterior", work, rows, L, M)
    assert got == {"work": 0, "stats": work, "cov": work + 8 * M, "need": work + 8 * M + rows * (L * (L + 1) // 2)}
