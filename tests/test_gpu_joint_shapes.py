"""The joint Laplace kernels of csrc/joint.hip at every size they treat differently: D up to 512 and around 256, rank 64,
L R and unit lengths past 256, 136 pairs of latents, exact multiples of the factor's panel, starts from which full steps
are rejected, and masked sets with two mask words -- the case table of tests/joint_shapes.py (whose docstring names, per
case, the loop or size it is the only one to reach), against the NumPy statements tests/joint_numpy.py and
tests/joint_cov_numpy.py.  tests/test_joint_shapes_host.py proves the table's ranks, D and convergence on the CPU.

Tolerance.  TOL = 5e-13 of tests/test_gpu_joint.py for every case and every quantity, with that file's and
tests/test_gpu_joint_cov.py's error definitions (imported): no case needed a bound of its own.  log_w is taken as
test_draws_equal_the_statement_at_the_devices_own_mode takes it, relative to the sum of the absolute terms behind it, but
against the statement at ITS OWN mode: both sides stop at a decrement <= 1e-20, so their modes differ by rounding.
Every case prints its errors (profiles/joint/measured_errors.txt, profiles/joint_cov/measured_errors.txt; the largest
over the table: v and cov 2.4e-15, log_w 2.0e-14 in the halving case).
"""
import numpy as np
import pytest

import joint_numpy as JN
import joint_shapes as JS
from test_gpu_joint import NEWTON_TOL, TOL, _errors as laplace_errors, _grad_norms
from test_gpu_joint_cov import REP, _errors as posterior_errors, _mask
from test_gpu_marginal import SET, _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _table_ranks(name):
    return np.array([r for _, r in JS.CASES[name]["units"]])


def _check_run(name, dev, st):
    assert np.array_equal(dev["D"], JS.dims(name))
    assert dev["n_failed"] == 0 and np.all(dev["converged"]) and np.all(dev["decrement"] <= NEWTON_TOL), (
        name, dev["n_failed"], dev["converged"], dev["decrement"])
    for i, s in enumerate(st):
        for l, r in enumerate(s["ranks"]):
            assert not np.any(dev["beta"][i, l, r:]), "beta beyond the rank must be zero"
    gn = _grad_norms(dev, st)
    assert np.all(gn <= 1e-6), gn


@pytest.mark.parametrize("name", sorted(JS.CASES))
def test_plain_set_equals_the_statements(V, name):
    units, params, gauss = JS.problem(name)
    st = JS.reference(name)
    eps = JS.draws(name)
    with _engine(V, units, params, gauss) as eng:
        ranks = eng.unit_ranks(SET)
        lap = eng.joint_laplace(SET, max_iter=50, tol=NEWTON_TOL, eps=eps)
        lap2 = eng.joint_laplace(SET, max_iter=50, tol=NEWTON_TOL, eps=eps)
        post = eng.joint_posterior(SET, max_iter=50, tol=NEWTON_TOL)
        post2 = eng.joint_posterior(SET, max_iter=50, tol=NEWTON_TOL)
    assert np.array_equal(ranks, _table_ranks(name))
    _check_run(name, lap, st)
    _check_run(name, post, st)
    err = laplace_errors(name, lap, st, units)
    err["log_w"] = max(float(np.max(np.abs(lap["log_w"][i] - s["log_w"]) / s["scale_k"])) for i, s in enumerate(st))
    print("joint errors [%s] log_w %.2e; newton of the statement %s, halvings %s"
          % (name, err["log_w"], [s["n_newton"] for s in st], [s["halvings"] for s in st]))
    err_cov = posterior_errors(name, post, st, units)
    for key, val in list(err.items()) + list(err_cov.items()):
        assert val <= TOL, (name, key, val)
    assert np.array_equal(lap["parts"][:, :, 0] + lap["parts"][:, :, 1], lap["log_w"])
    # the bits: cov's diagonal is v, the posterior is the Laplace call's, a repeated call repeats
    assert np.ascontiguousarray(np.diagonal(post["cov"], axis1=1, axis2=2)).tobytes() == lap["v"].tobytes()
    assert np.array_equal(post["cov"], post["cov"].transpose(0, 2, 1))
    for key in ("beta", "stats", "mu"):
        assert post[key].tobytes() == lap[key].tobytes(), key
    for key in ("beta", "stats", "mu", "v", "log_w", "parts"):
        assert lap[key].tobytes() == lap2[key].tobytes(), key
    for key in ("beta", "stats", "mu", "cov"):
        assert post[key].tobytes() == post2[key].tobytes(), key
    if name == "halving":  # the statement rejects a full step from this start; the device reaches the mode from it all the same
        assert min(s["halvings"] for s in st) >= 1
    if name == "late_rows_300":  # (what the rejected steps of this unit hang on: test_joint_shapes_host.py)
        assert st[0]["halvings"] >= 1


@pytest.mark.parametrize("name", JS.MASKED)
def test_masked_set_equals_the_statement(V, name):
    """joint_rows_masked from beta = 0 at D = 512 (one mask word) and at T = 600 with N = 70 (two)."""
    units, params, gauss = JS.problem(name)
    rows, N = sum(u["y"].shape[0] for u in units), params["ydim"]
    held = JS.mask(name)
    assert np.array_equal(held, _mask("random", rows, N)) and (N > 64) == (name == "rows_256_257_600")
    st = JS.masked_reference(name)
    poisoned, row = [], 0
    for u in units:  # NaN where held out: the device never reads it
        T = u["y"].shape[0]
        poisoned.append(dict(u, y=np.where(held[row:row + T], np.nan, u["y"])))
        row += T
    with _engine(V, poisoned, params, gauss) as eng:
        eng.replicate(SET, REP, held_out=held[None])
        dev = eng.joint_posterior(REP, max_iter=50, tol=NEWTON_TOL)
        again = eng.joint_posterior(REP, max_iter=50, tol=NEWTON_TOL)
        eng.free_units(REP)
    _check_run(name, dev, st)
    for key in ("beta", "stats", "mu", "cov"):
        assert np.all(np.isfinite(dev[key])), key
        assert dev[key].tobytes() == again[key].tobytes(), key
    err = posterior_errors("%s masked random" % name, dev, st, units)
    for key, val in err.items():
        assert val <= TOL, (name, key, val)


def test_D_513_is_refused_beside_an_accepted_D_512(V):
    """L = 9 at R = 64: [64] * 8 and one more column on the ninth latent is refused by name; [64] * 7 + [63, 1] in another
    set of the same engine is taken."""
    R, L, N = 64, 9, 4
    rng = np.random.default_rng(5)
    om = JS.omega(L)
    sets = {SET: (70, [64] * 8 + [1]), 1: (72, [64] * 7 + [63, 1])}
    params = {"ydim": N, "zdim": L, "xdim": 1, "rank": R, "a": 0.15 * rng.standard_normal((L, N)), "b": np.zeros((1, N)),
              "noise": np.ones(N), "cholesky": {T: np.stack([JS.factor(T, om[l], R, r) for l, r in enumerate(ranks)])
                                                for T, ranks in sets.values()}}
    gauss = np.zeros(N, bool)
    unit = {T: {"y": rng.poisson(1.0, (T, N)).astype(float), "x": None, "mu": np.zeros((T, L)), "v": np.zeros((T, L)),
                "w": np.ones((T, L))} for T, _ in sets.values()}
    with _engine(V, [unit[70]], params, gauss) as eng:
        eng.upload(1, [unit[72]])
        assert eng.unit_ranks(SET).sum() == 513 and eng.unit_ranks(1).sum() == 512
        with pytest.raises(V.engine.VlgpError, match="status -3.*D = 513 weights, at most 512"):
            eng.joint_laplace(SET)
        with pytest.raises(V.engine.VlgpError, match="status -3.*D = 513 weights, at most 512"):
            eng.joint_posterior(SET)
        dev = eng.joint_laplace(1, max_iter=50, tol=NEWTON_TOL)
    st = JN.statement([unit[72]], params["a"], params["b"], params["noise"], gauss, params["cholesky"])
    assert dev["D"].tolist() == [512] and dev["n_failed"] == 0 and np.all(dev["converged"])
    err = laplace_errors("L9_D512_beside_the_refusal", dev, st, [unit[72]])
    for key, val in err.items():
        assert val <= TOL, (key, val)
