"""The hyperparameter step of the Laplace EM on the device -- the window moments of vlgp_joint_posterior_moments
(Engine.joint_posterior(..., window=)) and vlgp_amd.refit_joint(..., hstep=True) -- against their NumPy statement
(tests/joint_hstep_numpy.py).

The moments.  Unit sets whose prior factors have EXACT ranks (tests/joint_shapes.py's ``factor``: oracle.ichol_gauss at a
rough omega with every column from r on zeroed), N = 5 channels, every unit of a set of its own length and with its own
rank pattern.  Per window length W the units are W - 1 (no window, beside ones that have some), W, W + 1, 2 W and 2 W + 1
rows long, or a ragged mixture; W runs over 2, 4, the sizes around a multiple of the kernel's 4 x 4 tile and of half its
64 x 64 sum (31, 32, 33), 50, 63 and 64; the ranks over 1, 3, 4, 5, 33, 64 and patterns that differ between the latents
of a unit; L over 1, 3, 5; one masked fit set has 70 channels (two mask words per row).

Tolerance of S: the error relative to max(1, largest entry of S), held at TOL = 5e-13, the bound of the joint suite
(tests/test_gpu_joint.py), whose cov -- the same two substitutions -- was measured at 2.4e-15.  An entry of S adds, per
window, a chain of r products over a chain of r products, and the windows and units on top: at most 2 r + n_w roundings of
2.2e-16 on terms that are bounded by the entry's own scale (Sigma_ll <= I, a row of a factor has norm <= 1), some 3e-14 at
r = 64 with every rounding in one direction, a tenth of the bound.  Every case prints its error; the largest measured on an
MI355X is 4.6e-16 (profiles/joint_hstep/measured_errors.txt).

S is symmetric to the bit by construction (the kernel sums the tiles at and below the diagonal and copies the mirror
images), two calls give equal bits, and everything vlgp_joint_posterior returns is returned bit for bit.

The loop.  refit_joint(hstep=True) against joint_hstep_numpy.refit_hstep on the tiny problems of joint_em_numpy and
joint_em_masked_numpy, and a run whose last iterate is rejected: omega, a, b, noise, mu, cov, the prior and the evidence
trace, twice.
  free    against the statement's own loop.  Its omega is SciPy's L-BFGS-B at its default tolerances on moments that
          differ from the device's in the last bit (4.6e-16 above), and that optimiser is no continuous function of
          them: on the CPU, perturbing the statement's S of the first iteration by 1e-16 ... 1e-12 relative moves its
          omega either by 1e-13 ... 1e-9 or by 6.3e-7 and by nothing in between, with the same iteration counts (a
          branch inside its line search; the objective's K^-1 S K^-1 amplifies the moments' rounding by up to
          1 / gp_noise^2).  Both sides stop where the optimiser's own tests let them; the jump is far below what those
          tests resolve.  From there the difference is carried through the factor into the next E-step.  The bounds are a
          hundred times the largest error measured on an MI355X per quantity (MEASURED_FREE), the project's
          convention.  The factors are compared as G G', which the order of the pivots of an incomplete Cholesky
          factorisation, itself a matter of last bits, leaves alone.
  pinned  against the statement's loop run on the DEVICE's omega_k (refit_hstep's omega_hook): everything but the
          optimiser's branch -- the moments handed on, the M-step, the rebuilt factors entry by entry, the E-step under
          them, the restore of a rejected iterate.  Largest measured 4.7e-15 (omega and the factors: equal bits); held
          at a hundred times that.
Every case prints both sets (profiles/joint_hstep/measured_errors.txt)."""
import functools

import numpy as np
import pytest

import joint_cov_numpy as JC
import joint_em_masked_numpy as EMM
import joint_em_numpy as EM
import joint_hstep_numpy as JH
import joint_shapes as JS
from test_gpu_joint import NEWTON_TOL, TOL
from test_gpu_joint_em_masked import BOUND_LOOP, loop_errors
from test_gpu_marginal import SET, _engine
from test_gpu_rates import STAGE

pytestmark = pytest.mark.gpu

MASKED = 2
# measured on an MI355X over the three loop tests (profiles/joint_hstep/measured_errors.txt; module docstring)
MEASURED_FREE = {"laplace": 1.37e-7, "a": 1.82e-6, "b": 2.21e-7, "noise": 2.06e-6, "mu": 6.13e-6, "cov": 1.23e-5,
                 "omega": 3.58e-5, "omega_trace": 3.58e-5, "prior_cov": 1.40e-5}
MEASURED_PINNED = 4.66e-15
BOUND_FREE = {k: 100.0 * e for k, e in MEASURED_FREE.items()}
BOUND_PINNED = min(100.0 * MEASURED_PINNED, STAGE)
CONFIG = {"Mniter": 5, "use_hessian": True, "eps": 1e-8, "learning_rate": 1.0, "da_bound": 5.0, "db_bound": 5.0,
          "method": "VB", "max_iter": 20, "dmu_bound": 5.0, "window": 10, "omega_bound": (5e-4, 5e-2)}
HYPER = {"gp_noise": 1e-4, "dt": 1}


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _lengths(W):
    return [W - 1, W, W + 1, 2 * W, 2 * W + 1]


# name: (W, R, N, [(length, ranks per latent)], masked)
CASES = {
    "W2_L3": (2, 5, 5, [(1, [1, 1, 1]), (2, [1, 2, 2]), (3, [3, 1, 2]), (4, [4, 3, 1]), (5, [5, 4, 3])], False),
    "W4_L1": (4, 5, 5, [(3, [3]), (4, [4]), (5, [5]), (8, [1]), (9, [3])], False),
    "W31_L5": (31, 33, 5, list(zip(_lengths(31), [[1, 3, 4, 5, 30], [31, 1, 5, 3, 4], [4, 32, 1, 3, 5], [33, 33, 33, 33, 33],
                                                   [5, 4, 33, 1, 3]])), False),
    "W32_L3": (32, 64, 5, list(zip(_lengths(32), [[31, 1, 3], [32, 4, 5], [33, 33, 1], [64, 33, 1], [64, 64, 5]])), False),
    "W33_L1": (33, 64, 5, list(zip(_lengths(33), [[32], [33], [4], [64], [5]])), False),
    "W50_L5": (50, 50, 5, list(zip(_lengths(50), [[49, 1, 3, 4, 5], [50, 50, 50, 50, 50], [33, 5, 4, 3, 1],
                                                   [50, 33, 50, 1, 4], [3, 50, 5, 33, 50]])), False),
    "W63_L3": (63, 64, 5, list(zip(_lengths(63), [[62, 1, 33], [63, 63, 63], [64, 3, 4], [64, 64, 64], [5, 64, 33]])), False),
    "W64_L5": (64, 64, 5, list(zip(_lengths(64), [[63, 1, 3, 4, 5], [64, 64, 64, 64, 64], [64, 33, 5, 1, 64],
                                                   [64, 64, 64, 64, 64], [33, 64, 4, 64, 3]])), False),
    "ragged_W50": (50, 64, 5, [(20, [20, 3]), (137, [64, 33]), (50, [5, 50]), (260, [33, 64]), (75, [1, 4])], False),
    "ragged_W4": (4, 16, 5, [(2, [1, 2, 1]), (30, [16, 3, 5]), (7, [4, 5, 7]), (64, [3, 16, 4]), (3, [1, 1, 3])], False),
    "masked_N70": (10, 16, 70, [(9, [9, 3, 1]), (10, [4, 10, 5]), (25, [16, 1, 16]), (31, [5, 16, 3])], True),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """(units, params, gauss, held, statement) of a case: Poisson counts drawn from the model under the cut factors, a
    random mean-field posterior to start from (tests/joint_shapes.py's ``problem``), the mask of a masked case (a fifth of
    the entries) and joint_cov_numpy.statement's per-unit dicts, computed once and shared."""
    W, R, N, spec, masked = CASES[name]
    L = len(spec[0][1])
    rng = np.random.default_rng(sum(map(ord, name)))
    a = 0.3 * rng.standard_normal((L, N)) * min(1.0, np.sqrt(8.0 / N))
    b = np.log(0.7) + 0.3 * rng.standard_normal((1, N))
    om = JS.omega(L)
    prior, units = {}, []
    for T, ranks in spec:
        assert T not in prior and len(ranks) == L and all(1 <= r <= min(T, R) for r in ranks), (name, T, ranks)
        prior[T] = np.stack([JS.factor(T, om[l], R, r) for l, r in enumerate(ranks)])
        lat = np.stack([prior[T][l] @ rng.standard_normal(R) for l in range(L)], axis=1)
        units.append({"y": rng.poisson(np.exp(lat @ a + b)).astype(float), "x": None, "mu": 0.3 * rng.standard_normal((T, L)),
                      "v": 0.05 * rng.random((T, L)), "w": rng.uniform(0.05, 2.0, (T, L))})
    gauss = np.zeros(N, bool)
    params = {"ydim": N, "zdim": L, "xdim": 1, "rank": R, "a": a, "b": b, "noise": np.ones(N), "cholesky": prior}
    held = rng.random((sum(T for T, _ in spec), N)) < 0.2 if masked else None
    st = JC.statement(units, a, b, params["noise"], gauss, prior, held=held)
    return units, params, gauss, held, st


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))


@pytest.mark.parametrize("name", sorted(CASES))
def test_window_moments_equal_the_statement(V, name):
    W = CASES[name][0]
    units, params, gauss, held, st = problem(name)
    L = params["zdim"]
    want, n_w = JH.window_moments(st, W)
    with _engine(V, units, params, gauss) as eng:
        sid = SET
        if held is not None:
            eng.replicate(SET, MASKED, held_out=held[None])
            sid = MASKED
        plain = eng.joint_posterior(sid, max_iter=50, tol=NEWTON_TOL)
        dev = eng.joint_posterior(sid, max_iter=50, tol=NEWTON_TOL, window=W)
        again = eng.joint_posterior(sid, max_iter=50, tol=NEWTON_TOL, window=W)
    S = dev["window_moments"]
    assert dev["n_failed"] == 0 and np.all(dev["converged"])
    assert dev["n_windows"] == n_w == JH.n_windows([u["y"].shape[0] for u in units], W)
    assert S.shape == (L, W, W) and np.all(np.isfinite(S))
    assert [r for s in st for r in s["ranks"]] == [r for _, ranks in CASES[name][3] for r in ranks]  # (the ranks are exact)
    for key in ("beta", "stats", "mu", "cov"):  # what vlgp_joint_posterior returns, bit for bit; and a second call
        assert dev[key].tobytes() == plain[key].tobytes(), key
        assert dev[key].tobytes() == again[key].tobytes(), key
    assert "window_moments" not in plain and "n_windows" not in plain
    assert S.tobytes() == again["window_moments"].tobytes()
    assert np.array_equal(S, S.transpose(0, 2, 1))
    err = _rel(S, want)
    cov_err = max(_rel(dev["cov"][r0:r0 + s["cov"].shape[0]], s["cov"])
                  for s, r0 in zip(st, np.cumsum([0] + [s["cov"].shape[0] for s in st])))
    print("joint_hstep moments [%s] W %d n_w %d D %s: S %.2e (largest entry %.3g), cov %.2e"
          % (name, W, n_w, dev["D"].tolist(), err, float(np.max(np.abs(want))), cov_err))
    assert err <= TOL, (name, err)


def test_a_failed_unit_makes_the_moments_nan_and_is_counted(V):
    units, params, gauss, _, _ = problem("W4_L1")
    bad = [dict(u) for u in units]
    w = bad[2]["w"].copy()
    w[3, 0] = np.nan  # (a NaN start, as tests/test_gpu_joint.py fails a unit: every pivot of its H is NaN)
    bad[2] = dict(bad[2], w=w)
    with _engine(V, bad, params, gauss) as eng:
        dev = eng.joint_posterior(SET, max_iter=50, tol=NEWTON_TOL, window=4)
    assert dev["n_failed"] == 1 and np.isnan(dev["laplace"][2]) and np.all(np.isnan(dev["window_moments"]))
    assert dev["n_windows"] == 0 + 1 + 2 + 2 + 3


def test_refusals_leave_parameters_and_the_set_as_they_were(V):
    from vlgp_amd.engine import VlgpError

    units, params, gauss, _, _ = problem("W4_L1")
    with _engine(V, units, params, gauss) as eng:
        before = (eng.get_params(), eng.download(SET))
        for window, word in ((1, "window = 1, need 2 <= window <= 64"), (65, "window = 65, need 2 <= window <= 64"),
                             (0, "window = 0"), (-3, "window = -3"), (10, r"as long as the window \(10\)")):
            with pytest.raises(VlgpError, match="vlgp_joint_posterior_moments: .*" + word):
                eng.joint_posterior(SET, window=window)
        with pytest.raises(VlgpError, match="max_iter = 0"):
            eng.joint_posterior(SET, max_iter=0, window=4)
        after = (eng.get_params(), eng.download(SET))
        for x, y in zip(before[0], after[0]):
            assert x.tobytes() == y.tobytes()
        for key in before[1]:
            assert before[1][key].tobytes() == after[1][key].tobytes(), key
        assert eng.joint_posterior(SET, window=4)["n_windows"] == 8  # ... and the handle goes on working
    # (the refusal of a rank above 64 cannot be reached on a handle, whose R is at most VLGP_MAX_RANK = 64: the host
    # driver of tests/test_joint_hstep_host.py walks it)


# ---- the loop ---------------------------------------------------------------------------------------------------------
def _want(units, params, gauss, missing, **kw):
    lengths = [u["y"].shape[0] for u in units]
    prior = {T: params["cholesky"][T] for T in set(lengths)}
    return JH.refit_hstep(units, params["a"], params["b"], params["noise"], gauss, prior, params["omega"], params["sigma"],
                          params["rank"], HYPER["gp_noise"], CONFIG["omega_bound"], CONFIG["window"], CONFIG["Mniter"],
                          dt=HYPER["dt"], missing=missing, max_iter=3, tol=0.0, **kw)


def _prior_cov(G):
    """(L, T, T): G_l G_l', the prior covariance a factor stands for -- what the order of its pivots leaves alone."""
    return np.einsum("lti,lsi->lts", G, G)


def _hstep_errors(tag, fit, want, entrywise):
    errs = loop_errors(fit, want)
    trace = fit["config"]["runtime"]["joint"]
    errs["omega"] = float(np.max(np.abs(fit["params"]["omega"] - want["omega"]) / want["omega"]))
    errs["omega_trace"] = float(np.max(np.abs(np.array(trace["omega"]) - np.array(want["trace"]["omega"]))
                                       / np.array(want["trace"]["omega"])))
    errs["prior_cov"] = max(_rel(_prior_cov(fit["params"]["cholesky"][T]), _prior_cov(G)) for T, G in want["prior"].items())
    if entrywise:
        errs["cholesky"] = max(_rel(fit["params"]["cholesky"][T], G) for T, G in want["prior"].items())
    print("joint_hstep refit_joint %-16s kept %d omega %s  " % (tag, want["kept"], fit["params"]["omega"].tolist())
          + "  ".join("%s %.2e" % kv for kv in errs.items()))
    return errs


def _check_loop(tag, fit, units, params, gauss, missing, want, **kw):
    """Both comparisons of the module docstring, printed, then asserted: the statement's own loop (``want``) at the
    measured bounds, and the statement's loop pinned to the device's omega at the tight one."""
    trace = fit["config"]["runtime"]["joint"]
    assert len(trace["omega"]) == len(trace["laplace"]) == len(want["trace"]["laplace"]) and all(trace["converged"])
    pinned = _want(units, params, gauss, missing, omega_hook=lambda k, om: np.array(trace["omega"][k]), **kw)
    assert pinned["kept"] == want["kept"] and len(pinned["trace"]["laplace"]) == len(trace["laplace"])
    free = _hstep_errors(tag + " free", fit, want, False)
    tight = _hstep_errors(tag + " pinned", fit, pinned, True)
    for k, e in free.items():
        assert e <= BOUND_FREE[k], (tag, "free", k, e)
    for k, e in tight.items():
        assert e <= BOUND_PINNED, (tag, "pinned", k, e)


@pytest.mark.parametrize("kind", ["plain", "missing"])
def test_refit_joint_with_hstep_follows_the_statements_loop(V, kind):
    if kind == "plain":
        units, params, gauss = EM.tiny_problem()
        missing = None
    else:
        units, params, gauss, missing = EMM.tiny_problem()
    params = dict(params, **HYPER)
    want = _want(units, params, gauss, missing)
    keep = dict(params), np.array(params["omega"])
    fit = V.refit_joint(units, params, CONFIG, max_iter=3, tol=0.0, newton_tol=1e-20, verbose=False, missing=missing,
                        hstep=True)
    assert all(params[key] is keep[0][key] for key in params) and np.array_equal(params["omega"], keep[1])
    trace = fit["config"]["runtime"]["joint"]
    assert np.array_equal(trace["omega"][0], params["omega"])
    assert np.array_equal(trace["omega"][want["kept"]], fit["params"]["omega"])
    assert not np.array_equal(fit["params"]["omega"], params["omega"])  # (the step moved the timescales)
    assert sorted(fit["params"]["cholesky"]) == sorted(want["prior"])
    _check_loop(kind, fit, units, params, gauss, missing, want)


def test_a_rejected_last_iterate_brings_the_previous_omega_and_factors_back(V, monkeypatch):
    """The evidence of iteration 2 is pushed down (the statement through its trace_hook, the device through the dict
    Engine.joint_posterior returns): the loop must return iteration 1 -- its a, b, noise, its omega and the factors built
    for that omega, which go back to the engine before the final update_w."""
    units, params, gauss = EM.tiny_problem()
    params = dict(params, **HYPER)
    want = _want(units, params, gauss, None, trace_hook=lambda k, ev: ev - 1e3 if k == 2 else ev)
    assert want["kept"] == 1 and len(want["trace"]["laplace"]) == 3
    calls, restored = [], []
    real_post, real_set = V.Engine.joint_posterior, V.Engine.set_prior

    def pushed_down(self, *a, **k):
        post = real_post(self, *a, **k)
        calls.append(k.get("window"))
        if len(calls) == 3:
            post["laplace"] = np.array([float(np.sum(post["laplace"])) - 1e3])
        return post

    def spy(self, T, G):
        if len(calls) == 3:
            restored.append((int(T), np.array(G)))
        return real_set(self, T, G)

    monkeypatch.setattr(V.Engine, "joint_posterior", pushed_down)
    monkeypatch.setattr(V.Engine, "set_prior", spy)
    fit = V.refit_joint(units, params, CONFIG, max_iter=3, tol=0.0, newton_tol=1e-20, verbose=False, hstep=True)
    trace = fit["config"]["runtime"]["joint"]
    assert calls == [CONFIG["window"]] * 3 and len(trace["laplace"]) == 3
    assert np.array_equal(fit["params"]["omega"], trace["omega"][1]) and not np.array_equal(trace["omega"][1], trace["omega"][2])
    assert sorted(T for T, _ in restored) == sorted(fit["params"]["cholesky"])
    for T, G in restored:  # what went back to the engine is what the caller gets, the factors of omega_1
        assert G.tobytes() == fit["params"]["cholesky"][T].tobytes()
    hook = lambda k, ev: ev - 1e3 if k == 2 else ev  # noqa: E731
    _check_loop("rejected", fit, units, params, gauss, None, want, trace_hook=hook)


def test_without_hstep_refit_joint_never_reaches_the_new_code(V, monkeypatch):
    """The default: no window moments, no optimiser, no rebuilt prior -- each made to fail -- and the result is that of
    joint_em_numpy's loop, held as tests/test_gpu_joint_em_masked.py holds it."""
    from vlgp_amd import _lib

    def never(*a, **k):
        raise AssertionError("refit_joint without hstep reached the hyperparameter step")

    units, params, gauss = EM.tiny_problem()
    monkeypatch.setattr(_lib.load(), "vlgp_joint_posterior_moments", never)
    monkeypatch.setattr(V.gp, "optimize_joint", never)
    monkeypatch.setattr(V.Engine, "build_prior", never)
    fit = V.refit_joint(units, params, CONFIG, max_iter=2, tol=0.0, newton_tol=1e-20, verbose=False)
    assert "omega" not in fit["config"]["runtime"]["joint"]
    assert fit["params"]["omega"] is params["omega"]
    want = EM.refit(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"], CONFIG["Mniter"], max_iter=2,
                    tol=0.0)
    errs = loop_errors(fit, want)
    print("joint_hstep refit_joint without hstep  " + "  ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < BOUND_LOOP, (k, e)
