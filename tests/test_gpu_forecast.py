"""Forward prediction on the device (vlgp_forecast, Engine.forecast, evaluation.forward_prediction, vlgp_amd.forecast)
against the NumPy restatement of its definitions (tests/forecast_numpy.py) and against the engine's own E-step and
variance kernels.

Tolerances.  STAGE = 1e-9 is the project's stage-wise tolerance, TRAJ = 1e-6 its trajectory tolerance (DESIGN.md
section 2).  Per (unit, latent) task:
- mu_ext and v_ext: largest error over the task's rows relative to the largest value (the rounding error of a
  triangular solve scales with the right-hand side, not with the entry);
- |mu|^2: plain relative error; |G beta - mu|^2 is the squared length of a difference of two vectors: its rounding error
  scales with the larger of the two squared lengths, so it is taken relative to max(|G beta - mu|^2, |mu|^2).
Every stage test asserts cond(I + H) <= 1e6 for every task on the CPU: the condition under which STAGE means anything.
The inputs are tame (a ~ 0.5 N(0, 1), b ~ -1).  The measured errors are printed by every case and recorded in
profiles/forecast/measured_errors.txt.
"""
import numpy as np
import pytest
from scipy.special import gammaln

import forecast_numpy as FN
from conftest import relerr
from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu

STAGE, TRAJ = 1e-9, 1e-6
SET = 0


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _split(full, T_in):
    return np.ascontiguousarray(full[:, :T_in]), np.ascontiguousarray(full[:, T_in:])


def _problem(held, n_ext, N, L, omega, seed, n_gauss=0, P=1, R=50, factors=None):
    """Units of the held-in lengths `held` (zero posterior), tame parameters, and per held-in length T the prior
    (L, T, R) and the extension rows (L, n_ext[T], R): the two parts of oracle.build_prior's factor of length
    T + n_ext[T] (or of factors[T], where given)."""
    rng = np.random.default_rng(seed)
    gauss = np.zeros(N, bool)
    if n_gauss:
        gauss[N - n_gauss:] = True
    a = 0.5 * rng.standard_normal((L, N))
    b = np.zeros((P, N))
    b[0] = -1.0 + 0.1 * rng.standard_normal(N)
    if P > 1:
        b[1:] = 0.2 * rng.standard_normal((P - 1, N))
    noise = np.where(gauss, rng.uniform(0.5, 2.0, N), 1.0)
    prior, ext = {}, {}
    for T in sorted(set(held)):
        full = factors[T] if factors and T in factors else \
            O.build_prior([T + n_ext[T]], np.asarray(omega, float), np.ones(L), R)[T + n_ext[T]]
        prior[T], ext[T] = _split(full, T)
    units = []
    for T in held:
        y = rng.poisson(0.6, (T, N)).astype(float)
        y[:, gauss] = rng.standard_normal((T, int(gauss.sum())))
        x = None
        if P > 1:
            x = np.ones((T, P, N))
            x[:, 1:] = 0.3 * rng.standard_normal((T, P - 1, N))
        units.append({"y": y, "x": x, "mu": np.zeros((T, L)), "v": np.zeros((T, L)), "w": np.zeros((T, L))})
    return units, (a, b, noise, gauss), prior, ext


def _engine(V, units, par, prior, P=1, R=50):
    a, b, noise, gauss = par
    eng = V.Engine(a.shape[1], a.shape[0], P, R, gauss)
    eng.set_params(a, b, noise)
    eng.upload(SET, units)
    for T, G in prior.items():
        eng.set_prior(T, G)
    return eng


def _with_state(units, state):
    off = np.concatenate([[0], np.cumsum([u["y"].shape[0] for u in units])])
    return [dict(u, **{k: state[k][off[i]:off[i + 1]].copy() for k in ("mu", "v", "w")}) for i, u in enumerate(units)]


def _swept(V, units, par, prior, vb, P=1, R=50, sweeps=3):
    """An engine after `sweeps` E-step sweeps from zero, and the units with the downloaded mu, v, w."""
    eng = _engine(V, units, par, prior, P, R)
    assert eng.estep(SET, sweeps, 5.0, vb) == 0
    return eng, _with_state(units, eng.download(SET, ("mu", "v", "w")))


def _task_errors(got, want, units, ext, vb):
    """Largest error per quantity over the (unit, latent) tasks, as the module docstring defines them."""
    mu_g, v_g, t_g = got
    mu_w, v_w, t_w = want
    assert mu_g.shape == mu_w.shape and v_g.shape == v_w.shape and t_g.shape == t_w.shape
    err = {"mu_ext": 0.0, "v_ext": 0.0, "resid": 0.0, "mu_sq": 0.0}
    at = 0
    for i, u in enumerate(units):
        n = ext[u["y"].shape[0]].shape[1]
        for l in range(mu_w.shape[1]):
            rows = slice(at, at + n)
            err["mu_ext"] = max(err["mu_ext"], relerr(mu_g[rows, l], mu_w[rows, l]))
            if vb:
                err["v_ext"] = max(err["v_ext"], relerr(v_g[rows, l], v_w[rows, l]))
            err["resid"] = max(err["resid"], abs(t_g[i, l, 0] - t_w[i, l, 0]) / max(t_w[i, l, 0], t_w[i, l, 1]))
            err["mu_sq"] = max(err["mu_sq"], abs(t_g[i, l, 1] - t_w[i, l, 1]) / t_w[i, l, 1])
        at += n
    assert at == mu_w.shape[0]
    if not vb:
        assert np.array_equal(v_g, np.zeros_like(v_g))
    return err


def _rough_and_single():
    """Shape (c): R = 64; latent 0 rough enough that its factor fills all 64 columns, latent 1 an injected one-column
    factor (r = 1)."""
    T, n = 70, 6
    full = np.zeros((2, T + n, 64))
    full[0] = O.ichol_gauss(T + n, 0.5, 64)
    full[1, :, 0] = 0.8 * np.cos(np.arange(T + n) / 25.0)
    return {T: full}


SHAPES = {
    # name: held-in lengths, n_ext, N, L, omega, n_gauss, P, R, injected factors
    "a_three_ranks": ([32, 32, 45], {32: 8, 45: 5}, 20, 3, (4e-3, 2e-2, 9e-3), 4, 1, 50, None),
    "b_tiles_and_regressors": ([90, 130], {90: 8, 130: 70}, 12, 2, (2e-3, 8e-3), 0, 2, 50, None),
    "c_rank_64_and_1": ([70, 70], {70: 6}, 10, 2, None, 0, 1, 64, _rough_and_single),
}


def _shape(name, seed=5):
    held, n_ext, N, L, omega, n_gauss, P, R, factors = SHAPES[name]
    units, par, prior, ext = _problem(held, n_ext, N, L, omega, seed, n_gauss=n_gauss, P=P, R=R,
                                      factors=factors() if factors else None)
    return units, par, prior, ext, P, R


@pytest.mark.parametrize("vb", [True, False], ids=["vb", "map"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_stage_equals_the_numpy_statement(V, name, vb):
    """Three sweeps from zero (the posterior has not converged: the w o mu term matters), then vlgp_forecast against
    the restatement fed the downloaded state."""
    units, par, prior, ext, P, R = _shape(name)
    ranks = {T: [FN.rank(G[l]) for l in range(G.shape[0])] for T, G in prior.items()}
    if name.startswith("a"):
        assert ranks[32] == [9, 16, 12], ranks
    if name.startswith("c"):
        assert ranks[70] == [64, 1], ranks
    eng, state = _swept(V, units, par, prior, vb, P, R)
    with eng:
        assert [list(r) for r in eng.unit_ranks(SET)] == [ranks[u["y"].shape[0]] for u in units]
        mu_ext, v_ext, terms, bad = eng.forecast(SET, ext, vb=vb)
    assert bad == 0
    mu_w, v_w, t_w, cond = FN.statement(state, *par, prior, ext, vb=vb)
    assert cond <= 1e6, cond
    assert np.max(t_w[:, :, 0] / t_w[:, :, 1]) > 1e-6  # (not at the fixed point: w o mu is exercised)
    err = _task_errors((mu_ext, v_ext, terms), (mu_w, v_w, t_w), state, ext, vb)
    print("forecast errors [%s, %s] ranks %s cond %.1e: %s" % (name, "vb" if vb else "map", ranks, cond,
                                                               ", ".join("%s %.2e" % kv for kv in err.items())))
    for key, val in err.items():
        assert val <= STAGE, (name, key, val)


@pytest.mark.parametrize("name", ["a_three_ranks", "b_tiles_and_regressors"])
def test_extension_onto_the_held_in_rows_is_the_engines_own_next_sweep(V, name):
    """G_ext := G.  v_ext is then the device's own v (vlgp_update_v) at STAGE, and mu_ext its own mu after one more
    sweep with dmu_bound = 1e300, at max(STAGE, 10 d): d is what the restatement and oracle.estep_unit differ by on the
    same state (the oracle's step formula cancels where the restatement's does not), computed here and held to 1e-8."""
    units, par, prior, _, P, R = _shape(name)
    a, b, noise, gauss = par
    eng, state = _swept(V, units, par, prior, True, P, R)
    with eng:
        mu_ext, v_ext, _, bad = eng.forecast(SET, prior, vb=True)
        assert bad == 0
        assert eng.update_v(SET, True) == 0
        v_dev = eng.download(SET, ("v",))["v"]
        eng.upload(SET, state)  # (the state the forecast saw, bit for bit)
        assert eng.estep(SET, 1, 1e300, True) == 0
        mu_dev = eng.download(SET, ("mu",))["mu"]
    mu_w, _, _, cond = FN.statement(state, *par, prior, prior, vb=True)
    assert cond <= 1e6, cond
    d = e_mu = e_v = 0.0
    at = 0
    for u in state:
        T = u["y"].shape[0]
        x = u["x"] if u["x"] is not None else np.ones((T, 1, len(noise)))
        nxt = O.estep_unit(u["y"], x, u["mu"], u["v"], u["w"], a, b, noise, gauss, prior[T], 1, dmu_bound=1e300)[0]
        for l in range(a.shape[0]):
            d = max(d, relerr(mu_w[at:at + T, l], nxt[:, l]))
            e_mu = max(e_mu, relerr(mu_ext[at:at + T, l], mu_dev[at:at + T, l]))
            e_v = max(e_v, relerr(v_ext[at:at + T, l], v_dev[at:at + T, l]))
        at += T
    print("forecast onto held-in rows [%s]: v %.2e, mu %.2e, d %.2e" % (name, e_v, e_mu, d))
    assert d <= 1e-8
    assert e_v <= STAGE
    assert e_mu <= max(STAGE, 10.0 * d)


def test_columns_beyond_the_held_in_rank_keep_their_prior_variance(V):
    """A factor whose last column is zero on the held-in rows and non-zero on the extension rows: v_ext contains its
    square, mu_ext is bit-equal to the run without that column."""
    units, par, prior, ext, P, R = _shape("a_three_ranks")
    extra = np.linspace(0.2, 0.6, 8)
    more = {T: G.copy() for T, G in ext.items()}
    assert FN.rank(prior[32][1]) == 16 and not more[32][1, :, 30:].any()
    more[32][1, :, 30] = extra
    eng, _ = _swept(V, units, par, prior, True, P, R)
    with eng:
        mu0, v0, t0, _ = eng.forecast(SET, ext)
        mu1, v1, t1, bad = eng.forecast(SET, more)
    assert bad == 0
    assert np.array_equal(mu0, mu1) and np.array_equal(t0, t1)
    want = v0.copy()
    for k in (0, 1):  # (the two units of length 32 come first, eight extension rows each)
        want[8 * k:8 * k + 8, 1] += extra ** 2
    assert not np.array_equal(v0, v1)
    assert np.max(np.abs(v1 - want) / want) <= 4 * np.finfo(float).eps  # (one fused multiply-add against an add)


def test_failed_task_is_nan_and_counted_the_others_stand(V):
    """An uploaded w made negative for one (unit, latent): a pivot of H is not positive.  That task's outputs are NaN and
    counted; every other task is bit-equal to the clean run."""
    units, par, prior, ext, P, R = _shape("a_three_ranks")
    eng, state = _swept(V, units, par, prior, True, P, R)
    with eng:
        clean = eng.forecast(SET, ext)
        broken = [dict(u) for u in state]
        broken[1]["w"] = state[1]["w"].copy()
        broken[1]["w"][:, 2] = -50.0
        eng.upload(SET, broken)
        mu, v, terms, bad = eng.forecast(SET, ext)
    assert clean[3] == 0 and bad == 1
    hit = np.zeros(mu.shape, bool)
    hit[8:16, 2] = True  # (unit 1: extension rows 8 ... 15)
    assert np.all(np.isnan(mu[hit])) and np.all(np.isnan(v[hit])) and np.all(np.isnan(terms[1, 2]))
    assert np.array_equal(mu[~hit], clean[0][~hit]) and np.array_equal(v[~hit], clean[1][~hit])
    keep = np.ones(terms.shape[:2], bool)
    keep[1, 2] = False
    assert np.array_equal(terms[keep], clean[2][keep])
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all() and np.isfinite(clean[2]).all()


def test_read_only_and_the_same_bits_on_every_call(V):
    units, par, prior, ext, P, R = _shape("b_tiles_and_regressors")
    eng, _ = _swept(V, units, par, prior, True, P, R)
    with eng:
        before, p_before = eng.download(SET), eng.get_params()
        one = eng.forecast(SET, ext)
        two = eng.forecast(SET, ext)
        after, p_after = eng.download(SET), eng.get_params()
    for x, y in zip(one[:3], two[:3]):
        assert np.array_equal(x, y)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    for x, y in zip(p_before, p_after):
        assert np.array_equal(x, y)


def test_refusals(V):
    units, par, prior, ext, P, R = _shape("a_three_ranks")
    eng = _engine(V, units, par, prior, P, R)
    with eng:
        def status(set_id, e):
            with pytest.raises(V.VlgpError) as info:
                eng.forecast(set_id, e)
            return info.value.status, info.value.detail

        assert status(SET, {32: ext[32]})[0] == -1                              # length 45 is not listed
        assert "45" in status(SET, {32: ext[32]})[1]
        assert status(SET, {32: ext[32], 45: np.zeros((3, 0, 50))})[0] == -1    # n_ext = 0
        eng.replicate(SET, 2, [1, 3])
        assert status(2, ext)[0] == -3                                          # a replicated set
        eng.free_units(2)
        eng.upload(1, units[:2])
        eng.set_prior(16, np.ascontiguousarray(prior[32][:, :16]))
        eng.cut(1, 3, [0, 16, 32, 48], 16)
        assert status(3, {16: np.ascontiguousarray(ext[32][:, :, :])})[0] == -3  # a cut set
        assert eng.forecast(SET, ext)[3] == 0                                   # (and the plain set still goes through)


# ---- the public path --------------------------------------------------------------------------------------------
def _public_problem(lengths, seed=7):
    """Trials whose latents are drawn from the squared-exponential kernel at omega = (2e-3, 5e-3), N = 40, L = 2; the
    true a, b are the parameters.  The draw is chosen on the CPU reference alone (oracle plus restatement, six trials of
    120 bins, sixty sweeps), by the two gates the test asserts: the reference has reached its fixed point in every trial
    (off_fixed_point <= 1e-18, a relative distance of STAGE: before that the comparison would measure how two
    sixty-sweep trajectories drift apart, not the prediction) and it predicts (fp_bps_past > 0.5).  Seeds 0 ... 7 give
    fp_bps_past 0.496, 0.63, 1.09, 1.39, 1.31, 0.39, 1.65, 0.52 and a largest off_fixed_point of 7e-23, 8e-11, 9e-07,
    1e-07, 6e-08, 2e-18, 2e-06, 8e-22: the draws that are easiest to forecast are those whose latents move far, and those
    are still 1e-3 away from their fixed point after sixty sweeps.  Seed 7 is the first that passes both."""
    N, L, omega = 40, 2, np.array([2e-3, 5e-3])
    rng = np.random.default_rng(seed)
    a = 0.8 * rng.standard_normal((L, N))
    b = np.log(0.3) + 0.3 * rng.standard_normal((1, N))
    trials = []
    for T in lengths:
        t = np.arange(T)
        lat = np.stack([np.linalg.cholesky(np.exp(-om * (t[:, None] - t[None, :]) ** 2) + 1e-8 * np.eye(T))
                        @ rng.standard_normal(T) for om in omega], axis=1)
        trials.append({"y": rng.poisson(np.exp(lat @ a + b)).astype(float)})
    params = {"ydim": N, "zdim": L, "xdim": 1, "rank": 50, "a": a, "b": b, "noise": np.ones(N), "omega": omega,
              "sigma": np.ones(L), "likelihood": np.array(["poisson"] * N)}
    return trials, params


def _public_statement(trials, params, nf, n_iter):
    """oracle.estep_unit on the held-in rows from zero, the restatement's extension, and the scores of the forward rows:
    mu_ahead, v_ahead per trial, ll per channel, fp_bps_past, and the largest off_fixed_point of the reference."""
    a, b, noise = params["a"], params["b"], params["noise"]
    N, L = a.shape[1], a.shape[0]
    gauss = np.zeros(N, bool)
    mus, vs, off = [], [], 0.0
    ll, ny, lg, past, rows_in = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N), 0
    for tr in trials:
        T = tr["y"].shape[0]
        G_in, G_ext = _split(O.build_prior([T], params["omega"], params["sigma"], 50)[T], T - nf)
        y_in, y_f = tr["y"][:T - nf], tr["y"][T - nf:]
        zero = np.zeros((T - nf, L))
        mu, v, w, _, bad = O.estep_unit(y_in, np.ones((T - nf, 1, N)), zero, zero, zero, a, b, noise, gauss, G_in, n_iter)
        assert bad == 0
        m, s, t, _, _ = FN.forecast_unit({"y": y_in, "x": None, "mu": mu, "v": v, "w": w}, a, b, noise, gauss, G_in, G_ext)
        off = max(off, float(np.max(t[:, 0] / t[:, 1])))
        mus.append(m)
        vs.append(s)
        log_rate = np.minimum(m @ a + b + 0.5 * (s @ a ** 2), 10.0)
        ll += np.sum(y_f * log_rate - np.exp(log_rate) - gammaln(y_f + 1.0), axis=0)
        ny += y_f.sum(axis=0)
        lg += gammaln(y_f + 1.0).sum(axis=0)
        past += y_in.sum(axis=0)
        rows_in += T - nf
    past /= rows_in
    use = (past > 0) & (ny > 0)
    null = ny[use] * np.log(past[use]) - nf * len(trials) * past[use] - lg[use]
    return mus, vs, ll, float((ll[use].sum() - null.sum()) / (ny[use].sum() * np.log(2.0))), off


@pytest.mark.parametrize("lengths", [[120] * 6, [120, 90]], ids=["six_trials", "ragged"])
def test_forward_prediction_equals_oracle_plus_restatement(V, lengths):
    nf, n_iter = 10, 60
    trials, params = _public_problem(lengths)
    config = V.get_config(max_iter=20)
    mus, vs, ll, fp, off = _public_statement(trials, params, nf, n_iter)
    print("forward prediction %s: CPU fp_bps_past %.4f, off_fixed_point %.1e" % (lengths, fp, off))
    assert off <= 1e-18
    if len(lengths) == 6:
        assert fp > 0.5
    else:  # (one of the two lengths comes from params["cholesky"], the other is built on the device)
        params["cholesky"] = {120: O.build_prior([120], params["omega"], params["sigma"], 50)[120]}
    keys = set(params)
    y0 = [t["y"].copy() for t in trials]
    got = V.evaluation.forward_prediction(trials, params, config, nf, n_iter=n_iter)
    assert set(params) == keys and set(params.get("cholesky", {})) <= {120}
    assert all(set(t) == {"y"} and np.array_equal(t["y"], y) for t, y in zip(trials, y0))
    assert got["n_failed"] == 0 and got["off_fixed_point"].shape == (len(trials), 2)
    e_mu = max(relerr(g, w) for g, w in zip(got["mu_ahead"], mus))
    e_v = max(relerr(g, w) for g, w in zip(got["v_ahead"], vs))
    e_ll = float(np.max(np.abs(got["ll"] - ll) / np.abs(ll)))
    print("  device fp_bps_past %.4f fp_bps %.4f; errors mu %.2e v %.2e ll %.2e; off_fixed_point max %.2e" % (
        got["fp_bps_past"], got["fp_bps"], e_mu, e_v, e_ll, got["off_fixed_point"].max()))
    assert e_mu <= TRAJ and e_v <= TRAJ and e_ll <= TRAJ
    assert abs(got["fp_bps_past"] - fp) <= TRAJ * abs(fp)
    assert all(r.shape == (nf, 40) for r in got["rate"])
    # the whole-trial forecast of the held-in parts is the same extension
    halves = [{"y": t["y"][:t["y"].shape[0] - nf].copy()} for t in trials]
    ahead = V.forecast(halves, params, config, nf, n_iter=n_iter)
    for f, m, s, h in zip(ahead, got["mu_ahead"], got["v_ahead"], halves):
        assert f["mu"].shape == f["v"].shape == f["w"].shape == (h["y"].shape[0], 2)
        assert relerr(f["mu_ahead"], m) <= TRAJ and relerr(f["v_ahead"], s) <= TRAJ
