"""The variational lower bound on the device (vlgp_elbo, vlgp_amd.evaluation.elbo, fit(track_elbo=True)) against the
NumPy statement of its definition (tests/elbo_numpy.py).

Tolerances.  STAGE = 1e-9 is the project's stage-wise tolerance, applied element by element:
- log det H, tr S and beta'beta are sums of positive terms: plain relative error;
- a row sum may cancel (a Gaussian channel's sum of eta, a log-likelihood near zero): the rounding error of a sum scales
  with the sum of the absolute values of its summands, so the error is taken relative to that;
- |mu - G beta|^2 is the squared length of a difference of two vectors of length |mu|: its rounding error scales with
  |mu|^2, not with its own value (which is 1e-30 |mu|^2 when mu lies in the range of G), so it is taken relative to
  |mu|^2.  The random-mu cases below have a residual of the order of |mu|^2, where this IS the plain relative error;
- the total is a difference of the two parts: relative to sum |ell| + sum |KL|.
The measured errors are printed by every case and recorded in DESIGN.md section 4.7.
"""
import math
import os
import sys
import tempfile

import numpy as np
import pytest

import elbo_numpy as EN
from conftest import GOLDEN, ROOT
from heldout_numpy import lagged

pytestmark = pytest.mark.gpu

STAGE = 1e-9
SET = 0


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def _problem(lengths, N, L, omega, seed, n_gauss=0, history=0, vb=True, in_range=False, rank=50):
    """Units with a given posterior (mu, v, w random and positive where they must be), parameters and the device-built
    prior factors of `omega` with `rank` columns.  in_range: mu = G c, as an E-step leaves it."""
    import vlgp_amd as V
    from vlgp_amd import synth

    rng = np.random.default_rng(seed)
    trials = synth.make_trials(len(lengths), max(lengths), N, min(L, 3), seed=seed, n_gauss=n_gauss, lengths=lengths)
    P = 1 + history
    gauss = np.zeros(N, bool)
    if n_gauss:
        gauss[N - n_gauss:] = True
    a = 0.3 * rng.standard_normal((L, N)) * (5.0 / L if L > 10 else 1.0)
    y = np.concatenate([t["y"] for t in trials])
    b = np.zeros((P, N))
    b[0] = np.where(gauss, y.mean(0), np.log(np.maximum(y.mean(0), 1e-3)))
    if history:
        b[1:] = -0.05 * rng.random((history, N))
    noise = np.where(gauss, 0.5 + rng.random(N), 1.0)
    omega = np.asarray(omega, dtype=float)
    sigma = np.ones(L)
    with V.Engine(N, L, P, rank, gauss) as eng:
        eng.build_prior(sorted(set(lengths)), omega, sigma)
        chol = {T: eng.get_prior(T) for T in sorted(set(lengths))}
    units = []
    for t in trials:
        T = t["y"].shape[0]
        mu = 0.3 * rng.standard_normal((T, L))
        if in_range:
            mu = np.stack([EN.compact(chol[T][l]) @ (0.5 * rng.standard_normal(EN.compact(chol[T][l]).shape[1]))
                           for l in range(L)], axis=1)
        units.append({"y": t["y"], "x": lagged(t["y"], history) if history else None, "mu": mu,
                      "v": 0.05 * rng.random((T, L)) if vb else np.zeros((T, L)), "w": rng.uniform(0.05, 2.0, (T, L))})
    params = {"ydim": N, "zdim": L, "xdim": P, "a": a, "b": b, "noise": noise, "omega": omega, "sigma": sigma,
              "rank": rank, "likelihood": np.where(gauss, "gaussian", "poisson"), "cholesky": chol}
    return units, params, gauss


def _device(V, units, params, gauss, vb, want_rows=True, rank=None):
    """vlgp_elbo on an engine of `rank` columns (default: the problem's own, params["rank"])."""
    with V.Engine(params["ydim"], params["zdim"], params["xdim"], params["rank"] if rank is None else rank, gauss) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(SET, units)
        for T, G in params["cholesky"].items():
            eng.set_prior(T, G)
        sums, terms, bad, row_ell = eng.elbo(SET, vb=vb, want_rows=want_rows)
        ranks = eng.unit_ranks(SET)
    return sums, terms, bad, row_ell, ranks


def _compare(name, dev, st, vb=True):
    """Element-wise errors of the device arrays against the statement, printed, then asserted at STAGE."""
    from vlgp_amd.evaluation import elbo_from_terms

    sums, terms, bad, row_ell, ranks = dev
    assert bad == 0
    assert np.array_equal(ranks, st["ranks"])
    err = {"row_sums": float(np.max(np.abs(sums - st["row_sums"]) / np.maximum(st["row_abs"], 1e-300)))}
    for k, key in enumerate(("logdet", "tr_s", "beta2")):
        err[key] = float(np.max(np.abs(terms[:, :, k] - st["terms"][:, :, k]) / np.abs(st["terms"][:, :, k])))
    err["resid"] = float(np.max(np.abs(terms[:, :, 3] - st["terms"][:, :, 3]) / st["mu_sq"]))
    if row_ell is not None:
        err["row_ell"] = float(np.max(np.abs(row_ell - st["row_ell"])) / np.max(np.abs(st["row_ell"])))
    out = elbo_from_terms(sums, terms, ranks, vb=vb, n_failed=bad, mu_sq=st["mu_sq"])
    abs_ell = float(st["row_abs"][:, 0].sum())
    if vb:
        want = st["row_sums"][:, 0].sum() - st["kl"].sum()
        err["total"] = abs(out["elbo"] - want) / (abs_ell + float(np.abs(st["kl"]).sum()))
        err["kl"] = float(np.max(np.abs(out["kl"] - st["kl"]) / (0.5 * np.abs(st["terms"][:, :, :3]).sum(axis=2)
                                                                  + 0.5 * st["ranks"])))
    else:
        want = st["row_sums"][:, 0].sum() - 0.5 * st["terms"][:, :, 2].sum()
        err["total"] = abs(out["log_joint"] - want) / (abs_ell + 0.5 * float(st["terms"][:, :, 2].sum()))
        assert math.isnan(out["elbo"]) and np.all(np.isnan(out["kl"]))
    print("elbo errors [%s] ranks %d..%d: %s" % (name, st["ranks"].min(), st["ranks"].max(),
                                                 ", ".join("%s %.2e" % kv for kv in err.items())))
    for key, val in err.items():
        assert val <= STAGE, (name, key, val)
    return out


CASES = {
    # name: lengths, N, L, omega, n_gauss, history, vb, in_range
    "ranks_around_14_and_32": ([64] * 7, 12, 6, [1e-4, 1e-3, 5e-3, 2e-2, 1e-1, 5e-1], 0, 0, True, False),
    "ranks_in_range": ([64] * 5, 12, 6, [1e-4, 1e-3, 5e-3, 2e-2, 1e-1, 5e-1], 0, 0, True, True),
    "long_rank50": ([1000, 1000, 1000], 10, 2, [1e-3, 2e-3], 0, 0, True, False),
    "long_rank50_in_range": ([1000, 1000], 10, 2, [1e-3, 1e-4], 0, 0, True, True),
    "c5_shape": ([100, 150, 200, 250, 100, 150, 200, 250], 40, 10, np.linspace(2e-2, 1e-3, 10), 10, 2, True, False),
    "twelve_latents": ([50] * 6, 14, 12, np.linspace(2e-2, 1e-3, 12), 0, 0, True, False),
    "map": ([50, 80, 50], 14, 3, [2e-2, 5e-3, 1e-3], 3, 0, False, True),
    "rank_64_61_and_1": ([70, 130], 12, 3, [0.5, 1.5, 3.0], 2, 0, True, False),
}
# Engines of 64 columns: the rough omega of the case fills all 64, and every column from the listed rank on is zeroed (as
# tests/joint_shapes.py cuts its factors): elbo_kl's two r x r matrices with every lane live, a rank that is no multiple
# of 8, and rank 1; mu off the range of G and vb = True, so that all four terms are at work.
CUT_RANKS = {"rank_64_61_and_1": [64, 61, 1]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_terms_equal_the_numpy_statement(V, name):
    lengths, N, L, omega, n_gauss, history, vb, in_range = CASES[name]
    units, params, gauss = _problem(lengths, N, L, omega, seed=11, n_gauss=n_gauss, history=history, vb=vb,
                                    in_range=in_range, rank=64 if name in CUT_RANKS else 50)
    for l, r in enumerate(CUT_RANKS.get(name, ())):
        assert not in_range and vb
        for G in params["cholesky"].values():
            assert np.all(np.any(G[l] != 0.0, axis=0))  # (all 64 columns filled before the cut)
            G[l][:, r:] = 0.0
    st = EN.statement(units, params["a"], params["b"], params["noise"], gauss, params["cholesky"], vb=vb)
    if name.startswith("ranks"):
        r = st["ranks"][0]
        assert r.min() < 14 and np.any((r > 14) & (r < 32)) and r.max() > 32, r
    if name.startswith("long"):
        assert st["ranks"].max() == 50
    if in_range:
        assert np.max(st["terms"][:, :, 3] / st["mu_sq"]) < 1e-20
    dev = _device(V, units, params, gauss, vb)
    if name in CUT_RANKS:
        assert np.array_equal(dev[4], [CUT_RANKS[name]] * len(units)) and np.all(st["terms"][:, :, 3] > 1e-3 * st["mu_sq"])
    _compare(name, dev, st, vb=vb)


def _c1_session(V, track=False, iters=2, **kw):
    from vlgp_amd import synth
    from vlgp_amd.api import FitSession

    trials = synth.make_trials(10, 200, 20, 3, seed=0)
    rng = np.random.default_rng(7)
    a0 = 0.3 * rng.standard_normal((3, 20))
    np.random.seed(5)
    return FitSession(trials, 3, verbose=False, max_iter=iters, min_iter=iters, a=a0, track_elbo=track, **kw)


def test_segment_set_of_vem_equals_the_numpy_statement(V):
    """C1-size windows (10 trials x 200 bins -> 40 segments of 50) after two EM iterations, through the segment set.
    (Taken after the iteration's H-step: the prior is the rebuilt one, which the posterior means have not seen yet, so
    off_prior is small here but not rounding noise.)"""
    from vlgp_amd.api import SET_SEGMENTS

    sess = _c1_session(V)
    try:
        sess.em_iteration()
        sess.em_iteration()
        eng, p = sess.eng, sess.params
        a, b, noise, _, _ = eng.get_params()
        state = eng.download(SET_SEGMENTS, ("mu", "v", "w"))
        dev = eng.elbo(SET_SEGMENTS, vb=True, want_rows=True) + (eng.unit_ranks(SET_SEGMENTS),)
        chol = {50: eng.get_prior(50)}
        assert sess.segs.unit_of is None and len(sess.segs) == 40
        units = [{"y": sg["y"], "x": None, **{k: state[k][50 * i:50 * (i + 1)] for k in ("mu", "v", "w")}}
                 for i, sg in enumerate(sess.segs)]
    finally:
        sess.close()
    gauss = np.zeros(20, bool)
    st = EN.statement(units, a, b, noise, gauss, chol, vb=True)
    out = _compare("c1_segments", dev, st)
    assert np.max(out["off_prior"]) < 1e-6 and np.all(out["kl"] > 0.0)


def _ref_fit(V):
    res = V.load(os.path.join(GOLDEN, "ref_result.npy"))
    return {"trials": [dict(t) for t in res["trials"]], "params": dict(res["params"]), "config": dict(res["config"])}


def test_evaluation_elbo_on_the_reference_fit(V):
    """evaluation.elbo of the real reference's stored fit equals the statement; two runs give the same bits; permuting
    the trials permutes kl, off_prior and elbo_per_trial."""
    fit = _ref_fit(V)
    p = fit["params"]
    gauss = np.asarray(p["likelihood"]) == "gaussian"
    units = [{"y": t["y"], "x": t.get("x"), "mu": t["mu"], "v": t["v"], "w": t["w"]} for t in fit["trials"]]
    st = EN.statement(units, p["a"], p["b"], p["noise"], gauss, p["cholesky"], vb=True)
    one = V.evaluation.elbo(fit, per_trial=True)
    two = V.evaluation.elbo(fit, per_trial=True)
    for key in ("elbo", "ell", "kl", "ell_per_channel", "off_prior", "elbo_per_trial"):
        assert np.array_equal(one[key], two[key]), key
    assert one["n_failed"] == 0 and "log_joint" not in one
    scale = float(st["row_abs"][:, 0].sum() + np.abs(st["kl"]).sum())
    want = st["row_sums"][:, 0].sum() - st["kl"].sum()
    print("ref fit: elbo %.6f ell %.6f kl %.6f, err %.2e; kl per pair %.2f..%.2f; off_prior max %.2e" % (
        one["elbo"], one["ell"], one["kl"].sum(), abs(one["elbo"] - want) / scale, one["kl"].min(), one["kl"].max(),
        one["off_prior"].max()))
    assert abs(one["elbo"] - want) <= STAGE * scale
    assert np.max(np.abs(one["kl"] - st["kl"]) / np.abs(st["kl"])) <= STAGE
    off = np.concatenate([[0], np.cumsum([u["y"].shape[0] for u in units])])
    per = np.array([st["row_ell"][off[i]:off[i + 1]].sum() - st["kl"][i].sum() for i in range(len(units))])
    assert np.max(np.abs(one["elbo_per_trial"] - per)) <= STAGE * scale
    assert one["off_prior"].max() <= 1e-24
    assert "elbo_per_trial" not in V.evaluation.elbo(fit)
    perm = [2, 0, 3, 1]
    shuffled = dict(fit, trials=[fit["trials"][i] for i in perm])
    got = V.evaluation.elbo(shuffled, per_trial=True)
    for key in ("kl", "off_prior", "elbo_per_trial"):  # (a unit's terms depend on that unit alone: the same bits)
        assert np.array_equal(got[key], one[key][perm]), key
    assert abs(got["elbo"] - one["elbo"]) <= 1e-12 * scale


def _same(x, y):
    if isinstance(x, dict):
        return set(x) == set(y) and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(_same(p, q) for p, q in zip(x, y))
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
        return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=np.asarray(x).dtype.kind == "f")
    return x == y or (x is y) or callable(x)


TIMERS = ("e_elapsed", "m_elapsed", "h_elapsed", "em_elapsed")


def test_fit_with_trace_computes_what_fit_without_computes(V):
    """track_elbo changes no number of the fit: trials' mu, v, w, every array of params and every shared config key
    are equal; one trace entry per EM iteration; elbo_final is evaluation.elbo of the returned fit."""
    from vlgp_amd import synth

    results = []
    for track in (False, True):
        trials = synth.make_trials(6, 230, 16, 3, seed=2)  # (230 = 4 x 50 + 30: overlapping segments)
        rng = np.random.default_rng(3)
        np.random.seed(9)
        results.append(V.fit(trials, 3, verbose=False, max_iter=4, min_iter=4, a=0.3 * rng.standard_normal((3, 16)),
                             track_elbo=track))
    off, on = results
    for t0, t1 in zip(off["trials"], on["trials"]):
        for key in ("mu", "v", "w"):
            assert np.array_equal(t0[key], t1[key]), key
    for key, val in off["params"].items():
        if isinstance(val, (np.ndarray, dict)) and key != "initial":
            assert _same(val, on["params"][key]), key
    for key, val in off["config"].items():
        if key != "runtime":
            assert _same(val, on["config"][key]), key
    r0, r1 = off["config"]["runtime"], on["config"]["runtime"]
    assert r0["it"] == r1["it"] == 4
    assert set(r1) - set(r0) == {"elbo", "elbo_ell", "elbo_kl", "elbo_final"}
    assert not [k for k in r0 if k.startswith("elbo")]
    for key in ("elbo", "elbo_ell", "elbo_kl"):
        assert len(r1[key]) == r1["it"] and np.all(np.isfinite(r1[key]))
    assert np.allclose(np.array(r1["elbo"]), np.array(r1["elbo_ell"]) - np.array(r1["elbo_kl"]), rtol=1e-12)
    again = V.evaluation.elbo(on)
    print("trace %s final %.6f evaluation.elbo %.6f" % (r1["elbo"], r1["elbo_final"], again["elbo"]))
    assert abs(r1["elbo_final"] - again["elbo"]) <= 1e-12 * abs(again["elbo"])


def test_elbo_call_in_the_middle_of_an_iteration_changes_nothing(V):
    """vlgp_elbo with the M-step in flight and the H-step prepared: the iteration gives the bits of one without."""
    from vlgp_amd.api import SET_SEGMENTS

    outs = []
    for poke in (False, True):
        sess = _c1_session(V, iters=3)
        try:
            eng = sess.eng
            calls = []
            if poke:
                inner = eng.hstep_prepare

                def prepare_then_elbo(sid, window):
                    inner(sid, window)  # (the M-step lane was started before the E-step's end: it is in flight here)
                    calls.append(eng.elbo(sid, vb=True)[0][:, 0].sum())

                eng.hstep_prepare = prepare_then_elbo
            for _ in range(3):
                sess.em_iteration()
            assert len(calls) == (3 if poke else 0)
            state = eng.download(SET_SEGMENTS)
            outs.append((state, eng.get_params(), np.array(sess.params["omega"]), np.array(sess.params["sigma"])))
        finally:
            sess.close()
    (s0, p0, om0, sg0), (s1, p1, om1, sg1) = outs
    for key in s0:
        assert np.array_equal(s0[key], s1[key]), key
    for x, y in zip(p0, p1):
        assert np.array_equal(x, y)
    assert np.array_equal(om0, om1) and np.array_equal(sg0, sg1)


def test_replicated_set_is_refused(V):
    units, params, gauss = _problem([50, 50], 8, 2, [1e-2, 1e-3], seed=4)
    with V.Engine(8, 2, 1, 50, gauss) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, units)
        eng.set_prior(50, params["cholesky"][50])
        eng.replicate(0, 2, [1, 3])
        with pytest.raises(V.engine.VlgpError, match="status -3"):
            eng.elbo(2)
        assert eng.elbo(0)[2] == 0


def test_singular_pair_is_counted_and_nan_not_a_fault(V):
    """A negative w makes I + G'WG indefinite for one (unit, latent): its terms are NaN and counted, the rest stand."""
    units, params, gauss = _problem([50, 50, 50], 8, 2, [1e-2, 1e-3], seed=6)
    units[1]["w"] = units[1]["w"].copy()
    units[1]["w"][:, 1] = -50.0
    sums, terms, bad, _, _ = _device(V, units, params, gauss, True)
    assert bad == 1
    assert np.all(np.isnan(terms[1, 1])) and np.isnan(terms).sum() == 4
    assert np.all(np.isfinite(sums))


def test_map_sums_of_y_and_rate_are_the_bits_of_vlgp_loglik(V):
    """vlgp_loglik and vlgp_elbo share the row model and the four-sum reduction (csrc/eval_wave.h).  With vb = False
    both form eta by the same chain, the bound adds a variance term of 0.0 to it, and both reduce in the same order:
    sum y and sum rate (Poisson) / sum eta (Gaussian) per channel are the same bits from either call."""
    units, params, gauss = _problem([50, 80, 50], 14, 3, [2e-2, 5e-3, 1e-3], seed=11, n_gauss=3, vb=False)
    with V.Engine(params["ydim"], params["zdim"], params["xdim"], params["rank"], gauss) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(SET, units)
        for T, G in params["cholesky"].items():
            eng.set_prior(T, G)
        ll = eng.loglik(SET, vb=False)[0]
        el = eng.elbo(SET, vb=False)[0]
    assert gauss.sum() == 3 and np.all(np.isfinite(ll)) and np.all(np.isfinite(el))
    for col in (1, 2):
        assert ll[:, col].tobytes() == el[:, col].tobytes(), (col, ll[:, col] - el[:, col])


def _rank_worker(rank, world, tmp, q):
    os.environ.update({"VLGP_COMM_TRANSPORT": "shm", "RANK": str(rank), "WORLD_SIZE": str(world),
                       "LOCAL_RANK": "0", "MASTER_PORT": "29998", "VLGP_RENDEZVOUS_DIR": tmp})
    sys.path.insert(0, ROOT)
    import vlgp_amd as V
    from vlgp_amd import engine as E
    from vlgp_amd.dist import Comm

    units, params, gauss = _problem([50] * 9, 10, 3, [2e-2, 5e-3, 1e-3], seed=8, in_range=True)
    comm = Comm.from_env() if world > 1 else None
    mine = comm.shard(units) if comm else units
    with V.Engine(10, 3, 1, 50, gauss) as eng:
        if comm:
            comm.attach(eng)
            assert eng.transport == "shm" and eng.world == world
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(SET, mine)
        eng.set_prior(50, params["cholesky"][50])
        tot = E._elbo_totals(eng, SET, True)
        local = tot.copy()
        if world > 1:
            eng.allreduce_host(tot)
    q.put((rank, len(mine), local, tot))


def test_two_ranks_sum_to_the_single_process_values():
    """The exchange, not a fit: each rank holds its shard of the SAME units with the same parameters, prior and
    posterior; the totals added over the ranks (allreduce_host, as fit(track_elbo=True) adds them) equal the single
    process's at 1e-12 -- only the order of the last additions differs."""
    import multiprocessing as mp

    from test_gpu_multirank import _collect

    ctx = mp.get_context("spawn")
    out = {}
    for world in (1, 2):
        q = ctx.Queue()
        with tempfile.TemporaryDirectory() as tmp:
            procs = [ctx.Process(target=_rank_worker, args=(r, world, tmp, q)) for r in range(world)]
            for p in procs:
                p.start()
            out[world] = sorted(_collect(q, procs, limit=300.0), key=lambda r: r[0])
            for p in procs:
                p.join(timeout=120)
                assert p.exitcode == 0
    single = out[1][0][3]
    assert sum(r[1] for r in out[2]) == out[1][0][1] == 9
    for r in out[2]:
        assert np.array_equal(r[3], out[2][0][3])          # every rank reports the same sum ...
        assert not np.array_equal(r[2], r[3])              # ... which is not its own shard's number
        assert np.all(np.abs(r[3] - single) <= 1e-12 * np.abs(single)), (r[3], single)
    assert np.all(np.abs(out[2][0][2] + out[2][1][2] - single) <= 1e-12 * np.abs(single))


def test_trace_rises_over_a_fit(V):
    """Sanity, not parity: the last entry of a 20-iteration trace exceeds the first (no monotonicity is asserted: the
    E-step's clipped Newton updates and the windowed H-step do not guarantee it).  The fit is the project's pinned C1
    workload (bench.build_inputs: synth.make_trials data with the injected a, b every parity test starts from) -- a
    fit that is known to behave, so that the assertion is about the trace and not about the fit."""
    sys.path.insert(0, ROOT)
    import bench

    trials, a0, b0, dims = bench.build_inputs("C1")
    res = V.fit(trials, dims[3], verbose=False, max_iter=20, min_iter=20, a=a0.copy(), b=b0.copy(), track_elbo=True)
    tr = res["config"]["runtime"]["elbo"]
    print("trace over 20 iterations: %s" % np.array2string(np.array(tr), precision=2))
    assert len(tr) == 20 and np.all(np.isfinite(tr))
    assert tr[-1] > tr[0]
