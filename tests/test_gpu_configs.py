"""BASELINE.json's configurations at FULL size through the C ABI (the stage-wise parity tests run at fixture
size): C2 against the real reference's golden trajectory, C3 (the headline, 4000 segments) M-step and H-step
objective against the oracle on every segment, C5 at its full channel / latent count on ragged mixed trials.
C4 (C3 over 2/4/8 GPUs) needs the multi-GPU node: tests/test_gpu_multirank.py runs its protocol on one GPU."""
import numpy as np
import pytest

from conftest import relerr_elem, relerr
from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu

STAGE = 1e-9
TRAJ = 1e-6


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


# ------------------------------------------------------------------ C2: 50 x 500 x 50, L = 3
def test_c2_full_size_vem_against_reference_golden(V, golden):
    """Three EM iterations with every default (H-step on) on all 500 segments against what the real reference
    produced (tests/golden/gen_golden.py: gen_vem_c2): per-iteration norms and omega, final a, b, noise and
    every 20th segment's posterior, 1e-6."""
    from vlgp_amd import synth
    from vlgp_amd.api import FitSession

    g = golden("vem_c2")
    n_trials, n_bins, N, L = synth.CONFIGS["C2"]
    trials = synth.make_trials(n_trials, n_bins, N, L, seed=0)
    assert float(np.concatenate([t["y"] for t in trials]).sum()) == float(g["y_checksum"][0])  # same inputs
    rng = np.random.default_rng(21)
    a0 = 0.3 * rng.standard_normal((L, N))
    b0 = np.log(np.maximum(np.mean(np.concatenate([t["y"] for t in trials]), axis=0, keepdims=True), 1e-8))
    for t in trials:
        t["mu"] = 0.2 * rng.standard_normal((n_bins, L))
    traj = []

    def spy(tr_, p_, c_):
        traj.append((np.linalg.norm(np.concatenate([s["mu"] for s in tr_])), np.linalg.norm(p_["a"]),
                     np.linalg.norm(p_["b"]), np.array(p_["omega"])))

    sess = FitSession(trials, L, verbose=False, a=a0.copy(), b=b0.copy(), max_iter=3, min_iter=3, callbacks=[spy])
    try:
        sess.run()
        sess.segs.pull(("mu", "v", "w"))
        segs = list(sess.segs)
        p = sess.params
        assert sess.runtime["it"] == int(g["it"])
        assert relerr([t[0] for t in traj], g["norm_mu"]) < TRAJ
        assert relerr([t[1] for t in traj], g["norm_a"]) < TRAJ
        assert relerr([t[2] for t in traj], g["norm_b"]) < TRAJ
        assert relerr(np.array([t[3] for t in traj]), g["omega"]) < TRAJ
        for k in ("a", "b", "noise"):
            assert relerr(p[k], g[k]) < TRAJ, k
        for k in ("mu", "v", "w"):
            assert relerr(np.stack([segs[i][k] for i in g["pick"]]), g["seg_" + k]) < TRAJ, k
    finally:
        sess.close()


# ------------------------------------------------------------------ the C5 combination against the REAL reference
def test_c5_small_vem_against_reference_golden(V, golden):
    """BASELINE.json configs[4]'s combination, small enough for the real reference (gen_golden.py c5_small; VERDICT round
    5, item 7 i): 24 trials of four distinct lengths x 40 channels (30 Poisson + 10 Gaussian), ten latents; two EM
    iterations with every default -- the H-step on the 50-bin segments of all lengths, a prior factor per distinct length
    (vlgp/gp.py:150-162), mixed likelihood in E- and M-step (vlgp/core.py:36-37,82-83,222-235).  1e-6."""
    import golden_cases
    from vlgp_amd.api import FitSession

    g = golden("c5_small")
    trials0, a0, b0, mu0, lik = golden_cases.c5_small_inputs()
    assert float(np.concatenate([t["y"] for t in trials0]).sum()) == float(g["y_checksum"][0])  # same inputs
    L = a0.shape[0]
    trials = [{"ID": t["ID"], "y": t["y"], "mu": m.copy()} for t, m in zip(trials0, mu0)]
    traj = []

    def spy(tr_, p_, c_):
        traj.append((np.linalg.norm(np.concatenate([s["mu"] for s in tr_])), np.linalg.norm(p_["a"]),
                     np.linalg.norm(p_["b"]), np.array(p_["omega"]), np.array(p_["noise"])))

    sess = FitSession(trials, L, verbose=False, a=a0.copy(), b=b0.copy(), lik=lik, max_iter=2, min_iter=2, callbacks=[spy])
    try:
        assert sorted(int(T) for T in sess.params["cholesky"].keys()) == [50]  # (the segments' factor; the trials' four on finish)
        sess.run()
        sess.segs.pull(("mu", "v", "w"))
        segs = list(sess.segs)
        p = sess.params
        assert sess.runtime["it"] == int(g["it"]) == 2
        assert relerr([t[0] for t in traj], g["norm_mu"]) < TRAJ
        assert relerr([t[1] for t in traj], g["norm_a"]) < TRAJ
        assert relerr([t[2] for t in traj], g["norm_b"]) < TRAJ
        assert relerr(np.array([t[3] for t in traj]), g["omega"]) < TRAJ
        assert relerr(np.array([t[4] for t in traj]), g["noise_traj"]) < TRAJ
        for k in ("a", "b", "noise"):
            assert relerr(p[k], g[k]) < TRAJ, k
        for k in ("mu", "v", "w"):
            assert relerr(np.stack([segs[i][k] for i in g["pick"]]), g["seg_" + k]) < TRAJ, k
        res = sess.finish()
        sess = None
        assert sorted(int(T) for T in res["params"]["cholesky"].keys()) == [100, 150, 200, 250]
        assert all(np.all(np.isfinite(t["mu"])) and t["mu"].shape == (t["y"].shape[0], L) for t in res["trials"])
    finally:
        if sess is not None:
            sess.close()


# ------------------------------------------------------------------ C3 (headline) against the REAL reference
def test_c3_full_size_vem_against_reference_golden(V, golden):
    """BASELINE.json configs[2], the headline: 200 trials x 1000 bins x 100 channels, 5 latents -> 4000 segments.
    Two EM iterations with every default (H-step on) against what the real reference produced from the same
    injected a, b, mu (tests/golden/gen_golden.py: gen_vem_c3, ~15 minutes of the reference): per-iteration norms
    and omega, final a, b, noise, every 20th segment's mu, v, w (every 80th after the first iteration), 1e-6.
    The E-steps run on the split E-step by size (ranks ~29 in the first iteration -> class 32, lower afterwards)."""
    from vlgp_amd import synth
    from vlgp_amd.api import FitSession

    g = golden("vem_c3")
    n_trials, n_bins, N, L = synth.CONFIGS["C3"]
    trials = synth.make_trials(n_trials, n_bins, N, L, seed=0)
    assert float(np.concatenate([t["y"] for t in trials]).sum()) == float(g["y_checksum"][0])  # same inputs
    rng = np.random.default_rng(31)
    a0 = 0.3 * rng.standard_normal((L, N))
    b0 = np.log(np.maximum(np.mean(np.concatenate([t["y"] for t in trials]), axis=0, keepdims=True), 1e-8))
    for t in trials:
        t["mu"] = 0.2 * rng.standard_normal((n_bins, L))
    pick = g["pick"]
    traj, paths = [], []

    def spy(tr_, p_, c_):
        traj.append((np.linalg.norm(np.concatenate([s["mu"] for s in tr_])), np.linalg.norm(p_["a"]),
                     np.linalg.norm(p_["b"]), np.array(p_["omega"]), np.stack([tr_[i]["mu"] for i in pick[::4]])))
        paths.append(tr_.engine.last_estep_path)

    sess = FitSession(trials, L, verbose=False, a=a0.copy(), b=b0.copy(), max_iter=2, min_iter=2, callbacks=[spy])
    try:
        sess.run()
        sess.segs.pull(("mu", "v", "w"))
        segs = list(sess.segs)
        p = sess.params
        assert all(p in ("split", "split_mixed") for p in paths) and len(paths) == 2
        assert sess.runtime["it"] == int(g["it"]) == 2
        assert relerr([t[0] for t in traj], g["norm_mu"]) < TRAJ
        assert relerr([t[1] for t in traj], g["norm_a"]) < TRAJ
        assert relerr([t[2] for t in traj], g["norm_b"]) < TRAJ
        assert relerr(np.array([t[3] for t in traj]), g["omega"]) < TRAJ
        assert relerr(traj[0][4], g["seg_mu_it1"]) < TRAJ
        for k in ("a", "b", "noise"):
            assert relerr(p[k], g[k]) < TRAJ, k
        for k in ("mu", "v", "w"):
            assert relerr(np.stack([segs[i][k] for i in pick]), g["seg_" + k]) < TRAJ, k
        # element by element as well (parity item 3): every entry of the picked segments' mu, v to
        # 1e-6 of its OWN size (floor: a tenth of the array's r.m.s.), not only of the largest entry
        for k in ("mu", "v"):
            assert relerr_elem(np.stack([segs[i][k] for i in pick]), g["seg_" + k]) < TRAJ, k
        assert relerr_elem(traj[0][4], g["seg_mu_it1"]) < TRAJ
    finally:
        sess.close()


# ------------------------------------------------------------------ C3: 200 x 1000 x 100, L = 5 -> 4000 segments
@pytest.fixture(scope="module")
def c3_state(V):
    """The headline workload after two EM iterations (so that mu, v, w are a real posterior), resident."""
    import bench
    from vlgp_amd.api import FitSession

    trials, a0, b0, dims = bench.build_inputs("C3")
    sess = FitSession(trials, dims[3], verbose=False, a=a0.copy(), b=b0.copy(), max_iter=2, min_iter=2)
    sess.run()
    sess.segs.pull(("mu", "v", "w"))
    yield sess
    sess.close()


def test_c3_mstep_one_newton_iteration_all_segments_vs_oracle(V, c3_state):
    """core.mstep with Mniter = 1 over the concatenation of all 4000 segments (200 000 rows x 100 channels)."""
    sess = c3_state
    p = sess.params
    a0, b0 = np.array(p["a"]), np.array(p["b"])
    segs = list(sess.segs)
    cat = lambda k: np.concatenate([s[k] for s in segs], axis=0)
    x = np.ones((cat("mu").shape[0], 1, a0.shape[1]))
    want = O.mstep_arrays(cat("y"), x, cat("mu"), cat("v"), a0.copy(), b0.copy(), np.zeros(a0.shape[1], bool), 1)
    eng = sess.eng
    eng.set_params(a0, b0, np.array(p["noise"]))
    eng.mstep(sess.segs.set_id, 1)
    a, b, noise, da, db = eng.get_params()
    eng.set_params(a0, b0, np.array(p["noise"]))  # leave the state as it was for the other tests
    assert relerr(a, want[0]) < STAGE and relerr(b, want[1]) < STAGE
    assert relerr(da, want[2]) < 1e-7 and relerr(db, want[3]) < 1e-7   # increments: differences of the above
    assert relerr(noise, want[4]) < STAGE


def test_c3_hstep_objective_all_segments_vs_oracle_and_additivity(V, c3_state):
    """gp.elbo summed over all 4000 segments, one point per latent, against the oracle on every segment; and
    the objective of the whole set equals the sum over a partition of it (the property a sharded run relies on)."""
    sess = c3_state
    p = sess.params
    L, T = p["zdim"], 50
    segs = list(sess.segs)
    lat = np.arange(L, dtype=np.int32)
    logp = np.log(np.array([[p["sigma"][l] ** 2, p["omega"][l] * (0.8 + 0.1 * l), p["gp_noise"]] for l in range(L)]))
    eng = sess.eng
    ll, dll = eng.hstep_objective(sess.segs.set_id, T, 1.0, lat, logp)
    t = np.arange(T) * 1.0
    mu = np.stack([s["mu"] for s in segs])  # (M, T, L)
    w = np.stack([s["w"] for s in segs])
    for l in range(L):
        want_ll, want_dll = O.gp_objective(logp[l], t, mu[:, :, l].T, w[:, :, l].T)
        assert abs(ll[l] - want_ll) <= STAGE * abs(want_ll), l
        assert abs(dll[l, 1] - want_dll[1]) <= STAGE * max(abs(want_dll[1]), 1e-3 * abs(want_ll)), l
    # additivity over a ragged three-way partition of the segments (second engine: the sets are independent)
    parts = (slice(0, 1203), slice(1203, 2900), slice(2900, 4000))
    tot_ll, tot_dll = np.zeros(L), np.zeros(L)
    with V.Engine(p["ydim"], L, 1, 50) as e2:
        for sl in parts:
            units = [{"y": s["y"], "mu": s["mu"], "w": s["w"], "v": s["v"]} for s in segs[sl]]
            e2.upload(0, units)
            l2, d2 = e2.hstep_objective(0, T, 1.0, lat, logp)
            tot_ll += l2
            tot_dll += d2[:, 1]
    assert relerr(tot_ll, ll) < 1e-10 and np.abs(tot_dll - dll[:, 1]).max() <= 1e-9 * np.abs(ll).max()


# ------------------------------------------------------------------ C5: ragged, 200 mixed channels, 10 latents
@pytest.mark.parametrize("split", [False, True])
def test_c5_full_channel_count_ragged_trials_vs_oracle(V, split, monkeypatch):
    """BASELINE.json configs[4] at its full channel / latent count (150 Poisson + 50 Gaussian channels, ten
    latents) on 20 ragged trials of 500 ... 2000 bins (the 500-trial job is the 8-GPU configuration; one EM
    iteration of the oracle on 20 trials already takes a minute): two EM iterations against the oracle through
    the parameters, the final stage of every trial under the returned parameters (see
    test_c5_like_ragged_mixed_ten_latents for why), the factors bit for bit."""
    from vlgp_amd import synth
    from vlgp_amd.api import SET_SEGMENTS, FitSession

    if split:  # 20 trials = ~500 segments sit below the size threshold: force the kernels the 500-trial job runs
        monkeypatch.setenv("VLGP_ESTEP_SPLIT", "1")
    rng = np.random.default_rng(12)
    lengths = [int(50 * k) for k in rng.integers(10, 41, 20)]
    L, N, n_gauss = 10, 200, 50
    trials = synth.make_trials(len(lengths), max(lengths), N, L, seed=6, n_gauss=n_gauss, lengths=lengths)
    a0 = 0.2 * rng.standard_normal((L, N))
    ycat = np.concatenate([t["y"] for t in trials])
    b0 = np.zeros((1, N))
    b0[0, :N - n_gauss] = np.log(np.maximum(ycat[:, :N - n_gauss].mean(0), 1e-8))
    lik = ["poisson"] * (N - n_gauss) + ["gaussian"] * n_gauss
    mu0 = [0.2 * rng.standard_normal((T, L)) for T in lengths]
    fresh = lambda: [{"ID": i, "y": t["y"].copy(), "mu": m.copy()} for i, (t, m) in enumerate(zip(trials, mu0))]
    kw = dict(a=a0.copy(), b=b0.copy(), lik=lik, max_iter=2, min_iter=2, Eniter=3, Mniter=3)

    mine = fresh()
    sess = FitSession(mine, L, verbose=False, **kw)
    sess.run()
    sess.eng.merge(SET_SEGMENTS)
    sess.dev_trials.pull(("mu", "v", "w"))
    after_vem = [{k: t[k].copy() for k in ("mu", "v", "w")} for t in mine]
    got = sess.finish()

    ref = fresh()
    for t in ref:
        T = t["y"].shape[0]
        t["x"] = np.ones((T, 1, N))
        t["w"] = np.zeros((T, L))
        t["v"] = np.zeros((T, L))
    cfg = O.make_config(max_iter=2, min_iter=2, Eniter=3, Mniter=3)
    params = O.make_params(ref, L, a=a0.copy(), b=b0.copy(), lik=lik)
    O.fit_given_init(ref, params, cfg)

    gp_ = got["params"]
    # (1e-5: the fit against the ORACLE's fit -- two L-BFGS-B runs on objectives that differ in the last bits stop within
    # ftol = 2.2e-9 of the same flat optimum, i.e. ~1e-6 apart in omega; the real reference's trajectory holds 1e-6)
    for k in ("omega", "a", "b", "noise"):
        assert relerr(gp_[k], params[k]) < 1e-5, k
    for T, Gg in gp_["cholesky"].items():
        for l in range(L):
            assert np.array_equal(Gg[l], O.ichol_gauss(T, gp_["omega"][l], 50) * gp_["sigma"][l])
    stage = [{"y": t["y"], "x": np.ones((t["y"].shape[0], 1, N)), "dmu": np.zeros_like(s["mu"]),
              **{k: s[k].copy() for k in ("mu", "v", "w")}} for t, s in zip(mine, after_vem)]
    p2 = dict(params)
    for k in ("a", "b", "noise", "omega", "sigma"):
        p2[k] = np.array(gp_[k])
    O.make_cholesky(stage, p2, cfg)
    O.update_w(stage, p2, cfg)
    O.update_v(stage, p2, cfg)
    O.infer(stage, p2, cfg)
    for tg, tr in zip(got["trials"], stage):
        for k in ("mu", "v", "w"):
            assert relerr(tg[k], tr[k]) < TRAJ, (k, tr["y"].shape[0])


def test_c5_full_size_500_ragged_trials(V):
    """BASELINE.json configs[4] at its REAL size on one GPU: 500 trials of 500 ... 2000 bins (multiples of the
    window), 150 Poisson + 50 Gaussian channels, ten latents -> ~12.9 k segments, ~640 k bins.  Two EM iterations
    with every default through FitSession, then every stage at full size against the oracle from the state the
    fit left on the device: the split E-step (L = 10, mixed likelihood) on 100 random segments, one Newton
    iteration of the M-step over ALL rows, the H-step objective over ALL segments, the final full-length
    inference of 10 trials; plus the size-independent bounds 0 <= v <= diag(GG')."""
    from vlgp_amd import synth
    from vlgp_amd.api import SET_SEGMENTS, FitSession

    n_trials, N, L, n_gauss, T = 500, 200, 10, 50, 50
    lengths = (50 * np.random.default_rng(0).integers(10, 41, n_trials)).tolist()
    trials = synth.make_trials(n_trials, 2000, N, L, seed=0, n_gauss=n_gauss, lengths=lengths)
    lik = ["poisson"] * (N - n_gauss) + ["gaussian"] * n_gauss
    gauss = np.array([k == "gaussian" for k in lik])
    np.random.seed(0)
    sess = FitSession(trials, L, verbose=False, lik=lik, max_iter=2, min_iter=2)
    try:
        eng, sid = sess.eng, sess.segs.set_id
        sess.run()
        assert eng.last_estep_path in ("split", "split_mixed")   # the E-step of the EM loop ran on the chip-wide launch sequence
        assert len(sess.segs) == sum(lengths) // T
        p = sess.params
        a, b, noise = np.array(p["a"]), np.array(p["b"]), np.array(p["noise"])
        omega, sigma = np.array(p["omega"]), np.array(p["sigma"])
        G = eng.get_prior(T)
        for l in range(L):  # the factor the next E-step uses is the reference's, bit for bit
            assert np.array_equal(G[l], O.ichol_gauss(T, omega[l], 50) * sigma[l])
        sess.segs.pull(("mu", "v", "w"))
        segs = list(sess.segs)
        M = len(segs)
        rng = np.random.default_rng(3)

        # ---- H-step objective: all segments, three latents
        lat = np.array([0, 4, 9], dtype=np.int32)
        logp = np.log(np.array([[sigma[l] ** 2, omega[l] * 1.1, p["gp_noise"]] for l in lat]))
        ll, dll = eng.hstep_objective(sid, T, 1.0, lat, logp)
        mu_all = np.stack([s["mu"] for s in segs])
        w_all = np.stack([s["w"] for s in segs])
        tgrid = np.arange(T) * 1.0
        for e, l in enumerate(lat):
            want_ll, want_dll = O.gp_objective(logp[e], tgrid, mu_all[:, :, l].T, w_all[:, :, l].T)
            assert abs(ll[e] - want_ll) <= STAGE * abs(want_ll), l
            assert abs(dll[e, 1] - want_dll[1]) <= STAGE * max(abs(want_dll[1]), 1e-3 * abs(want_ll)), l

        # ---- M-step: one Newton iteration over all rows
        cat = lambda k: np.concatenate([s[k] for s in segs], axis=0)
        y_all, v_all2 = cat("y"), cat("v")
        rows = y_all.shape[0]
        x_all = np.broadcast_to(np.ones((1, 1, 1)), (rows, 1, N))
        want = O.mstep_arrays(y_all, x_all, mu_all.reshape(rows, L), v_all2, a.copy(), b.copy(), gauss, 1)
        eng.mstep(sid, 1)
        a1, b1, noise1, _, _ = eng.get_params()
        eng.set_params(a, b, noise)
        assert relerr(a1, want[0]) < STAGE and relerr(b1, want[1]) < STAGE and relerr(noise1, want[4]) < STAGE
        del y_all, x_all, want

        # ---- E-step: three more sweeps on the device, 100 random segments against the oracle
        eng.estep(sid, 3)
        assert eng.last_estep_path in ("split", "split_mixed")
        got = eng.download(sid)
        sh = lambda arr: arr.reshape(M, T, L)
        ones = np.ones((T, 1, N))
        for m in rng.choice(M, 100, replace=False):
            s = segs[m]
            ref = O.estep_unit(s["y"], ones, s["mu"], s["v"], s["w"], a, b, noise, gauss, G, 3)
            for k, r in zip(("mu", "v", "w"), ref):
                assert relerr(sh(got[k])[m], r) < STAGE, (k, m)
            assert np.abs(sh(got["dmu"])[m] - ref[3]).max() < STAGE * np.abs(ref[0]).max(), m
        vmax = np.einsum("ltr,ltr->tl", G, G)
        v_dev = sh(got["v"])
        assert v_dev.min() >= 0 and np.all(v_dev <= vmax[None] * (1 + 1e-12))
        del got, mu_all, w_all

        # ---- final stage of fit (api.py:66-71): full-length inference, 10 trials against the oracle
        eng.merge(SET_SEGMENTS)
        sess.dev_trials.pull(("mu", "v", "w"))
        pick = rng.choice(n_trials, 10, replace=False)
        after_vem = {int(i): {k: trials[i][k].copy() for k in ("mu", "v", "w")} for i in pick}
        res = sess.finish()
    finally:
        sess.close()
    cfg = O.make_config(max_iter=2, min_iter=2)
    p2 = O.make_params([trials[i] for i in pick], L, a=a.copy(), b=b.copy(), lik=lik)
    for k, val in (("a", a), ("b", b), ("noise", noise), ("omega", omega), ("sigma", sigma)):
        p2[k] = np.array(val)
    stage = [{"y": trials[i]["y"], "x": np.ones((trials[i]["y"].shape[0], 1, N)),
              "dmu": np.zeros_like(after_vem[int(i)]["mu"]), **{k: after_vem[int(i)][k].copy() for k in ("mu", "v", "w")}}
             for i in pick]
    O.make_cholesky(stage, p2, cfg)
    O.update_w(stage, p2, cfg)
    O.update_v(stage, p2, cfg)
    O.infer(stage, p2, cfg)
    for i, tr in zip(pick, stage):
        for k in ("mu", "v", "w"):
            assert relerr(res["trials"][i][k], tr[k]) < TRAJ, (k, int(i))
        Tn = tr["y"].shape[0]
        for l in range(L):
            assert np.array_equal(res["params"]["cholesky"][Tn][l], p2["cholesky"][Tn][l]), (Tn, l)


# ------------------------------------------------------------------ bench.py: plain line, --dump-outputs, --full
def test_bench_plain_line_dump_and_full(tmp_path):
    """A plain bench run prints the headline without the figures that take runs of their own; --dump-outputs writes the
    last timed step's parameters and posterior (float64, the same from run to run); --full adds the per-kernel pass,
    the roofline and the CPU baseline."""
    import json
    import os
    import subprocess
    import sys

    from conftest import ROOT

    def run(*extra):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
               "--workload", "C1"] + list(extra)
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stderr[-2000:]
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])

    plain = run("--dump-outputs", str(tmp_path / "a"))
    assert plain["metric"] == "EM iterations/sec" and plain["unit"] == "EM it/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f64" and plain["steps"] == 2 and len(plain["phase_ms_per_step"]["em"]) == 2
    assert abs(plain["ms_per_step"] * plain["value"] - 1e3) < 1e-6
    assert not {"kernels", "roofline", "h_step", "cpu_baseline"} & set(plain)
    run("--dump-outputs", str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(k + ".npy" for k in ("a", "b", "noise", "omega", "sigma", "mu", "v", "w", "dmu"))
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and x.shape == y.shape and relerr(x, y) < 1e-12, f
    assert np.load(tmp_path / "a" / "mu.npy").shape == (10 * 200, 3)   # C1: 10 trials x 200 bins, 3 latents
    assert np.load(tmp_path / "a" / "a.npy").shape == (3, 20)
    full = run("--full", "--cpu-trials", "2")
    assert {"kernels", "roofline", "h_step", "cpu_baseline"} <= set(full) and full["steps"] == 2
