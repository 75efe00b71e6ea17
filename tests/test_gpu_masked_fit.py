"""Fit with missing observations on the device: the masked M-step (mstep_accum<..., KIND | K_MASKED, ...>), the entry
points relaxed for a masked fit set (vlgp_replicate_masked with one replica) and ``fit(..., missing=)``.

Reference: tests/masked_fit_numpy.py -- per channel the oracle's own ``mstep_arrays`` on the channel's observed rows, the
speckled restatement of the E-step from a warm start, composed in the oracle's order.  Stages are compared per channel
with ``per_channel_error`` at STAGE (1e-9, tests/test_gpu_rates.py), the whole fit at the trajectory tolerance 1e-6
(tests/test_gpu_parity.py).  Every case prints what it measured; profiles/masked_fit/measured_errors.txt records one run.
"""
import copy

import numpy as np
import pytest

import masked_fit_numpy as MF
from conftest import relerr
from oracle import vlgp_oracle as O
from test_gpu_mstep_shapes import (M_TILE, SWITCHES, channel_errors, compute_units, make_problem, params_of, ragged,
                                   units_of)
from test_gpu_rates import STAGE

pytestmark = pytest.mark.gpu

TRAJ = 1e-6
ITERS = (1, 3)
LT_OF = {1: 2, 2: 2, 3: 3, 4: 5, 5: 5, 8: 8, 9: 10, 10: 10}
PT_OF = {1: 1, 2: 2, 4: 4, 8: 8}
# N -> (CT, S, nthr, tiles) of plan(): lane <-> channel, the best-filled multiple of 64 threads
GEOMETRY = {5: (5, 64, 320, 1), 20: (20, 16, 320, 1), 24: (24, 8, 192, 1), 64: (64, 2, 128, 1), 65: (65, 7, 512, 1),
            130: (130, 3, 448, 1), 513: (512, 1, 512, 2)}
UNITS = [50, 64, 40]  # three units, 154 rows


def case(cid, N, L, P=1, lengths=UNITS, x_nonunit=False, one_wg=False):
    CT, S, nthr, tiles = GEOMETRY[N]
    expect = dict(LT=LT_OF[L], PT=PT_OF[P], exact=int(LT_OF[L] == L and P == 1), CT=CT, S=S, nthr=nthr, tiles=tiles)
    return dict(id=cid, N=N, L=L, P=P, lengths=list(lengths), rows=int(sum(lengths)), gauss=(), x_nonunit=x_nonunit,
                generic=False, one_wg=one_wg, G=1 if one_wg else None, expect=expect)


CASES = ([case("L%d" % L, 24, L) for L in (1, 2, 3, 4, 5, 8, 9, 10)]
         + [case("P1-xnonunit", 24, 3, x_nonunit=True)] + [case("P%d" % P, 24, 3, P=P) for P in (2, 4, 8)]
         + [case("N%d" % N, N, 3) for N in (5, 64, 65, 130, 513)]
         + [case("rows300-onewg", 20, 5, lengths=ragged(300), one_wg=True)])
BY_ID = {c["id"]: c for c in CASES}
MASKS = ("random30", "unit-channel", "row-all", "channel-all", "none")


def make_mask(kind, c, seed=0):
    rows, N = c["rows"], c["N"]
    m = np.zeros((rows, N), dtype=bool)
    if kind == "random30":
        m = np.random.default_rng(seed).random((rows, N)) < 0.3
    elif kind == "unit-channel":  # one channel missing in a whole unit (the second)
        m[c["lengths"][0]:c["lengths"][0] + c["lengths"][1], N - 1] = True
    elif kind == "row-all":  # one row with every channel missing
        m[rows // 2] = True
    elif kind == "channel-all":  # one channel missing everywhere
        m[:, N // 2] = True
    return m


def test_cases_cover_what_the_masked_kernels_compile():
    assert {c["expect"]["LT"] for c in CASES} == {2, 3, 5, 8, 10} and {c["expect"]["PT"] for c in CASES} == {1, 2, 4, 8}
    assert {c["L"] for c in CASES} >= {1, 2, 3, 4, 5, 8, 9, 10} and {c["N"] for c in CASES} >= {5, 64, 65, 130, 513}
    assert any(c["x_nonunit"] for c in CASES) and any(c["one_wg"] and c["rows"] > M_TILE for c in CASES)
    assert {(c["N"] + 63) // 64 for c in CASES} >= {1, 2, 3}


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def one_workgroup(V, env):
    env.setenv("VLGP_MSTEP_WG_PER_CU", repr(1.5 / compute_units(V)))


def assert_plan(eng, c):
    plan = eng.mstep_plan(c["rows"])
    for k, want in c["expect"].items():
        assert plan[k] == want, (c["id"], k, plan)
    if c["one_wg"]:
        assert plan["G"] == 1 and plan["rows_per_wg"] >= c["rows"] > M_TILE, (c["id"], plan)
    return plan


NOISE0 = lambda N: 0.5 + np.random.default_rng(99).random(N)  # noqa: E731


def masked_mstep(eng, p, mask, n_iter, **kw):
    """The M-step of the masked fit set (set 2) of the uploaded set 0, from the problem's parameters."""
    eng.set_params(p["a"], p["b"], NOISE0(p["a"].shape[1]))
    eng.replicate(0, 2, held_out=mask[None])
    try:
        bad = eng.mstep(2, n_iter, **kw)
        return params_of(eng), bad
    finally:
        eng.free_units(2)


WORST = {}


def check(tag, n_iter, got, want):
    errs = channel_errors(got, want)
    print("measured masked-fit %-34s Mniter %d  " % (tag, n_iter)
          + "  ".join("%s %.2e" % (k, float(e.max())) for k, e in errs.items()))
    for k, e in errs.items():
        WORST[k] = max(WORST.get(k, 0.0), float(e.max()))
        assert np.all(e < STAGE), (tag, n_iter, k, int(np.argmax(e)), float(e.max()))


# ------------------------------------------------------------------ 1. the masked M-step against the restatement
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_masked_mstep_matches_the_restatement(V, clean_env, cid):
    c = BY_ID[cid]
    p = make_problem(c)
    if c["one_wg"]:
        one_workgroup(V, clean_env)
    with V.Engine(c["N"], c["L"], c["P"], 50) as eng:
        assert_plan(eng, c)
        eng.upload(0, units_of(p))
        for kind in MASKS:
            mask = make_mask(kind, c)
            for n_iter in ITERS:
                # (eps = 0 for the channel without an observed row: its Newton systems are all zeros)
                kw = dict(eps=0.0) if kind == "channel-all" else {}
                want = MF.mstep_masked(p["y"], p["x"], p["mu"], p["v"], p["a"], p["b"], mask, n_iter, noise=NOISE0(c["N"]),
                                       **kw)
                got, bad = masked_mstep(eng, p, mask, n_iter, **kw)
                assert bad == 0, (cid, kind, n_iter, bad)
                check("%s/%s" % (cid, kind), n_iter, got, want)
                if kind == "channel-all":
                    n = c["N"] // 2
                    a1, b1, da, db, noise = got
                    assert np.array_equal(a1[:, n], p["a"][:, n]) and np.array_equal(b1[:, n], p["b"][:, n])
                    assert noise[n] == NOISE0(c["N"])[n] and not da[:, n].any() and not db[:, n].any()
    print("measured masked-fit worst so far: " + "  ".join("%s %.2e" % kv for kv in sorted(WORST.items())))


# ------------------------------------------------------------------ 2. no mask, same bits
@pytest.mark.parametrize("cid", ["L5", "L4", "P2", "N65", "N513", "rows300-onewg"])
def test_no_bit_set_gives_the_bits_of_the_plain_set(V, clean_env, cid):
    c = BY_ID[cid]
    p = make_problem(c)
    if c["one_wg"]:
        one_workgroup(V, clean_env)
    none = np.zeros((c["rows"], c["N"]), dtype=bool)
    out = {}
    for how in ("plain", "plain-passes", "masked"):
        if how == "plain-passes":
            clean_env.setenv("VLGP_NOISE_PASSES", "1")
        else:
            clean_env.delenv("VLGP_NOISE_PASSES", raising=False)
        with V.Engine(c["N"], c["L"], c["P"], 50) as eng:
            eng.upload(0, units_of(p))
            if how == "masked":
                out[how], bad = masked_mstep(eng, p, none, 3)
            else:
                eng.set_params(p["a"], p["b"], NOISE0(c["N"]))
                bad = eng.mstep(0, 3)
                out[how] = params_of(eng)
            assert bad == 0
    for k, name in enumerate(("a", "b", "da", "db")):
        assert np.array_equal(out["masked"][k], out["plain"][k]), name
        assert np.array_equal(out["masked"][k], out["plain-passes"][k]), name
    assert np.array_equal(out["masked"][4], out["plain-passes"][4]), "noise"


# ------------------------------------------------------------------ 3. missing values are never read
@pytest.mark.parametrize("cid", ["L5", "P2", "N130"])
def test_mstep_never_reads_a_missing_entry(V, clean_env, cid):
    c = BY_ID[cid]
    p = make_problem(c)
    mask = make_mask("random30", c, seed=4)
    mask[:, 1] = True  # and a channel whose every entry is garbage
    got = {}
    for fill in (0.0, np.nan, 1e300):
        q = dict(p, y=np.where(mask, fill, p["y"]))
        with V.Engine(c["N"], c["L"], c["P"], 50) as eng:
            eng.upload(0, units_of(q))
            got[repr(fill)], bad = masked_mstep(eng, q, mask, 3)
            assert bad == 0
    for fill in ("nan", "1e+300"):
        for k, name in enumerate(("a", "b", "da", "db", "noise")):
            assert np.array_equal(got[fill][k], got["0.0"][k]), (fill, name)
    assert all(np.all(np.isfinite(arr)) for arr in got["nan"])


def fit_problem(seed=13, M=3, window=40, N=12, L=2):
    """Three trials of two windows, 20 % of the entries missing, a given initialisation (a, b, mu).

    The seed is one at which the REFERENCE is a continuous function of its own intermediate results: the incomplete
    Cholesky factor of the prior is a discontinuous function of omega (pivot order; DESIGN 2, "pivot chaos"), and on a
    problem this small a relative change of 1e-12 in the omega of the first H-step can move the restated fit by 4e-6 (seed 5
    does: measured on the restatement alone).  tests/test_masked_fit_host.py checks, without a GPU, that at this seed a
    change of 1e-10 moves nothing by more than a tenth of the trajectory tolerance."""
    from vlgp_amd import synth

    trials = synth.make_trials(M, 2 * window, N, L, seed=seed)
    rng = np.random.default_rng(seed)
    missing = MF.random_missing(trials, 0.2, seed)
    y = np.concatenate([tr["y"] for tr in trials])
    M_all = np.concatenate(missing)
    a0 = 0.3 * rng.standard_normal((L, N))
    b0 = np.log(np.maximum(np.where(M_all, 0.0, y).sum(0) / (~M_all).sum(0), 1e-2))[None, :]
    for tr in trials:
        tr["mu"] = 0.2 * rng.standard_normal((tr["y"].shape[0], L))
    return trials, missing, a0, b0


def run_fit(V, trials, missing, a0, b0, window=40, **kw):
    np.random.seed(3)
    return V.fit(trials, a0.shape[0], a=a0.copy(), b=b0.copy(), missing=missing, max_iter=3, min_iter=3, window=window,
                 verbose=False, **kw)


def test_fit_never_reads_a_missing_entry(V, clean_env):
    base, missing, a0, b0 = fit_problem()
    out = {}
    for fill in (0.0, np.nan):
        trials = copy.deepcopy(base)
        for tr, m in zip(trials, missing):
            tr["y"] = np.where(m, fill, tr["y"])
        y_in = [tr["y"].copy() for tr in trials]
        out[repr(fill)] = run_fit(V, trials, missing, a0, b0)
        for tr, y0, m in zip(trials, y_in, missing):  # the caller's y is not modified, every trial carries its mask
            assert np.array_equal(tr["y"], y0, equal_nan=True) and np.array_equal(tr["missing"], m)
    for k in ("a", "b", "noise", "omega", "sigma"):
        assert np.array_equal(out["nan"]["params"][k], out["0.0"]["params"][k]), k
    for t0, t1 in zip(out["nan"]["trials"], out["0.0"]["trials"]):
        for k in ("mu", "v", "w"):
            assert np.all(np.isfinite(t0[k])) and np.array_equal(t0[k], t1[k]), k


# ------------------------------------------------------------------ 4. the relaxed entry points
def stage_problem(seed=8, lengths=(40, 40, 40), N=14, L=3):
    c = dict(id="stage", N=N, L=L, P=1, lengths=list(lengths), rows=sum(lengths), gauss=(), x_nonunit=False)
    p = make_problem(c, seed=seed)
    rng = np.random.default_rng(seed)
    p["w"] = 0.5 + rng.random(p["mu"].shape)
    p["omega"], p["sigma"] = np.array([2e-2, 5e-3, 1e-3])[:L], np.ones(L)
    return c, p


def test_relaxed_entry_points_match_the_oracle_on_a_masked_fit_set(V, clean_env):
    c, p = stage_problem()
    T, N, L = 40, c["N"], c["L"]
    mask = make_mask("random30", c, seed=2)
    gauss = np.zeros(N, dtype=bool)
    noise = np.ones(N)
    G = O.build_prior([T], p["omega"], p["sigma"], 50)[T]
    units = [dict(u, w=p["w"][s:s + T]) for u, s in zip(units_of(p), range(0, c["rows"], T))]
    y_nan = np.where(mask, np.nan, p["y"])
    for u, s in zip(units, range(0, c["rows"], T)):
        u["y"] = y_nan[s:s + T]
    with V.Engine(N, L, 1, 50) as eng:
        eng.set_params(p["a"], p["b"], noise)
        eng.set_prior(T, G)
        eng.upload(0, units)
        eng.replicate(0, 2, held_out=mask[None])
        # update_w: w of a row over its observed channels
        eng.update_w(2)
        w = eng.download(2, ("w",))["w"]
        w_ref = MF.curvature_masked(p["x"], p["mu"], p["v"], p["a"], p["b"], noise, gauss, ~mask)
        # update_v from that w
        assert eng.update_v(2, True) == 0
        v = eng.download(2, ("v",))["v"]
        v_ref = np.concatenate([O.variance_unit(w_ref[s:s + T], p["v"][s:s + T], G)[0] for s in range(0, c["rows"], T)])
        # norms, moments
        n_mu, n_dmu = eng.norms(2)
        s1, s2, cnt = eng.latent_moments(2)
        # H-step objective: the oracle on the same mu and w
        logp = np.log(np.array([[1.0, 1e-2, 1e-4]]))
        ll, dll = eng.hstep_objective(2, T, 1.0, [1], logp)
        ll_ref, dll_ref = O.gp_objective(logp[0], np.arange(T) * 1.0, p["mu"][:, 1].reshape(-1, T).T,
                                         w_ref[:, 1].reshape(-1, T).T)
        eng.hstep_begin(2, T)
        ll2, _ = eng.hstep_objective(2, T, 1.0, [1], logp)
        eng.hstep_end()
        # latent map
        mat = np.diag([2.0, 0.5, 3.0]) + 0.1
        shift = np.array([0.1, -0.2, 0.3])
        eng.apply_latent_map(2, mat, shift)
        mu_mapped = eng.download(2, ("mu",))["mu"]
    errs = {"w": relerr(w, w_ref), "v": relerr(v, v_ref), "norm_mu": abs(n_mu - np.linalg.norm(p["mu"])) / np.linalg.norm(p["mu"]),
            "sum_mu": relerr(s1, p["mu"].sum(0)), "sum_mu2": relerr(s2, (p["mu"] ** 2).sum(0)),
            "ll": abs(ll[0] - ll_ref) / abs(ll_ref), "dll": abs(dll[0, 1] - dll_ref[1]) / max(abs(dll_ref[1]), 1.0),
            "map": relerr(mu_mapped, (p["mu"] - shift) @ mat)}
    print("measured masked-fit entry points: " + "  ".join("%s %.2e" % kv for kv in errs.items()))
    assert n_dmu == 0.0 and cnt == c["rows"] and ll2[0] == ll[0]
    for k, e in errs.items():
        assert e < STAGE, (k, e)


# ------------------------------------------------------------------ 5. the whole fit against the restatement
@pytest.mark.parametrize("constrain_latent", [False, "both"])
def test_fit_with_missing_follows_the_restatement(V, clean_env, constrain_latent):
    base, missing, a0, b0 = fit_problem()
    window, L, N = 40, a0.shape[0], a0.shape[1]
    ref_trials = [{"y": tr["y"].copy(), "x": np.ones((tr["y"].shape[0], 1, N)), "mu": tr["mu"].copy()} for tr in base]
    params = O.make_params(ref_trials, L, a=a0.copy(), b=b0.copy())
    config = O.make_config(max_iter=3, min_iter=3, window=window, constrain_latent=constrain_latent)
    MF.fit_given_init(ref_trials, missing, params, config)
    trials = copy.deepcopy(base)
    for tr, m in zip(trials, missing):
        tr["y"] = np.where(m, np.nan, tr["y"])
    got = run_fit(V, trials, missing, a0, b0, window=window, constrain_latent=constrain_latent)
    assert got["config"]["runtime"]["it"] == 3
    errs = {k: relerr(got["params"][k], params[k]) for k in ("a", "b", "omega", "noise")}
    for k in ("mu", "v", "w"):
        errs[k] = relerr(np.concatenate([tr[k] for tr in got["trials"]]), np.concatenate([tr[k] for tr in ref_trials]))
    print("measured masked-fit whole fit (constrain_latent=%s): " % constrain_latent
          + "  ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < TRAJ, (k, e)


# ------------------------------------------------------------------ 6. graph replay
def test_graph_replay_takes_each_masks_own_result(V, clean_env):
    c = BY_ID["L5"]
    p = make_problem(c)
    masks = [make_mask("random30", c, seed=s) for s in (11, 12)]
    want = [MF.mstep_masked(p["y"], p["x"], p["mu"], p["v"], p["a"], p["b"], m, 3, noise=NOISE0(c["N"])) for m in masks]
    assert np.abs(want[0][0] - want[1][0]).max() > 1e-3
    with V.Engine(c["N"], c["L"], c["P"], 50) as eng:
        eng.upload(0, units_of(p))
        for rnd in range(2):  # mask A, mask B, then both again: every launch but the first may replay a captured graph
            for m, w in zip(masks, want):
                got, bad = masked_mstep(eng, p, m, 3)
                assert bad == 0
                check("replay-%d" % rnd, 3, got, w)
        # two masked fit sets alive at once: the same y, x, parameters and workspace, different mask and latents' buffers
        eng.set_params(p["a"], p["b"], NOISE0(c["N"]))
        eng.replicate(0, 2, held_out=masks[0][None])
        eng.replicate(0, 3, held_out=masks[1][None])
        for sid, w in ((2, want[0]), (3, want[1]), (2, want[0])):
            eng.set_params(p["a"], p["b"], NOISE0(c["N"]))
            assert eng.mstep(sid, 3) == 0
            check("replay-set%d" % sid, 3, params_of(eng), w)


# ------------------------------------------------------------------ 7. refusals on the device
def test_masked_mstep_refuses_what_it_cannot_mask(V, clean_env):
    def attempt(N, L, P, gauss=None, x_nonunit=False):
        c = dict(id="refuse", N=N, L=L, P=P, lengths=[40, 40], rows=80, gauss=(), x_nonunit=x_nonunit)
        p = make_problem(c, seed=1)
        with V.Engine(N, L, P, 50, gauss) as eng:
            eng.set_params(p["a"], p["b"], np.ones(N))
            eng.upload(0, units_of(p))
            eng.replicate(0, 2, held_out=make_mask("random30", dict(c), seed=1)[None])
            eng.mstep(2, 1)

    g = np.zeros(8, dtype=bool)
    g[3] = True
    with pytest.raises(V.VlgpError, match="Gaussian"):
        attempt(8, 3, 1, gauss=g)
    with pytest.raises(V.VlgpError, match="P > 8"):
        attempt(8, 3, 9)
    clean_env.setenv("VLGP_MSTEP_GENERIC", "1")
    with pytest.raises(V.VlgpError, match="VLGP_MSTEP_GENERIC"):
        attempt(8, 3, 1)
    clean_env.delenv("VLGP_MSTEP_GENERIC")
    attempt(8, 3, 1)  # the same call without the switch runs
