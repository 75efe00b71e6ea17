"""The M-step at every compiled kernel size and launch geometry, judged per channel.

csrc/mstep.hip compiles mstep_accum<LT, PT, KIND, EXACT> for LT in {2, 3, 5, 8, 10, 16} x PT in {1, 2, 4, 8} and
mstep_sum_solve_kernel<FIXED, ANYG> for FIXED in {0, 3, 5, 8, 10}; plan() chooses the launch geometry (channel tiles,
row slices, workgroups along the rows, LDS row tiles per workgroup).  The other M-step tests sample that space
thinly and under the max-norm; this module walks it:

  a  latent buckets L = 1 ... 16, exact and padded        f  row geometry: 1 ... 65 rows; 1, 2, 3 LDS tiles in ONE workgroup
  b  the same with Gaussian channels; all-Gaussian        g  partial-sum geometry: G = 1 ... 129 workgroups along the rows
  c  regressor buckets P = 1 (x != 1) ... 8               h  a slice of a, c, e, f through the loop-based kernels
  d  the corner L = 16, P = 8                             i  graph replay after new parameters, re-capture after new n_iter
  e  channel geometry N = 1 ... 1100 (one to three tiles)

Every case ASSERTS, through Engine.mstep_plan (vlgp_debug_mstep_plan: the functions the launches call, launching
nothing), that the instantiation or geometry it names is the one planned on this device -- G depends on the compute
units and on VLGP_MSTEP_WG_PER_CU -- so a retune of plan() cannot silently take the coverage away.

Reference: oracle.mstep_arrays.  a, b, da, db are compared PER CHANNEL (per_channel_error of tests/test_gpu_rates.py;
da, db on the channel's scale of a, b), the noise element-wise against the channel's own reference value, all at the
stage tolerance 1e-9, after one Newton iteration (a wrong statistic shows in da / db directly) and after three (the noise
is taken at the parameters entering the last one; the statistics buffers are reused).  The comparison rests on the
problems being well conditioned: test_every_case_is_well_conditioned checks that on the oracle alone, without a GPU.

Measured on an MI355X (profiles/mstep_shapes/measured_errors.txt, every case): a 1.4e-14, b 3.3e-15, da 1.2e-14,
db 2.2e-15, noise 2.0e-14 at worst; one ulp on every mu moves the oracle by at most 7.7e-15.  Case f-rows1 found the one
defect: the moments noise of a one-row set was +1e-16 where np.var has 0 exactly (noise_stats_kernel, fixed with it).
"""
import numpy as np
import pytest

from oracle import vlgp_oracle as O
from test_gpu_rates import STAGE, per_channel_error

gpu = pytest.mark.gpu  # per test: the conditioning check runs without a GPU

M_TILE = 256           # rows of (mu | v) per LDS tile (csrc/mstep.hip)
ITERS = (1, 3)
SWITCHES = ("VLGP_MSTEP_GENERIC", "VLGP_MSTEP_WG_PER_CU", "VLGP_NOISE_PASSES", "VLGP_NO_MGRAPH")

LT_OF = {1: 2, 2: 2, 3: 3, 4: 5, 5: 5, 6: 8, 7: 8, 8: 8, 9: 10, 10: 10, 11: 16, 13: 16, 16: 16}
PT_OF = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 7: 8, 8: 8}
FIXED_OF = {3: 3, 5: 5, 8: 8, 10: 10}  # with P == 1; 0 otherwise
# N -> (CT, S, nthr, tiles): lane <-> channel, S row slices per workgroup, the best-filled multiple of 64 threads
CHANNEL_GEOMETRY = {1: (1, 128, 128, 1), 8: (8, 16, 128, 1), 20: (20, 16, 320, 1), 24: (24, 8, 192, 1),
                    63: (63, 2, 128, 1), 64: (64, 2, 128, 1), 65: (65, 7, 512, 1), 100: (100, 5, 512, 1),
                    511: (511, 1, 512, 1), 512: (512, 1, 512, 1), 513: (512, 1, 512, 2), 1025: (512, 1, 512, 3),
                    1100: (512, 1, 512, 3)}


def ragged(total):
    """Unit lengths summing to `total` whose interior boundaries fall on no multiple of the LDS row tile."""
    out, left, k = [], total, 0
    while left > 0:
        t = min((37, 50, 23, 64, 41, 19)[k % 6], left)
        if t < left and (total - left + t) % M_TILE == 0:
            t -= 1
        out.append(t)
        left -= t
        k += 1
    inner = np.cumsum(out)[:-1]
    assert sum(out) == total and not np.any(inner % M_TILE == 0), out
    return out


def case(cid, N, L, lengths, P=1, gauss=(), x_nonunit=False, generic=False, one_wg=False, G=None, **expect):
    rows = int(sum(lengths))
    gauss = tuple(sorted(set(g for g in gauss if 0 <= g < N)))
    any_g, all_g = len(gauss) > 0, len(gauss) == N
    exp = {}
    if generic:
        exp.update(LT=0, PT=0, exact=0)
    else:
        exp.update(LT=LT_OF[L], PT=PT_OF[P], exact=int(LT_OF[L] == L and P == 1))
        CT, S, nthr, tiles = CHANNEL_GEOMETRY[N]
        exp.update(CT=CT, S=S, nthr=nthr, tiles=tiles)
    fixed = FIXED_OF.get(L, 0) if P == 1 else 0
    exp.update(fixed=fixed, anyg=int(fixed == 0 or any_g), noise_passes=int(any_g or P > 2))
    if G is not None:
        exp["G"] = G
    exp.update(expect)
    return dict(id=cid, N=N, L=L, P=P, lengths=list(lengths), rows=rows, gauss=gauss, x_nonunit=x_nonunit,
                generic=generic, one_wg=one_wg, G=G, all_gauss=all_g, expect=exp)


BASE = [50, 120, 64, 50, 50]  # 334 rows
SIX = (1, 4, 9, 13, 18, 23)   # Gaussian channels of the N = 24 cases


def build_matrix():
    m = []
    # a. latent buckets: EXACT at 2, 3, 5, 8, 10, 16, padded otherwise; FIXED 3, 5, 8, 10 and the general solve
    for L in (1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 16):
        m.append(case("a-L%d" % L, 24, L, BASE))
    # b. with Gaussian channels: both solve branches in one launch, the noise by two passes; all-Gaussian: no NEWTON
    # launch, mstep_solve_kernel alone
    for L in (3, 4, 5, 8, 10, 16):
        m.append(case("b-L%d-gauss" % L, 24, L, BASE, gauss=SIX))
    m.append(case("b-L5-allgauss", 24, 5, BASE, gauss=range(24)))
    # c. regressor buckets, exact and padded; P <= 2 takes the moments noise, more take the passes
    for L in (3, 7):
        # (x != 1 keeps L = 3 off the EXACT instantiation: PT = 1 with A.x read; the plan reports EXACT for x == 1)
        m.append(case("c-L%d-P1-xnonunit" % L, 24, L, BASE, x_nonunit=True))
        for P in (2, 3, 4, 5, 7, 8):
            m.append(case("c-L%d-P%d" % (L, P), 24, L, BASE, P=P))
    m.append(case("c-L3-P3-gauss", 24, 3, BASE, P=3, gauss=SIX))
    # d. the largest accumulator arrays of the compiled family
    m.append(case("d-L16-P8", 24, 16, BASE, P=8))
    m.append(case("d-L16-P8-gauss", 24, 16, BASE, P=8, gauss=SIX))
    # e. channel geometry: one channel, the wave edges, idle slices (N = 100: 12 idle lanes), one to three channel tiles
    # (N = 513: the second tile holds ONE channel)
    for lengths in ([50, 37, 43], [50, 120, 64, 23]):
        for N in (1, 63, 64, 65, 100, 511, 512, 513, 1025, 1100):
            m.append(case("e-N%d-rows%d" % (N, sum(lengths)), N, 3, lengths))
    for N in (513, 1100):  # Gaussian channels at the tile edges
        m.append(case("e-N%d-gauss" % N, N, 3, [50, 120, 64, 23], gauss=(0, 511, 512, N - 1)))
    m.append(case("e-N1100-P2", 1100, 3, [50, 120, 64, 23], P=2))  # x indexed across the tiles
    # f. row geometry: fewer rows than row slices (S = 16), the 64-row edges of the workgroup count ...
    for rows, lengths in ((1, [1]), (7, [3, 4]), (8, [5, 3]), (9, [4, 5]), (63, [37, 26]), (64, [37, 27]), (65, [37, 28])):
        m.append(case("f-rows%d" % rows, 20, 5, lengths, G=-(-rows // 64)))
    # ... and one, two, three LDS tiles in ONE workgroup: last tiles of 255, 256, 1, 256, 3 and 88 rows
    for rows in (255, 256, 257, 512, 515, 600):
        m.append(case("f-rows%d-onewg" % rows, 20, 5, ragged(rows), one_wg=True, G=1))
    # g. partial-sum geometry: the strided loops of sum_partials_kernel (8 slices, two loads per trip) and of
    # mstep_sum_solve_kernel (16 slices, eight loads in flight, main loop from G = 113 on)
    for G in (1, 8, 9, 16, 17, 112, 113, 128, 129):
        m.append(case("g-G%d" % G, 8, 3, ragged(64 * G), G=G))
    for G in (17, 113):  # the noise passes reduce through sum_partials_kernel
        m.append(case("g-G%d-gauss" % G, 8, 3, ragged(64 * G), gauss=(2, 5), G=G))
    # h. the loop-based kernels (VLGP_MSTEP_GENERIC=1) on a slice of a, c, e, f
    m.append(case("h-L4-generic", 24, 4, BASE, generic=True))
    m.append(case("h-P3-generic", 24, 3, BASE, P=3, generic=True))
    m.append(case("h-N513-generic", 513, 3, [50, 120, 64, 23], generic=True))
    m.append(case("h-rows257-onewg-generic", 20, 5, ragged(257), generic=True, one_wg=True, G=1))
    return m


MATRIX = build_matrix()
assert len({c["id"] for c in MATRIX}) == len(MATRIX)
BY_ID = {c["id"]: c for c in MATRIX}


def make_problem(c, seed=None):
    """Data on the model of _random_problem (tests/test_gpu_parity.py): smooth latents plus noise, v in 0.02 ... 0.07, the
    loadings scaled by 5 / L above ten latents; P == 1 with x = 1 + 0.3 randn on request."""
    N, L, P = c["N"], c["L"], c["P"]
    rng = np.random.default_rng(sum(map(ord, c["id"])) if seed is None else seed)
    a = 0.4 * rng.standard_normal((L, N))
    if L > 10:
        a *= 5.0 / L
    b = np.log(0.3) + 0.2 * rng.standard_normal((P, N))
    gauss = np.zeros(N, dtype=bool)
    gauss[list(c["gauss"])] = True
    ys, xs, mus, vs = [], [], [], []
    for T in c["lengths"]:
        z = np.stack([np.sin(np.linspace(0, (2 + l) * np.pi, T) + rng.random() * 6) for l in range(L)], 1)
        x = np.ones((T, P, N))
        if P > 1:
            x[:, 1:, :] = 0.3 * rng.standard_normal((T, P - 1, N))
        elif c["x_nonunit"]:
            x = 1.0 + 0.3 * rng.standard_normal((T, 1, N))
        eta = z @ a + np.einsum("tpn,pn->tn", x, b)
        y = rng.poisson(np.exp(np.minimum(eta, 3))).astype(float)
        y[:, gauss] = eta[:, gauss] + 0.7 * rng.standard_normal((T, int(gauss.sum())))
        ys.append(y)
        xs.append(x)
        mus.append(z + 0.3 * rng.standard_normal((T, L)))
        vs.append(0.02 + 0.05 * rng.random((T, L)))
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts, axis=0))
    return dict(y=cat(ys), x=cat(xs), mu=cat(mus), v=cat(vs), a=a, b=b, gauss=gauss, lengths=c["lengths"])


_cache = {}


def problem_and_reference(cid):
    """The case's problem and the oracle's (a, b, da, db, noise) per iteration count: computed once, shared, read-only."""
    if cid not in _cache:
        p = make_problem(BY_ID[cid])
        want = {n: O.mstep_arrays(p["y"], p["x"], p["mu"], p["v"], p["a"], p["b"], p["gauss"], n) for n in ITERS}
        for arr in list(p.values()) + [w for ws in want.values() for w in ws]:
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _cache[cid] = (p, want)
    return _cache[cid]


def channel_errors(got, want):
    """Per channel: a, b by per_channel_error; da, db on the same scales (the channel's a and b); the noise relative to
    the channel's own reference value."""
    a, b, da, db, noise = got
    ra, rb, rda, rdb, rnoise = want
    ea, eb = per_channel_error(a, b, ra, rb)
    eda = np.abs(da - rda).max(axis=0) / np.abs(ra).max(axis=0)
    edb = np.abs(db - rdb).max(axis=0) / np.maximum(np.abs(rb).max(axis=0), 1.0)
    en = np.abs(noise - rnoise) / np.maximum(np.abs(rnoise), 1e-300)
    return dict(a=ea, b=eb, da=eda, db=edb, noise=en)


def report_and_check(tag, n_iter, got, want, bound=STAGE):
    errs = channel_errors(got, want)
    print("mstep-shapes %-26s Mniter %d  " % (tag, n_iter)
          + "  ".join("%s %.2e" % (k, float(e.max())) for k, e in errs.items()))
    for k, e in errs.items():
        assert e.shape == (np.shape(want[0])[1],)
        assert np.all(e < bound), (tag, n_iter, k, int(np.argmax(e)), float(e.max()))  # (a NaN fails)


# ------------------------------------------------------------------ the condition the comparison rests on (no GPU)
def test_matrix_names_every_compiled_size():
    """The matrix reaches every compiled accumulator size, EXACT and padded, every FIXED / ANYG pair of the sum + solve
    launch and both sources of the noise (as the cases expect them; the GPU tests assert the plan agrees)."""
    compiled = [c["expect"] for c in MATRIX if not c["generic"]]
    assert {e["LT"] for e in compiled} == {2, 3, 5, 8, 10, 16} and {e["PT"] for e in compiled} == {1, 2, 4, 8}
    assert {(e["LT"], e["exact"]) for e in compiled} >= {(lt, ex) for lt in (2, 3, 5, 8, 10, 16) for ex in (0, 1)}
    assert {(e["PT"], c["P"]) for c in MATRIX for e in [c["expect"]] if not c["generic"]} >= \
        {(1, 1), (2, 2), (4, 3), (4, 4), (8, 5), (8, 7), (8, 8)}
    assert {(e["fixed"], e["anyg"]) for e in compiled} == {(0, 1)} | {(f, g) for f in (3, 5, 8, 10) for g in (0, 1)}
    assert {e["noise_passes"] for e in compiled} == {0, 1}
    assert {(16, 8)} <= {(e["LT"], e["PT"]) for e in compiled}
    assert any(c["x_nonunit"] and c["expect"]["PT"] == 1 and c["L"] == c["expect"]["LT"] for c in MATRIX)
    for c in MATRIX:
        assert c["P"] == 1 or c["rows"] >= 10 * c["P"], c["id"]  # x' diag(r) x has full rank: eps decides nothing


@pytest.mark.parametrize("cid", [c["id"] for c in MATRIX])
def test_every_case_is_well_conditioned(cid):
    """On the oracle alone: a random +-1 ulp perturbation of every mu moves no channel's a, b or noise by more than a
    tenth of the tolerance, after one and after three iterations."""
    p, want = problem_and_reference(cid)
    rng = np.random.default_rng(1)
    moved_mu = np.nextafter(p["mu"], np.where(rng.random(p["mu"].shape) < 0.5, -np.inf, np.inf))
    worst = {}
    for n in ITERS:
        base = want[n]
        moved = O.mstep_arrays(p["y"], p["x"], moved_mu, p["v"], p["a"], p["b"], p["gauss"], n)
        ea, eb = per_channel_error(moved[0], moved[1], base[0], base[1])
        en = np.abs(moved[4] - base[4]) / np.maximum(np.abs(base[4]), 1e-300)
        worst[n] = (float(ea.max()), float(eb.max()), float(en.max()))
        assert np.all(np.isfinite(base[0])) and np.all(np.isfinite(base[1])) and np.all(np.isfinite(base[4]))
    print("mstep-shapes %-26s one-ulp perturbation of mu (a, b, noise): %s" % (cid, worst))
    for n in ITERS:
        assert max(worst[n]) < 0.1 * STAGE, (cid, n, worst[n])


# ------------------------------------------------------------------ on the device
@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture
def clean_env(monkeypatch):
    """The library reads its switches when a handle is created: every handle below is created after its case's setting."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def compute_units(V):
    """The default cap of G (one workgroup per compute unit), from the plan of a set too long for anything else to bind."""
    with V.Engine(8, 3, 1, 50) as eng:
        assert eng.switch("VLGP_MSTEP_WG_PER_CU") == 1.0
        return eng.mstep_plan(1 << 30)["G"]


def set_case_switches(V, c, env):
    """VLGP_MSTEP_GENERIC and the workgroups per compute unit the case needs, the latter chosen from the device's own
    plan: a cap of one workgroup (cap = floor(value x compute units)), or a cap raised to the G the case names."""
    if c["generic"]:
        env.setenv("VLGP_MSTEP_GENERIC", "1")
    cu = compute_units(V)
    assert cu >= 1
    if c["one_wg"]:
        env.setenv("VLGP_MSTEP_WG_PER_CU", repr(1.5 / cu))
    elif c["G"] is not None and c["G"] > cu:
        env.setenv("VLGP_MSTEP_WG_PER_CU", repr((c["G"] + 0.5) / cu))
    with V.Engine(4, 2, 1, 50) as eng:  # a handle created now holds the setting
        assert eng.switch("VLGP_MSTEP_GENERIC") == float(c["generic"])


def units_of(p):
    off = np.concatenate([[0], np.cumsum(p["lengths"])])
    return [{k: p[k][s:e] for k in ("y", "x", "mu", "v")} for s, e in zip(off[:-1], off[1:])]


def assert_plan(eng, c):
    plan = eng.mstep_plan(c["rows"])
    for k, want in c["expect"].items():
        assert plan[k] == want, (c["id"], k, plan)
    assert plan["G"] * plan["rows_per_wg"] >= c["rows"] > (plan["G"] - 1) * plan["rows_per_wg"]
    if c["one_wg"]:
        assert plan["G"] == 1 and plan["rows_per_wg"] >= c["rows"], (c["id"], plan)
    return plan


def params_of(eng):
    """(a, b, da, db, noise), the order of oracle.mstep_arrays."""
    a, b, noise, da, db = eng.get_params()
    return a, b, da, db, noise


def run_mstep(V, c, p, n_iter):
    with V.Engine(c["N"], c["L"], c["P"], 50, p["gauss"]) as eng:
        plan = assert_plan(eng, c)
        eng.set_params(p["a"], p["b"], np.ones(c["N"]))
        eng.upload(0, units_of(p))
        assert eng.mstep(0, n_iter) == 0  # no singular Newton system
        return params_of(eng), plan


@gpu
def test_plan_entry_validates_and_reports(V, clean_env):
    with V.Engine(24, 4, 3, 50) as eng:
        for rows in (0, -5):
            with pytest.raises(V.VlgpError):
                eng.mstep_plan(rows)
        with pytest.raises(V.VlgpError):
            eng._ck(eng.lib.vlgp_debug_mstep_plan(eng.h, 100, None))
        plan = eng.mstep_plan(334)
        assert set(plan) == set(eng.MSTEP_PLAN_KEYS)
        assert (plan["LT"], plan["PT"], plan["exact"], plan["fixed"], plan["anyg"], plan["noise_passes"]) == (5, 4, 0, 0, 1, 1)
        assert (plan["G"], plan["rows_per_wg"]) == (6, 56)  # ceil(334 / 64) workgroups, an even split rounded up to 8 rows
    with V.Engine(24, 17, 1, 50) as eng:  # beyond the compiled sizes
        plan = eng.mstep_plan(334)
        assert (plan["LT"], plan["PT"], plan["exact"]) == (0, 0, 0)


@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in MATRIX])
def test_shapes_vs_oracle(V, cid, clean_env):
    """One case of the matrix: the plan it names, then a, b, da, db and the noise per channel at 1e-9 after one and after
    three iterations.  Gaussian channels with regressors keep b[1:, n] == 0 exactly."""
    c = BY_ID[cid]
    p, want = problem_and_reference(cid)
    set_case_switches(V, c, clean_env)
    for n_iter in ITERS:
        got, plan = run_mstep(V, c, p, n_iter)
        if n_iter == ITERS[0]:
            lds_tiles = -(-min(c["rows"], plan["rows_per_wg"]) // M_TILE)
            print("mstep-shapes %-26s plan %s, %d LDS row tile(s) per workgroup" % (cid, plan, lds_tiles))
            if c["one_wg"]:
                assert lds_tiles == -(-c["rows"] // M_TILE)
        if c["P"] > 1 and c["gauss"]:
            assert not got[1][1:, list(c["gauss"])].any()
        report_and_check(cid, n_iter, got, want[n_iter])


@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in MATRIX if c["generic"]])
def test_loop_based_slice_noise_source_leaves_a_b_bitwise(V, cid, clean_env):
    """Bit equality is claimed by the suite between the two sources of the noise only (a, b with and without
    VLGP_NOISE_PASSES: test_noise_from_sufficient_statistics_vs_two_passes_and_oracle), not between the loop-based and the
    compiled kernels, whose sums associate differently: those are both held to the oracle (test_shapes_vs_oracle).  Here
    the claimed equality on the loop-based slice."""
    c = BY_ID[cid]
    p, want = problem_and_reference(cid)
    set_case_switches(V, c, clean_env)
    out = []
    for passes in (False, True):
        if passes:
            clean_env.setenv("VLGP_NOISE_PASSES", "1")
        with V.Engine(c["N"], c["L"], c["P"], 50, p["gauss"]) as eng:
            assert eng.switch("VLGP_NOISE_PASSES") == float(passes)
            assert eng.mstep_plan(c["rows"])["noise_passes"] == int(passes or c["P"] > 2)
            eng.set_params(p["a"], p["b"], np.ones(c["N"]))
            eng.upload(0, units_of(p))
            assert eng.mstep(0, 3) == 0
            out.append(params_of(eng))
        report_and_check(cid + (" passes" if passes else " moments"), 3, out[-1], want[3])
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@gpu
def test_graph_replay_and_recapture(V, clean_env):
    """One handle: M-step, new parameters, the same M-step again -- a replay of the captured graph -- gives, bit for bit,
    what a fresh handle that enqueues every launch (VLGP_NO_MGRAPH=1) gives on the second inputs; another iteration count
    re-captures and matches the oracle."""
    c = BY_ID["b-L5-gauss"]
    p, want = problem_and_reference(c["id"])
    rng = np.random.default_rng(5)
    a2 = p["a"] + 0.05 * rng.standard_normal(p["a"].shape)
    b2 = p["b"] + 0.05 * rng.standard_normal(p["b"].shape)
    ones = np.ones(c["N"])
    with V.Engine(c["N"], c["L"], c["P"], 50, p["gauss"]) as eng:
        assert eng.switch("VLGP_NO_MGRAPH") == 0.0
        assert_plan(eng, c)
        eng.upload(0, units_of(p))
        eng.set_params(p["a"], p["b"], ones)
        assert eng.mstep(0, 3) == 0
        report_and_check("i-capture", 3, params_of(eng), want[3])
        eng.set_params(a2, b2, ones)
        assert eng.mstep(0, 3) == 0  # same key: replayed
        replayed = params_of(eng)
        eng.set_params(a2, b2, ones)
        assert eng.mstep(0, 2) == 0  # another iteration count: captured again
        recaptured = params_of(eng)
    clean_env.setenv("VLGP_NO_MGRAPH", "1")
    with V.Engine(c["N"], c["L"], c["P"], 50, p["gauss"]) as eng:
        assert eng.switch("VLGP_NO_MGRAPH") == 1.0
        eng.upload(0, units_of(p))
        eng.set_params(a2, b2, ones)
        assert eng.mstep(0, 3) == 0
        fresh = params_of(eng)
    for k, r, f in zip(("a", "b", "da", "db", "noise"), replayed, fresh):
        assert np.array_equal(r, f), k
    for n, got in ((3, replayed), (2, recaptured)):
        ref = O.mstep_arrays(p["y"], p["x"], p["mu"], p["v"], a2, b2, p["gauss"], n)
        report_and_check("i-replay" if n == 3 else "i-recapture", n, got, ref)
