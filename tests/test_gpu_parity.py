"""GPU parity: the HIP path (through the C ABI) against golden vectors captured
from the reference and against the CPU oracle on seeded inputs.

Tolerances (fp64, stated per SURVEY.md section 8c):
  * stage-wise with identical prior factor G: rel <= 1e-9 on mu, v, w, a, b
  * H-step objective (ll, dll): rel <= 1e-9; omega after L-BFGS-B: rel <= 1e-6
  * multi-iteration EM trajectories: rel <= 1e-6
"""
import copy

import numpy as np
import pytest

from conftest import relerr
from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu

STAGE = 1e-9
DLL_TOL = 1e-9  # (ll, dll) rel <= 1e-9
TRAJ = 1e-6


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture(params=["default", "split"])
def estep_path(request, monkeypatch):
    """Both dispatch paths of the short-unit E-step, every run: the size-based default (persistent kernels on
    fixture-sized sets) and the split E-step (estep_split.hip: the chip-wide launch sequence that takes over at
    more than 512 units -- the kernels the headline number is made of) forced onto the same inputs.
    The library reads its switches when a handle is created: the engines of these tests are created after this fixture ran."""
    if request.param == "split":
        monkeypatch.setenv("VLGP_ESTEP_SPLIT", "1")
        monkeypatch.setenv("VLGP_ESTEP_LSPLIT", "1")   # long units: one workgroup per (unit, latent) task
    else:
        monkeypatch.delenv("VLGP_ESTEP_SPLIT", raising=False)
        monkeypatch.delenv("VLGP_ESTEP_LSPLIT", raising=False)
    return request.param


def _handle_holds(V, name, value):
    """A handle created in the present environment -- as the temporary engines of V.estep / V.mstep are -- holds `value`
    for the library switch `name`: the toggle of a test that compares two settings took."""
    with V.Engine(4, 2, 1, 50) as eng:
        assert eng.switch(name) == value, (name, eng.switch(name), value)


def _ran(V, path, *calls):
    """The kernel family the seam call(s) just used is the one the parametrisation means to test."""
    from vlgp_amd import engine as E

    for c in calls:
        got = E.TRACE.get(c)
        if path == "split":
            assert got in ("split", "split_mixed", "long_split"), (c, got)
        else:
            assert got in ("fast", "generic", "long", "split", "split_mixed", "long_split"), (c, got)


def _params(g, L, N, P=1, rank=50, chol=None):
    lik = np.where(g["gauss"], "gaussian", "poisson")
    return {"ydim": N, "zdim": L, "xdim": P, "rank": rank, "a": g["a"].copy(), "b": g["b"].copy(),
            "noise": g["noise"].copy(), "likelihood": lik, "cholesky": chol or {},
            "gp_noise": 1e-4, "dt": 1}


def _units(g, keys=("y", "x", "mu", "v", "w")):
    M = g["y0"].shape[0]
    return [{k: g[k + "0"][m].copy() for k in keys} for m in range(M)]


# ------------------------------------------------------------------ prior
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_device_arithmetic_is_numpys(V):
    """The prior kernel's claim to the reference's pivots rests on the device doing NumPy's arithmetic
    bit for bit: exp as np.exp computes it (SVML restated), correctly rounded sqrt, division and fma."""
    import ctypes as C
    from vlgp_amd._lib import dptr

    rng = np.random.default_rng(0)
    parts = [-rng.uniform(0, 50, 300_000), -rng.uniform(0, 760, 300_000), rng.uniform(-1e-3, 1e-3, 50_000),
             rng.uniform(0, 709.9, 50_000), -np.exp(rng.uniform(-40, 7, 100_000)),
             np.array([0.0, -0.0, -745.2, -745.13, -746.0, -1e4, -np.inf, 1e-300, -1e-300, -708.396, -708.4, -707.7])]
    for om in (5e-2, 5e-3, 5e-4, 1.0, 0.0123456789):
        parts.append(-om * np.arange(2000.0) ** 2)
    x = np.concatenate(parts)
    a = rng.uniform(0, 4, 200_000) * np.exp(rng.uniform(-30, 30, 200_000))
    b = rng.standard_normal(200_000) * np.exp(rng.uniform(-30, 30, 200_000))
    c = rng.standard_normal(200_000)
    with V.Engine(4, 2, 1, 50) as eng:
        def probe(kind, p, q, out):
            eng._ck(eng.lib.vlgp_debug_npx(eng.h, kind, C.c_int64(p.size), dptr(p), dptr(q), dptr(out)))
            return out
        with np.errstate(over="ignore"):
            assert np.array_equal(_bits(probe(0, x, None, np.zeros_like(x))), _bits(np.exp(x)))
        assert np.array_equal(_bits(probe(1, a, None, np.zeros_like(a))), _bits(np.sqrt(a)))
        assert np.array_equal(_bits(probe(2, a, b, np.zeros_like(a))), _bits(a / b))
        # fma against exact rational arithmetic on a sample
        from fractions import Fraction as Fr
        got = probe(3, a[:2000], b[:2000], c[:2000].copy())
        want = np.array([float(Fr(float(p)) * Fr(float(q)) + Fr(float(r))) for p, q, r in zip(a[:2000], b[:2000], c[:2000])])
        assert np.array_equal(_bits(got), _bits(want))


def test_ichol_golden_bitwise(V, golden):
    """math.ichol_gauss (vlgp/math.py:76-126) on the device: the golden factors of the reference,
    rank-exhausted 1000-bin cases included, bit for bit -- i.e. the same pivot sequence."""
    g = golden("ichol")
    for i, (n, om, r) in enumerate(g["cases"]):
        n, r = int(n), int(r)
        with V.Engine(4, 1, 1, r) as eng:
            eng.build_prior([n], np.array([om]), np.ones(1))
            G, rk = eng.get_prior(n, with_rank=True)
        G = G[0]
        if n > 200:
            assert np.array_equal(G[::8], g["G%d_rows" % i])
            assert np.array_equal(G.sum(axis=0), g["G%d_colsum" % i])
        else:
            assert np.array_equal(G, g["G%d" % i])
        assert rk[0] == int((np.abs(G).sum(0) > 0).sum())


def test_ichol_one_wave_kernel_equals_block_kernel_and_oracle_bitwise(V, monkeypatch):
    """Unit lengths of at most 64 bins (the windows of vem) are factored by one wave per latent
    (ichol_exact_wave_kernel); VLGP_ICHOL_BLOCK=1 sends them through the workgroup kernel of the long lengths.  Every
    length 2 ... 64, ranks below, at and above the length, smooth to white kernels: the two and the oracle
    (math.ichol_gauss, vlgp/math.py:76-126) agree bit for bit, ranks included."""
    rng = np.random.default_rng(11)
    for T in list(range(2, 65)):
        for R in sorted({max(1, T // 2), min(50, T + 3), 64}):
            om = np.exp(rng.uniform(np.log(1e-5), np.log(8.0), 3))
            sg = 0.5 + rng.random(3)
            got = []
            for block in (False, True):
                if block:
                    monkeypatch.setenv("VLGP_ICHOL_BLOCK", "1")
                with V.Engine(4, 3, 1, R) as eng:
                    assert eng.switch("VLGP_ICHOL_BLOCK") == float(block)
                    eng.build_prior([T], om, sg)
                    got.append(eng.get_prior(T, with_rank=True))
                monkeypatch.delenv("VLGP_ICHOL_BLOCK", raising=False)
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), (T, R)
            for l in range(3):
                Go = O.ichol_gauss(T, om[l], R) * sg[l]
                assert np.array_equal(got[0][0][l], Go), (T, R, om[l])
                assert got[0][1][l] == int((np.abs(Go).sum(0) > 0).sum())


def test_switches_are_validated_reloaded_and_readable(V, monkeypatch):
    """The library's switch table on a live handle: an out-of-range or malformed value falls back to the default (and is
    reported on stderr), a valid one is held after vlgp_debug_reload_switches, an unset one returns to its default; one
    integer (VLGP_NORMS_BLOCKS, 1 ... 1024), one real (VLGP_HSTEP_LR_TOL, > 0), one flag (VLGP_ESTEP_GENERIC).
    VLGP_NORMS_BLOCKS=4096 used to let norms_kernel write its partial sums over its ticket word and past the buffer: now
    the default grid runs, and the two norms are the default's to 1e-14 relative (two sums of squares of doubles; the
    summation order follows the block count, hence not bit for bit at a VALID other count)."""
    for name in ("VLGP_NORMS_BLOCKS", "VLGP_HSTEP_LR_TOL", "VLGP_ESTEP_GENERIC"):
        monkeypatch.delenv(name, raising=False)
    rng = np.random.default_rng(8)
    units, params, gauss = _random_problem(rng, [50] * 400, 12, 3, 1, 0)  # 60 000 values: 59 blocks of 1024
    with V.Engine(12, 3, 1, 50) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, units)
        eng.set_prior(50, params["cholesky"][50])
        eng.estep(0, 2)  # (a dmu to sum)

        def norms():
            eng.norms_begin(0)
            return np.array(eng.norms_end())

        def setting(name, value):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, value)
            eng.reload_switches()
            return eng.switch(name)

        assert eng.switch("VLGP_NORMS_BLOCKS") == 256 and eng.switch("VLGP_HSTEP_LR_TOL") == 1e-12
        assert eng.switch("VLGP_ESTEP_GENERIC") == 0
        ref = norms()
        assert np.all(ref > 0)
        for bad in ("4096", "0", "-3", "12abc", ""):
            assert setting("VLGP_NORMS_BLOCKS", bad) == 256, bad
        assert setting("VLGP_NORMS_BLOCKS", "4096") == 256
        got = norms()
        assert np.all(np.abs(got - ref) <= 1e-14 * ref), (got, ref)
        assert setting("VLGP_NORMS_BLOCKS", "7") == 7
        got = norms()
        assert np.all(np.abs(got - ref) <= 1e-14 * ref), (got, ref)
        assert setting("VLGP_NORMS_BLOCKS", "1024") == 1024
        assert setting("VLGP_NORMS_BLOCKS", None) == 256
        for bad in ("0", "-1e-9", "nan", "tight"):
            assert setting("VLGP_HSTEP_LR_TOL", bad) == 1e-12, bad
        assert setting("VLGP_HSTEP_LR_TOL", "1e-10") == 1e-10
        assert setting("VLGP_HSTEP_LR_TOL", None) == 1e-12
        assert setting("VLGP_ESTEP_GENERIC", "1") == 1
        eng.estep(0, 1)
        assert eng.last_estep_path == "generic"
        assert setting("VLGP_ESTEP_GENERIC", None) == 0
        eng.estep(0, 1)
        assert eng.last_estep_path != "generic"
        with pytest.raises(V.VlgpError, match="unknown switch"):
            eng.switch("VLGP_NO_SUCH_SWITCH")


def test_iteration_tail_entry_points(V):
    """The pieces of an EM iteration's tail that no longer wait for the device: vlgp_norms_begin / _end (the sums of the
    stopping rule, vlgp/core.py:350-354, on their own stream) against vlgp_norms; vlgp_set_params and
    vlgp_apply_latent_map staged without a stream synchronisation (back-to-back calls reuse the staging buffers);
    the parameter snapshot the M-step lane leaves for vlgp_get_params, and what invalidates it."""
    rng = np.random.default_rng(5)
    N, L, T, M = 30, 4, 50, 600
    a = 0.3 * rng.standard_normal((L, N))
    b = np.log(0.4) + 0.1 * rng.standard_normal((1, N))
    y = rng.poisson(0.5, (M, T, N)).astype(float)
    mu = 0.3 * rng.standard_normal((M, T, L))
    with V.Engine(N, L, 1, 50) as eng:
        eng.set_params(a, b, np.ones(N))
        eng.upload(0, [{"y": y[m], "mu": mu[m]} for m in range(M)])
        eng.build_prior([T], np.array([1e-2, 3e-3, 2e-2, 5e-3]), np.ones(L))
        eng.update_w(0)
        eng.update_v(0)
        eng.estep(0, 3)
        eng.norms_begin(0)          # queued behind the running E-step
        eng.hstep_prepare(0, T)     # likewise
        eng.estep_wait()            # the E-step's own launches (vlgp_estep_wait), not what is queued behind them
        first = eng.norms_end()
        ref = eng.norms(0)
        assert first == ref
        eng.norms_begin(0)
        assert eng.norms_end() == ref
        with pytest.raises(V.VlgpError):
            eng.norms_end()  # nothing pending
        eng.norms_begin(0)
        eng.norms_begin(0)  # the first pass is dropped
        assert eng.norms_end() == ref
        # a writer of unit state waits for a pending pass; the pass saw the state before it
        eng.norms_begin(0)
        eng.apply_latent_map(0, np.diag([2.0, 1.0, 0.5, 1.0]))
        eng.apply_latent_map(0, np.diag([0.5, 1.0, 2.0, 1.0]), np.zeros(L))  # back to back: the staging buffer is reused
        assert eng.norms_end() == ref
        got = eng.download(0, keys=("mu",))["mu"]
        # parameters: set twice back to back, the second wins; then the M-step's snapshot
        eng.set_params(a + 1.0, b, np.ones(N))
        eng.set_params(a, b - 0.5, 2 * np.ones(N))
        a1, b1, n1, _, _ = eng.get_params()
        assert np.array_equal(a1, a) and np.array_equal(b1, b - 0.5) and np.array_equal(n1, 2 * np.ones(N))
        eng.set_params(a, b, np.ones(N))
        eng.mstep_begin(0, 3)
        bad, _ = eng.mstep_end()
        snap = eng.get_params()  # from the lane's pinned snapshot
        assert bad == 0 and not np.array_equal(snap[0], a)
        eng.set_loading(snap[0] * 2.0)  # invalidates it: the next pull reads the device
        a2, b2, _, da2, _ = eng.get_params()
        assert np.array_equal(a2, snap[0] * 2.0) and np.array_equal(b2, snap[1]) and np.array_equal(da2, snap[3])
    # the two latent maps composed: columns 0 and 2 scaled by 2 * 0.5 and 0.5 * 2
    with V.Engine(N, L, 1, 50) as eng:
        eng.set_params(a, b, np.ones(N))
        eng.upload(0, [{"y": y[m], "mu": mu[m]} for m in range(M)])
        eng.build_prior([T], np.array([1e-2, 3e-3, 2e-2, 5e-3]), np.ones(L))
        eng.update_w(0)
        eng.update_v(0)
        eng.estep(0, 3)
        plain = eng.download(0, keys=("mu",))["mu"]
    assert np.allclose(got, plain, rtol=1e-15, atol=0)


def test_ichol_device_vs_oracle_bitwise(V):
    """Several latents and lengths per call, sigma != 1, ranks, the compact copy's consumers (update_v)."""
    rng = np.random.default_rng(3)
    cases = [(50, [5e-2, 5e-3, 5e-4]), (64, [2e-2, 1e-3, 3e-2]), (37, [7e-3, 1e-2, 2e-3]), (400, [3e-2, 4e-3, 6e-4]),
             (1000, [5e-4, 2e-3, 5e-2]), (1503, [3e-3, 7e-4, 1e-2]), (50, [1.0, 5.0, 0.3]), (5, [1e-2, 1.0, 1e-4])]
    for T, omegas in cases:
        omegas = np.array(omegas)
        sigma = np.array([1.0, 0.9, 1.1])
        with V.Engine(4, 3, 1, 50) as eng:
            eng.build_prior([T], omegas, sigma)
            G, rk = eng.get_prior(T, with_rank=True)
            # rebuild in place with other hyper-parameters (the per-EM-iteration path), then back
            eng.build_prior([T], omegas[::-1].copy(), sigma)
            eng.build_prior([T], omegas, sigma)
            G2, rk2 = eng.get_prior(T, with_rank=True)
        assert np.array_equal(G, G2) and np.array_equal(rk, rk2)
        for l in range(3):
            Go = O.ichol_gauss(T, omegas[l], 50) * sigma[l]
            assert np.array_equal(G[l], Go), (T, l)
            assert rk[l] == int((np.abs(Go).sum(0) > 0).sum())
    # random lengths / timescales, several lengths in one call
    for _ in range(6):
        Ts = sorted({int(t) for t in rng.integers(2, 300, 3)})
        om = np.exp(rng.uniform(np.log(1e-5), np.log(3.0), 2))
        with V.Engine(4, 2, 1, 50) as eng:
            eng.build_prior(Ts, om, np.ones(2))
            for T in Ts:
                G = eng.get_prior(T)
                for l in range(2):
                    assert np.array_equal(G[l], O.ichol_gauss(T, om[l], 50)), (T, om[l])


# ------------------------------------------------------------------ E-step
@pytest.mark.parametrize("tag", ["pois", "mixed"])
def test_update_w_v_golden(V, golden, tag, estep_path):
    g = golden("estep_" + tag)
    units = [{"y": g["y0"][m].copy(), "x": g["x0"][m].copy(), "mu": g["mu0"][m].copy()}
             for m in range(4)]
    params = _params(g, 3, 20, chol={50: g["G"]})
    cfg = V.get_config()
    V.update_w(units, params, cfg)
    V.update_v(units, params, cfg)
    _ran(V, estep_path, "update_w", "update_v")
    for m in range(4):
        assert relerr(units[m]["w"], g["w_stage"][m]) < STAGE
        assert relerr(units[m]["v"], g["v_stage"][m]) < STAGE


@pytest.mark.parametrize("tag", ["pois", "mixed"])
@pytest.mark.parametrize("method", ["VB", "MAP"])
@pytest.mark.parametrize("n_it", [1, 25])
def test_estep_golden(V, golden, tag, method, n_it, estep_path):
    g = golden("estep_" + tag)
    units = _units(g)
    for u in units:
        u["dmu"] = np.zeros_like(u["mu"])
    params = _params(g, 3, 20, chol={50: g["G"]})
    cfg = V.get_config(method=method, Eniter=n_it)
    mu_id = [id(u["mu"]) for u in units]
    V.estep(units, params, cfg)
    _ran(V, estep_path, "estep")
    for m in range(4):
        assert id(units[m]["mu"]) == mu_id[m]  # mu updated in place, as the reference does
        for k in ("mu", "v", "w"):
            assert relerr(units[m][k], g["%s_%s_%d" % (k, method, n_it)][m]) < STAGE, (k, m)
        # the last increment is ~1e-7 |mu| after 25 sweeps: judge it on mu's scale
        ref = g["dmu_%s_%d" % (method, n_it)][m]
        assert np.abs(units[m]["dmu"] - ref).max() < STAGE * np.abs(units[m]["mu"]).max()


def test_estep_long_unit_golden(V, golden, estep_path):
    # T = 300: the persistent long-unit kernel (default for a single unit) and the task-parallel launch sequence
    # (forced), truncated-rank G injected
    g = golden("estep_long")
    units = _units(g)
    params = _params(g, 3, 20, chol={300: g["G"]})
    V.estep(units, params, V.get_config(Eniter=5))
    from vlgp_amd import engine as E
    assert E.TRACE["estep"] == ("long_split" if estep_path == "split" else "long")
    for k in ("mu", "v", "w", "dmu"):
        assert relerr(units[0][k], g[k + "_VB_5"][0]) < STAGE, k


def test_estep_zero_iterations_is_noop(V, golden):
    g = golden("estep_pois")
    units = _units(g)
    before = copy.deepcopy(units)
    V.estep(units, _params(g, 3, 20, chol={50: g["G"]}), V.get_config(Eniter=0))
    for u, b in zip(units, before):
        for k in ("mu", "v", "w"):
            assert np.array_equal(u[k], b[k])


def _random_problem(rng, lengths, N, L, P, n_gauss, rank=50):
    a = 0.4 * rng.standard_normal((L, N))
    if L > 10:  # keep eta = mu a in the range of the few-latent cases (the E-step's Newton sweeps amplify rounding ~1e3
        a *= 5.0 / L  # per sweep once rates reach e^7: 1e-12 after one sweep, 1e-6 after four, on either side)
    b = np.log(0.3) + 0.2 * rng.standard_normal((P, N))
    noise = 0.5 + rng.random(N)
    gauss = np.zeros(N, dtype=bool)
    if n_gauss:
        gauss[rng.choice(N, n_gauss, replace=False)] = True
    omega = 10 ** rng.uniform(-3.2, -1.4, size=L)
    sigma = 0.8 + 0.4 * rng.random(L)
    units = []
    for T in lengths:
        z = np.stack([np.sin(np.linspace(0, (2 + l) * np.pi, T) + rng.random() * 6) for l in range(L)], 1)
        x = np.ones((T, P, N))
        if P > 1:
            x[:, 1:, :] = 0.3 * rng.standard_normal((T, P - 1, N))
        eta = z @ a + np.einsum("tpn,pn->tn", x, b)
        y = rng.poisson(np.exp(np.minimum(eta, 3))).astype(float)
        y[:, gauss] = eta[:, gauss] + 0.7 * rng.standard_normal((T, int(gauss.sum())))
        units.append({"y": y, "x": x, "mu": z + 0.3 * rng.standard_normal((T, L))})
    chol = O.build_prior(lengths, omega, sigma, rank)
    for u in units:  # w, v consistent with mu, as api.fit prepares them (api.py:53-54)
        u["w"] = O.curvature_unit(u["y"], u["x"], u["mu"], np.zeros_like(u["mu"]), a, b, noise, gauss)
        u["v"] = O.variance_unit(u["w"], np.zeros_like(u["mu"]), chol[u["y"].shape[0]])[0]
    params = {"ydim": N, "zdim": L, "xdim": P, "rank": rank, "a": a, "b": b, "noise": noise,
              "likelihood": np.where(gauss, "gaussian", "poisson"), "cholesky": chol,
              "omega": omega, "sigma": sigma, "gp_noise": 1e-4, "dt": 1}
    return units, params, gauss


@pytest.mark.parametrize("case", [
    dict(lengths=[50] * 5, N=7, L=1, P=1, g=0),          # single latent, odd channel count
    dict(lengths=[64, 13, 50, 1, 37], N=33, L=4, P=1, g=5),  # ragged, a one-bin unit, mixed
    dict(lengths=[50, 50], N=130, L=6, P=3, g=0),        # general regressors, N > 128
    dict(lengths=[20, 45], N=1, L=2, P=1, g=0),          # one channel
    dict(lengths=[300, 150, 700], N=24, L=3, P=2, g=4),  # long ragged units, regressors
    dict(lengths=[50] * 3, N=40, L=10, P=1, g=10),       # ten latents
    dict(lengths=[1000, 1000], N=30, L=5, P=1, g=6),     # full-length trials: rank-exhausted prior (r = 50)
    dict(lengths=[65, 128, 1200], N=18, L=8, P=1, g=0),  # long-unit kernel, eight latents, just above 64 bins
])
def test_estep_random_vs_oracle(V, case, estep_path):
    _estep_case_vs_oracle(V, case, estep_path)


def _estep_case_vs_oracle(V, case, estep_path):
    import zlib
    rng = np.random.default_rng(zlib.crc32(str(sorted(case.items())).encode()))
    units, params, gauss = _random_problem(rng, case["lengths"], case["N"], case["L"], case["P"], case["g"])
    cfg = V.get_config(Eniter=4)
    want = [O.estep_unit(u["y"], u["x"], u["mu"], u["v"], u["w"], params["a"], params["b"],
                         params["noise"], gauss, params["cholesky"][u["y"].shape[0]], 4)
            for u in units]
    V.estep(units, params, cfg)
    if estep_path is not None:
        _ran(V, estep_path, "estep")
    for u, ref in zip(units, want):
        for k, r in zip(("mu", "v", "w", "dmu"), ref):
            assert relerr(u[k], r) < STAGE, (k, u["y"].shape)


@pytest.mark.parametrize("case", [
    dict(lengths=[50, 37, 120], N=26, L=20, P=1, g=3),   # twenty latents: the generic kernel compiled for 32
    dict(lengths=[50, 50], N=12, L=40, P=2, g=0),        # forty latents (compiled for 64), regressors
])
def test_estep_more_than_sixteen_latents_vs_oracle(V, case):
    """zdim > 16 (no bound in vlgp/core.py:68-113): the generic E-step kernel with its per-latent register arrays
    compiled for 32 / 64 (they spill; same arithmetic)."""
    from vlgp_amd import engine as E

    _estep_case_vs_oracle(V, case, None)
    assert E.TRACE.get("estep") == "generic"


@pytest.mark.parametrize("omega,lo,hi", [(1.6e-2, 17, 20), (3e-2, 21, 24), (4.5e-2, 25, 32)])
def test_estep_mid_rank_buckets_vs_oracle(V, omega, lo, hi, estep_path):
    """Effective ranks 17..20, 21..24 and 25..32 take their own instantiations (persistent kernel: register
    arrays of 24 / 32 entries; split E-step: the rank classes 20 / 24 / 32 of the augmented elimination): pin
    each against the oracle."""
    rng = np.random.default_rng(12)
    units, params, gauss = _random_problem(rng, [50] * 6, 30, 5, 1, 4)
    params["omega"] = np.full(5, omega)
    params["cholesky"] = O.build_prior([50], params["omega"], params["sigma"], 50)
    ranks = [int(np.any(params["cholesky"][50][l] != 0, axis=0).sum()) for l in range(5)]
    assert lo <= max(ranks) <= hi, ranks
    for u in units:
        u["w"] = O.curvature_unit(u["y"], u["x"], u["mu"], np.zeros_like(u["mu"]), params["a"], params["b"],
                                  params["noise"], gauss)
        u["v"] = O.variance_unit(u["w"], np.zeros_like(u["mu"]), params["cholesky"][50])[0]
    want = [O.estep_unit(u["y"], u["x"], u["mu"], u["v"], u["w"], params["a"], params["b"], params["noise"],
                         gauss, params["cholesky"][50], 5) for u in units]
    V.estep(units, params, V.get_config(Eniter=5))
    _ran(V, estep_path, "estep")
    for u, ref in zip(units, want):
        for k, r in zip(("mu", "v", "w", "dmu"), ref):
            assert relerr(u[k], r) < STAGE, k


@pytest.mark.parametrize("omegas,mixed,rerouted", [
    ([8e-3, 8e-3, 1.7e-2, 8e-3, 8e-3], False, True),  # every lane-per-task latent at rank 14 beside an 18: they all ride with
                                                      # the wave-per-task blocks, nothing is left to mix (the first version
                                                      # refused this launch: C3s2)
    ([5e-3, 8e-3, 1.7e-2, 6e-3, 1e-2], True, True),   # ranks 11, 14, 18, 12, 15: lane-per-task 11, 12 + wave-per-task 14, 15, 18
    ([8e-3, 8e-3, 8e-3, 8e-3, 8e-3], False, False),   # rank 14 only: the lane-per-task kernel compiled for it, no mixing
    ([5e-3, 5e-3, 8e-3, 5e-3, 2.2e-2], True, True),   # 11, 11, 14, 11, 21
    ([5e-3, 6e-3, 7e-3, 5e-3, 4.5e-2], True, False),  # ranks <= 13 beside a 29
])
def test_estep_mixed_rank_launches_vs_oracle(V, omegas, mixed, rerouted, estep_path):
    """The split E-step's per-latent launches with lane-per-task and wave-per-task latents in ONE grid (esplit_mix,
    estep_split.hip): every combination of rank classes the host can form, against the oracle -- and the same with the
    separate launches (VLGP_ESTEP_MIX=0): bit for bit where every latent keeps its kind of task (same arithmetic per task),
    to rounding where a rank-14 latent moves from a lane to a wave per task."""
    import os

    from vlgp_amd import engine as E

    rng = np.random.default_rng(21)
    units, params, gauss = _random_problem(rng, [50] * 70, 24, 5, 1, 0)
    params["omega"] = np.array(omegas)
    params["cholesky"] = O.build_prior([50], params["omega"], params["sigma"], 50)
    for u in units:
        u["w"] = O.curvature_unit(u["y"], u["x"], u["mu"], np.zeros_like(u["mu"]), params["a"], params["b"],
                                  params["noise"], gauss)
        u["v"] = O.variance_unit(u["w"], np.zeros_like(u["mu"]), params["cholesky"][50])[0]
    import copy

    units0 = copy.deepcopy(units)
    want = [O.estep_unit(u["y"], u["x"], u["mu"], u["v"], u["w"], params["a"], params["b"], params["noise"],
                         gauss, params["cholesky"][50], 4) for u in units[:12]]
    V.estep(units, params, V.get_config(Eniter=4))
    _ran(V, estep_path, "estep")
    if estep_path == "split":
        assert E.TRACE["estep"] == ("split_mixed" if mixed else "split"), (E.TRACE["estep"], omegas)
    for u, ref in zip(units, want):
        for k, r in zip(("mu", "v", "w", "dmu"), ref):
            assert relerr(u[k], r) < STAGE, k
    if estep_path == "split" and (mixed or rerouted):
        _handle_holds(V, "VLGP_ESTEP_MIX", -1.0)
        os.environ["VLGP_ESTEP_MIX"] = "0"
        try:
            _handle_holds(V, "VLGP_ESTEP_MIX", 0.0)
            V.estep(units0, params, V.get_config(Eniter=4))
            assert E.TRACE["estep"] == "split"
        finally:
            os.environ.pop("VLGP_ESTEP_MIX", None)
        for u, u0 in zip(units, units0):
            for k in ("mu", "v", "w", "dmu"):
                if rerouted:
                    assert relerr(u[k], u0[k]) < 1e-10, k
                else:
                    assert np.array_equal(u[k], u0[k]), k


def test_estep_singular_system_zeroes_update(V, estep_path):
    # a NaN curvature makes I + G'WG non-factorisable: the reference logs and
    # applies a zero update for that latent (core.py:92-94); other latents move
    rng = np.random.default_rng(3)
    units, params, gauss = _random_problem(rng, [50, 50], 12, 3, 1, 0)
    units[1]["w"][:, 1] = np.nan
    mu0 = units[1]["mu"].copy()
    v0 = units[1]["v"].copy()
    V.estep(units, params, V.get_config(Eniter=1))
    _ran(V, estep_path, "estep")
    assert np.array_equal(units[1]["mu"][:, 1], mu0[:, 1])
    assert np.array_equal(units[1]["dmu"][:, 1], np.zeros(50))
    assert not np.array_equal(units[1]["mu"][:, 0], mu0[:, 0])
    assert np.all(np.isfinite(units[0]["mu"]))
    del v0


# ------------------------------------------------------------------ M-step
@pytest.mark.parametrize("tag", ["p1", "p3", "mixed"])
@pytest.mark.parametrize("key", ["H_1", "H_25", "G_1", "G_25"])
def test_mstep_golden(V, golden, tag, key):
    g = golden("mstep_" + tag)
    M = g["y"].shape[0]
    units = [{k: g[k][m].copy() for k in ("y", "x", "mu", "v")} for m in range(M)]
    for u in units:
        u["w"] = np.zeros_like(u["mu"])
    L, N, P = g["a"].shape[0], g["a"].shape[1], g["b"].shape[0]
    params = _params(g, L, N, P)
    cfg = V.get_config(Mniter=int(key[2:]), use_hessian=key[0] == "H", learning_rate=float(g["lr_" + key]))
    V.mstep(units, params, cfg)
    for k in ("a", "b", "noise"):
        assert relerr(params[k], g["%s_%s" % (k, key)]) < STAGE, k
    # increments shrink to ~1e-7 after 25 Newton steps: judge them on the scale of a, b
    assert np.abs(params["da"] - g["da_" + key]).max() < STAGE * np.abs(params["a"]).max()
    assert np.abs(params["db"] - g["db_" + key]).max() < STAGE * np.abs(params["b"]).max()


def test_mstep_random_vs_oracle(V):
    rng = np.random.default_rng(11)
    units, params, gauss = _random_problem(rng, [50, 120, 64, 50, 50], 70, 5, 2, 9)
    cat = lambda k: np.concatenate([u[k] for u in units], axis=0)
    want = O.mstep_arrays(cat("y"), cat("x"), cat("mu"), cat("v"), params["a"], params["b"], gauss, 6)
    V.mstep(units, params, V.get_config(Mniter=6))
    for k, r in zip(("a", "b", "da", "db", "noise"), want):
        assert relerr(params[k], r) < STAGE, k


@pytest.mark.parametrize("L,P,generic", [(5, 1, False), (3, 2, False), (3, 3, False), (8, 2, True)])
def test_noise_from_sufficient_statistics_vs_two_passes_and_oracle(V, L, P, generic, monkeypatch):
    """Sets without Gaussian channels take noise = var(y - eta) (vlgp/core.py:177) from sums the M-step holds anyway
    (y'y, 1'y, 1'x beside mu'y, x'y, x'mu, x'x and the moments of mu: noise_stats_kernel) instead of two more passes over
    y; VLGP_NOISE_PASSES=1 keeps the passes (as do more than two regressors: case (3, 3)).  The two agree to rounding
    (1e-12), both with the oracle (1e-9), a / b bit for bit; regressors and the loop-based kernels included."""
    if generic:
        monkeypatch.setenv("VLGP_MSTEP_GENERIC", "1")
    _handle_holds(V, "VLGP_MSTEP_GENERIC", float(generic))
    out = []
    for passes in (False, True):
        rng = np.random.default_rng(300 + L + P)
        units, params, gauss = _random_problem(rng, [50, 120, 64, 50, 50, 77], 45, L, P, 0)
        if passes:
            monkeypatch.setenv("VLGP_NOISE_PASSES", "1")
        _handle_holds(V, "VLGP_NOISE_PASSES", float(passes))
        cat = lambda k: np.concatenate([u[k] for u in units], axis=0)
        want = O.mstep_arrays(cat("y"), cat("x"), cat("mu"), cat("v"), params["a"], params["b"], gauss, 4)
        V.mstep(units, params, V.get_config(Mniter=4))
        monkeypatch.delenv("VLGP_NOISE_PASSES", raising=False)
        assert relerr(params["noise"], want[4]) < STAGE
        out.append((params["a"].copy(), params["b"].copy(), params["noise"].copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert relerr(out[0][2], out[1][2]) < 1e-12


@pytest.mark.parametrize("tag", ["p1", "p3", "mixed"])
def test_mstep_golden_through_the_loop_based_kernels(V, golden, tag, monkeypatch):
    """The M-step fallback for more than 16 latents / 8 regressors (mstep_cache_gen, mstep_accum_gen, latent_moments_gen,
    Newton systems in global memory), forced at the golden sizes: same reference fixtures, same tolerance."""
    monkeypatch.setenv("VLGP_MSTEP_GENERIC", "1")
    _handle_holds(V, "VLGP_MSTEP_GENERIC", 1.0)
    for key in ("H_25", "G_1"):
        test_mstep_golden(V, golden, tag, key)


@pytest.mark.parametrize("L,P", [(20, 1), (5, 11), (33, 9)])
def test_mstep_many_latents_or_regressors_vs_oracle(V, L, P):
    """zdim > 16 and xdim > 8 (no bound in vlgp/core.py:174-235): six Newton iterations against the oracle."""
    rng = np.random.default_rng(100 + L + P)
    units, params, gauss = _random_problem(rng, [50, 120, 64, 50, 50], 70, L, P, 9)
    cat = lambda k: np.concatenate([u[k] for u in units], axis=0)
    want = O.mstep_arrays(cat("y"), cat("x"), cat("mu"), cat("v"), params["a"], params["b"], gauss, 6)
    V.mstep(units, params, V.get_config(Mniter=6))
    for k, r in zip(("a", "b", "da", "db", "noise"), want):
        assert relerr(params[k], r) < STAGE, k


# ------------------------------------------------------------------ H-step
def _resident(V, units, params, set_prior=True):
    eng = V.Engine(params["ydim"], params["zdim"], params["xdim"], params["rank"],
                   np.asarray(params["likelihood"]) == "gaussian")
    eng.set_params(params["a"], params["b"], params["noise"])
    eng.upload(0, units)
    if set_prior:
        for T, G in params["cholesky"].items():
            eng.set_prior(T, G)
    return V.DeviceTrials(units, eng, 0)


@pytest.mark.parametrize("lowrank", [False, True])
def test_hstep_objective_golden(V, golden, lowrank, monkeypatch):
    """(ll, dll) captured from the real reference (gp.py:12-43, 126-147) against BOTH round kernels: eight segments are
    below the size rule's threshold, so the default takes the dense matrix-pipe round; VLGP_HSTEP_LOWRANK=1 holds the
    low-rank round -- the kernel the headline runs -- to the same fixture directly (parity item 1)."""
    g = golden("hstep")
    M, T, L = g["mu"].shape
    units = [{"y": np.zeros((T, 2)), "mu": g["mu"][m].copy(), "w": g["w"][m].copy(),
              "v": np.zeros((T, L))} for m in range(M)]
    if lowrank:
        monkeypatch.setenv("VLGP_HSTEP_LOWRANK", "1")
    with V.Engine(2, L, 1, 50) as eng:
        eng.upload(0, units)
        if lowrank:
            # one round per fixture point (a point above rank 32 -- omega = 0.05 -- sends its whole round to the dense
            # kernel: in one call with the others it would take them along)
            n_pt = len(g["logp"])
            ll = np.empty((L, n_pt))
            dll = np.empty((L, n_pt, 3))
            for i in range(n_pt):
                li, di = eng.hstep_objective(0, T, 1.0, np.arange(L), np.tile(g["logp"][i], (L, 1)))
                ll[:, i], dll[:, i] = li, di
                assert eng.last_hstep_path == ("lowrank" if np.exp(g["logp"][i, 1]) < 2e-2 else "dense"), i
            ll, dll = ll.reshape(-1), dll.reshape(-1, 3)
        else:
            lat = np.repeat(np.arange(L), len(g["logp"]))
            logp = np.tile(g["logp"], (L, 1))
            ll, dll = eng.hstep_objective(0, T, 1.0, lat, logp)
            assert eng.last_hstep_path == "dense"
    ll = ll.reshape(L, -1)
    dll = dll.reshape(L, -1, 3)
    for l in range(L):
        for i in range(len(g["logp"])):
            assert abs(ll[l, i] - g["ll"][l, i]) <= STAGE * abs(g["ll"][l, i]), (l, i)
            assert abs(dll[l, i, 1] - g["dll"][l, i, 1]) <= STAGE * max(abs(g["dll"][l, i, 1]), 1e-3 * abs(g["ll"][l, i])), (l, i)
            assert dll[l, i, 0] == 0 and dll[l, i, 2] == 0


def test_hstep_bracket_and_paths_agree(V, golden, monkeypatch):
    """vlgp_hstep_begin/_end only caches the second moments of mu: same numbers with and without the
    bracket, through the dense and the generic kernels, and after the set changes inside a bracket-free sequence."""
    g = golden("hstep")
    M, T, L = g["mu"].shape
    rng = np.random.default_rng(5)
    units = [{"y": np.zeros((T, 2)), "mu": g["mu"][m].copy(), "w": g["w"][m].copy(),
              "v": np.zeros((T, L))} for m in range(M)]
    lat = np.arange(L)
    logp = np.tile(g["logp"][1], (L, 1))
    monkeypatch.setenv("VLGP_HSTEP_LOWRANK", "1")  # (eight segments: the size rule would pick the dense round)
    with V.Engine(2, L, 1, 50) as eng:
        eng.upload(0, units)
        plain = eng.hstep_objective(0, T, 1.0, lat, logp)
        eng.hstep_begin(0, T)
        first = eng.hstep_objective(0, T, 1.0, lat, logp)
        again = eng.hstep_objective(0, T, 1.0, lat, logp + 0.0)
        eng.hstep_end()
        assert eng.last_hstep_path == "lowrank"
        # vlgp_hstep_prepare: moments and the w copy enqueued ahead of the bracket -- the same numbers; dropped when an
        # entry point that may change the units runs in between (here the units DO change: the stale moments must go)
        eng.hstep_prepare(0, T)
        eng.hstep_begin(0, T)
        prepared = eng.hstep_objective(0, T, 1.0, lat, logp)
        eng.hstep_end()
        assert np.array_equal(prepared[0], plain[0]) and np.array_equal(prepared[1], plain[1])
        eng.hstep_prepare(0, T)
        eng.apply_latent_map(0, np.diag(np.full(L, 2.0)))
        eng.hstep_begin(0, T)
        scaled = eng.hstep_objective(0, T, 1.0, lat, logp)
        eng.hstep_end()
        eng.apply_latent_map(0, np.diag(np.full(L, 0.5)))  # (exact: back to the mu of the fixture)
        fresh = None
        with V.Engine(2, L, 1, 50) as eng2:
            eng2.upload(0, [dict(u, mu=2.0 * u["mu"]) for u in units])
            fresh = eng2.hstep_objective(0, T, 1.0, lat, logp)
        assert np.array_equal(scaled[0], fresh[0]) and np.array_equal(scaled[1], fresh[1])
        assert not np.array_equal(scaled[0], plain[0])
        # VLGP_HSTEP_FUSE_TABLES=1: every round workgroup factors the two folded kernel blocks itself instead of reading
        # the tables of a launch in front (measured, not faster: DESIGN 4.3) -- the same arithmetic, the same bits
        monkeypatch.setenv("VLGP_HSTEP_FUSE_TABLES", "1")
        eng.reload_switches()
        fused = eng.hstep_objective(0, T, 1.0, lat, logp)
        assert eng.last_hstep_path == "lowrank"
        assert np.array_equal(fused[0], plain[0]) and np.array_equal(fused[1], plain[1])
        monkeypatch.delenv("VLGP_HSTEP_FUSE_TABLES")
        monkeypatch.setenv("VLGP_HSTEP_DENSE", "1")
        eng.reload_switches()  # (the switches are cached when the handle is created)
        dense = eng.hstep_objective(0, T, 1.0, lat, logp)
        assert eng.last_hstep_path == "dense"
        monkeypatch.delenv("VLGP_HSTEP_DENSE")
        monkeypatch.setenv("VLGP_HSTEP_GENERIC", "1")
        eng.reload_switches()
        generic = eng.hstep_objective(0, T, 1.0, lat, logp)
        assert eng.last_hstep_path == "generic"
        monkeypatch.delenv("VLGP_HSTEP_GENERIC")
        eng.reload_switches()
        for other in (first, again):
            assert np.array_equal(other[0], plain[0]) and np.array_equal(other[1], plain[1])
        # three different algorithms (Woodbury form at the numerical rank, blocked elimination of the 50 x 50 matrices,
        # the reference's literal K^-1 + W): agreement to cond(K) x eps, far inside the parity tolerance
        assert relerr(dense[0], plain[0]) < 1e-11 and relerr(dense[1], plain[1]) < 1e-10
        assert relerr(generic[0], plain[0]) < 1e-10 and relerr(generic[1], plain[1]) < 1e-9
        # new mu: the cached moments must not survive the upload
        for u in units:
            u["mu"] = u["mu"] + 0.1 * rng.standard_normal(u["mu"].shape)
        eng.upload(0, units)
        moved = eng.hstep_objective(0, T, 1.0, lat, logp)
    t = np.arange(T) * 1.0
    for l in range(L):
        ll, dll = O.gp_objective(logp[l], t, np.stack([u["mu"][:, l] for u in units], 1),
                                 np.stack([u["w"][:, l] for u in units], 1))
        assert abs(moved[0][l] - ll) <= STAGE * abs(ll)
        assert abs(moved[1][l, 1] - dll[1]) <= STAGE * max(abs(dll[1]), 1e-3 * abs(ll))


def test_hstep_round_kernels_agree_at_scale(V, monkeypatch):
    """The low-rank round (one rank class per evaluation here: omega from 6e-4 to 1.5e-2), the dense matrix-pipe round
    and the generic kernels on 1203 segments (not a multiple of the sixteen / four segments of a block) and
    curvatures spanning five decades: same (ll, dll) to rounding; the low-rank and dense rounds repeat bit for bit."""
    rng = np.random.default_rng(8)
    M, T, L = 1203, 50, 3
    units = [{"y": np.zeros((T, 2)), "mu": rng.standard_normal((T, L)),
              "w": 10.0 ** rng.uniform(-3, 2, (T, L)), "v": np.zeros((T, L))} for _ in range(M)]
    lat = np.array([0, 1, 2, 1, 0])
    logp = np.log(np.array([[1.0, 2e-3, 1e-4], [0.8, 8e-3, 1e-4], [0.5, 1.5e-2, 1e-4], [1.0, 6e-4, 2e-4],
                            [0.3, 1e-2, 5e-5]]))
    monkeypatch.setenv("VLGP_HSTEP_LOWRANK", "1")  # (take the low-rank round whatever the size rule says)
    with V.Engine(2, L, 1, 50) as eng:
        eng.upload(0, units)
        low = eng.hstep_objective(0, T, 1.0, lat, logp)
        assert eng.last_hstep_path == "lowrank"
        again = eng.hstep_objective(0, T, 1.0, lat, logp)
        assert np.array_equal(low[0], again[0]) and np.array_equal(low[1], again[1])  # repeatable bit for bit
        monkeypatch.setenv("VLGP_HSTEP_DENSE", "1")
        eng.reload_switches()
        dense = eng.hstep_objective(0, T, 1.0, lat, logp)
        assert eng.last_hstep_path == "dense"
        assert np.array_equal(dense[0], eng.hstep_objective(0, T, 1.0, lat, logp)[0])
        monkeypatch.delenv("VLGP_HSTEP_DENSE")
        monkeypatch.setenv("VLGP_HSTEP_GENERIC", "1")
        eng.reload_switches()
        generic = eng.hstep_objective(0, T, 1.0, lat, logp)
        monkeypatch.delenv("VLGP_HSTEP_GENERIC")
        eng.reload_switches()
        # an evaluation above the rank the low-rank round takes goes to the dense kernel ALONE (a mixed round: two launches,
        # one ticket counter, one mailbox); the others keep the low-rank kernel and its bits
        rough = logp.copy()
        rough[2, 1] = np.log(4e-2)
        mixed = eng.hstep_objective(0, T, 1.0, lat, rough)
        assert eng.last_hstep_path == "mixed"
        assert np.array_equal(mixed[0][[0, 1, 3, 4]], low[0][[0, 1, 3, 4]])
        assert np.array_equal(mixed[1][[0, 1, 3, 4]], low[1][[0, 1, 3, 4]])
        st = eng.hstep_stats()
        monkeypatch.setenv("VLGP_HSTEP_DENSE", "1")
        eng.reload_switches()
        rough_dense = eng.hstep_objective(0, T, 1.0, lat, rough)
        monkeypatch.delenv("VLGP_HSTEP_DENSE")
        eng.reload_switches()
        assert np.array_equal(mixed[0][2], rough_dense[0][2]) and np.array_equal(mixed[1][2], rough_dense[1][2])
        again_mixed = eng.hstep_objective(0, T, 1.0, lat, rough)
        st2 = eng.hstep_stats()
        assert np.array_equal(again_mixed[0], mixed[0])
        assert st2[0] - st[0] == 4 and st2[2] - st[2] == 5 + 1  # (the all-dense call: 5; the mixed one: 1 dense, 4 low-rank)
    for other in (dense, generic):
        assert relerr(other[0], low[0]) < 1e-10
        assert relerr(other[1][:, 1], low[1][:, 1]) < 1e-9
    t = np.arange(T) * 1.0
    want = O.gp_objective(logp[2], t, np.stack([u["mu"][:, 2] for u in units[:40]], 1),
                          np.stack([u["w"][:, 2] for u in units[:40]], 1))
    with V.Engine(2, L, 1, 50) as eng:
        eng.upload(0, units[:40])
        got = eng.hstep_objective(0, T, 1.0, lat[2:3], logp[2:3])
    assert abs(got[0][0] - want[0]) <= STAGE * abs(want[0])
    assert abs(got[1][0, 1] - want[1][1]) <= STAGE * max(abs(want[1][1]), 1e-3 * abs(want[0]))


@pytest.mark.parametrize("dt", [0.5, 2.0, 0.02])
def test_hstep_objective_other_bin_widths_vs_oracle(V, dt, monkeypatch):
    """params["dt"] != 1 (vlgp/gp.py:113: the kernel matrix is built on t = arange(T) * dt): the low-rank round's tables and
    the host's rank thresholds take the bin width; omega scaled so that omega dt^2 spans the usual range, plus a round with
    one rough evaluation (mixed: that one on the dense kernel, the other on the low-rank one) and a round of two rough
    ones (dense).  (ll, dll) against gp.obj_func's restatement on every path."""
    rng = np.random.default_rng(int(dt * 100))
    M, T, L = 40, 50, 2
    units = [{"y": np.zeros((T, 2)), "mu": rng.standard_normal((T, L)), "w": 2.0 * rng.random((T, L)),
              "v": np.zeros((T, L))} for _ in range(M)]
    t = np.arange(T) * dt
    cases = [("lowrank", np.log(np.array([[1.0, 3e-3 / dt ** 2, 1e-4], [0.6, 1.2e-2 / dt ** 2, 1e-4]]))),
             ("mixed", np.log(np.array([[1.0, 3e-3 / dt ** 2, 1e-4], [0.6, 6e-2 / dt ** 2, 1e-4]]))),
             ("dense", np.log(np.array([[1.0, 5e-2 / dt ** 2, 1e-4], [0.6, 6e-2 / dt ** 2, 1e-4]])))]
    monkeypatch.setenv("VLGP_HSTEP_LOWRANK", "1")
    with V.Engine(2, L, 1, 50) as eng:
        eng.upload(0, units)
        for path, logp in cases:
            ll, dll = eng.hstep_objective(0, T, dt, np.arange(L), logp)
            assert eng.last_hstep_path == path
            monkeypatch.setenv("VLGP_HSTEP_GENERIC", "1")
            eng.reload_switches()
            llg, dllg = eng.hstep_objective(0, T, dt, np.arange(L), logp)
            monkeypatch.delenv("VLGP_HSTEP_GENERIC")
            eng.reload_switches()
            for l in range(L):
                want = O.gp_objective(logp[l], t, np.stack([u["mu"][:, l] for u in units], 1),
                                      np.stack([u["w"][:, l] for u in units], 1))
                for got_ll, got_dll in ((ll, dll), (llg, dllg)):
                    assert abs(got_ll[l] - want[0]) <= STAGE * abs(want[0]), (path, l)
                    assert abs(got_dll[l, 1] - want[1][1]) <= STAGE * max(abs(want[1][1]), 1e-3 * abs(want[0])), (path, l)


@pytest.mark.parametrize("T", [4, 7, 12, 20, 25, 40, 56, 64, 65, 80, 100, 127, 128, 129, 150, 200])
def test_hstep_objective_other_windows_vs_oracle(V, T, monkeypatch):
    """Windows other than 50: up to 64 bins the low-rank round (any window from 4 bins; the K block compiled for 50 /
    64 with identity padding) or, above rank 32, the dense matrix-pipe round; 65..128 the workgroup-per-segment
    kernels (hstep_prep_big / hstep_seg_big: A split at row 64, both 64 x 64 inverses and the four products on the
    matrix pipe); above 128 (round 4) the generic kernels with their matrices in global memory (any window, slow):
    (ll, dll) against gp.obj_func's restatement; 65 ... 128 also against the generic kernels."""
    rng = np.random.default_rng(T)
    M, L = 6, 2
    units = [{"y": np.zeros((T, 2)), "mu": rng.standard_normal((T, L)), "w": 2.0 * rng.random((T, L)),
              "v": np.zeros((T, L))} for _ in range(M)]
    logp = np.log(np.array([[1.0, 3e-3, 1e-4], [0.6, 2e-2, 1e-4]]))
    monkeypatch.setenv("VLGP_HSTEP_LOWRANK", "1")  # (six segments: the size rule would pick the dense round from 24 bins)
    with V.Engine(2, L, 1, 50) as eng:
        eng.upload(0, units)
        ll, dll = eng.hstep_objective(0, T, 1.0, np.arange(L), logp)
        assert eng.last_hstep_path == ("generic" if T > 128 else "big" if T > 64 else ("lowrank" if T < 56 else eng.last_hstep_path))
    t = np.arange(T) * 1.0
    for l in range(L):
        want_ll, want_dll = O.gp_objective(logp[l], t, np.stack([u["mu"][:, l] for u in units], 1),
                                           np.stack([u["w"][:, l] for u in units], 1))
        assert abs(ll[l] - want_ll) <= STAGE * abs(want_ll), (T, l)
        # windows above 64 bins (hstep_prep_big / hstep_seg_big): measured 3.2e-9 at window 128, 1e-9 holds up to 64 --
        # cond(K) grows with the window and the oracle's LAPACK path carries it as well
        assert abs(dll[l, 1] - want_dll[1]) <= (DLL_TOL if T <= 64 else 1e-8) * max(abs(want_dll[1]), 1e-3 * abs(want_ll)), (T, l)
    if 64 < T <= 128:
        monkeypatch.setenv("VLGP_HSTEP_GENERIC_SEG", "1")
        with V.Engine(2, L, 1, 50) as eng:
            eng.upload(0, units)
            ll2, dll2 = eng.hstep_objective(0, T, 1.0, np.arange(L), logp)
        assert np.abs(ll2 - ll).max() <= STAGE * np.abs(ll).max()
        assert np.abs(dll2[:, 1] - dll[:, 1]).max() <= 1e-8 * np.abs(ll).max()


def test_hstep_optimize_golden(V, golden):
    g = golden("hstep")
    M, T, L = g["mu"].shape
    units = [{"y": np.zeros((T, 2)), "mu": g["mu"][m].copy(), "w": g["w"][m].copy(),
              "v": np.zeros((T, L))} for m in range(M)]
    params = {"ydim": 2, "zdim": L, "xdim": 1, "rank": 50, "a": np.zeros((L, 2)), "b": np.zeros((1, 2)),
              "noise": np.ones(2), "likelihood": np.array(["poisson"] * 2), "sigma": g["sigma0"].copy(),
              "omega": g["omega0"].copy(), "gp_noise": 1e-4, "dt": 1, "cholesky": {}}
    dev = _resident(V, units, params, set_prior=False)
    try:
        V.hstep(dev, params, V.get_config())
        assert relerr(params["omega"], g["omega_opt"]) < 1e-6
        assert relerr(params["sigma"], g["sigma_opt"]) < 1e-9
        Gd = dev.engine.get_prior(T)
        # the rebuilt factor: the device ichol of the device's omega (bitwise the oracle's), and the
        # reference's K at its omega to the 1e-6 the optimiser is held to
        for l in range(L):
            assert np.array_equal(Gd[l], O.ichol_gauss(T, params["omega"][l], 50) * params["sigma"][l])
        assert relerr(np.einsum("ltr,lsr->lts", Gd, Gd),
                      np.einsum("ltr,lsr->lts", g["G_opt"], g["G_opt"])) < 2e-5
    finally:
        dev.engine.close()


def test_hstep_native_and_python_drivers_agree_bit_for_bit(V, golden, monkeypatch):
    """gp.optimize on the device objective through every driver: the own optimiser in C (csrc/lbfgsb.c, the default), SciPy's
    routine driven from C (VLGP_LBFGSB=scipy, the round-5 path), the Python loop (VLGP_LOCKSTEP_PYTHON=1) -- same steps, same
    arguments, same device objective -> identical omega, sigma; and the own optimiser on its own loops instead of SciPy's
    OpenBLAS (VLGP_LBFGSB_BLAS=own): the same minimiser to 1e-9."""
    from vlgp_amd import gp as G

    if G._lockstep_ext() is None:
        pytest.skip("vlgp_amd/_lockstep.so is not built")
    g = golden("hstep")
    M, T, L = g["mu"].shape
    out = {}
    for name, env in (("own", {}), ("scipy", {"VLGP_LBFGSB": "scipy"}), ("python", {"VLGP_LOCKSTEP_PYTHON": "1"}),
                      ("own_loops", {"VLGP_LBFGSB_BLAS": "own"})):
        for k in ("VLGP_LBFGSB", "VLGP_LOCKSTEP_PYTHON", "VLGP_LBFGSB_BLAS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        units = [{"y": np.zeros((T, 2)), "mu": g["mu"][m].copy(), "w": g["w"][m].copy(),
                  "v": np.zeros((T, L))} for m in range(M)]
        params = {"ydim": 2, "zdim": L, "xdim": 1, "rank": 50, "a": np.zeros((L, 2)), "b": np.zeros((1, 2)),
                  "noise": np.ones(2), "likelihood": np.array(["poisson"] * 2), "sigma": g["sigma0"].copy(),
                  "omega": g["omega0"].copy(), "gp_noise": 1e-4, "dt": 1, "cholesky": {}}
        dev = _resident(V, units, params, set_prior=False)
        try:
            V.hstep(dev, params, V.get_config())
            out[name] = (params["omega"].copy(), params["sigma"].copy())
        finally:
            dev.engine.close()
    if G._scipy_blas_addresses() is not None:
        for name in ("scipy", "python"):
            assert np.array_equal(out["own"][0], out[name][0]) and np.array_equal(out["own"][1], out[name][1]), name
    else:  # (no SciPy OpenBLAS on this host: "own" already ran on its own loops)
        assert np.array_equal(out["scipy"][0], out["python"][0])
    assert relerr(out["own_loops"][0], out["scipy"][0]) < 1e-9 and relerr(out["own_loops"][1], out["scipy"][1]) < 1e-9
    assert relerr(out["own"][0], g["omega_opt"]) < 1e-6  # ... and what the real reference's optimize returned


# ------------------------------------------------------------------ EM loop
def _c1(g):
    y = g["y"].astype(float)
    n, T, N = y.shape
    return [{"ID": i, "y": y[i].copy(), "mu": g["mu0"][i].copy()} for i in range(n)]


@pytest.mark.parametrize("tag,hs", [("H0", False), ("H1", True)])
@pytest.mark.parametrize("ichol", ["host", "device"])
def test_vem_trajectory_golden(V, golden, tag, hs, ichol):
    """Six EM iterations at C1 against the reference's trajectory.

    Both prior-factor producers -- the device kernel (default) and the host NumPy restatement --
    have the reference's pivots bit for bit, so both follow the trajectory at 1e-6.
    """
    g = golden("vem_c1")
    trials = _c1(g)
    traj = []

    def spy(tr_, p_, c_):
        traj.append((np.linalg.norm(np.concatenate([s["mu"] for s in tr_])), np.linalg.norm(p_["a"]),
                     np.linalg.norm(p_["b"]), np.array(p_["omega"])))

    np.random.seed(3)
    res = V.fit(trials, 3, a=g["a0"].copy(), b=g["b0"].copy(), Hstep=hs, max_iter=6, min_iter=6,
                callbacks=[spy], verbose=False, ichol=ichol)
    tol = TRAJ
    assert res["config"]["runtime"]["it"] == int(g["it_" + tag])
    assert relerr([t[0] for t in traj], g["norm_mu_" + tag]) < tol
    assert relerr([t[1] for t in traj], g["norm_a_" + tag]) < tol
    assert relerr([t[2] for t in traj], g["norm_b_" + tag]) < tol
    assert relerr(np.array([t[3] for t in traj]), g["omega_" + tag]) < tol
    assert relerr(res["params"]["a"], g["a_" + tag]) < tol
    assert relerr(res["params"]["b"], g["b_" + tag]) < tol
    assert relerr(res["params"]["noise"], g["noise_" + tag]) < tol


def test_fit_end_to_end_golden(V, golden):
    # H-step off: omega stays at 5e-2, where T = 200 exhausts the rank budget -- the full-length posterior
    # is only well-posed with the reference's pivots, which the device factor has (G200 compared bitwise)
    g = golden("fit_c1")
    trials = _c1(g)
    mu_ids = [id(t["mu"]) for t in trials]
    np.random.seed(3)
    res = V.fit(trials, 3, a=g["a0"].copy(), b=g["b0"].copy(), Hstep=False, max_iter=5, min_iter=5,
                verbose=False)
    assert res["trials"] is trials
    assert [id(t["mu"]) for t in trials] == mu_ids
    # the default regressors come back as the reference leaves them: a writable (T, xdim, N) array of ones
    assert trials[0]["x"].shape == (200, 1, 20) and trials[0]["x"].flags.writeable and np.all(trials[0]["x"] == 1.0)
    assert set(res) == {"trials", "params", "config"}
    for k in ("mu", "v", "w", "dmu"):
        assert relerr(np.stack([t[k] for t in trials]), g[k]) < TRAJ, k
    assert relerr(res["params"]["a"], g["a"]) < TRAJ
    assert relerr(res["params"]["b"], g["b"]) < TRAJ
    assert np.array_equal(res["params"]["cholesky"][200], g["G200"])
    assert res["config"]["runtime"]["it"] == int(g["it"])


def test_fit_default_arguments_golden(V, golden):
    """fit with the H-step on and every default left alone (vlgp/api.py:18-76) against the reference's result:
    (1) a, b, mu injected -- 5 iterations, full-length mu, v, w at 1e-6; (2) nothing injected -- factor-analysis
    initialisation from the seeded subsample, 8 iterations; the 1e-10 difference of the initialisation
    (own FactorAnalysis vs scikit-learn's) grows to ~1e-6 through the EM iterations, held to 1e-5."""
    g = golden("fit_c1_h1")
    y = g["y"].astype(float)
    trials = [{"ID": i, "y": y[i].copy(), "mu": g["mu0"][i].copy()} for i in range(y.shape[0])]
    np.random.seed(3)
    res = V.fit(trials, 3, a=g["a0"].copy(), b=g["b0"].copy(), max_iter=5, min_iter=5, verbose=False)
    p = res["params"]
    assert res["config"]["runtime"]["it"] == int(g["it"])
    for k in ("a", "b", "noise", "omega", "sigma"):
        assert relerr(p[k], g[k]) < TRAJ, k
    for k in ("mu", "v", "w", "dmu"):
        assert relerr(np.stack([t[k] for t in trials]), g[k]) < TRAJ, k
    for l in range(3):  # the returned factor is the reference's ichol_gauss of the returned omega, bit for bit
        assert np.array_equal(p["cholesky"][200][l], O.ichol_gauss(200, p["omega"][l], 50) * p["sigma"][l])
    trials = [{"ID": i, "y": y[i].copy()} for i in range(y.shape[0])]
    np.random.seed(5)
    res = V.fit(trials, 3, max_iter=8, verbose=False)
    p = res["params"]
    assert res["config"]["runtime"]["it"] == int(g["d_it"])
    for k in ("a", "b", "noise", "omega", "sigma"):
        assert relerr(p[k], g["d_" + k]) < 1e-5, k
    for k in ("mu", "v", "w"):
        assert relerr(np.stack([t[k] for t in trials]), g["d_" + k]) < 1e-5, k


def test_reference_smoke_test_fit_then_transform(V):
    # the reference's own tests/test_api.py:5-38, same data recipe, must not raise
    rng = np.random.default_rng(0)
    a = rng.standard_normal((2, 5))
    trials = []
    for i in range(5):
        z = np.column_stack((np.sin(np.linspace(0, 8 * np.pi, 100)), np.cos(np.linspace(0, 8 * np.pi, 100))))
        trials.append({"y": rng.poisson(np.exp(z @ a - 2)).astype(float), "id": i})
    res = V.fit(trials, n_factors=2, verbose=False)
    V.transform(res["trials"], res["params"], res["config"])
    assert all(np.all(np.isfinite(t["mu"])) for t in res["trials"])


# ------------------------------------------------------------------ headline-size properties
def test_headline_size_properties(V, monkeypatch):
    """C3 dims (4000 segments x 50 bins x 100 channels x 5 latents): properties
    that hold at any size -- E-step sweeps compose (25 = 10 + 15, bit for bit,
    since mu, v, w carry the whole state), units are independent (a permuted
    set gives permuted results), 0 <= v <= diag(GG')."""
    from vlgp_amd import synth

    trials = synth.make_trials(200, 1000, 100, 5, seed=0)
    rng = np.random.default_rng(1)
    L, N = 5, 100
    a = 0.3 * rng.standard_normal((L, N))
    a /= np.linalg.norm(a)
    b = np.log(np.maximum(np.mean(np.concatenate([t["y"] for t in trials]), 0, keepdims=True), 1e-8))
    omega = np.array([5e-2, 1e-2, 3e-3, 1e-3, 2e-2])
    y = np.concatenate([t["y"] for t in trials]).reshape(4000, 50, N)
    mu = 0.2 * rng.standard_normal((4000, 50, L))

    def run(order, splits, lanes=0):
        with V.Engine(N, L, 1, 50) as eng:
            assert eng.switch("VLGP_ESTEP_LANES") == lanes  # (0: unset, the lanes follow the set's size)
            eng.set_params(a, b, np.ones(N))
            eng.upload(0, [{"y": y[i], "mu": mu[i]} for i in order])
            eng.build_prior([50], omega, np.ones(L))
            eng.update_w(0)
            eng.update_v(0)
            for n in splits:
                eng.estep(0, n)
                assert eng.last_estep_path in ("split", "split_mixed")  # 4000 units / 200 k rows: the split E-step by size
            out = eng.download(0)
            G = eng.get_prior(50)
        return out, G

    ident = np.arange(4000)
    one, G = run(ident, [25])
    two, _ = run(ident, [10, 15])
    for k in ("mu", "v", "w"):
        assert np.array_equal(one[k], two[k]), k
    # the two lanes (streams) the unit set runs on by default change nothing: one lane, bit for bit
    monkeypatch.setenv("VLGP_ESTEP_LANES", "1")
    lane1, _ = run(ident, [25], lanes=1)
    monkeypatch.delenv("VLGP_ESTEP_LANES")
    for k in ("mu", "v", "w", "dmu"):
        assert np.array_equal(one[k], lane1[k]), k
    perm = np.random.default_rng(2).permutation(4000)
    shuf, _ = run(perm, [25])
    for k in ("mu", "v", "w", "dmu"):
        assert np.array_equal(shuf[k].reshape(4000, 50, L), one[k].reshape(4000, 50, L)[perm]), k
    vmax = np.einsum("ltr,ltr->tl", G, G)
    v = one["v"].reshape(4000, 50, L)
    assert v.min() >= 0 and np.all(v <= vmax[None] * (1 + 1e-12))
    # 200 random segments of the full-size run against the oracle (the run above went through the split E-step)
    ones, nz, ng = np.ones((50, 1, N)), np.ones(N), np.zeros(N, bool)
    for i in np.random.default_rng(5).choice(4000, 200, replace=False):
        w0 = O.curvature_unit(y[i], ones, mu[i], np.zeros((50, L)), a, b, nz, ng)
        v0, _ = O.variance_unit(w0, np.zeros((50, L)), G)
        ref = O.estep_unit(y[i], ones, mu[i], v0, w0, a, b, nz, ng, G, 25)
        for k, r in zip(("mu", "v", "w"), ref):
            assert relerr(one[k].reshape(4000, 50, L)[i], r) < STAGE, (k, i)
        # the 25th increment is ~1e-16 |mu| (converged): judged on mu's scale, as in test_estep_golden
        assert np.abs(one["dmu"].reshape(4000, 50, L)[i] - ref[3]).max() < STAGE * np.abs(ref[0]).max(), i


@pytest.mark.parametrize("case", [
    # regressors (x != 1 -> the HASXB passes), Gaussian channels, MAP (no variance update: the LASTSW variants), L = 8
    dict(M=1400, N=40, L=8, P=2, g=8, vb=False, n_it=4, omega=None),
    # N > 128 (lane-per-row y pass), three latents, mixed, one latent in each rank class 20 / 24 / 32
    dict(M=1320, N=130, L=3, P=1, g=5, vb=True, n_it=5, omega=[1.6e-2, 3e-2, 4.5e-2]),
    # ten latents, mixed likelihood (C5's shape), ranks <= 16 and one above
    dict(M=1311, N=24, L=10, P=1, g=6, vb=True, n_it=3, omega=[2e-3, 5e-3, 8e-3, 1e-3, 3e-3, 1.1e-2, 6e-3, 4e-3, 2e-2, 9e-4]),
    # all Gaussian, history-like regressors
    dict(M=1312, N=16, L=5, P=3, g=16, vb=True, n_it=3, omega=None),
])
def test_split_estep_at_dispatch_size_vs_oracle(V, case):
    """Sets at and above the size where the split E-step takes over BY ITSELF (more than 512 units, no
    environment switch): update_w, update_v and the E-step of every unit on the device, 60 random units against the
    oracle (core.infer_single_trial, vlgp/core.py:22-120; update_w/update_v :419-471)."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(repr(sorted((k, str(v)) for k, v in case.items())).encode()))
    M, N, L, P, T = case["M"], case["N"], case["L"], case["P"], 50
    a = 0.4 * rng.standard_normal((L, N))
    b = np.log(0.3) + 0.2 * rng.standard_normal((P, N))
    if P > 1:
        b[1:] *= 0.3
    noise = 0.5 + rng.random(N)
    gauss = np.zeros(N, dtype=bool)
    gauss[rng.choice(N, case["g"], replace=False)] = True
    omega = np.array(case["omega"]) if case["omega"] else 10 ** rng.uniform(-3.2, -1.9, size=L)
    sigma = 0.8 + 0.4 * rng.random(L)
    phase = rng.random((M, L)) * 6
    tt = np.linspace(0, 1, T)
    z = np.sin(tt[None, :, None] * (2 + np.arange(L))[None, None, :] * np.pi + phase[:, None, :])  # (M, T, L)
    x = np.ones((M, T, P, N))
    if P > 1:
        x[:, :, 1:, :] = 0.3 * rng.standard_normal((M, T, P - 1, N))
    eta = z @ a + np.einsum("mtpn,pn->mtn", x, b)
    y = rng.poisson(np.exp(np.minimum(eta, 3))).astype(float)
    y[:, :, gauss] = eta[:, :, gauss] + 0.7 * rng.standard_normal((M, T, int(gauss.sum())))
    mu = z + 0.3 * rng.standard_normal((M, T, L))
    with V.Engine(N, L, P, 50, gauss) as eng:
        eng.set_params(a, b, noise)
        eng.upload(0, [{"y": y[m], "x": x[m], "mu": mu[m], "v": np.zeros((T, L)), "w": np.zeros((T, L))} for m in range(M)])
        eng.build_prior([T], omega, sigma)
        G = eng.get_prior(T)
        eng.update_w(0)
        assert eng.last_estep_path in ("split", "split_mixed")
        eng.update_v(0, case["vb"])
        st0 = eng.download(0, keys=("v", "w"))
        eng.estep(0, case["n_it"], vb=case["vb"])
        assert eng.last_estep_path in ("split", "split_mixed")
        got = eng.download(0)
    for l in range(L):
        assert np.array_equal(G[l], O.ichol_gauss(T, omega[l], 50) * sigma[l])
    sh = lambda arr: arr.reshape(M, T, L)
    for m in rng.choice(M, 60, replace=False):
        w0 = O.curvature_unit(y[m], x[m], mu[m], np.zeros((T, L)), a, b, noise, gauss)
        assert relerr(sh(st0["w"])[m], w0) < STAGE
        v0 = O.variance_unit(w0, np.zeros((T, L)), G)[0] if case["vb"] else np.zeros((T, L))
        assert relerr(sh(st0["v"])[m], v0) < STAGE or not case["vb"]
        ref = O.estep_unit(y[m], x[m], mu[m], v0, w0, a, b, noise, gauss, G, case["n_it"], vb=case["vb"])
        for k, r in zip(("mu", "v", "w"), ref):
            if k == "v" and not case["vb"]:
                continue
            assert relerr(sh(got[k])[m], r) < STAGE, (k, m)
        assert np.abs(sh(got["dmu"])[m] - ref[3]).max() < STAGE * np.abs(ref[0]).max(), m


# ------------------------------------------------------------------ RCCL plumbing on one GPU
def test_single_rank_rccl_allreduce_is_identity(V, golden, monkeypatch):
    """With VLGP_FORCE_RCCL=1 a one-rank communicator is built: dlopen of librccl,
    unique id, ncclCommInitRank, in-stream fp64 all-reduces inside the M-step and the
    norms.  One rank -> the sums are unchanged -> results must equal the plain run."""
    monkeypatch.setenv("VLGP_FORCE_RCCL", "1")
    from vlgp_amd import engine as E
    from vlgp_amd.dist import Comm

    g = golden("mstep_mixed")
    M = g["y"].shape[0]
    units = [{k: g[k][m].copy() for k in ("y", "x", "mu", "v")} for m in range(M)]
    with V.Engine(20, 3, 1, 50, g["gauss"]) as eng:
        Comm(0, 1).attach(eng)
        assert eng.transport == "rccl" and eng.rccl_ranks == (1, 1)  # ncclCommCount of both lanes' communicators
        buf = np.arange(5.0)
        eng.allreduce_host(buf)
        assert np.array_equal(buf, np.arange(5.0))
        eng.barrier()
        eng.set_params(g["a"], g["b"], g["noise"])
        eng.upload(0, units)
        eng.mstep(0, 25)
        a, b, noise, _, _ = eng.get_params()
        n_mu, _ = eng.norms(0)
    assert relerr(a, g["a_H_25"]) < STAGE and relerr(b, g["b_H_25"]) < STAGE and relerr(noise, g["noise_H_25"]) < STAGE
    assert abs(n_mu - np.linalg.norm(g["mu"])) < 1e-12 * n_mu


# ------------------------------------------------------------------ C5-like: ragged trials, mixed likelihood, ten latents
def test_c5_like_ragged_mixed_ten_latents(V, estep_path):
    """BASELINE.json configs[4] in miniature: unequal trial lengths (multiples of the window), Poisson +
    Gaussian channels, ten latents.  Exercises the generic E-step kernels (L > 8), long units whose ten
    rank-50 factors do not fit LDS, the mixed-likelihood M-step and a ten-latent H-step, against the oracle
    run on the same inputs."""
    from vlgp_amd import synth

    lengths = [250, 400, 300, 350]
    L, N, n_gauss = 10, 24, 6
    trials = synth.make_trials(len(lengths), max(lengths), N, L, seed=4, n_gauss=n_gauss, lengths=lengths)
    rng = np.random.default_rng(8)
    a0 = 0.3 * rng.standard_normal((L, N))
    ycat = np.concatenate([t["y"] for t in trials])
    b0 = np.zeros((1, N))
    b0[0, :N - n_gauss] = np.log(np.maximum(ycat[:, :N - n_gauss].mean(0), 1e-8))
    lik = ["poisson"] * (N - n_gauss) + ["gaussian"] * n_gauss
    mu0 = [0.2 * rng.standard_normal((T, L)) for T in lengths]

    def fresh():
        return [{"ID": i, "y": t["y"].copy(), "mu": m.copy()} for i, (t, m) in enumerate(zip(trials, mu0))]

    kw = dict(a=a0.copy(), b=b0.copy(), lik=lik, max_iter=3, min_iter=3, Eniter=5, Mniter=5)
    from vlgp_amd.api import SET_SEGMENTS, FitSession

    mine = fresh()
    sess = FitSession(mine, L, verbose=False, **kw)
    sess.run()
    # state the final stage of fit starts from (api.py:66: the trials after vem, before make_cholesky/infer)
    sess.eng.merge(SET_SEGMENTS)
    sess.dev_trials.pull(("mu", "v", "w"))
    after_vem = [{k: t[k].copy() for k in ("mu", "v", "w")} for t in mine]
    got = sess.finish()

    ref_trials = fresh()
    for t in ref_trials:
        T = t["y"].shape[0]
        t["x"] = np.ones((T, 1, N))
        t["w"] = np.zeros((T, L))
        t["v"] = np.zeros((T, L))
    cfg = O.make_config(max_iter=3, min_iter=3, Eniter=5, Mniter=5)
    params = O.make_params(ref_trials, L, a=a0.copy(), b=b0.copy(), lik=lik)
    O.fit_given_init(ref_trials, params, cfg)

    # (1) the EM phase, through what it leaves in the parameters (1e-5: a fit against the ORACLE's fit -- both optimisers
    # stop within L-BFGS-B's ftol of the same flat optimum, ~1e-6 apart in omega, and a, b, noise follow)
    gp_ = got["params"]
    assert relerr(gp_["omega"], params["omega"]) < 1e-5
    assert relerr(gp_["a"], params["a"]) < 1e-5
    assert relerr(gp_["b"], params["b"]) < 1e-5
    assert relerr(gp_["noise"], params["noise"]) < 1e-5
    # (2) the returned factors are the reference's ichol_gauss of the returned omega, bit for bit, every length
    for T, Gg in gp_["cholesky"].items():
        for l in range(L):
            assert np.array_equal(Gg[l], O.ichol_gauss(T, gp_["omega"][l], 50) * gp_["sigma"][l])
    # (3) the full-length posterior of EVERY trial.  The two runs' omega differ at ~1e-9 after three L-BFGS-B
    # runs, and the rank-exhausted factor of a 250...600-bin trial is a discontinuous function of omega (pivot
    # chaos, SURVEY section 7: the reference against itself with a different LAPACK driver moves mu by 5 %), so
    # the final stage (api.py:66-71) is checked under the parameters the device run returned: oracle
    # make_cholesky / update_w / update_v / infer from the device's post-EM state, every trial, 1e-6
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
    # and where the two runs' factors happen to coincide, the end-to-end posterior agrees too
    same = [t["y"].shape[0] for t in ref_trials
            if np.array_equal(gp_["cholesky"][t["y"].shape[0]], params["cholesky"][t["y"].shape[0]])]
    for tg, tr in zip(got["trials"], ref_trials):
        if tr["y"].shape[0] in same:
            assert relerr(tg["mu"], tr["mu"]) < 1e-4  # (the final inference runs at the two fits' own a, b: 1e-5 apart)


# ------------------------------------------------------------------ other windows / likelihoods through fit
@pytest.mark.parametrize("window,lik_gauss", [(25, 0), (40, 0), (50, 12), (100, 0)])
def test_fit_other_windows_and_all_gaussian(V, window, lik_gauss):
    """window != 50 takes the generic H-step kernels (the register-resident fast path is
    compiled for the reference's default window); lik_gauss = N makes every channel Gaussian
    (closed-form M-step, no exp anywhere).  Three EM iterations against the oracle."""
    from vlgp_amd import synth

    N, L, n_bins = 12, 3, 200
    trials = synth.make_trials(6, n_bins, N, L, seed=9, n_gauss=lik_gauss)
    rng = np.random.default_rng(2)
    a0 = 0.3 * rng.standard_normal((L, N))
    ycat = np.concatenate([t["y"] for t in trials])
    b0 = np.zeros((1, N))
    npois = N - lik_gauss
    if npois:
        b0[0, :npois] = np.log(np.maximum(ycat[:, :npois].mean(0), 1e-8))
    lik = ["poisson"] * npois + ["gaussian"] * lik_gauss
    mu0 = [0.2 * rng.standard_normal((n_bins, L)) for _ in trials]
    fresh = lambda: [{"ID": i, "y": t["y"].copy(), "mu": m.copy()} for i, (t, m) in enumerate(zip(trials, mu0))]
    kw = dict(a=a0.copy(), b=b0.copy(), lik=lik, max_iter=3, min_iter=3, window=window)
    got = V.fit(fresh(), L, verbose=False, **kw)

    ref = fresh()
    for t in ref:
        t["x"] = np.ones((n_bins, 1, N))
        t["w"] = np.zeros((n_bins, L))
        t["v"] = np.zeros((n_bins, L))
    cfg = O.make_config(max_iter=3, min_iter=3, window=window)
    params = O.make_params(ref, L, a=a0.copy(), b=b0.copy(), lik=lik)
    O.fit_given_init(ref, params, cfg)
    # (1e-5: against the ORACLE's fit, see test_fit_end_to_end above)
    assert relerr(got["params"]["omega"], params["omega"]) < 1e-5
    assert relerr(got["params"]["a"], params["a"]) < 1e-5
    assert relerr(got["params"]["b"], params["b"]) < 1e-5
    assert relerr(got["params"]["noise"], params["noise"]) < 1e-5


def test_deferred_initialisation_matches_host(V):
    """fit's device-side half of preprocess.initialize (mu = transform(y), b = log mean y through
    vlgp_project_units) against the host path, which test_host_logic pins to the reference."""
    from vlgp_amd import synth
    from vlgp_amd.preprocess import get_config, get_params, initialize

    n_trials, n_bins, N, L = 12, 130, 37, 4
    host = synth.make_trials(n_trials, n_bins, N, L, seed=3)
    dev = synth.make_trials(n_trials, n_bins, N, L, seed=3)
    cfg = get_config()
    ph = get_params(host, L, omega_bound=cfg["omega_bound"])
    pd = get_params(dev, L, omega_bound=cfg["omega_bound"])
    np.random.seed(11)
    assert initialize(host, ph, cfg) is None
    np.random.seed(11)
    plan = initialize(dev, pd, cfg, defer_latent=True)
    assert plan is not None and plan["need_b"] and "b" not in {k for k, v in pd.items() if v is not None}
    assert relerr(pd["a"], ph["a"]) < 1e-12 and relerr(pd["noise"], ph["noise"]) < 1e-12
    with V.Engine(N, L, 1, 50) as eng:
        from vlgp_amd.preprocess import fill_trials
        fill_trials(dev)
        eng.upload(0, dev)
        colsum = eng.project_latent(0, plan["proj"], plan["shift"])
        mu = eng.download(0, keys=("mu",))["mu"]
    b = np.log(np.maximum(colsum[None, :] / plan["rows"], cfg["eps"]))
    assert relerr(b, ph["b"]) < 1e-13
    assert relerr(mu, np.concatenate([t["mu"] for t in host])) < 1e-12


def test_overlapping_cut_and_merge(V):
    """Trial lengths that are not multiples of the window: segments overlap at random offsets (util.cut_trial's
    multinomial draw).  The device set holds gathered copies, stored stage-major (`unit_of` maps a segment of the list to
    its unit); an in-place latent map touches a row shared by two segments twice, in both copies, as the reference's
    views would (vlgp/core.py:413-416); merging scatters the segments back."""
    from vlgp_amd.api import SET_SEGMENTS, SET_TRIALS, _segments

    rng = np.random.default_rng(4)
    lengths, N, L, window = [230, 170, 50, 120], 6, 2, 50
    trials = [{"y": rng.poisson(0.4, (T, N)).astype(float), "mu": rng.standard_normal((T, L)),
               "v": rng.random((T, L)), "w": rng.random((T, L))} for T in lengths]
    for tr in trials:
        tr["x"] = np.ones((tr["y"].shape[0], 1, N))
    mat, shift = np.array([[2.0, 0.5], [0.0, -1.0]]), np.array([0.25, -0.5])
    with V.Engine(N, L, 1, 50) as eng:
        eng.upload(SET_TRIALS, trials)
        np.random.seed(21)
        segs = _segments(trials, window, eng)
        from vlgp_amd.util import segment_starts
        np.random.seed(21)
        starts = [segment_starts(T, window) for T in lengths]
        assert len(segs) == sum(len(s) for s in starts) == 5 + 4 + 1 + 3
        assert segs.unit_of is not None and sorted(segs.unit_of) == list(range(len(segs)))
        got = eng.download(SET_SEGMENTS, keys=("mu", "v", "w"))
        unit_rows = np.concatenate([np.arange(u * window, (u + 1) * window) for u in segs.unit_of])
        want = {k: np.concatenate([tr[k][int(s):int(s) + window] for tr, st in zip(trials, starts) for s in st])
                for k in ("mu", "v", "w")}
        for k in want:
            assert np.array_equal(got[k][unit_rows], want[k]), k
        eng.apply_latent_map(SET_SEGMENTS, mat, shift)
        seg_mu = eng.download(SET_SEGMENTS, keys=("mu",))["mu"][unit_rows]
        eng.merge(SET_SEGMENTS)
        merged = eng.download(SET_TRIALS, keys=("mu",))["mu"]
    # host emulation with real views: every segment in turn, in place
    host = [tr["mu"].copy() for tr in trials]
    for mu_t, st in zip(host, starts):
        for s_ in st:
            view = mu_t[int(s_):int(s_) + window]
            view[...] = (view - shift) @ mat
    expect = np.concatenate(host)
    assert relerr(merged, expect) < 1e-14
    i = 0
    for mu_t, st in zip(host, starts):  # and both copies of a shared row hold the view's value
        for s_ in st:
            assert relerr(seg_mu[i * window:(i + 1) * window], mu_t[int(s_):int(s_) + window]) < 1e-14
            i += 1
    with pytest.raises(ValueError, match="shorter than window"):
        with V.Engine(N, L, 1, 50) as eng:
            short = [{"y": np.zeros((30, N)), "mu": np.zeros((30, L)), "v": np.zeros((30, L)), "w": np.zeros((30, L)),
                      "x": np.ones((30, 1, N))}]
            eng.upload(SET_TRIALS, short)
            _segments(short, window, eng)
