"""The kernels around the five large families on the device, at every launch class and size edge their sources define
(tests/support_cases.py; tests/test_support_shapes_host.py checks the table without a GPU), against the NumPy statements of
tests/support_numpy.py and the oracle's ichol_gauss:

  a  the initial projection (project_kernel, project_colsum_kernel): mu and the column sums, up to the N = 319 channels at
     which launch_project's LDS request reaches what a compute unit has (above that the launcher is open)
  b  the latent map (latent_map_kernel_t<5, 10, 16>, latent_map_kernel, links_map_kernel)
  c  cut and merge (gather_rows_kernel, scatter_rows_kernel, scatter_unit_kernel)
  d  the norms (norms_kernel)
  e  the prior factor (ichol_exact_wave_kernel, ichol_exact_kernel<64, 256, 1024>, prior_rank_kernel, prior_compact_kernel);
     no entry point reports which of them a length takes: the cases are placed by the launcher's conditions
     (tests/support_cases.py, read from the source), the wave kernel against the workgroup of 64 by the switch it reads
  f  the posterior draws (sample_posterior_kernel)

Three comparisons and no other tolerance.  EXACT: inputs whose sums round in no order (counts, small integers, multiples of
2^-8), compared in bits.  BOUND: one real-valued case each for (a) and (b) and the w == 0 draws, element by element against
the np.longdouble statement with |err| <= (K + 2) 2^-53 S, K the number of terms and S the sum of their absolute values.
MEASURED, the posterior draws only: 16 times the float64 oracle's own distance from the np.longdouble statement, relative to
max |want|, at least 64 x 2^-53 and (host suite) below 1e-10; the device's distances on an MI355X are in
profiles/support_shapes/measured_errors.txt.
"""
import ctypes as C

import numpy as np
import pytest

import support_cases as CS
import support_numpy as S

gpu = pytest.mark.gpu
RANK = 4  # of the handles that factor nothing


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want):
    return got.shape == np.shape(want) and np.array_equal(bits(got), bits(want))


def first_diff(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    return None if not len(bad) else (len(bad), tuple(bad[0]), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


def one_unit(y, L, **more):
    z = np.zeros((y.shape[0], L))
    return dict({"y": y, "mu": z, "v": z + 1.0, "w": z + 1.0}, **more)


# ---- a. initial projection ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CS.PROJECT])
def test_projection(V, cid):
    c = CS.PROJECT_BY_ID[cid]
    y, proj, shift = CS.project_problem(c)
    with V.Engine(c["N"], c["L"], 1, RANK) as eng:
        eng.upload(0, [one_unit(y, c["L"])])
        col = eng.project_latent(0, proj, shift)
        mu = eng.download(0, keys=("mu",))["mu"]
    print("support %-20s rows/wg %d  workgroups %d  LDS %d%s" % (cid, c["rpw"], c["G"], c["lds"], " (raised)" if c["raised"] else ""))
    want_mu, want_col = S.project(y, proj, shift, np.longdouble if c["real"] else np.float64)
    assert same_bits(col, want_col.astype(np.float64)), first_diff(col, want_col.astype(np.float64))  # sums of counts: exact either way
    if c["real"]:
        err, bound = np.abs(mu.astype(np.longdouble) - want_mu), S.project_bound(y, proj, shift)
        print("support %-20s max err / bound %.3f" % (cid, float(np.max(err / bound))))
        assert np.all(err <= bound), (cid, float(np.max(err / bound)))
    else:
        assert same_bits(mu, want_mu), first_diff(mu, want_mu)


# ---- b. latent map -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CS.MAP])
def test_latent_map(V, cid):
    c = CS.MAP_BY_ID[cid]
    mu, mat, shift = CS.map_problem(c)
    with V.Engine(1, c["L"], 1, RANK) as eng:
        eng.upload(0, [one_unit(np.zeros((c["rows"], 1)), c["L"], mu=mu)])
        eng.apply_latent_map(0, mat, shift)
        got = eng.download(0, keys=("mu",))["mu"]
    print("support %-20s kernel %s, %d grid-stride trip(s)" % (cid, "latent_map_kernel_t<%d>" % c["LT"] if c["LT"] else "latent_map_kernel", c["trips"]))
    if c["real"]:
        err = np.abs(got.astype(np.longdouble) - S.latent_map(mu, mat, shift, np.longdouble))
        bound = S.latent_map_bound(mu, mat, shift)
        print("support %-20s max err / bound %.3f" % (cid, float(np.max(err / bound))))
        assert np.all(err <= bound), (cid, float(np.max(err / bound)))
    else:
        want = S.latent_map(mu, mat, shift)
        assert same_bits(got, want), first_diff(got, want)


@gpu
@pytest.mark.parametrize("L", CS.OVERLAP_L)
def test_latent_map_on_overlapping_segments(V, L):
    """Trial lengths that are no multiple of the window (as test_gpu_parity.test_overlapping_cut_and_merge builds them): a row
    two segments share is mapped twice, in both copies, as the reference's views are; exact inputs, so in bits."""
    from vlgp_amd.api import SET_SEGMENTS, SET_TRIALS, _segments
    from vlgp_amd.util import segment_starts

    rng = np.random.default_rng(40 + L)
    lengths, N, window = [230, 170, 50, 120], 3, 50
    trials = [{"y": rng.poisson(0.4, (T, N)).astype(float), "mu": CS.dyadic(rng, (T, L)), "v": CS.dyadic(rng, (T, L)) + 5.0,
               "w": CS.dyadic(rng, (T, L)) + 5.0, "x": np.ones((T, 1, N))} for T in lengths]
    mat, shift = CS.dyadic(rng, (L, L)), CS.dyadic(rng, L)
    with V.Engine(N, L, 1, RANK) as eng:
        eng.upload(SET_TRIALS, trials)
        np.random.seed(21)
        segs = _segments(trials, window, eng)
        np.random.seed(21)
        starts = [segment_starts(T, window) for T in lengths]
        assert segs.unit_of is not None  # there are shared rows
        unit_rows = np.concatenate([np.arange(u * window, (u + 1) * window) for u in segs.unit_of])
        eng.apply_latent_map(SET_SEGMENTS, mat, shift)
        seg_mu = eng.download(SET_SEGMENTS, keys=("mu",))["mu"][unit_rows]
        eng.merge(SET_SEGMENTS)
        merged = eng.download(SET_TRIALS, keys=("mu",))["mu"]
    host = [tr["mu"].copy() for tr in trials]
    for mu_t, st in zip(host, starts):  # real views, every segment in turn, in place
        for s_ in st:
            view = mu_t[int(s_):int(s_) + window]
            view[...] = S.latent_map(view, mat, shift)
    want = np.concatenate(host)
    assert same_bits(merged, want), first_diff(merged, want)
    want_seg = np.concatenate([mu_t[int(s_):int(s_) + window] for mu_t, st in zip(host, starts) for s_ in st])
    assert same_bits(seg_mu, want_seg), first_diff(seg_mu, want_seg)


# ---- c. cut and merge --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CS.CUT])
def test_cut_and_merge(V, cid):
    """mu, v, w of the cut against NumPy slicing; y through the exact projection of the cut set; x through update_w, bit for
    bit against a set uploaded from NumPy's slices (no entry point reads y or x back); then the merge of a new mu (that
    projection) and a new v (update_v under an injected factor) against sequential view assignment."""
    c = CS.CUT_BY_ID[cid]
    p = CS.cut_problem(c)
    starts, window, L, N, P = c["starts"], c["window"], c["L"], c["N"], c["P"]
    sl = {k: S.cut(p[k], starts, window) for k in ("y", "x", "mu", "v", "w")}
    segments = lambda src: [{k: src[k][i * window:(i + 1) * window] for k in src} for i in range(len(starts))]
    print("support %-20s %s scatter, %d grid-stride trip(s) of the y gather" % (cid, "one-launch" if c["one_launch"] else "unit-by-unit", c["y_trips"]))
    with V.Engine(N, L, P, RANK) as eng:
        eng.set_params(p["a"], p["b"], np.ones(N))
        eng.upload(0, [{k: p[k] for k in ("y", "x", "mu", "v", "w")}])
        eng.cut(0, 1, starts, window)
        got = eng.download(1, keys=("mu", "v", "w"))
        for k in ("mu", "v", "w"):
            assert same_bits(got[k], sl[k]), (k, first_diff(got[k], sl[k]))
        # x (and mu) of the cut: the curvature pass reads them; the same pass over an uploaded copy of NumPy's slices
        eng.upload(2, segments(sl))
        eng.update_w(1)
        eng.update_w(2)
        w_cut, w_ref = eng.download(1, keys=("w",))["w"], eng.download(2, keys=("w",))["w"]
        assert np.all(np.isfinite(w_ref)) and same_bits(w_cut, w_ref), first_diff(w_cut, w_ref)
        if P > 1:  # ... and that pass does read x: other regressors, other curvature
            eng.upload(2, segments(dict(sl, x=sl["x"][::-1].copy())))
            eng.update_w(2)
            assert not same_bits(eng.download(2, keys=("w",))["w"], w_ref)
        # y of the cut: its projection, which exact inputs make a matter of bits
        col = eng.project_latent(1, p["proj"], p["shift"])
        want_mu, want_col = S.project(sl["y"], p["proj"], p["shift"])
        got_mu = eng.download(1, keys=("mu",))["mu"]
        assert same_bits(col, want_col), first_diff(col, want_col)
        assert same_bits(got_mu, want_mu), first_diff(got_mu, want_mu)
        # the cut set now holds mu = y proj - shift; give it a v of its own too (the variance pass under an injected factor of
        # at most `window` columns), so that a scatter of v that wrote nothing, or the wrong rows, shows
        G = np.zeros((L, window, RANK))
        G[:, :, :min(window, RANK)] = 0.5 * np.random.default_rng(CS._seed(cid)).standard_normal((L, window, min(window, RANK)))
        eng.set_prior(window, G)
        eng.update_v(1)
        seg_v = eng.download(1, keys=("v",))["v"]
        assert np.all(np.isfinite(seg_v)) and np.all(bits(seg_v) != bits(sl["v"]))  # (every element is new)
        eng.merge(1)
        back = eng.download(0, keys=("mu", "v", "w"))
    for k, seg in (("mu", want_mu), ("v", seg_v)):
        want = S.merge(p[k], seg, starts, window)
        assert same_bits(back[k], want), (k, first_diff(back[k], want))
    assert same_bits(back["w"], p["w"])  # a merge writes mu and v only


@gpu
@pytest.mark.parametrize("cid", ["c-overlap-sorted", "c-overlap-equal", "c-overlap-unsorted", "c-P2"])
def test_merge_of_changed_v_later_unit_wins(V, cid):
    """Two copies of a shared row that hold different values when they are merged: an E-step over the cut set (an injected
    prior) gives every segment its own mu and v; they are downloaded, and the parent after the merge equals sequential
    assignment of what was downloaded -- the later unit wins."""
    c = CS.CUT_BY_ID[cid]
    p = CS.cut_problem(c)
    starts, window, L, N = c["starts"], c["window"], c["L"], c["N"]
    rng = np.random.default_rng(3)
    with V.Engine(N, L, c["P"], RANK) as eng:
        eng.set_params(p["a"], p["b"], np.ones(N))
        eng.upload(0, [{k: p[k] for k in ("y", "x", "mu", "v", "w")}])
        eng.cut(0, 1, starts, window)
        eng.set_prior(window, 0.5 * rng.standard_normal((L, window, RANK)))
        eng.update_w(1)
        eng.update_v(1)
        eng.estep(1, 2)
        seg = eng.download(1, keys=("mu", "v"))
        eng.merge(1)
        back = eng.download(0, keys=("mu", "v"))
    for k in ("mu", "v"):
        assert np.all(np.isfinite(seg[k])) and not same_bits(seg[k], S.cut(p[k], starts, window))
        want = S.merge(p[k], seg[k], starts, window)
        assert same_bits(back[k], want), (k, first_diff(back[k], want))
        if c["overlapping"]:  # the copies of a shared row differ: the order of the assignment decides
            n = len(starts)
            rev = np.concatenate([seg[k][j * window:(j + 1) * window] for j in reversed(range(n))])
            assert not same_bits(want, S.merge(p[k], rev, starts[::-1], window))


# ---- d. norms ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CS.NORMS])
def test_norms(V, cid, monkeypatch):
    c = CS.NORMS_BY_ID[cid]
    mu = CS.norms_problem(c)
    last = np.zeros_like(mu)
    last[-1, 0] = -7.0
    if c["blocks"] is None:
        monkeypatch.delenv("VLGP_NORMS_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("VLGP_NORMS_BLOCKS", str(c["blocks"]))
    print("support %-26s %d workgroup(s), %d trip(s), %d of 4 loads in range on the last, %d fold trip(s)"
          % (cid, c["g"], c["trips"], c["loads_in_range"], c["fold_trips"]))
    with V.Engine(1, 1, 1, RANK) as eng:
        eng.reload_switches()
        assert eng.switch("VLGP_NORMS_BLOCKS") == (c["blocks"] or CS.NORMS_DEFAULT_BLOCKS)
        for arr, want in ((mu, float((mu.astype(np.int64) ** 2).sum())), (last, 49.0)):
            eng.upload(0, [one_unit(np.zeros((c["n"], 1)), 1, mu=arr)])
            eng.norms_begin(0)
            got = eng.norms_end()
            assert got == (float(np.sqrt(want)), 0.0), (cid, got, want)  # (sqrt is correctly rounded on both sides)
            assert eng.norms(0) == got
        monkeypatch.delenv("VLGP_NORMS_BLOCKS", raising=False)
        eng.reload_switches()


# ---- e. prior factor ---------------------------------------------------------------------------------------------------
def check_factors(eng, c, omega, tag):
    for T in c["lengths"]:
        G, rk = eng.get_prior(T, with_rank=True)
        for l in range(c["L"]):
            Go, ro = CS.oracle_factor(T, omega[l], c["sigma"][l], c["R"])
            assert rk[l] == ro, (c["id"], tag, T, l, int(rk[l]), ro)
            assert same_bits(G[l], Go), (c["id"], tag, T, l, first_diff(G[l], Go))


@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CS.PRIOR])
def test_prior_factor(V, cid, monkeypatch):
    monkeypatch.delenv("VLGP_ICHOL_BLOCK", raising=False)
    c = CS.PRIOR_BY_ID[cid]
    with V.Engine(2, c["L"], 1, c["R"]) as eng:
        assert eng.switch("VLGP_ICHOL_BLOCK") == 0.0
        eng.build_prior(c["lengths"], c["omega"], c["sigma"])
        check_factors(eng, c, c["omega"], "built")
        if c["rebuild"] is not None:  # the same lengths: rebuilt in place, the ranks deferred (<= 64 lengths) or waited for
            eng.build_prior(c["lengths"], c["rebuild"], c["sigma"])
            check_factors(eng, c, c["rebuild"], "rebuilt")
            eng.build_prior(c["lengths"], c["omega"], c["sigma"])
            assert np.array_equal(eng.prior_ranks(c["lengths"][-1]),
                                  [CS.oracle_factor(c["lengths"][-1], c["omega"][l], c["sigma"][l], c["R"])[1] for l in range(c["L"])])
            check_factors(eng, c, c["omega"], "rebuilt back")


@gpu
@pytest.mark.parametrize("T", [1, 2, 64])
def test_prior_factor_workgroup_of_64(V, T, monkeypatch):
    """VLGP_ICHOL_BLOCK=1: lengths up to 64 bins through ichol_exact_kernel<64> instead of the one-wave kernel."""
    monkeypatch.setenv("VLGP_ICHOL_BLOCK", "1")
    omega, sigma = np.array([CS.smooth(T), CS.ROUGH]), np.array([1.0, 0.75])
    for R in (50, 64):
        with V.Engine(2, 2, 1, R) as eng:
            assert eng.switch("VLGP_ICHOL_BLOCK") == 1.0
            eng.build_prior([T], omega, sigma)
            G, rk = eng.get_prior(T, with_rank=True)
        for l in range(2):
            Go, ro = CS.oracle_factor(T, omega[l], sigma[l], R)
            assert rk[l] == ro and same_bits(G[l], Go), (T, R, l, int(rk[l]), ro, first_diff(G[l], Go))


@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CS.COMPACT])
def test_prior_compact_copy_through_a_consumer(V, cid):
    """One E-step sweep on a handle whose prior the device factored equals, in bits, the sweep on a handle given the oracle's
    factor (set_prior: prior_rank_kernel + prior_compact_kernel): both compact copies and both rank tables are the same."""
    c = next(k for k in CS.COMPACT if k["id"] == cid)
    T, L, R, N = c["T"], c["L"], c["R"], c["N"]
    rng = np.random.default_rng(CS._seed(cid))
    a, b = 0.3 * rng.standard_normal((L, N)), np.log(0.5) + 0.1 * rng.standard_normal((1, N))
    unit = {"y": rng.poisson(0.5, (T, N)).astype(float), "mu": 0.2 * rng.standard_normal((T, L)), "v": 0.1 + rng.random((T, L)),
            "w": 0.1 + rng.random((T, L))}
    Go = np.stack([CS.oracle_factor(T, c["omega"][l], c["sigma"][l], R)[0] for l in range(L)])
    ranks = [CS.oracle_factor(T, c["omega"][l], c["sigma"][l], R)[1] for l in range(L)]
    out = []
    for built in (True, False):
        with V.Engine(N, L, 1, R) as eng:
            eng.set_params(a, b, np.ones(N))
            eng.upload(0, [unit])
            if built:
                eng.build_prior([T], c["omega"], c["sigma"])
            else:
                eng.set_prior(T, Go)
            assert list(eng.prior_ranks(T)) == ranks
            assert eng.estep(0, 1) == 0
            out.append(eng.download(0, keys=("mu", "v", "w")))
    for k in ("mu", "v", "w"):
        assert np.all(np.isfinite(out[0][k])) and same_bits(out[0][k], out[1][k]), (k, first_diff(out[0][k], out[1][k]))
    assert not same_bits(out[0]["mu"], unit["mu"])


@gpu
@pytest.mark.parametrize("cid", [f[0] for f in CS.injected_factors()])
def test_injected_factor_ranks(V, cid):
    G, ranks = next((f[1], f[2]) for f in CS.injected_factors() if f[0] == cid)
    L, T, R = G.shape
    with V.Engine(2, L, 1, R) as eng:
        eng.set_prior(T, G)
        got, rk = eng.get_prior(T, with_rank=True)
    assert same_bits(got, G) and list(rk) == ranks, (cid, list(rk), ranks)


# ---- f. posterior draws ------------------------------------------------------------------------------------------------
def device_draws(V, c, p):
    out = np.empty((c["n"], c["T"], c["L"]))
    bad = C.c_int(-1)
    from vlgp_amd._lib import dptr
    with V.Engine(2, c["L"], 1, c["R"]) as eng:
        mu, w, G, eps = (np.ascontiguousarray(p[k], dtype=np.float64) for k in ("mu", "w", "G", "eps"))
        eng._ck(eng.lib.vlgp_sample_posterior(eng.h, c["T"], dptr(mu), dptr(w), dptr(G), c["n"], dptr(eps), dptr(out), C.byref(bad)))
    assert bad.value == 0
    return out


@gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CS.DRAWS])
def test_posterior_draws(V, cid):
    c = CS.DRAW_BY_ID[cid]
    p, ref = CS.draw_problem(cid)
    got = device_draws(V, c, p)
    if c["compare"] == "bits":
        want = np.broadcast_to(p["mu"], got.shape)
        assert same_bits(got, want), first_diff(got, want)
    elif c["compare"] == "bound":
        err = np.abs(got.astype(np.longdouble) - ref["want"])
        print("support %-22s ranks %s  max err / bound %.3f" % (cid, p["ranks"], float(np.max(err / ref["bound"]))))
        assert np.all(err <= ref["bound"]), (cid, float(np.max(err / ref["bound"])))
    else:
        dist = CS.rel_distance(got, ref["want"])
        print("support %-22s ranks %s  device %.3e  oracle %.3e  allowance %.3e" % (cid, p["ranks"], dist, ref["oracle_distance"], ref["allowance"]))
        assert dist <= ref["allowance"], (cid, dist, ref["allowance"])
