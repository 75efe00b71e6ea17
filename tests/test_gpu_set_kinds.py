"""Which entry point takes which kind of unit set: every cell of the admission table (csrc/api.hip holds
it as data).  Six kinds of set on the smallest handle that has them all (N = 8, L = 3, two units of 40 bins); an admitted
cell is called with valid arguments and must succeed, a refused one must raise VlgpError with the status and the text the
library has always used.  The rule is the library's, so the file passes against any build that keeps it."""
import ctypes as C

import numpy as np
import pytest

from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu

N, L, T, W = 8, 3, 40, 25
KINDS = ("plain", "tiling", "copied", "groups", "masked2", "masked1")
GROUPS = [[1, 3], [5]]
LOGP = np.log(np.array([[1.0, 1e-2, 1e-4]]))
OK = None
REPLICATED = "status -3.*%s refuses a replicated set"  # (% the entry point's name)
SOURCE = "status -3.*source of a replicated set"
PLAIN_ONLY = "status -3.*plain uploaded set"


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture
def clean_env(monkeypatch):
    for name in ("VLGP_ESTEP_SPLIT", "VLGP_ESTEP_GENERIC", "VLGP_MSTEP_GENERIC", "VLGP_HSTEP_GENERIC"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(3)
    p = {"a": 0.3 * rng.standard_normal((L, N)), "b": np.full((1, N), -1.0), "noise": np.ones(N)}
    p["units"] = [{"y": rng.poisson(0.4, (T, N)).astype(float), "x": None, "mu": 0.1 * rng.standard_normal((T, L)),
                   "v": np.ones((T, L)), "w": 0.5 + rng.random((T, L))} for _ in range(2)]
    p["prior"] = O.build_prior([T, W], np.array([2e-2, 5e-3, 1e-3]), np.ones(L), 50)
    one = rng.random((2 * T, N)) < 0.3
    p["held"] = np.stack([one, ~one & (rng.random((2 * T, N)) < 0.3)])  # two masks that hold no entry out twice
    return p


def make(eng, p, kind):
    """Sets 0 ... 3 emptied, set 0 := the plain upload, then the set of `kind`: its id, rows and unit length."""
    for sid in (1, 2, 3, 0):
        eng.free_units(sid)
    eng.upload(0, p["units"])
    if kind == "plain":
        return 0, 2 * T, T
    if kind == "tiling":
        eng.cut(0, 1, np.array([0, T]), T)
        return 1, 2 * T, T
    if kind == "copied":  # stage-major: the first window of each trial, then the second, which shares 10 rows with it
        eng.cut(0, 1, np.array([0, T, T - W, 2 * T - W]), W)
        eng.set_overlaps(1, [0, 2, 4], [[0, 2, 2 * W - T], [1, 3, 2 * W - T]], [0, 0, 2])
        return 1, 4 * W, W
    kw = {"groups": dict(groups=GROUPS), "masked2": dict(held_out=p["held"]), "masked1": dict(held_out=p["held"][:1])}[kind]
    eng.replicate(0, 2, **kw)
    return 2, eng.sets[2][1], T


def replicate_units(eng, src, dst):
    ch = np.array([1, 4], dtype=np.int32)
    eng.check(eng.lib.vlgp_replicate_units(eng.h, src, dst, 2, ch.ctypes.data_as(C.POINTER(C.c_int))))


def table(p):
    """{entry point: (call(eng, set, rows, unit length), what each of KINDS gets: OK or the refusal's pattern)}."""
    fit = lambda name: (OK, OK, OK, REPLICATED % name, REPLICATED % name, OK)  # noqa: E731
    plain = lambda name, tiling=OK, copied=OK: (OK, tiling, copied) + (REPLICATED % name,) * 3  # noqa: E731
    every, ext = (OK,) * 6, lambda t: {t: p["prior"][t][:, :2]}  # noqa: E731
    return {
        "vlgp_estep": (lambda e, s, r, t: e.estep(s, 2), every),
        "vlgp_download_units": (lambda e, s, r, t: e.download(s), every),
        "vlgp_free_units": (lambda e, s, r, t: e.free_units(s), every),
        "vlgp_upload_units": (lambda e, s, r, t: e.upload(s, p["units"]), every),
        "vlgp_loglik": (lambda e, s, r, t: e.loglik(s, want_rate=True),
                        (OK, OK, "status -3.*vlgp_loglik on a copied cut: merge it and score the source set", OK, OK, OK)),
        "vlgp_update_w": (lambda e, s, r, t: e.update_w(s), fit("vlgp_update_w")),
        "vlgp_update_v": (lambda e, s, r, t: e.update_v(s, True), fit("vlgp_update_v")),
        "vlgp_mstep": (lambda e, s, r, t: e.mstep(s, 1), fit("vlgp_mstep_begin")),
        "vlgp_mstep_begin": (lambda e, s, r, t: (e.mstep_begin(s, 1), e.mstep_end()), fit("vlgp_mstep_begin")),
        "vlgp_hstep_objective": (lambda e, s, r, t: e.hstep_objective(s, t, 1.0, [1], LOGP), fit("vlgp_hstep_objective")),
        "vlgp_hstep_prepare": (lambda e, s, r, t: e.hstep_prepare(s, t), fit("vlgp_hstep_prepare")),
        "vlgp_hstep_begin": (lambda e, s, r, t: (e.hstep_begin(s, t), e.hstep_end()), fit("vlgp_hstep_begin")),
        "vlgp_apply_latent_map": (lambda e, s, r, t: e.apply_latent_map(s, np.eye(L) + 0.1, np.ones(L)),
                                  fit("vlgp_apply_latent_map")),
        "vlgp_norms": (lambda e, s, r, t: e.norms(s), fit("vlgp_norms")),
        "vlgp_norms_begin": (lambda e, s, r, t: (e.norms_begin(s), e.norms_end()), fit("vlgp_norms_begin")),
        "vlgp_latent_moments": (lambda e, s, r, t: e.latent_moments(s), fit("vlgp_latent_moments")),
        "vlgp_elbo": (lambda e, s, r, t: e.elbo(s), plain("vlgp_elbo")),
        "vlgp_forecast": (lambda e, s, r, t: e.forecast(s, ext(t)),
                          plain("vlgp_forecast", *("status -3.*vlgp_forecast refuses a cut set",) * 2)),
        "vlgp_stash_mu": (lambda e, s, r, t: (e.stash_mu(s), e.stash_mu(s, restore=True)), plain("vlgp_stash_mu")),
        "vlgp_set_overlaps": (lambda e, s, r, t: e.set_overlaps(s, [0, r // t], np.zeros((0, 3)), [0, 0]),
                              plain("vlgp_set_overlaps", tiling="status -3.*overlaps belong to a copied cut")),
        "vlgp_unshare_mu": (lambda e, s, r, t: e.unshare_mu(s), plain("vlgp_unshare_mu")),
        "vlgp_merge_units": (lambda e, s, r, t: e.merge(s),
                             ("status -3.*set 0 is not a cut", OK, OK) + (REPLICATED % "vlgp_merge_units",) * 3),
        "vlgp_project_units": (lambda e, s, r, t: e.project_latent(s, np.full((N, L), 0.1), np.zeros(L)),
                               plain("vlgp_project_units", tiling="status -3.*project the owning set, not an aliased cut")),
        "vlgp_cut_units": (lambda e, s, r, t: e.cut(s, 3, np.array([0, 7]), 5),
                           plain("vlgp_cut_units", tiling="status -3.*cannot cut a set that is itself a cut")),
        "vlgp_replicate_groups": (lambda e, s, r, t: e.replicate(s, 3, groups=GROUPS), (OK,) + (PLAIN_ONLY,) * 5),
        "vlgp_replicate_units": (lambda e, s, r, t: replicate_units(e, s, 3), (OK,) + (PLAIN_ONLY,) * 5),
        "vlgp_replicate_masked": (lambda e, s, r, t: e.replicate(s, 3, held_out=np.zeros((1, r, N), dtype=bool)),
                                  (OK,) + (PLAIN_ONLY,) * 5),
    }


def engine(V, p):
    eng = V.Engine(N, L, 1, 50)
    eng.set_params(p["a"], p["b"], p["noise"])
    for length, G in p["prior"].items():
        eng.set_prior(length, G)
    return eng


def test_every_entry_point_takes_or_refuses_the_kind(V, clean_env, problem):
    p = problem
    with engine(V, p) as eng:
        for k, kind in enumerate(KINDS):
            for name, (call, expected) in table(p).items():
                sid, rows, length = make(eng, p, kind)
                try:
                    if expected[k] is OK:
                        call(eng, sid, rows, length)
                    else:
                        with pytest.raises(V.VlgpError, match=expected[k]):
                            call(eng, sid, rows, length)
                except (Exception, pytest.fail.Exception) as exc:  # (say which cell it was)
                    want = expected[k] or "success"
                    raise AssertionError("%s on a %s set: %r, expected %s" % (name, kind, exc, want)) from exc
                eng.synchronize()
                eng.set_params(p["a"], p["b"], p["noise"])  # (an admitted M-step moved them)


def test_replicas_keep_their_shapes_and_their_source_its_rows(V, clean_env, problem):
    p = problem
    for kind, (n_rep, slots) in {"groups": (2, 3), "masked2": (2, N), "masked1": (1, N)}.items():
        with engine(V, p) as eng:
            sid, rows, _ = make(eng, p, kind)
            assert eng.estep(sid, 2) == 0
            assert eng.download(sid, ("mu",))["mu"].shape == (n_rep * 2 * T, L) and rows == n_rep * 2 * T
            sums, rate = eng.loglik(sid, want_rate=True)
            assert sums.shape == ((slots, 4) if kind == "groups" else (n_rep, N, 4)) and rate.shape == (2 * T, slots)
            assert np.all(np.isfinite(sums))
            # the source: no new contents while replicas alias its rows; everything else takes it as the plain set it is
            eng.upload(1, p["units"])
            for call in (lambda: eng.free_units(0), lambda: eng.upload(0, p["units"]),
                         lambda: eng.cut(1, 0, np.array([0]), 5), lambda: eng.replicate(1, 0, groups=GROUPS),
                         lambda: replicate_units(eng, 1, 0), lambda: eng.replicate(1, 0, held_out=p["held"])):
                with pytest.raises(V.VlgpError, match=SOURCE):
                    call()
            assert eng.estep(0, 1) == 0 and eng.mstep(0, 1) == 0
            eng.free_units(sid)
            eng.free_units(0)
