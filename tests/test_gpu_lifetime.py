"""Who frees what, on the device: every assertion is an equality on vlgp_debug_live_memory (live device blocks and bytes,
live pinned / mapped host blocks and bytes, over the whole process), taken after gc.collect().  The smallest handle that
has every kind of set and every borrowed pointer: N = 3 channels, one of them Gaussian, L = 2, rank 4, xdim = 2 (x is not
all ones, so x.b exists and replicas borrow it), units of 5, 7 and 12 bins in set 0; six 4-bin units in set 1 for the cuts.
A handle has four slots."""
import gc

import numpy as np
import pytest

from oracle import vlgp_oracle as O

pytestmark = pytest.mark.gpu

N, L, R, P = 3, 2, 4, 2
LENGTHS = (5, 7, 12)
GAUSS = np.array([False, True, False])
GROUPS = [[0, 2], [1]]
SOURCE = "status -3.*source of a replicated set"


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(11)

    def unit(T):
        y = rng.poisson(0.6, (T, N)).astype(float)
        y[:, 1] = rng.standard_normal(T)
        return {"y": y, "x": np.stack([np.ones((T, N)), 0.2 * rng.standard_normal((T, N))], axis=1),
                "mu": 0.1 * rng.standard_normal((T, L)), "v": np.ones((T, L)), "w": 0.5 + rng.random((T, L))}

    p = {"a": 0.3 * rng.standard_normal((L, N)), "b": np.stack([np.full(N, -0.5), 0.1 * rng.standard_normal(N)]),
         "noise": np.ones(N), "units": [unit(T) for T in LENGTHS], "short": [unit(4) for _ in range(6)]}
    p["prior"] = O.build_prior(list(LENGTHS) + [4], np.array([2e-2, 5e-3]), np.ones(L), R)
    rows = sum(LENGTHS)
    one = rng.random((rows, N)) < 0.3
    p["held"] = np.stack([one, ~one & (rng.random((rows, N)) < 0.3)])
    return p


def live(V):
    gc.collect()
    return V._lib.live_memory()


def engine(V, p):
    eng = V.Engine(N, L, P, R, gauss_mask=GAUSS)
    eng.set_params(p["a"], p["b"], p["noise"])
    for length, G in p["prior"].items():
        eng.set_prior(length, G)
    return eng


def cut_tiling(eng):
    eng.cut(1, 2, np.arange(12) * 2, 2)


def cut_copied(eng):  # stage-major: rows 0 ... 2 of every 4-bin unit, then rows 1 ... 3, which share two rows with them
    eng.cut(1, 2, np.concatenate([np.arange(6) * 4, np.arange(6) * 4 + 1]), 3)
    eng.set_overlaps(2, [0, 6, 12], [[k, 6 + k, 2] for k in range(6)], [0, 0, 6])


def test_make_free_pairs_give_everything_back(V, problem):
    p = problem
    base = live(V)
    with engine(V, p) as eng:
        eng.upload(0, p["units"])
        eng.upload(1, p["short"])
        pairs = {
            "upload": lambda: eng.upload(2, p["units"]),
            "tiling cut": lambda: cut_tiling(eng),
            "copied cut": lambda: cut_copied(eng),
            "group replicas": lambda: eng.replicate(0, 2, groups=GROUPS),
            "one masked replica": lambda: eng.replicate(0, 2, held_out=p["held"][:1]),
            "two masked replicas": lambda: eng.replicate(0, 2, held_out=p["held"]),
        }
        for name, make in pairs.items():
            before = live(V)
            make()
            made = live(V)
            assert made[0] > before[0] and made[1] > before[1], name
            eng.free_units(2)
            assert live(V) == before, name
        # a new upload over a set that has tiling cuts: the cuts go with the old rows
        before = live(V)
        cut_tiling(eng)
        eng.upload(1, p["short"])
        assert live(V) == before
        with pytest.raises(V.VlgpError, match="unit set 2 is empty"):
            eng.download(2)
    assert live(V) == base


def walk(eng, p):
    eng.set_params(p["a"], p["b"], p["noise"])
    assert eng.estep(0, 2) == 0 and eng.estep(2, 2) == 0 and eng.estep(3, 2) == 0
    eng.stash_mu(0)
    eng.elbo(0, want_rows=True)
    eng.hstep_prepare(1, 4)
    assert eng.mstep(0, 1) == 0
    eng.loglik(0, want_rate=True)
    eng.loglik(2, want_rate=True)
    eng.forecast(0, {T: p["prior"][T][:, :2] for T in LENGTHS})
    eng.synchronize()


def test_a_walk_through_the_lazy_buffers_settles_and_close_returns_all(V, problem):
    p = problem
    base = live(V)
    with engine(V, p) as eng:
        eng.upload(0, p["units"])
        eng.upload(1, p["short"])
        eng.replicate(0, 2, groups=GROUPS)
        eng.replicate(0, 3, held_out=p["held"])
        walk(eng, p)
        walk(eng, p)
        settled = live(V)
        assert settled[2] > base[2]  # (pinned and mapped host blocks exist by now)
        for _ in range(18):
            walk(eng, p)
        assert live(V) == settled
    assert live(V) == base


def test_refused_calls_change_nothing(V, problem):
    p = problem
    base = live(V)
    with engine(V, p) as eng:
        eng.upload(0, p["units"])
        eng.upload(1, p["short"])
        cut_tiling(eng)
        eng.replicate(0, 3, groups=GROUPS)
        before = live(V)
        with pytest.raises(V.VlgpError, match="status -3.*plain uploaded set"):
            eng.replicate(2, 1, groups=GROUPS)  # replicas of a cut
        assert live(V) == before
        with pytest.raises(V.VlgpError, match=SOURCE):
            eng.free_units(0)
        assert live(V) == before
        with pytest.raises(V.VlgpError, match=SOURCE):
            eng.upload(0, p["units"])
        assert live(V) == before
        assert eng.estep(3, 1) == 0  # the replicas still stand on their source's rows
    assert live(V) == base
