"""The case table of the held-out E-step's shape suite (tests/test_heldout_shapes_host.py, tests/test_gpu_heldout_shapes.py):
every exclusion instantiation of the row passes of csrc/estep_split.hip, with the channel order, the mask words and the
row-to-replica mapping at the places where they can go wrong.

A replicated set (Engine.replicate) is run by esplit_pass<LT (| EX_BY_ROW), KIND, HASXB, CS, true>, esplit_ya<LT (| EX_BY_ROW),
NJ, true>, esplit_excl_wconst and esplit_row_wconst and by nothing else.  `compiled()` reads what is compiled from the source
text -- the LT values of run_pass, the thresholds of pass_cs and ya_nj, EX_BY_ROW -- so a retune moves the cases with it, and
`instantiations(c, form)` names what a case launches from its (L, N, P, form).

  a  latent buckets: L = 1 ... 10 at N = 24, units of 50 bins (split) and of 70 (long split), vb off at LT 5 and 10
  b  channel split and y pass: N = 16 ... 129 at L = 5, N = 33, 100 at L = 3, 8, 10, N = 129 at every LT, N = 100 with every
     Gaussian channel in the first mask word
  c  regressors (P = 2, a real x: the HASXB passes) at N = 24, 33, 100, 129 and every LT
  d  rows and replicas: a source of 1, 63, 64, 65 rows; 2, 3, 16, 17 and 70 replicas; 3 x 50 rows at N = 65; stream lanes
  e  masks by entry: a random 30 % speckle at every LT and across three mask words, a blanked row, an empty replica, a dead
     channel, no Gaussian channel on the handle

Cases a-d have two FORMS: "groups" (one mask per replica, vlgp_replicate_groups) and "rows" (the same groups as masks that are
constant along the rows, vlgp_replicate_masked); the cases of e have the form "entries".  Unless a case says otherwise the
Gaussian channels are interleaved with the Poisson ones -- (1, 9, 14, 22) at N = 24, gauss_edges(N) elsewhere -- while
esplit_cols_kernel sorts the records Poisson first: a channel's record index is not its id (`record_order`), which is what the
passes must get right and what the earlier held-out tests, with their Gaussian channels last, could not see.

References (`restated_posterior`): the E-step of heldout_numpy.restated -- oracle.estep_unit with the group's loadings zeroed
-- for the form "groups", the E-step of speckled_numpy.restated -- speckled_numpy.estep_masked -- for the forms "rows" and
"entries"; computed once per (case, form, sweeps), shared, read-only.  Both start where the source units start (a replica is
a copy of its source: mu near the latents that made the data, w and v consistent with it, as test_gpu_estep_shapes starts
its units) and not at zero, where the two `restated` functions start: from zero the first mean step of these smooth latents
has no curvature to hold it, runs into the clip at 5 and the rates into their cap (w of 2e4), and 141 of the 265 runs were
then ill conditioned on the oracle itself, by up to 5e-4 for one ulp.  From zero, `restated_posterior` gives the bits of the
two `restated` functions (tests/test_heldout_shapes_host.py).
"""
import functools
import os
import re
import zlib

import numpy as np

import heldout_numpy as H
import speckled_numpy as S
import test_gpu_estep_shapes as E
from oracle import vlgp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "vlgp_amd", "csrc", "estep_split.hip")
STAGE = H.STAGE
SWEEPS = (1, 3)
RANK = 50
DMU_BOUND = 5.0
FIELDS = ("mu", "v", "w", "dmu")


# ------------------------------------------------------------------ what is compiled, from the source text
@functools.lru_cache(maxsize=None)
def compiled():
    with open(SOURCE) as f:
        src = f.read()
    lts = sorted({int(v) for v in re.findall(r"return run_passes<(\d+)>\(ctx, ln, A, kind, cols\);", src)})
    cs = re.search(r"int pass_cs\(int ntot\) \{ return ntot >= (\d+) \? 4 : \(ntot >= (\d+) \? 2 : 1\); \}", src)
    nj = re.search(r"int ya_nj\(int N\) \{ return N > (\d+) \? 0 : \(N <= (\d+) \? 4 : 8\); \}", src)
    ex = re.search(r"enum \{ EX_BY_ROW = (\d+) \};", src)
    ya = sorted({(int(lt), int(n)) for lt, n in re.findall(r"ESPLIT_YA\((\d+), (\d+)\)", src)})
    assert lts and cs and nj and ex and ya, "estep_split.hip no longer reads as this table expects"
    # the exclusion launches themselves: per replica and per row, with and without x.b, and the two constants of w
    for text in ("esplit_pass<LT | EX_BY_ROW, KIND, true, CS, true>", "esplit_pass<LT | EX_BY_ROW, KIND, false, CS, true>",
                 "esplit_pass<LT, KIND, true, CS, true>", "esplit_pass<LT, KIND, false, CS, true>",
                 "esplit_ya<LTV | EX_BY_ROW, NJV, true>", "esplit_ya<LTV, NJV, true>", "esplit_excl_wconst", "esplit_row_wconst",
                 "run_pass_cs<LT, SP_YA, 1>"):
        assert text in src, text
    return dict(LT=lts, cs4=int(cs.group(1)), cs2=int(cs.group(2)), row_above=int(nj.group(1)), nj4_upto=int(nj.group(2)),
                EX_BY_ROW=int(ex.group(1)), ya=ya)


def lt_of(L):
    return next(lt for lt in compiled()["LT"] if L <= lt)


def pass_cs(N):
    k = compiled()
    return 4 if N >= k["cs4"] else 2 if N >= k["cs2"] else 1


def ya_nj(N):
    k = compiled()
    return 0 if N > k["row_above"] else 4 if N <= k["nj4_upto"] else 8


def pass_name(lt, by_row, kind, hasxb, cs):
    return "esplit_pass<%d%s, %s, %s, %d, true>" % (lt, " | EX_BY_ROW" if by_row else "", kind, "true" if hasxb else "false", cs)


def ya_name(lt, by_row, nj):
    return "esplit_ya<%d%s, %d, true>" % (lt, " | EX_BY_ROW" if by_row else "", nj)


def compiled_instantiations():
    """Every exclusion instantiation a replicated set can launch, by name."""
    k = compiled()
    out = set()
    for lt in k["LT"]:
        for by_row in (False, True):
            for hasxb in (False, True):
                out.add(pass_name(lt, by_row, "SP_YA", hasxb, 1))
                for kind in ("SP_RES", "SP_W"):
                    for cs in (1, 2, 4):
                        out.add(pass_name(lt, by_row, kind, hasxb, cs))
    for lt, nj in k["ya"]:
        for by_row in (False, True):
            out.add(ya_name(lt, by_row, nj))
    return out | {"esplit_excl_wconst", "esplit_row_wconst"}


def instantiations(c, form):
    """What one E-step call on the case's replicated set launches of them (run_pass_cs, run_ya, launch_estep_split)."""
    lt, by_row, hasxb = lt_of(c["L"]), form != "groups", c["P"] > 1
    out = {pass_name(lt, by_row, kind, hasxb, pass_cs(c["N"])) for kind in ("SP_RES", "SP_W")}
    nj = ya_nj(c["N"])
    out.add(pass_name(lt, by_row, "SP_YA", hasxb, 1) if nj == 0 else ya_name(lt, by_row, nj))
    if not by_row:
        out.add("esplit_excl_wconst")
    elif c["gauss"]:
        out.add("esplit_row_wconst")
    return out


# ------------------------------------------------------------------ channel order
def record_order(N, gauss):
    """Channel ids in the order of esplit_cols_kernel's records: Poisson first, both lists in channel order."""
    g = set(gauss)
    return [n for n in range(N) if n not in g] + sorted(g)


def wave_share(N, gauss, part, cs):
    """The Poisson records wave `part` of a CS-wave row group walks: [np part / CS, np (part + 1) / CS) in record order."""
    pois = [n for n in range(N) if n not in set(gauss)]
    return pois[len(pois) * part // cs:len(pois) * (part + 1) // cs]


def record_words(N, gauss):
    """The mask word of every record's channel id, runs collapsed: the sequence a lane that walks all records goes through."""
    words = [n >> 6 for n in record_order(N, gauss)]
    return [w for i, w in enumerate(words) if i == 0 or w != words[i - 1]]


GROUPS24 = [[0, 9], [1], [22, 23], [14, 5, 6]]


def groups24(n_rep):
    """Two, three or all four of GROUPS24; each choice leaves a Poisson channel out that lies after a Gaussian one."""
    return [GROUPS24[k] for k in {2: (0, 3), 3: (0, 2, 3), 4: (0, 1, 2, 3)}[n_rep]]


EDGE_CHANNELS = (0, 15, 16, 31, 32, 47, 48, 63, 64, 65, 127, 128)


def groups_at_edges(N, gauss):
    """Four groups for N != 24: the channels at the edges of the mask words and of the 16-channel strides of esplit_ya's lanes,
    dealt alternately over two groups (each given a channel of the likelihood it lacks); the whole Poisson share of one wave of the
    channel split (the middle one; all Poisson channels where the passes are not split); every Gaussian channel."""
    edges = sorted({n for n in EDGE_CHANNELS + (N - 1,) if 0 <= n < N})
    g0, g1 = edges[0::2], edges[1::2]
    spare = [n for n in range(1, N) if n not in gauss and n not in edges]
    for g in (g0, g1):
        if all(n in gauss for n in g):
            g.append(spare.pop(0))
    if not any(n in gauss for n in g0 + g1):  # (the Gaussian channels are at no edge: one each from the middle of their list)
        g0.append(sorted(gauss)[1])
        g1.append(sorted(gauss)[2])
    cs = pass_cs(N)
    return [g0, g1, wave_share(N, gauss, cs // 2, cs), sorted(gauss)]


def groups_many(n_rep, N=24):
    """n_rep groups of two channels each; between them they hold every channel of both likelihoods."""
    return [sorted({k % N, (5 * k + 9) % N}) for k in range(n_rep)]


# ------------------------------------------------------------------ the table
RANKS = (13, 3, 9, 14, 6, 11, 4, 8, 12, 5)  # per latent at T >= 50: lane-per-task launches where the units are short


def ranks_for(T, L):
    if T >= 50:
        return list(RANKS[:L])
    return (E.ranks_near(T) * 2)[:L]


def case(cid, L, N=24, P=1, T=50, M=3, groups=None, gauss=None, vb=True, env=None, entries=None, n_rep=None, note=""):
    if gauss is None:
        gauss = (1, 9, 14, 22) if N == 24 else E.gauss_edges(N)
    gauss = tuple(sorted(gauss))
    if entries is None:
        groups = [list(g) for g in (groups if groups is not None else GROUPS24 if N == 24 else groups_at_edges(N, gauss))]
        forms, n_rep = ("groups", "rows"), len(groups)
    else:
        forms = ("entries",)
    e = {"VLGP_ESTEP_SPLIT": "1", "VLGP_ESTEP_LSPLIT": "1"}  # the plain twin: onto the family a replicated set always takes
    e.update(env or {})
    return dict(id=cid, L=L, N=N, P=P, T=T, M=M, rows=T * M, groups=groups, gauss=gauss, vb=vb, env=e, entries=entries,
                n_rep=n_rep, forms=forms, ranks=ranks_for(T, L), family="long_split" if T > 64 else "split", note=note)


def build_matrix():
    m = []
    # a. every latent bucket exact and padded, short and long units, per replica and per row; vb off at LT 5 and 10
    for L in range(1, 11):
        m.append(case("a-L%d-short" % L, L))
        m.append(case("a-L%d-long" % L, L, T=70))
    for L in (5, 10):
        m.append(case("a-L%d-short-novb" % L, L, vb=False))
        m.append(case("a-L%d-long-novb" % L, L, T=70, vb=False))
    # b. CS 1 | 2 | 4 and NJ 4 | 8 | lane-per-row on both sides of their thresholds; four units of 50 bins (replica
    # boundaries at rows 200, 400, 600: none on a wave's edge)
    g129 = (0, 63, 64, 127)
    note129 = ("channel 128 is Poisson here: the record ids run through mask words 0, 1, 2 and back to 0 where the Gaussian "
               "list starts, then on to 1")
    for N in (16, 31, 32, 33, 63, 64, 65, 127, 128):
        m.append(case("b-N%d-L5" % N, 5, N=N, M=4))
    for L in (3, 8, 10):
        for N in (33, 100):
            m.append(case("b-N%d-L%d" % (N, L), L, N=N, M=4))
    m.append(case("b-N100-L5-gauss-low", 5, N=100, M=4, gauss=(1, 9, 14, 22),
                  note="every Gaussian channel in mask word 0: the two waves whose Poisson share ends in word 1 step back to word 0"))
    for L in (3, 5, 8, 10):  # (the lane-per-row y pass is compiled per LT: every bucket has its N > 128)
        m.append(case("b-N129-L%d" % L, L, N=129, M=4, gauss=g129, note=note129))
    # c. regressors: xb read at the source row and at the record's channel id
    for L in (3, 5, 8, 10):
        for N in (24, 33, 100):
            m.append(case("c-N%d-L%d-P2" % (N, L), L, N=N, P=2))
        m.append(case("c-N129-L%d-P2" % L, L, N=129, P=2, gauss=g129, note=note129))
    # d. rows and replicas, one source unit each
    for n_rep in (2, 3):
        m.append(case("d-rows1-rep%d" % n_rep, 5, T=1, M=1, groups=groups24(n_rep)))
    m.append(case("d-rows1-rep70", 5, T=1, M=1, groups=groups_many(70),
                  note="every lane of a wave is another replica; more replicas than esplit_excl_wconst has per workgroup"))
    for T in (63, 64, 65):
        m.append(case("d-rows%d" % T, 5, T=T, M=1))
    for n_rep in (16, 17):
        m.append(case("d-rep%d" % n_rep, 5, M=1, groups=groups_many(n_rep)))
    m.append(case("d-3x50-N65", 5, N=65, M=3, note="rows 150, 300, 450: a replica boundary inside a wave and inside a CS = 4 "
                  "workgroup of 64 rows"))
    # stream lanes (wave-per-task latents: a part is at least 8 units, cuts at multiples of 4)
    wave = {"VLGP_ESTEP_LANEPT": "0"}
    for lanes in (2, 3):
        m.append(case("d-lanes%d-inside" % lanes, 5, M=9, groups=groups24(3), env=dict(wave, VLGP_ESTEP_LANES=str(lanes)),
                      note="27 units: every cut falls inside a replica of 9"))
        m.append(case("d-lanes%d-between" % lanes, 5, M=8, groups=groups24(lanes), env=dict(wave, VLGP_ESTEP_LANES=str(lanes)),
                      note="replicas of 8 units: every cut falls between two replicas"))
    # e. masks by entry
    for L in (3, 5, 8, 10):
        m.append(case("e-speckle-L%d" % L, L, entries="speckle", n_rep=3))
    m.append(case("e-speckle-N129", 5, N=129, gauss=g129, entries="speckle", n_rep=2, note=note129))
    m.append(case("e-blank-rows-L8", 8, entries="blank-rows", n_rep=2))
    m.append(case("e-empty-replica-L8", 8, entries="empty-replica", n_rep=2))
    m.append(case("e-dead-channel-L8", 8, entries="dead-channel", n_rep=2))
    for L in (5, 10):
        m.append(case("e-no-gauss-L%d" % L, L, gauss=(), entries="speckle", n_rep=2,
                      note="no Gaussian channel on the handle: d_wconst is null, the records are in channel order"))
    return m


# Cases whose first draw was ill conditioned ON THE ORACLE (test_every_case_is_well_conditioned) draw again with this salt.
SALT = {}

MATRIX = build_matrix()
assert len({c["id"] for c in MATRIX}) == len(MATRIX)
BY_ID = {c["id"]: c for c in MATRIX}
RUNS = [(c["id"], form) for c in MATRIX for form in c["forms"]]
GROUP_CASES = [c["id"] for c in MATRIX if c["entries"] is None]
LANE_CASES = [c["id"] for c in MATRIX if "VLGP_ESTEP_LANES" in c["env"]]


def expected_plan(c, n_units):
    """The plan of a set of `n_units` of the case's units, as test_gpu_estep_shapes states plan_estep_split's rules; LT, CS and
    NJ from the source text."""
    cc = dict(env=c["env"], N=c["N"], L=c["L"], what="estep", family=c["family"], lengths=[c["T"]] * n_units, M=n_units)
    exp = E.expected_plan(cc, c["ranks"])
    assert (exp["LT"], exp["CS"], exp["NJ"]) == (lt_of(c["L"]), pass_cs(c["N"]), ya_nj(c["N"])), c["id"]
    if c["family"] == "long_split":  # (long units have no lane-per-task launch)
        exp["classes"] = ["lo" if r <= 16 else "hi" for r in c["ranks"]]
    return exp


SAME_AS_TWIN = ("family", "LT", "CS", "NJ", "classes")


# ------------------------------------------------------------------ problems, masks and references
def held_of(c, form, rng=None):
    """bool (n_rep, rows, N): the entries each replica leaves out."""
    rows, N = c["rows"], c["N"]
    held = np.zeros((c["n_rep"], rows, N), dtype=bool)
    if form in ("groups", "rows"):
        for k, g in enumerate(c["groups"]):
            held[k][:, g] = True
        return held
    speckle = lambda: rng.random((rows, N)) < 0.3
    kind = c["entries"]
    if kind == "speckle":
        for k in range(c["n_rep"]):
            held[k] = speckle()
    elif kind == "blank-rows":
        held[0, 45:71] = True  # every entry of 26 rows, across a unit's edge (row 50) and a wave's (row 64)
        held[1] = speckle()
    elif kind == "empty-replica":
        held[1] = speckle()  # (replica 0 leaves nothing out)
    elif kind == "dead-channel":
        held[0][:, 5] = True   # a Poisson channel on every row
        held[0][:, 14] = True  # and a Gaussian one
        held[0, 7, 22] = True
        held[1] = speckle()
    else:
        raise AssertionError(kind)
    return held


def left_out_channels(held):
    """The channels some replica leaves out somewhere."""
    return sorted(set(np.nonzero(held.any(axis=(0, 1)))[0].tolist()))


def make_problem(c):
    """Loadings and rates as test_gpu_estep_shapes.make_problem draws them (a = 0.3 randn, scaled down above 32 channels; b
    about log 0.3; smooth latents; rates capped at e^3), every unit distinct, the posterior started as that module starts
    its units: mu = z + 0.3 randn, w the curvature there, v the variance under that w."""
    N, L, P, T = c["N"], c["L"], c["P"], c["T"]
    rng = np.random.default_rng(zlib.crc32(("%s:%d" % (c["id"], SALT.get(c["id"], 0))).encode()))
    a = 0.3 * rng.standard_normal((L, N))
    if N > 32:
        a *= np.sqrt(32.0 / N)
    b = np.log(0.3) + 0.2 * rng.standard_normal((P, N))
    noise = 0.5 + rng.random(N)
    gauss = np.zeros(N, dtype=bool)
    gauss[list(c["gauss"])] = True
    sigma = 0.8 + 0.4 * rng.random(L)
    omega = np.array([E.omega_for(T, r) for r in c["ranks"]])
    chol = O.build_prior([T], omega, sigma, RANK)
    trials = []
    for _ in range(c["M"]):
        z = np.stack([np.sin(np.linspace(0, (2 + l) * np.pi, T) + rng.random() * 6) for l in range(L)], 1)
        x = np.ones((T, P, N))
        if P > 1:
            x[:, 1:, :] = 0.3 * rng.standard_normal((T, P - 1, N))
        eta = z @ a + np.einsum("tpn,pn->tn", x, b)
        y = rng.poisson(np.exp(np.minimum(eta, 3))).astype(float)
        y[:, gauss] = eta[:, gauss] + 0.7 * rng.standard_normal((T, int(gauss.sum())))
        mu = z + 0.3 * rng.standard_normal((T, L))
        w = O.curvature_unit(y, x, mu, np.zeros_like(mu), a, b, noise, gauss)
        trials.append({"y": y, "x": x, "mu": mu, "w": w, "v": O.variance_unit(w, np.zeros_like(mu), chol[T])[0]})
    params = {"ydim": N, "zdim": L, "xdim": P, "a": a, "b": b, "noise": noise, "omega": omega, "sigma": sigma, "rank": RANK,
              "likelihood": np.where(gauss, "gaussian", "poisson")}
    config = {"method": "VB" if c["vb"] else "MAP", "max_iter": SWEEPS[-1], "dmu_bound": DMU_BOUND}
    held = {form: held_of(c, form, rng) for form in c["forms"]}
    host_ranks = [int(np.any(chol[T][l] != 0, axis=0).sum()) for l in range(L)]
    return dict(trials=trials, params=params, config=config, gauss=gauss, chol=chol, held=held, ranks=host_ranks)


def zeroed(a, group):
    a0 = a.copy()
    a0[:, group] = 0.0
    return a0


def restated_posterior(c, p, form, n_iter, mu=None, from_zero=False):
    """mu, v, w, dmu (n_rep, rows, L) after n_iter sweeps from the units' start: form "groups" by the E-step of
    heldout_numpy.restated, the other forms by that of speckled_numpy.restated.  `mu`: another start per unit (the
    conditioning check); `from_zero`: the start of the two `restated` functions."""
    par = p["params"]
    a, b, noise, gauss, G = par["a"], par["b"], par["noise"], p["gauss"], p["chol"][c["T"]]
    T, L = c["T"], c["L"]
    out = {k: np.zeros((c["n_rep"], c["rows"], L)) for k in FIELDS}
    z = np.zeros((T, L))
    for m, tr in enumerate(p["trials"]):
        r0 = m * T
        s = (z, z, z) if from_zero else (tr["mu"] if mu is None else mu[m], tr["v"], tr["w"])
        for k in range(c["n_rep"]):
            if form == "groups":
                res = O.estep_unit(tr["y"], tr["x"], s[0], s[1], s[2], zeroed(a, c["groups"][k]), b, noise, gauss, G, n_iter,
                                   DMU_BOUND, c["vb"])
            else:
                res = S.estep_masked(tr["y"], tr["x"], a, b, noise, gauss, G, ~p["held"][form][k, r0:r0 + T], n_iter,
                                     DMU_BOUND, c["vb"], start=s)
            assert res[4] == 0, (c["id"], form, m, k)
            for key, arr in zip(FIELDS, res):
                out[key][k, r0:r0 + T] = arr
    return out


_problems, _references = {}, {}


def problem(cid):
    """Computed once per case, shared, read-only."""
    if cid not in _problems:
        p = make_problem(BY_ID[cid])
        for arr in ([t[k] for t in p["trials"] for k in t] + [v for v in p["params"].values() if isinstance(v, np.ndarray)]
                    + list(p["held"].values()) + list(p["chol"].values())):
            arr.setflags(write=False)
        _problems[cid] = p
    return _problems[cid]


def reference(cid, form, n_iter):
    key = (cid, form, n_iter)
    if key not in _references:
        ref = restated_posterior(BY_ID[cid], problem(cid), form, n_iter)
        for arr in ref.values():
            arr.setflags(write=False)
        _references[key] = ref
    return _references[key]


def column_errors(c, got, ref):
    """Per field the largest error over the (replica, unit, latent) columns, each column as test_gpu_estep_shapes compares one:
    max over t of |got - ref| over the column's own max |ref|, dmu on the column's mu scale.  A NaN comes out as inf."""
    shape = (c["n_rep"], c["M"], c["T"], c["L"])
    out = {}
    for k in FIELDS:
        scale = np.abs(ref["mu" if k == "dmu" else k].reshape(shape)).max(axis=2)
        err = np.abs(got[k].reshape(shape) - ref[k].reshape(shape)).max(axis=2) / np.maximum(scale, 1e-300)
        out[k] = float(np.where(np.isfinite(err), err, np.inf).max())
    return out


# ------------------------------------------------------------------ two wrong lookups, stated on the host
def walks(c):
    """The record indices every lane that keeps one mask-word cache walks, in order, per kind of pass: each wave's share of the
    Poisson list and then of the Gaussian list (SP_RES), of the Poisson list alone (SP_W), every record (the lane-per-row
    SP_YA of N > 128).  esplit_ya's coalesced forms hold their words in registers and look nothing up by record."""
    N, cs = c["N"], pass_cs(c["N"])
    n_p = N - len(c["gauss"])
    out = []
    for part in range(cs):
        pois = list(range(n_p * part // cs, n_p * (part + 1) // cs))
        gaus = list(range(n_p + (N - n_p) * part // cs, n_p + (N - n_p) * (part + 1) // cs))
        out += [("SP_RES", pois + gaus), ("SP_W", pois)]
    if ya_nj(N) == 0:
        out.append(("SP_YA", list(range(N))))
    return out


def seen_left_out(c, mask, walk, lookup):
    """The channels of `walk` a lane takes as left out under the mask `mask` (bool (N,)): by esplit_pass's left_out ("id"),
    by the record index in place of the id stored in the record ("record-index"), or with a word cache that reloads only when
    the word number grows ("forward-only")."""
    order = record_order(c["N"], c["gauss"])
    bit = lambda n: bool(mask[n]) if n < c["N"] else False
    out, word = set(), 0
    for i in walk:
        n = order[i]
        if lookup == "id":
            hit = bit(n)
        elif lookup == "record-index":
            hit = bit(i)
        else:
            word = max(word, n >> 6)
            hit = bit(64 * word + (n & 63))
        if hit:
            out.add(n)
    return out


def caught_by(c, form, held, lookup):
    """The kinds of pass in which the wrong `lookup` leaves another set of channels out than the right one, for some mask of
    the case: there the bits of the plain twin and the restatement cannot both be met."""
    masks = np.unique(held.reshape(-1, c["N"]), axis=0)[:64]
    return sorted({kind for kind, walk in walks(c) for m in masks
                   if seen_left_out(c, m, walk, lookup) != seen_left_out(c, m, walk, "id")})
